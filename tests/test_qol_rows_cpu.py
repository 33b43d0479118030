"""Row-wise 2-norms without a GPU: the QuadOverLinRows atom and its rule tags, the canonical form of norm(X, 2, axis),
the tape layout of the third row-class member (OP_QUAD_OVER_LIN_ROWS = 36: two arguments, an arrow of 2K + 1 Hessian
entries per row), the rule of the host build (csrc/model.h sweep_qol_rows_segment over host loops) entry by entry
against mpmath (tests/qol_rows_reference.py: the definition, the rows, the derived bound), and solves by the host build
with closed forms, each also against the loop of scalar norms (tests/qol_rows_problems.py)."""
import numpy as np
import pytest

import dnlp_amd as cp
import lse_problems as lp
import qol_rows_problems as qp
import qol_rows_reference as qr
from batch_problems import oracle_solver
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.tape import serialize


# ---- 1. front-end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, 0, 1])
@pytest.mark.parametrize("keepdims", [False, True])
def test_value_and_shape(axis, keepdims):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((4, 6)) * 3
    want_ss = np.sum(v * v, axis=axis, keepdims=keepdims)
    yv = rng.uniform(0.5, 2.0, np.shape(want_ss))
    X, y = cp.Variable((4, 6)), cp.Variable(np.shape(want_ss))
    X.value, y.value = v, yv
    e = cp.quad_over_lin_rows(X, y, axis=axis, keepdims=keepdims)
    assert isinstance(e, cp.QuadOverLinRows) and e.shape == np.shape(want_ss) == cp.sum(X, axis=axis, keepdims=keepdims).shape
    assert np.array_equal(np.asarray(e.value), want_ss / yv)
    # the public names that reach it agree with numpy (axis None of a matrix is the spectral norm: not this atom)
    for n in (() if axis is None else (cp.norm(X, 2, axis=axis, keepdims=keepdims), cp.pnorm(X, 2, axis=axis, keepdims=keepdims))):
        assert n.shape == np.shape(want_ss) and np.allclose(n.value, np.sqrt(want_ss), rtol=1e-15)


def test_denominator_must_have_the_shape_of_the_result():
    X = cp.Variable((4, 6))
    for y, axis, keepdims in ((cp.Variable(4), 0, False), (cp.Variable(), 1, False), (cp.Variable(4), 1, True)):
        with pytest.raises(ValueError, match="quad_over_lin_rows must have the shape of the result"):
            cp.quad_over_lin_rows(X, y, axis=axis, keepdims=keepdims)
    with pytest.raises(ValueError, match="must be a scalar"):          # the scalar atom keeps its check
        cp.quad_over_lin(X, cp.Variable(4))


def test_sign_curvature_and_rule_tags_are_those_of_quad_over_lin():
    X, y, s = cp.Variable((3, 4)), cp.Variable(3), cp.Variable()
    for arg_of in (lambda v: v, cp.abs, lambda v: -cp.abs(v), cp.exp, cp.log):
        rows, one = cp.quad_over_lin_rows(arg_of(X), y, axis=1), cp.quad_over_lin(arg_of(X), s)
        for tag in ("is_nonneg", "is_nonpos", "is_convex", "is_concave", "is_atom_convex", "is_atom_concave", "is_atom_esr",
                    "is_atom_hsr", "is_esr", "is_hsr", "is_smooth"):
            assert getattr(rows, tag)() == getattr(one, tag)(), tag
        for idx in (0, 1):
            assert rows.is_incr(idx) == one.is_incr(idx) and rows.is_decr(idx) == one.is_decr(idx)
    e = cp.quad_over_lin_rows(X, y, axis=1)
    assert e.is_convex() and not e.is_concave() and e.is_nonneg() and e.is_decr(1) and not e.is_incr(1)
    assert cp.Problem(cp.Minimize(cp.sum(cp.norm(X, 2, axis=1)))).is_dnlp()


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------
def test_canonical_form_of_a_sum_of_row_norms():
    """sum(norm(X - A, 2, axis=1)), X 5 x 3: t (5, nonneg) is the epigraph variable, t1 (5 x 3) == X - A the aliased
    numerator, t2 (5, nonneg, started at ones) == t the denominator; rows in that order, then ratio <= t, then the user's."""
    X = cp.Variable((5, 3))
    X.value = np.full((5, 3), 2.0)
    A = np.arange(15.0).reshape(5, 3) / 4
    prob = cp.Problem(cp.Minimize(cp.sum(cp.norm(X - A, 2, axis=1))), [X >= 0.1])
    smooth, _ = Dnlp2Smooth().apply(prob)
    kinds = [(type(c).__name__, c.shape) for c in smooth.constraints]
    assert kinds == [("Equality", (5, 3)), ("Equality", (5,)), ("Inequality", (5,)), ("Inequality", (5, 3))]
    atom = smooth.constraints[2].args[0]
    while not isinstance(atom, cp.QuadOverLinRows):
        atom = atom.args[0]
    t1, t2 = atom.args
    t = smooth.objective.expr.args[0]
    assert (atom.axis, atom.keepdims) == (1, False)
    assert isinstance(t1, cp.Variable) and t1.shape == (5, 3) and not t1.attributes["nonneg"] and np.array_equal(t1.value, 2.0 - A)
    assert isinstance(t2, cp.Variable) and t2.shape == (5,) and t2.attributes["nonneg"] and np.array_equal(t2.value, np.ones(5))
    assert isinstance(t, cp.Variable) and t.shape == (5,) and t.attributes["nonneg"] and t.value is None
    from dnlp_amd.nlp_solver import build_nlp_data
    data = build_nlp_data(smooth)[0]
    a = data["tape_arrays"]
    N, m, Z, nseg, nd, nh = (int(v) for v in a["dims"][:6])
    assert (N, m, Z, nseg, nd, nh) == (40, 40, 5, 1, 20, 35) and list(a["seg_op"]) == [36]
    off = data["tape"].var_offsets
    assert [off[id(v)] for v in (t, t1, X, t2)] == [0, 5, 20, 35]
    F = lambda M: np.asarray(M).reshape(-1, order="F")
    assert np.array_equal(data["x0"], np.concatenate([np.ones(5), F(2.0 - A), np.full(15, 2.0), np.ones(5)]))
    assert np.array_equal(a["lb"], np.concatenate([np.zeros(5), np.full(30, -np.inf), np.zeros(5)]))
    assert np.array_equal(a["ub"], np.full(40, np.inf))
    assert np.array_equal(a["cl"], np.zeros(40)) and np.array_equal(a["cu"], np.concatenate([np.zeros(20), np.full(20, np.inf)]))


def test_the_issue_example_solves_on_the_host_build():
    values = []
    for loop in (False, True):
        prob, X, want = qp.norms_over_a_bound(loop)
        obj, status, iters, xv = oracle_solver(prob)
        assert status == 0 and abs(obj - want) <= qp.VALUE_TOL * want, (loop, status, obj, want)
        values.append(obj)
    assert abs(values[0] - values[1]) <= qp.VALUE_TOL * values[1], values


def test_constant_denominator_goes_through_power_and_sum():
    X = cp.Variable((4, 3))
    X.value = np.arange(12.0).reshape(4, 3)
    y = np.array([1.0, 2.0, 4.0, 0.5])
    prob = cp.Problem(cp.Minimize(cp.sum(cp.quad_over_lin_rows(X, y, axis=1))))
    smooth, _ = Dnlp2Smooth().apply(prob)
    assert not smooth.constraints
    a = lp.lower(prob)["tape_arrays"]
    assert len(a["seg_op"]) == 1 and int(a["seg_op"][0]) < 30                # the power segment: elementwise class
    assert np.allclose(smooth.objective.expr.value, np.sum(np.sum(X.value ** 2, axis=1) / y), rtol=1e-15)


@pytest.mark.parametrize("make", [lambda: cp.norm(cp.Variable(4), 2), lambda: cp.norm(cp.Variable((1, 4)), 2, axis=1),
                                  lambda: cp.norm(cp.Variable((1, 4)), 2, axis=1, keepdims=True),
                                  lambda: cp.norm(cp.Variable((4, 1)), 2, axis=0), lambda: cp.norm(cp.Variable((2, 2)), "fro")])
def test_scalar_valued_norms_keep_the_scalar_op(make):
    e = make()
    e.args[0].variables()[0].value = np.ones(e.args[0].variables()[0].shape)
    assert e.is_scalar()
    a = lp.lower(cp.Problem(cp.Minimize(cp.sum(e))))["tape_arrays"]
    assert list(a["seg_op"]) == [32] and int(a["seg_hcount"][0]) == 2 * 4 + 1 and int(a["seg_dcount"][0]) == 4 + 1


def test_other_exponents_keep_their_error():
    X = cp.Variable((3, 2))
    X.value = np.ones((3, 2))
    with pytest.raises(ValueError, match="Only p=2 is supported"):
        lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.pnorm(X, 3, axis=1)))))


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,keepdims", [(None, False), (0, False), (1, False), (1, True), (0, True)])
def test_tape_layout(axis, keepdims):
    shape = (5,) if axis is None else (4, 3)
    M, K = {None: (1, 5), 0: (3, 4), 1: (4, 3)}[axis]
    yshape = cp.sum(cp.Variable(shape), axis=axis, keepdims=keepdims).shape
    X, Y, P, Q = cp.Variable(shape), cp.Variable(yshape), cp.Variable(shape), cp.Variable(yshape)
    for v in (X, Y, P, Q):
        v.value = np.ones(v.shape)
    from dnlp_amd.lowering import lower_problem
    tape = lower_problem(cp.sum(cp.quad_over_lin_rows(X, Y, axis, keepdims)), [cp.quad_over_lin_rows(P, Q, axis, keepdims)],
                         [X, Y, P, Q])
    segs = tape.segments
    H = 2 * K + 1
    assert [g.op for g in segs] == [36, 36] and [g.dims for g in segs] == [(M, K, 0)] * 2 and [g.n for g in segs] == [M, M]
    assert [g.zcount for g in segs] == [M, M] and [g.dcount for g in segs] == [M * (K + 1)] * 2 and [g.hcount for g in segs] == [M * H] * 2
    assert [g.zoff for g in segs] == [0, M] and [g.doff for g in segs] == [0, M * (K + 1)] and [g.hoff for g in segs] == [0, M * H]
    want = []
    for s, (V, D) in enumerate(((X, Y), (P, Q))):
        full = tape.var_offsets[id(V)] + np.arange(V.size).reshape(shape, order="F")
        rows = full.reshape(1, -1) if axis is None else (full.T if axis == 0 else full)
        assert np.array_equal(segs[s].a0.reshape(M, K), rows)                # row r reads the entries the axis says
        yidx = tape.var_offsets[id(D)] + np.arange(M)
        assert np.array_equal(segs[s].a1, yidx)
        want.append(qr.arrow_pattern(rows, yidx, s * M + np.arange(M)))
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), [np.concatenate(parts) for parts in zip(*want)]):
        assert np.array_equal(getattr(tape, name), w), name
    assert np.all(tape.hrow >= tape.hcol)
    # the three blocks of the first segment: K diagonal entries per row, the denominators' diagonal, the cross entries
    r, c = tape.hrow[:M * H], tape.hcol[:M * H]
    assert np.all(r[:M * K + M] == c[:M * K + M]) and np.all(r[M * K + M:] > c[M * K + M:])


def _vars(*shapes):
    out = [cp.Variable(s) for s in shapes]
    for v in out:
        v.value = np.ones(v.shape)
    return out


def test_empty_argument_is_refused():
    from dnlp_amd.lowering import lower_problem
    x, y = _vars((0, 3), (3,))
    with pytest.raises(ValueError, match="quad_over_lin_rows of an empty argument"):
        lower_problem(cp.sum(cp.quad_over_lin_rows(x, y, axis=0)), [], [x, y])


def test_repeated_index_in_a_row_is_refused():
    from dnlp_amd.lowering import lower_problem
    x, y = _vars((3,), ())
    with pytest.raises(ValueError, match="quad_over_lin_rows.*twice"):
        lower_problem(cp.quad_over_lin_rows(cp.hstack([x[0], x[1], x[0]]), y), [], [x, y])


def test_denominator_among_its_rows_numerator_is_refused():
    from dnlp_amd.lowering import lower_problem
    X, = _vars((3, 2))
    with pytest.raises(ValueError, match="quad_over_lin_rows.*denominator is one of its own numerator"):
        lower_problem(cp.sum(cp.quad_over_lin_rows(X, X[:, 1], axis=1)), [], [X])
    # another row's entry is a different variable entry for this row: accepted
    x, = _vars((4,))
    num = cp.reshape(x, (2, 2), order="F")                                # rows (x0, x2), (x1, x3)
    with pytest.raises(ValueError, match="denominator is one of its own numerator"):
        lower_problem(cp.sum(cp.quad_over_lin_rows(num, cp.hstack([x[0], x[2]]), axis=1)), [], [x])
    tape = lower_problem(cp.sum(cp.quad_over_lin_rows(num, cp.hstack([x[1], x[0]]), axis=1)), [], [x])
    assert [g.op for g in tape.segments] == [36]


def test_counts_beyond_the_index_range_are_refused():
    """2K + 1 entries per row reach 2^31 only with 1e9 variable entries, so the tape's running counts are set as a tape
    that already holds that many entries would have them."""
    from dnlp_amd.lowering import Lowerer
    x, y = _vars((4, 3), (4,))
    e = cp.quad_over_lin_rows(x, y, axis=1)
    for field, start in (("nh", 2 ** 31 - 1 - 4 * 7 + 1), ("nd", 2 ** 31 - 1 - 4 * 4 + 1)):
        low = Lowerer([x, y], [e])
        setattr(low, field, start)
        with pytest.raises(ValueError, match="quad_over_lin_rows: 4 row.s. of length 3 need 28 Hessian entries.*2147483647"):
            low.lower(e)
        low = Lowerer([x, y], [e])
        setattr(low, field, start - 1)                                      # the last count that fits
        low.lower(e)


def test_tape_with_all_four_non_flat_opcodes_loads_in_the_host_build():
    """ops 32, 34, 35 and 36 in one tape: the host build evaluates each by its own rule."""
    from oracle.oracle_capi import OracleProblem
    from scipy.special import logsumexp
    U, yv = qr.rows_of_shape(3, 4)
    A, B, C, Y, q, s = _vars((3, 4), (3, 4), (3, 4), (3,), (4,), ())
    A.value, B.value, C.value, Y.value, q.value, s.value = U, U, U, yv, U[0], yv[0]
    prob = cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))),
                      [cp.quad_over_lin(q, s) <= 0, cp.log_sum_exp(A, axis=1) <= 0, cp.prod(B, axis=1) <= 0,
                       cp.quad_over_lin_rows(C, Y, axis=1) <= 0])
    data = lp.lower(prob)
    a = data["tape_arrays"]
    assert list(a["seg_op"]) == [32, 34, 35, 36] and list(a["seg_hcount"]) == [9, 30, 18, 27]
    x = np.array(data["x0"], dtype=float)
    o = OracleProblem(serialize(a))
    g = o.eval_g(x)
    e = qr.segment_entries(a, 3)
    # (the denominators the segments read are the canonicaliser's own nonneg variables: started at the value, all > 1e-4)
    assert np.array_equal(x[e["yidx"]], yv)
    assert np.allclose(e["sign"] * g[e["crow"]], np.sum(U * U, axis=1) / yv, rtol=1e-14)
    want = {32: np.sum(U[0] ** 2) / yv[0], 34: logsumexp(U, axis=1), 35: np.prod(U, axis=1)}
    found = np.abs(g)
    for op, v in want.items():
        for val in np.atleast_1d(v):
            assert np.any(np.isclose(found, abs(val), rtol=1e-13)), (op, val)
    assert o.eval_h(x, lp.multipliers(int(a["dims"][1])), 0.5).size == int(a["dims"][7])
    print("segment 3: worst error %.3f of its bound" % qr.check_segment("host build", o, (a, x, lp.multipliers(int(a["dims"][1])), 0.5), 3))


# ---- 4. rule ------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_within_the_derived_bound():
    for U, y in qr.grid() + [qr.planted()]:
        w = lp.multipliers(U.shape[0])
        got = qr.numpy_rule(U, y, w)
        worst = max(qr.check_row("numpy statement %s row %d" % (U.shape, r), {k: v[r] for k, v in got.items()}, U[r], y[r], w[r])
                    for r in range(U.shape[0]))
        print("%s: worst error %.3f of its bound" % (U.shape, worst))


_tapes = {}


def grid_tape():
    if "grid" not in _tapes:
        _tapes["grid"] = qp.rows_tape(qr.grid())
    return _tapes["grid"]


def planted_tape():
    if "planted" not in _tapes:
        _tapes["planted"] = qp.rows_tape([qr.planted()])
    return _tapes["planted"]


def check_grid(name, make):
    ev = make(grid_tape()[0])
    for s, (M, K) in enumerate(qr.GRID):
        print("%s, %d x %d: worst error %.3f of its bound" % (name, M, K, qr.check_segment(name, ev, grid_tape(), s)))
    return ev


def check_planted(name, make):
    """A NaN entry poisons its row's z, g_y and h_yy and its own g_l and h_ly; an inf entry likewise gives inf there;
    y = 0 gives inf, or NaN where ss = 0; y < 0 is plain arithmetic: positions and values as IEEE gives them."""
    a, x, lam, sigma = planted_tape()
    ev = make(a)
    qr.check_segment(name, ev, planted_tape())
    U, y, w, got = qr.rows_got(a, 0, x, lam, ev.eval_g(x), ev.eval_jac_g(x), ev.eval_h(x, lam, sigma))
    nan = {k: np.isnan(v) for k, v in got.items()}
    assert nan["z"].tolist() == [True, False, False, True, False, False] and np.isinf(got["z"][[1, 2]]).all()
    assert nan["g"][0].tolist() == [False, True, False] and nan["hly"][0].tolist() == [False, True, False]
    assert nan["gy"][0] and nan["hyy"][0] and not nan["hll"][0].any()
    assert np.isinf(got["g"][1]).tolist() == [False, True, False] and not nan["g"][1].any()
    assert np.isinf(got["g"][2]).all() and nan["g"][3].all()                    # u / 0 and 0 / 0
    assert got["z"][4] == (1.5 ** 2 + 4.0 + 0.0625) / -4.0 and got["z"][5] == 7.0
    return ev


def _oracle(a):
    from oracle.oracle_capi import OracleProblem
    return OracleProblem(serialize(a))


def test_host_build_against_mpmath_on_the_grid():
    check_grid("host build", _oracle)


def test_host_build_planted_rows():
    check_planted("host build", _oracle)


@pytest.mark.parametrize("axis", [None, 0])
def test_host_build_other_axes(axis):
    tape = qp.rows_tape([qr.rows_of_shape(1 if axis is None else 6, 5)], axis=axis)
    qr.check_segment("host build axis %r" % axis, _oracle(tape[0]), tape)


# ---- 5. host-build solves -------------------------------------------------------------------------------------------------------
def _solve_both(build, **opts):
    """The rows statement and the loop of scalar norms of the same problem by the host build -> the rows statement's
    (value, canonical x, problem objects); the two values must agree to the closed forms' tolerance."""
    out = []
    for loop in (False, True):
        made = build(loop)
        obj, status, iters, xv = oracle_solver(made[0], **opts)
        assert status == 0, (loop, status)
        out.append((obj, xv, made))
    ops = [list(lp.lower(o[2][0])["tape_arrays"]["seg_op"]) for o in out]
    assert 36 in ops[0] and 36 not in ops[1] and 32 in ops[1]
    assert abs(out[0][0] - out[1][0]) <= qp.VALUE_TOL * abs(out[1][0]), (out[0][0], out[1][0])
    return out


def test_host_build_fermat_weber():
    obj, xv, (prob, p) = _solve_both(lambda loop: qp.fermat_weber(loop))[0]
    qp.assert_optimum("Fermat-Weber", obj, qp.FW_VALUE, lp.value_in(prob, p, xv), qp.FW_POINT)


def test_host_build_enclosing_circle():
    """Both statements, each held to the closed form (qol_rows_problems.CIRCLE_OPTS says why this instance is solved at a
    tighter tolerance than the default)."""
    for (obj, xv, (prob, c, r)), name in zip(_solve_both(lambda loop: qp.enclosing_circle(loop), **qp.CIRCLE_OPTS), ("rows", "loop")):
        qp.assert_circle(name, obj, lp.value_in(prob, c, xv))


@pytest.mark.parametrize("axis", [1, 0])
def test_host_build_group_lasso(axis):
    obj, xv, (prob, X) = _solve_both(lambda loop: qp.group_lasso(axis, loop))[0]
    Xs, vs = qp.lasso_optimum()
    qp.assert_optimum("group lasso, axis %d" % axis, obj, vs, lp.value_in(prob, X, xv), Xs if axis == 1 else Xs.T)


def test_host_build_parametrised_fermat_weber():
    """Anchors as a Parameter: a shifted and scaled square has its centre as the point; both statements."""
    def build(loop):
        prob, p, params = qp.fermat_weber(loop=loop, parameters=True)
        params[0].value = 3.0 * qp.SQUARE + np.array([1.0, -2.0])
        return prob, p
    for (obj, xv, (prob, p)), name in zip(_solve_both(build), ("rows", "loop")):
        qp.assert_optimum("Fermat-Weber, parametrised, " + name, obj, 3.0 * qp.FW_VALUE, lp.value_in(prob, p, xv), np.array([2.5, -0.5]))
