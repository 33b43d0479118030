"""prod without a GPU: the front-end atom and its rule tags, the canonical form, the tape layout of the second row-class
member (OP_PROD = 35: the strict lower triangle), the rule of the host build (csrc/model.h sweep_prod_segment over host
loops) entry by entry against mpmath (tests/prod_reference.py: the definition, the rows, the derived bound), and solves by
the host build with closed forms and certificates written out in numpy (tests/prod_problems.py)."""
import numpy as np
import pytest

import dnlp_amd as cp
import lse_problems as lp
import lse_reference as lr
import prod_problems as pp
import prod_reference as pr
from batch_problems import oracle_solver
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.tape import serialize


# ---- 1. front-end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, 0, 1])
@pytest.mark.parametrize("keepdims", [False, True])
def test_value_and_shape(axis, keepdims):
    v = np.random.default_rng(3).standard_normal((4, 6)) * 3
    X = cp.Variable((4, 6))
    X.value = v
    e = cp.prod(X, axis=axis, keepdims=keepdims)
    want = np.prod(v, axis=axis, keepdims=keepdims)
    assert isinstance(e, cp.Prod) and e.shape == np.shape(want)
    assert np.array_equal(np.asarray(e.value), np.asarray(want))
    assert e.shape == cp.sum(X, axis=axis, keepdims=keepdims).shape


def test_list_form_is_the_product_of_the_stacked_entries():
    x, y = cp.Variable(2), cp.Variable()
    x.value, y.value = np.array([2.0, -3.0]), 0.5
    e = cp.prod([x, y])
    assert isinstance(e, cp.Prod) and e.shape == () and type(e.args[0]).__name__ == "Hstack" and e.args[0].shape == (3,)
    assert float(e.value) == -3.0


def test_sign_curvature_and_rule_table():
    x, X = cp.Variable(5), cp.Variable((3, 4))
    e = cp.prod(x)
    assert not e.is_convex() and not e.is_concave() and not e.is_nonneg() and not e.is_nonpos()
    assert cp.prod(cp.abs(x)).is_nonneg() and not cp.prod(-cp.abs(x)).is_nonpos()
    assert e.is_atom_esr() and e.is_atom_hsr() and not e.is_incr(0) and not e.is_decr(0)
    pos = cp.prod(cp.Variable(5, nonneg=True))
    assert pos.is_incr(0) and not pos.is_decr(0)
    assert e.is_smooth()
    a = cp.prod(cp.abs(x))
    assert a.is_esr() and not a.is_hsr()
    assert cp.Problem(cp.Minimize(a)).is_dnlp()
    assert cp.Problem(cp.Minimize(e)).is_dnlp() and cp.Problem(cp.Maximize(e)).is_dnlp()      # nonconvex, accepted both ways
    inner = cp.prod(cp.max(X, axis=1))                   # sign unknown and nonsmooth: no composition rule applies
    assert not inner.is_esr() and not inner.is_hsr()
    with pytest.raises(cp.DNLPError):
        cp.Problem(cp.Minimize(inner)).solve(nlp=True)


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------
def test_canonical_form_aliases_the_argument():
    rng = np.random.default_rng(4)
    A, b = rng.standard_normal((6, 3)), rng.standard_normal(6)
    x = cp.Variable(3)
    x.value = rng.standard_normal(3)
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.prod(A @ x + b)), [x >= -5]))
    assert len(smooth.constraints) == 2                                  # t == A x + b first, then the user's row
    t = smooth.objective.expr.args[0]
    assert isinstance(t, cp.Variable) and t.shape == (6,) and t.bounds is None          # no domain, no bounds
    assert np.array_equal(t.value, A @ x.value + b)
    # a bare variable is kept
    smooth2, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.prod(x))))
    assert smooth2.objective.expr.args[0] is x and not smooth2.constraints
    # a matrix argument with an axis: one auxiliary variable of the argument's size
    X = cp.Variable((3, 2))
    X.value = np.ones((3, 2))
    smooth3, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.prod(A @ X, axis=1)))))
    assert len(smooth3.constraints) == 1 and smooth3.variables()[0].size + smooth3.variables()[1].size == 6 + 12


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------
def _expected_pattern(a, s):
    op, M, K = int(a["seg_op"][s]), int(a["seg_d0"][s]), int(a["seg_d1"][s])
    off = int(a["seg_a0_off"][s])
    idx = np.asarray(a["gidx"][off:off + M * K], dtype=np.int64).reshape(M, K)
    zo = int(a["seg_zoff"][s])
    ii, jj = np.tril_indices(K, -1 if op == 35 else 0)
    z = zo + np.arange(M)
    hr, hc = idx[:, ii].reshape(-1), idx[:, jj].reshape(-1)
    return (np.repeat(z, K), idx.reshape(-1), np.maximum(hr, hc), np.minimum(hr, hc), np.repeat(z, ii.size)), idx


@pytest.mark.parametrize("axis", [None, 0, 1])
def test_tape_layout(axis):
    shape = (5,) if axis is None else (4, 3)
    X = cp.Variable(shape)
    X.value = np.arange(np.prod(shape), dtype=float).reshape(shape)
    Y = cp.Variable(shape)
    Y.value = np.ones(shape)
    prob = cp.Problem(cp.Minimize(cp.sum(cp.prod(X, axis=axis))), [cp.prod(Y, axis=axis) <= 1])
    a = lp.lower(prob)["tape_arrays"]
    M, K = {None: (1, 5), 0: (3, 4), 1: (4, 3)}[axis]
    T = K * (K - 1) // 2
    assert list(a["seg_op"]) == [35, 35] and list(a["seg_d0"]) == [M, M] and list(a["seg_d1"]) == [K, K]
    assert list(a["seg_n"]) == [M, M] and list(a["seg_zcount"]) == [M, M]
    assert list(a["seg_dcount"]) == [M * K] * 2 and list(a["seg_hcount"]) == [M * T] * 2
    assert list(a["seg_zoff"]) == [0, M] and list(a["seg_doff"]) == [0, M * K] and list(a["seg_hoff"]) == [0, M * T]
    assert int(a["dims"][4]) == 2 * M * K and int(a["dims"][5]) == 2 * M * T
    want = [np.concatenate(parts) for parts in zip(*[_expected_pattern(a, s)[0] for s in range(2)])]
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), want):
        assert np.array_equal(a[name], w), name
    assert np.all(a["hrow"] > a["hcol"])                                  # no diagonal entry anywhere
    # row r of the atom reads the entries the axis says (the variable X starts at x index 0, F order)
    idx = _expected_pattern(a, 0)[1]
    full = np.arange(np.prod(shape)).reshape(shape, order="F")
    rows = full.reshape(1, -1) if axis is None else (full.T if axis == 0 else full)
    assert np.array_equal(idx, rows)


def test_single_entry_rows_have_no_hessian_entries():
    X = cp.Variable((4, 1))
    X.value = np.ones((4, 1))
    a = lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.prod(X, axis=1)))))["tape_arrays"]
    assert list(a["seg_op"]) == [35] and (int(a["seg_d0"][0]), int(a["seg_d1"][0])) == (4, 1)
    assert int(a["seg_hcount"][0]) == 0 and int(a["seg_dcount"][0]) == 4 and a["hrow"].size == 0 and a["hz"].size == 0


def test_repeated_index_is_refused():
    x = cp.Variable(3)
    x.value = np.ones(3)
    from dnlp_amd.lowering import lower_problem
    with pytest.raises(ValueError, match="prod.*twice"):
        lower_problem(cp.prod(cp.hstack([x[0], x[1], x[0]])), [], [x])


def test_empty_argument_is_refused():
    x = cp.Variable((0, 3))
    from dnlp_amd.lowering import lower_problem
    with pytest.raises(ValueError, match="prod of an empty argument"):
        lower_problem(cp.sum(cp.prod(x, axis=0)), [], [x])


def test_hessian_count_beyond_the_index_range_is_refused():
    x = cp.Variable(70000)
    from dnlp_amd.lowering import lower_problem
    with pytest.raises(ValueError, match="prod.*70000.*2449965000"):
        lower_problem(cp.prod(x), [], [x])


def test_tape_with_both_row_class_members():
    """op 34 and op 35 segments in one tape: each keeps its own triangle; the host build evaluates both."""
    from oracle.oracle_capi import OracleProblem
    A, B = cp.Variable((3, 4)), cp.Variable((3, 4))
    rows = pr.rows_of_length(4, 3)
    A.value, B.value = rows, rows
    prob = cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [cp.log_sum_exp(A, axis=1) <= 0, cp.prod(B, axis=1) <= 0])
    data = lp.lower(prob)
    a = data["tape_arrays"]
    assert list(a["seg_op"]) == [34, 35] and list(a["seg_hcount"]) == [3 * 10, 3 * 6] and list(a["seg_hoff"]) == [0, 30]
    want = [np.concatenate(parts) for parts in zip(*[_expected_pattern(a, s)[0] for s in range(2)])]
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), want):
        assert np.array_equal(a[name], w), name
    x = np.array(data["x0"], dtype=float)
    o = OracleProblem(serialize(a))
    g, J = o.eval_g(x), o.eval_jac_g(x)
    from scipy.special import logsumexp, softmax
    sign = a["G_val"]
    assert np.all(np.abs(sign) == 1.0)
    assert np.allclose(sign[:3] * g[:3], logsumexp(rows, axis=1), rtol=1e-14)
    assert np.allclose(sign[3:] * g[3:], np.prod(rows, axis=1), rtol=1e-14)
    assert J.size == 24
    byrow = {r: J[np.asarray(a["jac_rows"]) == r] for r in range(6)}
    for r in range(3):
        assert np.allclose(np.sort(sign[r] * byrow[r]), np.sort(softmax(rows[r])), rtol=1e-13)
        assert np.allclose(np.sort(sign[3 + r] * byrow[3 + r]), np.sort(np.prod(rows[r]) / rows[r]), rtol=1e-13)
    assert o.eval_h(x, lp.multipliers(6), 0.5).size == int(a["dims"][7])


# ---- 4. rule ------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_within_the_derived_bound():
    table = pr.numpy_table()
    for kind, (worst, share, points) in table.items():
        print("%-6s worst %.2f eps relative, %.3f %% of %d points left out" % (kind, worst, 100 * share, points))
        assert share <= pr.LEFT_OUT_SHARE, (kind, share)


_tapes = {}


def grid_tape():
    """The grid rows and the planted rows as constraints, and the rows of lengths 3, 16 and 65 once more in the objective."""
    if "grid" not in _tapes:
        sets = [rows for n, rows in pr.grid()]
        _tapes["grid"] = pp.rows_tape(sets, [pr.rows_of_length(n) for n in (3, 16, 65)])
    return _tapes["grid"]


def planted_tape():
    if "planted" not in _tapes:
        _tapes["planted"] = pp.rows_tape([pr.planted_rows(), np.array([[0.0], [2.5], [-1.0], [1.0]])])
    return _tapes["planted"]


def check_callbacks(ev, tape, with_f=True, hsample=None):
    a, x, lam, sigma = tape
    exp = pr.expected_oracles(a, x, lam, sigma, hsample)
    for units, kind in zip(exp["units"], ("value", "d1", "d2")):
        ref = units.st != 2
        share = float(np.mean(units.st[ref] == 1)) if ref.any() else 0.0
        assert share <= pr.LEFT_OUT_SHARE, "%s: %.2f %% of the points left out" % (kind, 100 * share)
    failed = []
    checks = [("g", lambda: ev.eval_g(x)), ("jac", lambda: ev.eval_jac_g(x)), ("hess", lambda: ev.eval_h(x, lam, sigma))]
    if with_f:
        checks += [("f", lambda: [ev.eval_f(x)]), ("grad_f", lambda: ev.eval_grad_f(x))]
    for name, thunk in checks:
        try:
            print("%s: worst error %.3f of its bound" % (name, exp[name].check(thunk())))
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


def test_host_build_against_mpmath_on_the_grid():
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(grid_tape()[0])), grid_tape())


def test_host_build_planted_rows_are_exact_where_the_reference_is_zero():
    """0, 1, 2 and 3 zeros in first, middle and last position, negative entries, all ones, K = 1: the bound, and every
    entry whose reference is 0 is 0."""
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = planted_tape()
    o = OracleProblem(serialize(a))
    check_callbacks(o, planted_tape())
    exp = pr.expected_oracles(a, x, lam, sigma)
    for name, got in (("g", o.eval_g(x)), ("jac", o.eval_jac_g(x)), ("hess", o.eval_h(x, lam, sigma))):
        zero = exp[name].hi == 0
        assert zero.any() and not np.asarray(got)[zero].any(), name
    # K = 1: z = u, d = 1 (also at u = 0), no Hessian entry
    sign = a["G_val"]
    g, J = o.eval_g(x), o.eval_jac_g(x)
    assert np.array_equal(sign[-4:] * g[-4:], [0.0, 2.5, -1.0, 1.0]) and np.array_equal(sign[-4:] * J[-4:], np.ones(4))


def test_host_build_nan_and_inf_entries():
    """a NaN entry makes the row's value NaN, with or without a zero beside it; +-inf is a nonzero
    entry (beside a zero the value is 0); the clean row is untouched."""
    from oracle.oracle_capi import OracleProblem
    rows = np.array([[0.5, np.nan, 2.0], [0.0, np.nan, 2.0], [0.5, np.inf, 2.0], [0.0, -np.inf, 2.0], [1.0, 2.0, 3.0]])
    a, x, lam, sigma = pp.rows_tape([rows])
    o = OracleProblem(serialize(a))
    g, J = o.eval_g(x), o.eval_jac_g(x)
    sign = a["G_val"]
    assert np.isnan(g[0]) and np.isnan(g[1]) and sign[2] * g[2] == np.inf and g[3] == 0.0 and sign[4] * g[4] == 6.0
    assert np.isnan(J[:6]).all() and np.array_equal(np.sort(sign[4] * J[-3:]), [2.0, 3.0, 6.0])


def test_rows_that_share_entries_beyond_the_scratch_are_refused_at_load():
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = pp.rows_tape([pr.rows_of_length(2, 3)])
    a = dict(a)
    assert int(a["dims"][0]) == 7
    OracleProblem(serialize(a))                                   # 2 * 3 <= 7: fine
    a["dims"] = a["dims"].copy()
    a["dims"][0] = 5
    with pytest.raises(Exception, match="prod segment.*share entries"):
        OracleProblem(serialize(a))


# ---- 5. host-build solves -------------------------------------------------------------------------------------------------------
def _oracle_solve(prob):
    from oracle.oracle_capi import OracleProblem
    mini = cp.Problem(cp.Minimize(-prob.objective.expr), prob.constraints) if isinstance(prob.objective, cp.Maximize) else prob
    data = lp.lower(mini)
    info = OracleProblem(serialize(data["tape_arrays"])).solve(data["x0"])
    return info, data


def test_host_build_box_volume():
    prob, x = pp.box_problem()
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    pp.assert_box(lp.value_in(prob, x, xv), abs(obj))


def test_host_build_amgm_with_an_axis():
    prob, X = pp.amgm_problem()
    info, data = _oracle_solve(prob)
    assert info["status"] == 0
    Xv = lp.value_in(prob, X, info["x"])
    pp.assert_amgm(Xv, float(np.sum(Xv)), np.asarray(info["mult_g"])[:pp.AMGM_B.size])


def test_host_build_nonconvex_sphere():
    prob, x = pp.sphere_problem()
    info, data = _oracle_solve(prob)
    assert info["status"] == 0
    pp.assert_sphere_kkt(lp.value_in(prob, x, info["x"]), info["mult_g"][-1])


def test_host_build_parametrised_box_volume():
    prob, x, params = pp.box_problem(parameters=True)
    params[0].value, params[1].value = np.array([2.0, 1.0, 1.0, 0.5]), np.array([9.0])
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    pp.assert_box(lp.value_in(prob, x, xv), abs(obj), params[0].value, 9.0)
