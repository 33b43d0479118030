"""matrix_frac and tr_inv without a GPU: the front-end atom and its rule tags, the rewrite of a constant P, the canonical
form (X aliased, P replaced by a new variable with the symmetrising row), the tape layout of the fifth row-class member
(OP_MATRIX_FRAC = 38: one row of n^2 + n m entries, d2 = n), the refusals of the lowering and of the tape load, the rule
of the host build (csrc/row_class.h mfrac_row / mfrac_d / mfrac_h through csrc/model.h sweep_mfrac_segment over host
loops) entry by entry against mpmath within the brackets of tests/matrix_frac_reference.py, the out-of-domain table, the
bits of log_det (whose elimination step the new rule shares) against those recorded before the step was shared, and solves
by the host build with closed forms (tests/matrix_frac_problems.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import dnlp_amd as cp
import logdet_reference as lr
import lse_problems as lp
import matrix_frac_problems as mq
import matrix_frac_reference as mr
from batch_problems import oracle_solver
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.tape import serialize

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "log_det_host_bits.json")


def _host(a):
    from oracle.oracle_capi import OracleProblem
    return OracleProblem(serialize(a))


# ---- 1. front-end -----------------------------------------------------------------------------------------------------------
def test_value_shape_sign_and_curvature():
    P, X = mr.inputs_of(4, 2, 10.0, True)
    Pv, Xv = cp.Variable((4, 4)), cp.Variable((4, 2))
    Pv.value, Xv.value = P, X
    e = cp.matrix_frac(Xv, Pv)
    assert e.shape == () and isinstance(e, cp.MatrixFrac)
    want = np.trace(X.T @ np.linalg.inv((P + P.T) / 2) @ X)               # the symmetric part, as log_det's numeric
    assert abs(float(e.value) - want) <= 1e-13 * want
    assert e.is_convex() and not e.is_concave() and e.is_atom_convex() and not e.is_atom_concave()
    assert e.is_nonneg() and not e.is_nonpos()
    assert not e.is_incr(0) and not e.is_decr(0) and not e.is_incr(1) and not e.is_decr(1)
    assert e.is_atom_esr() and e.is_atom_hsr() and e.is_smooth()
    for bad in (np.diag([-1.0, -1.0, 1.0, 1.0]), np.zeros((4, 4)), np.diag([1.0, 2.0, -3.0, 4.0])):
        Pv.value = bad
        assert float(e.value) == np.inf
    xv = cp.Variable(4)                                                   # a 1-D X of length n is n x 1
    xv.value, Pv.value = X[:, 0], P
    want1 = X[:, 0] @ np.linalg.inv((P + P.T) / 2) @ X[:, 0]
    assert abs(float(cp.matrix_frac(xv, Pv).value) - want1) <= 1e-13 * want1


def test_validation_messages_of_the_reference():
    with pytest.raises(ValueError, match="The second argument to matrix_frac must be a square matrix."):
        cp.matrix_frac(cp.Variable(3), cp.Variable((3, 2)))
    with pytest.raises(ValueError, match="The second argument to matrix_frac must be a square matrix."):
        cp.matrix_frac(cp.Variable(3), cp.Variable(3))
    with pytest.raises(ValueError, match="The arguments to matrix_frac have incompatible dimensions."):
        cp.matrix_frac(cp.Variable((4, 2)), cp.Variable((3, 3)))
    with pytest.raises(ValueError, match="The arguments to matrix_frac have incompatible dimensions."):
        cp.matrix_frac(np.ones(4), np.eye(3))                             # the constant rewrite validates as the atom does
    with pytest.raises(ValueError, match=r"The argument .* to tr_inv must be a 2-d square array."):
        cp.tr_inv(cp.Variable((2, 3)))
    with pytest.raises(ValueError, match=r"to tr_inv must be a 2-d square array."):
        cp.tr_inv(cp.Variable(3))


def test_dnlp_accepts_smooth_arguments_and_refuses_a_nonsmooth_one():
    x, S = cp.Variable(3), cp.Variable((3, 3))
    A = np.random.default_rng(1).standard_normal((3, 3))
    assert cp.Problem(cp.Minimize(cp.matrix_frac(A @ x - 1, S + np.eye(3)))).is_dnlp()
    assert cp.Problem(cp.Minimize(cp.tr_inv(S))).is_dnlp()
    assert cp.Problem(cp.Minimize(cp.sum(x)), [cp.matrix_frac(x, S) <= 1]).is_dnlp()
    inner = cp.matrix_frac(cp.abs(x), S)                                  # neither increasing nor decreasing: no rule applies
    assert not inner.is_esr() and not inner.is_hsr()
    assert not cp.Problem(cp.Minimize(inner)).is_dnlp()
    with pytest.raises(cp.DNLPError):
        cp.Problem(cp.Minimize(inner)).solve(nlp=True)


def test_constant_P_is_rewritten_to_a_sum_of_squares():
    P, X = mr.inputs_of(4, 2, 100.0, True)
    Xv = cp.Variable((4, 2))
    Xv.value = X
    want = np.trace(X.T @ np.linalg.inv((P + P.T) / 2) @ X)
    for const in (P, cp.Constant(P), cp.Constant(P) + np.zeros((4, 4))):
        e = cp.matrix_frac(Xv, const)
        assert not isinstance(e, cp.MatrixFrac) and e.shape == ()
        assert abs(float(e.value) - want) <= 1e-12 * want
        a = lp.lower(cp.Problem(cp.Minimize(e)))["tape_arrays"]
        assert 38 not in [int(v) for v in a["seg_op"]]
    with pytest.raises(ValueError, match="matrix_frac.*not positive definite"):
        cp.matrix_frac(Xv, np.diag([1.0, -1.0, 1.0, 1.0]))
    assert isinstance(cp.matrix_frac(Xv, cp.Parameter((4, 4), value=P)), cp.MatrixFrac)       # a parameter is not a constant here


def test_tr_inv_is_matrix_frac_of_the_identity():
    P = lr.matrix(3, 10.0, False)
    Pv = cp.Variable((3, 3))
    Pv.value = P
    e = cp.tr_inv(Pv)
    assert isinstance(e, cp.MatrixFrac) and e.shape == () and e.is_convex() and e.is_nonneg()
    assert abs(float(e.value) - np.trace(np.linalg.inv(P))) <= 1e-13 * np.trace(np.linalg.inv(P))
    assert abs(float(cp.tr_inv(P).value) - np.trace(np.linalg.inv(P))) <= 1e-13 * np.trace(np.linalg.inv(P))
    a = lp.lower(cp.Problem(cp.Minimize(e)))["tape_arrays"]
    assert list(a["seg_op"]) == [38] and (int(a["seg_d1"][0]), int(a["seg_d2"][0])) == (18, 3)          # N = 2 n


def test_the_fused_builder_knows_no_matrix_frac():
    from dnlp_amd.fused import build_fused_spec
    S = cp.Variable((3, 3))
    S.value = np.eye(3)
    assert build_fused_spec(cp.Problem(cp.Minimize(cp.tr_inv(S)))) is None


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------
def _canon(X_expr, P_expr):
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.matrix_frac(X_expr, P_expr))))
    atom = smooth.objective.expr
    assert isinstance(atom, cp.MatrixFrac)
    return smooth, atom.args[0], atom.args[1]


def test_canonical_form_with_a_bare_variable_X():
    X, P = cp.Variable((3, 2)), cp.Variable((3, 3))
    A = lr.matrix(3, 100.0, True)
    P.value = A
    smooth, Xc, T = _canon(X, P)
    assert Xc is X                                                         # a bare Variable stays
    assert isinstance(T, cp.Variable) and T is not P and T.shape == (3, 3) and T.bounds is None      # P is always replaced
    assert len(smooth.constraints) == 1                                    # the row T == (P + P^T) / 2
    assert np.array_equal(T.value, (A + A.T) / 2)                          # the symmetric part where its Cholesky factor exists
    P.value = np.diag([1.0, -2.0, 3.0])
    assert np.array_equal(_canon(X, P)[2].value, np.eye(3))                # otherwise the identity
    assert np.array_equal(_canon(X, cp.Variable((3, 3)))[2].value, np.eye(3))          # and without a value
    arr = lp.lower(cp.Problem(cp.Minimize(cp.matrix_frac(X, P))))["tape_arrays"]
    assert list(arr["cl"]) == [0.0] * 9 and list(arr["cu"]) == [0.0] * 9
    assert np.all(arr["lb"] <= -1e19) and np.all(arr["ub"] >= 1e19)        # no bounds on T


@pytest.mark.parametrize("kind", ["affine", "constant"])
def test_canonical_form_aliases_any_other_X(kind):
    """Rows in argument order: t == X first, then T == (P + P^T) / 2; t starts at X's value."""
    x, P = cp.Variable(2), cp.Variable((3, 3))
    x.value = np.array([0.5, -1.5])
    A = np.random.default_rng(4).standard_normal((3, 2))
    Xe = A @ x + 1 if kind == "affine" else cp.Constant(np.array([1.0, -2.0, 3.0]))
    smooth, t, T = _canon(Xe, P)
    assert isinstance(t, cp.Variable) and isinstance(T, cp.Variable) and t is not T and t.bounds is None
    assert t.shape == (3,) and np.array_equal(t.value, Xe.value)
    assert len(smooth.constraints) == 2
    arr = lp.lower(cp.Problem(cp.Minimize(cp.matrix_frac(Xe, P))))          # (canonicalised anew: other t and T, the same layout)
    a, offs = arr["tape_arrays"], arr["tape"].var_offsets
    N = int(a["dims"][0])
    assert int(a["dims"][1]) == 3 + 9 and list(a["cl"]) == [0.0] * 12 and list(a["cu"]) == [0.0] * 12
    # every entry of the tape row is an x index: T's nine entries, then t's three, each variable contiguous in x
    off = int(a["seg_a0_off"][0])
    row = [int(v) for v in a["gidx"][off:off + 12]]
    oT, ot, oP = row[0], row[9], offs[id(P)]
    assert row == list(range(oT, oT + 9)) + list(range(ot, ot + 3)) and len({oT, ot, oP}) == 3
    assert N == 9 + 9 + 3 + (2 if kind == "affine" else 0)
    # in numbers, at any point: the first three rows are t - X, the next nine T - (P + P^T) / 2 (up to the rows' signs)
    xs = np.random.default_rng(5).standard_normal(N)
    g = _host(a).eval_g(xs)
    Pv, Tv = xs[oP:oP + 9].reshape(3, 3, order="F"), xs[oT:oT + 9].reshape(3, 3, order="F")
    Xv = (A @ xs[offs[id(x)]:offs[id(x)] + 2] + 1) if kind == "affine" else np.array([1.0, -2.0, 3.0])
    want = np.concatenate([xs[ot:ot + 3] - Xv, (Tv - (Pv + Pv.T) / 2).reshape(-1, order="F")])
    assert np.allclose(np.abs(g), np.abs(want), rtol=0, atol=1e-14)


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------
def test_tape_layout_of_a_two_by_two_with_one_column():
    P, X = mr.inputs_of(2, 1, 10.0, True)
    a, x, lam, sigma = mq.segments_tape([(P, X)], [(P, X)])
    n, m, K = 2, 1, 6
    T = K * (K + 1) // 2
    assert list(a["seg_op"]) == [38, 38]
    assert list(a["seg_d0"]) == [1, 1] and list(a["seg_d1"]) == [K, K] and list(a["seg_d2"]) == [n, n]       # m = (K - n^2) / n
    assert list(a["seg_n"]) == [1, 1] and list(a["seg_zcount"]) == [1, 1]
    assert list(a["seg_dcount"]) == [K, K] and list(a["seg_hcount"]) == [T, T]
    assert list(a["seg_zoff"]) == [0, 1] and list(a["seg_doff"]) == [0, K] and list(a["seg_hoff"]) == [0, T]
    ii, jj = np.tril_indices(K)
    want = [[], [], [], [], []]
    for s in range(2):
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
        # the gather order: P's entries in F order (the variable T, contiguous in x), then X's in F order
        assert np.array_equal(idx[:4], idx[0] + np.arange(4)) and np.array_equal(idx[4:], idx[4] + np.arange(2))
        assert np.array_equal(x[idx], mr.row_of(P, X))
        parts = (np.full(K, s), idx, np.maximum(idx[ii], idx[jj]), np.minimum(idx[ii], idx[jj]), np.full(T, s))
        for acc, part in zip(want, parts):
            acc.append(part)
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), want):
        assert np.array_equal(a[name], np.concatenate(w)), name
    # d: -G at i + j n, W + V at n^2 + i + c n; h: the packed triangle with its diagonal, row-major -- in numbers
    B = np.linalg.inv(P)
    W, V = B @ X, B.T @ X
    ev = _host(a)
    gf = ev.eval_grad_f(x)
    off = int(a["seg_a0_off"][0])
    idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
    want_d = np.concatenate([(-(V @ W.T)).reshape(-1, order="F"), (W + V).reshape(-1, order="F")])
    assert np.allclose(gf[idx], want_d, rtol=1e-12, atol=0)
    z, d, h = mr.numpy_rule(P, X, 1.0)
    H = ev.eval_h(x, 0 * lam, 1.0)
    hr, hc = np.asarray(a["hess_rows"]), np.asarray(a["hess_cols"])
    for q, (p_, q_) in enumerate(zip(ii, jj)):
        r, c = max(idx[p_], idx[q_]), min(idx[p_], idx[q_])
        (pos,) = np.nonzero((hr == r) & (hc == c))
        assert abs(H[pos[0]] - h[q]) <= 1e-12 * max(1.0, abs(h[q])), (p_, q_)


@pytest.mark.parametrize("n,m", [(45, 1), (44, 2), (1, 45)])
def test_bordered_order_46_is_refused_by_the_lowering(n, m):
    with pytest.raises(ValueError, match=r"matrix_frac: P of order %d with %d column\(s\).*order 46 with 2116 entries.*2048.*n \+ m <= 45.*"
                                         r"order 44 with one column.*split by columns" % (n, m)):
        lp.lower(cp.Problem(cp.Minimize(cp.matrix_frac(cp.Variable((n, m)), cp.Variable((n, n))))))


def test_the_largest_accepted_shapes_and_the_other_refusals():
    from dnlp_amd.lowering import lower_problem
    for n, m in ((44, 1), (1, 44), (22, 23)):
        a = lp.lower(cp.Problem(cp.Minimize(cp.matrix_frac(cp.Variable((n, m)), cp.Variable((n, n))))))["tape_arrays"]
        assert list(a["seg_d1"]) == [n * (n + m)] and list(a["seg_d2"]) == [n]
    with pytest.raises(ValueError, match="tr_inv|matrix_frac"):           # N = 2 n: tr_inv ends at order 22
        lp.lower(cp.Problem(cp.Minimize(cp.tr_inv(cp.Variable((23, 23))))))
    with pytest.raises(ValueError, match="matrix_frac of an empty argument"):
        lower_problem(cp.MatrixFrac(cp.Variable((0, 2)), cp.Variable((0, 0))), [], [])
    with pytest.raises(ValueError, match="matrix_frac of an empty argument"):
        lower_problem(cp.MatrixFrac(cp.Variable((3, 0)), cp.Variable((3, 3))), [], [])
    x = cp.Variable(4)
    x.value = np.ones(4)
    with pytest.raises(ValueError, match="matrix_frac.*twice"):
        lower_problem(cp.MatrixFrac(x[:2], cp.reshape(x, (2, 2), order="F")), [], [x])


@pytest.mark.parametrize("field,value,message", [
    ("seg_d2", 5, r"matrix_frac segment.*d1 % d2 != 0"),
    ("seg_d2", 0, r"matrix_frac segment.*d1 % d2 != 0"),
    ("seg_d2", 4, r"matrix_frac segment.*d1 < d2 \* d2"),
    ("seg_d2", 6, r"matrix_frac segment.*d1 < d2 \* d2"),
    ("seg_d0", 2, r"matrix_frac segment"),
])
def test_hand_edited_tapes_are_refused_at_load(field, value, message):
    a, x, lam, sigma = mq.segments_tape([mr.inputs_of(3, 1, 10.0, False)])       # K = 12
    _host(a)
    a = dict(a)
    a[field] = a[field].copy()
    a[field][0] = value
    with pytest.raises(Exception, match=message):
        _host(a)


def test_load_refuses_more_than_one_matrix_and_a_bordered_matrix_beyond_one_wavefront():
    X = cp.Variable((2, 12))
    X.value = np.ones((2, 12))
    a = dict(lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.log_sum_exp(X, axis=1)))))["tape_arrays"])
    _host(a)
    for name, v in (("seg_op", 38), ("seg_d2", 3)):
        a[name] = a[name].copy()
        a[name][0] = v
    with pytest.raises(Exception, match="matrix_frac segment with more than one matrix: M != 1"):
        _host(a)
    Y = cp.Variable((1, 100))                                              # d2 = 2: N = 50, N^2 = 2500 > 2048
    Y.value = np.ones((1, 100))
    b = dict(lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.log_sum_exp(Y, axis=1)))))["tape_arrays"])
    for name, v in (("seg_op", 38), ("seg_d2", 2)):
        b[name] = b[name].copy()
        b[name][0] = v
    with pytest.raises(Exception, match=r"matrix_frac segment whose bordered matrix has more than 2048 entries: \(d1 / d2\)\^2 = 2500"):
        _host(b)


# ---- 4. rule ------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_gives_the_written_constants():
    worst, consts = mr.measure_constants()
    print("numpy statement, worst ratios: %r -> constants %r" % (worst, consts))
    assert consts == mr.CONSTS


_tapes = {}


def shape_tape(n, m):
    """The inputs of one shape (four condition numbers, symmetric and not) as constraints and one more in the objective."""
    if (n, m) not in _tapes:
        pairs = [(P, X) for _, _, _, _, P, X in mr.inputs(((n, m),))]
        _tapes[(n, m)] = mq.segments_tape(pairs, [mr.inputs_of(n, m, 10.0, n > 1, seed=mr.SEED + 1)])
    return _tapes[(n, m)]


def check_callbacks(ev, tape, hsample=2000):
    a, x, lam, sigma = tape
    exp = mr.expected_oracles(a, x, lam, sigma, hsample)
    for units in exp["units"]:
        assert not np.any(units.st == 1)                   # no point is left out
    failed = []
    for name, thunk in (("g", lambda: ev.eval_g(x)), ("jac", lambda: ev.eval_jac_g(x)), ("hess", lambda: ev.eval_h(x, lam, sigma)),
                        ("f", lambda: [ev.eval_f(x)]), ("grad_f", lambda: ev.eval_grad_f(x))):
        try:
            print("%s: worst error %.3f of its bound" % (name, exp[name].check(thunk())))
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("n,m", mr.SHAPES)
def test_host_build_against_mpmath(n, m):
    """All d and 2000 seeded Hessian entries (all of them where there are fewer) of every segment."""
    check_callbacks(_host(shape_tape(n, m)[0]), shape_tape(n, m))


# ---- 5. out of the domain -----------------------------------------------------------------------------------------------------
def out_of_domain_pairs(n=3, m=1):
    """-> (pairs, what each gives).  'nan': every output of the segment is NaN -- an indefinite P (its determinant is
    positive), a P whose first pivot is zero, a NaN entry of P.  'x': a NaN entry of X leaves the pivots alone, so the
    outputs are NaN exactly where the rule's arithmetic carries the entry: the value, column c of W and V and what is
    built from them (G, hence every derivative by P; with one column every first derivative), but not the X-X block of
    the Hessian, which holds B alone.  'clean': finite."""
    P, X = mr.inputs_of(n, m, 10.0, True)
    neg = np.eye(n)
    neg[0, 0] = neg[1, 1] = -1.0
    zero = P.copy()
    zero[0, 0] = 0.0
    nanP = P.copy()
    nanP[n - 1, 1] = np.nan
    nanX = X.copy()
    nanX[1, m - 1] = np.nan
    pairs = [(P, X), (neg, X), (zero, X), (nanP, X), (P, nanX), (P.T.copy(), X)]
    return pairs, ("clean", "nan", "nan", "nan", "x", "clean")


def check_out_of_domain(ev, n=3, m=1):
    """What out_of_domain_pairs says, and nothing else is touched: everything else has the bits it has when clean inputs
    stand where the out-of-domain ones stood."""
    import scipy.sparse as sp
    pairs, kinds = out_of_domain_pairs(n, m)
    a, x, lam, sigma = mq.segments_tape(pairs)
    good = mr.inputs_of(n, m, 1.0, False)
    _, xg, _, _ = mq.segments_tape([pr_ if k == "clean" else good for pr_, k in zip(pairs, kinds)])
    h = ev(a)
    try:
        (g, J, H), (gg, Jg, Hg) = [(h.eval_g(v), h.eval_jac_g(v), h.eval_h(v, lam, sigma)) for v in (x, xg)]
    finally:
        if hasattr(h, "close"):
            h.close()
    N, mm, Z = (int(v) for v in a["dims"][:3])
    w = mr.pr.weights(a, lam, sigma)
    G = sp.csr_matrix((a["G_val"], a["G_idx"], a["G_ptr"]), shape=(mm, N + Z)).tocsc()
    jr, jc = np.asarray(a["jac_rows"]), np.asarray(a["jac_cols"])
    hr, hc = np.asarray(a["hess_rows"]), np.asarray(a["hess_cols"])
    hpos = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(hr, hc))}
    seg_g, seg_j, seg_h = np.zeros(mm, dtype=bool), np.zeros(J.size, dtype=bool), np.zeros(H.size, dtype=bool)
    for s, ((P, X), kind) in enumerate(zip(pairs, kinds)):
        if kind == "clean":
            continue
        row = int(G.indices[G.indptr[N + s]])
        K = P.size + X.size
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K])
        jpos = np.array([np.nonzero((jr == row) & (jc == c))[0][0] for c in idx])
        ii, jj = np.tril_indices(K)
        hp = np.array([hpos[(int(max(idx[p], idx[q])), int(min(idx[p], idx[q])))] for p, q in zip(ii, jj)])
        seg_g[row], seg_j[jpos], seg_h[hp] = True, True, True
        if kind == "nan":
            assert np.isnan(g[row]) and np.isnan(J[jpos]).all() and np.isnan(H[hp]).all(), s
        else:
            z0, d0, h0 = mr.numpy_rule(P, X, w[int(a["seg_zoff"][s])])
            assert np.isnan(z0) and np.isnan(d0).any() and np.isnan(h0).any() and not np.isnan(h0).all()
            assert np.isnan(g[row])
            for got, want in ((np.abs(J[jpos]), np.abs(d0)), (H[hp], h0)):
                assert np.array_equal(np.isnan(got), np.isnan(want)), s
                fin = ~np.isnan(want)
                assert np.allclose(got[fin], want[fin], rtol=1e-10, atol=1e-300), s
    # (the affine rows T - (V + V^T) / 2 that read the replaced entries differ between the two points and are not compared)
    moved = np.asarray(abs(sp.csr_matrix(G[:, :N])) @ ((x != xg) | np.isnan(x)).astype(float)).reshape(-1) > 0
    for name, got, ref, mine, skip in (("g", g, gg, seg_g, moved), ("jac", J, Jg, seg_j, False), ("hess", H, Hg, seg_h, False)):
        same = ~mine & ~skip
        assert np.isfinite(ref).all() and got[same].tobytes() == ref[same].tobytes(), name


def test_host_build_out_of_domain_table():
    check_out_of_domain(_host)
    check_out_of_domain(_host, 7, 2)


def test_with_h_off_writes_no_second_derivative():
    a, x, lam, sigma = shape_tape(3, 1)
    fresh, used = _host(a), _host(a)
    used.eval_h(x * 1.01, lam, sigma)
    assert used.eval_jac_g(x).tobytes() == fresh.eval_jac_g(x).tobytes() and used.eval_g(x).tobytes() == fresh.eval_g(x).tobytes()


def mixed_problem():
    """matrix_frac (both kernel forms), log_det, log_sum_exp and quad_over_lin_rows in one tape."""
    rng = np.random.default_rng(9)
    P1, X1 = mr.inputs_of(3, 2, 10.0, False)
    P2, X2 = mr.inputs_of(9, 3, 100.0, False)
    A, Xa, B, Xb = cp.Variable((3, 3)), cp.Variable((3, 2)), cp.Variable((9, 9)), cp.Variable((9, 3))
    A.value, Xa.value, B.value, Xb.value = P1, X1, P2, X2
    D, L, Q = cp.Variable((4, 4)), cp.Variable((3, 5)), cp.Variable((4, 3))
    D.value, L.value, Q.value = lr.matrix(4, 10.0, False), rng.standard_normal((3, 5)), rng.standard_normal((4, 3))
    cons = [cp.matrix_frac(Xa, A) <= 50, cp.log_sum_exp(L, axis=1) <= 3, cp.norm(Q, 2, axis=1) <= 2, cp.log_det(D) >= -5,
            cp.matrix_frac(Xb, B) <= 500]
    return cp.Problem(cp.Minimize(cp.sum_squares(L) + cp.sum(Q)), cons), (A, Xa, B, Xb, D)


def check_mixed(ev):
    prob, (A, Xa, B, Xb, D) = mixed_problem()
    data = lp.lower(prob)
    a = data["tape_arrays"]
    assert sorted(int(v) for v in a["seg_op"] if int(v) >= 34) == [34, 36, 37, 38, 38]
    x = np.array(data["x0"], dtype=float)
    h = ev(a)
    g = h.eval_g(x)
    lam = lp.multipliers(int(a["dims"][1]))
    assert np.isfinite(g).all() and np.isfinite(h.eval_jac_g(x)).all() and np.isfinite(h.eval_h(x, lam, 0.5)).all()
    vals = np.abs(g)
    for want in (abs(np.trace(Xa.value.T @ np.linalg.inv(A.value) @ Xa.value) - 50),
                 abs(np.trace(Xb.value.T @ np.linalg.inv(B.value) @ Xb.value) - 500), abs(np.linalg.slogdet(D.value)[1] + 5)):
        assert np.min(np.abs(vals - want)) <= 1e-11 * max(1.0, want), want
    if hasattr(h, "close"):
        h.close()
    return a, x, lam


def test_tape_with_four_row_class_members_on_the_host():
    check_mixed(_host)


# ---- 6. log_det keeps its bits --------------------------------------------------------------------------------------------------
def logdet_digests():
    """sha256 of the host build's g, Jacobian and Hessian bytes on the log_det tapes of tests/test_log_det_cpu.py."""
    import test_log_det_cpu as tl
    out = {}
    for n in tl.HOST_ORDERS:
        a, x, lam, sigma = tl.order_tape(n)
        ev = _host(a)
        out[str(n)] = [hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
                       for v in (ev.eval_g(x), ev.eval_jac_g(x), ev.eval_h(x, lam, sigma))]
    return out


def test_log_det_is_bit_identical_to_the_build_before_the_step_was_shared():
    """tests/golden/log_det_host_bits.json was recorded with the host build of the commit before csrc/row_class.h
    sweep_step was taken out of logdet_row."""
    with open(GOLDEN) as fh:
        assert logdet_digests() == json.load(fh)


# ---- 7. host-build solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count,width", [(3, 4, None), (6, 10, 4)])
def test_host_build_covariance_form_likelihood(n, count, width):
    """Nonconvex; from S = I the interior-point loop reaches the stationary point S = Y Y^T / N."""
    prob, s = mq.likelihood_problem(n, count, width)
    a = lp.lower(prob)["tape_arrays"]
    assert sorted(int(v) for v in a["seg_op"]) == [37] + [38] * (1 if width is None else -(-count // width))
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    from logdet_problems import matrix_from_entries
    mq.assert_likelihood(matrix_from_entries(lp.value_in(prob, s, xv), n), obj, mq.samples(n, count))


def test_host_build_diagonal_covariance():
    prob, d = mq.diagonal_problem()
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    mq.assert_diagonal(lp.value_in(prob, d, xv), obj)


def test_host_build_generalised_least_squares_through_a_constraint():
    prob, x, t = mq.gls_problem()
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    mq.assert_gls(lp.value_in(prob, x, xv), obj)


@pytest.mark.parametrize("kind", ["unit", "twelve"])
def test_host_build_a_optimal_design(kind):
    V = mq.a_design_points(kind)
    prob, lam = mq.a_design_problem(V)
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    mq.assert_a_design(V, lp.value_in(prob, lam, xv), obj)
