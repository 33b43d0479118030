"""log_det without a GPU: the front-end atom and its rule tags, the canonical form (a new variable with the symmetrising
row), the tape layout of the fourth row-class member (OP_LOG_DET = 37: one row of n^2 entries per matrix, d2 = n), the
refusals of the lowering and of the tape load, the rule of the host build (csrc/row_class.h logdet_row through
csrc/model.h sweep_logdet_segment over host loops) entry by entry against mpmath within the brackets of
tests/logdet_reference.py, the out-of-domain table, and solves by the host build with closed forms
(tests/logdet_problems.py)."""
import numpy as np
import pytest

import dnlp_amd as cp
import logdet_problems as lq
import logdet_reference as lr
import lse_problems as lp
from batch_problems import oracle_solver
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.tape import serialize


# ---- 1. front-end -----------------------------------------------------------------------------------------------------------
def test_value_shape_and_numeric():
    A = lr.matrix(4, 10.0, True)
    X = cp.Variable((4, 4))
    X.value = A
    e = cp.log_det(X)
    assert e.shape == () and isinstance(e, cp.log_det)
    assert abs(float(e.value) - np.linalg.slogdet((A + A.T) / 2)[1]) <= 1e-14 * 10      # the symmetric part, as the reference does
    for bad in (np.diag([-1.0, -1.0, 1.0, 1.0]), np.zeros((4, 4)), np.diag([1.0, 2.0, -3.0, 4.0])):
        X.value = bad
        assert float(e.value) == -np.inf


@pytest.mark.parametrize("shape", [(3,), (2, 3), (), (6, 1)])
def test_non_square_arguments_are_refused(shape):
    with pytest.raises(TypeError, match="The argument to log_det must be a 2-d square array."):
        cp.log_det(cp.Variable(shape))


def test_sign_curvature_and_rule_table():
    X = cp.Variable((3, 3))
    e = cp.log_det(X)
    assert e.is_concave() and not e.is_convex() and e.is_atom_concave() and not e.is_atom_convex()
    assert not e.is_nonneg() and not e.is_nonpos()                    # log det < 0 wherever det < 1
    assert not e.is_incr(0) and not e.is_decr(0)
    assert e.is_atom_esr() and e.is_atom_hsr() and e.is_smooth()
    x = cp.Variable(3)
    W = np.random.default_rng(1).standard_normal((9, 3))
    aff = cp.reshape(W @ x, (3, 3), order="F") + np.eye(3)
    assert cp.Problem(cp.Maximize(cp.log_det(aff))).is_dnlp()
    assert cp.Problem(cp.Minimize(-cp.log_det(aff))).is_dnlp()
    inner = cp.log_det(cp.abs(X))                                     # neither increasing nor decreasing: no rule applies
    assert not inner.is_esr() and not inner.is_hsr()
    assert not cp.Problem(cp.Maximize(inner)).is_dnlp()
    with pytest.raises(cp.DNLPError):
        cp.Problem(cp.Maximize(inner)).solve(nlp=True)


def test_trace_is_the_sum_of_the_diagonal():
    X = cp.Variable((3, 3))
    X.value = np.arange(9.0).reshape(3, 3)
    C = np.random.default_rng(2).standard_normal((3, 3))
    assert cp.trace(X).shape == () and float(cp.trace(X).value) == 12.0 and cp.trace(X).is_affine()
    assert abs(float(cp.trace(C @ X).value) - np.trace(C @ X.value)) <= 1e-13
    with pytest.raises(ValueError, match="square"):
        cp.trace(cp.Variable((2, 3)))


def test_the_fused_builder_knows_no_log_det():
    from dnlp_amd.fused import build_fused_spec
    X = cp.Variable((3, 3))
    X.value = np.eye(3)
    assert build_fused_spec(cp.Problem(cp.Minimize(-cp.log_det(X)))) is None


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------
def _canon(A_expr):
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(-cp.log_det(A_expr))))
    atom = smooth.objective.expr.args[0]
    assert isinstance(atom, cp.log_det)
    return smooth, atom.args[0]


def test_canonical_form_always_introduces_the_symmetrised_variable():
    X = cp.Variable((3, 3))
    X.value = lr.matrix(3, 10.0, True)
    smooth, T = _canon(X)                                  # a bare Variable is replaced too
    assert isinstance(T, cp.Variable) and T is not X and T.shape == (3, 3) and T.bounds is None
    assert len(smooth.constraints) == 1
    a = lp.lower(cp.Problem(cp.Minimize(-cp.log_det(X))))
    arr = a["tape_arrays"]
    # the row T - (X + X^T) / 2 == 0 in numbers: at any point, g = vec(T) - vec of the symmetric part of X
    from oracle.oracle_capi import OracleProblem
    rng = np.random.default_rng(3)
    x = rng.standard_normal(int(arr["dims"][0]))
    offs = a["tape"].var_offsets
    (ox, oT), = [(offs[id(X)], [v for k, v in offs.items() if k != id(X)][0])]
    Xv, Tv = x[ox:ox + 9].reshape(3, 3, order="F"), x[oT:oT + 9].reshape(3, 3, order="F")
    g = OracleProblem(serialize(arr)).eval_g(x)
    want = (Tv - (Xv + Xv.T) / 2).reshape(-1, order="F")
    assert np.allclose(np.abs(g), np.abs(want), rtol=0, atol=1e-15) and np.allclose(g, want * np.sign(g @ want), atol=1e-15)
    assert list(arr["cl"]) == [0.0] * 9 and list(arr["cu"]) == [0.0] * 9
    assert np.all(arr["lb"] <= -1e19) and np.all(arr["ub"] >= 1e19)                 # no bounds on T


def test_start_value_of_the_new_variable():
    X = cp.Variable((3, 3))
    A = lr.matrix(3, 100.0, True)
    X.value = A
    assert np.array_equal(_canon(X)[1].value, (A + A.T) / 2)          # the symmetric part where its Cholesky factor exists
    X.value = np.diag([1.0, -2.0, 3.0])
    assert np.array_equal(_canon(X)[1].value, np.eye(3))              # otherwise the identity
    assert np.array_equal(_canon(cp.Variable((3, 3)))[1].value, np.eye(3))           # and without a value


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tape_layout(n):
    A = lr.matrix(n, 10.0, False)
    a, x, lam, sigma = lq.matrices_tape([A], [A])
    K, T = n * n, n * n * (n * n + 1) // 2
    assert list(a["seg_op"]) == [37, 37]
    assert list(a["seg_d0"]) == [1, 1] and list(a["seg_d1"]) == [K, K] and list(a["seg_d2"]) == [n, n]
    assert list(a["seg_n"]) == [1, 1] and list(a["seg_zcount"]) == [1, 1]
    assert list(a["seg_dcount"]) == [K, K] and list(a["seg_hcount"]) == [T, T]
    assert list(a["seg_zoff"]) == [0, 1] and list(a["seg_doff"]) == [0, K] and list(a["seg_hoff"]) == [0, T]
    assert int(a["dims"][4]) == 2 * K and int(a["dims"][5]) == 2 * T
    ii, jj = np.tril_indices(K)
    want = [[], [], [], [], []]
    for s in range(2):
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
        # entry (i, j) at a0[i + j n]: the F order of the variable T, which lies contiguous in x
        assert np.array_equal(idx, idx[0] + np.arange(K))
        parts = (np.full(K, s), idx, np.maximum(idx[ii], idx[jj]), np.minimum(idx[ii], idx[jj]), np.full(T, s))
        for acc, part in zip(want, parts):
            acc.append(part)
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), want):
        assert np.array_equal(a[name], np.concatenate(w)), name


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_order_46_is_refused_by_the_lowering():
    X = cp.Variable((46, 46))
    with pytest.raises(ValueError, match="log_det.*order 46.*2116 entries.*2048"):
        lp.lower(cp.Problem(cp.Minimize(-cp.log_det(X))))
    Y = cp.Variable((45, 45))
    a = lp.lower(cp.Problem(cp.Minimize(-cp.log_det(Y))))["tape_arrays"]
    assert list(a["seg_d1"]) == [2025] and list(a["seg_d2"]) == [45]


def test_repeated_index_and_empty_argument_are_refused():
    from dnlp_amd.lowering import lower_problem
    x = cp.Variable(3)
    x.value = np.ones(3)
    with pytest.raises(ValueError, match="log_det.*twice"):
        lower_problem(cp.log_det(cp.reshape(cp.hstack([x[0], x[1], x[1], x[2]]), (2, 2), order="F")), [], [x])
    with pytest.raises(ValueError, match="log_det of an empty argument"):
        lower_problem(cp.log_det(cp.Variable((0, 0))), [], [])


@pytest.mark.parametrize("field,value,message", [
    ("seg_d2", 2, "log_det segment.*not a square matrix"),
    ("seg_d2", 0, "log_det segment.*not a square matrix"),
    ("seg_d0", 2, "log_det segment"),
])
def test_hand_edited_tapes_are_refused_at_load(field, value, message):
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = lq.matrices_tape([lr.matrix(3, 10.0, False)])
    OracleProblem(serialize(a))
    a = dict(a)
    a[field] = a[field].copy()
    a[field][0] = value
    with pytest.raises(Exception, match=message):
        OracleProblem(serialize(a))


def test_two_matrices_in_one_segment_are_refused_by_name():
    """M = 2 with counts that agree with it (two rows of 9 entries): the member takes one matrix per segment."""
    from oracle.oracle_capi import OracleProblem
    X = cp.Variable((2, 9))
    X.value = np.ones((2, 9))
    a = dict(lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.log_sum_exp(X, axis=1)))))["tape_arrays"])
    OracleProblem(serialize(a))
    for name, v in (("seg_op", 37), ("seg_d2", 3)):
        a[name] = a[name].copy()
        a[name][0] = v
    with pytest.raises(Exception, match="log_det segment with more than one matrix: M != 1"):
        OracleProblem(serialize(a))


# ---- 5. rule ------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_gives_the_written_constants():
    worst, consts = lr.measure_constants()
    print("numpy statement, worst ratios: value %.4f, d %.4f, h %.4f -> constants %r" % (worst["value"], worst["d1"], worst["d2"], consts))
    assert (consts["value"], consts["d1"], consts["d2"]) == (lr.C_V, lr.C_D, lr.C_H)


_tapes = {}
HOST_ORDERS = (1, 2, 3, 5, 8, 9, 16)


def order_tape(n):
    """The eight matrices of one order (four condition numbers, symmetric and not) as constraints and one more in the
    objective."""
    if n not in _tapes:
        mats = [A for _, _, _, A in lr.matrices((n,))]
        _tapes[n] = lq.matrices_tape(mats, [lr.matrix(n, 10.0, n > 1, seed=lr.SEED + 1)])
    return _tapes[n]


def check_callbacks(ev, tape, hsample=2000):
    a, x, lam, sigma = tape
    exp = lr.expected_oracles(a, x, lam, sigma, hsample)
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


@pytest.mark.parametrize("n", HOST_ORDERS)
def test_host_build_against_mpmath(n):
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(order_tape(n)[0])), order_tape(n))


def out_of_domain_matrices(n=3):
    """-> (the matrices, the positions of the clean ones).  Out of the domain: diag(-1, -1, 1) (its determinant is
    positive), a singular matrix, a NaN entry, and 1 x 1 matrices holding 0 and a negative number."""
    clean = lr.matrix(n, 10.0, True)
    neg = np.eye(n)
    neg[0, 0] = neg[1, 1] = -1.0
    sing = np.ones((n, n)) + np.diag(np.r_[np.zeros(2), np.arange(1.0, n - 1)])       # two equal rows
    nan = clean.copy()
    nan[n - 1, 1] = np.nan
    return [clean, neg, sing, nan, np.array([[0.0]]), np.array([[-2.5]]), np.array([[2.5]]), clean.T.copy()], (0, 6, 7)


def check_out_of_domain(ev, n=3):
    """Every output of an out-of-domain row is NaN and nothing else is touched: everything else has the bits it has when
    identity matrices stand where the out-of-domain ones stood."""
    import scipy.sparse as sp
    mats, keep = out_of_domain_matrices(n)
    a, x, lam, sigma = lq.matrices_tape(mats)
    _, xg, _, _ = lq.matrices_tape([A if s in keep else np.eye(A.shape[0]) for s, A in enumerate(mats)])
    h = ev(a)
    try:
        (g, J, H), (gg, Jg, Hg) = [(h.eval_g(v), h.eval_jac_g(v), h.eval_h(v, lam, sigma)) for v in (x, xg)]
    finally:
        if hasattr(h, "close"):
            h.close()
    N, m, Z = (int(v) for v in a["dims"][:3])
    G = sp.csr_matrix((a["G_val"], a["G_idx"], a["G_ptr"]), shape=(m, N + Z)).tocsc()
    jr, jc = np.asarray(a["jac_rows"]), np.asarray(a["jac_cols"])
    hr, hc = np.asarray(a["hess_rows"]), np.asarray(a["hess_cols"])
    bad_g, bad_j, bad_h = np.zeros(m, dtype=bool), np.zeros(J.size, dtype=bool), np.zeros(H.size, dtype=bool)
    for s, A in enumerate(mats):
        if s in keep:
            continue
        row = int(G.indices[G.indptr[N + s]])
        off, K = int(a["seg_a0_off"][s]), A.size
        idx = np.asarray(a["gidx"][off:off + K])
        mine_j, mine_h = (jr == row) & np.isin(jc, idx), np.isin(hr, idx) & np.isin(hc, idx)
        assert mine_j.sum() == K and mine_h.sum() == K * (K + 1) // 2
        bad_g[row] = True
        bad_j |= mine_j
        bad_h |= mine_h
    # (the affine rows T - (V + V^T) / 2 that read the replaced entries differ between the two points and are not compared)
    moved = np.asarray(abs(sp.csr_matrix(G[:, :N])) @ ((x != xg) | np.isnan(x)).astype(float)).reshape(-1) > 0
    for name, got, good, bad, skip in (("g", g, gg, bad_g, moved), ("jac", J, Jg, bad_j, False), ("hess", H, Hg, bad_h, False)):
        assert np.isnan(got[bad]).all(), name
        same = ~bad & ~skip
        assert np.isfinite(good).all() and got[same].tobytes() == good[same].tobytes(), name


def test_host_build_out_of_domain_table():
    from oracle.oracle_capi import OracleProblem
    check_out_of_domain(lambda a: OracleProblem(serialize(a)))


def test_with_h_off_writes_no_second_derivative():
    """eval_jac_g after eval_h at another point: the first derivatives are those of a fresh handle (the sweep without
    the Hessian does not depend on what the Hessian pass left)."""
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = order_tape(3)
    fresh, used = OracleProblem(serialize(a)), OracleProblem(serialize(a))
    used.eval_h(x * 1.01, lam, sigma)
    assert used.eval_jac_g(x).tobytes() == fresh.eval_jac_g(x).tobytes() and used.eval_g(x).tobytes() == fresh.eval_g(x).tobytes()


def mixed_problem(n_small=3, n_large=9):
    """log_det (both kernel forms), log_sum_exp and quad_over_lin_rows in one tape."""
    rng = np.random.default_rng(8)
    A, B = cp.Variable((n_small, n_small)), cp.Variable((n_large, n_large))
    A.value, B.value = lr.matrix(n_small, 10.0, False), lr.matrix(n_large, 100.0, False)
    L, Q = cp.Variable((3, 5)), cp.Variable((4, 3))
    L.value, Q.value = rng.standard_normal((3, 5)), rng.standard_normal((4, 3))
    cons = [cp.log_det(A) >= -1, cp.log_sum_exp(L, axis=1) <= 3, cp.norm(Q, 2, axis=1) <= 2, cp.log_det(B) >= -40]
    return cp.Problem(cp.Minimize(cp.sum_squares(L) + cp.sum(Q)), cons), (A, B, L, Q)


def check_mixed(ev):
    from scipy.special import logsumexp
    prob, (A, B, L, Q) = mixed_problem()
    data = lp.lower(prob)
    a = data["tape_arrays"]
    assert sorted(int(v) for v in a["seg_op"] if int(v) >= 34) == [34, 36, 37, 37]
    x = np.array(data["x0"], dtype=float)
    h = ev(a)
    g = h.eval_g(x)
    m = int(a["dims"][1])
    lam = lp.multipliers(m)
    assert np.isfinite(g).all() and np.isfinite(h.eval_jac_g(x)).all() and np.isfinite(h.eval_h(x, lam, 0.5)).all()
    # the rows that hold the atoms' values: among g there are -log det A + ..., the row values of log_sum_exp, ...
    vals = np.abs(g)
    for want in (abs(np.linalg.slogdet(A.value)[1] + 1), abs(np.linalg.slogdet(B.value)[1] + 40)):
        assert np.min(np.abs(vals - want)) <= 1e-12 * max(1.0, want), want
    for want in np.abs(logsumexp(L.value, axis=1) - 3):
        assert np.min(np.abs(vals - want)) <= 1e-12 * max(1.0, want), want
    if hasattr(h, "close"):
        h.close()
    return a


def test_tape_with_three_row_class_members_on_the_host():
    from oracle.oracle_capi import OracleProblem
    check_mixed(lambda a: OracleProblem(serialize(a)))


# ---- 6. host-build solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", list(lq.LIKELIHOOD_STARTS))
def test_host_build_gaussian_likelihood(start):
    prob, s = lq.likelihood_problem(start)
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    lq.assert_likelihood(lq.matrix_from_entries(lp.value_in(prob, s, xv), 4), obj)


def test_host_build_gaussian_likelihood_with_a_plain_matrix_variable():
    prob, X = lq.likelihood_plain_problem()
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    Xv = lp.value_in(prob, X, xv)
    lq.assert_likelihood((Xv + Xv.T) / 2, obj)


@pytest.mark.parametrize("kind", ["three", "twelve"])
def test_host_build_d_optimal_design(kind):
    V = lq.design_points(kind)
    prob, lam = lq.design_problem(V)
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    lq.assert_design(V, lp.value_in(prob, lam, xv), obj)


def test_host_build_largest_ellipsoid_in_a_box():
    prob, s, d = lq.ellipsoid_problem()
    a = lp.lower(cp.Problem(cp.Minimize(-prob.objective.expr), prob.constraints))["tape_arrays"]
    assert sorted(int(v) for v in a["seg_op"]) == [36, 37]                 # both ops in one sweep
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    lq.assert_ellipsoid(lp.value_in(prob, s, xv), lp.value_in(prob, d, xv), obj)
