"""log_sum_exp on the device: the row-class kernels (csrc/exec_hip_rows.h sweep_rows_kernel / sweep_rows_long_kernel /
sweep_rows_hess_kernel) entry by entry against mpmath with the bounds of tests/lse_reference.py, on the tapes of the CPU
tests and on row shapes that reach every kernel form and its edges; bit-for-bit repeats; the three solves of
tests/lse_problems.py through the front-end on every solver path; softmax regression at a user's size; the geometric program
as a batch template."""
import numpy as np
import pytest

import dnlp_amd as cp
import lse_problems as lp
import lse_reference as lr
from batch_problems import oracle_solver
from dnlp_amd.tape import serialize
from test_log_sum_exp_cpu import check_callbacks, grid_tape, minus_inf_tape

pytestmark = pytest.mark.gpu


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


def _rows(M, K, seed):
    """M seeded rows of length K in the grid's distribution."""
    return lr.rows_of_length(K, M, seed=seed)


_cache = {}


def _shape_tape(M, K, axis):
    key = (M, K, axis)
    if key not in _cache:
        _cache[key] = lp.rows_tape([_rows(M, K, 4000 + K)], axis=axis)
    return _cache[key]


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------
def test_device_build_against_mpmath_on_the_grid(gpu_required):
    dev = _device(grid_tape()[0])
    try:
        check_callbacks(dev, grid_tape())
    finally:
        dev.close()


def test_device_build_against_mpmath_on_a_row_containing_minus_inf(gpu_required):
    dev = _device(minus_inf_tape()[0])
    try:
        check_callbacks(dev, minus_inf_tape(), with_f=False)
    finally:
        dev.close()


@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 33, 64, 65, 257, 4097, 8193])
def test_single_row_of_every_form(K, gpu_required):
    """M = 1: the short form with every group width, its edge 64 / 65, the wavefront form, and the workgroup form (8193:
    3.4e7 Hessian entries through the spread launch; mpmath for the value, all of p and 2000 sampled Hessian entries)."""
    tape = _shape_tape(1, K, None)
    dev = _device(tape[0])
    try:
        check_callbacks(dev, tape, hsample=2000)
    finally:
        dev.close()


def _segment_entries(a, s):
    """Where segment s of a tape shows in g, J and H: (constraint row of every atom row, its sign in G, x indices (M, K),
    positions of d entries in J (M, K), positions of the packed triangle in H (M, T)).  Every atom row feeds one constraint."""
    import scipy.sparse as sp
    N, m, Z = (int(v) for v in a["dims"][:3])
    M, K = int(a["seg_d0"][s]), int(a["seg_d1"][s])
    off, zo = int(a["seg_a0_off"][s]), int(a["seg_zoff"][s])
    idx = np.asarray(a["gidx"][off:off + M * K], dtype=np.int64).reshape(M, K)
    G = sp.csr_matrix((a["G_val"], a["G_idx"], a["G_ptr"]), shape=(m, N + Z)).tocsc()
    cols = N + zo + np.arange(M)
    assert np.all(np.diff(G.indptr)[cols] == 1)
    crow = G.indices[G.indptr[cols]].astype(np.int64)
    sign = G.data[G.indptr[cols]]
    assert np.all(np.abs(sign) == 1.0)
    jkeys = np.asarray(a["jac_rows"], dtype=np.int64) * N + np.asarray(a["jac_cols"], dtype=np.int64)
    hkeys = np.asarray(a["hess_rows"], dtype=np.int64) * N + np.asarray(a["hess_cols"], dtype=np.int64)
    want_j = crow[:, None] * N + idx
    ii, jj = np.tril_indices(K)
    want_h = np.maximum(idx[:, ii], idx[:, jj]) * N + np.minimum(idx[:, ii], idx[:, jj])
    jpos, hpos = np.searchsorted(jkeys, want_j), np.searchsorted(hkeys, want_h)
    assert np.array_equal(jkeys[jpos], want_j) and np.array_equal(hkeys[hpos], want_h)
    return crow, sign, idx, jpos, hpos


def _check_segment_mpmath(a, x, lam, g, J, H, s, pick):
    """Rows `pick` of segment s against lr.row_reference with the measured K: value, every p, every Hessian entry."""
    crow, sign, idx, jpos, hpos = _segment_entries(a, s)
    KK = lr.measured_K()
    worst = 0.0
    for r in pick:
        V, D, Hs = lr.row_reference(x[idx[r]], sign[r] * lam[crow[r]])
        kh = np.where(Hs.diag, KK["d2 diagonal"], KK["d2 off-diag"])
        for got, U, kk in ((np.array([sign[r] * g[crow[r]]]), V, KK["value"]), (sign[r] * J[jpos[r]], D, KK["d1"]), (H[hpos[r]], Hs, kh)):
            bound = kk * lr.EPS * U.bracket + U.sterm + lr.EPS * np.abs(U.hi)
            cmp = U.st == 0
            err = np.abs(got - U.hi)
            assert not np.isnan(got).any()
            assert np.all(err[cmp] <= bound[cmp]), (s, int(r), float(np.max(err[cmp] / np.maximum(bound[cmp], 1e-320))))
            if np.any(cmp & (bound > 0)):
                worst = max(worst, float(np.max(err[cmp & (bound > 0)] / bound[cmp & (bound > 0)])))
    return worst


def _check_segment_numpy(a, x, lam, g, J, H, s):
    """EVERY row of segment s against the numpy statement of the rule (lr.numpy_rule's text, vectorised over rows).  That
    statement is itself within 1 unit of eps * bracket plus the summation term of mpmath (measured: 0.91 at worst), the
    device within K units plus the summation term: the difference of the two is held to the sum, with the brackets
    computed from the numpy values.  Entries below 1e-290 in magnitude are not compared (the brackets lose their meaning
    near the subnormal range; the sampled mpmath check decides there)."""
    crow, sign, idx, jpos, hpos = _segment_entries(a, s)
    KK = lr.measured_K()
    u = x[idx]
    M, K = u.shape
    sm = (K + 2) * lr.EPS
    mx = u.max(axis=1, keepdims=True)
    e = np.exp(u - mx)
    S = e.sum(axis=1, keepdims=True)
    r = (mx + np.log(S))[:, 0]
    p = e / S
    w = sign * lam[crow]
    ii, jj = np.tril_indices(K)
    diag = ii == jj
    h = w[:, None] * np.where(diag, p[:, ii] - p[:, ii] * p[:, jj], -(p[:, ii] * p[:, jj]))
    dist = np.abs(u - r[:, None])
    aw = np.abs(w)[:, None]
    br_v = np.abs(r) + np.sum(p * np.abs(u), axis=1)
    br_d = p * (1 + dist)
    br_h = aw * np.where(diag, p[:, ii] * (1 + dist[:, ii]), p[:, ii] * p[:, jj] * (2 + dist[:, ii] + dist[:, jj]))
    st_h = aw * np.where(diag, sm * p[:, ii], 2 * sm * p[:, ii] * p[:, jj])
    kh = np.where(diag, KK["d2 diagonal"], KK["d2 off-diag"])[None, :]
    for name, got, ref, bound in (("value", sign * g[crow], r, (KK["value"] + 1) * lr.EPS * br_v + 2 * sm),
                                  ("d1", sign[:, None] * J[jpos], p, (KK["d1"] + 1) * lr.EPS * br_d + 2 * sm * p),
                                  ("d2", H[hpos], h, (kh + 1) * lr.EPS * br_h + 2 * st_h)):
        assert not np.isnan(got).any(), name
        cmp = np.abs(ref) > 1e-290
        bad = cmp & ~(np.abs(got - ref) <= bound)
        assert not bad.any(), (s, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("M,K,axis", [(20000, 10, 1), (20000, 10, 0), (1000, 64, 1), (1000, 65, 1), (37, 129, 1)])
def test_many_rows(M, K, axis, gpu_required):
    """Many rows per launch: partly filled wavefronts (20000 rows, 4 per wavefront; 37 rows, 4 per workgroup), both axes.
    Every row is held to the numpy statement of the rule at the summed bound; a seeded sample of 100 rows, the first and
    the last among them, to mpmath with all of their entries (80-digit arithmetic on every entry of 20000 rows would take
    minutes of the run)."""
    a, x, lam, sigma = _shape_tape(M, K, axis)
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    _check_segment_numpy(a, x, lam, g, J, H, 0)
    pick = np.sort(np.random.default_rng(K).choice(M, min(M, 100), replace=False))
    pick[0], pick[-1] = 0, M - 1
    worst = _check_segment_mpmath(a, x, lam, g, J, H, 0, np.unique(pick))
    print("%d x %d axis %d: worst error %.3f of its bound over the mpmath sample" % (M, K, axis, worst))


def test_mixed_tape(gpu_required):
    """Flat, reduction and two row-class segments (a short-row one between flat segments, a wavefront-form one last) in one
    tape, seeded arguments, non-zero multipliers on every row: g, J and H of the row-class rows against mpmath with the
    measured bounds, through the pattern arrays; the rows of g, J and the entries of H and grad f that the other classes
    feed are the bits of the same problem without the row-class atoms."""
    P = np.diag(np.arange(1.0, 8.0)) + 0.25
    rowsA, rowsB = lr.rows_of_length(5, 6, seed=31), lr.rows_of_length(70, 1, seed=32)

    def problem(with_rows):
        rng = np.random.default_rng(9)
        u, v, q = cp.Variable(50), cp.Variable(9), cp.Variable(7)
        u.value, v.value, q.value = rng.standard_normal(50), rng.uniform(0.5, 2, 9), rng.standard_normal(7)
        cons = [cp.exp(u) <= 3, cp.quad_form(q, P) <= 4, cp.sin(v) >= -1]
        if with_rows:
            A, B = cp.Variable((6, 5)), cp.Variable(70)
            A.value, B.value = rowsA, rowsB[0]
            cons = cons[:1] + [cp.log_sum_exp(A, axis=1) <= 0] + cons[1:] + [cp.log_sum_exp(B) <= 0]
        return cp.Problem(cp.Minimize(cp.sum(cp.exp(u))), cons)

    full, bare = lp.lower(problem(True)), lp.lower(problem(False))
    a, b = full["tape_arrays"], bare["tape_arrays"]
    assert list(a["seg_op"]) == [1, 1, 34, 31, 6, 34] and list(b["seg_op"]) == [1, 1, 31, 6]
    xa, xb = np.array(full["x0"], dtype=float), np.array(bare["x0"], dtype=float)
    rows_a = np.r_[0:50, 56:66]                             # exp block, (6 log_sum_exp rows), quad_form, sin block, (1 row)
    lam_a = lp.multipliers(67)
    lam_b = lam_a[rows_a]
    da, db = _device(a), _device(b)
    try:
        ga, Ja, Ha, fa = da.eval_g(xa), da.eval_jac_g(xa), da.eval_h(xa, lam_a, 0.5), da.eval_grad_f(xa)
        gb, Jb, Hb, fb = db.eval_g(xb), db.eval_jac_g(xb), db.eval_h(xb, lam_b, 0.5), db.eval_grad_f(xb)
    finally:
        da.close()
        db.close()
    assert ga.size == gb.size + 7 == 67
    for s, M in ((2, 6), (5, 1)):
        worst = _check_segment_mpmath(a, xa, lam_a, ga, Ja, Ha, s, np.arange(M))
        print("mixed tape, segment %d: worst error %.3f of its bound" % (s, worst))
    # the other classes: the variables u, v, q keep their order, the atoms' variables come between and after them
    assert ga[rows_a].tobytes() == gb.tobytes()
    other_j = np.isin(np.asarray(a["jac_rows"]), rows_a)
    assert int(other_j.sum()) == Jb.size and Ja[other_j].tobytes() == Jb.tobytes()
    _, _, _, _, hposA = _segment_entries(a, 2)
    _, _, _, _, hposB = _segment_entries(a, 5)
    other_h = np.ones(Ha.size, dtype=bool)
    other_h[hposA.reshape(-1)] = False
    other_h[hposB.reshape(-1)] = False
    assert int(other_h.sum()) == Hb.size and Ha[other_h].tobytes() == Hb.tobytes()
    assert fa[:50].tobytes() == fb[:50].tobytes() and not fa[50:].any() and not fb[50:].any()


@pytest.mark.parametrize("K", [1, 3, 129, 2049])
def test_rows_with_inf_or_nan_give_nan(K, gpu_required):
    """+inf or NaN anywhere in a row: NaN for that row's value in every kernel form (groups of one and of four lanes, the
    wavefront form, the workgroup form), and the clean row beside them is untouched."""
    rows = lr.rows_of_length(K, 4, seed=41)
    rows[0, K // 2], rows[1, K - 1], rows[2, 0] = np.inf, np.nan, np.nan
    a, x, lam, sigma = lp.rows_tape([rows])
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    assert np.isnan(g[:3]).all() and np.isfinite(g[3])
    _check_segment_mpmath(a, x, lam, g, np.nan_to_num(J), np.nan_to_num(H), 0, [3])
    assert np.isfinite(J[-K:]).all()


@pytest.mark.parametrize("K", [129, 2049])
def test_extreme_rows_in_the_long_forms(K, gpu_required):
    """The planted rows of the grid at the long forms' lengths: all entries equal, one entry 745 above the rest, entries
    near +-700, a row containing -inf; every entry against mpmath."""
    rng = np.random.default_rng(K)
    rows = np.stack([np.full(K, 3.25), np.r_[746.5, rng.uniform(0, 2, K - 1)], 700.0 - rng.uniform(0, 3, K),
                     -700.0 + rng.uniform(0, 3, K), np.r_[rng.uniform(-1, 2, K - 1), -np.inf][rng.permutation(K)]])
    a, x, lam, sigma = lp.rows_tape([rows])
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    crow, sign, idx, jpos, hpos = _segment_entries(a, 0)
    KK = lr.measured_K()
    for r in range(5):
        hsel = None if K <= 257 else np.unique(np.r_[0, K * (K + 1) // 2 - 1, np.random.default_rng(r).integers(0, K * (K + 1) // 2, 2000)])
        V, D, Hs = lr.row_reference(x[idx[r]], sign[r] * lam[crow[r]], hsel)
        hgot = H[hpos[r]] if hsel is None else H[hpos[r]][hsel]
        kh = np.where(Hs.diag, KK["d2 diagonal"], KK["d2 off-diag"])
        for got, U, kk in ((np.array([sign[r] * g[crow[r]]]), V, KK["value"]), (sign[r] * J[jpos[r]], D, KK["d1"]), (hgot, Hs, kh)):
            bound = kk * lr.EPS * U.bracket + U.sterm + lr.EPS * np.abs(U.hi)
            cmp = U.st == 0
            assert not np.isnan(got).any(), r
            assert np.all(np.abs(got - U.hi)[cmp] <= bound[cmp]), (r, float(np.max((np.abs(got - U.hi) / np.maximum(bound, 1e-320))[cmp])))


def test_first_derivatives_do_not_depend_on_the_hessian_pass(gpu_required):
    for tape in (grid_tape(), _shape_tape(1, 4097, None)):
        a, x, lam, sigma = tape
        fresh = _device(a)
        try:
            j0, g0 = fresh.eval_jac_g(x).tobytes(), fresh.eval_grad_f(x).tobytes()
            fresh.eval_h(x, lam, sigma)
            assert fresh.eval_jac_g(x).tobytes() == j0 and fresh.eval_grad_f(x).tobytes() == g0
        finally:
            fresh.close()


# ---- 2. bit-for-bit repeat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,axis", [(20000, 10, 1), (1, 8193, None)])
def test_sweep_repeats_bit_for_bit(M, K, axis, gpu_required):
    a, x, lam, sigma = _shape_tape(M, K, axis)
    seen = set()
    for _ in range(2):
        dev = _device(a)
        try:
            for _ in range(2):
                seen.add((dev.eval_g(x).tobytes(), dev.eval_jac_g(x).tobytes(), dev.eval_h(x, lam, sigma).tobytes()))
        finally:
            dev.close()
    assert len(seen) == 1


# ---- 3. the three solves on every path --------------------------------------------------------------------------------------------
# ("in-kernel" is asked for by name: device_loop="yes" raises where the in-kernel loop cannot take the problem)
PATHS = {"in-kernel": {"device_loop": "yes"}, "host-driven": {"device_loop": "no"}, "limited-memory": {"hessian_approximation": "limited-memory"}}


def test_softmax_regression_on_every_path(gpu_required):
    X, Y = lp.softmax_data()
    values = {}
    for name, opts in dict(PATHS, lbfgs={"algorithm": "lbfgs"}).items():
        prob, W = lp.softmax_problem(X, Y)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        values[name] = lp.assert_softmax(X, Y, W.value, prob.value)
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * abs(values["host-driven"])


def test_box_design_gp_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, y = lp.gp_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lp.assert_gp(y.value, prob.value)
        values[name] = prob.value
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * abs(values["host-driven"])


def test_nonconvex_sphere_on_every_path(gpu_required):
    A = lp.sphere_data()
    for name, opts in PATHS.items():
        prob, x = lp.sphere_problem(A)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lp.assert_sphere_kkt(A, x.value, prob._nlp_last["mult_g"][-1])


# ---- 4. softmax regression at a user's size -----------------------------------------------------------------------------------------
def test_softmax_regression_20000_samples_lbfgs(gpu_required):
    X, Y = lp.softmax_data(20000, 20, 10, seed=12)
    prob, W = lp.softmax_problem(X, Y)
    prob.solve(nlp=True, algorithm="lbfgs")
    assert prob.status == cp.OPTIMAL, prob.status
    lp.assert_softmax(X, Y, W.value, prob.value)


# ---- 5. batch ---------------------------------------------------------------------------------------------------------------------
def _gp_thetas(count):
    rng = np.random.default_rng(21)
    return np.log(np.stack([rng.uniform(50, 200, count), rng.uniform(5, 20, count)], axis=1))


@pytest.mark.parametrize("count", [256, 1024])
def test_gp_batch_takes_the_generic_kernel(count, gpu_required):
    from dnlp_amd.batch import ParametricBatch
    thetas = _gp_thetas(count)
    runs = []
    for _ in range(2 if count == 256 else 1):
        tprob, y, params = lp.gp_problem(parameters=True)
        pb = ParametricBatch(tprob, params)
        try:
            res = pb.solve(thetas)
            launch = res.raw["launch"]
            assert launch["wave_form"] == 0 and not launch["wave_spec"] and not launch["wave_wg"], launch
            assert np.all(np.asarray(res.status) == 0)
            runs.append((np.array(res.x).tobytes(), np.array(res.raw["obj_val"]).tobytes(), np.array(res.status).tobytes(),
                         np.array(res.iterations).tobytes()))
            objs = np.array(res.raw["obj_val"])
        finally:
            pb.close()
    assert len(set(runs)) == 1                  # a fresh handle repeats the launch bit for bit
    for i in np.random.default_rng(3).choice(count, 32, replace=False):
        prob, _ = lp.gp_problem(float(np.exp(thetas[i, 0])), float(np.exp(thetas[i, 1])))
        ref, status, _, _ = oracle_solver(prob)
        assert status == 0 and abs(objs[i] - ref) <= 1e-8 * max(1.0, abs(ref)), (i, objs[i], ref)


# ---- 6. best_of -------------------------------------------------------------------------------------------------------------------
def test_best_of_on_the_sphere(gpu_required):
    A = lp.sphere_data()
    prob, x = lp.sphere_problem(A, start=False)
    x.sample_bounds = [-1, 1]
    prob.solve(nlp=True, best_of=8)
    assert prob.status == cp.OPTIMAL
    objs = np.asarray(prob.solver_stats.extra_stats["all_objs_from_best_of"])
    assert objs.size == 8 and abs(prob.value - np.max(objs)) <= 1e-9 * abs(prob.value)
