"""prod on the device: the row-class kernels of OP_PROD (csrc/exec_hip_rows.h sweep_prod_kernel / sweep_prod_long_kernel /
sweep_prod_hess_kernel) entry by entry against mpmath within the derived bound of tests/prod_reference.py, on the tapes
of the CPU tests and on row shapes that reach every kernel form and its edges; zeros in every form; bit-for-bit repeats;
the solves of tests/prod_problems.py through the front-end on every solver path; the box volume as a batch template."""
import numpy as np
import pytest

import dnlp_amd as cp
import lse_problems as lp
import lse_reference as lr
import prod_problems as pp
import prod_reference as pr
from dnlp_amd.tape import serialize
from test_prod_cpu import check_callbacks, grid_tape, planted_tape

pytestmark = pytest.mark.gpu


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


_cache = {}


def _shape_tape(M, K, axis):
    key = (M, K, axis)
    if key not in _cache:
        _cache[key] = pp.rows_tape([pr.rows_of_length(K, M, seed=4000 + K)], axis=axis)
    return _cache[key]


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------
def test_device_build_against_mpmath_on_the_grid(gpu_required):
    dev = _device(grid_tape()[0])
    try:
        check_callbacks(dev, grid_tape())
    finally:
        dev.close()


def test_device_build_against_mpmath_on_the_planted_rows(gpu_required):
    a, x, lam, sigma = planted_tape()
    dev = _device(a)
    try:
        check_callbacks(dev, planted_tape())
        exp = pr.expected_oracles(a, x, lam, sigma)
        for name, got in (("g", dev.eval_g(x)), ("jac", dev.eval_jac_g(x)), ("hess", dev.eval_h(x, lam, sigma))):
            zero = exp[name].hi == 0
            assert zero.any() and not np.asarray(got)[zero].any(), name
    finally:
        dev.close()


@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 33, 64, 65, 257, 4097, 8193])
def test_single_row_of_every_form(K, gpu_required):
    """M = 1: the short form with every group width, its edge 64 / 65, the wavefront form, and the workgroup form (8193:
    3.4e7 Hessian entries through the spread launch; mpmath for the value, all of g and 2000 sampled Hessian entries)."""
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
    ii, jj = np.tril_indices(K, -1 if int(a["seg_op"][s]) == 35 else 0)
    want_h = np.maximum(idx[:, ii], idx[:, jj]) * N + np.minimum(idx[:, ii], idx[:, jj])
    jpos, hpos = np.searchsorted(jkeys, want_j), np.searchsorted(hkeys, want_h)
    assert np.array_equal(jkeys[jpos], want_j) and np.array_equal(hkeys[hpos], want_h)
    return crow, sign, idx, jpos, hpos


def _check_rows_mpmath(a, x, lam, g, J, H, s, pick, hsel_of=None):
    """Rows `pick` of segment s against pr.row_reference: value, every g, every Hessian entry (or the packed positions
    hsel_of(r)); -> the worst error as a share of its bound."""
    crow, sign, idx, jpos, hpos = _segment_entries(a, s)
    worst = 0.0
    for r in pick:
        hsel = None if hsel_of is None else hsel_of(int(r))
        V, D, Hs = pr.row_reference(x[idx[r]], sign[r] * lam[crow[r]], hsel)
        hgot = H[hpos[r]] if hsel is None else H[hpos[r]][hsel]
        for kind, got, U in (("value", [sign[r] * g[crow[r]]], V), ("d1", sign[r] * J[jpos[r]], D), ("d2", hgot, Hs)):
            worst = max(worst, pr.check_units("segment %d row %d %s" % (s, r, kind), U, got))
            zero = (U.hi == 0) & (U.st == 0)
            assert not np.asarray(got, dtype=float)[zero].any()
    return worst


def _numpy_rows(u, w):
    """The rule in numpy over ALL rows of an (M, K) array at once (the text of pr.numpy_rule, vectorised)."""
    M, K = u.shape
    zero = u == 0
    nz = zero.sum(axis=1, keepdims=True)
    safe = np.where(zero, 1.0, u)
    P0 = np.prod(safe, axis=1, keepdims=True)
    Z0 = np.where(P0 != P0, P0, 0.0)
    z = np.where(nz == 0, P0, Z0)[:, 0]
    g = np.where(nz == 0, P0 / safe, np.where(zero & (nz == 1), P0, Z0))
    ii, jj = np.tril_indices(K, -1)
    h = np.where(~zero[:, jj], g[:, ii] / safe[:, jj], np.where(~zero[:, ii], g[:, jj] / safe[:, ii], np.where(nz == 2, P0, Z0)))
    return z, g, w[:, None] * h


def _check_rows_numpy(a, x, lam, g, J, H, s):
    """EVERY row of segment s against the numpy statement.  Both stand within gamma(K + 1) |ref| of the mpmath value, so
    they differ by at most 2 gamma |ref| <= 2 gamma / (1 - gamma) |numpy value|; a 0 there is a 0 here."""
    crow, sign, idx, jpos, hpos = _segment_entries(a, s)
    K = idx.shape[1]
    gm = pr.gamma(K + 1)
    rel = 2 * gm / (1 - gm)
    with np.errstate(all="ignore"):
        z, d, h = _numpy_rows(x[idx], sign * lam[crow])
    for name, got, ref in (("value", sign * g[crow], z), ("d1", sign[:, None] * J[jpos], d), ("d2", H[hpos], h)):
        assert not np.isnan(got).any(), name
        cmp = (np.abs(ref) > 1e-290) & (np.abs(ref) < 1e290) | (ref == 0)
        bad = cmp & ~(np.abs(got - ref) <= rel * np.abs(ref))
        assert not bad.any(), (s, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("M,K,axis", [(20000, 10, 1), (20000, 10, 0), (1000, 64, 1), (1000, 65, 1), (37, 129, 1)])
def test_many_rows(M, K, axis, gpu_required):
    """Many rows per launch: partly filled wavefronts (20000 rows, 4 per wavefront; 37 rows, 4 per workgroup), both axes.
    Every row against the numpy statement; a seeded sample of 100 rows, the first and the last among them, against mpmath
    with all of their entries."""
    a, x, lam, sigma = _shape_tape(M, K, axis)
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    _check_rows_numpy(a, x, lam, g, J, H, 0)
    pick = np.sort(np.random.default_rng(K).choice(M, min(M, 100), replace=False))
    pick[0], pick[-1] = 0, M - 1
    worst = _check_rows_mpmath(a, x, lam, g, J, H, 0, np.unique(pick))
    print("%d x %d axis %d: worst error %.3f of its bound over the mpmath sample" % (M, K, axis, worst))


def test_mixed_tape(gpu_required):
    """Elementwise, reduction, log_sum_exp and prod segments in one tape (a short prod block between flat segments, a
    log_sum_exp block, a wavefront-form prod row last), non-zero multipliers on every row: the prod rows against mpmath
    through the pattern arrays, the log_sum_exp rows by that atom's own check, and the rows of g that the other classes
    feed are the bits of the same problem without the row-class atoms."""
    from test_log_sum_exp_gpu import _check_segment_mpmath as check_lse
    P = np.diag(np.arange(1.0, 8.0)) + 0.25
    rowsA, rowsB, rowsC = pr.rows_of_length(5, 6, seed=31), pr.rows_of_length(70, 1, seed=32), lr.rows_of_length(5, 3, seed=33)

    def problem(with_rows):
        rng = np.random.default_rng(9)
        u, v, q = cp.Variable(50), cp.Variable(9), cp.Variable(7)
        u.value, v.value, q.value = rng.standard_normal(50), rng.uniform(0.5, 2, 9), rng.standard_normal(7)
        cons = [cp.exp(u) <= 3, cp.quad_form(q, P) <= 4, cp.sin(v) >= -1]
        if with_rows:
            A, B, C = cp.Variable((6, 5)), cp.Variable(70), cp.Variable((3, 5))
            A.value, B.value, C.value = rowsA, rowsB[0], rowsC
            cons = cons[:1] + [cp.prod(A, axis=1) <= 0] + cons[1:2] + [cp.log_sum_exp(C, axis=1) <= 0] + cons[2:] + [cp.prod(B) <= 0]
        return cp.Problem(cp.Minimize(cp.sum(cp.exp(u))), cons)

    full, bare = lp.lower(problem(True)), lp.lower(problem(False))
    a, b = full["tape_arrays"], bare["tape_arrays"]
    assert list(a["seg_op"]) == [1, 1, 35, 31, 34, 6, 35] and list(b["seg_op"]) == [1, 1, 31, 6]
    xa, xb = np.array(full["x0"], dtype=float), np.array(bare["x0"], dtype=float)
    rows_a = np.r_[0:50, 56, 60:69]                         # exp block, (6 prod rows), quad_form, (3 lse rows), sin block, (1 row)
    lam_a = lp.multipliers(70)
    lam_b = lam_a[rows_a]
    da, db = _device(a), _device(b)
    try:
        ga, Ja, Ha = da.eval_g(xa), da.eval_jac_g(xa), da.eval_h(xa, lam_a, 0.5)
        gb = db.eval_g(xb)
    finally:
        da.close()
        db.close()
    assert ga.size == gb.size + 10 == 70
    for s, M in ((2, 6), (6, 1)):
        print("mixed tape, prod segment %d: worst error %.3f of its bound" % (s, _check_rows_mpmath(a, xa, lam_a, ga, Ja, Ha, s, np.arange(M))))
    print("mixed tape, log_sum_exp segment: worst error %.3f of its bound" % check_lse(a, xa, lam_a, ga, Ja, Ha, 4, np.arange(3)))
    assert ga[rows_a].tobytes() == gb.tobytes()


def _zero_rows(K):
    """Rows with 1, 2 and 3 zeros in first, middle and last position, and one without."""
    rows = pr.rows_of_length(K, 7, seed=51)
    for r, zeros in enumerate(([0], [K // 2], [K - 1], [0, K - 1], [K // 2, K - 1], [0, K // 2, K - 1])):
        rows[r, zeros] = 0.0
    return rows


@pytest.mark.parametrize("K", [3, 129, 2049])
def test_rows_with_zeros_in_every_form(K, gpu_required):
    """The group form, the wavefront form and the workgroup form: every first derivative, and every Hessian entry (K <= 129)
    or the entries of all pairs of the zero positions with each other and with their neighbours plus 2000 sampled ones
    (K = 2049), against mpmath; what is 0 there is 0 here."""
    rows = _zero_rows(K)
    a, x, lam, sigma = pp.rows_tape([rows])
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    hsel_of = None
    if K > 257:
        T = K * (K - 1) // 2
        special = sorted({0, 1, K // 2 - 1, K // 2, K // 2 + 1, K - 2, K - 1})
        pairs = [i * (i - 1) // 2 + j for i in special for j in special if i > j]

        def hsel_of(r):
            return np.unique(np.r_[pairs, 0, T - 1, np.random.default_rng(r).integers(0, T, 2000)])
    worst = _check_rows_mpmath(a, x, lam, g, J, H, 0, np.arange(rows.shape[0]), hsel_of)
    print("zeros at K = %d: worst error %.3f of its bound" % (K, worst))
    if K <= 257:
        _check_rows_numpy(a, x, lam, g, J, H, 0)


@pytest.mark.parametrize("K", [3, 129, 2049])
def test_nan_and_inf_entries_in_every_form(K, gpu_required):
    """DESIGN.md section 2, the same in every form: a NaN entry gives a NaN value with or without a zero beside it; +-inf
    is a nonzero entry (beside a zero the value is 0); the clean row beside them is untouched."""
    rows = pr.rows_of_length(K, 5, seed=52)
    rows[0, K // 2] = np.nan
    rows[1, 0], rows[1, K - 1] = 0.0, np.nan
    rows[2, K - 1] = np.inf
    rows[3, 0], rows[3, K // 2] = -np.inf, 0.0
    a, x, lam, sigma = pp.rows_tape([rows])
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    crow, sign, idx, jpos, hpos = _segment_entries(a, 0)
    v = sign * g[crow]
    assert np.isnan(v[0]) and np.isnan(v[1]) and np.isinf(v[2]) and v[3] == 0.0 and np.isfinite(v[4])
    assert np.isnan(J[jpos[:2]]).all() and np.isnan(H[hpos[:2]]).all()
    _check_rows_mpmath(a, x, lam, g, np.nan_to_num(J), np.nan_to_num(H), 0, [4],
                       None if K <= 257 else (lambda r: np.random.default_rng(r).integers(0, K * (K - 1) // 2, 2000)))


def test_first_derivatives_do_not_depend_on_the_hessian_pass(gpu_required):
    for tape in (grid_tape(), _shape_tape(1, 4097, None)):
        a, x, lam, sigma = tape
        fresh = _device(a)
        try:
            j0, g0, v0 = fresh.eval_jac_g(x).tobytes(), fresh.eval_grad_f(x).tobytes(), fresh.eval_g(x).tobytes()
            fresh.eval_h(x, lam, sigma)
            assert fresh.eval_jac_g(x).tobytes() == j0 and fresh.eval_grad_f(x).tobytes() == g0 and fresh.eval_g(x).tobytes() == v0
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


# ---- 3. the solves on every path --------------------------------------------------------------------------------------------------
# ("in-kernel" is asked for by name: device_loop="yes" raises where the in-kernel loop cannot take the problem)
PATHS = {"in-kernel": {"device_loop": "yes"}, "host-driven": {"device_loop": "no"}, "limited-memory": {"hessian_approximation": "limited-memory"}}


def _agree(values):
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * abs(values["host-driven"]), values


def test_box_volume_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, x = pp.box_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        pp.assert_box(x.value, prob.value)
        values[name] = prob.value
    _agree(values)


def test_amgm_with_an_axis_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, X = pp.amgm_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        pp.assert_amgm(X.value, prob.value, np.asarray(prob._nlp_last["mult_g"])[:pp.AMGM_B.size])
        values[name] = prob.value
    _agree(values)


def test_nonconvex_sphere_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, x = pp.sphere_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        pp.assert_sphere_kkt(x.value, prob._nlp_last["mult_g"][-1])
        values[name] = prob.value
    _agree(values)


# ---- 4. batch ---------------------------------------------------------------------------------------------------------------------
def _box_thetas(count):
    rng = np.random.default_rng(21)
    return np.concatenate([rng.uniform(0.5, 4.0, (count, pp.BOX_A.size)), rng.uniform(6.0, 20.0, (count, 1))], axis=1)


@pytest.mark.parametrize("count", [256, 1024])
def test_box_batch_takes_the_generic_kernel(count, gpu_required):
    from dnlp_amd.batch import ParametricBatch
    thetas = _box_thetas(count)
    runs = []
    for _ in range(2):
        tprob, x, params = pp.box_problem(parameters=True)
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
        xs, vs = pp.box_optimum(thetas[i, :-1], thetas[i, -1])
        assert np.all(xs > pp.BOX_LO)
        assert abs(abs(objs[i]) - vs) <= pp.VALUE_TOL * vs, (i, objs[i], vs)


# ---- 5. best_of -------------------------------------------------------------------------------------------------------------------
def test_best_of_on_the_sphere_returns_the_global_value(gpu_required):
    prob, x = pp.sphere_problem(start=False)
    x.sample_bounds = [-2, 2]
    prob.solve(nlp=True, best_of=8)
    assert prob.status == cp.OPTIMAL
    objs = np.asarray(prob.solver_stats.extra_stats["all_objs_from_best_of"])
    assert objs.size == 8 and abs(prob.value - np.min(objs)) <= 1e-9 * abs(prob.value)
    assert abs(prob.value - pp.SPHERE_GLOBAL) <= pp.VALUE_TOL, prob.value
