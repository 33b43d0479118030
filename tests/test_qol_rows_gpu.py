"""Row-wise 2-norms on the device: the row-class kernels of OP_QUAD_OVER_LIN_ROWS (csrc/exec_hip_rows.h sweep_qol_kernel /
sweep_qol_long_kernel) entry by entry against mpmath within the derived bound of tests/qol_rows_reference.py, on the
tapes of the CPU tests and on row shapes that reach every kernel form and both sides of each switch; bit-for-bit repeats;
the solves of tests/qol_rows_problems.py through the front-end on every solver path; Fermat-Weber as a batch template."""
import numpy as np
import pytest

import dnlp_amd as cp
import lse_problems as lp
import lse_reference as lr
import prod_reference as pr
import qol_rows_problems as qp
import qol_rows_reference as qr
from dnlp_amd.tape import serialize
from test_qol_rows_cpu import check_grid, check_planted

pytestmark = pytest.mark.gpu


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


_cache = {}


def _shape_tape(M, K, axis):
    key = (M, K, axis)
    if key not in _cache:
        _cache[key] = qp.rows_tape([qr.rows_of_shape(M, K, seed=4100 + K)], axis=axis)
    return _cache[key]


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------
def test_device_build_against_mpmath_on_the_grid(gpu_required):
    check_grid("device build", _device).close()


def test_device_build_planted_rows(gpu_required):
    check_planted("device build", _device).close()


@pytest.mark.parametrize("K", [1, 2, 3, 7, 16, 33, 64, 65, 257, 2049, 4097])
def test_single_row_of_every_form(K, gpu_required):
    """M = 1: the group form with every group width, its edge 64 / 65, the wavefront form, its edge 2048 / 2049 and the
    workgroup form; every output of the row against mpmath."""
    tape = _shape_tape(1, K, None)
    dev = _device(tape[0])
    try:
        print("K = %d: worst error %.3f of its bound" % (K, qr.check_segment("single row", dev, tape)))
    finally:
        dev.close()


@pytest.mark.parametrize("M,K,axis", [(20000, 3, 1), (20000, 3, 0), (20000, 10, 1), (1000, 64, 1), (1000, 65, 1), (37, 129, 1)])
def test_many_rows(M, K, axis, gpu_required):
    """Many rows per launch, partly filled wavefronts and workgroups, both axes.  Every row against the numpy statement; a
    seeded sample of 100 rows, the first and the last among them, against mpmath with all of their entries."""
    tape = _shape_tape(M, K, axis)
    a, x, lam, sigma = tape
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, sigma)
    finally:
        dev.close()
    U, y, w, got = qr.rows_got(a, 0, x, lam, g, J, H)
    qr.check_all_rows_numpy(got, U, y, w)
    pick = np.sort(np.random.default_rng(K).choice(M, min(M, 100), replace=False))
    pick[0], pick[-1] = 0, M - 1
    worst = max(qr.check_row("row %d" % r, {k: v[r] for k, v in got.items()}, U[r], y[r], w[r]) for r in np.unique(pick))
    print("%d x %d axis %d: worst error %.3f of its bound over the mpmath sample" % (M, K, axis, worst))


def test_mixed_tape(gpu_required):
    """Elementwise, reduction (32), log_sum_exp, prod and quad_over_lin_rows segments in one tape, a short op-36 block
    between flat segments and a wavefront-form block last, non-zero multipliers on every row: the op-36 rows against
    mpmath, and the rows of g that the other classes feed are the bits of the same problem without the op-36 atoms."""
    UA, yA = qr.rows_of_shape(6, 5, seed=31)
    UB, yB = qr.rows_of_shape(2, 70, seed=32)

    def problem(with_rows):
        rng = np.random.default_rng(9)
        u, v, q, s = cp.Variable(50), cp.Variable(9), cp.Variable(7), cp.Variable()
        L, P = cp.Variable((3, 5)), cp.Variable((4, 3))
        u.value, v.value, q.value, s.value = rng.standard_normal(50), rng.uniform(0.5, 2, 9), rng.standard_normal(7), 2.0
        L.value, P.value = lr.rows_of_length(5, 3, seed=33), pr.rows_of_length(3, 4, seed=34)
        cons = [cp.exp(u) <= 3, cp.quad_over_lin(q, s) <= 4, cp.log_sum_exp(L, axis=1) <= 0, cp.sin(v) >= -1, cp.prod(P, axis=1) <= 0]
        if with_rows:
            A, ya, B, yb = cp.Variable((6, 5)), cp.Variable(6), cp.Variable((2, 70)), cp.Variable(2)
            A.value, ya.value, B.value, yb.value = UA, yA, UB, yB
            cons = cons[:1] + [cp.quad_over_lin_rows(A, ya, axis=1) <= 0] + cons[1:] + [cp.quad_over_lin_rows(B, yb, axis=1) <= 0]
        return cp.Problem(cp.Minimize(cp.sum(cp.exp(u))), cons)

    full, bare = lp.lower(problem(True)), lp.lower(problem(False))
    a, b = full["tape_arrays"], bare["tape_arrays"]
    assert list(a["seg_op"]) == [1, 1, 36, 32, 34, 6, 35, 36] and list(b["seg_op"]) == [1, 1, 32, 34, 6, 35]
    xa, xb = np.array(full["x0"], dtype=float), np.array(bare["x0"], dtype=float)
    ma, mb = int(a["dims"][1]), int(b["dims"][1])
    lam_a = lp.multipliers(ma)
    da, db = _device(a), _device(b)
    try:
        ga = da.eval_g(xa)
        gb = db.eval_g(xb)
        for s, M in ((2, 6), (7, 2)):
            # (the denominators are the canonicaliser's nonneg variables, started at the given values: all > 1e-4)
            print("mixed tape, segment %d: worst error %.3f of its bound" % (s, qr.check_segment("mixed tape", da, (a, xa, lam_a, 0.5), s)))
    finally:
        da.close()
        db.close()
    # the other atoms' constraint rows: those whose z column is not an op-36 segment's
    import scipy.sparse as sp
    def rows_of_other_atoms(t, skip):
        N, m, Z = (int(v) for v in t["dims"][:3])
        G = sp.csr_matrix((t["G_val"], t["G_idx"], t["G_ptr"]), shape=(m, N + Z)).tocsc()
        out = []
        for s in range(len(t["seg_op"])):
            if int(t["seg_op"][s]) in skip:
                continue
            zo, zc = int(t["seg_zoff"][s]), int(t["seg_zcount"][s])
            for col in N + zo + np.arange(zc):
                out.extend(G.indices[G.indptr[col]:G.indptr[col + 1]].tolist())
        return np.array(out)
    ra, rb = rows_of_other_atoms(a, {36}), rows_of_other_atoms(b, set())
    assert ra.size == rb.size == 50 + 1 + 3 + 9 + 4
    assert ga[ra].tobytes() == gb[rb].tobytes()


def test_mixed_tape_fills_all_six_row_tables(gpu_required):
    """All three members of the row class in both kernel forms in one tape -- log_sum_exp 3 x 5 and 2 x 70, prod 4 x 3 and
    2 x 66, quad_over_lin_rows 6 x 5, 2 x 70 and 1 x 2049 (the workgroup form) -- so that one sweep walks six non-empty row
    tables; an elementwise segment between the short and the long blocks, non-zero multipliers on every row.  Every
    row-class segment against its own mpmath reference within that atom's bound; two evaluations give the same bytes."""
    from test_log_sum_exp_gpu import _check_segment_mpmath as check_lse
    from test_prod_gpu import _check_rows_mpmath as check_prod
    qol_sets = [qr.rows_of_shape(6, 5, seed=61), qr.rows_of_shape(2, 70, seed=62), qr.rows_of_shape(1, 2049, seed=63)]
    rng = np.random.default_rng(9)
    u, v = cp.Variable(50), cp.Variable(9)
    u.value, v.value = rng.standard_normal(50), rng.uniform(0.5, 2, 9)
    Ls, Ll, Ps, Pl = cp.Variable((3, 5)), cp.Variable((2, 70)), cp.Variable((4, 3)), cp.Variable((2, 66))
    Ls.value, Ll.value = lr.rows_of_length(5, 3, seed=64), lr.rows_of_length(70, 2, seed=65)
    Ps.value, Pl.value = pr.rows_of_length(3, 4, seed=66), pr.rows_of_length(66, 2, seed=67)
    Qs, ys, Ql, yl, Qw, yw = cp.Variable((6, 5)), cp.Variable(6), cp.Variable((2, 70)), cp.Variable(2), cp.Variable(2049), cp.Variable()
    (Qs.value, ys.value), (Ql.value, yl.value) = qol_sets[0], qol_sets[1]
    Qw.value, yw.value = qol_sets[2][0][0], qol_sets[2][1][0]
    cons = [cp.exp(u) <= 3, cp.log_sum_exp(Ls, axis=1) <= 0, cp.prod(Ps, axis=1) <= 0, cp.quad_over_lin_rows(Qs, ys, axis=1) <= 0,
            cp.sin(v) >= -1, cp.log_sum_exp(Ll, axis=1) <= 0, cp.prod(Pl, axis=1) <= 0, cp.quad_over_lin_rows(Ql, yl, axis=1) <= 0,
            cp.quad_over_lin_rows(Qw, yw) <= 0]
    data = lp.lower(cp.Problem(cp.Minimize(cp.sum(cp.exp(u))), cons))
    a, x = data["tape_arrays"], np.array(data["x0"], dtype=float)
    assert list(a["seg_op"]) == [1, 1, 34, 35, 36, 6, 34, 35, 36, 36]
    assert [(int(a["seg_d0"][s]), int(a["seg_d1"][s])) for s in (2, 3, 4, 6, 7, 8, 9)] == [(3, 5), (4, 3), (6, 5), (2, 70), (2, 66), (2, 70), (1, 2049)]
    lam = lp.multipliers(int(a["dims"][1]))
    dev = _device(a)
    try:
        g, J, H = dev.eval_g(x), dev.eval_jac_g(x), dev.eval_h(x, lam, 0.5)
        assert (dev.eval_g(x).tobytes(), dev.eval_jac_g(x).tobytes(), dev.eval_h(x, lam, 0.5).tobytes()) == (g.tobytes(), J.tobytes(), H.tobytes())
        for s in (2, 6):
            print("six tables, log_sum_exp segment %d: worst error %.3f of its bound" % (s, check_lse(a, x, lam, g, J, H, s, np.arange(int(a["seg_d0"][s])))))
        for s in (3, 7):
            print("six tables, prod segment %d: worst error %.3f of its bound" % (s, check_prod(a, x, lam, g, J, H, s, np.arange(int(a["seg_d0"][s])))))
        for s in (4, 8, 9):
            print("six tables, quad_over_lin_rows segment %d: worst error %.3f of its bound" % (s, qr.check_segment("six tables", dev, (a, x, lam, 0.5), s)))
    finally:
        dev.close()


def test_first_derivatives_do_not_depend_on_the_hessian_pass(gpu_required):
    for tape in (_shape_tape(20000, 3, 1), _shape_tape(37, 129, 1), _shape_tape(1, 4097, None)):
        a, x, lam, sigma = tape
        fresh = _device(a)
        try:
            j0, v0 = fresh.eval_jac_g(x).tobytes(), fresh.eval_g(x).tobytes()            # (with_h off)
            fresh.eval_h(x, lam, sigma)                                                   # (with_h on)
            assert fresh.eval_jac_g(x).tobytes() == j0 and fresh.eval_g(x).tobytes() == v0
        finally:
            fresh.close()
        other = _device(a)
        try:
            other.eval_h(x, lam, sigma)
            assert other.eval_jac_g(x).tobytes() == j0 and other.eval_g(x).tobytes() == v0
        finally:
            other.close()


# ---- 2. bit-for-bit repeat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,axis", [(20000, 3, 1), (1000, 65, 1), (1, 4097, None)])
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
# (the paths of tests/test_prod_gpu.py; "in-kernel" is asked for by name: device_loop="yes" raises where the in-kernel loop
# cannot take the problem)
PATHS = {"in-kernel": {"device_loop": "yes"}, "host-driven": {"device_loop": "no"}, "limited-memory": {"hessian_approximation": "limited-memory"}}


def _agree(values):
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * abs(values["host-driven"]), values


def test_the_issue_example_solves(gpu_required):
    values = []
    for loop in (False, True):
        prob, X, want = qp.norms_over_a_bound(loop)
        prob.solve(nlp=True)
        assert prob.status == cp.OPTIMAL and abs(prob.value - want) <= qp.VALUE_TOL * want, (loop, prob.status, prob.value)
        values.append(prob.value)
    assert abs(values[0] - values[1]) <= qp.VALUE_TOL * values[1], values


def test_fermat_weber_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, p = qp.fermat_weber()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        qp.assert_optimum("Fermat-Weber, " + name, prob.value, qp.FW_VALUE, p.value, qp.FW_POINT)
        values[name] = prob.value
    _agree(values)
    loop, _ = qp.fermat_weber(loop=True)
    loop.solve(nlp=True)
    assert abs(loop.value - values["host-driven"]) <= qp.VALUE_TOL * abs(loop.value)


def test_enclosing_circle_on_every_path(gpu_required):
    """(solved at qol_rows_problems.CIRCLE_OPTS on every path, and so is the loop statement)"""
    values = {}
    for name, opts in PATHS.items():
        prob, c, r = qp.enclosing_circle()
        prob.solve(nlp=True, **opts, **qp.CIRCLE_OPTS)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        qp.assert_circle(name, prob.value, c.value)
        values[name] = prob.value
    _agree(values)
    loop, c, r = qp.enclosing_circle(loop=True)
    loop.solve(nlp=True, **qp.CIRCLE_OPTS)
    qp.assert_circle("loop", loop.value, c.value)
    assert abs(loop.value - values["host-driven"]) <= qp.VALUE_TOL * abs(loop.value)


@pytest.mark.parametrize("axis", [1, 0])
def test_group_lasso_on_every_path(axis, gpu_required):
    Xs, vs = qp.lasso_optimum()
    values = {}
    for name, opts in PATHS.items():
        prob, X = qp.group_lasso(axis)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        qp.assert_optimum("group lasso, axis %d, %s" % (axis, name), prob.value, vs, X.value, Xs if axis == 1 else Xs.T)
        values[name] = prob.value
    _agree(values)
    loop, _ = qp.group_lasso(axis, loop=True)
    loop.solve(nlp=True)
    assert abs(loop.value - values["host-driven"]) <= qp.VALUE_TOL * abs(loop.value)


def test_best_of_on_fermat_weber(gpu_required):
    """A convex problem: every start ends at the one optimum."""
    prob, p = qp.fermat_weber(start=False)
    p.sample_bounds = [-2, 3]
    prob.solve(nlp=True, best_of=8)
    assert prob.status == cp.OPTIMAL
    objs = np.asarray(prob.solver_stats.extra_stats["all_objs_from_best_of"])
    assert objs.size == 8 and np.max(np.abs(objs - qp.FW_VALUE)) <= qp.VALUE_TOL * qp.FW_VALUE, objs
    qp.assert_optimum("Fermat-Weber, best_of", prob.value, qp.FW_VALUE, p.value, qp.FW_POINT)


# ---- 4. batch ---------------------------------------------------------------------------------------------------------------------
def _anchor_thetas(count):
    """Per instance a scaled and shifted unit square: its centre is the point, scale * 2 sqrt(2) the value."""
    rng = np.random.default_rng(21)
    scale, shift = rng.uniform(0.5, 4.0, count), rng.uniform(-3.0, 3.0, (count, 2))
    anchors = scale[:, None, None] * qp.SQUARE[None] + shift[:, None, :]
    return np.stack([anchors[i].reshape(-1, order="F") for i in range(count)]), scale, shift


@pytest.mark.parametrize("count", [256, 1024])
def test_fermat_weber_batch_takes_the_generic_kernel(count, gpu_required):
    from dnlp_amd.batch import ParametricBatch
    thetas, scale, shift = _anchor_thetas(count)
    runs = []
    for _ in range(2):
        tprob, p, params = qp.fermat_weber(parameters=True)
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
    want = scale * qp.FW_VALUE
    assert np.max(np.abs(objs - want) / want) <= qp.VALUE_TOL, float(np.max(np.abs(objs - want) / want))
