"""matrix_frac on the device: the row-class kernels of OP_MATRIX_FRAC (csrc/exec_hip_rows.h sweep_mfrac_kernel /
sweep_mfrac_long_kernel / sweep_mfrac_hess_kernel) entry by entry against mpmath within the brackets of
tests/matrix_frac_reference.py, on shapes that reach both kernel forms and their edges; many segments of mixed shapes
beside log_det and log_sum_exp in one sweep; the out-of-domain table in both forms; bit-for-bit repeats; the solves of
tests/matrix_frac_problems.py through the front-end on every solver path; the covariance-form likelihood as a batch
template."""
import numpy as np
import pytest

import dnlp_amd as cp
import logdet_reference as lr
import lse_problems as lp
import matrix_frac_problems as mq
import matrix_frac_reference as mr
from dnlp_amd.tape import serialize
from logdet_problems import matrix_from_entries
from test_matrix_frac_cpu import check_callbacks, check_mixed, check_out_of_domain

pytestmark = pytest.mark.gpu


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


_cache = {}


def _shape_tape(n, m):
    if (n, m) not in _cache:
        _cache[(n, m)] = mq.segments_tape([mr.inputs_of(n, m, 100.0 if n > 1 else 1.0, n > 1)])
    return _cache[(n, m)]


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", mr.SHAPES)
def test_one_segment_of_every_shape(n, m, gpu_required):
    """N = n + m <= 8: the short form with every group width (N^2 = 4, 9, 16, 49, 64), 8 its last order; (6, 4): K = 60
    but N^2 = 100, the long form; 9 the first long order; (6, 3), (10, 35): m > 1 in the long form; N = 32 fills every
    lane's 16th entry exactly, 33 goes past it; N = 45 with m = 1 and with m > n; n = 1.  The value, every d and 2000
    sampled Hessian entries (all of them where there are no more) against mpmath through the callbacks."""
    tape = _shape_tape(n, m)
    dev = _device(tape[0])
    try:
        check_callbacks(dev, tape, hsample=2000)
    finally:
        dev.close()


def _forty_tape():
    if "forty" not in _cache:
        shapes = [((2, 1), (3, 2), (6, 4), (9, 2))[k % 4] for k in range(40)]
        pairs = [mr.inputs_of(n, m, mr.CONDS[k % 4], k % 2 == 1, seed=mr.SEED + 100 + k) for k, (n, m) in enumerate(shapes)]

        def extra(cp_):
            L = cp_.Variable((3, 5))
            L.value = np.zeros((3, 5))
            D3, D9 = cp_.Variable((3, 3)), cp_.Variable((9, 9))
            D3.value, D9.value = np.eye(3), np.eye(9)
            return [cp_.log_sum_exp(L, axis=1) <= 3, cp_.log_det(D3) <= 0, cp_.log_det(D9) <= 0]
        a, x, lam, sigma = mq.segments_tape(pairs, extra=extra)
        # the log_det segments read variables T of their own: positive definite matrices go there
        for s, n in ((41, 3), (42, 9)):
            off = int(a["seg_a0_off"][s])
            x[np.asarray(a["gidx"][off:off + n * n])] = lr.matrix(n, 100.0, True).reshape(-1, order="F")
        _cache["forty"] = (a, x, lam, sigma)
    return _cache["forty"]


def test_forty_segments_of_mixed_shapes_beside_log_det_and_log_sum_exp(gpu_required):
    """The table search, both matrix_frac tables, both log_det tables and log_sum_exp's in one sweep; the matrix_frac and
    the log_det segments against mpmath, the log_sum_exp rows against scipy."""
    from scipy.special import logsumexp
    a, x, lam, sigma = _forty_tape()
    assert list(a["seg_op"]) == [38] * 40 + [34, 37, 37]
    dev = _device(a)
    try:
        check_callbacks(dev, (a, x, lam, sigma), hsample=2000)
        g = dev.eval_g(x)
    finally:
        dev.close()
    off = int(a["seg_a0_off"][40])
    rows = x[np.asarray(a["gidx"][off:off + 15])].reshape(3, 5)
    want = np.abs(logsumexp(rows, axis=1) - 3)
    for v in want:
        assert np.min(np.abs(np.abs(g) - v)) <= 1e-13 * max(1.0, v)


@pytest.mark.parametrize("n,m", [(3, 1), (7, 2)])
def test_out_of_domain_table(n, m, gpu_required):
    """(3, 1): the short form; (7, 2): the long one.  What tests/test_matrix_frac_cpu.py out_of_domain_pairs says."""
    check_out_of_domain(_device, n, m)


def test_tape_with_four_row_class_members(gpu_required):
    """matrix_frac in both forms, log_det, log_sum_exp and quad_over_lin_rows in one sweep: what the host build gives."""
    from oracle.oracle_capi import OracleProblem
    a, x, lam = check_mixed(_device)
    dev, host = _device(a), OracleProblem(serialize(a))
    try:
        for name in ("eval_g", "eval_jac_g"):
            assert np.allclose(getattr(dev, name)(x), getattr(host, name)(x), rtol=1e-11, atol=1e-13), name
        assert np.allclose(dev.eval_h(x, lam, 0.5), host.eval_h(x, lam, 0.5), rtol=1e-10, atol=1e-13)
    finally:
        dev.close()


def test_first_derivatives_do_not_depend_on_the_hessian_pass(gpu_required):
    """(`hvals` itself is not visible through the callbacks: a sweep without the Hessian and one with it give the same
    values and first derivatives, in either order)"""
    for tape in (_shape_tape(3, 1), _shape_tape(6, 4), _shape_tape(32, 1)):
        a, x, lam, sigma = tape
        fresh = _device(a)
        try:
            j0, v0 = fresh.eval_jac_g(x).tobytes(), fresh.eval_g(x).tobytes()            # (with_h off)
            h0 = fresh.eval_h(x, lam, sigma).tobytes()                                    # (with_h on)
            assert fresh.eval_jac_g(x).tobytes() == j0 and fresh.eval_g(x).tobytes() == v0
            fresh.eval_jac_g(1.01 * x)                                                    # (with_h off, elsewhere)
            assert fresh.eval_h(x, lam, sigma).tobytes() == h0
        finally:
            fresh.close()
        other = _device(a)
        try:
            assert other.eval_h(x, lam, sigma).tobytes() == h0
            assert other.eval_jac_g(x).tobytes() == j0 and other.eval_g(x).tobytes() == v0
        finally:
            other.close()


# ---- 2. bit-for-bit repeat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["forty", (7, 1), (10, 35)])
def test_sweep_repeats_bit_for_bit(which, gpu_required):
    a, x, lam, sigma = _forty_tape() if which == "forty" else _shape_tape(*which)
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
# (the paths of tests/test_log_det_gpu.py; "in-kernel" is asked for by name: device_loop="yes" raises where the in-kernel
# loop cannot take the problem)
PATHS = {"in-kernel": {"device_loop": "yes"}, "host-driven": {"device_loop": "no"}, "limited-memory": {"hessian_approximation": "limited-memory"}}


def _agree(values):
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * max(1.0, abs(values["host-driven"])), values


@pytest.mark.parametrize("n,count,width", [(3, 4, None), (6, 10, 4)])
def test_covariance_form_likelihood_on_every_path(n, count, width, gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, s = mq.likelihood_problem(n, count, width)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        mq.assert_likelihood(matrix_from_entries(s.value, n), prob.value, mq.samples(n, count))
        values[name] = prob.value
    _agree(values)


def test_diagonal_covariance_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, d = mq.diagonal_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        mq.assert_diagonal(d.value, prob.value)
        values[name] = prob.value
    _agree(values)


def test_generalised_least_squares_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, x, t = mq.gls_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        mq.assert_gls(x.value, prob.value)
        values[name] = prob.value
    _agree(values)


@pytest.mark.parametrize("kind", ["unit", "twelve"])
def test_a_optimal_design_on_every_path(kind, gpu_required):
    V = mq.a_design_points(kind)
    values = {}
    for name, opts in PATHS.items():
        prob, lam = mq.a_design_problem(V)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        mq.assert_a_design(V, lam.value, prob.value)
        values[name] = prob.value
    _agree(values)


# ---- 4. batch ---------------------------------------------------------------------------------------------------------------------
def _sample_sets(count, n=4, per=8):
    rng = np.random.default_rng(31)
    Y = rng.standard_normal((count, n, per)) * np.linspace(0.5, 2.0, n)[None, :, None]
    return Y, np.stack([Y[i].reshape(-1, order="F") for i in range(count)])


@pytest.mark.parametrize("count", [256])
def test_likelihood_batch_takes_the_generic_kernel(count, gpu_required):
    """The wavefront solvers refuse a template that holds the op (the opcode-set check), so every instance runs on the
    generic in-kernel space, i.e. on csrc/model.h sweep_mfrac_segment; every instance is at its closed form."""
    from dnlp_amd.batch import ParametricBatch
    Y, thetas = _sample_sets(count)
    runs = []
    for _ in range(2):
        tprob, s, params = mq.likelihood_problem(Y=Y[0], parameters=True)
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
    want = np.array([mq.likelihood_optimum(Y[i])[1] for i in range(count)])
    assert np.max(np.abs(objs - want) / np.maximum(1.0, np.abs(want))) <= mq.VALUE_TOL, float(np.max(np.abs(objs - want) / np.maximum(1.0, np.abs(want))))
