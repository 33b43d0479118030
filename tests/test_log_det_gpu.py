"""log_det on the device: the row-class kernels of OP_LOG_DET (csrc/exec_hip_rows.h sweep_logdet_kernel /
sweep_logdet_long_kernel / sweep_logdet_hess_kernel) entry by entry against mpmath within the brackets of
tests/logdet_reference.py, on orders that reach both kernel forms and their edges; many segments of mixed orders beside
another member in one sweep; the out-of-domain table in both forms; bit-for-bit repeats; the solves of
tests/logdet_problems.py through the front-end on every solver path; the Gaussian likelihood as a batch template."""
import numpy as np
import pytest

import dnlp_amd as cp
import logdet_problems as lq
import logdet_reference as lr
from dnlp_amd.tape import serialize
from test_log_det_cpu import check_callbacks, check_mixed, check_out_of_domain, mixed_problem

pytestmark = pytest.mark.gpu


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


_cache = {}


def _order_tape(n):
    if n not in _cache:
        _cache[n] = lq.matrices_tape([lr.matrix(n, 100.0 if n > 1 else 1.0, n > 1)])
    return _cache[n]


# ---- 1. the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 8, 9, 16, 32, 33, 45])
def test_one_matrix_of_every_order(n, gpu_required):
    """n <= 8: the short form with every group width, 8 its last order (K = 64); 9 the first of the long form (K = 81);
    32: K = 1024 fills every lane's 16th entry exactly; 45 the last accepted order (K = 2025).  The value, every d and
    2000 sampled Hessian entries (all of them where there are no more) against mpmath through the callbacks."""
    tape = _order_tape(n)
    dev = _device(tape[0])
    try:
        check_callbacks(dev, tape, hsample=2000)
    finally:
        dev.close()


def _forty_tape():
    if "forty" not in _cache:
        orders = [(2, 3, 9)[k % 3] for k in range(40)]
        conds = [lr.CONDS[k % 4] for k in range(40)]
        mats = [lr.matrix(n, c, k % 2 == 1, seed=lr.SEED + 100 + k) for k, (n, c) in enumerate(zip(orders, conds))]

        def extra(cp_):
            L = cp_.Variable((3, 5))
            L.value = np.zeros((3, 5))
            return [cp_.log_sum_exp(L, axis=1) <= 3]
        _cache["forty"] = lq.matrices_tape(mats, extra=extra)
    return _cache["forty"]


def test_forty_segments_of_mixed_orders_beside_log_sum_exp(gpu_required):
    """The table search, both log_det tables and another member's table in one sweep; the log_sum_exp rows against scipy."""
    from scipy.special import logsumexp
    a, x, lam, sigma = _forty_tape()
    assert list(a["seg_op"]) == [37] * 40 + [34]
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


@pytest.mark.parametrize("n", [3, 9])
def test_out_of_domain_table(n, gpu_required):
    check_out_of_domain(_device, n)


def test_tape_with_three_row_class_members(gpu_required):
    """log_det in both forms, log_sum_exp and quad_over_lin_rows in one sweep: what the host build gives."""
    from oracle.oracle_capi import OracleProblem
    import lse_problems as lp
    a = check_mixed(_device)
    x = np.array(lp.lower(mixed_problem()[0])["x0"], dtype=float)
    lam = lp.multipliers(int(a["dims"][1]))
    dev, host = _device(a), OracleProblem(serialize(a))
    try:
        for name in ("eval_g", "eval_jac_g"):
            assert np.allclose(getattr(dev, name)(x), getattr(host, name)(x), rtol=1e-12, atol=1e-13), name
        assert np.allclose(dev.eval_h(x, lam, 0.5), host.eval_h(x, lam, 0.5), rtol=1e-11, atol=1e-13)
    finally:
        dev.close()


def test_first_derivatives_do_not_depend_on_the_hessian_pass(gpu_required):
    """(`hvals` itself is not visible through the callbacks: a sweep without the Hessian and one with it give the same
    values and first derivatives, in either order)"""
    for tape in (_order_tape(3), _order_tape(9), _order_tape(33)):
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
@pytest.mark.parametrize("which", ["forty", 8, 45])
def test_sweep_repeats_bit_for_bit(which, gpu_required):
    a, x, lam, sigma = _forty_tape() if which == "forty" else _order_tape(which)
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
    assert abs(values["in-kernel"] - values["host-driven"]) <= 1e-8 * max(1.0, abs(values["host-driven"])), values


@pytest.mark.parametrize("start", list(lq.LIKELIHOOD_STARTS))
def test_gaussian_likelihood_on_every_path(start, gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, s = lq.likelihood_problem(start)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lq.assert_likelihood(lq.matrix_from_entries(s.value, 4), prob.value)
        values[name] = prob.value
    _agree(values)


def test_gaussian_likelihood_with_a_plain_matrix_variable_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, X = lq.likelihood_plain_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lq.assert_likelihood((X.value + X.value.T) / 2, prob.value)
        values[name] = prob.value
    _agree(values)


@pytest.mark.parametrize("kind", ["three", "twelve"])
def test_d_optimal_design_on_every_path(kind, gpu_required):
    V = lq.design_points(kind)
    values = {}
    for name, opts in PATHS.items():
        prob, lam = lq.design_problem(V)
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lq.assert_design(V, lam.value, prob.value)
        values[name] = prob.value
    _agree(values)


def test_largest_ellipsoid_in_a_box_on_every_path(gpu_required):
    values = {}
    for name, opts in PATHS.items():
        prob, s, d = lq.ellipsoid_problem()
        prob.solve(nlp=True, **opts)
        assert prob.status == cp.OPTIMAL, (name, prob.status)
        lq.assert_ellipsoid(s.value, d.value, prob.value)
        values[name] = prob.value
    _agree(values)


# ---- 4. batch ---------------------------------------------------------------------------------------------------------------------
def _covariances(count):
    rng = np.random.default_rng(29)
    R = rng.standard_normal((count, 4, 12))
    C = R @ np.transpose(R, (0, 2, 1)) / 12 + 0.1 * np.eye(4)[None]
    return C, np.stack([C[i].reshape(-1, order="F") for i in range(count)])


@pytest.mark.parametrize("count", [256])
def test_likelihood_batch_takes_the_generic_kernel(count, gpu_required):
    """The wavefront solvers refuse a template that holds the op (the opcode-set check), so every instance runs on the
    generic in-kernel space, i.e. on csrc/model.h sweep_logdet_segment; every instance is at its closed form."""
    from dnlp_amd.batch import ParametricBatch
    C, thetas = _covariances(count)
    runs = []
    for _ in range(2):
        tprob, s, params = lq.likelihood_problem(parameters=True)
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
    want = np.array([lq.likelihood_optimum(C[i])[1] for i in range(count)])
    assert np.max(np.abs(objs - want) / np.abs(want)) <= lq.VALUE_TOL, float(np.max(np.abs(objs - want) / np.abs(want)))
