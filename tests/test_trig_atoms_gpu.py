"""cosh, atan, asin, acos and atan2 on the MI355X (flat tape ops 17, 18, 19 and 22): the hipcc build of csrc/atom_math.h through
_capi.DeviceProblem on sweep_flat_kernel's double2 path (the unary ops) and on its scalar path (contiguous and gathered
arguments, bit for bit equal on equal inputs), a tape that mixes the four ops with exp and multiply, the edge classes, repeats,
the hiprtc builds through eval_fused in this process and in one child process that imported torch first, the four solves of
tests/trig_problems.py on the in-kernel loop, the host-driven loop and the limited-memory mode, and the bearing template as a
batch of 64 (the library's wavefront kernel) and of 1024 (the kernel compiled per template at run time).  Same grids, same
bound, same K as tests/test_trig_atoms_cpu.py (tests/trig_reference.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import atom_reference as ar
import dnlp_amd as cp
import test_trig_atoms_cpu as cpu
import trig_problems as tp
import trig_reference as tr
from dnlp_amd.tape import serialize

pytestmark = pytest.mark.gpu

ATOMS = cpu.ATOMS
UNARY = ["cosh", "atan", "asin"]
OP = cpu.OP
SCALAR_SIZES = (1, 63, 64, 65, 257)


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


def unit_is_vector(a):
    """Per flat unit: does sweep_flat_kernel (csrc/exec_hip.h) move it as half of a double2?  Lane e0 (even) takes units e0 and
    e0 + 1 together when both lie in one UNARY segment with a contiguous argument and x, z, dvals and hvals offsets are all even."""
    n = np.asarray(a["seg_n"], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(n)])
    out = np.zeros(int(start[-1]), dtype=bool)
    for e0 in range(0, int(start[-1]), 2):
        s = int(np.searchsorted(start, e0, side="right") - 1)
        i = e0 - int(start[s])
        base = int(a["seg_a0_base"][s])
        offs = base + i, int(a["seg_zoff"][s]) + i, int(a["seg_doff"][s]) + i, int(a["seg_hoff"][s]) + i
        if int(a["seg_op"][s]) < 20 and e0 + 1 < start[s + 1] and base >= 0 and all(o % 2 == 0 for o in offs):
            out[e0] = out[e0 + 1] = True
    return out


def finite_grid(name):
    """The grid without the four points of cosh next to and past the overflow threshold (tests/test_trig_atoms_cpu.py has them
    on a tape of their own), plus one more point where the count is odd: every unit of a unary op is then half of a double2."""
    args = list(tr.grid_args(OP[name]))
    keep = np.abs(tr.reference(OP[name], *args)[0][0]) < 1e305
    args = [u[keep] for u in args]
    if args[0].size % 2:
        args = [np.concatenate([u, [0.75]]) for u in args]
    return args


_tapes = {}


def grid_tape(name):
    """One constraint of the atom on its whole grid, behind a placeholder variable of two entries (every offset even)."""
    if ("v", name) not in _tapes:
        args = finite_grid(name)
        a = cpu.lower(cp.Problem(cp.Minimize(0 * cp.sum(cpu._var(2))), [cpu.apply_atom(name, args[0].size) <= 0]))
        assert list(a["seg_op"]) == [OP[name]]
        _tapes[("v", name)] = (a, cpu.fill(a, [args]), cpu.multipliers(int(a["dims"][1])), 0.5, args)
    return _tapes[("v", name)]


def scalar_tape(name, gathered):
    """Segments of 1, 63, 64, 65 and 257 units on the first points of the grid, behind a placeholder variable of ONE entry: the
    x offset of every pair of units has the other parity than its z offset, so no unit is a double2.  `gathered[k]`: argument k
    is read through the gather list, in reversed order (the front end's segment with its base set to -1 and its list rewritten)."""
    key = ("s", name, tuple(gathered))
    if key not in _tapes:
        args = grid_tape(name)[4]
        # (lowered as written, without the canonical form: asin's auxiliary variables would sit between the arguments and give
        #  some segments the parity of a double2; every argument here is a bare variable, which is all the lowering needs)
        from dnlp_amd.nlp_solver import build_nlp_data
        plain = cp.Problem(cp.Minimize(0 * cp.sum(cpu._var(1))), [cpu.apply_atom(name, n) <= 0 for n in SCALAR_SIZES])
        a = dict(build_nlp_data(plain)[0]["tape_arrays"])
        assert list(a["seg_op"]) == [OP[name]] * len(SCALAR_SIZES) and list(a["seg_n"]) == list(SCALAR_SIZES)
        for k, which in enumerate(("a0", "a1")[:len(args)]):
            assert all(int(b) >= 0 for b in a["seg_%s_base" % which])
            if gathered[k]:
                a["seg_%s_base" % which], a["gidx"] = a["seg_%s_base" % which].copy(), a["gidx"].copy()
                for s, n in enumerate(SCALAR_SIZES):
                    o = int(a["seg_%s_off" % which][s])
                    a["gidx"][o:o + n] = a["gidx"][o:o + n][::-1].copy()
                    a["seg_%s_base" % which][s] = -1
        x = cpu.fill(a, [[u[:n] for u in args] for n in SCALAR_SIZES])
        _tapes[key] = (a, x, cpu.multipliers(int(a["dims"][1])), 0.5, args)
    return _tapes[key]


def check_tape(dev, a, x, lam, sigma):
    """g and the Jacobian (a sweep without the Hessian), then the Hessian (a sweep with it), entry by entry against mpmath."""
    exp = tr.expected_oracles(a, x, lam, sigma)
    for units in exp["units"]:
        assert np.mean(units.st == 1) <= tr.LEFT_OUT_SHARE
    got = {"g": dev.eval_g(x), "jac": dev.eval_jac_g(x), "hess": dev.eval_h(x, lam, sigma)}
    failed = []
    for k, v in got.items():
        try:
            exp[k].check(v)
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)
    return got


def per_unit(a, x, lam, sigma, got):
    """The outputs per flat unit in tape order, per segment: [value, derivative runs, Hessian runs / w] out of eval_g /
    eval_jac_g / eval_h (one-to-one maps with coefficients +-1, which is asserted; w = +-2^j, so the division is exact)."""
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])
    Gz = ar._csr(a, "G", (m, N + Z)).tocsc()[:, N:].tocsc()
    MJ, MH = ar._csr(a, "MJ", (nnzJ, nd)).tocsc(), ar._csr(a, "MH", (nnzH, nh)).tocsc()
    flat = []
    for M, vec in ((Gz, got["g"]), (MJ, got["jac"]), (MH, got["hess"])):
        assert np.all(np.diff(M.indptr) == 1) and np.all(np.abs(M.data) == 1.0)
        flat.append(np.asarray(vec)[M.indices] / M.data)
    out = []
    for s in range(nseg):
        n, zo, do, ho = (int(a[k][s]) for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff"))
        two = int(a["seg_op"][s]) == tr.OP_ATAN2
        cols = [flat[0][zo:zo + n]]
        cols += [flat[1][do + r * n:do + (r + 1) * n] for r in range(2 if two else 1)]
        with np.errstate(all="ignore"):
            cols += [flat[2][ho + r * n:ho + (r + 1) * n] / w[zo:zo + n] for r in range(3 if two else 1)]
        out.append(cols)
    return out


def callbacks(dev, x, lam, sigma):
    return {"g": dev.eval_g(x), "jac": dev.eval_jac_g(x), "hess": dev.eval_h(x, lam, sigma)}


# ---- 1. the rule: the hipcc build ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ATOMS)
def test_whole_grid_as_one_segment_against_mpmath(name, gpu_required):
    """The vector path for the unary ops (every unit half of a double2); atan2 has two arguments and always takes the scalar path."""
    a, x, lam, sigma, _ = grid_tape(name)
    assert unit_is_vector(a).all() == (name != "atan2") and unit_is_vector(a).any() == (name != "atan2")
    dev = _device(a)
    try:
        check_tape(dev, a, x, lam, sigma)
    finally:
        dev.close()


def _gather_cases(name):
    return [(False, False), (True, False), (False, True), (True, True)] if name == "atan2" else [(False,), (True,)]


@pytest.mark.parametrize("name,gathered", [(n, g) for n in ATOMS for g in _gather_cases(n)])
def test_scalar_path_against_mpmath_and_equal_to_the_grid_tape_bit_for_bit(name, gathered, gpu_required):
    a, x, lam, sigma, args = scalar_tape(name, gathered)
    assert not unit_is_vector(a).any()
    av, xv, lamv, sigmav, _ = grid_tape(name)
    ds, dv = _device(a), _device(av)
    try:
        s_out = per_unit(a, x, lam, sigma, check_tape(ds, a, x, lam, sigma))
        v_out = per_unit(av, xv, lamv, sigmav, callbacks(dv, xv, lamv, sigmav))[0]
    finally:
        ds.close()
        dv.close()
    for s, n in enumerate(SCALAR_SIZES):
        for k, (sc, ve) in enumerate(zip(s_out[s], v_out)):
            assert np.array_equal(cpu.bits(sc), cpu.bits(ve[:n])), (name, gathered, n, k)


_mixed = {}


def mixed_tape():
    """cosh, atan2 and exp in the objective; atan, asin, multiply and atan2 in constraints: segments of 37 units on points of the
    grids where nothing overflows in a sum."""
    if not _mixed:
        n = 37
        rng = np.random.default_rng(77)
        y2, x2 = tr.grid(tr.OP_ATAN2)
        obj = cp.sum(cp.cosh(cpu._var(n))) + cp.sum(cp.atan2(cpu._var(n), cpu._var(n))) + cp.sum(cp.exp(cpu._var(n)))
        cons = [cp.atan(cpu._var(n)) <= 0, cp.asin(cpu._var(n)) <= 0, cp.multiply(cpu._var(n), cpu._var(n)) <= 0,
                cp.atan2(cpu._var(n), cpu._var(n)) <= 0]
        a = cpu.lower(cp.Problem(cp.Minimize(obj), cons))
        assert list(a["seg_op"]) == [17, 22, 1, 18, 19, 20, 22]
        per_segment = [[tr.grid(tr.OP_COSH)[3000:3000 + n]], [y2[16000:16000 + n], x2[16000:16000 + n]], [rng.uniform(-2, 2, n)],
                       [tr.grid(tr.OP_ATAN)[:n]], [tr.grid(tr.OP_ASIN)[:n]], [rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)],
                       [y2[:n], x2[:n]]]
        _mixed["t"] = (a, cpu.fill(a, per_segment), cpu.multipliers(int(a["dims"][1])), 0.5)
    return _mixed["t"]


def test_callbacks_of_a_tape_that_mixes_the_ops_with_exp_and_multiply(gpu_required):
    a, x, lam, sigma = mixed_tape()
    exp = tr.expected_oracles(a, x, lam, sigma)
    dev = _device(a)
    try:
        got = {"f": [dev.eval_f(x)], "grad_f": dev.eval_grad_f(x), "g": dev.eval_g(x), "jac": dev.eval_jac_g(x), "hess": dev.eval_h(x, lam, sigma)}
    finally:
        dev.close()
    failed = []
    for k, v in got.items():
        try:
            exp[k].check(v)
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


def test_edge_classes_equal_the_host_builds(gpu_required):
    from oracle.oracle_capi import OracleProblem
    out = {}
    for tape_name in ("edges", "overflow"):
        a = cpu.tape(tape_name)[0]
        dev = _device(a)
        try:
            out[tape_name] = (cpu.unit_outputs(dev, tape_name), cpu.unit_outputs(OracleProblem(serialize(a)), tape_name))
        finally:
            dev.close()
    cpu.assert_edge_classes(out["edges"][0])
    for tape_name, (dev_out, host_out) in out.items():
        for name in dev_out:
            for k, (d, h) in enumerate(zip(dev_out[name], host_out[name])):
                assert np.array_equal(np.isnan(d), np.isnan(h)) and np.array_equal(np.isinf(d), np.isinf(h)), (tape_name, name, k, d, h)
                assert np.array_equal(np.sign(d[np.isinf(d)]), np.sign(h[np.isinf(h)])), (tape_name, name, k, d, h)
    val, d1, d2 = out["overflow"][0]["cosh"]
    assert np.array_equal(val[:2], [np.inf, np.inf]) and np.array_equal(d1[:2], [np.inf, -np.inf]) and np.array_equal(d2[:2], [np.inf, np.inf])


def test_cosh_next_to_its_overflow_against_mpmath(gpu_required):
    dev = _device(cpu.tape("overflow")[0])
    try:
        cpu.check_callbacks(dev, "overflow")
    finally:
        dev.close()


def test_two_fresh_handles_and_two_sweeps_give_identical_bits(gpu_required):
    runs = []
    for _ in range(2):
        for name in ATOMS:
            a, x, lam, sigma, _ = grid_tape(name)
            dev = _device(a)
            try:
                for _ in range(2):
                    runs.append((name, np.asarray(dev.eval_g(x)).tobytes(), np.asarray(dev.eval_jac_g(x)).tobytes(),
                                 np.asarray(dev.eval_h(x, lam, sigma)).tobytes()))
            finally:
                dev.close()
    assert len(set(runs)) == len(ATOMS)


# ---- 2. the rule: the hiprtc builds (fused objective) --------------------------------------------------------------------------
def _fused_case(name):
    from dnlp_amd.dnlp2smooth import Dnlp2Smooth
    from dnlp_amd.fused import build_fused_spec
    from dnlp_amd.nlp_solver import build_nlp_data
    u = finite_grid(name)[0]
    prob = cp.Problem(cp.Minimize(cp.sum(getattr(cp, name)(cpu._var(u.size)))), [])
    smooth, _ = Dnlp2Smooth().apply(prob)
    spec = build_fused_spec(prob)
    assert spec is not None
    data, _ = build_nlp_data(smooth, user_variables=prob.variables(), fused_spec=spec)
    ta = dict(data["tape_arrays"])
    assert data["fused"] and ta["free_idx"].size == u.size
    return ta, u


def _fused_results(out_path):
    """Runs every fused case on device 0 and stores f and grad (the child process calls this after importing torch)."""
    from dnlp_amd import _capi
    out = {}
    for name in UNARY:
        ta, u = _fused_case(name)
        dev = _capi.DeviceProblem(serialize(ta), None, device=0)
        try:
            f, g = dev.eval_fused(u.copy())
        finally:
            dev.close()
        out[name + "_f"], out[name + "_g"] = np.array([f]), g
    np.savez(out_path, **out)


def _check_fused(results):
    K = tr.measured_K()
    for name in UNARY:
        ta, u = _fused_case(name)
        hi, lo, br, st = tr.reference(OP[name], u)
        assert not np.any(st[0]) and np.mean(st[1] == 1) <= tr.LEFT_OUT_SHARE
        val, d1 = ar.Units(u.size), ar.Units(u.size)
        for k, units in ((0, val), (1, d1)):
            units.hi[:], units.lo[:], units.tol[:], units.st[:] = hi[k], lo[k], K[OP[name]][k] * tr.EPS * br[k], st[k]
            units.who = [(0, name, (float(v),)) for v in u]
        ar.Entries(None, None, None, sp.identity(u.size, format="csr"), d1, "fused grad").check(results[name + "_g"])
        ar.Entries(np.asarray(ta["fz_c0"], float)[:1], None, None, sp.csr_matrix(np.ones((1, u.size))), val, "fused f").check(results[name + "_f"])


def test_fused_kernels_of_this_process_against_mpmath(gpu_required, tmp_path):
    path = str(tmp_path / "fused.npz")
    _fused_results(path)
    _check_fused(np.load(path))


_TORCH_FIRST_CHILD = r"""
import sys
import torch                                  # FIRST: the process then compiles with the hiprtc / comgr torch ships
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import os
os.environ["DNLP_KERNEL_CACHE"] = sys.argv[2]          # (a cache of its own: the kernels are compiled here, by this compiler)
import test_trig_atoms_gpu
test_trig_atoms_gpu._fused_results(sys.argv[3])
print("DONE", flush=True)
"""


def test_fused_kernels_of_a_process_that_imported_torch_first_against_mpmath(gpu_required, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cache = tmp_path / "kc"
    cache.mkdir(mode=0o700)
    path = str(tmp_path / "fused_child.npz")
    e = dict(os.environ)
    e.pop("DNLP_RTC_COMPILER", None)
    r = subprocess.run([sys.executable, "-c", _TORCH_FIRST_CHILD, root, str(cache), path], capture_output=True, text=True,
                       timeout=600, env=e)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    _check_fused(np.load(path))


# ---- 3. solves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(tp.MODES))
@pytest.mark.parametrize("name", sorted(tp.SOLVES))
def test_solve_on_the_device(name, mode, gpu_required):
    prob, var, xs, fs = tp.SOLVES[name]()
    prob.solve(nlp=True, **tp.SOLVE_OPTS[name], **tp.MODES[mode])
    tp.assert_solution(name, prob, var, xs, fs)


def test_cosh_problem_takes_the_lbfgs_path(gpu_required):
    """Unconstrained and convex: algorithm='lbfgs' takes it (the rows t == A x - b only define t).  A x is a matrix product, not
    an elementwise term, so the objective has no fused program and the device L-BFGS loop evaluates the tape."""
    prob, var, xs, fs = tp.cosh_problem()
    prob.solve(nlp=True, algorithm="lbfgs", tol=1e-10)
    assert prob._nlp_cache["data"]["reducible"]
    tp.assert_solution("cosh", prob, var, xs, fs)
    assert np.max(np.abs(tp.cosh_gradient(var.value))) <= 1e-8


def test_elementwise_cosh_objective_takes_the_fused_lbfgs_path(gpu_required):
    """sum(cosh(x - b) + atan(x)^2): elementwise, so the fused f + grad f kernel drives the L-BFGS loop.  The optimum solves
    sinh(x_i - b_i) + 2 atan(x_i) / (1 + x_i^2) = 0 per entry (scipy's brentq, 1e-15)."""
    import scipy.optimize as so
    b = np.linspace(-1.0, 1.0, 50)
    x = cp.Variable(50)
    x.value = np.zeros(50)
    prob = cp.Problem(cp.Minimize(cp.sum(cp.cosh(x - b) + cp.square(cp.atan(x)))))
    prob.solve(nlp=True, algorithm="lbfgs", tol=1e-10)
    d = prob._nlp_cache["data"]
    assert prob._nlp_cache["sig"][0] == "direct" and d["fused"] and d["tape"].m == 0
    xs = np.array([so.brentq(lambda t: np.sinh(t - bi) + 2 * np.arctan(t) / (1 + t * t), -3, 3, xtol=1e-15, rtol=1e-15) for bi in b])
    fs = float(np.sum(np.cosh(xs - b) + np.arctan(xs) ** 2))
    assert prob.status == cp.OPTIMAL and abs(prob.value - fs) <= tp.REL_TOL * abs(fs)
    assert np.max(np.abs(np.asarray(x.value) - xs)) <= tp.REL_TOL * np.max(np.abs(xs))


# ---- 4. batch ------------------------------------------------------------------------------------------------------------------
BATCH_OPTS = {"linear_solver": "sparse", "tol": 1e-10}      # (order 32: the automatic choice is the dense KKT, which the wavefront kernels do not take)
_host_rows = {}


def host_answers(pb, thetas):
    """Per row (status, objective, x) of the host build solving that row's own tape; computed once for the 1024 rows."""
    if "rows" not in _host_rows:
        from dnlp_amd.batch import arrays_with_data
        from dnlp_amd.nlp_solver import HIPNLP
        from oracle.oracle_capi import OracleProblem
        mat = pb.data(thetas)
        out = []
        for i in range(mat.shape[0]):
            arr = arrays_with_data(pb.arrays0, mat[i])
            o = OracleProblem(serialize(arr))
            for k, v in dict(HIPNLP.DEFAULT_OPTIONS, **BATCH_OPTS).items():
                o.set_option(k, v)
            ref = o.solve(arr["x0"])
            out.append((int(ref["status"]), float(ref["obj_val"]), np.asarray(ref["x"], float).copy()))
        _host_rows["rows"] = out
    return _host_rows["rows"]


@pytest.mark.parametrize("count", [64, 1024])
def test_bearing_batch_agrees_with_the_host_build(count, gpu_required):
    """The bearing template with the five bearings as parameters.  64 instances: the library's wavefront kernel; 1024, the
    smallest launch that takes it: the kernel compiled for this template at run time.  Every instance has status 0 and lies
    within 1e-6 (relative) of the host build's answer for the same row, objective and point."""
    from dnlp_amd.batch import ParametricBatch
    tprob, params, p = tp.bearing_template()
    pb = ParametricBatch(tprob, params)
    assert 22 in list(pb.arrays0["seg_op"])
    all_rows = tp.bearing_rows(1024)
    assert np.all(np.abs(all_rows) <= np.pi - tp.CUT_MARGIN)
    try:
        ref = host_answers(pb, all_rows)[:count]
        res = pb.solve(all_rows[:count], **BATCH_OPTS)
        launch = res.raw["launch"]
        assert launch["wave_form"] != 0 and launch["wave_refused"] == 0 and not launch["wave_wg"], launch
        assert launch["wave_spec"] == (count >= 1024), launch
        assert np.all(np.asarray(res.status) == 0), np.flatnonzero(np.asarray(res.status))[:10]
        for i, (st, fv, xv) in enumerate(ref):
            assert st == 0, (i, st)
            assert abs(res.raw["obj_val"][i] - fv) <= 1e-6 * abs(fv), (i, res.raw["obj_val"][i], fv)
            assert np.max(np.abs(res.x[i] - xv)) <= 1e-6 * np.max(np.abs(xv)), (i, res.x[i], xv)
        xs, fs = tp.ANSWERS["bearing"]
        assert abs(res.raw["obj_val"][0] - fs) <= tp.REL_TOL * abs(fs)
        assert np.max(np.abs(np.asarray(res.value_of(p))[0].reshape(-1) - xs)) <= tp.REL_TOL * np.max(np.abs(xs))
    finally:
        pb.close()
