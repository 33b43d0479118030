"""log_normcdf, normcdf and loggamma on the MI355X (flat tape ops 14, 15, 16): the hipcc build of csrc/atom_math.h through
_capi.DeviceProblem on sweep_flat_kernel's double2 path and on its scalar path (bit for bit equal on equal inputs), the hiprtc
builds through eval_fused in this process and in one child process that imported torch first, repeats, the four solves of
tests/special_problems.py through Problem.solve(nlp=True), the fused L-BFGS path, and a 256-instance batch of the probit
template.  Same grids, same bound, same K as tests/test_special_atoms_cpu.py (tests/special_reference.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import atom_reference as ar
import dnlp_amd as cp
import special_problems as spb
import special_reference as sr
import test_special_atoms_cpu as cpu
from dnlp_amd.tape import serialize

pytestmark = pytest.mark.gpu

ATOMS = cpu.ATOMS
OP = cpu.OP
GATHER = 5                              # entries read through an index with stride 2


def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


def unit_is_vector(a):
    """Per flat unit: does sweep_flat_kernel (csrc/exec_hip.h) move it as half of a double2?  Lane e0 (even) takes units e0 and
    e0 + 1 together when both lie in one unary segment with a contiguous argument and x, z, dvals and hvals offsets are all even."""
    n = np.asarray(a["seg_n"], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(n)])
    out = np.zeros(int(start[-1]), dtype=bool)
    for e0 in range(0, int(start[-1]), 2):
        s = int(np.searchsorted(start, e0, side="right") - 1)
        i = e0 - int(start[s])
        base = int(a["seg_a0_base"][s])
        offs = base + i, int(a["seg_zoff"][s]) + i, int(a["seg_doff"][s]) + i, int(a["seg_hoff"][s]) + i
        if e0 + 1 < start[s + 1] and base >= 0 and all(o % 2 == 0 for o in offs):
            out[e0] = out[e0 + 1] = True
    return out


_tapes = {}


def vector_tape(name):
    """Two constraints of the atom on its grid plus one more point (an even count: every offset is even, every unit a double2)."""
    if ("v", name) not in _tapes:
        u = np.concatenate([sr.grid(OP[name]), [0.75]])
        f = getattr(cp, name)
        a = cpu.lower(cp.Problem(cp.Minimize(0 * cp.sum(cpu._var(2))), [f(cpu._var(u.size)) <= 0, f(cpu._var(u.size)) <= 0]))
        assert list(a["seg_op"]) == [OP[name]] * 2
        _tapes[("v", name)] = (a, cpu.fill(a, [u, u]), cpu.multipliers(int(a["dims"][1])), 0.5, u)
    return _tapes[("v", name)]


# (segment sizes, gathered entries, size of the placeholder variable in front of the arguments).  A pair of units inside one
# contiguous segment has even z / dvals / hvals offsets whatever the segment's own offset (they equal the unit index): what
# sends it down the scalar path is an x offset of the other parity, which a placeholder of one entry gives every segment.
SMALL_TAPES = {"crossing": ((513,), 0, 2),              # one 512-unit workgroup of double2's and a last unit alone
               "scalar": ((1, 2, 3, 513), GATHER, 1)}   # odd offsets throughout, and an argument gathered with stride 2


def small_tape(name, kind):
    """Segments on the first points of the grid."""
    if (kind, name) not in _tapes:
        shapes, gather, pad = SMALL_TAPES[kind]
        u = vector_tape(name)[4]
        f = getattr(cp, name)
        cons = [f(cpu._var(n)) <= 0 for n in shapes + ((gather,) if gather else ())]
        a = cpu.lower(cp.Problem(cp.Minimize(0 * cp.sum(cpu._var(pad))), cons))
        assert list(a["seg_op"]) == [OP[name]] * len(cons) and list(a["seg_n"]) == [c.args[0].size for c in cons]
        assert all(int(b) >= 0 for b in a["seg_a0_base"])
        x = cpu.fill(a, [u[:int(n)] for n in a["seg_n"]])
        if gather:
            # the last segment reads every other entry of the longest one's argument (tests/test_flat_sweep_layouts.py: a gathered
            # argument is the front end's segment with its base set to -1 and its gidx entries rewritten)
            s, big = len(cons) - 1, int(np.argmax(a["seg_n"]))
            for key in ("seg_a0_base", "gidx"):
                a[key] = a[key].copy()
            o = int(a["seg_a0_off"][s])
            a["gidx"][o:o + gather] = int(a["seg_a0_base"][big]) + 2 * np.arange(gather)
            a["seg_a0_base"][s] = -1
        _tapes[(kind, name)] = (a, x, cpu.multipliers(int(a["dims"][1])), 0.5, u)
    return _tapes[(kind, name)]


def check_tape(dev, a, x, lam, sigma):
    exp = sr.expected_oracles(a, x, lam, sigma)
    for units in exp["units"]:
        assert not np.any(units.st == 1)
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
    """(value, d1, d2) per flat unit in tape order out of eval_g / eval_jac_g / eval_h (one-to-one maps, as in the CPU file)."""
    assert np.array_equal(a["seg_hoff"], a["seg_zoff"]) and np.array_equal(a["seg_doff"], a["seg_zoff"])
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])
    Gz = ar._csr(a, "G", (m, N + Z)).tocsc()[:, N:].tocsc()
    MJ, MH = ar._csr(a, "MJ", (nnzJ, nd)).tocsc(), ar._csr(a, "MH", (nnzH, nh)).tocsc()
    out = []
    for M, vec, scale in ((Gz, got["g"], None), (MJ, got["jac"], None), (MH, got["hess"], w)):
        assert np.all(np.diff(M.indptr) == 1) and np.all(np.abs(M.data) == 1.0)
        v = np.asarray(vec)[M.indices] / M.data
        out.append(v if scale is None else v / scale[:v.size])
    return out


# ---- 1. the rule: the hipcc build ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ATOMS)
def test_vector_path_against_mpmath(name, gpu_required):
    a, x, lam, sigma, u = vector_tape(name)
    assert unit_is_vector(a).all()
    dev = _device(a)
    try:
        check_tape(dev, a, x, lam, sigma)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", sorted(SMALL_TAPES))
@pytest.mark.parametrize("name", ATOMS)
def test_scalar_path_against_mpmath_and_equal_to_the_vector_path_bit_for_bit(name, kind, gpu_required):
    a, x, lam, sigma, u = small_tape(name, kind)
    vec = unit_is_vector(a)
    start = np.concatenate([[0], np.cumsum(a["seg_n"])])
    if kind == "crossing":
        assert vec[:512].all() and not vec[512]          # the 513th unit is alone in its workgroup
    else:               # n = 1, n = 2, n = 513 and the gathered one entirely on the scalar path (n = 3 too where no auxiliary variable
        for seg in (0, 1, 3, 4):            # shifts its argument: loggamma's lies two entries further than its outputs)
            assert not vec[start[seg]:start[seg + 1]].any(), seg
        assert name == "loggamma" or not vec.any()
    av, xv, lamv, sigmav, _ = vector_tape(name)
    ds, dv = _device(a), _device(av)
    try:
        s_out = per_unit(a, x, lam, sigma, check_tape(ds, a, x, lam, sigma))
        v_out = per_unit(av, xv, lamv, sigmav, {"g": dv.eval_g(xv), "jac": dv.eval_jac_g(xv), "hess": dv.eval_h(xv, lamv, sigmav)})
    finally:
        ds.close()
        dv.close()
    for k in range(3):
        for s in range(len(start) - 1):
            n = int(a["seg_n"][s])
            gathered = int(a["seg_a0_base"][s]) < 0
            sc, ve = s_out[k][start[s]:start[s + 1]], (v_out[k][0:2 * n:2] if gathered else v_out[k][:n])
            # (d2 came back as (w d2) / w with w = +-2^j: exact)
            assert np.array_equal(sc.view(np.int64), ve.view(np.int64)), (name, k, s)


@pytest.mark.parametrize("name", ATOMS)
def test_objective_callbacks_against_mpmath(name, gpu_required):
    """eval_f and eval_grad_f with the atom in the objective (the tape of the CPU file: objective and constraint segment)."""
    a, x, lam, sigma = cpu.tape(name)
    dev = _device(a)
    try:
        cpu.check_callbacks(dev, name)
    finally:
        dev.close()


def test_edges_and_past_the_grid(gpu_required):
    dev = _device(cpu.tape("edges")[0])
    try:
        cpu.check_callbacks(dev, "edges")
        cpu.assert_edge_classes(cpu.unit_outputs(dev))
    finally:
        dev.close()


def test_two_fresh_handles_and_two_sweeps_give_identical_bits(gpu_required):
    runs = []
    for _ in range(2):
        for name in ATOMS:
            a, x, lam, sigma, u = vector_tape(name)
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
    u = sr.grid(OP[name])
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
    for name in ATOMS:
        ta, u = _fused_case(name)
        dev = _capi.DeviceProblem(serialize(ta), None, device=0)
        try:
            f, g = dev.eval_fused(u.copy())
        finally:
            dev.close()
        out[name + "_f"], out[name + "_g"] = np.array([f]), g
    np.savez(out_path, **out)


def _check_fused(results):
    K = sr.measured_K()
    for name in ATOMS:
        ta, u = _fused_case(name)
        hi, lo, br, st = sr.special_reference(OP[name], u)
        assert not np.any(st[:2])
        val, d1 = ar.Units(u.size), ar.Units(u.size)
        for k, units in ((0, val), (1, d1)):
            units.hi[:], units.lo[:], units.tol[:] = hi[k], lo[k], K[OP[name]][k] * sr.EPS * br[k]
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
import test_special_atoms_gpu
test_special_atoms_gpu._fused_results(sys.argv[3])
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
@pytest.mark.parametrize("name", sorted(spb.SOLVES))
def test_solve_on_the_device(name, gpu_required):
    prob, var, xs, fs = spb.SOLVES[name]()
    prob.solve(nlp=True, **spb.SOLVE_OPTS[name])
    spb.assert_solution(name, prob, var, xs, fs)


def test_unconstrained_probit_takes_the_fused_path(gpu_required):
    prob, var, xs, fs = spb.latent_problem()
    prob.solve(nlp=True, algorithm="lbfgs")
    d = prob._nlp_cache["data"]
    assert prob._nlp_cache["sig"][0] == "direct" and d["fused"] and d["tape"].m == 0 and d["tape"].N == spb.LATENT_N
    spb.assert_solution("latent", prob, var, xs, fs)


# ---- 4. batch ------------------------------------------------------------------------------------------------------------------
def test_probit_batch_agrees_with_the_host_build(gpu_required):
    """256 instances of the probit template, labels as parameters: the status of every instance is the host build's, the
    objectives agree to 1e-8 relative; the launch is the wavefront solver's (ops 14 - 16 are flat unary ops: csrc/wave_plan.h
    refuses nothing here), through unary_slow and the out-of-line rule."""
    from dnlp_amd.batch import ParametricBatch, arrays_with_data
    from dnlp_amd.nlp_solver import HIPNLP
    from oracle.oracle_capi import OracleProblem
    tprob, params, x = spb.probit_template()
    pb = ParametricBatch(tprob, params)
    thetas = spb.probit_label_rows(256)
    try:
        res = pb.solve(thetas)
        launch = res.raw["launch"]
        assert launch["wave_form"] != 0 and launch["wave_refused"] == 0 and not launch["wave_wg"], launch
        mat = pb.data(thetas)
        for i in range(256):
            arr = arrays_with_data(pb.arrays0, mat[i])
            o = OracleProblem(serialize(arr))
            for k, v in HIPNLP.DEFAULT_OPTIONS.items():
                o.set_option(k, v)
            ref = o.solve(arr["x0"])
            assert res.status[i] == ref["status"], (i, res.status[i], ref["status"])
            assert abs(res.raw["obj_val"][i] - ref["obj_val"]) <= 1e-8 * max(1.0, abs(ref["obj_val"])), (i, res.raw["obj_val"][i], ref["obj_val"])
        xs, fs = spb.probit_answer()
        assert res.status[0] == 0 and abs(res.raw["obj_val"][0] - fs) <= spb.VALUE_TOL * max(1.0, abs(fs))
    finally:
        pb.close()
