"""The atom rules (csrc/atom_math.h and the OP_MUL / OP_REL_ENTR / OP_MATMUL / quad_over_lin branches beside its callers)
against mpmath at 80 digits, on grids that reach the edges of every domain (tests/atom_reference.py: closed forms, grids,
the bound K eps (|r| + |u r'|) and how K is measured).

CPU: the numpy statement (oracle/tape_eval.py; this run also establishes K) and the host build of the same header through
oracle.oracle_capi.OracleProblem.  GPU: the hipcc build through _capi.DeviceProblem (eval_g / eval_jac_g / eval_h / eval_f /
eval_grad_f), and the hiprtc build through eval_fused, in this process and in one child process that imported torch first
(the runtime compiler torch ships)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import atom_reference as ar
import dnlp_amd as cp
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.nlp_solver import build_nlp_data
from dnlp_amd.tape import serialize
from oracle.tape_eval import (OP_ATANH, OP_ENTR, OP_LOG, OP_LOGISTIC, OP_MATMUL, OP_MUL, OP_POWER, OP_QUAD_OVER_LIN,
                              OP_REL_ENTR, TapeEvaluator)

ATOM = {ar.NAMES[op]: op for op in ar.UNARY_OPS}
ATOM_BINARY = {"mul": OP_MUL, "rel_entr": OP_REL_ENTR}
UNARY_NAMES = sorted(ATOM)
TAPES = UNARY_NAMES + ["power", "mul", "rel_entr", "sums", "edges"]


def _multipliers(m):
    """+-2^k, k in -2..2, neighbours always different (so is i ^ 1): the Hessian entry is lam_i d2 up to an exact scaling."""
    i = np.arange(m)
    return np.where((i // 5) % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 5) - 2)


def _lower(prob, fused=False):
    smooth, _ = Dnlp2Smooth().apply(prob)
    if fused:
        from dnlp_amd.fused import build_fused_spec
        spec = build_fused_spec(prob)
        assert spec is not None
        data, _ = build_nlp_data(smooth, user_variables=prob.variables(), fused_spec=spec)
    else:
        data, _ = build_nlp_data(smooth)
    return data


def _var(n, value=0.5):
    v = cp.Variable(n)
    v.value = np.full(n, value)
    return v


def _args(a, s, which):
    off, ln = int(a["seg_%s_off" % which][s]), int(a["seg_%s_len" % which][s])
    return np.asarray(a["gidx"][off:off + ln], dtype=np.int64)


def _power_cases():
    """(p_der, p_fwd, bases) for the sixteen exponents and the one split pair."""
    cases = [(p, p, ar.power_grid(p)) for p in ar.POWER_EXPONENTS]
    pf, pd = ar.POWER_SPLIT
    return cases + [(pd, pf, ar.power_grid(pf))]


_tapes = {}


def _tape(name):
    """-> (tape arrays, x, multipliers, sigma).  Every atom argument is written straight into x at the indices the tape's own
    segments read (seg_a0_off / seg_a1_off into gidx): evaluation needs no feasible point."""
    if name in _tapes:
        return _tapes[name]
    fill = []                          # per segment in tape order: (argument 0 values, argument 1 values or None)
    if name in ATOM:
        op = ATOM[name]
        u = ar.grid(op)
        f = getattr(cp, name)
        prob = cp.Problem(cp.Minimize(cp.sum(f(_var(u.size)))), [f(_var(u.size)) <= 0])
        a = dict(_lower(prob)["tape_arrays"])
        assert list(a["seg_op"]) == [op, op]
        fill = [(u, None), (u, None)]
    elif name == "power":
        # the front-end follows the reference and refuses negative exponents; the rule itself takes any: every segment is
        # lowered as power(., 3) and gets its exponents written into seg_param (derivatives) / seg_param2 (value)
        cases = _power_cases()
        prob = cp.Problem(cp.Minimize(cp.sum(cp.power(_var(cases[0][2].size), 3)) + cp.sum(cp.power(_var(cases[5][2].size), 3))),
                          [cp.power(_var(c[2].size), 3) <= 0 for c in cases])
        a = dict(_lower(prob)["tape_arrays"])
        assert (a["seg_op"] == OP_POWER).all() and a["seg_op"].size == len(cases) + 2
        a["seg_param"], a["seg_param2"] = a["seg_param"].copy(), a["seg_param2"].copy()
        todo = [cases[0], cases[5]] + cases
        for s in range(a["seg_op"].size):
            k = next(i for i, c in enumerate(todo) if c[2].size == int(a["seg_n"][s]))
            pd, pf, u = todo.pop(k)
            a["seg_param"][s], a["seg_param2"][s] = pd, pf
            fill.append((u, None))
        assert not todo
    elif name in ("mul", "rel_entr"):
        u, v = ar.mul_grid() if name == "mul" else ar.rel_entr_grid()
        f = cp.multiply if name == "mul" else cp.rel_entr
        prob = cp.Problem(cp.Minimize(cp.sum(f(_var(u.size), _var(u.size)))), [f(_var(u.size), _var(u.size)) <= 0])
        a = dict(_lower(prob)["tape_arrays"])
        assert list(a["seg_op"]) == [ATOM_BINARY[name]] * 2
        fill = [(u, v), (u, v)]
    elif name == "sums":
        rng = np.random.default_rng(2300)
        cons = []
        for n in (1, 7, 65):
            cons.append(cp.quad_over_lin(_var(n), _var(1)) <= 0)
            fill.append((rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n), np.array([10.0 ** rng.uniform(-3, 3)])))
        for (mm, kk, pp) in ((2, 1, 3), (3, 7, 2), (2, 65, 2)):
            U, V = cp.Variable((mm, kk)), cp.Variable((kk, pp))
            U.value, V.value = np.ones((mm, kk)), np.ones((kk, pp))
            cons.append(U @ V == 0)
            fill.append((rng.standard_normal(mm * kk) * 10.0 ** rng.uniform(-3, 3, mm * kk),
                         rng.standard_normal(kk * pp) * 10.0 ** rng.uniform(-3, 3, kk * pp)))
        a = dict(_lower(cp.Problem(cp.Minimize(0 * cp.sum(_var(1))), cons))["tape_arrays"])
        assert list(a["seg_op"]) == [OP_QUAD_OVER_LIN] * 3 + [OP_MATMUL] * 3
    elif name == "edges":
        cons, ops = [], []
        for op, pts in sorted(ar.EDGE_POINTS.items()):
            cons.append(getattr(cp, ar.NAMES[op])(_var(len(pts))) <= 0)
            fill.append((np.array(pts), None))
            ops.append(op)
        for p, base in ar.POWER_EDGE_POINTS:
            cons.append(cp.power(_var(1), 3) <= 0)
            fill.append((np.array([base]), None))
            ops.append(OP_POWER)
        a = dict(_lower(cp.Problem(cp.Minimize(0 * cp.sum(_var(1))), cons))["tape_arrays"])
        assert list(a["seg_op"]) == ops
        a["seg_param"], a["seg_param2"] = a["seg_param"].copy(), a["seg_param2"].copy()
        k0 = len(ar.EDGE_POINTS)
        for k, (p, base) in enumerate(ar.POWER_EDGE_POINTS):
            a["seg_param"][k0 + k] = a["seg_param2"][k0 + k] = p
    else:
        raise KeyError(name)
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x = np.zeros(N)
    seen = np.zeros(N, dtype=bool)
    for s, (u, v) in enumerate(fill):
        for which, vals in (("a0", u), ("a1", v)):
            if vals is None:
                continue
            idx = _args(a, s, which)
            assert idx.size == vals.size and not seen[idx].any(), "segment %d: every atom argument must have variables of its own" % s
            x[idx] = vals
            seen[idx] = True
    _tapes[name] = (a, x, _multipliers(m), 0.5)
    return _tapes[name]


def _assert_left_out_share(a, x, lam, sigma):
    """At most 2 % of a tape's units (per output kind) may lie outside the normal range: decided by mpmath alone."""
    w = TapeEvaluator(a).weights(lam, sigma)
    for units, kind in zip(ar.reference_sweep(a, x, w), ("value", "d1", "d2")):
        share = float(np.mean(units.st == 1)) if units.st.size else 0.0
        assert share <= ar.LEFT_OUT_SHARE, "%s: %.1f %% of the points left out" % (kind, 100 * share)


class _Callbacks:
    """oracle/tape_eval.TapeEvaluator under the C API's method names."""

    def __init__(self, a):
        self.ev = TapeEvaluator(a)
        self.eval_f, self.eval_grad_f, self.eval_g = self.ev.objective, self.ev.gradient, self.ev.constraints
        self.eval_jac_g, self.eval_h = self.ev.jacobian, self.ev.hessian


def _all_checks(checks):
    """Runs every (expectation, thunk) and reports all that fail together, so that one callback's failure does not hide another's."""
    failed = []
    for entries, thunk in checks:
        try:
            entries.check(thunk())
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


def _check_callbacks(ev, name):
    a, x, lam, sigma = _tape(name)
    exp = ar.expected_oracles(a, x, lam, sigma)
    checks = [(exp["g"], lambda: ev.eval_g(x)), (exp["jac"], lambda: ev.eval_jac_g(x)), (exp["hess"], lambda: ev.eval_h(x, lam, sigma))]
    if name != "edges":
        _assert_left_out_share(a, x, lam, sigma)
        checks += [(exp["f"], lambda: [ev.eval_f(x)]), (exp["grad_f"], lambda: ev.eval_grad_f(x))]
    _all_checks(checks)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_numpy_statement_against_mpmath_establishes_K():
    """oracle/tape_eval.unary_rules on every grid: the IEEE class is right everywhere, at most 2 % of an op's points are left
    out, and the worst error is below 4 units of eps * bracket, so that K = 4 x worst, up to a power of two and at least 8,
    lands on 8 or 16 for every op and output (the table in tests/atom_reference.py)."""
    wrong = []
    for row, (op, pd, pf, worst, where, bad, share) in ar.measured_table().items():
        if bad != [[], [], []]:
            wrong.append("%s: wrong IEEE class (value, d1, d2) at u = %r" % (row, [b[:6] for b in bad]))
        if max(share) > ar.LEFT_OUT_SHARE:
            wrong.append("%s: shares %r of the points left out" % (row, share))
        if max(worst) > 4.0:
            wrong.append("%s: %r units of eps * bracket (value, d1, d2) at u = %r" % (row, worst, where))
    assert not wrong, "\n".join(wrong)
    assert all(k in (8, 16) for ks in ar.measured_K().values() for k in ks), ar.measured_K()


def test_logistic_derivatives_do_not_overflow_at_a_large_margin():
    """The reference's e / (1 + e) and e / (1 + e)^2 are NaN from u = 709.8 on and lose d2 from u ~ 355 on; the rule here
    departs from it on purpose (csrc/atom_math.h OP_LOGISTIC)."""
    u = np.array([360.0, 710.5, 800.0, 1e4, -360.0, -710.5, -800.0, -1e4])
    val, d1, d2 = ar.numpy_rules(OP_LOGISTIC, u, 0.0, 0.0)
    assert np.array_equal(d1[:4], np.ones(4)) and np.all(np.isfinite(d2)) and np.all(np.isfinite(d1)) and np.all(d1[4:] >= 0)
    assert abs(d2[0] - np.exp(-360.0)) <= 16 * ar.EPS * 361 * np.exp(-360.0)


@pytest.mark.parametrize("name", TAPES)
def test_numpy_tape_evaluator_against_mpmath(name):
    """The expectations themselves (tests/atom_reference.expected_oracles through the tape's maps) against the numpy tape
    evaluator: what the host and device builds are held to below is attainable by an independent implementation."""
    _check_callbacks(_Callbacks(_tape(name)[0]), name)


@pytest.mark.parametrize("name", TAPES)
def test_host_build_against_mpmath(name):
    """csrc/atom_math.h compiled by g++ (csrc/model.h over host loops): g, Jacobian, Hessian, f, grad f entry by entry."""
    from oracle.oracle_capi import OracleProblem
    _check_callbacks(OracleProblem(serialize(_tape(name)[0])), name)


def test_edge_expectations_are_the_stated_classes():
    """log(0) = -inf, entr(0) = 0 with d1 = +inf, log(-1) = NaN, atanh(+-1) = +-inf, power(0, -1) = inf."""
    a, x, lam, sigma = _tape("edges")
    z, dv, _ = ar.reference_sweep(a, x, TapeEvaluator(a).weights(lam, sigma))
    by = {}
    for j, who in enumerate(z.who):
        by[(who[1], who[2][0], float(a["seg_param"][who[0]]))] = (z.hi[j], dv.hi[j])
    assert by[(OP_LOG, 0.0, 0.0)][0] == -np.inf and np.isnan(by[(OP_LOG, -1.0, 0.0)][0])
    assert by[(OP_ENTR, 0.0, 0.0)] == (0.0, np.inf)
    assert by[(OP_ATANH, 1.0, 0.0)][0] == np.inf and by[(OP_ATANH, -1.0, 0.0)][0] == -np.inf
    assert by[(OP_POWER, 0.0, -1.0)][0] == np.inf
    assert (z.st >= 1).all()            # (exp(800) and its like: inside the domain, beyond the range: must not be NaN)


# ---- GPU: the hipcc build ------------------------------------------------------------------------------------------------------

def _device(a):
    from dnlp_amd import _capi
    return _capi.DeviceProblem(serialize(a), None, device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TAPES)
def test_device_build_against_mpmath(name, gpu_required):
    """The tape kernels (csrc/exec_hip.h sweep_flat_kernel and the reduction segments' kernels, device math library):
    eval_g, eval_jac_g, eval_h, eval_f, eval_grad_f entry by entry."""
    dev = _device(_tape(name)[0])
    try:
        _check_callbacks(dev, name)
    finally:
        dev.close()


def _ieee_class(v):
    v = np.asarray(v, float)
    return np.where(np.isnan(v), 2, np.where(np.isinf(v), np.sign(v), 0)).astype(int)


@pytest.mark.gpu
def test_device_and_host_build_agree_in_ieee_class_on_the_edges(gpu_required):
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = _tape("edges")
    dev, orc = _device(a), OracleProblem(serialize(a))
    try:
        for what in ("eval_g", "eval_jac_g"):
            assert np.array_equal(_ieee_class(getattr(dev, what)(x)), _ieee_class(getattr(orc, what)(x))), what
        assert np.array_equal(_ieee_class(dev.eval_h(x, lam, sigma)), _ieee_class(orc.eval_h(x, lam, sigma)))
    finally:
        dev.close()


# ---- GPU: the hiprtc builds (fused objective) ------------------------------------------------------------------------------

FUSED = UNARY_NAMES + ["power"]


def _fused_case(name):
    """-> (tape arrays with the fused program, xfree, [(op, p_der, p_fwd, offset into xfree, arguments)])."""
    from oracle.fused_eval import F_LOADV, F_UNARY
    if name in ATOM:
        u = ar.grid(ATOM[name])
        data = _lower(cp.Problem(cp.Minimize(cp.sum(getattr(cp, name)(_var(u.size)))), []), fused=True)
        ta = dict(data["tape_arrays"])
        assert data["fused"] and ta["free_idx"].size == u.size
        return ta, u.copy(), [(ATOM[name], 0.0, 0.0, 0, u)]
    cases = _power_cases()
    f = 0
    for c in cases:
        f = f + cp.sum(cp.power(_var(c[2].size), 3))
    data = _lower(cp.Problem(cp.Minimize(f), []), fused=True)
    ta = dict(data["tape_arrays"])
    assert data["fused"]
    ta["fz_p"], ta["fz_p2"] = ta["fz_p"].copy(), ta["fz_p2"].copy()
    xfree = np.zeros(ta["free_idx"].size)
    parts, todo = [], list(cases)
    for pidx in range(int(ta["fz_dims"][0])):
        s0, s1 = int(ta["fz_prog_start"][pidx]), int(ta["fz_prog_start"][pidx + 1])
        n = int(ta["fz_prog_nelem"][pidx])
        for k in range(s0, s1):
            if int(ta["fz_op"][k]) != F_UNARY:
                continue
            assert int(ta["fz_b"][k]) == OP_POWER
            src = int(ta["fz_a"][k]) + s0
            assert int(ta["fz_op"][src]) == F_LOADV and int(ta["fz_stride"][src]) == 1
            off = int(ta["fz_off"][src])
            pd, pf, u = todo.pop(next(i for i, c in enumerate(todo) if c[2].size == n))
            ta["fz_p"][k], ta["fz_p2"][k] = pd, pf
            xfree[off:off + n] = u
            parts.append((OP_POWER, pd, pf, off, u))
    assert not todo
    return ta, xfree, parts


def _fused_expectation(ta, parts, nfree):
    """f = c0 + sum of the values, grad = the first derivatives, as tests/atom_reference.Entries."""
    import scipy.sparse as sp
    K = ar.measured_K()
    val, d1 = ar.Units(nfree), ar.Units(nfree)
    for op, pd, pf, off, u in parts:
        hi, lo, br, st = ar.unary_reference(op, u, pd, pf)
        for k, units in ((0, val), (1, d1)):
            sl = slice(off, off + u.size)
            units.hi[sl], units.lo[sl], units.st[sl] = hi[k], lo[k], st[k]
            units.tol[sl] = K[op][k] * ar.EPS * br[k]
            for i in range(u.size):
                units.who[off + i] = (0, op, (float(u[i]),))
    for units in (val, d1):
        assert np.mean(units.st == 1) <= ar.LEFT_OUT_SHARE
    return (ar.Entries(np.asarray(ta["fz_c0"], float)[:1], None, None, sp.csr_matrix(np.ones((1, nfree))), val, "fused f"),
            ar.Entries(None, None, None, sp.identity(nfree, format="csr"), d1, "fused grad"))


def _fused_results(out_path):
    """Runs every fused case on device 0 and stores f and grad (the child process calls this after importing torch)."""
    from dnlp_amd import _capi
    out = {}
    for name in FUSED:
        ta, xfree, parts = _fused_case(name)
        dev = _capi.DeviceProblem(serialize(ta), None, device=0)
        try:
            f, g = dev.eval_fused(xfree)
        finally:
            dev.close()
        out[name + "_f"], out[name + "_g"] = np.array([f]), g
    np.savez(out_path, **out)


def _check_fused(results):
    for name in FUSED:
        ta, xfree, parts = _fused_case(name)
        ef, eg = _fused_expectation(ta, parts, xfree.size)
        eg.check(results[name + "_g"])
        ef.check(results[name + "_f"])


@pytest.mark.gpu
def test_fused_kernels_of_this_process_against_mpmath(gpu_required, tmp_path):
    """csrc/atom_math.h as text, compiled at run time by the hiprtc this process loads: value and gradient of sum(atom(v))
    per atom on the atom's whole grid."""
    path = str(tmp_path / "fused.npz")
    _fused_results(path)
    _check_fused(np.load(path))


_TORCH_FIRST_CHILD = r"""
import sys
import torch                                  # FIRST: the process then compiles with the hiprtc / comgr torch ships
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import os
os.environ["DNLP_KERNEL_CACHE"] = sys.argv[2]          # (a cache of its own: the kernels are compiled here, by this compiler)
import test_atom_rules
test_atom_rules._fused_results(sys.argv[3])
print("DONE", flush=True)
"""


@pytest.mark.gpu
def test_fused_kernels_of_a_process_that_imported_torch_first_against_mpmath(gpu_required, tmp_path):
    """The same in one fresh child process that imported torch first: its kernels come from the runtime compiler torch
    ships, with a device math library of its own, from an empty kernel cache."""
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
