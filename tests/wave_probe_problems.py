"""TEST INFRASTRUCTURE — cases of the wavefront batch solver's KKT probe (include/dnlp_hip.h dnlp_batch_kkt_probe;
dnlp_amd/csrc/wave_ipm.h WaveIpm::probe): templates of batch_problems.py at sizes where a case asserts its own path from the
plan (`check`: the WaveHdr fields through orc_wave_hdr, the level statistics of orc_wave_plan_levels), the points, right-hand
sides and residual vectors every instance of a template is probed at, the reference of kkt_reference.py per instance, and
the host-lane figures a device run is measured against.  Everything is seeded; everything expensive is computed once per
process and shared.  Only tests/ may import this.

Points (the same for every instance of a template; the instances differ in their data rows):
  interior    Sx = s0 + 0.1 / (x - l)^2 + 0.1 / (u - x)^2 (a barrier state z = 0.1 / (x - l)), D in [0.5, 2], small multipliers.
              For the two large templates (order > kkt_reference.EIG_MAX_ORDER) s0 is the largest absolute row sum
              of the Hessian over the instances, doubled, plus one: H + Sx is strictly diagonally dominant, so the matrix is
              quasi-definite BY CONSTRUCTION and its inertia is (N, m, 0) with nothing to factorise (kkt_reference.inertia).
  indefinite  large multipliers of the sign that makes the Hessian of the Lagrangian concave, Sx of 1e-2: the reference matrix
              has MORE negative eigenvalues than constraint rows (asserted), so the inertia count is tested on something other
              than (N, m, 0).  Small templates only (there is no reference inertia above EIG_MAX_ORDER).
  fixed       the interior point with every sixth variable fixed in the data row (lb == ub == x): the fixm branches of assembly;
              delta_w = 2^-6 here and only here.
  singular    inertia only: the interior point with delta_w = 0, D = 0 on the equality rows and on ONE inequality row that is
              a 1x1 pivot block of the first level (`singular_row`): nothing updates that diagonal before it is pivoted, so the
              static pivot -D is exactly zero in every build (nzero > 0).  Only nneg, nzero and the ok flag are compared, with the
              host lane's.  The circle packing templates have such rows.  What does NOT give a zero pivot, tried on every
              template: D = 0 on the equality rows alone (the plan pairs every equality row with a variable into a 2x2 block
              whose determinant -c^2 is not zero; every 1x1 row block is an inequality row: nzero = 0 everywhere), a first-level
              1x1 VARIABLE block with Sx = 0 (none exists that the data does not fix), and a first-level 2x2 block with a zero
              diagonal and a coupling made exactly zero by equating two centre coordinates (none of the first-level pairs has
              such an entry).  Localization, path planning and power flow have no first-level 1x1 row block: no such point.
"""
import ctypes as C
import functools
import types

import numpy as np

import batch_problems as bp
import kkt_reference as ref
from dnlp_amd.batch import BATCH_DATA_KEYS, ParametricBatch, arrays_with_data
from dnlp_amd.tape import serialize
from oracle.oracle_capi import OracleProblem
from wave_oracle import HostBatch

LD = np.longdouble
UNIT = 2.0 ** -53
N_INST = 8
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_i32p = C.POINTER(C.c_int32)

HDR_FIELDS = (
    "total N m Z nd nh nnzJ nnzH nunits u_op u_a0 u_a1 u_z u_d0 u_d1 u_h u_p mm_idx keep_gen G_ptr G_idx Mg_ptr Mg_idx MJ_ptr MJ_idx "
    "Mw_ptr Mw_idx MH_ptr MH_idx jac_rows jac_cols hess_rows hess_cols jac_rowptr jr_ptr jr_ent jr_src jr_heavy jr_nheavy jc_ptr jc_ent "
    "jc_src jc_heavy jc_nheavy hs_ptr hs_ent hs_src hs_heavy hs_nheavy sp_nblk sp_nvals sp_nlev sp_ngrp sp_nfwd sp_ntrip sp_rows bnode soff "
    "loff doff lev_off sblk sidx lev_f fnode foff fa fu0 fu1 lev_g gdst goff tau tav hpos jpos dpos lev_r lev_t lev_fe keep_pad tail_L tail_T "
    "t_node t_d t_l t_fq t_fp t_nf l_c0 l_c l_b l_Jc l_G l_Mg l_Mw l_MJ l_MH l_fp l_fp2 l_x0 l_lb l_ub l_cl l_cu l_total state_doubles "
    "scr_doubles").split()
LDS_BYTES = 160 * 1024


# ---- the path checks: each fails when the template no longer selects the path the case is named for ------------------------
def _levels_before_tail(t):
    return t.levels[:t.hdr["tail_L"]]


def _all_lanes_levels(t):
    """Levels that take the interpreted text's all-lanes group sum (wave_ipm.h ldl_factor_impl: ngr * 8 <= L && ntr >= 16 * ngr, L = 64)."""
    return [k for k, lv in enumerate(_levels_before_tail(t)) if lv["groups"] > 0 and lv["groups"] * 8 <= 64 and lv["triples"] >= 16 * lv["groups"]]


def _check_localization(anchors, all_lanes):
    def check(t):
        """No dense tail; the two position variables meet every range row: the generated text's wide forms (the forward gathers
        of the last two levels run over 2 x anchors rows and more, through the DPP tree).  With 10 anchors (the default) no level
        has the 16 triples per group of the interpreted text's all-lanes group sum — 3 groups of 10; with 16 anchors one has."""
        assert t.hdr["tail_T"] == 0 and t.hdr["tail_L"] == t.hdr["sp_nlev"]
        assert max(lv["max_gather"] for lv in t.levels) >= 2 * anchors and max(lv["max_group"] for lv in t.levels) >= anchors
        assert bool(_all_lanes_levels(t)) == all_lanes, t.levels
    return check


def _check_tail(lo, hi, width):
    def check(t):
        T = t.hdr["tail_T"]
        assert lo <= T <= hi, T
        assert (12 if T <= 12 else 24 if T <= 24 else 32) == width
        assert t.hdr["tail_L"] + T == t.hdr["sp_nlev"]
        assert t.hdr["t_nf"] > 0                      # forward gathers reach from the levels before the tail into it
        chain = 0
        for lv in reversed(t.levels):
            if lv["blocks"] != 1 or lv["two"]:
                break
            chain += 1
        assert chain == T, (chain, T)                  # the whole chain is the tail: nothing truncated
    return check


def _check_truncated_tail(t):
    """A chain of one-block levels LONGER than 32: the tail is its last 32 levels (wave_plan.h), the one-block levels in
    front of it run as ordinary levels and forward gathers reach from them into the tail."""
    assert t.hdr["tail_T"] == 32 and t.hdr["tail_L"] + 32 == t.hdr["sp_nlev"]
    chain = 0
    for lv in reversed(t.levels):
        if lv["blocks"] != 1 or lv["two"]:
            break
        chain += 1
    assert chain > 32, chain
    before = t.levels[t.hdr["tail_L"] - (chain - 32):t.hdr["tail_L"]]
    assert before and all(lv["blocks"] == 1 and lv["rows"] >= 32 for lv in before)      # (each meets every tail row)
    assert t.hdr["t_nf"] > 0
    assert t.hdr["state_doubles"] * 8 > LDS_BYTES       # its state no longer fits LDS: the global-state form or the workgroup kernel


def _check_path_planning(t):
    """State beyond LDS (the workgroup-per-instance kernel, or the global-state form); the elimination ends in a long chain of
    levels of exactly TWO 1x1 blocks (the way points), then a short one-block chain that the library's kernels take as tail."""
    assert t.hdr["state_doubles"] * 8 > LDS_BYTES and t.n > ref.EIG_MAX_ORDER
    assert sum(1 for lv in t.levels if lv["blocks"] == 2 and lv["two"] == 0) >= 40, [lv["blocks"] for lv in t.levels]
    assert 3 <= t.hdr["tail_T"] <= 12
    assert max(lv["max_gather"] for lv in t.levels) >= 100


def _check_power_flow(t):
    """State beyond LDS; a chain of one-block levels whose block is 2x2 with 40 struct rows and more (the buses' voltage pairs),
    forward gathers of 100 rows and more, variables fixed in the data rows themselves (lb == ub)."""
    assert t.hdr["state_doubles"] * 8 > LDS_BYTES and t.n > ref.EIG_MAX_ORDER
    assert sum(1 for lv in t.levels if lv["blocks"] == 1 and lv["two"] == 1 and lv["max_struct"] >= 40) >= 3, [(lv["two"], lv["max_struct"]) for lv in t.levels]
    assert 3 <= t.hdr["tail_T"] <= 12
    assert max(lv["max_gather"] for lv in t.levels) >= 100
    assert data_fixed(t, t.mat).any()


TEMPLATES = {
    "localization": dict(make=bp.template_localization, opts={}, check=_check_localization(10, False)),
    "localization16": dict(make=lambda: bp.template_localization(16), opts={}, check=_check_localization(16, True)),
    "circle_packing4": dict(make=lambda: bp.template_circle_packing(4), opts={}, check=_check_tail(9, 9, 12)),
    "circle_packing10": dict(make=lambda: bp.template_circle_packing(10), opts={}, check=_check_tail(21, 21, 24)),
    # (from 24 chain levels on the handle's own plan has a dense tail matrix for the host-driven loop; a batch launch analyses
    #  again without it — capi.hip batch_runner — which is what sparse_dense_tail=no gives the host library's handle)
    "circle_packing12": dict(make=lambda: bp.template_circle_packing(12), opts={"sparse_dense_tail": "no"}, check=_check_tail(25, 32, 32)),
    "circle_packing17": dict(make=lambda: bp.template_circle_packing(17), opts={"sparse_dense_tail": "no"}, check=_check_truncated_tail),
    "path_planning": dict(make=bp.template_path_planning, opts={}, check=_check_path_planning),
    "power_flow": dict(make=bp.template_power_flow, opts={}, check=_check_power_flow),
}
LARGE = ["path_planning", "power_flow"]                            # state beyond LDS by far: the workgroup-per-instance kernel
BIG = ["circle_packing17"] + LARGE                                 # order above kkt_reference.EIG_MAX_ORDER: no eigenvalues
SMALL = [n for n in TEMPLATES if n not in BIG]
TAILED = ["circle_packing4", "circle_packing10", "circle_packing12", "circle_packing17"]


def _lib(hb):
    lib = hb.lib
    if not getattr(lib, "_wave_probe_bound", False):
        lib.orc_wave_hdr.restype = C.c_int
        lib.orc_wave_hdr.argtypes = [C.c_void_p, C.c_int, _i32p, C.c_int]
        lib.orc_wave_plan_levels.restype = C.c_int
        lib.orc_wave_plan_levels.argtypes = [C.c_void_p, _i32p, C.c_int]
        lib.orc_kkt_plan_detail.restype = C.c_longlong
        lib.orc_kkt_plan_detail.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_longlong]
        lib.orc_wave_probe.restype = C.c_int
        lib.orc_wave_probe.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, C.c_int] + [_dp] * 4 + [C.c_double, C.c_int] + [_dp] * 5 + [_ip] * 3
        lib._wave_probe_bound = True
    return lib


def wave_hdr(hb, no_tail=False):
    """The WaveHdr of the template's plan block as a dict (oracle_lib.cpp orc_wave_hdr)."""
    out = np.zeros(len(HDR_FIELDS) + 8, np.int32)
    n = _lib(hb).orc_wave_hdr(hb.handle.ptr, 1 if no_tail else 0, out.ctypes.data_as(_i32p), out.size)
    if n < 0:
        raise RuntimeError("orc_wave_hdr: %s" % hb.lib.orc_last_error().decode())
    assert n == len(HDR_FIELDS), (n, len(HDR_FIELDS))
    return dict(zip(HDR_FIELDS, out[:n].tolist()))


def wave_levels(hb):
    out = np.zeros(8 * 4096, np.int32)
    L = _lib(hb).orc_wave_plan_levels(hb.handle.ptr, out.ctypes.data_as(_i32p), out.size)
    assert 0 < L <= 4096
    rows = out[:8 * L].reshape(L, 8)
    keys = ("blocks", "two", "rows", "max_struct", "groups", "triples", "max_group")
    return [dict(zip(keys, r[:7].tolist()), forward=int(r[7]) // 1000, max_gather=int(r[7]) % 1000) for r in rows]


def plan_blocks(hb):
    """Pivot blocks in elimination order: (nb, 2) nodes, the second -1 for a 1x1 block."""
    cap = 2 * 8192
    out = np.zeros(cap, np.int64)
    nb = _lib(hb).orc_kkt_plan_detail(hb.handle.ptr, 1, out.ctypes.data_as(C.POINTER(C.c_int64)), cap)
    assert nb > 0
    return out[:2 * nb].reshape(nb, 2)


def _offsets(arrays0):
    off, o = {}, 0
    for k in BATCH_DATA_KEYS:
        off[k] = (o, arrays0[k].size)
        o += arrays0[k].size
    return off


@functools.lru_cache(maxsize=None)
def template(name):
    spec = TEMPLATES[name]
    prob, params, sample, _ = spec["make"]()
    pb = ParametricBatch(prob, params)
    hb = HostBatch(pb, spec["opts"])
    t = types.SimpleNamespace(name=name, pb=pb, hb=hb, opts=dict(spec["opts"]), N=hb.N, m=hb.m, n=hb.N + hb.m, check=spec["check"])
    t.thetas = np.stack([sample(i) for i in range(N_INST)])
    t.mat = np.ascontiguousarray(pb.data(t.thetas))
    assert len({r.tobytes() for r in t.mat}) == N_INST          # eight different data rows
    t.off = _offsets(pb.arrays0)
    t.hdr = wave_hdr(hb)
    t.levels = wave_levels(hb)
    t.blocks = plan_blocks(hb)
    return t


def _seg(t, mat, key):
    o, n = t.off[key]
    return mat[:, o:o + n]


def data_fixed(t, mat):
    """(rows, N) bool: the variables a data row fixes (lb == ub, as WaveIpm::probe and begin() read it)."""
    return _seg(t, mat, "lb") == _seg(t, mat, "ub")


def n_row_plan(t):
    """The longest sum into one entry: the longest update group or forward gather of the plan, and T for the tail (the longest
    forward gather sets it on every template here: 21, 33, 17, 41, 49, 69, 101, 126)."""
    return max([t.hdr["tail_T"], 1] + [max(lv["max_group"], lv["max_gather"]) for lv in t.levels])


# ---- points -------------------------------------------------------------------------------------------------------------
def _inside(x, lb, ub, margin=0.3):
    x = x.copy()
    for j in range(x.size):
        lo, hi = lb[j] > -1e19, ub[j] < 1e19
        if lo and hi and ub[j] - lb[j] < 2.5 * margin:      # (a variable fixed in the data sits on its value)
            x[j] = 0.5 * (lb[j] + ub[j])
        else:
            if lo:
                x[j] = max(x[j], lb[j] + margin)
            if hi:
                x[j] = min(x[j], ub[j] - margin)
    return x


def _barrier(x, lb, ub):
    s = np.zeros_like(x)
    lo, hi = (lb > -1e19) & (lb < ub), (ub < 1e19) & (lb < ub)
    s[lo] += 0.1 / (x[lo] - lb[lo]) ** 2
    s[hi] += 0.1 / (ub[hi] - x[hi]) ** 2
    return s


def singular_row(t):
    """An INEQUALITY row that is a 1x1 pivot block of the first level (see the module docstring), or None."""
    first = t.levels[0]["blocks"]
    eq = _seg(t, t.mat, "cl")[0] == _seg(t, t.mat, "cu")[0]
    for u0, u1 in t.blocks[:first]:
        if u1 < 0 and u0 >= t.N and not eq[u0 - t.N]:
            return int(u0 - t.N)
    return None


def _host_of(t, row):
    return OracleProblem(serialize(arrays_with_data(t.pb.arrays0, row)))


@functools.lru_cache(maxsize=None)
def points(name):
    """{point name: namespace(x, lam, Sx, D (one vector each: the same for every instance), dw, mat (the data rows), fixmask,
    inertia_only, quasi)}"""
    t = template(name)
    rng = np.random.default_rng(20261018 + sorted(TEMPLATES).index(name))
    lb, ub = _seg(t, t.mat, "lb").max(axis=0), _seg(t, t.mat, "ub").min(axis=0)
    x0 = _seg(t, t.mat, "x0")[0]
    x = _inside(x0 + 0.05 * rng.standard_normal(t.N), lb, ub)
    lam_small = 0.1 * rng.standard_normal(t.m)
    D = rng.uniform(0.5, 2.0, t.m)
    big = t.n > ref.EIG_MAX_ORDER
    s0 = 1.0
    if big:
        worst = 0.0
        for row in t.mat:
            h = _host_of(t, row)
            hr, hc = (a.astype(np.int64) for a in h.hess_structure())
            hv = np.abs(h.eval_h(x, lam_small, 1.0))
            off = hr != hc
            rows = np.zeros(t.N)
            np.add.at(rows, hr, hv)                       # (its own diagonal entry counts too: it may be negative)
            np.add.at(rows, hc[off], hv[off])
            worst = max(worst, float(rows.max()))
        s0 = 2.0 * worst + 1.0
    out = {}
    mk = lambda **kw: types.SimpleNamespace(**dict(dict(x=x, lam=lam_small, Sx=s0 + _barrier(x, lb, ub), D=D, dw=0.0, mat=t.mat, fixmask=None,
                                                        inertia_only=False, quasi=big), **kw))
    out["interior"] = mk()
    if not big:
        # (multipliers of one sign make the Hessian of the Lagrangian concave; which one is found on instance 0 — the tests
        #  assert nneg > m on the reference matrix of EVERY instance)
        mag, sx = 1.0 + np.abs(rng.standard_normal(t.m)), 1e-2 * (1.0 + rng.uniform(0.0, 1.0, t.N))
        for sign in (1.0, -1.0):
            K = ref.build_kkt(_host_of(t, t.mat[0]), x, sign * mag, 1.0, sx, D)
            if ref.inertia(K)[0] > t.m:
                break
        out["indefinite"] = mk(lam=sign * mag, Sx=sx)
    # fixed variables: every sixth, from the second on, pinned at the point in every data row
    fm = np.zeros(t.N)
    fm[1::6] = 1.0
    mat = t.mat.copy()
    for key in ("lb", "ub", "x0"):
        _seg(t, mat, key)[:, fm != 0.0] = x[fm != 0.0]
    out["fixed"] = mk(mat=mat, fixmask=fm, dw=0.015625)          # (the one point with delta_w != 0: assembly and the residual pass add it)
    r = singular_row(t)
    if r is not None:
        eq = (_seg(t, t.mat, "cl")[0] == _seg(t, t.mat, "cu")[0])
        d = np.where(eq, 0.0, D)
        d[r] = 0.0
        out["singular"] = mk(D=d, inertia_only=True)
    return out


POINTS_OF = {name: (["interior", "fixed"] if name in BIG else ["interior", "indefinite", "fixed"]) for name in TEMPLATES}
CASES = [(name, pt) for name in TEMPLATES for pt in POINTS_OF[name]]
SINGULAR = ["circle_packing4", "circle_packing10", "circle_packing12", "circle_packing17"]      # (asserted: test_wave_probe_cpu.py)


# ---- the reference per instance -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, pt, i):
    """Instance i of the template at the point: the reference matrix, three right-hand sides (random; K times a known vector,
    in longdouble, rounded; a unit vector on the last pivot node — the last tail row where there is a tail), the residual
    vectors (entries of mixed magnitude 1e-3 .. 1e3, two of them), the refined reference solutions and figures."""
    t, p = template(name), points(name)[pt]
    host = _host_of(t, p.mat[i])
    fixmask = data_fixed(t, p.mat[i:i + 1])[0].astype(np.float64)
    assert p.fixmask is None or np.all(fixmask[p.fixmask != 0.0] == 1.0)
    K = ref.build_kkt(host, p.x, p.lam, 1.0, p.Sx, p.D, fixmask, p.dw)
    rng = np.random.default_rng([sorted(TEMPLATES).index(name), sorted(points(name)).index(pt), i])
    known = rng.standard_normal(t.n)
    unit = np.zeros(t.n)
    unit[int(t.blocks[-1][0])] = 1.0
    rhs = np.stack([rng.standard_normal(t.n), K.matvec_ld(known).astype(np.float64), unit])
    v = np.sign(rng.standard_normal((2, t.n))) * 10.0 ** rng.uniform(-3.0, 3.0, (2, t.n))
    if fixmask.any():
        # (the residual pass multiplies by the WHOLE Hessian and Jacobian and takes the identity only in the fixed rows — as
        #  ipm_core.h kkt_residual does: it is rhs - K v on the vectors a solve hands it, whose fixed components are zero
        #  because the right-hand side's are)
        v[:, :t.N][:, fixmask != 0.0] = 0.0
    out = types.SimpleNamespace(K=K, rhs=rhs, v=v, known=known)
    if p.inertia_only:
        return out
    M = K.csc()
    out.n_row = int(np.diff(M.indptr).max())
    out.absK = abs(M)
    out.z, out.eta_ref = [], []
    for r in rhs:
        z, eta = ref.solve_refined(K, r)
        out.z.append(z)
        out.eta_ref.append(eta)
    out.res = [rhs[q].astype(LD) - K.matvec_ld(v[q]) for q in range(2)]
    out.res_scale = [np.abs(rhs[q]) + np.asarray(out.absK @ np.abs(v[q])).ravel() for q in range(2)]
    return out


@functools.lru_cache(maxsize=None)
def inertia(name, pt, i):
    t, p = template(name), points(name)[pt]
    return ref.inertia(reference(name, pt, i).K, quasi_definite=p.quasi)


def inputs(name, pt, count):
    """The arrays of one probe call over the first `count` instances."""
    t, p = template(name), points(name)[pt]
    tile = lambda a: np.ascontiguousarray(np.tile(a, (count, 1)))
    R = np.stack([reference(name, pt, i).rhs for i in range(count)])
    V = np.stack([reference(name, pt, i).v for i in range(count)])
    return dict(data=np.ascontiguousarray(p.mat[:count]), x=tile(p.x), lagrange=tile(p.lam), Sx=tile(p.Sx), D=tile(p.D), delta_w=p.dw, rhs=R, v=V)


def host_probe(hb, inp, which):
    """oracle_lib.cpp orc_wave_probe: which = 0 wave_ipm.h on one host lane, 1 the generic text with the template's plan."""
    B, nrhs, n = inp["rhs"].shape
    sol, sol2, res = np.full((B, nrhs, n), np.nan), np.full((B, 2, n), np.nan), np.full((B, 3, n), np.nan)
    nneg, nzero, ok = (np.zeros(B, np.int32) for _ in range(3))
    keep = [np.ascontiguousarray(inp[k], dtype=np.float64) for k in ("data", "x", "lagrange", "Sx", "D", "rhs", "v")]
    rc = _lib(hb).orc_wave_probe(hb.handle.ptr, B, keep[0].ctypes.data_as(_dp), keep[0].shape[1], which, keep[1].ctypes.data_as(_dp),
                                 keep[2].ctypes.data_as(_dp), keep[3].ctypes.data_as(_dp), keep[4].ctypes.data_as(_dp), float(inp["delta_w"]), nrhs,
                                 keep[5].ctypes.data_as(_dp), keep[6].ctypes.data_as(_dp), sol.ctypes.data_as(_dp),
                                 sol2.ctypes.data_as(_dp), res.ctypes.data_as(_dp), nneg.ctypes.data_as(_ip), nzero.ctypes.data_as(_ip),
                                 ok.ctypes.data_as(_ip))
    if rc != 0:
        raise RuntimeError("orc_wave_probe: %d %s" % (rc, hb.lib.orc_last_error().decode()))
    return {"sol": sol, "sol2": sol2, "res": res, "nneg": nneg, "nzero": nzero, "ok": ok.astype(bool)}


@functools.lru_cache(maxsize=None)
def host_lane(name, pt, count):
    """The host lane's probe of the first `count` instances (shared: the CPU tests judge it, the device tests measure against it)."""
    return host_probe(template(name).hb, inputs(name, pt, count), 0)


def figures(name, pt, i, res):
    """(eta, fe): the largest backward and forward error over the three right-hand sides of instance i."""
    r = reference(name, pt, i)
    knorm = r.K.norm_inf()
    eta = max(ref.backward_error(r.K, res["sol"][i, q], r.rhs[q], knorm) for q in range(3))
    fe = max(ref.forward_error(res["sol"][i, q], r.z[q]) for q in range(3))
    return eta, fe


def residual_excess(name, pt, i, res):
    """The kernel's residuals rhs - K v of instance i against the longdouble ones: the largest componentwise error in units of
    (n_row + 2) 2^-53 (|r| + |K| |v|) — the forward bound of a dot product of n_row terms and the two additions behind it —
    over the single pass and both systems of the two-system pass (at most 1 where the bound holds)."""
    r = reference(name, pt, i)
    worst = 0.0
    for slot, q in ((0, 0), (1, 0), (2, 1)):
        err = np.abs(res["res"][i, slot].astype(LD) - r.res[q]).astype(np.float64)
        bound = (r.n_row + 2) * UNIT * r.res_scale[q]
        assert np.all(bound > 0.0)
        worst = max(worst, float(np.max(err / bound)))
    return worst
