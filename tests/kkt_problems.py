"""Cases of the KKT probe tests (test_kkt_probe_cpu.py for the host build, test_kkt_probe_gpu.py for the device): the smallest inputs that still select
each assembly / factorisation / solve path, written with the front end.

A case is a problem, the options that choose its path, a point strictly inside the bounds, random O(1) multipliers and the
diagonals of an interior-point step: Sx log-uniform in [1e-2, 1e2], D log-uniform in [1e-3, 1] on inequality rows and
0 (or the delta_c-like 1e-8 IPOPT uses) on equality rows.  `check_path(handle)` asserts — through kkt_info(),
kkt_tail_nodes(), the plan's level statistics and, after the probe, kkt_mode() — that the handle takes the path the case
is meant for, so a refactor that moves a threshold fails loudly instead of silently testing something else.

The thresholds restated below are those of csrc/sparse_ldl.h (branches of the one-workgroup kernels, L = 256 lanes) and
csrc/exec_hip.h (sparse_grid_path, and the per-level kernel choice of sparse_factor / sparse_solve).
"""
import ctypes
import functools

import numpy as np

# csrc/exec_hip.h
LANES = 256                      # kBlock: lanes of the one-workgroup sparse_factor_kernel / sparse_solve_kernel
GRID_MIN_BLOCKS = 8192           # kSparseGridMin
GRID_MIN_TRIPLES = 200000        # kSparseGridMinTriples
WG_ITEMS = 128                   # >= 128 triples per destination / rows per target on a level: the _wg kernels
BWD_WAVE_STRUCT = 16             # average struct of a level >= 16: sp_bwd_kernel (a wavefront per block), else sp_bwd_thread
FUSE_STRUCT = 8                  # struct rows of a level <= 8 x blocks: sp_pivot_scale_kernel (with DNLP_LEVEL_FUSION)


def lower(prob):
    import dnlp_amd as cp
    from dnlp_amd.dnlp2smooth import Dnlp2Smooth
    from dnlp_amd.nlp_solver import build_nlp_data
    from dnlp_amd.tape import serialize
    if isinstance(prob.objective, cp.Maximize):
        prob = cp.Problem(cp.Minimize(-prob.objective.expr), prob.constraints)
    smooth, _ = Dnlp2Smooth().apply(prob)
    data, _ = build_nlp_data(smooth)
    return data, serialize(data["tape_arrays"])


def _plan_detail(host, what, width):
    from oracle.oracle_capi import api
    fn = api().lib.orc_kkt_plan_detail
    fn.restype = ctypes.c_longlong
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_longlong]
    cap = width * (host.n + host.m + 1)
    out = (ctypes.c_int64 * cap)()
    n = fn(host.ptr, what, out, cap)
    assert n > 0, n
    return np.array(out[:width * n], dtype=np.int64).reshape(n, width)


def plan_levels(host):
    """Per level of the host handle's sparse plan: dict of blocks, struct rows, update groups (destinations), triples,
    forward targets, the rows they gather, the longest gather, and the panel columns of a dense tail
    (orc_wave_plan_levels, orc_kkt_plan_detail)."""
    from oracle.oracle_capi import api
    fn = api().lib.orc_wave_plan_levels
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    cap = 8 * 8192
    out = (ctypes.c_int32 * cap)()
    n = fn(host.ptr, out, cap)
    assert 0 < n <= cap // 8
    a = np.array(out[:8 * n]).reshape(n, 8)
    d = _plan_detail(host, 0, 4)
    assert d.shape[0] == n
    return [dict(blocks=int(r[0]), struct_rows=int(r[2]), max_struct=int(r[3]), groups=int(r[4]), triples=int(r[5]),
                 max_group=int(r[6]), fwd_targets=int(e[0]), fwd_rows=int(e[1]), max_fwd=int(e[2]), panel_cols=int(e[3]))
            for r, e in zip(a, d)]


def static_pairs(host):
    """(variable, constraint row) of every static 2x2 pivot block of the host handle's sparse plan."""
    b = _plan_detail(host, 1, 2)
    b = b[b[:, 1] >= 0]
    assert np.all(b[:, 0] < host.n) and np.all(b[:, 1] >= host.n)
    return b[:, 0], b[:, 1] - host.n


def pair_entries(K, var, row):
    """(a, c, e) of the reference matrix on the 2x2 blocks [[a, c], [c, e]] of the (variable, row) pairs."""
    A = K.csc()
    a = np.asarray(A[var, var]).ravel()
    c = np.asarray(A[var, K.N + row]).ravel()
    e = np.asarray(A[K.N + row, K.N + row]).ravel()
    return a, c, e


# ---- the problems ------------------------------------------------------------------------------------------------------

def arrow(cp, leaves=300, shared=3, hubs=4, kinds="emq", seed=0):
    """`leaves` variables, each coupled through a smooth objective term (exp of a sum, a product, quad_over_lin) to the
    same `shared` variables (`kinds`: which of the three, in turn), `hubs` variables coupled to every shared one and to each other (they make the struct of the
    first shared block long enough for the all-lanes backward branch), and four sparse equalities between leaves."""
    rng = np.random.default_rng(seed)
    y = cp.Variable(leaves, bounds=[-1, 2])
    s = cp.Variable(shared, bounds=[0.5, 3])
    v = cp.Variable(max(hubs, 1), bounds=[-1, 2])
    y.value = rng.uniform(-0.5, 1.5, leaves)
    s.value = rng.uniform(1.0, 2.0, shared)
    v.value = rng.uniform(0.0, 1.0, max(hubs, 1))
    w = rng.uniform(0.5, 1.5, leaves)
    obj = cp.sum_squares(y) + cp.sum_squares(v)
    for k in range(shared):
        kind = kinds[k % len(kinds)]
        if kind == "e":
            obj = obj + cp.sum(cp.exp(0.3 * y + 0.2 * s[k]))
        elif kind == "m":
            obj = obj + cp.sum(cp.multiply(cp.multiply(w, y), s[k]))
        else:
            obj = obj + cp.quad_over_lin(y, s[k])
        if hubs:
            obj = obj + cp.quad_over_lin(v, s[k])
    for a in range(hubs - 1):
        obj = obj + v[a] * v[a + 1]
    cons = [y[2 * i] + y[2 * i + 1] == 0.5 for i in range(4)]
    return cp.Problem(cp.Minimize(obj), cons)


def overlap(cp):
    """Atoms whose Hessians land on the SAME entries: exp(x), square(x) and quad_over_lin(x, s) all write (x_i, x_i); exp(x + y)
    and multiply(x, y) go through auxiliary variables of the smooth form.  The assemblies add Hessian entries with +=
    inside a parallel map and store Jacobian entries with =: right only if positions are unique, which the lowering
    has to guarantee by merging the atoms' contributions before the assembly sees them (the map MH of the tape)."""
    x = cp.Variable(6, bounds=[-1, 1])
    y = cp.Variable(6, bounds=[-1, 1])
    s = cp.Variable(1, bounds=[0.5, 2])
    x.value = np.linspace(-0.5, 0.6, 6)
    y.value = np.linspace(0.4, -0.3, 6)
    s.value = np.ones(1)
    obj = (cp.sum(cp.exp(x + y)) + cp.sum(cp.multiply(x, y)) + cp.sum(cp.square(x)) + cp.sum(cp.exp(x))
           + cp.quad_over_lin(x, s[0]) + cp.sum_squares(y))
    return cp.Problem(cp.Minimize(obj), [cp.sum(cp.multiply(x, y)) <= 1.0, x[0] + y[0] == 0.1])


CONCAVE_PAIRS = 12


def bilinear(cp, n=60, seed=1):
    """An indefinite Hessian block: products of neighbouring variables, no regularisation — and CONCAVE_PAIRS variables u
    of strongly negative curvature (-400 + Sx <= -300), each in one equality row u_i + 0.5 v_i = 0.1 with a convex v_i.
    The static pairing takes u_i (the larger constant coefficient) as that row's partner, so with D = 1e-2 on equality
    rows the 2x2 pivot [[a, 1], [1, -D]] has a < 0 and det = |a| D - 1 >= 2 > 0: two negative eigenvalues from one
    block, the branch of sp_pivot that adds 2.  (If v_i, a 1x1 pivot d > 0 coupled to nothing else, is eliminated before
    the block, the block's e becomes -D - 0.25 / d: more negative, det larger, same branch.)  check_pairs() asserts
    these numbers on the reference matrix."""
    rng = np.random.default_rng(seed)
    x = cp.Variable(n, bounds=[-2, 2])
    u = cp.Variable(CONCAVE_PAIRS, bounds=[-2, 2])
    v = cp.Variable(CONCAVE_PAIRS, bounds=[-2, 2])
    x.value = rng.uniform(-1, 1, n)
    u.value = rng.uniform(-1, 1, CONCAVE_PAIRS)
    v.value = rng.uniform(-1, 1, CONCAVE_PAIRS)
    c = rng.uniform(0.5, 2.0, n - 1)
    obj = (cp.sum(cp.multiply(c, cp.multiply(x[:-1], x[1:]))) + 0.05 * cp.sum_squares(x)
           - 200.0 * cp.sum_squares(u) + cp.sum_squares(v))
    cons = [x[3 * i] + x[3 * i + 1] - x[3 * i + 2] == 0.2 for i in range(n // 6)]
    cons.append(u + 0.5 * v == 0.1)
    return cp.Problem(cp.Minimize(obj), cons)


def orphan(cp):
    """A variable that appears nowhere: with Sx = 0 and delta_w = 0 its pivot is exactly zero."""
    x = cp.Variable(5, bounds=[-1, 1])
    z = cp.Variable(1)
    x.value = np.linspace(-0.4, 0.4, 5)
    z.value = np.zeros(1)
    return cp.Problem(cp.Minimize(cp.sum(cp.exp(x)) + cp.sum_squares(x) + 0.0 * z[0]), [x[0] + x[1] == 0.3])


def _zoo(name):
    def make(cp):
        from problem_zoo import GOLDEN_ZOO
        return GOLDEN_ZOO[name](cp)
    return make


def _chain(n):
    def make(cp):
        from problem_zoo import rosenbrock_chain
        return rosenbrock_chain(cp, n)
    return make


def _dense_eq_qp(cp):
    from problem_zoo import dense_eq_qp
    return dense_eq_qp(cp, 260, 40)


def _nmf(images):
    def make(cp):
        from paper_examples import nb_nmf
        return nb_nmf(cp, images)
    return make


# ---- path checks -------------------------------------------------------------------------------------------------------

def _one_workgroup(info, tail):
    assert info["sparse"] and tail == 0
    assert info["pivot_blocks"] < GRID_MIN_BLOCKS and info["update_triples"] < GRID_MIN_TRIPLES


def _check_arrow_small(host, info, tail):
    """Arrow with 300 leaves, 3 shared variables and 4 hubs (sparse_ldl.h, L = 256 lanes): the level of the 296 free leaf
    blocks has 22 destinations (22 x 8 = 176 <= L) fed by 1 792 triples (>= 16 x 22): all-lanes update; a one-block level
    near the root gathers its single target from 607 rows (1 x 8 <= L, 607 > 2 x 1): all-lanes forward; the first blocks
    after the leaves stand alone on their levels with structs of 4 to 6 (1 x 4 < L, 4 > 3 x 1^2): all-lanes backward.
    The numbers are asserted below from the plan itself."""
    _one_workgroup(info, tail)
    lev = plan_levels(host)
    assert any(v["groups"] > 0 and v["groups"] * 8 <= LANES and v["triples"] >= 16 * v["groups"] for v in lev), lev
    assert any(v["fwd_targets"] > 0 and v["fwd_targets"] * 8 <= LANES and v["fwd_rows"] > 2 * v["fwd_targets"] for v in lev[1:]), lev
    assert any(v["blocks"] * 4 < LANES and v["struct_rows"] > 3 * v["blocks"] ** 2 for v in lev), lev
    # ... and the one-lane-per-item forms next to them
    assert any(v["groups"] * 8 > LANES for v in lev) and any(v["blocks"] * 4 >= LANES for v in lev)


def _check_small_sparse(host, info, tail):
    _one_workgroup(info, tail)
    # most level phases have fewer items than lanes
    assert sum(v["blocks"] < LANES for v in plan_levels(host)) >= 1


def _check_chain_small(host, info, tail):
    _one_workgroup(info, tail)
    assert info["levels"] >= 8 and info["pairs_2x2"] == host.m        # every equality row in a static 2x2 block


def _grid(info, tail):
    assert info["sparse"] and tail == 0 and info["pivot_blocks"] >= GRID_MIN_BLOCKS


def _check_chain_grid(host, info, tail):
    """sp_update_gather_kernel, sp_fwd_gather_kernel, sp_bwd_thread_kernel and the fused sp_pivot_scale_kernel: every
    level has short groups, short gathers and short structs."""
    _grid(info, tail)
    assert info["pivot_blocks"] < GRID_MIN_BLOCKS + 16                # the smallest chain that takes this path
    lev = plan_levels(host)
    assert all(v["triples"] < WG_ITEMS * max(v["groups"], 1) for v in lev)
    assert all(v["fwd_rows"] < WG_ITEMS * max(v["fwd_targets"], 1) for v in lev) and any(v["fwd_targets"] > 0 for v in lev)
    assert all(v["struct_rows"] < BWD_WAVE_STRUCT * v["blocks"] for v in lev)
    assert any(v["struct_rows"] <= FUSE_STRUCT * v["blocks"] and v["struct_rows"] > 0 for v in lev)


def _check_arrow_grid(host, info, tail):
    """sp_update_gather_wg_kernel (>= 128 triples per destination on the leaves' level), sp_fwd_gather_wg_kernel (>= 128
    rows per target), sp_bwd_kernel (a level whose structs average >= 16), and the unfused sp_pivot_kernel + sp_scale_kernel
    (struct rows > 8 x blocks)."""
    _grid(info, tail)
    lev = plan_levels(host)
    assert any(v["groups"] > 0 and v["triples"] >= WG_ITEMS * v["groups"] for v in lev), lev[:8]
    assert any(v["fwd_targets"] > 0 and v["fwd_rows"] >= WG_ITEMS * v["fwd_targets"] for v in lev[1:]), lev[:8]
    assert any(v["struct_rows"] >= BWD_WAVE_STRUCT * v["blocks"] and v["struct_rows"] > 0 for v in lev), lev[:8]
    assert any(v["struct_rows"] > FUSE_STRUCT * v["blocks"] for v in lev), lev[:8]


def _check_tail(host, info, tail):
    """A dense tail, and at least one level before it with panel columns: sp_panel_gather_kernel and the MFMA tail
    product run (exec_hip.h sparse_factor: h_pg_cols[lev] > 0)."""
    assert info["sparse"] and tail > 0
    assert any(v["panel_cols"] > 0 for v in plan_levels(host))


def _check_tail_off(host, info, tail):
    assert tail == 0


def _check_dense(host, info, tail):
    assert not info["sparse"] and tail == 0


# ---- checks of a case's inputs on the reference matrix (Case.check_inputs) ----------------------------------------------

ROTATE_BELOW = 0.6403882032022076        # csrc/kkt_dense.h: a pair is rotated when |w| < this x |coupling|


def _check_two_negative_pairs(host, refd):
    """sparse_ldl.h sp_pivot: a 2x2 block with det > 0 and a < 0 adds 2 to nneg.  At least CONCAVE_PAIRS static pairs
    of the reference matrix are such blocks, and the reference inertia has that many negative eigenvalues more than one
    per constraint row (every row is in a pair; a pair with det < 0 gives exactly one)."""
    var, row = static_pairs(host_handle(CASES_BY_NAME["bilinear-sparse"]))
    assert row.size == host.m
    a, c, e = pair_entries(refd["K"], var, row)
    two = (a < 0.0) & (a * e - c * c > 0.0)
    assert two.sum() >= CONCAVE_PAIRS and np.all(a[two] * e[two] >= 3.0 * c[two] ** 2), (a[two], c[two], e[two])
    assert np.sum(a * e - c * c < 0.0) == row.size - two.sum()
    assert refd["inertia"][0] >= host.m + two.sum() >= host.m + 2, refd["inertia"]
    assert refd["inputs"]["delta_w"] == 0.0 and host.n + host.m <= 400


def _check_pairs_of_both_kinds(host, refd):
    """kkt_dense.h rotates a matched (variable, equality row) pair when |H_jj + Sx_j + delta_w| < 0.64 |J_ij| and leaves
    it as it stands otherwise: the inputs put a good number of this case's pairs on either side."""
    var, row = static_pairs(host)
    a, c, _ = pair_entries(refd["K"], var, row)
    rotated = np.abs(a) < ROTATE_BELOW * np.abs(c)
    assert var.size >= 100 and rotated.sum() >= 20 and (~rotated).sum() >= 20, (var.size, int(rotated.sum()))


# ---- the cases ---------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, make, options, mode, check_path, *, host=True, fixed=(), eq_D=0.0, delta_w=0.0,
                 definite=False, sx_zero=(), nzero=0, grid=False, seed=0, share=None, check_inputs=None):
        self.name, self.make, self.options, self.mode, self.check_path = name, make, dict(options), mode, check_path
        self.host = host                 # False: too long for the non-GPU suite on the host build
        self.share = share               # the case with the same problem and inputs (its reference is shared)
        self.check_inputs = check_inputs # (host handle, reference) -> asserts what the inputs are chosen for
        self.fixed = fixed               # user picks by index into the lowered variables
        self.eq_D, self.delta_w, self.definite = eq_D, delta_w, definite
        self.sx_zero, self.nzero, self.grid, self.seed = sx_zero, nzero, grid, seed

    def __repr__(self):
        return self.name


SPARSE = {"linear_solver": "sparse"}
DENSE = {"linear_solver": "dense"}

CASES = [
    # one-workgroup sparse kernels
    Case("hs071-sparse", _zoo("hs071"), SPARSE, "sparse", _check_small_sparse),
    Case("localization-sparse", _zoo("localization"), SPARSE, "sparse", _check_small_sparse),
    Case("chain200-sparse", _chain(200), SPARSE, "sparse", _check_chain_small, definite=True, eq_D=1e-8),
    Case("arrow-sparse", arrow, SPARSE, "sparse", _check_arrow_small, definite=True, eq_D=1e-8),
    Case("arrow-fixed-sparse", arrow, SPARSE, "sparse", _check_arrow_small, fixed="arrow", definite=True, eq_D=1e-8),
    Case("overlap-sparse", overlap, SPARSE, "sparse", _check_small_sparse),
    Case("bilinear-sparse", bilinear, SPARSE, "sparse", _check_small_sparse, seed=3, eq_D=1e-2,
         check_inputs=_check_two_negative_pairs),
    Case("orphan-sparse", orphan, SPARSE, "sparse", _check_small_sparse, sx_zero="orphan", nzero=1),
    # grid-wide level kernels
    Case("chain-grid", _chain(2049), SPARSE, "sparse", _check_chain_grid, definite=True, eq_D=1e-8, grid=True),
    Case("arrow-grid", functools.partial(arrow, leaves=8200, shared=20, hubs=0, kinds="q"),
         {"linear_solver": "sparse", "sparse_dense_tail": "no"}, "sparse", _check_arrow_grid,
         definite=True, eq_D=1e-8, grid=True),
    # dense tail + panels, and the same operators through the level chain
    Case("phase-retrieval-tail", _zoo("nb_phase_retrieval"), {}, "sparse", _check_tail, definite=True, eq_D=1e-8),
    Case("phase-retrieval-chain", _zoo("nb_phase_retrieval"), {"linear_solver": "sparse", "sparse_dense_tail": "no"},
         "sparse", _check_tail_off, definite=True, eq_D=1e-8, share="phase-retrieval-tail"),
    Case("nmf-tail", _nmf(8), {}, "sparse", _check_tail, definite=True, eq_D=1e-8),
    Case("nmf-chain", _nmf(8), {"linear_solver": "sparse", "sparse_dense_tail": "no"}, "sparse", _check_tail_off,
         definite=True, eq_D=1e-8, share="nmf-tail"),
    # dense paths
    Case("hs071-dense", _zoo("hs071"), DENSE, "bunch-kaufman", _check_dense),
    Case("localization-dense", _zoo("localization"), DENSE, "bunch-kaufman", _check_dense),
    Case("overlap-dense", overlap, DENSE, "bunch-kaufman", _check_dense),
    Case("bilinear-dense", bilinear, DENSE, "bunch-kaufman", _check_dense, seed=3, eq_D=1e-2,
         check_inputs=_check_two_negative_pairs),
    Case("sphere60-dense", _zoo("sphere60"), {}, "bunch-kaufman", _check_dense),
    Case("sphere60-fixed-dense", _zoo("sphere60"), {}, "bunch-kaufman", _check_dense, fixed="tenth"),
    Case("dense-eq-qp-pivoted", _dense_eq_qp, {}, "bunch-kaufman", _check_dense),
    Case("dense-eq-qp-unpivoted", _dense_eq_qp, {"kkt_pivot_max_n": 64}, "unpivoted", _check_dense, eq_D=1e-2),
    Case("dense-eq-qp-fixed", _dense_eq_qp, {}, "bunch-kaufman", _check_dense, fixed="tenth"),
    # (paired mode: with Sx over four decades and O(1) couplings the matched pairs are of both kinds, rotated and not:
    #  _check_pairs_of_both_kinds)
    Case("sparse-recovery-paired", _zoo("nb_sparse_recovery"), {"linear_solver": "dense", "kkt_paired_min_n": 384},
         "paired", _check_dense, definite=True, eq_D=1e-8, check_inputs=_check_pairs_of_both_kinds),
]
CASES_BY_NAME = {c.name: c for c in CASES}


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


@functools.lru_cache(maxsize=None)
def lowered(name):
    import dnlp_amd as cp
    case = CASES_BY_NAME[name]
    return lowered(case.share) if case.share else lower(case.make(cp))


def inputs(case, host):
    """x strictly inside the bounds (the start point moved a little and kept 0.05 min(span, 1) off every finite bound), lambda,
    Sx, D, fixmask, delta_w and two right-hand sides; for `definite` cases delta_w is what Gershgorin's circles of
    H + diag(Sx) need to be strictly on the positive side (computed from the HOST library's Hessian)."""
    data, _ = lowered(case.name)
    rng = np.random.default_rng(1000 + case.seed)
    N, m = host.n, host.m
    lb, ub = np.asarray(data["lb"], float), np.asarray(data["ub"], float)
    cl, cu = np.asarray(data["cl"], float), np.asarray(data["cu"], float)
    x = np.asarray(data["x0"], float) + 0.01 * rng.standard_normal(N)
    span = np.where(np.isfinite(ub - lb), ub - lb, 1.0)
    x = np.minimum(np.maximum(x, lb + 0.05 * np.minimum(span, 1.0)), ub - 0.05 * np.minimum(span, 1.0))
    lam = rng.standard_normal(m)
    Sx = _loguniform(rng, 1e-2, 1e2, N)
    eq = cl == cu
    D = np.where(eq, case.eq_D, _loguniform(rng, 1e-3, 1.0, m)) if m else np.zeros(0)
    fixmask = None
    if case.fixed:
        fixmask = np.zeros(N)
        fixmask[rng.choice(N, max(1, N // 10), replace=False)] = 1.0
        if case.fixed == "arrow":
            # ... including a shared variable and one that appears in an equality (found by their Jacobian / Hessian degree)
            jr, jc = host.jac_structure()
            hr, hc = host.hess_structure()
            deg = np.bincount(np.concatenate([hr, hc, jc]), minlength=N)
            fixmask[int(np.argmax(deg))] = 1.0
            fixmask[int(jc[0])] = 1.0
    if case.sx_zero:
        hr, hc = host.hess_structure()
        jc = host.jac_structure()[1] if m else np.zeros(0, np.int32)
        used = np.bincount(np.concatenate([hr, hc, jc]).astype(np.int64), minlength=N)
        lonely = np.flatnonzero(used == 0)
        assert lonely.size == 1, lonely
        Sx[lonely] = 0.0
    delta_w = case.delta_w
    if case.definite:
        hr, hc = host.hess_structure()
        hv = host.eval_h(x, lam, 1.0)
        diag = np.zeros(N)
        offs = np.zeros(N)
        on = hr == hc
        np.add.at(diag, hr[on], hv[on])
        np.add.at(offs, hr[~on], np.abs(hv[~on]))
        np.add.at(offs, hc[~on], np.abs(hv[~on]))
        delta_w = float(max(0.0, np.max(offs - diag - Sx)) * 1.05 + 1e-2)
    rhs = rng.standard_normal((2, N + m))
    return dict(x=x, lam=lam, Sx=Sx, D=D, fixmask=fixmask, delta_w=delta_w, rhs=rhs)


def apply_options(handle, case):
    for k, v in case.options.items():
        handle.set_option(k, v)


def host_handle(case):
    from oracle.oracle_capi import OracleProblem
    h = OracleProblem(lowered(case.name)[1])
    apply_options(h, case)
    return h


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per case, computed once and shared (read-only): inputs, the reference matrix, its refined solutions with their
    backward errors, the reference inertia and the host build's probe with its figures."""
    import kkt_reference as ref
    case = CASES_BY_NAME[name]
    if case.share:
        return reference(case.share)
    host = host_handle(case)
    inp = inputs(case, host)
    K = ref.build_kkt(host, inp["x"], inp["lam"], 1.0, inp["Sx"], inp["D"], inp["fixmask"], inp["delta_w"])
    out = dict(inputs=inp, K=K, knorm=K.norm_inf())
    out["inertia"] = ref.inertia(K, quasi_definite=case.definite)
    if case.nzero == 0:
        sols = [ref.solve_refined(K, r) for r in inp["rhs"]]
        out["z_ref"] = [s[0] for s in sols]
        out["eta_ref"] = max(s[1] for s in sols)
    return out


@functools.lru_cache(maxsize=None)
def host_figures(name):
    """The host build's probe of the case (its own options, a fresh handle) and its (eta, fe): what a device run of the
    case is measured against.  Also the plan's level numbers, for n_row."""
    case = CASES_BY_NAME[name]
    h = host_handle(case)
    info = h.kkt_info()
    lev = plan_levels(h) if info["sparse"] else []
    res = probe(h, reference(name)["inputs"])
    eta, fe = figures(reference(name), res) if case.nzero == 0 else (None, None)
    return dict(res=res, eta=eta, fe=fe, info=info, levels=lev, order=h.n + h.m)


def probe(handle, inp):
    return handle.kkt_probe(inp["x"], inp["lam"], 1.0, inp["Sx"], inp["D"], inp["fixmask"], inp["delta_w"], inp["rhs"])


def figures(refd, res):
    """(eta, fe) of a probe's solutions: the largest over the right-hand sides."""
    import kkt_reference as ref
    K, rhs = refd["K"], refd["inputs"]["rhs"]
    eta = max(ref.backward_error(K, z, r, refd["knorm"]) for z, r in zip(res["sol"], rhs))
    fe = max(ref.forward_error(z, zr) for z, zr in zip(res["sol"], refd["z_ref"]))
    return eta, fe
