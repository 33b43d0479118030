"""log_normcdf, normcdf and loggamma without a GPU (flat tape ops 14, 15, 16; tests/special_reference.py: closed forms in mpmath,
grids, the bound and how K is measured; tests/special_problems.py: the solves and their answers).

The rule: the numpy / scipy statement establishes K; the host build of csrc/atom_math.h (oracle.oracle_capi.OracleProblem) is
held against mpmath on the full grids through eval_g, eval_jac_g, eval_h (non-unit multipliers), eval_f and eval_grad_f; the
edge and IEEE points are checked by class.  Front end: curvature, sign, monotonicity, rule tags, canonical form, opcodes and
segment counts.  Solves on the host build: probit regression, the Gamma shape MLE, a Dirichlet MLE and a chance-constrained LP,
each to 1e-6 on the value and 1e-4 on the point against an answer computed in mpmath."""
import numpy as np
import pytest
import scipy.sparse as sp

import atom_reference as ar
import dnlp_amd as cp
import special_problems as spb
import special_reference as sr
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.nlp_solver import build_nlp_data
from dnlp_amd.tape import serialize

ATOMS = ["log_normcdf", "normcdf", "loggamma"]
OP = {sr.NAMES[op]: op for op in sr.OPS}
NAN, INF = np.nan, np.inf
EDGE_POINTS = {
    "log_normcdf": sr.FAR_LEFT + sr.FAR_RIGHT + [-INF, NAN],
    "normcdf": [-40.0, 40.0, -INF, INF, NAN],
    "loggamma": [0.0, -0.5, -1.0, -INF, INF, NAN],
}


def multipliers(m):
    """+-2^k, k in -2..2, neighbours always different: the Hessian entry is lam_i d2 up to an exact scaling."""
    i = np.arange(m)
    return np.where((i // 5) % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 5) - 2)


def _var(n):
    v = cp.Variable(n)
    v.value = np.full(n, 0.5)
    return v


def lower(prob):
    smooth, _ = Dnlp2Smooth().apply(prob)
    return dict(build_nlp_data(smooth)[0]["tape_arrays"])


def fill(a, per_segment):
    """x with every segment's arguments written at the indices the segment reads (evaluation needs no feasible point)."""
    x = np.zeros(int(a["dims"][0]))
    seen = np.zeros(x.size, dtype=bool)
    for s, u in enumerate(per_segment):
        idx = sr._arg(a, s)
        assert idx.size == u.size and not seen[idx].any()
        x[idx], seen[idx] = u, True
    return x


_tapes = {}


def tape(name):
    """-> (tape arrays, x, multipliers, sigma): the atom once in the objective and once in a constraint, on its whole grid."""
    if name not in _tapes:
        if name == "edges":
            a = lower(cp.Problem(cp.Minimize(0 * cp.sum(_var(1))), [getattr(cp, n)(_var(len(EDGE_POINTS[n]))) <= 0 for n in ATOMS]))
            assert list(a["seg_op"]) == [OP[n] for n in ATOMS]
            x = fill(a, [np.array(EDGE_POINTS[n]) for n in ATOMS])
        else:
            u = sr.grid(OP[name])
            f = getattr(cp, name)
            a = lower(cp.Problem(cp.Minimize(cp.sum(f(_var(u.size)))), [f(_var(u.size)) <= 0]))
            assert list(a["seg_op"]) == [OP[name]] * 2
            x = fill(a, [u, u])
        _tapes[name] = (a, x, multipliers(int(a["dims"][1])), 0.5)
    return _tapes[name]


def check_callbacks(ev, name):
    """g, Jacobian, Hessian, f and grad f of `ev` entry by entry; every failing callback is reported."""
    a, x, lam, sigma = tape(name)
    exp = sr.expected_oracles(a, x, lam, sigma)
    checks = [(exp["g"], lambda: ev.eval_g(x)), (exp["jac"], lambda: ev.eval_jac_g(x)), (exp["hess"], lambda: ev.eval_h(x, lam, sigma))]
    if name == "edges":
        for entries, _ in checks:       # the linear rows t - v == 0 of loggamma's auxiliary variable at t = +-inf / NaN: class only
            entries.st[(entries.st == 0) & ~np.isfinite(entries.hi)] = 2
    else:
        for units in exp["units"]:
            assert not np.any(units.st == 1), "a grid point was left out of the magnitude comparison"
        checks += [(exp["f"], lambda: [ev.eval_f(x)]), (exp["grad_f"], lambda: ev.eval_grad_f(x))]
    failed = []
    for entries, thunk in checks:
        try:
            entries.check(thunk())
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


def unit_outputs(ev, name="edges"):
    """{atom: (value, d1, d2) arrays per point} read back out of eval_g / eval_jac_g / eval_h of a tape whose constraint rows are
    one atom entry each (the maps are then one-to-one, which is asserted)."""
    a, x, lam, sigma = tape(name)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])
    with np.errstate(all="ignore"):
        g, jac, hess = np.asarray(ev.eval_g(x)), np.asarray(ev.eval_jac_g(x)), np.asarray(ev.eval_h(x, lam, sigma))
    Gz = ar._csr(a, "G", (m, N + Z)).tocsc()[:, N:].tocsc()
    MJ, MH = ar._csr(a, "MJ", (nnzJ, nd)).tocsc(), ar._csr(a, "MH", (nnzH, nh)).tocsc()

    def only(M, c):
        rows = M.indices[M.indptr[c]:M.indptr[c + 1]]
        assert rows.size == 1 and abs(M.data[M.indptr[c]]) == 1.0
        return int(rows[0]), M.data[M.indptr[c]]

    def read(vec, M, c):
        r, coef = only(M, c)
        return vec[r] / coef

    out = {}
    for s in range(nseg):
        n, zo, do, ho = (int(a[k][s]) for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff"))
        val = np.array([read(g, Gz, zo + i) for i in range(n)])
        d1 = np.array([read(jac, MJ, do + i) for i in range(n)])
        d2 = np.array([read(hess, MH, ho + i) / w[zo + i] for i in range(n)])
        out[sr.NAMES[int(a["seg_op"][s])]] = (val, d1, d2)
    return out


def assert_edge_classes(out):
    """The IEEE table of DESIGN.md section 2 on the outputs of `unit_outputs`."""
    val, d1, d2 = (dict(zip(EDGE_POINTS["log_normcdf"], v)) for v in out["log_normcdf"])
    for u in sr.FAR_LEFT:
        assert np.isfinite(val[u]) and np.isfinite(d1[u]) and -1.0 <= d2[u] <= 0.0, (u, val[u], d1[u], d2[u])
    for u in sr.FAR_RIGHT:
        assert val[u] == 0.0 and d1[u] == 0.0 and d2[u] == 0.0, (u, val[u], d1[u], d2[u])
    assert val[-INF] == -INF and not np.isnan(d2[-INF])
    val, d1, d2 = out["normcdf"]
    assert np.array_equal(val[:4], [0.0, 1.0, 0.0, 1.0]) and not d1[:4].any() and not d2[:4].any()
    val, d1, d2 = out["loggamma"]
    assert (val[0], d1[0], d2[0]) == (INF, -INF, INF)
    assert np.isnan(val[1:4]).all() and np.isnan(d1[1:4]).all() and np.isnan(d2[1:4]).all()
    assert (val[4], d1[4], d2[4]) == (INF, INF, 0.0)
    for n in ATOMS:                                                     # NaN in, NaN out
        assert all(np.isnan(v[-1]) for v in out[n]), n


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_establishes_K():
    """The numpy / scipy statement on every grid: the right IEEE class everywhere, no point left out, within 4 units of the
    table in tests/special_reference.py; K = 4 x worst, up to a power of two and at least 8."""
    wrong = []
    for op, (worst, where, bad, left) in sr.measured_table().items():
        if bad != [[], [], []]:
            wrong.append("%s: wrong IEEE class at u = %r" % (sr.NAMES[op], [b[:6] for b in bad]))
        if any(left):
            wrong.append("%s: %r points left out" % (sr.NAMES[op], left))
    assert not wrong, "\n".join(wrong)
    K = sr.measured_K()
    sr.print_table()
    assert all(8 <= k <= 128 and k & (k - 1) == 0 for ks in K.values() for k in ks), K


@pytest.mark.parametrize("name", ATOMS)
def test_host_build_against_mpmath(name):
    """csrc/atom_math.h compiled by g++: g, Jacobian, Hessian, f, grad f entry by entry on the full grid."""
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(tape(name)[0])), name)


def test_host_build_on_the_edges_and_past_the_grid():
    from oracle.oracle_capi import OracleProblem
    ev = OracleProblem(serialize(tape("edges")[0]))
    check_callbacks(ev, "edges")                    # the far left points against mpmath like any other, the rest by class
    assert_edge_classes(unit_outputs(ev))


def test_far_left_second_derivative_is_the_series_not_the_cancellation():
    """At u = -1e8 the stated expression -lambda (u + lambda) has no correct digit (u + lambda is below an ulp of u) and at -1e3
    it has lost 20 bits; the rule's series there is good to the last bits, against the TIGHT bracket |r| + |u r'|."""
    from oracle.oracle_capi import OracleProblem
    d2 = dict(zip(EDGE_POINTS["log_normcdf"], unit_outputs(OracleProblem(serialize(tape("edges")[0])))["log_normcdf"][2]))
    for u in (-1e3, -1e8):
        r, rp, _ = sr.special_mp(sr.OP_LOG_NORMCDF, u)
        assert abs(d2[u] - float(r[2])) <= 8 * sr.EPS * float(abs(r[2]) + abs(u * rp[2])), (u, d2[u], float(r[2]))


# ---- 2. front end ----------------------------------------------------------------------------------------------------------------
def test_curvature_sign_monotonicity_and_rule_tags():
    x = cp.Variable(4)
    a, b, c = cp.log_normcdf(x), cp.normcdf(x), cp.loggamma(x)
    assert a.is_concave() and not a.is_convex() and a.is_incr(0) and not a.is_decr(0) and a.is_nonpos() and not a.is_nonneg()
    assert not b.is_convex() and not b.is_concave() and b.is_incr(0) and not b.is_decr(0) and b.is_nonneg() and not b.is_nonpos()
    assert c.is_convex() and not c.is_concave() and not c.is_incr(0) and not c.is_decr(0) and not c.is_nonneg() and not c.is_nonpos()
    for e, like in ((a, cp.log(x)), (b, cp.sin(x)), (c, cp.exp(x))):
        assert (e.is_atom_esr(), e.is_atom_hsr(), e.is_smooth()) == (like.is_atom_esr(), like.is_atom_hsr(), like.is_smooth()) == (True, True, True)
        assert e.shape == (4,)
    # composition: increasing atoms take an ESR / HSR argument on the matching side, loggamma (not monotone) only a smooth one
    assert cp.log_normcdf(-cp.abs(x)).is_hsr() and not cp.log_normcdf(-cp.abs(x)).is_esr()
    assert cp.normcdf(cp.abs(x)).is_esr() and not cp.normcdf(cp.abs(x)).is_hsr()
    assert not cp.loggamma(cp.abs(x)).is_esr() and not cp.loggamma(cp.abs(x)).is_hsr()


def test_is_dnlp_accepts_and_refuses():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, 3))
    x, y = cp.Variable(3), cp.Variable(6)
    assert cp.Problem(cp.Minimize(-cp.sum(cp.log_normcdf(A @ x)))).is_dnlp()
    # Minimize(sum(log_normcdf(x))) minimises a concave function.  Disciplined NLP, unlike DCP, accepts that: the atom is
    # tagged like log (ESR and HSR), a smooth atom of a variable is smooth, and Minimize asks for ESR only.  The verdict is
    # log's own; what IS refused is a nonsmooth argument on the side the atom's monotonicity does not carry
    assert cp.Problem(cp.Minimize(cp.sum(cp.log_normcdf(x)))).is_dnlp() == cp.Problem(cp.Minimize(cp.sum(cp.log(x)))).is_dnlp() == True  # noqa: E712
    assert not cp.Problem(cp.Minimize(cp.sum(cp.log_normcdf(-cp.abs(x))))).is_dnlp()
    assert cp.Problem(cp.Maximize(cp.sum(cp.log_normcdf(-cp.abs(x))))).is_dnlp()
    assert cp.Problem(cp.Minimize(x[0]), [cp.normcdf(A @ x) >= 0.9]).is_dnlp()
    assert cp.Problem(cp.Minimize(x[0]), [cp.normcdf(cp.abs(y)) <= 0.9]).is_dnlp()
    assert not cp.Problem(cp.Minimize(x[0]), [cp.normcdf(cp.abs(y)) >= 0.6]).is_dnlp()
    assert cp.Problem(cp.Minimize(cp.sum(cp.loggamma(A @ x)))).is_dnlp()
    assert not cp.Problem(cp.Minimize(cp.sum(cp.loggamma(cp.abs(x))))).is_dnlp()
    with pytest.raises(cp.DNLPError):
        cp.Problem(cp.Minimize(cp.sum(cp.loggamma(cp.abs(x))))).solve(nlp=True)


def test_numeric_uses_the_stable_formulas():
    import mpmath as mp
    u = np.array([-37.0, -8.0, -1e-3, 0.0, 0.5, 8.3, 16.5, 30.0])
    x = cp.Variable(u.size)
    x.value = u
    got = np.asarray(cp.log_normcdf(x).value)
    for ui, g in zip(u, got):
        r, _, _ = sr.special_mp(sr.OP_LOG_NORMCDF, ui)
        assert g != 0.0 and abs(g - float(r[0])) <= 64 * sr.EPS * 40 * 40 * abs(float(r[0])), (ui, g, r[0])     # (log_ndtr(16.5) is 0 in scipy 1.15)
    got = np.asarray(cp.normcdf(x).value)
    for ui, g in zip(u, got):
        r = float(mp.ncdf(mp.mpf(float(ui))))
        assert abs(g - r) <= 64 * sr.EPS * 40 * 40 * r, (ui, g, r)
    p = cp.Variable(4)
    p.value = np.array([0.5, 1.0, 3.0, 171.7])
    want = [float(mp.loggamma(mp.mpf(float(v)))) for v in p.value]
    assert np.allclose(np.asarray(cp.loggamma(p).value), want, rtol=1e-14, atol=1e-15)
    p.value = np.array([0.0, -1.0, 1.0, 2.0])
    v = np.asarray(cp.loggamma(p).value)
    assert v[0] == INF and np.isnan(v[1]) and v[2] == 0.0 and v[3] == 0.0


def test_canonical_form():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((5, 3))
    x = cp.Variable(3)
    x.value = np.array([0.3, -0.2, 0.1])
    for atom in (cp.log_normcdf, cp.normcdf):
        smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(-cp.sum(atom(A @ x)))))
        aux = [v for v in smooth.variables() if v is not x]
        assert len(smooth.constraints) == 1 and len(aux) == 1 and aux[0].shape == (5,) and aux[0].bounds is None
        assert np.array_equal(aux[0].value, A @ x.value)
        kept, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(-cp.sum(atom(x)))))
        assert not kept.constraints and kept.variables() == [x]                    # a bare variable is kept
    # loggamma: always a new variable on [0, inf), started at max(value, 1e-4)
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.loggamma(x)))))
    aux = [v for v in smooth.variables() if v is not x]
    assert len(smooth.constraints) == 1 and len(aux) == 1 and aux[0].shape == (3,)
    lo, hi = aux[0].bounds
    assert np.all(np.asarray(lo) == 0) and (hi is None or np.all(np.isinf(np.asarray(hi, float))))
    assert np.array_equal(aux[0].value, np.maximum(x.value, 1e-4))


def test_opcodes_and_segment_counts_are_those_of_exp():
    def arrays(atom):
        return lower(cp.Problem(cp.Minimize(cp.sum(atom(_var(7)))), [atom(_var(5)) <= 0]))
    ref = arrays(cp.exp)
    for name in ("log_normcdf", "normcdf"):
        a = arrays(getattr(cp, name))
        assert list(a["seg_op"]) == [OP[name]] * 2
        assert np.array_equal(a["dims"][:8], ref["dims"][:8])
        for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff"):
            assert np.array_equal(a[k], ref[k]), k
    a, ref = arrays(cp.loggamma), arrays(cp.log)                    # (both with an auxiliary variable and a row per argument)
    assert list(a["seg_op"]) == [16, 16] and np.array_equal(a["dims"][:8], ref["dims"][:8])
    for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff"):
        assert np.array_equal(a[k], ref[k]), k
    for name in ATOMS:
        one = lower(cp.Problem(cp.Minimize(cp.sum(getattr(cp, name)(_var(3))))))
        assert list(one["seg_op"]) == [OP[name]]


def test_the_atoms_are_fusable():
    from dnlp_amd.fused import build_fused_spec
    assert build_fused_spec(spb.latent_problem()[0]) is not None
    for name in ATOMS:
        assert build_fused_spec(cp.Problem(cp.Minimize(cp.sum(getattr(cp, name)(_var(4)))))) is not None


# ---- 3. solves on the host build -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(spb.SOLVES))
def test_solve_on_the_host_build(name):
    from oracle_frontend import oracle_engine
    prob, var, xs, fs = spb.SOLVES[name]()
    with oracle_engine():
        prob.solve(nlp=True, **spb.SOLVE_OPTS[name])
    spb.assert_solution(name, prob, var, xs, fs)


def test_probit_data_has_its_planted_rows():
    """Rows 0 and 1 have margin -12 at the point the solve starts from: its first sweeps run the left-tail formulas."""
    A, s = spb.probit_data()
    prob, x, xs, _ = spb.probit_problem()
    assert np.allclose(s[:2] * (A[:2] @ x.value), spb.PROBIT_MARGIN, rtol=1e-14) and np.max(np.abs(x.value - xs)) > 0.3


def test_fused_lbfgs_on_the_host_engine():
    from oracle_frontend import oracle_engine
    prob, var, xs, fs = spb.latent_problem()
    with oracle_engine():
        prob.solve(nlp=True, algorithm="lbfgs")
    assert prob._nlp_cache["sig"][0] == "direct" and prob._nlp_cache["data"]["tape"].m == 0
    spb.assert_solution("latent", prob, var, xs, fs)
