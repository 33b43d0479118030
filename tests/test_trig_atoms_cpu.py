"""cosh, atan, asin, acos and atan2 without a GPU (flat tape ops 17, 18, 19 and the two-argument op 22;
tests/trig_reference.py: closed forms in mpmath, grids, the bound and how K is measured; tests/trig_problems.py: the solves and
their answers).

The rule: the numpy statement establishes K; the host build of csrc/atom_math.h (oracle.oracle_capi.OracleProblem) is held
against mpmath on the full grids through eval_g, eval_jac_g, eval_h (non-unit multipliers), eval_f and eval_grad_f; the edge
points are checked by IEEE class; the two places where the naive formulas fail (atan's d2 at 1e90, asin's d1 next to 1) are
checked in magnitude.  Front end: curvature, sign, monotonicity, rule tags, is_dnlp, canonical forms, opcodes, argument counts
and Hessian index runs, the refusal of atan2(t, t).  Solves on the host build, fusability, and the one-host-lane wavefront
solver against the generic algorithm text on a template with atan2."""
import numpy as np
import pytest

import atom_reference as ar
import dnlp_amd as cp
import trig_problems as tp
import trig_reference as tr
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.nlp_solver import build_nlp_data
from dnlp_amd.tape import serialize

ATOMS = ["cosh", "atan", "asin", "atan2"]
OP = {tr.NAMES[op]: op for op in tr.OPS}
NAN, INF = np.nan, np.inf
# (argument lists per atom) at and beyond the edges: IEEE class only.  atan2: the origin with both signs of zero, and NaN in
EDGE_POINTS = {
    "cosh": [np.array([NAN])],
    "atan": [np.array([NAN])],
    "asin": [np.array(tr.ASIN_EDGES + [NAN])],
    "atan2": [np.array([0.0, 0.0, -0.0, -0.0, NAN, 1.0]), np.array([0.0, -0.0, 0.0, -0.0, 1.0, NAN])],
}
# where the naive statement of a formula fails while the rule's holds: (atom, output, argument)
COSH_OVERFLOW = np.array([711.0, -711.0, 710.4, -710.4])      # the first two overflow (not NaN), the other two are normal numbers
TRAPS = [("atan", 2, 1e90), ("atan", 2, -1e90), ("asin", 1, 1.0 - 1e-15), ("asin", 1, -(1.0 - 1e-15)),
         # next to 1 the product u u happens to be exact (u = 1 - k 2^-53); 1 - u u loses its digits a little further in
         ("asin", 1, 1.0 - 3.3e-9), ("asin", 1, -(1.0 - 1.7e-6)), ("asin", 2, 1.0 - 3.3e-9)]


def multipliers(m):
    """+-2^k, k in -2..2, neighbours always different: a Hessian entry is lam_i d2 up to an exact scaling."""
    i = np.arange(m)
    return np.where((i // 5) % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 5) - 2)


def _var(n):
    v = cp.Variable(n)
    v.value = np.full(n, 0.5)
    return v


def apply_atom(name, n):
    """The atom on fresh variables of n entries."""
    f = getattr(cp, name)
    return f(_var(n), _var(n)) if name == "atan2" else f(_var(n))


def lower(prob):
    smooth, _ = Dnlp2Smooth().apply(prob)
    return dict(build_nlp_data(smooth)[0]["tape_arrays"])


def fill(a, per_segment):
    """x with every segment's arguments (a list of arrays per segment: u, or y and x) written at the indices the segment reads
    (evaluation needs no feasible point)."""
    x = np.zeros(int(a["dims"][0]))
    seen = np.zeros(x.size, dtype=bool)
    for s, args in enumerate(per_segment):
        idx = tr.seg_args(a, s)
        assert len(idx) == len(args)
        for ix, u in zip(idx, args):
            assert ix.size == u.size and not seen[ix].any()
            x[ix], seen[ix] = u, True
    return x


_tapes = {}


def tape(name):
    """-> (tape arrays, x, multipliers, sigma): the atom once in the objective and once in a constraint, on its whole grid."""
    if name not in _tapes:
        if name in ("edges", "traps", "overflow"):
            if name == "edges":
                pts = EDGE_POINTS
            elif name == "traps":
                pts = {n: [np.array([u for (m, _, u) in TRAPS if m == n])] for n in ("atan", "asin")}
            elif name == "overflow":
                pts = {"cosh": [COSH_OVERFLOW]}
            names = [n for n in ATOMS if n in pts]
            a = lower(cp.Problem(cp.Minimize(0 * cp.sum(_var(1))), [apply_atom(n, pts[n][0].size) <= 0 for n in names]))
            assert list(a["seg_op"]) == [OP[n] for n in names]
            x = fill(a, [pts[n] for n in names])
        else:
            args = list(tr.grid_args(OP[name]))
            n = args[0].size
            # the objective adds its segment up, and f is c'[x; z] over EVERY z entry: a value that overflows (cosh(+-711); decided
            # by mpmath) anywhere on the tape makes f NaN through 0 * inf whatever the rule returns, and cosh(+-710.4) = 1.67e308
            # twice is past the double range as a sum.  Those four points have the "overflow" tape (constraint only) to themselves
            hi = tr.reference(OP[name], *args)[0][0]
            finite = np.abs(hi) < 1e305
            if name == "cosh":
                assert np.array_equal(np.sort(args[0][~finite]), np.sort(COSH_OVERFLOW))
            else:
                assert finite.all()
            args = [u[finite] for u in args]
            n = args[0].size
            a = lower(cp.Problem(cp.Minimize(cp.sum(apply_atom(name, n))), [apply_atom(name, n) <= 0]))
            assert list(a["seg_op"]) == [OP[name]] * 2
            x = fill(a, [args, args])
        # (next to the overflow threshold no multiplier above 1: 2 x 1.67e308 is past the range whatever the rule returns)
        _tapes[name] = (a, x, multipliers(int(a["dims"][1])) * (0.25 if name == "overflow" else 1.0), 0.5)
    return _tapes[name]


def check_callbacks(ev, name):
    """g, Jacobian, Hessian, f and grad f of `ev` entry by entry; every failing callback is reported."""
    a, x, lam, sigma = tape(name)
    exp = tr.expected_oracles(a, x, lam, sigma)
    if name != "overflow":
        for units in exp["units"]:
            assert np.mean(units.st == 1) <= tr.LEFT_OUT_SHARE, "more than 2 % of the grid left out of the magnitude comparison"
    checks = [(exp["g"], lambda: ev.eval_g(x)), (exp["jac"], lambda: ev.eval_jac_g(x)), (exp["hess"], lambda: ev.eval_h(x, lam, sigma))]
    if name != "overflow":
        checks += [(exp["f"], lambda: [ev.eval_f(x)]), (exp["grad_f"], lambda: ev.eval_grad_f(x))]
    failed = []
    with np.errstate(all="ignore"):
        for entries, thunk in checks:
            try:
                entries.check(thunk())
            except AssertionError as err:
                failed.append(str(err))
    assert not failed, "\n".join(failed)


def unit_outputs(ev, name="edges"):
    """{atom: outputs per point, in the order of tests/trig_reference.py (value, d1, d2 / value, gy, gx, hyy, hxx, hyx)} read
    back out of eval_g / eval_jac_g / eval_h of a tape whose constraint rows are one atom entry each (the maps are then
    one-to-one, which is asserted)."""
    a, x, lam, sigma = tape(name)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])
    with np.errstate(all="ignore"):
        g, jac, hess = np.asarray(ev.eval_g(x)), np.asarray(ev.eval_jac_g(x)), np.asarray(ev.eval_h(x, lam, sigma))
    Gz = ar._csr(a, "G", (m, N + Z)).tocsc()[:, N:].tocsc()
    MJ, MH = ar._csr(a, "MJ", (nnzJ, nd)).tocsc(), ar._csr(a, "MH", (nnzH, nh)).tocsc()

    def read(vec, M, c):
        rows = M.indices[M.indptr[c]:M.indptr[c + 1]]
        assert rows.size == 1 and abs(M.data[M.indptr[c]]) == 1.0
        return vec[int(rows[0])] / M.data[M.indptr[c]]

    out = {}
    for s in range(nseg):
        n, zo, do, ho = (int(a[k][s]) for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff"))
        two = int(a["seg_op"][s]) == tr.OP_ATAN2
        cols = [np.array([read(g, Gz, zo + i) for i in range(n)])]
        for run in range(2 if two else 1):
            cols.append(np.array([read(jac, MJ, do + run * n + i) for i in range(n)]))
        for run in range(3 if two else 1):
            with np.errstate(all="ignore"):
                cols.append(np.array([read(hess, MH, ho + run * n + i) / w[zo + i] for i in range(n)]))
        out[tr.NAMES[int(a["seg_op"][s])]] = cols
    return out


def assert_edge_classes(out):
    """The IEEE classes of DESIGN.md section 2 (tests/trig_reference.edge_class) on the outputs of `unit_outputs`."""
    for name, cols in out.items():
        pts = EDGE_POINTS[name]
        for i in range(pts[0].size):
            want = tr.edge_class(OP[name], *(p[i] for p in pts))
            for k, h in enumerate(want):
                g = cols[k][i]
                ok = (np.isnan(g) and np.isnan(h)) or (np.isinf(h) and g == h) or (np.isfinite(h) and g == h)
                assert ok, (name, [p[i] for p in pts], k, g, h)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_establishes_K():
    """The numpy statement on every grid: the right IEEE class everywhere, at most 2 % of an op's points left out for any output
    (only the planted extreme points are), within 4 units of the table in tests/trig_reference.py; K = 4 x worst, up to a power
    of two and at least 8."""
    wrong = []
    for op, (worst, where, bad, share) in tr.measured_table().items():
        if any(bad):
            wrong.append("%s: wrong IEEE class at %r" % (tr.NAMES[op], [b[:6] for b in bad]))
        if max(share) > tr.LEFT_OUT_SHARE:
            wrong.append("%s: shares %r of the grid left out" % (tr.NAMES[op], share))
    assert not wrong, "\n".join(wrong)
    n_left = {tr.NAMES[op]: [int(round(s * tr.grid_args(op)[0].size)) for s in t[3]] for op, t in tr.measured_table().items()}
    assert n_left == {"cosh": [2, 2, 2], "atan": [0, 2, 4], "asin": [0, 0, 0], "atan2": [0] * 6}, n_left
    K = tr.measured_K()
    tr.print_table()
    assert all(8 <= k <= 32 and k & (k - 1) == 0 for ks in K.values() for k in ks), K
    assert [len(K[op]) for op in tr.OPS] == [3, 3, 3, 6]


@pytest.mark.parametrize("name", ATOMS)
def test_host_build_against_mpmath(name):
    """csrc/atom_math.h compiled by g++: g, Jacobian, Hessian, f, grad f entry by entry on the full grid."""
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(tape(name)[0])), name)


def test_host_build_where_cosh_overflows():
    """+-711: mpmath puts value, d1 and d2 beyond the double range, so the outputs are +-inf (or the largest finite number), never
    NaN; +-710.4 beside them are normal numbers (1.67e308) and compared in magnitude."""
    from oracle.oracle_capi import OracleProblem
    ev = OracleProblem(serialize(tape("overflow")[0]))
    check_callbacks(ev, "overflow")
    val, d1, d2 = unit_outputs(ev, "overflow")["cosh"]
    assert np.array_equal(val[:2], [INF, INF]) and np.array_equal(d1[:2], [INF, -INF]) and np.array_equal(d2[:2], [INF, INF])


def test_host_build_on_the_edges():
    """asin at and beyond +-1, atan2 at the origin (value per IEEE atan2, both signs of zero; derivatives NaN), NaN in -> NaN out."""
    from oracle.oracle_capi import OracleProblem
    assert_edge_classes(unit_outputs(OracleProblem(serialize(tape("edges")[0]))))


def test_the_two_traps_are_correct_in_magnitude():
    """atan's d2 at +-1e90 is -+2e-270: -2 u / (q q) with q = 1 + u^2 returns 0 there (q q overflows).  asin's d1 at 1 - 1e-15 is
    2.2e7, and at 1 - 3.3e-9 the statement through 1 - u u is off by 7e6 eps.  All against mpmath within 8 eps |r| -- the TIGHT
    bracket, without |u r'|."""
    from oracle.oracle_capi import OracleProblem
    out = unit_outputs(OracleProblem(serialize(tape("traps")[0])), "traps")
    seen = {"atan": 0, "asin": 0}
    for name, k, u in TRAPS:
        got = out[name][k][seen[name]]
        seen[name] += 1
        r = float(tr.unary_mp(OP[name], u)[0][k])
        assert r != 0.0 and np.isfinite(r) and abs(got - r) <= 8 * tr.EPS * abs(r), (name, k, u, got, r)
    # the naive statements do fail here: the trap is real
    with np.errstate(all="ignore"):
        q = 1.0 + 1e90 * 1e90
        assert -2.0 * 1e90 / (q * q) == 0.0
        for u in (1.0 - 3.3e-9, 1.0 - 1.7e-6):
            r = float(tr.unary_mp(tr.OP_ASIN, u)[0][1])
            assert abs(1.0 / np.sqrt(1.0 - u * u) - r) > 1000 * tr.EPS * r


# ---- 2. front end ----------------------------------------------------------------------------------------------------------------
def test_curvature_sign_monotonicity_and_rule_tags():
    x, pos, neg = cp.Variable(4), cp.Variable(4, nonneg=True), cp.Variable(4, nonpos=True)
    c = cp.cosh(x)
    assert c.is_convex() and not c.is_concave() and c.is_nonneg() and not c.is_nonpos() and not c.is_incr(0) and not c.is_decr(0)
    assert cp.cosh(pos).is_incr(0) and not cp.cosh(pos).is_decr(0) and cp.cosh(neg).is_decr(0) and not cp.cosh(neg).is_incr(0)
    for f, concave_right in ((cp.atan, True), (cp.asin, False)):
        e, r, l = f(x), f(pos), f(neg)
        assert e.is_incr(0) and not e.is_decr(0) and not e.is_convex() and not e.is_concave() and not e.is_nonneg() and not e.is_nonpos()
        assert r.is_nonneg() and not r.is_nonpos() and l.is_nonpos() and not l.is_nonneg()
        assert (r.is_concave(), r.is_convex(), l.is_concave(), l.is_convex()) == (concave_right, not concave_right, not concave_right, concave_right)
    t = cp.atan2(x, pos)
    assert not t.is_convex() and not t.is_concave() and not t.is_nonneg() and not t.is_nonpos()
    assert not any((t.is_incr(0), t.is_incr(1), t.is_decr(0), t.is_decr(1)))
    for e in (c, cp.atan(x), cp.asin(x), t, cp.acos(x)):
        like = cp.sin(x)
        assert (e.is_esr(), e.is_hsr(), e.is_smooth()) == (like.is_esr(), like.is_hsr(), like.is_smooth()) == (True, True, True)
        assert e.shape == (4,)
    for e in (c, cp.atan(x), cp.asin(x), t):
        assert e.is_atom_esr() and e.is_atom_hsr()
    # composition: the increasing atoms take an ESR / HSR argument on the matching side; cosh only where its argument's sign
    # makes it monotone; atan2, monotone in neither argument, only smooth ones
    assert cp.atan(cp.abs(x)).is_esr() and not cp.atan(cp.abs(x)).is_hsr()
    assert cp.asin(-cp.abs(x)).is_hsr() and not cp.asin(-cp.abs(x)).is_esr()
    assert cp.cosh(cp.abs(x)).is_esr() and not cp.cosh(cp.abs(x)).is_hsr()
    assert not cp.atan2(cp.abs(x), pos).is_esr() and not cp.atan2(x, cp.abs(x)).is_hsr()
    # acos is a function, not a class: pi / 2 - asin
    assert not hasattr(cp.acos, "mro") and type(cp.acos(x)).__name__ == "AddExpression"


def test_numeric_and_broadcasting():
    x = cp.Variable(3)
    x.value = np.array([-0.5, 0.0, 0.9])
    assert np.array_equal(cp.cosh(x).value, np.cosh(x.value)) and np.array_equal(cp.atan(x).value, np.arctan(x.value))
    assert np.array_equal(cp.asin(x).value, np.arcsin(x.value))
    assert np.allclose(cp.acos(x).value, np.arccos(x.value), rtol=0, atol=4e-16)
    s = cp.Variable()
    s.value = np.array(-2.0)
    assert cp.atan2(x, s).shape == (3,) and cp.atan2(s, x).shape == (3,) and cp.atan2(1.0, x).shape == (3,)
    assert np.array_equal(cp.atan2(x, s).value, np.arctan2(x.value, -2.0))
    assert np.array_equal(cp.atan2(s, x).value, np.arctan2(-2.0, x.value))
    X = cp.Variable((2, 3))
    X.value = np.arange(6.0).reshape(2, 3) - 2.5
    assert cp.atan2(X, 2.0).shape == (2, 3) and np.array_equal(cp.atan2(X, 2.0).value, np.arctan2(X.value, 2.0))
    x.value = np.array([-1.5, 1.0, 2.0])
    v = np.asarray(cp.asin(x).value)
    assert np.isnan(v[0]) and v[1] == np.pi / 2 and np.isnan(v[2])


def test_is_dnlp_accepts_and_refuses():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((6, 3))
    x, y = cp.Variable(3), cp.Variable(6)
    for f in (cp.cosh, cp.atan, cp.asin, cp.acos):
        assert cp.Problem(cp.Minimize(cp.sum(f(A @ x)))).is_dnlp() and cp.Problem(cp.Maximize(cp.sum(f(A @ x)))).is_dnlp()
        assert cp.Problem(cp.Minimize(x[0]), [f(A @ x) <= 0.5, f(y) >= 0.1, f(y) == A @ x]).is_dnlp()
    assert cp.Problem(cp.Minimize(cp.sum_squares(cp.atan2(A @ x, y) - 0.3))).is_dnlp()
    assert cp.Problem(cp.Minimize(x[0]), [cp.atan2(A @ x, y) <= 0.5, cp.atan2(y, 2.0) >= 0.1, 0.2 == cp.atan2(1.0, y)]).is_dnlp()
    # a nonsmooth argument only on the side the atom's monotonicity carries
    assert cp.Problem(cp.Minimize(cp.sum(cp.atan(cp.abs(x))))).is_dnlp() and not cp.Problem(cp.Maximize(cp.sum(cp.atan(cp.abs(x))))).is_dnlp()
    assert cp.Problem(cp.Minimize(cp.sum(cp.cosh(cp.abs(x))))).is_dnlp() and not cp.Problem(cp.Minimize(cp.sum(cp.cosh(-cp.abs(x) + 1)))).is_dnlp()
    assert cp.Problem(cp.Minimize(x[0]), [cp.asin(cp.abs(x)) <= 0.5]).is_dnlp() and not cp.Problem(cp.Minimize(x[0]), [cp.asin(cp.abs(x)) >= 0.5]).is_dnlp()
    assert not cp.Problem(cp.Minimize(cp.sum(cp.acos(cp.abs(x))))).is_dnlp() and cp.Problem(cp.Maximize(cp.sum(cp.acos(cp.abs(x))))).is_dnlp()
    bad = cp.Problem(cp.Minimize(cp.sum(cp.atan2(cp.abs(x), 1.0))))
    assert not bad.is_dnlp() and not cp.Problem(cp.Maximize(cp.sum(cp.atan2(cp.abs(x), 1.0)))).is_dnlp()
    with pytest.raises(cp.DNLPError):
        bad.solve(nlp=True)


def test_canonical_forms():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((5, 3))
    x = cp.Variable(3)
    x.value = np.array([0.3, -0.2, 0.1])
    for atom in (cp.cosh, cp.atan):
        smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(atom(A @ x)))))
        aux = [v for v in smooth.variables() if v is not x]
        assert len(smooth.constraints) == 1 and len(aux) == 1 and aux[0].shape == (5,) and aux[0].bounds is None
        assert np.array_equal(aux[0].value, A @ x.value)
        kept, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(atom(x)))))
        assert not kept.constraints and kept.variables() == [x]                    # a bare variable is kept
    # asin: always a new variable on [-1, 1], like atanh's
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.asin(x)))))
    aux = [v for v in smooth.variables() if v is not x]
    assert len(smooth.constraints) == 1 and len(aux) == 1 and aux[0].shape == (3,)
    lo, hi = aux[0].bounds
    assert np.all(np.asarray(lo) == -1) and np.all(np.asarray(hi) == 1) and np.array_equal(aux[0].value, x.value)
    # atan2 of two affine expressions: two aliases, rows in argument order (y, then x)
    B = rng.standard_normal((5, 3))
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.atan2(A @ x, B @ x + 1.0)))))
    aux = [v for v in smooth.variables() if v is not x]
    assert len(smooth.constraints) == 2 and len(aux) == 2 and all(v.shape == (5,) and v.bounds is None for v in aux)
    vals = sorted((tuple(v.value) for v in aux))
    assert vals == sorted((tuple(A @ x.value), tuple(B @ x.value + 1.0)))
    a = lower(cp.Problem(cp.Minimize(cp.sum(cp.atan2(A @ x, B @ x + 1.0)))))
    assert list(a["seg_op"]) == [22] and int(a["dims"][1]) == 10
    # bare variables stay; a constant argument becomes t == c (no constant shortcut)
    y = cp.Variable(3)
    kept, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.atan2(y, x)))))
    assert not kept.constraints and set(map(id, kept.variables())) == {id(x), id(y)}
    const, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.atan2(y, np.array([1.0, 2.0, 3.0]))))))
    aux = [v for v in const.variables() if v is not y]
    assert len(const.constraints) == 1 and len(aux) == 1 and np.array_equal(aux[0].value, [1.0, 2.0, 3.0])
    # acos lowers to ONE op-19 segment (and a constant pi / 2 per entry in the objective)
    a = lower(cp.Problem(cp.Minimize(cp.sum(cp.acos(x)))))
    assert list(a["seg_op"]) == [19] and list(a["seg_n"]) == [3] and abs(float(a["c0"][0]) - 3 * np.pi / 2) < 4e-15


def test_opcodes_argument_counts_and_hessian_runs():
    def arrays(make):
        return lower(cp.Problem(cp.Minimize(cp.sum(make(7))), [make(5) <= 0]))
    ref = arrays(lambda n: cp.exp(_var(n)))
    for name in ("cosh", "atan"):
        a = arrays(lambda n: apply_atom(name, n))
        assert list(a["seg_op"]) == [OP[name]] * 2 and list(a["seg_a1_len"]) == [0, 0] and list(a["seg_a0_len"]) == [7, 5]
        assert np.array_equal(a["dims"][:8], ref["dims"][:8])
        for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff", "seg_dcount", "seg_hcount"):
            assert np.array_equal(a[k], ref[k]), k
    a, ref = arrays(lambda n: cp.asin(_var(n))), arrays(lambda n: cp.atanh(_var(n)))     # (both with an auxiliary variable per argument)
    assert list(a["seg_op"]) == [19, 19] and list(a["seg_a1_len"]) == [0, 0] and np.array_equal(a["dims"][:8], ref["dims"][:8])
    for k in ("seg_n", "seg_zoff", "seg_doff", "seg_hoff", "seg_dcount", "seg_hcount"):
        assert np.array_equal(a[k], ref[k]), k
    # atan2: the layout of rel_entr -- 2n derivative entries (y run, x run), 3n Hessian entries in the runs (y,y), (x,x), (y,x)
    y, x = _var(4), _var(4)
    a = lower(cp.Problem(cp.Minimize(cp.sum(cp.atan2(y, x)))))
    r = lower(cp.Problem(cp.Minimize(cp.sum(cp.rel_entr(_var(4), _var(4))))))
    assert list(a["seg_op"]) == [22] and list(r["seg_op"]) == [21]
    for k in ("seg_n", "seg_a0_len", "seg_a1_len", "seg_zcount", "seg_dcount", "seg_hcount"):
        assert np.array_equal(a[k], r[k]), k
    assert (int(a["seg_dcount"][0]), int(a["seg_hcount"][0]), int(a["seg_a0_len"][0]), int(a["seg_a1_len"][0])) == (8, 12, 4, 4)
    iy, ix = tr.seg_args(a, 0)
    assert np.array_equal(a["dcol"], np.concatenate([iy, ix])) and np.array_equal(a["drow"], np.tile(np.arange(4), 2))
    assert np.array_equal(a["hrow"], np.concatenate([iy, ix, np.maximum(iy, ix)]))
    assert np.array_equal(a["hcol"], np.concatenate([iy, ix, np.minimum(iy, ix)]))
    # a scalar argument is promoted like multiply's, and the promotion (not a bare variable) gets an alias of the full shape
    s = cp.Variable()
    s.value = np.array(2.0)
    a = lower(cp.Problem(cp.Minimize(cp.sum(cp.atan2(y, s)))))
    iy, ix = tr.seg_args(a, 0)
    assert int(a["dims"][1]) == 4 and iy.size == ix.size == 4 and np.unique(np.concatenate([iy, ix])).size == 8


def test_atan2_of_a_variable_with_itself_is_refused():
    """atan2(x, x) is piecewise constant; on the tape both index lists would be the same x entries and the cross Hessian entry
    would fall on the diagonal once instead of twice (multiply refuses a variable with itself for the same reason).  Anything
    that is not a bare variable gets an alias per argument, so entries of one variable lower correctly: to distinct x indices."""
    x = cp.Variable(3)
    x.value = np.array([0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="atan2 of a variable entry with itself"):
        lower(cp.Problem(cp.Minimize(cp.sum(cp.atan2(x, x)))))
    for prob in (cp.Problem(cp.Minimize(cp.atan2(x[0], x[2]))), cp.Problem(cp.Minimize(cp.atan2(x[1], x[1])))):
        a = lower(prob)
        iy, ix = tr.seg_args(a, 0)
        assert list(a["seg_op"]) == [22] and list(a["seg_n"]) == [1] and int(a["dims"][1]) == 2 and iy[0] != ix[0]


def test_the_atoms_are_fusable_where_their_twins_are():
    from dnlp_amd.fused import build_fused_spec
    for name in ("cosh", "atan", "asin", "acos"):
        assert build_fused_spec(cp.Problem(cp.Minimize(cp.sum(getattr(cp, name)(_var(4)))))) is not None
        assert build_fused_spec(cp.Problem(cp.Minimize(cp.sum(cp.square(getattr(cp, name)(2.0 * _var(4)) - 0.1))))) is not None
    # the two-argument atoms have no fused form: rel_entr has none, atan2 has none; such a problem keeps the tape path
    assert build_fused_spec(cp.Problem(cp.Minimize(cp.sum(cp.rel_entr(_var(4), _var(4)))))) is None
    assert build_fused_spec(cp.Problem(cp.Minimize(cp.sum(cp.atan2(_var(4), _var(4)))))) is None


def test_tape_validation_of_argument_counts():
    """csrc/tape.h: op 22 needs two arguments of n entries, ops 17 - 19 one."""
    from oracle.oracle_capi import OracleProblem
    a = lower(cp.Problem(cp.Minimize(cp.sum(cp.atan2(_var(4), _var(4))))))
    OracleProblem(serialize(a))
    for op, msg in ((19, "one argument"), (17, "one argument")):
        b = dict(a)
        b["seg_op"] = np.array([op], dtype=a["seg_op"].dtype)
        with pytest.raises(Exception, match=msg):
            OracleProblem(serialize(b))
    u = lower(cp.Problem(cp.Minimize(cp.sum(cp.atan(_var(4))))))
    b = dict(u)
    b["seg_op"] = np.array([22], dtype=u["seg_op"].dtype)
    with pytest.raises(Exception, match="two arguments"):
        OracleProblem(serialize(b))


# ---- 3. solves on the host build -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host_driven", "limited_memory"])
@pytest.mark.parametrize("name", sorted(tp.SOLVES))
def test_solve_on_the_host_build(name, mode):
    from oracle_frontend import oracle_engine
    prob, var, xs, fs = tp.SOLVES[name]()
    with oracle_engine():
        prob.solve(nlp=True, **tp.SOLVE_OPTS[name], **tp.MODES[mode])
    tp.assert_solution(name, prob, var, xs, fs)


def test_cosh_problem_on_the_lbfgs_path_of_the_host_engine():
    """Unconstrained and convex: algorithm='lbfgs' takes it (reduced space: the rows t == A x - b only define t).  A x is a matrix
    product, not an elementwise term, so the objective has no fused program and the L-BFGS loop evaluates the tape."""
    from oracle_frontend import oracle_engine
    prob, var, xs, fs = tp.cosh_problem()
    with oracle_engine():
        prob.solve(nlp=True, algorithm="lbfgs", tol=1e-10)
    assert prob._nlp_cache["data"]["reducible"]
    tp.assert_solution("cosh", prob, var, xs, fs)
    assert np.max(np.abs(tp.cosh_gradient(var.value))) <= 1e-8


def test_bearing_rows_stay_away_from_the_cut():
    rows = tp.bearing_rows(64)
    assert rows.shape == (64, 5) and np.all(np.abs(rows) <= np.pi - tp.CUT_MARGIN) and np.array_equal(rows[0], tp.bearing_data()[1])


# ---- 4. the wavefront solver's text --------------------------------------------------------------------------------------------
def test_wave_restatement_equals_the_generic_text_bit_for_bit_on_a_template_with_atan2():
    """The comparison of tests/test_wave_ipm_cpu.py on the bearing template: one host lane of csrc/wave_ipm.h against the host
    build of the generic algorithm text, over the same plan block and instance rows."""
    from dnlp_amd.batch import ParametricBatch
    from wave_oracle import HostBatch
    prob, params, _ = tp.bearing_template()
    pb = ParametricBatch(prob, params)
    assert 22 in list(pb.arrays0["seg_op"])
    hb = HostBatch(pb, {"linear_solver": "sparse"})      # (order 32: the automatic choice is the dense KKT, which the wavefront solver does not take)
    thetas = tp.bearing_rows(24)
    w, g = hb.solve(thetas, 0), hb.solve(thetas, 1)
    assert np.all(w["status"] == 0) and np.array_equal(w["status"], g["status"])
    for k in ("iters", "nfact", "x", "obj", "mult_g", "zl", "zu"):
        assert np.array_equal(bits(w[k]) if w[k].dtype == np.float64 else w[k], bits(g[k]) if g[k].dtype == np.float64 else g[k]), k
