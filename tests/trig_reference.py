"""TEST INFRASTRUCTURE — cosh, atan, asin (flat tape ops 17, 18, 19 of csrc/atom_math.h) and the two-argument atan2 (op 22)
restated in mpmath at 80 digits, their argument grids, the error bound and an independent numpy statement that establishes K.
In the style of tests/special_reference.py; Units, Entries, the splitting of a reference into hi + lo and the K recipe are
those of tests/atom_reference.py.

Closed forms (value, d1, d2, and the third derivative for the bound only).
    cosh    cosh u     sinh u                  cosh u                       sinh u
    atan    atan u     1 / (1 + u^2)           -2 u / (1 + u^2)^2           (6 u^2 - 2) / (1 + u^2)^3
    asin    asin u     (1 - u^2)^(-1/2)        u (1 - u^2)^(-3/2)           (1 + 2 u^2) (1 - u^2)^(-5/2)
atan2(y, x), argument 0 is y, with r^2 = x^2 + y^2, six outputs in tape order (z; dvals runs y, x; hvals runs yy, xx, yx):
    value atan2(y, x);   gy = x / r^2;   gx = -y / r^2;   hyy = -2 x y / r^4;   hxx = -hyy;   hyx = (y - x) (y + x) / r^4
and their own partial derivatives for the bound:
    d gy  = (hyy, hyx)        d gx = (hyx, -hyy)
    d hyy = (-2 x (x^2 - 3 y^2) / r^6, -2 y (y^2 - 3 x^2) / r^6)        d hyx = (2 y (3 x^2 - y^2) / r^6, -2 x (3 y^2 - x^2) / r^6)

The bound is the project's own, |got - r| <= K eps (|r| + |u r'(u)|), eps = 2^-53; a two-argument output gets the same term
for its second argument, |r| + |y r_y| + |x r_x|, as tests/atom_reference.py states it.

Grids (seeded).
    cosh    U(-700, 700) x 3000, U(-5, 5) x 3000, +-10^U(-300, 0) x 200 each, 0, +-710.4, +-711 (overflow: IEEE class)
    atan    U(-50, 50) x 3000, +-10^U(-8, 100) x 2000 each, +-10^U(-300, -8) x 200 each, 0, +-1, +-1e150, +-1e300
    asin    U(-1, 1) x 3000, +-(1 - 10^U(-16, 0)) x 1000 each, +-10^U(-300, 0) x 200 each, 0, +-(1 - 2^-53); the edge
            points +-1, +-(1 + 2^-52), +-2 are compared by IEEE class
    atan2   |x|, |y| independently 10^U(-60, 60) x 4000 over all four sign pairs; U(-3, 3)^2 x 3000; (y, x) = (0, +-1),
            (+-1, 0), (+-1e-300, -1) next to the cut; x = +-y exactly x 50; the origin is compared by IEEE class
A point is left out of the magnitude comparison only when mpmath alone puts that output outside the normal double range; the
result must still not be NaN, and at most 2 % of an op's points may be left out for any output (asserted by the tests).  What
falls out: every output of cosh at +-711 (overflow), atan's d1 at +-1e300 and its d2 at +-1e150 and +-1e300 (below the normal
range); 0.05 % of a grid at the most.

K is measured, not chosen: `measured_K()` runs `numpy_rules` / `numpy_atan2` below (the stable formulas of DESIGN.md section 2
over numpy: independent of csrc/) against mpmath on the grids and returns, per op and output, 4 x the worst ratio rounded up
to a power of two, never below 8.  The factor 4 is the allowance for the device math library and FMA contraction that
tests/atom_reference.py uses.  Measured with

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import trig_reference as tr; tr.print_table()"

(worst |error| in units of eps * bracket; numpy 2.x over glibc):

    op       value     d1     d2                                  K
    cosh      1.33   0.47   1.33                                  (8, 8, 8)        worst at u = 5.1e-04, -0.033, 5.1e-04
    atan      0.68   1.35   1.92                                  (8, 8, 8)        worst at u = -1.65, 0.126, -1.06
    asin      0.65   1.71   1.45                                  (8, 8, 8)        worst at u = 0.50, -7.2e-07, 2.9e-03
             value     gy     gx    hyy    hxx    hyx
    atan2     1.01   1.16   1.08   1.33   1.33   1.56             (8, 8, 8, 8, 8, 8)

`measured_K()` recomputes the table in every run and refuses a numpy statement that is more than 4 units above it.
"""
import mpmath as mp
import numpy as np
import scipy.sparse as sp

import atom_reference as ar

OP_EXP, OP_MUL = 1, 20
OP_COSH, OP_ATAN, OP_ASIN, OP_ATAN2 = 17, 18, 19, 22
UNARY = [OP_COSH, OP_ATAN, OP_ASIN]
OPS = UNARY + [OP_ATAN2]
NAMES = {OP_COSH: "cosh", OP_ATAN: "atan", OP_ASIN: "asin", OP_ATAN2: "atan2", OP_EXP: "exp", OP_MUL: "mul"}
NOUT = {OP_COSH: 3, OP_ATAN: 3, OP_ASIN: 3, OP_ATAN2: 6}
EPS = ar.EPS
LEFT_OUT_SHARE = 0.02
K_EXP = (8, 8, 8)                 # tests/atom_reference.py: the table's row of exp; OP_MUL's value has 8 (3 |u v|) there

# worst units of the numpy statement per output, as printed by print_table()
TABLE = {
    OP_COSH: (1.33, 0.47, 1.33),
    OP_ATAN: (0.68, 1.35, 1.92),
    OP_ASIN: (0.65, 1.71, 1.45),
    OP_ATAN2: (1.01, 1.16, 1.08, 1.33, 1.33, 1.56),
}

mp.mp.dps = 80


# ---- closed forms --------------------------------------------------------------------------------------------------------------

def unary_mp(op, u):
    """-> ([value, d1, d2], [their derivatives in u]) as mpmath numbers."""
    x = mp.mpf(float(u))
    if op == OP_COSH:
        c, s = mp.cosh(x), mp.sinh(x)
        return [c, s, c], [s, c, s]
    if op == OP_ATAN:
        q = 1 + x * x
        d1, d2 = 1 / q, -2 * x / (q * q)
        return [mp.atan(x), d1, d2], [d1, d2, (6 * x * x - 2) / q ** 3]
    if op == OP_ASIN:
        s = (1 - x) * (1 + x)
        rt = mp.sqrt(s)
        d1, d2 = 1 / rt, x / (s * rt)
        return [mp.asin(x), d1, d2], [d1, d2, (1 + 2 * x * x) / (s * s * rt)]
    raise ValueError(op)


def atan2_mp(yf, xf):
    """-> ([value, gy, gx, hyy, hxx, hyx], [(d/dy, d/dx) of each]) as mpmath numbers."""
    y, x = mp.mpf(float(yf)), mp.mpf(float(xf))
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    gy, gx = x / r2, -y / r2
    hyy, hyx = -2 * x * y / r4, (y - x) * (y + x) / r4
    t_yy = (-2 * x * (x * x - 3 * y * y) / r6, -2 * y * (y * y - 3 * x * x) / r6)
    t_yx = (2 * y * (3 * x * x - y * y) / r6, -2 * x * (3 * y * y - x * x) / r6)
    return ([mp.atan2(y, x), gy, gx, hyy, -hyy, hyx],
            [(gy, gx), (hyy, hyx), (hyx, -hyy), t_yy, (-t_yy[0], -t_yy[1]), t_yx])


def in_domain(op, *args):
    if not all(np.isfinite(a) for a in args):
        return False
    if op == OP_ASIN:
        return abs(args[0]) < 1
    if op == OP_ATAN2:
        return args[0] != 0 or args[1] != 0
    return True


def edge_class(op, *args):
    """The IEEE class of the outputs at and beyond the edges, as DESIGN.md section 2 states it (a finite entry: any finite number)."""
    if any(np.isnan(a) for a in args):
        return (np.nan,) * NOUT[op]
    if op == OP_ASIN:
        u = args[0]
        if abs(u) == 1:
            return (np.copysign(np.pi / 2, u), np.inf, np.copysign(np.inf, u))
        return (np.nan,) * 3
    if op == OP_ATAN2 and args[0] == 0 and args[1] == 0:
        return (float(np.arctan2(args[0], args[1])),) + (np.nan,) * 5
    raise ValueError("no edge class stated for %s%r" % (NAMES[op], args))


_points = {}


def _point(op, *args):
    """One argument (pair) -> ((hi, lo, bracket, status) per output), memoised: a grid is evaluated in mpmath once however many
    tapes, segments and tests read it."""
    key = (int(op),) + tuple(float(a).hex() for a in args)
    if key not in _points:
        if not in_domain(op, *args):
            _points[key] = tuple((c, 0.0, 0.0, 2) for c in edge_class(op, *args))
        else:
            if op == OP_ATAN2:
                r, rp = atan2_mp(*args)
                y, x = mp.mpf(float(args[0])), mp.mpf(float(args[1]))
                brs = [abs(v) + abs(y * d[0]) + abs(x * d[1]) for v, d in zip(r, rp)]
            else:
                r, rp = unary_mp(op, args[0])
                x = mp.mpf(float(args[0]))
                brs = [abs(v) + abs(x * d) for v, d in zip(r, rp)]
            out = []
            for v, b in zip(r, brs):
                if ar._left_out(v):
                    out.append((float(mp.sign(v)) * (np.inf if abs(v) > 1 else 0.0), 0.0, 0.0, 1))
                else:
                    out.append(ar._split(v) + (float(b), 0))
            _points[key] = tuple(out)
    return _points[key]


def reference(op, *args):
    """hi, lo, bracket (each (NOUT, n)) and status (NOUT, n) as tests/atom_reference.unary_reference: 0 compare in magnitude,
    1 left out (the mpmath value lies outside the normal range), 2 edge: hi holds the IEEE class (a finite hi: any finite number).
    `args` is u for the unary ops and (y, x) for atan2."""
    args = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in args]
    n, k = args[0].size, NOUT[op]
    hi, lo, br = np.zeros((k, n)), np.zeros((k, n)), np.zeros((k, n))
    st = np.zeros((k, n), dtype=np.int8)
    for i in range(n):
        for j, (h, l, b, s) in enumerate(_point(op, *(a[i] for a in args))):
            hi[j, i], lo[j, i], br[j, i], st[j, i] = h, l, b, s
    return hi, lo, br, st


# ---- grids -----------------------------------------------------------------------------------------------------------------------

ASIN_EDGES = [1.0, -1.0, 1.0 + 2.0 ** -52, -(1.0 + 2.0 ** -52), 2.0, -2.0]
ATAN2_ORIGIN = (0.0, 0.0)


def grid(op):
    """In-domain arguments: u for a unary op, (y, x) for atan2."""
    rng = np.random.default_rng(4000 + int(op))
    if op == OP_COSH:
        t = 10.0 ** rng.uniform(-300, 0, 400)
        return np.concatenate([rng.uniform(-700, 700, 3000), rng.uniform(-5, 5, 3000), t[:200], -t[200:],
                               [0.0, 710.4, -710.4, 711.0, -711.0]])
    if op == OP_ATAN:
        big, tiny = 10.0 ** rng.uniform(-8, 100, 4000), 10.0 ** rng.uniform(-300, -8, 400)
        return np.concatenate([rng.uniform(-50, 50, 3000), big[:2000], -big[2000:], tiny[:200], -tiny[200:],
                               [0.0, 1.0, -1.0, 1e150, -1e150, 1e300, -1e300]])
    if op == OP_ASIN:
        near, tiny = 1.0 - 10.0 ** rng.uniform(-16, 0, 2000), 10.0 ** rng.uniform(-300, 0, 400)
        v = np.concatenate([rng.uniform(-1, 1, 3000), near[:1000], -near[1000:], tiny[:200], -tiny[200:],
                            [0.0, 1.0 - 2.0 ** -53, -(1.0 - 2.0 ** -53)]])
        assert np.all(np.abs(v) < 1)
        return v
    if op == OP_ATAN2:
        ys, xs = [], []
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                ys.append(sy * 10.0 ** rng.uniform(-60, 60, 4000))
                xs.append(sx * 10.0 ** rng.uniform(-60, 60, 4000))
        ys.append(rng.uniform(-3, 3, 3000))
        xs.append(rng.uniform(-3, 3, 3000))
        ys.append(np.array([0.0, 0.0, 1.0, -1.0, 1e-300, -1e-300]))
        xs.append(np.array([1.0, -1.0, 0.0, 0.0, -1.0, -1.0]))
        d = rng.choice([-1.0, 1.0], 50) * 10.0 ** rng.uniform(-60, 60, 50)
        ys.append(d)
        xs.append(d * rng.choice([-1.0, 1.0], 50))
        return np.concatenate(ys), np.concatenate(xs)
    raise ValueError(op)


def grid_args(op):
    g = grid(op)
    return g if isinstance(g, tuple) else (g,)


# ---- the independent statement ---------------------------------------------------------------------------------------------------

def numpy_rules(op, u):
    """(value, d1, d2) by the stable formulas of DESIGN.md section 2 over numpy."""
    u = np.asarray(u, dtype=float)
    with np.errstate(all="ignore"):
        if op == OP_COSH:
            return np.cosh(u), np.sinh(u), np.cosh(u)
        if op == OP_ATAN:
            d1 = 1.0 / (1.0 + u * u)
            return np.arctan(u), d1, (-2.0 * u * d1) * d1
        if op == OP_ASIN:
            s = (1.0 - u) * (1.0 + u)
            return np.arcsin(u), 1.0 / np.sqrt(s), u / (s * np.sqrt(s))
    raise ValueError(op)


def numpy_atan2(y, x):
    """(value, gy, gx, hyy, hxx, hyx): fourth powers of r as products of two quotients by r^2."""
    y, x = np.asarray(y, dtype=float), np.asarray(x, dtype=float)
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        gy, gx = x / r2, -y / r2
        hyy = 2.0 * gy * gx
        return np.arctan2(y, x), gy, gx, hyy, -hyy, ((y - x) / r2) * ((y + x) / r2)


def numpy_outputs(op, *args):
    return numpy_atan2(*args) if op == OP_ATAN2 else numpy_rules(op, *args)


def worst_ratios(rules, op, *args):
    """`rules(op, *args)` -> outputs against mpmath: per output the worst |error| in units of eps * bracket, its argument(s),
    the arguments with a wrong IEEE class, and the share of points left out."""
    hi, lo, br, st = reference(op, *args)
    n, k = args[0].size, NOUT[op]
    got = [np.asarray(g, float) * np.ones(n) for g in rules(op, *args)]
    worst, where, bad, share = [0.0] * k, [None] * k, [[] for _ in range(k)], [0.0] * k
    for j in range(k):
        share[j] = float(np.mean(st[j] == 1))
        with np.errstate(all="ignore"):
            err = np.abs((got[j] - hi[j]) - lo[j])
        for i in range(n):
            g, at = got[j][i], tuple(float(a[i]) for a in args)
            if st[j, i] == 1:
                if np.isnan(g):
                    bad[j].append(at)
                continue
            if st[j, i] == 2:
                h = hi[j, i]
                if not ((np.isnan(g) and np.isnan(h)) or (np.isinf(h) and g == h) or (np.isfinite(h) and np.isfinite(g))):
                    bad[j].append(at)
                continue
            if not np.isfinite(g):
                bad[j].append(at)
                continue
            ratio = 0.0 if err[i] == 0.0 else (np.inf if br[j, i] == 0.0 else err[i] / (EPS * br[j, i]))
            if ratio > worst[j]:
                worst[j], where[j] = ratio, at
    return worst, where, bad, share


_K = {}


def measured_table():
    if "table" not in _K:
        _K["table"] = {op: worst_ratios(numpy_outputs, op, *grid_args(op)) for op in OPS}
    return _K["table"]


def measured_K():
    """{op: K per output}."""
    if "K" not in _K:
        out = {}
        for op, (worst, where, bad, share) in measured_table().items():
            # a numpy statement that is itself wrong must not widen the bound the host and device builds are held to
            for j, w in enumerate(worst):
                assert w <= TABLE[op][j] + 4.0, ("numpy statement of %s, output %d: %.2f units of eps * bracket at %r; the table "
                                                 "says %.2f" % (NAMES[op], j, w, where[j], TABLE[op][j]))
            out[op] = tuple(ar._to_K(w) for w in worst)
        _K["K"] = out
    return _K["K"]


def print_table():
    for op, (worst, where, bad, share) in measured_table().items():
        print("%-6s %s   K %s\n       worst at %r\n       left out %s  wrong class %s" %
              (NAMES[op], " ".join("%6.2f" % w for w in worst), tuple(ar._to_K(w) for w in worst), where,
               " ".join("%.4f" % s for s in share), [b[:3] for b in bad]))


# ---- a tape of ops 17 - 19 and 22 (with exp and multiply beside them) in mpmath ------------------------------------------------------

def seg_args(a, s):
    """x indices of the segment's argument lists: (a0,) or (a0, a1)."""
    out = []
    for which in ("a0", "a1"):
        off, ln = int(a["seg_%s_off" % which][s]), int(a["seg_%s_len" % which][s])
        if ln:
            out.append(np.asarray(a["gidx"][off:off + ln], dtype=np.int64))
    return out


def _fill(dst, off, n, scale, hi, lo, st, tol, who):
    sl = slice(off, off + n)
    with np.errstate(all="ignore"):
        dst.hi[sl], dst.lo[sl] = scale * hi, scale * lo
    dst.st[sl] = st
    dst.tol[sl] = np.abs(scale) * tol
    for i in range(n):
        dst.who[off + i] = who[i]


def reference_sweep(a, x, w=None):
    """z, dvals and (with the weights w of the z entries) hvals of a tape whose segments are ops 17 - 19, 22, exp or multiply,
    every unit from the closed forms, as tests/atom_reference.Units."""
    K = measured_K()
    Z, nseg, nd, nh = (int(a["dims"][i]) for i in (2, 3, 4, 5))
    z, dv, hv = ar.Units(Z), ar.Units(nd), ar.Units(nh if w is not None else 0)
    for s in range(nseg):
        op, n = int(a["seg_op"][s]), int(a["seg_n"][s])
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        idx = seg_args(a, s)
        ws = np.ones(n) if w is None else np.asarray(w[zo:zo + n], float)
        one = np.ones(n)
        if op in UNARY or op == OP_EXP:
            u = x[idx[0]]
            hi, lo, br, st = reference(op, u) if op in UNARY else ar.unary_reference(op, u)
            kk = K[op] if op in UNARY else K_EXP
            who = [(s, NAMES[op], (float(v),)) for v in u]
            for k, (dst, off, scale) in enumerate(((z, zo, one), (dv, do, one), (hv, ho, ws))):
                if k == 2 and w is None:
                    continue
                _fill(dst, off, n, scale, hi[k], lo[k], st[k], kk[k] * EPS * br[k], who)
        elif op == OP_ATAN2:
            yv, xv = x[idx[0]], x[idx[1]]
            hi, lo, br, st = reference(op, yv, xv)
            kk = K[op]
            who = [(s, "atan2", (float(p), float(q))) for p, q in zip(yv, xv)]
            for k, (dst, off, scale) in enumerate(((z, zo, one), (dv, do, one), (dv, do + n, one), (hv, ho, ws), (hv, ho + n, ws),
                                                   (hv, ho + 2 * n, ws))):
                if k >= 3 and w is None:
                    continue
                _fill(dst, off, n, scale, hi[k], lo[k], st[k], kk[k] * EPS * br[k], who)
        elif op == OP_MUL:
            for i in range(n):
                uf, vf = float(x[idx[0][i]]), float(x[idx[1][i]])
                u, v = mp.mpf(uf), mp.mpf(vf)
                who = (s, "mul", (uf, vf))
                z.put(zo + i, u * v, 8 * EPS * 3 * abs(u * v), who)
                dv.put(do + i, v, 0.0, who)
                dv.put(do + n + i, u, 0.0, who)
                if w is not None:
                    hv.put(ho + i, mp.mpf(float(w[zo + i])), 0.0, who)
        else:
            raise ValueError("opcode %d has no mpmath statement here" % op)
    return z, dv, hv


def expected_oracles(a, x, lam=None, sigma=1.0, with_h=True):
    """{'f', 'grad_f', 'g', 'jac', 'hess'} -> tests/atom_reference.Entries for the tape `a` at x (Hessian of sigma f + lam' g)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = None
    if with_h:
        w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], np.zeros(m) if lam is None else np.asarray(lam, float)])
    z, dv, hv = reference_sweep(a, x, w)
    c = np.asarray(a["c"], float)
    G = ar._csr(a, "G", (m, N + Z)).tocsc()
    out = {
        "f": ar.Entries(np.asarray(a["c0"], float)[:1], sp.csr_matrix(c[None, :N]), x, sp.csr_matrix(c[None, N:]), z, "f"),
        "grad_f": ar.Entries(c[:N], None, x, ar._csr(a, "Mg", (N, nd)), dv, "grad_f"),
        "g": ar.Entries(a["b"], G[:, :N].tocsr(), x, G[:, N:].tocsr(), z, "g"),
        "jac": ar.Entries(a["Jc"], None, x, ar._csr(a, "MJ", (nnzJ, nd)), dv, "jac"),
        "units": (z, dv, hv),
    }
    if with_h:
        out["hess"] = ar.Entries(None, None, x, ar._csr(a, "MH", (nnzH, nh)), hv, "hess")
    return out
