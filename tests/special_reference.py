"""TEST INFRASTRUCTURE — log_normcdf, normcdf and loggamma (flat tape ops 14, 15, 16 of csrc/atom_math.h) restated in mpmath
at 80 digits, their argument grids, the error bound and an independent numpy / scipy statement that establishes K.  In the
style of tests/atom_reference.py, whose pieces (Units, Entries, the splitting of a reference into hi + lo, the K recipe) it uses.

Closed forms.  phi(u) = exp(-u^2 / 2) / sqrt(2 pi), Phi the normal CDF, lambda = phi / Phi.
    log_normcdf   log Phi          lambda         -lambda (u + lambda)      third: -r2 (u + lambda) - lambda (1 + r2)
    normcdf       Phi              phi            -u phi                    third: (u^2 - 1) phi
    loggamma      ln Gamma         psi            psi_1                     third: psi_2
log Phi is mp.log(mp.ncdf(u)) for u <= 0 and mp.log1p(-mp.ncdf(-u)) for u > 0 (at 60 digits log(ncdf(16.5)) is already wrong).

The bound is the project's own, |got - r| <= K eps (|r| + |u r'(u)|), eps = 2^-53, with one exception: for log_normcdf's second
derivative the bracket is lambda (|u| + lambda) + |u r'|.  The stated expression -lambda (u + lambda) subtracts two numbers of
size |u| to get one of size 1 / |u| in the left tail; that conditioning belongs to the rule.  A rule that does better passes
the same test.

Grids (seeded).  Normal pair: U(-37, 37) x 3000, U(-8, 8) x 3000, U(-1, 1) x 500, +-10^U(-8, 0) x 200 each, and 0, +-37, -36.5,
8.3, +-5.  loggamma: 10^U(-6, 6) x 4000, U(0.5, 3) x 2000, and 1, 2 (the zeros of ln Gamma), 1.4616321449683623 (the zero of
psi), 1e-6, 1e6, 0.5, 3, 171.7, 172.  No output of any grid point lies outside the normal double range: zero points are left
out of the magnitude comparison, and the tests assert that.

K is measured, not chosen: `measured_K()` runs `numpy_rules` below (the formulas of DESIGN.md section 2 over
scipy.special.erfcx / gammaln / psi / polygamma: independent of csrc/) against mpmath on the grids and returns, per op and
output, 4 x the worst ratio rounded up to a power of two, never below 8.  The factor 4 is the allowance for the device math
library that tests/atom_reference.py uses.  Measured with

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import special_reference as sr; sr.print_table()"

(worst |error| in units of eps * bracket; scipy 1.15.3):

    op             value     d1     d2   K
    log_normcdf     10.3    7.9   16.1   (64, 32, 128)     worst at u = -5.1e-05, -6.0e-06, -6.0e-06
    normcdf          7.7    2.0    2.6   (32, 8, 16)       worst at u = 1.5e-05, -0.088, 1.04
    loggamma         9.4    2.3    3.0   (64, 16, 16)      worst at u = 1.4588, 3779.2, 2.0456

The worst points of the normal pair sit where scipy.special.erfcx itself is worst (small |u|).  `measured_K()` recomputes the
table in every run and refuses a numpy statement that is more than 4 units above it.
"""
import mpmath as mp
import numpy as np
import scipy.sparse as sp
import scipy.special as special

import atom_reference as ar

OP_LOG_NORMCDF, OP_NORMCDF, OP_LOGGAMMA = 14, 15, 16
OPS = [OP_LOG_NORMCDF, OP_NORMCDF, OP_LOGGAMMA]
NAMES = {OP_LOG_NORMCDF: "log_normcdf", OP_NORMCDF: "normcdf", OP_LOGGAMMA: "loggamma"}
EPS = ar.EPS

# worst units of the numpy statement (value, d1, d2), as printed by print_table()
TABLE = {
    OP_LOG_NORMCDF: (10.3, 7.9, 16.1),
    OP_NORMCDF: (7.7, 2.0, 2.6),
    OP_LOGGAMMA: (9.4, 2.3, 3.0),
}

mp.mp.dps = 80


# ---- closed forms --------------------------------------------------------------------------------------------------------------

_normal = {}


def _ncdf(u):
    """(the normal pair shares its grid: one mpmath evaluation of Phi per argument serves both ops)"""
    if u not in _normal:
        _normal[u] = mp.ncdf(u)
    return _normal[u]


def _log_ncdf(u):
    return mp.log(_ncdf(u)) if u <= 0 else mp.log1p(-_ncdf(-u))


def _mills(u):
    return mp.npdf(u) / _ncdf(u)


def special_mp(op, u):
    """-> ([value, d1, d2], [their derivatives in u], lambda or None) as mpmath numbers."""
    x = mp.mpf(float(u))
    if op == OP_LOG_NORMCDF:
        lam = _mills(x)
        r2 = -lam * (x + lam)
        r3 = -r2 * (x + lam) - lam * (1 + r2)
        return [_log_ncdf(x), lam, r2], [lam, r2, r3], lam
    if op == OP_NORMCDF:
        phi = mp.npdf(x)
        return [_ncdf(x) if x <= 0 else 1 - _ncdf(-x), phi, -x * phi], [phi, -x * phi, (x * x - 1) * phi], None
    if op == OP_LOGGAMMA:
        return [mp.loggamma(x), mp.psi(0, x), mp.psi(1, x)], [mp.psi(0, x), mp.psi(1, x), mp.psi(2, x)], None
    raise ValueError(op)


def _bracket(op, k, x, r, rp, lam):
    if op == OP_LOG_NORMCDF and k == 2:
        return lam * (abs(x) + lam) + abs(x * rp)
    return abs(r) + abs(x * rp)


def in_domain(op, u):
    return bool(np.isfinite(u)) and (u > 0 or op != OP_LOGGAMMA)


def edge_class(op, u):
    """The IEEE class of (value, d1, d2) at and beyond the edges, as DESIGN.md section 2 states it; None = any finite number."""
    if np.isnan(u):
        return (np.nan,) * 3
    if op == OP_LOGGAMMA:
        if u == 0:
            return (np.inf, -np.inf, np.inf)
        return (np.nan,) * 3 if u < 0 else (np.inf, np.inf, 0.0)
    if op == OP_LOG_NORMCDF:
        return (0.0, 0.0, 0.0) if u > 0 else (-np.inf, np.inf, None)
    return (1.0, 0.0, 0.0) if u > 0 else (0.0, 0.0, 0.0)


_points = {}


def _point(op, u):
    """One argument -> ((hi, lo, bracket, status) per output); memoised per (op, u): a grid is evaluated in mpmath once however
    many tapes, segments and tests read it."""
    key = (int(op), float(u).hex())
    if key not in _points:
        if not in_domain(op, u):
            _points[key] = tuple(((0.0 if c is None else c), 0.0, 0.0, 2) for c in edge_class(op, u))
        else:
            x = mp.mpf(float(u))
            r, rp, lam = special_mp(op, u)
            out = []
            for k in range(3):
                if ar._left_out(r[k]):
                    out.append((float(mp.sign(r[k])) * (np.inf if abs(r[k]) > 1 else 0.0), 0.0, 0.0, 1))
                else:
                    out.append(ar._split(r[k]) + (float(_bracket(op, k, x, r[k], rp[k], lam)), 0))
            _points[key] = tuple(out)
    return _points[key]


def special_reference(op, u):
    """hi, lo, bracket (each (3, n): value, d1, d2) and status (3, n) as tests/atom_reference.unary_reference: 0 compare in
    magnitude, 1 left out (mpmath value outside the normal range), 2 edge: hi holds the IEEE class (a finite hi: any finite
    number)."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    n = u.size
    hi, lo, br = np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n))
    st = np.zeros((3, n), dtype=np.int8)
    for i in range(n):
        for k, (h, l, b, s) in enumerate(_point(op, u[i])):
            hi[k, i], lo[k, i], br[k, i], st[k, i] = h, l, b, s
    return hi, lo, br, st


# ---- grids -----------------------------------------------------------------------------------------------------------------------

def grid(op):
    rng = np.random.default_rng(3000 + int(op == OP_LOGGAMMA))
    if op in (OP_LOG_NORMCDF, OP_NORMCDF):            # (one grid for the pair: one mpmath pass of Phi and phi serves both)
        t = 10.0 ** rng.uniform(-8, 0, 400)
        return np.concatenate([rng.uniform(-37, 37, 3000), rng.uniform(-8, 8, 3000), rng.uniform(-1, 1, 500), t[:200], -t[200:],
                               [0.0, 37.0, -37.0, -36.5, 8.3, 5.0, -5.0]])
    if op == OP_LOGGAMMA:
        return np.concatenate([10.0 ** rng.uniform(-6, 6, 4000), rng.uniform(0.5, 3, 2000),
                               [1.0, 2.0, 1.4616321449683623, 1e-6, 1e6, 0.5, 3.0, 171.7, 172.0]])
    raise ValueError(op)


# edges and beyond: (argument, what is compared) -- "mp": against mpmath like any grid point, "class": edge_class
FAR_LEFT = [-40.0, -1e3, -1e8]
FAR_RIGHT = [40.0, 1e3, np.inf]


# ---- the independent statement ---------------------------------------------------------------------------------------------------

_RT_HALF = np.sqrt(0.5)
_RT_2_OVER_PI = np.sqrt(2.0 / np.pi)


def numpy_rules(op, u):
    """(value, d1, d2) by the formulas of DESIGN.md section 2 over scipy.special (erfcx, gammaln, psi, polygamma)."""
    u = np.asarray(u, dtype=float)
    with np.errstate(all="ignore"):
        if op == OP_LOG_NORMCDF:
            neg = u <= 0
            un, up = np.where(neg, u, 0.0), np.where(neg, 0.0, u)
            E = special.erfcx(-un * _RT_HALF)
            g = np.exp(-0.5 * up * up)
            gE = g * special.erfcx(up * _RT_HALF)
            val = np.where(neg, np.log(0.5 * E) - 0.5 * un * un, np.log1p(-0.5 * gE))
            lam = np.where(neg, _RT_2_OVER_PI / E, _RT_2_OVER_PI * g / (2.0 - gE))
            return val, lam, -lam * (u + lam)
        if op == OP_NORMCDF:
            g = np.exp(-0.5 * u * u)
            tail = 0.5 * g * special.erfcx(np.abs(u) * _RT_HALF)
            phi = g / np.sqrt(2.0 * np.pi)
            return np.where(u <= 0, tail, 1.0 - tail), phi, -u * phi
        if op == OP_LOGGAMMA:
            return special.gammaln(u), special.psi(u), special.polygamma(1, u)
    raise ValueError(op)


def worst_ratios(rules, op, u):
    """`rules(op, u)` -> (value, d1, d2) against mpmath: per output the worst |error| in units of eps * bracket, its argument,
    the arguments with a wrong IEEE class, and the number of points left out."""
    hi, lo, br, st = special_reference(op, u)
    got = [np.asarray(g, float) * np.ones(u.size) for g in rules(op, u)]
    worst, where, bad, left = [0.0] * 3, [None] * 3, [[], [], []], [0] * 3
    for k in range(3):
        left[k] = int(np.sum(st[k] == 1))
        for i in range(u.size):
            g = got[k][i]
            if st[k, i] == 1:
                if np.isnan(g):
                    bad[k].append(float(u[i]))
                continue
            if not np.isfinite(g):
                bad[k].append(float(u[i]))
                continue
            err = abs((g - hi[k, i]) - lo[k, i])
            ratio = 0.0 if err == 0.0 else (np.inf if br[k, i] == 0.0 else err / (EPS * br[k, i]))
            if ratio > worst[k]:
                worst[k], where[k] = ratio, float(u[i])
    return worst, where, bad, left


_K = {}


def measured_table():
    if "table" not in _K:
        _K["table"] = {op: worst_ratios(numpy_rules, op, grid(op)) for op in OPS}
    return _K["table"]


def measured_K():
    """{op: (K value, K d1, K d2)}."""
    if "K" not in _K:
        out = {}
        for op, (worst, where, bad, left) in measured_table().items():
            # a numpy statement that is itself wrong must not widen the bound the host and device builds are held to
            for k in range(3):
                assert worst[k] <= TABLE[op][k] + 4.0, ("numpy statement of %s, output %d: %.1f units of eps * bracket at u = %r; "
                                                        "the table says %.1f" % (NAMES[op], k, worst[k], where[k], TABLE[op][k]))
            out[op] = tuple(ar._to_K(w) for w in worst)
        _K["K"] = out
    return _K["K"]


def print_table():
    for op, (worst, where, bad, left) in measured_table().items():
        print("%-14s %6.1f %6.1f %6.1f   K %s  at u = %r  left out %r  wrong class %s" %
              ((NAMES[op],) + tuple(worst) + (tuple(ar._to_K(w) for w in worst), where, left, [b[:3] for b in bad])))


# ---- a tape of flat unary segments in mpmath -------------------------------------------------------------------------------------

def _arg(a, s):
    off, ln = int(a["seg_a0_off"][s]), int(a["seg_a0_len"][s])
    return np.asarray(a["gidx"][off:off + ln], dtype=np.int64)


def reference_sweep(a, x, w=None):
    """z, dvals and (with the weights w of the z entries) hvals of a tape whose segments are all ops 14 - 16, every unit from
    the closed forms above, as tests/atom_reference.Units."""
    K = measured_K()
    Z, nseg, nd, nh = (int(a["dims"][i]) for i in (2, 3, 4, 5))
    z, dv, hv = ar.Units(Z), ar.Units(nd), ar.Units(nh if w is not None else 0)
    for s in range(nseg):
        op, n = int(a["seg_op"][s]), int(a["seg_n"][s])
        assert op in OPS, op
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        u = x[_arg(a, s)]
        hi, lo, br, st = special_reference(op, u)
        for k, (dst, off) in enumerate(((z, zo), (dv, do), (hv, ho))):
            if k == 2 and w is None:
                continue
            scale = np.ones(n) if k < 2 else np.asarray(w[zo:zo + n], float)
            sl = slice(off, off + n)
            with np.errstate(all="ignore"):
                dst.hi[sl], dst.lo[sl] = scale * hi[k], scale * lo[k]
            dst.st[sl] = st[k]
            dst.tol[sl] = np.abs(scale) * K[op][k] * EPS * br[k]
            for i in range(n):
                dst.who[off + i] = (s, NAMES[op], (float(u[i]),))
    return z, dv, hv


def expected_oracles(a, x, lam=None, sigma=1.0):
    """{'f', 'grad_f', 'g', 'jac', 'hess'} -> tests/atom_reference.Entries for the tape `a` at x (Hessian of sigma f + lam' g)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = ar._csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], np.zeros(m) if lam is None else np.asarray(lam, float)])
    z, dv, hv = reference_sweep(a, x, w)
    c = np.asarray(a["c"], float)
    G = ar._csr(a, "G", (m, N + Z)).tocsc()
    return {
        "f": ar.Entries(np.asarray(a["c0"], float)[:1], sp.csr_matrix(c[None, :N]), x, sp.csr_matrix(c[None, N:]), z, "f"),
        "grad_f": ar.Entries(c[:N], None, x, ar._csr(a, "Mg", (N, nd)), dv, "grad_f"),
        "g": ar.Entries(a["b"], G[:, :N].tocsr(), x, G[:, N:].tocsr(), z, "g"),
        "jac": ar.Entries(a["Jc"], None, x, ar._csr(a, "MJ", (nnzJ, nd)), dv, "jac"),
        "hess": ar.Entries(None, None, x, ar._csr(a, "MH", (nnzH, nh)), hv, "hess"),
        "units": (z, dv, hv),
    }
