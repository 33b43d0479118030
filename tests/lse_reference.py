"""TEST INFRASTRUCTURE -- log_sum_exp restated in mpmath (80 digits), the seeded rows and the error bound.

Scheme of tests/atom_reference.py.  For one row u of length n, with r = log sum_l exp(u_l), p_i = exp(u_i - r) and
h_ij = w (delta_ij p_i - p_i p_j), all in closed form at 80 digits (no numerical differentiation), an evaluator is held
to, with eps = 2^-53 and s = (n + 2) eps (the textbook bound of a sum of n rounded terms in any order):

    value   |got - r|      <= Kv eps (|r| + sum_i p_i |u_i|)                    + s
    d1      |got - p_i|    <= Kd eps p_i (1 + |u_i - r|)                        + s p_i
    d2 i=j  |got - h_ii|   <= Kh eps |w| p_i (1 + |u_i - r|)                    + s |w| p_i
    d2 i>j  |got - h_ij|   <= Kh eps |w| p_i p_j (2 + |u_i - r| + |u_j - r|)    + 2 s |w| p_i p_j

The diagonal bound is absolute in p_i, not in p_i (1 - p_i): p - p^2 cancels as p -> 1, and no evaluation order avoids
that.  An entry of g / J / H / f / grad f that the tape's constant maps build from several of these gets the sum of its
terms' bounds plus the summation bound of the map's own additions (`expected_oracles`).

A point is left out of the magnitude comparison only when its mpmath value lies outside the normal double range
(0 < |v| < 2.3e-308 or |v| > 1.7e308), decided from mpmath alone; there the result must still not be NaN.  An exact zero
(n = 1: h = 0; a row entry of -inf: p = 0) is compared.  At most 2 % of an output's points may be left out.

K is measured, not chosen: `measured_K()` runs `numpy_rule` below (independent text: a plain max-shifted statement over
numpy's pairwise sums and glibc's exp / log) against mpmath on the grid and returns 4 x the worst ratio -- the error
beyond the summation term, in units of eps * bracket -- rounded up to a power of two, never below 8.  The factor 4 is for
the device math library and FMA contraction.  A numpy statement more than 4 units off is refused.  Measured with

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import lse_reference as lr; lr.print_table()"

on the grid below (seed 2301):

    output        worst units   K    left out
    value              0.24     8    0.000 %
    d1                 0.91     8    0.065 %
    d2 diagonal        0.91     8    0.065 %
    d2 off-diag        0.84     8    0.012 %

(left out: the six entries beside the one that lies 745 above them, whose p is below the normal range.)

Grid: row lengths 1, 2, 3, 7, 16, 33, 64, 65 (40 rows each) and 257 (6 rows); row = shift + scale * N(0,1) with
scale = 10^U(-3, 2) and shift = N(0,1) * 10^U(-2, 2.5); planted rows: all entries equal, one entry 745 above the rest,
entries near +-700, a row containing -inf.
"""
import mpmath as mp          # a dependency of torch's sympy; a missing mpmath is an error, never a skip
import numpy as np
import scipy.sparse as sp

mp.mp.dps = 80
EPS = 2.0 ** -53
NORMAL_MAX = 1.7e308
NORMAL_MIN = 2.3e-308
LEFT_OUT_SHARE = 0.02
SEED = 2301
ROW_LENGTHS = (1, 2, 3, 7, 16, 33, 64, 65, 257)
OP_LOG_SUM_EXP = 34
KINDS = ("value", "d1", "d2 diagonal", "d2 off-diag")


def rows_of_length(n, count=None, seed=SEED):
    """The seeded random rows of one length: (count, n)."""
    count = (40 if n <= 65 else 6) if count is None else count
    rng = np.random.default_rng([seed, n])
    scale = 10.0 ** rng.uniform(-3, 2, (count, 1))
    shift = rng.standard_normal((count, 1)) * 10.0 ** rng.uniform(-2, 2.5, (count, 1))
    return shift + scale * rng.standard_normal((count, n))


def planted_rows():
    """Few enough that the 2 % cap holds (asserted by the tests): rows of length 7."""
    return np.array([
        [3.25] * 7,                                              # all entries equal: p = 1/7
        [745.0 + 1.5, 1.5, 1.0, 0.5, 2.0, 1.25, 0.0],            # one entry 745 above the rest: the others' p underflow
        [700.0, 699.5, 698.0, 700.25, 699.0, 697.0, 700.0],      # near +700: a sum of exp(u) overflows
        [-700.0, -699.5, -698.0, -700.25, -699.0, -697.0, -700.0],
        [0.5, -np.inf, 1.5, 0.25, -0.75, 1.0, 0.0],              # a row containing -inf: p there is 0
    ])


def grid():
    """-> list of (n, rows) in the order the tapes hold them."""
    return [(n, rows_of_length(n)) for n in ROW_LENGTHS] + [(7, planted_rows())]


def numpy_rule(u, w=1.0):
    """The rule in numpy for ONE row: r, p (n), h (n(n+1)/2, tril_indices order)."""
    u = np.asarray(u, dtype=float)
    with np.errstate(all="ignore"):
        mx = np.max(u)
        e = np.exp(u - mx)
        S = np.sum(e)
        r = mx + np.log(S)
        p = e / S
        ii, jj = np.tril_indices(u.size)
        h = w * np.where(ii == jj, p[ii] - p[ii] * p[jj], -(p[ii] * p[jj]))
    return r, p, h


def row_mp(u):
    """-> (r, [p_i]) as mpmath numbers."""
    xs = [mp.mpf(float(v)) if np.isfinite(v) else (mp.mpf("-inf") if v < 0 else mp.mpf("inf")) for v in u]
    mx = max(xs)
    S = mp.fsum(mp.exp(v - mx) if v != mp.mpf("-inf") else mp.mpf(0) for v in xs)
    r = mx + mp.log(S)
    return r, [mp.exp(v - r) if v != mp.mpf("-inf") else mp.mpf(0) for v in xs]


def _status(v):
    """0: compare; 1: outside the normal double range (mpmath alone decides)."""
    a = abs(v)
    return 1 if (a > NORMAL_MAX or (a != 0 and a < NORMAL_MIN)) else 0


class Units:
    """Reference values of one output kind: hi (float64 of the mpmath value), bracket (the bound's K-term without K eps),
    sterm (the summation term, complete), st (0 compare / 1 left out)."""

    def __init__(self, n):
        self.hi, self.bracket, self.sterm = np.zeros(n), np.zeros(n), np.zeros(n)
        self.st = np.zeros(n, dtype=np.int8)


def row_reference(u, w=1.0, hsel=None):
    """Units of value (1), d1 (n) and d2 (n(n+1)/2 in tril_indices order, or the packed positions `hsel` only) of one row;
    w is the row's Hessian weight, taken as given."""
    u = np.asarray(u, dtype=float)
    n = u.size
    s = (n + 2) * EPS
    r, p = row_mp(u)
    fin = np.isfinite(u)
    dist = [abs(mp.mpf(float(v)) - r) if f else mp.mpf(0) for v, f in zip(u, fin)]      # (p = 0 there: the term vanishes)
    V, D = Units(1), Units(n)
    V.hi[0], V.st[0] = float(r), _status(r)
    V.bracket[0] = float(abs(r) + mp.fsum(pi * abs(mp.mpf(float(v))) for pi, v, f in zip(p, u, fin) if f))
    V.sterm[0] = s
    for i in range(n):
        D.hi[i], D.st[i] = float(p[i]), _status(p[i])
        D.bracket[i] = float(p[i] * (1 + dist[i]))
        D.sterm[i] = s * float(p[i])
    if hsel is None:
        ii, jj = np.tril_indices(n)
    else:
        hsel = np.asarray(hsel, dtype=np.int64)
        ii = ((np.sqrt(8.0 * hsel + 1.0) - 1.0) * 0.5).astype(np.int64)
        ii -= (ii * (ii + 1) // 2 > hsel)
        ii += ((ii + 1) * (ii + 2) // 2 <= hsel)
        jj = hsel - ii * (ii + 1) // 2
    H = Units(ii.size)
    H.diag = ii == jj
    wm, aw = mp.mpf(float(w)), abs(float(w))
    for k, (i, j) in enumerate(zip(ii, jj)):
        if i == j:
            v = wm * (p[i] - p[i] * p[i])
            H.bracket[k] = aw * float(p[i] * (1 + dist[i]))
            H.sterm[k] = s * aw * float(p[i])
        else:
            v = -wm * p[i] * p[j]
            H.bracket[k] = aw * float(p[i] * p[j] * (2 + dist[i] + dist[j]))
            H.sterm[k] = 2 * s * aw * float(p[i] * p[j])
        H.hi[k], H.st[k] = float(v), _status(v)
    return V, D, H


_table = None


def measured_table():
    """kind -> (worst units, where, share left out, wrong NaN count) of `numpy_rule` on the grid."""
    global _table
    if _table is not None:
        return _table
    worst = {k: [0.0, None, 0, 0, 0] for k in KINDS}        # units, where, left out, total, NaN where a number is due
    for n, rows in grid():
        for ridx, u in enumerate(rows):
            V, D, H = row_reference(u, 1.0)
            r, p, h = numpy_rule(u, 1.0)
            parts = [("value", V, np.array([r]), slice(None)), ("d1", D, p, slice(None)),
                     ("d2 diagonal", H, h, H.diag), ("d2 off-diag", H, h, ~H.diag)]
            for kind, U, got, sel in parts:
                hi, br, stm, st, g = U.hi[sel], U.bracket[sel], U.sterm[sel], U.st[sel], got[sel]
                acc = worst[kind]
                acc[2] += int(np.sum(st == 1))
                acc[3] += st.size
                acc[4] += int(np.sum(np.isnan(g)))
                cmp = st == 0
                err = np.maximum(np.abs(g[cmp] - hi[cmp]) - stm[cmp] - EPS * np.abs(hi[cmp]), 0.0)
                with np.errstate(all="ignore"):
                    units = np.where(err > 0, err / (EPS * br[cmp]), 0.0)
                if units.size and np.nanmax(units) > acc[0]:
                    acc[0], acc[1] = float(np.nanmax(units)), (n, ridx)
    _table = {k: (v[0], v[1], v[2] / max(v[3], 1), v[4]) for k, v in worst.items()}
    return _table


def measured_K():
    """kind -> K: 4 x the worst ratio, rounded up to a power of two, never below 8; refuses a statement > 4 units off."""
    out = {}
    for kind, (units, where, share, nans) in measured_table().items():
        if units > 4.0 or nans:
            raise AssertionError("numpy statement of log_sum_exp: %s is %.2f units off at %r (%d NaN)" % (kind, units, where, nans))
        k = 8
        while k < 4.0 * units:
            k *= 2
        out[kind] = k
    return out


def print_table():
    K = measured_K()
    print("    output        worst units   K    left out")
    for kind, (units, where, share, nans) in measured_table().items():
        print("    %-14s %8.2f  %4d    %.3f %%" % (kind, units, K[kind], 100 * share))


class Entries:
    """Expected values of one callback with a bound per entry; `check(got)` asserts."""

    def __init__(self, name, hi, bound, st):
        self.name, self.hi, self.bound, self.st = name, np.asarray(hi), np.asarray(bound), np.asarray(st)

    def check(self, got):
        got = np.asarray(got, dtype=float).reshape(-1)
        assert got.size == self.hi.size, "%s: %d entries for %d" % (self.name, got.size, self.hi.size)
        assert not np.isnan(got).any(), "%s: NaN at %r" % (self.name, np.nonzero(np.isnan(got))[0][:8])
        cmp = self.st == 0
        err = np.abs(got - self.hi)
        bad = cmp & ~(err <= self.bound)
        if bad.any():
            k = int(np.argmax(np.where(bad, err / np.maximum(self.bound, 1e-320), 0.0)))
            raise AssertionError("%s: %d of %d entries beyond the bound; worst at %d: got %r, expected %r, |error| %.3e, bound %.3e"
                                 % (self.name, int(bad.sum()), got.size, k, got[k], self.hi[k], err[k], self.bound[k]))
        sel = cmp & (self.bound > 0)
        return float(np.max(err[sel] / self.bound[sel])) if sel.any() else 0.0


def _csr(a, name, shape):
    return sp.csr_matrix((a[name + "_val"], a[name + "_idx"], a[name + "_ptr"]), shape=shape)


def weights(a, lam, sigma):
    """w = Mw [sigma; lam]: the tape's own pull-back of the multipliers, in double (taken as given by the bound)."""
    N, m, Z = (int(v) for v in a["dims"][:3])
    return _csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])


def reference_sweep(a, x, w, hsample=None, seed=SEED):
    """Units of z, dvals, hvals of a tape whose segments are all log_sum_exp; for rows longer than 257 only `hsample`
    seeded Hessian entries per row are referenced (the others get st = 2: not compared, not counted)."""
    K = measured_K()
    N, m, Z, nseg, nd, nh = (int(v) for v in a["dims"][:6])
    z, d, h = Units(Z), Units(nd), Units(nh)
    h.st[:] = 2
    for u_ in (z, d, h):
        u_.bound = np.zeros(u_.hi.size)
    rng = np.random.default_rng([seed, 77])
    for s in range(nseg):
        assert int(a["seg_op"][s]) == OP_LOG_SUM_EXP
        M, L = int(a["seg_d0"][s]), int(a["seg_d1"][s])
        T = L * (L + 1) // 2
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + M * L], dtype=np.int64).reshape(M, L)
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        for r in range(M):
            hsel = None
            if L > 257 and hsample is not None:
                hsel = np.unique(np.concatenate([[0, T - 1], rng.integers(0, T, hsample)]))
            V, D, H = row_reference(x[idx[r]], w[zo + r], hsel)
            pos = ho + r * T + (np.arange(T) if hsel is None else hsel)
            for dst, src, at, kk in ((z, V, np.array([zo + r]), K["value"]), (d, D, do + r * L + np.arange(L), K["d1"])):
                dst.hi[at], dst.st[at] = src.hi, src.st
                dst.bound[at] = kk * EPS * src.bracket + src.sterm + EPS * np.abs(src.hi)
            kh = np.where(H.diag, K["d2 diagonal"], K["d2 off-diag"])
            h.hi[pos], h.st[pos] = H.hi, H.st
            h.bound[pos] = kh * EPS * H.bracket + H.sterm + EPS * np.abs(H.hi)
    return z, d, h


def _through(Mx, base, v, name):
    """base + Mx @ v.hi with the bound |Mx| @ v.bound + (terms + 2) eps (|base| + |Mx| @ |v.hi|); an entry that reads a unit
    outside the normal range, or an unreferenced one, is not compared."""
    A = abs(Mx)
    ok = np.where(v.st == 0, 1.0, 0.0)
    with np.errstate(all="ignore"):
        hi = base + Mx @ np.where(v.st == 0, v.hi, 0.0)
        terms = np.diff(Mx.indptr) + 2
        bound = A @ (v.bound * ok) + terms * EPS * (np.abs(base) + A @ np.abs(np.where(v.st == 0, v.hi, 0.0)))
    touched_bad = (A.astype(bool).astype(float) @ (1.0 - ok)) > 0
    return Entries(name, hi, bound, np.where(touched_bad, 1, 0))


def expected_oracles(a, x, lam, sigma, hsample=None):
    """g, jac, hess, f, grad_f of a tape of log_sum_exp segments as Entries, through the tape's own constant maps."""
    x = np.asarray(x, dtype=float)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = weights(a, lam, sigma)
    z, d, h = reference_sweep(a, x, w, hsample)
    G = _csr(a, "G", (m, N + Z))
    Gx, Gz = sp.csr_matrix(G[:, :N]), sp.csr_matrix(G[:, N:])
    c = np.asarray(a["c"], dtype=float)
    out = {"units": (z, d, h)}
    finite_x = np.where(np.isfinite(x), x, 0.0)          # (an argument of -inf enters through the atom only)
    out["g"] = _through(Gz, a["b"] + Gx @ finite_x, z, "g")
    fz = _through(sp.csr_matrix(c[N:].reshape(1, -1)), np.array([float(a["c0"][0]) + c[:N] @ finite_x]), z, "f")
    out["f"] = fz
    out["grad_f"] = _through(_csr(a, "Mg", (N, nd)), c[:N], d, "grad_f")
    out["jac"] = _through(_csr(a, "MJ", (nnzJ, nd)), np.asarray(a["Jc"], dtype=float), d, "jac")
    out["hess"] = _through(_csr(a, "MH", (nnzH, nh)), np.zeros(nnzH), h, "hess")
    return out
