"""TEST INFRASTRUCTURE -- prod restated in mpmath (80 digits), the seeded rows and the error bound.

For one row u of length K the reference is the definition, not the evaluators' rule: the value is the product of the
entries, g_i the product of all entries but u_i, h_ij (i > j) the product of all entries but u_i and u_j, times the
row's weight w.  With zeros in the row these are taken by cases on where the zeros stand, so no reference value ever
divides by zero, and a value that is 0 is an exact 0.

The bound is derived, not measured.  Correctly rounded, a value is K - 1 multiplications, a first derivative one more
division, a second derivative two, so with eps = 2^-53 and gamma(n) = n eps / (1 - n eps)

    |got - ref| <= gamma(K + 1) |ref|        for every z, d and h entry,

(the multiplication of h by the row's weight is not counted: the tests' weights are powers of two, tests/lse_problems.py
`multipliers`, so it is exact)
whatever the order of the multiplications.  The comparison is made against the mpmath value itself: it is kept as a
double pair (hi, lo) with ref = hi + lo to 106 bits, and the bound is rounded towards zero.  An exact zero in the
reference must be an exact zero.

An entry of g / J / H / f / grad f that the tape's constant maps build from several of these gets the sum of its terms'
bounds plus the summation bound of the map's own ROUNDED operations (`_through`): a term with coefficient +-1 is not
rounded, nor is the addition to a zero base, so an entry that is +-(one z, d or h) is held to the bound above unchanged.

Left out of the magnitude comparison: a point whose mpmath value, or whose row's mpmath P0 (the product of the nonzero
entries), lies outside the normal double range -- decided from mpmath alone; there the result must still not be NaN.
At most 2 % of an output's points may be left out.

Grid: row lengths 1, 2, 3, 7, 16, 33, 64, 65 (40 rows each) and 257 (6 rows); entries +-10^(sigma N(0,1)) with
sigma = min(1.5, 60 / sqrt(K)), so that log10 |P0| has a standard deviation of at most 60 against a range of 308;
planted rows with 0, 1, 2 and 3 zeros in first, middle and last position, negative entries, all ones.
"""
import mpmath as mp          # a dependency of torch's sympy; a missing mpmath is an error, never a skip
import numpy as np
import scipy.sparse as sp

mp.mp.dps = 80
EPS = 2.0 ** -53
NORMAL_MAX = 1.7e308
NORMAL_MIN = 2.3e-308
LEFT_OUT_SHARE = 0.02
SEED = 2302
ROW_LENGTHS = (1, 2, 3, 7, 16, 33, 64, 65, 257)
OP_PROD = 35


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


def sigma_of(K):
    return min(1.5, 60.0 / np.sqrt(K))


def rows_of_length(K, count=None, seed=SEED):
    """The seeded random rows of one length: (count, K), entries +-10^(sigma N(0,1))."""
    count = (40 if K <= 65 else 6) if count is None else count
    rng = np.random.default_rng([seed, K])
    mag = 10.0 ** (sigma_of(K) * rng.standard_normal((count, K)))
    return np.where(rng.random((count, K)) < 0.5, -mag, mag)


def planted_rows():
    """Rows of length 7: no zero, one / two / three zeros in first, middle and last position, negative entries, ones."""
    base = np.array([1.5, -2.25, 0.75, 3.0, -0.5, 1.25, 2.0])
    rows = [base.copy(), np.ones(7), -base]
    for zeros in ([0], [3], [6], [0, 3], [3, 6], [0, 6], [0, 3, 6], [0, 1, 2], [4, 5, 6]):
        r = base.copy()
        r[zeros] = 0.0
        rows.append(r)
    return np.array(rows)


def grid():
    """-> list of (K, rows) in the order the tapes hold them."""
    return [(K, rows_of_length(K)) for K in ROW_LENGTHS] + [(7, planted_rows())]


def numpy_rule(u, w=1.0):
    """The evaluators' rule in numpy for ONE row: z, g (K), h (K (K - 1) / 2, tril_indices(K, -1) order)."""
    u = np.asarray(u, dtype=float)
    zero = u == 0
    nz = int(zero.sum())
    P0 = float(np.prod(u[~zero])) if nz < u.size else 1.0
    Z0 = P0 if P0 != P0 else 0.0
    safe = np.where(zero, 1.0, u)
    with np.errstate(all="ignore"):
        z = P0 if nz == 0 else Z0
        g = P0 / safe if nz == 0 else np.where(zero & (nz == 1), P0, Z0)
        ii, jj = np.tril_indices(u.size, -1)
        h = np.where(~zero[jj], g[ii] / safe[jj], np.where(~zero[ii], g[jj] / safe[ii], P0 if nz == 2 else Z0))
    return z, g, w * h


def strict_decode(q):
    """Packed positions of the strict lower triangle -> (i, j), i > j."""
    q = np.asarray(q, dtype=np.int64)
    i = ((np.sqrt(8.0 * q + 1.0) - 1.0) * 0.5).astype(np.int64)
    i -= (i * (i + 1) // 2 > q)
    i += ((i + 1) * (i + 2) // 2 <= q)
    return i + 1, q - i * (i + 1) // 2


def _mpf(v):
    v = float(v)
    return mp.mpf(v) if np.isfinite(v) else (mp.mpf("nan") if v != v else mp.mpf("inf") * (1 if v > 0 else -1))


def _outside(v):
    a = abs(v)
    return a > NORMAL_MAX or (a != 0 and a < NORMAL_MIN)


class Units:
    """Reference values of one output kind: ref = hi + lo (double pair of the mpmath value), bound = gamma |ref| rounded
    towards zero, st (0 compare / 1 left out / 2 not referenced)."""

    def __init__(self, n):
        self.hi, self.lo, self.bound = np.zeros(n), np.zeros(n), np.zeros(n)
        self.st = np.zeros(n, dtype=np.int8)

    def put(self, k, v, nops, row_out):
        hi = float(v)
        self.hi[k] = hi
        self.lo[k] = float(v - mp.mpf(hi)) if np.isfinite(hi) else 0.0
        self.st[k] = 1 if (row_out or _outside(v)) else 0
        b = float(gamma(nops) * abs(v)) if np.isfinite(hi) else 0.0
        self.bound[k] = np.nextafter(b, 0.0)

    def error(self, got):
        """|got - ref| per entry (got - hi is exact where it matters: the two are within a factor of two)."""
        with np.errstate(all="ignore"):
            return np.abs((np.asarray(got, dtype=float) - self.hi) - self.lo)


def row_reference(u, w=1.0, hsel=None):
    """Units of value (1), d1 (K) and d2 (K (K - 1) / 2 in tril_indices(K, -1) order, or the packed positions `hsel` only)
    of one row; w is the row's Hessian weight, taken as given."""
    u = np.asarray(u, dtype=float)
    K = u.size
    xs = [_mpf(v) for v in u]
    zpos = [k for k, v in enumerate(u) if v == 0]
    nz = len(zpos)
    P0 = mp.mpf(1)
    for k, v in enumerate(xs):
        if u[k] != 0:
            P0 *= v
    out = _outside(P0)
    V, D = Units(1), Units(K)
    V.put(0, P0 if nz == 0 else mp.mpf(0), K + 1, out)
    for i in range(K):
        if nz == 0:
            v = P0 / xs[i]
        else:
            v = P0 if (nz == 1 and zpos[0] == i) else mp.mpf(0)
        D.put(i, v, K + 1, out)
    if hsel is None:
        ii, jj = np.tril_indices(K, -1)
    else:
        ii, jj = strict_decode(hsel)
    H = Units(ii.size)
    wm = mp.mpf(float(w))
    zs = set(zpos)
    for k, (i, j) in enumerate(zip(ii.tolist(), jj.tolist())):
        if nz == 0:
            v = P0 / (xs[i] * xs[j])
        elif not zs <= {i, j}:
            v = mp.mpf(0)
        elif nz == 2:
            v = P0
        else:
            v = P0 / (xs[j] if i in zs else xs[i])
        H.put(k, wm * v, K + 1, out)
    return V, D, H


def check_units(name, U, got):
    """Assert one output kind of one or more rows; -> the worst error as a share of its bound."""
    got = np.asarray(got, dtype=float).reshape(-1)
    assert got.size == U.hi.size, "%s: %d entries for %d" % (name, got.size, U.hi.size)
    ref = U.st != 2
    assert not np.isnan(got[ref]).any(), "%s: NaN at %r" % (name, np.nonzero(np.isnan(got) & ref)[0][:8])
    cmp = U.st == 0
    err = U.error(got)
    bad = cmp & ~(err <= U.bound)
    if bad.any():
        k = int(np.argmax(np.where(bad, err / np.maximum(U.bound, 1e-320), 0.0)))
        raise AssertionError("%s: %d of %d entries beyond the bound; worst at %d: got %r, expected %r, |error| %.3e, bound %.3e"
                             % (name, int(bad.sum()), got.size, k, got[k], U.hi[k], err[k], U.bound[k]))
    sel = cmp & (U.bound > 0)
    return float(np.max(err[sel] / U.bound[sel])) if sel.any() else 0.0


def numpy_table():
    """The numpy statement of the rule against mpmath on the grid: kind -> (worst error in eps relative, left-out share,
    points).  Asserts the bound."""
    acc = {"value": [0.0, 0, 0], "d1": [0.0, 0, 0], "d2": [0.0, 0, 0]}
    for K, rows in grid():
        for u in rows:
            V, D, H = row_reference(u, 1.0)
            z, g, h = numpy_rule(u, 1.0)
            for kind, U, got in (("value", V, [z]), ("d1", D, g), ("d2", H, h)):
                check_units("numpy statement, K = %d, %s" % (K, kind), U, got)
                cmp = (U.st == 0) & (U.hi != 0)
                a = acc[kind]
                if cmp.any():
                    a[0] = max(a[0], float(np.max(U.error(got)[cmp] / np.abs(U.hi[cmp]))) / EPS)
                a[1] += int(np.sum(U.st == 1))
                a[2] += U.st.size
    return {k: (v[0], v[1] / max(v[2], 1), v[2]) for k, v in acc.items()}


# ---- through the tape's constant maps --------------------------------------------------------------------------------------------
class Entries:
    """Expected values of one callback with a bound per entry; `check(got)` asserts."""

    def __init__(self, name, hi, lo, bound, st):
        self.name, self.hi, self.lo, self.bound, self.st = name, np.asarray(hi), np.asarray(lo), np.asarray(bound), np.asarray(st)

    def check(self, got):
        U = Units(self.hi.size)
        U.hi, U.lo, U.bound, U.st = self.hi, self.lo, self.bound, self.st
        return check_units(self.name, U, got)


def _csr(a, name, shape):
    return sp.csr_matrix((a[name + "_val"], a[name + "_idx"], a[name + "_ptr"]), shape=shape)


def weights(a, lam, sigma):
    """w = Mw [sigma; lam]: the tape's own pull-back of the multipliers, in double (taken as given by the bound)."""
    N, m, Z = (int(v) for v in a["dims"][:3])
    return _csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], lam])


def reference_sweep(a, x, w, hsample=None, seed=SEED):
    """Units of z, dvals, hvals of a tape whose segments are all prod; for rows longer than 257 only `hsample` seeded
    Hessian entries per row are referenced (the others get st = 2: not compared, not counted)."""
    N, m, Z, nseg, nd, nh = (int(v) for v in a["dims"][:6])
    z, d, h = Units(Z), Units(nd), Units(nh)
    h.st[:] = 2
    rng = np.random.default_rng([seed, 77])
    for s in range(nseg):
        assert int(a["seg_op"][s]) == OP_PROD
        M, L = int(a["seg_d0"][s]), int(a["seg_d1"][s])
        T = L * (L - 1) // 2
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + M * L], dtype=np.int64).reshape(M, L)
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        for r in range(M):
            hsel = None
            if L > 257 and hsample is not None:
                hsel = np.unique(np.concatenate([[0, T - 1], rng.integers(0, T, hsample)]))
            V, D, H = row_reference(x[idx[r]], w[zo + r], hsel)
            pos = ho + r * T + (np.arange(T) if hsel is None else hsel)
            for dst, src, at in ((z, V, np.array([zo + r])), (d, D, do + r * L + np.arange(L)), (h, H, pos)):
                dst.hi[at], dst.lo[at], dst.st[at], dst.bound[at] = src.hi, src.lo, src.st, src.bound
    return z, d, h


def _through(Mx, base, base_ops, v, name):
    """base + Mx @ v with the bound |Mx| @ v.bound + gamma(ops) (|base| + |Mx| @ |v|), ops = the ROUNDED operations of the
    entry: one per term whose coefficient is not +-1, one per addition beyond the first term, one for a non-zero base
    and `base_ops` for what built the base.  An entry that reads a unit outside the normal range, or an unreferenced one,
    is not compared."""
    Mx = sp.csr_matrix(Mx)
    A = abs(Mx)
    ok = np.where(v.st == 0, 1.0, 0.0)
    with np.errstate(all="ignore"):
        vhi, vlo = np.where(v.st == 0, v.hi, 0.0), np.where(v.st == 0, v.lo, 0.0)
        hi = base + Mx @ vhi
        lo = Mx @ vlo
        terms = np.diff(Mx.indptr)
        scaled = sp.csr_matrix((np.where(np.abs(Mx.data) == 1.0, 0.0, 1.0), Mx.indices, Mx.indptr), shape=Mx.shape)
        ops = np.asarray(scaled.sum(axis=1)).reshape(-1) + np.maximum(terms - 1, 0) + np.where(base != 0, 1 + base_ops, 0)
        # (hi itself is a rounded sum of `ops` operations when ops > 0: one more unit covers the reference's own rounding)
        ops = np.where(ops > 0, ops + 1, 0)
        bound = A @ (v.bound * ok) + gamma(ops) * (np.abs(base) + A @ np.abs(vhi))
    touched_bad = (A.astype(bool).astype(float) @ (1.0 - ok)) > 0
    return Entries(name, hi, lo, bound, np.where(touched_bad, 1, 0))


def expected_oracles(a, x, lam, sigma, hsample=None):
    """g, jac, hess, f, grad_f of a tape of prod segments as Entries, through the tape's own constant maps."""
    x = np.asarray(x, dtype=float)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = weights(a, lam, sigma)
    z, d, h = reference_sweep(a, x, w, hsample)
    G = _csr(a, "G", (m, N + Z))
    Gx, Gz = sp.csr_matrix(G[:, :N]), sp.csr_matrix(G[:, N:])
    c = np.asarray(a["c"], dtype=float)
    out = {"units": (z, d, h)}
    out["g"] = _through(Gz, a["b"] + Gx @ x, 2 * np.diff(Gx.indptr), z, "g")
    out["f"] = _through(sp.csr_matrix(c[N:].reshape(1, -1)), np.array([float(a["c0"][0]) + c[:N] @ x]),
                        np.array([2 * int(np.count_nonzero(c[:N]))]), z, "f")
    out["grad_f"] = _through(_csr(a, "Mg", (N, nd)), c[:N], np.zeros(N), d, "grad_f")
    out["jac"] = _through(_csr(a, "MJ", (nnzJ, nd)), np.asarray(a["Jc"], dtype=float), np.zeros(nnzJ), d, "jac")
    out["hess"] = _through(_csr(a, "MH", (nnzH, nh)), np.zeros(nnzH), np.zeros(nnzH), h, "hess")
    return out
