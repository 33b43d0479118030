"""TEST INFRASTRUCTURE -- quad_over_lin_rows restated in mpmath (50 digits), the seeded rows and the error bound.

For one row u of length K with denominator y and Hessian weight w the reference is the definition: ss = sum u_l^2,

    z = ss / y         g_l = 2 u_l / y          g_y = -ss / y^2
    h_ll = 2 w / y     h_ly = -2 w u_l / y^2    h_yy = 2 w ss / y^3

The bound is derived, not measured.  ss is a sum of K non-negative terms -- one rounded multiplication each and at most
K - 1 rounded additions on the way of any term to the total, in whatever order (a contraction to FMA only removes
roundings) -- so the computed ss lies within gamma(K) of the exact one, eps = 2^-53, gamma(n) = n eps / (1 - n eps).
Every further ROUNDED operation adds one (a factor 2 is exact; w is taken as a general double, so a product with it
counts).  The count per output, `OPS`:

    z     K + 1    ss, the division
    g_l   1        the division (2 u_l is exact)
    g_y   K + 2    ss, y y, the division
    h_ll  1        the division (2 w is exact)
    h_ly  3        (2 w) u_l, y y, the division
    h_yy  K + 4    ss, (2 w) ss, y y, (y y) y, the division

All are at most gamma(K + 4), the figure every output is held to in whatever summation order; the per-output counts
above are what the checks use (each is smaller or equal).  The counts hold while no intermediate leaves the normal
double range; the seeded rows keep |u|, |y| in [1e-6, 1e6], far inside it, and `mp_rule` asserts that.

Rows with non-finite entries, y = 0 or y < 0 (`planted`) have no branch in the rule: what IEEE arithmetic gives for the
expressions above is the expected result, stated by `numpy_rule`; an entry that is non-finite there must be the same
non-finite value here (NaN positions equal), every finite one is held to mpmath as above.
"""
import mpmath as mp          # a dependency of torch's sympy; a missing mpmath is an error, never a skip
import numpy as np

mp.mp.dps = 50
EPS = mp.mpf(2) ** -53
SEED = 3602
OP_QUAD_OVER_LIN_ROWS = 36
KINDS = ("z", "g", "gy", "hll", "hyy", "hly")
GRID = ((1, 1), (5, 1), (40, 2), (40, 3), (12, 7), (9, 16), (5, 33), (4, 64), (4, 65), (3, 257))      # (M, K)


def ops(kind, K):
    return {"z": K + 1, "g": 1, "gy": K + 2, "hll": 1, "hly": 3, "hyy": K + 4}[kind]


def gamma(n):
    return n * EPS / (1 - n * EPS)


def rows_of_shape(M, K, seed=SEED):
    """The seeded rows: U (M, K) with entries +-10^(1.5 N(0,1)) clipped to [1e-6, 1e6], y (M) = 10^(N(0,1)) > 0."""
    rng = np.random.default_rng([seed, M, K])
    mag = np.clip(10.0 ** (1.5 * rng.standard_normal((M, K))), 1e-6, 1e6)
    U = np.where(rng.random((M, K)) < 0.5, -mag, mag)
    y = np.clip(10.0 ** rng.standard_normal(M), 1e-6, 1e6)
    return U, y


def grid():
    return [rows_of_shape(M, K) for M, K in GRID]


def planted():
    """Rows of length 3: a NaN entry, an inf entry, y = 0 with ss > 0, y = 0 with ss = 0, y < 0, a clean row."""
    U = np.array([[0.5, np.nan, 2.0], [0.5, np.inf, 2.0], [1.5, -2.0, 0.25], [0.0, 0.0, 0.0], [1.5, -2.0, 0.25], [1.0, 2.0, 3.0]])
    y = np.array([2.0, 0.5, 0.0, 0.0, -4.0, 2.0])
    return U, y


def numpy_rule(U, y, w):
    """The numpy statement of the rule over all rows of U (M, K): kind -> array, IEEE semantics throughout."""
    U, y, w = np.asarray(U, dtype=float), np.asarray(y, dtype=float), np.asarray(w, dtype=float)
    with np.errstate(all="ignore"):
        ss = np.sum(U * U, axis=1)
        yc, wc = y[:, None], w[:, None]
        return {"z": ss / y, "g": 2.0 * U / yc, "gy": -ss / (y * y), "hll": np.broadcast_to(2.0 * wc / yc, U.shape).copy(),
                "hyy": 2.0 * w * ss / (y * y * y), "hly": -2.0 * wc * U / (yc * yc)}


def mp_rule(u, y, w):
    """One row in mpmath: kind -> list of mpf, None where an input of the entry is not finite or y == 0."""
    K = len(u)
    fin = [bool(np.isfinite(v)) for v in u]
    yok = bool(np.isfinite(y)) and y != 0
    us = [mp.mpf(float(v)) if f else None for v, f in zip(u, fin)]
    ym, wm = (mp.mpf(float(y)) if yok else None), mp.mpf(float(w))
    for v in list(u) + [y]:
        assert not np.isfinite(v) or v == 0 or 1e-100 < abs(v) < 1e100          # (the counts assume the normal range)
    ss = sum((v * v for v in us), mp.mpf(0)) if all(fin) else None
    rowok = yok and ss is not None
    return {"z": [ss / ym if rowok else None],
            "g": [2 * us[l] / ym if (yok and fin[l]) else None for l in range(K)],
            "gy": [-ss / ym ** 2 if rowok else None],
            "hll": [2 * wm / ym if yok else None for l in range(K)],
            "hyy": [2 * wm * ss / ym ** 3 if rowok else None],
            "hly": [-2 * wm * us[l] / ym ** 2 if (yok and fin[l]) else None for l in range(K)]}


def check_row(name, got, u, y, w):
    """`got`: kind -> the row's entries.  Non-finite where the numpy statement is non-finite, and the same value; every
    other entry within gamma(ops) of mpmath.  -> the worst error as a share of its bound."""
    K = len(u)
    ieee = numpy_rule(np.asarray(u, dtype=float)[None, :], np.array([y]), np.array([w]))
    ref = mp_rule(u, y, w)
    worst = 0.0
    for kind in KINDS:
        g = np.asarray(got[kind], dtype=float).reshape(-1)
        e = np.asarray(ieee[kind], dtype=float).reshape(-1)
        assert g.size == e.size == len(ref[kind]), (name, kind, g.size, e.size)
        bound_rel = gamma(ops(kind, K))
        assert bound_rel <= gamma(K + 4)
        for k in range(g.size):
            if not np.isfinite(e[k]):
                same = (np.isnan(e[k]) and np.isnan(g[k])) or g[k] == e[k]
                assert same, "%s %s[%d]: got %r, IEEE gives %r" % (name, kind, k, g[k], e[k])
                continue
            r = ref[kind][k]
            assert r is not None and np.isfinite(g[k]), "%s %s[%d]: got %r for a finite value %r" % (name, kind, k, g[k], e[k])
            err, bound = abs(mp.mpf(float(g[k])) - r), bound_rel * abs(r)
            assert err <= bound, "%s %s[%d]: got %r, expected %s, |error| %s, bound %s" % (
                name, kind, k, g[k], mp.nstr(r, 20), mp.nstr(err, 3), mp.nstr(bound, 3))
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


def arrow_pattern(idx, yidx, z):
    """The segment's pattern arrays stated from its indices alone (idx (M, K), yidx (M), z (M) = the rows' z indices):
    -> drow, dcol, hrow, hcol, hz with the Hessian's three blocks -- (u_l, u_l), (y, y), (u_l, y) -- lower oriented."""
    M, K = idx.shape
    zk = np.repeat(z, K)
    yk = np.repeat(yidx, K)
    flat = idx.reshape(-1)
    hr = np.concatenate([flat, yidx, np.maximum(flat, yk)])
    hc = np.concatenate([flat, yidx, np.minimum(flat, yk)])
    return np.concatenate([zk, z]), np.concatenate([flat, yidx]), hr, hc, np.concatenate([zk, z, zk])


# ---- a tape's op-36 segment as it shows in g, J and H ------------------------------------------------------------------------------
def segment_entries(a, s):
    """(constraint row of every atom row, its sign in G, x indices (M, K), denominator indices (M), positions in J of
    the g_l (M, K) and g_y (M) entries, positions in H of the h_ll (M, K), h_yy (M) and h_ly (M, K) entries).  Every atom
    row feeds one constraint, with coefficient +-1."""
    import scipy.sparse as sp
    assert int(a["seg_op"][s]) == OP_QUAD_OVER_LIN_ROWS
    N, m, Z = (int(v) for v in a["dims"][:3])
    M, K = int(a["seg_d0"][s]), int(a["seg_d1"][s])
    off, off1, zo = int(a["seg_a0_off"][s]), int(a["seg_a1_off"][s]), int(a["seg_zoff"][s])
    idx = np.asarray(a["gidx"][off:off + M * K], dtype=np.int64).reshape(M, K)
    yidx = np.asarray(a["gidx"][off1:off1 + M], dtype=np.int64)
    G = sp.csr_matrix((a["G_val"], a["G_idx"], a["G_ptr"]), shape=(m, N + Z)).tocsc()
    cols = N + zo + np.arange(M)
    assert np.all(np.diff(G.indptr)[cols] == 1)
    crow = G.indices[G.indptr[cols]].astype(np.int64)
    sign = G.data[G.indptr[cols]]
    assert np.all(np.abs(sign) == 1.0)
    jkeys = np.asarray(a["jac_rows"], dtype=np.int64) * N + np.asarray(a["jac_cols"], dtype=np.int64)
    hkeys = np.asarray(a["hess_rows"], dtype=np.int64) * N + np.asarray(a["hess_cols"], dtype=np.int64)

    def find(keys, want):
        pos = np.searchsorted(keys, want)
        assert np.array_equal(keys[pos], want)
        return pos
    yk = yidx[:, None]
    return {"crow": crow, "sign": sign, "idx": idx, "yidx": yidx,
            "g": find(jkeys, crow[:, None] * N + idx), "gy": find(jkeys, crow * N + yidx),
            "hll": find(hkeys, idx * N + idx), "hyy": find(hkeys, yidx * N + yidx),
            "hly": find(hkeys, np.maximum(idx, yk) * N + np.minimum(idx, yk))}


def rows_got(a, s, x, lam, g, J, H):
    """-> (U, y, w, kind -> array over all rows) of segment s from the callbacks' outputs (the sign of G taken out of the
    value and the first derivatives; it is part of w)."""
    e = segment_entries(a, s)
    sign = e["sign"]
    got = {"z": sign * g[e["crow"]], "g": sign[:, None] * J[e["g"]], "gy": sign * J[e["gy"]],
           "hll": H[e["hll"]], "hyy": H[e["hyy"]], "hly": H[e["hly"]]}
    return x[e["idx"]], x[e["yidx"]], sign * lam[e["crow"]], got


def check_segment(name, ev, tape, s=0, pick=None):
    """Rows `pick` (default: all) of segment s of `tape` = (a, x, lam, sigma), evaluated by `ev`, against mpmath."""
    a, x, lam, sigma = tape
    U, y, w, got = rows_got(a, s, x, lam, ev.eval_g(x), ev.eval_jac_g(x), ev.eval_h(x, lam, sigma))
    worst = 0.0
    for r in (range(U.shape[0]) if pick is None else pick):
        worst = max(worst, check_row("%s segment %d row %d" % (name, s, r), {k: v[r] for k, v in got.items()}, U[r], y[r], w[r]))
    return worst


def check_all_rows_numpy(got, U, y, w):
    """EVERY row against the numpy statement.  Both stand within gamma(ops) |ref| of the exact value, so they differ by
    at most 2 gamma |ref| <= 2 gamma / (1 - gamma) |numpy value|."""
    K = U.shape[1]
    ref = numpy_rule(U, y, w)
    for kind in KINDS:
        gm = float(gamma(ops(kind, K)))
        rel = 2 * gm / (1 - gm)
        g, e = np.asarray(got[kind]), ref[kind]
        assert g.shape == e.shape and np.isfinite(g).all(), kind
        bad = ~(np.abs(g - e) <= rel * np.abs(e))
        assert not bad.any(), (kind, int(bad.sum()), np.argwhere(bad)[:4].tolist())
