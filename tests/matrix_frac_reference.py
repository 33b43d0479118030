"""TEST INFRASTRUCTURE -- matrix_frac restated in mpmath (80 digits), the seeded inputs, the brackets and their constants.

For one segment -- P of order n, X of n x m, the K = n^2 + n m entries of the tape row in the order P (F), X (F) -- the
reference is, all in mpmath and out of ONE exact elimination without pivoting (the first n steps on the bordered matrix
[[P, X], [X^T, 0]] of order N = n + m),

    B = inv(P)     W = B X     V = B^T X     G = V W^T     z = tr(X^T B X) = minus the trace of the swept last block
    d[i + j n] = -G_ij                          d[n^2 + i + c n] = W_ic + V_ic
    h over the packed lower triangle of the K entries, row-major, times the weight w:
        P_ij, P_kl     B_li G_kj + B_jk G_il
        X_kc, P_ij     -(B_ki W_jc + V_ic B_jk)
        X_ic, X_jd     (c == d) (B_ij + B_ji)

The evaluators' rule (csrc/row_class.h mfrac_row, mfrac_d, mfrac_h) is that elimination in double.  With |.| entrywise,
E = |B| |P| |B|, eps = 2^-53 and

    beta_B = N E + |B|                                    (what Gauss-Jordan leaves of the inverse, as for log_det)
    beta_W = N (E + |B|) |X| + |W|                        beta_V = N (E + |B|)^T |X| + |V|
    beta_G = |V| beta_W^T + beta_V |W|^T + m |V| |W|^T

the brackets are

    value                  eps C_V (N tr(|X|^T (E + |B|) |X|) + |z|)
    d entry of P           eps C_DP beta_G_ij
    d entry of X           eps C_DX (beta_W_ic + beta_V_ic)
    h entry P, P           eps C_HPP |w| (|B_li| beta_G_kj + beta_B_li |G_kj| + |B_jk| beta_G_il + beta_B_jk |G_il| + 2 |t1| + 2 |t2|)
    h entry X, P           eps C_HXP |w| (|B_ki| beta_W_jc + beta_B_ki |W_jc| + |V_ic| beta_B_jk + beta_V_ic |B_jk| + 2 |t1| + 2 |t2|)
    h entry X, X, c == d   eps C_HXX |w| (beta_B_ij + beta_B_ji + |B_ij + B_ji|);   c != d: exactly 0

(t1, t2: the two products of the entry).  The constants are MEASURED on `numpy_rule`, an independent whole-array numpy
statement of the rule, over `inputs()`: four times the statement's worst ratio, rounded up to a power of two
(`measure_constants`; tests/test_matrix_frac_cpu.py asserts that the constants written here are what that gives).  A
device or host result that needs a larger constant is a finding.  No point is left out.

Inputs (seeded): P = logdet_reference.matrix(n, cond, skew) -- symmetric and with a skew part, condition numbers 1, 10,
100, 1e4 -- and a standard-normal X.
"""
import mpmath as mp
import numpy as np

import logdet_reference as lr
import prod_reference as pr

EPS = lr.EPS
SEED = 4111
OP_MATRIX_FRAC = 38
CONDS = lr.CONDS
# (n, m): every short group width, the last short N = 8, K <= 64 with N^2 > 64, the first long N = 9, m > 1 in the long
# form, N = 32 and 33, N = 45 with m = 1 and with m > n, n = 1
SHAPES = ((1, 1), (2, 1), (3, 1), (5, 2), (7, 1), (6, 4), (8, 1), (6, 3), (1, 44), (31, 1), (32, 1), (10, 35), (44, 1))
KINDS = ("value", "dP", "dX", "hPP", "hXP", "hXX")
# measured by measure_constants() on numpy_rule over inputs(): worst ratios 0.153 (value), 0.135 (dP), 0.154 (dX), 0.116 (hPP),
# 0.145 (hXP), 0.215 (hXX)
CONSTS = {"value": 1.0, "dP": 1.0, "dX": 1.0, "hPP": 0.5, "hXP": 1.0, "hXX": 1.0}


def inputs_of(n, m, cond, skew, seed=SEED):
    P = lr.matrix(n, cond if n > 1 else 1.0, skew and n > 1, seed=seed)
    X = np.random.default_rng([seed, n, m, int(round(np.log10(cond) * 10)), int(skew)]).standard_normal((n, m))
    return P, X


def inputs(shapes=SHAPES):
    """-> list of (n, m, cond, skew, P, X)."""
    out = []
    for n, m in shapes:
        for cond in (CONDS if n > 1 else (1.0,)):
            for skew in ((False, True) if n > 1 else (False,)):
                out.append((n, m, cond, skew) + inputs_of(n, m, cond, skew))
    return out


def row_of(P, X):
    """The tape row: P in F order, then X in F order."""
    return np.concatenate([np.asarray(P, dtype=float).reshape(-1, order="F"), np.asarray(X, dtype=float).reshape(-1, order="F")])


def split_row(u, n):
    u = np.asarray(u, dtype=float)
    return u[:n * n].reshape(n, n, order="F"), u[n * n:].reshape(n, -1, order="F")


def classify(n, m, qa, qb):
    """Packed pairs (a >= b) over the K entries -> kind (0 PP, 1 XP, 2 XX) and the indices (i, j) of a and (k, l) of b, the
    second index of an X entry being its column c."""
    nn = n * n
    aP, bP = qa < nn, qb < nn
    ai = np.where(aP, qa % n, (qa - nn) % n)
    aj = np.where(aP, qa // n, (qa - nn) // n)
    bi = np.where(bP, qb % n, (qb - nn) % n)
    bj = np.where(bP, qb // n, (qb - nn) // n)
    return np.where(aP, 0, np.where(bP, 1, 2)), ai, aj, bi, bj


def numpy_rule(P, X, w=1.0, hsel=None):
    """The rule in numpy for ONE segment: z, d (K), h (the packed triangle over the K entries, or the packed positions
    `hsel`).  Row operations and the products B, W, V, G as whole-array statements: an independent text, not the loops
    of the C++."""
    P, X = np.asarray(P, dtype=float), np.asarray(X, dtype=float)
    n, m = X.shape
    N, K = n + m, n * (n + m)
    a = np.zeros((N, N))
    a[:n, :n], a[:n, n:], a[n:, :n] = P, X, X.T
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = a[k, k]
            ok = ok and bool(piv > 0)
            row = a[k, :] / piv
            row[k] = 1.0 / piv
            f = a[:, k].copy()
            f[k] = 0.0
            a = a - np.outer(f, row)
            a[:, k] = -f * row[k]
            a[k, :] = row
        if not ok:
            a[:] = np.nan
        B, W, V = a[:n, :n], a[:n, n:], -a[n:, :n].T
        G = V @ W.T
        z = -float(np.sum(np.diag(a[n:, n:])))
        d = np.concatenate([(-G).reshape(-1, order="F"), (W + V).reshape(-1, order="F")])
        qa, qb = np.tril_indices(K) if hsel is None else lr.tri_decode(hsel)
        kind, ai, aj, bi, bj = classify(n, m, qa, qb)
        i0, j0, k0, l0 = (np.where(kind == 0, v, 0) for v in (ai, aj, bi, bj))
        hpp = B[l0, i0] * G[k0, j0] + B[j0, k0] * G[i0, l0]
        k1, c1, i1, j1 = (np.where(kind == 1, v, 0) for v in (ai, aj, bi, bj))
        hxp = -(B[k1, i1] * W[j1, c1] + V[i1, c1] * B[j1, k1])
        i2, c2, j2, d2 = (np.where(kind == 2, v, 0) for v in (ai, aj, bi, bj))
        s = B[i2, j2] + B[j2, i2]
        hxx = np.where(c2 == d2, s, np.where(np.isnan(s), s, 0.0))
        h = w * np.where(kind == 0, hpp, np.where(kind == 1, hxp, hxx))
    return z, d, h


_exact = {}


def exact(P, X):
    """-> dict of B, W, V, G (lists of lists of mpf) and z, by the first n steps of Gauss-Jordan without pivoting on the
    bordered matrix in mpmath; cached by the inputs' bytes."""
    P, X = np.asarray(P, dtype=float), np.asarray(X, dtype=float)
    key = P.tobytes() + X.tobytes()
    if key not in _exact:
        n, m = X.shape
        N = n + m
        a = [[mp.mpf(0)] * N for _ in range(N)]
        for i in range(n):
            for j in range(n):
                a[i][j] = mp.mpf(float(P[i, j]))
            for c in range(m):
                a[i][n + c] = mp.mpf(float(X[i, c]))
                a[n + c][i] = mp.mpf(float(X[i, c]))
        a = [list(r) for r in a]
        for k in range(n):
            p = a[k][k]
            rk = [v / p for v in a[k]]
            rk[k] = 1 / p
            for i in range(N):
                if i == k:
                    continue
                f = a[i][k]
                ai = a[i]
                a[i] = [ai[j] - f * rk[j] for j in range(N)]
                a[i][k] = -f * rk[k]
            a[k] = rk
        B = [a[i][:n] for i in range(n)]
        W = [a[i][n:] for i in range(n)]
        V = [[-a[n + c][i] for c in range(m)] for i in range(n)]
        G = [[mp.fsum(V[i][c] * W[j][c] for c in range(m)) for j in range(n)] for i in range(n)]
        z = -mp.fsum(a[n + c][n + c] for c in range(m))
        _exact[key] = {"B": B, "W": W, "V": V, "G": G, "z": z}
    return _exact[key]


def _dbl(M):
    return np.array([[float(v) for v in row] for row in M], dtype=float).reshape(len(M), -1)


def brackets(P, X):
    """The betas of the header in double (the brackets need no more than a few digits) and the value bracket."""
    ex = exact(P, X)
    n, m = np.asarray(X).shape
    N = n + m
    B, W, V, G = (np.abs(_dbl(ex[k])) for k in ("B", "W", "V", "G"))
    Pa, Xa = np.abs(np.asarray(P, dtype=float)), np.abs(np.asarray(X, dtype=float))
    E = B @ Pa @ B
    bB = N * E + B
    bW = N * (E + B) @ Xa + W
    bV = N * (E + B).T @ Xa + V
    bG = V @ bW.T + bV @ W.T + m * (V @ W.T)
    bv = N * float(np.trace(Xa.T @ (E + B) @ Xa)) + abs(float(ex["z"]))
    return {"B": bB, "W": bW, "V": bV, "G": bG, "value": bv, "aB": B, "aW": W, "aV": V, "aG": G}


def segment_reference(P, X, w=1.0, hsel=None, consts=None):
    """Units of value (1), d (K) and h (the whole packed triangle, or the packed positions `hsel`) of one segment with
    weight w, and the kind of every unit (an index into KINDS); `consts`: by kind, the written ones by default."""
    C = CONSTS if consts is None else consts
    P, X = np.asarray(P, dtype=float), np.asarray(X, dtype=float)
    n, m = X.shape
    K = n * (n + m)
    ex, bt = exact(P, X), brackets(P, X)
    B, W, V, G = ex["B"], ex["W"], ex["V"], ex["G"]
    Vu, D = pr.Units(1), pr.Units(K)
    lr._put(Vu, 0, ex["z"], EPS * C["value"] * bt["value"])
    dk = np.zeros(K, dtype=np.int8)
    for j in range(n):
        for i in range(n):
            lr._put(D, i + j * n, -G[i][j], EPS * C["dP"] * bt["G"][i, j])
            dk[i + j * n] = 1
    for c in range(m):
        for i in range(n):
            lr._put(D, n * n + i + c * n, W[i][c] + V[i][c], EPS * C["dX"] * (bt["W"][i, c] + bt["V"][i, c]))
            dk[n * n + i + c * n] = 2
    qa, qb = np.tril_indices(K) if hsel is None else lr.tri_decode(hsel)
    kind, ai, aj, bi, bj = classify(n, m, qa, qb)
    H = pr.Units(qa.size)
    wm, aw = mp.mpf(float(w)), abs(float(w))
    aB, aW, aV, aG = bt["aB"], bt["aW"], bt["aV"], bt["aG"]
    for t, (kd, i, j, k, l) in enumerate(zip(kind.tolist(), ai.tolist(), aj.tolist(), bi.tolist(), bj.tolist())):
        if kd == 0:
            t1, t2 = B[l][i] * G[k][j], B[j][k] * G[i][l]
            br = (aB[l, i] * bt["G"][k, j] + bt["B"][l, i] * aG[k, j] + aB[j, k] * bt["G"][i, l] + bt["B"][j, k] * aG[i, l]
                  + 2 * abs(float(t1)) + 2 * abs(float(t2)))
            lr._put(H, t, wm * (t1 + t2), EPS * C["hPP"] * aw * br)
        elif kd == 1:                      # a = X_kc with (k, c) = (i, j) here; b = P_ij with (i, j) = (k, l) here
            kk, c, ii, jj = i, j, k, l
            t1, t2 = B[kk][ii] * W[jj][c], V[ii][c] * B[jj][kk]
            br = (aB[kk, ii] * bt["W"][jj, c] + bt["B"][kk, ii] * aW[jj, c] + aV[ii, c] * bt["B"][jj, kk] + bt["V"][ii, c] * aB[jj, kk]
                  + 2 * abs(float(t1)) + 2 * abs(float(t2)))
            lr._put(H, t, -wm * (t1 + t2), EPS * C["hXP"] * aw * br)
        else:                              # a = X_ic, b = X_jd with (j, d) = (k, l) here
            if j == l:
                sB = B[i][k] + B[k][i]
                lr._put(H, t, wm * sB, EPS * C["hXX"] * aw * (bt["B"][i, k] + bt["B"][k, i] + abs(float(sB))))
            else:
                lr._put(H, t, mp.mpf(0), 0.0)
    return Vu, D, H, dk, kind + 3


def measure_constants(hsample=400):
    """The numpy statement against mpmath over inputs(): -> ({kind: worst ratio}, {kind: the constant that follows})."""
    worst = {k: 0.0 for k in KINDS}
    ones = {k: 1.0 for k in KINDS}
    rng = np.random.default_rng([SEED, 5])
    for n, m, cond, skew, P, X in inputs():
        K = n * (n + m)
        T = K * (K + 1) // 2
        hsel = None if T <= hsample else np.unique(np.r_[0, T - 1, rng.integers(0, T, hsample)])
        Vu, D, H, dk, hk = segment_reference(P, X, 1.0, hsel, consts=ones)
        z, d, h = numpy_rule(P, X, 1.0, hsel)
        for U, got, kinds in ((Vu, [z], np.zeros(1, dtype=int)), (D, d, dk), (H, h, hk)):
            err = U.error(np.asarray(got, dtype=float))
            for kd in np.unique(kinds):
                sel = (kinds == kd) & (U.bound > 0)
                if sel.any():
                    worst[KINDS[kd]] = max(worst[KINDS[kd]], float(np.max(err[sel] / U.bound[sel])))
                exact0 = (kinds == kd) & (U.bound == 0)
                assert not np.any(err[exact0] > 0)
    return worst, {k: float(2.0 ** np.ceil(np.log2(4.0 * v))) for k, v in worst.items()}


# ---- through the tape's constant maps ----------------------------------------------------------------------------------------
def reference_sweep(a, x, w, hsample=None, seed=SEED):
    """Units of z, dvals, hvals of a tape: the matrix_frac and the log_det segments are referenced, every other
    segment's entries are not (st = 2).  A segment with more than `hsample` Hessian entries has that many seeded ones
    referenced, the first and the last among them."""
    z, d, h = lr.reference_sweep(a, x, w, hsample)
    nseg = int(a["dims"][3])
    rng = np.random.default_rng([seed, 78])
    for s in range(nseg):
        if int(a["seg_op"][s]) != OP_MATRIX_FRAC:
            continue
        K, n = int(a["seg_d1"][s]), int(a["seg_d2"][s])
        assert int(a["seg_d0"][s]) == 1 and K % n == 0 and K >= n * n
        T = K * (K + 1) // 2
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        hsel = None
        if hsample is not None and T > hsample:
            hsel = np.unique(np.concatenate([[0, T - 1], rng.integers(0, T, hsample)]))
        P, X = split_row(x[idx], n)
        V, D, H, _, _ = segment_reference(P, X, w[zo], hsel)
        pos = ho + (np.arange(T) if hsel is None else hsel)
        for dst, src, at in ((z, V, np.array([zo])), (d, D, do + np.arange(K)), (h, H, pos)):
            dst.hi[at], dst.lo[at], dst.st[at], dst.bound[at] = src.hi, src.lo, src.st, src.bound
    return z, d, h


def expected_oracles(a, x, lam, sigma, hsample=None):
    """g, jac, hess, f, grad_f of a tape whose nonlinear segments are matrix_frac and log_det, as Entries, through the
    tape's own constant maps (prod_reference._through: the summation bound of the maps' rounded operations is added)."""
    import scipy.sparse as sp
    x = np.asarray(x, dtype=float)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = pr.weights(a, lam, sigma)
    z, d, h = reference_sweep(a, x, w, hsample)
    G = pr._csr(a, "G", (m, N + Z))
    Gx, Gz = sp.csr_matrix(G[:, :N]), sp.csr_matrix(G[:, N:])
    c = np.asarray(a["c"], dtype=float)
    out = {"units": (z, d, h)}
    out["g"] = pr._through(Gz, a["b"] + Gx @ x, 2 * np.diff(Gx.indptr), z, "g")
    out["f"] = pr._through(sp.csr_matrix(c[N:].reshape(1, -1)), np.array([float(a["c0"][0]) + c[:N] @ x]),
                           np.array([2 * int(np.count_nonzero(c[:N]))]), z, "f")
    out["grad_f"] = pr._through(pr._csr(a, "Mg", (N, nd)), c[:N], np.zeros(N), d, "grad_f")
    out["jac"] = pr._through(pr._csr(a, "MJ", (nnzJ, nd)), np.asarray(a["Jc"], dtype=float), np.zeros(nnzJ), d, "jac")
    out["hess"] = pr._through(pr._csr(a, "MH", (nnzH, nh)), np.zeros(nnzH), np.zeros(nnzH), h, "hess")
    return out
