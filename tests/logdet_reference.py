"""TEST INFRASTRUCTURE -- log_det restated in mpmath (80 digits), the seeded matrices, the brackets and their constants.

For one matrix A of order n (its n^2 entries in F order) the reference is B = inv(A), z = log det A and the products
h[(a, b)] = -w B[j, k] B[l, i] for a = i + j n >= b = k + l n, all in mpmath.  B and the pivots pi_k come from one exact
elimination without pivoting, so z = sum_k log pi_k is the same number as log det A.

The evaluators' rule (csrc/row_class.h logdet_row) is Gauss-Jordan without pivoting.  With E = |B| |A| |B| (entrywise
absolute values, matrix products) and eps = 2^-53 the brackets are

    value                 eps C_V (n tr(|B| |A|) + sum_k |log pi_k| + |z|)
    d entry holding B_ji  eps C_D (n E_ji + |B_ji|)
    h entry -w p q        eps C_H |w| (|p| beta_q + |q| beta_p + |p q|),   beta = n E + |B| of the entry behind p and q

The constants are MEASURED on `numpy_rule`, an independent numpy statement of the rule, over `matrices()`: four times the
statement's worst ratio, rounded up to a power of two (`measure_constants`; tests/test_log_det_cpu.py asserts that the
constants written here are what that gives).  A device result that needs a larger constant is a finding.  No point is
left out: every matrix here has pivots and entries far inside the normal double range.

Matrices (seeded): Q diag(geometric spectrum from 1 up to the condition number) Q^T with condition numbers 1, 10, 100, 1e4,
and the same plus
0.3 (S - S^T) / sqrt(n) with S standard normal (the rule is evaluated at a point the test chooses, so the argument need
not be symmetric there; the symmetric part stays positive definite, so every pivot stays positive).
"""
import mpmath as mp          # a dependency of torch's sympy; a missing mpmath is an error, never a skip
import numpy as np

import prod_reference as pr   # (Units / Entries / the walk through the tape's constant maps are shared)

mp.mp.dps = 80               # (prod_reference's own setting: one mpmath context per process)
EPS = 2.0 ** -53
SEED = 3707
OP_LOG_DET = 37
ORDERS = (1, 2, 3, 5, 7, 8, 9, 16, 32, 33, 45)
CONDS = (1.0, 10.0, 100.0, 1e4)
# measured by measure_constants() on numpy_rule over matrices(): worst ratios 0.131 (value), 0.287 (d), 0.275 (h)
C_V, C_D, C_H = 1.0, 2.0, 2.0


def matrix(n, cond, skew, seed=SEED):
    rng = np.random.default_rng([seed, n, int(round(np.log10(cond) * 10)), int(skew)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    spec = cond ** (np.arange(n) / max(n - 1, 1)) if n > 1 else np.array([1.0 + rng.random()])
    A = (Q * spec) @ Q.T
    A = (A + A.T) / 2
    if skew and n > 1:
        S = rng.standard_normal((n, n))
        A = A + 0.3 * (S - S.T) / np.sqrt(n)
    return A


def matrices(orders=ORDERS):
    """-> list of (n, cond, skew, A).  (A skew part leaves the symmetric part of every leading block positive definite, so
    every pivot of the elimination stays positive.)"""
    out = []
    for n in orders:
        for cond in (CONDS if n > 1 else (1.0,)):
            for skew in ((False, True) if n > 1 else (False,)):
                out.append((n, cond, skew, matrix(n, cond, skew)))
    return out


def numpy_rule(A, w=1.0, hsel=None):
    """The rule in numpy for ONE matrix: z, d (n^2, F order), h (the packed triangle over the n^2 entries, or the packed
    positions `hsel`).  Row operations as whole-array statements: an independent text, not the loops of the C++."""
    a = np.array(A, dtype=float)
    n = a.shape[0]
    ok, z = True, 0.0
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = a[k, k]
            ok = ok and bool(piv > 0)
            z += np.log(piv)
            row = a[k, :] / piv
            row[k] = 1.0 / piv
            f = a[:, k].copy()
            f[k] = 0.0
            a = a - np.outer(f, row)
            a[:, k] = -f * row[k]
            a[k, :] = row
        d = a.T.reshape(-1, order="F").copy()           # d[i + j n] = B[j, i]
        if not ok:
            z, d = np.nan, np.full(n * n, np.nan)
        qa, qb = np.tril_indices(n * n) if hsel is None else tri_decode(hsel)
        h = -w * d[qb % n + (qa // n) * n] * d[qa % n + (qb // n) * n]
    return z, d, h


def tri_decode(q):
    """Packed positions of the lower triangle with its diagonal, row-major -> (a, b), a >= b."""
    q = np.asarray(q, dtype=np.int64)
    a = ((np.sqrt(8.0 * q + 1.0) - 1.0) * 0.5).astype(np.int64)
    a -= (a * (a + 1) // 2 > q)
    a += ((a + 1) * (a + 2) // 2 <= q)
    return a, q - a * (a + 1) // 2


_exact = {}


def exact(A):
    """-> (B as an n x n list of mpf, pivots) by Gauss-Jordan without pivoting in mpmath; cached by the matrix's bytes."""
    A = np.asarray(A, dtype=float)
    key = A.tobytes()
    if key not in _exact:
        n = A.shape[0]
        a = [[mp.mpf(float(A[i, j])) for j in range(n)] for i in range(n)]
        piv = []
        for k in range(n):
            p = a[k][k]
            piv.append(p)
            rk = [v / p for v in a[k]]
            rk[k] = 1 / p
            for i in range(n):
                if i == k:
                    continue
                f = a[i][k]
                ai = a[i]
                a[i] = [ai[j] - f * rk[j] for j in range(n)]
                a[i][k] = -f * rk[k]
            a[k] = rk
        _exact[key] = (a, piv)
    return _exact[key]


def _put(U, k, v, bracket):
    hi = float(v)
    U.hi[k] = hi
    U.lo[k] = float(v - mp.mpf(hi))
    U.st[k] = 0
    U.bound[k] = np.nextafter(bracket, 0.0)


def brackets(A):
    """-> (value bracket without its constant, beta = n E + |B| as an n x n array indexed like B) in double, from mpmath
    B rounded to double (the brackets need no more than a few digits)."""
    B, piv = exact(A)
    n = len(piv)
    Bd = np.abs(np.array([[float(v) for v in row] for row in B]))
    Ad = np.abs(np.asarray(A, dtype=float))
    E = Bd @ Ad @ Bd
    z = mp.fsum(mp.log(p) for p in piv)
    bv = n * float(np.trace(Bd @ Ad)) + float(mp.fsum(abs(mp.log(p)) for p in piv)) + abs(float(z))
    return bv, n * E + Bd, z


def matrix_reference(A, w=1.0, hsel=None, consts=None):
    """Units of value (1), d (n^2) and h (the whole packed triangle, or the packed positions `hsel`) of one matrix with
    weight w; `consts`: (C_V, C_D, C_H), the written ones by default."""
    cv, cd, ch = (C_V, C_D, C_H) if consts is None else consts
    A = np.asarray(A, dtype=float)
    n = A.shape[0]
    B, piv = exact(A)
    bv, beta, z = brackets(A)
    V, D = pr.Units(1), pr.Units(n * n)
    _put(V, 0, z, EPS * cv * bv)
    for j in range(n):
        for i in range(n):
            _put(D, i + j * n, B[j][i], EPS * cd * beta[j, i])        # d[i + j n] = B_ji
    qa, qb = np.tril_indices(n * n) if hsel is None else tri_decode(hsel)
    H = pr.Units(qa.size)
    wm = mp.mpf(float(w))
    for t, (a, b) in enumerate(zip(qa.tolist(), qb.tolist())):
        i, j, k, l = a % n, a // n, b % n, b // n
        p, q = B[j][k], B[l][i]
        ap, aq = abs(float(p)), abs(float(q))
        _put(H, t, -wm * p * q, EPS * ch * abs(float(w)) * (ap * beta[l, i] + aq * beta[j, k] + ap * aq))
    return V, D, H


def ratios(U, got, const):
    """|error| / (bound / const) per entry: the error in units of eps times the bracket."""
    err = U.error(got)
    return err / (U.bound / const)


def measure_constants(hsample=400):
    """The numpy statement against mpmath over matrices(): -> {kind: worst ratio}, and the constants that follow."""
    worst = {"value": 0.0, "d1": 0.0, "d2": 0.0}
    rng = np.random.default_rng([SEED, 5])
    for n, cond, skew, A in matrices():
        T = n * n * (n * n + 1) // 2
        hsel = None if T <= hsample else np.unique(np.r_[0, T - 1, rng.integers(0, T, hsample)])
        V, D, H = matrix_reference(A, 1.0, hsel, consts=(1.0, 1.0, 1.0))
        z, d, h = numpy_rule(A, 1.0, hsel)
        for kind, U, got in (("value", V, [z]), ("d1", D, d), ("d2", H, h)):
            worst[kind] = max(worst[kind], float(np.max(ratios(U, np.asarray(got, dtype=float), 1.0))))
    return worst, {k: float(2.0 ** np.ceil(np.log2(4.0 * v))) for k, v in worst.items()}


# ---- through the tape's constant maps ----------------------------------------------------------------------------------------
def reference_sweep(a, x, w, hsample=None, seed=SEED):
    """Units of z, dvals, hvals of a tape: the log_det segments are referenced, every other segment's entries are not
    (st = 2).  A matrix with more than `hsample` Hessian entries has that many seeded ones referenced, the first and the
    last among them."""
    N, m, Z, nseg, nd, nh = (int(v) for v in a["dims"][:6])
    z, d, h = pr.Units(Z), pr.Units(nd), pr.Units(nh)
    z.st[:], d.st[:], h.st[:] = 2, 2, 2
    rng = np.random.default_rng([seed, 77])
    for s in range(nseg):
        if int(a["seg_op"][s]) != OP_LOG_DET:
            continue
        K, n = int(a["seg_d1"][s]), int(a["seg_d2"][s])
        assert int(a["seg_d0"][s]) == 1 and n * n == K
        T = K * (K + 1) // 2
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        hsel = None
        if hsample is not None and T > hsample:
            hsel = np.unique(np.concatenate([[0, T - 1], rng.integers(0, T, hsample)]))
        V, D, H = matrix_reference(x[idx].reshape(n, n, order="F"), w[zo], hsel)
        pos = ho + (np.arange(T) if hsel is None else hsel)
        for dst, src, at in ((z, V, np.array([zo])), (d, D, do + np.arange(K)), (h, H, pos)):
            dst.hi[at], dst.lo[at], dst.st[at], dst.bound[at] = src.hi, src.lo, src.st, src.bound
    return z, d, h


def expected_oracles(a, x, lam, sigma, hsample=None):
    """g, jac, hess, f, grad_f of a tape whose nonlinear segments are all log_det, as Entries, through the tape's own
    constant maps (prod_reference._through: the summation bound of the maps' rounded operations is added)."""
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
