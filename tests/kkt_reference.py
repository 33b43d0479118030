"""The independent side of the KKT probe tests (include/dnlp_hip.h dnlp_kkt_probe).

    K = [[H + diag(Sx) + delta_w I, J^T], [J, -diag(D)]]          (variables first, then constraint rows)

is built here as COO triplets in numpy from the HOST library's oracles (hess_structure / eval_h / jac_structure /
eval_jac_g: pinned against mpmath and the golden vectors by their own tests), so nothing on this side depends on the
device or on the assembly, the factorisations or the solves under test.  The row and the column of every variable with
fixmask != 0 are those of the identity.

Reference solution: float64 sparse LU (scipy splu) followed by refinement steps whose residual r - K z is accumulated in
np.longdouble over the COO arrays (np.add.at; scipy's products are float64) and whose iterate is kept in longdouble; it
stops when the longdouble backward error stops falling and returns the error it reached.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
EIG_MAX_ORDER = 600


class Kkt:
    """COO triplets of the full symmetric K (duplicates NOT merged: they are summed where the triplets are used)."""

    def __init__(self, n, rows, cols, vals, N, m):
        self.n, self.N, self.m = int(n), int(N), int(m)
        self.rows, self.cols, self.vals = rows, cols, vals
        self._vals_ld = vals.astype(LD)
        self._lu = None

    def csc(self):
        M = sp.coo_matrix((self.vals, (self.rows, self.cols)), shape=(self.n, self.n)).tocsc()
        M.sum_duplicates()
        return M

    def dense(self):
        return np.asarray(self.csc().todense())

    def matvec_ld(self, z):
        """K z in longdouble."""
        out = np.zeros(self.n, LD)
        np.add.at(out, self.rows, self._vals_ld * np.asarray(z, LD)[self.cols])
        return out

    def norm_inf(self):
        """||K||_inf (largest absolute row sum of the merged matrix), longdouble."""
        M = self.csc()
        return LD(np.max(np.abs(M).sum(axis=1))) if self.n else LD(0)

    def lu(self):
        if self._lu is None:
            self._lu = spla.splu(self.csc(), permc_spec="MMD_AT_PLUS_A")      # (symmetric pattern: 20x less fill than COLAMD)
        return self._lu


def build_kkt(host, x, lam, obj_factor, Sx, D, fixmask=None, delta_w=0.0):
    """`host`: a handle of the HOST library (oracle.oracle_capi.OracleProblem) of the same tape."""
    N, m = host.n, host.m
    x = np.asarray(x, float)
    fm = np.zeros(N) if fixmask is None else np.asarray(fixmask, float)
    fixed = fm != 0.0
    hr, hc = (a.astype(np.int64) for a in host.hess_structure())
    hv = host.eval_h(x, lam, obj_factor)
    keep = ~(fixed[hr] | fixed[hc])
    hr, hc, hv = hr[keep], hc[keep], hv[keep]
    off = hr != hc
    rows = [hr, hc[off]]                      # the oracle lists one triangle: mirror it
    cols = [hc, hr[off]]
    vals = [hv, hv[off]]
    if m:
        jr, jc = (a.astype(np.int64) for a in host.jac_structure())
        jv = host.eval_jac_g(x)
        keep = ~fixed[jc]
        jr, jc, jv = jr[keep], jc[keep], jv[keep]
        rows += [N + jr, jc]
        cols += [jc, N + jr]
        vals += [jv, jv]
        rows.append(N + np.arange(m, dtype=np.int64))
        cols.append(N + np.arange(m, dtype=np.int64))
        vals.append(-np.asarray(D, float))
    d = np.where(fixed, 1.0, np.asarray(Sx, float) + float(delta_w))
    rows.append(np.arange(N, dtype=np.int64))
    cols.append(np.arange(N, dtype=np.int64))
    vals.append(d)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    assert np.all(np.isfinite(vals)), "the point is outside the domain of an atom"
    return Kkt(N + m, rows, cols, vals, N, m)


def backward_error(K, z, r, knorm=None):
    """eta(z) = ||r - K z||_inf / (||K||_inf ||z||_inf + ||r||_inf), in longdouble."""
    z, r = np.asarray(z, LD), np.asarray(r, LD)
    knorm = K.norm_inf() if knorm is None else knorm
    res = r - K.matvec_ld(z)
    return float(np.max(np.abs(res)) / (knorm * np.max(np.abs(z)) + np.max(np.abs(r))))


def solve_refined(K, r, max_steps=12):
    """(z, eta): z in longdouble, eta = its backward error, the smallest the refinement reached."""
    lu, knorm = K.lu(), K.norm_inf()
    r_ld = np.asarray(r, LD)
    z = lu.solve(np.asarray(r, float)).astype(LD)
    best_z, best = z, backward_error(K, z, r_ld, knorm)
    for _ in range(max_steps):
        res = r_ld - K.matvec_ld(z)
        z = z + lu.solve(res.astype(np.float64)).astype(LD)
        eta = backward_error(K, z, r_ld, knorm)
        if not eta < best:
            break
        fell = eta < 0.5 * best
        best_z, best = z, eta
        if not fell:
            break
    return best_z, best


def forward_error(z, z_ref):
    z, z_ref = np.asarray(z, LD), np.asarray(z_ref, LD)
    return float(np.max(np.abs(z - z_ref)) / np.max(np.abs(z_ref)))


def cond_estimate(K):
    """||K||_inf ||K^-1||_inf with the second factor from Hager / Higham's estimator on the LU solves (K is symmetric, so
    its 1-norm is its inf-norm); the estimate is a lower bound, in practice within a factor 3."""
    lu = K.lu()
    inv = spla.LinearOperator((K.n, K.n), matvec=lambda b: lu.solve(np.asarray(b, float).ravel()),
                              rmatvec=lambda b: lu.solve(np.asarray(b, float).ravel(), "T"), dtype=float)
    return float(K.norm_inf()) * float(spla.onenormest(inv))


def inertia(K, quasi_definite=False):
    """(nneg, nzero).  Orders up to EIG_MAX_ORDER: from the eigenvalues of the dense K (zero: |lambda| <= n eps ||K||).
    Above: only for inputs that are quasi-definite BY CONSTRUCTION — the caller vouches that H + Sx + delta_w is positive
    definite by strict diagonal dominance with a positive diagonal, and D > 0 — where the inertia is (N, m, 0) with
    nothing to factorise; both halves of the claim are verified here (absolute row sums of the merged matrix)."""
    if K.n <= EIG_MAX_ORDER:
        A = K.dense()
        ev = np.linalg.eigvalsh(A)
        tol = K.n * np.finfo(float).eps * float(np.max(np.abs(ev))) if K.n else 0.0
        return int(np.sum(ev < -tol)), int(np.sum(np.abs(ev) <= tol))
    if not quasi_definite:
        raise ValueError("order %d: no reference inertia unless the input is quasi-definite by construction" % K.n)
    M = K.csc()
    diag = np.asarray(M.diagonal())
    A = M[:K.N, :K.N]
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(diag[:K.N])
    assert np.all(diag[:K.N] > off) and np.all(diag[K.N:] < 0.0)
    return K.m, 0
