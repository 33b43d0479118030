"""TEST INFRASTRUCTURE -- the log_det solves with closed forms (Gaussian maximum likelihood with a symmetric
parametrisation and with a plain matrix variable, D-optimal design, the largest ellipsoid in a box), their certificates
written out in numpy, and tapes that hold given matrices; shared by the CPU and the GPU tests."""
import numpy as np

from prod_problems import VALUE_TOL, VIOLATION_TOL   # the closed-form tolerances of tests/prod_problems.py, unchanged

POINT_TOL = 1e-4         # relative to the largest entry of the closed form (tests/prod_problems.py assert_box)


def sym_map(n):
    """E: the constant map from the n (n + 1) / 2 free entries of a symmetric matrix (its lower triangle, row-major) to
    its vec in F order."""
    ii, jj = np.tril_indices(n)
    E = np.zeros((n * n, ii.size))
    for k, (i, j) in enumerate(zip(ii, jj)):
        E[i + j * n, k] = 1.0
        E[j + i * n, k] = 1.0
    return E


def sym_entries(S):
    ii, jj = np.tril_indices(S.shape[0])
    return np.asarray(S, dtype=float)[ii, jj]


# ---- (1), (2) Gaussian maximum likelihood: minimise trace(C S) - log det S ---------------------------------------------------
def likelihood_C(n=4, seed=17):
    R = np.random.default_rng(seed).standard_normal((n, 3 * n))
    return R @ R.T / (3 * n) + 0.1 * np.eye(n)


LIKELIHOOD_STARTS = {
    "identity": np.eye(4),
    "hundredfold": 100.0 * np.eye(4),
    "hundredth": 0.01 * np.eye(4),
    "indefinite": np.diag([1.0, -1.0, 2.0, -0.5]) + 0.25,
}


def likelihood_problem(start="identity", C=None, parameters=False):
    """S = reshape(E s, (4, 4)) with s the free entries: -> (problem, s[, [C as a Parameter]])."""
    import dnlp_amd as cp
    C = likelihood_C() if C is None else C
    n = C.shape[0]
    s = cp.Variable(n * (n + 1) // 2, name="s")
    s.value = sym_entries(LIKELIHOOD_STARTS[start] if isinstance(start, str) else start)
    S = cp.reshape(sym_map(n) @ s, (n, n), order="F")
    if parameters:
        pc = cp.Parameter((n, n), name="C", value=np.asarray(C, dtype=float))
        return cp.Problem(cp.Minimize(cp.sum(cp.multiply(pc, S)) - cp.log_det(S))), s, [pc]
    return cp.Problem(cp.Minimize(cp.trace(C @ S) - cp.log_det(S))), s


def likelihood_plain_problem(C=None):
    """The same with a plain matrix variable: its skew part is not determined."""
    import dnlp_amd as cp
    C = likelihood_C() if C is None else C
    X = cp.Variable(C.shape, name="X")
    X.value = np.eye(C.shape[0])
    return cp.Problem(cp.Minimize(cp.trace(C @ X) - cp.log_det(X))), X


def likelihood_optimum(C):
    return np.linalg.inv(C), C.shape[0] + float(np.linalg.slogdet(C)[1])


def assert_likelihood(Sv, value, C=None):
    """`Sv`: the symmetric matrix found (for the plain variable: its symmetric part)."""
    C = likelihood_C() if C is None else C
    Ss, vs = likelihood_optimum(C)
    print("Gaussian likelihood: %.12g (closed form %.12g)" % (value, vs))
    assert abs(value - vs) <= VALUE_TOL * abs(vs), (value, vs)
    assert np.max(np.abs(Sv - Ss)) <= POINT_TOL * np.max(np.abs(Ss)), (Sv, Ss)


def matrix_from_entries(sv, n):
    return (sym_map(n) @ np.asarray(sv, dtype=float)).reshape(n, n, order="F")


# ---- (3) D-optimal design: maximise log det sum_i lam_i v_i v_i^T on the simplex ---------------------------------------------
def design_points(kind="three"):
    if kind == "three":                                   # the regression points (1, x, x^2) at x = -1, 0, 1
        xs = np.array([-1.0, 0.0, 1.0])
        return np.stack([np.ones(3), xs, xs * xs], axis=1)
    return np.random.default_rng(23).standard_normal((12, 3))


def design_problem(V):
    import dnlp_amd as cp
    p, n = V.shape
    W = np.stack([np.outer(v, v).reshape(-1, order="F") for v in V], axis=1)        # (n^2, p)
    lam = cp.Variable(p, name="lam")
    lam.value = np.arange(1.0, p + 1) / np.sum(np.arange(1.0, p + 1))      # (not the answer of the three-point design)
    M = cp.reshape(W @ lam, (n, n), order="F")
    return cp.Problem(cp.Maximize(cp.log_det(M)), [lam >= 0, cp.sum(lam) == 1]), lam


def assert_design(V, lv, value):
    """The equivalence theorem (Kiefer-Wolfowitz): lam is D-optimal iff max_i v_i^T M^-1 v_i = n, attained on the support."""
    p, n = V.shape
    viol = max(float(np.max(-lv)), abs(float(np.sum(lv)) - 1.0), 0.0)
    assert viol <= VIOLATION_TOL, viol
    M = V.T @ (lv[:, None] * V)
    assert abs(value - float(np.linalg.slogdet(M)[1])) <= VALUE_TOL * max(1.0, abs(value))
    var = np.einsum("ij,jk,ik->i", V, np.linalg.inv(M), V)
    support = lv > 1e-5
    print("D-optimal design: log det %.12g, variance function max %.9g, support %d of %d" % (value, var.max(), support.sum(), p))
    assert np.max(var) <= n * (1.0 + POINT_TOL), var
    assert np.max(np.abs(var[support] - n)) <= n * POINT_TOL, var[support]
    if p == n:
        assert np.max(np.abs(lv - 1.0 / n)) <= POINT_TOL


# ---- (4) the largest ellipsoid {B u + d : |u| <= 1} in the box |x_i| <= r_i ------------------------------------------------------
BOX_R = np.array([1.0, 2.0, 0.5])


def ellipsoid_problem():
    import dnlp_amd as cp
    A = np.vstack([np.eye(3), -np.eye(3)])
    b = np.concatenate([BOX_R, BOX_R])
    s = cp.Variable(6, name="s")
    s.value = sym_entries(0.25 * np.eye(3))
    d = cp.Variable(3, name="d")
    d.value = np.zeros(3)
    B = cp.reshape(sym_map(3) @ s, (3, 3), order="F")
    return cp.Problem(cp.Maximize(cp.log_det(B)), [cp.norm(B @ A.T, 2, axis=0) + A @ d <= b]), s, d


def assert_ellipsoid(sv, dvv, value):
    Bv = matrix_from_entries(sv, 3)
    vs = float(np.sum(np.log(BOX_R)))
    print("ellipsoid in the box: log det %.12g (closed form %.12g)" % (value, vs))
    assert abs(value - vs) <= VALUE_TOL * max(1.0, abs(vs)), (value, vs)
    assert np.max(np.abs(Bv - np.diag(BOX_R))) <= POINT_TOL * np.max(BOX_R), Bv
    assert np.max(np.abs(dvv)) <= POINT_TOL * np.max(BOX_R), dvv


# ---- tapes that hold given matrices, written straight into x at the indices the segments read ----------------------------------
def matrices_tape(constraint_mats, objective_mats=(), extra=None):
    """One `log_det(V) <= 0` row per matrix of `constraint_mats` and one term log_det(V) of the objective per matrix of
    `objective_mats` (`extra(cp)`: further constraints, appended).  The canonical form gives every atom a variable T of its
    own with the row T == (V + V^T) / 2; the matrix is written into T, so the rule is evaluated at a point where its
    argument need not be symmetric.  -> (tape arrays, x, multipliers, sigma)."""
    import dnlp_amd as cp
    from lse_problems import lower, multipliers

    def atom(A):
        V = cp.Variable(A.shape)
        V.value = np.eye(A.shape[0])
        return cp.log_det(V)

    obj = 0 * cp.sum(cp.Variable(1))
    for A in objective_mats:
        obj = obj + atom(A)
    cons = [atom(A) <= 0 for A in constraint_mats] + (extra(cp) if extra else [])
    a = dict(lower(cp.Problem(cp.Minimize(obj), cons))["tape_arrays"])
    fill = list(objective_mats) + list(constraint_mats)
    assert list(a["seg_op"][:len(fill)]) == [37] * len(fill)
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x = np.random.default_rng(41).uniform(0.5, 1.5, N)
    seen = np.zeros(N, dtype=bool)
    for s, A in enumerate(fill):
        n = A.shape[0]
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + n * n], dtype=np.int64)
        assert (int(a["seg_d0"][s]), int(a["seg_d1"][s]), int(a["seg_d2"][s])) == (1, n * n, n) and not seen[idx].any()
        x[idx] = np.asarray(A, dtype=float).reshape(-1, order="F")
        seen[idx] = True
    return a, x, multipliers(m), 0.5
