"""TEST INFRASTRUCTURE -- the matrix_frac / tr_inv solves with closed forms or certificates (Gaussian maximum likelihood in
covariance form, a diagonal covariance, generalised least squares through a constraint, A-optimal design), written out in
numpy, and tapes that hold given (P, X) pairs; shared by the CPU and the GPU tests.  None needs the reference."""
import numpy as np

from logdet_problems import POINT_TOL, VALUE_TOL, VIOLATION_TOL, design_points, sym_entries, sym_map   # unchanged tolerances

SOLVE_TOL = 1e-7          # the front-end's default `tol` (dnlp_amd/nlp_solver.py HIPNLP.DEFAULT_OPTIONS); the host build's is tighter
# The certificate of (d) is a statement about multipliers.  At a point whose complementarity products are <= tol, an
# entry lam_i > sqrt(tol) has a bound multiplier z_i <= sqrt(tol), which is the amount by which v_i^T M^-2 v_i may fall short
# of tr(M^-1); the factor 10 covers the interior-point loop's scaling of its own error measure.
CERT_TOL = 10.0 * np.sqrt(SOLVE_TOL)
SUPPORT = np.sqrt(SOLVE_TOL)


# ---- (a) Gaussian maximum likelihood in covariance form: minimise N log det S + tr(Y^T S^-1 Y) -----------------------------------
def samples(n, count, seed=31):
    return np.random.default_rng([seed, n, count]).standard_normal((n, count)) * np.linspace(0.5, 2.0, n)[:, None]


def likelihood_problem(n=3, count=4, width=None, Y=None, parameters=False):
    """S = reshape(E s, (n, n)) with s the free entries of a symmetric matrix, started at the identity; Y is split by
    columns into pieces of at most `width` columns (default: what fits one atom, n + m <= 45).  Nonconvex in S.
    -> (problem, s[, [Y as a Parameter]])."""
    import dnlp_amd as cp
    Y = samples(n, count) if Y is None else np.asarray(Y, dtype=float)
    n, count = Y.shape
    width = (45 - n) if width is None else width
    s = cp.Variable(n * (n + 1) // 2, name="s")
    s.value = sym_entries(np.eye(n))
    S = cp.reshape(sym_map(n) @ s, (n, n), order="F")
    src = cp.Parameter((n, count), name="Y", value=Y) if parameters else Y
    fit = 0
    for c0 in range(0, count, width):
        fit = fit + cp.matrix_frac(src[:, c0:min(c0 + width, count)], S)
    prob = cp.Problem(cp.Minimize(count * cp.log_det(S) + fit))
    return (prob, s, [src]) if parameters else (prob, s)


def likelihood_optimum(Y):
    n, count = Y.shape
    S = Y @ Y.T / count
    return S, count * float(np.linalg.slogdet(S)[1]) + count * n


def assert_likelihood(Sv, value, Y):
    Ss, vs = likelihood_optimum(Y)
    print("covariance-form likelihood: %.12g (closed form %.12g)" % (value, vs))
    assert abs(value - vs) <= VALUE_TOL * max(1.0, abs(vs)), (value, vs)
    assert np.max(np.abs(Sv - Ss)) <= POINT_TOL * np.max(np.abs(Ss)), (Sv, Ss)


# ---- (b) diagonal covariance: minimise sum(d) + y^T diag(d)^-1 y -------------------------------------------------------------------
DIAG_Y = np.array([1.5, -0.25, 2.0, -3.0])


def diagonal_problem(y=DIAG_Y):
    import dnlp_amd as cp
    n = y.size
    E = np.zeros((n * n, n))
    E[np.arange(n) * (n + 1), np.arange(n)] = 1.0           # d -> vec(diag(d)), affine atoms only
    d = cp.Variable(n, name="d")
    d.value = np.ones(n)
    return cp.Problem(cp.Minimize(cp.sum(d) + cp.matrix_frac(y, cp.reshape(E @ d, (n, n), order="F")))), d


def assert_diagonal(dv, value, y=DIAG_Y):
    vs = 2.0 * float(np.sum(np.abs(y)))
    print("diagonal covariance: %.12g (closed form %.12g)" % (value, vs))
    assert abs(value - vs) <= VALUE_TOL * vs, (value, vs)
    assert np.max(np.abs(dv - np.abs(y))) <= POINT_TOL * np.max(np.abs(y)), dv


# ---- (c) generalised least squares through a constraint: minimise t, matrix_frac(A x - b, S) <= t, S == S0 ---------------------------
def gls_data(rows=6, cols=3, seed=37):
    rng = np.random.default_rng(seed)
    A, b = rng.standard_normal((rows, cols)), rng.standard_normal(rows)
    R = rng.standard_normal((rows, 2 * rows))
    return A, b, R @ R.T / (2 * rows) + 0.2 * np.eye(rows)


def gls_problem():
    import dnlp_amd as cp
    A, b, S0 = gls_data()
    x, t = cp.Variable(A.shape[1], name="x"), cp.Variable(name="t")
    S = cp.Variable(S0.shape, name="S")
    x.value, t.value, S.value = np.zeros(A.shape[1]), 1.0, S0
    return cp.Problem(cp.Minimize(t), [cp.matrix_frac(A @ x - b, S) <= t, S == S0]), x, t


def assert_gls(xv, value):
    A, b, S0 = gls_data()
    Si = np.linalg.inv(S0)
    xs = np.linalg.solve(A.T @ Si @ A, A.T @ Si @ b)
    r = A @ xs - b
    vs = float(r @ Si @ r)
    print("generalised least squares: %.12g (closed form %.12g)" % (value, vs))
    assert abs(value - vs) <= VALUE_TOL * max(1.0, vs), (value, vs)
    assert np.max(np.abs(xv - xs)) <= POINT_TOL * np.max(np.abs(xs)), (xv, xs)


# ---- (d) A-optimal design: minimise tr inv(sum_i lam_i v_i v_i^T) on the simplex ---------------------------------------------------
def a_design_points(kind="unit"):
    return np.eye(3) if kind == "unit" else design_points(kind)


def a_design_problem(V):
    import dnlp_amd as cp
    p, n = V.shape
    W = np.stack([np.outer(v, v).reshape(-1, order="F") for v in V], axis=1)        # (n^2, p)
    lam = cp.Variable(p, name="lam")
    lam.value = np.arange(1.0, p + 1) / np.sum(np.arange(1.0, p + 1))               # (not the answer of the unit design)
    return cp.Problem(cp.Minimize(cp.tr_inv(cp.reshape(W @ lam, (n, n), order="F"))), [lam >= 0, cp.sum(lam) == 1]), lam


def assert_a_design(V, lv, value):
    """lam is A-optimal iff v_i^T M^-2 v_i <= tr(M^-1) for every i, with equality on the support (the stationarity of the
    Lagrangian with the simplex's multiplier tr(M^-1)); tolerances: CERT_TOL, from the solve's own tol."""
    p, n = V.shape
    viol = max(float(np.max(-lv)), abs(float(np.sum(lv)) - 1.0), 0.0)
    assert viol <= VIOLATION_TOL, viol
    Mi = np.linalg.inv(V.T @ (lv[:, None] * V))
    tr = float(np.trace(Mi))
    assert abs(value - tr) <= VALUE_TOL * max(1.0, tr), (value, tr)
    phi = np.einsum("ij,jk,ik->i", V, Mi @ Mi, V)
    support = lv > SUPPORT
    print("A-optimal design: tr inv %.12g, max v^T M^-2 v %.9g, support %d of %d" % (value, phi.max(), support.sum(), p))
    assert np.max(phi) <= tr * (1.0 + CERT_TOL), (phi, tr)
    assert np.max(np.abs(phi[support] - tr)) <= tr * CERT_TOL, (phi[support], tr)
    if np.array_equal(V, np.eye(n)):
        assert np.max(np.abs(lv - 1.0 / n)) <= POINT_TOL and abs(value - n * n) <= VALUE_TOL * n * n


# ---- tapes that hold given (P, X) pairs, written straight into x at the indices the segments read ----------------------------------
def segments_tape(constraint_pairs, objective_pairs=(), extra=None):
    """One `matrix_frac(Xv, Pv) <= 0` row per pair (P, X) of `constraint_pairs` and one term of the objective per pair of
    `objective_pairs` (`extra(cp)`: further constraints, appended).  The canonical form keeps the bare variable Xv and
    gives every atom a variable T of its own with the row T == (Pv + Pv^T) / 2; P is written into T and X into Xv, so
    the rule is evaluated at a point where P need not be symmetric.  -> (tape arrays, x, multipliers, sigma)."""
    import dnlp_amd as cp
    from lse_problems import lower, multipliers
    import matrix_frac_reference as mr

    def atom(P, X):
        Pv, Xv = cp.Variable(P.shape), cp.Variable(X.shape)
        Pv.value, Xv.value = np.eye(P.shape[0]), np.zeros(X.shape)
        return cp.matrix_frac(Xv, Pv)

    obj = 0 * cp.sum(cp.Variable(1))
    for P, X in objective_pairs:
        obj = obj + atom(P, X)
    cons = [atom(P, X) <= 0 for P, X in constraint_pairs] + (extra(cp) if extra else [])
    a = dict(lower(cp.Problem(cp.Minimize(obj), cons))["tape_arrays"])
    fill = list(objective_pairs) + list(constraint_pairs)
    assert list(a["seg_op"][:len(fill)]) == [38] * len(fill)
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x = np.random.default_rng(43).uniform(0.5, 1.5, N)
    seen = np.zeros(N, dtype=bool)
    for s, (P, X) in enumerate(fill):
        n, K = P.shape[0], P.size + X.size
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + K], dtype=np.int64)
        assert (int(a["seg_d0"][s]), int(a["seg_d1"][s]), int(a["seg_d2"][s])) == (1, K, n) and not seen[idx].any()
        x[idx] = mr.row_of(P, X.reshape(n, -1, order="F"))
        seen[idx] = True
    return a, x, multipliers(m), 0.5
