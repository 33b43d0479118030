"""TEST INFRASTRUCTURE -- the three log_sum_exp solves (softmax regression, a log-form geometric program, a nonconvex
maximisation) with their certificates written out in numpy, shared by the CPU and the GPU tests."""
import numpy as np
from scipy.special import logsumexp, softmax

RIDGE = 1e-2
GAP_TOL = 1e-4          # tests/convex_certificates.py: the reference's cross-check tolerance
VIOLATION_TOL = 1e-8    # tests/test_paper_examples.py
STATIONARITY_TOL = 1e-6


# ---- (a) softmax regression -----------------------------------------------------------------------------------------
def softmax_data(samples=120, features=4, classes=3, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((samples, features))
    W_true = rng.standard_normal((features, classes))
    labels = np.array([rng.choice(classes, p=softmax(row)) for row in X @ W_true])
    Y = np.eye(classes)[labels]
    return X, Y


def softmax_problem(X, Y, ridge=RIDGE):
    import dnlp_amd as cp
    W = cp.Variable((X.shape[1], Y.shape[1]), name="W")
    W.value = np.zeros(W.shape)
    S = X @ W
    obj = cp.sum(cp.log_sum_exp(S, axis=1)) - cp.sum(cp.multiply(Y, S)) + ridge * cp.sum_squares(W)
    return cp.Problem(cp.Minimize(obj), []), W


def softmax_certificate(X, Y, Wv, ridge=RIDGE):
    """-> (F(W), certified gap): F is 2 ridge-strongly convex, so F(W) - F* <= ||grad F(W)||^2 / (4 ridge)."""
    S = X @ Wv
    F = float(np.sum(logsumexp(S, axis=1)) - np.sum(Y * S) + ridge * np.sum(Wv * Wv))
    grad = X.T @ (softmax(S, axis=1) - Y) + 2 * ridge * Wv
    return F, float(np.sum(grad * grad) / (4 * ridge))


def assert_softmax(X, Y, Wv, value=None, ridge=RIDGE):
    F, gap = softmax_certificate(X, Y, Wv, ridge)
    print("softmax regression: F = %.12g, certified gap %.3e" % (F, gap))
    assert gap <= GAP_TOL * max(1.0, abs(F)), (F, gap)
    if value is not None:
        assert abs(value - F) <= 1e-9 * max(1.0, abs(F)), (value, F)
    return F


# ---- (b) the box-design geometric program in log form -----------------------------------------------------------------
# maximise h w d  subject to  2 (h w + h d) <= A_wall,  w d <= A_floor,  alpha <= h / w <= beta,  gamma <= d / w <= delta
GP_RATIOS = (0.5, 2.0, 0.5, 2.0)
GP_AREAS = (100.0, 10.0)


def gp_problem(a_wall=GP_AREAS[0], a_floor=GP_AREAS[1], parameters=False):
    """y = (log h, log w, log d).  With parameters=True the two areas enter as Parameters holding their logarithms
    (the tape must be affine in a Parameter)."""
    import dnlp_amd as cp
    al, be, ga, de = GP_RATIOS
    y = cp.Variable(3, name="y")
    y.value = np.zeros(3)
    if parameters:
        lw = cp.Parameter(1, name="log_a_wall", value=np.array([np.log(a_wall)]))
        lf = cp.Parameter(1, name="log_a_floor", value=np.array([np.log(a_floor)]))
        lwall, lfloor = lw[0], lf[0]
    else:
        lwall, lfloor = float(np.log(a_wall)), float(np.log(a_floor))
    c2 = float(np.log(2.0))
    wall = cp.log_sum_exp(cp.hstack([y[0] + y[1] + c2 - lwall, y[0] + y[2] + c2 - lwall])) <= 0
    cons = [wall, y[1] + y[2] <= lfloor,
            y[0] - y[1] >= float(np.log(al)), y[0] - y[1] <= float(np.log(be)),
            y[2] - y[1] >= float(np.log(ga)), y[2] - y[1] <= float(np.log(de))]
    prob = cp.Problem(cp.Minimize(-(y[0] + y[1] + y[2])), cons)
    return (prob, y, [lw, lf]) if parameters else (prob, y)


def gp_constraints(yv, a_wall=GP_AREAS[0], a_floor=GP_AREAS[1]):
    """g(y) <= 0 of the seven inequalities, and their Jacobian."""
    al, be, ga, de = GP_RATIOS
    c = np.log(2.0) - np.log(a_wall)
    t = np.array([yv[0] + yv[1] + c, yv[0] + yv[2] + c])
    p = softmax(t)
    g = np.array([logsumexp(t), yv[1] + yv[2] - np.log(a_floor), np.log(al) - (yv[0] - yv[1]), (yv[0] - yv[1]) - np.log(be),
                  np.log(ga) - (yv[2] - yv[1]), (yv[2] - yv[1]) - np.log(de)])
    J = np.array([[1.0, p[0], p[1]], [0, 1, 1], [-1, 1, 0], [1, -1, 0], [0, 1, -1], [0, -1, 1]])
    return g, J


def gp_slsqp(a_wall=GP_AREAS[0], a_floor=GP_AREAS[1]):
    """scipy's SLSQP on the same problem with analytic gradients -> (objective, y)."""
    from scipy.optimize import minimize
    res = minimize(lambda v: -np.sum(v), np.zeros(3), jac=lambda v: -np.ones(3), method="SLSQP",
                   constraints=[{"type": "ineq", "fun": lambda v: -gp_constraints(v, a_wall, a_floor)[0],
                                 "jac": lambda v: -gp_constraints(v, a_wall, a_floor)[1]}],
                   options={"ftol": 1e-14, "maxiter": 500})
    assert res.success, res.message
    assert np.max(gp_constraints(res.x, a_wall, a_floor)[0]) <= VIOLATION_TOL
    return float(res.fun), res.x


def assert_gp(yv, value, a_wall=GP_AREAS[0], a_floor=GP_AREAS[1]):
    ref, _ = gp_slsqp(a_wall, a_floor)
    viol = float(np.max(gp_constraints(yv, a_wall, a_floor)[0]))
    print("box GP: objective %.12g (SLSQP %.12g), violation %.3e" % (value, ref, viol))
    assert viol <= VIOLATION_TOL, viol
    assert abs(value + np.sum(yv)) <= 1e-9 * max(1.0, abs(value))
    assert abs(value - ref) <= 1e-4 * max(1.0, abs(ref)), (value, ref)


# ---- (c) a nonconvex use: maximise log_sum_exp(A x) on the unit sphere ------------------------------------------------------
def sphere_data(seed=5):
    return np.random.default_rng(seed).standard_normal((8, 3))


def sphere_problem(A, start=None):
    import dnlp_amd as cp
    x = cp.Variable(3, name="x")
    if start is not False:               # (False: no start value, for best_of sampling)
        x.value = np.array([0.6, -0.5, 0.4]) if start is None else start
    return cp.Problem(cp.Maximize(cp.log_sum_exp(A @ x)), [cp.sum_squares(x) == 1]), x


def assert_sphere_kkt(A, xv, mult):
    """Stationarity and violation of the ORIGINAL problem; `mult` is the multiplier of the sphere row of the canonical
    minimisation (-log_sum_exp): -grad f + mult * 2 x = 0."""
    grad = A.T @ softmax(A @ xv)
    stat = float(np.max(np.abs(-grad + mult * 2.0 * xv)))
    viol = abs(float(xv @ xv) - 1.0)
    print("sphere: stationarity %.3e, violation %.3e" % (stat, viol))
    assert stat <= STATIONARITY_TOL, stat
    assert viol <= VIOLATION_TOL, viol


# ---- tapes that hold given rows, atom arguments written straight into x (the scheme of test_atom_rules._tape) ---------------
def multipliers(m):
    """+-2^k, k in -2..2, neighbours always different (test_atom_rules._multipliers)."""
    i = np.arange(m)
    return np.where((i // 5) % 2 == 0, 1.0, -1.0) * 2.0 ** ((i % 5) - 2)


def lower(prob):
    from dnlp_amd.dnlp2smooth import Dnlp2Smooth
    from dnlp_amd.nlp_solver import build_nlp_data
    smooth, _ = Dnlp2Smooth().apply(prob)
    return build_nlp_data(smooth)[0]


def value_in(prob, var, xv):
    """The entries of user variable `var` in a canonical solution vector of `prob` (the canonical variable order is a
    function of the problem alone)."""
    import dnlp_amd as cp
    if isinstance(prob.objective, cp.Maximize):
        prob = cp.Problem(cp.Minimize(-prob.objective.expr), prob.constraints)
    off = lower(prob)["tape"].var_offsets[id(var)]
    return np.asarray(xv[off:off + var.size]).reshape(var.shape, order="F")


def rows_tape(constraint_sets, objective_sets=(), axis=1):
    """One `log_sum_exp(V, axis) <= 0` block per (M, K) array of `constraint_sets` and one term sum(log_sum_exp(V, axis)) of
    the objective per array of `objective_sets`; axis 1: V is M x K, axis 0: V is K x M, axis None: M must be 1.
    -> (tape arrays, x, multipliers, sigma) with x holding the rows at the indices the segments read."""
    import dnlp_amd as cp

    def atom(rows):
        M, K = rows.shape
        if axis is None:
            assert M == 1
            V = cp.Variable(K)
        else:
            V = cp.Variable((M, K) if axis == 1 else (K, M))
        V.value = np.ones(V.shape)
        return cp.log_sum_exp(V, axis=axis)

    obj = 0 * cp.sum(cp.Variable(1))
    for rows in objective_sets:
        obj = obj + cp.sum(atom(rows))
    cons = [atom(rows) <= 0 for rows in constraint_sets]
    a = dict(lower(cp.Problem(cp.Minimize(obj), cons))["tape_arrays"])
    fill = list(objective_sets) + list(constraint_sets)
    assert list(a["seg_op"]) == [34] * len(fill)
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x = np.zeros(N)
    seen = np.zeros(N, dtype=bool)
    for s, rows in enumerate(fill):
        off = int(a["seg_a0_off"][s])
        idx = np.asarray(a["gidx"][off:off + rows.size], dtype=np.int64)
        assert (int(a["seg_d0"][s]), int(a["seg_d1"][s])) == rows.shape and not seen[idx].any()
        x[idx] = rows.reshape(-1)
        seen[idx] = True
    return a, x, multipliers(m), 0.5
