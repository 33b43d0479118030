"""TEST INFRASTRUCTURE — four small problems over atan2, cosh, atan and asin / acos, each with an optimum computed on the
CPU by scipy, independent of the solver and of csrc/:

    bearing     bearing-only localisation: 5 anchors, 2 unknowns, noisy bearings theta_i; minimise the sum of squared
                atan2(p_y - a_iy, p_x - a_ix) - theta_i.  Every anchor lies left of the target (and of the start), so every line
                of sight is at least 0.5 rad away from the cut of atan2 along the negative x axis (asserted below)
    cosh        minimise sum(cosh(A x - b)), A of 30 x 6: unconstrained and convex
    step        an arctangent step fit y ~ a atan(b t + c), 40 points, least squares in (a, b, c)
    arcs        minimise sum_squares(asin(x) - phi) + rho square(sum(acos(x)) - s), x of length 5; phi_0 = 1.54 lies 0.03 below
                asin's largest value, so the optimum has x_0 within 1e-3 of the bound 1 (asserted below) without reaching it

The optima are the constants ANSWERS below.  They were produced by this script (scipy 1.15.3; run from the repository root):

    import sys; sys.path[:0] = ['.', 'tests']
    import numpy as np, scipy.optimize as so, trig_problems as tp
    def gauss_newton(res, jac, x):             # small residuals: the iteration contracts by a factor of a few hundred
        for _ in range(30): x = x - np.linalg.lstsq(jac(x), res(x), rcond=None)[0]
        return x
    def best(res, jac, starts):                # analytic Jacobians; every start must end at the same point to 1e-12
        sols = [gauss_newton(res, jac, so.least_squares(res, s0, jac=jac).x) for s0 in starts]
        assert max(np.max(np.abs(s - sols[0])) for s in sols) < 1e-12
        return sols[0], float(np.sum(res(sols[0]) ** 2))
    rng = np.random.default_rng(0)
    anchors, theta = tp.bearing_data()
    d = lambda p: (p[1] - anchors[:, 1], p[0] - anchors[:, 0])
    print('bearing', best(lambda p: np.arctan2(*d(p)) - theta,
                          lambda p: np.stack([-d(p)[0], d(p)[1]], axis=1) / (d(p)[0] ** 2 + d(p)[1] ** 2)[:, None],
                          [tp.BEARING_START + 0.3 * rng.standard_normal(2) for _ in range(8)]))
    A, b = tp.cosh_data()
    f = lambda x: np.sum(np.cosh(A @ x - b)); g = lambda x: A.T @ np.sinh(A @ x - b)
    H = lambda x: A.T @ (np.cosh(A @ x - b)[:, None] * A)
    sols = []
    for _ in range(4):
        x = so.minimize(f, rng.standard_normal(6), jac=g, method='BFGS', options={'gtol': 1e-10}).x
        for _ in range(5): x = x - np.linalg.solve(H(x), g(x))
        sols.append(x)
    assert max(np.max(np.abs(s - sols[0])) for s in sols) < 1e-12
    print('cosh', sols[0], f(sols[0]), np.max(np.abs(g(sols[0]))))
    t, y = tp.step_data()
    q = lambda v: 1 + (v[1] * t + v[2]) ** 2
    print('step', best(lambda v: v[0] * np.arctan(v[1] * t + v[2]) - y,
                       lambda v: np.stack([np.arctan(v[1] * t + v[2]), v[0] * t / q(v), v[0] / q(v)], axis=1),
                       [tp.STEP_START * (1 + 0.2 * rng.standard_normal(3)) for _ in range(8)]))
    phi, s, rho = tp.arcs_data()               # with x = sin(v), |v| < pi / 2: asin(x) = v and acos(x) = pi / 2 - v, so the
    M = np.vstack([np.eye(5), -np.sqrt(rho) * np.ones((1, 5))])     # problem is LINEAR least squares in v
    rhs = np.concatenate([phi, [np.sqrt(rho) * (s - 5 * np.pi / 2)]])
    v = np.linalg.lstsq(M, rhs, rcond=None)[0]
    assert np.all(np.abs(v) < np.pi / 2)
    print('arcs', np.sin(v), float(np.sum((M @ v - rhs) ** 2)))

Each builder returns (problem, variable, expected point, expected value).  Objective and point are held to 1e-6 relative, the
project's tolerance for a solve."""
import numpy as np

import dnlp_amd as cp

REL_TOL = 1e-6
CUT_MARGIN = 0.5

ANSWERS = {
    "bearing": (np.array([1.4706461279475391, 0.4222080938997084]), 0.003170175746076134),
    "cosh": (np.array([-0.08476626623114068, -0.1264414095586822, -0.07488012786048807, 0.1990460114797615, 0.17468685101699832,
                       0.07793735404009586]), 39.44397693464555),
    "step": (np.array([1.2984175774987066, 4.009598278342859, -2.005819234275267]), 0.004658290095561625),
    "arcs": (np.array([0.9995853388851558, 0.5662898517572899, -0.38757786135382577, 0.10182061390241552, -0.840390119985837]), 2.7926584085200917e-05),
}


# ---- bearing-only localisation -----------------------------------------------------------------------------------------------------
BEARING_ANCHORS = np.array([[-2.0, -3.0], [-1.0, 3.0], [-3.0, 0.5], [0.0, -2.5], [-0.5, 2.0]])
BEARING_TARGET = np.array([1.5, 0.4])
BEARING_START = np.array([1.0, 0.0])
BEARING_NOISE = 0.02


def bearings(target, noise_seed=None):
    d = np.asarray(target, float)[None, :] - BEARING_ANCHORS
    th = np.arctan2(d[:, 1], d[:, 0])
    if noise_seed is not None:
        th = th + BEARING_NOISE * np.random.default_rng(noise_seed).standard_normal(th.size)
    assert np.all(np.abs(th) <= np.pi - CUT_MARGIN), "a line of sight within 0.5 rad of the cut"
    return th


def bearing_data():
    return BEARING_ANCHORS, bearings(BEARING_TARGET, noise_seed=21)


def _bearing_objective(p, theta):
    ax, ay = BEARING_ANCHORS[:, 0], BEARING_ANCHORS[:, 1]
    return cp.sum_squares(cp.atan2(p[1] - ay, p[0] - ax) - theta)


def bearing_problem():
    _, theta = bearing_data()
    p = cp.Variable(2)
    p.value = BEARING_START.copy()
    assert np.all(np.abs(bearings(BEARING_START)) <= np.pi - CUT_MARGIN)
    return (cp.Problem(cp.Minimize(_bearing_objective(p, theta))), p) + ANSWERS["bearing"]


def bearing_template():
    """The same problem with the bearings as a Parameter: (problem, [theta], p)."""
    theta = cp.Parameter(BEARING_ANCHORS.shape[0], name="theta", value=bearing_data()[1])
    p = cp.Variable(2)
    p.value = BEARING_START.copy()
    return cp.Problem(cp.Minimize(_bearing_objective(p, theta))), [theta], p


def bearing_rows(count, seed=31):
    """`count` bearing vectors: row 0 is bearing_data(); the others are the noisy bearings of targets planted within 0.3 of
    BEARING_TARGET, all right of every anchor, so every instance stays away from the cut."""
    rng = np.random.default_rng(seed)
    rows = [bearing_data()[1]]
    for k in range(1, count):
        rows.append(bearings(BEARING_TARGET + rng.uniform(-0.3, 0.3, 2), noise_seed=1000 + k))
    return np.stack(rows)


# ---- sum of cosh ---------------------------------------------------------------------------------------------------------------------
def cosh_data(seed=22):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((30, 6)), rng.standard_normal(30)


def cosh_problem():
    A, b = cosh_data()
    x = cp.Variable(6)
    x.value = np.zeros(6)
    return (cp.Problem(cp.Minimize(cp.sum(cp.cosh(A @ x - b)))), x) + ANSWERS["cosh"]


def cosh_gradient(x):
    A, b = cosh_data()
    return A.T @ np.sinh(A @ np.asarray(x, float).reshape(-1) - b)


# ---- arctangent step fit ---------------------------------------------------------------------------------------------------------------
STEP_TRUE = np.array([1.3, 4.0, -2.0])
STEP_START = np.array([1.0, 3.0, -1.5])


def step_data(seed=23):
    t = np.linspace(0.0, 1.0, 40)
    a, b, c = STEP_TRUE
    return t, a * np.arctan(b * t + c) + 0.01 * np.random.default_rng(seed).standard_normal(t.size)


def step_problem():
    t, y = step_data()
    v = cp.Variable(3)
    v.value = STEP_START.copy()
    return (cp.Problem(cp.Minimize(cp.sum_squares(cp.multiply(v[0], cp.atan(v[1] * t + v[2])) - y))), v) + ANSWERS["step"]


# ---- asin / acos -------------------------------------------------------------------------------------------------------------------------
def arcs_data():
    """phi, s, rho.  sin(phi_0) = 1 - 4.7e-4, and s lies 0.014 below sum(pi / 2 - phi): the coupling pushes every x_i up a little."""
    phi = np.array([1.54, 0.6, -0.4, 0.1, -1.0])
    return phi, 7.0, 0.5


def arcs_problem():
    phi, s, rho = arcs_data()
    x = cp.Variable(5)
    x.value = np.sin(np.clip(phi, -1.2, 1.2))
    obj = cp.sum_squares(cp.asin(x) - phi) + rho * cp.square(cp.sum(cp.acos(x)) - s)
    assert 0.0 < 1.0 - ANSWERS["arcs"][0][0] < 1e-3
    return (cp.Problem(cp.Minimize(obj)), x) + ANSWERS["arcs"]


SOLVES = {"bearing": bearing_problem, "cosh": cosh_problem, "step": step_problem, "arcs": arcs_problem}
# the three ways every solve is run on the device
MODES = {"in_kernel": {"device_loop": "yes"}, "host_driven": {"device_loop": "no"},
         "limited_memory": {"hessian_approximation": "limited-memory"}}
# the default tol = 1e-8 stops where the value is good to 1e-6; the point of a flat least-squares valley needs more
SOLVE_OPTS = {"bearing": {"tol": 1e-10}, "cosh": {"tol": 1e-10}, "step": {"tol": 1e-10}, "arcs": {"tol": 1e-10}}


def assert_solution(name, prob, var, xs, fs):
    assert prob.status == cp.OPTIMAL, (name, prob.status)
    assert abs(prob.value - fs) <= REL_TOL * abs(fs), (name, prob.value, fs)
    got = np.asarray(var.value).reshape(-1)
    assert np.max(np.abs(got - xs)) <= REL_TOL * np.max(np.abs(xs)), (name, got, xs)
