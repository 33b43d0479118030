"""TEST INFRASTRUCTURE -- the prod solves with closed forms (box volume, AM-GM as a constraint with an axis, a nonconvex
minimisation on a sphere, the box volume as a batch template), their certificates written out in numpy, and tapes that
hold given rows; shared by the CPU and the GPU tests."""
import numpy as np

VIOLATION_TOL = 1e-8     # tests/test_paper_examples.py
STATIONARITY_TOL = 1e-6
VALUE_TOL = 1e-6         # relative, against the closed form (the interior-point loop stops at tol 1e-8)


# ---- (a) box volume: maximise prod(x)  subject to  a . x <= c,  x >= lo > 0 ------------------------------------------------------
BOX_A = np.array([1.0, 2.0, 0.5, 4.0])
BOX_C = 12.0
BOX_LO = 0.05


def box_optimum(a=BOX_A, c=BOX_C):
    """AM-GM on the terms a_i x_i: all equal c / K at the optimum (inside x >= lo for the data used here)."""
    x = c / (a.size * a)
    return x, float(np.prod(x))


def box_problem(a=BOX_A, c=BOX_C, parameters=False):
    import dnlp_amd as cp
    K = a.size
    x = cp.Variable(K, name="x")
    x.value = np.full(K, 0.5)
    if parameters:
        pa = cp.Parameter(K, name="a", value=np.asarray(a, dtype=float))
        pc = cp.Parameter(1, name="c", value=np.array([float(c)]))
        cons = [pa @ x <= pc[0], x >= BOX_LO]
        return cp.Problem(cp.Maximize(cp.prod(x)), cons), x, [pa, pc]
    return cp.Problem(cp.Maximize(cp.prod(x)), [a @ x <= c, x >= BOX_LO]), x


def assert_box(xv, value, a=BOX_A, c=BOX_C):
    xs, vs = box_optimum(a, c)
    assert np.all(xs > BOX_LO)
    viol = max(float(a @ xv - c), float(np.max(BOX_LO - xv)), 0.0)
    print("box volume: %.12g (closed form %.12g), violation %.3e" % (value, vs, viol))
    assert viol <= VIOLATION_TOL * max(1.0, c), viol
    assert abs(value - float(np.prod(xv))) <= 1e-9 * abs(vs)
    assert abs(value - vs) <= VALUE_TOL * abs(vs), (value, vs)
    assert np.max(np.abs(xv - xs)) <= 1e-4 * np.max(xs), (xv, xs)


# ---- (b) AM-GM as a constraint with an axis: minimise sum(X)  subject to  prod(X, axis=1) >= b,  X >= lo ----------------------------
# (without X >= lo the problem is unbounded: two entries of a row go to -inf together; the bound is inactive at the optimum)
AMGM_B = np.array([8.0, 1.0, 0.125, 27.0, 2.0])
AMGM_K = 3
AMGM_LO = 1e-2


def amgm_optimum(b=AMGM_B, K=AMGM_K):
    """X_rl = b_r^(1/K); multiplier of row r: 1 = lam_r prod / x = lam_r b_r^(1 - 1/K)."""
    root = b ** (1.0 / K)
    return np.repeat(root[:, None], K, axis=1), root / b


def amgm_problem(b=AMGM_B, K=AMGM_K):
    import dnlp_amd as cp
    X = cp.Variable((b.size, K), name="X")
    X.value = np.full((b.size, K), 2.0)
    return cp.Problem(cp.Minimize(cp.sum(X)), [cp.prod(X, axis=1) >= b, X >= AMGM_LO]), X


def assert_amgm(Xv, value, mult, b=AMGM_B, K=AMGM_K):
    """`mult`: the multipliers of the b.size product rows (the first rows of the canonical g), either sign convention."""
    Xs, lam = amgm_optimum(b, K)
    viol = max(float(np.max(b - np.prod(Xv, axis=1))), 0.0)
    print("AM-GM: sum %.12g (closed form %.12g), violation %.3e" % (value, Xs.sum(), viol))
    assert viol <= VIOLATION_TOL * np.max(b), viol
    assert abs(value - Xs.sum()) <= VALUE_TOL * Xs.sum(), (value, Xs.sum())
    assert np.max(np.abs(Xv - Xs)) <= 1e-4 * np.max(Xs)
    assert np.max(np.abs(np.abs(mult) - lam) / lam) <= 1e-4, (mult, lam)
    # stationarity of the Lagrangian in numpy: 1 - |mult_r| d prod_r / d X_rl = 0
    grad = np.prod(Xv, axis=1, keepdims=True) / Xv
    assert np.max(np.abs(1.0 - np.abs(mult)[:, None] * grad)) <= 1e-5


# ---- (c) nonconvex: minimise prod(x)  subject to  sum_squares(x) == 3,  K = 3 ----------------------------------------------------
SPHERE_START = np.array([1.2, -0.7, 0.9])
SPHERE_GLOBAL = -1.0


def sphere_problem(start=None):
    import dnlp_amd as cp
    x = cp.Variable(3, name="x")
    if start is not False:               # (False: no start value, for best_of sampling)
        x.value = SPHERE_START if start is None else start
    return cp.Problem(cp.Minimize(cp.prod(x)), [cp.sum_squares(x) == 3]), x


def assert_sphere_kkt(xv, mult):
    """Any returned point: grad prod(x) + mult * 2 x = 0 and |x|^2 = 3 (`mult`: the multiplier of the sphere row)."""
    grad = np.array([xv[1] * xv[2], xv[0] * xv[2], xv[0] * xv[1]])
    stat = float(np.max(np.abs(grad + mult * 2.0 * xv)))
    viol = abs(float(xv @ xv) - 3.0)
    print("prod on the sphere: value %.12g, stationarity %.3e, violation %.3e" % (float(np.prod(xv)), stat, viol))
    assert stat <= STATIONARITY_TOL, stat
    assert viol <= VIOLATION_TOL, viol


# ---- tapes that hold given rows, atom arguments written straight into x (the scheme of lse_problems.rows_tape) -------------------
def rows_tape(constraint_sets, objective_sets=(), axis=1):
    """One `prod(V, axis) <= 0` block per (M, K) array of `constraint_sets` and one term sum(prod(V, axis)) of the objective
    per array of `objective_sets`; axis 1: V is M x K, axis 0: V is K x M, axis None: M must be 1.
    -> (tape arrays, x, multipliers, sigma) with x holding the rows at the indices the segments read."""
    import dnlp_amd as cp
    from lse_problems import lower, multipliers

    def atom(rows):
        M, K = rows.shape
        if axis is None:
            assert M == 1
            V = cp.Variable(K)
        else:
            V = cp.Variable((M, K) if axis == 1 else (K, M))
        V.value = np.ones(V.shape)
        return cp.prod(V, axis=axis)

    obj = 0 * cp.sum(cp.Variable(1))
    for rows in objective_sets:
        obj = obj + cp.sum(atom(rows))
    cons = [atom(rows) <= 0 for rows in constraint_sets]
    a = dict(lower(cp.Problem(cp.Minimize(obj), cons))["tape_arrays"])
    fill = list(objective_sets) + list(constraint_sets)
    assert list(a["seg_op"]) == [35] * len(fill)
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
