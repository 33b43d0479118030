"""TEST INFRASTRUCTURE -- solves with row-wise 2-norms that have closed forms (Fermat-Weber point of a square, smallest
enclosing circle, group lasso along either axis, Fermat-Weber with the anchors as a Parameter), each also written as
the loop of scalar norms that was the only statement before, and tapes that hold given rows; shared by the CPU and
the GPU tests."""
import numpy as np

# the tolerances of tests/prod_problems.py (test_prod_cpu.py::test_host_build_box_volume -> assert_box): the value
# relative to the closed form, the point relative to its largest entry
VALUE_TOL = 1e-6
POINT_TOL = 1e-4


def assert_optimum(name, value, want_value, point, want_point):
    point, want_point = np.asarray(point, dtype=float), np.asarray(want_point, dtype=float)
    print("%s: %.12g (closed form %.12g), point error %.3e" % (name, value, want_value, np.max(np.abs(point - want_point))))
    assert abs(value - want_value) <= VALUE_TOL * abs(want_value), (value, want_value)
    assert np.max(np.abs(point - want_point)) <= POINT_TOL * np.max(np.abs(want_point)), (point, want_point)


def _spread(cp, p, rows):
    """1 p^T: the point p (length K) repeated in every one of `rows` rows."""
    return cp.Constant(np.ones((rows, 1))) @ cp.reshape(p, (1, p.size), order="F")


# ---- (a) Fermat-Weber: minimise the sum of distances to the unit square's corners --------------------------------------------------
SQUARE = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
FW_POINT, FW_VALUE = np.array([0.5, 0.5]), 2.0 * np.sqrt(2.0)
FW_START = np.array([0.3, 0.6])


def fermat_weber(loop=False, anchors=SQUARE, parameters=False, start=True):
    import dnlp_amd as cp
    p = cp.Variable(2, name="p")
    if start:                            # (False: no start value, for best_of sampling)
        p.value = FW_START
    A = cp.Parameter(anchors.shape, name="A", value=np.asarray(anchors, dtype=float)) if parameters else anchors
    if loop:
        obj = sum(cp.norm(p - A[i], 2) for i in range(anchors.shape[0]))
    else:
        obj = cp.sum(cp.norm(_spread(cp, p, anchors.shape[0]) - A, 2, axis=1))
    prob = cp.Problem(cp.Minimize(obj))
    return (prob, p, [A]) if parameters else (prob, p)


# ---- (b) smallest enclosing circle of (0,0), (2,0), (0,2) --------------------------------------------------------------------------
CIRCLE_POINTS = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]])
CIRCLE_CENTRE, CIRCLE_RADIUS = np.array([1.0, 1.0]), np.sqrt(2.0)
# (0, 0) lies on the optimal circle with multiplier 0, so the centre moves along (1, 1) at second order in the radius and
# converges like the square root of the complementarity the interior-point loop stops at: 2.0e-4 at the default tol 1e-7,
# 2.5e-5 at 1e-9, 6.9e-6 at 1e-10 (host build, both statements).  The instance is solved at 1e-10 and held to POINT_TOL.
CIRCLE_OPTS = {"tol": 1e-10}
VIOLATION_TOL = 1e-8     # tests/prod_problems.py


def assert_circle(name, radius, centre):
    far = float(np.max(np.linalg.norm(CIRCLE_POINTS - centre, axis=1)))
    print("enclosing circle, %s: r = %.12g, centre %r, farthest point at %.12g" % (name, radius, centre, far))
    assert_optimum("enclosing circle, " + name, radius, CIRCLE_RADIUS, centre, CIRCLE_CENTRE)
    assert far - radius <= VIOLATION_TOL, far - radius


def enclosing_circle(loop=False):
    import dnlp_amd as cp
    c, r = cp.Variable(2, name="c"), cp.Variable(name="r")
    c.value, r.value = np.array([0.4, 0.7]), 3.0
    n = CIRCLE_POINTS.shape[0]
    if loop:
        cons = [cp.norm(CIRCLE_POINTS[i] - c, 2) <= r for i in range(n)]
    else:
        cons = [cp.norm(CIRCLE_POINTS - _spread(cp, c, n), 2, axis=1) <= cp.promote(r, (n,))]
    return cp.Problem(cp.Minimize(r), cons), c, r


# ---- (c) group lasso: minimise 1/2 ||X - B||_F^2 + lam sum_r ||X_r||_2 -------------------------------------------------------------
LASSO_B = np.array([[3.0, 4.0, 0.0], [1.0, -2.0, 2.0], [-6.0, 2.0, 3.0], [0.5, 1.5, -1.0], [2.0, 2.0, 1.0]])
LASSO_LAM = 1.0


def lasso_optimum(B=LASSO_B, lam=LASSO_LAM):
    """Every ||B_r|| > lam, so no row sits at the kink: X_r = (1 - lam / ||B_r||) B_r."""
    nb = np.linalg.norm(B, axis=1)
    assert np.all(nb > lam)
    X = (1.0 - lam / nb)[:, None] * B
    return X, float(0.5 * np.sum((X - B) ** 2) + lam * np.sum(np.linalg.norm(X, axis=1)))


def group_lasso(axis=1, loop=False, B=LASSO_B, lam=LASSO_LAM):
    """axis = 0: the same problem on the transposed data (groups are columns)."""
    import dnlp_amd as cp
    D = B if axis == 1 else B.T
    X = cp.Variable(D.shape, name="X")
    X.value = D.copy()
    if loop:
        groups = [X[r, :] for r in range(D.shape[0])] if axis == 1 else [X[:, r] for r in range(D.shape[1])]
        pen = sum(cp.norm(g, 2) for g in groups)
    else:
        pen = cp.sum(cp.norm(X, 2, axis=axis))
    return cp.Problem(cp.Minimize(0.5 * cp.sum_squares(X - D) + lam * pen)), X


# ---- tapes that hold given rows, atom arguments written straight into x (the scheme of lse_problems.rows_tape) ---------------------
def rows_tape(sets, axis=1):
    """One `quad_over_lin_rows(V, Y, axis) <= 0` block per (U (M, K), y (M)) pair of `sets`; axis 1: V is M x K, axis 0: V
    is K x M, axis None: M must be 1.  -> (tape arrays, x, multipliers, sigma) with x holding the rows and their
    denominators at the indices the segments read."""
    import dnlp_amd as cp
    from lse_problems import lower, multipliers

    def atom(U):
        M, K = U.shape
        if axis is None:
            assert M == 1
            V, Y = cp.Variable(K), cp.Variable()
        else:
            V, Y = cp.Variable((M, K) if axis == 1 else (K, M)), cp.Variable(M)
        V.value, Y.value = np.ones(V.shape), np.ones(Y.shape)
        return cp.quad_over_lin_rows(V, Y, axis=axis)

    cons = [atom(U) <= 0 for U, y in sets]
    a = dict(lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), cons))["tape_arrays"])
    assert list(a["seg_op"]) == [36] * len(sets)
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x = np.zeros(N)
    seen = np.zeros(N, dtype=bool)
    for s, (U, y) in enumerate(sets):
        off, off1 = int(a["seg_a0_off"][s]), int(a["seg_a1_off"][s])
        idx = np.asarray(a["gidx"][off:off + U.size], dtype=np.int64)
        yidx = np.asarray(a["gidx"][off1:off1 + y.size], dtype=np.int64)
        assert (int(a["seg_d0"][s]), int(a["seg_d1"][s])) == U.shape and not seen[idx].any() and not seen[yidx].any()
        x[idx], x[yidx] = U.reshape(-1), y
        seen[idx] = seen[yidx] = True
    return a, x, multipliers(m), 0.5


# ---- (d) the smallest example: minimise sum_r ||X_r||_2 subject to X >= lo ----------------------------------------------------------
def norms_over_a_bound(loop=False, rows=5, cols=3, lo=0.1):
    """Every entry ends at its bound: value rows * lo * sqrt(cols)."""
    import dnlp_amd as cp
    X = cp.Variable((rows, cols), name="X")
    X.value = np.ones((rows, cols))
    obj = sum(cp.norm(X[r, :], 2) for r in range(rows)) if loop else cp.sum(cp.norm(X, 2, axis=1))
    return cp.Problem(cp.Minimize(obj), [X >= lo]), X, rows * lo * np.sqrt(cols)
