"""log_sum_exp without a GPU: the front-end atom and its rule tags, the canonical form, the tape layout of the row class
(OP_LOG_SUM_EXP = 34), the rule of the host build (csrc/model.h sweep_rows over host loops) entry by entry against mpmath
(tests/lse_reference.py: closed forms, rows, bound, measured K), and three solves by the host build with certificates
written out in numpy (tests/lse_problems.py)."""
import hashlib

import numpy as np
import pytest
from scipy.special import logsumexp

import dnlp_amd as cp
import lse_problems as lp
import lse_reference as lr
from batch_problems import oracle_solver
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.tape import serialize


# ---- 1. front-end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, 0, 1])
@pytest.mark.parametrize("keepdims", [False, True])
def test_value_and_shape(axis, keepdims):
    v = np.random.default_rng(3).standard_normal((4, 6)) * 30
    X = cp.Variable((4, 6))
    X.value = v
    e = cp.log_sum_exp(X, axis=axis, keepdims=keepdims)
    want = logsumexp(v, axis=axis, keepdims=keepdims)
    assert e.shape == np.shape(want)
    assert np.array_equal(np.asarray(e.value), np.asarray(want))
    assert e.shape == cp.sum(X, axis=axis, keepdims=keepdims).shape


def test_sign_curvature_and_rule_table():
    x, X = cp.Variable(5), cp.Variable((3, 4))
    e = cp.log_sum_exp(x)
    assert e.is_convex() and not e.is_concave() and not e.is_nonneg() and not e.is_nonpos()
    assert cp.log_sum_exp(cp.abs(x)).is_nonneg()
    assert e.is_atom_esr() and e.is_atom_hsr() and e.is_incr(0) and not e.is_decr(0)
    assert e.is_smooth()
    a = cp.log_sum_exp(cp.abs(x))
    assert a.is_esr() and not a.is_hsr()
    b = cp.log_sum_exp(cp.min(X, axis=0))
    assert b.is_hsr() and not b.is_esr()
    inner = cp.log_sum_exp(cp.max(X, axis=1))
    assert cp.Problem(cp.Minimize(inner)).is_dnlp()
    with pytest.raises(cp.DNLPError):
        cp.Problem(cp.Maximize(inner)).solve(nlp=True)
    assert cp.Problem(cp.Maximize(e)).is_dnlp()         # nonconvex, accepted


# ---- 2. canonical form --------------------------------------------------------------------------------------------------------
def test_canonical_form_aliases_the_argument():
    rng = np.random.default_rng(4)
    A, b = rng.standard_normal((6, 3)), rng.standard_normal(6)
    x = cp.Variable(3)
    x.value = rng.standard_normal(3)
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.log_sum_exp(A @ x + b)), [x >= -5]))
    assert len(smooth.constraints) == 2                                  # t == A x + b first, then the user's row
    t = smooth.objective.expr.args[0]
    assert isinstance(t, cp.Variable) and t.shape == (6,) and t.bounds is None
    assert np.array_equal(t.value, A @ x.value + b)
    data = lp.lower(cp.Problem(cp.Minimize(cp.log_sum_exp(A @ x + b)), [x >= -5]))
    a = data["tape_arrays"]
    assert (int(a["dims"][0]), int(a["dims"][1])) == (9, 9)               # N = 3 + 6, m = 6 equalities + 3 bounds rows
    assert np.array_equal(a["cl"][:6], a["cu"][:6])                        # the equality block comes first
    # a bare variable is kept
    smooth2, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.log_sum_exp(x))))
    assert smooth2.objective.expr.args[0] is x and not smooth2.constraints
    # a matrix argument with an axis: one auxiliary variable of the argument's size
    X = cp.Variable((3, 2))
    X.value = np.ones((3, 2))
    smooth3, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(cp.sum(cp.log_sum_exp(A @ X, axis=1)))))
    assert len(smooth3.constraints) == 1 and smooth3.variables()[0].size + smooth3.variables()[1].size == 6 + 12


# ---- 3. layout ----------------------------------------------------------------------------------------------------------------
def _expected_pattern(a, s):
    M, K = int(a["seg_d0"][s]), int(a["seg_d1"][s])
    off = int(a["seg_a0_off"][s])
    idx = np.asarray(a["gidx"][off:off + M * K], dtype=np.int64).reshape(M, K)
    zo = int(a["seg_zoff"][s])
    ii, jj = np.tril_indices(K)
    z = zo + np.arange(M)
    hr, hc = idx[:, ii].reshape(-1), idx[:, jj].reshape(-1)
    return (np.repeat(z, K), idx.reshape(-1), np.maximum(hr, hc), np.minimum(hr, hc), np.repeat(z, ii.size)), idx


@pytest.mark.parametrize("axis", [None, 0, 1])
def test_tape_layout(axis):
    shape = (5,) if axis is None else (4, 3)
    X = cp.Variable(shape)
    X.value = np.arange(np.prod(shape), dtype=float).reshape(shape)
    Y = cp.Variable(shape)
    Y.value = np.ones(shape)
    prob = cp.Problem(cp.Minimize(cp.sum(cp.log_sum_exp(X, axis=axis))), [cp.log_sum_exp(Y, axis=axis) <= 1])
    a = lp.lower(prob)["tape_arrays"]
    M, K = {None: (1, 5), 0: (3, 4), 1: (4, 3)}[axis]
    T = K * (K + 1) // 2
    assert list(a["seg_op"]) == [34, 34] and list(a["seg_d0"]) == [M, M] and list(a["seg_d1"]) == [K, K]
    assert list(a["seg_n"]) == [M, M] and list(a["seg_zcount"]) == [M, M]
    assert list(a["seg_dcount"]) == [M * K] * 2 and list(a["seg_hcount"]) == [M * T] * 2
    assert list(a["seg_zoff"]) == [0, M] and list(a["seg_doff"]) == [0, M * K] and list(a["seg_hoff"]) == [0, M * T]
    want = [np.concatenate(parts) for parts in zip(*[_expected_pattern(a, s)[0] for s in range(2)])]
    for name, w in zip(("drow", "dcol", "hrow", "hcol", "hz"), want):
        assert np.array_equal(a[name], w), name
    # row r of the atom reads the entries the axis says (the variable X starts at x index 0, F order)
    idx = _expected_pattern(a, 0)[1]
    full = np.arange(np.prod(shape)).reshape(shape, order="F")
    rows = full.reshape(1, -1) if axis is None else (full.T if axis == 0 else full)
    assert np.array_equal(idx, rows)


def test_repeated_index_is_refused():
    x = cp.Variable(3)
    x.value = np.ones(3)
    from dnlp_amd.lowering import lower_problem
    with pytest.raises(ValueError, match="twice"):
        lower_problem(cp.log_sum_exp(cp.hstack([x[0], x[1], x[0]])), [], [x])


def test_hessian_count_beyond_the_index_range_is_refused():
    x = cp.Variable(70000)
    from dnlp_amd.lowering import lower_problem
    with pytest.raises(ValueError, match="70000.*2450035000"):
        lower_problem(cp.log_sum_exp(x), [], [x])


PARENT_SHA256 = {       # recorded from the parent commit: tapes without the atom serialise to the same bytes
    "elementwise_zoo": "9bc816aaf10446f156330c9ffeb3c708cc2744223c7d9c6ed465993bf9d154c7",
    "bilinear_matmul": "94bd8d622db1943e965ff6fb8175f1188073c6a3a6d0a846ff6b9ce8cf4c15a6",
    "localization": "d8d7d99b282c4d32cd55f3ea49a5cfa0fa8eea83a2c0b671ea9173dff819554f",
}


@pytest.mark.parametrize("name", sorted(PARENT_SHA256))
def test_tapes_without_the_atom_keep_their_bytes(name):
    import problem_zoo as zoo
    np.random.seed(0)
    p = zoo.ZOO[name](cp)
    p = p[0] if isinstance(p, tuple) else p
    if isinstance(p.objective, cp.Maximize):
        p = cp.Problem(cp.Minimize(-p.objective.expr), p.constraints)
    blob = serialize(lp.lower(p)["tape_arrays"])
    assert hashlib.sha256(bytes(blob)).hexdigest() == PARENT_SHA256[name]


# ---- 4. rule ------------------------------------------------------------------------------------------------------------------
def test_numpy_statement_against_mpmath_establishes_K():
    table = lr.measured_table()
    for kind, (units, where, share, nans) in table.items():
        print("%-14s %.2f units at %r, %.3f %% left out" % (kind, units, where, 100 * share))
        assert nans == 0 and units <= 4.0 and share <= lr.LEFT_OUT_SHARE, (kind, units, where, share, nans)
    assert all(k in (8, 16) for k in lr.measured_K().values()), lr.measured_K()


_tapes = {}


def grid_tape():
    """The grid rows and the finite planted rows as constraints, and the rows of lengths 3, 16 and 65 once more in the
    objective.  (The planted rows stand among the grid's, so that the 2 % cap on what is left out holds per output.)"""
    if "grid" not in _tapes:
        sets = [rows for n, rows in lr.grid()[:-1]] + [lr.planted_rows()[:4]]
        _tapes["grid"] = lp.rows_tape(sets, [lr.rows_of_length(n) for n in (3, 16, 65)])
    return _tapes["grid"]


def minus_inf_tape():
    if "minus_inf" not in _tapes:
        _tapes["minus_inf"] = lp.rows_tape([lr.planted_rows()[4:]])
    return _tapes["minus_inf"]


def check_callbacks(ev, tape, with_f=True, hsample=None):
    a, x, lam, sigma = tape
    exp = lr.expected_oracles(a, x, lam, sigma, hsample)
    for units, kind in zip(exp["units"], ("value", "d1", "d2")):
        share = float(np.mean(units.st == 1)) if units.st.size else 0.0
        assert share <= lr.LEFT_OUT_SHARE, "%s: %.2f %% of the points left out" % (kind, 100 * share)
    failed = []
    checks = [("g", lambda: ev.eval_g(x)), ("jac", lambda: ev.eval_jac_g(x)), ("hess", lambda: ev.eval_h(x, lam, sigma))]
    if with_f:
        checks += [("f", lambda: [ev.eval_f(x)]), ("grad_f", lambda: ev.eval_grad_f(x))]
    for name, thunk in checks:
        try:
            print("%s: worst error %.3f of its bound" % (name, exp[name].check(thunk())))
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "\n".join(failed)


def test_host_build_against_mpmath_on_the_grid():
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(grid_tape()[0])), grid_tape())


def test_host_build_against_mpmath_on_a_row_containing_minus_inf():
    """p = 0 and h = 0 there, exactly; x holds -inf, so f = c . [x; z] is not asked for (0 * -inf)."""
    from oracle.oracle_capi import OracleProblem
    check_callbacks(OracleProblem(serialize(minus_inf_tape()[0])), minus_inf_tape(), with_f=False)


def test_host_build_single_entry_rows_are_exact():
    """K = 1: r = u, p = 1, h = 0 exactly."""
    from oracle.oracle_capi import OracleProblem
    rows = lr.rows_of_length(1)
    a, x, lam, sigma = lp.rows_tape([rows])
    o = OracleProblem(serialize(a))
    sign = float(a["G_val"][0])                  # (how the front-end orients `atom <= 0`)
    assert abs(sign) == 1.0 and np.all(a["G_val"] == sign) and not a["b"].any()
    assert np.array_equal(o.eval_g(x), sign * rows[:, 0]) and np.array_equal(o.eval_jac_g(x), sign * np.ones(40))
    assert np.array_equal(o.eval_h(x, lam, sigma), np.zeros(40))


def test_host_build_nan_and_inf_rows_give_nan():
    from oracle.oracle_capi import OracleProblem
    rows = np.array([[0.5, np.inf, 1.0], [0.5, np.nan, 1.0], [1.0, 2.0, 3.0]])
    a, x, lam, sigma = lp.rows_tape([rows])
    g = OracleProblem(serialize(a)).eval_g(x)
    assert np.isnan(g[0]) and np.isnan(g[1]) and abs(g[2]) == pytest.approx(logsumexp(rows[2]), rel=1e-15)


def test_host_build_single_entry_rows_with_inf_or_nan_give_nan():
    """K = 1 goes through the same expressions as longer rows: exp(u - u) is NaN for +-inf and NaN, as on the device."""
    from oracle.oracle_capi import OracleProblem
    rows = np.array([[np.inf], [np.nan], [-np.inf], [2.5]])
    a, x, lam, sigma = lp.rows_tape([rows])
    o = OracleProblem(serialize(a))
    g, J = o.eval_g(x), o.eval_jac_g(x)
    assert np.isnan(g[:3]).all() and abs(g[3]) == 2.5 and np.isnan(J[:3]).all() and abs(J[3]) == 1.0
    assert o.eval_h(x, lam, sigma)[3] == 0.0


def test_rows_that_share_entries_beyond_the_scratch_are_refused_at_load():
    """A hand-built tape whose rows share entries across rows (more rows of K >= 2 than half the variables) is refused where
    it is loaded, not inside a kernel."""
    from oracle.oracle_capi import OracleProblem
    a, x, lam, sigma = lp.rows_tape([lr.rows_of_length(2, 3)])
    a = dict(a)
    N = int(a["dims"][0])
    assert N == 7
    a["seg_d0"], a["seg_n"], a["seg_zcount"] = a["seg_d0"].copy(), a["seg_n"].copy(), a["seg_zcount"].copy()
    OracleProblem(serialize(a))                                   # 2 * 3 <= 7: fine
    a["dims"] = a["dims"].copy()
    a["dims"][0] = 5                                              # the same rows over fewer variables than 2 M
    with pytest.raises(Exception, match="share entries"):
        OracleProblem(serialize(a))


# ---- 5. host-build solves -------------------------------------------------------------------------------------------------------
def test_host_build_softmax_regression():
    X, Y = lp.softmax_data()
    prob, W = lp.softmax_problem(X, Y)
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    lp.assert_softmax(X, Y, lp.value_in(prob, W, xv), obj)


def test_host_build_box_design_gp():
    prob, y = lp.gp_problem()
    obj, status, iters, xv = oracle_solver(prob)
    assert status == 0
    lp.assert_gp(lp.value_in(prob, y, xv), obj)


def test_host_build_nonconvex_sphere():
    from oracle.oracle_capi import OracleProblem
    A = lp.sphere_data()
    prob, x = lp.sphere_problem(A)
    data = lp.lower(cp.Problem(cp.Minimize(-prob.objective.expr), prob.constraints))
    info = OracleProblem(serialize(data["tape_arrays"])).solve(data["x0"])
    assert info["status"] == 0
    lp.assert_sphere_kkt(A, lp.value_in(prob, x, info["x"]), info["mult_g"][-1])
