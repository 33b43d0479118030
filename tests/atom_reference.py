"""TEST INFRASTRUCTURE — the atom rules restated in mpmath (80 digits), the argument grids and the error bound.

What is here.  Value, first, second and (for the bound only) third derivative of every operation of
dnlp_amd/csrc/atom_math.h in closed form: the thirteen unary atoms, OP_POWER with its two exponents, OP_MUL,
OP_REL_ENTR, and quad_over_lin / matmul as plain sums.  No numerical differentiation.  On top of them a sweep over a
tape (`reference_sweep`) and the seven callbacks' values with a bound per entry (`expected_oracles`), so that a test
compares g, the Jacobian, the Hessian, f and grad f of ANY evaluator entry by entry with the mathematics.

The bound.  For one output r (value, d1 or d2) as a function of the argument u:

    |got - r(u)| <= K * eps * (|r(u)| + |u r'(u)|),        eps = 2^-53

K half-ulps of forward error after allowing the argument itself one rounding.  OP_POWER adds |q ln|u|| |r(u)| inside the
bracket, q the exponent the rule raises to (p, p - 1, p - 2): the rule computes p - 2.0 in floating point and ln u
amplifies that rounding.  A two-argument rule gets the same term for its second argument.  matmul and quad_over_lin are
sums of n rounded terms: theirs is the textbook bound of recursive summation in any order, (n + 2) eps sum |term| (no K).
An entry of g / J / H / grad f that adds several atom outputs through the tape's constant maps gets the sum of its terms'
bounds plus the same summation bound for the map's own additions.

A point is left out of the magnitude comparison only when the mpmath value of that output lies outside the normal double
range (|r| > 1.7e308 or 0 < |r| < 2.3e-308): decided from mpmath alone.  There the result must still not be NaN.  At and
beyond the edges of a domain (log(0), entr(0), log(-1), atanh(+-1), power(0, -1), ...) the IEEE class of
oracle/tape_eval.unary_rules is the expectation (`status` 2).

K is measured, not chosen: `measured_K()` runs oracle/tape_eval.unary_rules (independent text, numpy over glibc's math
library) against mpmath on the grids below and returns, per op and output, 4 x the worst ratio rounded up to a power of
two, never below 8.  The factor 4 is for the device math library (1-2 ulp functions where glibc's are below 1) and FMA
contraction.  Measured with

    python -c "import sys; sys.path[:0] = ['.', 'tests']; import atom_reference as ar; ar.print_table()"

(worst |error| in units of eps * bracket, numpy statement after the logistic fix, power term included):

    op                      value     d1     d2   K            left out (worst output)
    exp                      1.02   1.02   1.02   (8, 8, 8)    0.0 %
    log                      0.93   0.50   0.46   (8, 8, 8)    0.0 %
    entr                     1.19   1.35   0.50   (8, 8, 8)    0.0 %
    logistic                 1.41   1.72   3.48   (8, 8, 16)   0.6 %
    sin                      0.42   0.45   0.42   (8, 8, 8)    0.2 %
    cos                      0.45   0.42   0.45   (8, 8, 8)    0.2 %
    tan                      0.37   1.60   1.09   (8, 8, 8)    0.2 %
    sinh                     0.48   1.48   0.48   (8, 8, 8)    0.0 %
    tanh                     0.85   3.44   2.11   (8, 16, 16)  1.8 %
    asinh                    0.91   1.51   1.31   (8, 8, 8)    0.0 %
    atanh                    0.45   1.23   0.93   (8, 8, 8)    0.0 %
    xexp                     0.83   2.43   2.60   (8, 16, 16)  0.0 %
    power, shortcut exps     0.67   0.78   0.86   (8, 8, 8)    0.0 %
    power -2                 0.23   0.25   0.20   (8, 8, 8)    0.0 %
    power 2.5                0.29   0.56   0.93   (8, 8, 8)    0.0 %
    power 0.3                0.61   0.77   0.49   (8, 8, 8)    0.0 %
    power 0.333333           0.66   0.78   0.58   (8, 8, 8)    0.0 %
    power 0.9                0.35   1.27   0.90   (8, 8, 8)    0.0 %
    power 1.0001             0.50   1.93   0.83   (8, 8, 8)    0.0 %
    power 0.3, der +9e-13    0.61   0.62   0.59   (8, 8, 8)    0.0 %

The two-argument rules use the floor K = 8: the numpy tape evaluator's worst on their grids is 0.32 units (OP_MUL value) and
1.11 units (OP_REL_ENTR first derivatives), 4 x of which stays below 8.

("shortcut exps": 2, 3, 4, 0.5, -0.5, -1, 1.5, -1.5 of pow_fast, and 5, 7; the rows below them take pow().)  So K is 8 except
logistic d2, tanh d1 / d2 and xexp d1 / d2, where it is 16.  `measured_K()` recomputes this in every run and refuses a numpy
statement that is more than 4 units off; the test of the numpy statement asserts that every K is 8 or 16 and that at most
2 % of an op's points are left out.  tanh: its grid as first stated (U(-650, 650) and the planted points) leaves 24 % of d1 / d2
out, because sech(u)^2 underflows from |u| = 354.6 on; those points all stay and 9800 more from U(-354, 354) stand beside them.
"""
import numpy as np
import mpmath as mp          # a dependency of torch's sympy; a missing mpmath is an error, never a skip
import scipy.sparse as sp

from oracle.tape_eval import (OP_ASINH, OP_ATANH, OP_COS, OP_ENTR, OP_EXP, OP_LOG, OP_LOGISTIC, OP_MATMUL, OP_MUL,
                              OP_POWER, OP_QUAD_OVER_LIN, OP_REL_ENTR, OP_SIN, OP_SINH, OP_TAN, OP_TANH, OP_XEXP)
from oracle.tape_eval import unary_rules as numpy_rules

mp.mp.dps = 80
EPS = 2.0 ** -53
NORMAL_MAX = mp.mpf("1.7e308")
NORMAL_MIN = mp.mpf("2.3e-308")
LEFT_OUT_SHARE = 0.02

NAMES = {OP_EXP: "exp", OP_LOG: "log", OP_ENTR: "entr", OP_LOGISTIC: "logistic", OP_POWER: "power", OP_SIN: "sin",
         OP_COS: "cos", OP_TAN: "tan", OP_SINH: "sinh", OP_TANH: "tanh", OP_ASINH: "asinh", OP_ATANH: "atanh",
         OP_XEXP: "xexp", OP_MUL: "mul", OP_REL_ENTR: "rel_entr", OP_QUAD_OVER_LIN: "quad_over_lin", OP_MATMUL: "matmul"}
UNARY_OPS = [OP_EXP, OP_LOG, OP_ENTR, OP_LOGISTIC, OP_SIN, OP_COS, OP_TAN, OP_SINH, OP_TANH, OP_ASINH, OP_ATANH, OP_XEXP]
POWER_EXPONENTS = [2.0, 3.0, 4.0, 5.0, 7.0, 0.5, -0.5, -1.0, 1.5, -1.5, -2.0, 2.5, 0.3, 1.0 / 3, 0.9, 1.0001]
# the reference hands the derivative rules a rational approximation of the exponent: once, derivative exponent != forward one
POWER_SPLIT = (0.3, float(np.nextafter(0.3, 1.0)) + 2.0 ** -40)       # (p_fwd, p_der)

_one = mp.mpf(1)


def _sig(u):
    return _one / (1 + mp.exp(-u))


def _softplus(u):
    return (u if u > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(u)))


# f, f', f'', f''' in closed form, stable at the working precision
_CLOSED = {
    OP_EXP: [mp.exp] * 4,
    OP_LOG: [mp.log, lambda u: 1 / u, lambda u: -1 / u ** 2, lambda u: 2 / u ** 3],
    OP_ENTR: [lambda u: -u * mp.log(u), lambda u: -mp.log(u) - 1, lambda u: -1 / u, lambda u: 1 / u ** 2],
    OP_LOGISTIC: [_softplus, _sig, lambda u: _sig(u) * _sig(-u), lambda u: _sig(u) * _sig(-u) * (_sig(-u) - _sig(u))],
    OP_SIN: [mp.sin, mp.cos, lambda u: -mp.sin(u), lambda u: -mp.cos(u)],
    OP_COS: [mp.cos, lambda u: -mp.sin(u), lambda u: -mp.cos(u), mp.sin],
    OP_TAN: [mp.tan, lambda u: mp.sec(u) ** 2, lambda u: 2 * mp.tan(u) * mp.sec(u) ** 2,
             lambda u: 2 * mp.sec(u) ** 4 + 4 * mp.tan(u) ** 2 * mp.sec(u) ** 2],
    OP_SINH: [mp.sinh, mp.cosh, mp.sinh, mp.cosh],
    OP_TANH: [mp.tanh, lambda u: mp.sech(u) ** 2, lambda u: -2 * mp.tanh(u) * mp.sech(u) ** 2,
              lambda u: -2 * mp.sech(u) ** 4 + 4 * mp.tanh(u) ** 2 * mp.sech(u) ** 2],
    OP_ASINH: [mp.asinh, lambda u: 1 / mp.sqrt(1 + u * u), lambda u: -u / (1 + u * u) ** mp.mpf(1.5),
               lambda u: (2 * u * u - 1) / (1 + u * u) ** mp.mpf(2.5)],
    OP_ATANH: [mp.atanh, lambda u: 1 / (1 - u * u), lambda u: 2 * u / (1 - u * u) ** 2,
               lambda u: (2 + 6 * u * u) / (1 - u * u) ** 3],
    OP_XEXP: [lambda u: u * mp.exp(u), lambda u: (1 + u) * mp.exp(u), lambda u: (2 + u) * mp.exp(u),
              lambda u: (3 + u) * mp.exp(u)],
}


def in_domain(op, u, p=0.0):
    """Inside the open domain where value and both derivatives are finite real numbers."""
    if op in (OP_LOG, OP_ENTR):
        return u > 0
    if op == OP_ATANH:
        return abs(u) < 1
    if op == OP_POWER:
        if float(p).is_integer():
            return p >= 2 or u != 0
        return u > 0
    return True


def unary_mp(op, u, p_der=0.0, p_fwd=0.0):
    """-> ([value, d1, d2], [their derivatives in u], [the exponent each is raised to, or None]) as mpmath numbers."""
    x = mp.mpf(float(u))
    if op == OP_POWER:
        pf, pd = mp.mpf(float(p_fwd)), mp.mpf(float(p_der))
        r = [x ** pf, pd * x ** (pd - 1), pd * (pd - 1) * x ** (pd - 2)]
        rp = [pf * x ** (pf - 1), pd * (pd - 1) * x ** (pd - 2), pd * (pd - 1) * (pd - 2) * x ** (pd - 3)]
        return r, rp, [pf, pd - 1, pd - 2]
    v = [f(x) for f in _CLOSED[op]]
    return v[:3], v[1:], [None] * 3


def _bracket(x, r, rp, q):
    b = abs(r) + abs(x * rp)
    if q is not None and x != 0:
        b += abs(q * mp.log(abs(x))) * abs(r)
    return b


def _split(v):
    """mpmath number -> (hi, lo) doubles with hi + lo = v to ~32 digits; a comparison against hi + lo carries no rounding of
    the reference itself."""
    hi = float(v)
    if not np.isfinite(hi):
        return hi, 0.0
    return hi, float(v - mp.mpf(hi))


def _left_out(r):
    a = abs(r)
    return a > NORMAL_MAX or (a != 0 and a < NORMAL_MIN)


_unary_cache = {}


def unary_reference(op, u, p_der=0.0, p_fwd=0.0):
    """For an array of arguments: hi, lo, bracket (each (3, n): value, d1, d2) and status (3, n):
    0 compare in magnitude, 1 left out (mpmath value outside the normal range), 2 edge of the domain or beyond: hi holds the
    IEEE class to expect (NaN / +-inf / a finite number) from oracle/tape_eval.  Cached per (op, exponents, arguments)."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    key = (int(op), float(p_der), float(p_fwd), u.tobytes())
    hit = _unary_cache.get(key)
    if hit is not None:
        return hit
    n = u.size
    hi, lo, br = np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n))
    st = np.zeros((3, n), dtype=np.int8)
    edge = [i for i in range(n) if not (np.isfinite(u[i]) and in_domain(op, u[i], p_der))]
    if edge:
        cls = numpy_rules(op, u[edge], p_der, p_fwd)
        for k in range(3):
            hi[k, edge] = np.asarray(cls[k], float) * np.ones(len(edge))
            st[k, edge] = 2
    skip = set(edge)
    for i in range(n):
        if i in skip:
            continue
        x = mp.mpf(float(u[i]))
        r, rp, q = unary_mp(op, u[i], p_der, p_fwd)
        for k in range(3):
            if _left_out(r[k]):
                st[k, i] = 1
                hi[k, i] = float(mp.sign(r[k])) * (np.inf if abs(r[k]) > 1 else 0.0)
                continue
            hi[k, i], lo[k, i] = _split(r[k])
            br[k, i] = float(_bracket(x, r[k], rp[k], q[k]))
    out = (hi, lo, br, st)
    _unary_cache[key] = out
    return out


# ---- grids (seeded, fixed) ---------------------------------------------------------------------------------------------------

def _positive(rng):
    return np.concatenate([10.0 ** rng.uniform(-100, 100, 100), 10.0 ** rng.uniform(-8, 8, 300),
                           [1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52]])


def grid(op):
    """In-domain arguments of a unary op (not OP_POWER: `power_grid`)."""
    rng = np.random.default_rng(1000 + int(op))
    pos = _positive(rng)
    sym = np.concatenate([pos, -pos, [0.0]])
    small = sym[np.abs(sym) < 1]
    if op in (OP_LOG, OP_ENTR):
        return pos
    if op in (OP_EXP, OP_XEXP, OP_SINH):
        return np.concatenate([rng.uniform(-650, 650, 400), small])
    if op in (OP_LOGISTIC, OP_TANH):
        v = np.concatenate([rng.uniform(-650, 650, 400), small,
                            [19.1, -19.1, 36.7, -36.7, 37.5, -37.5, 360.0, 710.5, 800.0, -800.0, 1e4, -1e4]])
        if op == OP_TANH:
            # sech(u)^2 = 4 exp(-2|u|) leaves the normal range at |u| = 354.6: of the 400 points of U(-650, 650) above, 45 % have
            # no d1 / d2 to compare (24 % of the grid).  They all stay (the value and the IEEE class are checked there); enough
            # points where every output is a normal number are added for the left-out share to be a statement about the grid
            v = np.concatenate([v, rng.uniform(-354, 354, 9800)])
        return v
    if op in (OP_SIN, OP_COS, OP_TAN):
        k = np.arange(-6, 7) * (np.pi / 2)
        return np.concatenate([rng.uniform(-10, 10, 400), k, np.nextafter(k, np.inf), [1e5, 1e10, 1e22, 0.0]])
    if op == OP_ASINH:
        return sym
    if op == OP_ATANH:
        t = 10.0 ** rng.uniform(-16, 0, 300)
        v = np.concatenate([1 - t, -(1 - t), rng.uniform(-1, 1, 300), [0.0, 1 - 2.0 ** -53, -(1 - 2.0 ** -53)]])
        return v[np.abs(v) < 1]
    raise ValueError(op)


def power_grid(p):
    rng = np.random.default_rng(2000)
    pos = np.concatenate([10.0 ** rng.uniform(-30, 30, 150), 10.0 ** rng.uniform(-3, 3, 300),
                          [1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52]])
    return np.concatenate([pos, -pos]) if (float(p).is_integer() and p > 0) else pos


def rel_entr_grid():
    """(u, v): v from the positive range, u / v spanning 1e-30 .. 1e30, and u = v."""
    rng = np.random.default_rng(2100)
    v = np.concatenate([10.0 ** rng.uniform(-60, 60, 150), 10.0 ** rng.uniform(-8, 8, 250)])
    u = v * 10.0 ** rng.uniform(-30, 30, v.size)
    same = 10.0 ** rng.uniform(-60, 60, 40)
    return np.concatenate([u, same]), np.concatenate([v, same])


def mul_grid():
    rng = np.random.default_rng(2200)
    m = 300
    u = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-100, 100, m)
    v = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-100, 100, m)
    return np.concatenate([u, [0.0, 3.0]]), np.concatenate([v, [2.0, 0.0]])


# domain edges and beyond: only the IEEE class is compared there
EDGE_POINTS = {
    OP_LOG: [0.0, -1.0], OP_ENTR: [0.0, -1.0], OP_ATANH: [1.0, -1.0, 1.5],
    OP_EXP: [800.0, -800.0], OP_XEXP: [800.0], OP_SINH: [800.0, -800.0],
}
POWER_EDGE_POINTS = [(-1.0, 0.0), (0.5, 0.0), (0.5, -1.0), (-2.0, 0.0), (2.5, -3.0)]     # (exponent, base)


# ---- K ---------------------------------------------------------------------------------------------------------------------------

def worst_ratios(rules, op, u, p_der=0.0, p_fwd=0.0):
    """`rules(op, u, p_der, p_fwd)` -> (value, d1, d2) arrays against mpmath: per output the worst |error| in units of
    eps * bracket with its argument, the arguments where the IEEE class is wrong, and the left-out share."""
    hi, lo, br, st = unary_reference(op, u, p_der, p_fwd)
    got = [np.asarray(g, float) * np.ones(u.size) for g in rules(op, u, p_der, p_fwd)]
    worst, where, bad, share = [0.0] * 3, [None] * 3, [[], [], []], [0.0] * 3
    for k in range(3):
        share[k] = float(np.mean(st[k] == 1))
        for i in range(u.size):
            g = got[k][i]
            if st[k, i] == 1:
                if np.isnan(g):
                    bad[k].append(float(u[i]))
                continue
            if not np.isfinite(g):
                bad[k].append(float(u[i]))
                continue
            err = abs((g - hi[k, i]) - lo[k, i])
            ratio = 0.0 if err == 0.0 else (np.inf if br[k, i] == 0.0 else err / (EPS * br[k, i]))
            if ratio > worst[k]:
                worst[k], where[k] = ratio, float(u[i])
    return worst, where, bad, share


def _to_K(ratio):
    k = 8
    while k < 4.0 * ratio:
        k *= 2
    return k


_K = {}


def measured_table():
    """{row name: (op, p_der, p_fwd, worst ratios, arguments, wrong-class arguments, left-out shares)} of the numpy statement."""
    if "table" not in _K:
        rows = {}
        for op in UNARY_OPS:
            rows[NAMES[op]] = (op, 0.0, 0.0) + worst_ratios(numpy_rules, op, grid(op))
        for p in POWER_EXPONENTS:
            rows["power %.6g" % p] = (OP_POWER, p, p) + worst_ratios(numpy_rules, OP_POWER, power_grid(p), p, p)
        pf, pd = POWER_SPLIT
        rows["power %.6g / derivative %.17g" % (pf, pd)] = (OP_POWER, pd, pf) + worst_ratios(numpy_rules, OP_POWER, power_grid(pf), pd, pf)
        _K["table"] = rows
    return _K["table"]


def measured_K():
    """{op: (K value, K d1, K d2)}: 4 x the numpy statement's worst ratio, up to a power of two, at least 8 (OP_POWER: the
    worst over its exponents)."""
    if "K" not in _K:
        out = {}
        for name, (op, pd, pf, worst, where, bad, share) in measured_table().items():
            # a numpy statement that is itself wrong must not widen the bound every other evaluator is held to
            assert max(worst) <= 4.0, "numpy statement of %s: %r units of eps * bracket at u = %r" % (name, worst, where)
            ks = tuple(_to_K(w) for w in worst)
            out[op] = tuple(max(a, b) for a, b in zip(out.get(op, (8, 8, 8)), ks))
        _K["K"] = out
    return _K["K"]


def print_table():
    for name, (op, pd, pf, worst, where, bad, share) in measured_table().items():
        print("%-44s %6.2f %6.2f %6.2f   K %s  left out %.3f %.3f %.3f  wrong class %s" %
              ((name,) + tuple(worst) + (tuple(_to_K(w) for w in worst),) + tuple(share) + ([b[:3] for b in bad],)))


# ---- a tape's sweep in mpmath ------------------------------------------------------------------------------------------------

class Units:
    """hi + lo = the exact output, tol = its bound, status as in unary_reference; `who[i]` = (segment, op, arguments) for messages."""

    def __init__(self, n):
        self.hi, self.lo, self.tol = np.zeros(n), np.zeros(n), np.zeros(n)
        self.st = np.zeros(n, dtype=np.int8)
        self.who = [None] * n

    def put(self, i, v, tol, who, st=0):
        self.who[i] = who
        if st == 2:
            self.hi[i], self.st[i] = v, 2
            return
        if _left_out(v):
            self.st[i] = 1
            self.hi[i] = float(mp.sign(v)) * (np.inf if abs(v) > 1 else 0.0)
            return
        self.hi[i], self.lo[i] = _split(v)
        self.tol[i] = float(tol)


def _arg(a, s, which):
    off, ln = int(a["seg_%s_off" % which][s]), int(a["seg_%s_len" % which][s])
    return None if off < 0 else np.asarray(a["gidx"][off:off + ln], dtype=np.int64)


_sweep_cache = {}


def reference_sweep(a, x, w=None):
    """z, dvals and (with the weights w of the z entries) hvals of the tape `a` at x, in the layout of
    oracle/tape_eval.TapeEvaluator.sweep, every unit from the closed forms above."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (id(a), x.tobytes(), None if w is None else np.ascontiguousarray(w).tobytes(), a["gidx"].tobytes(),
           a["seg_a0_base"].tobytes(), a["seg_param"].tobytes())
    if key in _sweep_cache:
        return _sweep_cache[key]
    K = measured_K()
    Z, nseg, nd, nh = (int(a["dims"][i]) for i in (2, 3, 4, 5))
    z, dv, hv = Units(Z), Units(nd), Units(nh if w is not None else 0)
    M = mp.mpf
    for s in range(nseg):
        op, n = int(a["seg_op"][s]), int(a["seg_n"][s])
        zo, do, ho = int(a["seg_zoff"][s]), int(a["seg_doff"][s]), int(a["seg_hoff"][s])
        i0, i1 = _arg(a, s, "a0"), _arg(a, s, "a1")
        if op < OP_MUL:
            pd, pf = float(a["seg_param"][s]), float(a["seg_param2"][s])
            u = x[i0]
            hi, lo, br, st = unary_reference(op, u, pd, pf)
            kk = K[op]
            for i in range(n):
                who = (s, op, (float(u[i]),))
                for k, (dst, off) in enumerate(((z, zo), (dv, do), (hv, ho))):
                    if k == 2 and w is None:
                        continue
                    scale = 1.0 if k < 2 else float(w[zo + i])
                    j = off + i
                    dst.who[j] = who
                    dst.st[j] = st[k, i]
                    with np.errstate(all="ignore"):
                        dst.hi[j], dst.lo[j] = scale * hi[k, i], scale * lo[k, i]
                    dst.tol[j] = abs(scale) * kk[k] * EPS * br[k, i]
        elif op == OP_MUL:
            for i in range(n):
                uf, vf = float(x[i0[i]]), float(x[i1[i]])
                u, v = M(uf), M(vf)
                who = (s, op, (uf, vf))
                z.put(zo + i, u * v, 8 * EPS * 3 * abs(u * v), who)
                dv.put(do + i, v, 0.0, who)
                dv.put(do + n + i, u, 0.0, who)
                if w is not None:
                    hv.put(ho + i, M(float(w[zo + i])), 0.0, who)
        elif op == OP_REL_ENTR:
            for i in range(n):
                uf, vf = float(x[i0[i]]), float(x[i1[i]])
                who = (s, op, (uf, vf))
                if not (uf > 0 and vf > 0):
                    raise ValueError("rel_entr outside its domain is not part of these references")
                u, v = M(uf), M(vf)
                L = mp.log(u / v)
                k8 = 8 * EPS
                # bracket |r| + |u r_u| + |v r_v| of each output
                z.put(zo + i, u * L, k8 * (abs(u * L) + abs(u * (L + 1)) + abs(u)), who)
                dv.put(do + i, L + 1, k8 * (abs(L + 1) + 2), who)
                dv.put(do + n + i, -u / v, k8 * 3 * abs(u / v), who)
                if w is not None:
                    wi = M(float(w[zo + i]))
                    hv.put(ho + i, wi / u, k8 * 2 * abs(wi / u), who)
                    hv.put(ho + n + i, wi * u / (v * v), k8 * 4 * abs(wi * u / (v * v)), who)
                    hv.put(ho + 2 * n + i, -wi / v, k8 * 2 * abs(wi / v), who)
        elif op == OP_QUAD_OVER_LIN:
            u = [M(float(t)) for t in x[i0]]
            y = M(float(x[i1][0]))
            who = (s, op, (float(x[i0][0]), float(y)))
            ss = sum(t * t for t in u)
            e = (n + 4) * EPS
            z.put(zo, ss / y, e * abs(ss / y), who)
            for i in range(n):
                dv.put(do + i, 2 * u[i] / y, e * abs(2 * u[i] / y), who)
            dv.put(do + n, -ss / (y * y), e * abs(ss / (y * y)), who)
            if w is not None:
                ww = M(float(w[zo]))
                for i in range(n):
                    hv.put(ho + i, 2 * ww / y, e * abs(2 * ww / y), who)
                    hv.put(ho + n + 1 + i, -2 * ww * u[i] / (y * y), e * abs(2 * ww * u[i] / (y * y)), who)
                hv.put(ho + n, 2 * ww * ss / y ** 3, e * abs(2 * ww * ss / y ** 3), who)
        elif op == OP_MATMUL:
            mm, kk, pp = int(a["seg_d0"][s]), int(a["seg_d1"][s]), int(a["seg_d2"][s])
            cnt = mm * pp * kk
            for c in range(pp):
                for r in range(mm):
                    i = r + c * mm
                    us = [float(x[i0[r + l * mm]]) for l in range(kk)]
                    vs = [float(x[i1[l + c * kk]]) for l in range(kk)]
                    who = (s, op, (us[0], vs[0]))
                    terms = [M(p) * M(q) for p, q in zip(us, vs)]
                    z.put(zo + i, sum(terms), (kk + 2) * EPS * sum(abs(t) for t in terms), who)
                    for l in range(kk):
                        dv.put(do + i * kk + l, M(vs[l]), 0.0, who)
                        dv.put(do + cnt + i * kk + l, M(us[l]), 0.0, who)
                        if w is not None:
                            hv.put(ho + i * kk + l, M(float(w[zo + i])), 0.0, who)
        else:
            raise ValueError("opcode %d has no mpmath statement here" % op)
    if len(_sweep_cache) > 8:
        _sweep_cache.clear()
    _sweep_cache[key] = (z, dv, hv)
    return z, dv, hv


def _csr(a, name, shape):
    return sp.csr_matrix((a[name + "_val"], a[name + "_idx"], a[name + "_ptr"]), shape=shape)


class Entries:
    """The expectation for one callback's output vector."""

    def __init__(self, base, Mx, xv, M, units, name):
        """entries = base + Mx xv + M units (Mx: the constant linear part on x itself, may be None)."""
        self.name = name
        self.units = units
        self.M = M.tocsr()
        rows = self.M.shape[0]
        base = np.zeros(rows) if base is None else np.asarray(base, float)
        A = abs(self.M)
        with np.errstate(all="ignore"):
            lin = base if Mx is None else base + Mx @ xv
            lin_abs = np.abs(base) if Mx is None else np.abs(base) + abs(Mx) @ np.abs(xv)
            nterms = np.diff(self.M.indptr) + (0 if Mx is None else np.diff(Mx.tocsr().indptr)) + (base != 0)
            finite_hi = np.where(np.isfinite(units.hi), units.hi, 0.0)
            self.hi = lin + self.M @ units.hi
            self.lo = self.M @ units.lo
            # the map's own additions: recursive summation of nterms rounded products in any order
            mag = lin_abs + A @ np.abs(finite_hi)
            self.tol = A @ units.tol + np.where(nterms > 1, (nterms + 1) * EPS * mag, 0.0)
        # status of an entry: the worst of its terms (2: class only, 1: left out, 0: compare).  A term below the normal range
        # inside an entry of several terms does not take the entry out: it counts as 0 with the smallest normal number as bound
        tiny = (units.st == 1) & (units.hi == 0.0)
        several = nterms > 1
        self.st = np.zeros(rows, dtype=np.int8)
        self.st[(A @ ((units.st == 1) & ~tiny).astype(float)) > 0] = 1
        has_tiny = (A @ tiny.astype(float)) > 0
        self.st[has_tiny & ~several] = 1
        self.tol = self.tol + np.where(has_tiny & several, A @ (tiny * float(NORMAL_MIN)), 0.0)
        self.st[(A @ (units.st == 2).astype(float)) > 0] = 2

    def describe(self, r):
        cols = self.M.indices[self.M.indptr[r]:self.M.indptr[r + 1]][:3]
        parts = []
        for c in cols:
            who = self.units.who[c]
            if who is not None:
                parts.append("segment %d %s%r" % (who[0], NAMES.get(who[1], who[1]), who[2]))
        return "; ".join(parts)

    def check(self, got):
        """Entry by entry; raises AssertionError naming the first few offending entries and their arguments."""
        got = np.asarray(got, float).reshape(-1)
        assert got.shape == self.hi.shape, (self.name, got.shape, self.hi.shape)
        bad = []
        with np.errstate(all="ignore"):
            err = np.abs((got - self.hi) - self.lo)
        for r in range(got.size):
            g, s = got[r], self.st[r]
            if s == 2:
                h = self.hi[r]
                ok = (np.isnan(g) and np.isnan(h)) or (np.isinf(h) and g == h) or (np.isfinite(h) and np.isfinite(g))
            elif s == 1:
                ok = not np.isnan(g)
            else:
                ok = np.isfinite(g) and err[r] <= self.tol[r]
            if not ok:
                bad.append("%s[%d] = %r, expected %r (error %.3g, bound %.3g, status %d) from %s" %
                           (self.name, r, g, self.hi[r], err[r], self.tol[r], s, self.describe(r)))
        assert not bad, "%d of %d entries of %s outside their bound:\n  %s" % (len(bad), got.size, self.name, "\n  ".join(bad[:8]))

    def left_out_share(self):
        return float(np.mean(self.st == 1)) if self.st.size else 0.0


def expected_oracles(a, x, lam=None, sigma=1.0, with_h=True):
    """{'f', 'grad_f', 'g', 'jac', 'hess'} -> Entries for the tape `a` at x (Hessian of sigma f + lam' g)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    N, m, Z, nseg, nd, nh, nnzJ, nnzH = (int(v) for v in a["dims"][:8])
    w = None
    if with_h:
        w = _csr(a, "Mw", (Z, 1 + m)) @ np.concatenate([[sigma], np.zeros(m) if lam is None else np.asarray(lam, float)])
    z, dv, hv = reference_sweep(a, x, w)
    c = np.asarray(a["c"], float)
    G = _csr(a, "G", (m, N + Z)).tocsc()
    out = {
        "f": Entries(np.asarray(a["c0"], float)[:1], sp.csr_matrix(c[None, :N]), x, sp.csr_matrix(c[None, N:]), z, "f"),
        "grad_f": Entries(c[:N], None, x, _csr(a, "Mg", (N, nd)), dv, "grad_f"),
        "g": Entries(a["b"], G[:, :N].tocsr(), x, G[:, N:].tocsr(), z, "g"),
        "jac": Entries(a["Jc"], None, x, _csr(a, "MJ", (nnzJ, nd)), dv, "jac"),
    }
    if with_h:
        out["hess"] = Entries(None, None, x, _csr(a, "MH", (nnzH, nh)), hv, "hess")
    return out
