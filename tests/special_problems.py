"""TEST INFRASTRUCTURE — four likelihood / chance-constraint problems over log_normcdf, normcdf and loggamma, each with an
answer of its own computed in mpmath (30 digits), independent of the solver and of csrc/:

    probit          40 rows, 3 features, two rows planted at margin -12 at the generating point, where the solve starts (its
                    first sweeps run the left-tail formulas); the answer is a damped Newton iteration in mpmath on the same likelihood
    gamma shape     the Gamma MLE with the scale eliminated; the answer is the root of psi(k) - log k = mean(log x) - log(mean x)
    dirichlet       K = 3, 30 samples; the answer solves psi(alpha_k) - psi(sum alpha) = mean(log p_k)
    chance LP       minimise c'x with normcdf((a'x - b) / sigma) >= 0.9 on the unit box; the answer is the LP with
                    a'x - b >= sigma Phi^-1(0.9), a fractional knapsack solved by sorting
    latent probit   (unconstrained, elementwise: the fused path) sum of -log Phi(s_i x_i) + x_i^2 / 2; x_i = s_i t with t = lambda(t)

Each builder returns (problem, variable, expected point, expected value).  VALUE_TOL and POINT_TOL are what the solves are
held to."""
import functools

import mpmath as mp
import numpy as np

import dnlp_amd as cp

VALUE_TOL = 1e-6
POINT_TOL = 1e-4


def _mp30(fn):
    @functools.wraps(fn)
    def wrapped(*args):
        with mp.workdps(30):
            return fn(*args)
    return functools.lru_cache(maxsize=None)(wrapped)


# ---- probit ------------------------------------------------------------------------------------------------------------------------
PROBIT_ROWS, PROBIT_FEATURES, PROBIT_MARGIN = 40, 3, -12.0
PROBIT_TRUE = np.array([1.0, -0.7, 0.4])


def probit_data(seed=7):
    """(A, labels): labels from sign(A w + noise); rows 0 and 1 are rescaled to |a'w| = 12 and mislabelled."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((PROBIT_ROWS, PROBIT_FEATURES))
    s = np.where(A @ PROBIT_TRUE + rng.standard_normal(PROBIT_ROWS) >= 0, 1.0, -1.0)
    for i in (0, 1):
        A[i] *= -PROBIT_MARGIN / abs(A[i] @ PROBIT_TRUE)
        s[i] = -np.sign(A[i] @ PROBIT_TRUE)
    return A, s


def _logncdf_mp(m):
    return mp.log(mp.ncdf(m)) if m <= 0 else mp.log1p(-mp.ncdf(-m))


@_mp30
def probit_answer(labels_key=None):
    A, s = probit_data()
    if labels_key is not None:
        s = np.array(labels_key)
    Z = mp.matrix((s[:, None] * A).tolist())
    n = PROBIT_FEATURES

    def nll(w):
        return -sum(_logncdf_mp((Z[i, :] * w)[0]) for i in range(Z.rows))

    w = mp.zeros(n, 1)
    f = nll(w)
    for _ in range(100):
        g, H = mp.zeros(n, 1), mp.zeros(n, n)
        for i in range(Z.rows):
            m = (Z[i, :] * w)[0]
            lam = mp.npdf(m) / mp.ncdf(m)
            zi = Z[i, :].T
            g -= lam * zi
            H += lam * (m + lam) * (zi * zi.T)
        step = mp.lu_solve(H, -g)
        if mp.norm(step) < mp.mpf(10) ** -20:                # (quadratic convergence: the next step is below 1e-30)
            break
        t = mp.mpf(1)
        while nll(w + t * step) > f + mp.mpf(10) ** -25 and t > mp.mpf(2) ** -40:
            t /= 2
        w = w + t * step
        f = nll(w)
    else:
        raise AssertionError("the mpmath Newton iteration did not converge")
    return np.array([float(v) for v in w]), float(f)


def probit_problem():
    A, s = probit_data()
    x = cp.Variable(PROBIT_FEATURES)
    x.value = PROBIT_TRUE.copy()                    # the planted rows start at margin -12
    prob = cp.Problem(cp.Minimize(-cp.sum(cp.log_normcdf((s[:, None] * A) @ x))))
    xs, fs = probit_answer()
    return prob, x, xs, fs


def probit_template():
    """The same likelihood with the labels as a Parameter: (problem, [labels], x)."""
    A, s = probit_data()
    lab = cp.Parameter(PROBIT_ROWS, name="labels", value=s)
    x = cp.Variable(PROBIT_FEATURES)
    x.value = PROBIT_TRUE.copy()
    return cp.Problem(cp.Minimize(-cp.sum(cp.log_normcdf(cp.multiply(lab, A @ x))))), [lab], x


def probit_label_rows(count, seed=11):
    """`count` label vectors: the planted ones with up to three of rows 2.. flipped (rows 0 and 1 keep their margin)."""
    rng = np.random.default_rng(seed)
    _, s = probit_data()
    out = np.tile(s, (count, 1))
    for i in range(1, count):
        flip = rng.choice(np.arange(2, PROBIT_ROWS), size=int(rng.integers(1, 4)), replace=False)
        out[i, flip] *= -1.0
    return out


# ---- gamma shape -------------------------------------------------------------------------------------------------------------------
def gamma_data(seed=8):
    return np.random.default_rng(seed).gamma(2.5, 1.7, 50)


@_mp30
def gamma_answer():
    xs = gamma_data()
    s, lm = mp.mpf(float(np.mean(np.log(xs)))), mp.log(mp.mpf(float(np.mean(xs))))
    k = mp.findroot(lambda k: mp.psi(0, k) - mp.log(k) - (s - lm), mp.mpf(2))
    val = mp.loggamma(k) - k * mp.log(k) + k * (1 + lm - s) + s
    return np.array([float(k)]), float(val)


def gamma_problem():
    """-(mean log-likelihood) at scale = mean / k:  ln Gamma(k) - k log k + k (1 + log(mean x) - mean(log x)) + mean(log x)."""
    xs = gamma_data()
    s, lm = float(np.mean(np.log(xs))), float(np.log(np.mean(xs)))
    k = cp.Variable(1)
    k.value = np.ones(1)
    prob = cp.Problem(cp.Minimize(cp.sum(cp.loggamma(k) + cp.entr(k) + (1.0 + lm - s) * k) + s))
    ks, fs = gamma_answer()
    return prob, k, ks, fs


# ---- dirichlet ---------------------------------------------------------------------------------------------------------------------
def dirichlet_data(seed=9):
    p = np.random.default_rng(seed).dirichlet([2.0, 5.0, 1.2], 30)
    return np.mean(np.log(p), axis=0)


@_mp30
def dirichlet_answer():
    lp = [mp.mpf(float(v)) for v in dirichlet_data()]
    a = mp.findroot(lambda a0, a1, a2: [mp.psi(0, a) - mp.psi(0, a0 + a1 + a2) - l for a, l in zip((a0, a1, a2), lp)],
                    (mp.mpf(2), mp.mpf(4), mp.mpf(1)))
    val = sum(mp.loggamma(v) for v in a) - mp.loggamma(sum(a)) - sum((v - 1) * l for v, l in zip(a, lp))
    return np.array([float(v) for v in a]), float(val)


def dirichlet_problem():
    lp = dirichlet_data()
    a = cp.Variable(3)
    a.value = np.ones(3)
    prob = cp.Problem(cp.Minimize(cp.sum(cp.loggamma(a)) - cp.loggamma(cp.sum(a)) - lp @ (a - 1.0)))
    xs, fs = dirichlet_answer()
    return prob, a, xs, fs


# ---- chance-constrained LP ---------------------------------------------------------------------------------------------------------
CHANCE_C = np.array([1.0, 2.0, 3.0])
CHANCE_A = np.array([1.0, 1.0, 1.0])
CHANCE_B, CHANCE_SIGMA, CHANCE_P = 1.0, 0.5, 0.9


@_mp30
def chance_answer():
    need = float(CHANCE_B + CHANCE_SIGMA * mp.sqrt(2) * mp.erfinv(2 * mp.mpf(CHANCE_P) - 1))
    x = np.zeros(3)
    for i in np.argsort(CHANCE_C / CHANCE_A):                # cheapest cover of a'x >= need on the unit box
        x[i] = min(1.0, max(0.0, (need - CHANCE_A @ x) / CHANCE_A[i]))
    assert abs(CHANCE_A @ x - need) <= 1e-15 and 0 < x[1] < 1
    return x, float(CHANCE_C @ x)


def chance_problem():
    x = cp.Variable(3, bounds=[0, 1])
    x.value = np.full(3, 0.5)
    prob = cp.Problem(cp.Minimize(CHANCE_C @ x), [cp.normcdf((CHANCE_A @ x - CHANCE_B) / CHANCE_SIGMA) >= CHANCE_P])
    xs, fs = chance_answer()
    return prob, x, xs, fs


# ---- unconstrained, elementwise: the fused path ------------------------------------------------------------------------------------
LATENT_N = 300


@_mp30
def latent_answer():
    t = mp.findroot(lambda t: t - mp.npdf(t) / mp.ncdf(t), mp.mpf("0.6"))
    return float(t), float(LATENT_N * (-mp.log(mp.ncdf(t)) + t * t / 2))


def latent_problem():
    s = np.where(np.arange(LATENT_N) % 3 == 0, -1.0, 1.0)
    x = cp.Variable(LATENT_N)
    x.value = np.zeros(LATENT_N)
    prob = cp.Problem(cp.Minimize(cp.sum(-cp.log_normcdf(cp.multiply(s, x)) + 0.5 * cp.square(x))))
    t, fs = latent_answer()
    return prob, x, s * t, fs


SOLVES = {"probit": probit_problem, "gamma": gamma_problem, "dirichlet": dirichlet_problem, "chance": chance_problem}
# the enclosing-circle test's remedy: the default tol = 1e-8 stops where the VALUE is good to 1e-6; the point of a flat
# likelihood needs more
SOLVE_OPTS = {"probit": {}, "gamma": {}, "dirichlet": {}, "chance": {}}


def assert_solution(name, prob, var, xs, fs):
    assert prob.status == cp.OPTIMAL, (name, prob.status)
    assert abs(prob.value - fs) <= VALUE_TOL * max(1.0, abs(fs)), (name, prob.value, fs)
    assert np.max(np.abs(np.asarray(var.value).reshape(-1) - xs)) <= POINT_TOL * max(1.0, np.max(np.abs(xs))), (name, var.value, xs)
