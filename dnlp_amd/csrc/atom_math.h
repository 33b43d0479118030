// Per-element value / first / second derivative of the smooth elementwise atoms.
// One rule per reference atom: forward `numeric`, `_jacobian`
// diagonal and `_hess_vec` diagonal of cvxpy/atoms/elementwise/*.py (file:line per case).
// Shared by the HIP tape kernels (tape_kernels.hip) and the host reference backend.
#pragma once
#include "exec.h"

namespace dnlp {

enum Op : int {
  OP_EXP = 1, OP_LOG = 2, OP_ENTR = 3, OP_LOGISTIC = 4, OP_POWER = 5, OP_SIN = 6, OP_COS = 7,
  OP_TAN = 8, OP_SINH = 9, OP_TANH = 10, OP_ASINH = 11, OP_ATANH = 12, OP_XEXP = 13,
  OP_LOG_NORMCDF = 14, OP_NORMCDF = 15, OP_LOGGAMMA = 16,     // no reference rule: exact smooth atoms
  OP_COSH = 17, OP_ATAN = 18, OP_ASIN = 19,                    // no reference rule either: the partners of sinh / tan / sin (acos = pi / 2 - asin)
  OP_MUL = 20, OP_REL_ENTR = 21,
  OP_ATAN2 = 22,           // two arguments like OP_REL_ENTR: argument 0 is y, argument 1 is x
  OP_QUAD_FORM_DENSE = 30, OP_QUAD_FORM_SPARSE = 31, OP_QUAD_OVER_LIN = 32, OP_MATMUL = 33,
  OP_LOG_SUM_EXP = 34,     // row class (model.h sweep_rows): M rows of K entries, one dense K x K Hessian block per row
  OP_PROD = 35,            // row class: the same rows; the block's diagonal is zero and only the strict triangle is stored
  OP_QUAD_OVER_LIN_ROWS = 36,  // row class with a second argument: a denominator per row, an arrow of 2K + 1 Hessian entries
  OP_LOG_DET = 37,         // row class: ONE row holding the n x n entries of a matrix (d2 = n); the full triangle over those n^2 entries
  OP_MATRIX_FRAC = 38      // row class: ONE row holding P (n x n, d2 = n) and then X (n x m); the full triangle over those n (n + m) entries
};

DNLP_HD inline bool op_is_flat(int op) { return op < OP_QUAD_FORM_DENSE; }
// (constexpr: row_class.h checks its table of members against this at compile time)
DNLP_HD constexpr inline bool op_is_row(int op) { return op >= OP_LOG_SUM_EXP && op <= OP_MATRIX_FRAC; }

// integer-exponent fast paths keep x^2 etc. exact and cheap (pow() is ~50 instructions)
DNLP_HD inline double pow_fast(double u, double p) {
  if (p == 2.0) return u * u;
  if (p == 1.0) return u;
  if (p == 0.0) return 1.0;
  if (p == 3.0) return u * u * u;
  if (p == 0.5) return sqrt(u);
  if (p == -0.5) return 1.0 / sqrt(u);
  if (p == -1.0) return 1.0 / u;
  if (p == 1.5) return u * sqrt(u);
  if (p == -1.5) return 1.0 / (u * sqrt(u));
  if (p == 4.0) { double t = u * u; return t * t; }
  return pow(u, p);
}

// ---- special functions of the statistical atoms (log_normcdf, normcdf, loggamma) ---------------------------------------------
// One text for the host build, the tape kernels and the kernels compiled at run time.  Everything is straight-line
// arithmetic on literals: no table is read from memory.
// The three rules are functions of their own on the device: inlined into unary_rules they cost kernels that never meet them
// registers (batch_solve_kernel<64> spilled 32 more VGPRs, the fused kernels three times their scratch); see DESIGN.md section 2.
#if defined(__HIP_DEVICE_COMPILE__)
#define DNLP_OUTLINE __attribute__((noinline))
#else
#define DNLP_OUTLINE
#endif
struct Rule3 { double val, d1, d2; };      // returned by value: in registers (reference arguments of a called function live in scratch)

// E(t) = exp(t^2) erfc(t) for t >= 0, the scaled complementary error function.  q = (t - 4) / (t + 4) maps [0, inf) to
// [-1, 1), where (1 + 2 t) E(t) is a smooth function between 1 and 2 / sqrt(pi): 1 + a polynomial of degree 26 in q (the
// Chebyshev interpolant at 80 points, cut where its coefficients fall below 2^-60, in the monomial basis; sum |a_k| = 0.78, so
// Horner's rounding stays below one unit of the leading 1).  No exp is taken, so nothing overflows; at t -> 0 the result is
// 1 - 1.128 t with the rounding of 1, at t -> inf it is 1 / (t sqrt(pi)).  Worst error against mpmath: 1.6 ulp.
DNLP_HD inline double erfcx_nonneg(double t) {
  if (!(t < 1.152921504606846976e18)) return t != t ? t : 0.56418958354775629 / t;      // 1 + 2 t stays finite below; E = 1 / (t sqrt(pi)) to the last bit here
  const double m = t - 4.0, r = 1.0 / (t + 4.0);
  double q = m * r;
  q = fma(r, fma(q, -t, fma(q + 1.0, -4.0, t)), q);                    // one Newton step: q is (t - 4) / (t + 4) to half an ulp
  double p = 4.1808217396755443e-11;
  p = p * q - 1.3746529890011639e-10;
  p = p * q - 5.3771338210317935e-10;
  p = p * q + 1.7903326159489847e-09;
  p = p * q + 3.9508792541666846e-09;
  p = p * q - 1.4709550868669278e-08;
  p = p * q - 2.1868462576141457e-08;
  p = p * q + 1.1009737295274889e-07;
  p = p * q + 7.888177117406594e-08;
  p = p * q - 8.2491984275083543e-07;
  p = p * q + 2.9094470866632674e-07;
  p = p * q + 5.7092060530721826e-06;
  p = p * q - 1.1220772697788498e-05;
  p = p * q - 2.4398944545280832e-05;
  p = p * q + 0.00015062131406268513;
  p = p * q - 0.00019925677576336479;
  p = p * q - 0.00075777322105128491;
  p = p * q + 0.0050319699926699331;
  p = p * q - 0.016197734065728945;
  p = p * q + 0.037167515535929112;
  p = p * q - 0.066330365811668124;
  p = p * q + 0.093732834998438264;
  p = p * q - 0.10103906603632413;
  p = p * q + 0.068097054254690398;
  p = p * q + 0.015379652102620026;
  p = p * q - 0.1396211168405625;
  p = p * q + 0.2329951186255525;
  return (p + 1.0) / (1.0 + 2.0 * t);
}

// exp(-u^2 / 2) with the rounding of u^2 put back (u^2 = s + lo exactly): full relative accuracy where s / 2 is in the
// hundreds.  Zero from |u| = 40 on (exp(-800) is below the smallest subnormal); NaN stays NaN.
DNLP_HD inline double exp_neg_half_square(double u) {
  const double s = u * u;
  if (!(s < 1600.0)) return s != s ? s : 0.0;
  const double g = exp(-0.5 * s);
  return fma(-0.5 * fma(u, u, -s), g, g);
}

// digamma psi(u) and trigamma psi_1(u) for u > 0: psi(u) = psi(u + 1) - 1 / u and psi_1(u) = psi_1(u + 1) + 1 / u^2 upward until
// the argument reaches 10 (at most ten steps), there the asymptotic series in 1 / x^2 with the Bernoulli numbers up to B_16
// (psi; the first term left out is 3e-18) and B_18 (psi_1; 5e-19 of psi_1(10) = 0.105).
DNLP_HD inline void digamma_trigamma(double u, double& psi, double& psi1) {
  double x = u, s0 = 0.0, s1 = 0.0;
  while (x < 10.0) {
    const double r = 1.0 / x;
    s0 += r; s1 += r * r; x += 1.0;
  }
  const double r = 1.0 / x, w = r * r;
  double a = 3617.0 / 8160.0;                      // B_2k / (2 k), k = 8 .. 1
  a = a * w - 1.0 / 12.0;
  a = a * w + 691.0 / 32760.0;
  a = a * w - 1.0 / 132.0;
  a = a * w + 1.0 / 240.0;
  a = a * w - 1.0 / 252.0;
  a = a * w + 1.0 / 120.0;
  a = a * w - 1.0 / 12.0;
  psi = (log(x) - 0.5 * r + a * w) - s0;
  double b = 43867.0 / 798.0;                      // B_2k, k = 9 .. 1
  b = b * w - 3617.0 / 510.0;
  b = b * w + 7.0 / 6.0;
  b = b * w - 691.0 / 2730.0;
  b = b * w + 5.0 / 66.0;
  b = b * w - 1.0 / 30.0;
  b = b * w + 1.0 / 42.0;
  b = b * w - 1.0 / 30.0;
  b = b * w + 1.0 / 6.0;
  psi1 = (r + 0.5 * w + b * w * r) + s1;
}

// log Phi(u), lambda = phi / Phi, -lambda (u + lambda), through E alone: Phi(u) and 1 - Phi(u) never exist as rounded doubles where
// they cancel or underflow.
DNLP_OUTLINE DNLP_HD inline Rule3 log_normcdf_rules(double u) {
  double val, d1, d2;
  const double kRtHalf = 0.70710678118654752, kRt2OverPi = 0.79788456080286536;
  if (u <= 0.0) {
    const double E = erfcx_nonneg(-u * kRtHalf), lam = kRt2OverPi / E;
    val = log(0.5 * E) - 0.5 * u * u; d1 = lam;
    // lambda = -u - 1 / u + 2 / u^3 - ...: u + lambda is the difference of two numbers u^2 times its size, and beyond -2^26 nothing
    // of it is left.  From -128 on the product's own series in w = 1 / u^2 takes over (the first term left out, 6354 w^5, is
    // below 2^-57 there; the expression itself has lost 14 bits by then)
    if (u > -128.0) d2 = -lam * (u + lam);
    else { const double w = 1.0 / (u * u); d2 = (((-518.0 * w + 50.0) * w - 6.0) * w + 1.0) * w - 1.0; }
  } else {
    const double g = exp_neg_half_square(u), gE = g * erfcx_nonneg(u * kRtHalf), lam = kRt2OverPi * g / (2.0 - gE);
    val = log1p(-0.5 * gE); d1 = lam;
    d2 = (lam == 0.0) ? 0.0 : -lam * (u + lam);      // (u = +inf: 0 (inf + 0) would be NaN)
  }
  return {val, d1, d2};
}

DNLP_OUTLINE DNLP_HD inline Rule3 normcdf_rules(double u) {
  const double kRtHalf = 0.70710678118654752, kInvRt2Pi = 0.3989422804014327;
  const double g = exp_neg_half_square(u), tail = 0.5 * g * erfcx_nonneg(fabs(u) * kRtHalf), phi = kInvRt2Pi * g;
  return {(u <= 0.0) ? tail : 1.0 - tail, phi, (phi == 0.0) ? 0.0 : -u * phi};      // (u = +-inf: inf 0 would be NaN)
}

DNLP_OUTLINE DNLP_HD inline Rule3 loggamma_rules(double u) {
  if (u > 0.0) { Rule3 r; r.val = lgamma(u); digamma_trigamma(u, r.d1, r.d2); return r; }
  if (u == 0.0) return {kInf, -kInf, kInf};
  const double nan = u - u + (kInf - kInf);          // below the domain, and NaN: NaN
  return {nan, nan, nan};
}

// ---- cosh, atan, asin and the four-quadrant atan2 (ops 17 - 19 and 22) ------------------------------------
// Closed-form derivatives without a second transcendental.  Functions of their own on the device for the reason above.
DNLP_OUTLINE DNLP_HD inline Rule3 cosh_rules(double u) {
  const double ch = cosh(u);
  return {ch, sinh(u), ch};
}

// d2 = -2 u / (1 + u^2)^2 as (-2 u d1) d1: (1 + u^2)^2 overflows from |u| = 1e77 on, where the true value is a normal number up
// to 1e102.  |u| >= 1.4e154: 1 + u^2 = inf, d1 = 0 and d2 = -+0 (the true values lie below the subnormal range).
DNLP_OUTLINE DNLP_HD inline Rule3 atan_rules(double u) {
  const double d1 = 1.0 / (1.0 + u * u);
  return {atan(u), d1, (-2.0 * u * d1) * d1};
}

// 1 - u^2 as (1 - u) (1 + u): 1 - u u cancels next to +-1, the two factors are exact there (1 - u) or rounded once (1 + u).
// |u| = 1: s = 0, d1 = +inf, d2 = +-inf; |u| > 1: sqrt of a negative number, NaN throughout, like asin's own value.
DNLP_OUTLINE DNLP_HD inline Rule3 asin_rules(double u) {
  const double s = (1.0 - u) * (1.0 + u), rt = sqrt(s);
  return {asin(u), 1.0 / rt, u / (s * rt)};
}

// atan2(y, x) with r^2 = x^2 + y^2: gy = x / r^2, gx = -y / r^2, hyy = -2 x y / r^4 = 2 gy gx, hxx = -hyy,
// hyx = (y - x) (y + x) / r^4.  Every fourth power is a product of two quotients by r^2, so nothing leaves the double range that
// r^2 itself does not.  The origin: value per IEEE atan2, derivatives 0 / 0 = NaN.  The value jumps by 2 pi across the negative
// x axis; the derivatives are continuous there.
struct Rule2x2 { double val, gy, gx, hyy, hyx; };
DNLP_OUTLINE DNLP_HD inline Rule2x2 atan2_rules(double y, double x) {
  const double r2 = x * x + y * y, gy = x / r2, gx = -y / r2;
  return {atan2(y, x), gy, gx, 2.0 * gy * gx, ((y - x) / r2) * ((y + x) / r2)};
}

// value, d/du, d2/du2 of a unary atom.  p_der is the derivative exponent (reference uses
// p_rational there, power.py:410-419,433-450), p_fwd the forward one (power.py:187-188).
DNLP_HD inline void unary_rules(int op, double u, double p_der, double p_fwd, double& val,
                                double& d1, double& d2) {
  switch (op) {
    case OP_EXP: {                       // exp.py:34-35,112-121,102-107
      double e = exp(u); val = e; d1 = e; d2 = e; break; }
    case OP_LOG: {                       // log.py:33-36,118-127,108-113
      val = log(u); d1 = 1.0 / u; d2 = -1.0 / (u * u); break; }
    case OP_ENTR: {                      // entr.py:35-44,116-120,106-111
      double lg = log(u);
      val = (u > 0.0) ? -u * lg : (u == 0.0 ? 0.0 : -kInf);
      d1 = -lg - 1.0; d2 = -1.0 / u; break; }
    case OP_LOGISTIC: {                  // logistic.py:36-39 (value); the derivatives depart from :108-113,97-103
      // On purpose not the reference's e / (1 + e) and e / (1 + e)^2 with e = exp(u): e is +inf from u = 709.8 on (both
      // quotients NaN; the true values are 1 and ~0) and (1 + e)^2 overflows from u ~ 355 on (d2 = 0 where the true value
      // is a normal number).  Through t = exp(-|u|) <= 1 nothing overflows on either side: sigmoid(u) = 1 / (1 + t) for
      // u >= 0 and t / (1 + t) for u < 0, and sigmoid(u) sigmoid(-u) = t / (1 + t)^2 for both signs.
      double t = exp(-fabs(u)), s = 1.0 / (1.0 + t);
      val = (u > 0.0) ? u + log1p(t) : log1p(t);
      d1 = (u >= 0.0) ? s : t * s; d2 = t * s * s; break; }
    case OP_POWER: {                     // power.py:187-188,433-450,408-422
      val = pow_fast(u, p_fwd);
      d1 = p_der * pow_fast(u, p_der - 1.0);
      d2 = p_der * (p_der - 1.0) * pow_fast(u, p_der - 2.0); break; }
    case OP_SIN: {                       // trig.py:33-36,99-103,90-94
      double sv = sin(u), cv = cos(u); val = sv; d1 = cv; d2 = -sv; break; }
    case OP_COS: {                       // trig.py:113-116,179-183,170-174
      double sv = sin(u), cv = cos(u); val = cv; d1 = -sv; d2 = -cv; break; }
    case OP_TAN: {                       // trig.py:194-197,261-265,251-256
      double t = tan(u), c = cos(u); val = t; d1 = 1.0 / (c * c); d2 = 2.0 * t / (c * c); break; }
    case OP_SINH: {                      // hyperbolic.py:33-36,94-98,85-89
      double sh = sinh(u), ch = cosh(u); val = sh; d1 = ch; d2 = sh; break; }
    case OP_TANH: {                      // hyperbolic.py:108-111,169-173,160-164
      double th = tanh(u), ch = cosh(u); val = th; d1 = 1.0 / (ch * ch);
      d2 = -2.0 * th / (ch * ch); break; }
    case OP_ASINH: {                     // hyperbolic.py:183-186,228-232,219-223
      double q = 1.0 + u * u; val = asinh(u); d1 = 1.0 / sqrt(q); d2 = -u / (q * sqrt(q)); break; }
    case OP_ATANH: {                     // hyperbolic.py:242-245,287-291,278-282
      double q = 1.0 - u * u; val = atanh(u); d1 = 1.0 / q; d2 = 2.0 * u / (q * q); break; }
    case OP_XEXP: {                      // xexp.py:35-36,108-112,117-121
      double e = exp(u); val = u * e; d1 = e * (1.0 + u); d2 = e * (2.0 + u); break; }
    case OP_LOG_NORMCDF: { const Rule3 r = log_normcdf_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    case OP_NORMCDF: { const Rule3 r = normcdf_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    case OP_LOGGAMMA: { const Rule3 r = loggamma_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    case OP_COSH: { const Rule3 r = cosh_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    case OP_ATAN: { const Rule3 r = atan_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    case OP_ASIN: { const Rule3 r = asin_rules(u); val = r.val; d1 = r.d1; d2 = r.d2; break; }
    default: val = d1 = d2 = 0.0;
  }
}

}  // namespace dnlp
