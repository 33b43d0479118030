// The row class of the tape (atom_math.h op_is_row): M rows of K entries per segment, one value per row.  What its
// members share -- the table of members, the per-row counts, the tables the device sweep walks, the packed-index decodes
// and the read of an argument's entry -- for tape.h (Tape::load_rows), model.h (the rules over E::map) and
// exec_hip_rows.h (the hand-written kernels of the host-driven device space).
#pragma once
#include <cmath>

#include "atom_math.h"
#include "exec.h"

namespace dnlp {

// One member of the class.  `tri`: its Hessian is a packed lower triangle per row, row-major, with (+1) or without (-1)
// the diagonal; 0: no triangle but an arrow -- K diagonal entries, the denominator's, K cross entries -- and one more
// first derivative (by the denominator).  `parks`: the generic sweep keeps two numbers per row in an N-vector between
// its maps (model.h), so load_rows refuses 2 M > N.  `two_args`: a second argument with one entry per row.
// `spread_hess`: the Hessian entries of its long rows are written by a launch of their own that walks RowTable::hstart.
// `square`: a segment is ONE row (M = 1) that holds the K = n^2 entries of a matrix of order n = d2 in F order, and the
// whole row is one wavefront's work, so load_rows refuses K > kRowWaveMax.  `bordered` (a square member): behind the n^2
// entries stand the n m entries of an n x m matrix X in F order, K = n (n + m) with m >= 0; the member's work is the
// bordered matrix [[P, X], [X^T, 0]] of order N = K / n, and it is N^2 -- not K -- that one wavefront must hold and that
// decides the kernel form (`work`).
struct RowMember {
  int op;
  const char* name;          // in messages
  int tri;
  bool parks, two_args, spread_hess, square, bordered;
  DNLP_HD constexpr i64 row_tri(i64 K) const { return tri == 0 ? 0 : (tri < 0 ? K * (K - 1) / 2 : K * (K + 1) / 2); }
  DNLP_HD constexpr i64 row_hcount(i64 K) const { return tri == 0 ? 2 * K + 1 : row_tri(K); }
  DNLP_HD constexpr i64 row_dcount(i64 K) const { return two_args ? K + 1 : K; }
  // what a row of K entries (d2 as in the segment) asks of its kernel: the short form takes work <= kRowShortMax with
  // groups of next_pow2(work) lanes, one wavefront takes work <= kRowWaveMax
  DNLP_HD constexpr i64 work(i64 K, i64 d2) const { return bordered && d2 > 0 ? (K / d2) * (K / d2) : K; }
};
constexpr int kRowMembers = 5;
// (the order of the table is the order of the device launches and of TapeView::row_tab)
DNLP_HD constexpr RowMember row_member(int k) {
  constexpr RowMember members[kRowMembers] = {
    {OP_LOG_SUM_EXP, "log_sum_exp", +1, true, false, true, false, false},
    {OP_PROD, "prod", -1, true, false, true, false, false},
    {OP_QUAD_OVER_LIN_ROWS, "quad_over_lin_rows", 0, false, true, false, false, false},
    {OP_LOG_DET, "log_det", +1, false, false, true, true, false},
    {OP_MATRIX_FRAC, "matrix_frac", +1, false, false, true, true, true},
  };
  return members[k];
}
DNLP_HD constexpr int row_member_of(int op) {            // index into the table, -1: not a member
  for (int k = 0; k < kRowMembers; ++k) if (row_member(k).op == op) return k;
  return -1;
}
constexpr bool row_members_match_op_is_row() {
  for (int op = 0; op < 256; ++op) if (op_is_row(op) != (row_member_of(op) >= 0)) return false;
  return true;
}
static_assert(row_members_match_op_is_row(), "atom_math.h op_is_row and the table of row-class members disagree");

// K <= kRowShortMax: a row is a power-of-two group of lanes inside one wavefront.  Above: one wavefront per row up to
// kRowWaveMax entries (32 serial entries per lane), one 256-lane workgroup per row beyond.  The switch points are recorded
// with the measured shapes in profiles/log_sum_exp_sweep.jsonl; other values of kRowWaveMax have not been measured.
constexpr i64 kRowShortMax = 64;
constexpr i64 kRowWaveMax = 2048;
constexpr int kRowForms = 2;             // short (K <= kRowShortMax), long

// The segments of ONE member in ONE kernel form as the device sweep walks them (exec_hip_rows.h): one table row per
// segment, arrays in exec space.  A table has no opcode column: every kernel serves one member.  `start` is the prefix of
// launch work (wavefronts for the short form, workgroups for the long one), `hstart` the prefix of Hessian entries
// (spread_hess members, long form).  `park` (prod, long form): what waits for the Hessian launch -- one double per row
// slot 4 start[s] + row for the row's product, then, from 4 units on, a contiguous copy of every row's entries at
// ustart[s] + row K (`ustart`: the prefix of M K).  `park` (matrix_frac, long form): the swept bordered matrix of every
// segment, N^2 doubles in F order at ustart[s] (`ustart`: the prefix of N^2).  `a1b` / `a1o`: the second argument of a
// two_args member.  `ord` (a `square` member): the order n of the segment's matrix -- a column of its own and not a root
// of K taken in the kernels.
struct RowTable {
  i64 n = 0, units = 0, hunits = 0;
  i64 *start = nullptr, *hstart = nullptr;
  i64 *K = nullptr, *M = nullptr, *a0b = nullptr, *a0o = nullptr, *zoff = nullptr, *doff = nullptr, *hoff = nullptr;
  double* park = nullptr;
  i64* ustart = nullptr;
  i64 *a1b = nullptr, *a1o = nullptr;
  i64* ord = nullptr;
};

// Index into x of entry e of an argument given as (base, offset): contiguous from `base`, or gathered through the tape's
// index list from `off` where base < 0.
DNLP_HD inline i64 arg_at(i64 base, i64 off, const i32* gidx, i64 e) { return base >= 0 ? base + e : gidx[off + e]; }

// q -> (i, j), i >= j: entry q of a packed lower triangle in row-major (tril_indices) order.  `strict`: of the triangle
// without its diagonal -- entry q of the full one, a row further down.
// In double precision: exact for every q an index type holds here (the root is corrected by the two loops).
template <class I>
DNLP_HD inline void tri_decode(I q, bool strict, I& i, I& j) {
  I a = static_cast<I>((sqrt(8.0 * static_cast<double>(q) + 1.0) - 1.0) * 0.5);
  while (a * (a + 1) / 2 > q) --a;
  while ((a + 1) * (a + 2) / 2 <= q) ++a;
  j = q - a * (a + 1) / 2;
  i = strict ? a + 1 : a;
}
// In single precision, for the short rows of the device kernels: q < 2^23.
DNLP_HD inline void tri_decode(int q, int& i, int& j) {
  i = static_cast<int>((sqrtf(8.0f * static_cast<float>(q) + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > q) --i;
  while ((i + 1) * (i + 2) / 2 <= q) ++i;
  j = q - i * (i + 1) / 2;
}

// OP_LOG_DET, the rule of one matrix for the generic spaces (model.h sweep_logdet_segment): Gauss-Jordan WITHOUT pivoting,
// in place on the n x n entries `a` (F order: entry (i, j) at i + j n), then the transposition in place.  On return `a`
// holds the gradient inv(A)^T in the argument's own order and the result is sum_k log(pivot_k), summed in the order
// k = 0 .. n - 1.  No branch on the data: the elimination runs to its end, and a pivot that is not positive (or NaN) makes
// the result and every entry NaN at the end.  A function of its own on the device (the reason is atom_math.h DNLP_OUTLINE's).
// One step of the elimination, shared by the two rules below: pivot `piv` = a[k + k n] of the n x n array `a`.
DNLP_HD inline void sweep_step(double* a, i64 n, i64 k, double piv) {
  a[k + k * n] = 1.0 / piv;
  for (i64 j = 0; j < n; ++j) if (j != k) a[k + j * n] = a[k + j * n] / piv;
  for (i64 i = 0; i < n; ++i) {
    if (i == k) continue;
    const double f = a[i + k * n];
    a[i + k * n] = -f * a[k + k * n];
    for (i64 j = 0; j < n; ++j) if (j != k) a[i + j * n] = a[i + j * n] - f * a[k + j * n];
  }
}
DNLP_OUTLINE DNLP_HD inline double logdet_row(double* a, i64 n) {
  bool ok = true;
  double z = 0.0;
  for (i64 k = 0; k < n; ++k) {
    const double piv = a[k + k * n];
    ok = ok && (piv > 0.0);
    z += log(piv);
    sweep_step(a, n, k, piv);
  }
  const double nan = kInf - kInf;
  for (i64 i = 0; i < n; ++i)
    for (i64 j = 0; j <= i; ++j) {
      const double lo = a[i + j * n], up = a[j + i * n];
      a[i + j * n] = ok ? up : nan;
      a[j + i * n] = ok ? lo : nan;
    }
  return ok ? z : nan;
}

// OP_MATRIX_FRAC, z = tr(X^T P^-1 X) with P of order n and X n x m; the rule of one segment for the generic spaces
// (model.h sweep_mfrac_segment through mfrac_segment below) and, from mfrac_d on, for the device kernels too.  `a` is the bordered matrix
// [[P, X], [X^T, 0]] of order N = n + m (F order: entry (i, j) at i + j N).  The first n steps of the elimination above,
// WITHOUT pivoting, leave
//     B = inv(P)  top left        W = B X  top right        -V^T, V = B^T X,  bottom left        -X^T B X  bottom right
// so z is minus the trace of the bottom right block, summed in the order c = 0 .. m - 1.  No branch on the data: a pivot
// that is not positive (or NaN) makes the result and EVERY entry of `a` NaN at the end, and everything below inherits it.
DNLP_HD inline double mfrac_row(double* a, i64 N, i64 n) {
  bool ok = true;
  for (i64 k = 0; k < n; ++k) {
    const double piv = a[k + k * N];
    ok = ok && (piv > 0.0);
    sweep_step(a, N, k, piv);
  }
  const double nan = kInf - kInf;
  for (i64 l = 0; l < N * N; ++l) a[l] = ok ? a[l] : nan;
  double s = 0.0;
  for (i64 c = n; c < N; ++c) s += a[c + c * N];
  return -s;
}
// Where entry e of the argument row (P in F order, then X in F order) stands in the bordered matrix; the mirror image
// X^T is at (j, i) of an X entry's (i, j).
DNLP_HD inline void mfrac_place(i64 e, i64 n, i64& i, i64& j) {
  if (e < n * n) { i = e % n; j = e / n; }
  else { const i64 q = e - n * n; i = q % n; j = n + q / n; }
}
// With G = V W^T, out of the swept matrix `a`:
//     d[i + j n] = -G_ij = sum_c a[(n + c) + i N] a[j + (n + c) N]        d[n^2 + i + c n] = W_ic + V_ic
// (c = 0 .. m - 1 in this order).
DNLP_HD inline double mfrac_d(const double* a, i64 N, i64 n, i64 e) {
  i64 i, j;
  mfrac_place(e, n, i, j);
  if (j >= n) return a[i + j * N] - a[j + i * N];
  double s = 0.0;
  for (i64 c = n; c < N; ++c) s += a[c + i * N] * a[j + c * N];
  return s;
}
// The row map of the generic spaces: build the bordered matrix in `a` (N^2 doubles) out of x, sweep it, write the K first
// derivatives to `d`; -> z.  Functions of their own on the device, this one and mfrac_h (atom_math.h DNLP_OUTLINE).
DNLP_OUTLINE DNLP_HD inline double mfrac_segment(double* a, double* d, const double* x, const i32* gidx, i64 a0b, i64 a0o, i64 N, i64 n) {
  for (i64 l = 0; l < N * N; ++l) a[l] = 0.0;
  for (i64 e = 0; e < n * N; ++e) {
    i64 i, j;
    mfrac_place(e, n, i, j);
    const double u = x[arg_at(a0b, a0o, gidx, e)];
    a[i + j * N] = u;
    if (j >= n) a[j + i * N] = u;
  }
  const double z = mfrac_row(a, N, n);
  for (i64 e = 0; e < n * N; ++e) d[e] = mfrac_d(a, N, n, e);
  return z;
}
// Entry (p, q), p >= q, of the Hessian over the K = n N argument entries, before its weight, out of the swept matrix and
// the d slots (P entries come first, so a mixed pair has p in X and q in P):
//     P_ij, P_kl     B_li G_kj + B_jk G_il  =  -(B_li d[k + j n] + B_jk d[i + l n])
//     X_kc, P_ij     -(B_ki W_jc + V_ic B_jk)
//     X_ic, X_jd     c == d ? B_ij + B_ji : 0      (NaN where that sum is NaN: an out-of-domain segment has no zero)
DNLP_OUTLINE DNLP_HD inline double mfrac_h(const double* a, const double* d, i64 N, i64 n, i64 p, i64 q) {
  const i64 nn = n * n;
  if (p < nn) {
    const i64 i = p % n, j = p / n, k = q % n, l = q / n;
    return -(a[l + i * N] * d[k + j * n] + a[j + k * N] * d[i + l * n]);
  }
  const i64 pk = (p - nn) % n, c = n + (p - nn) / n;
  if (q < nn) {
    const i64 i = q % n, j = q / n;
    return -(a[pk + i * N] * a[j + c * N] - a[c + i * N] * a[j + pk * N]);
  }
  const i64 qj = (q - nn) % n, dd = n + (q - nn) / n;
  const double s = a[pk + qj * N] + a[qj + pk * N];
  return c == dd ? s : (s == s ? 0.0 : s);
}

}  // namespace dnlp
