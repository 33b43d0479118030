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
// whole row is one wavefront's work, so load_rows refuses K > kRowWaveMax.
struct RowMember {
  int op;
  const char* name;          // in messages
  int tri;
  bool parks, two_args, spread_hess, square;
  DNLP_HD constexpr i64 row_tri(i64 K) const { return tri == 0 ? 0 : (tri < 0 ? K * (K - 1) / 2 : K * (K + 1) / 2); }
  DNLP_HD constexpr i64 row_hcount(i64 K) const { return tri == 0 ? 2 * K + 1 : row_tri(K); }
  DNLP_HD constexpr i64 row_dcount(i64 K) const { return two_args ? K + 1 : K; }
};
constexpr int kRowMembers = 4;
// (the order of the table is the order of the device launches and of TapeView::row_tab)
DNLP_HD constexpr RowMember row_member(int k) {
  constexpr RowMember members[kRowMembers] = {
    {OP_LOG_SUM_EXP, "log_sum_exp", +1, true, false, true, false},
    {OP_PROD, "prod", -1, true, false, true, false},
    {OP_QUAD_OVER_LIN_ROWS, "quad_over_lin_rows", 0, false, true, false, false},
    {OP_LOG_DET, "log_det", +1, false, false, true, true},
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
// ustart[s] + row K (`ustart`: the prefix of M K).  `a1b` / `a1o`: the second argument of a two_args member.  `ord` (a
// `square` member): the order n of the segment's matrix -- a column of its own and not a root of K taken in the kernels.
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
DNLP_OUTLINE DNLP_HD inline double logdet_row(double* a, i64 n) {
  bool ok = true;
  double z = 0.0;
  for (i64 k = 0; k < n; ++k) {
    const double piv = a[k + k * n];
    ok = ok && (piv > 0.0);
    z += log(piv);
    a[k + k * n] = 1.0 / piv;
    for (i64 j = 0; j < n; ++j) if (j != k) a[k + j * n] = a[k + j * n] / piv;
    for (i64 i = 0; i < n; ++i) {
      if (i == k) continue;
      const double f = a[i + k * n];
      a[i + k * n] = -f * a[k + k * n];
      for (i64 j = 0; j < n; ++j) if (j != k) a[i + j * n] = a[i + j * n] - f * a[k + j * n];
    }
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

}  // namespace dnlp
