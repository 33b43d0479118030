// Tape sweep over the row-class segments in the host-driven device space: the hand-written forms of the rules that
// model.h states (sweep_lse_segment, sweep_prod_segment, sweep_qol_rows_segment, sweep_logdet_segment,
// sweep_mfrac_segment).  Included by exec_hip.h.
//
// Every launch walks one RowTable (row_class.h: the segments of one member in one kernel form) by its prefix of work, so
// a sweep is at most fourteen launches whatever the number of segments and rows, and a kernel serves one member (a table
// with an opcode column would make it three launches, at the price of one kernel text with the registers of the largest
// member).  The order of every sum and product depends on (K, form) alone: a sweep repeats bit for bit.  No
// floating-point atomics.
//
//   short form (K <= 64)     a row is a group of G = next_pow2(K) lanes, 64 / G consecutive rows per wavefront.  Reductions
//                            go through an xor butterfly inside the group (a + b == b + a: every lane of a group ends with
//                            the same bits), padding lanes carry the operation's identity.  Every lane keeps what it
//                            computed; a member with a packed triangle has the wavefront write the triangles of its rows
//                            -- one contiguous run of the Hessian array -- with its lanes linear over that run.
//   long form (K > 64)       one wavefront per row (four rows per workgroup) up to kRowWaveMax entries, one 256-lane
//                            workgroup per row beyond.  Lane-strided partial results, the wavefront's fixed DPP tree, and
//                            for the workgroup form its four wavefront totals combined in one fixed order through LDS.
//   spread Hessian launch    (members with a packed triangle) the entries of all long rows over the grid: one entry per
//                            lane, consecutive addresses per wavefront, reading what the launch before left in the d slots
//                            (and, for prod, in RowTable::park).
#pragma once

// ---- what the kernels share ----
// the table row whose prefix interval [start[s], start[s + 1]) holds unit u
__device__ __forceinline__ i64 row_find(const i64* __restrict__ start, i64 n, i64 u) {
  i64 lo = 0, hi = n;
  while (hi - lo > 1) {
    const i64 mid = (lo + hi) >> 1;
    if (start[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}
// the same for a launch of one unit per lane: lane 0 searches for the workgroup's first unit u_blk and hands the row on
// through LDS (every lane of the workgroup meets the barrier); a lane then walks on from there to its own unit
__device__ __forceinline__ i64 row_find_block(const i64* __restrict__ start, i64 n, i64 u_blk) {
  __shared__ i64 s_first;
  if (threadIdx.x == 0) s_first = row_find(start, n, u_blk);
  __syncthreads();
  return s_first;
}

// Short form: where this lane stands.  Segment s; its wavefront's first row r0; the lane's row r, its entry l of the row,
// e = r K + l; u = that entry of the argument, `pad` in the lanes that have none (!valid).  false: the whole wavefront has
// no work and leaves (the shuffles of the others see 64 lanes).
struct ShortRow {
  i64 s, M, r0, r, e;
  int K, G, lg, per, lane, l;
  bool valid;
  double u;
};
__device__ __forceinline__ bool short_row(const RowTable& t, const i32* __restrict__ gidx, const double* __restrict__ x, double pad,
                                          ShortRow& w) {
  const int lane = threadIdx.x & 63;
  const i64 wv = static_cast<i64>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  if (wv >= t.units) return false;
  const i64 s = row_find(t.start, t.n, wv);
  const int K = static_cast<int>(t.K[s]);
  const i64 M = t.M[s];
  int G = 1, lg = 0;
  while (G < K) { G <<= 1; ++lg; }
  const int per = 64 >> lg;
  const i64 r0 = (wv - t.start[s]) * per;
  const int l = lane & (G - 1);
  const i64 r = r0 + (lane >> lg);
  const bool valid = r < M && l < K;
  const i64 e = r * K + l;
  const i64 a0b = t.a0b[s];
  double u = pad;
  if (valid) u = x[a0b >= 0 ? a0b + e : gidx[t.a0o[s] + e]];
  w = ShortRow{s, M, r0, r, e, K, G, lg, per, lane, l, valid, u};
  return true;
}

// Short form: the wavefront walks the packed triangles (T entries each, `strict`: without the diagonal) of its rows, one
// contiguous run of the Hessian array.  entry(row, i, j, on) gives h_ij of the wavefront's row `row` before its weight;
// EVERY lane calls it in every trip (uniform trip count), so it may fetch from the lanes that own i and j.
template <class F>
__device__ __forceinline__ void short_row_triangles(const RowTable& t, const ShortRow& w, int T, bool strict, double* __restrict__ hv,
                                                    const double* __restrict__ ww, F entry) {
  const i64 left = w.M - w.r0;
  const int tot = static_cast<int>(left < w.per ? left : w.per) * T;
  double* __restrict__ hrun = hv + t.hoff[w.s] + w.r0 * T;
  const double* __restrict__ wrow = ww + t.zoff[w.s] + w.r0;
  for (int q0 = 0; q0 < tot; q0 += 64) {
    const int q = q0 + w.lane;
    const bool on = q < tot;
    const int qq = on ? q : 0;
    const int row = qq / T;
    int i, j;
    tri_decode(qq - row * T, i, j);
    if (strict) ++i;
    const double h = entry(row, i, j, on);
    if (on) hrun[q] = wrow[row] * h;
  }
}

// Long form: where this lane stands.  Segment s; `row` of it (rowon: it exists -- wavefront-uniform, and the reductions
// need all 64 lanes, so a wavefront without a row walks Kon = 0 entries instead of leaving); the row is walked by W lanes,
// this one is tid of them: for (l = tid; l < Kon; l += W) ... u(l).  wg: the W = 256 lanes of the workgroup.
struct LongRow {
  i64 s, K, M, row, base, Kon, a0b;
  bool wg, rowon;
  int lane, wid, W, tid;
  const i32* __restrict__ gi;
  const double* __restrict__ xr;
  const double* __restrict__ x;
  __device__ __forceinline__ double u(i64 l) const { return a0b >= 0 ? xr[l] : x[gi[l]]; }
};
__device__ __forceinline__ LongRow long_row(const RowTable& t, const i32* __restrict__ gidx, const double* __restrict__ x) {
  static_assert(kBlock == 256, "four wavefronts per workgroup: Tape::load_rows counts four rows per workgroup, and wg_fold reads sm[0..3]");
  const i64 b = blockIdx.x;
  const i64 s = row_find(t.start, t.n, b);
  const i64 K = t.K[s], M = t.M[s];
  const bool wg = K > kRowWaveMax;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const i64 row = wg ? b - t.start[s] : (b - t.start[s]) * (kBlock / 64) + wid;
  const bool rowon = row < M;
  const int W = wg ? kBlock : 64, tid = wg ? static_cast<int>(threadIdx.x) : lane;
  const i64 a0b = t.a0b[s], base = row * K;
  const i32* __restrict__ gi = gidx + t.a0o[s] + base;
  const double* __restrict__ xr = x + (a0b >= 0 ? a0b + base : 0);
  const i64 Kon = rowon ? K : 0;
  return LongRow{s, K, M, row, base, Kon, a0b, wg, rowon, lane, wid, W, tid, gi, xr, x};
}

// Long form, one workgroup per row: the four wavefront totals through sm[0..3], combined as (a0 . a1) . (a2 . a3).
// (wg_post, a barrier, wg_fold; the condition around them is uniform over the workgroup: every wavefront meets the barrier)
template <class T>
__device__ __forceinline__ void wg_post(T* sm, const LongRow& w, T v) { if (w.lane == 0) sm[w.wid] = v; }
template <class T, class F>
__device__ __forceinline__ T wg_fold(const T* sm, F op) { return op(op(sm[0], sm[1]), op(sm[2], sm[3])); }
template <class T, class F>
__device__ __forceinline__ T wg_combine(T* sm, const LongRow& w, T v, F op) {
  wg_post(sm, w, v);
  __syncthreads();
  return wg_fold(sm, op);
}
struct OpAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMul { __device__ __forceinline__ double operator()(double a, double b) const { return a * b; } };
struct OpMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };

// Spread Hessian launch: where this lane's entry stands.  Segment s, entry qa of the segment = entry (i, j) of the packed
// triangle of its row `row`.  false: the lane has no entry.
struct SpreadEntry {
  i64 s;
  unsigned K, row, i, j, qa;
};
__device__ __forceinline__ bool spread_entry(const RowTable& t, bool strict, SpreadEntry& en) {
  const i64 e_blk = static_cast<i64>(blockIdx.x) * kBlock;
  i64 s = row_find_block(t.hstart, t.n, e_blk);
  const i64 e = e_blk + threadIdx.x;
  if (e >= t.hunits) return false;
  while (t.hstart[s + 1] <= e) ++s;
  const unsigned qa = static_cast<unsigned>(e - t.hstart[s]);       // (a segment's entries fit 31 bits: the lowering's limit)
  const unsigned K = static_cast<unsigned>(t.K[s]), T = strict ? K * (K - 1) / 2 : K * (K + 1) / 2;
  const unsigned row = qa / T;
  unsigned i, j;
  tri_decode(qa - row * T, strict, i, j);
  en = SpreadEntry{s, K, row, i, j, qa};
  return true;
}

// The product form of the DPP tree of wave_ops.h (not there: that text also travels into the run-time-compiled kernels).
// Lanes without a source keep the identity, 1.0; lane 63 ends with the wavefront's product, broadcast through an SGPR.
__device__ inline double wave_all_prod(double v) {
  v *= dpp_shift_f64<0x111, 0xf>(v, 1.0);
  v *= dpp_shift_f64<0x112, 0xf>(v, 1.0);
  v *= dpp_shift_f64<0x114, 0xf>(v, 1.0);
  v *= dpp_shift_f64<0x118, 0xf>(v, 1.0);
  v *= dpp_shift_f64<0x142, 0xa>(v, 1.0);
  v *= dpp_shift_f64<0x143, 0xc>(v, 1.0);
  return wave_lane63(v);
}
__device__ inline int wave_all_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}

// ---- log_sum_exp ----
// Short rows: max and sum through the butterfly (padding lanes: exp(-inf - mx) = 0), every lane keeps its p; p_i and p_j
// of a Hessian entry come from the owning lanes.
__global__ void __launch_bounds__(kBlock) sweep_rows_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                            double* __restrict__ z, double* __restrict__ dv,
                                                            double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  ShortRow w;
  if (!short_row(t, gidx, x, -kInf, w)) return;
  double mx = w.u;
  for (int d = 1; d < w.G; d <<= 1) mx = fmax(mx, __shfl_xor(mx, d));
  const double ev = exp(w.u - mx);
  double S = ev;
  for (int d = 1; d < w.G; d <<= 1) S += __shfl_xor(S, d);
  const double p = ev / S;
  if (w.valid) {
    dv[t.doff[w.s] + w.e] = p;
    if (w.l == 0) z[t.zoff[w.s] + w.r] = mx + log(S);
  }
  if (!with_h) return;
  const int lg = w.lg;
  short_row_triangles(t, w, w.K * (w.K + 1) / 2, false, hv, ww, [=](int row, int i, int j, bool) {
    const double pi = __shfl(p, (row << lg) + i), pj = __shfl(p, (row << lg) + j);
    return i == j ? pi - pi * pj : -(pi * pj);
  });
}

// Long rows: e_l = exp(u_l - mx) is parked in the row's d slots by the lane that later scales it to p_l.  The Hessian
// entries are written by sweep_rows_hess_kernel.
__global__ void __launch_bounds__(kBlock) sweep_rows_long_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                                 double* __restrict__ z, double* __restrict__ dv) {
  __shared__ double sm[kBlock / 64];
  const LongRow w = long_row(t, gidx, x);
  double* __restrict__ dr = dv + t.doff[w.s] + w.base;
  double mx = -kInf;
  for (i64 l = w.tid; l < w.Kon; l += w.W) mx = fmax(mx, w.u(l));
  mx = wave_all_max(mx);
  if (w.wg) {
    mx = wg_combine(sm, w, mx, OpMax());
    __syncthreads();                                 // (sm is posted to once more below)
  }
  double S = 0.0;
  for (i64 l = w.tid; l < w.Kon; l += w.W) {
    const double ev = exp(w.u(l) - mx);
    dr[l] = ev;
    S += ev;
  }
  S = wave_all_sum(S);
  if (w.wg) S = wg_combine(sm, w, S, OpAdd());
  for (i64 l = w.tid; l < w.Kon; l += w.W) dr[l] = dr[l] / S;
  if (w.rowon && w.tid == 0) z[t.zoff[w.s] + w.row] = mx + log(S);
}

// p_i (nearly uniform across a wavefront) and p_j (consecutive) from the d slots the launch before filled
__global__ void __launch_bounds__(kBlock) sweep_rows_hess_kernel(RowTable t, const double* __restrict__ dv, double* __restrict__ hv,
                                                                 const double* __restrict__ ww) {
  SpreadEntry en;
  if (!spread_entry(t, false, en)) return;
  const double* __restrict__ pr = dv + t.doff[en.s] + static_cast<i64>(en.row) * en.K;
  const double pi = pr[en.i], pj = pr[en.j];
  hv[t.hoff[en.s] + en.qa] = ww[t.zoff[en.s] + en.row] * (en.i == en.j ? pi - pi * pj : -(pi * pj));
}

// ---- prod ----
// what the rule writes where it says 0: a NaN product stays NaN
__device__ inline double prod_zero(double P0) { return P0 != P0 ? P0 : 0.0; }

// Short rows: padding lanes and zero entries carry 1.0 into the butterfly of the product, the zeros are counted beside
// it.  Every lane keeps its g and u.  g_i and u_j of a Hessian entry come from the owning lanes; the other four values are
// fetched only by a wavefront that meets u_j == 0 (wavefront-uniform branch: the fetches need all 64 lanes).
__global__ void __launch_bounds__(kBlock) sweep_prod_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                            double* __restrict__ z, double* __restrict__ dv,
                                                            double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  ShortRow w;
  if (!short_row(t, gidx, x, 1.0, w)) return;
  const double u = w.u;
  const bool zero = u == 0.0;
  double P0 = zero ? 1.0 : u;
  int nz = zero ? 1 : 0;
  for (int d = 1; d < w.G; d <<= 1) { P0 *= __shfl_xor(P0, d); nz += __shfl_xor(nz, d); }
  const double g = nz == 0 ? P0 / u : ((nz == 1 && zero) ? P0 : prod_zero(P0));
  if (w.valid) {
    dv[t.doff[w.s] + w.e] = g;
    if (w.l == 0) z[t.zoff[w.s] + w.r] = nz == 0 ? P0 : prod_zero(P0);
  }
  if (!with_h || w.K < 2) return;
  const int lg = w.lg;
  short_row_triangles(t, w, w.K * (w.K - 1) / 2, true, hv, ww, [=](int row, int i, int j, bool on) {
    const int li = (row << lg) + i, lj = (row << lg) + j;
    const double gi = __shfl(g, li), uj = __shfl(u, lj);
    double h = gi / (uj == 0.0 ? 1.0 : uj);          // (no division by zero, not even in a value that is replaced below)
    if (__any(on && uj == 0.0)) {
      const double gj = __shfl(g, lj), ui = __shfl(u, li), Pr = __shfl(P0, li);
      const int nr = __shfl(nz, li);
      if (uj == 0.0) h = ui != 0.0 ? gj / ui : (nr == 2 ? Pr : prod_zero(Pr));
    }
    return h;
  });
}

// Long rows: g needs u once more (re-read: nothing is parked in the d slots).  With the Hessian on, two things wait in
// the table's park array for the next launch: what it cannot rebuild from g and u -- the entry of two zero positions,
// nz == 2 ? P0 : Z0, one double per row -- and a contiguous copy of the row (an axis-1 row of an F-ordered argument lies
// strided in x, and the Hessian launch reads u_j with consecutive j in consecutive lanes).
__global__ void __launch_bounds__(kBlock) sweep_prod_long_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                                 double* __restrict__ z, double* __restrict__ dv, int with_h) {
  __shared__ double sm[kBlock / 64];
  __shared__ int sn[kBlock / 64];
  const LongRow w = long_row(t, gidx, x);
  double* __restrict__ dr = dv + t.doff[w.s] + w.base;
  double P0 = 1.0;
  int nz = 0;
  for (i64 l = w.tid; l < w.Kon; l += w.W) {
    const double u = w.u(l);
    if (u == 0.0) ++nz; else P0 *= u;
  }
  P0 = wave_all_prod(P0);
  nz = wave_all_sum_i32(nz);
  if (w.wg) {
    wg_post(sm, w, P0);
    wg_post(sn, w, nz);
    __syncthreads();
    P0 = wg_fold(sm, OpMul());
    nz = wg_fold(sn, OpAdd());
  }
  const double Z0 = prod_zero(P0);
  double* __restrict__ ur = t.park + 4 * t.units + t.ustart[w.s] + w.base;
  for (i64 l = w.tid; l < w.Kon; l += w.W) {
    const double u = w.u(l);
    dr[l] = nz == 0 ? P0 / u : ((nz == 1 && u == 0.0) ? P0 : Z0);
    if (with_h) ur[l] = u;
  }
  if (w.rowon && w.tid == 0) {
    z[t.zoff[w.s] + w.row] = nz == 0 ? P0 : Z0;
    if (with_h) t.park[4 * t.start[w.s] + w.row] = nz == 2 ? P0 : Z0;
  }
}

// g from the d slots and u from the copy the launch before filled
__global__ void __launch_bounds__(kBlock) sweep_prod_hess_kernel(RowTable t, const double* __restrict__ dv, double* __restrict__ hv,
                                                                 const double* __restrict__ ww) {
  SpreadEntry en;
  if (!spread_entry(t, true, en)) return;
  const i64 s = en.s, base = static_cast<i64>(en.row) * en.K;
  const double* __restrict__ gr = dv + t.doff[s] + base;
  const double* __restrict__ ur = t.park + 4 * t.units + t.ustart[s] + base;
  const double uj = ur[en.j];
  double h;
  if (uj != 0.0) h = gr[en.i] / uj;
  else {
    const double ui = ur[en.i];
    h = ui != 0.0 ? gr[en.j] / ui : t.park[4 * t.start[s] + en.row];
  }
  hv[t.hoff[s] + en.qa] = ww[t.zoff[s] + en.row] * h;
}

// ---- quad_over_lin_rows ----
// A row's Hessian is an arrow of 2K + 1 entries, written by the lanes that hold u_l: no third launch, no packed-index decode.
//
// Short rows (K = 2, 3: 32 and 16 rows per wavefront): u^2 through the butterfly, padding lanes carry 0.  Every lane of a
// group reads the group's y and w (one address per group: the hardware merges them) and writes its g_l, h_ll, h_ly at
// r K + l -- across the wavefront consecutive addresses in each of the three blocks; lane 0 of the group writes z, g_y,
// h_yy.  No LDS.
__global__ void __launch_bounds__(kBlock) sweep_qol_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                           double* __restrict__ z, double* __restrict__ dv,
                                                           double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  ShortRow w;
  if (!short_row(t, gidx, x, 0.0, w)) return;
  const i64 s = w.s, r = w.r, e = w.e, M = w.M;
  const double u = w.u;
  double ss = u * u;
  for (int d = 1; d < w.G; d <<= 1) ss += __shfl_xor(ss, d);
  if (!w.valid) return;                              // (no exchange between lanes from here on)
  const i64 a1b = t.a1b[s], MK = M * w.K;
  const double y = x[a1b >= 0 ? a1b + r : gidx[t.a1o[s] + r]];
  double* __restrict__ ds = dv + t.doff[s];
  ds[e] = 2.0 * u / y;
  if (w.l == 0) {
    z[t.zoff[s] + r] = ss / y;
    ds[MK + r] = -ss / (y * y);
  }
  if (!with_h) return;
  const double wr = ww[t.zoff[s] + r];
  double* __restrict__ hs = hv + t.hoff[s];
  hs[e] = 2.0 * wr / y;
  hs[MK + M + e] = -2.0 * wr * u / (y * y);
  if (w.l == 0) hs[MK + r] = 2.0 * wr * ss / (y * y * y);
}

// Long rows: partial sums of u^2, then a second lane-strided pass over the row (u re-read: a row of 8 K bytes that the
// first pass has just brought in) writes g and both Hessian blocks.
__global__ void __launch_bounds__(kBlock) sweep_qol_long_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                                double* __restrict__ z, double* __restrict__ dv,
                                                                double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  __shared__ double sm[kBlock / 64];
  const LongRow w = long_row(t, gidx, x);
  const i64 s = w.s, row = w.row, K = w.K, M = w.M;
  double ss = 0.0;
  for (i64 l = w.tid; l < w.Kon; l += w.W) {
    const double u = w.u(l);
    ss += u * u;
  }
  ss = wave_all_sum(ss);
  if (w.wg) ss = wg_combine(sm, w, ss, OpAdd());
  if (!w.rowon) return;
  const i64 a1b = t.a1b[s], MK = M * K;
  const double y = x[a1b >= 0 ? a1b + row : gidx[t.a1o[s] + row]];
  const double wr = with_h ? ww[t.zoff[s] + row] : 0.0;
  double* __restrict__ dr = dv + t.doff[s] + w.base;
  double* __restrict__ hd = hv + t.hoff[s] + w.base;
  double* __restrict__ hc = hv + t.hoff[s] + MK + M + w.base;
  for (i64 l = w.tid; l < K; l += w.W) {
    const double u = w.u(l);
    dr[l] = 2.0 * u / y;
    if (with_h) {
      hd[l] = 2.0 * wr / y;
      hc[l] = -2.0 * wr * u / (y * y);
    }
  }
  if (w.tid == 0) {
    z[t.zoff[s] + row] = ss / y;
    dv[t.doff[s] + MK + row] = -ss / (y * y);
    if (with_h) hv[t.hoff[s] + MK + row] = 2.0 * wr * ss / (y * y * y);
  }
}

// ---- log_det ----
// A segment is one matrix A of order n (RowTable::ord), its K = n^2 entries in F order: entry l is (i, j) = (l % n, l / n).
// The rule is Gauss-Jordan without pivoting (row_class.h logdet_row states it): n dependent steps, each needing the pivot,
// the pivot row and the pivot column; afterwards the lanes hold B = inv(A) and d[i + j n] = B_ji.  No branch on the data:
// `ok` (every pivot > 0) selects NaN at the stores, and the Hessian entries inherit it from d.
//
// Short form (n <= 8, K <= 64): one entry per lane; pivot, a_kj and a_ik come from the owning lanes by __shfl.  No LDS.
// (M = 1, so a wavefront holds one matrix; the lanes beyond K run the same steps on zeros and store nothing.)
__global__ void __launch_bounds__(kBlock) sweep_logdet_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                              double* __restrict__ z, double* __restrict__ dv,
                                                              double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  ShortRow w;
  if (!short_row(t, gidx, x, 0.0, w)) return;
  const int n = static_cast<int>(t.ord[w.s]), lg = w.lg;
  const int g0 = w.lane & ~(w.G - 1);                  // first lane of this lane's group
  const int l = w.l < w.K ? w.l : 0;                   // (padding lanes follow entry 0: every fetch stays inside the group)
  const int i = l % n, j = l / n;
  double a = w.u, zs = 0.0;
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const double piv = __shfl(a, g0 + k + k * n), rk = __shfl(a, g0 + k + j * n), f = __shfl(a, g0 + i + k * n);
    ok = ok && (piv > 0.0);
    zs += log(piv);
    const double akj = j == k ? 1.0 / piv : rk / piv;  // the new a_kj, a_kk among them
    a = i == k ? akj : (j == k ? -f * akj : a - f * akj);
  }
  const double nan = kInf - kInf;
  const double g = ok ? __shfl(a, g0 + j + i * n) : nan;           // d[i + j n] = B_ji
  if (w.valid) {
    dv[t.doff[w.s] + w.e] = g;
    if (w.l == 0) z[t.zoff[w.s] + w.r] = ok ? zs : nan;
  }
  if (!with_h) return;
  short_row_triangles(t, w, w.K * (w.K + 1) / 2, false, hv, ww, [=](int row, int qa, int qb, bool) {
    const int b0 = row << lg;
    return -(__shfl(g, b0 + qb % n + (qa / n) * n) * __shfl(g, b0 + qa % n + (qb / n) * n));
  });
}

// Long form (9 <= n <= 45, K <= kRowWaveMax = 2048): one wavefront per matrix, the matrix in REGISTERS, 32 entries per lane
// (entry l = lane + 64 q), indexed by the unrolled q only (a run-time index would send the array to scratch).  Where the
// lane's entries stand is taken once: per entry the LDS byte offsets of slot j of a row array and of slot i of a column
// array, which are also what a step compares against (i == k, j == k); an entry beyond K gets slot n of both, which no
// step names and which lies inside the n + 1 slots of each array.  Pivot row and pivot column of step k + 1 are posted to
// the wavefront's own LDS arrays by their owners while step k updates them (two pairs of arrays, by the parity of k);
// lanes 0 .. n - 1 divide the posted row by the pivot into a fifth array, and all lanes read that and the column back.
// The four wavefronts of a workgroup share a segment, hence n: a wavefront without a matrix walks the same steps, so the
// two barriers of a step are met by all.
constexpr int kLogdetMaxN = 45;
static_assert((kLogdetMaxN + 1) * (kLogdetMaxN + 1) > kRowWaveMax && kLogdetMaxN * kLogdetMaxN <= kRowWaveMax, "the largest order whose entries fit one wavefront's 32 per lane");
constexpr int kLogdetPerLane = static_cast<int>(kRowWaveMax / 64);
constexpr int kLogdetSlots = kLogdetMaxN + 1;
__global__ void __launch_bounds__(kBlock) sweep_logdet_long_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                                   double* __restrict__ z, double* __restrict__ dv) {
  // per wavefront: (row, column) as posted for even steps, the same for odd steps, the row divided by its pivot
  __shared__ double sm[(kBlock / 64) * 5 * kLogdetSlots];
  const LongRow w = long_row(t, gidx, x);
  const int n = static_cast<int>(t.ord[w.s]), Kon = static_cast<int>(w.Kon);
  char* const base = reinterpret_cast<char*>(sm + w.wid * 5 * kLogdetSlots);
  constexpr unsigned kCol = kLogdetSlots * 8, kPair = 2 * kLogdetSlots * 8, kNrm = 4 * kLogdetSlots * 8;      // byte offsets
  auto at = [base](unsigned off) -> double& { return *reinterpret_cast<double*>(base + off); };
  double a[kLogdetPerLane];
  unsigned oj[kLogdetPerLane], oi[kLogdetPerLane];
#pragma unroll
  for (int q = 0; q < kLogdetPerLane; ++q) {
    const int l = w.lane + 64 * q;
    const bool on = l < Kon;
    a[q] = on ? w.u(l) : 0.0;
    oj[q] = 8u * static_cast<unsigned>(on ? l / n : n);
    oi[q] = 8u * static_cast<unsigned>(on ? l % n : n);
    if (oi[q] == 0u) at(oj[q]) = a[q];                 // row 0 and column 0 for step 0
    if (oj[q] == 0u) at(kCol + oi[q]) = a[q];
  }
  bool ok = true;
  double zs = 0.0;
  for (int k = 0; k < n; ++k) {
    const unsigned k8 = 8u * static_cast<unsigned>(k), cur = (k & 1) ? kPair : 0u, nxt = kPair - cur;
    __syncthreads();
    const double piv = at(cur + k8);
    ok = ok && (piv > 0.0);
    zs += log(piv);
    if (w.lane < n) at(kNrm + 8u * w.lane) = w.lane == k ? 1.0 / piv : at(cur + 8u * w.lane) / piv;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kLogdetPerLane; ++q) {
      const double akj = at(kNrm + oj[q]), f = at(cur + kCol + oi[q]);
      const double v = oi[q] == k8 ? akj : (oj[q] == k8 ? -f * akj : a[q] - f * akj);
      a[q] = v;
      if (oi[q] == k8 + 8u) at(nxt + oj[q]) = v;
      if (oj[q] == k8 + 8u) at(nxt + kCol + oi[q]) = v;
    }
  }
  const double nan = kInf - kInf;
  double* __restrict__ dr = dv + t.doff[w.s] + w.base;
#pragma unroll
  for (int q = 0; q < kLogdetPerLane; ++q)                            // B_ij is the derivative by entry (j, i)
    if (w.lane + 64 * q < Kon) dr[(oj[q] >> 3) + (oi[q] >> 3) * n] = ok ? a[q] : nan;
  if (w.rowon && w.lane == 0) z[t.zoff[w.s] + w.row] = ok ? zs : nan;
}

// h[(a, b)] = -w d[k + j n] d[i + l n] for a = i + j n >= b = k + l n, out of the d slots the launch before filled
__global__ void __launch_bounds__(kBlock) sweep_logdet_hess_kernel(RowTable t, const double* __restrict__ dv, double* __restrict__ hv,
                                                                   const double* __restrict__ ww) {
  SpreadEntry en;
  if (!spread_entry(t, false, en)) return;
  const unsigned n = static_cast<unsigned>(t.ord[en.s]);
  const double* __restrict__ dr = dv + t.doff[en.s] + static_cast<i64>(en.row) * en.K;
  const double p = dr[en.j % n + (en.i / n) * n], q = dr[en.i % n + (en.j / n) * n];
  hv[t.hoff[en.s] + en.qa] = ww[t.zoff[en.s] + en.row] * -(p * q);
}

// ---- matrix_frac ----
// A segment is P of order n (RowTable::ord) and X of n x m, its K = n (n + m) entries in the order P (F), X (F).  The rule
// (row_class.h mfrac_row states it) is the first n steps of log_det's elimination on the bordered matrix [[P, X], [X^T, 0]]
// of order N = K / n: afterwards it holds B = inv(P), W = B X, -V^T and -X^T B X, and a pivot that was not positive has
// made every entry NaN, which every output inherits.  The kernel form follows N^2 (RowMember::work), not K.
//
// Short form (N <= 8): one entry of the BORDERED matrix per lane, l = i + j N; every lane fetches its own entry of the
// argument (the mirror image X^T from the same x index as X, the zero block 0).  Pivot, row and column by __shfl as for
// log_det; z, the m diagonal entries of the last block, summed in the order c = 0 .. m - 1 in every lane; lane e < K then
// takes d[e] (m products for an entry of P).  No LDS.  One segment per wavefront (M = 1), as for log_det.
__device__ __forceinline__ int mfrac_arg_of(int i, int j, int n) {       // the argument entry behind bordered (i, j); -1: the zero block
  return (i < n && j < n) ? i + j * n : (i < n ? n * n + i + (j - n) * n : (j < n ? n * n + j + (i - n) * n : -1));
}
__global__ void __launch_bounds__(kBlock) sweep_mfrac_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                             double* __restrict__ z, double* __restrict__ dv,
                                                             double* __restrict__ hv, const double* __restrict__ ww, int with_h) {
  const int lane = threadIdx.x & 63;
  const i64 wv = static_cast<i64>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  if (wv >= t.units) return;
  const i64 s = row_find(t.start, t.n, wv);
  const int K = static_cast<int>(t.K[s]), n = static_cast<int>(t.ord[s]), N = K / n, NN = N * N;
  const int lb = lane < NN ? lane : 0;                  // (lanes beyond the matrix follow entry 0 and store nothing)
  const int i = lb % N, j = lb / N;
  const int arg = mfrac_arg_of(i, j, n);
  const i64 a0b = t.a0b[s];
  double a = arg >= 0 ? x[a0b >= 0 ? a0b + arg : gidx[t.a0o[s] + arg]] : 0.0;
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const double piv = __shfl(a, k + k * N), rk = __shfl(a, k + j * N), f = __shfl(a, i + k * N);
    ok = ok && (piv > 0.0);
    const double akj = j == k ? 1.0 / piv : rk / piv;
    a = i == k ? akj : (j == k ? -f * akj : a - f * akj);
  }
  const double nan = kInf - kInf;
  a = ok ? a : nan;
  double zs = 0.0;
  for (int c = n; c < N; ++c) zs += __shfl(a, c + c * N);
  // d of argument entry e = lane (lanes beyond K follow entry 0)
  const int e = lane < K ? lane : 0;
  const bool inP = e < n * n;
  const int ei = inP ? e % n : (e - n * n) % n, ej = inP ? e / n : n + (e - n * n) / n;
  const double wic = __shfl(a, ei + ej * N), vic = __shfl(a, ej + ei * N);
  double gs = 0.0;
  for (int c = n; c < N; ++c) gs += __shfl(a, c + ei * N) * __shfl(a, ej + c * N);
  const double g = inP ? gs : wic - vic;
  if (lane < K) dv[t.doff[s] + lane] = g;
  if (lane == 0) z[t.zoff[s]] = -zs;
  if (!with_h) return;
  ShortRow w{s, 1, 0, 0, lane, K, 64, 6, 1, lane, lane, lane < K, 0.0};
  const int nn = n * n;
  short_row_triangles(t, w, K * (K + 1) / 2, false, hv, ww, [=](int, int p, int q, bool) {
    // (every lane makes every fetch: the three kinds differ in their indices only)
    const bool pP = p < nn, qP = q < nn;
    const int pi = pP ? p % n : (p - nn) % n, pj = pP ? p / n : n + (p - nn) / n;
    const int qi = qP ? q % n : (q - nn) % n, qj = qP ? q / n : n + (q - nn) / n;
    // PP: B_li d[k + j n], B_jk d[i + l n] with (i, j) = p, (k, l) = q.  XP: B_ki W_jc, L_ci B_jk with (k, c) = p, (i, j) = q.
    // XX: B_ij, B_ji with (i, c) = p, (j, d) = q.
    const double u1 = __shfl(a, pP ? qj + pi * N : pi + qi * N);
    const double u2 = __shfl(a, pP ? pj + qi * N : (qP ? qj + pi * N : qi + pi * N));
    const double g1 = __shfl(g, pP ? qi + pj * n : 0), g2 = __shfl(g, pP ? pi + qj * n : 0);
    const double a1 = __shfl(a, !pP && qP ? qj + pj * N : 0), a2 = __shfl(a, !pP && qP ? pj + qi * N : 0);
    const double v1 = pP ? g1 : a1, v2 = pP ? g2 : a2;
    const double sx = u1 + u2;
    return pP ? -(u1 * v1 + u2 * v2) : (qP ? -(u1 * v1 - v2 * u2) : (pj == qj ? sx : (sx == sx ? 0.0 : sx)));
  });
}

// Long form (9 <= N <= 45): log_det's, on the bordered matrix and over n steps.  The wavefront then parks the swept matrix
// (RowTable::park, N^2 doubles from ustart[s]; NaN throughout after a pivot that was not positive), writes z through the
// fixed DPP tree, and -- after a barrier, out of what it has just parked -- the K first derivatives, entry e = lane + 64 q.
__global__ void __launch_bounds__(kBlock) sweep_mfrac_long_kernel(RowTable t, const i32* __restrict__ gidx, const double* __restrict__ x,
                                                                  double* __restrict__ z, double* __restrict__ dv) {
  __shared__ double sm[(kBlock / 64) * 5 * kLogdetSlots];
  const LongRow w = long_row(t, gidx, x);
  const int n = static_cast<int>(t.ord[w.s]), K = static_cast<int>(w.K), N = K / n, NNon = w.rowon ? N * N : 0;
  char* const base = reinterpret_cast<char*>(sm + w.wid * 5 * kLogdetSlots);
  constexpr unsigned kCol = kLogdetSlots * 8, kPair = 2 * kLogdetSlots * 8, kNrm = 4 * kLogdetSlots * 8;      // byte offsets
  auto at = [base](unsigned off) -> double& { return *reinterpret_cast<double*>(base + off); };
  double a[kLogdetPerLane];
  unsigned oj[kLogdetPerLane], oi[kLogdetPerLane];
#pragma unroll
  for (int q = 0; q < kLogdetPerLane; ++q) {
    const int l = w.lane + 64 * q;
    const bool on = l < NNon;
    const int i = on ? l % N : N, j = on ? l / N : N;
    const int arg = on ? mfrac_arg_of(i, j, n) : -1;
    a[q] = arg >= 0 ? w.u(arg) : 0.0;
    oj[q] = 8u * static_cast<unsigned>(j);
    oi[q] = 8u * static_cast<unsigned>(i);
    if (oi[q] == 0u) at(oj[q]) = a[q];                 // row 0 and column 0 for step 0
    if (oj[q] == 0u) at(kCol + oi[q]) = a[q];
  }
  bool ok = true;
  double zs = 0.0;
  for (int k = 0; k < n; ++k) {                        // (log_det's step on order N; lanes 0 .. N - 1 divide the row)
    const unsigned k8 = 8u * static_cast<unsigned>(k), cur = (k & 1) ? kPair : 0u, nxt = kPair - cur;
    __syncthreads();
    const double piv = at(cur + k8);
    ok = ok && (piv > 0.0);
    if (w.lane < N) at(kNrm + 8u * w.lane) = w.lane == k ? 1.0 / piv : at(cur + 8u * w.lane) / piv;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kLogdetPerLane; ++q) {
      const double akj = at(kNrm + oj[q]), f = at(cur + kCol + oi[q]);
      const double v = oi[q] == k8 ? akj : (oj[q] == k8 ? -f * akj : a[q] - f * akj);
      a[q] = v;
      if (oi[q] == k8 + 8u) at(nxt + oj[q]) = v;
      if (oj[q] == k8 + 8u) at(nxt + kCol + oi[q]) = v;
    }
  }
  const double nan = kInf - kInf;
  const unsigned n8 = 8u * static_cast<unsigned>(n);
  double* __restrict__ pk = t.park + t.ustart[w.s];
#pragma unroll
  for (int q = 0; q < kLogdetPerLane; ++q) {
    a[q] = ok ? a[q] : nan;
    if (w.lane + 64 * q < NNon) pk[w.lane + 64 * q] = a[q];
    if (oi[q] == oj[q] && oi[q] >= n8 && w.lane + 64 * q < NNon) zs += a[q];
  }
  zs = wave_all_sum(zs);
  if (w.rowon && w.lane == 0) z[t.zoff[w.s]] = -zs;
  __threadfence_block();
  __syncthreads();
  if (!w.rowon) return;
  double* __restrict__ dr = dv + t.doff[w.s];
  for (int e = w.lane; e < K; e += 64) dr[e] = mfrac_d(pk, N, n, e);
}

// Spread Hessian launch: entry (p, q) of the segment's packed triangle out of the parked matrix and the d slots
// (row_class.h mfrac_h classifies it by comparison with n^2)
__global__ void __launch_bounds__(kBlock) sweep_mfrac_hess_kernel(RowTable t, const double* __restrict__ dv, double* __restrict__ hv,
                                                                  const double* __restrict__ ww) {
  SpreadEntry en;
  if (!spread_entry(t, false, en)) return;
  const i64 n = t.ord[en.s], N = static_cast<i64>(en.K) / n;
  hv[t.hoff[en.s] + en.qa] = ww[t.zoff[en.s]] * mfrac_h(t.park + t.ustart[en.s], dv + t.doff[en.s], N, n, en.i, en.j);
}
