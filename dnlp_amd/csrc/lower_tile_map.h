// Index map of the `lower` Schur-update launches (csrc/ldlt_blocked.h, gemm_nt_update_fast): only the 128 x 128 tiles
// that touch the lower triangle are launched.  With square tiles a tile (tm, tn) has an element on or below the diagonal
// exactly when tm >= tn, so tile column tn holds the ntm - tn tiles tm = tn .. ntm - 1 and the launch enumerates them
// column by column, tm ascending — the order the full ntm x ntn grid visits them in, without its empty workgroups.
// Plain C++ (the host build of tests/test_update_forms.py includes this file alone); integers only.
#pragma once

#if defined(__HIPCC__)
#define DNLP_TILE_MAP_FN __host__ __device__ inline
#else
#define DNLP_TILE_MAP_FN inline
#endif

namespace dnlp {

// tiles in the first tn columns (tn <= ntm)
DNLP_TILE_MAP_FN long long lower_tile_offset(int ntm, int tn) {
  return static_cast<long long>(tn) * ntm - static_cast<long long>(tn) * (tn - 1) / 2;
}

// tiles of an ntm x ntn launch (ntn <= ntm)
DNLP_TILE_MAP_FN long long lower_tile_count(int ntm, int ntn) { return lower_tile_offset(ntm, ntn); }

// idx in [0, lower_tile_count(ntm, ntn)) -> (tm, tn): the last column whose offset is <= idx, by bisection
// (at most 10 steps for ntn <= 1024, on a workgroup-uniform value)
DNLP_TILE_MAP_FN void lower_tile_map(long long idx, int ntm, int ntn, int* tm, int* tn) {
  int lo = 0, hi = ntn - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lower_tile_offset(ntm, mid) <= idx) lo = mid;
    else hi = mid - 1;
  }
  *tn = lo;
  *tm = lo + static_cast<int>(idx - lower_tile_offset(ntm, lo));
}

// The same tiles in bands of `band` tile rows: band b holds the rows [b * band, min(ntm, (b + 1) * band)) and is walked
// column by column (tn ascending while tn < ntn and tn < the band's end), tm ascending from max(tn, b * band).  A band's
// W rows are then read again one tile column later, not one whole panel height later.  band >= ntm is lower_tile_map.
// The tiles above band b are the lower tiles of a (b * band)-row launch, so the band is the last b whose closed-form
// prefix is <= idx (bisection, at most 10 steps); inside the band the columns left of the diagonal block are full
// (one division) and the diagonal block is a triangle of its own (lower_tile_map).
DNLP_TILE_MAP_FN long long lower_tile_band_offset(int ntn, int band, int b) {
  const long long r0 = static_cast<long long>(b) * band;
  return lower_tile_offset(static_cast<int>(r0), static_cast<int>(r0 < ntn ? r0 : ntn));
}

DNLP_TILE_MAP_FN void lower_tile_map_banded(long long idx, int ntm, int ntn, int band, int* tm, int* tn) {
  if (band < 1) band = 1;
  int lo = 0, hi = (ntm - 1) / band;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lower_tile_band_offset(ntn, band, mid) <= idx) lo = mid;
    else hi = mid - 1;
  }
  const int r0 = lo * band;                                   // (lo <= (ntm - 1) / band: no overflow)
  const int r1 = ntm - r0 < band ? ntm : r0 + band;
  const int h = r1 - r0;
  const int nc = ntn < r1 ? ntn : r1;                         // columns of this band
  const int full = nc < r0 ? nc : r0;                         // ... of which these hold all h rows
  long long rem = idx - lower_tile_band_offset(ntn, band, lo);
  if (rem < static_cast<long long>(full) * h) {
    const int q = static_cast<int>(rem / h);
    *tn = q;
    *tm = r0 + static_cast<int>(rem - static_cast<long long>(q) * h);
    return;
  }
  rem -= static_cast<long long>(full) * h;
  int dm, dn;
  lower_tile_map(rem, h, nc - r0, &dm, &dn);
  *tm = r0 + dm;
  *tn = r0 + dn;
}

}  // namespace dnlp
