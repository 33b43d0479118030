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

}  // namespace dnlp
