// A/B of the forms of the Schur update kernel (csrc/ldlt_blocked.h, gemm_nt_update_fast*; DNLP_LDLT_UPDATE_FORM): one
// `lower` update C -= W L^T of order M and depth K through BlockedLdlt::gemm in the parent form (0) and in another form
// (default 3: pipelined operand reads on the lower-triangle grid) on identical copies of C, the two results compared
// bit for bit (on the device: at M = 90 112 a copy of C is 65 GB), then 5 timed launches of each after 2 warm-ups, the
// forms alternating.  One JSON line.  `update_ab M K form` runs that one form alone (one kernel for a counter pass).
// UPDATE_AB_FORM / UPDATE_AB_BASE choose the two forms of the A/B (default 3 against 0), e.g. each lever on its own;
// UPDATE_AB_BAND the band height of the banded forms (4-7) in tiles.  `update_ab M K form LD [LDW]` (form -1: the A/B)
// gives C and L the leading dimension LD >= M and W the leading dimension LDW (default LD), so that a lone launch runs
// at the column stride of a trailing block inside a larger matrix (n = 1e5: LD 100 008, LDW 100 000), not at M.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -I dnlp_amd/csrc tools/micro/update_ab.hip -o tools/micro/bin/update_ab -lhiprtc
#include "ldlt_blocked.h"
#include <cstdio>
#include <cstdlib>
using namespace dnlp;

#define CK(x)                                                                                   \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } \
  } while (0)

// seeded generator: element e of stream `seed` -> uniform [-1, 1) (splitmix64 of the index)
__device__ inline double ab_value(unsigned long long seed, unsigned long long e) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + e + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<double>(static_cast<long long>(z >> 11)) * (1.0 / 4503599627370496.0) - 1.0;
}

__global__ void ab_fill(double* p, unsigned long long count, unsigned long long seed) {
  for (unsigned long long e = blockIdx.x * static_cast<unsigned long long>(blockDim.x) + threadIdx.x; e < count;
       e += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
    p[e] = ab_value(seed, e);
}

__global__ void ab_diff(const unsigned long long* a, const unsigned long long* b, unsigned long long count,
                        unsigned long long* ndiff) {
  unsigned long long mine = 0;
  for (unsigned long long e = blockIdx.x * static_cast<unsigned long long>(blockDim.x) + threadIdx.x; e < count;
       e += static_cast<unsigned long long>(gridDim.x) * blockDim.x)
    mine += a[e] != b[e];
  if (mine) atomicAdd(ndiff, mine);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: update_ab M K [form [LD [LDW]]]\n"); return 2; }
  const int M = atoi(argv[1]), K = atoi(argv[2]);
  const int single = argc > 3 ? atoi(argv[3]) : -1;
  const int other = std::getenv("UPDATE_AB_FORM") ? atoi(std::getenv("UPDATE_AB_FORM")) : 3;   // the form set against ...
  const int base = std::getenv("UPDATE_AB_BASE") ? atoi(std::getenv("UPDATE_AB_BASE")) : 0;     // ... this one (0: the parent's)
  const int LD = argc > 4 ? atoi(argv[4]) : M, LDW = argc > 5 ? atoi(argv[5]) : LD;
  const int band = std::getenv("UPDATE_AB_BAND") ? atoi(std::getenv("UPDATE_AB_BAND")) : 0;    // 0: BlockedLdlt's default
  if (M <= 0 || M % 8 || K <= 0 || K % GM_BK) { fprintf(stderr, "M: a multiple of 8, K: a multiple of %d\n", GM_BK); return 2; }
  if (LD < M || LD % 8 || LDW < M || LDW % 8) { fprintf(stderr, "LD, LDW: multiples of 8, at least M\n"); return 2; }
  const size_t nC = static_cast<size_t>(LD) * M, nL = static_cast<size_t>(LD) * K, nW = static_cast<size_t>(LDW) * K, slack = 256;
  double *W, *L, *Cs[2] = {nullptr, nullptr};
  unsigned long long* ndiff;
  CK(hipMalloc(&W, (nW + slack) * 8));
  CK(hipMalloc(&L, (nL + slack) * 8));
  CK(hipMalloc(&ndiff, 8));
  const int ncopies = single >= 0 ? 1 : 2;
  for (int c = 0; c < ncopies; ++c) CK(hipMalloc(&Cs[c], (nC + slack) * 8));
  hipLaunchKernelGGL(ab_fill, dim3(4096), dim3(256), 0, 0, W, nW + slack, 11ull);
  hipLaunchKernelGGL(ab_fill, dim3(4096), dim3(256), 0, 0, L, nL + slack, 12ull);
  for (int c = 0; c < ncopies; ++c) hipLaunchKernelGGL(ab_fill, dim3(8192), dim3(256), 0, 0, Cs[c], nC + slack, 13ull);
  CK(hipMemset(ndiff, 0, 8));
  CK(hipDeviceSynchronize());

  BlockedLdlt bl;                 // only what gemm() reads: no workspace, no streams
  bl.ld = LD; bl.ldw = LDW; bl.padded = true; bl.small_tiles_below = 0;
  if (band > 0) bl.update_band = band;
  auto run = [&](int form, double* C) {
    bl.update_form = form;
    bl.gemm(nullptr, C, W, L, LD, M, M, K, 1);
  };
  const double flops = 2.0 * K * (static_cast<double>(M) * (M + 1) / 2);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  if (single >= 0) {
    double ms = 0;
    for (int r = 0; r < 3; ++r) {
      CK(hipEventRecord(e0, 0));
      run(single, Cs[0]);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float t;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r) ms += t / 2;
    }
    printf("{\"tool\": \"update_ab\", \"M\": %d, \"K\": %d, \"LD\": %d, \"LDW\": %d, \"band\": %d, \"form\": %d, \"launches\": 3, "
           "\"ms\": %.4f, \"TF\": %.3f}\n", M, K, LD, LDW, bl.update_band, single, ms, flops / (ms * 1e-3) * 1e-12);
    return 0;
  }
  const int forms[2] = {base, other};
  for (int v = 0; v < 2; ++v) run(forms[v], Cs[v]);
  hipLaunchKernelGGL(ab_diff, dim3(8192), dim3(256), 0, 0, reinterpret_cast<const unsigned long long*>(Cs[0]),
                     reinterpret_cast<const unsigned long long*>(Cs[1]), nC + slack, ndiff);
  unsigned long long nd = 0;
  CK(hipMemcpy(&nd, ndiff, 8, hipMemcpyDeviceToHost));
  double ms[2] = {0, 0}, best[2] = {1e30, 1e30};
  for (int r = 0; r < 7; ++r)
    for (int v = 0; v < 2; ++v) {
      CK(hipEventRecord(e0, 0));
      run(forms[v], Cs[v]);
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float t;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r >= 2) { ms[v] += t / 5; best[v] = t < best[v] ? t : best[v]; }
    }
  // the timed launches went on updating both copies with the same operands: still the same bits
  hipLaunchKernelGGL(ab_diff, dim3(8192), dim3(256), 0, 0, reinterpret_cast<const unsigned long long*>(Cs[0]),
                     reinterpret_cast<const unsigned long long*>(Cs[1]), nC + slack, ndiff);
  unsigned long long nd2 = 0;
  CK(hipMemcpy(&nd2, ndiff, 8, hipMemcpyDeviceToHost));
  printf("{\"tool\": \"update_ab\", \"M\": %d, \"K\": %d, \"LD\": %d, \"LDW\": %d, \"band\": %d, \"forms\": [%d, %d], "
         "\"ms\": [%.4f, %.4f], \"ms_min\": [%.4f, %.4f], "
         "\"TF\": [%.3f, %.3f], \"speedup\": %.4f, \"words_differing_first_launch\": %llu, \"words_differing_after_8\": %llu, "
         "\"bits_equal\": %s}\n",
         M, K, LD, LDW, bl.update_band, base, other, ms[0], ms[1], best[0], best[1], flops / (ms[0] * 1e-3) * 1e-12, flops / (ms[1] * 1e-3) * 1e-12,
         ms[0] / ms[1], nd, nd2, (nd == 0 && nd2 == 0) ? "true" : "false");
  return (nd == 0 && nd2 == 0) ? 0 : 1;
}
