// Batched Levenshtein distance for the on-device consensus path (gfx950).
//
// SURVEY §5.8 / VERDICT r1 item 9: the consolidator's string-similarity
// matrices should run on-device. Long (>50 char) strings already go through
// the batched embedding + cosine GEMM path (consensus/accel.py); this kernel
// covers the SHORT pairs, which the reference scores with normalized
// Levenshtein (k_llms consensus_utils.py:745-761). Normalized strings are
// lowercase alphanumeric ASCII <= 64 chars, so one thread computes one pair
// with Myers' bit-parallel algorithm (Hyyrö's formulation): the whole DP
// column lives in two 64-bit registers, O(n) steps of pure bit math with the
// pattern-match mask Eq built on the fly (m <= 64 compares per step through
// L1-resident pattern bytes).
//
// Grid-stride over pairs; each pair reads two <=64-byte rows of the packed
// [N, 64] char matrix. 100k pairs ~ a few hundred us.

#include "launch.h"

extern "C" __global__ void levenshtein_kernel(
    int* __restrict__ out_dist,          // [P]
    const unsigned char* __restrict__ chars,  // [N, 64] packed normalized strings
    const int* __restrict__ lens,        // [N]
    const int* __restrict__ pair_i,      // [P]
    const int* __restrict__ pair_j,      // [P]
    long n_pairs) {
  const long p0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long p = p0; p < n_pairs; p += stride) {
    const int ia = pair_i[p];
    const int ib = pair_j[p];
    // pattern = the SHORTER string (fits the bit vector; fewer Eq compares)
    int m = lens[ia], n = lens[ib];
    const unsigned char* pa = chars + (long)ia * 64;
    const unsigned char* pb = chars + (long)ib * 64;
    if (m > n) {
      int t = m; m = n; n = t;
      const unsigned char* tp = pa; pa = pb; pb = tp;
    }
    if (m == 0) { out_dist[p] = n; continue; }

    unsigned long long PV = ~0ULL;
    unsigned long long MV = 0ULL;
    const unsigned long long high = 1ULL << (m - 1);
    int score = m;
    for (int j = 0; j < n; ++j) {
      const unsigned char c = pb[j];
      unsigned long long Eq = 0ULL;
      for (int i = 0; i < m; ++i) {
        Eq |= ((unsigned long long)(pa[i] == c)) << i;
      }
      const unsigned long long Xv = Eq | MV;
      const unsigned long long Xh = (((Eq & PV) + PV) ^ PV) | Eq;
      unsigned long long Ph = MV | ~(Xh | PV);
      unsigned long long Mh = PV & Xh;
      if (Ph & high) ++score;
      else if (Mh & high) --score;
      Ph = (Ph << 1) | 1ULL;
      Mh <<= 1;
      PV = Mh | ~(Xv | Ph);
      MV = Ph & Xv;
    }
    out_dist[p] = score;
  }
}

extern "C" void launch_levenshtein(int* out, const unsigned char* chars, const int* lens,
                                   const int* pi, const int* pj, long n_pairs,
                                   hipStream_t stream) {
  int blocks = (int)((n_pairs + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(levenshtein_kernel, dim3(blocks), dim3(256), 0, stream,
                     out, chars, lens, pi, pj, n_pairs);
}
