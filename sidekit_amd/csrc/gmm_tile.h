// What the diagonal-GMM kernels share (gmm.hip: frame log-likelihoods and statistics; gmm_score.hip: GMM-UBM scoring): the frame tile and
// its load, the cut of a segment into slabs, and the merge of two log-sum-exp states.  One copy of each, so that both files cut a
// segment the same way and see the same bits.
#pragma once
#include <cmath>

#include "../../include/sidekit_amd/mixture.h"
#include "dgemm_tile.h"

namespace sk {

constexpr int GT = 64;              // frames per tile, components per tile

__host__ __device__ inline int gmm_xld(int D) { return D | 1; }

// The cut of a segment of `len` frames: slab i is frames [i * slab, min(len, (i + 1) * slab)) of the segment; gmm_slabs(len) of them are not empty.
__host__ __device__ inline long gmm_slabs(long len) {
  const long n = (len + SC_GMM_SLAB_FRAMES - 1) / SC_GMM_SLAB_FRAMES;
  return n < 1 ? 1 : (n > SC_GMM_MAX_SLABS ? SC_GMM_MAX_SLABS : n);
}
__host__ __device__ inline long gmm_slab_len(long len) {
  const long n = gmm_slabs(len), s = (len + n - 1) / n;
  return s < GT ? GT : (s + GT - 1) / GT * GT;
}

// Frames [f0, f0 + nvalid) of X into Xs (rows beyond nvalid and the padding column: zeros, nothing is read for them).  One wave per row.
template <typename T>
__device__ inline void gmm_load_frames(const T* __restrict__ X, int D, long f0, int nvalid, double* Xs, int xld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < GT; r += 4) {
    const T* src = X + (f0 + r) * D;
    for (int d = lane; d < xld; d += 64) {
      double v = 0.0;
      if (r < nvalid && d < D) v = (double)src[d];
      Xs[r * xld + d] = v;
    }
  }
}

// (M, S) <- the log-sum-exp state of both: sum = S exp(M); symmetric in its two states bit for bit
__device__ inline void lse_merge(double& M, double& S, double m2, double s2) {
  const double m = fmax(M, m2);
  S = m == -INFINITY ? 0.0 : S * exp(M - m) + s2 * exp(m2 - m);
  M = m;
}

// More than 64 KB of dynamic LDS has to be allowed per kernel before the launch; below that nothing is to be done.
template <typename K>
static int gmm_allow_lds(K kernel, size_t bytes) {
  if (bytes > 65536) SK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return SK_OK;
}

}  // namespace sk
