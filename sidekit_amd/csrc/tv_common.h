// What the two total-variability files share (ivector.hip: ranks up to SC_TV_MAX_RANK with the matrix in LDS; ivector_wide.hip: ranks up
// to SC_TVW_MAX_RANK with the matrix in caller-owned scratch): the packed-triangle index and the launch of the ONE Gram kernel.
#pragma once
#include "common.h"

namespace sk {

__host__ __device__ inline long tv_packed(int R) { return (long)R * (R + 1) / 2; }
// i R - i (i + 1) / 2: (i, k), i <= k, is at tv_rb(i) + k.  The 24-bit product i (2 R - i - 1) stays below 2^24 up to R = 2896.
__device__ inline int tv_rb(int i, int R) { return (int)(__umul24(i, 2 * R - i - 1) >> 1); }

// Enqueues tv_gram_kernel (ivector.hip), which has nothing in it that depends on a rank cap: G[c] = F_c' F_c packed, C x R (R + 1) / 2.
// nt = cdiv(R, 64), the tile rows of the output.  The sizes are the caller's to check.  Returns SK_OK or SK_EHIP.
int tv_gram_launch(const double* d_F, int C, int D, int R, int nt, double* d_G, hipStream_t stream);

}  // namespace sk
