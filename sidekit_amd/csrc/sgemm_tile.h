// The f32 MFMA wave tile shared by gemm.hip, score_norm.hip and scoring.hip: the f32 counterpart of dgemm_tile.h, without an operand
// loader (the kernels stage differently; their fetches, LDS stores and barriers are their own).
#pragma once
#include "common.h"

namespace sk {

// v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31]; D: sixteen floats per lane, element q at the row below
// and column l & 31.  A wave owns WT x WT such tiles: WT = 1 in gemm_kernel, 2 everywhere else.

template <int WT>
__device__ __forceinline__ void sgemm_zero(f32x16 (&acc)[WT][WT]) {
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
}

// One k-tile of 32 from LDS ([row][k] images, `ld` floats per row, ld = 36: conflict-free ds_read_b128) into the wave's accumulators;
// arow / brow: the wave's first row in each image, h = lane >> 5.  The accumulators take turns, so consecutive MFMAs are independent;
// each element still sees k in ascending order, one FMA per k, whatever WT and whichever kernel: the same bits.
template <int WT>
__device__ __forceinline__ void sgemm_wave_step(const float* As, const float* Bs, int ld, int arow, int brow, int h, f32x16 (&acc)[WT][WT]) {
#pragma unroll
  for (int kk = 0; kk < 32; kk += 8) {
    float4 a[WT], b[WT];
#pragma unroll
    for (int i = 0; i < WT; ++i) {
      a[i] = *reinterpret_cast<const float4*>(&As[(arow + i * 32) * ld + kk + 4 * h]);
      b[i] = *reinterpret_cast<const float4*>(&Bs[(brow + i * 32) * ld + kk + 4 * h]);
    }
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
  }
}

// tile row of accumulator element q (0..15) in lane half h; the column is lane & 31
__device__ __forceinline__ int sgemm_acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

}  // namespace sk
