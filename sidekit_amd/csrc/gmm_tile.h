// What the diagonal-GMM kernels share (gmm.hip: frame log-likelihoods, statistics and top-C lists; gmm_score.hip: GMM-UBM scoring;
// gmm_topc.hip: the same on the lists; gmm_topc_stats.hip: sparse posteriors and statistics; gmm_topc_em.hip: list refinement), one copy
// of each:
// the frame tile and its load; a segment's rows and its cut into slabs (the one place seg_off is read, so a join reads the workspace slots
// its producer's cut says were written); the online log-sum-exp update, the merge of two states and the value of one; the argument
// checks; and the launchers of the kernels that one file defines and another launches too (launch_slab_reduce's pattern, kernels.h).
// What the top-C kernels share among themselves is gmm_topc_tile.h's.
#pragma once
#include <cmath>
#include <mutex>

#include "../../include/sidekit_amd/gmm_topc.h"
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

struct GmmRows {
  long begin, end;   // rows [begin, end) of X
  __device__ long len() const { return end - begin; }
};
// Segment seg's rows.  Bounds: the offsets are clamped to [0, N] and to each other and the length to max_len, so whatever seg_off holds,
// 0 <= begin <= end <= N.
__device__ inline GmmRows gmm_segment(const int* __restrict__ seg_off, int seg, long N, long max_len) {
  long r0 = seg_off[seg], r1 = seg_off[seg + 1];
  r0 = r0 < 0 ? 0 : (r0 > N ? N : r0);
  r1 = r1 < r0 ? r0 : (r1 > N ? N : r1);
  return {r0, r0 + (r1 - r0 < max_len ? r1 - r0 : max_len)};
}
// Slab i's rows of a segment, within the segment's own; empty (begin >= end) for i >= gmm_slabs(seg.len()): a grid is sized for the longest segment.
__device__ inline GmmRows gmm_slab(GmmRows seg, int i) {
  const long sl = gmm_slab_len(seg.len()), b = seg.begin + i * sl;
  return {b, b + sl < seg.end ? b + sl : seg.end};
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

// (M, S) <- the log-sum-exp state with v added: sum = S exp(M).  S exp(M - v) + 1 for a new maximum, S + exp(v - M) otherwise, with one
// exp for both cases (its argument is -|v - M| either way); v = -inf and nan add nothing.
__device__ inline void lse_add(double& M, double& S, double v) {
  if (v > -INFINITY) {
    const bool top = v > M;
    const double e = exp(top ? M - v : v - M);
    S = top ? S * e + 1.0 : S + e;
    M = top ? v : M;
  }
}

// (M, S) <- the log-sum-exp state of both: sum = S exp(M); symmetric in its two states bit for bit
__device__ inline void lse_merge(double& M, double& S, double m2, double s2) {
  const double m = fmax(M, m2);
  S = m == -INFINITY ? 0.0 : S * exp(M - m) + s2 * exp(m2 - m);
  M = m;
}

// log(S exp(M)), the value of a log-sum-exp state; -inf for the empty one
__device__ inline double lse_value(double m, double s) { return m == -INFINITY ? m : m + log(s); }

// More than 64 KB of dynamic LDS has to be allowed per kernel before the launch; below that nothing is to be done.
template <typename K>
static int gmm_allow_lds(K kernel, size_t bytes) {
  if (bytes > 65536) SK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return SK_OK;
}

// The checks every entry point makes before anything is enqueued: the frames and the sizes ...
static int gmm_check_frames(const char* who, const void* d_X, int32_t x_dtype, int64_t N, int32_t D, int32_t C) {
  SK_CHECK(d_X, SK_EARG, "%s: null argument", who);
  SK_CHECK(x_dtype == XT_F32 || x_dtype == XT_F64, SK_EARG, "%s: X must be XT_F32 or XT_F64 (got %d)", who, x_dtype);
  SK_CHECK(N >= 1 && N <= 0x7fffffffLL && D >= 1 && D <= SC_GMM_MAX_D && C >= 1 && C <= SC_GMM_MAX_C, SK_EARG,
           "%s: bad sizes (N=%lld, D=%d with at most %d, C=%d with at most %d)", who, (long long)N, D, SC_GMM_MAX_D, C, SC_GMM_MAX_C);
  return SK_OK;
}
// ... with the mixture's three operands, for those that take a mixture ...
static int gmm_check_common(const char* who, const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov,
                            const double* d_A, int32_t C) {
  SK_CHECK(d_X && d_mu && d_invcov && d_A, SK_EARG, "%s: null argument", who);
  return gmm_check_frames(who, d_X, x_dtype, N, D, C);
}
// ... of the entry points that take segments, that the grid's x = segment * slabs + slab fits ...
static int gmm_check_segments(const char* who, int64_t N, int32_t S, int64_t max_len) {
  SK_CHECK(S >= 1 && max_len >= 0 && max_len <= N && (long long)S * gmm_slabs(max_len) <= 0x7fffffffLL, SK_EARG,
           "%s: bad sizes (S=%d, max_len=%lld, N=%lld)", who, S, (long long)max_len, (long long)N);
  return SK_OK;
}
// ... and of those that take lists, their length.
static int gmm_check_topc(const char* who, int32_t K, int32_t C) {
  SK_CHECK(K >= 1 && K <= C && K <= SC_GMM_TOPC_MAX, SK_EARG, "%s: K=%d outside [1, min(C=%d, %d)]", who, K, C, SC_GMM_TOPC_MAX);
  return SK_OK;
}

// gmm.hip: llk[s] = the sum of lse over segment s
int launch_gmm_seg_llk(const double* lse, long N, const int* seg_off, int S, long max_len, double* llk, hipStream_t st);
// gmm.hip: the two ends of a statistics launcher (the dense one's and gmm_topc_stats.hip's).  The kernel between them stores stat0/1/2's
// n0/n1/n2 elements (n2 = 0 for order 1) of slab i at p0/1/2 + i n: with one slab the outputs themselves, otherwise the stream's workspace,
// leased under `lock` (g_plda_mu, deferred), which the caller keeps until its last launch is enqueued (see plda_workspace_locked).
// gmm_stats_finish joins the slabs in slab order (launch_slab_reduce) and forms llk, if asked for, from lse.
struct GmmStatParts { int nslab; long n0, n1, n2; double *p0, *p1, *p2, *stat0, *stat1, *stat2; };
int gmm_stats_lease(hipStream_t st, std::unique_lock<std::mutex>& lock, int S, long max_len, int C, int D, int order, double* stat0,
                    double* stat1, double* stat2, GmmStatParts* out);
int gmm_stats_finish(const GmmStatParts& p, const double* lse, long N, const int* seg_off, int S, long max_len, double* llk, hipStream_t st);
// gmm_score.hip: llk[m][s] = a scoring kernel's slab partials part[slab][m][s] in ascending slab order, for the trials of the mask
int launch_gmm_score_join(const double* part, long N, const int* seg_off, int S, long max_len, long MS, const unsigned char* mask, double* llk,
                          hipStream_t st);

}  // namespace sk
