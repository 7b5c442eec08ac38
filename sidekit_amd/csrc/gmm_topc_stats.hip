// Top-C Baum-Welch statistics (include/sidekit_amd/gmm_topc_stats.h): the posteriors of a diagonal mixture renormalised over the K
// components per frame that a list names (sc_gmm_top_components, gmm.hip), and the statistics per segment accumulated from them:
//   sc_gmm_topc_posteriors   lp[n][k] = -0.5 (sum_d (X[n][d] - mu[c][d])^2 invcov[c][d] + B[c]), c = idx[n][k];  lse[n] = log sum_k exp lp[n][k];
//                            post[n][k] = exp(lp[n][k] - lse[n])
//   sc_gmm_topc_stats        per segment and component, stat0 / stat1 / stat2 = the sum of post . [1, X, X^2] over the entries that name it,
//                            and the sum of lse
// Against gmm.hip's dense route (12 C D FLOP per frame, 8 C D of them pass B) what remains after the lists is K D of gather work per frame
// for the vector ALU, twice: no N x C array, no matrix cores.  float64, no floating-point atomics (global or LDS), every sum in one
// fixed order.  The segment and its slab and the argument checks are gmm_tile.h's; the two ends of the statistics launcher (the
// workspace and its cut, the slab join by launch_slab_reduce and the segment's llk sum) are gmm.hip's, declared there too; the loop over
// a frame's list and the end of a tile of posteriors are gmm_topc_tile.h's, the same functions gmm_topc_em.hip calls, and their fetch,
// term and sum over the 64 lanes are the ones gmm_topc.hip's scoring kernel calls for four models.
//
// Posteriors.  One workgroup = 256 threads = 4 waves owns a tile of GT = 64 frames; wave w takes frames w, w + 4, ... one at a time;
// lane = d (and d + 64 above 64, added to the lane's term before the join).  The wave holds the frame's list in a register (lane k:
// entry k); per entry the component is wave-uniform, the lane reads invcov[c][d] and mu[c][d] -- a row is one coalesced 8 D-byte load --
// and the rows of entry k + 1 are fetched while entry k is reduced.  lp goes to LDS; then thread f < 64 folds frame f's K values in list
// order with lse_add, and thread (f, k) forms the posterior: the K exponentials are computed once per frame, not once per lane.
// LDS: 64 x K + 64 doubles, 17 KB at K = 32.
//
// Statistics.  grid: x = segment * nslab + slab (gmm_tile.h's cut), y = a block of GT = 64 components.  The block's accumulators,
// 64 rows of [stat0, stat1[0 .. D), stat2[0 .. D)] = 64 x (order D + 1) doubles, live in LDS: 62 KB at D = 60, order 2; 31 KB for order 1.
// Wave w owns components 16 w .. 16 w + 15 of the block: it walks the slab's list entries (frame-major, the order idx and post are stored
// in) 64 at a time, each lane tests one entry (its component within the wave's 16 and below C, its posterior not 0), and a ballot gives
// the hits, taken in ascending entry order = frame order, then list order.  Per hit, component, posterior and frame are wave-uniform and
// lane = d adds post x[d] (and post x[d]^2) to its element of the row, lane 0 post to the row's stat0.  A row is touched by its
// owning wave alone, whose LDS operations complete in program order: no barrier between hits, no atomics.  Every component block scans
// the slab's lists (12 K bytes per frame and block, from L2); the frames are read per hit, K rows of D values per frame over all blocks.
#include "../../include/sidekit_amd/gmm_topc_stats.h"
#include "gmm_topc_tile.h"
#include "kernels.h"

namespace sk {

// Bounds: frames beyond N are neither read nor stored; a frame's list is read for k < K only; what is read through an entry is
// topc_frame_lps's to bound; Lp is indexed with a frame of the tile and k < K.
template <typename T>
__global__ __launch_bounds__(256) void gmm_topc_post_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                            const double* __restrict__ invcov, const double* __restrict__ B, int C,
                                                            const int* __restrict__ idx, int K, double* __restrict__ post,
                                                            double* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  double* Lp = gmm_smem;       // [GT][K]
  double* fl = Lp + GT * K;    // [GT]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long f0 = (long)blockIdx.x * GT;
  const int nvalid = N - f0 < GT ? (int)(N - f0) : GT;
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  for (int f = wave; f < nvalid; f += 4) {
    const long n = f0 + f;
    const double x0 = ok0 ? (double)X[n * D + lane] : 0.0;
    const double x1 = ok1 ? (double)X[n * D + lane + 64] : 0.0;
    const int mine = lane < K ? idx[n * K + lane] : -1;   // K <= 32 < 64
    topc_frame_lps(x0, x1, mine, K, lane, D, mu, invcov, B, C, [&](int k, double lp) {
      if (lane == 0) Lp[f * K + k] = lp;
    });
  }
  topc_fold_and_posteriors(Lp, fl, f0, nvalid, K, post, lse);
}

__host__ __device__ inline int gmm_topc_stats_ld(int D, int order) { return order * D + 1; }

// Bounds: the slab's rows lie within [0, N] (gmm_segment, gmm_slab), so the entries read from idx and post lie within [0, N K) and a
// hit's frame within the slab; a hit's component lies within the wave's 16 of the block and below C, so its row is one of the block's
// 64; lanes beyond D touch nothing; stores are guarded by c < C; slot < nslab S.  A slab has at most 2^25 frames (N < 2^31 over at most
// SC_GMM_MAX_SLABS slabs, rounded up to a tile) of at most 32 entries: an entry's index within the slab fits an int.
template <typename T>
__global__ __launch_bounds__(256) void gmm_topc_stats_kernel(const T* __restrict__ X, long N, int D, int C, const int* __restrict__ idx,
                                                             const double* __restrict__ post, int K, const int* __restrict__ seg_off, int S,
                                                             long max_len, int nslab, int order, double* __restrict__ part0,
                                                             double* __restrict__ part1, double* __restrict__ part2) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int ld = gmm_topc_stats_ld(D, order);
  double* acc = gmm_smem;   // [GT][ld]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int seg = blockIdx.x / nslab, slab = blockIdx.x % nslab, c0 = blockIdx.y * GT;
  const GmmRows rows = gmm_slab(gmm_segment(seg_off, seg, N, max_len), slab);   // empty for a slab beyond the segment's own cut: zeros
  for (int e = tid; e < GT * ld; e += 256) acc[e] = 0.0;
  __syncthreads();
  const int lo = c0 + wave * 16, hi = lo + 16 < C ? lo + 16 : C;   // the wave's components
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  if (rows.begin < rows.end && lo < hi) {
    const int nent = (int)(rows.end - rows.begin) * K;
    const int* ip = idx + rows.begin * K;
    const double* pp = post + rows.begin * K;
    for (int e0 = 0; e0 < nent; e0 += 64) {
      const int e = e0 + lane;
      int c = -1, f = 0;
      double p = 0.0;
      if (e < nent) {
        c = ip[e];
        if (c >= lo && c < hi) { p = pp[e]; f = e / K; }
      }
      unsigned long long hits = __ballot(c >= lo && c < hi && p != 0.0);
      while (hits) {
        const int j = __ffsll(hits) - 1;
        hits &= hits - 1;
        const int r = __builtin_amdgcn_readlane(c, j) - c0;
        const long n = rows.begin + __builtin_amdgcn_readlane(f, j);
        const double pj = __shfl(p, j);
        double* row = acc + r * ld;
        const T* x = X + n * D;
        if (lane == 0) row[0] += pj;
        if (ok0) {
          const double v = (double)x[lane];
          row[1 + lane] += pj * v;
          if (order == 2) row[1 + D + lane] += pj * (v * v);
        }
        if (ok1) {
          const double v = (double)x[lane + 64];
          row[1 + lane + 64] += pj * v;
          if (order == 2) row[1 + D + lane + 64] += pj * (v * v);
        }
      }
    }
  }
  __syncthreads();
  const long slot = (long)slab * S + seg;
  for (int e = tid; e < GT * ld; e += 256) {
    const int r = e / ld, col = e - r * ld, cc = c0 + r;
    if (cc >= C) break;   // r ascends with e
    const long out = slot * C + cc;
    if (col == 0) part0[out] = acc[e];
    else if (col <= D) part1[out * D + col - 1] = acc[e];
    else part2[out * D + col - 1 - D] = acc[e];
  }
}

template <typename T>
static int launch_gmm_topc_post(const T* X, long N, int D, const double* mu, const double* invcov, const double* B, int C, const int* idx, int K,
                                double* post, double* lse, hipStream_t st) {
  const size_t lds = (size_t)(GT * K + GT) * 8;
  hipLaunchKernelGGL(gmm_topc_post_kernel<T>, dim3((unsigned)((N + GT - 1) / GT)), dim3(256), lds, st, X, N, D, mu, invcov, B, C, idx, K, post, lse);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <typename T>
static int launch_gmm_topc_stats(const T* X, long N, int D, int C, const int* idx, const double* post, int K, const double* lse,
                                 const int* seg_off, int S, long max_len, int order, double* stat0, double* stat1, double* stat2, double* llk,
                                 hipStream_t st) {
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);   // held, if gmm_stats_lease takes it, until this function returns
  GmmStatParts p;
  SK_TRY(gmm_stats_lease(st, lock, S, max_len, C, D, order, stat0, stat1, stat2, &p));
  const size_t lds = (size_t)GT * gmm_topc_stats_ld(D, order) * 8;
  SK_TRY(gmm_allow_lds(gmm_topc_stats_kernel<T>, lds));
  const dim3 grid((unsigned)((long)S * p.nslab), (unsigned)((C + GT - 1) / GT));
  hipLaunchKernelGGL(gmm_topc_stats_kernel<T>, grid, dim3(256), lds, st, X, N, D, C, idx, post, K, seg_off, S, max_len, p.nslab, order, p.p0, p.p1,
                     p.p2);
  SK_HIP(hipGetLastError());
  return gmm_stats_finish(p, lse, N, seg_off, S, max_len, llk, st);
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_topc_posteriors(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_B,
                           int32_t C, const int32_t* d_idx, int32_t K, double* d_post, double* d_lse, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_topc_posteriors", d_X, x_dtype, N, D, d_mu, d_invcov, d_B, C));
  SK_CHECK(d_idx && d_post && d_lse, SK_EARG, "sc_gmm_topc_posteriors: null argument");
  SK_TRY(gmm_check_topc("sc_gmm_topc_posteriors", K, C));
  if (x_dtype == XT_F32)
    return launch_gmm_topc_post((const float*)d_X, (long)N, D, d_mu, d_invcov, d_B, C, d_idx, K, d_post, d_lse, (hipStream_t)stream);
  return launch_gmm_topc_post((const double*)d_X, (long)N, D, d_mu, d_invcov, d_B, C, d_idx, K, d_post, d_lse, (hipStream_t)stream);
}

int sc_gmm_topc_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, int32_t C, const int32_t* d_idx, const double* d_post, int32_t K,
                      const double* d_lse, const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order, double* d_stat0, double* d_stat1,
                      double* d_stat2, double* d_llk, void* stream) {
  SK_TRY(gmm_check_frames("sc_gmm_topc_stats", d_X, x_dtype, N, D, C));
  SK_CHECK(order == 1 || order == 2, SK_EARG, "sc_gmm_topc_stats: order must be 1 or 2 (got %d)", order);
  SK_CHECK(d_idx && d_post && d_lse && d_seg_off && d_stat0 && d_stat1 && (order == 1 || d_stat2), SK_EARG, "sc_gmm_topc_stats: null argument");
  SK_TRY(gmm_check_segments("sc_gmm_topc_stats", N, S, max_len));
  SK_TRY(gmm_check_topc("sc_gmm_topc_stats", K, C));
  if (x_dtype == XT_F32)
    return launch_gmm_topc_stats((const float*)d_X, (long)N, D, C, d_idx, d_post, K, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1,
                                 d_stat2, d_llk, (hipStream_t)stream);
  return launch_gmm_topc_stats((const double*)d_X, (long)N, D, C, d_idx, d_post, K, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1,
                               d_stat2, d_llk, (hipStream_t)stream);
}

}  // extern "C"
