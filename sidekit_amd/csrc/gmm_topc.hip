// Top-C GMM-UBM scoring (include/sidekit_amd/gmm_topc.h): the log-likelihood of every test segment under M mean-adapted models of one
// diagonal mixture on the K components per frame that a list names (sc_gmm_top_components, gmm.hip),
// llk[m][s] = sum_n log sum_k exp lp_m[n][idx[n][k]],  lp_m[n][c] = -0.5 (sum_d (X[n][d] - mus[m][c][d])^2 invcov[c][d] + B[c]).
// K D multiply-adds per frame and model instead of gmm_score.hip's 2 C D: this is gather work for the vector ALU, not for the matrix cores,
// so lp_m takes the direct form -- no A_m, no cancellation between the squares and the linear half.  float64, no floating-point atomics.
// The frame load, the segment and its slab, the log-sum-exp update and the argument checks are gmm_tile.h's, the same functions gmm.hip and
// gmm_score.hip call, and so is the join of the slabs (launch_gmm_score_join, gmm_score.hip's kernel); a list entry's operand, its fetch,
// the lane's terms and the sum over the wave are gmm_topc_tile.h's, the same functions the posteriors and the refinement call at G = 1.
//
// One workgroup = 256 threads = 4 waves owns one slab of one segment (gmm_tile.h's cut) and one group of G = 4 consecutive models, and works
// through the slab's 64-frame tiles in ascending order, a tile in two halves of 32 frames.  Wave w takes frames w, w + 4, ... of the half,
// one at a time; lane = d (and d + 64 above 64, added to the lane's term before the join).  Per (frame, k) the component c = idx[n][k] is
// wave-uniform; the lane reads invcov[c][d] and its frame value once and one mean value per model -- a model's row is one coalesced
// 8 D-byte load -- and the rows of entry k + 1 are fetched while entry k is reduced.  The four models' terms are joined over the 64 lanes
// by one fixed butterfly that halves the models a lane carries as it goes (topc_wave_sums) and lp goes to LDS.  Then thread (frame, model)
// of the half folds its K values in list order with lse_add: the exponentials, which would otherwise be computed 64 times over by a
// wave, are computed once.
// LDS, in doubles: Xs 64 x (D | 1), the frame tile, widened;  fl G x 64, the frames' log-likelihoods;  Lp 32 x K x G, a half's lp;  and
// 64 x K int32, the tile's lists.  At D = 60, K = 10: 46 KB, three workgroups per CU.
// grid: x = segment * nslab + slab, y = model group: workgroups that are resident together hold different frames and the same group, whose
// operand (the listed rows of C x D invcov and G x C x D means) then comes from L2.
#include "../../include/sidekit_amd/gmm_topc.h"
#include "gmm_topc_tile.h"
#include "kernels.h"

namespace sk {

constexpr int TOPC_G = 4;    // models per workgroup: the butterfly below is written for four
constexpr int TOPC_H = 32;   // frames of half a tile

__host__ __device__ inline size_t gmm_topc_score_lds(int D, int K) {
  return (size_t)(GT * gmm_xld(D) + TOPC_G * GT + TOPC_H * K * TOPC_G) * 8 + (size_t)GT * K * 4;
}

// Bounds: the slab's rows lie within [0, N] (gmm_segment, gmm_slab) and so do the rows of idx that are read; frames beyond the slab's end
// are neither read nor added; a component outside [0, C) is skipped before anything is read through it and lanes beyond D read nothing
// (topc_fetch); for models beyond M nothing is read, and what the butterfly carries in their place is neither folded nor stored; Lp is
// indexed with a frame of the half, k < K and a model of the group; mask and part are indexed with m < M and seg < S only.
template <int G, typename T>
__global__ __launch_bounds__(256) void gmm_topc_score_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mus, int M,
                                                             const double* __restrict__ invcov, const double* __restrict__ B, int C,
                                                             const int* __restrict__ seg_off, int S, long max_len, int nslab,
                                                             const unsigned char* __restrict__ mask, const int* __restrict__ idx, int K,
                                                             double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* fl = Xs + GT * xld;      // [G][GT]
  double* Lp = fl + G * GT;                 // [TOPC_H][K][G]
  int* Is = (int*)(Lp + TOPC_H * K * G);    // [GT][K]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int seg = blockIdx.x / nslab, slab = blockIdx.x % nslab, m0 = blockIdx.y * G;
  const int nmod = M - m0 < G ? M - m0 : G;
  if (mask) {   // a group without a trial on this segment has nothing to do
    bool any = false;
    for (int j = 0; j < nmod; ++j) any = any || mask[(long)(m0 + j) * S + seg] != 0;
    if (!any) return;
  }
  const GmmRows segment = gmm_segment(seg_off, seg, N, max_len);
  if (slab >= gmm_slabs(segment.len())) return;   // the grid is sized for the longest segment
  const GmmRows rows = gmm_slab(segment, slab);
  const long k_begin = rows.begin, k_end = rows.end;
  const long CD = (long)C * D;
  const bool two = D > 64;                      // a second pass over d for lanes d + 64
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  const double* mg = mus + (long)m0 * CD;

  auto fetch = [&](int f, int k, TopcRow<G>& r) {
    topc_fetch<G>(__builtin_amdgcn_readfirstlane(Is[f * K + k]), C, D, lane, invcov, mg, CD, nmod, r);
  };

  double total = 0.0;   // thread j < nmod: model m0 + j's sum over the slab
  for (long t0 = k_begin; t0 < k_end; t0 += GT) {
    const int nvalid = k_end - t0 < GT ? (int)(k_end - t0) : GT;
    __syncthreads();   // every wave is done with the previous tile's Xs, Is and fl
    gmm_load_frames(X, D, t0, nvalid, Xs, xld);
    for (int e = tid; e < nvalid * K; e += 256) Is[e] = idx[t0 * K + e];
    __syncthreads();
    for (int h0 = 0; h0 < nvalid; h0 += TOPC_H) {
      const int hend = h0 + TOPC_H < nvalid ? h0 + TOPC_H : nvalid;
      for (int f = h0 + wave; f < hend; f += 4) {
        const double x0 = ok0 ? Xs[f * xld + lane] : 0.0;
        const double x1 = two && ok1 ? Xs[f * xld + lane + 64] : 0.0;
        TopcRow<G> cur, nxt;
        fetch(f, 0, cur);
        for (int k = 0; k < K; ++k) {
          if (k + 1 < K) fetch(f, k + 1, nxt);
          double lp = -INFINITY;   // a component outside [0, C): nothing to add
          if (cur.c >= 0) {
            double t[G];
            topc_terms<G>(cur, x0, x1, two, t);
            lp = -0.5 * (topc_wave_sums(t, lane) + B[cur.c]);
          }
          if ((lane & 15) == 0) Lp[((f - h0) * K + k) * G + (lane >> 4)] = lp;   // a model beyond nmod: a value nobody reads
          if (k + 1 < K) cur = nxt;
        }
      }
      __syncthreads();
      if (tid < TOPC_H * G) {   // thread (frame, model) of the half: the fold over k in list order
        const int f = h0 + tid / G, j = tid % G;
        if (f < hend && j < nmod) {
          double m = -INFINITY, s = 0.0;
          for (int k = 0; k < K; ++k) lse_add(m, s, Lp[((f - h0) * K + k) * G + j]);
          fl[j * GT + f] = lse_value(m, s);
        }
      }
      __syncthreads();   // Lp is free
    }
    if (tid < nmod) {   // the tile's frames in frame order
      double s = 0.0;
      for (int f = 0; f < nvalid; ++f) s += fl[tid * GT + f];
      total += s;
    }
  }
  if (tid < nmod && (!mask || mask[(long)(m0 + tid) * S + seg])) part[((long)slab * M + m0 + tid) * S + seg] = total;
}

template <typename T>
static int launch_gmm_topc_score(const T* X, long N, int D, const double* mus, int M, const double* invcov, const double* B, int C,
                                 const int* seg_off, int S, long max_len, const unsigned char* mask, const int* idx, int K, double* llk,
                                 hipStream_t st) {
  constexpr int G = TOPC_G;
  const int nslab = (int)gmm_slabs(max_len);
  const long MS = (long)M * S;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);
  double* part = llk;
  if (nslab > 1) {
    void* ws = nullptr;
    lock.lock();   // held until the launches that use the workspace are enqueued (see plda_workspace_locked)
    SK_TRY(plda_workspace_locked(st, (size_t)nslab * MS * 8, &ws));
    part = (double*)ws;
  }
  static_assert(G == 4, "topc_wave_sums joins four models");
  const size_t lds = gmm_topc_score_lds(D, K);
  SK_TRY(gmm_allow_lds(gmm_topc_score_kernel<G, T>, lds));
  const dim3 grid((unsigned)((long)S * nslab), (unsigned)((M + G - 1) / G));
  hipLaunchKernelGGL((gmm_topc_score_kernel<G, T>), grid, dim3(256), lds, st, X, N, D, mus, M, invcov, B, C, seg_off, S, max_len, nslab, mask, idx, K,
                     part);
  SK_HIP(hipGetLastError());
  if (nslab > 1) SK_TRY(launch_gmm_score_join(part, N, seg_off, S, max_len, MS, mask, llk, st));
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_score_models_topc(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mus, int32_t M, const double* d_invcov,
                             const double* d_B, int32_t C, const int32_t* d_seg_off, int32_t S, int64_t max_len, const uint8_t* d_mask,
                             const int32_t* d_idx, int32_t K, double* d_llk, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_score_models_topc", d_X, x_dtype, N, D, d_mus, d_invcov, d_B, C));
  SK_CHECK(d_seg_off && d_idx && d_llk, SK_EARG, "sc_gmm_score_models_topc: null argument");
  SK_CHECK(M >= 1 && M <= SC_GMM_SCORE_MAX_M, SK_EARG, "sc_gmm_score_models_topc: bad sizes (M=%d with at most %d)", M, SC_GMM_SCORE_MAX_M);
  SK_TRY(gmm_check_segments("sc_gmm_score_models_topc", N, S, max_len));
  SK_TRY(gmm_check_topc("sc_gmm_score_models_topc", K, C));
  if (x_dtype == XT_F32)
    return launch_gmm_topc_score((const float*)d_X, (long)N, D, d_mus, M, d_invcov, d_B, C, d_seg_off, S, (long)max_len, d_mask, d_idx, K, d_llk,
                                 (hipStream_t)stream);
  return launch_gmm_topc_score((const double*)d_X, (long)N, D, d_mus, M, d_invcov, d_B, C, d_seg_off, S, (long)max_len, d_mask, d_idx, K, d_llk,
                               (hipStream_t)stream);
}

}  // extern "C"
