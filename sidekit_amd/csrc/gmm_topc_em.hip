// Top-C EM (include/sidekit_amd/gmm_topc_em.h): a frame's list of K components refreshed from a row of Kc <= 64 candidates,
//   sc_gmm_topc_refine   lp[j] = -0.5 (sum_d (X[n][d] - mu[c][d])^2 invcov[c][d] + B[c]), c = cand[n][j] where valid; idx[n] = the K best by
//                        (lp, then the lower index), ascending; optionally post / lse over idx[n] as sc_gmm_topc_posteriors forms them
// 2 Kc D of gather work per frame whatever C is: what keeps the lists of EM_split's mixture current between two E-steps (the children of
// the parents a frame listed) without gmm.hip's pass over all C components.  float64, no atomics, no workspace.  The scoring loop
// over a row held in a register and the end of a tile of posteriors are gmm_topc_tile.h's, the functions gmm_topc_post_kernel
// (gmm_topc_stats.hip) calls: lp, post and lse have the bits that kernel forms for the same list.
//
// One workgroup = 256 threads = 4 waves owns a tile of GT = 64 frames; wave w takes frames w, w + 4, ... one at a time; lane = d (and
// d + 64 above 64) in the scoring, lane = candidate in the selection.  The wave holds the frame's row of candidates in a register (lane j:
// entry j).  An entry is struck out (-1) when it lies outside [0, C) or an earlier lane holds the same value: Kc scalar broadcasts.
// Scoring is topc_frame_lps: per entry the component is wave-uniform, a row of invcov and of mu is one coalesced 8 D-byte
// load each, the rows of entry j + 1 are fetched while entry j is reduced; lane j keeps lp[j].  Selection: lane j counts the valid
// entries that beat its own (Kc broadcasts), the winners are the lanes with fewer than K; a ballot gives them, and a winner's place in
// the list is the number of winners with a lower component (at most K broadcasts).  With the posteriors, a winner's lp goes to LDS at
// its place and the tile ends as gmm_topc_post_kernel does: thread f folds frame f's K values in list order, thread (f, k) forms the
// posterior.  LDS: 64 x K + 64 doubles, 17 KB at K = 32; none without the posteriors.
#include "../../include/sidekit_amd/gmm_topc_em.h"
#include "gmm_topc_tile.h"
#include "kernels.h"

namespace sk {

// Bounds: frames beyond N are neither read nor stored; a frame's row of candidates is read for j < Kc <= 64 only; a candidate outside
// [0, C) is struck out here (and again by topc_frame_lps) before anything is read through it; a winner's place is below its frame's number of
// winners <= K, so idx, post and Lp are indexed with a frame of the tile and k < K.
template <typename T>
__global__ __launch_bounds__(256) void gmm_topc_refine_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                              const double* __restrict__ invcov, const double* __restrict__ B, int C,
                                                              const int* __restrict__ cand, int Kc, int K, int* __restrict__ idx,
                                                              double* __restrict__ post, double* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  double* Lp = gmm_smem;       // [GT][K]   (post != null)
  double* fl = Lp + GT * K;    // [GT]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long f0 = (long)blockIdx.x * GT;
  const int nvalid = N - f0 < GT ? (int)(N - f0) : GT;
  const bool ok0 = lane < D, ok1 = lane + 64 < D;
  for (int f = wave; f < nvalid; f += 4) {
    const long n = f0 + f;
    const double x0 = ok0 ? (double)X[n * D + lane] : 0.0;
    const double x1 = ok1 ? (double)X[n * D + lane + 64] : 0.0;
    int mine = lane < Kc ? cand[n * Kc + lane] : -1;
    if (mine < 0 || mine >= C) mine = -1;
    {
      bool dup = false;   // an earlier entry of the row holds the same value
      for (int j = 0; j + 1 < Kc; ++j) dup |= j < lane && __builtin_amdgcn_readlane(mine, j) == mine;
      if (dup) mine = -1;
    }
    double mylp = -INFINITY;   // lane j: the lp of entry j as formed, -inf for a struck-out entry
    topc_frame_lps(x0, x1, mine, Kc, lane, D, mu, invcov, B, C, [&](int j, double lp) {
      if (lane == j) mylp = lp;
    });
    const double key = mylp != mylp ? -INFINITY : mylp;   // its ranking key: a nan lp ranks as -inf
    // how many valid entries beat mine: the larger key, at equal keys the lower component; the valid entries are distinct, so the
    // ranks of the valid lanes are 0 .. (their number) - 1, each once
    int rank = 0;
    for (int j = 0; j < Kc; ++j) {
      const int cj = __builtin_amdgcn_readlane(mine, j);
      const double kj = topc_em_readlane(key, j);
      rank += cj >= 0 && (kj > key || (kj == key && cj < mine));
    }
    const bool win = mine >= 0 && rank < K;
    unsigned long long winners = __ballot(win);
    const int nwin = __popcll(winners);   // min(K, valid entries)
    int place = 0;                        // ascending component order
    while (winners) {
      const int j = __ffsll(winners) - 1;
      winners &= winners - 1;
      place += __builtin_amdgcn_readlane(mine, j) < mine;
    }
    if (win) idx[n * K + place] = mine;
    if (lane >= nwin && lane < K) idx[n * K + lane] = -1;   // K <= 32 < 64
    if (post) {
      if (win) Lp[f * K + place] = mylp;
      if (lane >= nwin && lane < K) Lp[f * K + lane] = -INFINITY;   // what gmm_topc_post_kernel forms for an index of -1
    }
  }
  if (!post) return;   // a kernel argument: the whole workgroup leaves
  topc_fold_and_posteriors(Lp, fl, f0, nvalid, K, post, lse);
}

template <typename T>
static int launch_gmm_topc_refine(const T* X, long N, int D, const double* mu, const double* invcov, const double* B, int C, const int* cand,
                                  int Kc, int K, int* idx, double* post, double* lse, hipStream_t st) {
  const size_t lds = post ? (size_t)(GT * K + GT) * 8 : 0;
  hipLaunchKernelGGL(gmm_topc_refine_kernel<T>, dim3((unsigned)((N + GT - 1) / GT)), dim3(256), lds, st, X, N, D, mu, invcov, B, C, cand, Kc, K, idx,
                     post, lse);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_topc_refine(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_B,
                       int32_t C, const int32_t* d_cand, int32_t Kc, int32_t K, int32_t* d_idx, double* d_post, double* d_lse, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_topc_refine", d_X, x_dtype, N, D, d_mu, d_invcov, d_B, C));
  SK_CHECK(d_cand && d_idx, SK_EARG, "sc_gmm_topc_refine: null argument");
  SK_CHECK(!d_post == !d_lse, SK_EARG, "sc_gmm_topc_refine: d_post and d_lse are both null or both given");
  SK_CHECK(Kc >= 1 && Kc <= SC_GMM_TOPC_CAND_MAX, SK_EARG, "sc_gmm_topc_refine: Kc=%d outside [1, %d]", Kc, SC_GMM_TOPC_CAND_MAX);
  SK_TRY(gmm_check_topc("sc_gmm_topc_refine", K, C));
  if (x_dtype == XT_F32)
    return launch_gmm_topc_refine((const float*)d_X, (long)N, D, d_mu, d_invcov, d_B, C, d_cand, Kc, K, d_idx, d_post, d_lse, (hipStream_t)stream);
  return launch_gmm_topc_refine((const double*)d_X, (long)N, D, d_mu, d_invcov, d_B, C, d_cand, Kc, K, d_idx, d_post, d_lse, (hipStream_t)stream);
}

}  // extern "C"
