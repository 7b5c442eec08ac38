// GMM-UBM scoring (sidekit/gmm_scoring.py:53-116): the log-likelihood of every test segment under M mean-adapted models of one diagonal
// mixture, llk[m][s] = sum_n log sum_c exp lp_m[n][c] (include/sidekit_amd/gmm_scoring.h).  The body is pass A of gmm.hip with a model
// dimension; the frame load, the segment and its slab, the log-sum-exp update, merge and value and the argument checks are gmm_tile.h's,
// the same functions gmm.hip calls; half_gemm and the join of a tile's frames below are copies of gmm.hip's (gmm_lp_tile's chunk loop, pass A's
// end), kept identical by hand: lp_m = -0.5 ([X^2, X] . [invcov, -2 mu_m invcov]' + A_m) tile by tile on v_mfma_f64_16x16x4_f64.  The squares' half of that
// GEMM does not depend on the model, so a workgroup computes it once per component tile for a group of G consecutive models and every
// model's accumulator starts from it: (1 + G) / 2 G of the FLOP of G separate passes.  float64, no floating-point atomics.
//
// One workgroup = 256 threads = 4 waves owns one slab of one segment (gmm_tile.h's cut) and one group of G models, and works through the
// slab's 64-frame tiles in ascending order.  Per tile it walks the component tiles in ascending order; wave w owns components
// 16 w .. 16 w + 15 of the tile and all 64 frames (16 accumulator doubles per lane, kept for the squares, and 16 more per model in turn).
// Each lane keeps an online log-sum-exp state (max, sum) for its 16 frames and each of the G models: 64 G VGPRs.  LDS, in doubles:
//   Xs  64 x (D | 1)   the frame tile, widened; squares are formed in the fragment read
//   Gs  64 x 17        one 16-wide k-chunk of the component operand (invcov, or -2 mu_m invcov formed in the load); the next chunk --
//                      of the next half, model or component tile -- is fetched into registers meanwhile
//   red 2 x 4 x 64     the four waves' states of a frame;   fl  G x 64   the frames' log-likelihoods of the tile
//   Qs  16 x 256       G = 2 only: the squares' accumulator while the second model takes its turn (gmm_score_qlds below)
// At D = 60: 45 KB (78 KB with Qs), two workgroups per CU for G <= 2; at D = 128: 80 KB (113 KB with Qs).
// grid: x = segment * nslab + slab, y = model group: workgroups that are resident together hold different frames and the same group, whose
// operand (C x D invcov and G x C x D means) then comes from L2.
#include "../../include/sidekit_amd/gmm_scoring.h"
#include "gmm_tile.h"
#include "kernels.h"

#ifndef SC_GMM_SCORE_G
#define SC_GMM_SCORE_G 2   // models per workgroup (1, 2 or 4): DESIGN section 4 "GMM-UBM scoring" has the measurement
#endif

namespace sk {

// A[m][c] = sum_d mus[m][c][d]^2 invcov[c][d] + B[c]: one thread per (m, c), d ascending, so a row's bits depend on that row alone.
__global__ __launch_bounds__(256) void gmm_score_A_kernel(const double* __restrict__ mus, const double* __restrict__ invcov,
                                                          const double* __restrict__ B, long MC, int C, int D, double* __restrict__ A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MC) return;
  const int c = (int)(i % C);
  const double* mu = mus + i * D;
  const double* ic = invcov + (long)c * D;
  double s = 0.0;
  for (int d = 0; d < D; ++d) s += mu[d] * mu[d] * ic[d];
  A[i] = s + B[c];
}

// Where the squares' half of a component tile waits while the models take their turns: in 32 VGPRs, or in LDS (16 doubles per lane, 32 KB,
// each lane its own) where the registers are what keeps two workgroups on a CU: G = 2 needs 283 VGPRs with it in registers, 256 are there.
__host__ __device__ constexpr bool gmm_score_qlds(int G) { return G == 2; }
__host__ __device__ inline size_t gmm_score_lds(int G, int D) {
  return (size_t)(GT * gmm_xld(D) + GT * DLD + 8 * GT + G * GT + (gmm_score_qlds(G) ? 16 * 256 : 0)) * 8;
}

// Bounds: the slab's rows lie within [0, N] (gmm_segment, gmm_slab); frames beyond the slab's end are zero rows that are not added;
// components beyond C are zero operand rows that are skipped in the fold; models beyond M are neither computed nor
// stored; mask and part are indexed with m < M and seg < S only.
template <int G, typename T>
__global__ __launch_bounds__(256, G <= 2 ? 2 : 1) void gmm_score_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mus,
                                                                        int M, const double* __restrict__ invcov, const double* __restrict__ A, int C,
                                                                        const int* __restrict__ seg_off, int S, long max_len, int nslab,
                                                                        const unsigned char* __restrict__ mask, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Gs = Xs + GT * xld;
  double* red = Gs + GT * DLD;   // [2][4][GT]
  double* fl = red + 8 * GT;     // [G][GT]
  double* Qs = fl + G * GT;      // [16][256] when the squares' half is kept in LDS
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  constexpr bool QLDS = gmm_score_qlds(G);
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

  const int sr = tid >> 2, sd = (tid & 3) * 4;   // staging: component row sr, four consecutive d from sd
  const int nchunk = (D + DK - 1) / DK, nhalf = 1 + nmod;
  const long CD = (long)C * D;
  // the operand chunk after the one in LDS: (component tile, half: 0 = squares, 1 + j = model j's linear half, 16-wide chunk)
  int n_c0 = 0, n_half = 0, n_ch = 0;
  double g[4];
  auto fetch = [&]() {
    const int d0 = n_ch * DK + sd;
    const bool ok = n_c0 + sr < C;
    const int row = (n_c0 + sr) * D;   // C D < 2^31 (SC_GMM_MAX_C, SC_GMM_MAX_D)
    const double* mu = n_half > 0 ? mus + (long)(m0 + n_half - 1) * CD : invcov;   // the squares' half reads invcov alone
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double v = 0.0;
      if (ok && d0 + u < D) {
        const double ic = invcov[row + d0 + u];
        v = n_half > 0 ? -2.0 * mu[row + d0 + u] * ic : ic;
      }
      g[u] = v;
    }
    if (++n_ch == nchunk) {
      n_ch = 0;
      if (++n_half == nhalf) { n_half = 0; n_c0 += GT; }
    }
  };
  // one half of the GEMM (K = D) into acc: the operand chunks come through Gs in order, the next one is fetched during the multiplies
  auto half_gemm = [&](f64x4 (&acc)[4], const bool lin) {
    for (int ch = 0; ch < nchunk; ++ch) {
      __syncthreads();   // every wave is done with the previous chunk (and, the first time, Xs is complete)
#pragma unroll
      for (int u = 0; u < 4; ++u) Gs[sr * DLD + sd + u] = g[u];
      __syncthreads();
      if (n_c0 < C) fetch();
      const int d0 = ch * DK;
#pragma unroll
      for (int kk = 0; kk < DK; kk += 4) {
        const int d = d0 + kk + lk;
        const double b = Gs[(wave * 16 + lr) * DLD + kk + lk];
        double a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double x = d < D ? Xs[(i * 16 + lr) * xld + d] : 0.0;
          a[i] = lin ? x : x * x;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b, acc[i], 0, 0, 0);
      }
    }
  };

  double total = 0.0;   // thread j < nmod: model m0 + j's sum over the slab
  for (long t0 = k_begin; t0 < k_end; t0 += GT) {
    const int nvalid = k_end - t0 < GT ? (int)(k_end - t0) : GT;
    __syncthreads();   // every wave is done with the previous tile's Xs and fl
    gmm_load_frames(X, D, t0, nvalid, Xs, xld);
    double Mx[G][4][4], Sx[G][4][4];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) { Mx[j][i][q] = -INFINITY; Sx[j][i][q] = 0.0; }
    n_c0 = 0; n_half = 0; n_ch = 0;
    fetch();
    for (int c0 = 0; c0 < C; c0 += GT) {
      f64x4 accq[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) accq[i] = f64x4{0.0, 0.0, 0.0, 0.0};
      half_gemm(accq, false);
      if (QLDS && nmod > 1) {   // a lane reads back what it wrote: no barrier
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) Qs[(i * 4 + q) * 256 + tid] = accq[i][q];
      }
      const int c = c0 + wave * 16 + lr;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (j >= nmod) break;
        f64x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (QLDS && j > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = Qs[(i * 4 + q) * 256 + tid];
          } else {
            acc[i] = accq[i];
          }
        }
        half_gemm(acc, true);
        if (c < C) {
          const double a = A[(long)(m0 + j) * C + c];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) lse_add(Mx[j][i][q], Sx[j][i][q], -0.5 * (acc[i][q] + a));
        }
      }
    }
    // per model: the 16 lanes of a frame by a butterfly, the four waves through LDS in wave order (pass A's join), then log
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (j >= nmod) break;
      __syncthreads();   // red is free
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) {
            const double m2 = __shfl_xor(Mx[j][i][q], o), s2 = __shfl_xor(Sx[j][i][q], o);
            lse_merge(Mx[j][i][q], Sx[j][i][q], m2, s2);
          }
          if (lr == 0) {
            red[wave * GT + i * 16 + lk + 4 * q] = Mx[j][i][q];
            red[(4 + wave) * GT + i * 16 + lk + 4 * q] = Sx[j][i][q];
          }
        }
      __syncthreads();
      if (tid < GT) {
        double m = red[tid], s = red[4 * GT + tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) lse_merge(m, s, red[w * GT + tid], red[(4 + w) * GT + tid]);
        fl[j * GT + tid] = lse_value(m, s);
      }
    }
    __syncthreads();
    if (tid < nmod) {   // the tile's frames in frame order; a row outside the slab is not added
      double s = 0.0;
      for (int f = 0; f < nvalid; ++f) s += fl[tid * GT + f];
      total += s;
    }
  }
  if (tid < nmod && (!mask || mask[(long)(m0 + tid) * S + seg])) part[((long)slab * M + m0 + tid) * S + seg] = total;
}

// llk[m][s] = the segment's slab partials in ascending order, for the trials of the mask (gmm_topc.hip's scoring kernel cuts and stores
// as gmm_score_kernel does and is joined by the same launch)
__global__ __launch_bounds__(256) void gmm_score_join_kernel(const double* __restrict__ part, long N, const int* __restrict__ seg_off, int S,
                                                             long max_len, long MS, const unsigned char* __restrict__ mask,
                                                             double* __restrict__ llk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MS || (mask && !mask[i])) return;
  const int seg = (int)(i % S);
  const long n = gmm_slabs(gmm_segment(seg_off, seg, N, max_len).len());   // the slots the scoring kernel wrote
  double s = part[i];
  for (long k = 1; k < n; ++k) s += part[k * MS + i];
  llk[i] = s;
}

int launch_gmm_score_join(const double* part, long N, const int* seg_off, int S, long max_len, long MS, const unsigned char* mask, double* llk,
                          hipStream_t st) {
  hipLaunchKernelGGL(gmm_score_join_kernel, dim3((unsigned)((MS + 255) / 256)), dim3(256), 0, st, part, N, seg_off, S, max_len, MS, mask, llk);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <typename T>
static int launch_gmm_score(const T* X, long N, int D, const double* mus, int M, const double* invcov, const double* B, int C, const int* seg_off,
                            int S, long max_len, const unsigned char* mask, double* llk, hipStream_t st) {
  constexpr int G = SC_GMM_SCORE_G;
  static_assert(G == 1 || G == 2 || G == 4, "SC_GMM_SCORE_G: 1, 2 or 4 models per workgroup");
  const int nslab = (int)gmm_slabs(max_len);
  const long MC = (long)M * C, MS = (long)M * S;
  std::unique_lock<std::mutex> lock(g_plda_mu);   // held until the launches that use the workspace are enqueued (see plda_workspace_locked)
  void* ws = nullptr;
  SK_TRY(plda_workspace_locked(st, (size_t)(MC + (nslab > 1 ? nslab * MS : 0)) * 8, &ws));
  double* A = (double*)ws;
  double* part = nslab > 1 ? A + MC : llk;
  hipLaunchKernelGGL(gmm_score_A_kernel, dim3((unsigned)((MC + 255) / 256)), dim3(256), 0, st, mus, invcov, B, MC, C, D, A);
  SK_HIP(hipGetLastError());
  const size_t lds = gmm_score_lds(G, D);
  SK_TRY(gmm_allow_lds(gmm_score_kernel<G, T>, lds));
  const dim3 grid((unsigned)((long)S * nslab), (unsigned)((M + G - 1) / G));
  hipLaunchKernelGGL((gmm_score_kernel<G, T>), grid, dim3(256), lds, st, X, N, D, mus, M, invcov, A, C, seg_off, S, max_len, nslab, mask, part);
  SK_HIP(hipGetLastError());
  if (nslab > 1) SK_TRY(launch_gmm_score_join(part, N, seg_off, S, max_len, MS, mask, llk, st));
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_score_models(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mus, int32_t M, const double* d_invcov,
                        const double* d_B, int32_t C, const int32_t* d_seg_off, int32_t S, int64_t max_len, const uint8_t* d_mask, double* d_llk,
                        void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_score_models", d_X, x_dtype, N, D, d_mus, d_invcov, d_B, C));
  SK_CHECK(d_seg_off && d_llk, SK_EARG, "sc_gmm_score_models: null argument");
  SK_CHECK(M >= 1 && M <= SC_GMM_SCORE_MAX_M, SK_EARG, "sc_gmm_score_models: bad sizes (M=%d with at most %d)", M, SC_GMM_SCORE_MAX_M);
  SK_TRY(gmm_check_segments("sc_gmm_score_models", N, S, max_len));
  if (x_dtype == XT_F32)
    return launch_gmm_score((const float*)d_X, (long)N, D, d_mus, M, d_invcov, d_B, C, d_seg_off, S, (long)max_len, d_mask, d_llk, (hipStream_t)stream);
  return launch_gmm_score((const double*)d_X, (long)N, D, d_mus, M, d_invcov, d_B, C, d_seg_off, S, (long)max_len, d_mask, d_llk, (hipStream_t)stream);
}

}  // extern "C"
