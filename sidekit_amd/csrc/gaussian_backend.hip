// Gaussian back-end (sidekit/lid_utils.py:57-263): closed-set identification of x-vectors that stay on the device.  Three entry points:
//   sc_class_scatter    the C per-class scatters S_c = sum_{k in c} (x_k - m_c)' (x_k - m_c) of gaussian_backend_train_hetero (:110-115)
//   sc_gauss_loglik     out[c][n] = cst_c - 0.5 |(x_n - m_c) W_c|^2, P_c = W_c W_c': the heteroscedastic log-likelihoods (:246-257)
//   sc_closed_set_llr   compute_log_likelihood_ratio (:57-72) on a C x N matrix
// The tied model needs no kernel of its own: it is sc_plda_fast with Phi = -P, Psi = P (sidekit_amd/lid_utils.py).  The D x D algebra
// (one Cholesky per class, slogdet) stays on the host.  float64 throughout, on v_mfma_f64_16x16x4_f64 through dgemm_tile.h; no
// floating-point atomics, every sum has a fixed order, so a call's bits depend on its arguments alone.
//
// Memory: sc_class_scatter writes C D^2 8 bytes (0.5 GB at C = 1000, D = 256) and, when long classes are cut into slabs, at most 512
// partial tiles of workspace (tn_cut); sc_gauss_loglik writes the C N 8 bytes of its output and C D 8 bytes of workspace, never an
// (N x D) or (N x C x D) intermediate; sc_closed_set_llr works in place.
#include <cmath>

#include "../../include/sidekit_amd/gaussian_backend.h"
#include "dgemm_tile.h"
#include "kernels.h"

namespace sk {

// ---- per-class scatters ----------------------------------------------------------------------------------------------------------
// dgemm_tile's A_KM form with A = B = the rows of one class and ca = cb = its mean.  grid: x = column tile, y = row tile,
// z = slab * C + class; a slab is rows [off[c] + slab * s, + slab) of the class, and its tile goes to out[z][D][D] (one slab: S itself).
// Bounds: offsets are clamped to [0, N] and to each other, a slab past its class's end multiplies nothing and stores zeros; the tile
// zero-fills beyond D and the slab's end; stores are guarded by m < D, n < D.
template <int WT, typename T>
__global__ __launch_bounds__(256, WT == 4 ? 2 : 4) void class_scatter_kernel(const T* __restrict__ X, long N, int D, const int* __restrict__ class_off,
                                                                             const double* __restrict__ Mc, int C, int slab,
                                                                             double* __restrict__ out) {
  constexpr int TL = 32 * WT;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  __shared__ double cs[2 * TL];
  const dgemm_lanes<WT> at;
  const int m0 = blockIdx.y * TL, n0 = blockIdx.x * TL;
  const int c = blockIdx.z % C, s = blockIdx.z / C;
  long r0 = class_off[c], r1 = class_off[c + 1];
  r0 = r0 < 0 ? 0 : (r0 > N ? N : r0);
  r1 = r1 < r0 ? r0 : (r1 > N ? N : r1);
  const long k_begin = r0 + (long)s * slab, left = r1 - k_begin;
  const int kl = left <= 0 ? 0 : (left < (long)slab ? (int)left : slab);
  const T* rows = X + (kl > 0 ? k_begin : 0L) * D;
  const double* mean = Mc + (long)c * D;
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true, true, T, T>(rows, rows, D, D, kl, m0, n0, As, Bs, acc, nullptr, mean, mean, cs);
  dgemm_store_tile(acc, at, out + (long)blockIdx.z * D * D, D, m0, n0, D, D);
}

// ---- heteroscedastic log-likelihoods -----------------------------------------------------------------------------------------------
// V[c][:] = m_c' W_c, the D-vector that centres the product: (x - m_c) W_c = x W_c - V[c].  One thread per column, k ascending.
__global__ __launch_bounds__(256) void class_offset_kernel(const double* __restrict__ means, const double* __restrict__ W, int D,
                                                           double* __restrict__ V) {
  const int c = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const double* m = means + (long)c * D;
  const double* Wc = W + (long)c * D * D;
  double v = 0.0;
  for (int k = 0; k < D; ++k) v += m[k] * Wc[(long)k * D + d];
  V[(long)c * D + d] = v;
}

// grid: x = tile of T = 32 WT rows, y = class.  The workgroup walks the column tiles of Y = X W_c - V[c] in ascending order
// (dgemm_tile<WT, true>, K = D) and never stores Y: a row's sum of squares is taken from the accumulators in an order that is the same
// for both tile edges, so that the bits of a row depend on neither N, nor the row's place in its tile, nor the tile edge --
//   1. registers: the two 16-column MFMA tiles of a 32-column group, left to right,
//   2. the 16 lanes that hold the group's columns of one row (col = lane & 15), by a butterfly (every lane ends with the same sum),
//   3. the two groups of a 64-column block, through LDS (the 64-row tile: its two column-side waves),
//   4. the 64-column blocks, ascending,
// and then out[c][n] = cst_c - 0.5 q.  Bounds: the tile zero-fills beyond N and D, V is read for n < D only (columns past D add an exact
// 0), the store is guarded by row < N.
template <int WT>
__global__ __launch_bounds__(256, WT == 4 ? 2 : 4) void gauss_loglik_kernel(const double* __restrict__ X, int N, int D, const double* __restrict__ W,
                                                                            const double* __restrict__ V, const double* __restrict__ cst,
                                                                            double* __restrict__ out) {
  constexpr int T = 32 * WT, G = WT / 2;   // G: 32-column groups per wave
  __shared__ __attribute__((aligned(16))) double As[T * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[T * DLD];
  __shared__ double red[WT][T];
  const dgemm_lanes<WT> at;
  const int tid = threadIdx.x, wn = at.wn, lr = at.lr;
  const int c = blockIdx.y, m0 = blockIdx.x * T;
  const double* Wc = W + (long)c * D * D;
  const double* Vc = V + (long)c * D;
  double qsum = 0.0;   // thread t < T: row m0 + t
  for (int n0 = 0; n0 < D; n0 += T) {
    f64x4 acc[WT][WT];
    int mt = m0, Dt = D;
    const double* Xt = X;
    const double* Wt = Wc;
    asm volatile("" : "+s"(mt), "+s"(Dt), "+s"(Xt), "+s"(Wt));   // the tile's operand addresses are formed anew per column tile: hoisted out of this loop they spill (128 tile)
    dgemm_tile<WT, true>(Xt, Wt, N, Dt, Dt, mt, n0, As, Bs, acc);
#pragma unroll
    for (int h = 0; h < G; ++h) {   // the wave's 32-column groups
      const int na = n0 + at.col(2 * h), nb = na + 16;
      const double off0 = na < D ? Vc[na] : 0.0, off1 = nb < D ? Vc[nb] : 0.0;
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double y0 = acc[i][2 * h][q] - off0, y1 = acc[i][2 * h + 1][q] - off1;
          double s = y0 * y0;
          s += y1 * y1;
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
          if (lr == 0) red[wn * G + h][at.row(i, q)] = s;
        }
    }
    __syncthreads();   // the next tile's k loop has barriers between this read of `red` and its next write
    if (tid < T) {
#pragma unroll
      for (int b = 0; b < G; ++b) qsum += red[2 * b][tid] + red[2 * b + 1][tid];
    }
  }
  if (tid < T && m0 + tid < N) out[(long)c * N + m0 + tid] = cst[c] - 0.5 * qsum;
}

// ---- closed-set log-likelihood ratios ----------------------------------------------------------------------------------------------
// llr[c][n] = log p_tar + M[c][n] - (log((1 - p_tar) / (C - 1)) + LSE_{j != c} M[j][n]); one thread per column, out may be M.
// The leave-one-out LSE is never "total minus own term" about one maximum (which loses everything where one class dominates): with
// m1 = M[a] the largest value (first index on ties) and m2 the largest of the others,
//   S1 = sum_j exp(M[j] - m1),  S2 = sum_{j != a} exp(M[j] - m2),
//   LSE_{j != a} = m2 + log S2,   LSE_{j != c} = m1 + log(S1 - exp(M[c] - m1)) for c != a, where S1 - exp(M[c] - m1) >= 1 (the term of a).
// A thread reads its column's element c before it stores it and touches no other column.
__global__ __launch_bounds__(256) void closed_set_llr_kernel(const double* M, int C, long N, double log_tar, double log_non, double* out) {
  const long n = blockIdx.x * 256L + threadIdx.x;
  if (n >= N) return;
  double m1 = M[n], m2 = -INFINITY;
  int a = 0;
  for (int c = 1; c < C; ++c) {
    const double v = M[(long)c * N + n];
    if (v > m1) { m2 = m1; m1 = v; a = c; }
    else if (v > m2) m2 = v;
  }
  double S1 = 0.0, S2 = 0.0;
  for (int c = 0; c < C; ++c) {
    const double v = M[(long)c * N + n];
    S1 += exp(v - m1);
    if (c != a) S2 += exp(v - m2);
  }
  const double lse_a = m2 + log(S2);
  for (int c = 0; c < C; ++c) {
    const double v = M[(long)c * N + n];
    const double lse = c == a ? lse_a : m1 + log(S1 - exp(v - m1));
    out[(long)c * N + n] = log_tar + v - (lse + log_non);
  }
}

template <typename T>
static int launch_class_scatter(const T* X, long N, int D, const int* class_off, const double* Mc, int C, long max_count, double* S, hipStream_t st) {
  const TnCut cut = tn_cut(max_count, D, D, C);
  SK_CHECK(cut.nsplit * C <= 65535, SK_EARG, "sc_class_scatter: %ld slabs x %d classes exceed the grid (65535)", cut.nsplit, C);
  const long total = (long)C * D * D;
  double* out = S;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);
  if (cut.nsplit > 1) {
    void* ws = nullptr;
    lock.lock();   // held until both launches are enqueued (see plda_workspace_locked)
    SK_TRY(plda_workspace_locked(st, (size_t)cut.nsplit * total * 8, &ws));
    out = (double*)ws;
  }
  const dim3 grid(cdiv(D, cut.TL), cdiv(D, cut.TL), (unsigned)(cut.nsplit * C));
  if (cut.big) hipLaunchKernelGGL((class_scatter_kernel<4, T>), grid, dim3(256), 0, st, X, N, D, class_off, Mc, C, (int)cut.slab, out);
  else hipLaunchKernelGGL((class_scatter_kernel<2, T>), grid, dim3(256), 0, st, X, N, D, class_off, Mc, C, (int)cut.slab, out);
  SK_HIP(hipGetLastError());
  if (cut.nsplit > 1) SK_TRY(launch_slab_reduce(out, (int)cut.nsplit, total, S, st));
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_class_scatter(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_class_off, const double* d_Mc, int32_t C,
                     int64_t max_count, double* d_S, void* stream) {
  SK_CHECK(d_X && d_class_off && d_Mc && d_S, SK_EARG, "sc_class_scatter: null argument");
  SK_CHECK(x_dtype == XT_F32 || x_dtype == XT_F64, SK_EARG, "sc_class_scatter: X must be XT_F32 or XT_F64 (got %d)", x_dtype);
  SK_CHECK(N > 0 && N <= 0x7fffffffLL && D > 0 && D <= 16384 && C > 0 && C <= N && max_count > 0 && max_count <= N, SK_EARG,
           "sc_class_scatter: bad sizes (N=%lld, D=%d, C=%d, max_count=%lld)", (long long)N, D, C, (long long)max_count);
  if (x_dtype == XT_F32) return launch_class_scatter((const float*)d_X, (long)N, D, d_class_off, d_Mc, C, (long)max_count, d_S, (hipStream_t)stream);
  return launch_class_scatter((const double*)d_X, (long)N, D, d_class_off, d_Mc, C, (long)max_count, d_S, (hipStream_t)stream);
}

int sc_gauss_loglik(const double* d_X, int64_t N, int32_t D, const double* d_means, const double* d_W, const double* d_cst, int32_t C,
                    double* d_out, void* stream) {
  SK_CHECK(d_X && d_means && d_W && d_cst && d_out, SK_EARG, "sc_gauss_loglik: null argument");
  SK_CHECK(N > 0 && N <= 0x7fffff00LL && D > 0 && D <= 16384 && C > 0 && C <= 65535, SK_EARG, "sc_gauss_loglik: bad sizes (N=%lld, D=%d, C=%d)",
           (long long)N, D, C);
  hipStream_t st = (hipStream_t)stream;
  void* ws = nullptr;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until both launches are enqueued (see plda_workspace_locked)
  SK_TRY(plda_workspace_locked(st, (size_t)C * D * 8, &ws));
  double* V = (double*)ws;
  hipLaunchKernelGGL(class_offset_kernel, dim3(cdiv(D, 256), C), dim3(256), 0, st, d_means, d_W, D, V);
  SK_HIP(hipGetLastError());
  const bool big = (long)cdiv((int)N, 128) * C >= 512;   // sc_plda_fast's rule: two 128 x 128 workgroups per CU and still two rounds of them
  if (big) hipLaunchKernelGGL(gauss_loglik_kernel<4>, dim3(cdiv((int)N, 128), C), dim3(256), 0, st, d_X, (int)N, D, d_W, V, d_cst, d_out);
  else hipLaunchKernelGGL(gauss_loglik_kernel<2>, dim3(cdiv((int)N, 64), C), dim3(256), 0, st, d_X, (int)N, D, d_W, V, d_cst, d_out);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_closed_set_llr(const double* d_M, int32_t C, int64_t N, double p_tar, double* d_out, void* stream) {
  SK_CHECK(d_M && d_out, SK_EARG, "sc_closed_set_llr: null argument");
  SK_CHECK(C >= 2, SK_EARG, "sc_closed_set_llr: a closed set has at least two classes (C=%d)", C);
  SK_CHECK(N > 0 && N <= (1LL << 38), SK_EARG, "sc_closed_set_llr: bad size (N=%lld)", (long long)N);
  SK_CHECK(p_tar > 0.0 && p_tar < 1.0, SK_EARG, "sc_closed_set_llr: p_tar must be in (0, 1) (got %g)", p_tar);
  hipLaunchKernelGGL(closed_set_llr_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_M, C, (long)N, std::log(p_tar),
                     std::log((1.0 - p_tar) / (C - 1)), d_out);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
