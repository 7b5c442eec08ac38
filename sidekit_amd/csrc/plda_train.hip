// PLDA training (sidekit/factor_analyser.py:830-932, FactorAnalyser.plda) from x-vectors that stay on the device.
//
// Everything with an utterance (N) or class (C) dimension runs here in float64; the D x D and rank x rank algebra (eigh, solve,
// cholesky, one inverse) stays on the host, the split scoring.hip makes.  Four entry points:
//   sc_class_sums   per-class sums of the rows of X (StatServer.sum_stat_per_model, statserver.py:1335-1355) and the column sums
//   sc_gemm_tn      G = sum_k w[k] (A[k][:] - a)^T (B[k][:] - b): the total scatter (K = N) and the three class-sized accumulators
//   sc_dgemm_nn     C = A . B with a rank-one or a posterior-scale epilogue: the whitened class sums and the E-step
//   sc_scatter_within  G = sum_k w[cls[k]] (X[k][:] - Mc[cls[k]][:])^T (X[k][:] - Mc[cls[k]][:]): the within-class scatter of the
//                   back-end normalisations (statserver.py:940-1054), the TN product with a gathered per-row centre
// x-vectors arrive as float32 or float64 and are widened in the load.  No floating-point atomics: partial sums (class slices, row
// slabs of the TN product) are written to the sc_* workspace and added in a fixed order, so a call's bits depend on its arguments alone.
#include "../../include/sidekit_amd.h"
#include "dgemm_tile.h"
#include "kernels.h"

namespace sk {

// ---- class sums ------------------------------------------------------------------------------------------------------------------
// The host hands over a CSR of the class index: rows[] = row numbers grouped by class (ascending inside a class), cut into slices of
// at most a few hundred rows that never straddle a class.  One workgroup per slice adds its rows in that order (thread = column), one
// workgroup per class then adds the class's slices in order.  Bounds: rows[] entries outside [0, N) are skipped, offsets are clamped to
// [0, N] / [0, n_slices].
template <typename T>
__global__ __launch_bounds__(256) void class_slice_sum_kernel(const T* __restrict__ X, long N, int D, const int* __restrict__ rows,
                                                              const int* __restrict__ slice_off, double* __restrict__ part) {
  const int s = blockIdx.x, r0 = slice_off[s] < 0 ? 0 : slice_off[s], r1 = (long)slice_off[s + 1] > N ? (int)N : slice_off[s + 1];
  auto at = [&](int r, int d) {
    const long row = rows[r];
    return row >= 0 && row < N ? (double)X[row * D + d] : 0.0;
  };
  for (int d = threadIdx.x; d < D; d += 256) {
    double acc = 0.0;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {   // four loads in flight, added in row order
      const double v0 = at(r, d), v1 = at(r + 1, d), v2 = at(r + 2, d), v3 = at(r + 3, d);
      acc += v0; acc += v1; acc += v2; acc += v3;
    }
    for (; r < r1; ++r) acc += at(r, d);
    part[(long)s * D + d] = acc;
  }
}

__global__ __launch_bounds__(256) void class_reduce_kernel(const double* __restrict__ part, const int* __restrict__ class_slice_off, int n_slices,
                                                           int D, double* __restrict__ S) {
  const int c = blockIdx.x, s0 = class_slice_off[c] < 0 ? 0 : class_slice_off[c], s1 = class_slice_off[c + 1] > n_slices ? n_slices : class_slice_off[c + 1];
  for (int d = threadIdx.x; d < D; d += 256) {
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += part[(long)s * D + d];
    S[(long)c * D + d] = acc;
  }
}

// colsum[d] = sum_c S[c][d]: four interleaved class streams per column, joined in a fixed order
__global__ __launch_bounds__(256) void column_sum_kernel(const double* __restrict__ S, int C, int D, double* __restrict__ colsum) {
  __shared__ double red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  double acc = 0.0;
  if (col < D) for (int c = q; c < C; c += 4) acc += S[(long)c * D + col];
  red[q][threadIdx.x & 63] = acc;
  __syncthreads();
  if (q == 0 && col < D) colsum[col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- TN product ------------------------------------------------------------------------------------------------------------------
// grid: x = column tile, y = row tile, z = row slab [z * slab, z * slab + slab) of K; out = G (one slab) or the slab's partial tile
// part[z][M][N].  Bounds: the tile zero-fills beyond M, N and the slab's end; stores are guarded by m < M, n < N.
// The operands of either TN kernel.  With cls: the centre of row k is gathered through its class number (scatter_within_kernel: B = A,
// N = M, ca = the [C][M] class means, w = the [C] class weights; cb is unused).
template <typename T>
struct TnOperands {
  const T *A, *B;
  const double *w, *ca, *cb;
  const int* cls;
  int C;
};

template <int WT, typename T>
__global__ __launch_bounds__(256, WT == 4 ? 2 : 4) void dgemm_tn_kernel(TnOperands<T> o, long K, int M, int N, int slab, double* __restrict__ out) {
  constexpr int TL = 32 * WT;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  __shared__ double cs[2 * TL];
  const dgemm_lanes<WT> at;
  const int m0 = blockIdx.y * TL, n0 = blockIdx.x * TL;
  const long k_begin = (long)blockIdx.z * slab;
  const int kl = (int)(K - k_begin < (long)slab ? K - k_begin : (long)slab);
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true, true, T, T>(o.A + k_begin * M, o.B + k_begin * N, M, N, kl, m0, n0, As, Bs, acc, o.w ? o.w + k_begin : nullptr, o.ca, o.cb, cs);
  dgemm_store_tile(acc, at, out + (long)blockIdx.z * M * N, N, m0, n0, M, N);
}

// The same grid and slabs with the centre of row k gathered through its class number (dgemm_tile's ROWC form): A = B = X, M = N = D.
// Bounds: as above; a class number outside [0, C) gives its row weight 0 and reads no centre.  Its own kernel with dgemm_lanes' map written
// out, as it was before dgemm_tn_kernel took TnOperands: as dgemm_tn_kernel<WT, T, ROWC> sc_scatter_within measured slower.
template <int WT, typename T>
__global__ __launch_bounds__(256, WT == 4 ? 2 : 4) void scatter_within_kernel(const T* __restrict__ X, long K, int D, int slab,
                                                                              const int* __restrict__ cls, const double* __restrict__ Mc,
                                                                              const double* __restrict__ w, int C, double* __restrict__ out) {
  constexpr int TL = 32 * WT;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.y * TL, n0 = blockIdx.x * TL;
  const long k_begin = (long)blockIdx.z * slab;
  const int kl = (int)(K - k_begin < (long)slab ? K - k_begin : (long)slab);
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true, true, T, T, true>(X + k_begin * D, X + k_begin * D, D, D, kl, m0, n0, As, Bs, acc, w, Mc, nullptr, nullptr, cls + k_begin, C);
  double* dst = out + (long)blockIdx.z * D * D;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + wm * 16 * WT + i * 16 + lk + 4 * q;
      if (m >= D) continue;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + wn * 16 * WT + j * 16 + lr;
        if (n < D) dst[(long)m * D + n] = acc[i][j][q];
      }
    }
}

__global__ __launch_bounds__(256) void slab_reduce_kernel(const double* __restrict__ part, int nslabs, long mn, double* __restrict__ G) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= mn) return;
  double acc = 0.0;
  for (int p = 0; p < nslabs; ++p) acc += part[p * mn + i];
  G[i] = acc;
}

// ---- NN product with the two class-sized epilogues -----------------------------------------------------------------------------------
//   SC_EPI_RANK1:     C[m][n] = alpha * sum_k A[m][k] B[k][n] - rowv[m] * colv[n]            (rowv == nullptr: no second term)
//   SC_EPI_POSTERIOR: C[m][n] = alpha * sum_k A[m][k] B[k][n] / (1 + rowv[m] * colv[n])
__global__ __launch_bounds__(256, 4) void dgemm_nn_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C, int M,
                                                          int N, int K, double alpha, const double* __restrict__ rowv,
                                                          const double* __restrict__ colv, int epilogue) {
  constexpr int WT = 2, TL = 64;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  const dgemm_lanes<WT> at;
  const int m0 = blockIdx.y * TL, n0 = blockIdx.x * TL;
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true>(A, B, M, N, K, m0, n0, As, Bs, acc);
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + at.row(i, q);
      if (m >= M) continue;
      const double rv = rowv ? rowv[m] : 0.0;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + at.col(j);
        if (n >= N) continue;
        const double t = rowv ? rv * colv[n] : 0.0, v = alpha * acc[i][j][q];
        C[(long)m * N + n] = epilogue == SC_EPI_POSTERIOR ? v / (1.0 + t) : v - t;
      }
    }
}

// The cut of a TN product: 128 x 128 tiles when the output has them and K is long (the total scatter), 64 x 64 otherwise; K is cut into
// slabs (a multiple of the k-tile) until about 512 workgroups exist.  A function of (M, N, K, batch) alone (TnCut: kernels.h).
TnCut tn_cut(long K, int M, int N, long batch) {
  TnCut c;
  c.big = M >= 128 && N >= 128 && K >= 4096;
  c.TL = c.big ? 128 : 64;
  const long tiles = batch * cdiv(M, c.TL) * cdiv(N, c.TL);
  c.nsplit = (K + 511) / 512;
  const long want = tiles >= 512 ? 1 : 512 / tiles;
  if (c.nsplit > want) c.nsplit = want;
  c.slab = (K + c.nsplit - 1) / c.nsplit;
  c.slab = (c.slab + DK - 1) / DK * DK;
  c.nsplit = (K + c.slab - 1) / c.slab;
  return c;
}

int launch_slab_reduce(const double* part, int nslabs, long mn, double* G, hipStream_t st) {
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, part, nslabs, mn, G);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

// launch(big, grid, slab, out) enqueues the tile kernel; with more than one slab its partial tiles go to the workspace and are added in
// slab order.
template <typename Launch>
static int launch_tn_slabs(long K, int M, int N, double* G, hipStream_t st, Launch launch) {
  const TnCut c = tn_cut(K, M, N);
  double* out = G;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);
  if (c.nsplit > 1) {
    void* ws = nullptr;
    lock.lock();   // held until both launches are enqueued (see plda_workspace_locked)
    SK_TRY(plda_workspace_locked(st, (size_t)c.nsplit * M * N * 8, &ws));
    out = (double*)ws;
  }
  launch(c.big, dim3(cdiv(N, c.TL), cdiv(M, c.TL), (unsigned)c.nsplit), (int)c.slab, out);
  SK_HIP(hipGetLastError());
  if (c.nsplit > 1) SK_TRY(launch_slab_reduce(out, (int)c.nsplit, (long)M * N, G, st));
  return SK_OK;
}

template <bool ROWC, typename T>
static int launch_gemm_tn(const TnOperands<T>& o, long K, int M, int N, double* G, hipStream_t st) {
  return launch_tn_slabs(K, M, N, G, st, [&](bool big, dim3 grid, int slab, double* out) {
    if constexpr (ROWC) {
      if (big) hipLaunchKernelGGL((scatter_within_kernel<4, T>), grid, dim3(256), 0, st, o.A, K, M, slab, o.cls, o.ca, o.w, o.C, out);
      else hipLaunchKernelGGL((scatter_within_kernel<2, T>), grid, dim3(256), 0, st, o.A, K, M, slab, o.cls, o.ca, o.w, o.C, out);
    } else {
      if (big) hipLaunchKernelGGL((dgemm_tn_kernel<4, T>), grid, dim3(256), 0, st, o, K, M, N, slab, out);
      else hipLaunchKernelGGL((dgemm_tn_kernel<2, T>), grid, dim3(256), 0, st, o, K, M, N, slab, out);
    }
  });
}

// the operands of either dtype, and the launch
template <bool ROWC>
static int launch_gemm_tn(const void* A, const void* B, int32_t dtype, long K, int M, int N, const double* w, const double* ca, const double* cb,
                          const int* cls, int C, double* G, hipStream_t st) {
  if (dtype == XT_F32) return launch_gemm_tn<ROWC>(TnOperands<float>{(const float*)A, (const float*)B, w, ca, cb, cls, C}, K, M, N, G, st);
  return launch_gemm_tn<ROWC>(TnOperands<double>{(const double*)A, (const double*)B, w, ca, cb, cls, C}, K, M, N, G, st);
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_class_sums(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_rows, const int32_t* d_slice_off,
                  int32_t n_slices, const int32_t* d_class_slice_off, int32_t C, double* d_S, double* d_colsum, void* stream) {
  SK_CHECK(d_X && d_rows && d_slice_off && d_class_slice_off && d_S, SK_EARG, "sc_class_sums: null argument");
  SK_CHECK(x_dtype == XT_F32 || x_dtype == XT_F64, SK_EARG, "sc_class_sums: X must be XT_F32 or XT_F64 (got %d)", x_dtype);
  SK_CHECK(N > 0 && N <= 0x7fffffffLL && D > 0 && C > 0 && C <= N && n_slices >= C, SK_EARG,
           "sc_class_sums: bad sizes (N=%lld, D=%d, C=%d, slices=%d)", (long long)N, D, C, n_slices);
  hipStream_t st = (hipStream_t)stream;
  void* ws = nullptr;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until the launches are enqueued (see plda_workspace_locked)
  SK_TRY(plda_workspace_locked(st, (size_t)n_slices * D * 8, &ws));
  double* part = (double*)ws;
  if (x_dtype == XT_F32) hipLaunchKernelGGL(class_slice_sum_kernel<float>, dim3(n_slices), dim3(256), 0, st, (const float*)d_X, (long)N, D, d_rows, d_slice_off, part);
  else hipLaunchKernelGGL(class_slice_sum_kernel<double>, dim3(n_slices), dim3(256), 0, st, (const double*)d_X, (long)N, D, d_rows, d_slice_off, part);
  SK_HIP(hipGetLastError());
  hipLaunchKernelGGL(class_reduce_kernel, dim3(C), dim3(256), 0, st, part, d_class_slice_off, n_slices, D, d_S);
  SK_HIP(hipGetLastError());
  if (d_colsum) {
    hipLaunchKernelGGL(column_sum_kernel, dim3(cdiv(D, 64)), dim3(256), 0, st, d_S, C, D, d_colsum);
    SK_HIP(hipGetLastError());
  }
  return SK_OK;
}

int sc_gemm_tn(const void* d_A, const void* d_B, int32_t dtype, int64_t K, int32_t M, int32_t Nn, const double* d_w, const double* d_ca,
               const double* d_cb, double* d_G, void* stream) {
  SK_CHECK(d_A && d_B && d_G, SK_EARG, "sc_gemm_tn: null argument");
  SK_CHECK(dtype == XT_F32 || dtype == XT_F64, SK_EARG, "sc_gemm_tn: operands must be XT_F32 or XT_F64 (got %d)", dtype);
  SK_CHECK(K > 0 && M > 0 && Nn > 0 && (int64_t)M * Nn <= (1LL << 28), SK_EARG, "sc_gemm_tn: bad sizes (K=%lld, M=%d, Nn=%d)", (long long)K, M, Nn);
  return launch_gemm_tn<false>(d_A, d_B, dtype, (long)K, M, Nn, d_w, d_ca, d_cb, nullptr, 0, d_G, (hipStream_t)stream);
}

int sc_scatter_within(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_cls, const double* d_Mc, const double* d_w,
                      int32_t C, double* d_G, void* stream) {
  SK_CHECK(d_X && d_cls && d_Mc && d_G, SK_EARG, "sc_scatter_within: null argument");
  SK_CHECK(x_dtype == XT_F32 || x_dtype == XT_F64, SK_EARG, "sc_scatter_within: X must be XT_F32 or XT_F64 (got %d)", x_dtype);
  SK_CHECK(N > 0 && N <= 0x7fffffffLL && D > 0 && D <= 16384 && C > 0, SK_EARG, "sc_scatter_within: bad sizes (N=%lld, D=%d, C=%d)",
           (long long)N, D, C);
  return launch_gemm_tn<true>(d_X, d_X, x_dtype, (long)N, D, D, d_w, d_Mc, nullptr, d_cls, C, d_G, (hipStream_t)stream);
}

int sc_dgemm_nn(const double* d_A, const double* d_B, int32_t M, int32_t N, int32_t K, double alpha, const double* d_rowv,
                const double* d_colv, int32_t epilogue, double* d_C, void* stream) {
  SK_CHECK(d_A && d_B && d_C, SK_EARG, "sc_dgemm_nn: null argument");
  SK_CHECK(M > 0 && N > 0 && K > 0, SK_EARG, "sc_dgemm_nn: bad sizes (M=%d, N=%d, K=%d)", M, N, K);
  SK_CHECK(epilogue == SC_EPI_RANK1 || epilogue == SC_EPI_POSTERIOR, SK_EARG, "sc_dgemm_nn: unknown epilogue %d", epilogue);
  SK_CHECK((d_rowv != nullptr) == (d_colv != nullptr) && (epilogue != SC_EPI_POSTERIOR || d_rowv), SK_EARG,
           "sc_dgemm_nn: rowv and colv come together, and the posterior epilogue needs both");
  hipLaunchKernelGGL(dgemm_nn_kernel, dim3(cdiv(N, 64), cdiv(M, 64)), dim3(256), 0, (hipStream_t)stream, d_A, d_B, d_C, M, N, K, alpha, d_rowv,
                     d_colv, epilogue);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
