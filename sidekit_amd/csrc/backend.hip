// Back-end normalisation of x-vectors that stay on the device: the row transform of whiten_stat1 + norm_stat1 (one iteration of
// spectral_norm_stat1, sidekit/statserver.py:797-800,852-896,1317-1333), rotate_stat1 (:802-808: the LDA projection, the WCCN rotation)
// and whiten_cholesky_stat1 (:898-918).  One entry point:
//   sc_whiten_rows   Y[i][:] = f((X[i][:] - mu) . R),  f = identity or v / max(|v|, 1e-8)
// The matrices it applies come from sc_class_sums / sc_scatter_within / sc_gemm_tn (plda_train.hip) and the host's D x D algebra
// (sidekit_amd/backend.py).  X is float32 or float64 and is widened in the load; the product runs in float64 on v_mfma_f64_16x16x4_f64.
// A workgroup owns 64 rows and ALL of up to 256 output columns, so that a row's length is known before its one store: the four waves sit
// side by side along the columns (64 x 64 each at P > 128: 64 accumulator doubles per lane, the budget of dgemm_tile's 128 x 128 tile).
// No floating-point atomics; every sum has a fixed order, so a call's bits depend on its arguments alone.
#include "../../include/sidekit_amd.h"
#include "dgemm_tile.h"
#include "kernels.h"

namespace sk {

// what a launch does with its tile of (X - mu) . R
enum { WR_STORE = 0,          // store it; `normalize`: divided by the row's length, all of whose columns this workgroup holds (gridDim.y == 1)
       WR_SUMSQ = 1,          // P > 256, first pass: store nothing but the tile's share of each row's sum of squares, ss[blockIdx.y][row]
       WR_STORE_SCALED = 2    // P > 256, second pass: the product again, divided by the length the first pass's shares add up to
};

// grid: x = strip of 64 rows, y = block of 64 * CT columns.  LDS images as in dgemm_tile: [row][k] and [column][k], 17-double stride, the
// next k-tile in registers while this one is multiplied.  Bounds: the tile zero-fills beyond N, D and P; stores are guarded by
// row < N, column < P; ss is indexed [blockIdx.y][row < N].
template <int CT, typename TX, typename TY>
__global__ __launch_bounds__(256, 2) void whiten_rows_kernel(const TX* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                             const double* __restrict__ R, int P, TY* __restrict__ Y, int normalize, int mode,
                                                             double* __restrict__ ss) {
  constexpr int TR = 64, TC = 64 * CT;   // rows and columns of the workgroup tile
  constexpr int PX = TR * DK / 2 / 256;  // double pairs of X per thread and k-tile
  constexpr int PR = TC * DK / 2 / 256;  // double pairs of R
  __shared__ __attribute__((aligned(16))) double As[TR * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TC * DLD];
  __shared__ double red[4][TR];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const long r0 = blockIdx.x * (long)TR;
  const int n0 = blockIdx.y * TC;
  const bool vec_x = (D & 1) == 0 && (reinterpret_cast<size_t>(X) & (2 * sizeof(TX) - 1)) == 0;
  const bool vec_mu = (reinterpret_cast<size_t>(mu) & 15) == 0;   // mu + k with k even
  const bool vec_r = (P & 1) == 0 && (reinterpret_cast<size_t>(R) & 15) == 0;
  double2 rx[PX], rr[PR];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < PX; ++q) {   // X: 64 rows along k, less the centre (mu: one row, the same pair of it)
      const int idx = tid + 256 * q;
      double2 v = fetch_along_k(X, vec_x, r0, N, k0, D, idx);
      if (mu && r0 + along_k_row(idx) < N) {
        const double2 c = fetch_along_k(mu, vec_mu, 0, 1, k0, D, idx & 7);
        v.x -= c.x; v.y -= c.y;
      }
      rx[q] = v;
    }
#pragma unroll
    for (int q = 0; q < PR; ++q) rr[q] = fetch_across<TC>(R, vec_r, k0, D, n0, P, tid + 256 * q);   // R [D][P]
  };
  f64x4 acc[4][CT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += DK) {
    __syncthreads();   // every wave is done reading the previous k-tile
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int at = along_k_at(tid + 256 * q);
      As[at] = rx[q].x; As[at + 1] = rx[q].y;
    }
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int idx = tid + 256 * q, kk = across_k<TC>(idx), np = across_col<TC>(idx);   // across_at's places, spelled as before: through
      Bs[np * DLD + kk] = rr[q].x; Bs[(np + 1) * DLD + kk] = rr[q].y;                      // across_at, CT = 4 takes one register more
    }
    __syncthreads();
    if (k0 + DK < D) fetch(k0 + DK);
#pragma unroll
    for (int kk = 0; kk < DK; kk += 4) {
      double a[4], b[CT];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[(i * 16 + lr) * DLD + kk + lk];
#pragma unroll
      for (int j = 0; j < CT; ++j) b[j] = Bs[(wave * 16 * CT + j * 16 + lr) * DLD + kk + lk];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // acc[i][j][q] is row i * 16 + lk + 4 q, column wave * 16 CT + j * 16 + lr (columns beyond P hold zeros)
  const bool want_ss = mode == WR_SUMSQ || (mode == WR_STORE && normalize);
  if (want_ss) {   // a row's sum of squares: the lane's column tiles in order, the 16 lanes of its row group by a butterfly, the waves in order
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < CT; ++j) s += acc[i][j][q] * acc[i][j][q];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
        if (lr == 0) red[wave][i * 16 + lk + 4 * q] = s;
      }
    __syncthreads();
  }
  if (mode == WR_SUMSQ) {
    const long m = r0 + tid;
    if (tid < TR && m < N) ss[blockIdx.y * N + m] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = i * 16 + lk + 4 * q;
      const long m = r0 + row;
      if (m >= N) continue;
      double len = 1.0;
      if (mode == WR_STORE_SCALED) {
        double t = 0.0;
        for (unsigned yb = 0; yb < gridDim.y; ++yb) t += ss[yb * N + m];
        len = fmax(sqrt(t), 1e-8);
      } else if (normalize) {
        len = fmax(sqrt(((red[0][row] + red[1][row]) + red[2][row]) + red[3][row]), 1e-8);
      }
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        const int n = n0 + wave * 16 * CT + j * 16 + lr;
        if (n >= P) continue;
        const double v = acc[i][j][q];
        Y[m * P + n] = (TY)(mode == WR_STORE && !normalize ? v : v / len);   // float32 output: the float64 result rounded once
      }
    }
}

template <int CT, typename TX, typename TY>
static void launch_whiten_ct(const TX* X, long N, int D, const double* mu, const double* R, int P, TY* Y, int normalize, int mode, double* ss,
                             hipStream_t st) {
  hipLaunchKernelGGL((whiten_rows_kernel<CT, TX, TY>), dim3((unsigned)((N + 63) / 64), cdiv(P, 64 * CT)), dim3(256), 0, st, X, N, D, mu, R, P, Y,
                     normalize, mode, ss);
}

template <typename TX, typename TY>
static int launch_whiten(const TX* X, long N, int D, const double* mu, const double* R, int P, TY* Y, int normalize, hipStream_t st) {
  // the narrowest tile that holds every column: 64, 128 or 256 columns per workgroup; beyond 256 columns a normalising call runs twice,
  // first for the column blocks' shares of the rows' sums of squares (workspace, [block][row]), then for the scaled product
  if (P <= 64) { launch_whiten_ct<1>(X, N, D, mu, R, P, Y, normalize, WR_STORE, nullptr, st); SK_HIP(hipGetLastError()); return SK_OK; }
  if (P <= 128) { launch_whiten_ct<2>(X, N, D, mu, R, P, Y, normalize, WR_STORE, nullptr, st); SK_HIP(hipGetLastError()); return SK_OK; }
  if (P <= 256 || !normalize) { launch_whiten_ct<4>(X, N, D, mu, R, P, Y, normalize, WR_STORE, nullptr, st); SK_HIP(hipGetLastError()); return SK_OK; }
  void* ws = nullptr;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until both launches are enqueued (see plda_workspace_locked)
  SK_TRY(plda_workspace_locked(st, (size_t)cdiv(P, 256) * N * 8, &ws));
  launch_whiten_ct<4>(X, N, D, mu, R, P, Y, 1, WR_SUMSQ, (double*)ws, st);
  SK_HIP(hipGetLastError());
  launch_whiten_ct<4>(X, N, D, mu, R, P, Y, 1, WR_STORE_SCALED, (double*)ws, st);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_whiten_rows(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_R, int32_t P, int32_t normalize,
                   void* d_Y, int32_t y_dtype, void* stream) {
  SK_CHECK(d_X && d_R && d_Y, SK_EARG, "sc_whiten_rows: null argument");
  SK_CHECK(x_dtype == XT_F32 || x_dtype == XT_F64, SK_EARG, "sc_whiten_rows: X must be XT_F32 or XT_F64 (got %d)", x_dtype);
  SK_CHECK(y_dtype == XT_F32 || y_dtype == XT_F64, SK_EARG, "sc_whiten_rows: Y must be XT_F32 or XT_F64 (got %d)", y_dtype);
  SK_CHECK(N > 0 && N <= 0x7fffffffLL && D > 0 && D <= (1 << 20) && P > 0 && P <= (1 << 20), SK_EARG,
           "sc_whiten_rows: bad sizes (N=%lld, D=%d, P=%d)", (long long)N, D, P);
  const char* x0 = (const char*)d_X;
  const char* y0 = (const char*)d_Y;
  const size_t xb = (size_t)N * D * (x_dtype == XT_F32 ? 4 : 8), yb = (size_t)N * P * (y_dtype == XT_F32 ? 4 : 8);
  SK_CHECK(x0 + xb <= y0 || y0 + yb <= x0, SK_EARG, "sc_whiten_rows: Y may not alias X (a row's inputs are read after other rows are stored)");
  hipStream_t st = (hipStream_t)stream;
  const int nz = normalize != 0;
  if (x_dtype == XT_F32) {
    if (y_dtype == XT_F32) return launch_whiten((const float*)d_X, (long)N, D, d_mu, d_R, P, (float*)d_Y, nz, st);
    return launch_whiten((const float*)d_X, (long)N, D, d_mu, d_R, P, (double*)d_Y, nz, st);
  }
  if (y_dtype == XT_F32) return launch_whiten((const double*)d_X, (long)N, D, d_mu, d_R, P, (float*)d_Y, nz, st);
  return launch_whiten((const double*)d_X, (long)N, D, d_mu, d_R, P, (double*)d_Y, nz, st);
}

}  // extern "C"
