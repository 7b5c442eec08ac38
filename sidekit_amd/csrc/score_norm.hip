// Cohort score normalisation: z-, t-, zt- and s-norm of a trial matrix (sidekit/score_normalization.py:44-117, and the
// enrolment x test form of :120-140).
//
// What a normalisation needs from an impostor cohort is two numbers per enrolment (or test) vector: the mean and the standard
// deviation of its scores against the cohort.  sc_cohort_moments forms them straight from the accumulators of the cosine GEMM
// (f32 MFMA through sgemm_wave_step, the k-ordered FMA chain of sc_cosine's kernels: the same bits), so the (N x M) cohort score matrix is never written;
// sc_matrix_moments does the same for a score matrix that already exists (the Scores-level mirrors); sc_topk_stats gives the adaptive
// statistics (the k best scores of a row); sc_norm_apply / sc_snorm_apply are the elementwise pass, one kernel with three modes.  Sums
// are float64, partial sums go through the sc_* workspace and are added in a fixed order: no floating-point atomics.
// PLDA log-likelihood ratios get the same in float64 throughout: sc_plda_cohort_moments (the f64 MFMA tile of dgemm_tile.h, the scores
// of sc_plda_fast never written), sc_topk_stats_f64 and sc_norm_apply_f64 (the float32 kernels' templates at double).
#include "../../include/sidekit_amd.h"
#include "dgemm_tile.h"
#include "kernels.h"
#include "sgemm_tile.h"

namespace sk {

// Tile: 128 cohort rows x 128 X rows per 256-thread workgroup, four waves of 64 x 64 (2 x 2 accumulator tiles), k-tiles of 32 through
// LDS with the next k-tile prefetched into registers: gemm128_kernel's loop with sgemm_wave_step as the k-tile step.  The COHORT is the MFMA's row operand, so a lane's
// 32 accumulator values per 32 x 32 tile are 32 cohort scores of ONE X row: its running sum and sum of squares are two doubles per
// column tile (8 registers), not two per accumulator row (128).  a * b is commutative, so every score is the k-ordered FMA chain
// sc_cosine computes.  A workgroup walks the `tiles_per_slab` cohort tiles of slab blockIdx.y; the slab size depends on M alone, so a
// row's additions -- lane (i, q) order inside a tile, tiles in order, the two lane halves, the two cohort-side waves, then the slabs
// in cohort_moments_final_kernel -- do not depend on N, on the row's place in its tile or on the launch.
constexpr int CT = 128, CLD = 36;

template <bool AFFINE>
__global__ __launch_bounds__(256, 2) void cohort_moments_kernel(const float* __restrict__ X, int N, const float* __restrict__ C, int M, int D,
                                                                const float* __restrict__ shift, const float* __restrict__ scale, long self_off,
                                                                int tiles_per_slab, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Cs[CT * CLD];
  __shared__ __attribute__((aligned(16))) float Xs[CT * CLD];
  __shared__ double red[CT][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;   // wm: cohort side, wn: X side
  const int n0 = blockIdx.x * CT;
  const int tiles_m = (M + CT - 1) / CT, t0 = blockIdx.y * tiles_per_slab, t1 = t0 + tiles_per_slab < tiles_m ? t0 + tiles_per_slab : tiles_m;
  const int nk = (D + 31) / 32;
  const int srow = tid >> 3, sk4 = (tid & 7) * 4;   // 32 rows x 8 chunks per pass, four passes per operand
  float4 rc[4], rx[4];
  auto fetch = [&](int c0, int k0) {   // (the zero is a prvalue: a named float4 in the ternary makes it a select of ADDRESSES and the registers an array in scratch)
    const int k = k0 + sk4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = srow + q * 32;
      rc[q] = (c0 + row < M && k < D) ? *reinterpret_cast<const float4*>(C + (long)(c0 + row) * D + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      rx[q] = (n0 + row < N && k < D) ? *reinterpret_cast<const float4*>(X + (long)(n0 + row) * D + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
  fetch(t0 * CT, 0);
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * CT;
    f32x16 acc[2][2];
    sgemm_zero(acc);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<float4*>(&Cs[(srow + q * 32) * CLD + sk4]) = rc[q];
        *reinterpret_cast<float4*>(&Xs[(srow + q * 32) * CLD + sk4]) = rx[q];
      }
      __syncthreads();
      const bool wrap = kt + 1 == nk;           // then: the next cohort tile's first k-tile
      if (!wrap || t + 1 < t1) fetch(wrap ? c0 + CT : c0, wrap ? 0 : (kt + 1) * 32);
      sgemm_wave_step<2>(Cs, Xs, CLD, wm * 64 + r, wn * 64 + r, h, acc);
      __syncthreads();
    }
    // acc[i][j][q] = <C[c0 + wm*64 + i*32 + sgemm_acc_row(q, h)], X[n0 + wn*64 + j*32 + r]>
    // (a dropped value enters the sums as an exact zero: the kept values' additions are unchanged by it)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long drop = self_off >= 0 ? (long)(n0 + wn * 64 + j * 32 + r) + self_off : -1L;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int m = c0 + wm * 64 + i * 32 + sgemm_acc_row(q, h);
          double v = (double)acc[i][j][q];
          if constexpr (AFFINE) {
            const int mc = m < M ? m : M - 1;
            v = (v - (double)shift[mc]) * (double)scale[mc];
          }
          v = (m < M && (long)m != drop) ? v : 0.0;
          s1[j] += v;
          s2[j] = fma(v, v, s2[j]);
        }
    }
  }
  // the two lane halves hold the two interleaved halves of a tile's cohort rows, the two wm waves its two 64-row halves
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
    if (wm == 1 && h == 0) { red[wn * 64 + j * 32 + r][0] = s1[j]; red[wn * 64 + j * 32 + r][1] = s2[j]; }
  }
  __syncthreads();
  if (wm == 0 && h == 0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = wn * 64 + j * 32 + r, n = n0 + row;
      if (n >= N) continue;
      double* o = part + ((long)blockIdx.y * N + n) * 2;
      o[0] = s1[j] + red[row][0];
      o[1] = s2[j] + red[row][1];
    }
  }
}

// mean and population std of the values a row kept: the slabs' partials in slab order, variance clamped at 0
template <typename T>
__global__ __launch_bounds__(256) void cohort_moments_final_kernel(const double* __restrict__ part, int N, int slabs, int M, long self_off,
                                                                   T* __restrict__ mean, T* __restrict__ stdv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double a = 0.0, b = 0.0;
  for (int p = 0; p < slabs; ++p) {
    a += part[((long)p * N + i) * 2];
    b += part[((long)p * N + i) * 2 + 1];
  }
  const long d = self_off >= 0 ? (long)i + self_off : -1L;
  const double cnt = (double)(M - ((d >= 0 && d < (long)M) ? 1 : 0));
  const double m = a / cnt, var = b / cnt - m * m;
  mean[i] = (T)m;
  stdv[i] = (T)sqrt(var > 0.0 ? var : 0.0);
}

// ---- the same statistics of PLDA log-likelihood ratios (sc_plda_cohort_moments) ----------------------------------------------------
// v_ij = alpha * (x_i' Psi c_j + xterm(i) + cterm(j) + cst): dgemm_nt_kernel's value for sc_plda_fast(X, C), never written.  Tile:
// 128 cohort rows x 128 X rows per 256-thread workgroup through dgemm_tile<4, false>, the COHORT as the tile's row operand and X . Psi
// (plda_prep_kernel's) as its column operand: a * b is commutative, so an accumulator is the chain of v_mfma_f64_16x16x4_f64 over
// ascending k that sc_plda_fast computes for the pair.  In the f64 accumulator map a lane's acc[i][j][q] is then cohort row
// wm * 64 + i * 16 + lk + 4 q against X row wn * 64 + j * 16 + lr: sixteen cohort scores of ONE X row per j, so a lane carries two
// running doubles per j (8 registers).  The two terms are summed over the partials in ascending p, X's once per workgroup, the cohort's
// once per tile, and reach the epilogue through 2 KB of LDS as in plda_hist_kernel.  Slabs as in cohort_moments_kernel: a row's additions
// -- lane (i, q) order inside a tile, tiles in order, the four lane groups (lk), the two cohort-side waves, then the slabs in
// cohort_moments_final_kernel<double> -- do not depend on N, on the row's place in its tile or on the launch.
constexpr int PCT = 128;

__global__ __launch_bounds__(256, 2) void plda_cohort_moments_kernel(const double* __restrict__ XPsi, int N, const double* __restrict__ C, int M, int D,
                                                                     const double* __restrict__ xpart, long x_stride, const double* __restrict__ cpart,
                                                                     int nparts, double cst, double alpha, long self_off, int tiles_per_slab,
                                                                     double* __restrict__ part) {
  constexpr int WT = PCT / 32;
  __shared__ __attribute__((aligned(16))) double As[PCT * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[PCT * DLD];
  __shared__ double term[2 * PCT];   // [0, PCT): the tile's cohort terms, [PCT, 2 PCT): the workgroup's X terms
  __shared__ double red[PCT][2];
  const dgemm_lanes<WT> at;   // wm: cohort side, wn: X side
  const int tid = threadIdx.x, wm = at.wm, lk = at.lk;
  const int n0 = blockIdx.x * PCT;
  const int tiles_m = (M + PCT - 1) / PCT, t0 = blockIdx.y * tiles_per_slab, t1 = t0 + tiles_per_slab < tiles_m ? t0 + tiles_per_slab : tiles_m;
  if (tid >= PCT) {   // rows past the end are never written
    double t = 0.0;
    if (n0 + tid - PCT < N) for (int p = 0; p < nparts; ++p) t += xpart[(long)p * x_stride + n0 + tid - PCT];
    term[tid] = t;    // read after the first tile's barriers
  }
  double s1[WT], s2[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
  for (int t = t0; t < t1; ++t) {
    const int c0 = t * PCT;
    f64x4 acc[WT][WT];
    dgemm_tile<WT, false>(C, XPsi, M, N, D, c0, n0, As, Bs, acc);
    if (tid < PCT) {   // the k loop's barriers lie between the previous tile's last read of `term` and this write
      double tsum = 0.0;   // (summed here, not across the k loop: the kernel sits at its 256 registers)
      if (c0 + tid < M) for (int p = 0; p < nparts; ++p) tsum += cpart[(long)p * M + c0 + tid];
      term[tid] = tsum;
    }
    __syncthreads();
    // (a dropped value enters the sums as an exact zero: the kept values' additions are unchanged by it)
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int ln_ = at.col(j);
      const long drop = self_off >= 0 ? (long)(n0 + ln_) + self_off : -1L;
      const double xt = term[PCT + ln_];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int lm = at.row(i, q), m = c0 + lm;
          double v = alpha * (acc[i][j][q] + xt + term[lm] + cst);   // dgemm_nt_kernel's expression: X is sc_plda_fast's row side
          v = (m < M && (long)m != drop) ? v : 0.0;
          s1[j] += v;
          s2[j] = fma(v, v, s2[j]);
        }
    }
  }
  // the four lane groups hold the four interleaved quarters of a 16-row block, the two wm waves a tile's two 64-row halves
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    s1[j] += __shfl_xor(s1[j], 16);
    s2[j] += __shfl_xor(s2[j], 16);
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
    const int row = at.col(j);
    if (wm == 1 && lk == 0) { red[row][0] = s1[j]; red[row][1] = s2[j]; }
  }
  __syncthreads();
  if (wm == 0 && lk == 0) {
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int row = at.col(j), n = n0 + row;
      if (n >= N) continue;
      double* o = part + ((long)blockIdx.y * N + n) * 2;
      o[0] = s1[j] + red[row][0];
      o[1] = s2[j] + red[row][1];
    }
  }
}

// ---- moments of a score matrix that exists (the Scores-level mirrors) ------------------------------------------------------------
// per row: one workgroup per row, every thread a strided float64 partial, the 256 partials added in thread order
__global__ __launch_bounds__(256) void row_moments_kernel(const float* __restrict__ S, int cols, int skip_diag, float* __restrict__ mean,
                                                          float* __restrict__ stdv) {
  __shared__ double red[2 * 256];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = S + (long)row * cols;
  double s1 = 0.0, s2 = 0.0;
  for (int c = tid; c < cols; c += 256) {
    if (skip_diag && c == row) continue;
    const double v = (double)x[c];
    s1 += v;
    s2 = fma(v, v, s2);
  }
  red[tid] = s1; red[256 + tid] = s2;
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < 256; ++q) { a += red[q]; b += red[256 + q]; }
    const double cnt = (double)(cols - (skip_diag ? 1 : 0));
    const double m = a / cnt, var = b / cnt - m * m;
    mean[row] = (float)m;
    stdv[row] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
}

// per column: 64 columns x 4 row phases per workgroup (coalesced 256-B row segments); a phase sums its rows in order, the four phases
// are added in phase order
__global__ __launch_bounds__(256) void col_moments_kernel(const float* __restrict__ S, int rows, int cols, int skip_diag, float* __restrict__ mean,
                                                          float* __restrict__ stdv) {
  __shared__ double red[4][64][2];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  double s1 = 0.0, s2 = 0.0;
  if (c < cols)
    for (int rr = ph; rr < rows; rr += 4) {
      if (skip_diag && rr == c) continue;
      const double v = (double)S[(long)rr * cols + c];
      s1 += v;
      s2 = fma(v, v, s2);
    }
  red[ph][threadIdx.x & 63][0] = s1; red[ph][threadIdx.x & 63][1] = s2;
  __syncthreads();
  if (ph == 0 && c < cols) {
    double a = 0.0, b = 0.0;
    for (int p = 0; p < 4; ++p) { a += red[p][threadIdx.x][0]; b += red[p][threadIdx.x][1]; }
    const double cnt = (double)(rows - (skip_diag ? 1 : 0));
    const double m = a / cnt, var = b / cnt - m * m;
    mean[c] = (float)m;
    stdv[c] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
}

// ---- adaptive s-norm support (sidekit/score_normalization.py:120-140) -----------------------------------------
// Mean and unbiased std of the k largest values of every row: an exact radix select on the order-preserving
// integer image of the floats (four 8-bit passes narrow the k-th largest key), then one pass for the mean and one for the
// variance centred on it.  Ties at the threshold contribute exactly the copies torch.topk would keep, so the statistics
// equal those of any valid top-k.
// sc_topk_stats_f64 is the same kernel at double: eight 8-bit passes over the 64-bit image.
__device__ inline unsigned fkey(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // larger float <=> larger key
}
__device__ inline unsigned long long fkey(double f) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, f);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
template <typename T> struct key_of;
template <> struct key_of<float> { typedef unsigned type; };
template <> struct key_of<double> { typedef unsigned long long type; };

template <typename T>
__global__ __launch_bounds__(256) void topk_stats_kernel(const T* __restrict__ x, int ncols, int k, T* __restrict__ mean,
                                                         T* __restrict__ stdv) {
  typedef typename key_of<T>::type K;
  __shared__ unsigned hist[256];
  __shared__ K s_prefix;
  __shared__ unsigned s_remaining;
  __shared__ double red[2 * 256];
  const T* row = x + (size_t)blockIdx.x * ncols;
  const int tid = threadIdx.x;
  K prefix = 0, mask = 0;
  unsigned remaining = (unsigned)k;   // how many of the still-undecided keys belong to the top-k
  for (int shift = 8 * (int)sizeof(K) - 8; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < ncols; i += 256) {
      const K key = fkey(row[i]);
      if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned acc = 0;
      int b = 255;
      for (; b > 0; --b) {
        if (acc + hist[b] >= remaining) break;
        acc += hist[b];
      }
      s_prefix = prefix | ((K)b << shift);
      s_remaining = remaining - acc;
    }
    __syncthreads();
    prefix = s_prefix;
    remaining = s_remaining;
    mask |= (K)255u << shift;
    __syncthreads();
  }
  // prefix == key of the k-th largest value; `remaining` copies of it are inside the top-k.  The mean first: the values above the
  // threshold as 256 strided partials added in thread order, then the copies of the threshold.
  double s1 = 0.0;
  T tval = 0;
  for (int i = tid; i < ncols; i += 256) {
    const T v = row[i];
    const K key = fkey(v);
    if (key > prefix) s1 += (double)v;
    if (key == prefix) tval = v;
  }
  red[tid] = s1;
  __shared__ T s_tval;
  __shared__ double s_mean;
  if (fkey(tval) == prefix) s_tval = tval;   // every writer holds the same value
  __syncthreads();
  double tv = 0.0;
  if (tid == 0) {
    double a = 0.0;
    for (int q = 0; q < 256; ++q) a += red[q];
    tv = (double)s_tval;
    a += tv * (double)remaining;
    s_mean = a / (double)k;
    mean[blockIdx.x] = (T)s_mean;
  }
  __syncthreads();
  // The variance CENTRED on that mean, in a second pass over the same keys: sum (v - m)^2 has no cancellation, where the one-pass
  // (sum v^2 - k m^2) / (k - 1) lost every digit of a double std once mean^2 / var reached 1 / eps (scores of -600 +- 1: 3e-8 relative).
  const double m = s_mean;
  double s2 = 0.0;
  for (int i = tid; i < ncols; i += 256) {
    const T v = row[i];
    if (fkey(v) > prefix) { const double d = (double)v - m; s2 += d * d; }
  }
  red[256 + tid] = s2;
  __syncthreads();
  if (tid == 0) {
    double b = 0.0;
    for (int q = 0; q < 256; ++q) b += red[256 + q];
    const double d = tv - m;
    b += d * d * (double)remaining;
    stdv[blockIdx.x] = (T)sqrt(b / (double)(k - 1));
  }
}

// S[i][j] <- (S[i][j] - me[i]) / se[i] (NA_ENROL: z-norm), (S[i][j] - mt[j]) / st[j] (NA_TEST: t-norm), or half the one plus half the
// other (NA_BOTH: s-norm); a pair a mode does not use is never read
enum { NA_ENROL = 1, NA_TEST = 2, NA_BOTH = 3 };
template <int MODE, typename T>
__global__ void norm_apply_kernel(T* __restrict__ S, int ne, int nt, const T* __restrict__ me, const T* __restrict__ se,
                                  const T* __restrict__ mt, const T* __restrict__ st) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)ne * nt) return;
  const int r = (int)(i / nt), c = (int)(i % nt);
  const T v = S[i];
  if constexpr (MODE == NA_ENROL) S[i] = (v - me[r]) / se[r];
  if constexpr (MODE == NA_TEST) S[i] = (v - mt[c]) / st[c];
  if constexpr (MODE == NA_BOTH) S[i] = (T)0.5 * ((v - me[r]) / se[r]) + (T)0.5 * ((v - mt[c]) / st[c]);
}

template <int MODE, typename T>
static int launch_norm_apply(T* d_S, int32_t Ne, int32_t Nt, const T* d_mean_e, const T* d_std_e, const T* d_mean_t, const T* d_std_t,
                             void* stream) {
  hipLaunchKernelGGL((norm_apply_kernel<MODE, T>), dim3((unsigned)(((long)Ne * Nt + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_S, Ne, Nt,
                     d_mean_e, d_std_e, d_mean_t, d_std_t);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_cohort_moments(const float* d_X, int32_t N, const float* d_C, int32_t M, int32_t D, const float* d_col_shift, const float* d_col_scale,
                      int32_t self_offset, float* d_mean, float* d_std, void* stream) {
  SK_CHECK(N >= 0 && M > 0 && D > 0 && D % 4 == 0, SK_EARG, "sc_cohort_moments: need N >= 0, M > 0 and D a positive multiple of 4 (N=%d, M=%d, D=%d)", N, M, D);
  SK_CHECK((d_col_shift == nullptr) == (d_col_scale == nullptr), SK_EARG, "sc_cohort_moments: col_shift and col_scale come together or not at all");
  SK_CHECK(!(M == 1 && self_offset == 0 && N > 0), SK_EARG, "sc_cohort_moments: row 0 keeps no pair (M = 1 and self_offset = 0)");
  if (N == 0) return SK_OK;
  SK_CHECK(d_X && d_C && d_mean && d_std, SK_EARG, "sc_cohort_moments: null pointer");
  SK_CHECK(aligned16(d_X, d_C), SK_EARG, "sc_cohort_moments: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // the slab size is a function of M alone (at most 64 slabs, at least two cohort tiles each): N = 1000 against M = 20 000 is
  // 8 row tiles x 53 slabs of workgroups, and a row's summation order is the same whatever N it arrives with
  const int tiles_m = cdiv(M, CT), per = tiles_m > 128 ? cdiv(tiles_m, 64) : 2, slabs = cdiv(tiles_m, per);
  constexpr int ROWS = 32768;   // rows per launch: bounds the partials at slabs x 32768 x 16 B (32 MB at 64 slabs)
  const int rows_max = N < ROWS ? N : ROWS;
  void* ws = nullptr;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until every launch is enqueued (see plda_workspace_locked)
  SK_TRY(plda_workspace_locked(st, (size_t)slabs * rows_max * 16, &ws));
  for (int r0 = 0; r0 < N; r0 += ROWS) {
    const int n = N - r0 < ROWS ? N - r0 : ROWS;
    const long self_off = self_offset >= 0 ? (long)self_offset + r0 : -1L;
    const float* x = d_X + (long)r0 * D;
    const dim3 grid(cdiv(n, CT), slabs);
    if (d_col_shift) hipLaunchKernelGGL(cohort_moments_kernel<true>, grid, dim3(256), 0, st, x, n, d_C, M, D, d_col_shift, d_col_scale, self_off, per, (double*)ws);
    else hipLaunchKernelGGL(cohort_moments_kernel<false>, grid, dim3(256), 0, st, x, n, d_C, M, D, d_col_shift, d_col_scale, self_off, per, (double*)ws);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cohort_moments_final_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const double*)ws, n, slabs, M, self_off, d_mean + r0, d_std + r0);
    SK_HIP(hipGetLastError());
  }
  return SK_OK;
}

int sc_plda_cohort_moments(const double* d_X, int32_t N, const double* d_C, int32_t M, int32_t D, const double* d_Phi, const double* d_Psi, double cst,
                           double scaling, int32_t self_offset, double* d_mean, double* d_std, void* stream) {
  SK_CHECK(N >= 0 && M > 0 && D > 0, SK_EARG, "sc_plda_cohort_moments: need N >= 0, M > 0 and D > 0 (N=%d, M=%d, D=%d)", N, M, D);
  SK_CHECK(!(M == 1 && self_offset == 0 && N > 0), SK_EARG, "sc_plda_cohort_moments: row 0 keeps no pair (M = 1 and self_offset = 0)");
  if (N == 0) return SK_OK;
  SK_CHECK(d_X && d_C && d_Phi && d_Psi && d_mean && d_std, SK_EARG, "sc_plda_cohort_moments: null pointer");
  hipStream_t st = (hipStream_t)stream;
  // slabs as in sc_cohort_moments: a function of M alone (at most 64, at least two cohort tiles each)
  const int tiles_m = cdiv(M, PCT), per = tiles_m > 128 ? cdiv(tiles_m, 64) : 2, slabs = cdiv(tiles_m, per);
  constexpr int ROWS = 32768;   // rows per launch: bounds the partials at slabs x 32768 x 16 B (32 MB at 64 slabs)
  const int rows_max = N < ROWS ? N : ROWS;
  PldaPrep w;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until every launch is enqueued (see plda_workspace_locked)
  // ONE workspace request: X . Psi, the quadratic-form partials of X (as E) and of the cohort (as T), and the moment partials
  SK_TRY(plda_prep_locked(d_X, N, d_C, M, D, d_Phi, d_Psi, st, &w, (size_t)slabs * rows_max * 2));
  for (int r0 = 0; r0 < N; r0 += ROWS) {
    const int n = N - r0 < ROWS ? N - r0 : ROWS;
    const long self_off = self_offset >= 0 ? (long)self_offset + r0 : -1L;
    hipLaunchKernelGGL(plda_cohort_moments_kernel, dim3(cdiv(n, PCT), slabs), dim3(256), 0, st, w.epsi + (long)r0 * D, n, d_C, M, D, w.qe + r0, (long)N,
                       w.qt, w.nparts, cst, scaling, self_off, per, w.extra);
    SK_HIP(hipGetLastError());
    hipLaunchKernelGGL(cohort_moments_final_kernel<double>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const double*)w.extra, n, slabs, M, self_off,
                       d_mean + r0, d_std + r0);
    SK_HIP(hipGetLastError());
  }
  return SK_OK;
}

int sc_matrix_moments(const float* d_S, int32_t rows, int32_t cols, int32_t axis, int32_t skip_diag, float* d_mean, float* d_std, void* stream) {
  SK_CHECK(d_S && d_mean && d_std && rows > 0 && cols > 0 && (axis == 0 || axis == 1), SK_EARG, "sc_matrix_moments: bad arguments (axis is 0 or 1)");
  SK_CHECK(!skip_diag || (rows == cols && rows > 1), SK_EARG, "sc_matrix_moments: skip_diag needs a square matrix of at least 2 x 2 (%d x %d)", rows, cols);
  hipStream_t st = (hipStream_t)stream;
  if (axis == 1) hipLaunchKernelGGL(row_moments_kernel, dim3(rows), dim3(256), 0, st, d_S, cols, skip_diag ? 1 : 0, d_mean, d_std);
  else hipLaunchKernelGGL(col_moments_kernel, dim3(cdiv(cols, 64)), dim3(256), 0, st, d_S, rows, cols, skip_diag ? 1 : 0, d_mean, d_std);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_norm_apply(float* d_S, int32_t Ne, int32_t Nt, const float* d_mean_e, const float* d_std_e, const float* d_mean_t, const float* d_std_t,
                  void* stream) {
  const bool e = d_mean_e && d_std_e, t = d_mean_t && d_std_t;
  SK_CHECK(d_S && Ne > 0 && Nt > 0 && (e || t), SK_EARG, "sc_norm_apply: need the matrix and at least one (mean, std) pair");
  SK_CHECK((d_mean_e == nullptr) == (d_std_e == nullptr) && (d_mean_t == nullptr) == (d_std_t == nullptr), SK_EARG,
           "sc_norm_apply: a mean and its std come together");
  if (e && t) return launch_norm_apply<NA_BOTH>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);   // sc_snorm_apply's kernel
  if (e) return launch_norm_apply<NA_ENROL>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
  return launch_norm_apply<NA_TEST>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
}

int sc_topk_stats(const float* d_scores, int32_t n_rows, int32_t n_cols, int32_t k, float* d_mean, float* d_std, void* stream) {
  SK_CHECK(d_scores && d_mean && d_std && n_rows > 0 && k > 1 && k <= n_cols, SK_EARG, "sc_topk_stats: need 1 < k <= n_cols (k=%d, n_cols=%d)", k, n_cols);
  hipLaunchKernelGGL(topk_stats_kernel<float>, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, d_scores, n_cols, k, d_mean, d_std);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_norm_apply_f64(double* d_S, int32_t Ne, int32_t Nt, const double* d_mean_e, const double* d_std_e, const double* d_mean_t,
                      const double* d_std_t, void* stream) {
  const bool e = d_mean_e && d_std_e, t = d_mean_t && d_std_t;
  SK_CHECK(d_S && Ne > 0 && Nt > 0 && (e || t), SK_EARG, "sc_norm_apply_f64: need the matrix and at least one (mean, std) pair");
  SK_CHECK((d_mean_e == nullptr) == (d_std_e == nullptr) && (d_mean_t == nullptr) == (d_std_t == nullptr), SK_EARG,
           "sc_norm_apply_f64: a mean and its std come together");
  if (e && t) return launch_norm_apply<NA_BOTH>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
  if (e) return launch_norm_apply<NA_ENROL>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
  return launch_norm_apply<NA_TEST>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
}

int sc_topk_stats_f64(const double* d_scores, int32_t n_rows, int32_t n_cols, int32_t k, double* d_mean, double* d_std, void* stream) {
  SK_CHECK(d_scores && d_mean && d_std && n_rows > 0 && k > 1 && k <= n_cols, SK_EARG, "sc_topk_stats_f64: need 1 < k <= n_cols (k=%d, n_cols=%d)", k, n_cols);
  hipLaunchKernelGGL(topk_stats_kernel<double>, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, d_scores, n_cols, k, d_mean, d_std);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_snorm_apply(float* d_S, int32_t Ne, int32_t Nt, const float* d_mean_e, const float* d_std_e, const float* d_mean_t,
                   const float* d_std_t, void* stream) {
  SK_CHECK(d_S && d_mean_e && d_std_e && d_mean_t && d_std_t && Ne > 0 && Nt > 0, SK_EARG, "sc_snorm_apply: bad arguments");
  return launch_norm_apply<NA_BOTH>(d_S, Ne, Nt, d_mean_e, d_std_e, d_mean_t, d_std_t, stream);
}

}  // extern "C"
