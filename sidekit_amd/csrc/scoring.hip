// Trial-matrix scoring: cosine (sidekit/iv_scoring.py:98-109), fast PLDA (:448-462) and the
// per-trial cosine of sidekit/bin/compute_spk_cosine.py:18-26.
//
// This file holds the scores and their histograms; everything that normalises a score is score_norm.hip.
// cosine is one f32 MFMA GEMM over the already normalised rows.  PLDA keeps the reference's
// float64 arithmetic end to end: the 256x256 algebra (Phi, Psi, constant) stays on the host; here ONE
// launch forms E.Psi and the two quadratic forms, and the N^2 part runs as an f64 MFMA GEMM
// (C = A . B^T, v_mfma_f64_16x16x4_f64) whose epilogue adds the quadratic terms and the constant, so
// the (Ne x Nt) matrix is written exactly once.  For
// trial sets too large to materialise, sc_cosine_hist (cosine) and sc_plda_hist (PLDA; f64 tile of dgemm_tile.h)
// count target / non-target scores into histograms straight from the accumulators (sc_cosine_hist_norm / sc_plda_hist_norm: cohort-normalised first); the entry points share one host prologue (hist_args_ok,
// hist_begin).  The two kernels keep their own k-tile step and LDS histogram code: through shared helpers both measured slower.
#include <cmath>
#include <map>
#include <mutex>
#include <utility>

#include "../../include/sidekit_amd.h"
#include "dgemm_tile.h"
#include "kernels.h"

namespace sk {

// C[m][n] = alpha * (sum_k A[m][k] B[n][k] + rowterm(m) + colterm(n) + cst); the two terms arrive as `nparts` partial sums each
// (rowterm(m) = sum_p rowpart[p * M + m], fixed order), which is how plda_prep_kernel leaves the quadratic forms.
template <int WT>
__global__ __launch_bounds__(256, WT == 4 ? 2 : 4) void dgemm_nt_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                          int M, int N, int K, const double* __restrict__ rowpart,
                                                          const double* __restrict__ colpart, int nparts, double cst, double alpha) {
  constexpr int T = 32 * WT;
  __shared__ __attribute__((aligned(16))) double As[T * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[T * DLD];
  // dgemm_lanes' map, written out: through the struct, WT = 4 takes one register more
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.y * T, n0 = blockIdx.x * T;
  f64x4 acc[WT][WT];
  dgemm_tile<WT, false>(A, B, M, N, K, m0, n0, As, Bs, acc);
  double ct[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const int n = n0 + wn * 16 * WT + j * 16 + lr;
    double t = 0.0;
    if (n < N) for (int p = 0; p < nparts; ++p) t += colpart[(long)p * N + n];
    ct[j] = t;
  }
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + wm * 16 * WT + i * 16 + lk + 4 * q;
      if (m >= M) continue;
      double rt = 0.0;
      for (int p = 0; p < nparts; ++p) rt += rowpart[(long)p * M + m];
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + wn * 16 * WT + j * 16 + lr;
        if (n < N) C[(long)m * N + n] = alpha * (acc[i][j][q] + rt + ct[j] + cst);
      }
    }
}

// Everything fast PLDA needs before its N^2 product, in ONE launch (sidekit/iv_scoring.py:449-458):
//   qpart_e[p][i] = 0.5 * sum_{n in column tile p} (E Phi)[i][n] E[i][n]      -> model_part = sum_p qpart_e[p]   (:449)
//   qpart_t[p][j] = the same for T                                          -> seg_part                        (:450)
//   EPsi = E . Psi                                                           (left factor of :458)
// Grid: x = column tile of [Phi | Psi] (D/64 + D/64), y = row tile of [E ; T]; the (T rows, Psi columns) workgroups have nothing to
// do.  The products X Phi are never written: each workgroup folds its 64 x 64 tile with the matching slice of X straight from the
// accumulators (16-lane reduction, then the two column waves through LDS; deterministic).
__global__ __launch_bounds__(256) void plda_prep_kernel(const double* __restrict__ E, int Ne, const double* __restrict__ Tm, int Nt, int D,
                                                        const double* __restrict__ Phi, const double* __restrict__ Psi,
                                                        double* __restrict__ qpart_e, double* __restrict__ qpart_t, double* __restrict__ EPsi) {
  constexpr int WT = 2, T = 64;
  __shared__ __attribute__((aligned(16))) double As[T * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[T * DLD];
  __shared__ double red[2][T];
  const int ctiles = (D + T - 1) / T, etiles = (Ne + T - 1) / T;
  const bool psi = (int)blockIdx.x >= ctiles, is_t = (int)blockIdx.y >= etiles;
  if (psi && is_t) return;
  const double* X = is_t ? Tm : E;
  const int M = is_t ? Nt : Ne;
  const int m0 = (is_t ? (int)blockIdx.y - etiles : (int)blockIdx.y) * T, p = psi ? (int)blockIdx.x - ctiles : (int)blockIdx.x, n0 = p * T;
  const dgemm_lanes<WT> at;
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true>(X, psi ? Psi : Phi, M, D, D, m0, n0, As, Bs, acc);
  if (psi) {
    dgemm_store_tile(acc, at, EPsi, D, m0, n0, M, D);
    return;
  }
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = at.row(i, q), m = m0 + r;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + at.col(j);
        if (m < M && n < D) s = fma(acc[i][j][q], X[(long)m * D + n], s);
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);   // the 16 lanes that share lk hold this row's 16 columns of each tile
      if (at.lr == 0) red[at.wn][r] = s;
    }
  __syncthreads();
  if (threadIdx.x < T && m0 + (int)threadIdx.x < M)
    (is_t ? qpart_t : qpart_e)[(long)p * M + m0 + threadIdx.x] = 0.5 * (red[0][threadIdx.x] + red[1][threadIdx.x]);
}

// ---- all-pairs cosine scoring WITHOUT the score matrix (100k x 100k trials are 40 GB of float32) ---------------------
// Persistent workgroups walk the 256 x 256 tiles of E . T^T (f32 MFMA, the arithmetic of sc_cosine: sgemm_wave_step<2> of sgemm_tile.h written out), classify every score as
// target / non-target from the two label vectors and count it into a private LDS histogram pair; the histograms are added to
// the global 64-bit counters once, at the end.  EER / ROCCH then come from the counts (bosaris.detplot.eer_from_histograms).
constexpr int HB = 8192;   // bins per histogram: 2 x 32 KB of LDS per workgroup, one persistent workgroup per CU

// Tile: 256 x 256 per 1024-thread workgroup, sixteen waves of 64 x 64 (2 x 2 accumulator tiles each), k-tiles of 32 staged through
// LDS with the next k-tile's operands prefetched into registers.  The 64 KB of histograms allow only ONE workgroup per CU, so the
// latency hiding has to come from inside it: four waves per SIMD put 16 k matrix-pipe cycles between a prefetch and its use
// (64 x 64 tiles with load-then-compute kept the pipes 26 % busy, 128 x 128 with four waves 33 %).
constexpr int HT = 256, HLD = 36, HTHREADS = 1024;

// NORM: what stands between an accumulator and its bin.  HN_NONE: nothing (sc_cosine_hist).  The others (sc_cosine_hist_norm) apply a
// cohort normalisation with per-row statistics, in the expressions of the kernels that normalise a score matrix that exists
// (norm_apply_kernel<NA_ENROL>, <NA_TEST>, <NA_BOTH> of score_norm.hip): the same accumulator through the same IEEE operations (the
// library is built with -ffp-contract=off) is the same bits, so the counts are those of sc_cosine + sc_norm_apply + binning.  A tile's
// 256 enrolment-side and 256 test-side (mean, std) go through 4 KB of LDS, once per tile; HN_NONE declares none of it.
// Scores that are not finite.  The rule of plda_hist_kernel (a NaN in no bin, a raw +-inf in an end bin, a normalised score that is not
// finite in no bin) is NOT this kernel's: it converts floorf(x) to int before it clamps, which C++ leaves undefined for a NaN, an infinity
// or a value past the int range.  The hardware conversion saturates and turns a NaN into 0, so +-inf land in the end bins and a NaN in
// bin 0, normalised or not (tests/test_gpu_hist_bins.py pins exactly that).  Testing x and clamping it in float first was measured on the
// benchmark shapes and left out: +0.29 ms on 23.87 ms at N = 65 536 with one comparison per score, +0.83 ms with the PLDA kernel's three,
// against a run-to-run spread of the parent's medians of 0.02 - 0.09 ms (profiles/hist_bins_bench.json): the epilogue is not hidden
// behind the matrix cores.
enum { HN_NONE = 0, HN_ENROL = 1, HN_TEST = 2, HN_BOTH = 3 };
struct HistNorm { const float *me, *se, *mt, *st; };   // Ne, Ne, Nt, Nt entries; a side a mode does not use is never read

template <int NORM>
__global__ __launch_bounds__(HTHREADS) void cosine_hist_kernel(const float* __restrict__ E, int Ne, const float* __restrict__ T, int Nt, int D,
                                                               const int* __restrict__ le, const int* __restrict__ lt, int self_offset,
                                                               float lo, float inv_width, unsigned long long* __restrict__ hist_tar,
                                                               unsigned long long* __restrict__ hist_non, HistNorm nrm) {
  __shared__ unsigned hist[2 * HB];
  __shared__ __attribute__((aligned(16))) float Es[HT * HLD];
  __shared__ __attribute__((aligned(16))) float Ts[HT * HLD];
  float* stat = nullptr;   // [0, HT): enrolment means, [HT, 2 HT): test means, then the two stds in the same order
  if constexpr (NORM != HN_NONE) {
    __shared__ float stat_lds[4 * HT];
    stat = stat_lds;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5, wm = wave >> 2, wn = wave & 3;
  for (int i = tid; i < 2 * HB; i += HTHREADS) hist[i] = 0u;
  const long tiles_n = (Nt + HT - 1) / HT, ntiles = (long)((Ne + HT - 1) / HT) * tiles_n;
  const int srow = tid >> 3, sk4 = (tid & 7) * 4;   // 128 rows x 8 chunks per pass, two passes per operand
  const int nk = (D + 31) / 32;
  auto flush = [&]() {   // LDS counts -> the global 64-bit counters
    for (int i = tid; i < 2 * HB; i += HTHREADS) {
      const unsigned c = hist[i];
      if (c) atomicAdd((i < HB ? hist_tar : hist_non) + (i & (HB - 1)), (unsigned long long)c);
      hist[i] = 0u;
    }
  };
  int since_flush = 0;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // a tile adds at most 65 536 counts to one 32-bit LDS bin: flush before 2^15 tiles could wrap it (a few million x a few
    // million trials per workgroup get there in the central non-target bins)
    if (++since_flush == (1 << 15)) { __syncthreads(); flush(); since_flush = 0; __syncthreads(); }
    const int m0 = (int)(tile / tiles_n) * HT, n0 = (int)(tile % tiles_n) * HT;
    float4 re[2], rt[2];
    auto fetch = [&](int k0) {
      const int k = k0 + sk4;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int row = srow + q * 128;
        re[q] = (m0 + row < Ne && k < D) ? *reinterpret_cast<const float4*>(E + (long)(m0 + row) * D + k) : z;
        rt[q] = (n0 + row < Nt && k < D) ? *reinterpret_cast<const float4*>(T + (long)(n0 + row) * D + k) : z;
      }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    fetch(0);
    float smean = 0.f, sstd = 1.f;   // thread t < 256: enrolment row m0 + t; 256 <= t < 512: test row n0 + t - 256 (rows past the end are never binned)
    if constexpr (NORM != HN_NONE) {
      if (tid < HT) {
        if ((NORM & HN_ENROL) && m0 + tid < Ne) { smean = nrm.me[m0 + tid]; sstd = nrm.se[m0 + tid]; }
      } else if (tid < 2 * HT) {
        if ((NORM & HN_TEST) && n0 + tid - HT < Nt) { smean = nrm.mt[n0 + tid - HT]; sstd = nrm.st[n0 + tid - HT]; }
      }
    }
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();            // every wave is done reading the previous k-tile
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        *reinterpret_cast<float4*>(&Es[(srow + q * 128) * HLD + sk4]) = re[q];
        *reinterpret_cast<float4*>(&Ts[(srow + q * 128) * HLD + sk4]) = rt[q];
      }
      __syncthreads();
      if (kt + 1 < nk) fetch((kt + 1) * 32);
#pragma unroll
      for (int kk = 0; kk < 32; kk += 8) {
        float4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const float4*>(&Es[(wm * 64 + i * 32 + r) * HLD + kk + 4 * h]);
          b[i] = *reinterpret_cast<const float4*>(&Ts[(wn * 64 + i * 32 + r) * HLD + kk + 4 * h]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
      }
    }
    if constexpr (NORM != HN_NONE) {   // the k loop's barriers lie between the previous tile's last read of `stat` and this write
      if (tid < 2 * HT) { stat[tid] = smean; stat[2 * HT + tid] = sstd; }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + r;
      if (n >= Nt) continue;
      const int ln = lt[n];
      float mtn = 0.f, stn = 1.f;
      if constexpr ((NORM & HN_TEST) != 0) { mtn = stat[HT + wn * 64 + j * 32 + r]; stn = stat[3 * HT + wn * 64 + j * 32 + r]; }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int lm = wm * 64 + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, m = m0 + lm;
          if (m >= Ne || (self_offset >= 0 && m + self_offset == n)) continue;
          float v = acc[i][j][q];
          if constexpr (NORM == HN_ENROL) v = (v - stat[lm]) / stat[2 * HT + lm];
          if constexpr (NORM == HN_TEST) v = (v - mtn) / stn;
          if constexpr (NORM == HN_BOTH) v = 0.5f * ((v - stat[lm]) / stat[2 * HT + lm]) + 0.5f * ((v - mtn) / stn);
          int bin = (int)floorf((v - lo) * inv_width);
          bin = bin < 0 ? 0 : (bin >= HB ? HB - 1 : bin);
          atomicAdd(&hist[(le[m] == ln ? 0 : HB) + bin], 1u);
        }
    }
  }
  __syncthreads();
  flush();
}

// ---- all-pairs PLDA scoring WITHOUT the score matrix (100k x 100k float64 log-likelihood ratios are 80 GB) ------------------------
// The scores of sidekit/iv_scoring.py:448-462 as sc_plda_fast computes them, counted instead of stored: the counts are those of
// sc_plda_fast + binning.  Persistent workgroups walk the 128 x 128 tiles of (E Psi) . T^T with dgemm_tile<4, false>, the tile of
// dgemm_nt_kernel<4>; an accumulator element is the same chain of v_mfma_f64_16x16x4_f64 over ascending k whatever the tile edge, so
// dgemm_nt_kernel<2>'s value for the pair is the same double.  The epilogue is dgemm_nt_kernel's expression,
// alpha * (acc + rowterm + colterm + cst) from left to right (the library is built with -ffp-contract=off), with the two terms summed
// over the partials in ascending p -- once per tile: thread t < 128 sums row m0 + t's, thread 128 + t column n0 + t's, during the k
// loop, and 2 KB of LDS hand them to the epilogue.  The bin is taken in float64 and clamped BEFORE the conversion to int, so +-inf
// lands in an end bin; a NaN score is counted nowhere and the caller sees it missing from the total.  Histograms, flush and launch
// follow cosine_hist_kernel: 2 x 32 KB of 32-bit LDS counters beside the 34 KB of operand tiles, so one workgroup (four waves) per CU.
//
// NORM (sc_plda_hist_norm), as in cosine_hist_kernel: HN_NONE is sc_plda_hist's kernel; the others put the score through the float64
// expression of norm_apply_kernel<NA_ENROL | NA_TEST | NA_BOTH, double> (score_norm.hip) between the epilogue and the bin, so the counts
// are those of sc_plda_fast + sc_norm_apply_f64 + binning.  A tile's 128 enrolment-side and 128 test-side (mean, std) go through 4 KB of
// LDS once per tile (256 threads: one row each); HN_NONE declares none of it and reads no field of `nrm`.
constexpr int PT = 128, PTHREADS = 256;
struct PldaHistNorm { const double *me, *se, *mt, *st; };   // Ne, Ne, Nt, Nt entries; a side a mode does not use is never read

template <int NORM>
__global__ __launch_bounds__(PTHREADS) void plda_hist_kernel(const double* __restrict__ EPsi, int Ne, const double* __restrict__ T, int Nt, int D,
                                                             const double* __restrict__ rowpart, const double* __restrict__ colpart, int nparts,
                                                             double cst, double alpha, const int* __restrict__ le, const int* __restrict__ lt,
                                                             int self_offset, double lo, double inv_width,
                                                             unsigned long long* __restrict__ hist_tar, unsigned long long* __restrict__ hist_non,
                                                             PldaHistNorm nrm) {
  constexpr int WT = PT / 32;
  __shared__ unsigned hist[2 * HB];
  __shared__ __attribute__((aligned(16))) double As[PT * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[PT * DLD];
  __shared__ double term[2 * PT];   // [0, PT): the tile's row terms, [PT, 2 PT): its column terms
  double* stat = nullptr;           // [0, PT): enrolment means, [PT, 2 PT): test means, then the two stds in the same order
  if constexpr (NORM != HN_NONE) {
    __shared__ double stat_lds[4 * PT];
    stat = stat_lds;
  }
  const dgemm_lanes<WT> at;
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * HB; i += PTHREADS) hist[i] = 0u;
  const long tiles_n = (Nt + PT - 1) / PT, ntiles = (long)((Ne + PT - 1) / PT) * tiles_n;
  auto flush = [&]() {   // LDS counts -> the global 64-bit counters
    for (int i = tid; i < 2 * HB; i += PTHREADS) {
      const unsigned c = hist[i];
      if (c) atomicAdd((i < HB ? hist_tar : hist_non) + (i & (HB - 1)), (unsigned long long)c);
      hist[i] = 0u;
    }
  };
  int since_flush = 0;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // a tile adds at most 128 x 128 = 2^14 counts to one 32-bit LDS bin: flushing before the 2^17-th tile keeps a bin below 2^31
    if (++since_flush == (1 << 17)) { __syncthreads(); flush(); since_flush = 0; __syncthreads(); }
    const int m0 = (int)(tile / tiles_n) * PT, n0 = (int)(tile % tiles_n) * PT;
    double tsum = 0.0;   // rows and columns past the end are never binned
    if (tid < PT) {
      if (m0 + tid < Ne) for (int p = 0; p < nparts; ++p) tsum += rowpart[(long)p * Ne + m0 + tid];
    } else if (n0 + tid - PT < Nt) {
      for (int p = 0; p < nparts; ++p) tsum += colpart[(long)p * Nt + n0 + tid - PT];
    }
    double smean = 0.0, sstd = 1.0;   // thread t < 128: enrolment row m0 + t; else test row n0 + t - 128 (rows past the end are never binned)
    if constexpr (NORM != HN_NONE) {
      if (tid < PT) {
        if ((NORM & HN_ENROL) && m0 + tid < Ne) { smean = nrm.me[m0 + tid]; sstd = nrm.se[m0 + tid]; }
      } else if ((NORM & HN_TEST) && n0 + tid - PT < Nt) {
        smean = nrm.mt[n0 + tid - PT]; sstd = nrm.st[n0 + tid - PT];
      }
    }
    f64x4 acc[WT][WT];
    dgemm_tile<WT, false>(EPsi, T, Ne, Nt, D, m0, n0, As, Bs, acc);
    term[tid] = tsum;   // the k loop's barriers lie between the previous tile's last read of `term` and this write
    if constexpr (NORM != HN_NONE) { stat[tid] = smean; stat[2 * PT + tid] = sstd; }   // (and of `stat`)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const int ln_ = at.col(j), n = n0 + ln_;
      if (n >= Nt) continue;
      const int labn = lt[n];
      const double ct = term[PT + ln_];
      double mtn = 0.0, stn = 1.0;
      if constexpr ((NORM & HN_TEST) != 0) { mtn = stat[PT + ln_]; stn = stat[3 * PT + ln_]; }
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int lm = at.row(i, q), m = m0 + lm;
          if (m >= Ne || (self_offset >= 0 && m + self_offset == n)) continue;
          double v = alpha * (acc[i][j][q] + term[lm] + ct + cst);
          if constexpr (NORM == HN_ENROL) v = (v - stat[lm]) / stat[2 * PT + lm];
          if constexpr (NORM == HN_TEST) v = (v - mtn) / stn;
          if constexpr (NORM == HN_BOTH) v = 0.5 * ((v - stat[lm]) / stat[2 * PT + lm]) + 0.5 * ((v - mtn) / stn);
          const double x = (v - lo) * inv_width;
          if constexpr (NORM == HN_NONE) { if (x != x) continue; }
          else { if (!(x - x == 0.0)) continue; }   // a normalised score that is not finite (a zero std: +-inf, or NaN) has no bin
          const int bin = x < 0.0 ? 0 : (x >= (double)HB ? HB - 1 : (int)x);
          atomicAdd(&hist[(le[m] == labn ? 0 : HB) + bin], 1u);
        }
    }
  }
  __syncthreads();
  flush();
}

__global__ void cosine_trials_kernel(const float* __restrict__ E, const float* __restrict__ T, int D, const int* __restrict__ ei,
                                     const int* __restrict__ ti, long n, double* __restrict__ out) {
  const long k = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n) return;
  const float* e = E + (long)ei[k] * D;
  const float* t = T + (long)ti[k] * D;
  double uv = 0, uu = 0, vv = 0;
  for (int d = lane; d < D; d += 64) {
    const double a = e[d], b = t[d];
    uv = fma(a, b, uv); uu = fma(a, a, uu); vv = fma(b, b, vv);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { uv += __shfl_xor(uv, o); uu += __shfl_xor(uu, o); vv += __shfl_xor(vv, o); }
  if (lane == 0) out[k] = uv / (sqrt(uu) * sqrt(vv));  // 1 - scipy.spatial.distance.cosine
}

// ---- workspace of sc_plda_fast and sc_plda_hist (E . Psi (Ne x D) and the partial quadratic forms) and of the PLDA training calls (plda_train.hip), cached per (device, stream) so that a call
// allocates nothing in the steady state (three hipMallocAsync / hipFreeAsync pairs per call were most of a 1000 x 1000 scoring).  A
// stream's calls are ordered, so reuse needs no further synchronisation; growth waits for that stream's earlier calls first.  The
// caller holds g_plda_mu from the lookup until its two kernels are enqueued (with the lock dropped in between, a second host
// thread growing the same stream's entry could free the buffer a first thread was about to launch on).  Entries live until
// sc_release_workspace() (called by the Python shim at interpreter exit and by tests); a stream handle the runtime recycles finds the
// old entry, which is harmless for the same reason reuse is: work on one stream handle is ordered.
struct PldaWs { void* p = nullptr; size_t bytes = 0; };
std::mutex g_plda_mu;
static std::map<std::pair<int, hipStream_t>, PldaWs> g_plda_ws;

int plda_workspace_locked(hipStream_t st, size_t bytes, void** out) {
  int dev = 0;
  SK_HIP(hipGetDevice(&dev));
  PldaWs& w = g_plda_ws[{dev, st}];
  if (bytes > w.bytes) {
    if (w.p) { SK_HIP(hipStreamSynchronize(st)); SK_HIP(hipFree(w.p)); w.p = nullptr; w.bytes = 0; }
    const size_t want = bytes + bytes / 4;
    SK_HIP(hipMalloc(&w.p, want));
    w.bytes = want;
  }
  *out = w.p;
  return SK_OK;
}

// the CU count of the device the stream belongs to (the NULL stream: the current device)
static int stream_cus(hipStream_t st) {
  int dev = 0, cus = 256;
  hipDevice_t sdev;
  if (st && hipStreamGetDevice(st, &sdev) == hipSuccess) dev = (int)sdev;
  else (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus > 0 ? cus : 256;
}

// What sc_plda_fast, sc_plda_hist and sc_plda_cohort_moments share (kernels.h): the stream's workspace cut into E . Psi, the partial
// quadratic forms and what the caller asked for beyond them, and the ONE launch that fills the first three.  The caller holds g_plda_mu,
// and keeps it until its own N^2 kernel is enqueued (see plda_workspace_locked).
int plda_prep_locked(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                     hipStream_t st, PldaPrep* out, size_t extra_doubles) {
  const int ctiles = cdiv(D, 64);
  const size_t n_epsi = ((size_t)Ne * D + 1) & ~(size_t)1, n_qe = (size_t)ctiles * Ne, n_qt = (size_t)ctiles * Nt;
  void* ws = nullptr;
  SK_TRY(plda_workspace_locked(st, (n_epsi + n_qe + n_qt + extra_doubles) * 8, &ws));
  out->epsi = (double*)ws;
  out->qe = out->epsi + n_epsi;
  out->qt = out->qe + n_qe;
  out->extra = out->qt + n_qt;
  out->nparts = ctiles;
  // model_part / seg_part = 0.5 * diag(X Phi X') as per-column-tile partials, and E . Psi   (iv_scoring.py:449-450,458)
  hipLaunchKernelGGL(plda_prep_kernel, dim3(2 * ctiles, cdiv(Ne, 64) + cdiv(Nt, 64)), dim3(256), 0, st, d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, out->qe, out->qt,
                     out->epsi);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

// What the histogram entry points do before their persistent launch: the counters zeroed on the stream, and the grid: one workgroup
// per CU (the caller's LDS budget allows no second one), at most one per tile.
static int hist_begin(uint64_t* d_hist_tar, uint64_t* d_hist_non, long ntiles, hipStream_t st, int* grid) {
  SK_HIP(hipMemsetAsync(d_hist_tar, 0, (size_t)HB * 8, st));
  SK_HIP(hipMemsetAsync(d_hist_non, 0, (size_t)HB * 8, st));
  const int cus = stream_cus(st);
  *grid = (int)(ntiles < (long)cus ? ntiles : (long)cus);
  return SK_OK;
}

// the condition on the arguments every histogram entry point takes: no null pointer, no size that is not positive
static bool hist_args_ok(const void* d_E, const void* d_T, const int32_t* d_labels_e, const int32_t* d_labels_t, const uint64_t* d_hist_tar,
                         const uint64_t* d_hist_non, int32_t Ne, int32_t Nt, int32_t D) {
  return d_E && d_T && d_labels_e && d_labels_t && d_hist_tar && d_hist_non && Ne > 0 && Nt > 0 && D > 0;
}

// the persistent launch of both cosine histogram entry points
template <int NORM>
static int launch_cosine_hist(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e,
                              const int32_t* d_labels_t, int32_t self_offset, HistNorm nrm, float lo, float hi, uint64_t* d_hist_tar,
                              uint64_t* d_hist_non, hipStream_t st) {
  int grid = 0;
  SK_TRY(hist_begin(d_hist_tar, d_hist_non, (long)cdiv(Ne, HT) * cdiv(Nt, HT), st, &grid));   // one workgroup per CU: 64 KB of histograms + 74 KB of operand tiles
  hipLaunchKernelGGL(cosine_hist_kernel<NORM>, dim3(grid), dim3(HTHREADS), 0, st, d_E, Ne, d_T, Nt, D, d_labels_e, d_labels_t, self_offset, lo,
                     (float)HB / (hi - lo), (unsigned long long*)d_hist_tar, (unsigned long long*)d_hist_non, nrm);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

// the preparation and the persistent launch of both PLDA histogram entry points
template <int NORM>
static int launch_plda_hist(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                            double cst, double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, PldaHistNorm nrm,
                            double lo, double hi, uint64_t* d_hist_tar, uint64_t* d_hist_non, hipStream_t st) {
  PldaPrep w;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until everything is enqueued (see plda_workspace_locked)
  SK_TRY(plda_prep_locked(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, st, &w));
  int grid = 0;
  SK_TRY(hist_begin(d_hist_tar, d_hist_non, (long)cdiv(Ne, PT) * cdiv(Nt, PT), st, &grid));   // one workgroup per CU: 64 KB of histograms + 36 KB of tiles and terms (+ 4 KB of statistics)
  hipLaunchKernelGGL(plda_hist_kernel<NORM>, dim3(grid), dim3(PTHREADS), 0, st, w.epsi, Ne, d_T, Nt, D, w.qe, w.qt, w.nparts, cst, scaling, d_labels_e,
                     d_labels_t, self_offset, lo, (double)HB / (hi - lo), (unsigned long long*)d_hist_tar, (unsigned long long*)d_hist_non, nrm);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_cosine(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, float* d_out, void* stream) {
  SK_CHECK(d_E && d_T && d_out && Ne > 0 && Nt > 0 && D > 0 && D % 4 == 0, SK_EARG, "sc_cosine: bad arguments (D must be a multiple of 4)");
  SK_CHECK(aligned16(d_E, d_T), SK_EARG, "sc_cosine: operands must be 16-byte aligned");
  GemmArgs g = gemm_args();
  g.A = d_E; g.lda = D; g.a_rows = Ne; g.W = d_T; g.ldw = D; g.C = d_out; g.ldc = Nt; g.M = Ne; g.N = Nt; g.K = D;
  return launch_gemm(g, (hipStream_t)stream);
}

int sc_plda_fast(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                 double cst, double scaling, double* d_out, void* stream) {
  SK_CHECK(d_E && d_T && d_Phi && d_Psi && d_out && Ne > 0 && Nt > 0 && D > 0, SK_EARG, "sc_plda_fast: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  PldaPrep w;
  std::lock_guard<std::mutex> lock(g_plda_mu);   // held until both launches are enqueued (see plda_workspace_locked)
  // 1) the workspace, E . Psi and the partial quadratic forms
  SK_TRY(plda_prep_locked(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, st, &w));
  // 2) scoremat = (model_part[:, None] + seg_part + cst + (E Psi) T') * scaling   (:458-460)
  const bool big = (long)cdiv(Ne, 128) * cdiv(Nt, 128) >= 512;   // two 128 x 128 workgroups per CU and still two rounds of them
  if (big) hipLaunchKernelGGL(dgemm_nt_kernel<4>, dim3(cdiv(Nt, 128), cdiv(Ne, 128)), dim3(256), 0, st, w.epsi, d_T, d_out, Ne, Nt, D, w.qe, w.qt, w.nparts, cst, scaling);
  else hipLaunchKernelGGL(dgemm_nt_kernel<2>, dim3(cdiv(Nt, 64), cdiv(Ne, 64)), dim3(256), 0, st, w.epsi, d_T, d_out, Ne, Nt, D, w.qe, w.qt, w.nparts, cst, scaling);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_plda_hist(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi, double cst,
                 double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, double lo, double hi, int32_t nbins,
                 uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream) {
  SK_CHECK(hist_args_ok(d_E, d_T, d_labels_e, d_labels_t, d_hist_tar, d_hist_non, Ne, Nt, D) && d_Phi && d_Psi, SK_EARG,
           "sc_plda_hist: bad arguments (a null pointer or a size that is not positive)");
  SK_CHECK(nbins == HB, SK_EARG, "sc_plda_hist: nbins must be %d", HB);
  SK_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, SK_EARG, "sc_plda_hist: lo and hi must be finite and hi > lo");
  return launch_plda_hist<HN_NONE>(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, cst, scaling, d_labels_e, d_labels_t, self_offset,
                                   PldaHistNorm{nullptr, nullptr, nullptr, nullptr}, lo, hi, d_hist_tar, d_hist_non, (hipStream_t)stream);
}

int sc_plda_hist_norm(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi, double cst,
                      double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, const double* d_mean_e,
                      const double* d_std_e, const double* d_mean_t, const double* d_std_t, double lo, double hi, int32_t nbins,
                      uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream) {
  SK_CHECK(hist_args_ok(d_E, d_T, d_labels_e, d_labels_t, d_hist_tar, d_hist_non, Ne, Nt, D) && d_Phi && d_Psi, SK_EARG,
           "sc_plda_hist_norm: bad arguments (a null pointer or a size that is not positive)");
  SK_CHECK(nbins == HB, SK_EARG, "sc_plda_hist_norm: nbins must be %d", HB);
  SK_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, SK_EARG, "sc_plda_hist_norm: lo and hi must be finite and hi > lo");
  const bool e = d_mean_e && d_std_e, t = d_mean_t && d_std_t;   // sc_norm_apply_f64's rules
  SK_CHECK((d_mean_e == nullptr) == (d_std_e == nullptr) && (d_mean_t == nullptr) == (d_std_t == nullptr), SK_EARG,
           "sc_plda_hist_norm: a mean and its std come together");
  SK_CHECK(e || t, SK_EARG, "sc_plda_hist_norm: need at least one (mean, std) pair");
  const PldaHistNorm nrm{d_mean_e, d_std_e, d_mean_t, d_std_t};
  hipStream_t st = (hipStream_t)stream;
  if (e && t) return launch_plda_hist<HN_BOTH>(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, cst, scaling, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
  if (e) return launch_plda_hist<HN_ENROL>(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, cst, scaling, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
  return launch_plda_hist<HN_TEST>(d_E, Ne, d_T, Nt, D, d_Phi, d_Psi, cst, scaling, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
}

int sc_normalize_rows(const float* d_X, int32_t N, int32_t D, float* d_out, void* stream) {
  SK_CHECK(d_X && d_out && N > 0 && D > 0, SK_EARG, "sc_normalize_rows: bad arguments");
  return launch_normalize_rows(d_X, d_out, D, N, 1e-12f, (hipStream_t)stream);
}

int sc_release_workspace(void) {
  std::lock_guard<std::mutex> lock(g_plda_mu);
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (auto& kv : g_plda_ws) {
    if (!kv.second.p) continue;
    if (hipSetDevice(kv.first.first) != hipSuccess) continue;
    (void)hipDeviceSynchronize();
    (void)hipFree(kv.second.p);
  }
  g_plda_ws.clear();
  (void)hipSetDevice(cur);
  return SK_OK;
}

int sc_cosine_hist(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e, const int32_t* d_labels_t,
                   int32_t self_offset, float lo, float hi, int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream) {
  SK_CHECK(hist_args_ok(d_E, d_T, d_labels_e, d_labels_t, d_hist_tar, d_hist_non, Ne, Nt, D) && D % 4 == 0, SK_EARG,
           "sc_cosine_hist: bad arguments (D must be a multiple of 4)");
  SK_CHECK(nbins == HB && hi > lo, SK_EARG, "sc_cosine_hist: nbins must be %d and hi > lo", HB);
  SK_CHECK(aligned16(d_E, d_T), SK_EARG, "sc_cosine_hist: operands must be 16-byte aligned");
  return launch_cosine_hist<HN_NONE>(d_E, Ne, d_T, Nt, D, d_labels_e, d_labels_t, self_offset, HistNorm{nullptr, nullptr, nullptr, nullptr}, lo, hi,
                                     d_hist_tar, d_hist_non, (hipStream_t)stream);
}

int sc_cosine_hist_norm(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e, const int32_t* d_labels_t,
                        int32_t self_offset, const float* d_mean_e, const float* d_std_e, const float* d_mean_t, const float* d_std_t, float lo,
                        float hi, int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream) {
  SK_CHECK(hist_args_ok(d_E, d_T, d_labels_e, d_labels_t, d_hist_tar, d_hist_non, Ne, Nt, D) && D % 4 == 0, SK_EARG,
           "sc_cosine_hist_norm: bad arguments (D must be a multiple of 4)");
  SK_CHECK(nbins == HB && hi > lo, SK_EARG, "sc_cosine_hist_norm: nbins must be %d and hi > lo", HB);
  const bool e = d_mean_e && d_std_e, t = d_mean_t && d_std_t;   // sc_norm_apply's rules
  SK_CHECK((d_mean_e == nullptr) == (d_std_e == nullptr) && (d_mean_t == nullptr) == (d_std_t == nullptr), SK_EARG,
           "sc_cosine_hist_norm: a mean and its std come together");
  SK_CHECK(e || t, SK_EARG, "sc_cosine_hist_norm: need at least one (mean, std) pair");
  SK_CHECK(aligned16(d_E, d_T), SK_EARG, "sc_cosine_hist_norm: operands must be 16-byte aligned");
  const HistNorm nrm{d_mean_e, d_std_e, d_mean_t, d_std_t};
  hipStream_t st = (hipStream_t)stream;
  if (e && t) return launch_cosine_hist<HN_BOTH>(d_E, Ne, d_T, Nt, D, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
  if (e) return launch_cosine_hist<HN_ENROL>(d_E, Ne, d_T, Nt, D, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
  return launch_cosine_hist<HN_TEST>(d_E, Ne, d_T, Nt, D, d_labels_e, d_labels_t, self_offset, nrm, lo, hi, d_hist_tar, d_hist_non, st);
}

int sc_cosine_trials(const float* d_E, const float* d_T, int32_t D, const int32_t* d_enr_idx, const int32_t* d_tst_idx, int64_t n_trials,
                     double* d_out, void* stream) {
  SK_CHECK(d_E && d_T && d_enr_idx && d_tst_idx && d_out && D > 0 && n_trials > 0, SK_EARG, "sc_cosine_trials: bad arguments");
  hipLaunchKernelGGL(cosine_trials_kernel, dim3((unsigned)((n_trials + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_E, d_T, D,
                     d_enr_idx, d_tst_idx, (long)n_trials, d_out);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
