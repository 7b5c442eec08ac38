// Feature post-processing of a stacked ragged batch (sidekit/frontend/normfeat.py, frontend/features.py:133-166): RASTA filtering, the
// delta convolution, per-segment moments and the five normalisations (cms, cmvn, their sliding forms, feature warping).  Four entry
// points (include/sidekit_amd/features.h).  float32 rows in, float64 in registers, one rounding to float32 on store; no atomics, every
// sum in a fixed order.  grid.x is always the segment and every tile, run and pass is counted from the segment's first row, so a
// segment's bits do not depend on the batch around it.
//
// A workgroup is 256 threads on FC = 16 columns.  Where rows are independent (delta, the table modes) thread t takes column t & 15 and
// rows (t >> 4) + 16 i of a tile of FT = 256 rows: a wave reads 4 rows x 64 B.  The windowed modes stage the rows a tile's windows
// touch, at most FT + win - 1 of them, column-major in LDS (column stride = FT + win - 1 rounded up to 2 mod 4 words: the 16 columns of
// a staging store start on the 16 even banks), then thread t owns row t of the tile and walks its window column by column: consecutive
// lanes read consecutive words (ds_read2_b32, two words a lane, conflict-free; rows whose window is clamped read the same word, a broadcast).  Results
// cross a 256 x 17 float tile in LDS so that the store to global memory is 64 B per row again.  At win = SC_FEAT_MAX_WIN that is
// 1258 * 16 * 4 + 256 * 17 * 4 = 97,920 B of the 163,840 B a workgroup may declare; at win = 301 53,120 B (three workgroups per CU).
// The tiles of a segment are dealt to grid.z = FZ workgroups round robin (the entries take no row count, so the grid cannot be sized
// by the longest segment; a workgroup whose first tile lies beyond its segment leaves at once).
#include <cmath>

#include "../../include/sidekit_amd/features.h"
#include "common.h"

namespace sk {

constexpr int FT = SC_FEAT_TILE, FC = SC_FEAT_COLS, FZ = 8;
constexpr int FOUT = FC + 1;              // row stride of the result tile
constexpr int RASTA_RUN = 32, RASTA_LANES = 16, RASTA_PASS = RASTA_RUN * RASTA_LANES;
constexpr double RASTA_POLE = 0.94;

__host__ __device__ inline int feat_stride(int win) {
  const int s = FT + win - 1;
  return (s & 3) == 2 ? s : s + 2;     // FT + win - 1 is even
}
__host__ inline size_t feat_lds_bytes(int win) { return ((size_t)feat_stride(win) * FC + (size_t)FT * FOUT) * 4; }

struct Seg { long r0, n; };
__device__ inline Seg feat_segment(const int64_t* seg_off, int s) {
  long r0 = seg_off[s], r1 = seg_off[s + 1];
  if (r0 < 0) r0 = 0;
  return Seg{r0, r1 > r0 ? r1 - r0 : 0};
}

// ---- RASTA -------------------------------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk.  Lane l = tid >> 4 of 16 owns run l (32 rows) of each pass of 512 rows from row 4 on.  First it
// runs the recurrence from a zero state to get the run's end value e[l]; then the carries follow in run order from the pass's entry
// state, c[0] = carry, c[l + 1] = e[l] + 0.94^32 c[l] (every thread walks the chain of its own column: 16 steps); then the run is
// computed again from c[l] and stored.  A run that is not full has no successor, so 0.94^32 is the only power needed.
// Bounds: rows t < n and columns c < D only; the FIR reads rows t - 4 .. t with t >= 4.
__global__ __launch_bounds__(256) void feat_rasta_kernel(const float* x, long ldx, const int64_t* __restrict__ seg_off, int D, float* y, long ldy) {
  __shared__ double ends[RASTA_LANES][FC];
  const Seg sg = feat_segment(seg_off, blockIdx.x);
  const int tid = threadIdx.x, col = tid & 15, lane = tid >> 4, c = blockIdx.y * FC + col;
  const bool cok = c < D;
  const long n = sg.n;
  if (n == 0) return;
  const float* xs = x + sg.r0 * ldx + c;
  float* ys = y + sg.r0 * ldy + c;
  if (cok && lane < 4 && lane < n) ys[lane * ldy] = 0.f;
  double pw = 1.0;
  for (int i = 0; i < RASTA_RUN; ++i) pw *= RASTA_POLE;
  double carry = 0.0;
  for (long base = 4; base < n; base += RASTA_PASS) {
    const long t0 = base + (long)lane * RASTA_RUN;
    const long t1 = t0 + RASTA_RUN < n ? t0 + RASTA_RUN : n;
    double x4 = 0, x3 = 0, x2 = 0, x1 = 0;
    if (cok && t0 < n) {
      x4 = xs[(t0 - 4) * ldx]; x3 = xs[(t0 - 3) * ldx]; x2 = xs[(t0 - 2) * ldx]; x1 = xs[(t0 - 1) * ldx];
    }
    double e = 0.0;
    if (cok) {
      double a4 = x4, a3 = x3, a2 = x2, a1 = x1;
      for (long t = t0; t < t1; ++t) {
        const double a0 = xs[t * ldx];
        e = (0.2 * a0 + 0.1 * a1 - 0.1 * a3 - 0.2 * a4) + RASTA_POLE * e;
        a4 = a3; a3 = a2; a2 = a1; a1 = a0;
      }
    }
    ends[lane][col] = e;
    __syncthreads();
    double mine = carry, chain = carry;
    for (int l = 0; l < RASTA_LANES; ++l) {
      if (l == lane) mine = chain;
      chain = ends[l][col] + pw * chain;
    }
    carry = chain;
    if (cok) {
      double v = mine;
      for (long t = t0; t < t1; ++t) {
        const double a0 = xs[t * ldx];
        v = (0.2 * a0 + 0.1 * x1 - 0.1 * x3 - 0.2 * x4) + RASTA_POLE * v;
        x4 = x3; x3 = x2; x2 = x1; x1 = a0;
        ys[t * ldy] = (float)v;
      }
    }
    __syncthreads();   // ends is free for the next pass
  }
}

// ---- deltas ------------------------------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk, z = tile lane.  y[t] = sum_k filt[k] x[t + half - k] over the rows inside the segment, k ascending.
// x and y carry no __restrict__: they may be column blocks of one matrix.
__global__ __launch_bounds__(256) void feat_delta_kernel(const float* x, long ldx, const int64_t* __restrict__ seg_off, int D,
                                                         const double* __restrict__ filt, int L, float* y, long ldy) {
  __shared__ double f[SC_FEAT_MAX_TAPS];
  const Seg sg = feat_segment(seg_off, blockIdx.x);
  const int tid = threadIdx.x, col = tid & 15, c = blockIdx.y * FC + col, half = (L - 1) / 2;
  if (tid < L) f[tid] = filt[tid];
  __syncthreads();
  if (c >= D) return;
  const float* xs = x + sg.r0 * ldx + c;
  float* ys = y + sg.r0 * ldy + c;
  for (long t0 = (long)blockIdx.z * FT; t0 < sg.n; t0 += (long)FZ * FT)
    for (int r = tid >> 4; r < FT; r += 16) {
      const long t = t0 + r;
      if (t >= sg.n) break;
      double acc = 0.0;
      for (int k = 0; k < L; ++k) {
        const long j = t + half - k;
        if (j >= 0 && j < sg.n) acc += f[k] * (double)xs[j * ldx];
      }
      ys[t * ldy] = (float)acc;
    }
}

// ---- moments -----------------------------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk.  Lane l = tid >> 4 adds rows l, l + 16, ... of its column; the 16 partial sums are added in lane
// order.  Two passes: the mean, then the squared deviations from it (numpy.std).
__device__ inline double feat_join16(double (*red)[FC], int lane, int col, double v) {
  __syncthreads();   // the previous join has been read
  red[lane][col] = v;
  __syncthreads();
  double s = 0.0;
  for (int l = 0; l < 16; ++l) s += red[l][col];
  return s;
}

__global__ __launch_bounds__(256) void feat_moments_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ seg_off, int D,
                                                           double* __restrict__ mean, double* __restrict__ sd) {
  __shared__ double red[16][FC];
  const Seg sg = feat_segment(seg_off, blockIdx.x);
  const int tid = threadIdx.x, col = tid & 15, lane = tid >> 4, c = blockIdx.y * FC + col;
  const bool cok = c < D;
  const float* xs = x + sg.r0 * ldx + c;
  double s = 0.0;
  if (cok)
    for (long t = lane; t < sg.n; t += 16) s += (double)xs[t * ldx];
  const double mu = sg.n > 0 ? feat_join16(red, lane, col, s) / (double)sg.n : 0.0;
  double q = 0.0;
  if (cok)
    for (long t = lane; t < sg.n; t += 16) {
      const double d = (double)xs[t * ldx] - mu;
      q += d * d;
    }
  const double var = sg.n > 0 ? feat_join16(red, lane, col, q) / (double)sg.n : 1.0;
  if (cok && lane == 0) {
    mean[(long)blockIdx.x * D + c] = mu;
    sd[(long)blockIdx.x * D + c] = sqrt(var);
  }
}

// ---- normalisation -----------------------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk, z = tile lane.  See the head of the file for the tile.
// Bounds: the staged rows are [slo, shi) with shi - slo <= FT + w - 1 <= the column stride; a row index beyond n - 1 (the one duplicated
// row of an even short segment in the warp) reads row n - 1; columns beyond D are staged as zeros and never stored.
// One kernel per mode (MODE: a SC_FEAT_* value), so that only the warp carries normcdfinv -- and that behind a call: inlined, its
// constants are hoisted out of the tile loop into 430 registers (one wave per SIMD), or spilled when the registers are bounded.
__device__ __noinline__ double feat_probit(double p) { return normcdfinv(p); }

template <int MODE>
__global__ __launch_bounds__(256, 3) void feat_norm_kernel(const float* x, long ldx, const int64_t* __restrict__ seg_off, int D, int win,
                                                           const double* __restrict__ mean, const double* __restrict__ sd, float* y, long ldy) {
  constexpr int mode = MODE;
  extern __shared__ __attribute__((aligned(16))) float feat_smem[];
  const Seg sg = feat_segment(seg_off, blockIdx.x);
  const long n = sg.n;
  const int tid = threadIdx.x, c0 = blockIdx.y * FC;
  const float* xs = x + sg.r0 * ldx + c0;
  float* ys = y + sg.r0 * ldy + c0;
  const bool reduce = mode == SC_FEAT_CENTER_REDUCE || mode == SC_FEAT_SLIDING_CENTER_REDUCE;
  const bool warp = mode == SC_FEAT_WARP;
  if (mode <= SC_FEAT_CENTER_REDUCE || (!warp && n <= win)) {
    const int col = tid & 15;
    if (c0 + col >= D) return;
    const double mu = mean[(long)blockIdx.x * D + c0 + col], s = reduce ? sd[(long)blockIdx.x * D + c0 + col] : 1.0;
    for (long t0 = (long)blockIdx.z * FT; t0 < n; t0 += (long)FZ * FT)
      for (int r = tid >> 4; r < FT; r += 16) {
        const long t = t0 + r;
        if (t >= n) break;
        double v = (double)xs[t * ldx + col] - mu;
        if (reduce) v /= s;
        ys[t * ldy + col] = (float)v;
      }
    return;
  }
  // the window: w rows of the segment extended to m rows
  long w = win;
  if (warp && n < win) w = (n & 1) ? n : n + 1;
  const long m = n > w ? n : w, h = (w - 1) / 2;
  const int stride = feat_stride(win);
  float* out = feat_smem + (size_t)stride * FC;
  const int ncol = D - c0 < FC ? D - c0 : FC;
  for (long t0 = (long)blockIdx.z * FT; t0 < n; t0 += (long)FZ * FT) {
    const long t1 = t0 + FT < n ? t0 + FT : n;
    auto lo_of = [&](long t) { const long l = t - h < 0 ? 0 : t - h; return l > m - w ? m - w : l; };
    const long slo = lo_of(t0), shi = lo_of(t1 - 1) + w;
    const int cnt = (int)(shi - slo);
    __syncthreads();   // every thread is done with the previous tile
#pragma unroll 4
    for (int i = tid; i < cnt * FC; i += 256) {
      const int col = i & 15, j = i >> 4;
      long row = slo + j;
      if (row > n - 1) row = n - 1;
      feat_smem[col * stride + j] = col < ncol ? xs[row * ldx + col] : 0.f;
    }
    __syncthreads();
    const long t = t0 + tid;
    if (t < t1) {
      const int base = (int)(lo_of(t) - slo), self = (int)(t - slo), wi = (int)w;
#pragma unroll 1
      for (int col = 0; col < ncol; ++col) {      // one column at a time: a copy of the loops below per column would take every register
        const float* p = feat_smem + col * stride + base;
        const float xt = feat_smem[col * stride + self];
        double v;
        if (warp) {
          int below = 0;
#pragma unroll 8
          for (int j = 0; j < wi; ++j) below += p[j] < xt ? 1 : 0;
          v = feat_probit(((double)below + 0.5) / (double)wi);
        } else {
          double s = 0.0;
#pragma unroll 8
          for (int j = 0; j < wi; ++j) s += (double)p[j];
          const double mu = s / (double)wi;
          v = (double)xt - mu;
          if (reduce) {
            double q = 0.0;
#pragma unroll 8
            for (int j = 0; j < wi; ++j) {
              const double d = (double)p[j] - mu;
              q += d * d;
            }
            v /= sqrt(q / (double)(wi - 1));
          }
        }
        out[tid * FOUT + col] = (float)v;
      }
    }
    __syncthreads();
    const int rows = (int)(t1 - t0);
    for (int i = tid; i < rows * FC; i += 256) {
      const int col = i & 15, r = i >> 4;
      if (col < ncol) ys[(t0 + r) * ldy + col] = out[r * FOUT + col];
    }
  }
}

static int feat_check_common(const char* who, const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D) {
  SK_CHECK(d_x && d_seg_off, SK_EARG, "%s: null argument", who);
  SK_CHECK(S >= 0 && D >= 1 && D <= SC_FEAT_MAX_D && ldx >= D, SK_EARG, "%s: bad sizes (S=%d, D=%d with at most %d, ldx=%lld)", who, S, D,
           SC_FEAT_MAX_D, (long long)ldx);
  return SK_OK;
}

static int feat_check_out(const char* who, const float* d_x, int32_t D, const float* d_y, int64_t ldy, bool in_place_ok) {
  SK_CHECK(d_y, SK_EARG, "%s: null argument", who);
  SK_CHECK(ldy >= D, SK_EARG, "%s: bad sizes (D=%d, ldy=%lld)", who, D, (long long)ldy);
  SK_CHECK(in_place_ok || d_y != d_x, SK_EARG, "%s: y must not be x", who);
  return SK_OK;
}

static dim3 feat_grid(int S, int D, int z) { return dim3((unsigned)S, (unsigned)((D + FC - 1) / FC), (unsigned)z); }

}  // namespace sk

using namespace sk;

extern "C" {

int sc_feat_rasta(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, float* d_y, int64_t ldy, void* stream) {
  SK_TRY(feat_check_common("sc_feat_rasta", d_x, ldx, d_seg_off, S, D));
  SK_TRY(feat_check_out("sc_feat_rasta", d_x, D, d_y, ldy, false));
  if (S == 0) return SK_OK;
  hipLaunchKernelGGL(feat_rasta_kernel, feat_grid(S, D, 1), dim3(256), 0, (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_y, (long)ldy);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_feat_delta(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, const double* d_filt, int32_t L, float* d_y,
                  int64_t ldy, void* stream) {
  SK_TRY(feat_check_common("sc_feat_delta", d_x, ldx, d_seg_off, S, D));
  SK_TRY(feat_check_out("sc_feat_delta", d_x, D, d_y, ldy, false));
  SK_CHECK(d_filt, SK_EARG, "sc_feat_delta: null argument");
  SK_CHECK(L >= 1 && L <= SC_FEAT_MAX_TAPS && (L & 1), SK_EARG, "sc_feat_delta: the filter length must be odd and at most %d (got %d)",
           SC_FEAT_MAX_TAPS, L);
  if (S == 0) return SK_OK;
  hipLaunchKernelGGL(feat_delta_kernel, feat_grid(S, D, FZ), dim3(256), 0, (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_filt, L, d_y,
                     (long)ldy);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_feat_moments(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, double* d_mean, double* d_std, void* stream) {
  SK_TRY(feat_check_common("sc_feat_moments", d_x, ldx, d_seg_off, S, D));
  SK_CHECK(d_mean && d_std, SK_EARG, "sc_feat_moments: null argument");
  if (S == 0) return SK_OK;
  hipLaunchKernelGGL(feat_moments_kernel, feat_grid(S, D, 1), dim3(256), 0, (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_mean, d_std);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_feat_norm(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int32_t mode, int32_t win, const double* d_mean,
                 const double* d_std, float* d_y, int64_t ldy, void* stream) {
  SK_TRY(feat_check_common("sc_feat_norm", d_x, ldx, d_seg_off, S, D));
  SK_CHECK(mode >= SC_FEAT_CENTER && mode <= SC_FEAT_WARP, SK_EARG, "sc_feat_norm: unknown mode %d", mode);
  const bool windowed = mode >= SC_FEAT_SLIDING_CENTER;
  SK_TRY(feat_check_out("sc_feat_norm", d_x, D, d_y, ldy, !windowed));
  SK_CHECK(!windowed || (win >= 3 && win <= SC_FEAT_MAX_WIN && (win & 1)), SK_EARG, "sc_feat_norm: the window must be odd and within [3, %d] (got %d)",
           SC_FEAT_MAX_WIN, win);
  const bool divides = mode == SC_FEAT_CENTER_REDUCE || mode == SC_FEAT_SLIDING_CENTER_REDUCE;
  SK_CHECK(mode == SC_FEAT_WARP || (d_mean && (d_std || !divides)), SK_EARG, "sc_feat_norm: null argument (mode %d needs its tables)", mode);
  if (S == 0) return SK_OK;
  const size_t lds = windowed ? feat_lds_bytes(win) : 0;
#define FEAT_NORM(M)                                                                                                                            \
  case M:                                                                                                                                       \
    if (lds > 65536)                                                                                                                            \
      SK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(feat_norm_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   \
    hipLaunchKernelGGL(feat_norm_kernel<M>, feat_grid(S, D, FZ), dim3(256), lds, (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, win, d_mean, \
                       d_std, d_y, (long)ldy);                                                                                                  \
    break
  switch (mode) {
    FEAT_NORM(SC_FEAT_CENTER);
    FEAT_NORM(SC_FEAT_CENTER_REDUCE);
    FEAT_NORM(SC_FEAT_SLIDING_CENTER);
    FEAT_NORM(SC_FEAT_SLIDING_CENTER_REDUCE);
    FEAT_NORM(SC_FEAT_WARP);
  }
#undef FEAT_NORM
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
