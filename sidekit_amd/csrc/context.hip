// Context features of a stacked ragged batch (sidekit/frontend/features.py:169-223 pca_dct and shifted_delta_cepstral,
// sidekit/features_server.py:325-394 get_context and get_traps): a linear map over a window of frames around t, the segment's first and
// last row repeated past its ends.  Three entry points (include/sidekit_amd/context.h).  float32 rows in; no atomics, every sum in a
// fixed order; grid.x is always the segment and every tile is counted from the segment's first row, so a segment's bits do not depend on
// the batch around it.  The tiles of a segment are dealt round robin to grid.z workgroups; the host sizes grid.z from max_rows and S (a
// workgroup whose first tile lies beyond its segment leaves at once), and which workgroup takes a tile changes no bit of it.
//
//   ctx_gather_kernel   streaming: the GT + span rows a tile of GT = 256 rows touches are staged once, row-major, 16 columns wide
//                       ((256 + 256) x 16 x 4 + 2 x 256 x 4 = 34,816 B at the largest span); the stores walk (row, block, column) with
//                       the column fastest, so that with D <= 16 a row of y is one contiguous run.
//   ctx_basis_kernel    the basis (W x J float64) and the BT + W - 1 rows of a tile of BT = 128, column-major, in LDS
//                       (64 x 64 x 8 + 191 x 16 x 4 = 44,992 B at W = J = 64).  A wave takes four rows at a time and its lanes the
//                       outputs (c, j) of the column chunk, j fastest: the basis is read once per four fused multiply-adds, lanes of one
//                       coefficient share their frame words (a broadcast), and a row's outputs leave as one contiguous run.
//   ctx_project_kernel  64 x 64 tiles of y on v_mfma_f64_16x16x4_f64 with dgemm_tile.h's LDS images ([row][k], 17 doubles a row), lane
//                       map and tile store, around a k-loop and an A loader of its own: element k = w D + c of row t is
//                       x[cl(t + w - left)][c], fetched as pairs (one 8-byte load where the pair lies inside a frame and is aligned)
//                       and widened on the way into LDS; the next k-tile is fetched while this one is multiplied.  The result tile
//                       crosses LDS (64 x 65 doubles) so that a row is stored as one run of floats: 2 x 8,704 + 33,280 = 50,688 B.
#include "../../include/sidekit_amd/context.h"
#include "common.h"
#include "dgemm_tile.h"

namespace sk {

constexpr int GT = SC_CTX_TILE, GC = SC_CTX_COLS, BT = SC_CTX_BASIS_TILE, PT = SC_CTX_PROJ_TILE, BR = 4;
constexpr int CTX_WORKGROUPS = 8192;   // what the grid aims at: 32 workgroups for each of 256 CUs, so that the last round of them is short

struct CtxSeg { long r0, n; };
__device__ inline CtxSeg ctx_segment(const int64_t* seg_off, int s) {
  long r0 = seg_off[s], r1 = seg_off[s + 1];
  if (r0 < 0) r0 = 0;
  return CtxSeg{r0, r1 > r0 ? r1 - r0 : 0};
}
__device__ inline long ctx_clamp(long i, long n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

__host__ __device__ inline int ctx_basis_stride(int W) { return (BT + W - 1) | 1; }
__host__ inline size_t ctx_basis_lds(int W, int J) { return (size_t)W * J * 8 + (size_t)ctx_basis_stride(W) * GC * 4; }

// e / n for 0 <= e * (n - 1) < 65536 with inv = ceil(65536 / n): e inv / 65536 = e / n + e d / (65536 n), d = inv n - 65536 < n, and
// the second term cannot carry the quotient over while e d < 65536
__host__ __device__ inline int ctx_inv(int n) { return (65536 + n - 1) / n; }
__device__ inline int ctx_div(int e, int inv) { return (int)(((unsigned)e * (unsigned)inv) >> 16); }

// ---- stacked context, shifted deltas -------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk, z = tile lane.  Bounds: an offset is clamped into [lo, lo + span], so a staged row index
// (t - t0) + (o - lo) lies in [0, rows + span) with rows + span <= GT + SC_CTX_MAX_SPAN; global rows are clamped into the segment;
// columns c < D only.  x and y carry no __restrict__: they may be column blocks of one matrix.
__global__ __launch_bounds__(256) void ctx_gather_kernel(const float* x, long ldx, const int64_t* __restrict__ seg_off, int D,
                                                         const int32_t* __restrict__ plus, const int32_t* __restrict__ minus, int J, int lo,
                                                         int span, float* y, long ldy) {
  __shared__ float rows_s[(GT + SC_CTX_MAX_SPAN) * GC];
  __shared__ int off_s[2][SC_CTX_MAX_BLOCKS];
  const CtxSeg sg = ctx_segment(seg_off, blockIdx.x);
  const long n = sg.n;
  const int tid = threadIdx.x, c0 = blockIdx.y * GC;
  const int ncol = D - c0 < GC ? D - c0 : GC;
  if ((long)blockIdx.z * GT >= n) return;
  for (int b = tid; b < J; b += 256) {
    const int p = plus[b], m = minus ? minus[b] : 0;
    off_s[0][b] = (p < lo ? lo : (p > lo + span ? lo + span : p)) - lo;
    off_s[1][b] = (m < lo ? lo : (m > lo + span ? lo + span : m)) - lo;
  }
  const float* xs = x + sg.r0 * ldx + c0;
  float* ys = y + sg.r0 * ldy + c0;
  const int E = J * ncol, inv = ctx_inv(ncol);        // E <= 256 * 16: (E - 1) * 15 < 65536
  const int step_r = 256 / E, step_e = 256 % E;
  const bool sub = minus != nullptr;
  for (long t0 = (long)blockIdx.z * GT; t0 < n; t0 += (long)gridDim.z * GT) {
    const int rows = (int)(t0 + GT < n ? GT : n - t0), cnt = rows + span;
    __syncthreads();   // every thread is done with the previous tile (and, the first time, the offsets are in LDS)
    for (int i = tid; i < cnt * GC; i += 256) {
      const int col = i & 15, j = i >> 4;
      rows_s[i] = col < ncol ? xs[ctx_clamp(t0 + lo + j, n) * ldx + col] : 0.f;
    }
    __syncthreads();
    int r = tid / E, e = tid % E;
    while (r < rows) {
      const int b = ctx_div(e, inv), col = e - b * ncol;
      float v = rows_s[(r + off_s[0][b]) * GC + col];
      if (sub) v -= rows_s[(r + off_s[1][b]) * GC + col];
      ys[(t0 + r) * ldy + (long)b * D + col] = v;
      r += step_r; e += step_e;
      if (e >= E) { e -= E; ++r; }
    }
  }
}

// ---- a temporal basis per coefficient ------------------------------------------------------------------------------------------------
// grid: x = segment, y = column chunk, z = tile lane.  Bounds: staged rows j < rows + W - 1 <= BT + W - 1 <= the column stride are
// written, rows up to BT + W - 2 of the stride are read (those past rows + W - 2 feed results that are never stored); outputs of rows
// t < n and columns c < D only.
__global__ __launch_bounds__(256) void ctx_basis_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ seg_off, int D,
                                                        const double* __restrict__ basis, int W, int J, int left, float* __restrict__ y,
                                                        long ldy) {
  extern __shared__ __attribute__((aligned(16))) double ctx_smem[];
  double* bs = ctx_smem;
  float* fr = reinterpret_cast<float*>(ctx_smem + W * J);
  const CtxSeg sg = ctx_segment(seg_off, blockIdx.x);
  const long n = sg.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c0 = blockIdx.y * GC;
  const int ncol = D - c0 < GC ? D - c0 : GC, stride = ctx_basis_stride(W);
  if ((long)blockIdx.z * BT >= n) return;
  for (int i = tid; i < W * J; i += 256) bs[i] = basis[i];
  for (int i = tid; i < stride * GC; i += 256) fr[i] = 0.f;
  const float* xs = x + sg.r0 * ldx + c0;
  float* ys = y + sg.r0 * ldy + (long)c0 * J;
  const int E = ncol * J, inv = ctx_inv(J);           // E <= 16 * 64: (E - 1) * 63 < 65536
  for (long t0 = (long)blockIdx.z * BT; t0 < n; t0 += (long)gridDim.z * BT) {
    const int rows = (int)(t0 + BT < n ? BT : n - t0), cnt = rows + W - 1;
    __syncthreads();   // every wave is done with the previous tile (and, the first time, the basis is in LDS)
    for (int i = tid; i < cnt * GC; i += 256) {
      const int col = i & 15, j = i >> 4;
      if (col < ncol) fr[col * stride + j] = xs[ctx_clamp(t0 - left + j, n) * ldx + col];
    }
    __syncthreads();
    for (int r = wave * BR; r < rows; r += 4 * BR)
      for (int o = lane; o < E; o += 64) {
        const int c = ctx_div(o, inv), j = o - c * J;
        const float* p = fr + c * stride + r;
        const double* q = bs + j;
        double acc[BR] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < W; ++w) {
          const double b = q[w * J];
#pragma unroll
          for (int i = 0; i < BR; ++i) acc[i] = fma(b, (double)p[w + i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i)
          if (r + i < rows) ys[(t0 + r + i) * ldy + o] = (float)acc[i];
      }
  }
}

// ---- the windowed projection ---------------------------------------------------------------------------------------------------------
// grid: x = segment, y = column tile of y, z = tile lane.  Bounds: a row of the tile beyond the segment and an element k >= K are zeros
// and read nothing; frame rows are clamped into the segment; a pair is read with one load only when both elements lie in one frame
// (c + 1 < D) and the address is 8-byte aligned; columns of M beyond Q are zeros (fetch_across); rows t < n and columns q < Q are stored.
__device__ inline double2 ctx_fetch_window(const float* __restrict__ xs, long ldx, long n, long t, bool live, int left, int D, int K, int k) {
  double2 v = {0.0, 0.0};
  if (!live || k >= K) return v;
  const int w = k / D, c = k - w * D;
  const float* p = xs + ctx_clamp(t - left + w, n) * ldx + c;
  v = fetch_pair(p, (reinterpret_cast<size_t>(p) & 7) == 0, c, D);
  if (c + 1 == D && k + 1 < K) v.y = (double)xs[ctx_clamp(t - left + w + 1, n) * ldx];   // the pair straddles two frames
  return v;
}

__global__ __launch_bounds__(256) void ctx_project_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ seg_off, int D,
                                                          const double* __restrict__ M, int W, int left, int Q, float* __restrict__ y,
                                                          long ldy) {
  constexpr int WT = PT / 32, PA = PT * DK / 2 / 256, OLD = PT + 1;
  __shared__ double As[PT * DLD], Bs[PT * DLD], Os[PT * OLD];
  const CtxSeg sg = ctx_segment(seg_off, blockIdx.x);
  const long n = sg.n;
  if ((long)blockIdx.z * PT >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, n0 = blockIdx.y * PT, K = W * D;
  const dgemm_lanes<WT> at;
  const float* xs = x + sg.r0 * ldx;
  float* ys = y + sg.r0 * ldy;
  const bool vec_b = (Q & 1) == 0 && (reinterpret_cast<size_t>(M) & 15) == 0;
  for (long t0 = (long)blockIdx.z * PT; t0 < n; t0 += (long)gridDim.z * PT) {
    double2 ra[PA], rb[PA];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int idx = tid + 256 * q;
        const long t = t0 + along_k_row(idx);
        ra[q] = ctx_fetch_window(xs, ldx, n, t, t < n, left, D, K, k0 + (idx & 7) * 2);
        rb[q] = fetch_across<PT>(M, vec_b, k0, K, n0, Q, idx);
      }
    };
    f64x4 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += DK) {
      __syncthreads();   // every wave is done reading the previous k-tile (and the previous tile's result)
#pragma unroll
      for (int q = 0; q < PA; ++q) {
        const int idx = tid + 256 * q, a = along_k_at(idx), b = across_at<PT>(idx);
        As[a] = ra[q].x; As[a + 1] = ra[q].y;
        Bs[b] = rb[q].x; Bs[b + DLD] = rb[q].y;
      }
      __syncthreads();
      if (k0 + DK < K) fetch(k0 + DK);
#pragma unroll
      for (int kk = 0; kk < DK; kk += 4) {
        double a[WT], b[WT];
#pragma unroll
        for (int i = 0; i < WT; ++i) {
          a[i] = As[(at.wm * 16 * WT + i * 16 + at.lr) * DLD + kk + at.lk];
          b[i] = Bs[(at.wn * 16 * WT + i * 16 + at.lr) * DLD + kk + at.lk];
        }
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
          for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    dgemm_store_tile<WT>(acc, at, Os, OLD, 0, 0, PT, PT);
    __syncthreads();
    const int rows = (int)(t0 + PT < n ? PT : n - t0), cols = Q - n0 < PT ? Q - n0 : PT;
    for (int r = tid >> 6; r < rows; r += 4)
      if (lane < cols) ys[(t0 + r) * ldy + n0 + lane] = (float)Os[r * OLD + lane];
  }
}

static int ctx_check_common(const char* who, const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int max_d,
                            int64_t max_rows, const float* d_y) {
  SK_CHECK(d_x && d_seg_off && d_y, SK_EARG, "%s: null argument", who);
  SK_CHECK(S >= 0 && D >= 1 && D <= max_d && ldx >= D && max_rows >= 1, SK_EARG,
           "%s: bad sizes (S=%d, D=%d with at most %d, ldx=%lld, max_rows=%lld)", who, S, D, max_d, (long long)ldx, (long long)max_rows);
  SK_CHECK(d_y != d_x, SK_EARG, "%s: y must not be x", who);
  return SK_OK;
}

// grid.z: the tiles of the longest segment, but no more than brings the grid to CTX_WORKGROUPS
static unsigned ctx_lanes(int64_t max_rows, int tile, int S, int chunks) {
  const int64_t tiles = (max_rows + tile - 1) / tile, per = (int64_t)S * chunks;
  int64_t want = (CTX_WORKGROUPS + per - 1) / per;
  if (want > tiles) want = tiles;
  if (want > 65535) want = 65535;
  return (unsigned)(want < 1 ? 1 : want);
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_ctx_gather(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const int32_t* d_plus,
                  const int32_t* d_minus, int32_t J, int32_t lo, int32_t span, float* d_y, int64_t ldy, void* stream) {
  SK_TRY(ctx_check_common("sc_ctx_gather", d_x, ldx, d_seg_off, S, D, SC_CTX_MAX_D, max_rows, d_y));
  SK_CHECK(d_plus, SK_EARG, "sc_ctx_gather: null argument");
  SK_CHECK(J >= 1 && J <= SC_CTX_MAX_BLOCKS, SK_EARG, "sc_ctx_gather: the output blocks must be within [1, %d] (got %d)", SC_CTX_MAX_BLOCKS, J);
  SK_CHECK(span >= 0 && span <= SC_CTX_MAX_SPAN && lo >= -SC_CTX_MAX_SPAN && lo <= SC_CTX_MAX_SPAN, SK_EARG,
           "sc_ctx_gather: the offsets must span at most %d rows and lie within %d rows of t (got lo=%d, span=%d)", SC_CTX_MAX_SPAN,
           SC_CTX_MAX_SPAN, lo, span);
  SK_CHECK(ldy >= (int64_t)J * D, SK_EARG, "sc_ctx_gather: bad sizes (J=%d, D=%d, ldy=%lld)", J, D, (long long)ldy);
  if (S == 0) return SK_OK;
  const int chunks = (D + GC - 1) / GC;
  hipLaunchKernelGGL(ctx_gather_kernel, dim3((unsigned)S, (unsigned)chunks, ctx_lanes(max_rows, GT, S, chunks)), dim3(256), 0,
                     (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_plus, d_minus, J, lo, span, d_y, (long)ldy);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_ctx_basis(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const double* d_basis,
                 int32_t W, int32_t J, int32_t left, float* d_y, int64_t ldy, void* stream) {
  SK_TRY(ctx_check_common("sc_ctx_basis", d_x, ldx, d_seg_off, S, D, SC_CTX_MAX_D, max_rows, d_y));
  SK_CHECK(d_basis, SK_EARG, "sc_ctx_basis: null argument");
  SK_CHECK(W >= 1 && W <= SC_CTX_MAX_W && J >= 1 && J <= W && left >= 0 && left < W, SK_EARG,
           "sc_ctx_basis: the window must be within [1, %d], the basis within [1, W] and left within [0, W) (got W=%d, J=%d, left=%d)",
           SC_CTX_MAX_W, W, J, left);
  SK_CHECK(ldy >= (int64_t)J * D, SK_EARG, "sc_ctx_basis: bad sizes (J=%d, D=%d, ldy=%lld)", J, D, (long long)ldy);
  if (S == 0) return SK_OK;
  const int chunks = (D + GC - 1) / GC;
  hipLaunchKernelGGL(ctx_basis_kernel, dim3((unsigned)S, (unsigned)chunks, ctx_lanes(max_rows, BT, S, chunks)), dim3(256), ctx_basis_lds(W, J),
                     (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_basis, W, J, left, d_y, (long)ldy);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_ctx_project(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const double* d_m,
                   int32_t W, int32_t left, int32_t Q, float* d_y, int64_t ldy, void* stream) {
  SK_TRY(ctx_check_common("sc_ctx_project", d_x, ldx, d_seg_off, S, D, SC_CTX_PROJ_MAX_D, max_rows, d_y));
  SK_CHECK(d_m, SK_EARG, "sc_ctx_project: null argument");
  SK_CHECK(W >= 1 && W <= SC_CTX_MAX_W && left >= 0 && left < W && Q >= 1 && Q <= SC_CTX_PROJ_MAX_Q, SK_EARG,
           "sc_ctx_project: the window must be within [1, %d], left within [0, W) and Q within [1, %d] (got W=%d, left=%d, Q=%d)",
           SC_CTX_MAX_W, SC_CTX_PROJ_MAX_Q, W, left, Q);
  SK_CHECK(ldy >= Q, SK_EARG, "sc_ctx_project: bad sizes (Q=%d, ldy=%lld)", Q, (long long)ldy);
  if (S == 0) return SK_OK;
  const int chunks = (Q + PT - 1) / PT;
  hipLaunchKernelGGL(ctx_project_kernel, dim3((unsigned)S, (unsigned)chunks, ctx_lanes(max_rows, PT, S, chunks)), dim3(256), 0,
                     (hipStream_t)stream, d_x, (long)ldx, d_seg_off, D, d_m, W, left, Q, d_y, (long)ldy);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
