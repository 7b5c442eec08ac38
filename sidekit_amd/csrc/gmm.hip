// Diagonal Gaussian mixture (sidekit/mixture.py:52-64, 510-536, 586-617): frame log-likelihoods, posteriors and Baum-Welch statistics of
// frames that stay on the device, without the N x C posterior matrix.  Two entry points (include/sidekit_amd/mixture.h):
//   sc_gmm_frame_loglik   pass A: lse[n] = log sum_c exp lp[n][c] (and lp itself on request)
//   sc_gmm_stats          pass B: per segment, stat0 / stat1 / stat2 = pp' . [1, X, X^2] with pp = exp(lp - lse), and the sum of lse
// and one of include/sidekit_amd/gmm_topc.h, here because it chooses from pass A's lp:
//   sc_gmm_top_components per frame, the K components with the largest lp (the lists of top-C scoring, gmm_topc.hip)
// Both form lp = -0.5 ([X^2, X] . [invcov, -2 mu invcov]' + A) tile by tile on v_mfma_f64_16x16x4_f64 (one GEMM with K = 2 D), by the
// same function in the same order (gmm_lp_tile), so pass B recomputes the bits pass A saw.  Recomputing costs 4 C D of the 12 C D FLOP
// per frame; storing lp would cost N C 8 bytes.  float64 throughout, no floating-point atomics, every sum in a fixed order.
// gmm_tile.h holds what this file shares with gmm_score.hip and the gmm_topc*.hip files, one copy each: the frame load, a segment's rows
// and slabs (the one place seg_off is read), the log-sum-exp update, merge and value, the argument checks; it also declares what this
// file defines for gmm_topc_stats.hip: the segment llk launcher and the two ends of a statistics launcher.  The chunk loop of
// gmm_lp_tile and the join of a tile's frames at the end of pass A exist a second time in gmm_score.hip, by copy: as shared functions
// they cost the scoring kernel 0.5 - 1.1 % (DESIGN section 4 "GMM-UBM scoring"), so a change to either is made in both files.
//
// One workgroup = 256 threads = 4 waves works on a tile of GT = 64 frames x 64 components; wave w owns components 16 w .. 16 w + 15 of
// the tile and all 64 frames (four 16 x 16 MFMA tiles, 16 accumulator doubles per lane).  LDS per workgroup, in doubles:
//   Xs  64 x (D | 1)   the frame tile, widened; the operand [X^2, X] is formed from it in the fragment read (odd row stride)
//   Gs  64 x 17        one 16-wide k-chunk of the component operand, the next chunk is fetched into registers meanwhile (dgemm_tile.h's scheme)
//   Ps  64 x 65        pass B: the posterior tile, [component][frame], the A operand of the second GEMM
// pass B at D = 60: 73 KB (two workgroups per CU), at D = 128: 108 KB (one); pass A: 40 KB / 75 KB.  Pass B's accumulator is
// 16 components x 16 NT columns per wave (NT tiles cover 2 D + 1 columns, or D + 1 for order 1): 4 NT doubles per lane, 32 at D = 60.
#include "../../include/sidekit_amd/gmm_topc.h"
#include "gmm_tile.h"
#include "kernels.h"

namespace sk {

constexpr int PLD = GT + 1;         // row stride of the posterior tile

// acc[i][q] = sum_d Xs[f][d]^2 invcov[c][d] + sum_d Xs[f][d] (-2 mu[c][d] invcov[c][d]),  f = 16 i + (lane >> 4) + 4 q,  c = c0 + 16 wave + (lane & 15);
// the squares first, then the linear half, each in chunks of 16 d (zeros beyond D and C).  Starts with a barrier (Xs is complete, Gs is free).
__device__ inline void gmm_lp_tile(const double* Xs, int xld, double* Gs, const double* __restrict__ mu, const double* __restrict__ invcov, int C,
                                   int D, int c0, f64x4 (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const int sr = tid >> 2, sd = (tid & 3) * 4;   // staging: component row sr, four consecutive d from sd
  const long srow = (long)(c0 + sr) * D;
  const bool sok = c0 + sr < C;
  const int nchunk = (D + DK - 1) / DK, total = 2 * nchunk;
  double g[4];
  auto fetch = [&](int ch) {
    const bool lin = ch >= nchunk;
    const int d0 = (lin ? ch - nchunk : ch) * DK + sd;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double v = 0.0;
      if (sok && d0 + u < D) {
        const double ic = invcov[srow + d0 + u];
        v = lin ? -2.0 * mu[srow + d0 + u] * ic : ic;
      }
      g[u] = v;
    }
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  fetch(0);
  for (int ch = 0; ch < total; ++ch) {
    __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
    for (int u = 0; u < 4; ++u) Gs[sr * DLD + sd + u] = g[u];
    __syncthreads();
    if (ch + 1 < total) fetch(ch + 1);
    const bool lin = ch >= nchunk;
    const int d0 = (lin ? ch - nchunk : ch) * DK;
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
}

// ---- pass A ------------------------------------------------------------------------------------------------------------------------
// grid: x = frame tile.  The workgroup walks the component tiles in ascending order; a lane keeps an online log-sum-exp state for each of
// its 16 frames over the components it sees (c = lane & 15 + 16 wave mod 64; lse_add), then the 16 lanes of a frame are joined by a
// butterfly (every lane ends with the same state), the four waves through LDS in wave order.  The order depends on C alone.
// Bounds: frames beyond N are zero rows whose lse is not stored; components beyond C are skipped; lp stores are guarded by both.
template <typename T>
__global__ __launch_bounds__(256, 2) void gmm_loglik_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                            const double* __restrict__ invcov, const double* __restrict__ A, int C,
                                                            double* __restrict__ lse, double* __restrict__ lp) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Gs = Xs + GT * xld;
  double* red = Gs + GT * DLD;   // [2][4][GT]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const long f0 = (long)blockIdx.x * GT;
  const int nvalid = N - f0 < GT ? (int)(N - f0) : GT;
  gmm_load_frames(X, D, f0, nvalid, Xs, xld);
  double M[4][4], S[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) { M[i][q] = -INFINITY; S[i][q] = 0.0; }
  for (int c0 = 0; c0 < C; c0 += GT) {
    f64x4 acc[4];
    gmm_lp_tile(Xs, xld, Gs, mu, invcov, C, D, c0, acc);
    const int c = c0 + wave * 16 + lr;
    if (c < C) {
      const double a = A[c];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double v = -0.5 * (acc[i][q] + a);
          const int fr = i * 16 + lk + 4 * q;
          if (lp && fr < nvalid) lp[(f0 + fr) * C + c] = v;
          lse_add(M[i][q], S[i][q], v);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(M[i][q], o), s2 = __shfl_xor(S[i][q], o);
        lse_merge(M[i][q], S[i][q], m2, s2);
      }
      if (lr == 0) {
        red[wave * GT + i * 16 + lk + 4 * q] = M[i][q];
        red[(4 + wave) * GT + i * 16 + lk + 4 * q] = S[i][q];
      }
    }
  __syncthreads();
  if (tid < nvalid) {
    double m = red[tid], s = red[4 * GT + tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) lse_merge(m, s, red[w * GT + tid], red[(4 + w) * GT + tid]);
    lse[f0 + tid] = lse_value(m, s);
  }
}

// ---- component lists -----------------------------------------------------------------------------------------------------------------
// grid: x = frame tile.  The workgroup walks the component tiles in ascending order as pass A does; after gmm_lp_tile the 64 x 64 tile of
// lp = -0.5 (acc + A) goes through Ps (nan staged as -inf) and is merged into a list of K (value, index) pairs per frame, Lv / Li, that
// lives in LDS.  The merge has two steps.  All four waves: thread (frame, quarter) compares its 16 components with the value of the
// list's worst entry as it stood before this tile (thr) and leaves a 16-bit set of candidates; after the first tile or two almost every
// set is empty.  Then thread f < 64 walks frame f's candidates in ascending component order: components below K fill the list as they
// are, a later one replaces the worst entry if its lp is larger -- an equal lp loses, it has the higher index -- and the worst entry
// (the smallest lp, at equal lp the highest index) is found again by a scan of the K pairs.  So a list always holds K distinct components
// below C, whatever the values are.  At the end entry k of a frame is stored at its rank among the frame's indices: ascending component.
// A frame's list is a function of its own row of acc alone, which is a function of the frame and the mixture.
// Bounds: frames beyond N are zero rows whose lists are not stored; components beyond C are never candidates; K <= min(C, 32, 64).
template <typename T>
__global__ __launch_bounds__(256, 2) void gmm_topc_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                          const double* __restrict__ invcov, const double* __restrict__ A, int C, int K,
                                                          int* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Gs = Xs + GT * xld;
  double* Ps = Gs + GT * DLD;               // [component][frame]
  double* Lv = Ps + GT * PLD;               // [K][GT]
  double* thr = Lv + K * GT;                // [GT]
  int* Li = (int*)(thr + GT);               // [K][GT]
  unsigned* cand = (unsigned*)Gs;           // [4][GT]: Gs is free from the barrier after the tile's last multiply to the next tile's first
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const long f0 = (long)blockIdx.x * GT;
  const int nvalid = N - f0 < GT ? (int)(N - f0) : GT;
  gmm_load_frames(X, D, f0, nvalid, Xs, xld);
  if (tid < GT) thr[tid] = -INFINITY;
  double wv = -INFINITY;   // thread f < 64: the worst entry of frame f's list, its value, component and place
  int wi = 0, wp = 0;
  auto worst = [&]() {
    wv = Lv[tid]; wi = Li[tid]; wp = 0;
    for (int k = 1; k < K; ++k) {
      const double v = Lv[k * GT + tid];
      const int i = Li[k * GT + tid];
      if (v < wv || (v == wv && i > wi)) { wv = v; wi = i; wp = k; }
    }
  };
  for (int c0 = 0; c0 < C; c0 += GT) {
    f64x4 acc[4];
    gmm_lp_tile(Xs, xld, Gs, mu, invcov, C, D, c0, acc);
    {
      const int c = c0 + wave * 16 + lr;
      const double a = c < C ? A[c] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double v = -0.5 * (acc[i][q] + a);
          Ps[(wave * 16 + lr) * PLD + i * 16 + lk + 4 * q] = v != v ? -INFINITY : v;
        }
    }
    __syncthreads();   // Ps is complete, every wave is done with Gs
    {
      const double t = thr[lane];
      unsigned m = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int c = c0 + wave * 16 + j;
        const double v = Ps[(wave * 16 + j) * PLD + lane];
        if (c < C && (c < K || v > t)) m |= 1u << j;
      }
      cand[wave * GT + lane] = m;
    }
    __syncthreads();
    if (tid < GT) {
      for (int q = 0; q < 4; ++q) {
        unsigned m = cand[q * GT + tid];
        while (m) {
          const int j = __ffs(m) - 1;
          m &= m - 1;
          const int c = c0 + q * 16 + j;
          const double v = Ps[(q * 16 + j) * PLD + tid];
          if (c < K) {
            Lv[c * GT + tid] = v;
            Li[c * GT + tid] = c;
            if (c == K - 1) worst();
          } else if (v > wv) {
            Lv[wp * GT + tid] = v;
            Li[wp * GT + tid] = c;
            worst();
          }
        }
      }
      thr[tid] = wv;
    }
    // the next tile's first barrier (gmm_lp_tile) comes before anything of Gs, Ps or thr is touched again
  }
  __syncthreads();
  for (int e = tid; e < K * GT; e += 256) {
    const int f = e & (GT - 1), k = e / GT;
    if (f >= nvalid) continue;
    const int me = Li[k * GT + f];
    int rank = 0;
    for (int k2 = 0; k2 < K; ++k2) rank += Li[k2 * GT + f] < me;
    out[(f0 + f) * K + rank] = me;
  }
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------------
// grid: x = segment * nslab + slab, y = component tile.  Per frame tile of its slab (tiles start at the slab's first frame) the workgroup
// recomputes lp, forms pp = exp(lp - lse[n]) in registers -- 0 by assignment for a frame outside the slab or a component beyond C, whose
// lse / A are not read -- stages it through Ps and accumulates pp' . Y on the matrix cores, Y[n][:] = [1, X[n][:], X[n][:]^2] read from
// Xs (ncols = 2 D + 1, or D + 1 for order 1; NT 16-column tiles cover it).  The partial goes to part0/1/2 at (slab * S + segment): with one
// slab per segment these are the outputs themselves, otherwise workspace that slab_reduce joins in slab order.  A slab beyond the
// segment's own cut (the grid is sized for the longest segment) multiplies nothing and stores zeros.
// Bounds: the slab's rows lie within [0, N] (gmm_segment, gmm_slab); frames beyond the slab's end are zero rows; stores are guarded by
// c < C and the column's range.
template <int NT, typename T>
__global__ __launch_bounds__(256, NT <= 8 ? 2 : 1) void gmm_stats_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                                         const double* __restrict__ invcov, const double* __restrict__ A, int C,
                                                                         const double* __restrict__ lse, const int* __restrict__ seg_off, int S,
                                                                         long max_len, int nslab, int ncols, double* __restrict__ part0,
                                                                         double* __restrict__ part1, double* __restrict__ part2) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Gs = Xs + GT * xld;
  double* Ps = Gs + GT * DLD;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const int seg = blockIdx.x / nslab, slab = blockIdx.x % nslab, c0 = blockIdx.y * GT;
  const GmmRows rows = gmm_slab(gmm_segment(seg_off, seg, N, max_len), slab);
  const long k_begin = rows.begin, k_end = rows.end;
  f64x4 st[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) st[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int c = c0 + wave * 16 + lr;
  const double a_c = c < C ? A[c] : 0.0;
  for (long t0 = k_begin; t0 < k_end; t0 += GT) {
    const int nvalid = k_end - t0 < GT ? (int)(k_end - t0) : GT;
    __syncthreads();   // every wave is done with the previous tile's Xs and Ps
    gmm_load_frames(X, D, t0, nvalid, Xs, xld);
    f64x4 acc[4];
    gmm_lp_tile(Xs, xld, Gs, mu, invcov, C, D, c0, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int fr = i * 16 + lk + 4 * q;
        double p = 0.0;
        if (c < C && fr < nvalid) p = exp(-0.5 * (acc[i][q] + a_c) - lse[t0 + fr]);
        Ps[(wave * 16 + lr) * PLD + fr] = p;
      }
    __syncthreads();
    for (int kk = 0; kk < GT; kk += 4) {
      const double a = Ps[(wave * 16 + lr) * PLD + kk + lk];
      const double* xrow = Xs + (kk + lk) * xld;
      double b[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = j * 16 + lr;
        double v = 0.0;
        if (col == 0) v = 1.0;
        else if (col <= D) v = xrow[col - 1];
        else if (col < ncols) { const double x = xrow[col - 1 - D]; v = x * x; }
        b[j] = v;
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) st[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], st[j], 0, 0, 0);
    }
  }
  const long slot = (long)slab * S + seg;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cc = c0 + wave * 16 + lk + 4 * q;
    if (cc >= C) continue;
    const long row = slot * C + cc;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = j * 16 + lr;
      if (col == 0) part0[row] = st[j][q];
      else if (col <= D) part1[row * D + col - 1] = st[j][q];
      else if (col < ncols) part2[row * D + col - 1 - D] = st[j][q];
    }
  }
}

// llk[s] = sum of lse over segment s: thread t adds frames t, t + 256, ... of the segment, then a tree over the 256 threads.
__global__ __launch_bounds__(256) void gmm_seg_llk_kernel(const double* __restrict__ lse, long N, const int* __restrict__ seg_off, long max_len,
                                                          double* __restrict__ llk) {
  __shared__ double red[256];
  const int tid = threadIdx.x, seg = blockIdx.x;
  const GmmRows rows = gmm_segment(seg_off, seg, N, max_len);
  double s = 0.0;
  for (long i = rows.begin + tid; i < rows.end; i += 256) s += lse[i];
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) llk[seg] = red[0];
}

int launch_gmm_seg_llk(const double* lse, long N, const int* seg_off, int S, long max_len, double* llk, hipStream_t st) {
  hipLaunchKernelGGL(gmm_seg_llk_kernel, dim3((unsigned)S), dim3(256), 0, st, lse, N, seg_off, max_len, llk);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int gmm_stats_lease(hipStream_t st, std::unique_lock<std::mutex>& lock, int S, long max_len, int C, int D, int order, double* stat0,
                    double* stat1, double* stat2, GmmStatParts* out) {
  const int nslab = (int)gmm_slabs(max_len);
  const long n0 = (long)S * C, n1 = n0 * D, n2 = order == 2 ? n1 : 0;
  *out = {nslab, n0, n1, n2, stat0, stat1, stat2, stat0, stat1, stat2};
  if (nslab > 1) {
    void* ws = nullptr;
    lock.lock();
    SK_TRY(plda_workspace_locked(st, (size_t)nslab * (n0 + n1 + n2) * 8, &ws));
    out->p0 = (double*)ws;
    out->p1 = out->p0 + nslab * n0;
    out->p2 = out->p1 + nslab * n1;
  }
  return SK_OK;
}

int gmm_stats_finish(const GmmStatParts& p, const double* lse, long N, const int* seg_off, int S, long max_len, double* llk, hipStream_t st) {
  if (p.nslab > 1) {
    SK_TRY(launch_slab_reduce(p.p0, p.nslab, p.n0, p.stat0, st));
    SK_TRY(launch_slab_reduce(p.p1, p.nslab, p.n1, p.stat1, st));
    if (p.n2) SK_TRY(launch_slab_reduce(p.p2, p.nslab, p.n2, p.stat2, st));
  }
  if (llk) SK_TRY(launch_gmm_seg_llk(lse, N, seg_off, S, max_len, llk, st));
  return SK_OK;
}

template <typename T>
static int launch_gmm_loglik(const T* X, long N, int D, const double* mu, const double* invcov, const double* A, int C, double* lse, double* lp,
                             hipStream_t st) {
  const size_t lds = (size_t)(GT * gmm_xld(D) + GT * DLD + 8 * GT) * 8;
  SK_TRY(gmm_allow_lds(gmm_loglik_kernel<T>, lds));
  hipLaunchKernelGGL(gmm_loglik_kernel<T>, dim3((unsigned)((N + GT - 1) / GT)), dim3(256), lds, st, X, N, D, mu, invcov, A, C, lse, lp);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

__host__ __device__ inline size_t gmm_topc_lds(int D, int K) {
  return (size_t)(GT * gmm_xld(D) + GT * DLD + GT * PLD + K * GT + GT) * 8 + (size_t)K * GT * 4;
}

template <typename T>
static int launch_gmm_topc(const T* X, long N, int D, const double* mu, const double* invcov, const double* A, int C, int K, int* idx, hipStream_t st) {
  const size_t lds = gmm_topc_lds(D, K);
  SK_TRY(gmm_allow_lds(gmm_topc_kernel<T>, lds));
  hipLaunchKernelGGL(gmm_topc_kernel<T>, dim3((unsigned)((N + GT - 1) / GT)), dim3(256), lds, st, X, N, D, mu, invcov, A, C, K, idx);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <int NT, typename T>
static int launch_gmm_stats_nt(const T* X, long N, int D, const double* mu, const double* invcov, const double* A, int C, const double* lse,
                               const int* seg_off, int S, long max_len, int nslab, int ncols, double* p0, double* p1, double* p2, hipStream_t st) {
  const size_t lds = (size_t)(GT * gmm_xld(D) + GT * DLD + GT * PLD) * 8;
  SK_TRY(gmm_allow_lds(gmm_stats_kernel<NT, T>, lds));
  const dim3 grid((unsigned)((long)S * nslab), (unsigned)((C + GT - 1) / GT));
  hipLaunchKernelGGL((gmm_stats_kernel<NT, T>), grid, dim3(256), lds, st, X, N, D, mu, invcov, A, C, lse, seg_off, S, max_len, nslab, ncols, p0, p1, p2);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <typename T>
static int launch_gmm_stats(const T* X, long N, int D, const double* mu, const double* invcov, const double* A, int C, const double* lse,
                            const int* seg_off, int S, long max_len, int order, double* stat0, double* stat1, double* stat2, double* llk,
                            hipStream_t st) {
  const int ncols = order == 2 ? 2 * D + 1 : D + 1, nt = (ncols + 15) / 16;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);   // held, if gmm_stats_lease takes it, until this function returns
  GmmStatParts p;
  SK_TRY(gmm_stats_lease(st, lock, S, max_len, C, D, order, stat0, stat1, stat2, &p));
#define GMM_STATS(NT) \
  SK_TRY((launch_gmm_stats_nt<NT, T>(X, N, D, mu, invcov, A, C, lse, seg_off, S, max_len, p.nslab, ncols, p.p0, p.p1, p.p2, st)))
  if (nt <= 2) GMM_STATS(2);
  else if (nt <= 4) GMM_STATS(4);
  else if (nt <= 8) GMM_STATS(8);
  else if (nt <= 12) GMM_STATS(12);
  else GMM_STATS(17);
#undef GMM_STATS
  return gmm_stats_finish(p, lse, N, seg_off, S, max_len, llk, st);
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_frame_loglik(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A,
                        int32_t C, double* d_lse, double* d_lp, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_frame_loglik", d_X, x_dtype, N, D, d_mu, d_invcov, d_A, C));
  SK_CHECK(d_lse, SK_EARG, "sc_gmm_frame_loglik: null argument");
  if (x_dtype == XT_F32) return launch_gmm_loglik((const float*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, d_lse, d_lp, (hipStream_t)stream);
  return launch_gmm_loglik((const double*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, d_lse, d_lp, (hipStream_t)stream);
}

int sc_gmm_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A, int32_t C,
                 const double* d_lse, const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order, double* d_stat0, double* d_stat1,
                 double* d_stat2, double* d_llk, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_stats", d_X, x_dtype, N, D, d_mu, d_invcov, d_A, C));
  SK_CHECK(order == 1 || order == 2, SK_EARG, "sc_gmm_stats: order must be 1 or 2 (got %d)", order);
  SK_CHECK(d_lse && d_seg_off && d_stat0 && d_stat1 && (order == 1 || d_stat2), SK_EARG, "sc_gmm_stats: null argument");
  SK_TRY(gmm_check_segments("sc_gmm_stats", N, S, max_len));
  if (x_dtype == XT_F32)
    return launch_gmm_stats((const float*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1, d_stat2,
                            d_llk, (hipStream_t)stream);
  return launch_gmm_stats((const double*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1, d_stat2,
                          d_llk, (hipStream_t)stream);
}

int sc_gmm_top_components(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A,
                          int32_t C, int32_t K, int32_t* d_idx, void* stream) {
  SK_TRY(gmm_check_common("sc_gmm_top_components", d_X, x_dtype, N, D, d_mu, d_invcov, d_A, C));
  SK_CHECK(d_idx, SK_EARG, "sc_gmm_top_components: null argument");
  SK_TRY(gmm_check_topc("sc_gmm_top_components", K, C));
  if (x_dtype == XT_F32) return launch_gmm_topc((const float*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, K, d_idx, (hipStream_t)stream);
  return launch_gmm_topc((const double*)d_X, (long)N, D, d_mu, d_invcov, d_A, C, K, d_idx, (hipStream_t)stream);
}

}  // extern "C"
