// Full-covariance Gaussian mixture (sidekit/mixture.py:490-508, 586-617, 673-686): frame log-likelihoods and Baum-Welch statistics with
// the full second-order statistic, of frames that stay on the device, without an N x C or an N x D x D array.  Two entry points
// (include/sidekit_amd/gmm_full.h):
//   sc_gmm_full_frame_loglik   pass A: lse[n] = log sum_c exp lp[n][c] (and lp itself on request)
//   sc_gmm_full_stats          pass B: per segment, stat0 / stat1 / stat2 = sum_n pp [1, X, X X'] with pp = exp(lp - lse), and the sum of lse
// Both form lp[n][c] = g[c] - 0.5 |M[c] (X[n] - mu[c])|^2 for one component and 64 frames at a time on v_mfma_f64_16x16x4_f64, by the same
// function in the same order (full_lp), so pass B recomputes the bits pass A saw.  M[c] is a general D x D matrix.  float64 throughout,
// no floating-point atomics, every sum in a fixed order.  gmm_tile.h gives the frame tile and its load, a segment's rows, the
// log-sum-exp helpers, the checks and the two ends of a statistics launcher; the cut of a segment into slabs is this file's own
// (full_slabs: it depends on C as well as on the length, see the header).
//
// One workgroup = 256 threads = 4 waves; wave w owns frames 16 w .. 16 w + 15 of the tile of GT = 64.  LDS per workgroup, in doubles:
//   Xs   64 x (D | 1)          the frame tile, widened; centred in the fragment read (x - mu[c], then the multiply)
//   Ms   16 NT x (Kp + 1)      M[c] as [m][k], zeros beyond D in both directions; NT = D / 16 + 1 tiles of 16, Kp = D rounded up to 4
//   mus  Kp                    mu[c]
//   Ps   64                    pass B: the posteriors of the tile's frames for the component
// D = 60: 62 KB (two workgroups per CU), D = 96: 137 KB (one).  Pass A fetches the next component's matrix, pass B the next frame tile,
// into registers while the current one is multiplied (full_fetch_* / full_stage_*).
// full_lp: the wave's accumulator is 16 frames x 16 NT outputs y[n][m] (4 NT doubles per lane); the squares are summed over the NT tiles
// in ascending order within a lane, then over the 16 lanes of a frame by a butterfly, which leaves every lane the same bits.
// Pass B: Z[n][:] = [1, X[n][:]] has D + 1 <= 16 NT columns and Z' diag(pp) Z holds stat0 (corner), stat1 (column 0) and stat2; its
// NT (NT + 1) / 2 tiles (i, j <= i) of 16 x 16 go round the four waves, A = pp Z[:, tile i], B = Z[:, tile j], k = the 64 frames.  Order
// 1 runs the tiles (i, 0) alone.  A diagonal tile's upper half is not stored: stat2 is the lower triangle and its mirror image.
#include "../../include/sidekit_amd/gmm_full.h"
#include "gmm_tile.h"
#include "kernels.h"

namespace sk {

__host__ __device__ inline int full_kp(int D) { return (D + 3) & ~3; }
__host__ __device__ inline int full_mld(int D) { return full_kp(D) + 1; }
__host__ __device__ inline size_t full_lds(int D, int nt) { return (size_t)(GT * gmm_xld(D) + 16 * nt * full_mld(D) + full_kp(D) + GT) * 8; }

// The cut of a segment of `len` frames of a mixture of C components (the header's slabs(L, C)) and a slab's length
__host__ __device__ inline long full_slabs(long len, int C) {
  long cap = SC_GMM_FULL_SLAB_TARGET / C;
  cap = cap < 1 ? 1 : (cap > SC_GMM_MAX_SLABS ? SC_GMM_MAX_SLABS : cap);
  const long n = (len + SC_GMM_SLAB_FRAMES - 1) / SC_GMM_SLAB_FRAMES;
  return n < 1 ? 1 : (n > cap ? cap : n);
}
__host__ __device__ inline long full_slab_len(long len, int C) {
  const long n = full_slabs(len, C), s = (len + n - 1) / n;
  return s < GT ? GT : (s + GT - 1) / GT * GT;
}
// Slab i's rows of a segment, within the segment's own; empty (begin >= end) for i >= full_slabs(seg.len(), C)
__device__ inline GmmRows full_slab(GmmRows seg, int i, int C) {
  const long sl = full_slab_len(seg.len(), C), b = seg.begin + i * sl;
  return {b < seg.end ? b : seg.end, b + sl < seg.end ? b + sl : seg.end};
}

// M[c] and mu[c] into Ms ([16 nt][mld], zeros beyond D by assignment: nothing is read for them) and mus ([Kp]).  One wave per row.
__device__ inline void full_load_component(const double* __restrict__ Mc, const double* __restrict__ muc, int D, int nt, double* Ms, double* mus) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kp = full_kp(D), mld = full_mld(D);
  for (int m = wave; m < 16 * nt; m += 4) {
    const double* src = Mc + (long)m * D;
    for (int k = lane; k < mld; k += 64) {
      double v = 0.0;
      if (m < D && k < D) v = src[k];
      Ms[m * mld + k] = v;
    }
  }
  for (int k = threadIdx.x; k < kp; k += 256) mus[k] = k < D ? muc[k] : 0.0;
}

// The same load in two halves, so that the next operand is on its way from memory while the current one is multiplied: fetch issues all
// of a thread's loads into registers (4 NT rows per wave, KI = ceil(NT / 4) columns per lane: 16 NT >= Kp), stage writes them to LDS.
// Ms's padding column (k = Kp) is never read and is left as it is.
template <int NT>
__device__ inline void full_fetch_component(const double* __restrict__ Mc, const double* __restrict__ muc, int D, double (&rm)[4 * NT][(NT + 3) / 4],
                                            double& rmu) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4 * NT; ++i) {
    const int m = wave + 4 * i;
#pragma unroll
    for (int j = 0; j < (NT + 3) / 4; ++j) {
      const int k = lane + 64 * j;
      rm[i][j] = m < D && k < D ? Mc[(long)m * D + k] : 0.0;
    }
  }
  rmu = (int)threadIdx.x < D ? muc[threadIdx.x] : 0.0;
}
template <int NT>
__device__ inline void full_stage_component(const double (&rm)[4 * NT][(NT + 3) / 4], double rmu, int D, double* Ms, double* mus) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kp = full_kp(D), mld = full_mld(D);
#pragma unroll
  for (int i = 0; i < 4 * NT; ++i) {
    const int m = wave + 4 * i;
#pragma unroll
    for (int j = 0; j < (NT + 3) / 4; ++j) {
      const int k = lane + 64 * j;
      if (k < kp) Ms[m * mld + k] = rm[i][j];
    }
  }
  if ((int)threadIdx.x < kp) mus[threadIdx.x] = rmu;
}
// Frames [f0, f0 + nvalid) of X likewise (gmm_load_frames in two halves: 16 rows per wave, KI columns per lane: 64 KI >= D | 1)
template <int NT, typename T>
__device__ inline void full_fetch_frames(const T* __restrict__ X, int D, long f0, int nvalid, T (&rx)[16][(NT + 3) / 4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i;
#pragma unroll
    for (int j = 0; j < (NT + 3) / 4; ++j) {
      const int d = lane + 64 * j;
      rx[i][j] = r < nvalid && d < D ? X[(f0 + r) * D + d] : (T)0;
    }
  }
}
template <int NT, typename T>
__device__ inline void full_stage_frames(const T (&rx)[16][(NT + 3) / 4], double* Xs, int xld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i;
#pragma unroll
    for (int j = 0; j < (NT + 3) / 4; ++j) {
      const int d = lane + 64 * j;
      if (d < xld) Xs[r * xld + d] = (double)rx[i][j];
    }
  }
}

// lp[r] = gc - 0.5 sum_m (sum_k Ms[m][k] (Xs[f][k] - mus[k]))^2 for the lane's frames f = 16 wave + (lane >> 4) + 4 r; the 16 lanes of a
// frame end with the same bits.  No barrier inside: Xs, Ms and mus are complete when it is called.
template <int NT>
__device__ inline void full_lp(const double* Xs, int xld, const double* Ms, const double* mus, int D, double gc, double (&lp)[4]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lk = lane >> 4, kp = full_kp(D), mld = full_mld(D);
  const double* xr = Xs + (wave * 16 + lr) * xld;
  f64x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < kp; k0 += 4) {
    const int k = k0 + lk;
    const double a = k < D ? xr[k] - mus[k] : 0.0;
    double b[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) b[j] = Ms[(j * 16 + lr) * mld + k];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < NT; ++j) q += acc[j][r] * acc[j][r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) q += __shfl_xor(q, o);
    lp[r] = gc - 0.5 * q;
  }
}

// ---- pass A ------------------------------------------------------------------------------------------------------------------------
// grid: x = frame tile.  The workgroup walks the components in ascending order, one matrix in LDS at a time; a lane keeps an online
// log-sum-exp state for each of its four frames (the 16 lanes of a frame hold the same state; lane & 15 == 0 stores).
// Bounds: frames beyond N are zero rows whose lse and lp are not stored.
template <int NT, typename T>
__global__ __launch_bounds__(256) void gmm_full_loglik_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                              const double* __restrict__ M, const double* __restrict__ g, int C,
                                                              double* __restrict__ lse, double* __restrict__ lp) {
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Ms = Xs + GT * xld;
  double* mus = Ms + 16 * NT * full_mld(D);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const long f0 = (long)blockIdx.x * GT;
  const int nvalid = N - f0 < GT ? (int)(N - f0) : GT;
  gmm_load_frames(X, D, f0, nvalid, Xs, xld);
  double Mx[4], Sx[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { Mx[r] = -INFINITY; Sx[r] = 0.0; }
  double rm[4 * NT][(NT + 3) / 4], rmu;
  full_fetch_component<NT>(M, mu, D, rm, rmu);
  for (int c = 0; c < C; ++c) {
    __syncthreads();   // every wave is done with the previous component
    full_stage_component<NT>(rm, rmu, D, Ms, mus);
    __syncthreads();
    if (c + 1 < C) full_fetch_component<NT>(M + (long)(c + 1) * D * D, mu + (long)(c + 1) * D, D, rm, rmu);   // in flight during the multiply
    double v[4];
    full_lp<NT>(Xs, xld, Ms, mus, D, g[c], v);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int fr = wave * 16 + lk + 4 * r;
      if (lp && lr == 0 && fr < nvalid) lp[(f0 + fr) * C + c] = v[r];
      lse_add(Mx[r], Sx[r], v[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int fr = wave * 16 + lk + 4 * r;
    if (lr == 0 && fr < nvalid) lse[f0 + fr] = lse_value(Mx[r], Sx[r]);
  }
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------------
// grid: x = (segment * nslab + slab) * C + component.  The component's matrix is loaded once; per frame tile of its slab (tiles start
// at the slab's first frame) the workgroup recomputes lp, forms pp = exp(lp - lse[n]) -- 0 by assignment for a frame outside the slab,
// whose lse is not read, and for a frame whose lse is -inf -- and accumulates the tiles of Z' diag(pp) Z it owns.  The partial goes to
// part0/1/2 at (slab * S + segment): with one slab per segment these are the outputs themselves, otherwise workspace that slab_reduce
// joins in slab order.  A slab beyond the segment's own cut (the grid is sized for the longest segment) multiplies nothing and stores zeros.
// Bounds: the slab's rows lie within [0, N] (gmm_segment, full_slab); frames beyond the slab's end are zero rows; a column of Z beyond D
// is zero by assignment; stores are guarded by the row's and the column's range.
template <int NT, typename T>
__global__ __launch_bounds__(256) void gmm_full_stats_kernel(const T* __restrict__ X, long N, int D, const double* __restrict__ mu,
                                                             const double* __restrict__ M, const double* __restrict__ g, int C,
                                                             const double* __restrict__ lse, const int* __restrict__ seg_off, int S, long max_len,
                                                             int nslab, int order, double* __restrict__ part0, double* __restrict__ part1,
                                                             double* __restrict__ part2) {
  constexpr int TT = NT * (NT + 1) / 2, SL = (TT + 3) / 4;   // the tiles of the lower triangle, and a wave's share of them
  extern __shared__ __attribute__((aligned(16))) double gmm_smem[];
  const int xld = gmm_xld(D);
  double* Xs = gmm_smem;
  double* Ms = Xs + GT * xld;
  double* mus = Ms + 16 * NT * full_mld(D);
  double* Ps = mus + full_kp(D);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const int c = blockIdx.x % C, ss = blockIdx.x / C, seg = ss / nslab, slab = ss % nslab;
  const GmmRows rows = full_slab(gmm_segment(seg_off, seg, N, max_len), slab, C);
  const double gc = g[c];
  full_load_component(M + (long)c * D * D, mu + (long)c * D, D, NT, Ms, mus);
  f64x4 st[SL];
  int ti[SL], tj[SL];
  bool on[SL];
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    st[s] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int t = s * 4 + wave;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti[s] = i;
    tj[s] = t - i * (i + 1) / 2;
    on[s] = t < TT && (order == 2 || tj[s] == 0);
  }
  T rx[16][(NT + 3) / 4];
  if (rows.begin < rows.end) full_fetch_frames<NT, T>(X, D, rows.begin, rows.end - rows.begin < GT ? (int)(rows.end - rows.begin) : GT, rx);
  for (long t0 = rows.begin; t0 < rows.end; t0 += GT) {
    const int nvalid = rows.end - t0 < GT ? (int)(rows.end - t0) : GT;
    __syncthreads();   // every wave is done with the previous tile's Xs and Ps
    full_stage_frames<NT, T>(rx, Xs, xld);
    __syncthreads();   // Xs is complete (and, the first time, Ms and mus)
    if (t0 + GT < rows.end)   // the next tile is in flight during this one's arithmetic
      full_fetch_frames<NT, T>(X, D, t0 + GT, rows.end - t0 - GT < GT ? (int)(rows.end - t0 - GT) : GT, rx);
    double v[4];
    full_lp<NT>(Xs, xld, Ms, mus, D, gc, v);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int fr = wave * 16 + lk + 4 * r;
      double p = 0.0;
      if (fr < nvalid) {
        const double l = lse[t0 + fr];
        if (l > -INFINITY) p = exp(v[r] - l);
      }
      if (lr == 0) Ps[fr] = p;
    }
    __syncthreads();
#pragma unroll 2
    for (int kk = 0; kk < GT; kk += 4) {
      const double p = Ps[kk + lk];
      const double* xrow = Xs + (kk + lk) * xld;
#pragma unroll
      for (int s = 0; s < SL; ++s) {
        if (!on[s]) continue;
        const int ci = ti[s] * 16 + lr, cj = tj[s] * 16 + lr;
        const double zi = ci == 0 ? 1.0 : (ci <= D ? xrow[ci - 1] : 0.0);
        const double zj = cj == 0 ? 1.0 : (cj <= D ? xrow[cj - 1] : 0.0);
        st[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(p * zi, zj, st[s], 0, 0, 0);
      }
    }
  }
  const long row = ((long)slab * S + seg) * C + c;
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    if (!on[s]) continue;
    const int cj = tj[s] * 16 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ri = ti[s] * 16 + lk + 4 * r;
      if (ri > D || cj > ri) continue;   // beyond Z, or the upper half of a diagonal tile
      const double val = st[s][r];
      if (cj == 0) {
        if (ri == 0) part0[row] = val;
        else part1[row * D + ri - 1] = val;
      } else if (order == 2) {
        double* s2 = part2 + row * D * D;
        s2[(long)(ri - 1) * D + cj - 1] = val;
        if (ri != cj) s2[(long)(cj - 1) * D + ri - 1] = val;
      }
    }
  }
}

template <int NT, typename T>
static int launch_full_loglik_nt(const T* X, long N, int D, const double* mu, const double* M, const double* g, int C, double* lse, double* lp,
                                 hipStream_t st) {
  const size_t lds = full_lds(D, NT);
  SK_TRY(gmm_allow_lds(gmm_full_loglik_kernel<NT, T>, lds));
  hipLaunchKernelGGL((gmm_full_loglik_kernel<NT, T>), dim3((unsigned)((N + GT - 1) / GT)), dim3(256), lds, st, X, N, D, mu, M, g, C, lse, lp);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <int NT, typename T>
static int launch_full_stats_nt(const T* X, long N, int D, const double* mu, const double* M, const double* g, int C, const double* lse,
                                const int* seg_off, int S, long max_len, int nslab, int order, double* p0, double* p1, double* p2, hipStream_t st) {
  const size_t lds = full_lds(D, NT);
  SK_TRY(gmm_allow_lds(gmm_full_stats_kernel<NT, T>, lds));
  hipLaunchKernelGGL((gmm_full_stats_kernel<NT, T>), dim3((unsigned)((long)S * nslab * C)), dim3(256), lds, st, X, N, D, mu, M, g, C, lse, seg_off, S,
                     max_len, nslab, order, p0, p1, p2);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

// NT = D / 16 + 1 tiles of 16 cover the D + 1 columns of Z (and the D outputs of M)
#define FULL_BY_NT(CALL)                \
  switch (D / 16 + 1) {                 \
    case 1: return CALL(1);             \
    case 2: return CALL(2);             \
    case 3: return CALL(3);             \
    case 4: return CALL(4);             \
    case 5: return CALL(5);             \
    case 6: return CALL(6);             \
    default: return CALL(7);            \
  }

template <typename T>
static int launch_full_loglik(const T* X, long N, int D, const double* mu, const double* M, const double* g, int C, double* lse, double* lp,
                              hipStream_t st) {
#define FULL_LOGLIK(NT) (launch_full_loglik_nt<NT, T>(X, N, D, mu, M, g, C, lse, lp, st))
  FULL_BY_NT(FULL_LOGLIK)
#undef FULL_LOGLIK
}

template <typename T>
static int launch_full_stats_kernel(const T* X, long N, int D, const double* mu, const double* M, const double* g, int C, const double* lse,
                                    const int* seg_off, int S, long max_len, int order, const GmmStatParts& p, hipStream_t st) {
#define FULL_STATS(NT) (launch_full_stats_nt<NT, T>(X, N, D, mu, M, g, C, lse, seg_off, S, max_len, p.nslab, order, p.p0, p.p1, p.p2, st))
  FULL_BY_NT(FULL_STATS)
#undef FULL_STATS
}

template <typename T>
static int launch_full_stats(const T* X, long N, int D, const double* mu, const double* M, const double* g, int C, const double* lse,
                             const int* seg_off, int S, long max_len, int order, double* stat0, double* stat1, double* stat2, double* llk,
                             hipStream_t st) {
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);   // held, once taken, until this function returns (see plda_workspace_locked)
  const int nslab = (int)full_slabs(max_len, C);
  const long n0 = (long)S * C, n1 = n0 * D, n2 = order == 2 ? n1 * D : 0;
  GmmStatParts p = {nslab, n0, n1, n2, stat0, stat1, stat2, stat0, stat1, stat2};
  if (nslab > 1) {
    void* ws = nullptr;
    lock.lock();
    SK_TRY(plda_workspace_locked(st, (size_t)nslab * (n0 + n1 + n2) * 8, &ws));
    p.p0 = (double*)ws;
    p.p1 = p.p0 + nslab * n0;
    p.p2 = p.p1 + nslab * n1;
  }
  SK_TRY(launch_full_stats_kernel(X, N, D, mu, M, g, C, lse, seg_off, S, max_len, order, p, st));
  return gmm_stats_finish(p, lse, N, seg_off, S, max_len, llk, st);
}

static int full_check(const char* who, const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_M,
                      const double* d_g, int32_t C) {
  SK_CHECK(d_X && d_mu && d_M && d_g, SK_EARG, "%s: null argument", who);
  SK_TRY(gmm_check_frames(who, d_X, x_dtype, N, D, C));
  SK_CHECK(D <= SC_GMM_FULL_MAX_D, SK_EARG, "%s: D=%d with at most %d", who, D, SC_GMM_FULL_MAX_D);
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_gmm_full_frame_loglik(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_M, const double* d_g,
                             int32_t C, double* d_lse, double* d_lp, void* stream) {
  SK_TRY(full_check("sc_gmm_full_frame_loglik", d_X, x_dtype, N, D, d_mu, d_M, d_g, C));
  SK_CHECK(d_lse, SK_EARG, "sc_gmm_full_frame_loglik: null argument");
  if (x_dtype == XT_F32) return launch_full_loglik((const float*)d_X, (long)N, D, d_mu, d_M, d_g, C, d_lse, d_lp, (hipStream_t)stream);
  return launch_full_loglik((const double*)d_X, (long)N, D, d_mu, d_M, d_g, C, d_lse, d_lp, (hipStream_t)stream);
}

int sc_gmm_full_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_M, const double* d_g, int32_t C,
                      const double* d_lse, const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order, double* d_stat0, double* d_stat1,
                      double* d_stat2, double* d_llk, void* stream) {
  SK_TRY(full_check("sc_gmm_full_stats", d_X, x_dtype, N, D, d_mu, d_M, d_g, C));
  SK_CHECK(order == 1 || order == 2, SK_EARG, "sc_gmm_full_stats: order must be 1 or 2 (got %d)", order);
  SK_CHECK(d_lse && d_seg_off && d_stat0 && d_stat1 && (order == 1 || d_stat2), SK_EARG, "sc_gmm_full_stats: null argument");
  SK_TRY(gmm_check_segments("sc_gmm_full_stats", N, S, max_len));
  SK_CHECK((long long)S * full_slabs(max_len, C) * C <= 0x7fffffffLL, SK_EARG, "sc_gmm_full_stats: S=%d x %lld slabs x C=%d workgroups exceed the grid", S,
           (long long)full_slabs(max_len, C), C);
  if (x_dtype == XT_F32)
    return launch_full_stats((const float*)d_X, (long)N, D, d_mu, d_M, d_g, C, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1, d_stat2,
                             d_llk, (hipStream_t)stream);
  return launch_full_stats((const double*)d_X, (long)N, D, d_mu, d_M, d_g, C, d_lse, d_seg_off, S, (long)max_len, order, d_stat0, d_stat1, d_stat2,
                           d_llk, (hipStream_t)stream);
}

}  // extern "C"
