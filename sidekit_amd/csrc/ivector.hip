// Total variability (sidekit/factor_analyser.py:51-163, 433-828): what lies between the GEMMs of the i-vector E-step.  Two entry points
// (include/sidekit_amd/ivector.h):
//   sc_tv_gram        G[c] = F_c' F_c for every component, packed upper triangles (once per EM iteration / extraction)
//   sc_tv_posterior   per session: Lambda = I + unpack(Lp), inv_lambda, e_h = inv_lambda b, E_hh = inv_lambda + e_h e_h' (packed, and / or its diagonal)
// The products around them (Lp = stat0 . G, B = S_w . F, the accumulators) are sc_dgemm_nn / sc_gemm_tn (plda_train.hip).  float64
// throughout, no floating-point atomics, every sum in a fixed order.
//
// sc_tv_posterior: one workgroup of 256 threads per session.  The session's matrix is ONE packed upper triangle T of P = R (R + 1) / 2
// doubles in LDS, in the order it has in memory (row i holds columns i .. R - 1 contiguously, (i, k) at rb(i) + k with
// rb(i) = i R - i (i + 1) / 2), from its single load to its single store; at R = 192 a second triangle would not fit, so every step works
// in place.  Beside it: three R-vectors -- vec (the row or column a step replaces, copied before it is overwritten), bs (b), es (e_h) --
// and 2 x 256 doubles of partial sums.
//   1. Cholesky Lambda = U' U, row k after row k - 1: U[k][j] = (T[k][j] - sum_m<k U[m][k] U[m][j]) / U[k][k] for j >= k;
//      U[m][k] is one address for the lanes of a chunk (broadcast), U[m][j] consecutive ones (no bank conflict).
//   2. V = U^-1, column j after column j - 1 (LAPACK's dtrti2): V[i][j] = -V[j][j] sum_{i <= k < j} V[i][k] U[k][j]; column j of U goes
//      through vec.
//   3. inv_lambda = V V', row i after row i - 1: entry (i, j >= i) = sum_{k >= j} V[i][k] V[j][k], row i of V through vec; rows above i
//      are already replaced and no longer needed.
//   4. e_h = inv_lambda b: for entry i, column i down to the diagonal, then row i.
//   5. E_hh = inv_lambda + e_h e_h' in place, then the stores.
// Every step of 1 to 4 is n dot products (n = R - k, j, R - i, R) of up to R terms.  The 256 threads are dealt as Q = min(16, 256 / n)
// chunks per dot: thread t works on output t mod n, chunk t / n, a contiguous Q-th of that dot's terms; the partial sums go through LDS
// and the thread of chunk 0 adds them in chunk order.  Q and the cut are functions of R and the step alone, so a session's bits do not
// depend on where it lies.  A barrier separates the reads and the writes of every stage (two per row in step 1, three in steps 2 and 3).
// The dots are compensated (Dot2 of Ogita, Rump and Oishi: the exact product by fma, the exact sum by TwoSum, the errors gathered in
// a second double), ten FP64 operations per term where a plain dot has one, which makes every dot as accurate as one computed in twice
// the precision and rounded once; a chunk is four interleaved sums (tv_dot), so that eight LDS reads are in flight instead of one chain
// of dependent operations.  The inverse is formed from the inverse of the factor, whose residual Lambda X - I carries three stacked
// dot-product errors of R terms each: with plain dots it was 5 to 12 times the residual of a column-by-column LU solve at
// cond(Lambda) = 1e7 (numpy emulation of this kernel, R = 17 .. 64); with compensated dots what is left is the rounding of the stored
// entries of U and V.  About R^3 / 2 terms and twice as many 8-byte LDS reads per session.
#include <cmath>

#include "../../include/sidekit_amd/ivector.h"
#include "dgemm_tile.h"
#include "tv_common.h"

namespace sk {

constexpr int TV_THREADS = 256, TV_MAX_CHUNKS = 16;

// s + c = the sum so far as if added in twice the precision (the file is built with -ffp-contract=off: nothing here is fused or reordered)
struct Dot2 {
  double s, c;
  __device__ inline explicit Dot2(double start = 0.0) : s(start), c(0.0) {}
  __device__ inline void add(double a, double b) {
    const double p = a * b, e = fma(a, b, -p);   // a b = p + e exactly
    const double t = s + p, z = t - s;
    c += ((s - (t - z)) + (p - z)) + e;          // s + p = t + (...) exactly
    s = t;
  }
  __device__ inline void merge(double os, double oc) {
    const double t = s + os, z = t - s;
    c += ((s - (t - z)) + (os - z)) + oc;
    s = t;
  }
  __device__ inline double value() const { return s + c; }
};

// start + sum_{lo <= i < hi} a(i) b(i): four interleaved compensated sums (term lo + i goes to sum i mod 4, the tail to sum 0), merged as
// (0 + 1) + (2 + 3).  The order is a function of hi - lo alone.
template <typename FA, typename FB>
__device__ inline Dot2 tv_dot(int lo, int hi, FA a, FB b, double start) {
  Dot2 d0(start), d1, d2, d3;
  int i = lo;
  for (; i + 4 <= hi; i += 4) {
    const double a0 = a(i), b0 = b(i), a1 = a(i + 1), b1 = b(i + 1), a2 = a(i + 2), b2 = b(i + 2), a3 = a(i + 3), b3 = b(i + 3);
    d0.add(a0, b0);
    d1.add(a1, b1);
    d2.add(a2, b2);
    d3.add(a3, b3);
  }
  for (; i < hi; ++i) d0.add(a(i), b(i));
  d0.merge(d1.s, d1.c);
  d2.merge(d3.s, d3.c);
  d0.merge(d2.s, d2.c);
  return d0;
}

// The deal of a step with n >= 1 dots: thread t -> output o = t mod n, chunk q = t / n of Q = min(TV_MAX_CHUNKS, 256 / n); on = it has one.
struct TvDeal {
  int o, q, Q;
  bool on;
  __device__ inline TvDeal(int n, int tid) {
    Q = TV_THREADS / n;
    if (Q > TV_MAX_CHUNKS) Q = TV_MAX_CHUNKS;
    q = tid / n;
    o = tid - q * n;
    on = q < Q;
  }
  // chunk q of a dot of L terms: [lo, hi), ceil(L / Q) terms each but the last ones
  __device__ inline void cut(int L, int& lo, int& hi) const {
    const int len = (L + Q - 1) / Q;
    lo = q * len < L ? q * len : L;
    hi = lo + len < L ? lo + len : L;
  }
};

// chunk 0's thread adds the chunks of output o (n outputs) in chunk order
__device__ inline double tv_join(const double* ps, const double* pc, int o, int n, int Q) {
  Dot2 d(ps[o]);
  d.c = pc[o];
  for (int q = 1; q < Q; ++q) d.merge(ps[o + q * n], pc[o + q * n]);
  return d.value();
}

// grid: x = component, y = upper tile (tm, tn >= tm) of the R x R output in row-major order of the pairs.  Bounds: the tile zero-fills
// beyond R and D; stores are guarded by m <= n < R.
__global__ __launch_bounds__(256, 4) void tv_gram_kernel(const double* __restrict__ F, int D, int R, double* __restrict__ G) {
  constexpr int WT = 2, TL = 64;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  __shared__ double cs[2 * TL];
  const dgemm_lanes<WT> at;
  const int nt = (R + TL - 1) / TL;
  int t = blockIdx.y, tm = 0;
  while (tm < nt - 1 && t >= nt - tm) { t -= nt - tm; ++tm; }
  const int m0 = tm * TL, n0 = (tm + t) * TL;
  const double* Fc = F + (long)blockIdx.x * D * R;
  double* Gc = G + (long)blockIdx.x * tv_packed(R);
  f64x4 acc[WT][WT];
  dgemm_tile<WT, true, true, double, double>(Fc, Fc, R, R, D, m0, n0, As, Bs, acc, nullptr, nullptr, nullptr, cs);
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + at.row(i, q);
      if (m >= R) continue;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + at.col(j);
        if (n < R && n >= m) Gc[tv_rb(m, R) + n] = acc[i][j][q];
      }
    }
}

// grid: x = session.  Lp and Ehh may be the same buffer (no __restrict__ on either): the row is in LDS before anything is stored.
// Bounds: every LDS index is (i, k) with i <= k < R, below R in a vector, or a thread number in the partial sums; global rows are
// session * P and session * R long.
__global__ __launch_bounds__(TV_THREADS) void tv_posterior_kernel(const double* Lp, const double* __restrict__ B, int R, double* __restrict__ Eh,
                                                                  double* Ehh, double* __restrict__ diag) {
  extern __shared__ __attribute__((aligned(16))) double tv_smem[];
  const int P = (int)tv_packed(R);
  double* T = tv_smem;
  double* vec = T + P;
  double* bs = vec + R;
  double* es = bs + R;
  double* ps = es + R;
  double* pc = ps + TV_THREADS;
  const int tid = threadIdx.x;
  const long session = blockIdx.x;
  {
    const double* src = Lp + session * P;
    for (int p = tid; p < P; p += TV_THREADS) T[p] = src[p];
    if (tid < R) bs[tid] = B[session * R + tid];
  }
  __syncthreads();
  if (tid < R) T[tv_rb(tid, R) + tid] += 1.0;
  __syncthreads();
  // 1. Lambda = U' U.  Output o of row k is column k + o; output 0 is the pivot, which every joining thread forms for itself.
  for (int k = 0; k < R; ++k) {
    const int n = R - k, rk = tv_rb(k, R);
    const TvDeal deal(n, tid);
    const int j = k + deal.o;
    if (deal.on) {
      int lo, hi;
      deal.cut(k, lo, hi);
      const Dot2 d = tv_dot(lo, hi, [&](int m) { return -T[tv_rb(m, R) + k]; }, [&](int m) { return T[tv_rb(m, R) + j]; },
                            deal.q == 0 ? T[rk + j] : 0.0);
      ps[tid] = d.s;
      pc[tid] = d.c;
    }
    __syncthreads();
    if (tid < n) {
      const double pivot = sqrt(tv_join(ps, pc, 0, n, deal.Q));
      T[rk + j] = tid == 0 ? pivot : tv_join(ps, pc, tid, n, deal.Q) / pivot;
    }
    __syncthreads();
  }
  // 2. V = U^-1.  Output o of column j is row o < j; thread 0 also writes the diagonal.
  for (int j = 0; j < R; ++j) {
    if (tid <= j) vec[tid] = T[tv_rb(tid, R) + j];
    __syncthreads();
    const int n = j > 0 ? j : 1;
    const TvDeal deal(n, tid);
    const int row = tv_rb(deal.o, R);
    if (deal.on && j > 0) {
      int lo, hi;
      deal.cut(j - deal.o, lo, hi);
      const double* a = T + row + deal.o;
      const double* b = vec + deal.o;
      const Dot2 d = tv_dot(lo, hi, [&](int k) { return a[k]; }, [&](int k) { return b[k]; }, 0.0);
      ps[tid] = d.s;
      pc[tid] = d.c;
    }
    __syncthreads();
    const double vjj = 1.0 / vec[j];
    if (tid < j) T[row + j] = -(tv_join(ps, pc, tid, n, deal.Q) * vjj);
    if (tid == 0) T[tv_rb(j, R) + j] = vjj;
    __syncthreads();
  }
  // 3. inv_lambda = V V'.  Output o of row i is column i + o; row i is read through vec only.
  for (int i = 0; i < R; ++i) {
    const int n = R - i, ri = tv_rb(i, R);
    if (tid < n) vec[i + tid] = T[ri + i + tid];
    __syncthreads();
    const TvDeal deal(n, tid);
    const int j = i + deal.o;
    if (deal.on) {
      int lo, hi;
      deal.cut(R - j, lo, hi);
      const double* a = vec + j;
      const double* b = (deal.o == 0 ? vec : T + tv_rb(j, R)) + j;
      const Dot2 d = tv_dot(lo, hi, [&](int k) { return a[k]; }, [&](int k) { return b[k]; }, 0.0);
      ps[tid] = d.s;
      pc[tid] = d.c;
    }
    __syncthreads();
    if (tid < n) T[ri + j] = tv_join(ps, pc, tid, n, deal.Q);
    __syncthreads();
  }
  // 4. e_h = inv_lambda b
  {
    const TvDeal deal(R, tid);
    const int i = deal.o, own = tv_rb(i, R);
    if (deal.on) {
      int lo, hi;
      deal.cut(R, lo, hi);
      const Dot2 d = tv_dot(lo, hi, [&](int j) { return T[j < i ? tv_rb(j, R) + i : own + j]; }, [&](int j) { return bs[j]; }, 0.0);
      ps[tid] = d.s;
      pc[tid] = d.c;
    }
    __syncthreads();
    if (tid < R) {
      const double e = tv_join(ps, pc, tid, R, deal.Q);
      es[tid] = e;
      Eh[session * R + tid] = e;
    }
  }
  __syncthreads();
  // 5. E_hh = inv_lambda + e_h e_h': one wave per row
  for (int i = tid >> 6; i < R; i += 4) {
    const int ri = tv_rb(i, R);
    const double ei = es[i];
    for (int j = i + (tid & 63); j < R; j += 64) T[ri + j] = fma(ei, es[j], T[ri + j]);
  }
  __syncthreads();
  if (Ehh) {
    double* dst = Ehh + session * P;
    for (int p = tid; p < P; p += TV_THREADS) dst[p] = T[p];
  }
  if (diag && tid < R) diag[session * R + tid] = T[tv_rb(tid, R) + tid];
}

// the launch of both Gram entries (sc_tv_gram here, sc_tvw_gram of ivector_wide.hip)
int tv_gram_launch(const double* d_F, int C, int D, int R, int nt, double* d_G, hipStream_t stream) {
  hipLaunchKernelGGL(tv_gram_kernel, dim3((unsigned)C, (unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, stream, d_F, D, R, d_G);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_tv_gram(const double* d_F, int32_t C, int32_t D, int32_t R, double* d_G, void* stream) {
  SK_CHECK(d_F && d_G, SK_EARG, "sc_tv_gram: null argument");
  SK_CHECK(C >= 1 && D >= 1 && R >= 1 && R <= SC_TV_MAX_RANK, SK_EARG, "sc_tv_gram: bad sizes (C=%d, D=%d, R=%d with at most %d)", C, D, R,
           SC_TV_MAX_RANK);
  const int nt = cdiv(R, 64);
  return tv_gram_launch(d_F, C, D, R, nt, d_G, (hipStream_t)stream);
}

int sc_tv_posterior(const double* d_Lp, const double* d_B, int32_t N, int32_t R, double* d_Eh, double* d_Ehh, double* d_diag, void* stream) {
  SK_CHECK(d_Lp && d_B && d_Eh, SK_EARG, "sc_tv_posterior: null argument");
  SK_CHECK(d_Ehh || d_diag, SK_EARG, "sc_tv_posterior: at least one of d_Ehh and d_diag is not null");
  SK_CHECK(N >= 1 && R >= 1 && R <= SC_TV_MAX_RANK, SK_EARG, "sc_tv_posterior: bad sizes (N=%d, R=%d with at most %d)", N, R, SC_TV_MAX_RANK);
  const size_t lds = (size_t)(tv_packed(R) + 3 * R + 2 * TV_THREADS) * 8;
  // more than 64 KB of dynamic LDS has to be allowed before the launch
  if (lds > 65536) SK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tv_posterior_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(tv_posterior_kernel, dim3((unsigned)N), dim3(TV_THREADS), lds, (hipStream_t)stream, d_Lp, d_B, R, d_Eh, d_Ehh, d_diag);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
