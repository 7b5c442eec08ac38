// Joint factor analysis (sidekit/statserver.py:1376-1949, sidekit/jfa_scoring.py): the passes over the N x (C D) first-order statistics
// that lie around the total-variability posterior (ivector.hip).  Two entry points (include/sidekit_amd/jfa.h):
//   sc_jfa_shift     out = (stat1 - stat0 (mean + H[row] W')) * scale: the shift by the hidden variables, the centring and the whitening
//                    in one pass (the reference's duplicate_y, Vy / Ux, subtract_weighted_stat1, whiten_stat1 and their StatServer copies)
//   sc_jfa_map_acc   the two accumulators of an E-step of the diagonal MAP term (estimate_map's loop over models)
// float64 throughout, no floating-point atomics, every sum in a fixed order.
//
// sc_jfa_shift is the A . B^T form of the f64 tile (dgemm_tile.h) with M = sessions, N = C D, K = R and an epilogue that reads stat1 and
// stat0: an output element belongs to one lane, which reads it and writes it (so out may be stat1), and its low-rank sum runs over r in
// the k-order of the tile wherever it falls in its 128 x 128 tile, so a session's bits do not depend on N or on its row.  The factors are
// gathered through `row` into the sc_* workspace first (N x R doubles, a row outside [0, Nh) as zeros), which keeps the tile's own
// loaders; without `row` the tile zero-fills the sessions beyond Nh itself.
//
// sc_jfa_map_acc: one thread per column (consecutive lanes read consecutive doubles of a row), grid y = slabs of SC_JFA_MAP_SLAB rows
// added in row order; with more than one slab the partial sums go to the workspace and are added in slab order.
#include "../../include/sidekit_amd/jfa.h"
#include "dgemm_tile.h"
#include "kernels.h"

namespace sk {

// grid: x = session tile, y = column tile (the workgroups of one W tile are neighbours).  Bounds: the tile zero-fills beyond Mh rows of H,
// CD rows of W and R; loads and stores of the epilogue are guarded by m < N and n < CD, and n < CD gives n / D < C.
__global__ __launch_bounds__(256, 2) void jfa_shift_kernel(const double* stat1, const double* __restrict__ stat0, int N, int C, int D,
                                                           const double* __restrict__ W, const double* __restrict__ H, int Mh, int R,
                                                           const double* __restrict__ mean, const double* __restrict__ scale, double* out) {
  constexpr int WT = 4, TL = 32 * WT;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  const dgemm_lanes<WT> at;
  const int m0 = blockIdx.x * TL, n0 = blockIdx.y * TL, CD = C * D;
  f64x4 acc[WT][WT];
  if (R > 0) {
    dgemm_tile<WT, false>(H, W, Mh, CD, R, m0, n0, As, Bs, acc);
  } else {
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  int comp[WT];
  double mu[WT], sc[WT];
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const int n = n0 + at.col(j);
    const bool in = n < CD;
    comp[j] = in ? n / D : 0;
    mu[j] = in && mean ? mean[n] : 0.0;
    sc[j] = in && scale ? scale[n] : 1.0;
  }
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + at.row(i, q);
      if (m >= N) continue;
      const double* cnt = stat0 + (long)m * C;
      const long base = (long)m * CD;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + at.col(j);
        if (n >= CD) continue;
        const double v = stat1[base + n] - cnt[comp[j]] * (mu[j] + acc[i][j][q]);
        out[base + n] = v * sc[j];
      }
    }
}

// Hg[i] = H[row[i]], zeros when row[i] is outside [0, Nh): one thread per element of the N x R output
__global__ __launch_bounds__(256) void jfa_gather_kernel(const double* __restrict__ H, int Nh, int R, const int* __restrict__ row, long total,
                                                         double* __restrict__ Hg) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= total) return;
  const long i = e / R;
  const int r = (int)(e - i * R), src = row[i];
  Hg[e] = src >= 0 && src < Nh ? H[(long)src * R + r] : 0.0;
}

// grid: x = 256 columns, y = slab of SC_JFA_MAP_SLAB rows.  pa / pc: the outputs themselves (one slab) or [slab][CD] partial sums.
__global__ __launch_bounds__(256) void jfa_map_acc_kernel(const double* __restrict__ stat0, const double* __restrict__ stat1, int M, int C, int D,
                                                          const double* __restrict__ Dv, const double* __restrict__ Sigma, double* __restrict__ pa,
                                                          double* __restrict__ pc) {
  const int CD = C * D, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= CD) return;
  const int c = k / D, first = blockIdx.y * SC_JFA_MAP_SLAB, last = first + SC_JFA_MAP_SLAB < M ? first + SC_JFA_MAP_SLAB : M;
  const double d = Dv[k], s = Sigma[k], d2 = d * d;
  double a = 0.0, cc = 0.0;
  for (int i = first; i < last; ++i) {
    const double n = stat0[(long)i * C + c], f = stat1[(long)i * CD + k];
    const double L = 1.0 + n * d2 / s;
    const double e = f * d / (L * s);
    a += (1.0 / L + e * e) * n;
    cc += e * f;
  }
  pa[(long)blockIdx.y * CD + k] = a;
  pc[(long)blockIdx.y * CD + k] = cc;
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_jfa_shift(const double* d_stat1, const double* d_stat0, int32_t N, int32_t C, int32_t D, const double* d_W, const double* d_H,
                 int32_t Nh, int32_t R, const int32_t* d_row, const double* d_mean, const double* d_scale, double* d_out, void* stream) {
  SK_CHECK(d_stat1 && d_stat0 && d_out, SK_EARG, "sc_jfa_shift: null argument");
  SK_CHECK(N >= 1 && C >= 1 && D >= 1 && (int64_t)C * D <= 65535LL * 128, SK_EARG, "sc_jfa_shift: bad sizes (N=%d, C=%d, D=%d)", N, C, D);
  SK_CHECK(R >= 0 && R <= SC_TV_MAX_RANK, SK_EARG, "sc_jfa_shift: R=%d is outside [0, %d]", R, SC_TV_MAX_RANK);
  SK_CHECK(R > 0 ? (d_W && d_H && Nh >= 1) : (!d_W && !d_H), SK_EARG,
           "sc_jfa_shift: d_W, d_H and Nh >= 1 come with R > 0, and neither d_W nor d_H with R = 0 (R=%d, Nh=%d)", R, Nh);
  hipStream_t st = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);
  const double* factors = d_H;
  int rows = N < Nh ? N : Nh;
  if (R > 0 && d_row) {
    void* ws = nullptr;
    lock.lock();   // held until both launches are enqueued (see plda_workspace_locked)
    SK_TRY(plda_workspace_locked(st, (size_t)N * R * 8, &ws));
    const long total = (long)N * R;
    hipLaunchKernelGGL(jfa_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_H, Nh, R, d_row, total, (double*)ws);
    SK_HIP(hipGetLastError());
    factors = (const double*)ws;
    rows = N;
  }
  const int CD = C * D;
  hipLaunchKernelGGL(jfa_shift_kernel, dim3(cdiv(N, 128), cdiv(CD, 128)), dim3(256), 0, st, d_stat1, d_stat0, N, C, D, d_W, factors, rows, R, d_mean,
                     d_scale, d_out);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sc_jfa_map_acc(const double* d_stat0, const double* d_stat1, int32_t M, int32_t C, int32_t D, const double* d_D, const double* d_Sigma,
                   double* d_A, double* d_Cacc, void* stream) {
  SK_CHECK(d_stat0 && d_stat1 && d_D && d_Sigma && d_A && d_Cacc, SK_EARG, "sc_jfa_map_acc: null argument");
  SK_CHECK(M >= 1 && C >= 1 && D >= 1 && (int64_t)C * D <= 0x7fffffffLL && cdiv(M, SC_JFA_MAP_SLAB) <= 65535, SK_EARG,
           "sc_jfa_map_acc: bad sizes (M=%d, C=%d, D=%d)", M, C, D);
  hipStream_t st = (hipStream_t)stream;
  const int CD = C * D, nslab = cdiv(M, SC_JFA_MAP_SLAB);
  double *pa = d_A, *pc = d_Cacc;
  std::unique_lock<std::mutex> lock(g_plda_mu, std::defer_lock);
  if (nslab > 1) {
    void* ws = nullptr;
    lock.lock();   // held until the launches are enqueued (see plda_workspace_locked)
    SK_TRY(plda_workspace_locked(st, (size_t)2 * nslab * CD * 8, &ws));
    pa = (double*)ws;
    pc = pa + (size_t)nslab * CD;
  }
  hipLaunchKernelGGL(jfa_map_acc_kernel, dim3(cdiv(CD, 256), nslab), dim3(256), 0, st, d_stat0, d_stat1, M, C, D, d_D, d_Sigma, pa, pc);
  SK_HIP(hipGetLastError());
  if (nslab > 1) {
    SK_TRY(launch_slab_reduce(pa, nslab, CD, d_A, st));
    SK_TRY(launch_slab_reduce(pc, nslab, CD, d_Cacc, st));
  }
  return SK_OK;
}

}  // extern "C"
