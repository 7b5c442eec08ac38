// What the top-C kernels share (gmm_topc.hip: scoring on the lists; gmm_topc_stats.hip: sparse posteriors; gmm_topc_em.hip: list
// refinement), one copy of each, device code only: the sum over a wave's 64 lanes and the f64 scalar broadcast; one list entry's operand
// (TopcRow), its fetch and the lane's term; the loop over a frame's list held in a register; the end of a tile of posteriors.  A frame's
// lp, lse and posterior have the same bits in all three files because they are formed by the same functions, in the same order.
#pragma once
#include "gmm_tile.h"

namespace sk {

// The sum of t over the wave's 64 lanes in every lane: the butterfly xor 32, 16, 8 .. 1.
__device__ inline double topc_wave_sum(double t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  return t;
}

// The sums of t[0 .. 4) over the wave's 64 lanes: lane l ends with the sum of t[l >> 4].  One butterfly that halves the models a lane
// carries as it goes (xor 32: two of four, xor 16: one of two, then xor 8 .. 1 on that one: 7 exchanges for 4 models).  Each model's
// tree is topc_wave_sum's (a + b is b + a bit for bit), wherever the model stands in the group: sum j has the bits topc_wave_sum(t[j]) has.
__device__ inline double topc_wave_sums(const double (&t)[4], int lane) {
  const bool h32 = lane & 32, h16 = lane & 16;
  double a0 = h32 ? t[2] : t[0], a1 = h32 ? t[3] : t[1];
  a0 += __shfl_xor(h32 ? t[0] : t[2], 32);
  a1 += __shfl_xor(h32 ? t[1] : t[3], 32);
  double v = h16 ? a1 : a0;
  v += __shfl_xor(h16 ? a0 : a1, 16);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Lane j's double in every lane (j wave-uniform): two scalar broadcasts.
__device__ inline double topc_em_readlane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// One list entry's operand at this lane's d (lane) and d + 64: the component (-1: struck out, nothing to add), its invcov values and
// the mean values of G models.
template <int G>
struct TopcRow { int c; double ic0, ic1, mu0[G], mu1[G]; };

// r <- the operand of component c (wave-uniform); model j's means are mu + j CD, j < nmod <= G, the others' stay 0.
// Bounds: c outside [0, C) is struck out before anything is read through it; a lane reads row c at d = lane < D and at d + 64 < D only.
template <int G>
__device__ inline void topc_fetch(int c, int C, int D, int lane, const double* __restrict__ invcov, const double* __restrict__ mu, long CD,
                                  int nmod, TopcRow<G>& r) {
  if (c < 0 || c >= C) c = -1;
  r.c = c;
  r.ic0 = r.ic1 = 0.0;
#pragma unroll
  for (int j = 0; j < G; ++j) r.mu0[j] = r.mu1[j] = 0.0;
  if (c < 0) return;
  const long row = (long)c * D;
  if (lane < D) {
    r.ic0 = invcov[row + lane];
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j < nmod) r.mu0[j] = mu[j * CD + row + lane];
  }
  if (lane + 64 < D) {   // the second pass over d, above 64
    r.ic1 = invcov[row + lane + 64];
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j < nmod) r.mu1[j] = mu[j * CD + row + lane + 64];
  }
}

// t[j] <- this lane's part of sum_d (x[d] - mu_j[c][d])^2 invcov[c][d]: d = lane, and d + 64 added to it where D > 64 (`two`).
// 0 for a lane beyond D: x, mu and invcov are 0 there.
template <int G>
__device__ inline void topc_terms(const TopcRow<G>& r, double x0, double x1, bool two, double (&t)[G]) {
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const double e0 = x0 - r.mu0[j];
    t[j] = e0 * e0 * r.ic0;
    if (two) {
      const double e1 = x1 - r.mu1[j];
      t[j] += e1 * e1 * r.ic1;
    }
  }
}

// The lp of one frame's list of n <= 64 entries, held in a register (lane j of `mine`: entry j), under one model: for j < n in order,
// sink(j, lp) with lp = -0.5 (sum_d (x[d] - mu[c][d])^2 invcov[c][d] + B[c]), c = entry j, the same value in every lane, or -INFINITY
// for an entry outside [0, C).  x0 / x1: the frame at d = lane and d + 64, 0 beyond D.  Per entry the component is wave-uniform, a row
// of invcov and of mu is one coalesced 8 D-byte load each, and the rows of entry j + 1 are fetched while entry j is reduced.
// Bounds: entries are read from the register for j < n only; topc_fetch has the rest.
template <typename Sink>
__device__ inline void topc_frame_lps(double x0, double x1, int mine, int n, int lane, int D, const double* __restrict__ mu,
                                      const double* __restrict__ invcov, const double* __restrict__ B, int C, Sink sink) {
  const bool two = D > 64;
  TopcRow<1> cur, nxt;
  topc_fetch<1>(__builtin_amdgcn_readlane(mine, 0), C, D, lane, invcov, mu, 0, 1, cur);
  for (int j = 0; j < n; ++j) {
    if (j + 1 < n) topc_fetch<1>(__builtin_amdgcn_readlane(mine, j + 1), C, D, lane, invcov, mu, 0, 1, nxt);
    double lp = -INFINITY;
    if (cur.c >= 0) {
      double t[1];
      topc_terms<1>(cur, x0, x1, two, t);
      lp = -0.5 * (topc_wave_sum(t[0]) + B[cur.c]);
    }
    sink(j, lp);
    if (j + 1 < n) cur = nxt;
  }
}

// The end of a tile of posteriors.  Lp[f][0 .. K) holds the lp of frame f0 + f's list, f < nvalid <= GT; fl is GT doubles of LDS.
// Thread f folds its frame's K values in list order with lse_add and writes lse[f0 + f]; thread (f, k) then writes
// post[f0 + f][k] = exp(lp - lse), 0 by assignment for -inf and nan.  Two barriers, the first before Lp is read: every thread of the
// workgroup calls this or none does.  Bounds: Lp, lse and post are indexed with f < nvalid and k < K.
__device__ inline void topc_fold_and_posteriors(const double* Lp, double* fl, long f0, int nvalid, int K, double* __restrict__ post,
                                                double* __restrict__ lse) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < nvalid) {
    double m = -INFINITY, s = 0.0;
    for (int k = 0; k < K; ++k) lse_add(m, s, Lp[tid * K + k]);
    const double l = lse_value(m, s);
    fl[tid] = l;
    lse[f0 + tid] = l;
  }
  __syncthreads();
  for (int e = tid; e < nvalid * K; e += 256) {
    const double lp = Lp[e], l = fl[e / K];
    post[f0 * K + e] = lp > -INFINITY && l > -INFINITY ? exp(lp - l) : 0.0;
  }
}

}  // namespace sk
