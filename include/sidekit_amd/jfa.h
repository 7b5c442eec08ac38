/* sidekit_amd/jfa.h -- the joint-factor-analysis extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Two entry points of the same library, under the same conventions (error classes, device pointers, the stream argument).  Like the
 * i-vector's they live in a header of their own, bound by a table of their own (sidekit_amd/_lib.py JFA_SIGNATURES): the core header
 * and its table are pinned symbol for symbol.
 *
 * JFA (sidekit/statserver.py:1376-1949, sidekit/jfa_scoring.py) models a super-vector as M = m + V y + U x + D z.  The E-step of its two
 * sub-space estimations is the total-variability posterior (ivector.h); what it adds are passes over the N x (C D) first-order
 * statistics, which the reference makes on whole copies of its StatServer.  These two calls are those passes.  float64 throughout.  No
 * floating-point atomics; every sum has a fixed order, so a call's bits depend on its arguments alone.  Arguments are checked (SK_EARG)
 * before anything is enqueued: null pointers, R outside [0, SC_TV_MAX_RANK], C, D, N or M below 1, a loading matrix without factors or
 * factors without a loading matrix. */
#ifndef SIDEKIT_AMD_JFA_H
#define SIDEKIT_AMD_JFA_H
#include "ivector.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shift by the hidden variables, the centring and the whitening of a batch of sessions in one pass (the reference's duplicate_y,
 * Vy / Ux, subtract_weighted_stat1 and whiten_stat1):
 *   d_out[i][k] = (d_stat1[i][k] - d_stat0[i][k / D] * (d_mean[k] + sum_r d_H[row[i]][r] * d_W[k][r])) * d_scale[k]
 * d_stat1, d_out: N x (C D); d_stat0: N x C; d_W: (C D) x R row-major; d_H: Nh x R; d_row: N int32, or null for row[i] = i; d_mean,
 * d_scale: C D doubles, each may be null (0 and 1).  The low-rank product runs on the f64 matrix cores, the rest is its epilogue.
 * R = 0 with d_W and d_H null is the plain whitening.  A session whose row[i] is outside [0, Nh) gets a zero factor.  d_out may be
 * d_stat1 itself: an element is read and written by the same lane.  A session's bits depend neither on N nor on its place in the batch.
 * With d_row the gathered factors (N x R doubles) go through the sc_* workspace. */
int sc_jfa_shift(const double* d_stat1, const double* d_stat0, int32_t N, int32_t C, int32_t D, const double* d_W, const double* d_H,
                 int32_t Nh, int32_t R, const int32_t* d_row, const double* d_mean, const double* d_scale, double* d_out, void* stream);

/* The accumulators of one E-step of the diagonal MAP term (estimate_map, :1666-1677, the loop over models) in one pass over the
 * per-model statistics, centred and shifted but not whitened.  Per column k, with n = d_stat0[i][k / D] and f = d_stat1[i][k]:
 *   L = 1 + n d_D[k]^2 / d_Sigma[k]     e = f d_D[k] / (L d_Sigma[k])     d_A[k] = sum_i (1 / L + e^2) n     d_Cacc[k] = sum_i e f
 * d_stat0: M x C; d_stat1: M x (C D); d_D, d_Sigma, d_A, d_Cacc: C D.  Rows are cut into slabs of SC_JFA_MAP_SLAB; a slab is added in
 * row order, the slabs' partial sums (sc_* workspace) in slab order.  The new D = d_Cacc / d_A is formed by the caller. */
#define SC_JFA_MAP_SLAB 256
int sc_jfa_map_acc(const double* d_stat0, const double* d_stat1, int32_t M, int32_t C, int32_t D, const double* d_D, const double* d_Sigma,
                   double* d_A, double* d_Cacc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_JFA_H */
