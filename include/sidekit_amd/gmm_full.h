/* sidekit_amd/gmm_full.h -- the full-covariance GMM extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Two entry points of the same library, under the same conventions (error classes, device pointers, the stream argument, the sc_*
 * workspace freed by sc_release_workspace).  Like the diagonal mixture's (mixture.h) they live in a header of their own, bound by a
 * table of their own (sidekit_amd/_lib.py GMM_FULL_SIGNATURES): the core header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_GMM_FULL_H
#define SIDEKIT_AMD_GMM_FULL_H
#include "mixture.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- full-covariance Gaussian mixture: frame log-likelihoods and Baum-Welch statistics (sidekit/mixture.py:490-508, 586-617) ----------
 * For a mixture of C Gaussians in D dimensions given as mu (C x D float64), M (C x D x D float64, one GENERAL matrix per component:
 * nothing assumes it triangular) and g (C float64, g[c] = log w[c] + log cst[c], formed on the host), and N frames X (N x D, XT_F32 or
 * XT_F64, widened in the load):
 *   y[n][c][m] = sum_k M[c][m][k] (X[n][k] - mu[c][k])         (centred first, in float64, then multiplied)
 *   lp[n][c]   = g[c] - 0.5 sum_m y[n][c][m]^2
 *   lse[n]     = log sum_c exp lp[n][c]                    pp[n][c] = exp(lp[n][c] - lse[n])
 *   stat0[s][c]       = sum_{n in s} pp[n][c]
 *   stat1[s][c][:]    = sum_{n in s} pp[n][c] X[n][:]
 *   stat2[s][c][:][:] = sum_{n in s} pp[n][c] X[n][:] X[n][:]'      (order 2 only)
 * With M[c] any factor of the precision matrix, M[c]' M[c] = invcov[c], lp is log(w[c] N(x; mu[c], invcov[c]^-1)).  float64 on the f64
 * matrix cores.  Neither call builds an N x C array (sc_gmm_full_frame_loglik writes lp only when asked) or an N x D x D one:
 * sc_gmm_full_stats recomputes each lp tile from the frames, by the same function in the same order, so it sees the bits
 * sc_gmm_full_frame_loglik saw.  No floating-point atomics; every sum has a fixed order, so a call's bits depend on its arguments alone.
 * Arguments are checked (SK_EARG) before anything is enqueued: null pointers, C outside [1, SC_GMM_MAX_C], D outside
 * [1, SC_GMM_FULL_MAX_D], N outside [1, 2^31), S < 1, max_len outside [0, N], S x slabs x C beyond 2^31 - 1 workgroups, a dtype other
 * than XT_F32 / XT_F64, order outside {1, 2}, order 2 without d_stat2.  D = 1, D that is no multiple of 4 (the MFMA k-step) and every
 * tile edge are padded with zeros by assignment: nothing is read past an operand. */
#define SC_GMM_FULL_MAX_D 96             /* 64 x D frames and one (D + 16) x D matrix share 160 KiB of LDS: 137 KiB at D = 96 */
#define SC_GMM_FULL_SLAB_TARGET 1024     /* workgroups per segment the cut aims at: one per component and slab */

/* lse[n] for every frame (online log-sum-exp over the components in ascending order) and, when d_lp is not null, the N x C matrix lp
 * itself (compute_log_posterior_probabilities_full; the only output with an N x C footprint, and only on request).  A frame whose lp
 * is -inf for every component has lse = -inf. */
int sc_gmm_full_frame_loglik(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_M, const double* d_g,
                             int32_t C, double* d_lse, double* d_lp, void* stream);

/* Per-segment statistics.  Segments as sc_gmm_stats takes them: segment s is frames [d_seg_off[s], d_seg_off[s + 1]) (S + 1 ascending
 * int32 offsets on the device, clamped to [0, N] and to each other by the kernel); max_len: the longest segment (frames of a segment
 * beyond max_len are not read).  d_lse: the output of sc_gmm_full_frame_loglik for the same X and mixture.  order 1: d_stat0 (S x C) and
 * d_stat1 (S x C x D); order 2: d_stat2 (S x C x D x D) as well (not null then).  d_llk (S, or null): the sum of lse over the segment, in
 * an order that depends on its length alone.  Order 1 is order 2 without stat2, bit for bit.  stat2[s][c] is symmetric bit for bit: the
 * lower triangle is computed and mirrored.  A frame whose lse is -inf has posterior 0 for every component.
 *
 * The cut.  One workgroup takes one component of one slab of one segment, so the components give the parallelism first and slabs only
 * where C is small: a segment of L frames is cut into
 *   slabs(L, C) = min(ceil(L / SC_GMM_SLAB_FRAMES), max(1, min(SC_GMM_MAX_SLABS, SC_GMM_FULL_SLAB_TARGET / C)))      (at least 1)
 * slabs of equal length rounded up to a multiple of 64, whose partial statistics are added in slab order.  The cut, the frame tiles
 * (aligned to the segment's first frame) and every sum's order depend on L and C alone -- not on the order, the other segments or S --
 * so a segment's statistics are the same bits alone or among others, wherever it lies in X and however segments are grouped into calls.
 * Frames of a tile that lie outside its slab get pp = 0 by assignment and their lse is not read; an empty segment gives exact zeros.
 *
 * Workspace of a call, from the stream's lease: none when slabs(max_len, C) = 1, otherwise
 *   slabs(max_len, C) x S x C x (1 + D + (order == 2 ? D x D : 0)) x 8 bytes,
 * at most max(SC_GMM_FULL_SLAB_TARGET, C) component partials per segment whatever N is. */
int sc_gmm_full_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_M, const double* d_g, int32_t C,
                      const double* d_lse, const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order, double* d_stat0, double* d_stat1,
                      double* d_stat2, double* d_llk, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GMM_FULL_H */
