/* sidekit_amd/mixture.h -- the diagonal-GMM extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Two entry points of the same library, under the same conventions (error classes, device pointers, the stream argument, the sc_*
 * workspace freed by sc_release_workspace).  Like the Gaussian back-end's they live in a header of their own, bound by a table of their
 * own (sidekit_amd/_lib.py MIXTURE_SIGNATURES): the core header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_MIXTURE_H
#define SIDEKIT_AMD_MIXTURE_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagonal Gaussian mixture: frame log-likelihoods and Baum-Welch statistics (sidekit/mixture.py:52-64, 510-536, 586-617) ---------
 * For a mixture of C diagonal Gaussians (mu, invcov: C x D float64; A: C float64, the data-independent term of Mixture._compute_all,
 * A[c] = sum_d mu[c][d]^2 invcov[c][d] - 2 (log w[c] + log cst[c])) and N frames X (N x D, XT_F32 or XT_F64, widened in the load):
 *   lp[n][c]  = -0.5 (sum_d X[n][d]^2 invcov[c][d] - 2 sum_d X[n][d] mu[c][d] invcov[c][d] + A[c])
 *   lse[n]    = log sum_c exp lp[n][c]                    pp[n][c] = exp(lp[n][c] - lse[n])
 *   stat0[c]  = sum_n pp[n][c]      stat1[c][:] = sum_n pp[n][c] X[n][:]      stat2[c][:] = sum_n pp[n][c] X[n][:]^2
 * float64 on the f64 matrix cores.  Neither call builds the N x C posterior matrix (sc_gmm_frame_loglik writes lp only when asked):
 * sc_gmm_stats recomputes each lp tile from the frames.  No floating-point atomics; every sum has a fixed order, so a call's bits
 * depend on its arguments alone.  Arguments are checked (SK_EARG) before anything is enqueued: null pointers, C outside
 * [1, SC_GMM_MAX_C], D outside [1, SC_GMM_MAX_D], N outside [1, 2^31), S < 1, max_len outside [0, N], a dtype other than XT_F32 / XT_F64, order outside {1, 2}, order 2 without
 * d_stat2. */
#define SC_GMM_MAX_D 128          /* the frame tile (64 x D), a 64 x 16 operand chunk and the 64 x 64 posterior tile share 160 KiB of LDS */
#define SC_GMM_MAX_C 4194240      /* 65535 component tiles of 64 */
#define SC_GMM_SLAB_FRAMES 512    /* a segment of L frames is cut into ceil(L / SC_GMM_SLAB_FRAMES) slabs ... */
#define SC_GMM_MAX_SLABS 64       /* ... and at most this many: the workspace of sc_gmm_stats is at most
                                     SC_GMM_MAX_SLABS partial C x (2 D + 1) statistics per segment, never proportional to N C */

/* lse[n] for every frame (online log-sum-exp over component tiles) and, when d_lp is not null, the N x C matrix lp itself
 * (Mixture.compute_log_posterior_probabilities; the only output with an N x C footprint, and only on request).  A frame whose lp is
 * -inf for every component has lse = -inf. */
int sc_gmm_frame_loglik(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A,
                        int32_t C, double* d_lse, double* d_lp, void* stream);

/* Per-segment statistics.  Segment s is frames [d_seg_off[s], d_seg_off[s + 1]) (S + 1 ascending int32 offsets on the device, clamped to
 * [0, N] and to each other by the kernel); max_len: the longest segment (frames of a segment beyond max_len are not read).  d_lse: the
 * output of sc_gmm_frame_loglik for the same X and mixture.  order 1: d_stat0 (S x C) and d_stat1 (S x C x D); order 2: d_stat2
 * (S x C x D) as well (not null then).  d_llk (S, or null): the sum of lse over the segment, in an order that depends on its length alone.
 * A segment of L frames is cut into ceil(L / SC_GMM_SLAB_FRAMES) slabs (at most SC_GMM_MAX_SLABS) of equal length rounded up to a
 * multiple of 64; the slabs' partial statistics are added in slab order.  The cut, the frame tiles (aligned to the segment's first frame) and every sum's
 * order depend on L alone, so a segment's statistics are the same bits alone or among others, wherever it lies in X.  Frames of a
 * tile that lie outside its slab get pp = 0 by assignment and their lse is not read; an empty segment gives exact zeros. */
int sc_gmm_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A, int32_t C,
                 const double* d_lse, const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order, double* d_stat0, double* d_stat1,
                 double* d_stat2, double* d_llk, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_MIXTURE_H */
