/* sidekit_amd/gmm_topc_stats.h -- top-C Baum-Welch statistics (Gaussian selection, then sparse posteriors and statistics: Kaldi's gselect
 * and post, ALIZE's topDistribsCount): the posteriors of a diagonal mixture renormalised over the K components per frame that a list
 * names, and the zeroth, first and second order statistics per segment accumulated from them.  The reference has no such function: an
 * addition beside its surface.  Two entry points of libsidekit_amd.so under the conventions of gmm_topc.h (error classes, device
 * pointers, the stream argument, the sc_* workspace freed by sc_release_workspace), in a header of their own and bound by a table of
 * their own (sidekit_amd/_lib.py GMM_TOPC_STATS_SIGNATURES): mixture.h, gmm_scoring.h, gmm_topc.h and their tables are pinned symbol for
 * symbol. */
#ifndef SIDEKIT_AMD_GMM_TOPC_STATS_H
#define SIDEKIT_AMD_GMM_TOPC_STATS_H
#include "gmm_topc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lp[n][k]   = -0.5 (sum_d (X[n][d] - mu[c][d])^2 invcov[c][d] + B[c]),  c = d_idx[n][k],  B[c] = -2 (log w[c] + log cst[c])
 * d_lse[n]   = log sum_{k < K} exp lp[n][k]
 * d_post[n][k] = exp(lp[n][k] - d_lse[n]): the posteriors renormalised over the list, they sum to 1 per frame.
 * X: N x D frames (XT_F32 or XT_F64, widened in the load); mu, invcov: C x D; d_idx: N x K int32, row n the components of frame n
 * (sc_gmm_top_components, or the caller's own); d_post: N x K; d_lse: N.  Nothing with an N x C footprint exists.
 * lp takes the direct form of sc_gmm_score_models_topc: the sum over d in one fixed order (the lanes' terms joined by that kernel's
 * butterfly), the fold over k in list order, so d_lse[n] is bit for bit the per-frame term sc_gmm_score_models_topc forms for a model
 * whose means are mu.  An index outside [0, C) contributes nothing (the read is guarded) and gets posterior 0; an entry with lp = -inf
 * (zero weight) or nan gets posterior 0 by assignment; a frame with no finite entry has d_lse = -inf and posteriors 0.  A frame's row
 * depends on that frame, its list and the mixture alone -- not on N or on where the frame lies in X.  No floating-point atomics.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_mu, d_invcov, d_B, d_idx, d_post or d_lse; a dtype other than
 * XT_F32 / XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], K outside [1, min(C, SC_GMM_TOPC_MAX)]. */
int sc_gmm_topc_posteriors(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov,
                           const double* d_B, int32_t C, const int32_t* d_idx /* N x K */, int32_t K, double* d_post /* N x K */,
                           double* d_lse /* N */, void* stream);

/* Per segment s (frames [seg_off[s], seg_off[s + 1]), offsets clamped to [0, N], at most max_len frames) and component c:
 *   stat0[s][c]    = sum over the frames n of the segment and the entries k with d_idx[n][k] == c of d_post[n][k]
 *   stat1[s][c][:] = the same sum of d_post[n][k] X[n][:]
 *   stat2[s][c][:] = the same sum of d_post[n][k] X[n][:]^2      (order == 2)
 *   llk[s]         = sum over the segment of d_lse[n]            (d_llk != null)
 * d_idx, d_post, d_lse as sc_gmm_topc_posteriors leaves them; the outputs have sc_gmm_stats's shapes: S x C, S x C x D, S x C x D, S.
 * An index outside [0, C) and an entry whose posterior is 0 add nothing (nothing is read through either), so a frame with
 * d_lse = -inf adds nothing to the statistics and -inf to llk.  A component no frame of a segment lists gets exact zeros; an empty
 * segment gives exact zeros and llk = 0.  A segment is cut as sc_gmm_stats cuts it (slabs); within a slab a component's entries are
 * added in frame order, within a frame in list order, a segment's slabs in ascending order, with no floating-point atomics, global or
 * LDS: a segment's statistics depend on its own frames, lists and posteriors alone -- not on S, the other segments or where the
 * segment lies in X.
 * Workspace (the sc_* workspace): when the longest segment has more than one slab, at most SC_GMM_MAX_SLABS partials of the outputs.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_idx, d_post, d_lse, d_seg_off, d_stat0 or d_stat1; a dtype
 * other than XT_F32 / XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], K outside
 * [1, min(C, SC_GMM_TOPC_MAX)], S < 1, max_len outside [0, N], S x slabs(max_len) beyond 2^31 - 1, order outside {1, 2}, order 2
 * without d_stat2. */
int sc_gmm_topc_stats(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, int32_t C,
                      const int32_t* d_idx /* N x K */, const double* d_post /* N x K */, int32_t K, const double* d_lse /* N */,
                      const int32_t* d_seg_off, int32_t S, int64_t max_len, int32_t order,
                      double* d_stat0 /* S x C */, double* d_stat1 /* S x C x D */, double* d_stat2 /* S x C x D, order 2 */,
                      double* d_llk /* S, or null */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GMM_TOPC_STATS_H */
