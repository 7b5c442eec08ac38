/* sidekit_amd/gmm_topc_em.h -- top-C EM (Gaussian selection carried down the split tree of EM_split): the lists of a mixture that
 * changes every iteration are kept current from a short row of candidates per frame -- after a split, the two children of every parent
 * the frame listed -- instead of another pass over all C components.  One entry point of libsidekit_amd.so under the conventions of
 * gmm_topc_stats.h (error classes, device pointers, the stream argument), in a header of its own and bound by a table of its own
 * (sidekit_amd/_lib.py GMM_TOPC_EM_SIGNATURES): mixture.h, gmm_scoring.h, gmm_topc.h, gmm_topc_stats.h and their tables are pinned symbol
 * for symbol.  The reference has no such function: an addition beside its surface. */
#ifndef SIDEKIT_AMD_GMM_TOPC_EM_H
#define SIDEKIT_AMD_GMM_TOPC_EM_H
#include "gmm_topc_stats.h"

#define SC_GMM_TOPC_CAND_MAX 64   /* candidates per frame: one per lane */

#ifdef __cplusplus
extern "C" {
#endif

/* Per frame n, from the row of Kc candidates d_cand[n][:], the K that score best under the mixture, and optionally their posteriors.
 * X: N x D frames (XT_F32 or XT_F64, widened in the load); mu, invcov: C x D; B[c] = -2 (log w[c] + log cst[c]).
 * Valid candidates: entry j of a frame's row is valid when it lies in [0, C) and no earlier entry of the same row holds the same value.
 *   Nothing is read through an invalid entry.
 * Scoring: for each valid candidate c, lp = -0.5 (sum_d (X[n][d] - mu[c][d])^2 invcov[c][d] + B[c]) in the direct form of
 *   sc_gmm_topc_posteriors (lane = d, and d + 64 above 64, joined by the same butterfly): lp has the bits that kernel forms.
 * Ranking: the larger lp wins; at equal lp the lower component index wins.  A nan lp ranks as -inf.
 * Output list: d_idx[n] holds the min(K, number of valid candidates) winners in ascending component order; any remaining entries
 *   are -1 (every top-C kernel skips an index outside [0, C)).  K > Kc is legal.
 * Posteriors: d_post and d_lse are both null or both given.  When given they are bit for bit what sc_gmm_topc_posteriors writes for
 *   d_idx: the fold over k in list order; posterior 0 for -1, -inf and nan entries; d_lse = -inf for a frame with no finite entry.
 *   The lists do not depend on whether they are requested.
 * A frame's outputs depend on that frame, its candidate row and the mixture alone -- not on N or on where the frame lies in X.
 * float64, no floating-point atomics, no workspace.  d_idx must not overlap d_cand.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_mu, d_invcov, d_B, d_cand or d_idx; exactly one of d_post /
 * d_lse null; a dtype other than XT_F32 / XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], Kc
 * outside [1, SC_GMM_TOPC_CAND_MAX], K outside [1, min(C, SC_GMM_TOPC_MAX)]. */
int sc_gmm_topc_refine(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov,
                       const double* d_B, int32_t C, const int32_t* d_cand /* N x Kc */, int32_t Kc, int32_t K,
                       int32_t* d_idx /* N x K */, double* d_post /* N x K, or null */, double* d_lse /* N, or null */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GMM_TOPC_EM_H */
