/* sidekit_amd/gmm_topc.h -- top-C (fast) GMM-UBM scoring (Reynolds et al. 2000; ALIZE's topDistribsCount): per frame the K components
 * that score best under the UBM, and the log-likelihood of every test segment under many mean-adapted models on those components alone.
 * The reference has no such function: an addition beside its surface.  Two entry points of libsidekit_amd.so under the conventions of
 * mixture.h (error classes, device pointers, the stream argument, the sc_* workspace freed by sc_release_workspace), in a header of their
 * own and bound by a table of their own (sidekit_amd/_lib.py GMM_TOPC_SIGNATURES): mixture.h, gmm_scoring.h and their tables are pinned
 * symbol for symbol. */
#ifndef SIDEKIT_AMD_GMM_TOPC_H
#define SIDEKIT_AMD_GMM_TOPC_H
#include "gmm_scoring.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SC_GMM_TOPC_MAX 32   /* components per frame: a frame's list of (value, index) pairs lives in LDS beside the tiles of pass A */

/* d_idx[n][0 .. K) = the indices of the K components with the largest lp[n][c] under the mixture (mu, invcov, A as sc_gmm_frame_loglik
 * takes them; lp is formed by the same function in the same order, so a list is chosen from the bits sc_gmm_frame_loglik sees).
 * X: N x D frames (XT_F32 or XT_F64, widened in the load); d_idx: N x K int32.  The larger lp wins, at equal lp the lower index.  A list
 * is stored by ascending component index and holds K distinct indices in [0, C) whatever the frame holds: where fewer than K components
 * have a finite lp (zero weights give -inf) or the frame holds nan the choice among the others is unspecified but valid.  A frame's
 * list depends on that frame and the mixture alone -- not on N or on where the frame lies in X.  No floating-point atomics.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_mu, d_invcov, d_A or d_idx; a dtype other than XT_F32 /
 * XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], K outside [1, min(C, SC_GMM_TOPC_MAX)]. */
int sc_gmm_top_components(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_invcov, const double* d_A,
                          int32_t C, int32_t K, int32_t* d_idx, void* stream);

/* llk[m][s] = sum over the frames n of segment s of  log sum_{k < K} exp lp_m[n][d_idx[n][k]],
 * lp_m[n][c] = -0.5 (sum_d (X[n][d] - mus[m][c][d])^2 invcov[c][d] + B[c]),   B[c] = -2 (log w[c] + log cst[c])
 * for every (m, s) with mask[m][s] != 0; the other entries of d_llk are not written.
 * X, mus, invcov, B, the segments, max_len and the mask as sc_gmm_score_models takes them; d_idx: N x K int32, row n the components of
 * frame n (sc_gmm_top_components, or the caller's own).  An index outside [0, C) contributes nothing (the read is guarded); a frame all
 * of whose terms are -inf or absent contributes -inf.  float64 on the vector ALU: this is gather work, K D doubles per frame and model.
 * The sum over d has one fixed order (the lanes' terms joined by a fixed butterfly), the fold over k runs in list order.  A segment is
 * cut as sc_gmm_score_models cuts it (slabs, then 64-frame tiles from the slab's first frame); a tile's frames are added in frame
 * order, a slab's tiles and a segment's slabs in ascending order, with no floating-point atomics: llk[m][s] depends on model m, on the
 * mixture, on the frames of segment s and on their lists alone -- not on the other models, the mask, M, S or where the segment lies in
 * X.  An empty segment gives 0.
 * Workspace (the sc_* workspace): when the longest segment has more than one slab, at most SC_GMM_MAX_SLABS x M x S doubles.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_mus, d_invcov, d_B, d_seg_off, d_idx or d_llk; a dtype other
 * than XT_F32 / XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], M outside
 * [1, SC_GMM_SCORE_MAX_M], S < 1, max_len outside [0, N], S x slabs(max_len) beyond 2^31 - 1, K outside [1, min(C, SC_GMM_TOPC_MAX)]. */
int sc_gmm_score_models_topc(const void* d_X, int32_t x_dtype, int64_t N, int32_t D,
                             const double* d_mus, int32_t M, const double* d_invcov, const double* d_B, int32_t C,
                             const int32_t* d_seg_off, int32_t S, int64_t max_len,
                             const uint8_t* d_mask /* M x S, or null: all trials */, const int32_t* d_idx /* N x K */, int32_t K,
                             double* d_llk /* M x S */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GMM_TOPC_H */
