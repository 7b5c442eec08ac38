/* sidekit_amd/gmm_scoring.h -- GMM-UBM verification: the log-likelihood of every test segment under many mean-adapted models of one
 * diagonal mixture (sidekit/gmm_scoring.py:53-116).  One entry point of libsidekit_amd.so under the conventions of mixture.h (error
 * classes, device pointers, the stream argument, the sc_* workspace freed by sc_release_workspace), in a header of its own and bound by
 * a table of its own (sidekit_amd/_lib.py GMM_SCORING_SIGNATURES): mixture.h and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_GMM_SCORING_H
#define SIDEKIT_AMD_GMM_SCORING_H
#include "mixture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SC_GMM_SCORE_MAX_M 65535   /* models of one call: one grid row per group of models, at most 65535 rows */

/* llk[m][s] = sum over the frames n of segment s of  log sum_c exp lp_m[n][c],
 * lp_m[n][c] = -0.5 (sum_d X[n][d]^2 invcov[c][d] - 2 sum_d X[n][d] mus[m][c][d] invcov[c][d] + A_m[c]),
 * A_m[c] = sum_d mus[m][c][d]^2 invcov[c][d] + B[c],   B[c] = -2 (log w[c] + log cst[c])
 * for every (m, s) with mask[m][s] != 0; the other entries of d_llk are not written.
 * X: N x D frames (XT_F32 or XT_F64, widened in the load); mus: M x C x D means; invcov: C x D; B: C; segment s is frames
 * [d_seg_off[s], d_seg_off[s + 1]) (S + 1 ascending int32 offsets on the device, clamped to [0, N] and to each other by the kernel;
 * frames of a segment beyond max_len are not read).  float64 on the f64 matrix cores; no N x M array exists: only segment sums leave
 * the kernel.  lp_m is formed as sc_gmm_frame_loglik forms it (the squares first, then the linear half, in chunks of 16 d); the squares'
 * half is computed once per group of models and reused.  A segment is cut as sc_gmm_stats cuts it (a function of its length alone: slabs,
 * then 64-frame tiles from the segment's first frame); a tile's frames are added in frame order, a slab's tiles and a segment's slabs in
 * ascending order, with no floating-point atomics: llk[m][s] depends on model m, on the mixture and on the frames of segment s alone --
 * not on the other models, the mask, M, S or where the segment lies in X.  An empty segment gives 0.
 * Workspace (the sc_* workspace): M x C doubles for A and, when the longest segment has more than one slab, at most
 * SC_GMM_MAX_SLABS x M x S doubles of partial sums.
 * Arguments are checked (SK_EARG) before anything is enqueued: null d_X, d_mus, d_invcov, d_B, d_seg_off or d_llk; a dtype other than
 * XT_F32 / XT_F64; N outside [1, 2^31), D outside [1, SC_GMM_MAX_D], C outside [1, SC_GMM_MAX_C], M outside [1, SC_GMM_SCORE_MAX_M],
 * S < 1, max_len outside [0, N], S x slabs(max_len) beyond 2^31 - 1. */
int sc_gmm_score_models(const void* d_X, int32_t x_dtype, int64_t N, int32_t D,
                        const double* d_mus, int32_t M, const double* d_invcov, const double* d_B, int32_t C,
                        const int32_t* d_seg_off, int32_t S, int64_t max_len,
                        const uint8_t* d_mask /* M x S, or null: all trials */, double* d_llk /* M x S */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GMM_SCORING_H */
