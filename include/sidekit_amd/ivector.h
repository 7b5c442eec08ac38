/* sidekit_amd/ivector.h -- the total-variability (i-vector) extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Two entry points of the same library, under the same conventions (error classes, device pointers, the stream argument).  Like the
 * Gaussian back-end's and the mixture's they live in a header of their own, bound by a table of their own (sidekit_amd/_lib.py
 * IVECTOR_SIGNATURES): the core header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_IVECTOR_H
#define SIDEKIT_AMD_IVECTOR_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- total variability: the per-session posterior of e_on_batch (sidekit/factor_analyser.py:51-91) -------------------------------------
 * For a loading matrix F ((C D) x R, row-major, whitened by the UBM) and a session with zero-order statistics n (C) and whitened
 * first-order statistics s (C D):
 *   Lambda = I + sum_c n[c] F_c' F_c      inv_lambda = Lambda^-1      e_h = inv_lambda F' s      E_hh = inv_lambda + e_h e_h'
 * Symmetric R x R matrices travel as their upper triangle, P = R (R + 1) / 2 doubles in the order of numpy.triu_indices(R): entry
 * (i, j), i <= j, is at p = i R - i (i - 1) / 2 + (j - i).  The large products (sum_c n[c] G[c] = stat0 . G, F' s = S_w . F and the
 * accumulators) are sc_dgemm_nn / sc_gemm_tn of the core header; these two calls are what lies between them.  float64 throughout.
 * No floating-point atomics; every sum has a fixed order, so a call's bits depend on its arguments alone.  Arguments are checked
 * (SK_EARG) before anything is enqueued: null pointers, R outside [1, SC_TV_MAX_RANK], C, D or N below 1, sc_tv_posterior without
 * either of its two second-order outputs. */
#define SC_TV_MAX_RANK 192        /* sc_tv_posterior keeps ONE packed triangle in LDS and works in place on it: 192 * 193 / 2 * 8 =
                                     148,224 B, plus three R-vectors of 1,536 B and 4,096 B of partial sums = 156,928 B of the
                                     163,840 B a workgroup may declare (rank 200 would need 169,696 B) */

/* G[c] = F_c' F_c packed (C x P), F_c = rows c D .. (c + 1) D of F: a batched TN product with K = D on the f64 matrix cores; only the
 * 64 x 64 tiles that hold part of the upper triangle are computed. */
int sc_tv_gram(const double* d_F, int32_t C, int32_t D, int32_t R, double* d_G, void* stream);

/* Per session i of N: Lambda = I + unpack(d_Lp[i]) (d_Lp: N x P, the packed sum WITHOUT the identity), inv_lambda by Cholesky,
 * d_Eh[i] = inv_lambda d_B[i] (d_B, d_Eh: N x R), E_hh = inv_lambda + e_h e_h' to d_Ehh[i] packed (N x P, or null) and its diagonal to
 * d_diag[i] (N x R, or null; the same bits as the packed diagonal entries); at least one of the two is not null.  d_Ehh may be d_Lp
 * itself: a session reads its row completely before it writes it.  d_Eh and d_diag must not overlap d_Lp or d_B.  One workgroup per
 * session, whose bits do not depend on N or on its position.  Lambda = I + a positive semi-definite matrix when the counts are finite
 * and not negative, so no pivot can fail; a session with non-finite input gets non-finite output, the others are not affected, and no
 * error is raised. */
int sc_tv_posterior(const double* d_Lp, const double* d_B, int32_t N, int32_t R, double* d_Eh, double* d_Ehh, double* d_diag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_IVECTOR_H */
