/* sidekit_amd/gaussian_backend.h -- the Gaussian back-end's extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Three entry points of the same library, under the same conventions (error classes, device pointers, the stream argument, the sc_*
 * workspace freed by sc_release_workspace).  They live in a header of their own, bound by a table of their own
 * (sidekit_amd/_lib.py GAUSSIAN_SIGNATURES): the core header and its table are pinned symbol for symbol by the tests of the features
 * before this one. */
#ifndef SIDEKIT_AMD_GAUSSIAN_BACKEND_H
#define SIDEKIT_AMD_GAUSSIAN_BACKEND_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Gaussian back-end: closed-set identification (sidekit/lid_utils.py:57-263) -----------------------------------------------------
 * Which of C known classes (a language, a speaker of a closed set, a channel) produced an x-vector.  The device half; the D x D algebra
 * (one Cholesky per class, slogdet) stays on the host (sidekit_amd/lid_utils.py).  The conventions of PLDA training: float64, partial
 * sums through the sc_* workspace and added in a fixed order, no floating-point atomics, arguments checked (SK_EARG) before anything is
 * enqueued.  The tied model (one covariance) has no entry point of its own: cst - 0.5 (x - m_c)' P (x - m_c) is sc_plda_fast with the
 * class means as E, Phi = -P and Psi = P. */

/* The C per-class scatters of gaussian_backend_train_hetero (:110-115) in one call:
 *   S[c][m][n] = sum_{k in class c} (X[k][m] - Mc[c][m]) (X[k][n] - Mc[c][n]),   S: C x D x D float64 -- C D^2 8 bytes of output
 *   (0.5 GB at C = 1000, D = 256).
 * X: N x D, XT_F32 or XT_F64 (widened in the load), its rows GROUPED by class: class c is rows [d_class_off[c], d_class_off[c + 1]) (C + 1
 * ascending int32 offsets on the device, clamped to [0, N] by the kernel); d_Mc: C x D float64 class means (sc_class_sums over the counts);
 * max_count: the longest class (the host knows the counts; rows of a class beyond max_count would not be read).  A long class is cut
 * into row slabs whose partial tiles are added in slab order; the cut is a function of (max_count, D, C).  A class of one row, whose
 * mean is that row, gives an exact zero matrix. */
int sc_class_scatter(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_class_off, const double* d_Mc, int32_t C,
                     int64_t max_count, double* d_S, void* stream);

/* The heteroscedastic log-likelihood matrix (:246-257, diag=False), in the Scores.scoremat orientation:
 *   out[c][n] = cst[c] - 0.5 |(X[n][:] - means[c][:]) . W[c]|^2,   P_c = inv(Sigma_c) = W[c] W[c]'  (W[c] = inv(L_c)' of Sigma_c = L_c L_c').
 * X: N x D, d_means: C x D, d_W: C x D x D, d_cst: C, d_out: C x N, all float64.  The product runs on the f64 matrix cores per (row tile,
 * class) and is never stored: no (N x D) or (N x C x D) intermediate exists, only C D doubles of workspace (means[c] . W[c]).  A row's
 * D squares are added in one fixed order, so out[c][n] depends on row n, class c and D alone -- not on N, the row's position or the
 * stream.  C <= 65535. */
int sc_gauss_loglik(const double* d_X, int64_t N, int32_t D, const double* d_means, const double* d_W, const double* d_cst, int32_t C,
                    double* d_out, void* stream);

/* compute_log_likelihood_ratio (:57-72) on a C x N float64 matrix of log-likelihoods:
 *   out[c][n] = log p_tar + M[c][n] - LSE_{j != c}(M[j][n] + log((1 - p_tar) / (C - 1))).
 * d_out may be d_M (in place).  Stable where one class dominates: the leave-one-out sums are taken about the largest and the second
 * largest value of the column, never as "total minus own term".  C < 2, or p_tar outside (0, 1), is SK_EARG. */
int sc_closed_set_llr(const double* d_M, int32_t C, int64_t N, double p_tar, double* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_GAUSSIAN_BACKEND_H */
