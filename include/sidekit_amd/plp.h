/* sidekit_amd/plp.h -- the PLP tail of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * One entry point of the same library, under the same conventions (error classes, device pointers, the stream argument).  Like the
 * cepstral front end's it lives in a header of its own, bound by a table of its own (sidekit_amd/_lib.py PLP_SIGNATURES): the core
 * header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_PLP_H
#define SIDEKIT_AMD_PLP_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SC_PLP_MIN_BANDS 4        /* the fewest critical bands */
#define SC_PLP_MAX_BANDS 32       /* the most */
#define SC_PLP_ROWS 64            /* frames of one workgroup, one per lane */

/* ---- from log critical-band energies to liftered LPC cepstra (sidekit/frontend/features.py: postaud, dolpc, levinson, lpc2cep, lifter)
 * d_logband: float32 rows [N][ldb]; the first nb columns of a row are the log critical-band energies of a frame (sc_mfcc's fb block
 * under a bark bank, or sc_feat_rasta's output on it).  d_eql: float64 [nb], the equal-loudness weights.  d_acw: float64
 * [order + 1][nb], the cosine-transform weights: with M = 2 (nb - 1), acw[k][j] = 2 cos(pi j k / (nb - 1)) / M for 0 < j < nb - 1,
 * 1 / M for j = 0 and (-1)^k / M for j = nb - 1 (the real inverse FFT of the mirrored spectrum, written out).  d_lift: float64
 * [order + 1], the lifter weights.
 *
 * Per frame, in float64, products and sums rounded separately:
 *   a[j] = exp((double)logband[j])
 *   z[j] = pow(eql[j] * a[j], 0.33)
 *   y = z with y[0] = z[1] and y[nb - 1] = z[nb - 2]
 *   r[k] = sum_j acw[k][j] y[j], j ascending from a zero start, k = 0 .. order
 *   Levinson-Durbin on r: P = r[0]; for k = 0 .. order - 1: s = r[k + 1], then s = s + A[j] r[k - j] for j = 0 .. k - 1 ascending;
 *     t = -s / P; P = P (1 - t t); A[k] = t; then for j = 0 .. (k + 1) / 2 - 1 with i = k - j - 1: (A[j], A[i]) = (A[j] + t A[i],
 *     A[i] + t A[j]) from the old values (once when i = j).  Nothing looks at the sign of P: a non-positive or NaN P runs on.
 *   c[0] = log(P); c[n] = -(A[n - 1] + (sum_{m = 1}^{n - 1} ((n - m) A[m - 1]) c[n - m]) / n), m ascending from a zero start
 *   cep[n] = c[n] lift[n], n = 0 .. order
 *
 * d_cep: float32 rows [N][ldc], columns 0 .. order.  d_post: null, or float32 rows [N][ldp] whose columns 0 .. nb - 1 receive y.
 * Columns beyond those are not touched.  A frame of zero power (-inf in its row) gives NaN cepstra in its own row only.
 *
 * One lane per frame; no atomics; every sum has the order above; a frame's bits depend on its own row and the tables alone, so a row
 * gives the same bits alone or anywhere in a batch.
 * Checked (SK_EARG) before anything is enqueued: null pointers (d_post may be null), N < 0, nb outside [SC_PLP_MIN_BANDS,
 * SC_PLP_MAX_BANDS], order outside [1, nb - 2], ldb < nb, ldc < order + 1, ldp < nb with d_post given, d_cep or d_post equal to
 * d_logband.  N == 0 enqueues nothing. */
int sc_plp_cepstra(const float* d_logband, int64_t ldb, int64_t N, int32_t nb, int32_t order, const double* d_eql, const double* d_acw,
                   const double* d_lift, float* d_cep, int64_t ldc, float* d_post, int64_t ldp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_PLP_H */
