/* sidekit_amd/ivector_wide.h -- total variability at ranks above SC_TV_MAX_RANK (ivector.h): the ranks i-vector systems are trained at
 * (400, 600).  A surface of its own beside ivector.h, whose entries keep their cap, their bits and their refusals; bound by a table of
 * its own (sidekit_amd/_lib.py IVECTOR_WIDE_SIGNATURES).  Same conventions as ivector.h: error classes, device pointers, the stream
 * argument, float64 throughout, symmetric R x R matrices as packed upper triangles of P = R (R + 1) / 2 doubles in the order of
 * numpy.triu_indices(R).  No floating-point atomics; every sum has a fixed order.  Arguments are checked (SK_EARG) before anything is
 * enqueued: null pointers, R outside [1, SC_TVW_MAX_RANK], C, D or N below 1, a shift that is negative or not finite, scratch smaller
 * than sc_tvw_workspace says, d_Eh without d_B or d_B without d_Eh, sc_tvw_posterior without either of its two second-order outputs. */
#ifndef SIDEKIT_AMD_IVECTOR_WIDE_H
#define SIDEKIT_AMD_IVECTOR_WIDE_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SC_TVW_MAX_RANK 1024      /* where G of sc_tvw_gram reaches 8.6 GB at C = 2048 (2048 * 1024 * 1025 / 2 * 8 B); the packed index's
                                     24-bit product i (2 R - i - 1) would stay below 2^24 up to R = 2896 */

/* G[c] = F_c' F_c packed (C x P): the kernel of sc_tv_gram (ivector.h), launched for R up to SC_TVW_MAX_RANK; for R <= SC_TV_MAX_RANK
 * the bits of sc_tv_gram. */
int sc_tvw_gram(const double* d_F, int32_t C, int32_t D, int32_t R, double* d_G, void* stream);

/* Bytes of scratch sc_tvw_posterior needs for N sessions of rank R: N * 2 Rp^2 doubles, Rp = R rounded up to 64 (the session's matrix
 * beside the inverse of its factor).  SK_EARG for N < 1 or R outside [1, SC_TVW_MAX_RANK]. */
int sc_tvw_workspace(int32_t N, int32_t R, int64_t* bytes);

/* Per session i of N: Lambda = shift * I + unpack(d_Lp[i]) (d_Lp: N x P), inv_lambda = Lambda^-1 by a blocked Cholesky factorisation on
 * the f64 matrix cores, d_Eh[i] = inv_lambda d_B[i] (d_B, d_Eh: N x R), E_hh = inv_lambda + e_h e_h' to d_Ehh[i] packed (N x P, or null)
 * and its diagonal to d_diag[i] (N x R, or null; the same bits as the packed diagonal entries); at least one of the two is not null.
 * shift is finite and >= 0: 1.0 for the posterior, 0.0 for a matrix that is inverted as it is.  d_B may be null: then d_Eh must be null
 * and the outputs are inv_lambda alone.  d_Ehh may be d_Lp itself: a session's row is read completely into scratch before it is
 * written.  d_Eh and d_diag must not overlap d_Lp or d_B.  d_work: caller-owned scratch of work_bytes >= sc_tvw_workspace(N, R) bytes;
 * nothing is allocated inside the call.  One workgroup per session, working on its own slice of d_work; a session's bits depend on its
 * own row, R and shift alone -- not on N, its position, which outputs are asked for, or aliasing.  Lambda must be positive definite
 * (it is, for shift = 1 and finite counts that are not negative); a session that is not, or that has non-finite input, gets non-finite
 * output, the others are not affected, and no error is raised. */
int sc_tvw_posterior(const double* d_Lp, const double* d_B, int32_t N, int32_t R, double shift, double* d_Eh, double* d_Ehh,
                     double* d_diag, void* d_work, int64_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_IVECTOR_WIDE_H */
