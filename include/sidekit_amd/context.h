/* sidekit_amd/context.h -- the context-feature extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Three entry points of the same library, under the same conventions (error classes, device pointers, the stream argument), in a
 * header of their own bound by a table of their own (sidekit_amd/_lib.py CONTEXT_SIGNATURES), like features.h beside them. */
#ifndef SIDEKIT_AMD_CONTEXT_H
#define SIDEKIT_AMD_CONTEXT_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a linear map over a window of frames around t, on a stacked ragged batch (sidekit/frontend/features.py:169-223, 969-1001;
 *      sidekit/features_server.py:325-394) -------------------------------------------------------------------------------------------------
 * x: float32 rows of D coefficients, row r at d_x + r * ldx (ldx >= D).  d_seg_off: S + 1 ascending int64 row offsets on the device;
 * segment s is rows [d_seg_off[s], d_seg_off[s + 1]); empty segments are allowed; the caller vouches that the offsets lie inside the
 * matrix.  A segment of n rows is read at cl(i) = min(max(i, 0), n - 1): its first and last row are repeated past its ends.
 * max_rows (>= 1) sizes the grid and nothing else: give the longest segment's rows or any bound of them, such as the matrix's rows; a
 * longer segment is still computed in full, and no bit of the result depends on the value.  No atomics; every sum has a fixed order;
 * time is tiled relative to the segment's first row, so a segment's output bits depend on its own rows alone, wherever it lies in the
 * batch, and are the same run to run.  Arguments are checked (SK_EARG) before anything is enqueued: null pointers, S < 0, max_rows < 1,
 * D outside its range, a leading dimension below the row's width, x == y, the sizes beyond the limits below.  S == 0 enqueues nothing. */
#define SC_CTX_TILE 256           /* rows of one tile of sc_ctx_gather: tile i of a segment is its rows [256 i, 256 i + 256) */
#define SC_CTX_COLS 16            /* columns of one tile of sc_ctx_gather and sc_ctx_basis */
#define SC_CTX_MAX_D 1048560      /* sc_ctx_gather, sc_ctx_basis: 65535 column chunks of 16 */
#define SC_CTX_MAX_BLOCKS 256     /* sc_ctx_gather: output blocks J */
#define SC_CTX_MAX_SPAN 256       /* sc_ctx_gather: the largest offset less the smallest one, and the largest |offset| */
#define SC_CTX_BASIS_TILE 128     /* rows of one tile of sc_ctx_basis */
#define SC_CTX_MAX_W 64           /* sc_ctx_basis, sc_ctx_project: frames of a window */
#define SC_CTX_PROJ_TILE 64       /* sc_ctx_project: rows and columns of one tile */
#define SC_CTX_PROJ_MAX_D 128     /* sc_ctx_project: coefficients of a frame */
#define SC_CTX_PROJ_MAX_Q 512     /* sc_ctx_project: columns of the projection */
/* LDS of one workgroup:
 *   sc_ctx_gather   (SC_CTX_TILE + SC_CTX_MAX_SPAN) rows x 16 float32 + 2 x SC_CTX_MAX_BLOCKS int32            = 34,816 B
 *   sc_ctx_basis    W x J float64 + (SC_CTX_BASIS_TILE + W - 1 rounded up to odd) rows x 16 float32; W = J = 64  = 44,992 B
 *   sc_ctx_project  two 64 x 17 float64 operand images + the 64 x 65 float64 result tile                         = 50,688 B */

/* Stacked context and shifted deltas.  d_plus: J int32 row offsets on the device; d_minus: J more, or null.
 *   y[t, b D + c] = x[cl(t + plus[b]), c]                               (d_minus null: a copy)
 *   y[t, b D + c] = x[cl(t + plus[b]), c] - x[cl(t + minus[b]), c]      (one float32 subtraction)
 * y: rows of J D float32, ldy >= J D; it may be a column block of the matrix x is a column block of (never an overlapping one).  lo, span:
 * the smallest offset of both arrays and the largest less the smallest, 0 <= span <= SC_CTX_MAX_SPAN and |lo| <= SC_CTX_MAX_SPAN; the
 * offsets themselves are read on the device only, where one outside [lo, lo + span] is clamped into it. */
int sc_ctx_gather(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const int32_t* d_plus,
                  const int32_t* d_minus, int32_t J, int32_t lo, int32_t span, float* d_y, int64_t ldy, void* stream);

/* A temporal basis per coefficient (the DCT of pca_dct without a projection; TRAPs).  d_basis: W x J float64 on the device, row-major.
 *   y[t, c J + j] = sum_w basis[w J + j] x[cl(t + w - left), c],   w ascending, fused multiply-adds in float64, one rounding to float32.
 * 1 <= W <= SC_CTX_MAX_W, 1 <= J <= W, 0 <= left < W; y: rows of D J float32, ldy >= D J. */
int sc_ctx_basis(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const double* d_basis,
                 int32_t W, int32_t J, int32_t left, float* d_y, int64_t ldy, void* stream);

/* The windowed projection on the f64 matrix cores: y (N x Q) = windows (N x W D) . M (W D x Q) without the window matrix.
 *   y[t, q] = sum_k a[t, k] M[k, q],   k = w D + c (time-major),   a[t, k] = x[cl(t + w - left), c] widened to float64,
 * summed by v_mfma_f64_16x16x4_f64 in k-steps of 4, k ascending, one rounding to float32.  d_m: W D x Q float64 on the device,
 * row-major.  1 <= W <= SC_CTX_MAX_W, 0 <= left < W, 1 <= D <= SC_CTX_PROJ_MAX_D, 1 <= Q <= SC_CTX_PROJ_MAX_Q; y: ldy >= Q.
 * Row tiles are per segment: tile i of a segment is its rows [64 i, 64 i + 64). */
int sc_ctx_project(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int64_t max_rows, const double* d_m,
                   int32_t W, int32_t left, int32_t Q, float* d_y, int64_t ldy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_CONTEXT_H */
