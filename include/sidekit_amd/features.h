/* sidekit_amd/features.h -- the feature post-processing extension of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * Four entry points of the same library, under the same conventions (error classes, device pointers, the stream argument).  Like the
 * mixture's and the i-vector's they live in a header of their own, bound by a table of their own (sidekit_amd/_lib.py
 * FEATURES_SIGNATURES): the core header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_FEATURES_H
#define SIDEKIT_AMD_FEATURES_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- RASTA, deltas, moments and normalisation of a stacked ragged batch (sidekit/frontend/normfeat.py, features.py:133-166) -----------
 * x: float32 rows of D coefficients, row r at d_x + r * ldx (ldx >= D).  d_seg_off: S + 1 ascending int64 row offsets on the device;
 * segment s is rows [d_seg_off[s], d_seg_off[s + 1]); empty segments are allowed; the caller vouches that the offsets lie inside the
 * matrix (the entries take no row count and read the offsets on the device only).  Arithmetic is float64 in registers, rounded once to
 * float32 on store.  No atomics; every sum has a fixed order; time is tiled relative to the segment's first row, so a segment's output
 * bits depend on its own rows alone, wherever it lies in the batch.  Arguments are checked (SK_EARG) before anything is enqueued: null
 * pointers, S < 0, D outside [1, SC_FEAT_MAX_D], a leading dimension below D, a bad mode, an even or out-of-range window or filter
 * length, x == y where that is forbidden.  S == 0 enqueues nothing. */
#define SC_FEAT_MAX_TAPS 15       /* sc_feat_delta: the longest filter (2 win + 1 with win up to 7) */
#define SC_FEAT_MAX_WIN 1001      /* sc_feat_norm: the longest window */
#define SC_FEAT_TILE 256          /* rows of one tile of sc_feat_norm / sc_feat_delta: tile i of a segment is its rows [256 i, 256 i + 256) */
#define SC_FEAT_COLS 16           /* columns of one tile */
#define SC_FEAT_MAX_D 1048560     /* 65535 column chunks of 16 */

#define SC_FEAT_CENTER 0
#define SC_FEAT_CENTER_REDUCE 1
#define SC_FEAT_SLIDING_CENTER 2
#define SC_FEAT_SLIDING_CENTER_REDUCE 3
#define SC_FEAT_WARP 4

/* rasta_filt (normfeat.py:45-74) per segment and column, t counted from the segment's first row: y[t] = 0 for t < 4;
 * u[t] = 0.2 x[t] + 0.1 x[t-1] - 0.1 x[t-3] - 0.2 x[t-4], y[t] = u[t] + 0.94 y[t-1] for t >= 4 (y[3] = 0).  The rows from 4 on are cut
 * into 16 runs of 32 per pass of 512; a run's end state from a zero start and 0.94^32 give every run its carry, in run order.
 * d_y != d_x. */
int sc_feat_rasta(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, float* d_y, int64_t ldy, void* stream);

/* compute_delta as the reference executes it (numpy.convolve(column, filt)[win:-win], L = 2 win + 1): a 'same' convolution with zeros
 * outside the segment, y[t] = sum_k filt[k] x[t + (L - 1) / 2 - k], k ascending.  d_filt: L float64 taps on the device, L odd in
 * [1, SC_FEAT_MAX_TAPS].  d_x and d_y may be different column blocks of one matrix, never overlapping ones (d_y != d_x is checked). */
int sc_feat_delta(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, const double* d_filt, int32_t L, float* d_y,
                  int64_t ldy, void* stream);

/* d_mean, d_std: S x D float64, the mean and the population standard deviation (ddof = 0, two passes) of each segment's rows; an empty
 * segment gets mean 0 and std 1. */
int sc_feat_moments(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, double* d_mean, double* d_std, void* stream);

/* Normalisation of segments whose rows are the speech frames.  n: the segment's rows, h = (win - 1) / 2; win odd in [3, SC_FEAT_MAX_WIN]
 * (read and checked by the three windowed modes only).
 *   SC_FEAT_CENTER / SC_FEAT_CENTER_REDUCE   y = x - mean[s], y = (x - mean[s]) / std[s]   (d_mean, d_std: S x D; plain IEEE, a zero std gives inf / nan)
 *   SC_FEAT_SLIDING_*, n <= win              the same from the tables (the reference's fallback to cms / cmvn)
 *   SC_FEAT_SLIDING_*, n > win               the window of row t is rows [lo, lo + win), lo = min(max(t - h, 0), n - win); y = x[t] - mean_w,
 *                                            divided by the window's SAMPLE standard deviation (ddof = 1) for _REDUCE; both summed
 *                                            directly over the window, index ascending, two passes
 *   SC_FEAT_WARP                             w = win for n >= win, else n (odd n) or n + 1 (even n, the last row counted twice);
 *                                            m = max(n, w); lo = min(max(t - (w - 1) / 2, 0), m - w); c = the number of window
 *                                            values strictly below x[t]; y = normcdfinv((c + 0.5) / w).  d_mean, d_std may be null.
 * d_std may be null for the modes that do not divide.  d_y != d_x for the three windowed modes. */
int sc_feat_norm(const float* d_x, int64_t ldx, const int64_t* d_seg_off, int32_t S, int32_t D, int32_t mode, int32_t win, const double* d_mean,
                 const double* d_std, float* d_y, int64_t ldy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_FEATURES_H */
