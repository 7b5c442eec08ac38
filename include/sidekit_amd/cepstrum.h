/* sidekit_amd/cepstrum.h -- the cepstral front end of the C ABI of libsidekit_amd.so (../sidekit_amd.h).
 *
 * One entry point of the same library, under the same conventions (error classes, device pointers, the stream argument).  Like the
 * feature post-processing's it lives in a header of its own, bound by a table of its own (sidekit_amd/_lib.py CEPSTRUM_SIGNATURES):
 * the core header and its table are pinned symbol for symbol. */
#ifndef SIDEKIT_AMD_CEPSTRUM_H
#define SIDEKIT_AMD_CEPSTRUM_H
#include "../sidekit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SC_MFCC_MAX_FILT 128      /* the most filters of a bank */

/* ---- log-energy, log filter-bank outputs and cepstra of a ragged batch (sidekit/frontend/features.py: power_spectrum, mfcc) ---------
 * d_wav: B rows of wav_ld samples, XT_F32 or XT_I16 (wav_dtype); a sample is widened to double, multiplied by `scale` and rounded to
 * float32 on load (the reference works at the int16 scale: scale = 1).  d_nsamples: int32 [B], the samples of each row (a value above
 * wav_ld is read as wav_ld).  d_frame_off: int64 [B + 1], ascending row offsets of the stacked output; utterance b owns rows
 * [off[b], off[b + 1]) and off[b + 1] - off[b] = max((n_b - nwin) / shift + 1, 0); N = off[B] is passed by the host.  A row whose
 * frame would leave its utterance's samples is not written.
 *
 * Frame t of utterance b is samples x[0 .. nwin) from t * shift on.  In float32:
 *   y[0] = x[0] - p x[0], y[j] = x[j] - p x[j - 1]            (p = prefac rounded to float32; product rounded, then the difference)
 *   energy = log(sum_j y[j]^2)
 *   X = rfft(window * y, n_fft), P[k] = re^2 + im^2, k = 0 .. n_fft / 2
 *   fb[i] = log(sum_k bank[i][k] P[k]), k ascending over [bank_lo[i], bank_hi[i])
 *   cep[c] = sum_i dct[c][i] fb[i], i ascending
 * The logs are plain IEEE: a zero argument gives -inf.  d_window: nwin float32.  d_bank: float32 [nfilt][n_fft / 2 + 1] dense;
 * d_bank_lo / d_bank_hi: int32 [nfilt], the first and one-past-last non-zero bin of each filter (clamped to the row by the kernel).
 * d_dct: float32 [nceps][nfilt].
 *
 * d_out: float32 rows [N][ld], ld >= 1 + nceps + nfilt; columns energy | cep | fb; columns beyond those are not touched.
 * d_spec: null, or float32 rows [N][lds], lds >= n_fft / 2 + 1, which receive P.
 *
 * No atomics; every sum has a fixed order; a frame's bits depend on its own samples and the tables alone, so an utterance gives the
 * same bits alone or anywhere in a batch, and as XT_I16 or as XT_F32 holding the same integers.
 * Checked (SK_EARG) before anything is enqueued: null pointers, a wav_dtype other than XT_F32 / XT_I16, B < 1, N < 0, n_fft not in
 * {256, 512}, nwin outside [n_fft / 2 + 1, n_fft], shift outside [1, nwin], nfilt outside [1, SC_MFCC_MAX_FILT], nceps outside
 * [1, nfilt - 1], wav_ld < 1, ld < 1 + nceps + nfilt, lds < n_fft / 2 + 1 with d_spec given.  N == 0 enqueues nothing. */
int sc_mfcc(const void* d_wav, int32_t wav_dtype, int64_t wav_ld, double scale, const int32_t* d_nsamples, const int64_t* d_frame_off, int32_t B,
            int64_t N, int32_t nwin, int32_t shift, int32_t n_fft, double prefac, const float* d_window, const float* d_bank,
            const int32_t* d_bank_lo, const int32_t* d_bank_hi, int32_t nfilt, const float* d_dct, int32_t nceps, float* d_out, int64_t ld,
            float* d_spec, int64_t lds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_CEPSTRUM_H */
