/* sidekit_amd C ABI -- MI355X (gfx950) x-vector extraction and trial scoring.
 *
 * The reference (deep-privacy/sidekit) is pure Python and has no FFI layer: the drop-in boundary
 * is its Python API.  This header is the C ABI that sits underneath the Python
 * mirror in `sidekit_amd/` -- plain pointers and sizes, no torch types.  Each entry point names
 * the reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - every function returns 0 on success, a negative SK_E* class otherwise; the message is
 *     available from xt_last_error() (thread-local).  No exception crosses the ABI.
 *   - `d_` pointers are device (HIP) pointers owned by the caller, `h_` pointers are host memory.
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on that stream.
 *   - a handle is bound to the device current at xt_create(); handles on different devices are independent (one process per GPU).
 *   - streams: consecutive calls on one handle may arrive on DIFFERENT streams.  The handle's workspaces are reused from call to call;
 *     the library orders that reuse itself: every call that touches a workspace (xt_forward*, xt_forward_begin, xt_forward_features,
 *     xt_features) records an event on the stream it was given, and a call that arrives on another stream first makes its stream wait for
 *     that event and for every batch still in flight on the handle's own streams.  (The caller still orders its own buffers: d_wav must be
 *     ready, and d_emb is complete, in the order of the stream passed.)
 *   - threads: one host thread at a time per handle.  A second thread that enters a handle while another is inside gets SK_ESTATE and
 *     nothing is enqueued; use one handle per driving thread (the reference, too, drives a model from one thread: SURVEY 8b).
 */
#ifndef SIDEKIT_AMD_H
#define SIDEKIT_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_OK 0
#define SK_EARG (-1)       /* bad argument            -> AssertionError / ValueError in the shim */
#define SK_ESHAPE (-2)     /* shape / key mismatch    -> RuntimeError (as torch load_state_dict) */
#define SK_EHIP (-3)       /* HIP runtime error       -> RuntimeError                            */
#define SK_EWORKSPACE (-4) /* batch exceeds xt_reserve -> RuntimeError                           */
#define SK_ESTATE (-5)     /* call order (e.g. forward before finalize), concurrent entry -> RuntimeError */

enum { XT_ARCH_HALFRESNET34 = 0, XT_ARCH_TDNN = 1 };
enum { XT_F32 = 0, XT_BF16 = 1, XT_F64 = 2, XT_I64 = 3, XT_I16 = 4 };
enum { XT_LOSS_AAM = 0, XT_LOSS_CCE = 1 };

typedef struct xt_handle xt_handle;

/* Mirrors the arguments of sidekit.nnet.xvector.Xtractor.__init__ (sidekit/nnet/xvector.py:424-431)
 * that matter at inference, plus the compute dtype of the trunk. */
typedef struct xt_config {
  int32_t arch;     /* XT_ARCH_*: model_archi "halfresnet34" (xvector.py:569-599) | "xvector" (:453-513) */
  int32_t dtype;    /* XT_F32 (parity path, exact-f32 MFMA) | XT_BF16 (bf16 MFMA, f32 accumulate)     */
  int32_t loss;     /* XT_LOSS_AAM | XT_LOSS_CCE                                                      */
  int32_t n_spk;    /* speaker_number                                                                 */
  int32_t emb_dim;  /* embedding_size (256)                                                           */
  float aam_s;      /* ArcMarginProduct scale: 30 (halfresnet34) / 64 (xvector)                       */
} xt_config;

/* Xtractor(...) : build an empty model on the current device. */
int xt_create(const xt_config* cfg, xt_handle** out);
int xt_destroy(xt_handle* h);

/* Xtractor.load_state_dict (sidekit/bin/extract_xvectors.py:86, strict=True): hand over one
 * checkpoint tensor by its reference key name (host memory, contiguous, row-major `shape`).
 * dtype: XT_F32, or XT_I64 for the `num_batches_tracked` counters.  Unknown keys and wrong shapes
 * fail with SK_ESHAPE. */
int xt_set_tensor(xt_handle* h, const char* key, const void* h_data, const int64_t* shape, int32_t ndim, int32_t dtype);
/* Number of keys / i-th key name the architecture expects (for strict checking in the shim). */
int xt_num_keys(xt_handle* h);
const char* xt_key_name(xt_handle* h, int32_t i);
/* Fold BatchNorm, repack to kernel layouts, upload.  Fails with SK_ESHAPE naming the first missing key. */
int xt_finalize(xt_handle* h);

/* Size the device workspace for a batch shape of max_batch utterances x max_samples samples each (TDNN: max_batch x
 * max_samples bounds the total).  Buffers only grow; a later forward runs when ONE reserved shape covers its batch in
 * both dimensions, so reserving (256, 64000) and (1, 20000000) sizes the workspace for those two products, not for
 * 256 x 20000000. */
int xt_reserve(xt_handle* h, int32_t max_batch, int64_t max_samples);

/* Xtractor.forward(x, is_eval=True) (sidekit/nnet/xvector.py:876-907).
 *   d_wav       float32 [B][wav_ld] waveform, utterance b uses its first h_nsamples[b] samples
 *   h_nsamples  NULL = every utterance has L samples
 *   d_emb       float32 [B][emb_dim]  L2-normalised x-vectors (tuple slot 1 of the reference)
 *   d_logits    float32 [B][n_spk] s*cos logits (tuple slot 0), or NULL to skip them */
int xt_forward(xt_handle* h, const float* d_wav, int64_t wav_ld, const int32_t* h_nsamples, int32_t B, int64_t L,
               float* d_emb, float* d_logits, void* stream);

/* Same, for 16-bit PCM as the files hold it: the decode of the reference driver (sidekit/bin/extract_xvectors.py:57-70,
 * soundfile.read -> float32 = int16 / 32768) happens inside the front-end kernel's load, so a wav file's payload goes
 * disk -> pinned memory -> device -> STFT without a conversion pass on either side.  x-vectors are bit-identical to
 * xt_forward on the widened samples.  d_pcm int16 [B][pcm_ld]. */
int xt_forward_pcm16(xt_handle* h, const int16_t* d_pcm, int64_t pcm_ld, const int32_t* h_nsamples, int32_t B, int64_t L,
                     float* d_emb, float* d_logits, void* stream);

/* Pipelined forwards: two WHOLE batches in flight instead of the two halves of one.  The reference driver's loop
 * (sidekit/bin/extract_xvectors.py:130-150) is one forward at a time; a corpus is many independent batches, and two of them half a step
 * apart use the chip better than one alone (one batch's HBM-bound first layer beside the other's MFMA-bound deep layers: 5.67 vs 5.87 ms
 * per batch of 256 on MI355X).  xt_reserve_slots sizes `slots` (<= 4; 2 is what pays) full workspaces, each with a stream the handle
 * owns.  xt_forward_begin queues the whole forward of a batch on slot `slot`'s stream -- behind everything queued on `stream` so far --
 * and returns without joining; in_dtype XT_F32 (d_wav float32) or XT_I16 (16-bit PCM as in xt_forward_pcm16).  xt_forward_end makes
 * `stream` wait for that slot's last forward: d_emb / d_logits are complete behind it.  A slot's forwards run in the order they were
 * begun; reusing a slot before its previous batch was ended is allowed only if the caller no longer needs that batch's outputs.
 * x-vectors are the bits xt_forward gives (tests/test_gpu_fullsize.py::test_pipelined_forwards_are_bit_identical). */
int xt_reserve_slots(xt_handle* h, int32_t slots, int32_t max_batch, int64_t max_samples);
int xt_forward_begin(xt_handle* h, int32_t slot, const void* d_wav, int32_t in_dtype, int64_t wav_ld, const int32_t* h_nsamples, int32_t B,
                     int64_t L, float* d_emb, float* d_logits, void* stream);
int xt_forward_end(xt_handle* h, int32_t slot, void* stream);

/* Same, entered after the front-end (everything after xvector.py:885): the features->embedding
 * seam the parity fixtures are cut at.  d_feats float32 (B, 80, T) as MelSpecFrontEnd / MfccFrontEnd
 * return it; h_frames NULL = all T. */
int xt_forward_features(xt_handle* h, const float* d_feats, const int32_t* h_frames, int32_t B, int32_t T,
                        float* d_emb, float* d_logits, void* stream);

/* Front-end only: MelSpecFrontEnd.forward(is_eval=True) (sidekit/nnet/preprocessor.py:267-285) or
 * MfccFrontEnd.forward (:113-124).  d_feats_out float32 (B, 80, T), T = 1 + L / hop. */
int xt_features(xt_handle* h, const float* d_wav, int64_t wav_ld, const int32_t* h_nsamples, int32_t B, int64_t L,
                float* d_feats_out, void* stream);

/* forward(..., norm_embedding=False) (xvector.py:876,893-898): only observable for loss='cce', whose
 * eval output is then the un-normalised linear6 output; the 'aam' branch always normalises (:903). */
int xt_set_norm_embedding(xt_handle* h, int32_t on);

/* Split forward.  With lanes = n (default 2, at most 4; SIDEKIT_AMD_LANES in the environment or xt_set_lanes) a HalfResNet34 batch
 * of >= 128 utterances is forwarded as up to n parts of at least 64 utterances on n HIP streams, all of them owned by the handle
 * (the caller's stream only forks and joins): one part's latency-bound kernels run under another part's convolutions.  Results do not change (every kernel is batch-size
 * invariant).  lanes = 1 serialises the forward again, for profiles in which one kernel's duration has to mean something.  Measured on MI355X: two and three
 * lanes are 1-4 % faster than one, FOUR are slower (a constant +2.3 ms per forward: the fourth lane's stream shares a hardware queue).
 * The reference has no counterpart: its forward is one
 * stream of cuDNN calls (sidekit/nnet/xvector.py:876-907). */
int xt_set_lanes(xt_handle* h, int32_t lanes);
int xt_get_lanes(xt_handle* h);

/* Diagnostics for stage-wise parity tests: keep a device copy of intermediate activations of the
 * next forward ("feats", "stem", "layer1".."layer4", "pooled", "pre_norm", TDNN: "conv1".."conv5").
 * xt_debug_tap copies one to host (raw element type of the trunk: f32, or bf16 for XT_BF16 trunk
 * activations) and returns its byte size in *bytes. */
int xt_set_debug(xt_handle* h, int32_t on);
int xt_debug_tap(xt_handle* h, const char* name, void* h_dst, size_t capacity, size_t* bytes);

/* Measurement: when on, every kernel launch of the forward is bracketed by HIP events recorded on
 * the launch stream.  xt_get_profile synchronises and returns, per slot, the summed device time (ms)
 * and the number of launches since the last reset.  Slots 0, 2, 4, 5, 7, 8, 10 are the 3x3 trunk convolution
 * shapes L1, L2a, L2, L3a, L3, L4a, L4; slots 1, 3, 6, 9 (once the layers' stand-alone 1x1 shortcut convolutions) are
 * unused and stay zero since the shortcut runs in the epilogue of the block's second convolution.
 * `on`: 0 = off, 1 = every slot, otherwise a mask with bit (slot + 1) set for each slot to bracket -- an event pair
 * costs about 2 us of stream time, so a timed run brackets only the class it reports (bench.py: the dominant one). */
#define XT_PROF_FRONTEND 11
#define XT_PROF_STEM 12
#define XT_PROF_SE_RES 13
#define XT_PROF_POOL_TAIL 14
#define XT_PROF_TDNN 15
#define XT_PROF_SLOTS 16
int xt_set_profile(xt_handle* h, int32_t on);
int xt_get_profile(xt_handle* h, double* ms /*[XT_PROF_SLOTS]*/, int64_t* launches /*[XT_PROF_SLOTS]*/, int32_t reset);

/* Tuning harness (diagnostic): mean device ms of `iters` launches of trunk convolution `shape` (slot order of
 * xt_get_profile) on a B x T batch; variant bit0 = no stores, bit1 = no MFMA loop, bit2 = no staging, bit4 = residual epilogue (conv2 of a block), otherwise
 * the statistics epilogue runs (conv1 of a block; bit3, which once selected it, is accepted and implied), bit5 = one workgroup per tile even for the persistent
 * shapes, bit6 = print the runtime's occupancy for the kernel; shapes 0, 2, 4, 5, 7, 8, 10 are the trunk's seven (2, 5, 8, the stride-2 first convolutions,
 * have no residual form), 42 / 43 the small-grid tilings of layers 3 / 4, which have the residual form only (csrc/conv3x3.hip). */
int sk_bench_conv(int32_t shape, int32_t dtype, int32_t B, int32_t T, int32_t iters, int32_t variant, float* ms_out,
                  double* phase_cycles /* [8] mean shader cycles per kernel phase, or NULL */);

/* One trunk block on caller-supplied input (diagnostic; not used by the product path): exactly the launches the forward makes for block
 * `block` (0..15) of a finalised HalfResNet34 handle, with the handle's own packed weights -- conv1 in statistics form, the SE gate, conv2
 * in residual form (first block of a layer: with the 1x1 shortcut in its epilogue).
 *   d_x       block input, NHWC in the handle's compute type: [B][halve(T, lin)][W_in][C_in] (lin: stride-2 stages before the input)
 *   h_frames  feature frames per utterance, NULL = all T
 *   form      0 = batch tiling; 1 = small-grid tiling of conv2 (bf16 layers 3 and 4 only, SK_EARG elsewhere)
 *   d_o1      relu(bn1(conv1(x))), [B][H_out][W_out][C] in the compute type;  d_gate  the SE gate, float32 [B][C];  d_out  the block output
 * Rows past an utterance's length are not written: the caller pre-fills the outputs.  Scratch is allocated and released inside the call,
 * which returns after the launches have completed. */
int xt_debug_block(xt_handle* h, int32_t block, const void* d_x, const int32_t* h_frames, int32_t B, int32_t T, int32_t form, void* d_o1,
                   float* d_gate, void* d_out, void* stream);

const char* xt_last_error(void);

/* Sample-rate conversion of one utterance on the device: `torchaudio.transforms.Resample(orig_freq, new_freq)` as
 * sidekit/bin/extract_xvectors.py:141-143 applies it to a file whose rate differs from the model's (torchaudio 0.8.2, un-vendored:
 * windowed-sinc interpolation, lowpass_filter_width 6, roll-off 0.99 -- restated from the published algorithm, parity unpinned).
 * d_in: n_in samples, XT_F32 or XT_I16 (widened as x / 32768); *n_out = ceil(new * n_in / orig) after reducing the rates by their
 * gcd; d_out = NULL only queries *n_out. */
int sk_resample(const void* d_in, int32_t in_dtype, int64_t n_in, int32_t orig_freq, int32_t new_freq, float* d_out,
                int64_t out_capacity, int64_t* n_out, void* stream);

/* ---- speech activity: energy VAD and chunk gathering (csrc/vad.hip) --------------------------------------------------------------
 * What `extract_xvectors.py --vad` does to a signal before the forward (sidekit/bin/extract_xvectors.py:98-151): find speech, keep only
 * those samples.  The detector is the reference's own energy VAD (sidekit/mixture.py:67-113 on the log-energy of
 * sidekit/frontend/features.py:363-389, smoothed by label_fusion, sidekit/frontend/vad.py:409-428); timestamps from any detector (the
 * reference's `<out>_vad.json` cache) are applied by sk_collect_segments.  float64 throughout, fixed-order reductions, no atomics: the
 * bits are a function of the arguments alone. */

/* power_spectrum's log-energy.  d_wav [B][wav_ld], XT_F32 or XT_I16 (widened as x / 32768); d_nsamples: B sample counts on the device
 * (clamped to [0, wav_ld]).  Utterance b has nframes = (n - nwin) / shift + 1 frames (0 if n < nwin: the reference's `framing` is not
 * defined there); frame t is samples [t shift, t shift + nwin), pre-emphasised inside the frame (y[0] = x[0] - prefac x[0],
 * y[j] = x[j] - prefac x[j-1]); d_le[b][t] = log(sum_j y[j]^2), float64 [B][T_ld] (columns from nframes[b] on are zero),
 * T_ld >= the frames of wav_ld samples.  d_nframes: int32 [B]. */
int sk_frame_log_energy(const void* d_wav, int32_t in_dtype, int64_t wav_ld, const int32_t* d_nsamples, int32_t B, int32_t nwin, int32_t shift,
                        double prefac, double* d_le, int32_t T_ld, int32_t* d_nframes, void* stream);

/* vad_energy(log_energy, distrib_nb=3, nb_train_it=n_iter, flooring, ceiling, alpha) per utterance, then label_fusion(win=fusion_win)
 * (0 = none, else odd, 3..255: grey closing followed by grey opening, scipy's 'reflect' boundary).  d_label uint8 [B][T_ld] (0 beyond
 * nframes[b]); d_threshold float64 [B], in units of the standardised log-energy.  The first E-step runs with the reference's constant term
 * A = 0 (its Mixture is scored before _compute_all ever ran).  Degenerate utterances -- no frame, zero or non-finite standard deviation
 * (any non-finite log-energy), a NaN threshold, or no frame left labelled after the fusion -- keep ALL their frames and report a NaN
 * threshold: the driver's `len(speech_timestamps) == 0` fallback (extract_xvectors.py:137-138). */
int sk_vad_energy(const double* d_le, const int32_t* d_nframes, int32_t B, int32_t T_ld, int32_t n_iter, double flooring, double ceiling, double alpha,
                  int32_t fusion_win, uint8_t* d_label, double* d_threshold, void* stream);

/* Keep sample s of utterance b iff d_label[b][min(s / shift, nframes[b] - 1)] is set (an utterance without a frame is kept whole): the
 * kept samples go to d_dst[b][0 .. out_len[b]), same element type (XT_F32 / XT_I16) as d_src; the rest of a dst row is not written.
 * dst_ld >= src_ld; dst may not overlap src.  d_out_len: int32 [B] on the device.  The reference's x-vector path has no label-to-sample
 * rule (its labels select feature frames); this one makes frame t own samples [t shift, (t + 1) shift) and the last frame the tail. */
int sk_collect_labels(const void* d_src, int32_t dtype, int64_t src_ld, const int32_t* d_nsamples, const uint8_t* d_label, int32_t T_ld,
                      const int32_t* d_nframes, int32_t B, int32_t shift, void* d_dst, int64_t dst_ld, int32_t* d_out_len, void* stream);

/* collect_chunks(speech_timestamps, signal) for a batch: utterance b keeps the sample ranges [seg[2 i], seg[2 i + 1]) for i in
 * [seg_off[b], seg_off[b + 1]), concatenated in d_dst[b][0 ..).  The CSR is passed twice: the host copy (h_nsamples, h_seg_off [B + 1],
 * h_seg [2 n]) is validated before anything is enqueued -- 0 <= start <= end <= nsamples[b], ascending, no overlap, kept total <= dst_ld;
 * anything else is SK_EARG -- and the device copy (d_seg_off, d_seg: the same numbers, uploaded by the caller in the order of `stream`)
 * is what the kernel reads.  h_out_len (B, may be NULL) receives the kept lengths: no read-back on this path. */
int sk_collect_segments(const void* d_src, int32_t dtype, int64_t src_ld, const int32_t* h_nsamples, const int32_t* h_seg_off, const int32_t* h_seg,
                        const int32_t* d_seg_off, const int32_t* d_seg, int32_t B, void* d_dst, int64_t dst_ld, int32_t* h_out_len, void* stream);

/* ---- trial scoring ------------------------------------------------------------------------- */

/* sidekit.iv_scoring.cosine_scoring, the einsum of sidekit/iv_scoring.py:108-109: rows already
 * L2-normalised by the caller (StatServer.norm_stat1).  d_out[i][j] = <E_i, T_j>, float32.  D % 4 == 0, and d_E / d_T on 16-byte
 * boundaries (rows are read with 16-byte loads): SK_EARG otherwise, here and in sc_cosine_hist, sc_cosine_hist_norm and sc_cohort_moments. */
int sc_cosine(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, float* d_out, void* stream);

/* sidekit.iv_scoring.fast_PLDA_scoring, sidekit/iv_scoring.py:448-462:
 *   out[i][j] = scaling * ( 0.5 e_i' Phi e_i + 0.5 t_j' Phi t_j + cst + e_i' Psi t_j ),  float64.
 * Phi, Psi (D x D, row-major) and cst come from the 256x256 float64 algebra that stays on the
 * host (iv_scoring.py:428-446).  E, T are the centred (and optionally Vtrans-rotated) vectors. */
int sc_plda_fast(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi,
                 const double* d_Psi, double cst, double scaling, double* d_out, void* stream);

/* torch.nn.functional.normalize(x, dim=1) (eps 1e-12) on the device: what the reference applies to cohort and test x-vectors before
 * cosine scoring (sidekit/score_normalization.py:128, sidekit/nnet/xvector.py:243,258-259).  d_out may alias d_X. */
int sc_normalize_rows(const float* d_X, int32_t N, int32_t D, float* d_out, void* stream);

/* sc_plda_fast (and sc_plda_hist) keeps its intermediate buffer (E.Psi and the quadratic-form partials) cached per (device, stream) so that a call
 * allocates nothing; this frees every cached buffer (after a device synchronise).  The Python shim calls it at interpreter exit;
 * a long-lived host that creates and destroys many streams may call it whenever no sc_plda_fast call is in flight.  The reference
 * has no counterpart (its temporaries are numpy arrays, sidekit/iv_scoring.py:449-460). */
int sc_release_workspace(void);

/* All-pairs cosine scoring without the score matrix (100k x 100k trials = 40 GB of float32): the scores of
 * sc_cosine are classified target (labels_e[i] == labels_t[j]) / non-target and counted into two histograms of `nbins`
 * (= 8192) equal bins over [lo, hi) (out-of-range scores land in the end bins); self_offset >= 0 drops the trials
 * j == i + self_offset, i.e. the self-trials when E is rows [self_offset, self_offset + Ne) of T (a set, or one rank's row
 * shard of it, scored against itself: the trials sidekit/nnet/xvector.py:240-262 masks out through its Ndx); < 0 keeps all.
 * The EER of the binned scores follows on the host (sidekit_amd.bosaris.detplot.eer_from_histograms). */
int sc_cosine_hist(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e,
                   const int32_t* d_labels_t, int32_t self_offset, float lo, float hi, int32_t nbins, uint64_t* d_hist_tar,
                   uint64_t* d_hist_non, void* stream);

/* The same histograms of cohort-normalised scores: every score of sc_cosine goes through the expression of sc_norm_apply before it
 * is binned -- the enrolment pair alone (z-norm) (s - mean_e[i]) / std_e[i], the test pair alone (t-norm) (s - mean_t[j]) / std_t[j],
 * both (s-norm, adaptive or not) 0.5 ((s - mean_e[i]) / std_e[i]) + 0.5 ((s - mean_t[j]) / std_t[j]) -- with IEEE float32 operations in
 * that order, so the counts are exactly those of sc_cosine + sc_norm_apply + binning the matrix, which is never formed.  d_mean_e /
 * d_std_e: Ne entries, d_mean_t / d_std_t: Nt entries (sc_cohort_moments or sc_topk_stats produce them); a mean and its std come
 * together and at least one pair is given, anything else is SK_EARG.  A score that normalises to NaN (a zero or non-finite std) has no
 * defined bin (the conversion to an integer comes before the clamp; today it is counted in bin 0, and +-inf in the end bins, as in
 * sc_cosine_hist): callers check the stds first (sidekit_amd.iv_scoring.cosine_histograms does).  Everything else -- labels, self_offset, lo / hi /
 * nbins, the stream contract -- is sc_cosine_hist's.  zt-norm (t-norm against a z-normalised cohort) is a different chain and not here. */
int sc_cosine_hist_norm(const float* d_E, int32_t Ne, const float* d_T, int32_t Nt, int32_t D, const int32_t* d_labels_e,
                        const int32_t* d_labels_t, int32_t self_offset, const float* d_mean_e, const float* d_std_e,
                        const float* d_mean_t, const float* d_std_t, float lo, float hi, int32_t nbins, uint64_t* d_hist_tar,
                        uint64_t* d_hist_non, void* stream);

/* All-pairs PLDA scoring without the score matrix (100k x 100k float64 trials = 80 GB): the log-likelihood ratios of
 * sidekit/iv_scoring.py:448-462, each the double sc_plda_fast would have stored for the pair (the same preparation launch, the same
 * f64 MFMA chain over ascending k, the same epilogue expression from left to right), are classified and counted as sc_cosine_hist
 * counts cosine scores: the counts are those of sc_plda_fast + binning the matrix, which is never formed.  E, T, Phi, Psi, cst and
 * scaling are sc_plda_fast's.  The bin of a score v is taken in float64, x = (v - lo) * (nbins / (hi - lo)), and clamped before the
 * conversion to an integer: x < 0 is bin 0, x >= nbins the last bin, so +-inf lands in an end bin; a NaN score is counted nowhere and
 * shows as a missing trial in the total.  Log-likelihood ratios have no natural range: lo and hi are finite, hi > lo, nbins = 8192,
 * anything else (or a null pointer, or a size <= 0) is SK_EARG before anything is enqueued.  Only integer atomics are used: the
 * counts are a function of the arguments alone.  Labels, self_offset, the zeroing of the counters on the stream and the stream
 * contract are sc_cosine_hist's; the intermediate buffer is sc_plda_fast's (sc_release_workspace). */
int sc_plda_hist(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                 double cst, double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset, double lo,
                 double hi, int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream);

/* The same histograms of cohort-normalised PLDA scores: what sc_cosine_hist_norm is to sc_cosine_hist.  Every score is the double
 * sc_plda_hist forms and goes through the expression of sc_norm_apply_f64 for the mode (the enrolment pair alone, the test pair alone,
 * or both), with IEEE float64 operations in that order, before sc_plda_hist's float64 binning: the counts are exactly those of
 * sc_plda_fast + sc_norm_apply_f64 + binning the matrix, which is never formed.  d_mean_e / d_std_e: Ne entries, d_mean_t / d_std_t: Nt
 * entries (sc_plda_cohort_moments or sc_topk_stats_f64 produce them); a mean and its std come together and at least one pair is given,
 * anything else is SK_EARG.  A normalised score that is not finite (a zero std gives +-inf or NaN) has no bin and shows as a missing
 * trial in the total: callers check the stds first (sidekit_amd.iv_scoring.plda_histograms does).  Everything else is sc_plda_hist's.
 * zt-norm is not here. */
int sc_plda_hist_norm(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                      double cst, double scaling, const int32_t* d_labels_e, const int32_t* d_labels_t, int32_t self_offset,
                      const double* d_mean_e, const double* d_std_e, const double* d_mean_t, const double* d_std_t, double lo, double hi,
                      int32_t nbins, uint64_t* d_hist_tar, uint64_t* d_hist_non, void* stream);

/* Speaker-mean enrolment + cosine over a listed trial set, sidekit/bin/compute_spk_cosine.py:18-26:
 * out[k] = <E[enr_idx[k]], T[tst_idx[k]]> / (|E| |T|), float32 in, float64 maths. */
int sc_cosine_trials(const float* d_E, const float* d_T, int32_t D, const int32_t* d_enr_idx, const int32_t* d_tst_idx,
                     int64_t n_trials, double* d_out, void* stream);

/* Adaptive symmetric score normalisation, sidekit.score_normalization.asnorm (sidekit/score_normalization.py:120-140).
 * sc_topk_stats: per row of a (n_rows x n_cols) float32 score matrix, mean and unbiased std of its k largest values
 * (the reference's `topk(200, dim=1)` + mean/std).  sc_snorm_apply: S[i][j] <- 0.5 ((S - mean_e[i]) / std_e[i] +
 * (S - mean_t[j]) / std_t[j]) in place. */
int sc_topk_stats(const float* d_scores, int32_t n_rows, int32_t n_cols, int32_t k, float* d_mean, float* d_std, void* stream);
int sc_snorm_apply(float* d_S, int32_t Ne, int32_t Nt, const float* d_mean_e, const float* d_std_e, const float* d_mean_t,
                   const float* d_std_t, void* stream);

/* Cohort score normalisation: znorm / tnorm / ztnorm (sidekit/score_normalization.py:44-117) and s-norm of an enrolment x test
 * trial matrix (the general form of :120-140).
 *
 * sc_cohort_moments: for every row i of X (N x D) the mean and the population standard deviation (numpy's .std(), :69,90) of
 *   v_ij = (<X_i, C_j> - col_shift[j]) * col_scale[j]    over the M cohort rows j   (col_shift = col_scale = NULL: shift 0, scale 1),
 * formed from the accumulators of sc_cosine's GEMM: the N x M cohort score matrix is never written.  self_offset >= 0 drops the
 * pair j == i + self_offset (X is rows [self_offset, self_offset + N) of C, the convention of sc_cosine_hist; the divisor of such a
 * row is M - 1: the diagonal-free statistics of :64-66), < 0 keeps every pair.  The sums are float64, added in an order that depends
 * on M alone (partials through the sc_* workspace, no floating-point atomics); the variance is clamped at 0.  D % 4 == 0.
 * M == 0, or a row that keeps no pair, is SK_EARG; N == 0 does nothing. */
int sc_cohort_moments(const float* d_X, int32_t N, const float* d_C, int32_t M, int32_t D, const float* d_col_shift,
                      const float* d_col_scale, int32_t self_offset, float* d_mean, float* d_std, void* stream);

/* In place, S: Ne x Nt.  Both pairs: the s-norm of sc_snorm_apply (the same bits).  The enrolment pair alone (d_mean_t = d_std_t =
 * NULL): S[i][j] <- (S[i][j] - mean_e[i]) / std_e[i], z-norm (:70, applied per model).  The test pair alone:
 * S[i][j] <- (S[i][j] - mean_t[j]) / std_t[j], t-norm (:91).  Neither: SK_EARG.  A zero std gives the inf / NaN IEEE division gives,
 * as in the reference. */
int sc_norm_apply(float* d_S, int32_t Ne, int32_t Nt, const float* d_mean_e, const float* d_std_e, const float* d_mean_t,
                  const float* d_std_t, void* stream);

/* Cohort normalisation of PLDA log-likelihood ratios, float64 throughout (what score_normalization.py's znorm / tnorm / asnorm applied
 * to fast_PLDA_scoring output amount to).
 *
 * sc_plda_cohort_moments: for every row i of X (N x D, centred as sc_plda_fast takes them) the mean and the population standard
 * deviation of
 *   v_ij = scaling * (0.5 x_i' Phi x_i + 0.5 c_j' Phi c_j + cst + x_i' Psi c_j)    over the M cohort rows j,
 * each the double sc_plda_fast(X, C) would store at [i][j] (the same preparation launch, the same f64 MFMA chain over ascending k, the
 * same epilogue expression); the N x M matrix is never written.  self_offset is sc_cohort_moments': >= 0 drops the pair
 * j == i + self_offset (divisor M - 1 for such a row), < 0 keeps every pair.  The sums are float64 (s1 += v, s2 = fma(v, v, s2)), added
 * in an order that depends on M alone (partials through the sc_* workspace, no floating-point atomics); the variance is clamped at 0.
 * The statistics of the TEST side of a trial, s(c_j, t_i) with cross term t_i' Psi' c_j, are this call with the transpose of Psi.
 * N == 0 does nothing; M <= 0, D <= 0, a null pointer with N > 0, or a row that keeps no pair is SK_EARG before anything is enqueued.
 * The stream contract and the intermediate buffer are sc_plda_fast's. */
int sc_plda_cohort_moments(const double* d_X, int32_t N, const double* d_C, int32_t M, int32_t D, const double* d_Phi,
                           const double* d_Psi, double cst, double scaling, int32_t self_offset, double* d_mean, double* d_std,
                           void* stream);

/* sc_topk_stats for float64 rows: an exact radix select on the order-preserving 64-bit integer image of the doubles (eight 8-bit
 * passes), then the mean and the unbiased std of the k largest; ties at the threshold contribute exactly the copies any valid top-k
 * keeps.  1 < k <= n_cols, else SK_EARG. */
int sc_topk_stats_f64(const double* d_scores, int32_t n_rows, int32_t n_cols, int32_t k, double* d_mean, double* d_std, void* stream);

/* sc_norm_apply on a float64 matrix, in place: the same three modes, the same expressions in the same order.  A mean without its std,
 * or neither pair, is SK_EARG; a zero std gives what IEEE division gives. */
int sc_norm_apply_f64(double* d_S, int32_t Ne, int32_t Nt, const double* d_mean_e, const double* d_std_e, const double* d_mean_t,
                      const double* d_std_t, void* stream);

/* Mean and population std of the rows (axis = 1: scoremat.mean(1) / .std(1), :68-69) or the columns (axis = 0: :89-90) of a
 * rows x cols float32 score matrix; float64 sums in a fixed order.  skip_diag != 0 (square matrices only) leaves S[i][i] out and
 * divides by n - 1 (:64-66). */
int sc_matrix_moments(const float* d_S, int32_t rows, int32_t cols, int32_t axis, int32_t skip_diag, float* d_mean, float* d_std,
                      void* stream);

/* ---- PLDA training: sidekit.factor_analyser.FactorAnalyser.plda (sidekit/factor_analyser.py:830-932) ----------------------------
 * The device half of the EM: everything with an utterance (N) or class (C) dimension, in float64 on the f64 matrix cores; the D x D and
 * rank x rank algebra stays on the host (sidekit_amd/factor_analyser.py).  X is XT_F32 or XT_F64 and is widened in the load.  No
 * floating-point atomics: partial sums go through the sc_* workspace (sc_release_workspace) and are added in a fixed order, so the
 * result's bits are a function of the arguments alone. */

/* StatServer.sum_stat_per_model (sidekit/statserver.py:1335-1355): S[c][:] = sum of the rows of X (N x D) that belong to class c.
 * The class index arrives as a CSR built by the host: d_rows (N row numbers, grouped by class, ascending inside a class) is cut into
 * n_slices slices d_rows[d_slice_off[s] .. d_slice_off[s + 1]) that never straddle a class, and class c owns the slices
 * [d_class_slice_off[c], d_class_slice_off[c + 1]).  d_S: C x D; d_colsum (D column sums of X, i.e. N * mean) may be NULL. */
int sc_class_sums(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_rows, const int32_t* d_slice_off,
                  int32_t n_slices, const int32_t* d_class_slice_off, int32_t C, double* d_S, double* d_colsum, void* stream);

/* G[m][n] = sum_k w[k] (A[k][m] - ca[m]) (B[k][n] - cb[n]),  A: K x M, B: K x Nn row-major, both `dtype` (XT_F32 / XT_F64), G: M x Nn
 * float64; d_w, d_ca, d_cb may each be NULL (weight 1, centre 0).  K is the long dimension: it is cut into row slabs whose partial
 * tiles are added in slab order.  With A = B = X and ca = cb = mean this is the total scatter of the x-vectors. */
int sc_gemm_tn(const void* d_A, const void* d_B, int32_t dtype, int64_t K, int32_t M, int32_t Nn, const double* d_w, const double* d_ca,
               const double* d_cb, double* d_G, void* stream);

/* C = epilogue(alpha * A . B),  A: M x K, B: K x N, C: M x N, float64 row-major; d_rowv (M) and d_colv (N) come together or not at all.
 *   SC_EPI_RANK1:     C[m][n] = alpha * (A B)[m][n] - rowv[m] * colv[n]        (whitened, centred class sums: (S - n mu') W)
 *   SC_EPI_POSTERIOR: C[m][n] = alpha * (A B)[m][n] / (1 + rowv[m] * colv[n])  (the E-step's posterior scale in the eigenbasis of F'F) */
#define SC_EPI_RANK1 0
#define SC_EPI_POSTERIOR 1
int sc_dgemm_nn(const double* d_A, const double* d_B, int32_t M, int32_t N, int32_t K, double alpha, const double* d_rowv,
                const double* d_colv, int32_t epilogue, double* d_C, void* stream);

/* ---- back-end normalisation: LDA, WCCN, Mahalanobis and spectral normalisation (sidekit/statserver.py:797-1054, 1279-1333) ---------
 * The device half, for x-vectors (one distribution per session); the D x D algebra stays on the host (sidekit_amd/backend.py).  Same
 * conventions as PLDA training: X is XT_F32 or XT_F64 and is widened in the load, partial sums go through the sc_* workspace and are
 * added in a fixed order, no floating-point atomics. */

/* The class-centred, class-weighted scatter
 *   G[m][n] = sum_k w[cls[k]] (X[k][m] - Mc[cls[k]][m]) (X[k][n] - Mc[cls[k]][n]),   G: D x D float64.
 * X: N x D; d_cls: one class number per row (rows whose number is outside [0, C) are skipped); d_Mc: C x D float64 class means
 * (sc_class_sums over the counts); d_w: C float64 class weights, or NULL for weight 1.  With w = 1 and G / N this is
 * get_within_covariance_stat1 (:940-956), with w = 1 / n_c the Sw of get_lda_matrix_stat1 (:980-1019) and, over C, the WCCN matrix
 * (:1031-1054).  Formed directly, never as total minus between: that difference loses |total| / |within| in relative accuracy. */
int sc_scatter_within(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const int32_t* d_cls, const double* d_Mc, const double* d_w,
                      int32_t C, double* d_G, void* stream);

/* Centre, right-multiply and (normalize != 0) length-normalise in one pass over the rows:
 *   Y[i][:] = f((X[i][:] - mu) . R),   f = identity, or v / max(|v|, 1e-8)  (norm_stat1, :797-800).
 * X: N x D; d_mu: D float64 or NULL; d_R: D x P float64 row-major; d_Y: N x P, XT_F64 or XT_F32 (the float64 result rounded once); Y may
 * not overlap X.  This is whiten_stat1 + norm_stat1 (one iteration of spectral_norm_stat1), rotate_stat1 and whiten_cholesky_stat1.  Up
 * to P = 256 a workgroup holds whole rows and the length costs no extra pass; a normalising call with P > 256 computes the product
 * twice (first the rows' sums of squares, through the workspace, then the scaled rows). */
int sc_whiten_rows(const void* d_X, int32_t x_dtype, int64_t N, int32_t D, const double* d_mu, const double* d_R, int32_t P, int32_t normalize,
                   void* d_Y, int32_t y_dtype, void* stream);

/* ---- EER support (host code, no GPU needed) --------------------------------------------------- */

/* sidekit.bosaris.detplot.pavx (sidekit/bosaris/detplot.py:289-351): isotonic (non-decreasing) fit of y.
 * width / height need room for n entries; *nbins receives the number of bins.  ghat_out (n) may be NULL. */
int sk_pavx(const double* y, int64_t n, double* ghat_out, int64_t* width, double* height, int64_t* nbins);

/* Vertex walk of sidekit.bosaris.detplot.rocch (detplot.py:414-434): pideal is the 1/0 target indicator
 * ordered by ascending score (stable sort), width the PAV bins; pmiss / pfa receive nbins + 1 vertices. */
int sk_rocch_vertices(const double* pideal, int64_t n, int64_t n_tar, int64_t n_non, const int64_t* width, int64_t nbins,
                      double* pmiss, double* pfa);

/* ---- wav staging for the streaming extractor (host code, no GPU needed) ---------------------------
 * Replaces the per-file `torchaudio.load` of sidekit/bin/extract_xvectors.py:57-70 for canonical files: a pool of `threads`
 * host threads (no interpreter lock) walks the RIFF headers / reads the samples.
 * sk_wav_probe: kind[i] = 1 for RIFF/WAVE PCM 16-bit mono (nsamples / rate / data_offset filled), 0 for any other wav (the
 *   caller decodes it), -1 if the file cannot be opened.
 * sk_wav_read_pcm16: file i's samples -> dst[row[i] * ld .. + nsamples[i]) (dst: a pinned int16 staging buffer of n_rows rows, ld in
 *   elements); status[i] = 0 on success, -1 on a short read / open failure / nsamples[i] > ld / row[i] outside [0, n_rows). */
int sk_wav_probe(const char* const* paths, int32_t n, int32_t threads, int32_t* nsamples, int32_t* rate, int64_t* data_offset,
                 int32_t* kind);
int sk_wav_read_pcm16(const char* const* paths, const int64_t* data_offset, const int32_t* nsamples, const int32_t* row, int32_t n,
                      int32_t threads, int16_t* dst, int64_t ld, int32_t n_rows, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_H */
