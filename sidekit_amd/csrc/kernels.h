// Internal kernel-launcher interface of libsidekit_amd (not part of the C ABI).
#pragma once
#include <mutex>

#include "common.h"

namespace sk {

enum { DT_F32 = 0, DT_BF16 = 1, DT_F64 = 2, DT_I64 = 3 };

// ---- conv3x3.hip ------------------------------------------------------------------------
// The values are the xt_get_profile slot numbers and the sk_bench_conv shape numbers.  1, 3, 6, 9 were the layers' stand-alone 1x1 shortcut
// convolutions; the shortcut runs in conv2's epilogue, so those slots stay unused (and zero).
enum ConvShape {
  CONV_L1 = 0, CONV_L2A = 2, CONV_L2 = 4, CONV_L3A = 5, CONV_L3 = 7, CONV_L4A = 8, CONV_L4 = 10,
  CONV_NSHAPES,
  // small-grid forms of CONV_L3 / CONV_L4 (conv3x3.hip: 3- / 2-row tiles)
  CONV_L3T = 42, CONV_L4T = 43
};

struct SeArgs {
  const float* se_part; const float* col_part; const float* edge;   // as written by the statistics-mode conv
  int tiles, wm, th;
  const void* w2t;       // conv2 weights as consumed by the MFMA, [tap][ci][co]: bf16 in the bf16 path (w2t_bf16), else f32
  int w2t_bf16;
  const float* scale2; const float* shift2;
  const float* fc1; const float* fc2;   // se.fc.0 [C/16][C], se.fc.2 [C][C/16]
  float* gate;           // [B][C]
  Lens lens; int halvings; int wout; int C; int B;
};

struct ConvArgs {
  const void* in;      // [B][Hin][WIN][CIN]   (bf16 or f32)
  const void* wpack;   // fragment-ordered weights
  const float* scale;  // [COUT] folded BatchNorm scale
  const float* shift;  // [COUT] folded BatchNorm shift
  void* out;           // [B][Hout][WOUT][COUT]
  // -- statistics mode (conv1 of a BasicBlock; se_part != nullptr): sums of the stored (rounded) output that determine
  //    the plane mean of the 3x3 convolution that FOLLOWS (SELayer input, res_net.py:278-279) by linearity
  float* se_part;      // [B][tiles][WM][COUT] per-workgroup totals
  float* col_part;     // [B][tiles][2][COUT]  first / last column sums over the tile's valid rows
  float* edge;         // [B][6][COUT]         first-row sum, last-row sum, corners (0,0) (0,W-1) (last,0) (last,W-1)
  // -- residual mode (conv2 of a BasicBlock; gate != nullptr): out = relu(bn(conv) * gate[b][c] + shortcut)  (res_net.py:316-319)
  const float* gate;   // [B][COUT]
  const void* shortcut;  // NHWC, same shape and type as out
  // -- residual mode of the FIRST block of a layer (gate != nullptr && sc_in != nullptr): the shortcut is not a stored
  //    tensor but bn(conv1x1_stride(x)) of the block input x (res_net.py:301-307), computed in this epilogue from x's
  //    own rows: sc_in = x [B][sc_hin][WOUT*s][cin_x], weights sc_wpack (the shortcut BatchNorm's scale folded in), its shift sc_shift
  const void* sc_in; int sc_hin;
  const void* sc_wpack; const float* sc_shift;
  const void* zeros;   // >= 16 zero bytes in device memory (source of the conv zero padding)
  Lens lens;           // feature frames per utterance
  int halvings_in;     // stride-2 stages between the features and this conv's input
  int B, Hin, Hout;    // allocated rows of in / out
  int persist_cap;     // > 0: at most this many workgroups per CU for the persistent (weight-resident) shapes, see launch_cfg
  unsigned long long* stamps;  // diagnostics only: per-workgroup s_memtime stamps at the phase boundaries (8 per block), or nullptr
  int dbg;             // diagnostics only (sk_bench_conv): bit0 skip stores, bit1 skip MFMA loop, bit2 skip staging
};

struct ConvGeom { int cin, cout, stride, win, th, wm, ck, taps, ks, eb, nw; int m16; };   // m16: weights packed for v_mfma_f32_16x16x32_bf16 (16 x 32 fragments)

int conv_geom(int shape, int dtype, ConvGeom* g);
int launch_conv(int shape, int dtype, const ConvArgs& a, hipStream_t st);
size_t conv_pack_bytes(const ConvGeom& g);
void conv_pack_weights(const ConvGeom& g, const float* w, int kh_kw, void* dst);

// ---- trunk_misc.hip -----------------------------------------------------------------------
// stem: features (strides sf, st in elements) -> relu(bn(conv3x3 1->32)) NHWC [B][T][80][32]; w = tap-major [9][32] weights with the
// BatchNorm scale folded in, shift = the BatchNorm shift
int launch_stem(const float* feats, long sb, long sf, long st, const float* w, const float* shift, void* out, int dtype, Lens lens, int B,
                int T, hipStream_t s);
// SE gate of a BasicBlock computed BEFORE its second convolution runs: the plane mean of bn2(conv2(o1)) is linear in
// o1, so it follows from the sums conv1 left behind (total, first/last row and column, corners) and conv2's weights:
//   mean[co] = scale2[co] / (H W) * sum_{ci,dh,dw} W2[co][ci][dh][dw] * S[ci][dh][dw] + shift2[co]
// then FC -> ReLU -> FC -> sigmoid (res_net.py:262-281).
int launch_se_pre(const SeArgs& a, hipStream_t s);

// ---- gemm.hip ---------------------------------------------------------------------------
// C[m][n] = epi( sum_k A(m,k) * W[n][k] ), fp32 MFMA (exact f32 FMA chain), W row-major [N][K].
// A(m,k) = A[(m + (k / kc) * dil) * lda + k % kc]  (kc == 0: A[m*lda + k]); f32 or bf16 rows
//   -- the (kc, dil) form is a dilated "valid" conv1d over channel-contiguous rows (TDNN)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU02 = 2, ACT_RELU_BN_TANH = 3, ACT_LOG_EPS = 4 };
struct GemmArgs {
  const void* A;        // f32 or bf16 rows
  int a_bf16;           // A element type
  long lda;             // elements between consecutive rows of A
  long a_rows;          // rows that exist in A (reads beyond return 0)
  int kc, dil;          // see A(m,k) above
  const float* W;       // [N][K]
  long ldw;
  float* C;             // [M][ldc]
  long ldc;
  int M, N, K;
  const float* bias;    // [N] or null (added before the activation)
  const float* rowbias; // [M / rows_per_group][N] or null: per-group bias (attention context term)
  int rows_per_group;
  int act;
  const float* scale;   // [N] or null: applied after the activation (BatchNorm that follows it)
  const float* shift;   // [N]
  float alpha;          // final multiplier
  // split-K for skinny problems (M <= 512, K large: 16 workgroups would otherwise walk thousands of k-steps serially):
  const void* W_bf16;   // optional bf16 copy of W ([N][K], ldw elements): with bf16 A rows, kc == 0 and K % 64 == 0 the product runs on
                        // the bf16 MFMA (f32 accumulate) -- used by the bf16 compute path only
  float* splitk_ws;     // [ksplit][M][N] partial sums (M <= 512), or null: plain k order.  Non-null selects the sliced summation order for every M
  int ksplit;           // set by launch_gemm: slices run as blockIdx.z (1: inside the workgroup)
  int kslices;          // set by launch_gemm: slices the K range is summed in (a function of K alone)
  // optional fused tail of the embedding GEMM: when the slices run as blockIdx.z (small M) the kernel that adds them also L2-normalises
  // each finished row into l2_out [M][N] (the arithmetic of l2norm_kernel on the same values: same bits) and sets *l2_done = 1; otherwise
  // *l2_done = 0 and the caller launches the normalisation itself
  float* l2_out;
  int* l2_done;         // host
};
GemmArgs gemm_args();   // zero-initialised, alpha = 1
int launch_gemm(const GemmArgs& g, hipStream_t s);

// ---- frontend_fft.hip ------------------------------------------------------------------------
// |rFFT_1024(window * preemph(frame))|^2 for the log-mel front-end (n_fft 1024, win 400), one wave per frame
struct FftArgs {
  const void* wav; long wav_ld;                // [B][wav_ld] float32 samples, or int16 PCM (pcm16 != 0: widened as x / 32768 in the load)
  int pcm16;
  const int* nsamples; int nsamples_uniform;   // per-utterance sample counts (device) or one value for all
  int n_fft;                                   // 1024 (window 400, log-mel front-end) or 2048 (window 1024, MFCC front-end)
  const float* window;                         // [400] / [1024]
  const float* tw512;                          // exp(-2 pi i m / (n_fft/2)), m = 0..n_fft/2-1, interleaved (re, im): the complex transform's twiddles
  const float* tw1024;                         // exp(-2 pi i k / n_fft),     k = 0..n_fft/2: the real-FFT split's
  float* P; long ldp;                          // [M][ldp] power spectrum, ldp >= n_fft/2 + 1 (extra columns zeroed)
  int M, t_max, hop;
  const int* row_b; const int* row_t;          // optional ragged row map
  float preemph;
  // fused mel projection (mel_cw != nullptr): instead of P the kernel writes logmel[m][j] = log(sum_k fb[k][j] P[k] + 1e-6).
  // Every filter is a short run of bins (triangles: <= 31 of 513) cut into chunks of 8 taps: chunk c = bins [mel_ck0[c], + 8) with
  // weights mel_cw[c][0..8) (zero beyond the filter's run); filter j owns the consecutive chunks [cb, cb + nc), mel_fmeta[j] = cb | nc << 16;
  // mel_chunks is padded to a multiple of 64 with all-zero chunks
  const float* mel_cw; const int* mel_ck0; const int* mel_fmeta; int mel_chunks; int n_mels;
  float* logmel; long ldl;
};
int launch_stft_power_fft(const FftArgs& a, hipStream_t s);

// ---- pool.hip ---------------------------------------------------------------------------
// rows layout: x[(row0[b] + t) * ld + d], t < count[b]
struct RowSpan {
  const int* offsets;  // [B] device row offset per utterance, or null -> b * stride
  int stride;
  Lens lens;           // feature frames per utterance
  int halvings;        // count = halve(frames, halvings) - shrink
  int shrink;
  __device__ inline int row0(int b) const { return offsets ? offsets[b] : b * stride; }
  __device__ inline int count(int b) const { return halve(lens.get(b), halvings) - shrink; }
};
// out[b][0:D] = mean_t, out[b][D:2D] = unbiased std_t  (pooling.py:55-70)
int launch_mean_std(const void* x, int x_bf16, long ld, int D, RowSpan rs, float* out, int B, hipStream_t s);
// attentive statistics: w = softmax_t(e); mu = sum x w; rh = sqrt(clamp(sum x^2 w - mu^2, 1e-9)) (pooling.py:165-168)
int launch_att_stats(const float* x, const float* e, long ld, int D, RowSpan rs, float* out, int B, hipStream_t s);
// bf16 path: attention.4 (h [rows][128] f32 x W2 [D][128] bf16 + b2), softmax over time and the weighted statistics in one kernel:
// the (rows x D) score matrix e is never written
int launch_att_fused(const void* x_bf16, const float* h, const void* w2_bf16, const float* b2, long ld, int D, RowSpan rs, float* out, int B,
                     hipStream_t s);
// per-(b, column) CMVN over rows: (x - mean) / sqrt(var_biased + eps), in place (InstanceNorm1d)
int launch_cmvn(float* x, long ld, int D, RowSpan rs, float eps, int B, hipStream_t s);
// x / ||x||_2 (loss.py:91-100) followed by F.normalize(eps=1e-12) (xvector.py:903)
int launch_l2norm(const float* x, float* out, int D, int B, hipStream_t s);
// x / max(||x||_2, eps) per row (F.normalize)
int launch_normalize_rows(const float* x, float* out, int D, int B, float eps, hipStream_t s);

// ---- scoring.hip --------------------------------------------------------------------------
// The sc_* workspace (also score_norm.hip's, plda_train.hip's and backend.hip's): one buffer per (device, stream), grown on demand, freed
// by sc_release_workspace().  The caller holds g_plda_mu from the lookup until the kernels that use the buffer are enqueued.
// (The f32 / f64 MFMA tiles shared between files are headers of their own: sgemm_tile.h, dgemm_tile.h.)
extern std::mutex g_plda_mu;
int plda_workspace_locked(hipStream_t st, size_t bytes, void** out);
// What the PLDA entry points share: the stream's workspace cut into E . Psi (Ne x D), the partial quadratic forms of both sides
// (nparts x Ne, nparts x Nt; a term is the sum of its partials in ascending p) and `extra_doubles` more for the caller (the buffer is ONE
// request: a second one could free the first), and the ONE plda_prep_kernel launch that fills the first three.  The caller holds
// g_plda_mu and keeps it until its own kernels are enqueued.
struct PldaPrep { double *epsi, *qe, *qt, *extra; int nparts; };
int plda_prep_locked(const double* d_E, int32_t Ne, const double* d_T, int32_t Nt, int32_t D, const double* d_Phi, const double* d_Psi,
                     hipStream_t st, PldaPrep* out, size_t extra_doubles = 0);
// sc_cosine, the cosine histograms and sc_cohort_moments read their float32 rows with 16-byte loads: D % 4 == 0 keeps every row on such a
// boundary only if the base pointer is on one (a view that starts 4 bytes into a larger buffer is not)
inline bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0; }

// ---- plda_train.hip -------------------------------------------------------------------------
// The cut of a TN product (sc_gemm_tn, sc_scatter_within; sc_class_scatter: `batch` products of the same M x N whose longest K is given):
// the tile edge TL (big: 128), and K in `nsplit` slabs of `slab` rows whose partial tiles are added in slab order.
struct TnCut { bool big; int TL; long nsplit, slab; };
TnCut tn_cut(long K, int M, int N, long batch = 1);
// G[i] = sum_p part[p * mn + i], p ascending: the slabs' partial tiles joined in slab order
int launch_slab_reduce(const double* part, int nslabs, long mn, double* G, hipStream_t st);

}  // namespace sk
