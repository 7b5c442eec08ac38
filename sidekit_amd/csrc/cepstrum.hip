// The cepstral front end of the classical chain (sidekit/frontend/features.py: power_spectrum, mfcc): log-energy, log filter-bank
// outputs and cepstra of every frame of a ragged batch, one entry point (include/sidekit_amd/cepstrum.h).  Not the x-vector front end
// of frontend_fft.hip, which mirrors torchaudio: here frames are not centred, pre-emphasis runs inside a frame, the window has the
// frame's own length, n_fft is 256 or 512 and the log has no floor.
//
// One wavefront per frame, four frames per workgroup, the wave index scalar (readfirstlane): row, utterance, frame and every base
// address live in SGPRs; no workgroup barrier is needed.  The n_fft-point real transform is an NH = n_fft / 2 point complex Stockham
// (autosort) transform of z[n] = x[2n] + i x[2n + 1] followed by the real-FFT split by mirror pairs:
//   NH = 256: four radix-4 passes, every lane one butterfly per pass;
//   NH = 128: one radix-2 pass on all 64 lanes (it takes the samples), then three radix-4 passes on 32 lanes.
// Passes exchange data through the wave's own LDS buffer of complex slots, index padded by i >> 2 (the stride-4 scatter of the first
// radix-4 pass then falls on 32 distinct bank pairs).  The power row stays in LDS for the filter bank (lane i sums filter i and i + 64
// over its support, bins ascending) and the log filter-bank row for the DCT (lane c sums cepstrum c and c + 64, filters ascending):
// only the 1 + nceps + nfilt outputs go to HBM unless the spectrum is asked for.
// LDS per wave: 320 complex slots (2 560 B) + 260 power floats (1 040 B) + 128 log filter-bank floats (512 B) = 4 112 B;
// per workgroup 4 x 4 112 = 16 448 B of the 163 840 B of a CU (nine workgroups by LDS; the wave slots bind first).
// The twiddles exp(-2 pi i m / 512) are a compile-time table (double Taylor series on the first octant, symmetries elsewhere).
// Logs: the argument is split into exponent and a mantissa in [sqrt(1/2), sqrt(2)); v_log_f32 (1 ulp) sees the mantissa only, where
// its absolute error is below 6e-8, and the exponent is added with ln 2 in two parts.  No atomics, every sum in a fixed order.
// No packed-f32 instructions: the file is built without SLP vectorisation (Makefile) and forms none by hand.
#include "../../include/sidekit_amd/cepstrum.h"
#include "common.h"

namespace sk {

struct cf { float x, y; };
__device__ inline cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
__device__ inline cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
__device__ inline cf cmulf(cf a, cf b) { return {fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)}; }
__device__ inline cf mul_mi(cf a) { return {a.y, -a.x}; }  // a * (-i)

// ---- exp(-2 pi i m / 512), m = 0 .. 511, made by the compiler ---------------------------------------------------------------------
struct TwTable { float v[1024]; };
constexpr double tw_sin(double x) {   // |x| <= pi / 4: the series is exact to double precision after 11 terms
  double term = x, sum = x;
  for (int n = 1; n < 12; ++n) { term *= -x * x / ((2 * n) * (2 * n + 1)); sum += term; }
  return sum;
}
constexpr double tw_cos(double x) {
  double term = 1.0, sum = 1.0;
  for (int n = 1; n < 12; ++n) { term *= -x * x / ((2 * n - 1) * (2 * n)); sum += term; }
  return sum;
}
constexpr TwTable make_tw() {
  TwTable t{};
  const double step = 6.283185307179586476925286766559 / 512.0;
  for (int m = 0; m < 512; ++m) {
    const int q = m / 128, r = m % 128;
    const double c = r <= 64 ? tw_cos(r * step) : tw_sin((128 - r) * step), s = r <= 64 ? tw_sin(r * step) : tw_cos((128 - r) * step);
    const double co = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s, si = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    t.v[2 * m] = (float)co;
    t.v[2 * m + 1] = (float)-si;
  }
  return t;
}
__device__ const TwTable TW512 = make_tw();
__device__ inline cf tw(int m) { return {TW512.v[2 * m], TW512.v[2 * m + 1]}; }

struct MfccArgs {
  const void* wav; long wav_ld; double scale;
  const int* nsamples; const int64_t* frame_off; int B; long N;
  int nwin, shift; float prefac;
  const float* window; const float* bank; const int* bank_lo; const int* bank_hi; int nfilt;
  const float* dct; int nceps;
  float* out; long ld; float* spec; long lds;
};

constexpr int MF_WAVES = 4;
constexpr int MF_ZBUF = 320, MF_PW = 260, MF_FB = SC_MFCC_MAX_FILT;   // per-wave LDS: complex slots, power floats, log filter-bank floats

__device__ inline int pad(int i) { return i + (i >> 2); }
// Lanes of a wave exchange data through LDS with no workgroup barrier: a wave's LDS instructions execute in order, and this keeps the
// compiler from moving a lane's loads above its stores to addresses that only ANOTHER lane's loads alias.  It emits no instruction.
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ inline void fft4(cf* v) {
  const cf a0 = cadd(v[0], v[2]), a1 = cadd(v[1], v[3]), b0 = csub(v[0], v[2]), b1 = mul_mi(csub(v[1], v[3]));
  v[0] = cadd(a0, a1); v[1] = cadd(b0, b1); v[2] = csub(a0, a1); v[3] = csub(b0, b1);
}

// one radix-4 Stockham pass of an NH-point transform, butterfly j < NH / 4; NS = the product of the radices before it
template <int NH, int NS>
__device__ inline void pass4(cf* buf, int j) {
  cf v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = buf[pad(j + r * (NH / 4))];
  const int k = j & (NS - 1);
  if (NS > 1) {
#pragma unroll
    for (int r = 1; r < 4; ++r) v[r] = cmulf(v[r], tw(r * k * (512 / (4 * NS))));
  }
  fft4(v);
  const int j0 = (j - k) * 4 + k;
  wave_sync();
#pragma unroll
  for (int r = 0; r < 4; ++r) buf[pad(j0 + r * NS)] = v[r];
  wave_sync();
}

// natural logarithm, plain IEEE at the ends (0 -> -inf, inf -> inf, negative or NaN -> NaN)
__device__ inline float log_f32(float x) {
  int e = 0;
  if (x < 1.17549435e-38f) { x *= 4294967296.0f; e = -32; }       // subnormal arguments: v_log_f32 and v_frexp may flush them
  float m = __builtin_amdgcn_frexp_mantf(x);                        // [0.5, 1); 0, inf and NaN come through
  e += __builtin_amdgcn_frexp_expf(x);
  if (m < 0.70710678118654752440f) { m *= 2.0f; e -= 1; }
  const float l2 = __builtin_amdgcn_logf(m), ef = (float)e;         // log2 of [sqrt(1/2), sqrt(2)): |l2| <= 1/2
  return fmaf(ef, 0.693145751953125f, fmaf(l2, 0.69314718055994530942f, ef * 1.42860682030941723212e-6f));
}

// sum_k w[k] p[k], k = 0 .. n - 1 ascending, one fused multiply-add per term in that order (w: global, p: LDS).  The loads of eight
// terms are issued together so that their latencies overlap; the chain of additions is the same as one term at a time.
__device__ inline float dot_ordered(const float* __restrict__ w, const float* p, int n) {
  float acc = 0.f;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    float wv[8], pv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { wv[j] = w[k + j]; pv[j] = p[k + j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(wv[j], pv[j], acc);
  }
  for (; k < n; ++k) acc = fmaf(w[k], p[k], acc);
  return acc;
}

template <bool I16>
__device__ inline float sample(const void* row, long i, double scale) {
  return I16 ? (float)((double)reinterpret_cast<const short*>(row)[i] * scale) : (float)((double)reinterpret_cast<const float*>(row)[i] * scale);
}

// z[n] of a frame: the windowed pre-emphasised samples 2n and 2n + 1 (zero from nwin on); adds their squares, unwindowed, to e
template <bool I16>
__device__ inline cf frame_input(const void* row, long s0, int n, const MfccArgs& a, float& e) {
  const int j0 = 2 * n, j1 = j0 + 1;
  const bool ok0 = j0 < a.nwin, ok1 = j1 < a.nwin;
  const int i0 = ok0 ? j0 : 0, i1 = ok1 ? j1 : i0, im = i0 > 0 ? i0 - 1 : 0;     // every index read lies inside the frame
  const float xm = sample<I16>(row, s0 + im, a.scale), x0 = sample<I16>(row, s0 + i0, a.scale), x1 = sample<I16>(row, s0 + i1, a.scale);
  const float w0 = a.window[i0], w1 = a.window[i1];
  const float pm = a.prefac * xm, p0 = a.prefac * x0;
  const float y0 = ok0 ? x0 - pm : 0.f, y1 = ok1 ? x1 - p0 : 0.f;
  e = fmaf(y0, y0, e);
  e = fmaf(y1, y1, e);
  return {w0 * y0, w1 * y1};
}

template <int NH, bool I16>
__global__ __launch_bounds__(MF_WAVES * 64) void mfcc_kernel(MfccArgs a) {
  __shared__ __attribute__((aligned(16))) cf zbuf[MF_WAVES * MF_ZBUF];
  __shared__ float pwbuf[MF_WAVES * MF_PW];
  __shared__ float fbbuf[MF_WAVES * MF_FB];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // everything per frame below is scalar
  const long m = (long)blockIdx.x * MF_WAVES + wave;
  if (m >= a.N) return;
  cf* buf = zbuf + wave * MF_ZBUF;
  float* pw = pwbuf + wave * MF_PW;
  float* fb = fbbuf + wave * MF_FB;
  // the utterance of row m: the last b with off[b] <= m (empty utterances own no row)
  int b = 0, hi = a.B;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (a.frame_off[mid] <= m) b = mid; else hi = mid;
  }
  const long t = m - a.frame_off[b];
  long ns = a.nsamples[b];
  if (ns > a.wav_ld) ns = a.wav_ld;
  const long s0 = t * a.shift;
  if (t < 0 || s0 + a.nwin > ns) return;       // offsets that do not match the lengths: nothing is read outside the row
  const void* row = I16 ? (const void*)(reinterpret_cast<const short*>(a.wav) + (long)b * a.wav_ld)
                        : (const void*)(reinterpret_cast<const float*>(a.wav) + (long)b * a.wav_ld);
  float e = 0.f;
  if (NH == 256) {
    cf v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = frame_input<I16>(row, s0, lane + 64 * r, a, e);
    fft4(v);
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[pad(4 * lane + r)] = v[r];
    wave_sync();
    pass4<256, 4>(buf, lane);
    pass4<256, 16>(buf, lane);
    pass4<256, 64>(buf, lane);
  } else {
    const cf v0 = frame_input<I16>(row, s0, lane, a, e), v1 = frame_input<I16>(row, s0, lane + 64, a, e);
    buf[pad(2 * lane)] = cadd(v0, v1);
    buf[pad(2 * lane + 1)] = csub(v0, v1);
    wave_sync();
    if (lane < 32) pass4<128, 2>(buf, lane);
    if (lane < 32) pass4<128, 8>(buf, lane);
    if (lane < 32) pass4<128, 32>(buf, lane);
    wave_sync();      // lanes 32 .. 63 took none of the passes' fences: one for the whole wave before the split reads buf
  }
  e = wave_sum(e);
  // ---- real-FFT split by mirror pairs: from Z[k], Z[NH - k] and W^k (W = exp(-2 pi i / n_fft)) the powers of bins k and NH - k,
  //   X[k] = s/2 - i W^k d/2,  X[NH - k] = conj(s/2 + i W^k d/2),  s = Z[k] + conj Z[NH - k],  d = Z[k] - conj Z[NH - k]
  // (k = 0 pairs with itself and gives bins 0 and NH; k = NH / 2 pairs with itself)
  for (int k = lane; k <= NH / 2; k += 64) {
    const cf zk = buf[pad(k)], zm = buf[pad((NH - k) & (NH - 1))], w = tw(k * (256 / NH));
    const cf s = {zk.x + zm.x, zk.y - zm.y}, d = {zk.x - zm.x, zk.y + zm.y};
    const cf wd = cmulf(w, d);
    const float re = 0.5f * (s.x + wd.y), im = 0.5f * (s.y - wd.x), rm = 0.5f * (s.x - wd.y), jm = 0.5f * (s.y + wd.x);
    pw[k] = fmaf(re, re, im * im);
    pw[NH - k] = fmaf(rm, rm, jm * jm);
  }
  wave_sync();
  if (a.spec) {
    float* srow = a.spec + m * a.lds;
    for (int k = lane; k <= NH; k += 64) srow[k] = pw[k];
  }
  float* orow = a.out + m * a.ld;
  if (lane == 0) orow[0] = log_f32(e);
  // ---- filter bank: lane i owns filters i and i + 64
  for (int i = lane; i < a.nfilt; i += 64) {
    int lo = a.bank_lo[i], up = a.bank_hi[i];
    if (lo < 0) lo = 0;
    if (up > NH + 1) up = NH + 1;
    const float* brow = a.bank + (long)i * (NH + 1);
    const float l = log_f32(up > lo ? dot_ordered(brow + lo, pw + lo, up - lo) : 0.f);
    fb[i] = l;
    orow[1 + a.nceps + i] = l;
  }
  wave_sync();
  // ---- cepstrum: lane c owns coefficients c and c + 64
  for (int c = lane; c < a.nceps; c += 64) {
    const float* drow = a.dct + (long)c * a.nfilt;
    orow[1 + c] = dot_ordered(drow, fb, a.nfilt);
  }
}

}  // namespace sk

extern "C" {

int sc_mfcc(const void* d_wav, int32_t wav_dtype, int64_t wav_ld, double scale, const int32_t* d_nsamples, const int64_t* d_frame_off, int32_t B,
            int64_t N, int32_t nwin, int32_t shift, int32_t n_fft, double prefac, const float* d_window, const float* d_bank,
            const int32_t* d_bank_lo, const int32_t* d_bank_hi, int32_t nfilt, const float* d_dct, int32_t nceps, float* d_out, int64_t ld,
            float* d_spec, int64_t lds, void* stream) {
  using namespace sk;
  SK_CHECK(d_wav && d_nsamples && d_frame_off && d_window && d_bank && d_bank_lo && d_bank_hi && d_dct && d_out, SK_EARG, "sc_mfcc: null argument");
  SK_CHECK(wav_dtype == XT_F32 || wav_dtype == XT_I16, SK_EARG, "sc_mfcc: the samples must be XT_F32 or XT_I16 (got dtype %d)", wav_dtype);
  SK_CHECK(B >= 1 && N >= 0 && N <= 4 * (int64_t)0x7fffffff && wav_ld >= 1, SK_EARG, "sc_mfcc: B = %d utterances (at least one), N = %lld rows, wav_ld = %lld",
           B, (long long)N, (long long)wav_ld);
  SK_CHECK(n_fft == 256 || n_fft == 512, SK_EARG, "sc_mfcc: n_fft = %d (256 or 512)", n_fft);
  SK_CHECK(nwin >= n_fft / 2 + 1 && nwin <= n_fft, SK_EARG, "sc_mfcc: nwin = %d outside [%d, %d]", nwin, n_fft / 2 + 1, n_fft);
  SK_CHECK(shift >= 1 && shift <= nwin, SK_EARG, "sc_mfcc: shift = %d outside [1, %d]", shift, nwin);
  SK_CHECK(nfilt >= 1 && nfilt <= SC_MFCC_MAX_FILT, SK_EARG, "sc_mfcc: nfilt = %d outside [1, %d]", nfilt, SC_MFCC_MAX_FILT);
  SK_CHECK(nceps >= 1 && nceps <= nfilt - 1, SK_EARG, "sc_mfcc: nceps = %d outside [1, %d]", nceps, nfilt - 1);
  SK_CHECK(ld >= 1 + (int64_t)nceps + nfilt, SK_EARG, "sc_mfcc: ld = %lld below 1 + nceps + nfilt = %d", (long long)ld, 1 + nceps + nfilt);
  SK_CHECK(!d_spec || lds >= n_fft / 2 + 1, SK_EARG, "sc_mfcc: lds = %lld below n_fft / 2 + 1 = %d", (long long)lds, n_fft / 2 + 1);
  if (N == 0) return SK_OK;
  const MfccArgs a = {d_wav, (long)wav_ld, scale, d_nsamples, d_frame_off, B, (long)N, nwin, shift, (float)prefac, d_window, d_bank, d_bank_lo,
                      d_bank_hi, nfilt, d_dct, nceps, d_out, (long)ld, d_spec, (long)lds};
  const dim3 grid((unsigned)((N + MF_WAVES - 1) / MF_WAVES)), block(MF_WAVES * 64);
  const bool i16 = wav_dtype == XT_I16;
  hipStream_t s = (hipStream_t)stream;
  if (n_fft == 512) {
    if (i16) hipLaunchKernelGGL((mfcc_kernel<256, true>), grid, block, 0, s, a); else hipLaunchKernelGGL((mfcc_kernel<256, false>), grid, block, 0, s, a);
  } else {
    if (i16) hipLaunchKernelGGL((mfcc_kernel<128, true>), grid, block, 0, s, a); else hipLaunchKernelGGL((mfcc_kernel<128, false>), grid, block, 0, s, a);
  }
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
