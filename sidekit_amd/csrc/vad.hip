// Speech activity: the energy detector of sidekit/mixture.py:67-113 (vad_energy: standardised log-energy, 8 EM iterations of a
// 3-component 1-D GMM, threshold mu_max - alpha * sigma_max) on the frames of sidekit/frontend/features.py:363-389 (power_spectrum's
// framing, per-frame pre-emphasis and log(sum(frame^2))), label_fusion (sidekit/frontend/vad.py:409-428: closing then opening), and the
// gather that applies labels or speech timestamps to a padded batch before the trunk sees it.  Four entry points:
//   sk_frame_log_energy   waveform [B][wav_ld] (float32 / int16) -> float64 le[B][T_ld], nframes[B]     one wave per frame
//   sk_vad_energy         le -> label[B][T_ld], threshold[B]                                           one workgroup per utterance
//   sk_collect_labels     kept frames -> contiguous samples, out_len[B] on the device
//   sk_collect_segments   host-validated {start, end} ranges (CSR) -> contiguous samples
// Everything is float64 with fixed-order reductions (lane-strided partial sums, a butterfly inside the wave, the four waves in order):
// no atomics, the bits are a function of the arguments alone.
#include <math.h>

#include "../../include/sidekit_amd.h"
#include "kernels.h"

namespace sk {

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T> __device__ inline double widen(T v);
template <> __device__ inline double widen<float>(float v) { return (double)v; }
template <> __device__ inline double widen<int16_t>(int16_t v) { return (double)v / 32768.0; }   // exact, the front-end's x / 32768

__host__ __device__ inline int frames_of(long n, int nwin, int shift) { return n >= nwin ? (int)((n - nwin) / shift) + 1 : 0; }

// ---- log-energy ---------------------------------------------------------------------------------------------------------------------
// grid (ceil(T_ld / 4), B), 256 threads: wave w of block x owns frame t = 4 x + w of utterance b.  Frame t is samples [t shift, t shift + nwin);
// pre-emphasis inside the frame (y[0] = x[0] - p x[0], y[j] = x[j] - p x[j - 1]: the reference filters AFTER framing); le = log(sum y^2).
// Bounds: t < nframes <= T_ld, and t shift + nwin <= n <= wav_ld by the definition of nframes; columns [nframes, T_ld) are zeroed.
template <typename T>
__global__ __launch_bounds__(256) void frame_log_energy_kernel(const T* __restrict__ wav, long wav_ld, const int* __restrict__ nsamples, int nwin,
                                                               int shift, double prefac, double* __restrict__ le, int T_ld,
                                                               int* __restrict__ nframes) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  long n = nsamples[b];
  n = n < 0 ? 0 : (n > wav_ld ? wav_ld : n);
  int nf = frames_of(n, nwin, shift);
  nf = nf > T_ld ? T_ld : nf;
  if (blockIdx.x == 0 && threadIdx.x == 0) nframes[b] = nf;
  if (t >= T_ld) return;
  if (t >= nf) {
    if (lane == 0) le[(long)b * T_ld + t] = 0.0;
    return;
  }
  const T* x = wav + (long)b * wav_ld + (long)t * shift;
  double s = 0.0;
  for (int j = lane; j < nwin; j += 64) {
    const double cur = widen<T>(x[j]), prev = widen<T>(x[j > 0 ? j - 1 : 0]);
    const double y = cur - prev * prefac;
    s += y * y;
  }
  s = wave_sum_f64(s);
  if (lane == 0) le[(long)b * T_ld + t] = log(s);
}

// ---- the detector -------------------------------------------------------------------------------------------------------------------
constexpr int VAD_THREADS = 256;
constexpr int VAD_TILE = 2048;       // frames of label fusion per pass through LDS
constexpr int VAD_MAX_WIN = 255;     // fusion_win <= 255: a halo of 4 * (win / 2) <= 508 frames on each side of a tile

// Sum of NV values per thread over the workgroup: butterfly inside each wave, then the four waves in order.  `red` is [4][NV]; the caller
// alternates between two such buffers so that one barrier per call is enough.
template <int NV>
__device__ inline void block_sum(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double s = wave_sum_f64(v[i]);
    if (lane == 0) red[wave * NV + i] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = ((red[i] + red[NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
}

__device__ inline int reflect_index(int i, int n) {   // scipy.ndimage mode='reflect': (d c b a | a b c d | d c b a)
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// One workgroup per utterance.  z = (le - mean) / std (population std, numpy.std); the mixture starts at means (-2, 0, 2), unit variances,
// equal weights and -- as the reference leaves it -- a constant term A = 0 in the FIRST E-step (Mixture() sets A = 0 and vad_energy never
// calls _compute_all before the loop), so iteration 1 scores lp_k = -0.5 (z^2 invcov_k - 2 z mu_k invcov_k); from the first M-step on
// A_k = mu_k^2 invcov_k - 2 (log w_k + log cst_k).  Degenerate utterances (no frame, zero / non-finite std -- which any non-finite
// log-energy produces --, a NaN threshold, or no frame left labelled) keep every frame and report threshold NaN.
// Bounds: every index into le / label is t < n <= T_ld; the fusion tiles index LDS by t - (c0 - halo) in [0, VAD_TILE + 2 halo).
__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const double* __restrict__ le_all, const int* __restrict__ nframes, int T_ld,
                                                                 int n_iter, double flooring, double ceiling, double alpha, int fusion_win,
                                                                 uint8_t* __restrict__ label_all, double* __restrict__ threshold) {
  __shared__ double red[2][4 * 9];
  __shared__ uint8_t fa[VAD_TILE + 8 * (VAD_MAX_WIN / 2)], fb[VAD_TILE + 8 * (VAD_MAX_WIN / 2)];
  __shared__ int cnt[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* le = le_all + (long)b * T_ld;
  uint8_t* label = label_all + (long)b * T_ld;
  int n = nframes[b];
  n = n < 0 ? 0 : (n > T_ld ? T_ld : n);
  for (int t = n + tid; t < T_ld; t += VAD_THREADS) label[t] = 0;
  const double nan = __builtin_nan("");
  int phase = 0;
  double thr = nan, mean = 0.0, sd = 0.0;
  bool ok = n >= 1;
  if (ok) {
    double v1[1] = {0.0};
    for (int t = tid; t < n; t += VAD_THREADS) v1[0] += le[t];
    block_sum<1>(v1, red[phase]); phase ^= 1;
    mean = v1[0] / n;
    v1[0] = 0.0;
    for (int t = tid; t < n; t += VAD_THREADS) { const double d = le[t] - mean; v1[0] += d * d; }
    block_sum<1>(v1, red[phase]); phase ^= 1;
    sd = sqrt(v1[0] / n);
    ok = isfinite(sd) && sd > 0.0;
  }
  if (ok) {
    double w[3] = {1.0 / 3, 1.0 / 3, 1.0 / 3}, mu[3] = {-2.0, 0.0, 2.0}, ic[3] = {1.0, 1.0, 1.0}, A[3] = {0.0, 0.0, 0.0};
    for (int it = 0; it < n_iter; ++it) {
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int t = tid; t < n; t += VAD_THREADS) {
        const double z = (le[t] - mean) / sd, z2 = z * z;
        double lp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) lp[k] = -0.5 * ((z2 * ic[k] - 2.0 * (z * (mu[k] * ic[k]))) + A[k]);
        const double m = fmax(fmax(lp[0], lp[1]), lp[2]);
        double ll = m + log((exp(lp[0] - m) + exp(lp[1] - m)) + exp(lp[2] - m));
        if (!isfinite(m)) ll = m;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double pp = exp(lp[k] - ll);
          acc[k] += pp; acc[3 + k] += z * pp; acc[6 + k] += z2 * pp;
        }
      }
      block_sum<9>(acc, red[phase]); phase ^= 1;
      const double wsum = (acc[0] + acc[1]) + acc[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        w[k] = acc[k] / wsum;
        mu[k] = acc[3 + k] / acc[k];
        double cov = acc[6 + k] / acc[k] - mu[k] * mu[k];
        if (cov <= flooring) cov = flooring;      // variance_control with cov_var_ctl = 1 (a NaN passes through both, as in numpy)
        if (cov >= ceiling) cov = ceiling;
        ic[k] = 1.0 / cov;
        const double det = 1.0 / ic[k];
        const double cst = 1.0 / (sqrt(det) * 2.5066282746310002);   // (2 pi)^(1/2)
        A[k] = mu[k] * mu[k] * ic[k] - 2.0 * (log(w[k]) + log(cst));
      }
    }
    int km = 0;
    for (int k = 1; k < 3; ++k) if (mu[k] > mu[km]) km = k;
    thr = mu[km] - alpha * sqrt(1.0 / ic[km]);
    if (isnan(mu[0]) || isnan(mu[1]) || isnan(mu[2])) thr = nan;
    ok = !isnan(thr);
  }
  int kept = 0;
  if (ok) {
    const int r = fusion_win / 2, halo = 4 * r;
    if (fusion_win == 0) {
      for (int t = tid; t < n; t += VAD_THREADS) {
        const uint8_t l = (le[t] - mean) / sd > thr;
        label[t] = l;
        kept += l;
      }
    } else {
      // closing (dilate, erode) then opening (erode, dilate) with a flat window of fusion_win frames.  A symmetric window commutes with the
      // reflect extension, so the four passes on the reflect-extended raw labels of [c0 - 4r, c0 + TILE + 4r) give the tile exactly
      for (int c0 = 0; c0 < n; c0 += VAD_TILE) {
        const int lo = c0 - halo, len = VAD_TILE + 2 * halo;
        __syncthreads();   // the previous tile's last pass has been read
        for (int i = tid; i < len; i += VAD_THREADS) fa[i] = (le[reflect_index(lo + i, n)] - mean) / sd > thr;
        uint8_t* src = fa;
        uint8_t* dst = fb;
        for (int pass = 0; pass < 4; ++pass) {   // valid range shrinks by r on each side per pass
          const bool dilate = pass == 0 || pass == 3;
          const int m0 = (pass + 1) * r, m1 = len - (pass + 1) * r;
          __syncthreads();
          for (int i = m0 + tid; i < m1; i += VAD_THREADS) {
            uint8_t v = dilate ? 0 : 1;
            for (int j = -r; j <= r; ++j) v = dilate ? (v | src[i + j]) : (v & src[i + j]);
            dst[i] = v;
          }
          uint8_t* sw = src; src = dst; dst = sw;
        }
        __syncthreads();
        for (int i = tid; i < VAD_TILE && c0 + i < n; i += VAD_THREADS) {
          const uint8_t l = src[halo + i];
          label[c0 + i] = l;
          kept += l;
        }
      }
    }
    // any frame left?  (integer sum: order-free)
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    __syncthreads();
    if ((tid & 63) == 0) cnt[tid >> 6] = kept;
    __syncthreads();
    kept = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    ok = kept > 0;
  }
  if (!ok) {
    thr = nan;
    for (int t = tid; t < n; t += VAD_THREADS) label[t] = 1;
  }
  if (tid == 0) threshold[b] = thr;
}

// ---- gather -------------------------------------------------------------------------------------------------------------------------
constexpr int CG_THREADS = 256;   // runs per tile = threads
constexpr int CG_SPLIT = 4;       // workgroups (blockIdx.z) that share one tile's output range

// What is kept of utterance b, as an ascending list of runs (source start, length); a length may be zero.
struct LabelRuns {   // run i = frame i if labelled: samples [i shift, (i + 1) shift), the last frame up to the end of the utterance
  const uint8_t* label; const int* nframes; const int* nsamples; int T_ld, shift; long src_ld;
  __device__ inline long samples(int b) const { const long n = nsamples[b]; return n < 0 ? 0 : (n > src_ld ? src_ld : n); }
  __device__ inline int frames(int b) const { const int f = nframes[b]; return f < 0 ? 0 : (f > T_ld ? T_ld : f); }
  __device__ inline int count(int b) const { const int f = frames(b); return f < 1 ? 1 : f; }   // no frame: one run, the whole signal
  __device__ inline void get(int b, int i, long* start, long* len) const {
    const long n = samples(b);
    const int f = frames(b);
    if (f < 1) { *start = 0; *len = n; return; }
    long s = (long)i * shift, e = i == f - 1 ? n : s + shift;
    s = s > n ? n : s; e = e > n ? n : e;
    *start = s;
    *len = label[(long)b * T_ld + i] ? e - s : 0;
  }
};
struct SegmentRuns {   // run i = the utterance's i-th {start, end} pair (validated by the host; clamped again to the row for memory safety)
  const int* seg_off; const int* seg; long src_ld;
  __device__ inline int count(int b) const { const int c = seg_off[b + 1] - seg_off[b]; return c < 0 ? 0 : c; }
  __device__ inline void get(int b, int i, long* start, long* len) const {
    long s = seg[2 * (long)(seg_off[b] + i)], e = seg[2 * (long)(seg_off[b] + i) + 1];
    s = s < 0 ? 0 : (s > src_ld ? src_ld : s);
    e = e < s ? s : (e > src_ld ? src_ld : e);
    *start = s; *len = e - s;
  }
};

// Exclusive scan of one value per thread over the 256 threads (wave scan by shuffles, the four wave totals through LDS); *total = the sum.
__device__ inline long block_exclusive_scan(long v, long* wave_tot, long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  long base = 0;
  for (int k = 0; k < wave; ++k) base += wave_tot[k];
  *total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
  return base + inc - v;
}

// grid (tiles of 256 runs, B, CG_SPLIT).  A workgroup adds up the lengths of the runs before its tile (thread-strided, integer), scans its
// own 256 runs, and copies its share of the tile's output range [base, base + tile_total): 16-byte slots of the DESTINATION, each thread one
// slot at a time.  A whole slot whose 16 / sizeof(T) elements come from consecutive source samples at a 16-byte aligned address is one vector
// load + one vector store; a whole slot otherwise is gathered element by element and stored as one vector; the head and tail of the
// range (partial slots) are element stores.  Bounds: source indices are < n <= src_ld (the run getters clamp), destination indices are
// < min(total kept, dst_ld).
template <typename T, typename Runs>
__global__ __launch_bounds__(CG_THREADS) void collect_kernel(const T* __restrict__ src_all, long src_ld, Runs runs, T* __restrict__ dst_all,
                                                             long dst_ld, int* __restrict__ out_len) {
  constexpr int VE = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VE)));
  __shared__ long s_src[CG_THREADS], s_dst[CG_THREADS + 1], wave_tot[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nruns = runs.count(b), r0 = blockIdx.x * CG_THREADS;
  if (r0 >= nruns && !(r0 == 0 && nruns == 0)) return;   // uniform for the workgroup
  long before = 0;
  for (int i = tid; i < r0; i += CG_THREADS) {
    long s, l;
    runs.get(b, i, &s, &l);
    before += l;
  }
  long base;
  block_exclusive_scan(before, wave_tot, &base);
  long start = 0, len = 0;
  if (r0 + tid < nruns) runs.get(b, r0 + tid, &start, &len);
  long tile_total;
  const long off = block_exclusive_scan(len, wave_tot, &tile_total);
  s_src[tid] = start;
  s_dst[tid] = base + off;
  if (tid == 0) s_dst[CG_THREADS] = base + tile_total;
  __syncthreads();
  if (out_len && blockIdx.z == 0 && tid == 0 && r0 + CG_THREADS >= nruns) {
    const long tot = base + tile_total;
    out_len[b] = (int)(tot > dst_ld ? dst_ld : tot);
  }
  const T* src = src_all + (long)b * src_ld;
  T* dst = dst_all + (long)b * dst_ld;
  long lo = base, hi = base + tile_total;
  hi = hi > dst_ld ? dst_ld : hi;
  if (lo >= hi) return;
  // slots are counted from the 16-byte boundary at or below dst: element o sits in slot (o + a0) / VE
  const long a0 = (long)((reinterpret_cast<size_t>(dst) & 15) / sizeof(T));
  const long v_lo = (lo + a0) / VE, v_hi = (hi + a0 + VE - 1) / VE;
  const long per = (v_hi - v_lo + CG_SPLIT - 1) / CG_SPLIT;
  const long v0 = v_lo + per * blockIdx.z, v1 = v0 + per < v_hi ? v0 + per : v_hi;
  for (long v = v0 + tid; v < v1; v += CG_THREADS) {
    const long o0 = v * VE - a0;
    const long e0 = o0 < lo ? lo : o0, e1 = o0 + VE > hi ? hi : o0 + VE;
    // the run of the first element: the last r with s_dst[r] <= e0 among runs of non-zero length (zero-length runs share their successor's s_dst)
    int lo_r = 0, hi_r = CG_THREADS - 1;
    while (lo_r < hi_r) {
      const int mid = (lo_r + hi_r + 1) >> 1;
      if (s_dst[mid] <= e0) lo_r = mid; else hi_r = mid - 1;
    }
    int r = lo_r;
    if (e1 - e0 == VE && s_dst[r + 1] - e0 >= VE) {   // whole slot inside one run
      const T* p = src + s_src[r] + (e0 - s_dst[r]);
      vec_t val;
      if ((reinterpret_cast<size_t>(p) & 15) == 0) {
        val = *reinterpret_cast<const vec_t*>(p);
      } else {
#pragma unroll
        for (int j = 0; j < VE; ++j) val[j] = p[j];
      }
      *reinterpret_cast<vec_t*>(dst + e0) = val;
      continue;
    }
    T tmp[VE];
    for (long e = e0; e < e1; ++e) {
      while (s_dst[r + 1] <= e) ++r;    // e < hi <= s_dst[CG_THREADS]: stops at r <= CG_THREADS - 1
      tmp[e - e0] = src[s_src[r] + (e - s_dst[r])];
    }
    if (e1 - e0 == VE) {
      vec_t val;
#pragma unroll
      for (int j = 0; j < VE; ++j) val[j] = tmp[j];
      *reinterpret_cast<vec_t*>(dst + e0) = val;
    } else {
      for (long e = e0; e < e1; ++e) dst[e] = tmp[e - e0];
    }
  }
}

template <typename T, typename Runs>
static int launch_collect(const void* src, long src_ld, const Runs& runs, int max_runs, int B, void* dst, long dst_ld, int* out_len, hipStream_t st) {
  const int tiles = max_runs < 1 ? 1 : cdiv(max_runs, CG_THREADS);
  hipLaunchKernelGGL((collect_kernel<T, Runs>), dim3(tiles, B, CG_SPLIT), dim3(CG_THREADS), 0, st, (const T*)src, src_ld, runs, (T*)dst, dst_ld,
                     out_len);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

static bool ranges_overlap(const void* a, size_t ab, const void* b, size_t bb) {
  const char* a0 = (const char*)a;
  const char* b0 = (const char*)b;
  return !(a0 + ab <= b0 || b0 + bb <= a0);
}

}  // namespace sk

using namespace sk;

extern "C" {

int sk_frame_log_energy(const void* d_wav, int32_t in_dtype, int64_t wav_ld, const int32_t* d_nsamples, int32_t B, int32_t nwin, int32_t shift,
                        double prefac, double* d_le, int32_t T_ld, int32_t* d_nframes, void* stream) {
  SK_CHECK(d_wav && d_nsamples && d_le && d_nframes, SK_EARG, "sk_frame_log_energy: null argument");
  SK_CHECK(in_dtype == XT_F32 || in_dtype == XT_I16, SK_EARG, "sk_frame_log_energy: the waveform must be XT_F32 or XT_I16 (got %d)", in_dtype);
  SK_CHECK(B > 0 && B <= 65535 && wav_ld > 0 && nwin > 0 && shift > 0, SK_EARG, "sk_frame_log_energy: bad sizes (B=%d, wav_ld=%lld, nwin=%d, shift=%d)", B,
           (long long)wav_ld, nwin, shift);
  SK_CHECK(T_ld >= 1 && T_ld >= frames_of(wav_ld, nwin, shift), SK_EARG, "sk_frame_log_energy: T_ld=%d is less than the %d frames of wav_ld=%lld samples", T_ld,
           frames_of(wav_ld, nwin, shift), (long long)wav_ld);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(T_ld, 4), B);
  if (in_dtype == XT_I16)
    hipLaunchKernelGGL(frame_log_energy_kernel<int16_t>, grid, dim3(256), 0, st, (const int16_t*)d_wav, (long)wav_ld, d_nsamples, nwin, shift, prefac,
                       d_le, T_ld, d_nframes);
  else
    hipLaunchKernelGGL(frame_log_energy_kernel<float>, grid, dim3(256), 0, st, (const float*)d_wav, (long)wav_ld, d_nsamples, nwin, shift, prefac, d_le,
                       T_ld, d_nframes);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sk_vad_energy(const double* d_le, const int32_t* d_nframes, int32_t B, int32_t T_ld, int32_t n_iter, double flooring, double ceiling, double alpha,
                  int32_t fusion_win, uint8_t* d_label, double* d_threshold, void* stream) {
  SK_CHECK(d_le && d_nframes && d_label && d_threshold, SK_EARG, "sk_vad_energy: null argument");
  SK_CHECK(B > 0 && T_ld > 0 && n_iter >= 0, SK_EARG, "sk_vad_energy: bad sizes (B=%d, T_ld=%d, n_iter=%d)", B, T_ld, n_iter);
  SK_CHECK(fusion_win == 0 || (fusion_win >= 3 && fusion_win <= VAD_MAX_WIN && (fusion_win & 1)), SK_EARG,
           "sk_vad_energy: fusion_win must be 0 or odd in [3, %d] (got %d)", VAD_MAX_WIN, fusion_win);
  hipLaunchKernelGGL(vad_energy_kernel, dim3(B), dim3(VAD_THREADS), 0, (hipStream_t)stream, d_le, d_nframes, T_ld, n_iter, flooring, ceiling, alpha,
                     fusion_win, d_label, d_threshold);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

int sk_collect_labels(const void* d_src, int32_t dtype, int64_t src_ld, const int32_t* d_nsamples, const uint8_t* d_label, int32_t T_ld,
                      const int32_t* d_nframes, int32_t B, int32_t shift, void* d_dst, int64_t dst_ld, int32_t* d_out_len, void* stream) {
  SK_CHECK(d_src && d_nsamples && d_label && d_nframes && d_dst && d_out_len, SK_EARG, "sk_collect_labels: null argument");
  SK_CHECK(dtype == XT_F32 || dtype == XT_I16, SK_EARG, "sk_collect_labels: samples must be XT_F32 or XT_I16 (got %d)", dtype);
  SK_CHECK(B > 0 && B <= 65535 && src_ld > 0 && src_ld <= 0x7fffffffLL && T_ld > 0 && shift > 0, SK_EARG,
           "sk_collect_labels: bad sizes (B=%d, src_ld=%lld, T_ld=%d, shift=%d)", B, (long long)src_ld, T_ld, shift);
  SK_CHECK(dst_ld >= src_ld, SK_EARG, "sk_collect_labels: dst_ld=%lld is less than src_ld=%lld", (long long)dst_ld, (long long)src_ld);
  const size_t es = dtype == XT_F32 ? 4 : 2;
  SK_CHECK(!ranges_overlap(d_src, (size_t)B * src_ld * es, d_dst, (size_t)B * dst_ld * es), SK_EARG, "sk_collect_labels: dst may not overlap src");
  const LabelRuns runs = {d_label, d_nframes, d_nsamples, T_ld, shift, (long)src_ld};
  if (dtype == XT_I16) return launch_collect<int16_t>(d_src, (long)src_ld, runs, T_ld, B, d_dst, (long)dst_ld, d_out_len, (hipStream_t)stream);
  return launch_collect<float>(d_src, (long)src_ld, runs, T_ld, B, d_dst, (long)dst_ld, d_out_len, (hipStream_t)stream);
}

int sk_collect_segments(const void* d_src, int32_t dtype, int64_t src_ld, const int32_t* h_nsamples, const int32_t* h_seg_off, const int32_t* h_seg,
                        const int32_t* d_seg_off, const int32_t* d_seg, int32_t B, void* d_dst, int64_t dst_ld, int32_t* h_out_len, void* stream) {
  SK_CHECK(d_src && h_nsamples && h_seg_off && d_seg_off && d_dst, SK_EARG, "sk_collect_segments: null argument");
  SK_CHECK(dtype == XT_F32 || dtype == XT_I16, SK_EARG, "sk_collect_segments: samples must be XT_F32 or XT_I16 (got %d)", dtype);
  SK_CHECK(B > 0 && B <= 65535 && src_ld > 0 && src_ld <= 0x7fffffffLL && dst_ld > 0, SK_EARG, "sk_collect_segments: bad sizes (B=%d, src_ld=%lld, dst_ld=%lld)", B,
           (long long)src_ld, (long long)dst_ld);
  SK_CHECK(h_seg_off[0] == 0, SK_EARG, "sk_collect_segments: seg_off[0] must be 0");
  int max_runs = 0;
  for (int b = 0; b < B; ++b) {   // everything is checked before anything is enqueued
    const int n0 = h_seg_off[b], n1 = h_seg_off[b + 1];
    SK_CHECK(n1 >= n0, SK_EARG, "sk_collect_segments: seg_off decreases at utterance %d", b);
    SK_CHECK(h_nsamples[b] >= 0 && h_nsamples[b] <= src_ld, SK_EARG, "sk_collect_segments: utterance %d has %d samples, the row holds %lld", b, h_nsamples[b],
             (long long)src_ld);
    SK_CHECK(n1 == n0 || (h_seg && d_seg), SK_EARG, "sk_collect_segments: null segment list");
    long prev_end = 0, total = 0;
    for (int i = n0; i < n1; ++i) {
      const long s = h_seg[2 * (long)i], e = h_seg[2 * (long)i + 1];
      SK_CHECK(s >= 0 && s <= e && e <= h_nsamples[b], SK_EARG, "sk_collect_segments: utterance %d, segment %d: [%ld, %ld) is not inside [0, %d]", b, i - n0, s, e,
               h_nsamples[b]);
      SK_CHECK(s >= prev_end, SK_EARG, "sk_collect_segments: utterance %d, segment %d starts at %ld before the previous one ends (%ld): ranges must ascend "
               "without overlap", b, i - n0, s, prev_end);
      prev_end = e;
      total += e - s;
    }
    SK_CHECK(total <= dst_ld, SK_EARG, "sk_collect_segments: utterance %d keeps %ld samples, dst_ld is %lld", b, total, (long long)dst_ld);
    if (h_out_len) h_out_len[b] = (int32_t)total;
    max_runs = n1 - n0 > max_runs ? n1 - n0 : max_runs;
  }
  const size_t es = dtype == XT_F32 ? 4 : 2;
  SK_CHECK(!ranges_overlap(d_src, (size_t)B * src_ld * es, d_dst, (size_t)B * dst_ld * es), SK_EARG, "sk_collect_segments: dst may not overlap src");
  if (max_runs == 0) return SK_OK;   // nothing kept anywhere: nothing to copy
  const SegmentRuns runs = {d_seg_off, d_seg, (long)src_ld};
  if (dtype == XT_I16) return launch_collect<int16_t>(d_src, (long)src_ld, runs, max_runs, B, d_dst, (long)dst_ld, nullptr, (hipStream_t)stream);
  return launch_collect<float>(d_src, (long)src_ld, runs, max_runs, B, d_dst, (long)dst_ld, nullptr, (hipStream_t)stream);
}

}  // extern "C"
