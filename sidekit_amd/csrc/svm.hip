// The SVM back end's solver (sidekit/svm_training.py trains one libsvm problem per speaker, one after the other): M independent
// two-class C-SVC duals over one shared B x B background Gram block, one workgroup per model (include/sidekit_amd/svm.h has the problem,
// the algorithm -- libsvm's solver without shrinking -- and the tie rule).  float64, no atomics, nothing passes between workgroups.
//
// One workgroup = 256 threads = 4 waves.  Point t of a model belongs to thread t % 256.  LDS, in doubles: a[n], G[n], the kernel's
// diagonal QD[n], then the reductions' slots.  An iteration reads two kernel rows (i's for the second-order selection of j, i's and
// j's for the gradient) from global memory, each B contiguous doubles and the model's few own entries.  The background block is the
// same for every model: the workgroups share it through L2 and the Infinity Cache.  The gradient update and the next iteration's
// selection of i are one pass.  Three barriers per iteration.
#include "../../include/sidekit_amd/svm.h"
#include "kernels.h"

namespace sk {

constexpr int SVM_T = 256;
constexpr int SVM_W = SVM_T / 64;
constexpr double SVM_TAU = 1e-12;
static_assert(SC_SVM_LDS_RESERVED >= (int)(3 * SVM_W * (sizeof(double) + sizeof(int)) + 2 * SVM_W * sizeof(double)), "the reductions' slots");

// The larger value; of equal values the larger index (svm.h: the tie rule).  A total order, so any reduction tree gives the same pair.
__device__ inline void svm_take(double& v, int& i, double v2, int i2) {
  if (v2 > v || (v2 == v && i2 > i)) { v = v2; i = i2; }
}
__device__ inline void svm_wave_argmax(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(v, o);
    const int i2 = __shfl_xor(i, o);
    svm_take(v, i, v2, i2);
  }
}
__device__ inline double svm_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ inline double svm_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ inline double svm_wave_sum(double v) {   // a butterfly: the same tree in every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The kernel rows of one model, read as stored.  Bounds: i, t in [0, B + csn); Keb points at the model's first enrolment row, whose csn
// rows lie inside K_eb, and Kee at its csn x csn block inside K_ee (checked by the kernel before the first read).
struct SvmRows {
  const double* Kbb; const double* Keb; const double* Kee;
  int B, csn;
  // point i's kernel row against the background: B contiguous doubles, for a background point and for a target alike ...
  __device__ const double* head(int i) const { return i < B ? Kbb + (long)i * B : Keb + (long)(i - B) * B; }
  // ... and its entry against the model's own target r
  __device__ double tail(int i, int r) const { return i < B ? Keb[(long)r * B + i] : Kee[(i - B) * csn + r]; }
  __device__ double at(int i, int t) const { return t < B ? head(i)[t] : tail(i, t - B); }
};

// SVM_CH of a thread's entries of a background row, t0, t0 + 256, ... (0 past the row's end), all requested before the first is used.
// Left to itself the compiler moves each load into the branch that uses it and waits for it there: one round trip to memory per entry
// (a 4 096 x 4 096 block is 134 MB, beyond L2).  The empty statements pin the values between the loads and the uses.
constexpr int SVM_CH = 8;
__device__ inline void svm_request_chunk(const double* __restrict__ row, int t0, int B, double (&k)[SVM_CH]) {
#pragma unroll
  for (int u = 0; u < SVM_CH; ++u) {
    const int t = t0 + u * SVM_T;
    k[u] = t < B ? row[t] : 0.0;
  }
}
__device__ inline void svm_pin_chunk(double (&k)[SVM_CH]) {
#pragma unroll
  for (int u = 0; u < SVM_CH; ++u) asm volatile("" : "+v"(k[u]));
}

__global__ __launch_bounds__(SVM_T) void svm_train_kernel(const double* __restrict__ Kbb, int B, const double* __restrict__ Keb, int Ne,
                                                          const double* __restrict__ Kee, long ee_len, const int* __restrict__ en_off,
                                                          const long* __restrict__ ee_off, int max_csn, const double* __restrict__ Cs, double eps,
                                                          int max_iter, double* __restrict__ coef, double* __restrict__ rho_out,
                                                          int* __restrict__ iters_out, double* __restrict__ gap_out, int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) double svm_smem[];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ldc = B + max_csn;
  const int row0 = en_off[m], row1 = en_off[m + 1];
  const int csn = row1 - row0;
  const long ee0 = ee_off[m];
  if (row0 < 0 || row1 > Ne || csn < 1 || csn > max_csn || ee0 < 0 || ee0 + (long)csn * csn > ee_len) {   // the same for every thread
    if (tid == 0) status_out[m] = SC_SVM_BAD_OFFSETS;
    return;
  }
  const int n = B + csn;   // <= ldc <= SC_SVM_MAX_N: the three arrays below hold ldc doubles each
  double* a = svm_smem;
  double* G = a + ldc;
  double* QD = G + ldc;
  double* red_v = QD + ldc;                     // [3][SVM_W]: the pass that selects i, the pass that selects j, rho's bounds
  double* red_w = red_v + 3 * SVM_W;            // [2][SVM_W]: the second value of a pass
  int* red_i = (int*)(red_w + 2 * SVM_W);       // [3][SVM_W]
  const SvmRows K{Kbb, Keb + (long)row0 * B, Kee + ee0, B, csn};
  const double C = Cs[m];

  // a = 0, G = -e; the first selection of i: every background point is in I_up with -y G = 1, no target is (a = 0)
  double gmax = -INFINITY;
  int gi = -1;
  for (int t = tid; t < n; t += SVM_T) {
    a[t] = 0.0;
    G[t] = -1.0;
    QD[t] = K.at(t, t);
    if (t < B && 0.0 < C) svm_take(gmax, gi, 1.0, t);
  }
  int iter = 0, status = SC_SVM_CONVERGED;
  double gap = 0.0;
  for (;;) {   // at most max_iter + 1 rounds
    svm_wave_argmax(gmax, gi);
    if (lane == 0) { red_v[wave] = gmax; red_i[wave] = gi; }
    __syncthreads();   // (1) a, G (and, the first time, QD) are complete; the slots of the selection of i are written
    gmax = red_v[0]; gi = red_i[0];
#pragma unroll
    for (int w = 1; w < SVM_W; ++w) svm_take(gmax, gi, red_v[w], red_i[w]);
    const int i = gi;
    // the selection of j: second order, over I_low
    double gmax2 = -INFINITY, best = -INFINITY;
    int bj = -1;
    if (i >= 0) {
      const double qdi = QD[i];
      const double* ri = K.head(i);
      auto candidate = [&](int t, bool pos, double kit) {
        const double at = a[t], gt = G[t];
        if (pos ? at > 0.0 : at < C) {
          const double mg = pos ? gt : -gt;   // y_t G_t
          const double gd = gmax + mg;
          gmax2 = fmax(gmax2, mg);
          if (gd > 0.0) {
            double qc = qdi + QD[t] - 2.0 * kit;
            if (!(qc > 0.0)) qc = SVM_TAU;
            svm_take(best, bj, (gd * gd) / qc, t);   // the largest decrease of the objective
          }
        }
      };
      // the row is read for every background point, in I_low or not
      for (int t0 = tid; t0 < B; t0 += SVM_CH * SVM_T) {
        double ki[SVM_CH];
        svm_request_chunk(ri, t0, B, ki);
        svm_pin_chunk(ki);
#pragma unroll
        for (int u = 0; u < SVM_CH; ++u)
          if (t0 + u * SVM_T < B) candidate(t0 + u * SVM_T, true, ki[u]);
      }
      for (int t = B + tid; t < n; t += SVM_T) candidate(t, false, K.tail(i, t - B));
    }
    svm_wave_argmax(best, bj);
    gmax2 = svm_wave_max(gmax2);
    if (lane == 0) { red_v[SVM_W + wave] = best; red_i[SVM_W + wave] = bj; red_w[wave] = gmax2; }
    __syncthreads();   // (2) the slots of the selection of j
    best = red_v[SVM_W]; bj = red_i[SVM_W]; gmax2 = red_w[0];
#pragma unroll
    for (int w = 1; w < SVM_W; ++w) { svm_take(best, bj, red_v[SVM_W + w], red_i[SVM_W + w]); gmax2 = fmax(gmax2, red_w[w]); }
    const int j = bj;
    gap = gmax + gmax2;
    if (gap < eps || j < 0) { status = SC_SVM_CONVERGED; break; }
    if (iter == max_iter) { status = SC_SVM_MAX_ITER; break; }
    ++iter;
    // the pair update, by every thread on the same numbers
    const bool ipos = i < B, jpos = j < B;
    const double Gi = G[i], Gj = G[j], old_ai = a[i], old_aj = a[j];
    double qc = QD[i] + QD[j] - 2.0 * K.at(i, j);
    if (!(qc > 0.0)) qc = SVM_TAU;
    double ai = old_ai, aj = old_aj;
    if (ipos != jpos) {
      const double delta = (-Gi - Gj) / qc, diff = ai - aj;
      ai += delta; aj += delta;
      if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
      else            { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
      if (diff > 0.0) { if (ai > C) { ai = C; aj = C - diff; } }   // C_i = C_j: diff > C_i - C_j is diff > 0
      else            { if (aj > C) { aj = C; ai = C + diff; } }
    } else {
      const double delta = (Gi - Gj) / qc, sum = ai + aj;
      ai -= delta; aj += delta;
      if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
      else         { if (aj < 0.0) { aj = 0.0; ai = sum; } }
      if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
      else         { if (ai < 0.0) { ai = 0.0; aj = sum; } }
    }
    const double dai = ai - old_ai, daj = aj - old_aj;
    const double yi = ipos ? 1.0 : -1.0, yj = jpos ? 1.0 : -1.0;
    __syncthreads();   // (3) every thread has read G[i], G[j], a[i], a[j] and the slots before any of them is written
    // G_k += Q_ik da_i + Q_jk da_j, and the next selection of i on the new G and a; the owner of i and of j stores their new a
    gmax = -INFINITY; gi = -1;
    const double* ri = K.head(i);
    const double* rj = K.head(j);
    auto update = [&](int t, bool pos, double kit, double kjt) {
      const double yt = pos ? 1.0 : -1.0;
      const double g = G[t] + ((yi * yt * kit) * dai + (yj * yt * kjt) * daj);
      G[t] = g;
      double at = a[t];
      if (t == i) { at = ai; a[t] = ai; }
      if (t == j) { at = aj; a[t] = aj; }
      if (pos ? at < C : at > 0.0) svm_take(gmax, gi, pos ? -g : g, t);
    };
    for (int t0 = tid; t0 < B; t0 += SVM_CH * SVM_T) {
      double ki[SVM_CH], kj[SVM_CH];
      svm_request_chunk(ri, t0, B, ki);
      svm_request_chunk(rj, t0, B, kj);
      svm_pin_chunk(ki);
      svm_pin_chunk(kj);
#pragma unroll
      for (int u = 0; u < SVM_CH; ++u)
        if (t0 + u * SVM_T < B) update(t0 + u * SVM_T, true, ki[u], kj[u]);
    }
    for (int t = B + tid; t < n; t += SVM_T) update(t, false, K.tail(i, t - B), K.tail(j, t - B));
  }
  // here every thread is past barrier (2) of the last round and nothing was written since: a and G are final
  // rho and the coefficients
  double ub = INFINITY, lb = -INFINITY, sum_free = 0.0, n_free = 0.0;
  for (int t = tid; t < n; t += SVM_T) {
    const double at = a[t];
    const bool pos = t < B;
    const double yg = pos ? G[t] : -G[t];
    if (at >= C) { if (!pos) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
    else if (at <= 0.0) { if (pos) ub = fmin(ub, yg); else lb = fmax(lb, yg); }
    else { n_free += 1.0; sum_free += yg; }
    coef[(long)m * ldc + t] = pos ? at : -at;
  }
  ub = svm_wave_min(ub); lb = svm_wave_max(lb); sum_free = svm_wave_sum(sum_free); n_free = svm_wave_sum(n_free);
  __syncthreads();   // the slots of the last round have been read
  if (lane == 0) { red_v[wave] = ub; red_v[SVM_W + wave] = lb; red_v[2 * SVM_W + wave] = sum_free; red_w[wave] = n_free; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SVM_W; ++w) {   // in wave order
      ub = fmin(ub, red_v[w]); lb = fmax(lb, red_v[SVM_W + w]); sum_free += red_v[2 * SVM_W + w]; n_free += red_w[w];
    }
    rho_out[m] = n_free > 0.0 ? sum_free / n_free : (ub + lb) / 2.0;
    iters_out[m] = iter;
    gap_out[m] = gap;
    status_out[m] = status;
  }
}

}  // namespace sk

using namespace sk;

extern "C" {

int sc_svm_train(const double* d_Kbb, int32_t B, const double* d_Keb, int32_t Ne, const double* d_Kee, int64_t ee_len, const int32_t* d_en_off,
                 const int64_t* d_ee_off, int32_t M, int32_t max_csn, const double* d_C, double eps, int32_t max_iter, double* d_coef,
                 double* d_rho, int32_t* d_iters, double* d_gap, int32_t* d_status, void* stream) {
  SK_CHECK(d_Kbb && d_Keb && d_Kee && d_en_off && d_ee_off && d_C && d_coef && d_rho && d_iters && d_gap && d_status, SK_EARG,
           "sc_svm_train: null argument");
  SK_CHECK(B >= 1 && Ne >= 1 && M >= 1 && max_csn >= 1 && ee_len >= 1, SK_EARG,
           "sc_svm_train: bad sizes (B=%d, Ne=%d, M=%d, max_csn=%d, ee_len=%lld)", B, Ne, M, max_csn, (long long)ee_len);
  SK_CHECK((long long)B + max_csn <= SC_SVM_MAX_N, SK_EARG,
           "sc_svm_train: a problem of B + csn = %lld points does not fit the LDS of one workgroup (at most %d); it is never split",
           (long long)B + max_csn, (int)SC_SVM_MAX_N);
  SK_CHECK(eps > 0.0, SK_EARG, "sc_svm_train: eps must be positive (got %g)", eps);
  SK_CHECK(max_iter >= 1, SK_EARG, "sc_svm_train: max_iter must be at least 1 (got %d)", max_iter);
  const size_t lds = (size_t)(B + max_csn) * 24 + SC_SVM_LDS_RESERVED;   // <= SC_SVM_LDS_BYTES
  if (lds > 65536)
    SK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(svm_train_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(svm_train_kernel, dim3((unsigned)M), dim3(SVM_T), lds, (hipStream_t)stream, d_Kbb, B, d_Keb, Ne, d_Kee, (long)ee_len,
                     d_en_off, (const long*)d_ee_off, max_csn, d_C, eps, max_iter, d_coef, d_rho, d_iters, d_gap, d_status);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
