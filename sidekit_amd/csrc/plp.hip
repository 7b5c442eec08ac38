// The PLP tail of the classical chain (sidekit/frontend/features.py: postaud, dolpc, levinson, lpc2cep, lifter): from the log
// critical-band energies of every frame to its liftered LPC cepstra, one entry point (include/sidekit_amd/plp.h).  What comes before
// it is sc_mfcc under a bark bank (cepstrum.hip) and, for RASTA-PLP, sc_feat_rasta (featnorm.hip).
//
// Lane = frame: the recursions are serial and tiny, so nothing is shared between lanes but the tables.  A workgroup is one wave of
// SC_PLP_ROWS = 64 frames.  Its rows of log energies are fetched by all lanes together, element i of the block by lane i mod 64
// (contiguous when ldb = nb, runs of nb floats otherwise), into a float stage of [row][nb | 1]: the odd stride makes lane l's walk
// along its own row free of bank conflicts.  The per-lane arrays are indexed by loop variables, so they live in LDS as float64
// [index][lane] (ds_read_b64 / ds_write_b64 of 64 consecutive doubles: conflict-free), in two regions that are reused:
//   U: y[0 .. nb)          then A[0 .. order)       (y is dead once r is formed)
//   V: r[0 .. order]       then c[0 .. order]       (r is dead once the recursion ends)
// No array is indexed at run time in registers: the kernel uses no scratch memory.  The cepstra and y go back through the float stage
// and leave by the same all-lanes walk as the input came.  The tables are read by uniform index through ordinary loads (the scalar
// cache).  LDS: 64 ((nb | 1) 4 + (nb + order + 1) 8) bytes, 22 784 at nb = 21, order = 12.  No atomics; -ffp-contract=off (Makefile)
// keeps every product and sum separately rounded, in the order the header gives.
#include "../../include/sidekit_amd/plp.h"
#include "common.h"

namespace sk {

struct PlpArgs {
  const float* logband; long ldb; long N; int nb, order;
  const double* eql; const double* acw; const double* lift;
  float* cep; long ldc; float* post; long ldp;
};

constexpr int PLP_ROWS = SC_PLP_ROWS;

// rows x cols floats between the stage (row stride sld) and global rows (row stride ld), element i by lane i mod 64
template <bool LOAD>
__device__ inline void plp_move(float* stage, int sld, float* g, long ld, int rows, int cols, int lane) {
  const int n = rows * cols;
  for (int i = lane; i < n; i += PLP_ROWS) {
    const int row = i / cols, col = i - row * cols;
    if (LOAD) stage[row * sld + col] = g[(long)row * ld + col]; else g[(long)row * ld + col] = stage[row * sld + col];
  }
}

__global__ __launch_bounds__(PLP_ROWS) void plp_cepstra_kernel(PlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char plp_lds[];
  const int nb = a.nb, order = a.order, sld = nb | 1, lane = threadIdx.x;
  double* U = reinterpret_cast<double*>(plp_lds);                  // [nb][64]
  double* V = U + nb * PLP_ROWS;                                   // [order + 1][64]
  float* stage = reinterpret_cast<float*>(V + (order + 1) * PLP_ROWS);   // [64][sld]
  const long row0 = (long)blockIdx.x * PLP_ROWS;
  const int rows = a.N - row0 < PLP_ROWS ? (int)(a.N - row0) : PLP_ROWS;   // >= 1: the grid has no empty workgroup
  const bool live = lane < rows;

  plp_move<true>(stage, sld, const_cast<float*>(a.logband) + row0 * a.ldb, a.ldb, rows, nb, lane);
  __syncthreads();

  // ---- equal loudness, the 0.33 power, the two edge bands replaced by their neighbours
  if (live) {
    for (int j = 0; j < nb; ++j) U[j * PLP_ROWS + lane] = pow(a.eql[j] * exp((double)stage[lane * sld + j]), 0.33);
    U[lane] = U[PLP_ROWS + lane];
    U[(nb - 1) * PLP_ROWS + lane] = U[(nb - 2) * PLP_ROWS + lane];
  }
  __syncthreads();        // every lane has read its staged row: the stage takes y
  if (live && a.post) {
    for (int j = 0; j < nb; ++j) stage[lane * sld + j] = (float)U[j * PLP_ROWS + lane];
  }
  __syncthreads();
  if (a.post) plp_move<false>(stage, sld, a.post + row0 * a.ldp, a.ldp, rows, nb, lane);
  __syncthreads();        // the stage is free for the cepstra

  if (live) {
    // ---- autocorrelation: the cosine transform of y, lag by lag
    for (int k = 0; k <= order; ++k) {
      const double* w = a.acw + (long)k * nb;
      double r = 0.0;
      for (int j = 0; j < nb; ++j) r = r + w[j] * U[j * PLP_ROWS + lane];
      V[k * PLP_ROWS + lane] = r;
    }
    // ---- Levinson-Durbin; A overwrites y
    double* A = U;
    double P = V[lane];
    for (int k = 0; k < order; ++k) {
      double s = V[(k + 1) * PLP_ROWS + lane];
      for (int j = 0; j < k; ++j) s = s + A[j * PLP_ROWS + lane] * V[(k - j) * PLP_ROWS + lane];
      const double t = -s / P;
      P = P * (1.0 - t * t);
      A[k * PLP_ROWS + lane] = t;
      const int half = (k + 1) >> 1;
      for (int j = 0; j < half; ++j) {
        const int i = k - j - 1;
        const double aj = A[j * PLP_ROWS + lane], ai = A[i * PLP_ROWS + lane];
        A[j * PLP_ROWS + lane] = aj + t * ai;
        if (i != j) A[i * PLP_ROWS + lane] = ai + t * aj;
      }
    }
    // ---- LPC to cepstra; c overwrites r; the lifter on the way to the stage
    double* c = V;
    const double c0 = log(P);
    c[lane] = c0;
    stage[lane * sld] = (float)(c0 * a.lift[0]);
    for (int n = 1; n <= order; ++n) {
      double sum = 0.0;
      for (int m = 1; m < n; ++m) sum = sum + ((double)(n - m) * A[(m - 1) * PLP_ROWS + lane]) * c[(n - m) * PLP_ROWS + lane];
      const double cn = -(A[(n - 1) * PLP_ROWS + lane] + sum / (double)n);
      c[n * PLP_ROWS + lane] = cn;
      stage[lane * sld + n] = (float)(cn * a.lift[n]);
    }
  }
  __syncthreads();
  plp_move<false>(stage, sld, a.cep + row0 * a.ldc, a.ldc, rows, order + 1, lane);
}

}  // namespace sk

extern "C" {

int sc_plp_cepstra(const float* d_logband, int64_t ldb, int64_t N, int32_t nb, int32_t order, const double* d_eql, const double* d_acw,
                   const double* d_lift, float* d_cep, int64_t ldc, float* d_post, int64_t ldp, void* stream) {
  using namespace sk;
  SK_CHECK(d_logband && d_eql && d_acw && d_lift && d_cep, SK_EARG, "sc_plp_cepstra: null argument");
  SK_CHECK(N >= 0 && N <= (int64_t)PLP_ROWS * 0x7fffffff, SK_EARG, "sc_plp_cepstra: N = %lld rows", (long long)N);
  SK_CHECK(nb >= SC_PLP_MIN_BANDS && nb <= SC_PLP_MAX_BANDS, SK_EARG, "sc_plp_cepstra: nb = %d outside [%d, %d]", nb, SC_PLP_MIN_BANDS, SC_PLP_MAX_BANDS);
  SK_CHECK(order >= 1 && order <= nb - 2, SK_EARG, "sc_plp_cepstra: order = %d outside [1, %d]", order, nb - 2);
  SK_CHECK(ldb >= nb, SK_EARG, "sc_plp_cepstra: ldb = %lld below nb = %d", (long long)ldb, nb);
  SK_CHECK(ldc >= order + 1, SK_EARG, "sc_plp_cepstra: ldc = %lld below order + 1 = %d", (long long)ldc, order + 1);
  SK_CHECK(!d_post || ldp >= nb, SK_EARG, "sc_plp_cepstra: ldp = %lld below nb = %d", (long long)ldp, nb);
  SK_CHECK(d_cep != d_logband && d_post != d_logband, SK_EARG, "sc_plp_cepstra: an output aliases d_logband");
  if (N == 0) return SK_OK;
  const PlpArgs a = {d_logband, (long)ldb, (long)N, nb, order, d_eql, d_acw, d_lift, d_cep, (long)ldc, d_post, (long)ldp};
  const size_t lds = (size_t)PLP_ROWS * ((size_t)(nb | 1) * sizeof(float) + (size_t)(nb + order + 1) * sizeof(double));
  hipLaunchKernelGGL(plp_cepstra_kernel, dim3((unsigned)((N + PLP_ROWS - 1) / PLP_ROWS)), dim3(PLP_ROWS), lds, (hipStream_t)stream, a);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
