// Total variability at ranks above SC_TV_MAX_RANK (include/sidekit_amd/ivector_wide.h): the per-session posterior with the session's
// matrix in caller-owned scratch instead of LDS, blocked on 64 x 64 tiles, every large product on the f64 matrix cores.
//   sc_tvw_gram        tv_gram_kernel of ivector.hip (tv_common.h), launched for R up to SC_TVW_MAX_RANK
//   sc_tvw_workspace   the scratch sc_tvw_posterior needs
//   sc_tvw_posterior   per session: Lambda = shift I + unpack(Lp), inv_lambda, e_h = inv_lambda b, E_hh = inv_lambda + e_h e_h'
//
// sc_tvw_posterior: one workgroup of 256 threads per session, alone on its slice of the scratch: W, Rp rows of ld = 2 Rp doubles,
// Rp = R rounded up to 64 (nt tiles), the augmented matrix [Lambda | I].  No other workgroup touches the slice, so there is no flag, no
// atomic and no fence beyond the __syncthreads() between a tile's stores and the workgroup's own later loads.  Rows and columns R .. Rp
// carry an identity diagonal: they stay decoupled (their products are exact zeros) and are never stored to an output.
//   0. The left half's upper tiles <- Lambda.  The identity of the right half is implied, never stored.
//   1. Left-looking block-row Cholesky of the augmented matrix, U' [U | Y] = [Lambda | I]: for block row I and column tile J
//        S_IJ = Aug_IJ - sum_{m < 64 I} U[m][I-tile]' Aug'[m][J-tile]       (dgemm_tile's TN form, the rows by pointer offset and K)
//        J = I: U_II' U_II = S_II, factored in LDS (right-looking, one row per step)
//        else:  Aug'_IJ = U_II^-T S_IJ by forward substitution, a column per lane group
//      The left half becomes U (upper tiles J >= I); the right half Y = U^-T (lower: tiles J <= I, whose sums start at row 64 J because
//      Y is zero above; Y_II is the substitution of the identity).
//   2. inv_lambda = Y' Y, upper tiles (I, J >= I) summed over rows >= 64 J (TN form again), written with their mirror image into the
//      left half, which U no longer needs: the symmetric inverse, whose columns the next step reads along rows.
//   3. e_h = inv_lambda b: thread i adds column i in four interleaved sums (j mod 4), joined (0 + 1) + (2 + 3).
//   4. E_hh = fma(e_i, e_j, inv_lambda_ij) to the packed output and / or its diagonal, one wave per row.
// About R^3 flop in the products of a session (a third each in U, Y and Y' Y), plus 64 x 64 substitutions on nt (nt + 1) tiles.
// Substitution (LAPACK's dtrsm order), not a product with the inverted diagonal tile: the residual of the result is then that of a
// Cholesky inverse with another blocking (tests/test_gpu_ivector_wide.py judges it against dpotrf + dpotri).  Plain float64 sums in a
// fixed order: a session's bits depend on its row, R and shift alone.  Zeros go through the MFMA exactly and sqrt(1) = 1, so all-zero
// counts with shift = 1 give inv_lambda = I and e_h = b bit for bit.
// LDS: two operand images (2 x 64 x DLD doubles), the centres dgemm_tile wants (128) and ONE 64 x 65 tile (U_II; later b and e_h) =
// 51,712 B: three workgroups fit the LDS of a CU.  S_IJ travels from the accumulators' lanes to the substitution's through the
// tile's own place in W (L2), not through a second LDS tile.
// Registers: 252 VGPRs, no scratch, two waves per SIMD = two workgroups per CU (__launch_bounds__(256, 2)), not the 128 VGPRs of
// tv_gram_kernel: the substitution keeps a lane's 16 rows beside the tile product's accumulators and fetch registers, and the compiler
// spends what the bound allows on addresses it hoists out of the job loop.  A third workgroup would only wait on the same division
// chain: a session is latency-bound in its 64 x 64 steps (the substitution is 64 dependent steps of shuffle, divide and FMA per tile).
#include <cmath>

#include "../../include/sidekit_amd/ivector_wide.h"
#include "dgemm_tile.h"
#include "tv_common.h"

namespace sk {

constexpr int TVW_THREADS = 256, TVW_TL = 64, TVW_ULD = TVW_TL + 1;

// Forward substitution U' x = s for 16 columns per wave: lane l holds rows g + 4 q (g = l >> 4, q < 16) of column l & 15 in s[q].
// Step k = 4 qk + gk: the owner of row k (lane group gk) hands s_k to the column's four lanes, x_k = s_k / U[k][k], and every later
// row m loses U[k][m] x_k.  After four steps the rows 4 qk + g are final: they go to dst[4 qk ld] and the registers move down by
// one, so that every register number is a constant while the loop over qk stays a loop (unrolled 64 times, the kernel needed 256
// VGPRs and 2.3 KB of scratch per lane).  The registers that have moved past row 63 hold nothing that is stored; their row number
// is clamped so that the reads stay inside Us.
__device__ inline void tvw_substitute(const double* Us, double (&s)[16], int g, int lane, double* dst, int ld) {
  const int col_lane = lane & 15;
#pragma unroll 1
  for (int qk = 0; qk < 16; ++qk) {
#pragma unroll
    for (int gk = 0; gk < 4; ++gk) {
      const double* Ur = Us + (4 * qk + gk) * TVW_ULD;   // row k of U_II
      const double x = __shfl(s[0], col_lane + 16 * gk, 64) / Ur[4 * qk + gk];
      if (g > gk) s[0] = fma(-Ur[4 * qk + g], x, s[0]);
#pragma unroll
      for (int q = 1; q < 16; ++q) {
        const int m = 4 * (qk + q) + g;
        s[q] = fma(-Ur[m < TVW_TL ? m : TVW_TL - 1], x, s[q]);
      }
      if (g == gk) s[0] = x;
    }
    dst[4 * qk * ld] = s[0];
#pragma unroll
    for (int q = 0; q < 15; ++q) s[q] = s[q + 1];
    s[15] = 0.0;
  }
}

// grid: x = session.  Lp and Ehh may be the same buffer (no __restrict__ on either): the row is in W before anything is stored.
// Bounds: W is indexed (row < Rp) * ld + (column < 2 Rp), the session's slice being Rp * ld doubles; dgemm_tile reads columns
// m0 .. m0 + 63 and n0 .. n0 + 63 < ld of K rows from a row offset r with r + K <= Rp; Us is indexed (< 64) * 65 + (< 64), and as
// b / e_h below 2 * 1024 <= 64 * 65; the outputs are indexed (i <= j < R) packed and (< R), rows of P and R doubles per session.
__global__ __launch_bounds__(TVW_THREADS, 2) void tvw_posterior_kernel(const double* Lp, const double* __restrict__ B, int R, int Rp, double shift,
                                                                         double* __restrict__ Eh, double* Ehh, double* __restrict__ diag,
                                                                         double* work) {
  constexpr int WT = 2, TL = TVW_TL, ULD = TVW_ULD;
  __shared__ __attribute__((aligned(16))) double As[TL * DLD];
  __shared__ __attribute__((aligned(16))) double Bs[TL * DLD];
  __shared__ double cs[2 * TL];
  __shared__ double Us[TL * ULD];
  const dgemm_lanes<WT> at;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub_n = 16 * wave + (lane & 15), sub_g = lane >> 4;   // the substitution's column and row group
  const int ld = 2 * Rp, nt = Rp / TL;
  const long session = blockIdx.x, P = tv_packed(R);
  double* W = work + session * ((long)Rp * ld);
  f64x4 acc[WT][WT];

  // 0. Lambda into the upper tiles of the left half (the whole diagonal tile: zeros below the diagonal), identity beyond R
  {
    const double* src = Lp + session * P;
    for (int i = wave; i < Rp; i += 4) {
      const int ri = i < R ? tv_rb(i, R) : 0;
      for (int j = (i & ~(TL - 1)) + lane; j < Rp; j += 64) {
        double v = i == j ? 1.0 : 0.0;
        if (j >= i && j < R) v = src[ri + j] + (i == j ? shift : 0.0);
        W[i * ld + j] = v;
      }
    }
  }

  // 1. U' [U | Y] = [Lambda | I], block row after block row.  The jobs of block row I, in this order: t = 0 the diagonal tile,
  // t < nt - I the tiles U_IJ (J = I + t), t < nt the tiles Y_IJ (J = t - (nt - I) < I; Y is zero above row 64 J, where the sum starts),
  // t = nt the tile Y_II = U_II^-T, the substitution of the identity.  One loop, so that the tile product and the substitution are
  // in the kernel once each.
  for (int I = 0; I < nt; ++I) {
    const int r0 = I * TL;
    double* Wr = W + r0 * ld;
    for (int t = 0; t <= nt; ++t) {
      const bool left = t < nt - I;
      const int J = left ? I + t : t - (nt - I);      // t = nt: J = I
      const int n0 = left ? J * TL : Rp + J * TL;
      double s[16];
      if (t < nt) {
        const double* Wj = W + (left ? 0 : J * TL * ld);
        __syncthreads();   // the stores of the jobs before (and of step 0); at t = 0 every lane is done with the last U_II
        dgemm_tile<WT, true, true, double, double>(Wj, Wj, ld, ld, left ? r0 : r0 - J * TL, r0, n0, As, Bs, acc, nullptr, nullptr, nullptr, cs);
      }
      if (t == 0) {
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < WT; ++j) {
              const int m = at.row(i, q), n = at.col(j);
              Us[m * ULD + n] = Wr[m * ld + r0 + n] - acc[i][j][q];
            }
        __syncthreads();
        // U_II' U_II = S_II on the upper triangle of Us: row k is scaled by its pivot, then leaves the rows below it
        for (int k = 0; k < TL; ++k) {
          const double pivot = sqrt(Us[k * ULD + k]);
          if (tid > k && tid < TL) Us[k * ULD + tid] /= pivot;
          __syncthreads();
          for (int i = k + 1 + wave; i < TL; i += 4)
            if (lane >= i) Us[i * ULD + lane] = fma(-Us[k * ULD + i], Us[k * ULD + lane], Us[i * ULD + lane]);
          if (tid == 0) Us[k * ULD + k] = pivot;
          __syncthreads();
        }
        for (int i = wave; i < TL; i += 4) Wr[i * ld + r0 + lane] = lane >= i ? Us[i * ULD + lane] : 0.0;
        continue;
      }
      if (t < nt) {
        // S = (left ? Aug_IJ : 0) - acc at the tile's place in W, then read back in the substitution's lanes
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < WT; ++j) {
              double* p = Wr + at.row(i, q) * ld + n0 + at.col(j);
              *p = (left ? *p : 0.0) - acc[i][j][q];
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) s[q] = Wr[(sub_g + 4 * q) * ld + n0 + sub_n];
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) s[q] = sub_g + 4 * q == sub_n ? 1.0 : 0.0;
      }
      tvw_substitute(Us, s, sub_g, lane, Wr + sub_g * ld + n0 + sub_n, ld);   // U_II^-T S, stored over S
    }
  }

  // 2. inv_lambda = Y' Y into the left half, both triangles; a diagonal tile's lower half is the mirror of its upper one
  for (int I = 0; I < nt; ++I)
    for (int J = I; J < nt; ++J) {
      const double* Yj = W + J * TL * ld;
      __syncthreads();
      dgemm_tile<WT, true, true, double, double>(Yj, Yj, ld, ld, Rp - J * TL, Rp + I * TL, Rp + J * TL, As, Bs, acc, nullptr, nullptr, nullptr, cs);
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int j = 0; j < WT; ++j) {
            const int m = I * TL + at.row(i, q), n = J * TL + at.col(j);
            if (n >= m) {
              W[m * ld + n] = acc[i][j][q];
              W[n * ld + m] = acc[i][j][q];
            }
          }
    }
  __syncthreads();

  // 3. e_h = inv_lambda b
  double* es = Us;
  double* bs = Us + SC_TVW_MAX_RANK;
  if (B) {
    for (int i = tid; i < R; i += TVW_THREADS) bs[i] = B[session * R + i];
    __syncthreads();
    for (int i = tid; i < R; i += TVW_THREADS) {
      double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
      int j = 0;
      for (; j + 4 <= R; j += 4) {
        e0 = fma(W[j * ld + i], bs[j], e0);
        e1 = fma(W[(j + 1) * ld + i], bs[j + 1], e1);
        e2 = fma(W[(j + 2) * ld + i], bs[j + 2], e2);
        e3 = fma(W[(j + 3) * ld + i], bs[j + 3], e3);
      }
      for (; j < R; ++j) e0 = fma(W[j * ld + i], bs[j], e0);
      const double e = (e0 + e1) + (e2 + e3);
      es[i] = e;
      Eh[session * R + i] = e;
    }
    __syncthreads();
  }

  // 4. E_hh = inv_lambda + e_h e_h' (inv_lambda alone without b): one wave per row
  for (int i = wave; i < R; i += 4) {
    const int ri = tv_rb(i, R);
    const double ei = B ? es[i] : 0.0;
    for (int j = i + lane; j < R; j += 64) {
      double v = W[i * ld + j];
      if (B) v = fma(ei, es[j], v);
      if (Ehh) Ehh[session * P + ri + j] = v;
      if (diag && j == i) diag[session * R + i] = v;
    }
  }
}

static int tvw_padded(int R) { return cdiv(R, TVW_TL) * TVW_TL; }

}  // namespace sk

using namespace sk;

extern "C" {

int sc_tvw_gram(const double* d_F, int32_t C, int32_t D, int32_t R, double* d_G, void* stream) {
  SK_CHECK(d_F && d_G, SK_EARG, "sc_tvw_gram: null argument");
  SK_CHECK(C >= 1 && D >= 1 && R >= 1 && R <= SC_TVW_MAX_RANK, SK_EARG, "sc_tvw_gram: bad sizes (C=%d, D=%d, R=%d with at most %d)", C, D, R,
           SC_TVW_MAX_RANK);
  return tv_gram_launch(d_F, C, D, R, cdiv(R, 64), d_G, (hipStream_t)stream);
}

int sc_tvw_workspace(int32_t N, int32_t R, int64_t* bytes) {
  SK_CHECK(bytes, SK_EARG, "sc_tvw_workspace: null argument");
  SK_CHECK(N >= 1 && R >= 1 && R <= SC_TVW_MAX_RANK, SK_EARG, "sc_tvw_workspace: bad sizes (N=%d, R=%d with at most %d)", N, R, SC_TVW_MAX_RANK);
  const int64_t Rp = tvw_padded(R);
  *bytes = (int64_t)N * 2 * Rp * Rp * (int64_t)sizeof(double);
  return SK_OK;
}

int sc_tvw_posterior(const double* d_Lp, const double* d_B, int32_t N, int32_t R, double shift, double* d_Eh, double* d_Ehh, double* d_diag,
                     void* d_work, int64_t work_bytes, void* stream) {
  SK_CHECK(d_Lp && d_work, SK_EARG, "sc_tvw_posterior: null argument");
  SK_CHECK((d_B != nullptr) == (d_Eh != nullptr), SK_EARG, "sc_tvw_posterior: d_B and d_Eh are both null or both set");
  SK_CHECK(d_Ehh || d_diag, SK_EARG, "sc_tvw_posterior: at least one of d_Ehh and d_diag is not null");
  SK_CHECK(N >= 1 && R >= 1 && R <= SC_TVW_MAX_RANK, SK_EARG, "sc_tvw_posterior: bad sizes (N=%d, R=%d with at most %d)", N, R, SC_TVW_MAX_RANK);
  SK_CHECK(shift >= 0.0 && std::isfinite(shift), SK_EARG, "sc_tvw_posterior: shift = %g is negative or not finite", shift);
  int64_t need = 0;
  sc_tvw_workspace(N, R, &need);
  SK_CHECK(work_bytes >= need, SK_EARG, "sc_tvw_posterior: %lld bytes of scratch, %lld needed (sc_tvw_workspace)", (long long)work_bytes,
           (long long)need);
  hipLaunchKernelGGL(tvw_posterior_kernel, dim3((unsigned)N), dim3(TVW_THREADS), 0, (hipStream_t)stream, d_Lp, d_B, R, tvw_padded(R), shift, d_Eh,
                     d_Ehh, d_diag, (double*)d_work);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

}  // extern "C"
