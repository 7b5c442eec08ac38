// The f64 MFMA GEMM tile of the float64 back end (scoring.hip, score_norm.hip, plda_train.hip, gaussian_backend.hip, ivector.hip, jfa.hip)
// and what its users share beside it: the pair loader (fetch_pair), the two operand layouts and their LDS places (fetch_along_k / along_k_at,
// fetch_across / across_at; whiten_rows_kernel of backend.hip, whose wave grid is its own, stands on these too), the accumulators' lane map
// (dgemm_lanes) and the plain guarded store of a tile (dgemm_store_tile).
#pragma once
#include "common.h"

namespace sk {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// f64 GEMM tile on the matrix cores, the core of fast / full PLDA scoring and of PLDA training.
//   v_mfma_f64_16x16x4_f64: A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], D: four doubles per lane at row (l >> 4) + 4 * reg,
//   col l & 15 (the f64 map, which differs from the f32 one); 64 matrix-pipe cycles each (78.6 TFLOP/s = 32 FLOP / clk / SIMD).
// Four waves in a 2 x 2 grid, each WT x WT MFMA tiles: WT = 2 -> 64 x 64 per workgroup (small trial sets: enough workgroups to fill 256
// CUs), WT = 4 -> 128 x 128 (half the operand traffic per FLOP, 64 accumulator doubles per lane, two workgroups per CU).  Operands are
// staged through LDS as [row][k] with a 17-double row stride (ds_read_b64 fragment reads: 16 rows x 2 k per half-wave land on 32
// different bank pairs but one), the next k-tile's operands are fetched into registers (16-byte loads) while this one is multiplied.
//   B_KN = false: B is [N][K] (C = A . B^T);  B_KN = true: B is [K][N] (C = A . B)
//   A_KM = false: A is [M][K];  A_KM = true: A is [K][M] (C = A^T . B, the "TN" product of PLDA training: K is the long dimension)
// The A_KM form reads float32 or float64 operands (TA, TB; widened in the load) and can weight and centre them on the way into LDS:
//   C[m][n] = sum_k w[k] (A[k][m] - ca[m]) (B[k][n] - cb[n]),   w, ca, cb optional; cs = 2 * T doubles of LDS for the two centres.
// ROWC (with A_KM, B = A, N = M): the centre is a per-ROW one gathered through a class number, and so is the weight:
//   C[m][n] = sum_k w[cls[k]] (A[k][m] - ca[cls[k]][m]) (A[k][n] - ca[cls[k]][n]),   ca: [C][M] class means, w: [C] or null;
//   rows whose class number is outside [0, C) get weight 0 and no centre is read for them; cb and cs are unused.
constexpr int DK = 16, DLD = DK + 1;

template <typename T> struct pair_of;
template <> struct pair_of<double> { typedef double2 type; };
template <> struct pair_of<float> { typedef float2 type; };

// elements i, i + 1 of a row of n (zero beyond it); vec: the pair may be read with one load.  The one place a pair is read.
template <typename T>
__device__ inline double2 fetch_pair(const T* __restrict__ src, bool vec, int i, int n) {
  double2 v = {0.0, 0.0};
  if (vec && i + 1 < n) {
    const typename pair_of<T>::type p = *reinterpret_cast<const typename pair_of<T>::type*>(src);
    v.x = (double)p.x; v.y = (double)p.y;
  } else {
    if (i < n) v.x = (double)src[0];
    if (i + 1 < n) v.y = (double)src[1];
  }
  return v;
}

// The two operand layouts of a k-tile, by the thread's pair number idx: which pair it fetches, and where the pair goes in the LDS image
// ([row][k], DLD doubles per row).
//   "along k": src is [rows][K]; 8 threads take the 8 pairs of row r0 + along_k_row(idx); zero beyond `rows` and K.  I: the type of the
//   row numbers (int, or long where a row number times K passes 2^31).
__device__ inline int along_k_row(int idx) { return idx >> 3; }

template <typename T, typename I>
__device__ inline double2 fetch_along_k(const T* __restrict__ src, bool vec, I r0, I rows, int k0, int K, int idx) {
  const I r = r0 + along_k_row(idx);
  const int k = k0 + (idx & 7) * 2;
  double2 v = {0.0, 0.0};
  if (r < rows) v = fetch_pair(src + (long)r * K + k, vec, k, K);
  return v;
}

__device__ inline int along_k_at(int idx) { return along_k_row(idx) * DLD + (idx & 7) * 2; }   // the pair's place in LDS: [at], [at + 1]

//   "across": src is [K][cols]; TC / 2 threads take the pairs of k-row k0 + across_k(idx), from column c0 + across_col(idx) on; zero
//   beyond K and `cols`.  TC: the columns of the tile.
template <int TC> __device__ inline int across_k(int idx) { return idx / (TC / 2); }
template <int TC> __device__ inline int across_col(int idx) { return (idx % (TC / 2)) * 2; }

template <int TC, typename T>
__device__ inline double2 fetch_across(const T* __restrict__ src, bool vec, int k0, int K, int c0, int cols, int idx) {
  const int k = k0 + across_k<TC>(idx), c = c0 + across_col<TC>(idx);
  double2 v = {0.0, 0.0};
  if (k < K) v = fetch_pair(src + (long)k * cols + c, vec, c, cols);
  return v;
}

template <int TC> __device__ inline int across_at(int idx) { return across_col<TC>(idx) * DLD + across_k<TC>(idx); }   // [at], [at + DLD]

// Where a lane's accumulators lie in dgemm_tile's workgroup tile (four waves, 2 x 2): acc[i][j][q] is row row(i, q), column col(j).
template <int WT>
struct dgemm_lanes {
  int wm, wn, lr, lk;
  __device__ dgemm_lanes() {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    wm = wave >> 1; wn = wave & 1; lr = lane & 15; lk = lane >> 4;
  }
  __device__ int row(int i, int q) const { return wm * 16 * WT + i * 16 + lk + 4 * q; }
  __device__ int col(int j) const { return wn * 16 * WT + j * 16 + lr; }
};

// dst[m][n] = the tile's element (m, n) for m < M and n < N; ld doubles per row of dst
template <int WT>
__device__ inline void dgemm_store_tile(const f64x4 (&acc)[WT][WT], const dgemm_lanes<WT>& at, double* __restrict__ dst, int ld, int m0, int n0,
                                        int M, int N) {
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + at.row(i, q);
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int n = n0 + at.col(j);
        if (n < N) dst[(long)m * ld + n] = acc[i][j][q];
      }
    }
}

template <int WT, bool B_KN, bool A_KM = false, typename TA = double, typename TB = double, bool ROWC = false>
__device__ inline void dgemm_tile(const TA* __restrict__ A, const TB* __restrict__ B, int M, int N, int K, int m0, int n0,
                                  double* As, double* Bs, f64x4 (&acc)[WT][WT], const double* __restrict__ w = nullptr,
                                  const double* __restrict__ ca = nullptr, const double* __restrict__ cb = nullptr, double* cs = nullptr,
                                  const int* __restrict__ cls = nullptr, int C = 0) {
  static_assert(!A_KM || B_KN, "the A [K][M] form comes with B [K][N]");
  static_assert(!ROWC || (A_KM && std::is_same<TA, TB>::value), "gathered row centres: A_KM form with B = A");
  static_assert(A_KM || (std::is_same<TA, double>::value && std::is_same<TB, double>::value), "float32 operands: A_KM form only");
  constexpr int T = 32 * WT;            // workgroup tile edge
  constexpr int PA = T * DK / 2 / 256;  // double pairs per thread and operand
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const bool vec_a = ((A_KM ? M : K) & 1) == 0 && (reinterpret_cast<size_t>(A) & (2 * sizeof(TA) - 1)) == 0;
  const bool vec_b = ((B_KN ? N : K) & 1) == 0 && (reinterpret_cast<size_t>(B) & (2 * sizeof(TB) - 1)) == 0;
  double2 ra[PA], rb[PA];
  double rw[A_KM ? PA : 1];   // A_KM: the weight of each fetched k-row, 0 beyond K (which also zeroes the centred padding)
  if constexpr (A_KM && !ROWC) {
    for (int i = tid; i < 2 * T; i += 256) {
      const int j = i < T ? m0 + i : n0 + i - T;
      cs[i] = i < T ? (ca && j < M ? ca[j] : 0.0) : (cb && j < N ? cb[j] : 0.0);
    }
  }
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < PA; ++q) {
      const int idx = tid + 256 * q;
      if constexpr (ROWC) {  // A [K][M] and the same rows again as B, each less its class's mean (rows of ca are M long: N = M).
        // The "across" layout in its own spelling, here and in stage: through the shared functions sc_scatter_within measured slower.
        const int kk = idx / (T / 2), mp = (idx % (T / 2)) * 2, m = m0 + mp, n = n0 + mp, k = k0 + kk;
        double2 va = {0.0, 0.0}, vb = {0.0, 0.0};
        double wk = 0.0;
        if (k < K) {
          const int c = cls[k];
          if (c >= 0 && c < C) {
            const bool vec_c = (M & 1) == 0 && (reinterpret_cast<size_t>(ca) & 15) == 0;
            const double2 xa = fetch_pair(A + (long)k * M + m, vec_a, m, M), xb = fetch_pair(A + (long)k * M + n, vec_a, n, M);
            const double2 ma = fetch_pair(ca + (long)c * M + m, vec_c, m, M), mb = fetch_pair(ca + (long)c * M + n, vec_c, n, M);
            va.x = xa.x - ma.x; va.y = xa.y - ma.y; vb.x = xb.x - mb.x; vb.y = xb.y - mb.y;
            wk = w ? w[c] : 1.0;
          }
        }
        ra[q] = va; rb[q] = vb; rw[q] = wk;
      } else {
        if constexpr (A_KM) {
          const int k = k0 + across_k<T>(idx);
          ra[q] = fetch_across<T>(A, vec_a, k0, K, m0, M, idx);
          rw[q] = k < K ? (w ? w[k] : 1.0) : 0.0;
        } else {
          ra[q] = fetch_along_k(A, vec_a, m0, M, k0, K, idx);
        }
        if constexpr (B_KN) rb[q] = fetch_across<T>(B, vec_b, k0, K, n0, N, idx);
        else rb[q] = fetch_along_k(B, vec_b, n0, N, k0, K, idx);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < PA; ++q) {
      const int idx = tid + 256 * q;
      if constexpr (ROWC) {   // in its own spelling, as in fetch
        const int kk = idx / (T / 2), np = (idx % (T / 2)) * 2;
        As[np * DLD + kk] = ra[q].x * rw[q]; As[(np + 1) * DLD + kk] = ra[q].y * rw[q];
        Bs[np * DLD + kk] = rb[q].x; Bs[(np + 1) * DLD + kk] = rb[q].y;
      } else {
        const int along = along_k_at(idx), x = across_at<T>(idx), y = x + DLD;
        const int c = across_col<T>(idx);   // the column whose centre cs holds (A_KM)
        if constexpr (!A_KM) { As[along] = ra[q].x; As[along + 1] = ra[q].y; }
        else { As[x] = (ra[q].x - cs[c]) * rw[q]; As[y] = (ra[q].y - cs[c + 1]) * rw[q]; }
        if constexpr (!B_KN) { Bs[along] = rb[q].x; Bs[along + 1] = rb[q].y; }
        else if constexpr (!A_KM) { Bs[x] = rb[q].x; Bs[y] = rb[q].y; }
        else { Bs[x] = rb[q].x - cs[T + c]; Bs[y] = rb[q].y - cs[T + c + 1]; }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += DK) {
    __syncthreads();   // every wave is done reading the previous k-tile (and, the first time, the centres are in LDS)
    stage();
    __syncthreads();
    if (k0 + DK < K) fetch(k0 + DK);
#pragma unroll
    for (int kk = 0; kk < DK; kk += 4) {
      double a[WT], b[WT];
#pragma unroll
      for (int i = 0; i < WT; ++i) {
        a[i] = As[(wm * 16 * WT + i * 16 + lr) * DLD + kk + lk];
        b[i] = Bs[(wn * 16 * WT + i * 16 + lr) * DLD + kk + lk];
      }
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
}

}  // namespace sk
