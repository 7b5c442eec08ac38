// 3x3 convolution + folded BatchNorm (+ReLU) (+SE plane sums) (+residual, + the first block's 1x1 shortcut) for the
// HalfResNet34 trunk: reference BasicBlock.forward, sidekit/nnet/res_net.py:309-320 (K5/K6 of
// SURVEY 2.3), built MI355X-first:
//
//  * activations are NHWC ([B][H=time][W=freq][C]); one workgroup owns TH full-width output rows,
//    stages the (TH-1)*S+3 input rows (+1 zero column each side) ONCE in LDS and reads all nine
//    taps from there, so HBM sees each input row ~(1 + 2/TH) times instead of 9;
//  * the contraction runs on the matrix cores as an implicit GEMM D[cout][pos] += W[cout][k] *
//    X[k][pos] (k = tap x cin) with 32x32 MFMA tiles: v_mfma_f32_32x32x16_bf16 for the bf16
//    path, v_mfma_f32_32x32x2_f32 (exact f32 FMA chain) for the fp32 parity path;
//  * weights are pre-packed on the host in MFMA *fragment order* (64 lanes x 16 B per k-step), so
//    every wave streams its A operand from L2 with perfectly coalesced 1-KiB loads and the LDS is
//    left to the activations;
//  * positions sit on the MFMA lanes, channels in the accumulator registers; the epilogue applies BN
//    scale/shift, ReLU and the squeeze-excite plane sums in registers, transposes the tile through the
//    consumed LDS buffer and writes it as contiguous 16-B-per-lane NHWC rows;
//  * per-utterance lengths: rows >= the utterance's own row count are read as zero
//    padding and never written, so a padded batch reproduces each utterance run alone;
//  * one template, three compile-time epilogue forms (statistics for the SE gate / residual / residual with the
//    first block's 1x1 shortcut convolution evaluated in place), two LDS images (padded, or pad-free and swizzled),
//    per-shape occupancy: persistent weight-resident workgroups for the 32-channel inputs, three workgroups per
//    CU at 168 registers for layers 2-3, small tiles for the stride-2 shapes (DESIGN.md section 4 has the measurements
//    behind each choice).
#include "kernels.h"

namespace sk {

template <typename T> __device__ inline void mma_step(f32x16& acc, const uint4& w, const uint4& x);

template <> __device__ inline void mma_step<bf16_t>(f32x16& acc, const uint4& w, const uint4& x) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}
template <> __device__ inline void mma_step<float>(f32x16& acc, const uint4& w, const uint4& x) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.x), __builtin_bit_cast(float, x.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.y), __builtin_bit_cast(float, x.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.z), __builtin_bit_cast(float, x.z), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(float, w.w), __builtin_bit_cast(float, x.w), acc, 0, 0, 0);
}

enum { LANES_LINEAR = 0, LANES_GRID = 1, LANES_DENSE = 2 };
template <typename T_, int CIN_, int COUT_, int S_, int WIN_, int TH_, int WM_, int WN_, int MW_, int NW_, int CK_, int OCC_ = 0, int PD_ = 0, bool SWZ_ = false, int BLK_ = LANES_LINEAR, bool M16_ = false, bool S2G_ = false>
struct ConvCfg {
  using T = T_;
  static constexpr int EB = elem<T_>::bytes;
  static constexpr int CIN = CIN_, COUT = COUT_, S = S_, WIN = WIN_, TH = TH_, WM = WM_, WN = WN_, MW = MW_, NW = NW_, CK = CK_;
  static constexpr int WOUT = WIN / S;
  static constexpr int MT = TH * WOUT;           // positions per workgroup
  static constexpr int NT = WN * NW * 32;        // output channels per workgroup
  static constexpr int RIN = (TH - 1) * S + 3;   // staged input rows
  static constexpr int WP = WIN + 2;             // staged input columns (zero column each side)
  static constexpr int CB = CK * EB;             // channel bytes staged per position
  // Two LDS images of the halo tile:
  //  padded   (SWZ = false): [zero col][WIN positions][zero col], CB + 16 B per position (the +16 makes ds_read_b128 of 32
  //           neighbouring positions conflict-free), rows on 1-KiB piece boundaries.  Pad slots and zero columns are DMA
  //           lanes that read the zero page: 70 pieces for a layer1 tile of 51 KB.
  //  swizzled (SWZ = true): CB bytes per position, no pad slots; the 16-B chunk c of column p sits at slot c ^ f(p)
  //           (f below), which is as conflict-free as the padding and costs nothing to stage because a DMA lane may fetch any
  //           global address; ONE zero position after each row serves as the zero column on both sides (column -1 of a
  //           row is read from that row's own trailing zero position) and is written by ds_write.  A row is WIN * CB
  //           bytes = whole pieces: 50 pieces for the same layer1 tile, and a 128-channel layer3 tile is 10 x 5376 B =
  //           53760 B = exactly 42 of the 1280-B LDS allocation granules, so three workgroups fit a CU.
  static constexpr bool SWZ = SWZ_;
  // Which output position an MFMA lane owns.  A wave64 ds_read_b128 is served in four 16-lane groups -- lanes {0-3, 12-15, 20-27}
  // and {4-11, 16-19, 28-31} of each half (MI355X_MICROARCH.md, LDS table) -- and a group takes one LDS cycle only when its 16
  // addresses fall on 16 different 16-B slots of the 256-B bank row.  With lanes in linear tile order (LANES_LINEAR: m = tile*32 +
  // lane, row = m / W) a group straddles rows whenever W is not a multiple of 16, and a column-only swizzle then repeats slots:
  // rocprofv3 counted 55 % (layer 3), 62 % (layer 4), 70 % (layer 4 stride 2) of all LDS cycles as bank-conflict cycles, exactly
  // what scripts/lds_conflicts.py computes from the addresses.  Two conflict-free assignments (swizzled image, stride 1, 3x3):
  //  LANES_GRID : the 16 lanes of read group (wave row wm, M-tile i, group g) own the GR x GC block (GR * GC = 16) at block row
  //               2*wm + g, block column i of the TH x W tile; swizzle key = (row & (GR-1), col & (GC-1)) -> 16 distinct slots under
  //               every tap shift.  Needs W = MW * GC and TH = 2 * WM * GR: layer 1 (1 x 16), layer 2 (2 x 8), layer 3 (4 x 4).
  //  LANES_DENSE: lanes enumerate the tile INCLUDING the zero column, L = row * (W+1) + col = tile*32 + lane, key = L & 15: any 32
  //               consecutive L are conflict-free and a tap shift is a constant added to L.  Lanes on the zero column compute
  //               nothing useful: layer 4 (17 x 11 = 187 of its 192 lane slots, no extra MFMA work).
  // In both, M-tile i and tap (dh, dw) enter a lane's LDS address only through an instruction immediate: the per-lane part is
  // one register per tap (or per dw), XORed with the k-step -- one VALU instruction per k-step instead of one per M-tile.
  static constexpr int BLK = BLK_;
  static constexpr int GC = BLK == LANES_GRID ? (WIN_ / S_) / MW_ : 16, GR = 16 / GC;   // read-group block (GRID)
  static_assert(BLK == LANES_LINEAR || (SWZ_ && S_ == 1), "block lane orders: swizzled image, stride 1");
  static_assert(BLK != LANES_GRID || (GC * MW_ == WIN_ / S_ && GR * GC == 16 && TH_ == 2 * WM_ * GR), "GRID: W = MW * GC, TH = 2 * WM * GR");
  static_assert(BLK != LANES_DENSE || (WM_ == 1 && CK_ * elem<T_>::bytes == 256 && TH_ * (WIN_ + 1) <= MW_ * 32), "DENSE: 256-B positions, one wave row");
  // a leading zero position in front of the image makes column -1 of a row the physically preceding position (no address
  // remap); layer 3 has no room for it (53760 B = 42 LDS granules exactly) and remaps column -1 of block column 0 instead
  // MFMA shape.  M16: v_mfma_f32_16x16x32_bf16 instead of 32x32x16 -- the same FLOPs per matrix-pipe cycle and the same operand
  // bytes per FLOP, but the chip holds a much higher clock on it (bare MFMA loops on random operands: 2.1 vs 1.65 GHz,
  // scripts/probe_mfma_power.hip; layer 3 timed with this shape: 102 vs 151 us).  A lane then owns ONE position (l & 15) of a
  // 16-position tile = one read-group block (GRID) or 16 consecutive padded-image positions (DENSE), and the 16-B chunk
  // 4 * s + (l >> 4) of a 32-channel k-step s; its accumulator holds output channels 4 * (l >> 4) .. + 3 of a 16-channel tile.
  static constexpr bool M16 = M16_;
  static_assert(!M16 || ((BLK != LANES_LINEAR || S2G_) && elem<T_>::bytes == 2 && (CK_ * 2) % 64 == 0), "M16: bf16, block lane orders (or the planar stride-2 image), 64-B k-steps");
  static constexpr bool LEAD = BLK == LANES_DENSE || (BLK == LANES_GRID && CK_ * elem<T_>::bytes < 256);
  static constexpr int IMG0 = LEAD ? CK_ * elem<T_>::bytes : 0;
  static constexpr int PSTRIDE = SWZ ? CB : CB + 16;
  static constexpr int SPP = PSTRIDE / 16;                // 16-B slots per staged position
  static constexpr int PPR = ((SWZ ? WIN : WP) * SPP + 63) / 64;   // 1-KiB LDS-DMA pieces per staged row
  static constexpr int RS = SWZ ? (WIN + 1) * CB : PPR * 1024;     // LDS row stride
  static constexpr int LDS_SWZ = (RIN - 1) * RS + (PPR * 1024 > RS ? PPR * 1024 : RS);   // a masked partial last piece still addresses whole KiB
  // DENSE: idle lanes past the tile read up to two rows beyond the staged image (never used: keep them inside the allocation)
  static constexpr int LDS_BLK = BLK == LANES_DENSE ? IMG0 + (MW * 32 + 2 * (WIN + 1) + 2) * CB : IMG0 + LDS_SWZ;
  static constexpr int LDS_IN = BLK ? (LDS_BLK + 255) / 256 * 256 : (SWZ ? (LDS_SWZ + 255) / 256 * 256 : RIN * RS);
  static constexpr int LDS_OUT = TH_ * (WIN_ / S_) * (WN_ * 32 * elem<T_>::bytes + 16);   // the epilogue's transposition tile reuses the buffer
  static constexpr int LDS = LDS_IN > LDS_OUT ? LDS_IN : (LDS_OUT + 255) / 256 * 256;
  static constexpr int SWF = SPP < 16 ? SPP : 16;         // swizzle period in slots
  static constexpr int SWSH = SPP == 4 ? 2 : (SPP == 8 ? 1 : 0);   // f(p) = (p >> SWSH) & (SWF - 1): 16 consecutive columns hit 16 distinct bank groups
  // swizzle key of the staged position (staged row, column): XORed into the 16-B chunk index of the position
  static constexpr int KCMASK = (GC >> SWSH) - 1;                   // GRID: column bits of the key, (col >> SWSH) & KCMASK
  static constexpr int KRSH = SWSH == 0 ? (GC == 4 ? 2 : (GC == 8 ? 3 : 4)) : (SWSH == 1 ? (GC == 8 ? 2 : 3) : 2);   // log2(GC) - SWSH
  // S2G: the stride-2 first convolution of a layer on a PLANAR image, with the 16x16x32 MFMA.  A tap of a stride-2 convolution
  // reads every other staged column, so on the row-major image its lanes only ever touch half of the 16-B slots of a bank row (rocprofv3:
  // 48 / 58 / 70 % of the LDS cycles of layers 2 / 3 / 4 were conflict cycles; scripts/lds_conflicts.py: 7.8 / 10 / 14 cycles per read).
  // Staged row = [even columns | odd columns | zero position] (a DMA lane may fetch any global address, so the permutation is free): a
  // tap's lanes then read CONSECUTIVE positions of one plane, in S2GR x S2GC blocks of 16 output positions (2 x 8 at W_out 40, 4 x 4 at 20,
  // 8 x 2 at 10).  Key = (output-row bits, the position bits above the bank row).
  static constexpr bool S2G = S2G_;
  static_assert(!S2G_ || M16_, "S2G: the planar image is read by the 16x16x32 MFMA lane order only");
  static constexpr int S2GR = S2G_ ? TH_ / WM_ : 1, S2GC = 16 / S2GR, S2NBC = (WIN_ / S_) / S2GC;
  static constexpr int S2PPB = 256 / (CK_ * elem<T_>::bytes) > 0 ? 256 / (CK_ * elem<T_>::bytes) : 1;   // positions per 256-B bank row
  static constexpr int S2PB = S2GC / S2PPB > 0 ? S2GC / S2PPB : 1;                                         // key values taken from the position
  static_assert(!S2G_ || (BLK_ == LANES_LINEAR && SWZ_ && S_ == 2 && TH_ % WM_ == 0 && S2GR * S2GC == 16 &&
                          (WIN_ / 2) % S2GC == 0 && 2 * MW_ >= S2NBC && S2GC >= S2PPB && S2GR * S2PB == CK_ * elem<T_>::bytes / 16),
                "S2G: stride 2, swizzled image, 16-position blocks that tile the output rows, one key value per slot of a position");
  __host__ __device__ static constexpr int unplanar(int P) { return P < WIN / 2 ? 2 * P : 2 * (P - WIN / 2) + 1; }   // P < WIN
  // A lane is ONE position (l & 15) of a 16-position tile = one S2GR x S2GC block (block row = wave row, block column = tile index: W_out / S2GC = 5 tiles per wave for all three shapes, no idle
  // MFMA rows -- the 32-row tiles wasted a sixth) and the 16-B chunk 4 s + (l >> 4) of a 32-channel k-step.  A read group of a
  // ds_read_b128 then carries chunk q for tile positions {0-3, 12-15} and chunk q + 1 for {4-11}, so besides 16 different (bank-row
  // part, key) pairs no position of the first half may have a key that differs from one of the second half in bit 0 alone:
  //   2 x 8 (layer 2): halves = the two rows (the row bit of the key separates them, as in layer 2's stride-1 shape);
  //   4 x 4 (layer 3): halves = rows {0, 1} / {2, 3} (row-pair bits 1-2 of the key);
  //   8 x 2 (layer 4): halves = even / odd rows and the 3-bit row key ROTATED left by one (key bit 0 = bit 2 of the row pair): two rows
  //                    whose keys differ in bit 0 alone are 4 apart, i.e. in the same half -- also after the (dh = 2) shift of the row pair.
  // scripts/lds_conflicts.py (s2_m16_report): 4.27 LDS cycles per read for all three (the tile-0 reads of the zero position are the .27).
  __host__ __device__ static constexpr int s2_rowkey(int row) {
    const int hp = (row >> 1) & (S2GR - 1);
    return (S2GR == 8 ? (((hp << 1) & 7) | (hp >> 2)) : hp) * S2PB;
  }
  __host__ __device__ static constexpr int s2p_half(int p) { return (p >= 4 && p < 12) ? 1 : 0; }
  __host__ __device__ static constexpr int s2p_j(int p) { return p < 4 ? p : (p < 12 ? p - 4 : p - 8); }
  __host__ __device__ static constexpr int s2p_row(int p) { return S2GR == 8 ? 2 * (s2p_j(p) / S2GC) + s2p_half(p) : s2p_half(p) * (S2GR / 2) + s2p_j(p) / S2GC; }
  __host__ __device__ static constexpr int s2p_col(int p) { return s2p_j(p) % S2GC; }
  static constexpr int PT16 = S2G_ ? S2NBC : 2 * MW_;   // 16-position tiles per wave (M16); MT16 = 2 * MW tile slots
  __host__ __device__ static constexpr int swz_key(int row, int col) {   // (staged row, staged position)
    if (S2G) return s2_rowkey(row) | ((col / S2PPB) & (S2PB - 1));
    if (BLK == LANES_GRID) return (((row & (GR - 1)) << KRSH) | ((col >> SWSH) & KCMASK)) & (SWF - 1);
    if (BLK == LANES_DENSE) return dense_key((row * (WIN + 1) + col) & 15);
    return (col >> SWSH) & (SWF - 1);
  }
  // 16x16x32 operand reads (M16): a 16-lane read group is NOT sixteen positions with one chunk -- lanes {0-3, 12-15} carry chunk q of
  // their positions and lanes {20-27} (tile positions 4-11) chunk q + 1 (the other group: positions 4-11 with chunk q, 0-3 and 12-15 with
  // q + 1).  Round 2 placed tile positions linearly and measured 41 % (layer 2) and 36 % (layer 4) of all LDS cycles as conflicts, which is
  // what the address model gives (6.67 / 6.22 cycles per read instead of 4).  Both vanish with a permutation of the tile positions over
  // the 16 lanes (scripts/lds_conflicts.py):
  //  GRID 2 x 8 (layer 2): lanes 0-3 and 12-15 own block row 0 (columns 0-3, 4-7), lanes 4-11 block row 1.  Each half group is then eight
  //    consecutive columns of ONE row: its 4 + 4 positions of either bank-row parity take four different column keys, and the row bit of the
  //    key separates the two halves -- 16 different slots under every tap shift.
  //  DENSE (layer 4): lanes 8-11 and 12-15 swap, so positions {0-3, 8-11} / {4-7, 12-15} form the two half groups, and the key of padded
  //    index x is ((x & 7) << 1) | (x >> 3): the two halves of a group then always differ in bit 0 of the key of index pairs (x, x + 8),
  //    which the chunk difference of 1 cannot undo.
  __host__ __device__ static constexpr int dense_key(int x) { return (M16_ && BLK_ == LANES_DENSE) ? (((x & 7) << 1) | (x >> 3)) : x; }
  __host__ __device__ static constexpr int p16_row(int p) { return GR == 2 ? ((p >= 4 && p < 12) ? 1 : 0) : p / GC; }
  __host__ __device__ static constexpr int p16_col(int p) { return GR == 2 ? (p < 4 ? p : (p < 12 ? p - 4 : p - 8)) : p % GC; }
  __host__ __device__ static constexpr int p16_dense(int p) { return p < 8 ? p : (p < 12 ? p + 4 : p - 4); }
  static_assert(!SWZ || (SPP == 4 || SPP == 8 || SPP == 16 || SPP == 32), "swizzled image: 64..512 B per position");
  static constexpr int KS = CB / 32;             // MFMA k-steps (32 B of k) per tap per chunk
  static constexpr int NCH = CIN / CK;           // channel chunks
  static constexpr int KTOT = NCH * 9 * KS;   // k-steps per output-channel tile
  // waves per SIMD the kernel is compiled for (caps the register budget at 512 / OCC): by default two workgroups per
  // CU whenever two halo tiles fit the LDS and the accumulators are small enough
  static constexpr int OCC = OCC_ ? OCC_ : ((MW * NW <= 5 && 160 * 1024 / LDS * WM * WN >= 8) ? 2 : 1);
  static constexpr int NK = 9 * KS;              // k-steps per channel chunk (nine taps)
  static constexpr int KS32 = CB / 64, NK32 = 9 * KS32, KTOT32 = NCH * NK32;   // M16: 32-channel k-steps
  static constexpr int MT16 = 2 * MW, NT16 = 2 * NW;                              // M16: position / output-channel tiles of 16 per wave
  // weight prefetch depth; PD_ names it where the default does not serve, in the k-steps of the shape's MFMA
  static constexpr int PD = PD_ ? PD_ : ((NK * NW <= 24) ? NK : (NW == 1 ? 8 : 4));   // 32x32: k-steps
  static constexpr int PD16 = NK32 * NT16 <= 18 ? NK32 : (PD_ ? PD_ : 2);             // M16: 32-channel steps (two 1-KB fragments each per NW)
  static constexpr bool RESIDENT = NCH == 1 && (M16 ? PD16 == NK32 : PD == NK) && NT == COUT;   // a wave keeps all its weight fragments in registers
  // register-lean epilogue (constants per channel group, shortcut prefetch in two halves).  The two epilogue walks add the statistics form's plane sums in
  // different orders (group-major / tile-major)
  static constexpr bool LEAN = RESIDENT || OCC >= 3;
  static_assert(MT <= WM * MW * 32, "positions must be covered by the waves' 32-row MFMA tiles (trailing tiles may be partial or idle)");
  static constexpr bool PARTIAL_M = MT < WM * MW * 32;   // lanes past the tile compute on a duplicate of the last position and store nothing
  // M16: tile-linear output position of lane position p (0..15) of 16-position tile t of wave row wm; >= MT: none
  __device__ static inline int lane_pos16(int wm, int t, int p) {
    if constexpr (S2G) {
      return t < S2NBC ? (wm * S2GR + s2p_row(p)) * WOUT + t * S2GC + s2p_col(p) : MT;
    } else if constexpr (BLK == LANES_GRID) {
      return ((2 * wm + t / MW) * GR + p16_row(p)) * WOUT + (t % MW) * GC + p16_col(p);
    } else {
      const int L = t * 16 + p16_dense(p), row = L / (WIN + 1), col = L % (WIN + 1);
      return (col < WIN && row < TH) ? row * WOUT + col : MT;
    }
  }
  // tile-linear output position (row * WOUT + col) of lane r (0..31) of M-tile i of wave row wm; >= MT: the lane owns none
  __device__ static inline int lane_pos(int wm, int i, int r) {
    if constexpr (BLK == LANES_GRID) {
      const int g = ((r >= 4 && r < 12) || (r >= 16 && r < 20) || r >= 28) ? 1 : 0;   // lanes 4-11, 16-19, 28-31 form the second read group
      const int j = r - (r < 4 ? 0 : (r < 12 ? 4 : (r < 20 ? 8 : (r < 28 ? 12 : 16))));
      return ((2 * wm + g) * GR + j / GC) * WOUT + i * GC + j % GC;
    } else if constexpr (BLK == LANES_DENSE) {
      const int L = i * 32 + r, row = L / (WIN + 1), col = L % (WIN + 1);
      return (col < WIN && row < TH) ? row * WOUT + col : MT;
    } else {
      return (wm * MW + i) * 32 + r;
    }
  }
  static_assert(COUT % NT == 0 && CIN % CK == 0 && CB % 32 == 0, "channel tiling");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

// second launch-bound = waves per SIMD: two workgroups per CU whenever two halo tiles fit the LDS, which caps the
// kernel at 256 registers (VGPR + AGPR) per lane
// FORM selects the epilogue at compile time (the statistics form carries no shortcut registers, the residual form no
// plane sums): 1 statistics (conv1 of a block), 2 residual (conv2 of a block), 3 residual with the layer's
// first-block 1x1 shortcut convolution evaluated in the epilogue
enum { FORM_STATS = 1, FORM_RESID = 2, FORM_RESID_SC = 3 };
template <int F> struct FormTag { static constexpr int value = F; };

template <class C, int FORM>
__global__ __launch_bounds__(C::WM * C::WN * 64, C::OCC)
void conv3x3_kernel(ConvArgs a) {
  using T = typename C::T;
  constexpr bool STATS = FORM == FORM_STATS, RESID = FORM == FORM_RESID, RSC = FORM == FORM_RESID_SC;
  constexpr int NWAVES = C::WM * C::WN, NTHREADS = NWAVES * 64;
  // NT < COUT (layer 4: 128 of 256 output channels per workgroup): the NY workgroups of a work item read the SAME halo tile, so
  // they sit NY x 8 apart in a 1-D grid -- block ids b and b + 8 share an XCD (round-robin dispatch) and start together, which
  // makes the second read of the tile an L2 hit instead of a second trip to HBM (grid.y = 2 moved 1.58 x the algorithmic bytes)
  constexpr int NY = C::COUT / C::NT;
  const int bidx = NY == 1 ? (int)blockIdx.x : (int)(((blockIdx.x >> 3) / NY) * 8 + (blockIdx.x & 7));
  const int nt0 = (NY == 1 ? 0 : (int)((blockIdx.x >> 3) % NY)) * (C::NT / 32);  // first 32-channel output tile of this workgroup
  __shared__ __attribute__((aligned(1024))) unsigned char smem[C::LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int wm = __builtin_amdgcn_readfirstlane(wave / C::WN), wn = __builtin_amdgcn_readfirstlane(wave % C::WN);
  const int tiles = (a.Hout + C::TH - 1) / C::TH;
  // XCD-aware order: blocks are dealt round-robin over the 8 XCDs (bid % 8 shares an L2), so give every XCD a
  // contiguous run of (utterance, row-tile) work items -> vertically adjacent tiles share their halo rows in L2
  // The grid is either one workgroup per work item or (weight-resident shapes, see RESIDENT) as many workgroups as the
  // chip holds at once, each walking every wstride-th item of its XCD's run -- neighbouring workgroups of an XCD are
  // then always on neighbouring tiles.
  const int nwork = a.B * tiles, q8 = nwork >> 3, r8 = nwork & 7, xcd = bidx & 7;
  const int wfirst = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8, wcount = q8 + (xcd < r8 ? 1 : 0);
  const int wstride = (int)(gridDim.x >> 3) + (xcd < (int)(gridDim.x & 7) ? 1 : 0);
  auto stamp = [&](int k) {  // diagnostic build path only (a.stamps == nullptr in the product)
    if (a.stamps && tid == 0) {
      unsigned long long* sp = a.stamps + (size_t)bidx * 8;
      sp[k] = __builtin_amdgcn_s_memtime();
      // slot 7: the workgroup's span on the constant 100 MHz clock (s_memrealtime) -> in-kernel shader clock = cycles / span
      if (k == 0) sp[7] = __builtin_amdgcn_s_memrealtime();
      if (k == 6) sp[7] = __builtin_amdgcn_s_memrealtime() - sp[7];
    }
  };

  // per-lane LDS byte offset of (M-tile i, horizontal tap dw) at k-step 0; the swizzled image folds the column's
  // swizzle into it, and a later k-step ks is then `offset ^ (ks << 5)` instead of `offset + ks * 32`
  int base[C::BLK ? 1 : C::MW][C::SWZ ? 3 : 1];
  // block lane orders: ONE per-lane register per tap (i-independent), M-tile and tap offsets are instruction immediates
  constexpr int NTR = (C::BLK == LANES_GRID && C::GR >= 4) ? 3 : 1;   // distinct row variants of the key
  int tapreg[C::BLK == LANES_GRID ? NTR : 1][3];
  int fixreg = 0;   // GRID without a leading zero position: column -1 of block column 0 is the row's own trailing zero position
  if constexpr (C::BLK == LANES_GRID && C::M16) {
    const int p = lane & 15, q = lane >> 4;
    const int row0 = C::p16_row(p), col0 = C::p16_col(p);    // inside the 16-position block; the block's own offset is an immediate (+ the wave row)
    const int lanebase = (2 * wm * C::GR + row0) * C::RS + col0 * C::CB;
#pragma unroll
    for (int t = 0; t < NTR; ++t)
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) tapreg[t][dw] = lanebase + ((C::swz_key(row0 + t, col0 + dw - 1) ^ q) << 4);
    if constexpr (!C::LEAD) fixreg = col0 == 0 ? C::RS - C::CB : -C::CB;
  } else if constexpr (C::BLK == LANES_GRID) {
    const int g = ((r >= 4 && r < 12) || (r >= 16 && r < 20) || r >= 28) ? 1 : 0;
    const int j = r - (r < 4 ? 0 : (r < 12 ? 4 : (r < 20 ? 8 : (r < 28 ? 12 : 16))));
    const int row0 = (2 * wm + g) * C::GR + j / C::GC, col0 = j % C::GC;
    const int lanebase = row0 * C::RS + col0 * C::CB;
#pragma unroll
    for (int t = 0; t < NTR; ++t)
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) tapreg[t][dw] = lanebase + ((C::swz_key(row0 + t, col0 + dw - 1) ^ h) << 4);
    if constexpr (!C::LEAD) fixreg = col0 == 0 ? C::RS - C::CB : -C::CB;
  }
  int s2x = 0;   // S2G: taps of the third kernel row read the next output row's staged pair -> another row key: one XOR on the address
  // S2G: per-lane byte offset of (tile 0, horizontal tap dw) at k-step 0; tile t adds the immediate t * S2GC * CB (the column part of
  // the key has period S2GC), except that column -1 of tile 0 is the row's zero position (s2bz)
  int s2b[3] = {0, 0, 0}, s2bz = 0;
  if constexpr (C::S2G) {
    const int p = lane & 15, q = lane >> 4;
    const int ho = wm * C::S2GR + C::s2p_row(p), pcol = C::s2p_col(p);
    s2x = (C::s2_rowkey(2 * ho) ^ C::s2_rowkey(2 * ho + 2)) << 4;
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      const int P = dw == 1 ? pcol : C::WIN / 2 + pcol - (dw == 0 ? 1 : 0);   // even plane / odd plane (dw = 0: one position to the left)
      s2b[dw] = (2 * ho) * C::RS + P * C::CB + ((q ^ C::swz_key(2 * ho, P)) << 4);
    }
    const int Pz = pcol == 0 ? C::WIN : C::WIN / 2 + pcol - 1;
    s2bz = (2 * ho) * C::RS + Pz * C::CB + ((q ^ C::swz_key(2 * ho, Pz)) << 4);
  }
#pragma unroll
  for (int i = 0; i < ((C::BLK || C::S2G) ? 0 : C::MW); ++i) {
    const int mraw = (wm * C::MW + i) * 32 + r, m = (C::PARTIAL_M && mraw >= C::MT) ? C::MT - 1 : mraw;
    const int ho = m / C::WOUT, wo = m % C::WOUT;
    if constexpr (C::SWZ) {
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        int col = wo * C::S + dw - 1;
        if (col < 0) col = C::WIN;            // column -1 and column WIN are both the row's trailing zero position
        const int f = (col >> C::SWSH) & (C::SWF - 1);
        base[i][dw] = (ho * C::S) * C::RS + col * C::CB + ((h ^ f) << 4);
      }
    } else {
      base[i][0] = (ho * C::S) * C::RS + (wo * C::S) * C::PSTRIDE + h * 16;
    }
  }
  // Output-channel tile of (wave column wn, repeat j) = j*WN + wn: for a fixed j the workgroup's WN*32 channels are
  // contiguous, so the staged out tile leaves as contiguous NHWC rows.  Fragment address = wave-uniform (SGPR)
  // offset + 32-bit lane offset, so no per-fragment 64-bit VGPR address is kept alive.
  const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.wpack);
  const unsigned lane16 = (unsigned)lane * 16u;
  auto wload = [&](int j, int kidx) {
    const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(((nt0 + j * C::WN + wn) * C::KTOT + kidx) * 1024);
    return *reinterpret_cast<const uint4*>(wbase + soff + lane16);
  };
  const unsigned char* in = reinterpret_cast<const unsigned char*>(a.in);

  // Weight fragments stream L2 -> VGPR through a small software ring: PD k-steps ahead of their use, so the ~700-cycle
  // L2 latency is paid once per chunk, under the staging DMA.  When ALL of a wave's fragments fit the ring (C = 32
  // inputs: 72 registers) they are loaded once per workgroup and the workgroup is persistent: per tile that removes
  // 72 KB of L2->VGPR traffic from a vector-memory path that also has to carry the tile's 50 KB of DMA and its stores.
  constexpr int NK = C::NK, PD = C::PD;
  constexpr bool RESIDENT = C::RESIDENT;
  // packed-weight index (tap * KS + ks) of the kk-th k-step of a chunk (see the k-step order below)
  auto kord = [](int kk) {
    return (C::SWZ && !C::BLK) ? ((kk % 3) * 3 + kk / (3 * C::KS)) * C::KS + (kk / 3) % C::KS : kk;
  };
  uint4 wq[C::M16 ? 1 : PD][C::NW];
  // M16: fragments of 16 output channels x 32 input channels; a wave's 32-channel tile j is the pair of 16-channel tiles 2j, 2j + 1
  constexpr int PD16 = C::PD16, NK32 = C::NK32;
  uint4 wq16[C::M16 ? PD16 : 1][C::M16 ? C::NT16 : 1];
  auto wload16 = [&](int jn, int kidx32) {
    const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(((2 * (nt0 + (jn >> 1) * C::WN + wn) + (jn & 1)) * C::KTOT32 + kidx32) * 1024);
    return *reinterpret_cast<const uint4*>(wbase + soff + lane16);
  };
  auto load_weights = [&](int ch) {
    if constexpr (C::M16) {
#pragma unroll
      for (int d = 0; d < PD16; ++d)
#pragma unroll
        for (int jn = 0; jn < C::NT16; ++jn) wq16[d][jn] = wload16(jn, ch * NK32 + d);
      return;
    }
#pragma unroll
    for (int d = 0; d < PD; ++d)
#pragma unroll
      for (int j = 0; j < C::NW; ++j) wq[d][j] = wload(j, ch * NK + kord(d));
  };
  if constexpr (RESIDENT) load_weights(0);

  const int tid0 = tid;
  auto do_item = [&](int work, bool first_item) -> bool {  // returns whether the tile touched the LDS
  // persistent form: hide the thread index from loop-invariant code motion -- hoisting every tile-independent DMA and
  // copy-out offset out of the tile loop costs ~40 registers (spills); recomputing them per tile is a few VALU ops
  int tid = tid0;
  if constexpr (RESIDENT) asm volatile("" : "+v"(tid));
  const int lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int b = work / tiles, tile = work % tiles;
  const int ho0 = tile * C::TH;
  const int hin_b = halve(a.lens.get_uniform(b), a.halvings_in);  // scalar load: the row bounds live in SGPRs and the tile does not wait for the previous tile's stores
  const int hout_b = (C::S == 2) ? ((hin_b + 1) >> 1) : hin_b;
  if (ho0 >= hout_b) return false;  // nothing valid in this tile (its SE partial is never read)
  if (!first_item) __syncthreads();  // the previous tile's copy-out has left the LDS
  stamp(0);
  const int hi0 = ho0 * C::S - 1;
  f32x16 acc[C::MW][C::NW];
#pragma unroll
  for (int i = 0; i < C::MW; ++i)
#pragma unroll
    for (int j = 0; j < C::NW; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  for (int ch = 0; ch < C::NCH; ++ch) {
    if constexpr (!RESIDENT) load_weights(ch);
    __builtin_amdgcn_sched_barrier(0);  // keep the loads up here: the scheduler otherwise sinks them next to their use
    if (ch) __syncthreads();
    // stage the halo tile with LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B land on 1 KiB of LDS, no VGPRs,
    // every piece in flight at once).  A lane whose slot is a pad slot or a zero-padding position reads the zero page
    // (measured: masking those lanes off and zero-filling with ds_write instead is 20 % slower).
    constexpr int CPP = C::CB / 16, NPIECE = C::RIN * C::PPR;
    if constexpr (C::SWZ) {
      if (ch == 0) {  // the zero position after each row: never touched by the DMA, valid for every channel chunk
        for (int s = tid; s < C::RIN * C::SPP; s += NTHREADS)
          *reinterpret_cast<uint4*>(smem + C::IMG0 + (s / C::SPP) * C::RS + C::WIN * C::CB + (s % C::SPP) * 16) = make_uint4(0, 0, 0, 0);
        if constexpr (C::LEAD) {  // the position in front of the image: column -1 of staged row 0
          if (tid < C::SPP) *reinterpret_cast<uint4*>(smem + tid * 16) = make_uint4(0, 0, 0, 0);
        }
      }
    }
    for (int it = (a.dbg & 4) ? NPIECE : wave; it < NPIECE; it += NWAVES) {
      const int row = it / C::PPR, q = it % C::PPR;          // wave-uniform
      const int hi = hi0 + row;
      const bool rowok = hi >= 0 && hi < hin_b;
      const unsigned char* rowbase = in + ((((size_t)b * a.Hin + hi) * C::WIN) * C::CIN + ch * C::CK) * C::EB;
      const int slot = q * 64 + lane;
      const unsigned char* src = reinterpret_cast<const unsigned char*>(a.zeros);
      if constexpr (C::SWZ) {
        const int col = slot / C::SPP, cs = slot % C::SPP;     // staged position, slot inside it
        const int cc = cs ^ C::swz_key(row, col);
        if (rowok) src = rowbase + (C::S2G ? C::unplanar(col) : col) * (C::CIN * C::EB) + cc * 16;
        if ((C::WIN * C::SPP) % 64 == 0 || slot < C::WIN * C::SPP)  // a partial last piece must not run into the next row
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)(smem + C::IMG0 + row * C::RS + q * 1024), 16, 0, 0);
      } else {
        const int col = slot / C::SPP, cc = slot - col * C::SPP;
        if (rowok && cc < CPP && col >= 1 && col <= C::WIN) src = rowbase + (col - 1) * (C::CIN * C::EB) + cc * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(smem + it * 1024), 16, 0, 0);
      }
    }
    stamp(1);
    __syncthreads();
    stamp(2);
    __builtin_amdgcn_s_setprio(0);
    // k-step order inside a chunk: (tap, ks) for the padded image; the swizzled image walks (dw, ks, dh) so that one
    // swizzled address serves three consecutive steps (the row offset is an instruction immediate) and then dies
    auto step_tap = [](int kk) { return (C::SWZ && !C::BLK) ? (kk % 3) * 3 + kk / (3 * C::KS) : kk / C::KS; };
    auto step_ks = [](int kk) { return (C::SWZ && !C::BLK) ? (kk / 3) % C::KS : kk % C::KS; };
    int rl = r;
    if constexpr (C::BLK == LANES_DENSE) asm volatile("" : "+v"(rl));
    auto xaddr = [&](int i, int kk) {
      const int tap = step_tap(kk), ks = step_ks(kk);
      if constexpr (C::BLK != LANES_LINEAR) {
        const int dh = tap / 3, dw = tap % 3;
        if constexpr (C::BLK == LANES_DENSE) {
          // lane L reads position L + delta(tap) of the padded image, key = (L + delta) & 15: three VALU operations per tap (k-steps
          // walk tap-major), from a lane index re-read per channel chunk so that the nine values are not kept live as loop invariants
          const int v = (rl * C::CB + ((((rl + dh * (C::WIN + 1) + dw - 1) & 15) ^ h) << 4)) ^ (ks << 5);
          return smem + v + (32 * i + dh * (C::WIN + 1) + dw) * C::CB;   // IMG0 = CB: + 1 position
        } else {
          // GR == 2: the row bit of the key flips with dh for every lane alike -> part of the compile-time XOR constant
          const int v = tapreg[NTR == 3 ? dh : 0][dw] ^ ((ks << 5) ^ ((C::GR == 2 && (dh & 1)) ? (16 << C::KRSH) : 0));
          if (!C::LEAD && dw == 0 && i == 0) return smem + (v + fixreg) + dh * C::RS;
          return smem + v + (C::IMG0 + (i * C::GC + dw - 1) * C::CB + dh * C::RS);
        }
      } else if constexpr (C::SWZ) return smem + (base[i][tap % 3] ^ (ks << 5)) + (tap / 3) * C::RS;
      else return smem + base[i][0] + (tap / 3) * C::RS + (tap % 3) * C::PSTRIDE + ks * 32;
    };
    if constexpr (C::M16) {
      // 16x16x32 k-loop: step kk = (tap, s) covers 32 channels; position tile t reads ONE fragment that feeds the wave's NT16
      // output-channel tiles.  Lane part of the address: one register per tap (GRID) or three VALU operations per tap (DENSE),
      // XORed with the k-step; tile and tap offsets are immediates.
      typedef float f32x4v __attribute__((ext_vector_type(4)));
      const int q16 = lane >> 4;
      int pl = C::BLK == LANES_DENSE ? C::p16_dense(lane & 15) : (lane & 15);
      if constexpr (C::BLK == LANES_DENSE) asm volatile("" : "+v"(pl));
      auto xaddr16 = [&](int t, int kk) {
        const int tap = kk / C::KS32, sk = kk % C::KS32, dh = tap / 3, dw = tap % 3;
        if constexpr (C::S2G) {
          const int tt = t < C::PT16 ? t : C::PT16 - 1;   // the idle sixth tile slot re-reads the last tile (never multiplied)
          const int v = ((dw == 0 && tt == 0) ? s2bz : s2b[dw]) ^ ((sk << 6) ^ (dh == 2 ? s2x : 0));
          return smem + v + (tt * C::S2GC * C::CB + dh * C::RS);
        } else if constexpr (C::BLK == LANES_DENSE) {
          const int v = (pl * C::CB + ((C::dense_key((pl + dh * (C::WIN + 1) + dw - 1) & 15) ^ q16) << 4)) ^ (sk << 6);
          return smem + v + (16 * t + dh * (C::WIN + 1) + dw) * C::CB;   // IMG0 = CB: + 1 position
        } else {
          const int v = tapreg[NTR == 3 ? dh : 0][dw] ^ ((sk << 6) ^ ((C::GR == 2 && (dh & 1)) ? (16 << C::KRSH) : 0));
          const int brow = (t / C::MW) * C::GR, bcol = (t % C::MW) * C::GC;   // block origin inside the wave's two block rows
          if (!C::LEAD && dw == 0 && bcol == 0) return smem + (v + fixreg) + (brow + dh) * C::RS;
          return smem + v + (C::IMG0 + (bcol + dw - 1) * C::CB + (brow + dh) * C::RS);
        }
      };
      // the position tiles of a k-step are walked in two halves so that only MW fragments are live (registers: 3 workgroups per CU)
      constexpr int HT = C::MW;
      uint4 x16[HT];
#pragma unroll
      for (int t = 0; t < HT; ++t) x16[t] = *reinterpret_cast<const uint4*>(xaddr16(t, 0));
      if (!(a.dbg & 2))
#pragma unroll
      for (int u = 0; u < 2 * NK32; ++u) {
        const int kk = u >> 1, t0 = (u & 1) * HT;
        uint4 wf[C::NT16];
#pragma unroll
        for (int jn = 0; jn < C::NT16; ++jn) wf[jn] = wq16[kk % PD16][jn];
        if ((u & 1) && kk + PD16 < NK32) {   // the ring slot is free once the step's second half has its fragments.  (Round 3 measured this refill at 9-10 % of layers 2 / 3 by
                                             // switching it off at run time -- and the switch itself, a condition around the loads, cost layers 3 / 4 another 5 %: it is gone.)
#pragma unroll
          for (int jn = 0; jn < C::NT16; ++jn) wq16[kk % PD16][jn] = wload16(jn, ch * NK32 + kk + PD16);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < HT; ++t)      // (round 5: the other order -- one weight fragment held over HT consecutive MFMAs -- is no cheaper for the power-limited
#pragma unroll                            //  chip: layers 3 / 4 1.406 / 0.693 vs 1.397 / 0.681 ms per step, profiles/r05_ab_mfma_issue_order.txt)
          for (int jn = 0; jn < C::NT16; ++jn) {
            if (t0 + t >= C::PT16) continue;   // S2G: five tiles in six slots
            // accumulator of (position tile t, channel tile jn) = quarter 2 * (t & 1) + (jn & 1) of acc[t / 2][jn / 2]
            f32x16& A = acc[(t0 + t) >> 1][jn >> 1];
            const int q0 = 4 * (2 * ((t0 + t) & 1) + (jn & 1));
            f32x4v part = {A[q0], A[q0 + 1], A[q0 + 2], A[q0 + 3]};
            part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[jn]), __builtin_bit_cast(bf16x8, x16[t]), part, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) A[q0 + e] = part[e];
          }
        if (u + 1 < 2 * NK32) {
#pragma unroll
          for (int t = 0; t < HT; ++t) x16[t] = *reinterpret_cast<const uint4*>(xaddr16(((u + 1) & 1) * HT + t, (u + 1) >> 1));
        }
      }
      continue;
    }
    uint4 xc[C::MW], xn[C::MW];
#pragma unroll
    for (int i = 0; i < C::MW; ++i) xc[i] = *reinterpret_cast<const uint4*>(xaddr(i, 0));
    if (!(a.dbg & 2))
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
      if (kk + 1 < NK && C::OCC < 3) {  // the next k-step's activation fragments are read while this step's MFMAs run
#pragma unroll                           // (three waves per SIMD hide the LDS latency themselves and have no registers for it)
        for (int i = 0; i < C::MW; ++i) xn[i] = *reinterpret_cast<const uint4*>(xaddr(i, kk + 1));
      }
      uint4 wf[C::NW];
#pragma unroll
      for (int j = 0; j < C::NW; ++j) wf[j] = wq[kk % PD][j];
      if (kk + PD < NK) {
#pragma unroll
        for (int j = 0; j < C::NW; ++j) wq[kk % PD][j] = wload(j, ch * NK + kord(kk + PD));
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < C::MW; ++i)
#pragma unroll
        for (int j = 0; j < C::NW; ++j) mma_step<T>(acc[i][j], wf[j], xc[i]);
      if (kk + 1 < NK) {
#pragma unroll
        for (int i = 0; i < C::MW; ++i) {
          if constexpr (C::OCC < 3) xc[i] = xn[i];
          else xc[i] = *reinterpret_cast<const uint4*>(xaddr(i, kk + 1));
        }
      }
    }
  }

  // ---- epilogue: BN scale/shift, then the kernel's form:
  //   statistics (+ReLU, conv1 of a block)     -> store + the sums the SE gate of the block is derived from
  //   residual   (conv2 of a block)            -> * gate[b][c] + shortcut -> ReLU -> store
  // The tile is transposed through the (now consumed) LDS halo buffer and leaves as whole 1-KiB, 16-B-per-lane NHWC
  // rows (direct 8-B stores ran at 2.9 TB/s); the shortcut rows are read the same way in the residual form.
  constexpr int NC = C::WN * 32;                // channels of one out sub-tile
  constexpr int OPS = NC * C::EB + 16;          // out-tile position stride in LDS (padded against bank conflicts)
  static_assert(C::MT * OPS <= C::LDS, "out tile must fit the consumed input buffer");
  // memory phases (epilogue, stores, next tile's DMA) ahead of other workgroups' MFMAs.  The test is always true (nothing sets bit 7 of dbg);
  // it stays because the branch ends a scheduling region: without it seven kernels change registers and layer 1's in-place-shortcut form spills
  if (!(a.dbg & 128)) __builtin_amdgcn_s_setprio(3);
  const int mvalid = (hout_b - ho0) * C::WOUT < C::MT ? (hout_b - ho0) * C::WOUT : C::MT;
  const size_t gpos0 = ((size_t)b * a.Hout + ho0) * C::WOUT;
  auto lds_elem = [&](int m, int c) {
    if constexpr (C::EB == 2) return bf16_to_f32(*reinterpret_cast<const uint16_t*>(smem + m * OPS + c * 2));
    else return *reinterpret_cast<const float*>(smem + m * OPS + c * 4);
  };
  stamp(3);
  // The epilogue is a lambda called once, below, and its body is written at the level of do_item.  It is kept as one on purpose: written
  // inline (with or without these four values as locals) the same statements compile to another schedule and register allocation in
  // every kernel of the file ("what the trunk convolution no longer carries").
  auto emit = [&](auto& accv, const float* scale, const float* shift, unsigned char* out) {
  const float* gate = (RESID || RSC) ? a.gate : nullptr;
  float* se_part = STATS ? a.se_part : nullptr;
#pragma unroll
  for (int j = 0; j < C::NW; ++j) {
    const int nbase = (nt0 + j * C::WN + wn) * 32;
    // residual form: this thread's shortcut chunks are fetched now and consumed after the out tile is staged
    constexpr int CPR = NC * C::EB / 16;             // 16-B chunks per position
    constexpr int NIT = (C::MT * CPR + NTHREADS - 1) / NTHREADS;   // copy-out iterations per thread
    const unsigned char* scut = reinterpret_cast<const unsigned char*>(a.shortcut);
    // persistent shapes keep 72 registers of weights alive through the epilogue: only the first half of the shortcut
    // chunks is fetched ahead of the epilogue arithmetic, the second half once the accumulators are dead
    constexpr int NPRE = (RESID && C::LEAN) ? (NIT + 1) / 2 : NIT;
    uint4 sreg[RESID ? NIT : 1];
    // NC == COUT (every product shape but layer 4's two half-channel workgroups): the tile's rows are one contiguous run of the tensor, chunk
    // idx sits idx * 16 bytes into it -> wave-uniform base + 32-bit lane offset instead of a 64-bit address per chunk
    constexpr bool ROWRUN = NC == C::COUT;
    const size_t run0 = gpos0 * C::COUT * C::EB;
    auto fetch_shortcut = [&](int q) {
      const int idx = tid + q * NTHREADS, m = idx / CPR, cc = idx % CPR;
      if constexpr (ROWRUN) return (idx < mvalid * CPR) ? *reinterpret_cast<const uint4*>(scut + run0 + (unsigned)idx * 16u) : make_uint4(0, 0, 0, 0);
      return (idx < mvalid * CPR) ? *reinterpret_cast<const uint4*>(scut + ((gpos0 + m) * C::COUT + nt0 * 32 + j * NC) * C::EB + cc * 16)
                                  : make_uint4(0, 0, 0, 0);
    };
    if constexpr (RESID) {
#pragma unroll
      for (int q = 0; q < NPRE; ++q) sreg[q] = fetch_shortcut(q);
    }
    __syncthreads();  // every wave is done with the halo tile (j == 0) / the previous sub-tile has been copied out; the shortcut loads above are on their way while the wave waits here
    // The 16 accumulator registers of (M-tile i, channel tile j) are four groups g of 4 consecutive output channels:
    //   32x32 MFMA: position lane_pos(i, r), channels 8 g + 4 h .. + 3 of the 32-channel tile;
    //   M16       : quarter g = 2 * (position-tile half) + (channel-tile half): position lane_pos16(2 i + (g >> 1), l & 15),
    //               channels 16 (g & 1) + 4 (l >> 4) .. + 3.
    const int p16 = lane & 15, q16 = lane >> 4;
    auto pos_of = [&](int i, int g) { return C::M16 ? C::lane_pos16(wm, 2 * i + (g >> 1), p16) : C::lane_pos(wm, i, r); };
    auto coff = [&](int g) { return C::M16 ? 16 * (g & 1) + 4 * q16 : 8 * g + 4 * h; };
    constexpr int NSUM = C::M16 ? 8 : 16;            // per-lane channel sums of the statistics form
    auto sidx = [](int g) { return C::M16 ? 4 * (g & 1) : 4 * g; };
    float* sp = nullptr;
    if constexpr (STATS) sp = se_part + (((size_t)b * tiles + tile) * C::WM + wm) * C::COUT + nbase;
    float ssum[STATS ? NSUM : 1];
    if constexpr (STATS) {
#pragma unroll
      for (int q = 0; q < NSUM; ++q) ssum[q] = 0.f;
    }
    auto ld4 = [&](const float* p, int g) { return *reinterpret_cast<const f32x4*>(p + nbase + coff(g)); };
    const float* gate_b = (RESID || RSC) ? gate + (size_t)b * C::COUT : scale;
    // one (M-tile i, channel group g) cell: 4 values -> BN, gate or ReLU, rounding, plane sums, 8/16 B into the out tile
    auto cell = [&](int i, int g, const f32x4& sc, const f32x4& sh, const f32x4& gt, auto full_tag) {
      const int m = pos_of(i, g);
      const bool valid = decltype(full_tag)::value || m < mvalid;   // mvalid <= MT; full tiles (all but an utterance's last) carry no per-value select
      unsigned char* lp = smem + m * OPS + (wn * 32 + coff(g)) * C::EB;
      const bool store = !C::PARTIAL_M || m < C::MT;
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x = fmaf(accv[i][j][4 * g + q], sc[q], sh[q]);   // one rounding (the file is built with -ffp-contract=off); residual form: sc, sh carry the gate
        if constexpr (STATS) x = relu_nan(x);   // conv1 + bn1 + ReLU of a block; the residual form applies its ReLU after the shortcut, at the copy-out
        v[q] = x;
      }
      if constexpr (C::EB == 2) {
        const uint32_t u01 = pack_bf16x2(v[0], v[1]), u23 = pack_bf16x2(v[2], v[3]);   // what is stored (and what the next conv reads)
        if constexpr (STATS) {   // the plane sums are those of the stored values: widen the packed halves back (one shift / mask each) instead of rounding twice
          const float r[4] = {__builtin_bit_cast(float, u01 << 16), __builtin_bit_cast(float, u01 & 0xffff0000u),
                              __builtin_bit_cast(float, u23 << 16), __builtin_bit_cast(float, u23 & 0xffff0000u)};
#pragma unroll
          for (int q = 0; q < 4; ++q) ssum[sidx(g) + q] += valid ? r[q] : 0.f;
        }
        if (store) *reinterpret_cast<uint2*>(lp) = make_uint2(u01, u23);
      } else {
        if constexpr (STATS) {
#pragma unroll
          for (int q = 0; q < 4; ++q) ssum[sidx(g) + q] += valid ? v[q] : 0.f;
        }
        if (store) *reinterpret_cast<float4*>(lp) = make_float4(v[0], v[1], v[2], v[3]);
      }
    };
    if constexpr (RSC) {
      // first block of a layer: x = bn2(conv2) * gate + bn_s(conv1x1_s(block input)); the 1x1 conv runs here on the
      // matrix cores with the block input's rows as the position operand, read straight from global memory (a lane's
      // fragment is 16 B of its own position, exactly the layout the halo tile has in LDS)
      constexpr int SS = C::COUT == 32 ? 1 : 2, CX = C::COUT == 32 ? 32 : C::COUT / 2;   // the trunk's shortcut geometry
      constexpr int KX = CX * C::EB / 32;                                               // k-steps of the 1x1
      const unsigned char* xin = reinterpret_cast<const unsigned char*>(a.sc_in);
      const unsigned char* scb = reinterpret_cast<const unsigned char*>(a.sc_wpack);
      constexpr int KX16 = C::M16 ? CX * C::EB / 64 : 1;                                  // M16: 32-channel k-steps of the 1x1
      uint4 wx[C::M16 ? 1 : KX];
      uint4 wx16[C::M16 ? 2 : 1][KX16];
      if constexpr (C::M16) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int sk = 0; sk < KX16; ++sk) {
            const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(((2 * (nt0 + j * C::WN + wn) + n) * KX16 + sk) * 1024);
            wx16[n][sk] = *reinterpret_cast<const uint4*>(scb + soff + (unsigned)lane * 16u);
          }
      } else {
#pragma unroll
        for (int ks = 0; ks < KX; ++ks) {
          const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(((nt0 + j * C::WN + wn) * KX + ks) * 1024);
          wx[ks] = *reinterpret_cast<const uint4*>(scb + soff + (unsigned)lane * 16u);
        }
      }
      // x = (bn2(conv2) * gate) + bn_s(conv1x1(x_in)) = k1 * acc + [scale_s folded into the 1x1 weights] + k0 with
      // k1 = scale2 * gate, k0 = shift2 * gate + shift_s: scale the accumulators, let the 1x1's MFMAs accumulate into
      // them, add k0.  Constants are taken one channel group at a time (4 registers each), so the form fits the
      // product configurations (168 registers at three workgroups per CU, resident weights in the persistent ones).
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sc = ld4(scale, g), gt = ld4(gate_b, g);
#pragma unroll
        for (int i = 0; i < C::MW; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) accv[i][j][4 * g + q] *= sc[q] * gt[q];
      }
      if constexpr (C::M16) {
        typedef float f32x4v __attribute__((ext_vector_type(4)));
        auto xload16 = [&](int t, uint4* dst) {   // block-input row of this lane's position: chunk q16 of every 32-channel step
          const int m = C::lane_pos16(wm, t, p16);
          const int ho = m / C::WOUT, wo = m % C::WOUT;
          const unsigned char* xp = xin + ((((size_t)b * a.sc_hin + (size_t)(ho0 + ho) * SS) * (C::WOUT * SS) + wo * SS) * CX) * C::EB + q16 * 16;
#pragma unroll
          for (int sk = 0; sk < KX16; ++sk) dst[sk] = (m < mvalid) ? *reinterpret_cast<const uint4*>(xp + sk * 64) : make_uint4(0, 0, 0, 0);
        };
        uint4 xf[KX16], xn[KX16];
        xload16(0, xf);
#pragma unroll
        for (int t = 0; t < C::MT16; ++t) {
          if (t + 1 < C::MT16) xload16(t + 1, xn);
#pragma unroll
          for (int sk = 0; sk < KX16; ++sk)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              f32x16& A = accv[t >> 1][j];
              const int q0 = 4 * (2 * (t & 1) + n);
              f32x4v part = {A[q0], A[q0 + 1], A[q0 + 2], A[q0 + 3]};
              part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wx16[n][sk]), __builtin_bit_cast(bf16x8, xf[sk]), part, 0, 0, 0);
#pragma unroll
              for (int e = 0; e < 4; ++e) A[q0 + e] = part[e];
            }
#pragma unroll
          for (int sk = 0; sk < KX16; ++sk) xf[sk] = xn[sk];
        }
      }
      constexpr bool AHEAD = KX <= 4;   // block-input fragments one M-tile ahead of their use
      auto xload = [&](int i, uint4* dst) {
        const int m = C::lane_pos(wm, i, r);
        const int ho = m / C::WOUT, wo = m % C::WOUT;
        const unsigned char* xp = xin + ((((size_t)b * a.sc_hin + (size_t)(ho0 + ho) * SS) * (C::WOUT * SS) + wo * SS) * CX) * C::EB + h * 16;
#pragma unroll
        for (int ks = 0; ks < KX; ++ks) dst[ks] = (m < mvalid) ? *reinterpret_cast<const uint4*>(xp + ks * 32) : make_uint4(0, 0, 0, 0);
      };
      if constexpr (!C::M16) {
      uint4 xf[KX], xn[AHEAD ? KX : 1];
      xload(0, xf);
#pragma unroll
      for (int i = 0; i < C::MW; ++i) {
        if constexpr (AHEAD) { if (i + 1 < C::MW) xload(i + 1, xn); }
#pragma unroll
        for (int ks = 0; ks < KX; ++ks) mma_step<T>(accv[i][j], wx[ks], xf[ks]);
        if (i + 1 < C::MW) {
          if constexpr (AHEAD) {
#pragma unroll
            for (int ks = 0; ks < KX; ++ks) xf[ks] = xn[ks];
          } else {
            xload(i + 1, xf);
          }
        }
      }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sh = ld4(shift, g), gt = ld4(gate_b, g), h2 = ld4(a.sc_shift, g);
#pragma unroll
        for (int i = 0; i < C::MW; ++i) {
          const int m = pos_of(i, g);
          unsigned char* lp = smem + m * OPS + (wn * 32 + coff(g)) * C::EB;
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = relu_nan(accv[i][j][4 * g + q] + (sh[q] * gt[q] + h2[q]));
          if (!C::PARTIAL_M || m < C::MT) {
            if constexpr (C::EB == 2) *reinterpret_cast<uint2*>(lp) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
            else *reinterpret_cast<float4*>(lp) = make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
    } else if constexpr (C::LEAN) {
      // persistent shapes (72 registers of weights stay live) and the three-workgroups-per-CU shapes (168 registers): one channel group at a time, the next group's
      // constants in flight while this one is processed -> 24 instead of 48 registers of constants
      f32x4 sc_n = ld4(scale, 0), sh_n = ld4(shift, 0), gt_n = ld4(gate_b, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sc = sc_n, sh = sh_n, gt = gt_n;
        if (g + 1 < 4) {
          sc_n = ld4(scale, g + 1);
          sh_n = ld4(shift, g + 1);
          if constexpr (RESID) gt_n = ld4(gate_b, g + 1);
        }
        f32x4 sck = sc, shk = sh;
        if constexpr (RESID) {   // (acc * scale + shift) * gate = acc * (scale * gate) + shift * gate: two products per channel instead of one per value
#pragma unroll
          for (int q = 0; q < 4; ++q) { sck[q] = sc[q] * gt[q]; shk[q] = sh[q] * gt[q]; }
        }
        if (STATS && !C::PARTIAL_M && mvalid == C::MT) {   // wave-uniform
#pragma unroll
          for (int i = 0; i < C::MW; ++i) cell(i, g, sck, shk, gt, FormTag<1>{});
        } else {
#pragma unroll
          for (int i = 0; i < C::MW; ++i) cell(i, g, sck, shk, gt, FormTag<0>{});
        }
      }
    } else {
      f32x4 sc[4], sh[4], gt[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        sc[g] = ld4(scale, g);
        sh[g] = ld4(shift, g);
        gt[g] = RESID ? ld4(gate_b, g) : sc[g];
        if constexpr (RESID) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { sc[g][q] *= gt[g][q]; sh[g][q] *= gt[g][q]; }
        }
      }
#pragma unroll
      for (int i = 0; i < C::MW; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) cell(i, g, sc[g], sh[g], gt[g], FormTag<0>{});
    }
    if constexpr (STATS && C::M16) {  // a lane's 8 sums belong to its 16-lane row (one row per 4 output channels of each 16-channel tile)
#pragma unroll
      for (int q = 0; q < 8; ++q) ssum[q] = row_sum16(ssum[q]);
      if (p16 == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
          *reinterpret_cast<float4*>(sp + 16 * n + 4 * q16) = make_float4(ssum[4 * n], ssum[4 * n + 1], ssum[4 * n + 2], ssum[4 * n + 3]);
      }
    } else if constexpr (STATS) {  // sixteen independent DPP reductions after the arithmetic (per-group chains serialised it)
#pragma unroll
      for (int q = 0; q < 16; ++q) ssum[q] = half_sum_upper_row(ssum[q]);
      if (r == 16) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(sp + 4 * h + 8 * g) = make_float4(ssum[4 * g], ssum[4 * g + 1], ssum[4 * g + 2], ssum[4 * g + 3]);
      }
    }
    if constexpr (RESID && NPRE < NIT) {  // accumulators are dead: the second half of the shortcut rides out the barrier
#pragma unroll
      for (int q = NPRE; q < NIT; ++q) sreg[q] = fetch_shortcut(q);
    }
    if (j == 0) stamp(4);
    __syncthreads();  // out sub-tile complete
    if (j == 0) stamp(5);
    if (STATS && tid < 2 * NC) {
      // edge sums for the next conv's zero padding: a tap shifted by (dh, dw) misses one border row and/or column.  Threads [0, NC) take
      // the first column / first row, threads [NC, 2 NC) the last column / last row (round 4: one thread per channel walked both chains
      // of dependent LDS reads while the rest of the workgroup waited for it at the next tile's barrier); each sum keeps its order
      const int side = tid >= NC ? 1 : 0;
      const int c = tid - side * NC, cg = nt0 * 32 + j * NC + c, rows_valid = mvalid / C::WOUT, hl = hout_b - 1;
      const int wcol = side ? C::WOUT - 1 : 0;
      float cs = 0.f;
      for (int hr = 0; hr < rows_valid; ++hr) cs += lds_elem(hr * C::WOUT + wcol, c);
      a.col_part[((size_t)b * tiles + tile) * 2 * C::COUT + side * C::COUT + cg] = cs;
      float* eg = a.edge + (size_t)b * 6 * C::COUT + cg;
      if (tile == 0) {   // first row: its sum (side 0) and its two corners
        if (side == 0) {
          float s = 0.f;
          for (int wo = 0; wo < C::WOUT; ++wo) s += lds_elem(wo, c);
          eg[0] = s;
          eg[2 * C::COUT] = lds_elem(0, c);
        } else {
          eg[3 * C::COUT] = lds_elem(C::WOUT - 1, c);
        }
      }
      if (tile == hl / C::TH) {   // last row: its sum (side 1) and its two corners
        const int m0 = (hl - ho0) * C::WOUT;
        if (side == 1) {
          float s = 0.f;
          for (int wo = 0; wo < C::WOUT; ++wo) s += lds_elem(m0 + wo, c);
          eg[1 * C::COUT] = s;
          eg[5 * C::COUT] = lds_elem(m0 + C::WOUT - 1, c);
        } else {
          eg[4 * C::COUT] = lds_elem(m0, c);
        }
      }
    }
    if (!(a.dbg & 1)) {
      // chunk idx = tid + q * NTHREADS of the tile: position m = idx / CPR, 16-B piece cc = idx % CPR.  With NTHREADS a multiple of CPR the
      // lane part (tid / CPR, tid % CPR) is computed once and a step of q is a constant LDS offset (the compiler does not see that through the
      // signed divisions: seven address instructions per chunk)
      static_assert(NTHREADS % CPR == 0, "copy-out: whole positions per round");
      const unsigned lane_lds = ((unsigned)tid / CPR) * OPS + ((unsigned)tid % CPR) * 16;
#pragma unroll
      for (int q = 0; q < NIT; ++q) {
        const int idx = tid + q * NTHREADS, m = idx / CPR, cc = idx % CPR;
        if (idx >= mvalid * CPR) break;
        uint4 v = *reinterpret_cast<const uint4*>(smem + lane_lds + q * (NTHREADS / CPR) * OPS);
        if constexpr (RESID) {
          const uint4 s = sreg[q];
          if constexpr (C::EB == 2) {
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w}, ss[4] = {s.x, s.y, s.z, s.w};
            uint32_t rr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)   // bf16 halves widened with ONE instruction each (shift for the low half, mask for the high one)
              rr[e] = pack_bf16x2(relu_nan(__builtin_bit_cast(float, vv[e] << 16) + __builtin_bit_cast(float, ss[e] << 16)),
                                  relu_nan(__builtin_bit_cast(float, vv[e] & 0xffff0000u) + __builtin_bit_cast(float, ss[e] & 0xffff0000u)));
            v = make_uint4(rr[0], rr[1], rr[2], rr[3]);
          } else {
            const float4 vf = __builtin_bit_cast(float4, v), sf = __builtin_bit_cast(float4, s);
            v = __builtin_bit_cast(uint4, make_float4(relu_nan(vf.x + sf.x), relu_nan(vf.y + sf.y), relu_nan(vf.z + sf.z), relu_nan(vf.w + sf.w)));
          }
        }
        if constexpr (ROWRUN) *reinterpret_cast<uint4*>(out + run0 + (unsigned)idx * 16u) = v;
        else *reinterpret_cast<uint4*>(out + ((gpos0 + m) * C::COUT + nt0 * 32 + j * NC) * C::EB + cc * 16) = v;
      }
    }
  }
  };
  emit(acc, a.scale, a.shift, reinterpret_cast<unsigned char*>(a.out));
  stamp(6);
  return true;
  };
  if constexpr (RESIDENT) {
    bool first_item = true;
    for (int wi = bidx >> 3; wi < wcount; wi += wstride)
      if (do_item(wfirst + wi, first_item)) first_item = false;
  } else {  // one work item per workgroup (no loop: its invariants would cost these kernels registers)
    if ((bidx >> 3) < wcount) do_item(wfirst + (bidx >> 3), true);
  }
}

static int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
    else n = 256;
  }
  return n;
}

// the forms a shape is launched in (HAS_RESID: with a stored shortcut and with the in-place one)
enum { HAS_STATS = 1, HAS_RESID = 2 };

template <class C, int FORM>
static int launch_form(const ConvArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  if (a.dbg & 16) {  // tuning aid: what the runtime says about residency of the kernel
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, conv3x3_kernel<C, FORM>, block.x, 0);
    fprintf(stderr, "[conv occupancy] LDS %d B, compiled for %d waves/SIMD: %d workgroups per CU\n", C::LDS, C::OCC, nb);
  }
  hipLaunchKernelGGL((conv3x3_kernel<C, FORM>), grid, block, 0, st, a);
  SK_HIP(hipGetLastError());
  return SK_OK;
}

template <class C, int FORMS>
static int launch_cfg(const ConvArgs& a, hipStream_t st) {
  static_assert(!(FORMS & HAS_RESID) || (C::S == 1 && C::CIN == C::COUT), "residual forms: conv2 of a block");
  const int tiles = cdiv(a.Hout, C::TH), nwork = a.B * tiles;
  // weight-resident shapes: just the workgroups the chip holds at once (LDS and the compiled-for occupancy), persistent
  constexpr int NWV = C::WM * C::WN;
  const int occ = C::OCC * 4 / NWV, by_lds = 160 * 1024 / C::LDS;
  // persist_cap (pipelined forwards, xt_forward_begin): a persistent shape takes fewer workgroups per CU than fit, so that the OTHER batch in flight finds room beside it -- with
  // all of a CU's registers and LDS held by a persistent layer-1 grid the other batch's kernels could only wait for it to end.  One per CU: 5.59 vs 5.63 ms per step with two batches
  // in flight (and 6.57 vs 5.92 ms for a forward on its own, which is why it is not the default of the plain forward).
  const int per_cu = (occ < by_lds ? (occ > 0 ? occ : 1) : by_lds);
  const int resident_wgs = cu_count() * ((a.persist_cap > 0 && a.persist_cap < per_cu) ? a.persist_cap : per_cu);
  constexpr int NY = C::COUT / C::NT;   // workgroups per work item (output-channel split): folded into a 1-D grid, see the kernel
  static_assert(NY == 1 || !C::RESIDENT, "persistent shapes cover all output channels");
  dim3 grid((unsigned)(NY > 1 ? cdiv(nwork, 8) * 8 * NY : ((C::RESIDENT && !(a.dbg & 8) && nwork > resident_wgs) ? resident_wgs : nwork)), 1);
  const dim3 block(NWV * 64);
  SK_CHECK(!a.gate != !a.se_part, SK_EARG, "a convolution is either the statistics form (se_part) or a residual form (gate)");
  SK_CHECK(!a.sc_wpack || a.sc_in, SK_EARG, "the 1x1 shortcut weights belong to the in-place shortcut form (sc_in)");
  if (a.se_part) {
    if constexpr (FORMS & HAS_STATS) return launch_form<C, FORM_STATS>(a, grid, block, st);
  } else if (a.sc_in) {  // first block of a layer: the 1x1 shortcut conv of the block input evaluated in this epilogue
    if constexpr (FORMS & HAS_RESID) {
      SK_CHECK(a.sc_wpack && a.sc_shift && !a.shortcut, SK_EARG, "in-place shortcut form: bad arguments");
      return launch_form<C, FORM_RESID_SC>(a, grid, block, st);
    }
  } else {
    if constexpr (FORMS & HAS_RESID) return launch_form<C, FORM_RESID>(a, grid, block, st);
  }
  set_error("this convolution shape has no %s form", a.se_part ? "statistics" : "residual");
  return SK_EARG;
}

// ---- the trunk's convolution shapes ---------------------------------------------------------
//                      T      CIN COUT S WIN TH WM WN MW NW  CK  OCC PD SWZ BLK M16 S2G
using B_L1  = ConvCfg<bf16_t,  32,  32, 1, 80,  8, 4, 1, 5, 1,  32, 0, 0, true>;     // two persistent weight-resident workgroups per CU; linear lanes + 32x32x16 MFMA kept: HBM-bound, 1 x 16 blocks / 16x16x32 measured no gain in the forward and the A,B,B,A read-group pattern of the 16-lane shape cannot be made conflict-free at 4 slots per position
using B_L2A = ConvCfg<bf16_t,  32,  64, 2, 80,  4, 2, 2, 3, 1,  32, 3, 0, true, LANES_LINEAR, true, true>;     // planar image (even | odd columns), 2 x 8 blocks, 16x16x32 MFMA, weights resident; 4-row tiles (47 KB), THREE persistent workgroups per CU (166 registers).  Statistics form alone: 174 us against 214 us for the row-major 32x32x16 shape and 184 us at two workgroups per CU
using B_L2  = ConvCfg<bf16_t,  64,  64, 1, 40,  8, 2, 2, 5, 1,  64, 3, 0, true, LANES_GRID, true>;     // three workgroups per CU; 2 x 8 read-group blocks
using B_L3A = ConvCfg<bf16_t,  64, 128, 2, 40,  4, 1, 4, 3, 1,  64, 2, 0, true, LANES_LINEAR, true, true>;     // planar image, 4 x 4 blocks, 16x16x32 MFMA (five 16-position tiles per wave, no idle MFMA rows): statistics form 132 us against 142 us row-major
using B_L3  = ConvCfg<bf16_t, 128, 128, 1, 20,  8, 1, 4, 5, 1, 128, 3, 0, true, LANES_GRID, true>;    // three workgroups per CU: 53760 B = 42 LDS granules; 4 x 4 read-group blocks
using B_L4A = ConvCfg<bf16_t, 128, 256, 2, 20,  8, 1, 4, 3, 1,  64, 2, 0, true, LANES_LINEAR, true, true>;     // planar image, 8 x 2 blocks with the rotated row key, 16x16x32 MFMA: 91 us against 135 us row-major (and 125 us for the planar image on the 32x32x16 MFMA); NT = 128: two workgroups per tile on one XCD
using B_L4  = ConvCfg<bf16_t, 256, 256, 1, 10, 17, 1, 4, 6, 1, 128, 2, 0, true, LANES_DENSE, true>;   // 187 of 192 lane slots enumerate the 17 x 11 padded tile; NT = 128: two workgroups per CU

// Small-grid forms (round 5; batches of at most xt_handle::SMALL_GRID_MAX_B = 12 utterances -- 1 is the reference driver's call shape -- xt_api.hip), residual forms only (conv2 of a
// block: no statistics whose order a tiling would change).  At batch 1 a launch is a handful of workgroups on an empty chip and its duration is ONE
// wave's dependent chain: a layer-4 launch is 3 row tiles x 2 channel halves = 6 workgroups whose waves each walk 1 728 MFMAs (25 us,
// profiles/r05_b1_kernel_stats_before.csv), a layer-3 launch 13 workgroups x 720 MFMAs (12.7 us).  3- / 5-row tiles on the DENSE lane order (any
// tile height whose padded enumeration fits the lanes: 3 x 21 = 63 of 64, 5 x 11 = 55 of 64, 2 x 11 = 22 of 32) make that 34 / 22 workgroups x 288 / 576
// MFMAs: 9.1 and 14.7 us.  Same MFMA shape, same k order, same epilogue arithmetic: the product shapes' bits.
// (Measured and NOT kept, profiles/r05_latency_matrix.txt: the product tilings with a deep or resident weight ring for every form of layers 2-4 --
// the idea being that two k-steps of prefetch are shorter than an L2 miss -- were 1-2 us SLOWER per launch: 0.710 vs 0.685 ms per utterance.)
// With tiles this short the weight ring matters as well (the product shapes fetch two k-steps ahead -- 168 registers at three workgroups per CU
// leave no more; here the register file is free): twelve k-steps ahead 0.625 vs 0.645 ms per utterance; layer 4 in 2-row tiles (52 workgroups
// x 288 MFMAs) 0.631 vs 0.645 (profiles/r05_latency_matrix.txt).
using B_L3T = ConvCfg<bf16_t, 128, 128, 1, 20,  3, 1, 4, 2, 1, 128, 1, 12, true, LANES_DENSE, true>;
using B_L4T = ConvCfg<bf16_t, 256, 256, 1, 10,  2, 1, 4, 1, 1, 128, 1, 12, true, LANES_DENSE, true>;

using F_L1  = ConvCfg<float,   32,  32, 1, 80,  8, 4, 1, 5, 1,  32, 0, 0, true>;
using F_L2A = ConvCfg<float,   32,  64, 2, 80,  8, 2, 2, 5, 1,  16, 0, 0, true>;
using F_L2  = ConvCfg<float,   64,  64, 1, 40,  8, 2, 2, 5, 1,  64, 0, 0, true>;
using F_L3A = ConvCfg<float,   64, 128, 2, 40,  8, 1, 4, 5, 1,  32>;
using F_L3  = ConvCfg<float,  128, 128, 1, 20,  8, 1, 4, 5, 1, 128>;
using F_L4A = ConvCfg<float,  128, 256, 2, 20, 16, 1, 4, 5, 2,  32>;
using F_L4  = ConvCfg<float,  256, 256, 1, 10, 16, 1, 4, 5, 2, 128>;
using F_L3T = F_L3; using F_L4T = F_L4;   // the f32 parity path keeps its shapes at every batch size

template <class C>
static void fill_geom(ConvGeom& g) {
  g.cin = C::CIN; g.cout = C::COUT; g.stride = C::S; g.win = C::WIN; g.th = C::TH; g.wm = C::WM;
  g.ck = C::CK; g.taps = 9; g.ks = C::KS; g.eb = C::EB; g.nw = C::NW; g.m16 = C::M16 ? 1 : 0;
}

// the product's shapes (the trunk's seven + the two small-grid tilings) and the forms the forward launches each in: a layer's stride-2
// first convolution is a conv1 (statistics), the small-grid tilings are conv2 only (residual)
#define SK_CONV_CASES(X) \
  X(CONV_L1, L1, HAS_STATS | HAS_RESID) X(CONV_L2A, L2A, HAS_STATS) X(CONV_L2, L2, HAS_STATS | HAS_RESID) X(CONV_L3A, L3A, HAS_STATS) \
  X(CONV_L3, L3, HAS_STATS | HAS_RESID) X(CONV_L4A, L4A, HAS_STATS) X(CONV_L4, L4, HAS_STATS | HAS_RESID)                           \
  X(CONV_L3T, L3T, HAS_RESID) X(CONV_L4T, L4T, HAS_RESID)

int conv_geom(int shape, int dtype, ConvGeom* g) {
  switch (shape) {
#define X(id, name, forms)                                       \
  case id:                                                       \
    if (dtype == DT_BF16) fill_geom<B_##name>(*g); else fill_geom<F_##name>(*g); \
    return SK_OK;
    SK_CONV_CASES(X)
#undef X
  }
  set_error("conv_geom: unknown conv shape %d", shape);
  return SK_EARG;
}

int launch_conv(int shape, int dtype, const ConvArgs& a, hipStream_t st) {
  switch (shape) {
#define X(id, name, forms) \
  case id: return dtype == DT_BF16 ? launch_cfg<B_##name, forms>(a, st) : launch_cfg<F_##name, forms>(a, st);
    SK_CONV_CASES(X)
#undef X
  }
  set_error("launch_conv: unknown conv shape %d", shape);
  return SK_EARG;
}

// Host-side packer: torch layout W[cout][cin][kh][kw] (f32) -> MFMA fragment order.
// Fragment (ntile, kidx=(chunk,tap,ks)), lane (r = lane&31, h = lane>>5), element j:
//   W[ntile*32 + r][chunk*CK + ks*KE + h*KE/2 + j][tap]      (KE = 32 B / element size)
size_t conv_pack_bytes(const ConvGeom& g) { return (size_t)g.cout * g.cin * g.taps * g.eb; }

// M16 (bf16 only): fragment (16-channel tile n16, kidx32 = (chunk, tap, s)), lane (r = lane & 15, q = lane >> 4), element j:
//   W[n16*16 + r][chunk*CK + s*32 + q*8 + j][tap]
void conv_pack_weights(const ConvGeom& g, const float* w, int kh_kw, void* dst) {
  if (g.m16) {
    const int nch = g.cin / g.ck, ks32 = g.ck * g.eb / 64, ktot32 = nch * g.taps * ks32;
    for (int n16 = 0; n16 < g.cout / 16; ++n16)
      for (int ch = 0; ch < nch; ++ch)
        for (int t = 0; t < g.taps; ++t) {
          const int tap = (g.taps == 9) ? t : (kh_kw == 9 ? 4 : 0);
          for (int sk = 0; sk < ks32; ++sk) {
            const size_t kidx = (size_t)(ch * g.taps + t) * ks32 + sk;
            for (int lane = 0; lane < 64; ++lane)
              for (int j = 0; j < 8; ++j) {
                const int co = n16 * 16 + (lane & 15), ci = ch * g.ck + sk * 32 + (lane >> 4) * 8 + j;
                reinterpret_cast<uint16_t*>(dst)[(((size_t)n16 * ktot32 + kidx) * 64 + lane) * 8 + j] = f32_to_bf16(w[((size_t)co * g.cin + ci) * kh_kw + tap]);
              }
          }
        }
    return;
  }
  const int KE = 32 / g.eb, nch = g.cin / g.ck, ktot = nch * g.taps * g.ks;
  for (int nt = 0; nt < g.cout / 32; ++nt)
    for (int ch = 0; ch < nch; ++ch)
      for (int t = 0; t < g.taps; ++t) {
        const int tap = (g.taps == 9) ? t : (kh_kw == 9 ? 4 : 0);
        for (int ks = 0; ks < g.ks; ++ks) {
          const size_t kidx = (size_t)(ch * g.taps + t) * g.ks + ks;
          for (int lane = 0; lane < 64; ++lane) {
            const int r = lane & 31, h = lane >> 5;
            for (int j = 0; j < KE / 2; ++j) {
              const int co = nt * 32 + r, ci = ch * g.ck + ks * KE + h * (KE / 2) + j;
              const float v = w[((size_t)co * g.cin + ci) * kh_kw + tap];
              const size_t e = (((size_t)nt * ktot + kidx) * 64 + lane) * (KE / 2) + j;
              if (g.eb == 2) reinterpret_cast<uint16_t*>(dst)[e] = f32_to_bf16(v);
              else reinterpret_cast<float*>(dst)[e] = v;
            }
          }
        }
      }
}

}  // namespace sk
