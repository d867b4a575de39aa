// mfma_core.h -- what the kernel sources share (all but point_ops.hip, neighbors.hip, voxel_points.hip, fps.hip and sa_msg.hip, which take host_util.h; the probes under tools/micro include
// it too).  Device code only, __forceinline__ in an anonymous namespace: nothing here is a symbol.
//   * types and LDS maps: Geo<NC> (a workgroup's NC activation columns as [channel][column] f32 rows, XOR-swizzled: swz),
//     PG<LL> (the same tensors as pre-split f16 planes in B-fragment order), Ctx;
//   * split-f16 arithmetic: an f32 operand travels as hi + lo f16 (kSplit = 2), a product is three v_mfma_f32_16x16x32_f16
//     (mfma_split); split_f16x2 / split_planes8 / store_planes4 make the planes, range_pow2 / pow2_inv their range scale;
//   * cross-lane reductions on the VALU (DPP, permlane swaps), and over all 64 lanes by shuffles (wave_max, wave_sum);
//   * GEMM cores, weights streamed L2 -> VGPR as whole fragments (wstream.h).  f32 pipe (v_mfma_f32_16x16x4_f32):
//     gemm_fast_pf / gemm_fast_tap3 / gemm_fast / gemm_small, store_tiles, gemm_passes with the GroupNorm + scale/shift + SiLU
//     + residual epilogue, conv_gemm dealing a layer's output tiles over the waves.  Split-f16 pipe: gemm1_pl (1x1, B from planes).
// GLDM_API marks the exported entry points; GLDM_SKIP / GLDM_STAMPS are the hooks of -DGLDM_DEBUG_KNOBS diagnostic builds.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gldm.h"
#include "wstream.h"
#include "devstate.h"

#define GLDM_API extern "C" __attribute__((visibility("default")))

// Diagnostic knobs (phase skipping, per-op cycle stamps, workgroup stagger) exist only in builds made
// with -DGLDM_DEBUG_KNOBS (make EXTRA=-DGLDM_DEBUG_KNOBS); the shipped kernels contain none of them.
#ifdef GLDM_DEBUG_KNOBS
#define GLDM_SKIP(c, bit) ((c).skip & (bit))
#define GLDM_STAMPS(p) (p)
#else
#define GLDM_SKIP(c, bit) false
#define GLDM_STAMPS(p) ((long long *)nullptr)
#endif

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((address_space(3))) float lds_f;   // explicit LDS pointers: 32-bit ds_* addressing
typedef __attribute__((address_space(3))) f32x4 lds_f4;

constexpr int kHeads = 4, kDimHead = 32, kHidden = kHeads * kDimHead;  // LinearAttention defaults
constexpr int kMaxC = 256;

// Geometry and LDS map (floats) of one workgroup.  X: block input / residual stream, H: scratch.
template <int NC>
struct Geo {
  static constexpr int kWaves = NC / 8;           // 8 waves at 64 columns, 4 at 32
  static constexpr int kThreads = kWaves * 64;
  static constexpr int kNT = NC / 16;             // 16-column n-tiles
  static constexpr int kRP = 64 / NC;             // rows a wave touches per pass: lane = (sub, column)
  static constexpr int kSlots = kWaves * kRP;     // row slots of the norm passes
  static constexpr int kBufX = 0;
  static constexpr int kBufH = kMaxC * NC;
  static constexpr int kBufY = 128 * NC;          // attention: LayerNorm output, later to_out output
  static constexpr int kBufO = kBufH;             // attention output, 128 rows
  static constexpr int kBufQKV = kBufO + kHidden * NC;  // two heads of q,k,v: 192 rows
  static constexpr int kArena = kBufQKV + 192 * NC;
  static constexpr int kMiscLat = kArena;         // [NC] current latent row
  static constexpr int kMiscEps = kMiscLat + NC;
  static constexpr int kMiscG = kMiscEps + NC;    // [S][E] <= 320
  static constexpr int kMiscRed1 = kMiscG + 320;  // [kWaves][NC] cross-wave exchange slots (per wave and column)
  static constexpr int kMiscRed2 = kMiscRed1 + kWaves * NC;
  static constexpr int kMiscTape = kMiscRed2 + kWaves * NC;  // [kMaxOps][12] ints: the step program (+ its length)
  static constexpr int kMiscSegs = kMiscTape + 1024;         // [kMaxSegs][4] ints: this workgroup's (tile, s0, s1) list
  static constexpr int kMiscOld = kMiscSegs + 256;           // [NC] previous step's denoised row (DPM++ 2M)
  // 64-column engines: per-sample range of a ResnetBlock's H (conv_pm3_wave): [8 waves][16] published bounds, [16] scales
  static constexpr int kMiscHb = kMiscOld + NC;
  static constexpr int kMiscHs = kMiscHb + (NC == 64 ? 8 * 16 : 0);
  static constexpr int kMiscQ = kMiscHs + (NC == 64 ? 16 : 0);    // quad engine hand-shake words (quad_narrow.h): 8 + 4 x 64 ints
  static constexpr int kMiscQTab = kMiscQ + (NC == 64 ? 16 + 4 * 64 : 0);   // [2 x 380] byte offsets of the quad engines' weight streams (292 / 336 / 380 fragments)
  static constexpr int kLdsFloats = kMiscQTab + (NC == 64 ? 2 * 380 : 0);
};
static_assert(Geo<64>::kLdsFloats * 4 <= 160 * 1024, "LDS budget (1 WG/CU)");
static_assert(Geo<32>::kLdsFloats * 4 * 2 <= 160 * 1024, "LDS budget (2 WG/CU)");

// (Tried: XOR with row bit 0 ^ row bit 2, which also frees the accumulator stores (rows 4 kq + r) of their 2-way bank
// conflict.  The B-fragment reads of a k-block then need two base registers instead of one with immediate offsets,
// and every GEMM phase got 5-7 % slower.)
template <int NC>
__device__ __forceinline__ int swz(int row, int col) { return row * NC + (col ^ ((row & 1) << 4)); }

// Position-major engine (64 columns, split-f16 GEMMs): a B fragment of v_mfma_f32_16x16x32_f16 is rows 8 g + j
// (g = lane >> 4, j = 0..7) of one column per lane, so the four lane groups of a read sit 8 rows apart in the same
// columns.  XOR-ing the column's position tile with bits 3-4 of the row sends them to four different 16-bank groups:
// every B read is conflict free, with ONE lane base per tile (the XOR does not depend on j or on the 32-row block).
__device__ __forceinline__ int pswz(int row, int col) { return row * 64 + (col ^ (((row >> 3) & 3) << 4)); }

// Split operands (see "split-f16 GEMM core" below): every f32 value travels as kSplit = 2 f16 numbers, hi + lo.
constexpr int kSplit = 2;
constexpr int kFragBytes = kSplit * 1024;        // one weight fragment: [plane][lane 64][8 f16]

// Pre-split activation planes of the 64-column engines.  A tensor that is only ever read as a GEMM B operand is kept
// in LDS already split into its two f16 planes, in B-fragment order:
//   [32-channel block kb][plane hi|lo][g = 0..3][column 0..63][8 f16 = channels 32 kb + 8 g + 0..7]
// (8 KiB per 32 channels).  The producer's epilogue splits each element ONCE (its accumulators hold 4 consecutive
// channels of a column: one ds_write_b64 per plane); the eight consumer waves read a whole fragment plane with one
// ds_read_b128 per lane and their k-loops are loads + MFMA only.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((address_space(3))) u32x4 lds_u4;
typedef __attribute__((address_space(3))) u32x2_t lds_u2;
// Geometry of the plane rows.  LL = 4 (position-major tiles of the 4-position denoiser): 64 columns per (block, plane, g)
// row.  LL = 16 (the 16-position nets: pose decoder, ppc denoiser; column = 4 * position + sample, 4 samples per tile):
// 72 entries per row, the 64 columns at entries 4 .. 67 between four ZERO entries on each side, so that the taps of a
// k = 3 conv are the same reads shifted by one position = 4 entries (entry 4 t + column for tap t), with no masks.
template <int LL>
struct PG {
  static constexpr int kCols = LL == 16 ? 72 : 64;   // 16-byte entries per row
  static constexpr int kOff = LL == 16 ? 4 : 0;      // entry of column 0
  static constexpr int kPlaneU4 = 4 * kCols;         // entries per plane of a 32-channel block
  static constexpr int kBlockU4 = kSplit * kPlaneU4; // per block
  static constexpr int kBlockFloats = 4 * kBlockU4;
  static constexpr int kH = 128 * 64;                // H planes (floats), 4 blocks
  static constexpr int kX = kH + 4 * kBlockFloats;   // X planes
  // the 256-channel level's one set, 8 blocks.  LL = 4: behind the 256 f32 rows of X; LL = 16: over both regions (its f32
  // rows 128 .. 255 lie over the first blocks: the residual stream is parked in global scratch, Ctx::park)
  static constexpr int kW = LL == 16 ? kH : 256 * 64;
  static constexpr int kEnd = kW + 8 * kBlockFloats;
};
static_assert(PG<4>::kEnd <= 512 * 64, "position-major planes end in front of the attention exchange slots");
static_assert(PG<16>::kEnd <= Geo<64>::kArena, "padded planes fit the arena");
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
// (a, b) -> packed f16 hi parts and packed f16 lo parts: x = hi + lo up to 2^-22 |x| (f16 subnormals are kept by the
// matrix pipe -- tools/micro/mfma_f16_split -- so small lo parts lose nothing but bits below 2^-25).
// v_cvt_pk_f16_f32 (round to nearest even), the remainders from the packed halves by v_fma_mix_f32, v_cvt_pk_f16_f32.
__device__ __forceinline__ void split_f16x2(float a, float b, unsigned &hi, unsigned &lo) {
  const f16x2 h = __builtin_convertvector(f32x2{a, b}, f16x2);
  const float ra = __builtin_fmaf((float)h[0], -1.0f, a), rb = __builtin_fmaf((float)h[1], -1.0f, b);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{ra, rb}, f16x2));
}
// rows c0 .. c0 + 3 (c0 % 4 == 0) of column n -> the two planes
template <int LL = 4>
__device__ __forceinline__ void store_planes4(float *planes, int c0, int n, float v0, float v1, float v2, float v3) {
  unsigned h0, h1, l0, l1;
  split_f16x2(v0, v1, h0, l0);
  split_f16x2(v2, v3, h1, l1);
  // dword address: (((kb * kSplit + plane) * 4 + g) * kCols + kOff + n) * 4 + 2 * (half of the 8-group)
  using G = PG<LL>;
  const int a = ((((c0 >> 5) * kSplit) * 4 + ((c0 >> 3) & 3)) * G::kCols + G::kOff + n) * 4 + ((c0 >> 2) & 1) * 2;
  lds_u2 *d = (lds_u2 *)(planes + a);
  d[0] = u32x2_t{h0, h1};
  d[2 * G::kPlaneU4] = u32x2_t{l0, l1};    // next plane: kPlaneU4 entries of 16 bytes = 2 kPlaneU4 u2
}

// ---- range scale of split operands ------------------------------------------------------------------------------------
// f16 carries 5 exponent bits: a value of 65520 or more has hi = inf (and lo = x - inf = NaN), one below 2^-14 a subnormal
// hi.  Where the DATA sets an operand's magnitude (a gathered neighbourhood, a cloud's features, the ReLU outputs behind
// them: BatchNorm is folded, so everything scales with the input) the tile is split as x / s with s a power of two chosen
// from the tile's largest magnitude (measured where the staged values sit in registers, a bound  R m + B  -- R the layer's
// largest row sum of |W|, B its largest |bias| -- for the hidden layers behind them) and s is folded back where the
// accumulators leave the matrix pipe: exact, wave uniform, three or four VALU instructions per tile and layer.  s = 1 for
// anything ordinary (2^-8 <= m < 2^14): every bit is then what it was without the scale.
__device__ __forceinline__ float range_pow2(float m) {   // m >= 0 (a maximum of magnitudes or a bound on one), wave uniform
  int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - 127;   // floor(log2 m) of a normal m
  if ((e >= -8 && e < 14) || e < -100 || e > 100) return 1.0f;   // ordinary; nothing there; beyond rescue (inf / nan included)
  e = e < -40 ? -40 : e;                                     // biases divided by s stay finite
  return __uint_as_float((unsigned)(e - 13 + 127) << 23);    // m / s in [2^13, 2^14)
}
__device__ __forceinline__ float pow2_inv(float s) { return __uint_as_float((254u << 23) - __float_as_uint(s)); }   // s = 2^k, |k| <= 126

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + fast_exp(-x)); }

// Cross-lane reductions on the VALU: DPP operands for the lanes of a sample (quad / row mirrors: each
// step adds the partial sum of the complementary lane group, so every lane ends with the total) and
// v_permlane32_swap for the two halves of a wave.  A ds_bpermute shuffle costs an LDS round trip each.
// (mov_dpp leaves the destination's previous value undefined for lanes without a source -- every control used with it
// covers all lanes; update_dpp(0, ...) made the compiler clear the destination with a v_mov_b32 in front of every one.)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  static_assert(CTRL <= 0xFF || (CTRL >= 0x121 && CTRL <= 0x12F) || CTRL == 0x140 || CTRL == 0x141, "a control that covers all lanes");
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xf, 0xf, false));
}
// max(a, b) as ONE instruction: fmaxf on values that come out of a bit cast (DPP / permlane results) gets a canonicalising
// v_max_f32 x, x per operand in front of it
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// max(x, x seen through the DPP control): one v_max_f32_dpp (the s_nop covers the VALU-write -> DPP-read hazard, which
// nobody checks inside an asm statement)
template <int CTRL>
__device__ __forceinline__ float dpp_max(float x) {
  float r;
  if constexpr (CTRL == 0x124) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else if constexpr (CTRL == 0x128) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else if constexpr (CTRL == 0xB1) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else if constexpr (CTRL == 0x4E) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else static_assert(CTRL == 0x124, "add the control's assembler spelling");
  return r;
}
template <int L>
__device__ __forceinline__ float group_sum(float x) {  // sum over the L lanes (columns) of a sample
  x += dpp_mov<0xB1>(x);                   // quad_perm [1,0,3,2]
  x += dpp_mov<0x4E>(x);                   // quad_perm [2,3,0,1]
  if constexpr (L >= 8) x += dpp_mov<0x141>(x);   // row_half_mirror
  if constexpr (L >= 16) x += dpp_mov<0x140>(x);  // row_mirror
  return x;
}
__device__ __forceinline__ float half_sum(float x) {  // lanes i and i ^ 32
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float row_pair_sum(float x) {  // lanes i and i ^ 16
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float row_pair_max(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return vmax(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return vmax(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// All 64 lanes, where the reduction is not the hot path (one per tile or row): shuffles, offsets 1, 2, .. 32.  The
// sum's order is part of its result: a fixed tree, the same bits on every run.
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o);
  return x;
}

__device__ __forceinline__ float row16_max(float x) {  // max over the 16 lanes of a DPP row
  x = dpp_max<0xB1>(x);   // quad_perm [1,0,3,2]
  x = dpp_max<0x4E>(x);   // quad_perm [2,3,0,1]
  x = fmaxf(x, dpp_mov<0x141>(x));  // row_half_mirror
  x = fmaxf(x, dpp_mov<0x140>(x));  // row_mirror
  return x;
}

struct Ctx {
  const float *w;   // packed weights
  float *lds;
  int tid, wave, lane;
  int skip;         // diagnostic phase-skip mask (GLDM_R1D_SKIP), 0 in production
  int nta;          // live 16-column n-tiles of this workgroup (kNT = full tile, 1 = tail tile)
  // scale / shift rows precomputed per conditioning cloud (pose decoder: ss_table_kernel), for the tile's samples 0 and
  // 1 (16-position engine: a 16-column n-tile is one sample), or null: computed in the epilogue
  const float *ss_row[2] = {nullptr, nullptr};
  const float *ss_lane = nullptr;   // 16-position 64-column engine: the same rows for THIS LANE's sample (lane & 3), or null
  // position-major engine, 256-channel level: this workgroup's 64 KiB of global scratch where the residual stream is
  // parked (f32) between the level's down conv and the end of its ResnetBlock, while LDS holds the split planes
  float *park = nullptr;
};

// ---------------------------------------------------------------- GEMM ----
// Every conv / 1x1 is  acc[mi][ni] += W[16(mt0+mi).., :] * im2col(src)[:, 16(nt0+ni)..]
// on v_mfma_f32_16x16x4_f32.  Packed weights: k = tap * Cin + ci, 16-deep k-blocks.
template <int L>
__device__ __forceinline__ float tap_left(float v, bool keep) {  // value of column n-1
  const float f = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111 /*row_shr:1*/, 0xf, 0xf, true));
  return (L >= 16 || keep) ? f : 0.f;
}
template <int L>
__device__ __forceinline__ float tap_right(float v, bool keep) {  // value of column n+1
  const float f = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x101 /*row_shl:1*/, 0xf, 0xf, true));
  return (L >= 16 || keep) ? f : 0.f;
}

// Fast path (Cin % 16 == 0).  A 16-column tile never straddles a sample (L divides 16), so the
// row-boundary lanes of the halo shift are exactly the lanes whose tap falls outside the sample:
// zero fill (bound_ctrl) for L = 16, an extra (col % L) mask for L = 4.
struct NoPre { __device__ __forceinline__ void operator()() const {} };
// pre(): work that does not depend on the GEMM, run right after the first weight fragments have been requested (it
// then costs nothing while their round trip is outstanding).
template <int NC, int L, int TAPS, int MT, int NT, int PF, class PRE = NoPre>
__device__ __forceinline__ void gemm_fast_pf(const Ctx &c, const float *__restrict__ wp, int cblocks, int mt0, int nt0,
                                             const float *src, f32x4 (&acc)[MT][NT], const PRE &pre = PRE()) {
  // PF = weight blocks in flight; cblocks % PF == 0.  The unrolled body is UNCONDITIONAL: a load
  // whose only consumer sits behind a branch is sunk into that branch by the compiler (and then
  // waited for at once), and a branch around a load forces s_waitcnt 0 at the join.  Block indices
  // are clamped instead; the redundant re-loads at the tail are harmless.
  const int col = c.lane & 15, kq = c.lane >> 4;
  const int kblocks = TAPS * cblocks;
  const WStream wv(wp, c.lane);
  // B-fragment addresses.  Row 4 j + kq has the parity of kq for every j, so the swizzle is the same for all four
  // k-steps, and with nt0 even it only swaps the n-tiles of a pair: at 8 n-tiles (nt0 = 0) two lane-dependent bases
  // (even / odd n-tile) plus compile-time offsets, which the reads carry as immediates -- not 32 registers.  (At 2 and
  // 4 n-tiles the engine's phases measured 1 % slower this way, spill-free as they became.)
  int boff[4][NT];
  if constexpr (NT >= 8) {
    int bb[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) bb[e] = swz<NC>(kq, 16 * (nt0 + e) + col);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) boff[j][ni] = bb[ni & 1] + 4 * j * NC + 16 * (ni & ~1);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) boff[j][ni] = swz<NC>(4 * j + kq, 16 * (nt0 + ni) + col);
  }
  f32x4 a[PF][TAPS][MT];
  // B values: double buffered over k-blocks, except at 8 n-tiles, where a k-step's 8+ MFMAs are cover enough: the row
  // of step j is refilled from the next block the moment step j's MFMAs have issued (three steps to arrive), in ONE
  // set of registers (32 fewer at NT = 8).
  constexpr bool kBS = NT >= 8 && PF > 1;
  float b[kBS ? 1 : 2][4][NT];
  f32x4 side[TAPS > 1 ? 2 : 1][MT][NT];  // tap 0 and tap 2 partial results (tap 1 goes to acc)
  if (TAPS == 3) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) side[t][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // part = -1: the whole block; part 0..2: the third of the block's fragments issued beside
  // k-step `part` (a burst of every wave's loads at the block boundary stalls all of them in the
  // vector-memory issue queue while the MFMA pipe idles: spread, the two pipes overlap)
  auto load_a = [&](int buf, int cb, int part) {
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
        if (part < 0 || (t * MT + mi) % 3 == part)
          a[buf][t][mi] = wv[((size_t)(mt0 + mi) * kblocks + t * cblocks + cb) * 64];
  };
  const lds_f *src3 = (const lds_f *)src;
  auto load_b = [&](int buf, int cb) {
    const lds_f *s = src3 + cb * 16 * NC;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) b[buf][j][ni] = s[boff[j][ni]];
  };
  auto mfma_step = [&](int abuf, int bbuf, int j) {
    if (TAPS == 3) {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          side[0][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[abuf][0][mi][j], b[bbuf][j][ni], side[0][mi][ni], 0, 0, 0);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[abuf][TAPS > 1 ? 1 : 0][mi][j], b[bbuf][j][ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          side[TAPS > 1 ? 1 : 0][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[abuf][TAPS > 2 ? 2 : 0][mi][j], b[bbuf][j][ni], side[TAPS > 1 ? 1 : 0][mi][ni], 0, 0, 0);
    } else {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[abuf][0][mi][j], b[bbuf][j][ni], acc[mi][ni], 0, 0, 0);
    }
  };
  const int last = cblocks - 1;
  if constexpr (PF == 1) {
    for (int cb = 0; cb < cblocks; ++cb) {
      load_a(0, cb, -1);
      load_b(0, cb);
      if (cb == 0) pre();
#pragma unroll
      for (int j = 0; j < 4; ++j) mfma_step(0, 0, j);
    }
  } else {
#pragma unroll
    for (int u = 0; u < PF - 1; ++u) load_a(u, u < last ? u : last, -1);
    load_b(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    pre();
    __builtin_amdgcn_sched_barrier(0);
    for (int cb0 = 0; cb0 < cblocks; cb0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int cb = cb0 + u;
        const int acb = cb + PF - 1 < last ? cb + PF - 1 : last, bcb = cb + 1 < last ? cb + 1 : last;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < 3) load_a((u + PF - 1) % PF, acb, j);
          if (!kBS && j == 0) load_b((u + 1) & 1, bcb);
          __builtin_amdgcn_sched_barrier(0);
          mfma_step(u, kBS ? 0 : (u & 1), j);
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (kBS) {
            const lds_f *sn = src3 + bcb * 16 * NC;
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) b[0][j][ni] = sn[boff[j][ni]];
          }
        }
      }
    }
  }
  if (TAPS == 3) {
    const bool keepL = (col & (L - 1)) != 0, keepR = (col & (L - 1)) != (L - 1);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[mi][ni][r] += tap_left<L>(side[0][mi][ni][r], keepL) + tap_right<L>(side[TAPS > 1 ? 1 : 0][mi][ni][r], keepR);
  }
}

// k = 3 convs, tap-major: inside a 16-channel block the three taps are swept one after the other
// (4 k-steps each), and the moment a tap's sweep has issued its MFMAs its fragment registers are
// refilled with the NEXT block's fragments of that tap.  Every weight load then has exactly one
// block of MFMAs (48 at 2 x 2 tiles) to arrive, with ONE set of fragment registers and never more
// than a block's worth of loads in flight per wave: the double-buffered form kept up to two, and
// a long weight stream queued in the CU's vector-memory path is what delays the co-resident
// workgroup's short phases.
template <int NC, int L, int MT, int NT>
__device__ __forceinline__ void gemm_fast_tap3(const Ctx &c, const float *__restrict__ wp, int cblocks, int mt0, int nt0,
                                               const float *src, f32x4 (&acc)[MT][NT]) {
  const int col = c.lane & 15, kq = c.lane >> 4;
  const int kblocks = 3 * cblocks;
  const WStream wv(wp, c.lane);
  int boff[4][NT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) boff[j][ni] = swz<NC>(4 * j + kq, 16 * (nt0 + ni) + col);
  f32x4 a[3][MT];
  float b[2][4][NT];
  f32x4 side[2][MT][NT];  // tap 0 and tap 2 partial results (tap 1 goes to acc)
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) side[t][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  const lds_f *src3 = (const lds_f *)src;
  auto load_b = [&](int buf, int cb) {
    const lds_f *s = src3 + cb * 16 * NC;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) b[buf][j][ni] = s[boff[j][ni]];
  };
  const int last = cblocks - 1;
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) a[t][mi] = wv[((size_t)(mt0 + mi) * kblocks + t * cblocks) * 64];
  load_b(0, 0);
  for (int cb0 = 0; cb0 < cblocks; cb0 += 2) {  // two blocks per trip: the B double buffer alternates statically
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cb = cb0 + u;
      const int nb = cb + 1 < last ? cb + 1 : last;  // clamped: the loads stay unconditional
      load_b(1 - u, nb);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) {
              f32x4 &d = t == 1 ? acc[mi][ni] : side[t >> 1][mi][ni];
              d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][mi][j], b[u][j][ni], d, 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) a[t][mi] = wv[((size_t)(mt0 + mi) * kblocks + t * cblocks + nb) * 64];
      }
    }
  }
  const bool keepL = (col & (L - 1)) != 0, keepR = (col & (L - 1)) != (L - 1);
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[mi][ni][r] += tap_left<L>(side[0][mi][ni][r], keepL) + tap_right<L>(side[1][mi][ni][r], keepR);
}

// ---- split-f16 GEMM core of the 64-column engines ------------------------------------------------------------
// f32 matrix products on the f16 matrix pipe.  v_mfma_f32_16x16x32_f16 delivers 16x the FLOP/cycle of
// v_mfma_f32_16x16x4_f32, so an f32 product computed EXACTLY ENOUGH from f16 pieces still wins: every f32 operand is
// written as hi + lo, two f16 numbers (11 + 11 significant bits; the matrix pipe keeps f16 subnormals, so a small lo
// part loses only bits below 2^-25), and a product a b is the sum of three partial products,
//   a b ~ a_hi b_lo + a_lo b_hi + a_hi b_hi      (three MFMAs, f32 accumulation),
// the dropped one (lo lo) being <= 2^-22 |a b|.  3/16 of the f32-MFMA time -- and half of what the three-piece bf16
// split of rounds 3-4 took (six products) at the same measured accuracy: on a 16 x 16 x 768 product the error relative
// to sum |a b| is 1.3e-7 (f32 fma chain: 1.3e-7; bf16 x 3: 1.5e-7), on operands spread over 15 binades 3.5e-7 (5.6e-7;
// 3.4e-7) -- tools/micro/mfma_f16_split, profiles/r05_mfma_f16_split.txt.  Weights are split once on the host
// (r1d_pack.py: mfma_a_fragments_f16x2, layout in gldm.h); activations are split by the producing epilogue
// (store_planes4) or as they are read from LDS (split_planes8).  Range: |x| < 65504 (f16); the packers refuse weights
// beyond it, activations of these nets are O(10) behind their norms.
// Measured against the reference's vectors: single forwards 1.7e-6 from the f32 graph, 100 DDIM steps 1.8e-6
// (tools/study/f16x2_error.py), well inside the 2e-5 / 1e-4 parity bars.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// x[0..7] (consecutive k of one column) -> the planes of a B fragment
__device__ __forceinline__ void split_planes8(const float (&x)[8], u32x4 (&pl)[kSplit]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned h, l;
    split_f16x2(x[2 * q], x[2 * q + 1], h, l);
    pl[0][q] = h;
    pl[1][q] = l;
  }
}
__device__ __forceinline__ f32x4 mfma_h(const u32x4 &a, const u32x4 &b, const f32x4 &c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// acc += A B with both operands split: small terms first
__device__ __forceinline__ f32x4 mfma_split(const u32x4 (&a)[kSplit], const u32x4 (&b)[kSplit], f32x4 acc) {
  acc = mfma_h(a[0], b[1], acc);
  acc = mfma_h(a[1], b[0], acc);
  return mfma_h(a[0], b[0], acc);
}

// PRE of the position-major k = 3 convs: NoPreA, or the engine's PreA (first weight fragments requested by the caller)
struct NoPreA { static constexpr bool on = false; };

// 1x1 conv with the B operand from pre-split planes (the folded-LayerNorm qkv conv reads the X planes).
// MS: stride between the wave's m-tiles (the fused qkv + attention phase takes a head's q, k and v rows: 8 m-tiles apart).
// FIRST: NoFirst, or Frag3 = block 0's fragments of the first m-tile, requested by the caller ahead of the call (by value in
// registers: a pointer to them would put the array on the stack).
struct NoFirst { static constexpr bool on = false; };
struct Frag3 { static constexpr bool on = true; u32x4 p[kSplit]; };
template <int KB32, int MT, int NT, class PRE = NoPre, int MS = 1, int LL = 4, class FIRST = NoFirst>
__device__ __forceinline__ void gemm1_pl(const Ctx &c, const float *__restrict__ wp3, int mt0, int nt0, const float *planes,
                                         f32x4 (&acc)[MT][NT], const PRE &pre = PRE(), const FIRST &first = FIRST()) {
  const int col = c.lane & 15, g = c.lane >> 4;
  const WStream wv(wp3, c.lane);
  using PGx = PG<LL>;
  const lds_u4 *pl3 = (const lds_u4 *)planes + g * PGx::kCols + PGx::kOff + 16 * nt0 + col;
  u32x4 a[2][MT][kSplit];
  u32x4 bs[2][kSplit];
  auto load_a = [&](int buf, int kb) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      const int sb = ((mt0 + mi * MS) * KB32 + kb) * kFragBytes;   // one scalar offset per (m-tile, block), the planes by immediates
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) a[buf][mi][pl] = wv.raw_at(sb, pl * 1024);
    }
  };
  auto load_b = [&](int buf, int kb, int ni) {
#pragma unroll
    for (int pl = 0; pl < kSplit; ++pl) bs[buf][pl] = pl3[(kb * kSplit + pl) * PGx::kPlaneU4 + 16 * ni];
  };
  if constexpr (FIRST::on) {
#pragma unroll
    for (int pl = 0; pl < kSplit; ++pl) a[0][0][pl] = first.p[pl];
    if constexpr (MT > 1) {
#pragma unroll
      for (int mi = 1; mi < MT; ++mi) {
        const int sb = ((mt0 + mi * MS) * KB32) * kFragBytes;
#pragma unroll
        for (int pl = 0; pl < kSplit; ++pl) a[0][mi][pl] = wv.raw_at(sb, pl * 1024);
      }
    }
  } else {
    load_a(0, 0);
  }
  load_b(0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  pre();
  __builtin_amdgcn_sched_barrier(0);
  // The requests are pinned in front of the MFMAs they are to run under: left to the scheduler, the next block's
  // fragment loads sank to their first use (load, s_waitcnt vmcnt(0), MFMA -- six to nine L2 round trips per block; the
  // 128-channel qkv conv took 18.4 k cycles for 9.2 k of MFMAs).
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb) {
    if (kb + 1 < KB32) load_a((kb + 1) & 1, kb + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int step = kb * NT + ni, nxt = step + 1;
      if (nxt < KB32 * NT) load_b(nxt & 1, nxt / NT, nxt % NT);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) acc[mi][ni] = mfma_split(a[kb & 1][mi], bs[step & 1], acc[mi][ni]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int NC, int L, int TAPS, int MT, int NT>
__device__ __forceinline__ void gemm_fast(const Ctx &c, const float *__restrict__ wp, int cblocks, int mt0, int nt0,
                                          const float *src, f32x4 (&acc)[MT][NT]) {
  constexpr int PFMAX = (MT * TAPS > 6) ? 2 : (MT * TAPS > 4 ? 2 : 4);  // register budget
  if constexpr (TAPS == 3) {
    if ((cblocks & 1) == 0) {
      gemm_fast_tap3<NC, L, MT, NT>(c, wp, cblocks, mt0, nt0, src, acc);
      return;
    }
  }
  if (PFMAX == 4 && (cblocks & 3) == 0) gemm_fast_pf<NC, L, TAPS, MT, NT, PFMAX>(c, wp, cblocks, mt0, nt0, src, acc);
  else if ((cblocks & 1) == 0) gemm_fast_pf<NC, L, TAPS, MT, NT, 2>(c, wp, cblocks, mt0, nt0, src, acc);
  else gemm_fast_pf<NC, L, TAPS, MT, NT, 1>(c, wp, cblocks, mt0, nt0, src, acc);
}

// Generic path (Cin % 16 != 0: the 4-channel level of the latent denoiser): masked reads.
template <int NC, int L, int MT, int NT>
__device__ __forceinline__ void gemm_small(const Ctx &c, const float *__restrict__ wp, int kblocks, int mt0, int nt0,
                                           const float *src, int cin, int ktaps, f32x4 (&acc)[MT][NT]) {
  const int col = c.lane & 15, kq = c.lane >> 4;
  const WStream wv(wp, c.lane);
  const lds_f *src3 = (const lds_f *)src;
  int dk = 0, cib = 0;
  const int pad = ktaps == 3 ? 1 : 0;
  for (int kb = 0; kb < kblocks; ++kb) {
    f32x4 a[MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) a[mi] = wv[((size_t)(mt0 + mi) * kblocks + kb) * 64];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ci = cib + kq;
      const int shift = dk - pad;
      float b[NT];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = 16 * (nt0 + ni) + col;
        const int p = (n & (L - 1)) + shift;
        const bool ok = (dk < ktaps) && (ci < cin) && (p >= 0) && (p < L);
        float v = src3[swz<NC>(ok ? ci : 0, ok ? n + shift : 0)];
        asm volatile("" : "+v"(v));  // keep the LDS read unconditional (no branch + wait per element)
        b[ni] = ok ? v : 0.f;
      }
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], b[ni], acc[mi][ni], 0, 0, 0);
      cib += 4;
      if (cib >= cin) {
        cib = 0;
        ++dk;
      }
    }
  }
}

template <int NC, int MT, int NT>
__device__ __forceinline__ void store_tiles(const Ctx &c, const f32x4 (&acc)[MT][NT], int mt0, int nt0, float *dst,
                                            int cout, int act) {
  const int col = c.lane & 15, kq = c.lane >> 4;
  lds_f *d3 = (lds_f *)dst;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * (mt0 + mi) + 4 * kq + r;
      if (row < cout) {
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const float v = acc[mi][ni][r];
          d3[swz<NC>(row, 16 * (nt0 + ni) + col)] = act ? fmaxf(v, 0.f) : v;
        }
      }
    }
  }
}

// GroupNorm fused into the conv epilogue (Block: proj -> GroupNorm -> [scale/shift] -> SiLU,
// resnets.py:104-122; ResnetBlock: time/cond MLP -> (scale, shift), residual add, :125-151).
// The rows of a group always sit inside one wave's accumulators (4 groups; a wave owns a quarter of
// the rows, or part of its single m-tile on narrow levels), so the statistics are reductions over
// registers: in-lane over tiles and the 4 rows of a lane, DPP over the columns of the sample,
// permlane swaps over the row quarters.  The scale/shift rows are not a table either: each wave
// computes the ones for its own output rows with a few MFMAs against G (the per-sample embedding sum
// in LDS) right here, in the accumulator layout of the conv tile.  No LDS round trip, no barrier.
struct GnEpilogue {
  int mode;            // 0: plain conv, 1: dst = act(GN(conv)), 2: res += act(GN(conv))
  int gamma_off, beta_off;
  int ss_w, ss_b, E;   // packed [2C x E] scale/shift Linear (A fragments) + combined bias, or ss_w < 0
  int C, cpg;          // channels, channels per group (1, 4, 8, 16 or the rows of a wave)
  float *res;          // residual stream (mode 2)
  int tab_off = 0;     // this ResnetBlock's rows in the per-cloud scale/shift table (Ctx::ss_row)
};

// One wave's share of a GEMM: PASSES x MT m-tiles by NT n-tiles, one k-sweep per pass.  Passes keep
// the register footprint of a sweep small (MT * TAPS <= 6 fragments per block) so that every variant
// fits beside the other phases of the kernel without spilling; the extra cost of a pass is one
// pipeline fill.  The bias is folded into the accumulator start value.
template <int NC, int L, int TAPS, int MT, int NT, int PASSES>
__device__ __forceinline__ void gemm_passes(const Ctx &c, const float *wp, int mt0, int nt0, bool active,
                                            const float *src, int cin, float *dst, int cout, const float *bias,
                                            bool alias, int act, const GnEpilogue &g) {
  using GG = Geo<NC>;
  f32x4 acc[PASSES][MT][NT];
  const int kq = c.lane >> 4, col = c.lane & 15;
  // ---- parameters of the GroupNorm epilogue.  Every load goes out in one batch: before the k-sweep when the
  // variant is a single pass (registers to spare: the round trip hides behind the GEMM), else at the start of
  // the epilogue, in the shadow of the statistics.
  constexpr bool kEarlyParams = TAPS == 3 && NC == 32 && PASSES == 1;
  const bool has_ss = g.ss_w >= 0;
  const bool wide = g.C >= 16;  // else C = 4: one m-tile holds scale rows 0..3 (row quarter 0) and shift rows 4..7
  const int ekb = g.E >> 4;
  const WStream wss(c.w + (has_ss ? g.ss_w : 0), c.lane);
  f32x4 ga[PASSES][MT], be[PASSES][MT], sc0[PASSES][MT], sh0[PASSES][MT], a_sc[PASSES][MT], a_sh[PASSES][MT];
#define GLDM_LOAD_GN_PARAMS()                                                                                       \
  _Pragma("unroll") for (int p = 0; p < PASSES; ++p) _Pragma("unroll") for (int mi = 0; mi < MT; ++mi) {            \
    const int mt_ = mt0 + p * MT + mi;                                                                              \
    const int row0_ = 16 * mt_ + 4 * kq;                                                                            \
    const int prow_ = row0_ + 3 < cout ? row0_ : 0; /* rows past cout (narrow levels) are not stored */             \
    ga[p][mi] = *reinterpret_cast<const f32x4 *>(c.w + g.gamma_off + prow_);                                        \
    be[p][mi] = *reinterpret_cast<const f32x4 *>(c.w + g.beta_off + prow_);                                         \
    sc0[p][mi] = f32x4{1.f, 1.f, 1.f, 1.f};                                                                         \
    sh0[p][mi] = f32x4{0.f, 0.f, 0.f, 0.f};                                                                         \
    if (has_ss) {                                                                                                   \
      const float *sb_ = c.w + g.ss_b;                                                                              \
      if (wide) { /* scale rows: m-tile mt, shift rows: m-tile C/16 + mt of the [2C x E] Linear */                  \
        sc0[p][mi] = *reinterpret_cast<const f32x4 *>(sb_ + row0_);                                                 \
        sh0[p][mi] = *reinterpret_cast<const f32x4 *>(sb_ + g.C + row0_);                                           \
        a_sc[p][mi] = wss[(size_t)mt_ * ekb * 64];                                                                  \
        a_sh[p][mi] = wss[(size_t)((g.C >> 4) + mt_) * ekb * 64];                                                   \
      } else {                                                                                                      \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) sc0[p][mi][r] = sb_[4 * kq + r < 2 * g.C ? 4 * kq + r : 0];   \
        a_sc[p][mi] = wss[0];                                                                                       \
      }                                                                                                             \
    }                                                                                                               \
  }
  if (kEarlyParams && g.mode && active) { GLDM_LOAD_GN_PARAMS() }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (bias) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * (mt0 + p * MT + mi) + 4 * kq + r;
          bv[r] = bias[row < cout ? row : cout - 1];
        }
      }
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) acc[p][mi][ni] = bv;
    }
    if (active) {
      if ((cin & 15) == 0) gemm_fast<NC, L, TAPS, MT, NT>(c, wp, cin >> 4, mt0 + p * MT, nt0, src, acc[p]);
      else gemm_small<NC, L, MT, NT>(c, wp, (TAPS * cin + 15) >> 4, mt0 + p * MT, nt0, src, cin, TAPS, acc[p]);
    }
  }
  if constexpr (TAPS == 3 && NC == 32) {
    if (g.mode) {
      if (!active) return;
      const float inv_cnt = 1.0f / (float)(g.cpg * L);  // a power of two: exact
      lds_f *d3 = (lds_f *)(g.mode == 2 ? g.res : dst);
      if (!kEarlyParams) { GLDM_LOAD_GN_PARAMS() }
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int n = 16 * (nt0 + ni) + col;
        const lds_f *Gs = (const lds_f *)(c.lds + GG::kMiscG) + (n / L) * g.E;  // this column's sample
        // ---- statistics
        float mean[PASSES][MT][4], rstd[PASSES][MT][4];
        if (g.cpg >= 32) {  // the group is everything this wave accumulates
          float s1 = 0.f;
#pragma unroll
          for (int p = 0; p < PASSES; ++p)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
              for (int r = 0; r < 4; ++r) s1 += acc[p][mi][ni][r];
          s1 = half_sum(row_pair_sum(group_sum<L>(s1)));
          const float m = s1 * inv_cnt;
          float s2 = 0.f;
#pragma unroll
          for (int p = 0; p < PASSES; ++p)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float dx = acc[p][mi][ni][r] - m;
                s2 += dx * dx;
              }
          s2 = half_sum(row_pair_sum(group_sum<L>(s2)));
          const float rs = __builtin_amdgcn_rsqf(s2 * inv_cnt + 1e-5f);
#pragma unroll
          for (int p = 0; p < PASSES; ++p)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                mean[p][mi][r] = m;
                rstd[p][mi][r] = rs;
              }
        } else {
#pragma unroll
          for (int p = 0; p < PASSES; ++p)
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
              if (g.cpg == 1) {  // every accumulator row is its own group
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float x = acc[p][mi][ni][r];
                  const float m = group_sum<L>(x) * inv_cnt;
                  const float dx = x - m;
                  mean[p][mi][r] = m;
                  rstd[p][mi][r] = __builtin_amdgcn_rsqf(group_sum<L>(dx * dx) * inv_cnt + 1e-5f);
                }
              } else {  // 4, 8 or 16 rows of this m-tile: the lane's 4 rows, then row quarters
                float s1 = acc[p][mi][ni][0] + acc[p][mi][ni][1] + acc[p][mi][ni][2] + acc[p][mi][ni][3];
                s1 = group_sum<L>(s1);
                if (g.cpg >= 8) s1 = row_pair_sum(s1);
                if (g.cpg >= 16) s1 = half_sum(s1);
                const float m = s1 * inv_cnt;
                float s2 = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float dx = acc[p][mi][ni][r] - m;
                  s2 += dx * dx;
                }
                s2 = group_sum<L>(s2);
                if (g.cpg >= 8) s2 = row_pair_sum(s2);
                if (g.cpg >= 16) s2 = half_sum(s2);
                const float rs = __builtin_amdgcn_rsqf(s2 * inv_cnt + 1e-5f);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  mean[p][mi][r] = m;
                  rstd[p][mi][r] = rs;
                }
              }
            }
        }
        // ---- scale/shift rows of this column's sample, normalise, SiLU, store / accumulate
        float gb[4];
        if (has_ss) {
#pragma unroll
          for (int j = 0; j < 4; ++j) gb[j] = Gs[4 * j + kq];
        }
#pragma unroll
        for (int p = 0; p < PASSES; ++p)
#pragma unroll
          for (int mi = 0; mi < MT; ++mi) {
            const int mt = mt0 + p * MT + mi;
            const int row0 = 16 * mt + 4 * kq;
            f32x4 sc = sc0[p][mi], sh = sh0[p][mi];
            const float *tab = L == 16 ? (((nt0 + ni) & 1) ? c.ss_row[1] : c.ss_row[0]) : nullptr;  // wave uniform (a select: a run-time index keeps Ctx in scratch)
            if (has_ss && wide && tab) {
              // The pose decoder's embedding does not depend on the grasp: the rows were computed once per cloud
              // (ss_table_kernel).  In here they cost 32 MFMAs per m-tile and SAMPLE (E = 64), 17 % on top of a
              // 256-wide conv's own, 15 of every n-tile's 16 columns repeating the first.
              sc = *reinterpret_cast<const f32x4 *>(tab + g.tab_off + row0);
              sh = *reinterpret_cast<const f32x4 *>(tab + g.tab_off + g.C + row0);
            } else if (has_ss) {
              if (wide) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_sc[p][mi][j], gb[j], sc, 0, 0, 0);
                  sh = __builtin_amdgcn_mfma_f32_16x16x4f32(a_sh[p][mi][j], gb[j], sh, 0, 0, 0);
                }
                // (E = 64, the pose decoder: 32 of these per m-tile and sample, 17 % on top of a 256-wide conv's own
                // MFMAs -- a 16-column n-tile is ONE sample there, so 15 of its 16 columns repeat the first.  Requesting
                // the kb >= 1 fragments together instead of one round trip each changed nothing: it is MFMA time.)
                for (int kb = 1; kb < ekb; ++kb) {  // wide embeddings
                  const f32x4 a2 = wss[((size_t)mt * ekb + kb) * 64], a3 = wss[((size_t)((g.C >> 4) + mt) * ekb + kb) * 64];
#pragma unroll
                  for (int j = 0; j < 4; ++j) {
                    const float bj = Gs[16 * kb + 4 * j + kq];
                    sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j], bj, sc, 0, 0, 0);
                    sh = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[j], bj, sh, 0, 0, 0);
                  }
                }
              } else {
                f32x4 t = sc;
#pragma unroll
                for (int j = 0; j < 4; ++j) t = __builtin_amdgcn_mfma_f32_16x16x4f32(a_sc[p][mi][j], gb[j], t, 0, 0, 0);
                for (int kb = 1; kb < ekb; ++kb) {
                  const f32x4 a2 = wss[(size_t)kb * 64];
#pragma unroll
                  for (int j = 0; j < 4; ++j) t = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j], Gs[16 * kb + 4 * j + kq], t, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(t[r]), __float_as_uint(t[r]), false, false);
                  sc[r] = t[r];                    // valid in row quarter 0, the only one that is stored
                  sh[r] = __uint_as_float(sw[1]);  // quarter 1's value seen from quarter 0
                }
              }
            }
            // the four values of the lane, without wave-uniform branches between them (mode, scale/shift and the row
            // bound are tested once per m-tile: tested per value they cut the exp / rcp chains into basic blocks)
            auto finish4 = [&](auto mode_c, auto ss_c, auto full_c) {
              constexpr int kMode = decltype(mode_c)::value;
              constexpr bool kSS = decltype(ss_c)::value, kFull = decltype(full_c)::value;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                float y = (acc[p][mi][ni][r] - mean[p][mi][r]) * rstd[p][mi][r] * ga[p][mi][r] + be[p][mi][r];
                if (kSS) y = y * sc[r] + sh[r];
                y = silu(y);
                if (kFull || row0 + r < cout) {
                  const int a = swz<NC>(row0 + r, n);
                  d3[a] = kMode == 2 ? d3[a] + y : y;
                }
              }
            };
            using std::integral_constant;
            typedef integral_constant<bool, true> T;
            typedef integral_constant<bool, false> F;
            const bool full = row0 + 3 < cout;
            if (g.mode == 2) {
              if (has_ss) { if (full) finish4(integral_constant<int, 2>{}, T{}, T{}); else finish4(integral_constant<int, 2>{}, T{}, F{}); }
              else { if (full) finish4(integral_constant<int, 2>{}, F{}, T{}); else finish4(integral_constant<int, 2>{}, F{}, F{}); }
            } else {
              if (has_ss) { if (full) finish4(integral_constant<int, 1>{}, T{}, T{}); else finish4(integral_constant<int, 1>{}, T{}, F{}); }
              else { if (full) finish4(integral_constant<int, 1>{}, F{}, T{}); else finish4(integral_constant<int, 1>{}, F{}, F{}); }
            }
          }
      }
      return;
    }
  }
  if (alias) __syncthreads();
  if (active) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) store_tiles<NC, MT, NT>(c, acc[p], mt0 + p * MT, nt0, dst, cout, act);
  }
}

#undef GLDM_LOAD_GN_PARAMS

// The k = 3 convs of the 64-column engines belong to the ResNet1D engine alone: resnet1d.hip defines them.  conv_gemm only
// names them, in the ktaps == 3 branch of its 64-column half; a source that passes ktaps = 1 as a constant (the set
// abstraction's 1x1 layers) compiles that branch away and carries no definition, hence the silenced warning.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-internal"
struct NoHook { __device__ __forceinline__ void operator()() const {} };
template <int MT, int P0, int NP, int GK, int FIN, class PRE, class HOOK, int LL>
__device__ __forceinline__ void conv_pm3_wave(const Ctx &c, const float *wp, const float *bias, int mt0,
                                              const float *src, int cin, float *dst, int cout, bool alias,
                                              const GnEpilogue &g, const PRE &pre = PRE(), const HOOK &hook = HOOK(),
                                              bool live = true);
__device__ __forceinline__ void conv_pm3_cin4(const Ctx &c, const float *wp, const float *bias, const float *src,
                                              float *dst, int cout, bool alias);
#pragma clang diagnostic pop

// dst[cout][NC] = W * im2col(src[cin][NC]) + bias: the waves split the output rows (all n-tiles each).
// Ends with a barrier.  alias: dst overlaps src -> all reads complete (barrier) before any store.
// Output widths are 16 x {1, 2, 4, 8, 12, 16} rows (validate() enforces it).
// (Tried and dropped: running the <= 64-channel levels column-parallel, one wave per n-tile with no
// barriers inside the level: those phases are bound by per-wave issue, not by the barriers, and with
// half the waves active every op took 1.7-2x longer.  And the opposite, 8 waves per 32-column tile
// with the statistics of a wide group exchanged between wave pairs: correct, but at 128 VGPRs per
// wave the k-loops spill and the launch was 5-7 % slower than with 4 waves.)
template <int NC, int L>
__device__ __forceinline__ void conv_gemm(const Ctx &c, int w_off, int b_off, const float *src, int cin, int ktaps,
                                          float *dst, int cout, bool alias, int act = 0,
                                          const GnEpilogue &g = GnEpilogue{0, 0, 0, -1, 0, 0, 0, 0, nullptr}) {
  if (GLDM_SKIP(c, 8)) return;
  const float *wp = c.w + w_off;
  const float *bias = b_off >= 0 ? c.w + b_off : nullptr;
  const int mtiles = (cout + 15) >> 4;
  const int w = c.wave;
  // G3: k = 3 taps (<= 2 m-tiles per sweep), G1: 1x1
#define GLDM_G3(MT, NT, P, mt0, nt0, on) gemm_passes<NC, L, 3, MT, NT, P>(c, wp, mt0, nt0, on, src, cin, dst, cout, bias, alias, act, g)
#define GLDM_G1(MT, NT, P, mt0, nt0, on) gemm_passes<NC, L, 1, MT, NT, P>(c, wp, mt0, nt0, on, src, cin, dst, cout, bias, alias, act, g)
  if constexpr (NC == 64) {
    if (ktaps == 3) {
      // 64-column engines: 8 waves share the m-tiles (L = 4: the three taps tie the 4 position tiles together; L = 16:
      // tiles of 4 positions x 4 samples, taps by shifted plane reads).  Only the levels' down convs come this way.
      constexpr int LL = L == 16 ? 16 : 4;
      if (LL == 4 && (cin & 15)) conv_pm3_cin4(c, wp, bias, src, dst, cout, alias);
      else if (mtiles == 16) conv_pm3_wave<2, 0, 4, 0, 0, NoPreA, NoHook, LL>(c, wp, bias, 2 * w, src, cin, dst, cout, alias, g);
      else if (mtiles == 8) conv_pm3_wave<1, 0, 4, 0, 0, NoPreA, NoHook, LL>(c, wp, bias, w, src, cin, dst, cout, alias, g);
      else if (mtiles == 4) {
        if (w < 4) conv_pm3_wave<1, 0, 2, 1, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 3, src, cin, dst, cout, alias, g);
        else conv_pm3_wave<1, 2, 2, 1, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 3, src, cin, dst, cout, alias, g);
      } else {  // 2 m-tiles: wave = (m-tile, position / tile)
        const int pw = w >> 1;
        if (pw == 0) conv_pm3_wave<1, 0, 1, 2, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 1, src, cin, dst, cout, alias, g);
        else if (pw == 1) conv_pm3_wave<1, 1, 1, 2, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 1, src, cin, dst, cout, alias, g);
        else if (pw == 2) conv_pm3_wave<1, 2, 1, 2, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 1, src, cin, dst, cout, alias, g);
        else conv_pm3_wave<1, 3, 1, 2, 0, NoPreA, NoHook, LL>(c, wp, bias, w & 1, src, cin, dst, cout, alias, g);
      }
    }
    // 1x1 layers (layout agnostic): 8 waves x 4 n-tiles; also the fused set abstraction
    else if (mtiles == 16) GLDM_G1(2, 4, 1, 2 * w, 0, true);
    else if (mtiles == 12) GLDM_G1(3, 2, 1, 3 * (w & 3), 2 * (w >> 2), true);
    else if (mtiles == 8) GLDM_G1(1, 4, 1, w, 0, true);
    else if (mtiles == 4) GLDM_G1(1, 2, 1, w & 3, 2 * (w >> 2), true);
    else if (mtiles == 2) GLDM_G1(1, 1, 1, w & 1, w >> 1, true);
    else GLDM_G1(1, 1, 1, 0, w & 3, w < 4);
  } else if (ktaps == 3) {
    if (c.nta == 1) {  // tail workgroup: only columns 0..15 are live
      if (mtiles == 16) GLDM_G3(2, 1, 2, 4 * w, 0, true);
      else if (mtiles == 12) GLDM_G3(1, 1, 3, 3 * w, 0, true);
      else if (mtiles == 8) GLDM_G3(2, 1, 1, 2 * w, 0, true);
      else GLDM_G3(1, 1, 1, w < mtiles ? w : 0, 0, w < mtiles);
    } else if (mtiles == 16) GLDM_G3(2, 2, 2, 4 * w, 0, true);
    else if (mtiles == 12) GLDM_G3(1, 2, 3, 3 * w, 0, true);
    else if (mtiles == 8) GLDM_G3(2, 2, 1, 2 * w, 0, true);
    else if (mtiles == 4) GLDM_G3(1, 2, 1, w, 0, true);
    else if (mtiles == 2) GLDM_G3(1, 1, 1, w & 1, w >> 1, true);
    else GLDM_G3(1, 1, 1, 0, w & 1, w < 2);
  } else {
    if (c.nta == 1) {
      if (mtiles == 16) GLDM_G1(4, 1, 1, 4 * w, 0, true);
      else if (mtiles == 12) GLDM_G1(3, 1, 1, 3 * w, 0, true);
      else if (mtiles == 8) GLDM_G1(2, 1, 1, 2 * w, 0, true);
      else GLDM_G1(1, 1, 1, w < mtiles ? w : 0, 0, w < mtiles);
    } else if (mtiles == 16) GLDM_G1(4, 2, 1, 4 * w, 0, true);
    else if (mtiles == 12) GLDM_G1(3, 2, 1, 3 * w, 0, true);
    else if (mtiles == 8) GLDM_G1(2, 2, 1, 2 * w, 0, true);
    else if (mtiles == 4) GLDM_G1(1, 2, 1, w, 0, true);
    else if (mtiles == 2) GLDM_G1(1, 1, 1, w & 1, w >> 1, true);
    else GLDM_G1(1, 1, 1, 0, w & 1, w < 2);
  }
#undef GLDM_G3
#undef GLDM_G1
  __syncthreads();
}

}  // namespace
