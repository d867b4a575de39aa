// mfma_prims.h -- the primitives every MFMA kernel source shares: the bottom of three layers (tile_gemm.h, the tile GEMMs of
// sa_mlp.hip / pointwise_mlp.hip / resnet1d.hip, is built on it; r1d_gemm.h, the ResNet1D engine's own part, on that).
// Device code only, __forceinline__ in an anonymous namespace: nothing here is a symbol.
//   * GLDM_API (the exported entry points), vector and LDS pointer types, the LinearAttention constants;
//   * split-f16 arithmetic: an f32 operand travels as hi + lo f16 (kSplit = 2), a product is three v_mfma_f32_16x16x32_f16
//     (mfma_split); split_f16x2 / split_planes8 make the planes, range_pow2 / pow2_inv their range scale;
//   * fast_exp, silu; cross-lane reductions on the VALU (DPP, permlane swaps), and over all 64 lanes by shuffles (wave_max,
//     wave_sum);
//   * wstream.h (weight fragments L2 -> VGPR) and devstate.h come with it.
// Included directly by conv3d.hip, voxel_norm.hip, pointwise_small.hip, unet1d.hip, point_attention.hip,
// point_attention_fused.hip and grasp_classifier.hip, which take nothing above it (point_ops.hip, neighbors.hip,
// voxel_points.hip, fps.hip and sa_msg.hip take host_util.h instead).  It includes no other header of this directory than the
// three named here, and holds no LDS map, no launch context and no matrix product larger than one instruction group.
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

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((address_space(3))) float lds_f;   // explicit LDS pointers: 32-bit ds_* addressing
typedef __attribute__((address_space(3))) f32x4 lds_f4;

constexpr int kHeads = 4, kDimHead = 32, kHidden = kHeads * kDimHead;  // LinearAttention defaults

// Split operands (see "split-f16 products" below): every f32 value travels as kSplit = 2 f16 numbers, hi + lo.
constexpr int kSplit = 2;
constexpr int kFragBytes = kSplit * 1024;        // one weight fragment: [plane][lane 64][8 f16]
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((address_space(3))) u32x4 lds_u4;
typedef __attribute__((address_space(3))) u32x2_t lds_u2;
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

// ---- split-f16 products ------------------------------------------------------------------------------------------------
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
// (store_planes4 of tile_gemm.h) or as they are read from LDS (split_planes8).  Range: |x| < 65504 (f16); the packers refuse weights
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

}  // namespace
