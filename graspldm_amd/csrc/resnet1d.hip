// resnet1d.hip -- the fused 1-D ResNet engine of GraspLDM on gfx950 and the small ops either side:
//   * gldm_denoise[_rng] : the whole reverse-diffusion loop (T steps of TimeConditionedResNet1D.forward + the scheduler
//                          update) in ONE launch; the latent never leaves the chip between steps;
//   * gldm_decode        : ConditionalGraspPoseDecoder.forward (in_layer, ResNet1D, tmrp / class_logits heads);
//   * gldm_encode        : GraspCVAE.encode (in_layer, ResNet1D, out_layer folded into mu / logvar, reparameterisation);
//   * gldm_r1d_cond_embed, gldm_pose_prologue, gldm_pose_epilogue, gldm_step_noise_rng; ss_table_kernel (the per-cloud
//     scale / shift table of nets without a time embedding) runs in front of decode / encode.
// One kernel template, r1d_kernel<NC, L>: a workgroup owns NC activation columns = NC / L samples x L positions and walks
// every layer with the activations resident in LDS; weights (standardised, folded and laid out in fragment order by
// r1d_pack.py) stream L2 -> VGPR.  GroupNorm, the time / condition scale-shift, SiLU and the residual add live in the conv
// epilogues; LinearAttention at n = L is reassociated, out = V (K^T Q); persistent workgroups splice the left-over tiles'
// steps between them over {value, tag} granules in global memory (the chain).  Four instantiations:
//   <64, 4>   the shipped latent denoiser: 8 waves, one workgroup per CU, position-major columns (16 position + sample: a
//             k = 3 tap is the neighbouring n-tile), GEMMs on the f16 matrix pipe through the hi + lo split with the B
//             operands in LDS as pre-split planes (conv_pm3_wave, gemm_pm3_pl); a ResnetBlock is one op; the 4 / 32 /
//             64-channel levels are one wave-local op in registers (quad_narrow.h).
//   <64, 16>  the shipped pose decoder, grasp encoder and 16-position denoiser: column = 4 position + sample, zero-padded
//             plane rows so that taps are shifted reads (gemm_sm3_pl); narrow levels in quad16_narrow.h, qkv_att16_pm.
//   <32, *>   the f32 engine (numerics.f32_only(), and every descriptor outside pm_supported() / pm16_supported()): 4 waves,
//             two workgroups per CU, sample-major columns, v_mfma_f32_16x16x4_f32 through mfma_core.h's conv_gemm.
// The step is a tape of ops built on the host (build_tape) and interpreted by run_tape with every phase inlined: in the
// kernel arguments (RunArgs::pm_tape) for the 64-column engines, built in LDS by the 32-column one.
// Device code first (engine pieces, the network, r1d_kernel, the small kernels), then the host side, then the entry points.
#include "mfma_core.h"

namespace {

constexpr int kMaxSegs = 64;  // tiles (+ one spliced step segment) a persistent workgroup can be given
constexpr int kPlaneH = 128 * 64;                 // H planes: floats [8192, 16384): 4 blocks of 32 channels
constexpr int kPlaneX = kPlaneH + 4 * kSplit * 1024;   // X planes: floats [16384, 24576)
constexpr int kPlaneMaxC = 128;
// The 256-channel level (only ever the last one: a down conv into it and one ResnetBlock) keeps ONE tensor in LDS as
// planes (8 blocks x 8 KiB = 64 KiB, floats [16384, 32768): behind the level's f32 residual stream X, rows 0..255 =
// floats [0, 16384)): the down conv writes the planes of the new residual stream X there (and X itself as f32 rows);
// conv1 reads the planes and, behind its GroupNorm exchange barrier (every wave is past its k-loop), overwrites them with
// the planes of H; conv2 reads those and adds act(GN(conv)) to the f32 rows for the final 1x1.
static_assert(PG<4>::kH == kPlaneH && PG<4>::kX == kPlaneX, "plane regions");
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_WAVE_STAMPS)   // per-wave conv stamps cost ~1.5 k cycles per op: their own switch
__device__ long long g_wv_stamp[8][32][8];   // per wave, ring of the last 32 position-major convs: in, k-loop done, out, shape,
                                             // statistics published (in front of the exchange barrier), partners merged
__device__ int g_wv_cnt[8];
#define GLDM_WV_STAMP(c, k, v) \
  do { if (blockIdx.x == 0 && (c).lane == 0) g_wv_stamp[(c).wave][g_wv_cnt[(c).wave] & 31][k] = (v); } while (0)
#define GLDM_WV_NEXT(c) do { if (blockIdx.x == 0 && (c).lane == 0) g_wv_cnt[(c).wave]++; } while (0)
#else
#define GLDM_WV_STAMP(c, k, v) do {} while (0)
#define GLDM_WV_NEXT(c) do {} while (0)
#endif

// Position-major k = 3 conv on split-f16 operands.  wp3: split fragments
// of [Cout x 3 Cin], k = tap * Cin + ci, 32-deep k-blocks (Cin % 32 == 0).  One set of A registers per tap: the
// moment a tap's MFMAs have issued, its registers are refilled with the next channel block's fragments of that tap,
// which then have the two other taps' MFMAs (and the partner wave's) to arrive.  The raw f32 B values of the next
// block are read from LDS while the current block's MFMAs run and split at the top of the next trip.
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_NO_A)   // timing experiments only (wrong results): operands of block 0 reused
constexpr bool kExpNoA = true;
#else
constexpr bool kExpNoA = false;
#endif
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_NO_B)
constexpr bool kExpNoB = true;
#else
constexpr bool kExpNoB = false;
#endif
// First weight fragments of a position-major k = 3 conv, requested by the CALLER ahead of the conv (the fused
// ResnetBlock op asks for its second conv's while the first conv's epilogue runs): block 0's three tap sets of a
// one-m-tile wave, tap 0's set of a two-m-tile wave -- what the k-loop would otherwise request cold and wait ~1 k cycles for.
template <int MT>
struct PreA {
  static constexpr bool on = true;
  static constexpr int kSets = MT == 1 ? 3 : 1;
  u32x4 a[kSets][MT][kSplit];
  __device__ __forceinline__ void request(const WStream &wv, int mt0, int cin) {
    const int kb32 = cin >> 5, kblocks = 3 * kb32;
#pragma unroll
    for (int t = 0; t < kSets; ++t)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int pl = 0; pl < kSplit; ++pl) a[t][mi][pl] = wv.raw_at(((mt0 + mi) * kblocks + t * kb32) * kFragBytes, pl * 1024);
  }
};

// The conv with the B operand read from pre-split planes: ds_read_b128 per (tile, plane), no VALU.
// B planes of the next channel block are requested while the current block's MFMAs run (second register set).
template <int MT, int P0, int NP, class PRE = NoPreA>
__device__ __forceinline__ void gemm_pm3_pl(const Ctx &c, const float *__restrict__ wp3, int cin, int mt0,
                                            const float *planes, f32x4 (&acc)[MT][NP], const PRE &pre = PRE()) {
  constexpr int PB0 = P0 > 0 ? P0 - 1 : 0, PB1 = P0 + NP < 4 ? P0 + NP : 3, NB = PB1 - PB0 + 1;
  const int col = c.lane & 15, g = c.lane >> 4;
  const int kb32 = cin >> 5, kblocks = 3 * kb32;
  const WStream wv(wp3, c.lane);
  const lds_u4 *pl3 = (const lds_u4 *)planes + g * 64 + 16 * PB0 + col;   // + (kb * kSplit + plane) * 256 + 16 q
  // A registers.  One m-tile per wave: a set per tap, refilled with the next block's fragments right after the tap's
  // MFMAs (a whole block to arrive).  Two m-tiles: 72 registers that way, so two sets alternate over the tap steps
  // instead (the next step's fragments are requested in front of the current step's MFMAs: 36-48 of them, and the
  // partner wave's, to arrive); the trip covers two blocks so that the alternation is static.
  constexpr int NA = MT == 1 ? 3 : 2;
  constexpr int NBUF = (MT == 1 && NB <= 3) ? 2 : 1;   // 4 tiles x 2 sets = 96 registers: spills
  u32x4 a[NA][MT][kSplit];
  u32x4 bs[NBUF][NB][kSplit];
  auto load_a = [&](int buf, int t, int kb) {
    if (kExpNoA && kb > 0) return;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl)
        a[buf][mi][pl] = wv.raw_at(((mt0 + mi) * kblocks + t * kb32 + kb) * kFragBytes, pl * 1024);
  };
  auto load_b = [&](int buf, int kb) {
    if (kExpNoB && kb > 0) return;
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) bs[buf][q][pl] = pl3[(kb * kSplit + pl) * 256 + 16 * q];
  };
  auto tap_mfmas = [&](int abuf, int bbuf, int t) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int sp = P0 + p + t - 1;
        if (sp >= 0 && sp <= 3) {
          const int qi = sp - PB0 < 0 ? 0 : (sp - PB0 >= NB ? NB - 1 : sp - PB0);
          acc[mi][p] = mfma_split(a[abuf][mi], bs[bbuf][qi], acc[mi][p]);
        }
      }
  };
  const int last = kb32 - 1;
  load_b(0, 0);
  auto first_a = [&]() {   // block 0's fragments (three tap sets, or tap 0's with two m-tiles): the caller's, or requested here
#pragma unroll
    for (int t = 0; t < (MT == 1 ? 3 : 1); ++t) {
      if constexpr (PRE::on) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int pl = 0; pl < kSplit; ++pl) a[t][mi][pl] = pre.a[t][mi][pl];
      } else {
        load_a(t, t, 0);
      }
    }
  };
  if constexpr (MT == 1) {
    first_a();
    auto block = [&](int bbuf, int nb) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        __builtin_amdgcn_sched_barrier(0);
        tap_mfmas(t, bbuf, t);
        __builtin_amdgcn_sched_barrier(0);
        load_a(t, t, nb);
      }
    };
    if (kb32 == 1) {
      block(0, 0);
      return;
    }
    if constexpr (NBUF == 2) {
      for (int kb0 = 0; kb0 < kb32; kb0 += 2) {   // kb32 is 2 or 4 here: the two sets of B planes alternate statically
        load_b(1, kb0 + 1);
        block(0, kb0 + 1);
        load_b(0, kb0 + 2 < last ? kb0 + 2 : last);
        block(NBUF - 1, kb0 + 2 < last ? kb0 + 2 : last);
      }
    } else {
      for (int kb = 0; kb < kb32; ++kb) {
        if (kb) load_b(0, kb);
        block(0, kb < last ? kb + 1 : last);
      }
    }
  } else {
    first_a();
    auto step = [&](int st, int kb0) {
        const int t = st % 3, kb = kb0 + st / 3;
        const int nt = (st + 1) % 3, nkb = kb0 + (st + 1) / 3;
        if (t == 0 && kb > 0) load_b(0, kb);
        load_a((st + 1) & 1, nt, nkb < last ? nkb : last);
        __builtin_amdgcn_sched_barrier(0);
        tap_mfmas(st & 1, 0, t);
        __builtin_amdgcn_sched_barrier(0);
    };
    if (kb32 == 1) {
      step(0, 0); step(1, 0); step(2, 0);
    } else {
      for (int kb0 = 0; kb0 < kb32; kb0 += 2) {
#pragma unroll
        for (int st = 0; st < 6; ++st) step(st, kb0);
      }
    }
  }
}

// k = 3 conv of the 16-position engine (LL = 16: column = 4 * position + sample).  A tap is the same B read shifted by
// one position = 4 entries of the zero-padded plane rows (PG<16>): no masks, and no (tap, position) product is padding
// except at a sample's two end positions (46 of 48 are real).  Every (tap, tile) has its own B fragments, read from LDS
// in front of the MFMAs they feed: one m-tile per wave -> the next tap step's set while the current one multiplies (two
// register sets; the trip covers two channel blocks so that the alternation is static); two m-tiles (256 channels) -> tile
// by tile, the next tile's planes under the current tile's 12 MFMAs.  A fragments exactly as in gemm_pm3_pl.
// T0, NT: the wave's n-tiles (tile = 4 consecutive positions x 4 samples).  Cin = 16 runs as one 32-channel block whose
// upper half has zero weights (r1d_pack.pad_cin32).
template <int MT, int T0, int NT, class PRE = NoPreA>
__device__ __forceinline__ void gemm_sm3_pl(const Ctx &c, const float *__restrict__ wp3, int cin, int mt0,
                                            const float *planes, f32x4 (&acc)[MT][NT], const PRE &pre = PRE()) {
  using G = PG<16>;
  const int col = c.lane & 15, g = c.lane >> 4;
  const int kb32 = (cin + 31) >> 5, kblocks = 3 * kb32;
  const WStream wv(wp3, c.lane);
  const lds_u4 *pl3 = (const lds_u4 *)planes + g * G::kCols + 16 * T0 + col;   // + (kb * kSplit + plane) * kPlaneU4 + 16 q + 4 t
  constexpr int NA = MT == 1 ? 3 : 2;
  u32x4 a[NA][MT][kSplit];
  auto load_a = [&](int buf, int t, int kb) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl)
        a[buf][mi][pl] = wv.raw_at(((mt0 + mi) * kblocks + t * kb32 + kb) * kFragBytes, pl * 1024);
  };
  auto first_a = [&]() {   // block 0's fragments (three tap sets, or tap 0's with two m-tiles): the caller's, or requested here
#pragma unroll
    for (int t = 0; t < (MT == 1 ? 3 : 1); ++t) {
      if constexpr (PRE::on) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int pl = 0; pl < kSplit; ++pl) a[t][mi][pl] = pre.a[t][mi][pl];
      } else {
        load_a(t, t, 0);
      }
    }
  };
  const int last = kb32 - 1;
  if constexpr (MT == 1) {
    // ONE rolling set of B fragments: the moment a tile's six MFMAs of a tap step have issued, its registers are refilled
    // with the same tile's planes of the NEXT tap step, which then have the other tiles' MFMAs to arrive (two full sets
    // were 96 registers at four tiles: spills inside the loop)
    u32x4 bs[NT][kSplit];
    auto load_b1 = [&](int q, int kb, int t) {
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) bs[q][pl] = pl3[(kb * kSplit + pl) * G::kPlaneU4 + 16 * q + 4 * t];
    };
#pragma unroll
    for (int q = 0; q < NT; ++q) load_b1(q, 0, 0);
    first_a();
    // st: tap step inside a trip of two blocks (0..5); A set = tap
    auto step = [&](int st, int kb0) {
      const int t = st % 3, kb = kb0 + st / 3;
      const int nt = (st + 1) % 3, nkb0 = kb0 + (st + 1) / 3, nkb = nkb0 < last ? nkb0 : last;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        __builtin_amdgcn_sched_barrier(0);
        acc[0][q] = mfma_split(a[t][0], bs[q], acc[0][q]);
        __builtin_amdgcn_sched_barrier(0);
        load_b1(q, nkb, nt);
      }
      load_a(t, t, kb < last ? kb + 1 : last);
    };
    if (kb32 == 1) {
      step(0, 0); step(1, 0); step(2, 0);
    } else {
      for (int kb0 = 0; kb0 < kb32; kb0 += 2) {
#pragma unroll
        for (int st = 0; st < 6; ++st) step(st, kb0);
      }
    }
  } else {
    static_assert(MT == 1 || NT == 4, "two m-tiles per wave: all four tiles");
    u32x4 bs[2][kSplit];
    auto load_b1 = [&](int buf, int kb, int t, int q) {
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) bs[buf][pl] = pl3[(kb * kSplit + pl) * G::kPlaneU4 + 16 * q + 4 * t];
    };
    first_a();
    load_b1(0, 0, 0, 0);
    auto step = [&](int st, int kb0) {
      const int t = st % 3, kb = kb0 + st / 3;
      const int nt = (st + 1) % 3, nkb0 = kb0 + (st + 1) / 3, nkb = nkb0 < last ? nkb0 : last;
      load_a((st + 1) & 1, nt, nkb);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < 3) load_b1((q + 1) & 1, kb, t, q + 1);
        else load_b1(0, nkb, nt, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) acc[mi][q] = mfma_split(a[st & 1][mi], bs[q & 1], acc[mi][q]);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    for (int kb0 = 0; kb0 < kb32; kb0 += 2) {   // 4 or 8 blocks here
#pragma unroll
      for (int st = 0; st < 6; ++st) step(st, kb0);
    }
  }
}
constexpr int kOpInts = 12, kMaxOps = 84;  // op tape: 84 * 12 = 1008 ints; the op count lives in int 1023
constexpr int kPmMaxOps = 8 * GLDM_R1D_MAX_LEVELS + 2;   // 64-column engines: at most 8 entries per level + the last ResnetBlock's 2

// ==== Position-major engine pieces (L = 4, 64-column tiles = 16 samples x 4 positions, column = 16 * pos + sample,
// 8 waves, one workgroup per CU).  1x1 convs, LayerNorm and the final 1x1 are layout agnostic and shared with
// the sample-major engine; what follows are the layout-aware phases.

// One wave's share of a k = 3 conv: MT m-tiles x out positions P0..P0+NP-1, with the GroupNorm / scale-shift /
// SiLU / residual epilogue.  A group's rows no longer sit in one wave (8 waves share 16 m-tiles and the taps
// tie the 4 position tiles together), so the statistics are combined across waves: every wave reduces its own
// share to (sum, M2 about its own mean) per sample -- in-lane over its accumulators, permlane swaps over the
// row quarters -- publishes the pair in LDS, and after ONE barrier merges its partners' pairs with the
// parallel-variance formula (exact for equal counts, no E[x^2] - m^2 cancellation).
//   GK 0: partner = the adjacent wave (C = 256: 2 m-tiles per wave, C = 128: 1; all 4 positions)
//   GK 1: partner = wave ^ 4 (C = 64: one m-tile = one group, positions split in two halves)
//   GK 2: four waves (one per position) x two groups per m-tile (C = 32: 8 channels per group)
constexpr float sqrt_up(int n) {   // >= sqrt(n), n a power of two
  float r = 1.f;
  while (n >= 4) { r *= 2.f; n /= 4; }
  return n >= 2 ? r * 1.41422f : r;
}
// FIN: which epilogues this instance carries (code size: the kernel's straight-line phases must stay inside the instruction
// cache): 0 = none (the level's down conv, mode 0), 1 = block1 (H = act(GN(conv)), scale/shift at run time), 2 = block2
// (X += act(GN(conv)), no scale/shift).  Modes 1 and 2 only ever run inside the fused ResnetBlock op.
// LL: 4 = position-major tiles of the 4-position denoiser (P0 / NP: positions); 16 = the 16-position engine (P0 / NP: the
// wave's n-tiles of 4 positions x 4 samples; sample = lane & 3; GK 3: C = 16, one m-tile whose four row quarters are the
// four groups, waves 0-3 one tile each -- waves 4-7 repeat their work with `live` false so that every wave meets the
// barriers).  The statistics of a sample then also sum over the four positions inside a tile (DPP row rotations).
template <int MT, int P0, int NP, int GK, int FIN, class PRE, class HOOK, int LL>
__device__ __forceinline__ void conv_pm3_wave(const Ctx &c, const float *wp, const float *bias, int mt0,
                                              const float *src, int cin, float *dst, int cout, bool alias,
                                              const GnEpilogue &g, const PRE &pre, const HOOK &hook, bool live) {
  using GG = Geo<64>;
  using PGx = PG<LL>;
  const int kq = c.lane >> 4, cl = c.lane & 15;
  const int sm = LL == 16 ? (c.lane & 3) : cl;   // the lane's sample
  f32x4 acc[MT][NP];
  const bool has_ss = FIN == 1 && g.ss_w >= 0;
  const bool ss_tab = LL == 16 && has_ss && c.ss_lane != nullptr;   // rows precomputed per cloud (pose decoder)
  const int ekb = g.E >> 4;
  const WStream wss(c.w + (has_ss ? g.ss_w : 0), c.lane);
  f32x4 ga[MT], be[MT], sc[MT], sh[MT], a_sc[MT], a_sh[MT];
  // Epilogue parameters are requested right after the k-sweep (measured: requesting them before it, live through
  // the sweep, is 0-10 % slower on the narrow convs and no faster on the wide ones: the gemm_pm_rate probe of DESIGN_HISTORY.md)
  auto load_params = [&]() {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      const int mt = mt0 + mi, row0 = 16 * mt + 4 * kq;
      ga[mi] = *reinterpret_cast<const f32x4 *>(c.w + g.gamma_off + row0);
      be[mi] = *reinterpret_cast<const f32x4 *>(c.w + g.beta_off + row0);
      sc[mi] = f32x4{1.f, 1.f, 1.f, 1.f};
      sh[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ss_tab) {
        sc[mi] = *reinterpret_cast<const f32x4 *>(c.ss_lane + g.tab_off + row0);
        sh[mi] = *reinterpret_cast<const f32x4 *>(c.ss_lane + g.tab_off + g.C + row0);
      } else if (has_ss) {
        const float *sb = c.w + g.ss_b;
        sc[mi] = *reinterpret_cast<const f32x4 *>(sb + row0);
        sh[mi] = *reinterpret_cast<const f32x4 *>(sb + g.C + row0);
        a_sc[mi] = wss[(size_t)mt * ekb * 64];
        a_sh[mi] = wss[(size_t)((g.C >> 4) + mt) * ekb * 64];
      }
    }
  };
  // Range of H.  A ResnetBlock's H = act((scale + 1) GN(conv1) + shift) is the one operand whose size is set by the DATA
  // (the conditioning embedding through scale / shift: 5e5 with wild conditioning rows, tests/test_cli.py), and f16
  // planes end at 65504.  block1 therefore writes H / hs, hs a power of two per SAMPLE chosen from a bound it already has
  // in registers (1 for anything ordinary: every operation below is then bit for bit what it was); block2 computes
  // conv(H) / hs (bias / hs in the accumulator) and folds hs back into its GroupNorm coefficients (per-sample
  // statistics: mean and M2 scale with hs and hs^2).  Everything else these engines feed the f16 pipe is bounded by the
  // weights alone (norm outputs, residual sums of them, softmax-weighted values).
  lds_f *hsc = (lds_f *)(c.lds + GG::kMiscHs);
  float hs = 1.0f;
  if constexpr (FIN == 2) hs = hsc[sm];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4 *>(bias + 16 * (mt0 + mi) + 4 * kq);
    if constexpr (FIN == 2) {
      const float hinv = __builtin_amdgcn_rcpf(hs);   // a power of two: exact
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] *= hinv;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[mi][p] = bv;
  }
  // B operand: pre-split planes.  Up to 128 input channels: the X planes or the H planes, by which buffer `src` is; 256
  // (the last level's ResnetBlock): the level's one plane set (kW)
  GLDM_WV_STAMP(c, 0, (long long)__builtin_readcyclecounter());
  GLDM_WV_STAMP(c, 3, (long long)(cin * 1000 + cout));
  const bool src_is_x = src == c.lds + GG::kBufX;
  const float *bplanes = c.lds + (cin > kPlaneMaxC ? PGx::kW : (src_is_x ? PGx::kX : PGx::kH));
  if constexpr (LL == 16) gemm_sm3_pl<MT, P0, NP, PRE>(c, wp, cin, mt0, bplanes, acc, pre);
  else gemm_pm3_pl<MT, P0, NP, PRE>(c, wp, cin, mt0, bplanes, acc, pre);
  GLDM_WV_STAMP(c, 1, (long long)__builtin_readcyclecounter());
  if (FIN != 0) load_params();
  // 256-channel level (two m-tiles per wave).  16-position engine: this lane's slice of the parked residual stream, one
  // f32x4 per (m-tile, position) (its 256 f32 rows do not fit beside the padded planes); the 4-position engine keeps the
  // f32 rows in LDS (PG<4>::kW lies behind them)
  constexpr bool kWide = MT == 2;
  constexpr bool kPark = kWide && LL == 16;
  f32x4 *pk = reinterpret_cast<f32x4 *>(c.park) + (size_t)(c.wave * MT * NP) * 64 + c.lane;
  f32x4 parked[FIN == 2 && kPark ? MT : 1][FIN == 2 && kPark ? NP : 1];
  if constexpr (FIN == 2 && kPark) {   // requested here, in flight under the statistics and the exchange barrier
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int p = 0; p < NP; ++p) parked[mi][p] = pk[(mi * NP + p) * 64];
  }
  hook();   // the fused ResnetBlock's request for its second conv's first fragments: in flight under this epilogue
  if constexpr (FIN == 0) {  // the level's down conv: the new residual stream X as planes, and as f32 rows (up to 128
                             // channels: in LDS) or parked in global scratch (256: see kPlaneW)
    if (alias) __syncthreads();
    if (live) {
      lds_f *d3 = (lds_f *)dst;
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if constexpr (kPark) {
            pk[(mi * NP + p) * 64] = acc[mi][p];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) d3[pswz(16 * (mt0 + mi) + 4 * kq + r, 16 * (P0 + p) + cl)] = acc[mi][p][r];
          }
          store_planes4<LL>(c.lds + (kWide ? PGx::kW : PGx::kX), 16 * (mt0 + mi) + 4 * kq, 16 * (P0 + p) + cl, acc[mi][p][0],
                            acc[mi][p][1], acc[mi][p][2], acc[mi][p][3]);
        }
    }
    GLDM_WV_STAMP(c, 2, (long long)__builtin_readcyclecounter());
    GLDM_WV_NEXT(c);
    return;
  }
  if constexpr (FIN != 0) {
  // ---- this wave's share of the statistics, per sample
  constexpr int kRows = GK == 3 ? 4 : (GK == 2 ? 8 : 16 * MT);   // rows behind one published pair
  constexpr int kNloc = kRows * NP * (LL == 16 ? 4 : 1);         // values behind it
  constexpr int kParts = (GK == 2 || GK == 3) ? 4 : 2;
  auto over_sample = [&](float v) {   // the lanes that hold this sample's other positions / row quarters of the group
    if constexpr (LL == 16) {
      v += dpp_mov<0x124>(v);   // row_ror:4
      v += dpp_mov<0x128>(v);   // row_ror:8: the four positions inside the tile
    }
    if constexpr (GK != 3) v = row_pair_sum(v);
    if constexpr (GK == 0 || GK == 1) v = half_sum(v);
    return v;
  };
  float s1 = 0.f;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) s1 += acc[mi][p][r];
  s1 = over_sample(s1);
  const float mloc = s1 * (1.0f / (float)kNloc);
  float s2 = 0.f;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dx = acc[mi][p][r] - mloc;
        s2 += dx * dx;
      }
  s2 = over_sample(s2);
  lds_f *red1 = (lds_f *)(c.lds + GG::kMiscRed1), *red2 = (lds_f *)(c.lds + GG::kMiscRed2);
  const int slot = GK == 3 ? kq : (GK == 2 ? (kq >> 1) : 0);
  const bool pub = (GK == 3 || (kq & (GK == 2 ? 1 : 3)) == 0) && (LL != 16 || (cl >> 2) == 0);
  if (pub && live) {
    red1[(c.wave * 4 + slot) * 16 + sm] = s1;
    red2[(c.wave * 4 + slot) * 16 + sm] = s2;
  }
  // ---- scale / shift rows of this lane's sample (the same for all positions: once per m-tile).  They do not depend
  // on the statistics, so they are issued in front of the exchange barrier: the MFMA chain runs while the wave waits
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_NO_SS)   // timing experiment only (wrong results): no scale/shift chain
  if (false) {
#else
  if (has_ss && !ss_tab) {
#endif
    const lds_f *Gs = (const lds_f *)(c.lds + GG::kMiscG) + sm * g.E;
    float gb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gb[j] = Gs[4 * j + kq];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_sc[mi][j], gb[j], sc[mi], 0, 0, 0);
        sh[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_sh[mi][j], gb[j], sh[mi], 0, 0, 0);
      }
      for (int kb = 1; kb < ekb; ++kb) {
        const int mt = mt0 + mi;
        const f32x4 a2 = wss[((size_t)mt * ekb + kb) * 64], a3 = wss[((size_t)((g.C >> 4) + mt) * ekb + kb) * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float bj = Gs[16 * kb + 4 * j + kq];
          sc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[j], bj, sc[mi], 0, 0, 0);
          sh[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[j], bj, sh[mi], 0, 0, 0);
        }
      }
    }
  }
  if constexpr (FIN == 1) {
    // |H| <= |gamma (scale + 1)| R + |beta (scale + 1) + shift| over this lane's rows, R = sqrt(group size) >= any
    // normalised value of the group; max over the lanes of the sample, then over the eight waves behind the barrier
    constexpr float kR = sqrt_up(kNloc * kParts);
    float hb = 0.f;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        hb = fmaxf(hb, fmaf(__builtin_fabsf(ga[mi][r] * sc[mi][r]), kR, __builtin_fabsf(fmaf(be[mi][r], sc[mi][r], sh[mi][r]))));
    if constexpr (LL == 16) {
      hb = dpp_max<0x124>(hb);
      hb = dpp_max<0x128>(hb);
    }
    hb = half_max(row_pair_max(hb));
    if (kq == 0 && (LL != 16 || (cl >> 2) == 0)) ((lds_f *)(c.lds + GG::kMiscHb))[c.wave * 16 + sm] = hb;   // shadow waves too
  }
  GLDM_WV_STAMP(c, 4, (long long)__builtin_readcyclecounter());
  __syncthreads();
  GLDM_WV_STAMP(c, 5, (long long)__builtin_readcyclecounter());
  float hinv = 1.0f;   // block1: 1 / hs of this lane's sample
  if constexpr (FIN == 1) {
    const lds_f *hbp = (const lds_f *)(c.lds + GG::kMiscHb) + sm;
    float hb = hbp[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) hb = fmaxf(hb, hbp[16 * q]);
    // hb in [2^k, 2^(k+1)): hs = 2^max(0, k - 14) puts H / hs below 2^15
    int e = (int)((__float_as_uint(hb) >> 23) & 0xffu) - 127 - 14;
    e = e < 0 ? 0 : e;
    hinv = __uint_as_float((unsigned)(127 - e) << 23);
    if (c.wave == 0 && kq == 0 && (LL != 16 || (cl >> 2) == 0)) hsc[sm] = __uint_as_float((unsigned)(127 + e) << 23);
  }
  float tot = 0.f, ps1[kParts], ps2[kParts];
#pragma unroll
  for (int q = 0; q < kParts; ++q) {
    // partners: GK 0 the adjacent wave; GK 1 wave ^ 4 (the other half of the positions / tiles); GK 2 the four waves of the
    // m-tile (one per position / tile); GK 3 waves 0-3 (one tile each)
    const int pw = GK == 0 ? ((c.wave & ~1) + q) : (GK == 1 ? ((c.wave & 3) + 4 * q) : (GK == 2 ? ((c.wave & 1) + 2 * q) : q));
    ps1[q] = red1[(pw * 4 + slot) * 16 + sm];
    ps2[q] = red2[(pw * 4 + slot) * 16 + sm];
    tot += ps1[q];
  }
  const float mean = tot * (1.0f / (float)(kNloc * kParts));
  float m2 = 0.f;
#pragma unroll
  for (int q = 0; q < kParts; ++q) {
    const float dm = ps1[q] * (1.0f / (float)kNloc) - mean;
    m2 += ps2[q] + (float)kNloc * dm * dm;
  }
  // block2: the accumulators hold conv / hs: the true variance is hs^2 times theirs, and (acc - mean') hs rstd is the
  // normalised value (hs = 1: the same bits as without it)
  const float rstd = __builtin_amdgcn_rsqf((m2 * hs) * hs * (1.0f / (float)(kNloc * kParts)) + 1e-5f) * hs;
  // mode 1 (block1): H = y, as planes only (H is only ever a conv input);
  // mode 2 (block2): X += y in f32 (the residual stream), plus the planes of the new X up to 128 channels; at 256
  // channels X = parked + y as f32 rows only (what follows is the final 1x1 conv).
  // One straight-line instance per (mode, scale/shift): with the two tested per VALUE (wave-uniform branches inside
  // the unrolled loops) every value was its own chain of basic blocks -- 61 branches and no overlap between the 16-32
  // exp / rcp chains of a lane: 3.8-4.9 k cycles for the 16 values of a one-m-tile conv, alone on the SIMD or not.
  lds_f *d3 = (lds_f *)(FIN == 2 ? g.res : dst);
  auto finish = [&](auto mode_c, auto ss_c) {
    constexpr int kMode = decltype(mode_c)::value;
    constexpr bool kSS = decltype(ss_c)::value;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      // GroupNorm, its affine and the scale/shift are ONE fma per value, y = acc A + B, and SiLU's exponent a second one
      // from the same accumulator (u = -log2(e) y): the coefficients depend on the row only and serve the wave's NP
      // positions (with a single position per wave the plain chain is shorter).  VALU instructions per value: 6 instead of 9.
      constexpr bool kFold = NP >= 2;
      float fa[4], fb[4], na[4], nb[4];
      if constexpr (kFold) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float A = rstd * ga[mi][r];
          float B = be[mi][r] - mean * A;
          if (kSS) {
            B = B * sc[mi][r] + sh[mi][r];
            A = A * sc[mi][r];
          }
          fa[r] = A; fb[r] = B;
          na[r] = -1.44269504088896340736f * A; nb[r] = -1.44269504088896340736f * B;
        }
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t;
          if constexpr (kFold) {
            const float v = acc[mi][p][r];
            t = fmaf(v, fa[r], fb[r]);
            t = t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(fmaf(v, na[r], nb[r])));
          } else {
            t = (acc[mi][p][r] - mean) * (rstd * ga[mi][r]) + be[mi][r];
            if (kSS) t = t * sc[mi][r] + sh[mi][r];
            t = silu(t);
          }
          const int a = pswz(16 * (mt0 + mi) + 4 * kq + r, 16 * (P0 + p) + cl);
          if constexpr (kMode == 2) {
            if constexpr (kPark) t = parked[mi][p][r] + t;
            else t = d3[a] + t;
            d3[a] = t;
          }
          y[r] = kMode == 1 ? t * hinv : t;
        }
        if constexpr (!(kMode == 2 && kWide))
          store_planes4<LL>(c.lds + (kMode == 2 ? PGx::kX : (kWide ? PGx::kW : PGx::kH)), 16 * (mt0 + mi) + 4 * kq,
                            16 * (P0 + p) + cl, y[0], y[1], y[2], y[3]);
      }
    }
  };
  using std::integral_constant;
  if (live) {
    if constexpr (FIN == 2) {
      finish(integral_constant<int, 2>{}, integral_constant<bool, false>{});
    } else {
      if (has_ss) finish(integral_constant<int, 1>{}, integral_constant<bool, true>{});
      else finish(integral_constant<int, 1>{}, integral_constant<bool, false>{});
    }
  }
  }
  GLDM_WV_STAMP(c, 2, (long long)__builtin_readcyclecounter());
  GLDM_WV_NEXT(c);
}

// Conv1d(4 -> cout, k = 3) of the first level (Cin = 4 is below the MFMA k-block): VALU, lane = column, wave w
// computes output channels 4w .. 4w+3 (cout = 32).  Weights are wave uniform (scalar loads); fma chain in the
// MFMA's k order (tap major, channel minor) from the bias.  src may alias dst.
template <int ROUNDS>   // 32 output channels per round (4 per wave); cout == 32 ROUNDS exactly: no per-value guards
__device__ __forceinline__ void conv_pm3_cin4_rounds(const Ctx &c, const float *wp, const float *bias, const float *src,
                                                     float *dst, bool alias) {
  const int n = c.lane, p = n >> 4;
  const lds_f *s3 = (const lds_f *)src;
  float x[3][4];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const float l = s3[pswz(ci, p > 0 ? n - 16 : n)], m = s3[pswz(ci, n)], r = s3[pswz(ci, p < 3 ? n + 16 : n)];
    x[0][ci] = p > 0 ? l : 0.f;
    x[1][ci] = m;
    x[2][ci] = p < 3 ? r : 0.f;
  }
  // all rounds are computed before the (possibly aliased) destination is written
  float out[ROUNDS][4];
#pragma unroll
  for (int rd = 0; rd < ROUNDS; ++rd) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cc = __builtin_amdgcn_readfirstlane(rd * 32 + c.wave * 4 + k);
      float acc = bias ? bias[cc] : 0.f;
      const float *wr = wp + (size_t)(cc >> 4) * 256 + (cc & 15) * 4;  // [(ci * 16 + co % 16) * 4 + tap]
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) acc = fmaf(wr[ci * 64 + t], x[t][ci], acc);
      out[rd][k] = acc;
    }
  }
  if (alias) __syncthreads();
  lds_f *d3 = (lds_f *)dst;
#pragma unroll
  for (int rd = 0; rd < ROUNDS; ++rd) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d3[pswz(rd * 32 + c.wave * 4 + k, n)] = out[rd][k];
    // the new residual stream's planes (a wave's 4 channels are one half of an 8-group)
    if (ROUNDS * 32 <= kPlaneMaxC)
      store_planes4(c.lds + kPlaneX, rd * 32 + c.wave * 4, n, out[rd][0], out[rd][1], out[rd][2], out[rd][3]);
  }
}
__device__ __forceinline__ void conv_pm3_cin4_any(const Ctx &c, const float *wp, const float *bias, const float *src,
                                              float *dst, int cout, bool alias) {
  const int n = c.lane, p = n >> 4;
  const lds_f *s3 = (const lds_f *)src;
  float x[3][4];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const float l = s3[pswz(ci, p > 0 ? n - 16 : n)], m = s3[pswz(ci, n)], r = s3[pswz(ci, p < 3 ? n + 16 : n)];
    x[0][ci] = p > 0 ? l : 0.f;
    x[1][ci] = m;
    x[2][ci] = p < 3 ? r : 0.f;
  }
  // 32 output channels per round (4 per wave); wider first levels take more rounds.  All rounds are computed before
  // the (possibly aliased) destination is written.
  constexpr int kMaxRounds = kMaxC / 32;
  float out[kMaxRounds][4];
#pragma unroll
  for (int rd = 0; rd < kMaxRounds; ++rd) {
    if (rd * 32 < cout) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int co = __builtin_amdgcn_readfirstlane(rd * 32 + c.wave * 4 + k);
        const int cc = co < cout ? co : cout - 1;
        float acc = bias ? bias[cc] : 0.f;
        const float *wr = wp + (size_t)(cc >> 4) * 256 + (cc & 15) * 4;  // [(ci * 16 + co % 16) * 4 + tap]
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
          for (int ci = 0; ci < 4; ++ci) acc = fmaf(wr[ci * 64 + t], x[t][ci], acc);
        out[rd][k] = acc;
      }
    }
  }
  if (alias) __syncthreads();
  lds_f *d3 = (lds_f *)dst;
#pragma unroll
  for (int rd = 0; rd < kMaxRounds; ++rd) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int co = rd * 32 + c.wave * 4 + k;
      if (co < cout) d3[pswz(co, n)] = out[rd][k];
    }
    // the new residual stream's planes (a wave's 4 channels are one half of an 8-group; cout % 32 == 0)
    if (rd * 32 < cout && cout <= kPlaneMaxC)
      store_planes4(c.lds + kPlaneX, rd * 32 + c.wave * 4, n, out[rd][0], out[rd][1], out[rd][2], out[rd][3]);
  }
}

__device__ __forceinline__ void conv_pm3_cin4(const Ctx &c, const float *wp, const float *bias, const float *src,
                                              float *dst, int cout, bool alias) {
  // the shipped 32-channel level without per-value `co < cout` tests (32 branches in the common body); wider first
  // levels on the common body (an instance per width spilled 361 registers across the kernel)
  if (cout == 32) conv_pm3_cin4_rounds<1>(c, wp, bias, src, dst, alias);
  else conv_pm3_cin4_any(c, wp, bias, src, dst, cout, alias);
}

// ResnetBlock of the 4-channel level on the VALU of one wave: lane = column (16 samples x 4 positions), every
// lane carries all 4 channels of its column.  Taps come from the lanes 16 below / above (the neighbouring
// positions of the same sample), GroupNorm (one channel per group) reduces over lanes n ^ 16, n ^ 32.  Every
// weight is wave uniform (scalar loads: nothing queues in the vector-memory path).
__device__ __forceinline__ void resblock4_pm(const Ctx &c, const int (&o)[kOpInts], int E) {
  using GG = Geo<64>;
  if (c.wave != 0) return;
  const int n = c.lane, sm = n & 15, p = n >> 4;
  const bool has_l = p != 0, has_r = p != 3;
  lds_f *X = (lds_f *)(c.lds + GG::kBufX);
  const lds_f *G = (const lds_f *)(c.lds + GG::kMiscG) + sm * E;
  const float *w = c.w;
  const int c1_w = o[1], c1_b = o[2], n1_w = o[3], n1_b = o[4], c2_w = o[5], c2_b = o[6], n2_w = o[7], n2_b = o[8],
            ss_w = o[9], ss_b = o[10];
  // Every weight of the phase is staged by explicit 16-byte loads issued in two batches in front of their use (wave-uniform
  // addresses; all offsets are multiples of 4 floats in the packed buffer).  Left to the scheduler, one build of this
  // kernel issued them one by one with a full wait each (18.7 k cycles for the phase instead of 5.8 k).
  struct ConvW { f32x4 wt[16], b, g, be; };   // W[co][ci][tap] at f32x4 index ci * 16 + co (co < 4), taps in .xyz
  auto load_conv = [&](ConvW &cw, int w_off, int b_off, int g_off, int be_off) {
    const f32x4 *wv = reinterpret_cast<const f32x4 *>(w + w_off);
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int co = 0; co < 4; ++co) cw.wt[4 * ci + co] = wv[ci * 16 + co];
    cw.b = *reinterpret_cast<const f32x4 *>(w + b_off);
    cw.g = *reinterpret_cast<const f32x4 *>(w + g_off);
    cw.be = *reinterpret_cast<const f32x4 *>(w + be_off);
  };
  f32x4 wss[4][8], bss[2];   // scale/shift Linear: W[row][e] at ((e & 3) * 16 + row) * 4 + (e >> 2): f32x4 (e & 3) * 16 + row
  {
    const f32x4 *wv = reinterpret_cast<const f32x4 *>(w + ss_w);
#pragma unroll
    for (int kq = 0; kq < 4; ++kq)
#pragma unroll
      for (int row = 0; row < 8; ++row) wss[kq][row] = wv[kq * 16 + row];
    bss[0] = *reinterpret_cast<const f32x4 *>(w + ss_b);
    bss[1] = *reinterpret_cast<const f32x4 *>(w + ss_b + 4);
  }
  ConvW k1, k2;
  load_conv(k1, c1_w, c1_b, n1_w, n1_b);
  float x[4];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) x[ci] = X[pswz(ci, n)];
  float gq[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) gq[e] = e < E ? G[e] : 0.f;
  __builtin_amdgcn_sched_barrier(0);
  float sc[4], sh[4];
#pragma unroll
  for (int co = 0; co < 4; ++co) {
    float a = bss[0][co], b = bss[1][co];
#pragma unroll
    for (int kq = 0; kq < 4; ++kq)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a += wss[kq][co][j] * gq[4 * j + kq];
        b += wss[kq][4 + co][j] * gq[4 * j + kq];
      }
    sc[co] = a;
    sh[co] = b;
  }
  __builtin_amdgcn_sched_barrier(0);
  load_conv(k2, c2_w, c2_b, n2_w, n2_b);   // in flight under the first conv
  __builtin_amdgcn_sched_barrier(0);
  auto conv3 = [&](const float (&in)[4], const ConvW &cw, float (&out)[4]) {
    float lft[4], rgt[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const float a = __shfl(in[ci], (n + 48) & 63, 64), b = __shfl(in[ci], (n + 16) & 63, 64);
      lft[ci] = has_l ? a : 0.f;
      rgt[ci] = has_r ? b : 0.f;
    }
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      float acc = cw.b[co];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const f32x4 wr = cw.wt[4 * ci + co];
        acc += wr[0] * lft[ci];
        acc += wr[1] * in[ci];
        acc += wr[2] * rgt[ci];
      }
      out[co] = acc;
    }
  };
  auto gn_act = [&](float (&v)[4], const ConvW &cw, bool ss) {
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      const float m = half_sum(row_pair_sum(v[co])) * 0.25f;
      const float d = v[co] - m;
      const float rs = __builtin_amdgcn_rsqf(half_sum(row_pair_sum(d * d)) * 0.25f + 1e-5f);
      float y = d * rs * cw.g[co] + cw.be[co];
      if (ss) y = y * sc[co] + sh[co];
      v[co] = silu(y);
    }
  };
  float y[4], z[4];
  conv3(x, k1, y);
  gn_act(y, k1, true);
  conv3(y, k2, z);
  gn_act(z, k2, false);
#pragma unroll
  for (int co = 0; co < 4; ++co) X[pswz(co, n)] = x[co] + z[co];
}

// to_out of LinearAttention: Conv1d(128 -> C, k = 1) -> LayerNorm over the channels -> residual add
// (resnets.py:211-235, Residual(PreNorm(...)) :59-65,116-124), as ONE phase of the 64-column engine: the LayerNorm
// statistics of a column are merged across the waves that hold its rows -- per-wave (sum, M2 about the wave's own
// mean) over its 16 rows, one LDS exchange, parallel-variance merge -- and x += LN(y) g is applied to the
// accumulators.  Replaces a conv phase that stored y plus a LayerNorm phase that read it back (3 barriers).
// NPW = partner waves of the LayerNorm merge, FULL = every row of the m-tile is a channel (C >= 16): compile-time, so that
// the per-value code has no wave-uniform branches (each value used to be its own chain of basic blocks)
// FIRST: block 0's fragments of the wave's m-tile, requested by the caller ahead of the call (Frag3), or NoFirst.
template <int NT, int NPW, bool FULL, int LL = 4, class FIRST = NoFirst>
__device__ __forceinline__ void out_ln_wave(const Ctx &c, const float *wp, const float *bias, int mt0, int nt0,
                                            bool active, int p0, const float *src, int cin, float *xres, int C,
                                            const float *gain, const FIRST &first = FIRST()) {
  using GG = Geo<64>;
  constexpr int NC = 64;
  const int kq = c.lane >> 4, col = c.lane & 15;
  f32x4 acc[1][NT];
  lds_f *red1 = (lds_f *)(c.lds + GG::kMiscRed1), *red2 = (lds_f *)(c.lds + GG::kMiscRed2);
  const int row0 = 16 * mt0 + 4 * kq;
  const int nloc = C < 16 ? C : 16;  // rows behind one published pair
  f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + row0);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[0][ni] = bv;
    gemm1_pl<kHidden / 32, 1, NT, NoPre, 1, LL, FIRST>(c, wp, mt0, nt0, c.lds + PG<LL>::kH, acc, NoPre(), first);  // the attention output's planes (cin = 128)
    gv = *reinterpret_cast<const f32x4 *>(gain + row0);
    const float inv_n = __builtin_amdgcn_rcpf((float)nloc);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      float s1 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) s1 += (FULL || row0 + r < C) ? acc[0][ni][r] : 0.f;
      s1 = half_sum(row_pair_sum(s1));
      const float ml = s1 * inv_n;
      float s2 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = (FULL || row0 + r < C) ? acc[0][ni][r] - ml : 0.f;
        s2 += d * d;
      }
      s2 = half_sum(row_pair_sum(s2));
      if (kq == 0) {
        red1[c.wave * NC + 16 * (nt0 + ni) + col] = s1;
        red2[c.wave * NC + 16 * (nt0 + ni) + col] = s2;
      }
    }
  }
  __syncthreads();
  if (active) {
    const float inv_c = __builtin_amdgcn_rcpf((float)C), inv_n = __builtin_amdgcn_rcpf((float)nloc);
    lds_f *x3 = (lds_f *)xres;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int cc = 16 * (nt0 + ni) + col;
      float ps[NPW], pm[NPW], tot = 0.f;
#pragma unroll
      for (int q = 0; q < NPW; ++q) {  // each partner's pair is read once
        ps[q] = red1[(p0 + q) * NC + cc];
        pm[q] = red2[(p0 + q) * NC + cc];
        tot += ps[q];
      }
      const float mean = tot * inv_c;
      float m2 = 0.f;
#pragma unroll
      for (int q = 0; q < NPW; ++q) {
        const float dm = ps[q] * inv_n - mean;
        m2 += pm[q] + (float)nloc * dm * dm;
      }
      const float rstd = __builtin_amdgcn_rsqf(m2 * inv_c + 1e-5f);
      float xn[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (FULL || row0 + r < C) {
          const int a = pswz(row0 + r, cc);
          xn[r] = x3[a] + (acc[0][ni][r] - mean) * rstd * gv[r];
          x3[a] = xn[r];
        }
      if (FULL && C >= 16) store_planes4<LL>(c.lds + PG<LL>::kX, row0, cc, xn[0], xn[1], xn[2], xn[3]);  // the new X's planes
    }
  }
  __syncthreads();
}

// The 128-channel level's to_out with its first weight fragments requested by the caller in front of the attention op
// (run_tape: OP_QKVATT followed by OP_OUTLN run as one case): cold at the top of this op they cost an L2 round trip with all
// eight waves waiting.
__device__ __forceinline__ Frag3 out_ln_request(const Ctx &c, int w_off) {
  const WStream wv(c.w + w_off, c.lane);
  Frag3 f;
#pragma unroll
  for (int pl = 0; pl < kSplit; ++pl) f.p[pl] = wv.raw_at((c.wave * (kHidden / 32)) * kFragBytes, pl * 1024);   // m-tile = wave, block 0
  return f;
}
template <int LL = 4>
__device__ __forceinline__ void out_ln_pm128(const Ctx &c, int w_off, int b_off, const float *src, int cin, float *xres, int g_off,
                                             const Frag3 &first) {
  out_ln_wave<4, 8, true, LL, Frag3>(c, c.w + w_off, c.w + b_off, c.wave, 0, true, 0, src, cin, xres, 128, c.w + g_off, first);
}
template <int LL = 4>
__device__ __forceinline__ void out_ln_pm(const Ctx &c, int w_off, int b_off, const float *src, int cin, float *xres,
                                          int C, int g_off) {
  const float *wp = c.w + w_off, *bias = c.w + b_off, *gain = c.w + g_off;
  const int mtiles = (C + 15) >> 4, w = c.wave;
  if (mtiles == 8) out_ln_wave<4, 8, true, LL>(c, wp, bias, w, 0, true, 0, src, cin, xres, C, gain);
  else if (mtiles == 4) out_ln_wave<2, 4, true, LL>(c, wp, bias, w & 3, 2 * (w >> 2), true, 4 * (w >> 2), src, cin, xres, C, gain);
  else if (mtiles == 2) out_ln_wave<1, 2, true, LL>(c, wp, bias, w & 1, w >> 1, true, 2 * (w >> 1), src, cin, xres, C, gain);
  else if (LL == 16) out_ln_wave<1, 1, true, LL>(c, wp, bias, 0, w & 3, w < 4, w & 3, src, cin, xres, C, gain);   // C = 16
  else out_ln_wave<1, 1, false, LL>(c, wp, bias, 0, w & 3, w < 4, w & 3, src, cin, xres, C, gain);
}

// Rows of the per-column LayerNorm statistics the fused qkv + attention phase needs (see qkv_att_pm): wave w owns columns
// 8 w .. 8 w + 7, lane = (row part, column), two passes over the C / 8 values in its registers (the reference's mean,
// then sum (x - mean)^2), the parts meet through DPP / permlane swaps, (mean, rstd) go to LDS.
template <int RP>  // rows per lane: C / 8
__device__ __forceinline__ void column_stats8(const Ctx &c, const float *src, float inv_c) {
  constexpr int NC = 64;
  using GG = Geo<NC>;
  const lds_f *s3 = (const lds_f *)src;
  const int n = 8 * c.wave + (c.lane & 7), rp = c.lane >> 3;
  float v[RP], sum = 0.f;
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    v[i] = s3[pswz(rp + 8 * i, n)];
    sum += v[i];
  }
  auto all_parts = [](float x) {  // lanes differing in bits 3, 4, 5
    x += dpp_mov<0x128>(x);  // row_ror:8
    return half_sum(row_pair_sum(x));
  };
  const float mean = all_parts(sum) * inv_c;
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const float d = v[i] - mean;
    m2 = fmaf(d, d, m2);
  }
  const float rstd = __builtin_amdgcn_rsqf(all_parts(m2) * inv_c + 1e-5f);
  if (rp == 0) {
    ((lds_f *)(c.lds + GG::kMiscRed1))[n] = mean;
    ((lds_f *)(c.lds + GG::kMiscRed2))[n] = rstd;
  }
}

// Residual(PreNorm(LinearAttention)) up to its to_out conv (resnets.py:104-124, 211-235) as ONE phase of the position-major
// engine: PreNorm LayerNorm, to_qkv 1x1 conv and the attention core of all four heads, with q, k and v never leaving the
// accumulators (they used to be stored as a [384][64] f32 block -- 96 KiB through ds_write_b32 -- and read back by a
// separate three-barrier attention phase).
//   * Wave = (head h, channel half): its three m-tiles are rows 32 h + 16 half .. + 15 of q, of k and of v (to_qkv's own
//     row order: m-tiles 2 h + half, + 8, + 16).  In the C layout of the MFMA a lane then holds, for ONE sample (lane & 15),
//     four channels (4 (lane >> 4) + r) at all four positions (the n-tiles), of q, k and v alike.
//   * LayerNorm is folded into the conv for the 16 | C levels:  W (g (x - mean) rstd) = rstd (W' x - mean s),  W' = W diag(g),
//     s = W' 1  (both prepared on the host); the column statistics are taken while the first weight fragments are on their
//     way (column_stats8) and applied to the accumulators after the one barrier that publishes them.  The 4-channel level
//     normalises its columns in the lanes and multiplies with K = 4 f32 MFMAs (the packed A fragment's first element is
//     the operand as it stands).
//   * Attention, reassociated at n = L = 4:  out[e][n] = sum_m v[e][m] A[m][n],  A[m][n] = scale / sum_d exp(q[d][n] - max_n)
//     * sum_d softmax_m(k[d])[m] exp(q[d][n] - max_n).  The key softmax over a sample's 4 positions and the products with v
//     are in-lane; the sums over d (32 channels of the head) are in-lane over the lane's 4 channels, permlane swaps over
//     the four row quarters, and ONE exchange through LDS between the two waves of the head: each publishes
//     (max, sum, A) taken over its own 16 channels and merges the partner's like two blocks of an online softmax.
//   * The output leaves as split-f16 planes (it is only ever the B operand of to_out), into the H-plane region.
// Barriers: statistics, exchange, end (the two phases this replaces had five).
constexpr int kAttExch = 512 * 64;   // floats [32768, 35840): 8 waves x 24 rows x 16 samples, behind the X planes
static_assert(kAttExch + 8 * 24 * 16 <= Geo<64>::kArena, "attention exchange slots");
template <int KB32>   // C / 32 (0: the 4-channel level)
__device__ __forceinline__ void qkv_att_pm(const Ctx &c, int w_off, int s_off, const float *src, int C) {
  constexpr int NC = 64;
  using GG = Geo<NC>;
  if (GLDM_SKIP(c, 8)) return;
  const int head = c.wave >> 1, half = c.wave & 1;
  const int mt0 = 2 * head + half;   // q rows; k: m-tile + 8, v: + 16
  const int sm = c.lane & 15, kq = c.lane >> 4;
  f32x4 acc[3][4];
  if constexpr (KB32 == 0) {
    const int n = c.lane;
    const lds_f *s3 = (const lds_f *)src;
    float x[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) x[ci] = s3[pswz(ci, n)];
    const float mean = (x[0] + x[1] + x[2] + x[3]) * 0.25f;
    float vt = 0.f;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const float d = x[ci] - mean;
      vt += d * d;
    }
    const float rstd = __builtin_amdgcn_rsqf(vt * 0.25f + 1e-5f);
    // every wave normalises all 64 columns itself and writes the same values to the same scratch rows, then reads its
    // own writes in B-operand order (lane col + 16 k = y[k] of column 16 j + col): no barrier
    lds_f *ysc = (lds_f *)(c.lds + GG::kMiscRed1);   // [4][64]
#pragma unroll
    for (int k = 0; k < 4; ++k) ysc[64 * k + n] = (x[k] - mean) * rstd;
    const WStream wv(c.w + w_off, c.lane);
    f32x4 f[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) f[t] = wv[(size_t)(mt0 + 8 * t) * 64];
    float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = ysc[64 * kq + 16 * j + sm];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[t][0], b[j], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  } else {
    const float *wp = c.w + w_off, *srow = c.w + s_off;
    f32x4 sv[3];
#pragma unroll
    for (int mi = 0; mi < 3; ++mi) sv[mi] = *reinterpret_cast<const f32x4 *>(srow + 16 * (mt0 + 8 * mi) + 4 * kq);
#pragma unroll
    for (int mi = 0; mi < 3; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float inv_c = __builtin_amdgcn_rcpf((float)C);  // C: a power of two -> exact
    auto stats = [&]() { column_stats8<4 * KB32>(c, src, inv_c); };
    gemm1_pl<KB32, 3, 4, decltype(stats), 8>(c, wp, mt0, 0, c.lds + kPlaneX, acc, stats);
    __syncthreads();  // every column's (mean, rstd) is in LDS
    const lds_f *mean3 = (const lds_f *)(c.lds + GG::kMiscRed1), *rstd3 = (const lds_f *)(c.lds + GG::kMiscRed2);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const float rstd = rstd3[16 * ni + sm];
      const float mr = mean3[16 * ni + sm] * rstd;
#pragma unroll
      for (int mi = 0; mi < 3; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mi][ni][r] = acc[mi][ni][r] * rstd - mr * sv[mi][r];
    }
  }
  // ---- keys: softmax over the sample's 4 positions, per channel (in lane)
  float kn[4][4];   // [position][channel r]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float km = fmaxf(fmaxf(acc[1][0][r], acc[1][1][r]), fmaxf(acc[1][2][r], acc[1][3][r]));
    float ks = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      kn[p][r] = fast_exp(acc[1][p][r] - km);
      ks += kn[p][r];
    }
    const float inv = __builtin_amdgcn_rcpf(ks);
#pragma unroll
    for (int p = 0; p < 4; ++p) kn[p][r] *= inv;
  }
  // ---- queries: exp(q - max) and their sum over this wave's 16 channels of the head, per position
  float qe[4][4], qm[4], qs[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float m = fmaxf(fmaxf(acc[0][p][0], acc[0][p][1]), fmaxf(acc[0][p][2], acc[0][p][3]));
    m = half_max(row_pair_max(m));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qe[p][r] = fast_exp(acc[0][p][r] - m);
      sum += qe[p][r];
    }
    qm[p] = m;
    qs[p] = half_sum(row_pair_sum(sum));
  }
  // ---- A[m][n] over this wave's channels
  float A[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      float a = kn[m][0] * qe[n][0];
#pragma unroll
      for (int r = 1; r < 4; ++r) a = fmaf(kn[m][r], qe[n][r], a);
      A[m][n] = half_sum(row_pair_sum(a));
    }
  // ---- exchange with the other half of the head (wave ^ 1): rows [max 4 | sum 4 | A 16] x 16 samples
  lds_f *ex = (lds_f *)(c.lds + kAttExch);
  if (kq == 0) {
    lds_f *mine = ex + c.wave * 384 + sm;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      mine[16 * n] = qm[n];
      mine[16 * (4 + n)] = qs[n];
#pragma unroll
      for (int m = 0; m < 4; ++m) mine[16 * (8 + 4 * m + n)] = A[m][n];
    }
  }
  __syncthreads();
  const lds_f *oth = ex + (c.wave ^ 1) * 384 + sm;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float mo = oth[16 * n], so = oth[16 * (4 + n)];
    const float m = fmaxf(qm[n], mo);
    const float fs = fast_exp(qm[n] - m), fo = fast_exp(mo - m);
    const float sc = 0.17677669529663687f * __builtin_amdgcn_rcpf(qs[n] * fs + so * fo);   // dim_head ** -0.5 / sum
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) A[mm][n] = (A[mm][n] * fs + oth[16 * (8 + 4 * mm + n)] * fo) * sc;
  }
  // ---- out[e][n] = sum_m v[e][m] A[m][n] for the lane's 4 channels e, as planes (32-channel block = head)
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      o[r] = acc[2][0][r] * A[0][n] + acc[2][1][r] * A[1][n] + acc[2][2][r] * A[2][n] + acc[2][3][r] * A[3][n];
    store_planes4(c.lds + kPlaneH, kDimHead * head + 16 * half + 4 * kq, 16 * n + sm, o[0], o[1], o[2], o[3]);
  }
  __syncthreads();
}

// ---- attention block of the 16-position 64-column engine: qkv_att16_pm (behind quad16_narrow.h, whose core it shares).
// (Rounds 4-5: qkv_ln16_pm + attention16_pm, q | k | v through LDS as a [384][64] f32 block over both plane regions.)
// The four zero entries either side of every plane row (8 blocks x 3 planes x 4 g rows x 8 entries) of the 16-position
// engine.  Two things overwrite them: the f32 rows of the 256-channel level's output (rows 128 .. 255 of X lie over the
// first H-plane blocks) and the weight ring of the wave-local narrow levels (quad16_narrow.h): restored behind each.
__device__ __forceinline__ void zero_plane_pads16(float *lds, int t) {
  using G = PG<16>;
  lds_u4 *pl = (lds_u4 *)(lds + G::kH);
  const u32x4 z4 = u32x4{0u, 0u, 0u, 0u};
  for (int i = t; i < 8 * 12 * 8; i += 512) {
    const int rowi = i >> 3, e8 = i & 7;
    pl[rowi * G::kCols + (e8 < 4 ? e8 : 64 + e8)] = z4;
  }
}

// A whole ResnetBlock of the position-major engine as ONE op: conv1 (GroupNorm, scale/shift, SiLU -> H), barrier, conv2
// (GroupNorm, SiLU, X += ...).  Straight-line code, so the first weight fragments of conv2 can be requested while conv1's
// epilogue runs and be there when its k-loop starts: requested cold at the top of the loop they cost ~1.8 k cycles per
// conv (a build that loads no fragments at all runs the step 8 % faster; across two tape ops the compiler waits for
// such loads at the op switch).  One tape decode and dispatch less, too.
template <int MT, int P0, int NP, int GK, int LL = 4>
__device__ __forceinline__ void resblock_pm_wave(const Ctx &c, const float *wp1, const float *b1, const float *wp2,
                                                 const float *b2, int mt0, float *X, float *H, int C,
                                                 const GnEpilogue &g1, const GnEpilogue &g2, long long *stamp2,
                                                 bool live = true) {
  PreA<MT> pa;
  const WStream wv2(wp2, c.lane);
  const int cin = C < 32 ? 32 : C;   // a 16-channel level is one zero-padded 32-channel block of planes
  auto ask = [&]() { pa.request(wv2, mt0, cin); };
  conv_pm3_wave<MT, P0, NP, GK, 1, NoPreA, decltype(ask), LL>(c, wp1, b1, mt0, X, C, H, C, false, g1, NoPreA(), ask, live);
  __syncthreads();
  if (stamp2 && c.tid == 0) *stamp2 = (long long)__builtin_readcyclecounter();
  conv_pm3_wave<MT, P0, NP, GK, 2, PreA<MT>, NoHook, LL>(c, wp2, b2, mt0, H, C, X, C, false, g2, pa, NoHook(), live);
}
template <int LL = 4>
__device__ __forceinline__ void resblock_pm(const Ctx &c, int w1, int b1, int w2, int b2, float *X, float *H, int C,
                                            const GnEpilogue &g1, const GnEpilogue &g2, long long *stamp2) {
  const float *wp1 = c.w + w1, *bp1 = c.w + b1, *wp2 = c.w + w2, *bp2 = c.w + b2;
  const int w = c.wave;
  if (C == 256) resblock_pm_wave<2, 0, 4, 0, LL>(c, wp1, bp1, wp2, bp2, 2 * w, X, H, C, g1, g2, stamp2);
  else if (C == 128) resblock_pm_wave<1, 0, 4, 0, LL>(c, wp1, bp1, wp2, bp2, w, X, H, C, g1, g2, stamp2);
  else if (C == 64) {
    if (w < 4) resblock_pm_wave<1, 0, 2, 1, LL>(c, wp1, bp1, wp2, bp2, w & 3, X, H, C, g1, g2, stamp2);
    else resblock_pm_wave<1, 2, 2, 1, LL>(c, wp1, bp1, wp2, bp2, w & 3, X, H, C, g1, g2, stamp2);
  } else if (C == 32 || LL == 4) {
    const int pw = w >> 1;
    if (pw == 0) resblock_pm_wave<1, 0, 1, 2, LL>(c, wp1, bp1, wp2, bp2, w & 1, X, H, C, g1, g2, stamp2);
    else if (pw == 1) resblock_pm_wave<1, 1, 1, 2, LL>(c, wp1, bp1, wp2, bp2, w & 1, X, H, C, g1, g2, stamp2);
    else if (pw == 2) resblock_pm_wave<1, 2, 1, 2, LL>(c, wp1, bp1, wp2, bp2, w & 1, X, H, C, g1, g2, stamp2);
    else resblock_pm_wave<1, 3, 1, 2, LL>(c, wp1, bp1, wp2, bp2, w & 1, X, H, C, g1, g2, stamp2);
  } else if constexpr (LL == 16) {   // C = 16: one m-tile, a tile per wave of 0-3; waves 4-7 shadow them
    const int t = w & 3;
    const bool live = w < 4;
    if (t == 0) resblock_pm_wave<1, 0, 1, 3, 16>(c, wp1, bp1, wp2, bp2, 0, X, H, C, g1, g2, stamp2, live);
    else if (t == 1) resblock_pm_wave<1, 1, 1, 3, 16>(c, wp1, bp1, wp2, bp2, 0, X, H, C, g1, g2, stamp2, live);
    else if (t == 2) resblock_pm_wave<1, 2, 1, 3, 16>(c, wp1, bp1, wp2, bp2, 0, X, H, C, g1, g2, stamp2, live);
    else resblock_pm_wave<1, 3, 1, 3, 16>(c, wp1, bp1, wp2, bp2, 0, X, H, C, g1, g2, stamp2, live);
  }
  __syncthreads();
}

// ----------------------------------------------------------- LayerNorm ----
// dst = LN_channels(src) * g  (or res += LN(src) * g when res != null).  Row slot = wave*kRP + sub
// (kSlots = kWaves * kRP of them), rows slot + kSlots i.
template <int NC, int ITERS>
__device__ __forceinline__ void layer_norm_rows(const Ctx &c, const float *src, float *dst, float *res, int C,
                                                int g_off) {
  using GG = Geo<NC>;
  float *red1 = c.lds + GG::kMiscRed1, *red2 = c.lds + GG::kMiscRed2;
  const int n = c.lane & (NC - 1), slot = c.wave * GG::kRP + c.lane / NC;
  const lds_f *s3 = (const lds_f *)src;
  const float *g = c.w + g_off;
  float v[ITERS], gv[ITERS];  // the gains are requested up front: their L2 round trip hides behind the statistics
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float x = s3[swz<NC>(row < C ? row : 0, n)];
    gv[i] = g[row < C ? row : 0];
    v[i] = row < C ? x : 0.f;
    sum += v[i];
  }
  if (GG::kRP == 2) sum = half_sum(sum);
  red1[c.wave * NC + n] = sum;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) tot += red1[q * NC + n];
  const float mean = tot / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float d = row < C ? v[i] - mean : 0.f;
    sq += d * d;
  }
  if (GG::kRP == 2) sq = half_sum(sq);
  red2[c.wave * NC + n] = sq;
  __syncthreads();
  float vt = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) vt += red2[q * NC + n];
  const float rstd = __builtin_amdgcn_rsqf(vt / (float)C + 1e-5f);
  lds_f *d3 = (lds_f *)dst, *r3 = (lds_f *)res;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    if (row < C) {
      const float y = (v[i] - mean) * rstd * gv[i];
      const int a = swz<NC>(row, n);
      if (res) r3[a] = r3[a] + y;
      else d3[a] = y;
    }
  }
  __syncthreads();
}

// One-exchange form for the 64-column engine (lane = column, wave = row slot): every wave reduces its rows to
// (sum, M2 about its own mean), ONE barrier, then the parallel-variance merge of the 8 pairs: two barriers per
// LayerNorm instead of three.
template <int ITERS>
__device__ __forceinline__ void layer_norm_rows_1x(const Ctx &c, const float *src, float *dst, float *res, int C,
                                                   int g_off) {
  constexpr int NC = 64;
  using GG = Geo<NC>;
  lds_f *red1 = (lds_f *)(c.lds + GG::kMiscRed1), *red2 = (lds_f *)(c.lds + GG::kMiscRed2);
  const int n = c.lane, slot = c.wave;
  const lds_f *s3 = (const lds_f *)src;
  const float *g = c.w + g_off;
  float v[ITERS], gv[ITERS];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float x = s3[swz<NC>(row < C ? row : 0, n)];
    gv[i] = g[row < C ? row : 0];
    v[i] = row < C ? x : 0.f;
    sum += v[i];
  }
  const int cnt = slot < C ? (C - slot + GG::kSlots - 1) / GG::kSlots : 0;  // rows of this slot (wave uniform)
  const float mloc = sum * __builtin_amdgcn_rcpf((float)(cnt > 0 ? cnt : 1));  // C, cnt: powers of two -> exact
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float d = row < C ? v[i] - mloc : 0.f;
    m2 += d * d;
  }
  red1[slot * NC + n] = sum;
  red2[slot * NC + n] = m2;
  __syncthreads();
  float tot = 0.f, ps[GG::kWaves], pm[GG::kWaves];
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) {
    ps[q] = red1[q * NC + n];
    pm[q] = red2[q * NC + n];
    tot += ps[q];
  }
  const float inv_c = __builtin_amdgcn_rcpf((float)C);
  const float mean = tot * inv_c;
  float vt = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) {
    const int cq = q < C ? (C - q + GG::kSlots - 1) / GG::kSlots : 0;  // wave uniform
    const float fq = (float)cq, iq = __builtin_amdgcn_rcpf((float)(cq > 0 ? cq : 1));
    const float dm = ps[q] * iq - mean;
    vt += cq > 0 ? pm[q] + fq * dm * dm : 0.f;
  }
  const float rstd = __builtin_amdgcn_rsqf(vt * inv_c + 1e-5f);
  lds_f *d3 = (lds_f *)dst, *r3 = (lds_f *)res;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    if (row < C) {
      const float y = (v[i] - mean) * rstd * gv[i];
      const int a = swz<NC>(row, n);
      if (res) r3[a] = r3[a] + y;
      else d3[a] = y;
    }
  }
  __syncthreads();
}

template <int NC>
__device__ __forceinline__ void layer_norm_pass(const Ctx &c, const float *src, float *dst, float *res, int C, int g_off) {
  if (GLDM_SKIP(c, 2)) return;
  C = __builtin_amdgcn_readfirstlane(C);
  if constexpr (NC == 64) {
    const int it1 = (C + Geo<NC>::kSlots - 1) / Geo<NC>::kSlots;
    if (it1 <= 1) layer_norm_rows_1x<1>(c, src, dst, res, C, g_off);
    else if (it1 <= 4) layer_norm_rows_1x<4>(c, src, dst, res, C, g_off);
    else if (it1 <= 8) layer_norm_rows_1x<8>(c, src, dst, res, C, g_off);
    else layer_norm_rows_1x<16>(c, src, dst, res, C, g_off);
    return;
  }
  const int it = (C + Geo<NC>::kSlots - 1) / Geo<NC>::kSlots;
  if (it <= 1) layer_norm_rows<NC, 1>(c, src, dst, res, C, g_off);
  else if (it <= 2) layer_norm_rows<NC, 2>(c, src, dst, res, C, g_off);
  else if (it <= 4) layer_norm_rows<NC, 4>(c, src, dst, res, C, g_off);
  else if (it <= 8) layer_norm_rows<NC, 8>(c, src, dst, res, C, g_off);
  else layer_norm_rows<NC, 16>(c, src, dst, res, C, g_off);
}

// -------------------------------------------------- linear attention -------
// qkv: [192][NC] = q(2 heads x 32) | k | v for one head pair; writes 64 rows of o.
// (Sample-major 32-column engine; the 64-column engine has attention_pair_pm.)
template <int NC, int L>
__device__ __forceinline__ void attention_pair(const Ctx &c, float *qkv, float *o_rows) {
  if (GLDM_SKIP(c, 4)) return;
  using GG = Geo<NC>;
  static_assert(NC == 32 && GG::kWaves == 4 && (L == 4 || L == 16), "sample-major engine geometry");
  const lds_f *q3 = (const lds_f *)qkv;
  lds_f *o3 = (lds_f *)o_rows;
  if constexpr (L == 4 && NC == 32 && GG::kWaves == 4) {
    // wave = (head of the pair, 16-column half); lane = (column, part): 8 of the head's 32 channels.  The softmax
    // statistics and the 4 x 4 matrix A = softmax_n(k)^T softmax_d(q) combine over the parts with permlane swaps
    // inside the wave: no LDS exchange and no barrier but the final one.
    const int h2 = c.wave >> 1, nn = 16 * (c.wave & 1) + (c.lane & 15), pt = c.lane >> 4, d0 = 8 * pt, sb = nn & ~3;
    const int qr = h2 * kDimHead + d0, kr = 64 + h2 * kDimHead + d0, vr = 128 + h2 * kDimHead + d0;
    float q[8];
    float qmax = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q[i] = q3[swz<NC>(qr + i, nn)];
      qmax = fmaxf(qmax, q[i]);
    }
    f32x4 kv[8], vv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kv[i] = *(const lds_f4 *)(q3 + swz<NC>(kr + i, sb));
#pragma unroll
    for (int i = 0; i < 8; ++i) vv[i] = *(const lds_f4 *)(q3 + swz<NC>(vr + i, sb));
    qmax = half_max(row_pair_max(qmax));
    float qsum = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float e = fast_exp(q[i] - qmax);
      qsum += e;
      const float km = fmaxf(fmaxf(kv[i].x, kv[i].y), fmaxf(kv[i].z, kv[i].w));
      const float k0 = fast_exp(kv[i].x - km), k1 = fast_exp(kv[i].y - km), k2 = fast_exp(kv[i].z - km),
                  k3 = fast_exp(kv[i].w - km);
      const float f = e * __builtin_amdgcn_rcpf(k0 + k1 + k2 + k3);
      a0 += k0 * f; a1 += k1 * f; a2 += k2 * f; a3 += k3 * f;
    }
    qsum = half_sum(row_pair_sum(qsum));
    a0 = half_sum(row_pair_sum(a0)); a1 = half_sum(row_pair_sum(a1));
    a2 = half_sum(row_pair_sum(a2)); a3 = half_sum(row_pair_sum(a3));
    const float sc = 0.17677669529663687f * __builtin_amdgcn_rcpf(qsum);  // dim_head ** -0.5 / sum
    a0 *= sc; a1 *= sc; a2 *= sc; a3 *= sc;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      o3[swz<NC>(h2 * kDimHead + d0 + i, nn)] = vv[i].x * a0 + vv[i].y * a1 + vv[i].z * a2 + vv[i].w * a3;
    __syncthreads();
  } else {
    // L = 16 (pose decoder): 2 samples x 16 positions per tile, 4 waves.  Both softmaxes are normalised in place
    // first (keys over a sample's 16 positions: two lanes per (head, channel, sample); queries over the 32 channels,
    // scaled by dim_head^-0.5: four lanes per (head, column)), then a wave per (head, sample) takes
    // A = Kn^T Qn (16 x 16, K = 32) and out = V A (32 x 16, K = 16) as 16 MFMAs: A's accumulator registers are the
    // B operand of the second product as they stand (k-step r = key positions {4 kq + r}).  (The first form had every
    // lane recompute A with 512 exponentials: 30-80 k cycles per op, a third of the whole decode.)
    static_assert(NC == 32, "decoder tile");
    const int t = c.tid;
    lds_f *w3 = (lds_f *)qkv;
    {
      const int item = t >> 1, half = t & 1, h = item >> 6, d = (item >> 1) & 31, sm = item & 1;
      const int row = 64 + h * kDimHead + d, col0 = sm * 16 + 8 * half;
      float k[8];
      float km = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        k[j] = w3[swz<NC>(row, col0 + j)];
        km = fmaxf(km, k[j]);
      }
      km = dpp_max<0xB1>(km);  // the other half of the sample's positions: lane ^ 1
      float ks = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        k[j] = fast_exp(k[j] - km);
        ks += k[j];
      }
      ks += dpp_mov<0xB1>(ks);
      const float inv = __builtin_amdgcn_rcpf(ks);
#pragma unroll
      for (int j = 0; j < 8; ++j) w3[swz<NC>(row, col0 + j)] = k[j] * inv;
    }
    {
      const int item = t >> 2, qt = t & 3, h = item >> 5, col = item & 31;
      const int row0 = h * kDimHead + 8 * qt;
      float q[8];
      float qm = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q[j] = w3[swz<NC>(row0 + j, col)];
        qm = fmaxf(qm, q[j]);
      }
      qm = dpp_max<0xB1>(qm);
      qm = dpp_max<0x4E>(qm);  // the four channel quarters of a column: one quad
      float qs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q[j] = fast_exp(q[j] - qm);
        qs += q[j];
      }
      qs += dpp_mov<0xB1>(qs);
      qs += dpp_mov<0x4E>(qs);
      const float sc = 0.17677669529663687f * __builtin_amdgcn_rcpf(qs);  // dim_head ** -0.5 / sum
#pragma unroll
      for (int j = 0; j < 8; ++j) w3[swz<NC>(row0 + j, col)] = q[j] * sc;
    }
    __syncthreads();
    const int h = c.wave >> 1, sm = c.wave & 1, m = c.lane & 15, kq = c.lane >> 4;
    f32x4 am = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // channel d = 4 j + kq
      const float ka = q3[swz<NC>(64 + h * kDimHead + 4 * j + kq, sm * 16 + m)];  // Kn^T[key position m][d]
      const float qb = q3[swz<NC>(h * kDimHead + 4 * j + kq, sm * 16 + m)];       // Qn[d][query position m]
      am = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, qb, am, 0, 0, 0);
    }
    // am: lane (query position m, kq), register r = A[key position 4 kq + r][m]
    f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // k-step r: key positions 4 kq + r
      const float v0 = q3[swz<NC>(128 + h * kDimHead + m, sm * 16 + 4 * kq + r)];
      const float v1 = q3[swz<NC>(128 + h * kDimHead + 16 + m, sm * 16 + 4 * kq + r)];
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, am[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, am[r], o1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o3[swz<NC>(h * kDimHead + 4 * kq + r, sm * 16 + m)] = o0[r];
      o3[swz<NC>(h * kDimHead + 16 + 4 * kq + r, sm * 16 + m)] = o1[r];
    }
    __syncthreads();
  }
}

#include "quad_narrow.h"
#include "quad16_narrow.h"

// ---------------------------------------------------------- the network ----
// Step-segment hand-off between workgroups (a tile whose steps are split over a chain of slots).
// The whole state of a tile between two steps is its latent row: NC floats.  Each float travels as ONE
// naturally aligned 8-byte granule {value, tag} written by one write-through (agent-scope) store and
// polled with agent-scope loads: a granule is never torn, so no fence, flag or ordering between
// granules is needed (MI355X_MICROARCH.md, "R2's granule").  tag = (launch epoch, step count) is
// unique per launch and step; the zero-initialised workspace holds tag 0, which no hand-off uses.
struct ChainHdr { unsigned ticket, done, epoch, error; };
constexpr int kChainHdrBytes = 256;
constexpr int kParkBytes = 256 * 64 * 4;   // one [256][64] f32 tile per workgroup (Ctx::park)
__device__ __forceinline__ unsigned chain_tag(unsigned epoch, int step) { return (epoch << 12) | (unsigned)step; }
__device__ __forceinline__ void chain_give(unsigned long long *g, float v, unsigned tag) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float chain_take(unsigned long long *g, unsigned tag, unsigned *error) {
  unsigned long long x = 0;
  for (int spin = 0; spin < (1 << 22); ++spin) {  // bounded: ~2 s; a healthy wait is a few ms at most
    x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)(x >> 32) == tag) return __uint_as_float((unsigned)x);
    __builtin_amdgcn_s_sleep(16);
  }
  // The wait expired: the tile's latent is lost.  The error word is what the host reads (R1dEngine checks it after
  // every chained launch and raises); the NaN makes every output of this tile NaN whether or not anyone looks.
  __hip_atomic_store(error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_nanf("");
}

struct RunArgs {
  gldm_r1d_desc d;
  const float *weights;
  const float *temb;      // [T][E] or null
  const float *cemb;      // [n_cond][R][E]
  const float *semb;      // [n][E] per-sample embedding added to the time embedding (class conditioning), or null
  int samples_per_cond;
  const float *x_in;      // denoise: [n][L]; decode: z_h [n][D]
  int n_samples;
  const int32_t *timesteps;
  const int32_t *sample_t;
  int n_steps;
  int sched_kind, clip_sample;
  const float *sched_coef;
  const float *step_noise;
  // DDPM noise drawn IN the kernel when step_noise is null and noise_on is set: unit normals from Philox4x32-10 keyed on
  // noise_seed, counter = (global latent index noise_base + gi, position block, step): independent of tiling, batch
  // split and world size by construction
  unsigned long long noise_seed;
  long long noise_base;
  int noise_on;
  float *out0;            // denoise: x_out [n][L]; decode: tmrp [n][6]
  float *out1;            // decode: logit [n]; encode: logvar [n][Lz]
  // encode (GLDM_HEAD_ENCODER; out0 = mu [n][Lz]): z = mix_mu mu + mix_eps eps (exp(logvar / 2) if eps_times_std), or null
  float *out2;
  const float *eps;       // [n][Lz] or null
  float mix_mu, mix_eps;
  int eps_times_std;
  float *ws;              // workspace: chain header + hand-off granules (+ the decoder's scale/shift table)
  float *park;            // position-major engine with a 256-channel last level: 64 KiB of scratch per workgroup (Ctx::park)
  const float *ss_tab;    // [n_cond][ss_stride] scale/shift rows of every ResnetBlock per conditioning cloud, or null
  int ss_stride;
  int skip;               // diagnostic phase-skip mask (GLDM_R1D_SKIP env; 0 in production)
  // Work distribution (make_plan): `slots` persistent workgroups; slot p owns tiles p, p + slots, ... (`rounds` of
  // them) for all steps; each of the `left_tiles` tiles beyond the whole rounds is cut into `chain` step segments of
  // `seglen` steps that consecutive slots run one after the other, handing the latent on through the workspace.
  int slots, rounds, left_tiles, chain, seglen;
  int stagger_ticks, n_cus;  // start offset (100 MHz ticks) of the second workgroup of a CU
  long long *stamps;         // diagnostic (GLDM_R1D_STAMP): cycle counter at every op of the last step, block 0
  // Position-major engine: the step program, built on the host (launch_r1d), travels in the kernel arguments: an op's
  // 12 ints are three scalar loads from the kernarg segment, straight into SGPRs.  (From the LDS copy the interpreter
  // paid three ds_read_b128, their latency and 12 v_readfirstlane per op -- ~0.7 k cycles on every wave, 28 ops a step.)
  int pm_nops;
  int pm_tape[kPmMaxOps * kOpInts];
};

// One denoiser / decoder step is a fixed program of barrier-separated ops (45 for the shipped
// denoiser: per level 2 x [conv+GN, conv+GN+residual], LN, 2 x [qkv conv, attention], out conv, LN,
// down conv).  It is written once per workgroup into LDS (12 ints per op) and interpreted by a switch
// inside the step loop, so every phase body exists once, inlined, with registers allocated across the
// whole kernel: no calls, no callee-save traffic and no spilled kernel state between phases.
enum { OP_CONV = 1, OP_RES4 = 2, OP_LN = 3, OP_ATT = 4, OP_QKVLN = 5, OP_OUTLN = 6, OP_QKVATT = 7, OP_QUAD = 8 };
// The levels of 4, 32 and 64 channels in front of a 128-channel one run wave-local (quad_narrow.h): the shipped denoiser
__host__ __device__ __forceinline__ bool quad_levels(const gldm_r1d_desc &d) {
  return d.seq_len == 4 && d.emb_dim == 16 && d.n_levels >= 3 && d.dims[0] == 4 && d.dims[1] == 32 && d.dims[2] == 64 &&
         d.dims[3] == 128 && d.lv[0].out_wq > 0 && d.lv[1].out_wq > 0 && d.lv[1].qkvn_wq > 0 && d.lv[1].down_wq > 0 &&
         d.lv[2].out_wq > 0 && d.lv[2].qkvn_wq > 0 && d.lv[2].down_wq > 0 && d.rb[2].c1_wq > 0 && d.rb[2].c2_wq > 0 &&
         d.rb[3].c1_wq > 0 && d.rb[3].c2_wq > 0 && d.rb[4].c1_wq > 0 && d.rb[4].c2_wq > 0 && d.rb[5].c1_wq > 0 && d.rb[5].c2_wq > 0;
}
// The same for the 16-position nets (quad16_narrow.h): levels of 16, 32 and 64 channels in front of a 128-channel one.  The
// scale / shift rows come from the per-cloud table (pose decoder: ss_table_rows) or the 64-wide embedding (the launcher
// checks that one of the two holds).
__host__ __device__ __forceinline__ bool quad16_levels(const gldm_r1d_desc &d) {
  return d.seq_len == 16 && d.groups == 4 && d.n_levels >= 3 && d.dims[0] == 16 && d.dims[1] == 32 && d.dims[2] == 64 && d.dims[3] == 128 &&
         d.lv[0].out_wq > 0 && d.lv[0].qkvn_wq > 0 && d.lv[0].down_wq > 0 && d.lv[1].out_wq > 0 && d.lv[1].qkvn_wq > 0 &&
         d.lv[1].down_wq > 0 && d.lv[2].out_wq > 0 && d.lv[2].qkvn_wq > 0 && d.lv[2].down_wq > 0 && d.rb[0].c1_wq > 0 &&
         d.rb[0].c2_wq > 0 && d.rb[1].c1_wq > 0 && d.rb[1].c2_wq > 0 && d.rb[2].c1_wq > 0 && d.rb[2].c2_wq > 0 && d.rb[3].c1_wq > 0 &&
         d.rb[3].c2_wq > 0 && d.rb[4].c1_wq > 0 && d.rb[4].c2_wq > 0 && d.rb[5].c1_wq > 0 && d.rb[5].c2_wq > 0;
}
// conv flags (int 7): taps | alias << 8 | GroupNorm epilogue mode << 9 | (scale/shift table offset / 4) << 12
constexpr int kFlagAlias = 1 << 8;
constexpr int kFlagFused = 1 << 11;   // position-major engine: this conv and the next tape entry are one ResnetBlock op
constexpr int kFlagTabShift = 12;

// ResnetBlock of a 4-channel level with 4-position samples (the first level of the latent denoiser) on the
// VALU of ONE wave, in registers: as two MFMA ops it is two padded 16x16 tiles and two long epilogues for
// 48 MACs per output.  lane = (channel pair h, column n): every lane keeps all 4 input channels of its column
// and produces output channels 2h, 2h+1.  Taps come from the neighbouring lanes of the quad (= the sample),
// GroupNorm (one channel per group) is a quad reduction, the two channel pairs meet through a permlane swap.
// Weights are read in their packed MFMA-fragment order: conv W[co][ci][tap] at ((ci * 16 + co) * 4 + tap),
// scale/shift Linear W[row][e] at (((e & 3) * 16 + row) * 4 + (e >> 2)).
template <int NC>
__device__ __forceinline__ void resblock4_valu(const Ctx &c, const int (&o)[kOpInts], int E) {
  using GG = Geo<NC>;
  if (c.wave != 0) return;
  const int n = c.lane & 31, h = c.lane >> 5, l = n & 3;
  const bool has_l = l != 0, has_r = l != 3;
  lds_f *X = (lds_f *)(c.lds + GG::kBufX);
  const lds_f *G = (const lds_f *)(c.lds + GG::kMiscG) + (n >> 2) * E;
  const float *w = c.w;
  const int c1_w = o[1], c1_b = o[2], n1_w = o[3], n1_b = o[4], c2_w = o[5], c2_b = o[6], n2_w = o[7], n2_b = o[8],
            ss_w = o[9], ss_b = o[10];
  // ---- every parameter of the block is requested up front (one L2 round trip for all of them)
  f32x4 wss[4][2][2], wc1[4][2], wc2[4][2];
  float bss[2][2], bc1[2], bc2[2], g1[2], b1[2], g2[2], b2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int co = 2 * h + k;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      wss[kq][k][0] = *reinterpret_cast<const f32x4 *>(w + ss_w + (kq * 16 + co) * 4);      // scale row co
      wss[kq][k][1] = *reinterpret_cast<const f32x4 *>(w + ss_w + (kq * 16 + 4 + co) * 4);  // shift row 4 + co
      wc1[kq][k] = *reinterpret_cast<const f32x4 *>(w + c1_w + (kq * 16 + co) * 4);         // kq = input channel
      wc2[kq][k] = *reinterpret_cast<const f32x4 *>(w + c2_w + (kq * 16 + co) * 4);
    }
    bss[k][0] = w[ss_b + co]; bss[k][1] = w[ss_b + 4 + co];
    bc1[k] = w[c1_b + co]; bc2[k] = w[c2_b + co];
    g1[k] = w[n1_w + co]; b1[k] = w[n1_b + co]; g2[k] = w[n2_w + co]; b2[k] = w[n2_b + co];
  }
  float x[4];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) x[ci] = X[swz<NC>(ci, n)];
  // ---- scale / shift of my two channels: rows 2h + k (scale, the +1 is in the packed bias) and 4 + 2h + k (shift)
  float sc[2], sh[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    sc[k] = bss[k][0];
    sh[k] = bss[k][1];
  }
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) {
    f32x4 gq = f32x4{0.f, 0.f, 0.f, 0.f};  // G[4 j + kq], j = 0..3 (E = 16: the whole embedding)
#pragma unroll
    for (int j = 0; j < 4; ++j) gq[j] = 4 * j + kq < E ? G[4 * j + kq] : 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[k] += wss[kq][k][0][j] * gq[j];
        sh[k] += wss[kq][k][1][j] * gq[j];
      }
  }
  auto conv3 = [&](const float (&in)[4], const f32x4 (&wc)[4][2], const float (&bc)[2], float (&out)[2]) {
    float lft[4], rgt[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const float a = dpp_mov<0x90>(in[ci]), b = dpp_mov<0xF9>(in[ci]);  // quad_perm [0,0,1,2] / [1,2,3,3]
      lft[ci] = has_l ? a : 0.f;
      rgt[ci] = has_r ? b : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float acc = bc[k];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        acc += wc[ci][k].x * lft[ci];
        acc += wc[ci][k].y * in[ci];
        acc += wc[ci][k].z * rgt[ci];
      }
      out[k] = acc;
    }
  };
  auto gn_act = [&](float (&v)[2], const float (&gw)[2], const float (&gb)[2], bool ss) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float m = group_sum<4>(v[k]) * 0.25f;
      const float d = v[k] - m;
      const float rs = __builtin_amdgcn_rsqf(group_sum<4>(d * d) * 0.25f + 1e-5f);
      float y = d * rs * gw[k] + gb[k];
      if (ss) y = y * sc[k] + sh[k];
      v[k] = silu(y);
    }
  };
  auto gather4 = [&](const float (&mine)[2], float (&all)[4]) {  // channels 0,1 live in half 0, channels 2,3 in half 1
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine[k]), __float_as_uint(mine[k]), false, false);
      all[k] = __uint_as_float(r[0]);      // [lo, lo]: half 0's value in both halves
      all[2 + k] = __uint_as_float(r[1]);  // [hi, hi]
    }
  };
  float y[2], ya[4], z[2];
  conv3(x, wc1, bc1, y);
  gn_act(y, g1, b1, !GLDM_SKIP(c, 16));
  gather4(y, ya);
  conv3(ya, wc2, bc2, z);
  gn_act(z, g2, b2, false);
#pragma unroll
  for (int k = 0; k < 2; ++k) X[swz<NC>(2 * h + k, n)] = x[2 * h + k] + z[k];
}

// GroupNorm rides in the conv epilogue: the rows of a group must sit inside one wave's accumulators
__host__ __device__ __forceinline__ bool gn_fusable(int C, int groups) {
  if (groups != 4 || C % 4) return false;
  const int cpg = C / 4;
  return cpg == 1 || cpg == 4 || cpg == 8 || (cpg % 16 == 0 && cpg <= 64);
}

template <int NC>
__host__ __device__ __forceinline__ int build_tape(const gldm_r1d_desc &d, int *tape, bool use_quad = true) {
  using GG = Geo<NC>;
  int n = 0;
  auto emit = [&](int type, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0, int a6 = 0, int a7 = 0,
                  int a8 = 0, int a9 = 0, int a10 = 0, int a11 = 0) {
    int *o = tape + kOpInts * n++;
    o[0] = type; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4; o[5] = a5; o[6] = a6; o[7] = a7;
    o[8] = a8; o[9] = a9; o[10] = a10; o[11] = a11;
  };
  constexpr int X = GG::kBufX, H = GG::kBufH, Y = GG::kBufY, O = GG::kBufO, QKV = GG::kBufQKV;
  int tab_off = 0;  // rows [2C] of every ResnetBlock, in block order (ss_table_kernel writes the same layout)
  auto resblock = [&](const gldm_r1d_resblock &rb, int C, bool last_of_pair) {
    const int toff = tab_off;
    tab_off += 2 * C;
    if (C == 4 && d.seq_len == 4) {  // one-wave VALU form; the barrier comes after the second block
      emit(OP_RES4, rb.c1_w, rb.c1_b, rb.n1_w, rb.n1_b, rb.c2_w, rb.c2_b, rb.n2_w, rb.n2_b, rb.ss_w, rb.ss_b,
           last_of_pair ? 1 : 0);
      return;
    }
    // the position-major engine reads the split-f16 copies of the conv weights (gemm_pm3_bf)
    emit(OP_CONV, NC == 64 ? rb.c1_w3 : rb.c1_w, rb.c1_b, X, H, C, C,
         3 | (1 << 9) | (NC == 64 ? kFlagFused : 0) | ((toff >> 2) << kFlagTabShift), rb.n1_w, rb.n1_b, rb.ss_w, rb.ss_b);
    emit(OP_CONV, NC == 64 ? rb.c2_w3 : rb.c2_w, rb.c2_b, H, X, C, C, 3 | (2 << 9), rb.n2_w, rb.n2_b, -1, 0);  // X += act(GN(conv(H)))
  };
  const bool quad = NC == 64 && use_quad && (quad_levels(d) || quad16_levels(d));
  if (quad) emit(OP_QUAD);
  // constant indices only: a dynamically indexed kernel argument is copied to scratch memory
#pragma unroll
  for (int lv = 0; lv < GLDM_R1D_MAX_LEVELS; ++lv) {
    if (quad && lv < 3) { tab_off += 4 * d.dims[lv]; continue; }   // two ResnetBlocks' table rows each (16-position engine only)
    if (lv < d.n_levels) {
      const int C = d.dims[lv], Cn = d.dims[lv + 1];
      resblock(d.rb[2 * lv], C, false);
      resblock(d.rb[2 * lv + 1], C, true);
      const gldm_r1d_level &v = d.lv[lv];
      // position-major engine (C <= 128 at attention levels): X rows [0, 128) | q,k,v of the four heads: 384 rows, o in
      // place of q.  The PreNorm LayerNorm is folded into the qkv conv (C = 4: computed in the lanes of the qkv phase).
      int Oa = O;
      if (NC == 64) {   // PreNorm + to_qkv + attention core of the four heads: one op, the output as planes (kPlaneH)
        emit(OP_QKVATT, C == 4 ? v.qkvn_w : v.qkvn_w3, v.qkvn_s, X, C);
        Oa = kPlaneH;
      } else {
        emit(OP_LN, X, Y, -1, C, v.ln_g);
        emit(OP_CONV, v.qkv_w[0], -1, Y, QKV, C, 192, 1);
        emit(OP_ATT, QKV, O);
        emit(OP_CONV, v.qkv_w[1], -1, Y, QKV, C, 192, 1);
        emit(OP_ATT, QKV, O + 64 * NC);
      }
      if (NC == 64 && (C == 4 || C == 16 || C == 32 || C == 64 || C == 128)) {  // to_out conv + LayerNorm + residual: one phase
        emit(OP_OUTLN, v.out_w3, v.out_b, Oa, X, kHidden, C, v.ln2_g);
      } else {
        emit(OP_CONV, v.out_w, v.out_b, Oa, Y, kHidden, C, 1);
        emit(OP_LN, Y, -1, X, C, v.ln2_g);
      }
      emit(OP_CONV, (NC == 64 && C >= 16) ? v.down_w3 : v.down_w, v.down_b, X, X, C, Cn, 3 | kFlagAlias);
    }
  }
#pragma unroll
  for (int lv = 1; lv <= GLDM_R1D_MAX_LEVELS; ++lv)
    if (lv == d.n_levels) resblock(d.rb[2 * lv], d.dims[lv], true);
  return n;
}

// One tape entry -> 12 wave-uniform ints.  LDS tape (sample-major engines): three 16-byte reads + v_readfirstlane;
// kernarg tape (position-major engine): scalar loads from the constant address space, no vector instruction at all.
typedef __attribute__((address_space(4))) const int kernarg_int;
typedef __attribute__((ext_vector_type(4))) int i32x4;
template <bool KARG>
__device__ __forceinline__ void read_op(const int *tape, kernarg_int *ktape, int op, int (&o)[kOpInts]) {
  if constexpr (KARG) {
    typedef __attribute__((address_space(4))) const i32x4 kernarg_i4;
    kernarg_i4 *t4 = reinterpret_cast<kernarg_i4 *>(ktape + kOpInts * op);
    const i32x4 q0 = t4[0], q1 = t4[1], q2 = t4[2];
    o[0] = q0.x; o[1] = q0.y; o[2] = q0.z; o[3] = q0.w; o[4] = q1.x; o[5] = q1.y; o[6] = q1.z; o[7] = q1.w;
    o[8] = q2.x; o[9] = q2.y; o[10] = q2.z; o[11] = q2.w;
  } else {
    const int4 *t4 = reinterpret_cast<const int4 *>(tape + kOpInts * op);
    const int4 q0 = t4[0], q1 = t4[1], q2 = t4[2];
    o[0] = q0.x; o[1] = q0.y; o[2] = q0.z; o[3] = q0.w; o[4] = q1.x; o[5] = q1.y; o[6] = q1.z; o[7] = q1.w;
    o[8] = q2.x; o[9] = q2.y; o[10] = q2.z; o[11] = q2.w;
#pragma unroll
    for (int i = 0; i < kOpInts; ++i) o[i] = __builtin_amdgcn_readfirstlane(o[i]);
  }
}

// ---- PreNorm + to_qkv + attention core of the 16-position 64-column engine as ONE op (round 6) ---------------------------
// Until round 6 this was two ops: qkv_ln16_pm wrote q | k | v as a [384][64] f32 block over both plane regions and
// attention16_pm worked from there (three barriers, 96 KiB through ds_write_b32 and back, the plane rows' zero entries
// restored behind it): 25 k of a 236 k-cycle pass at 128 channels.  The wave-local chain of the narrow levels
// (quad16_narrow.h) keeps a (head, sample) pair's q, k and v on the accumulators; the same holds here once the GEMM is dealt
// by PAIRS instead of by rows: wave w = head w >> 1, samples 2 (w & 1) and 2 (w & 1) + 1; an n-tile is one SAMPLE's 16 positions
// (columns 4 p + s of the engine's layout, p = lane & 15: the B fragment reads stride over the plane row), its six m-tiles the
// head's q, k and v rows (to_qkv's own order: m-tiles 2 h + half, + 8, + 16), v with the MFMA operands swapped so that it
// arrives transposed (quad16_attention_head).  LayerNorm folded into the conv as before (W' = W diag(g), s = W' 1: rstd
// (W' x - mean s), the column statistics taken by column_stats8 under the first fragment loads and applied behind ONE barrier);
// q and k leave multiplied by log2(e) for the core's 2^x.  The output goes to the H planes (head h = 32-channel block h) for
// out_ln_pm, as before.  Nothing overwrites a plane region any more.
// Same MFMA count as the row split (144 per wave at 128 channels); a wave now draws six m-tiles' fragments for two n-tiles
// instead of three for four (the head's pair of waves share them in L1).
template <int KB32>   // ceil(C / 32): a 16-channel level is one zero-padded block
__device__ __forceinline__ void qkv_att16_pm(const Ctx &c, int w_off, int s_off, const float *src, int C) {
  using GG = Geo<64>;
  using PGx = PG<16>;
  const float *wp = c.w + w_off, *srow = c.w + s_off;
  const int h = c.wave >> 1, s0 = 2 * (c.wave & 1);
  const int p = c.lane & 15, g = c.lane >> 4;
  const WStream wv(wp, c.lane);
  // m-tile of accumulator i = 2 part + half: rows 128 part + 32 h + 16 half ..
  auto mtile = [&](int i) { return 8 * (i >> 1) + 2 * h + (i & 1); };
  const lds_u4 *pl3 = (const lds_u4 *)(c.lds + PGx::kX) + g * PGx::kCols + PGx::kOff + 4 * p + s0;
  // One set of fragment registers: m-tile i's are refilled with the next block's behind the matrix instructions of m-tile
  // i + 1 (a load into registers the pipe is still reading waits for it; double buffered, 96 registers of fragments beside 48
  // accumulators, the op spilled 46).
  u32x4 a[6][kSplit], bs[2][kSplit];
  f32x4 acc[6][2];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int e = 0; e < 2; ++e) acc[i][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto load_a = [&](int i, int kb) {
    const int sb = (mtile(i) * KB32 + kb) * kFragBytes;
#pragma unroll
    for (int pl = 0; pl < kSplit; ++pl) a[i][pl] = wv.raw_at(sb, pl * 1024);
  };
#pragma unroll
  for (int i = 0; i < 6; ++i) load_a(i, 0);
  __builtin_amdgcn_sched_barrier(0);
  {
    const float inv_c = __builtin_amdgcn_rcpf((float)C);  // C: a power of two -> exact
    if (C == 16) column_stats8<2>(c, src, inv_c);
    else column_stats8<4 * KB32>(c, src, inv_c);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int kb = 0; kb < KB32; ++kb) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) bs[e][pl] = pl3[(kb * kSplit + pl) * PGx::kPlaneU4 + e];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (i < 4) acc[i][e] = mfma_split(a[i], bs[e], acc[i][e]);
        else acc[i][e] = mfma_split(bs[e], a[i], acc[i][e]);   // v^T: rows = positions, columns = v rows
      }
      __builtin_amdgcn_sched_barrier(0);
      if (kb + 1 < KB32 && i >= 1) load_a(i - 1, kb + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kb + 1 < KB32) load_a(5, kb + 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  f32x4 sv[4];   // s of the q and k rows 4 g + r of the wave's m-tiles; of the v rows: one per lane (row lane & 15)
#pragma unroll
  for (int i = 0; i < 4; ++i) sv[i] = *reinterpret_cast<const f32x4 *>(srow + 16 * mtile(i) + 4 * g);
  const float svv[2] = {srow[16 * mtile(4) + p], srow[16 * mtile(5) + p]};
  __syncthreads();  // every column's (mean, rstd) is in LDS
  const lds_f *mean3 = (const lds_f *)(c.lds + GG::kMiscRed1), *rstd3 = (const lds_f *)(c.lds + GG::kMiscRed2);
  constexpr float kL2e = 1.44269504088896340736f;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int sm = s0 + e;
    {   // q, k: the lane's column is position p of the sample
      const float rstd = rstd3[4 * p + sm];
      const float mr = mean3[4 * p + sm] * rstd;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][e][r] = (acc[i][e][r] * rstd - mr * sv[i][r]) * kL2e;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // v^T: register r is position 4 g + r
      const float rstd = rstd3[4 * (4 * g + r) + sm];
      const float mr = mean3[4 * (4 * g + r) + sm] * rstd;
      acc[4][e][r] = acc[4][e][r] * rstd - mr * svv[0];
      acc[5][e][r] = acc[5][e][r] * rstd - mr * svv[1];
    }
    const f32x4 qa[2] = {acc[0][e], acc[1][e]}, ka[2] = {acc[2][e], acc[3][e]}, vt[2] = {acc[4][e], acc[5][e]};
    f32x4 o[2];
    quad16_attention_head(qa, ka, vt, o);
#pragma unroll
    for (int u = 0; u < 2; ++u)   // o[u][r]: channel 16 u + 4 g + r of head h at position p of sample sm
      store_planes4<16>(c.lds + PGx::kH, kDimHead * h + 16 * u + 4 * g, 4 * p + sm, o[u][0], o[u][1], o[u][2], o[u][3]);
  }
  __syncthreads();
}

template <int NC, int L>
__device__ __forceinline__ void run_tape(const Ctx &c0, const gldm_r1d_desc &d, const int *tape, kernarg_int *ktape, int n_ops, int E, long long *stamps) {
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_LDS_TAPE)   // A/B experiment: the tape from LDS as before
  constexpr bool KARG = false;
#else
  constexpr bool KARG = NC == 64;
#endif
  for (int op = 0; op < n_ops; ++op) {
    if (stamps && c0.tid == 0) stamps[op] = (long long)__builtin_readcyclecounter();
    // the lane ids are laundered per op: otherwise every variant's lane-derived LDS offsets are
    // hoisted out of the step loop as invariants and live (spilled) across the whole kernel
    Ctx c = c0;
    asm volatile("" : "+v"(c.tid), "+v"(c.lane));
    int o[kOpInts];
    read_op<KARG>(tape, ktape, op, o);
    // the short latency-bound phases get issue priority over the co-resident workgroup's long MFMA
    // streams (which need one issue slot per 32 cycles and lose nothing)
    if (o[0] == OP_CONV && o[5] * o[6] >= 128 * 128) __builtin_amdgcn_s_setprio(0);
    else __builtin_amdgcn_s_setprio(3);
    switch (o[0]) {
      case OP_CONV: {
        if constexpr (NC == 64) {
          if (o[7] & kFlagFused) {   // ResnetBlock: this entry is conv1, the next one conv2 (same width, H -> X)
            int q[kOpInts];
            read_op<KARG>(tape, ktape, op + 1, q);
            const GnEpilogue g1{1, o[8], o[9], o[10], o[11], E, o[6], o[6] / 4, c.lds + o[4], (o[7] >> kFlagTabShift) << 2};
            const GnEpilogue g2{2, q[8], q[9], -1, 0, E, q[6], q[6] / 4, c.lds + q[4], 0};
            resblock_pm<L == 16 ? 16 : 4>(c, o[1], o[2], q[1], q[2], c.lds + o[3], c.lds + o[4], o[6], g1, g2, stamps ? stamps + op + 1 : nullptr);
            ++op;
            break;
          }
        }
        const int mode = GLDM_SKIP(c, 1) ? 0 : (o[7] >> 9) & 3;
        const GnEpilogue g{mode, o[8], o[9], GLDM_SKIP(c, 16) ? -1 : o[10], o[11], E, o[6], o[6] / 4, c.lds + o[4],
                           (o[7] >> kFlagTabShift) << 2};
        conv_gemm<NC, L>(c, o[1], o[2], c.lds + o[3], o[5], o[7] & 255, c.lds + o[4], o[6], (o[7] & kFlagAlias) != 0, 0, g);
        break;
      }
      case OP_QUAD:
        if constexpr (NC == 64 && L == 4) {
          if (c.wave < 4)
            quad_narrow_levels(c, (kernarg_desc *)((__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr() +
                                                    offsetof(RunArgs, d)));
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_QEXP_DUP)
          // timing experiment (wrong results): GLDM_QEXP_DUP=2 -> waves 4-7 run the chain of quads 0-3 a second time beside
          // them (two compute waves per SIMD); =1 -> they do nothing (one compute wave per SIMD, no loader)
          else if (GLDM_QEXP_DUP == 2)
            quad_narrow_levels(c, (kernarg_desc *)((__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr() +
                                                    offsetof(RunArgs, d)));
#else
          else quad_loader(c);
#endif
          __syncthreads();
        } else if constexpr (NC == 64 && L == 16) {
          kernarg_desc *dkp = (kernarg_desc *)((__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr() +
                                               offsetof(RunArgs, d));
          const float *sstab;   // the wave's sample's scale / shift rows of the six narrow ResnetBlocks
          if (c.ss_lane) {   // pose decoder: the per-cloud table (wave uniform: the launch has one or not); Ctx::ss_lane of a
                             // lane whose sample (lane & 3) is the wave's
            const unsigned long long pv = (unsigned long long)c.ss_lane;
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)pv, c.wave & 3);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(pv >> 32), c.wave & 3);
            sstab = (const float *)(((unsigned long long)hi << 32) | lo);
          } else {   // time-conditioned net: the step's rows by all eight waves first, into LDS behind the ring
            quad16_ss_rows(c, dkp);
            __syncthreads();
            sstab = c.lds + kQ16SsLds + (c.wave & 3) * kQ16SsRows;
          }
          if (c.wave < 4) quad16_narrow_levels<1>(c, dkp, sstab);
          else quad_loader<QStream16<1>>(c);
          __syncthreads();
          zero_plane_pads16(c.lds, c.tid);   // the ring's slots lie over the H plane rows (conv2 of the next ResnetBlock reads them behind a barrier)
        }
        break;
      case OP_RES4:
        if (!GLDM_SKIP(c, 8)) {
          if constexpr (NC == 64 && L == 4) resblock4_pm(c, o, E);
          else if constexpr (NC != 64) resblock4_valu<NC>(c, o, E);
        }
        if (o[11]) __syncthreads();
        break;
      case OP_QKVATT:
        if constexpr (NC == 64) {
          if (o[4] == 128) {   // the 128-channel level: this op and the to_out op behind it as one case (see out_ln_request)
            int q[kOpInts];
            read_op<KARG>(tape, ktape, op + 1, q);
            if (q[0] == OP_OUTLN && q[6] == 128) {
              const Frag3 first = out_ln_request(c, q[1]);
              if constexpr (L == 4) qkv_att_pm<4>(c, o[1], o[2], c.lds + o[3], o[4]);
              else qkv_att16_pm<4>(c, o[1], o[2], c.lds + o[3], o[4]);
              ++op;
              if (stamps && c0.tid == 0) stamps[op] = (long long)__builtin_readcyclecounter();
              out_ln_pm128<L == 16 ? 16 : 4>(c, q[1], q[2], c.lds + q[3], q[5], c.lds + q[4], q[7], first);
              break;
            }
          }
        }
        if constexpr (NC == 64 && L == 4) {
          if (o[4] == 128) qkv_att_pm<4>(c, o[1], o[2], c.lds + o[3], o[4]);
          else if (o[4] == 64) qkv_att_pm<2>(c, o[1], o[2], c.lds + o[3], o[4]);
          else if (o[4] == 32) qkv_att_pm<1>(c, o[1], o[2], c.lds + o[3], o[4]);
          else qkv_att_pm<0>(c, o[1], o[2], c.lds + o[3], o[4]);
        } else if constexpr (NC == 64 && L == 16) {
          if (o[4] == 128) qkv_att16_pm<4>(c, o[1], o[2], c.lds + o[3], o[4]);
          else if (o[4] == 64) qkv_att16_pm<2>(c, o[1], o[2], c.lds + o[3], o[4]);
          else qkv_att16_pm<1>(c, o[1], o[2], c.lds + o[3], o[4]);
        }
        break;
      case OP_OUTLN:
        if constexpr (NC == 64) out_ln_pm<L == 16 ? 16 : 4>(c, o[1], o[2], c.lds + o[3], o[5], c.lds + o[4], o[6], o[7]);
        break;
      case OP_LN:
        layer_norm_pass<NC>(c, c.lds + o[1], o[2] >= 0 ? c.lds + o[2] : nullptr, o[3] >= 0 ? c.lds + o[3] : nullptr,
                            o[4], o[5]);
        break;
      default:
        if constexpr (NC != 64) attention_pair<NC, L>(c, c.lds + o[1], c.lds + o[2]);
        break;
    }
  }
}

// Philox4x32-10 (Salmon et al., SC'11: the counter-based generator of curand / torch's device RNG) and Box-Muller: four
// unit normals per (key, counter).  z[0..3] of counter (latent, position block, step) are positions 4 block + 0..3.
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3, float (&z)[4]) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const unsigned u[4] = {c0, c1, c2, c3};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float a = ((float)u[2 * h] + 1.0f) * 2.3283064365386963e-10f;   // (0, 1]
    const float ang = (float)u[2 * h + 1] * (6.283185307179586f * 2.3283064365386963e-10f);
    const float rad = sqrtf(-2.0f * __logf(a));
    z[2 * h] = rad * __cosf(ang);
    z[2 * h + 1] = rad * __sinf(ang);
  }
}

#pragma clang fp contract(off)
// DPM-Solver++(2M) step of ElucidatedDiffusion.sample_using_dpmpp (elucidated_diffusion.py:259-313) on one element:
// denoised = c_skip x + c_out net (:134, optional clamp :137); denoised_d = (1 - gamma) denoised + gamma old (:303);
// x' = (sigma_next / sigma) x - expm1(-h) denoised_d (:305).  cf = [c_in, c_skip, c_out, 1 - gamma, gamma,
// sigma_fn(t_next) / sigma_fn(t), expm1(-h), use_old].  Every operation rounds once, in the reference's order.
__device__ __forceinline__ float dpmpp_update(int clamp, const float *cf, float x, float net, float *old) {
  const float a = cf[1] * x;
  const float b = cf[2] * net;
  float den = a + b;
  if (clamp) den = fminf(fmaxf(den, -1.0f), 1.0f);
  float d = den;
  if (cf[7] != 0.f) {
    const float p = cf[3] * den;
    const float q = cf[4] * *old;
    d = p + q;
  }
  *old = den;
  const float u = cf[5] * x;
  const float v = cf[6] * d;
  return u - v;
}

__device__ __forceinline__ float scheduler_update(int kind, int clip, const float *cf, float x, float eps, float noise) {
  float x0 = (x - cf[0] * eps) / cf[1];
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  if (kind == GLDM_SCHED_DDIM) {
    const float a = cf[2] * x0;
    const float b = cf[3] * eps;
    return a + b;
  }
  const float a = cf[4] * x0;
  const float b = cf[5] * x;
  float prev = a + b;
  if (cf[7] != 0.f) {
    const float nz = cf[6] * noise;
    prev = prev + nz;
  }
  return prev;
}
#pragma clang fp contract(fast)

template <int NC, int L>
__global__ __launch_bounds__(Geo<NC>::kThreads, 2) void r1d_kernel(const RunArgs a) {
  using GG = Geo<NC>;
  extern __shared__ float lds[];
  const gldm_r1d_desc &d = a.d;
  constexpr int S = NC / L;
  // column <-> (sample, position): sample-major tiles (column = sample * L + position) or, for the 64-column
  // engine of the L = 4 denoiser, position-major ones (column = 16 * position + sample)
  // (4 positions: column = 16 * position + sample, 16 samples) or of the 16-position nets (column = 4 * position + sample,
  // 4 samples)
  constexpr bool PM = NC == 64;
  static_assert(!PM || L == 4 || L == 16, "64-column engines: 4- and 16-position nets");
  auto samp_of = [](int n) { return PM ? (L == 4 ? (n & 15) : (n & 3)) : n / L; };
  auto pos_of = [](int n) { return PM ? (L == 4 ? (n >> 4) : (n >> 2)) : n % L; };
  auto col_of = [](int sm, int l) { return PM ? (L == 4 ? 16 * l + sm : 4 * l + sm) : sm * L + l; };
  Ctx c{a.weights, lds, (int)threadIdx.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), (int)threadIdx.x & 63,
        a.skip, GG::kNT};
  if constexpr (PM && L == 16) c.park = a.park + (size_t)blockIdx.x * (kParkBytes / 4);
  const int E = d.emb_dim, R = d.cond_rows;
  float *lat = lds + GG::kMiscLat, *epsr = lds + GG::kMiscEps, *G = lds + GG::kMiscG;
  float *X = lds + GG::kBufX;
  const bool has_in = d.latent_dim > 0, has_head = d.n_head > 0;
  int CF = d.dims[1];  // width of the last level (constant indices: see build_tape)
#pragma unroll
  for (int lv = 2; lv <= GLDM_R1D_MAX_LEVELS; ++lv) CF = lv == d.n_levels ? d.dims[lv] : CF;

  for (int i = c.tid; i < GG::kLdsFloats; i += GG::kThreads) lds[i] = 0.f;  // dead columns must stay finite
  __syncthreads();
  // the wave-local narrow levels are in use when the step program (built by the launcher) starts with their op
  const bool quad16 = PM && L == 16 && a.pm_nops > 0 && a.pm_tape[0] == OP_QUAD;
  if constexpr (PM && L == 4) {
    static_assert(2 * kQNEnd <= GG::kLdsFloats - GG::kMiscQTab, "kMiscQTab size");
    if (quad_levels(d)) quad_build_table(d, reinterpret_cast<int *>(lds + GG::kMiscQTab), c.tid, GG::kThreads);
  }
  if constexpr (PM && L == 16) {
    if (quad16) quad16_build_table<1>(d, reinterpret_cast<int *>(lds + GG::kMiscQTab), c.tid, GG::kThreads);
  }
  int *tape = reinterpret_cast<int *>(lds + GG::kMiscTape);
  ChainHdr *hdr = reinterpret_cast<ChainHdr *>(a.ws);
  unsigned long long *state = reinterpret_cast<unsigned long long *>(a.ws) + kChainHdrBytes / 8;
  const bool chained = a.left_tiles > 0 && a.chain > 1;
  if (c.tid == 0) {
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_LDS_TAPE)
    tape[1023] = build_tape<NC>(d, tape);
#else
    tape[1023] = PM ? a.pm_nops : build_tape<NC>(d, tape);
#endif
    // Slot = order of arrival, not blockIdx: a slot only ever waits for the slot before it, which has
    // then already started, so the hand-offs cannot deadlock whatever the dispatch order or residency.
    tape[1022] = chained ? (int)__hip_atomic_fetch_add(&hdr->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                         : (int)blockIdx.x;
    tape[1021] = chained ? (int)hdr->epoch : 0;  // written by the previous launch on this workspace
  }
  __syncthreads();
  const int n_ops = __builtin_amdgcn_readfirstlane(tape[1023]);
  // the kernel's one argument (RunArgs, by value) sits at offset 0 of the kernarg segment
  kernarg_int *ktape = (kernarg_int *)((__attribute__((address_space(4))) const char *)__builtin_amdgcn_kernarg_segment_ptr() +
                                       offsetof(RunArgs, pm_tape));
  const int slot = __builtin_amdgcn_readfirstlane(tape[1022]);
  const unsigned epoch = (unsigned)__builtin_amdgcn_readfirstlane(tape[1021]);
#ifdef GLDM_DEBUG_KNOBS
  if (a.stagger_ticks > 0 && ((blockIdx.x / a.n_cus) & 1)) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < a.stagger_ticks) __builtin_amdgcn_s_sleep(32);
  }
#endif
  // ---- this slot's program: its own tiles for all steps, with (at most) one step segment of a left-over tile
  // spliced in at the step at which the previous slot of the chain delivers it.  Built once, by one thread,
  // into LDS (like the op tape): the step loop keeps no scheduling state in registers.
  int *segs = reinterpret_cast<int *>(lds + GG::kMiscSegs);
  if (c.tid == 0) {
    const int N = a.n_steps;
    const int cj = slot / a.chain, ci = slot - cj * a.chain;
    const bool has_left = a.left_tiles > 0 && cj < a.left_tiles && ci * a.seglen < N;
    const int cut = has_left ? ci * a.seglen : 0;
    int n = 0;
    auto put = [&](int tile, int s0, int s1) {
      segs[4 * n] = tile; segs[4 * n + 1] = s0; segs[4 * n + 2] = s1;
      ++n;
    };
    if (cut > 0) put(slot, 0, cut);  // own tile 0 runs in two parts around the spliced segment
    if (has_left) put(a.rounds * a.slots + cj, cut, min(N, cut + a.seglen));
    put(slot, cut, N);
    for (int r = 1; r < a.rounds; ++r) put(r * a.slots + slot, 0, N);
    segs[4 * kMaxSegs - 1] = n;
  }
  __syncthreads();
  const int nseg = __builtin_amdgcn_readfirstlane(segs[4 * kMaxSegs - 1]);
  for (int sg = 0; sg < nseg; ++sg) {
  const int tile = __builtin_amdgcn_readfirstlane(segs[4 * sg]);
  const int s0 = __builtin_amdgcn_readfirstlane(segs[4 * sg + 1]), s1 = __builtin_amdgcn_readfirstlane(segs[4 * sg + 2]);
  const int N = a.n_steps;
  const int samp0 = tile * S;
  const int nsamp = min(S, a.n_samples - samp0);  // samples this tile holds (the batch's last tile may be short)
  c.nta = (nsamp * L <= 16) ? 1 : GG::kNT;
  if (L == 16 && a.ss_tab) {
    if constexpr (PM) {   // this lane's sample (lane & 3) -> its cloud's rows
      const int gi = min(samp0 + min(c.lane & 3, nsamp - 1), a.n_samples - 1);
      c.ss_lane = a.ss_tab + (size_t)(gi / a.samples_per_cond) * a.ss_stride;
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int gi = min(samp0 + min(q, nsamp - 1), a.n_samples - 1);
        c.ss_row[q] = a.ss_tab + (size_t)(gi / a.samples_per_cond) * a.ss_stride;
      }
    }
  }
  // ---- latent row for this tile: from the input (first step) or from the slot that ran the steps before s0
  int tid_s = c.tid;   // opaque (see tid_o below): the segment prologue's pointers are rebuilt per segment, not kept from kernel start
  asm volatile("" : "+v"(tid_s));
  if (tid_s < NC) {
    const int s = samp_of(tid_s), l = pos_of(tid_s);
    const int gi = min(samp0 + min(s, nsamp - 1), a.n_samples - 1);
    float v;
    if (s0 > 0) {
      v = chain_take(state + (size_t)tile * NC + tid_s, chain_tag(epoch, s0), &hdr->error);
    } else if (has_in) {
      const float *wi = a.weights + d.in_w + l * d.latent_dim;
      v = a.weights[d.in_b + l];
      for (int q = 0; q < d.latent_dim; ++q) v += wi[q] * a.x_in[(size_t)gi * d.latent_dim + q];
    } else {
      v = a.x_in[(size_t)gi * L + l];
    }
    lat[tid_s] = v;
  }
  __syncthreads();

  // The conditioning part of the embedding sum is the same at every step: thread i < S E keeps its (sample, e) entry's
  // cond rows in registers for the whole segment (validate(): S E <= 320 <= threads of the 64-column engine; the
  // 32-column engines take the loop below) and requests the NEXT step's time-embedding value a step ahead, so that the
  // step prologue is three SiLUs and an LDS store instead of a chain of L2 round trips.
  constexpr int kMaxR = 4;
  // 64-column engines (the step program travels in the kernel arguments: the LDS tape region holds three scalars at its
  // end): the cond rows wait there, [r][thread], instead of in registers -- four values alive across the whole op tape were
  // spilled to scratch and reloaded every step.  (More rows than fit there: the general loop below.)
#if defined(GLDM_DEBUG_KNOBS) && defined(GLDM_EXP_LDS_TAPE)
  constexpr bool kCeLds = false;   // (that experiment reads the step program from the region)
#else
  constexpr bool kCeLds = PM;
#endif
  const bool g_fast = S * E <= GG::kThreads && R <= kMaxR && !a.sample_t && (!kCeLds || R * S * E <= 1020);
  lds_f *ce_l = (lds_f *)(lds + GG::kMiscTape);
  float ce_reg[kCeLds ? 1 : kMaxR] = {}, se_reg = 0.f, te_next = 0.f;
  if (g_fast && tid_s < S * E) {
    const int s = tid_s / E, e = tid_s - s * E;
    const int gi = min(samp0 + min(s, nsamp - 1), a.n_samples - 1);
    const float *ce = a.cemb + ((size_t)(gi / a.samples_per_cond) * R) * E + e;
    if constexpr (kCeLds) {
#pragma unroll
      for (int r = 0; r < kMaxR; ++r)
        if (r < R) ce_l[r * S * E + tid_s] = ce[r * E];
    } else {
#pragma unroll
      for (int r = 0; r < kMaxR; ++r) ce_reg[r] = ce[(r < R ? r : 0) * E];
    }
    if (a.semb) se_reg = a.semb[(size_t)gi * E + e];  // latent_emb += cls_emb (class_conditioned_resnet.py:99-101)
    if (a.temb) te_next = a.temb[(size_t)a.timesteps[s0] * E + e];
  }
  for (int step = s0; step < s1; ++step) {
    if (GLDM_STAMPS(a.stamps) && blockIdx.x == 0 && c.tid == 0) a.stamps[kMaxOps + 1] = (long long)__builtin_readcyclecounter();
    // The thread index as this step's short phases see it: opaque, so that the index maps and LDS addresses derived from
    // it are recomputed here (a handful of integer instructions) instead of being hoisted out of the step loop, kept
    // across the whole op tape and spilled (14 scratch reloads per step, each a round trip in front of its use).
    int tid_o = c.tid;
    asm volatile("" : "+v"(tid_o));
    // ---- G[s][e] = sum_r silu(temb[t][e] + cemb[cond][r][e])
    if (g_fast) {
      if (tid_o < S * E) {
        const float te = te_next + se_reg;
        if (a.temb) te_next = a.temb[(size_t)a.timesteps[step + 1 < s1 ? step + 1 : step] * E + (tid_o % E)];
        float g = 0.f;
        if constexpr (kCeLds) {   // (a thread reads back what it wrote itself: no barrier)
#pragma unroll
          for (int r = 0; r < kMaxR; ++r) g += r < R ? silu(te + ce_l[(r < R ? r : 0) * S * E + tid_o]) : 0.f;
        } else {
#pragma unroll
          for (int r = 0; r < kMaxR; ++r) g += r < R ? silu(te + ce_reg[r]) : 0.f;
        }
        G[tid_o] = g;
      }
    } else if (!GLDM_SKIP(c, 32))
    for (int i = tid_o; i < S * E; i += GG::kThreads) {
      const int s = i / E, e = i - s * E;
      const int gi = min(samp0 + min(s, nsamp - 1), a.n_samples - 1);
      const float *ce = a.cemb + ((size_t)(gi / a.samples_per_cond) * R) * E + e;
      float te = 0.f;
      if (a.temb) {
        const int t = a.sample_t ? a.sample_t[gi] : a.timesteps[step];
        te = a.temb[(size_t)t * E + e];
      }
      if (a.semb) te += a.semb[(size_t)gi * E + e];  // latent_emb += cls_emb (class_conditioned_resnet.py:99-101)
      float g = 0.f;
      for (int r = 0; r < R; ++r) g += silu(te + ce[r * E]);
      G[s * E + e] = g;
    }
    if constexpr (PM) {   // quad engine hand-shake words (quad_narrow.h): every step starts from zero
      if ((L == 4 || quad16) && tid_o < 16 + 4 * 64) reinterpret_cast<int *>(lds + GG::kMiscQ)[tid_o] = 0;
    }
    // ---- init conv (k = 7, one input channel); the barrier below also publishes G
    const int C0 = d.dims[0];
    // DPM++ feeds the network c_in(sigma) * x (elucidated_diffusion.py:127-128)
    const float in_scale = a.sched_kind == GLDM_SCHED_DPMPP ? a.sched_coef[(size_t)step * GLDM_SCHED_COEF_STRIDE] : 1.0f;
    const bool scale_in = a.sched_kind == GLDM_SCHED_DPMPP;
    if (!GLDM_SKIP(c, 64))
    for (int i = tid_o; i < C0 * NC; i += GG::kThreads) {
      const int ch = i / NC, n = i - ch * NC;
      const int l = pos_of(n), sm = samp_of(n);
      float acc = a.weights[d.init_b + ch];
      const float *wk = a.weights + d.init_w + ch * 7;
      // the seven taps are requested together, in range or not: behind the range test each was a round trip of its own
      float wq[7];
#pragma unroll
      for (int q = 0; q < 7; ++q) wq[q] = wk[q];
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const int p = l + q - 3;
        const bool in = p >= 0 && p < L;
        float xv = lat[col_of(sm, in ? p : l)];
        if (scale_in) xv = in_scale * xv;
        acc = in ? acc + wq[q] * xv : acc;
      }
      X[PM ? pswz(ch, n) : swz<NC>(ch, n)] = acc;
    }
    __syncthreads();
    if constexpr (PM && L == 16) if (!quad16) {   // the first ResnetBlock reads the planes of the init conv's 16 rows (the
                                                  // wave-local chain reads the f32 rows and restores the zero entries itself)
      zero_plane_pads16(lds, c.tid);   // the previous step's (or tile's) 256-channel output rows lie over some of them
      {   // ... and over channels 16 .. 31 of H-plane block 0, which the 16-channel level multiplies with zero weights
        lds_u4 *hb = (lds_u4 *)(lds + PG<16>::kH);
        const u32x4 z4 = u32x4{0u, 0u, 0u, 0u};
        if (c.tid < 3 * 2 * 64) {
          const int plane = c.tid / 128, gg = 2 + ((c.tid >> 6) & 1), col = c.tid & 63;
          hb[(plane * 4 + gg) * PG<16>::kCols + PG<16>::kOff + col] = z4;
        }
      }
      if (c.tid < 256) {
        const int rg = c.tid >> 6, n = c.tid & 63;
        const lds_f *x3 = (const lds_f *)X;
        store_planes4<16>(lds + PG<16>::kX, 4 * rg, n, x3[pswz(4 * rg, n)], x3[pswz(4 * rg + 1, n)], x3[pswz(4 * rg + 2, n)],
                          x3[pswz(4 * rg + 3, n)]);
      }
      __syncthreads();
    }

    run_tape<NC, L>(c, d, tape, ktape, n_ops, E, blockIdx.x == 0 ? GLDM_STAMPS(a.stamps) : nullptr);
    if (GLDM_STAMPS(a.stamps) && blockIdx.x == 0 && c.tid == 0) a.stamps[n_ops] = (long long)__builtin_readcyclecounter();

    // ---- final 1x1 conv to one channel: eps[n] = b + sum_c w[c] X[c][n]
    if (!GLDM_SKIP(c, 128)) {
      // this step's scheduler coefficients, requested now (two 16-byte loads, in flight under the reduction): read one
      // by one where the update uses them they were six dependent L2 round trips per step
      f32x4 cf_lo = f32x4{0.f, 1.f, 0.f, 0.f}, cf_hi = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a.sched_kind != GLDM_SCHED_NONE) {
        const f32x4 *cfp = reinterpret_cast<const f32x4 *>(a.sched_coef + (size_t)step * GLDM_SCHED_COEF_STRIDE);
        cf_lo = cfp[0];
        cf_hi = cfp[1];
      }
      const float final_b = a.weights[d.final_b];
      float *red1 = lds + GG::kMiscRed1;
      int tid_f = c.tid;
      asm volatile("" : "+v"(tid_f));
      const int lane_f = tid_f & 63;
      const int n = lane_f & (NC - 1), slot = c.wave * GG::kRP + lane_f / NC;
      float part = 0.f;
      for (int row = slot; row < CF; row += GG::kSlots)
        part += a.weights[d.final_w + row] * X[PM ? pswz(row, n) : swz<NC>(row, n)];
      if (GG::kRP == 2) part = half_sum(part);
      red1[c.wave * NC + n] = part;
      __syncthreads();
      if (tid_f < NC) {
        float e = final_b;
#pragma unroll
        for (int q = 0; q < GG::kWaves; ++q) e += red1[q * NC + tid_f];
        epsr[tid_f] = e;
        if (a.sched_kind != GLDM_SCHED_NONE) {
          const int s = samp_of(tid_f), l = pos_of(tid_f);
          const int gi = min(samp0 + min(s, nsamp - 1), a.n_samples - 1);
          const float cf[8] = {cf_lo[0], cf_lo[1], cf_lo[2], cf_lo[3], cf_hi[0], cf_hi[1], cf_hi[2], cf_hi[3]};
          float nz = 0.f;
          if (a.sched_kind == GLDM_SCHED_DDPM && cf[7] != 0.f) {
            if (a.step_noise) {
              nz = a.step_noise[((size_t)step * a.n_samples + gi) * L + l];
            } else if (a.noise_on) {
              const unsigned long long g = (unsigned long long)(a.noise_base + gi);
              float z4[4];
              philox_normal4(a.noise_seed, (unsigned)g, (unsigned)(g >> 32), (unsigned)(l >> 2), (unsigned)step, z4);
              nz = (l & 3) == 0 ? z4[0] : ((l & 3) == 1 ? z4[1] : ((l & 3) == 2 ? z4[2] : z4[3]));
            }
          }
          if (a.sched_kind == GLDM_SCHED_DPMPP) lat[tid_f] = dpmpp_update(a.clip_sample, cf, lat[tid_f], e, lds + GG::kMiscOld + tid_f);
          else lat[tid_f] = scheduler_update(a.sched_kind, a.clip_sample, cf, lat[tid_f], e, nz);
        }
      }
      __syncthreads();
    }
  }

  // ---- outputs of the segment: the result after the last step, else the latent for the next slot of the chain
  int tid_e = c.tid;   // opaque like tid_o: nothing derived from it lives across the steps
  asm volatile("" : "+v"(tid_e));
  if (s1 < N) {
    if (tid_e < NC) chain_give(state + (size_t)tile * NC + tid_e, lat[tid_e], chain_tag(epoch, s1));
  } else if (!has_head) {
    if (tid_e < NC) {
      const int s = samp_of(tid_e), l = pos_of(tid_e);
      const int gi = samp0 + s;
      if (s < nsamp && gi < a.n_samples) a.out0[(size_t)gi * L + l] = a.sched_kind == GLDM_SCHED_NONE ? epsr[tid_e] : lat[tid_e];
    }
  } else if (L == 16 && d.head_kind == GLDM_HEAD_ENCODER) {   // (16-position nets only: gldm_encode checks)
    // out_layer folded into the bottleneck (r1d_pack): thread (sample, j) takes rows j (mu) and Lz + j (logvar) of the
    // [2 Lz][L] head and, when asked, mixes the latent from them (grasp_vae.py:552-561; add_noise of mu)
    int nl = d.n_head >> 1;
    asm volatile("" : "+s"(nl));   // opaque, like nh below
    if (tid_e < S * nl) {
      const int s = tid_e / nl, j = tid_e - s * nl;
      const int gi = samp0 + s;
      if (s < nsamp && gi < a.n_samples) {
        const float *wm = a.weights + d.head_w + j * L, *wv = wm + nl * L;
        float mu = a.weights[d.head_b + j], lv = a.weights[d.head_b + nl + j];
        for (int l = 0; l < L; ++l) {
          const float e = epsr[col_of(s, l)];
          mu += wm[l] * e;
          lv += wv[l] * e;
        }
        const size_t o = (size_t)gi * nl + j;
        a.out0[o] = mu;
        a.out1[o] = lv;
        if (a.out2) {
          float z = a.mix_mu * mu;
          if (a.eps) z += a.mix_eps * a.eps[o] * (a.eps_times_std ? expf(0.5f * lv) : 1.0f);
          a.out2[o] = z;
        }
      }
    }
  } else {
    // heads: rows 0..5 tmrp, row 6 class logit; input = the L-vector of each sample
    int nh = d.n_head;
    asm volatile("" : "+s"(nh));   // opaque here: the reciprocal of the division below was computed at kernel entry and spilled
    if (tid_e < S * nh) {
      const int s = tid_e / nh, r = tid_e - s * nh;
      const int gi = samp0 + s;
      if (s < nsamp && gi < a.n_samples) {
        const float *wr = a.weights + d.head_w + r * L;
        float acc = a.weights[d.head_b + r];
        for (int l = 0; l < L; ++l) acc += wr[l] * epsr[col_of(s, l)];
        if (r < 6) a.out0[(size_t)gi * 6 + r] = acc;
        else a.out1[gi] = acc;
      }
    }
  }
  __syncthreads();  // lat / epsr are rewritten by the next segment
  }  // segments
  if (chained && c.tid == 0) {  // the last workgroup to finish re-arms the header for the next launch
    const unsigned done = __hip_atomic_fetch_add(&hdr->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (done == gridDim.x - 1) {
      __hip_atomic_store(&hdr->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&hdr->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&hdr->epoch, (epoch + 1u) & 0xFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void cond_embed_kernel(const float *__restrict__ z, const float *__restrict__ w,
                                  const float *__restrict__ b, int rows_total, int dc, int e, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows_total * e) return;
  const int row = i / e, col = i - row * e;
  const float *zr = z + (size_t)row * dc, *wr = w + (size_t)col * dc;
  float acc = b[col];
  for (int q = 0; q < dc; ++q) acc += wr[q] * zr[q];
  out[i] = acc / (1.0f + expf(-acc));
}

#pragma clang fp contract(off)
__global__ void pose_epilogue_kernel(const float *__restrict__ tmrp, const float *__restrict__ logit,
                                     const float *__restrict__ mean, const float *__restrict__ stdv, int n, int gpc,
                                     float *__restrict__ H, float *__restrict__ un, float *__restrict__ conf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cl = i / gpc;
  float v[6];
  for (int q = 0; q < 6; ++q) {
    v[q] = tmrp[(size_t)i * 6 + q] * stdv[cl * 6 + q] + mean[cl * 6 + q];
    un[(size_t)i * 6 + q] = v[q];
  }
  // rotations.py:218-252 (mrp -> quat) and :171-215 (quat -> rotmat, SciPy convention)
  const float magsq = v[3] * v[3] + v[4] * v[4] + v[5] * v[5];
  const float den = 1.0f + magsq;
  const float x = (2.0f * v[3]) / den, y = (2.0f * v[4]) / den, z = (2.0f * v[5]) / den;
  const float w = (1.0f - magsq) / den;
  const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const float xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  float *h = H + (size_t)i * 16;
  h[0] = x2 - y2 - z2 + w2;  h[1] = 2.0f * (xy - zw);     h[2] = 2.0f * (xz + yw);      h[3] = v[0];
  h[4] = 2.0f * (xy + zw);   h[5] = -x2 + y2 - z2 + w2;   h[6] = 2.0f * (yz - xw);      h[7] = v[1];
  h[8] = 2.0f * (xz - yw);   h[9] = 2.0f * (yz + xw);     h[10] = -x2 - y2 + z2 + w2;   h[11] = v[2];
  h[12] = 0.f; h[13] = 0.f; h[14] = 0.f; h[15] = 1.0f;
  if (conf) conf[i] = 1.0f / (1.0f + expf(-logit[i]));
}

// The way back (rotations.py:305-309,115-163): arg-max over (R00, R11, R22, trace) with the first maximum winning (torch
// argmax), the SciPy branch formulas, normalise, q.xyz / (1 + q.w), then the dataset's (x - mean) / std.  Same operation
// order as the reference on the same f32 values (no contraction), so the branch is the reference's.
__global__ void pose_prologue_kernel(const float *__restrict__ H, const float *__restrict__ label,
                                     const float *__restrict__ mean, const float *__restrict__ stdv, int n, int gpc,
                                     float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cl = i / gpc;
  const float *h = H + (size_t)i * 16;
  float m[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[r][c] = h[4 * r + c];
  const float dg[4] = {m[0][0], m[1][1], m[2][2], (m[0][0] + m[1][1]) + m[2][2]};
  int ch = 0;
  for (int q = 1; q < 4; ++q) ch = dg[q] > dg[ch] ? q : ch;
  float q4[4];
  if (ch == 3) {
    q4[0] = m[2][1] - m[1][2];
    q4[1] = m[0][2] - m[2][0];
    q4[2] = m[1][0] - m[0][1];
    q4[3] = 1.0f + dg[3];
  } else {
    // constant indices only (a runtime-indexed register array would go to scratch)
    const float mii = ch == 0 ? m[0][0] : (ch == 1 ? m[1][1] : m[2][2]);
    const float mji = ch == 0 ? m[1][0] : (ch == 1 ? m[2][1] : m[0][2]), mij = ch == 0 ? m[0][1] : (ch == 1 ? m[1][2] : m[2][0]);
    const float mki = ch == 0 ? m[2][0] : (ch == 1 ? m[0][1] : m[1][2]), mik = ch == 0 ? m[0][2] : (ch == 1 ? m[1][0] : m[2][1]);
    const float mkj = ch == 0 ? m[2][1] : (ch == 1 ? m[0][2] : m[1][0]), mjk = ch == 0 ? m[1][2] : (ch == 1 ? m[2][0] : m[0][1]);
    const float qi = (1.0f - dg[3]) + 2.0f * mii, qj = mji + mij, qk = mki + mik;
    q4[0] = ch == 0 ? qi : (ch == 1 ? qk : qj);
    q4[1] = ch == 0 ? qj : (ch == 1 ? qi : qk);
    q4[2] = ch == 0 ? qk : (ch == 1 ? qj : qi);
    q4[3] = mkj - mjk;
  }
  const float nrm = sqrtf(((q4[0] * q4[0] + q4[1] * q4[1]) + q4[2] * q4[2]) + q4[3] * q4[3]);
  const float den = 1.0f + q4[3] / nrm;
  const float v[6] = {h[3], h[7], h[11], (q4[0] / nrm) / den, (q4[1] / nrm) / den, (q4[2] / nrm) / den};
  const int w = label ? 7 : 6;
  for (int q = 0; q < 6; ++q) out[(size_t)i * w + q] = (v[q] - mean[cl * 6 + q]) / stdv[cl * 6 + q];
  if (label) out[(size_t)i * 7 + 6] = label[i];
}
#pragma clang fp contract(fast)

// Scale / shift rows of every ResnetBlock for one conditioning cloud (ResnetBlock.mlp, resnets.py:125-151, when the
// embedding has no time part: the pose decoder):  ss[rb][row] = comb_b[row] + sum_e W[row][e] G[e],  G = sum over the
// cond rows of SiLU(cemb) -- the value the conv epilogue would compute with MFMAs for every sample and column.
// Table layout per cloud: blocks in tape order, [scale rows (C) | shift rows (C)] each (build_tape's tab_off).
__global__ __launch_bounds__(256) void ss_table_kernel(const gldm_r1d_desc d, const float *__restrict__ w,
                                                       const float *__restrict__ cemb, int stride,
                                                       float *__restrict__ tab) {
  __shared__ float G[256];
  const int cond = blockIdx.x, E = d.emb_dim, R = d.cond_rows, ekb = E >> 4;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    float g = 0.f;
    for (int r = 0; r < R; ++r) g += silu(cemb[((size_t)cond * R + r) * E + e]);
    G[e] = g;
  }
  __syncthreads();
  float *out = tab + (size_t)cond * stride;
  int off = 0;
  const int n_rb = 2 * d.n_levels + 1;
  for (int i = 0; i < n_rb; ++i) {
    const int C = d.dims[i < 2 * d.n_levels ? i / 2 : d.n_levels];
    const gldm_r1d_resblock &rb = d.rb[i];
    for (int row = threadIdx.x; row < 2 * C; row += blockDim.x) {
      // packed A fragments of the [2C x E] Linear: W[row][e] at ((mt * ekb + kb) * 64 + 16 kq + i) * 4 + j,
      // row = 16 mt + i, e = 16 kb + 4 j + kq
      const float *wr = w + rb.ss_w + (size_t)(row >> 4) * ekb * 256 + (row & 15) * 4;
      float acc = w[rb.ss_b + row];
      for (int kb = 0; kb < ekb; ++kb)
        for (int j = 0; j < 4; ++j)
          for (int kq = 0; kq < 4; ++kq) acc = fmaf(wr[kb * 256 + kq * 64 + j], G[16 * kb + 4 * j + kq], acc);
      out[off + row] = acc;
    }
    off += 2 * C;
  }
}

}  // namespace

// The generator on its own (n latents x L positions of one step), for the statistical tests: out [n][L]
__global__ void philox_normal_kernel(unsigned long long seed, long long base, int step, int n, int L, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * L) return;
  const int gi = i / L, l = i - gi * L;
  const unsigned long long g = (unsigned long long)(base + gi);
  float z4[4];
  philox_normal4(seed, (unsigned)g, (unsigned)(g >> 32), (unsigned)(l >> 2), (unsigned)step, z4);
  out[i] = z4[l & 3];
}

namespace {

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

constexpr int kEngineNC = 32;  // denoiser / decoder geometry: 32 columns, two workgroups per CU
int engine_nc() { return kEngineNC; }

int validate(const gldm_r1d_desc *d) {
  if (!d) return GLDM_ERR_INVALID_ARG;
  if (d->seq_len != 4 && d->seq_len != 16) return GLDM_ERR_UNSUPPORTED;
  if (d->n_levels < 1 || d->n_levels > GLDM_R1D_MAX_LEVELS || 12 * d->n_levels + 2 > kMaxOps) return GLDM_ERR_UNSUPPORTED;
  const int nc = engine_nc(), waves = 4;
  const int S = nc / d->seq_len;
  if (d->emb_dim <= 0 || (d->emb_dim & 15) || S * d->emb_dim > 320) return GLDM_ERR_UNSUPPORTED;
  if (d->groups != 4 || waves != 4) return GLDM_ERR_UNSUPPORTED;  // GroupNorm lives in the conv epilogue
  for (int i = 0; i <= d->n_levels; ++i) {
    const int C = d->dims[i];
    if (C > kMaxC || C < 4 || !pow2(C) || !gn_fusable(C, d->groups)) return GLDM_ERR_UNSUPPORTED;
    if (i < d->n_levels && C > 128) return GLDM_ERR_UNSUPPORTED;  // attention levels keep 4 regions in LDS
  }
  return GLDM_OK;
}

// Rows of the per-cloud scale/shift table (ss_table_kernel) when the engine uses one: the 16-position pose decoder
// (no time embedding, wide embedding: E >= 32).  0 = no table.
int ss_table_rows(const gldm_r1d_desc *d) {
  if (d->seq_len != 16 || d->latent_dim <= 0 || d->emb_dim < 32 || d->emb_dim > 256 || d->dims[0] < 16) return 0;
  int rows = 0;
  for (int i = 0; i < 2 * d->n_levels + 1; ++i) rows += 2 * d->dims[i < 2 * d->n_levels ? i / 2 : d->n_levels];
  return rows;
}

// The position-major 64-column engine (r1d_kernel<64, 4>) serves the latent denoiser of the shipped
// configurations: 4 positions, no input layer / heads, emb_dim 16, a 4-channel first level and 32..256-channel
// ones after it.  Anything else runs on the sample-major 32-column engine.
bool pm_supported(const gldm_r1d_desc *d) {
  if (d->seq_len != 4 || d->latent_dim != 0 || d->n_head != 0 || d->emb_dim != 16 || d->groups != 4) return false;
  if (d->dims[0] != 4) return false;
  for (int i = 0; i < d->n_levels; ++i)  // to_qkv with the PreNorm gain folded in (ABI 4 packers provide it)
    if (d->lv[i].qkvn_w <= 0 || d->lv[i].qkvn_s <= 0) return false;
  for (int i = 1; i < d->n_levels; ++i)  // split-f16 conv weights (ABI 5 packers provide them)
    if (d->lv[i].down_w3 <= 0 || d->lv[i].qkvn_w3 <= 0 || d->lv[i].out_w3 <= 0 || d->rb[2 * i].c1_w3 <= 0 || d->rb[2 * i].c2_w3 <= 0 || d->rb[2 * i + 1].c1_w3 <= 0 ||
        d->rb[2 * i + 1].c2_w3 <= 0)
      return false;
  if (d->rb[2 * d->n_levels].c1_w3 <= 0 || d->rb[2 * d->n_levels].c2_w3 <= 0 || d->lv[0].out_w3 <= 0) return false;
  for (int i = 1; i <= d->n_levels; ++i) {
    const int C = d->dims[i];
    if (!(C == 32 || C == 64 || C == 128 || C == 256)) return false;
    if (i < d->n_levels && C > 128) return false;
  }
  return true;
}

// The 16-position 64-column engine (r1d_kernel<64, 16>: tiles of 4 samples x 16 positions, column = 4 * position +
// sample, split-f16 GEMMs on pre-split planes) serves the nets both shipped experiments run at 16 positions: the pose
// decoder (latent_dim > 0, heads) and the ppc experiment's latent denoiser.  emb_dim 64, a 16-channel first level
// and 32..256-channel ones after it, every split-f16 weight copy present (ABI 5 packers; 16-channel levels zero-padded
// to one 32-channel block: r1d_pack.pad_cin32).
bool pm16_supported(const gldm_r1d_desc *d) {
  if (d->seq_len != 16 || d->emb_dim != 64 || d->groups != 4 || d->dims[0] != 16 || d->cond_rows > 4) return false;
  for (int i = 0; i < d->n_levels; ++i)
    if (d->lv[i].qkvn_w3 <= 0 || d->lv[i].qkvn_s <= 0 || d->lv[i].out_w3 <= 0 || d->lv[i].down_w3 <= 0) return false;
  for (int i = 0; i <= 2 * d->n_levels; ++i)
    if (d->rb[i].c1_w3 <= 0 || d->rb[i].c2_w3 <= 0) return false;
  for (int i = 1; i <= d->n_levels; ++i) {
    const int C = d->dims[i];
    if (!(C == 32 || C == 64 || C == 128 || C == 256)) return false;
    if (i < d->n_levels && C > 128) return false;
  }
  return true;
}
bool wide_engine(const gldm_r1d_desc *d) { return pm_supported(d) || pm16_supported(d); }   // 64-column tiles

using gldm_dev::cu_count;

// Scratch behind the hand-off granules where the 16-position 64-column engine parks the residual stream of a 256-channel
// last level (PG<16>::kW): 64 KiB per workgroup of the launch (at most one per CU), 256-byte aligned.  *base is rounded up to the
// alignment; returns the bytes to add behind it (0: this descriptor never parks).
struct WsLayout { long long tiles, ss_off, park_off, total; int nc; };
long long park_bytes(const gldm_r1d_desc *d, long long tiles, long long *base);
// header | hand-off granules | (256-byte aligned) the decoder's scale/shift table | (256-byte aligned) park scratch
WsLayout ws_layout(const gldm_r1d_desc *d, int n_samples) {
  WsLayout w{};
  w.nc = wide_engine(d) ? 64 : engine_nc();
  const int S = w.nc / d->seq_len;
  w.tiles = (n_samples + S - 1) / S;
  long long bytes = kChainHdrBytes + w.tiles * w.nc * 8;
  w.ss_off = -1;
  if (ss_table_rows(d) > 0) {
    bytes = (bytes + 255) & ~255LL;
    w.ss_off = bytes;
    bytes += (long long)n_samples * ss_table_rows(d) * 4;
  }
  const long long pb = park_bytes(d, w.tiles, &bytes);
  w.park_off = pb > 0 ? bytes : -1;
  w.total = bytes + pb;
  return w;
}
long long park_bytes(const gldm_r1d_desc *d, long long tiles, long long *base) {
  if (pm_supported(d) || !pm16_supported(d) || d->dims[d->n_levels] != 256) return 0;   // the 4-position engine keeps it in LDS
  *base = (*base + 255) & ~255LL;
  const long long wgs = tiles < cu_count() ? tiles : cu_count();
  return wgs * kParkBytes;
}

// Work plan of one launch.  `slots` = workgroups resident at once (two 32-column tiles per CU).  A batch of
// up to `slots` tiles is one workgroup per tile.  A larger one runs `slots` persistent workgroups: each owns
// `rounds` whole tiles, and the `left` tiles beyond the whole rounds are NOT run as a last, partly empty
// round (5120 latents = 640 tiles on 512 slots would take two rounds for 1.25 rounds of work): each is cut
// along the step axis into `chain` segments that a group of `chain` consecutive slots runs in turn, so every
// slot ends up with (nearly) the same number of tile-steps.
struct Plan { int grid, slots, rounds, left, chain, seglen; };

Plan make_plan(int n_samples, int n_steps, int L, int nc, bool allow_chain = true) {
  int slots = cu_count() * (nc == 32 ? 2 : 1);
#ifdef GLDM_DEBUG_KNOBS
  // co-residence experiment: fewer persistent workgroups than CUs, so that another stream's kernels find free
  // CUs while the fused launch runs
  if (const char *e = getenv("GLDM_R1D_SLOTS")) slots = atoi(e) > 0 ? atoi(e) : slots;
#endif
  const int S = nc / L;
  const int tiles = (n_samples + S - 1) / S;
  Plan p{tiles, slots, 1, 0, 1, n_steps};
  if (tiles <= slots) return p;
  if (tiles / slots + 2 > kMaxSegs) { p.grid = -1; return p; }  // more tiles per workgroup than its list holds
  p.grid = slots;
  p.rounds = tiles / slots;
  p.left = tiles - p.rounds * slots;
  if (p.left > 0) {
    int g = slots / p.left;
    if (g > 8) g = 8;             // a hand-off is ~3 us; finer cuts buy nothing
    if (g > n_steps) g = n_steps;
    if (n_steps > 4095) g = 1;  // chain_tag() carries the step in 12 bits: longer loops run their left-over tiles whole
    if (!allow_chain) g = 1;  // DPM++ carries two rows of state per tile (x and the previous denoised): whole tiles only
    p.chain = g < 1 ? 1 : g;
    p.seglen = (n_steps + p.chain - 1) / p.chain;
  }
  return p;
}

template <int NC, int L>
int launch_one(const RunArgs &a, int tiles, hipStream_t s) {
  size_t lds_bytes = (size_t)Geo<NC>::kLdsFloats * sizeof(float);
#ifdef GLDM_DEBUG_KNOBS
  if (getenv("GLDM_R1D_ONE_WG") && lds_bytes < 100 * 1024) lds_bytes = 100 * 1024;  // one workgroup per CU: phases on their own
#endif
  gldm_dev::launch_dynamic_lds<r1d_kernel<NC, L>>(dim3(tiles), dim3(Geo<NC>::kThreads), (int)lds_bytes, lds_bytes, s, a);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

int launch_r1d(const RunArgs &a_in, hipStream_t s) {
  const bool pm4 = pm_supported(&a_in.d), pm16 = !pm4 && pm16_supported(&a_in.d), pm = pm4 || pm16;
  const int L = a_in.d.seq_len, nc = pm ? 64 : engine_nc();
  const Plan pl = make_plan(a_in.n_samples, a_in.n_steps, L, nc, a_in.sched_kind != GLDM_SCHED_DPMPP);
  const int tiles = pl.grid;
  if (tiles <= 0) return GLDM_ERR_UNSUPPORTED;  // > ~250 k samples in one launch: split the batch
  RunArgs a = a_in;
  a.slots = pl.slots; a.rounds = pl.rounds; a.left_tiles = pl.left; a.chain = pl.chain; a.seglen = pl.seglen;
  a.park = nullptr;
  a.pm_nops = 0;
  if (pm) {
    static_assert(8 * GLDM_R1D_MAX_LEVELS + 2 <= kPmMaxOps && sizeof(RunArgs) <= 4096, "64-column tape in the kernel arguments");
    bool use_quad = true;
#ifdef GLDM_DEBUG_KNOBS
    if (getenv("GLDM_R1D_NOQUAD")) use_quad = false;   // A/B: the narrow levels as position-major phases
#endif
    // 16-position nets: the wave-local levels take their scale / shift rows from the per-cloud table or a 64-wide embedding
    if (pm16 && !(a_in.ss_tab != nullptr || a_in.d.emb_dim == 64)) use_quad = false;
    a.pm_nops = build_tape<64>(a_in.d, a.pm_tape, use_quad);
    const WsLayout wl = ws_layout(&a_in.d, a_in.n_samples);
    if (wl.park_off >= 0) a.park = reinterpret_cast<float *>(reinterpret_cast<char *>(a_in.ws) + wl.park_off);
  }
  a.n_cus = cu_count();
#ifdef GLDM_DEBUG_KNOBS
  // diagnostic builds only (make EXTRA=-DGLDM_DEBUG_KNOBS): phase skipping, a start offset for the
  // second workgroup of a CU, and per-op cycle stamps.  The shipped library reads no environment.
  {
    const char *e = getenv("GLDM_R1D_SKIP");
    a.skip = e ? atoi(e) : 0;
    const char *g = getenv("GLDM_R1D_STAGGER_US");
    a.stagger_ticks = g ? atoi(g) * 100 : 0;
  }
  const bool stamp = getenv("GLDM_R1D_STAMP") != nullptr;  // blocks, copies and prints
#else
  const bool stamp = false;
#endif
  static long long *dstamps = nullptr;
  if (stamp && !dstamps) (void)hipMalloc(&dstamps, (kMaxOps + 2) * sizeof(long long));
  a.stamps = stamp ? dstamps : nullptr;
  const int rc = pm4 ? launch_one<64, 4>(a, tiles, s)
                     : (pm16 ? launch_one<64, 16>(a, tiles, s)
                             : (L == 4 ? launch_one<kEngineNC, 4>(a, tiles, s) : launch_one<kEngineNC, 16>(a, tiles, s)));
  if (stamp) {
    static long long host[kMaxOps + 2];
    static const char *names[] = {"", "CONV", "RES4", "LN", "ATT", "QKVLN", "OUTLN", "QKVAT", "QUAD"};
    const bool quad = (pm4 || pm16) && a.pm_nops > 0 && a.pm_tape[0] == OP_QUAD;
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(host, dstamps, sizeof(host), hipMemcpyDeviceToHost);
    // the tape is rebuilt on the host only to label the stamps
    int dims[GLDM_R1D_MAX_LEVELS + 1];
    for (int i = 0; i <= a.d.n_levels; ++i) dims[i] = a.d.dims[i];
    int op = 0;
    auto line = [&](int type, int C, int cout, int taps) {
      printf("op %3d %-5s C=%3d cout=%3d k=%d : %7lld clk\n", op, names[type], C, cout, taps, host[op + 1] - host[op]);
      ++op;
    };
    auto resblock = [&](int C) {
      if (C == 4 && a.d.seq_len == 4) line(2, C, C, 3);
      else { line(1, C, C, 3); line(1, C, C, 3); }
    };
    if (quad) line(8, dims[0], 128, 3);
    for (int lv = quad ? 3 : 0; lv < a.d.n_levels; ++lv) {
      const int C = dims[lv];
      resblock(C); resblock(C);
      if (pm) line(7, C, 384, 1);
      else { line(3, C, C, 0); line(1, C, 192, 1); line(4, C, 64, 0); line(1, C, 192, 1); line(4, C, 64, 0); }
      if (pm && (C == 4 || C == 16 || C == 32 || C == 64 || C == 128)) line(6, 128, C, 1);
      else { line(1, 128, C, 1); line(3, C, C, 0); }
      line(1, C, dims[lv + 1], 3);
    }
    resblock(dims[a.d.n_levels]);
    printf("step total (ops): %lld clk; step prologue (embedding sums, init conv): %lld clk\n", host[op] - host[0],
           host[0] - host[kMaxOps + 1]);
#ifdef GLDM_DEBUG_KNOBS
    if (quad) {
      static long long qs[4][16];
      (void)hipMemcpyFromSymbol(qs, HIP_SYMBOL(g_q_stamp), sizeof(qs));
      static const char *qn4[] = {"pads", "rb4", "rb4", "att4", "down4", "rb32", "rb32", "att32", "down32", "rb64", "rb64", "att64", "down64"};
      static const char *qn16[] = {"pads", "rb16", "rb16", "att16", "down16", "rb32", "rb32", "att32", "down32", "rb64", "rb64", "att64", "down64"};
      const char **qn = pm16 ? qn16 : qn4;
      for (int q = 0; q < 4; ++q) {
        printf("quad %d:", q);
        for (int i = 1; i <= 12; ++i) printf(" %s %lld", qn[i], qs[q][i] - qs[q][i - 1]);
        printf(" | total %lld, polls that waited %lld\n", qs[q][12] - qs[q][0], qs[q][13]);
      }
    }
#ifdef GLDM_WAVE_STAMPS
    if (pm) {   // per-wave view of the last 32 position-major convs of workgroup 0: k-loop / epilogue, relative to wave 0's entry
      static long long wv[8][32][8];
      int cnt[8];
      (void)hipMemcpyFromSymbol(wv, HIP_SYMBOL(g_wv_stamp), sizeof(wv));
      (void)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_wv_cnt), sizeof(cnt));
      for (int i = 0; i < 32; ++i) {
        const int e = (cnt[0] + i) & 31;
        printf("conv %3lld->%3lld:", wv[0][e][3] / 1000, wv[0][e][3] % 1000);
        for (int w = 0; w < 8; ++w)
          printf("  w%d in %+5lld loop %6lld epi %6lld (stats %5lld wait %5lld finish %5lld) |", w, wv[w][e][0] - wv[0][e][0],
                 wv[w][e][1] - wv[w][e][0], wv[w][e][2] - wv[w][e][1], wv[w][e][4] - wv[w][e][1], wv[w][e][5] - wv[w][e][4],
                 wv[w][e][2] - wv[w][e][5]);
        printf("\n");
      }
    }
#endif
#endif
  }
  return rc;
}

// gldm_decode / gldm_encode of a net with a per-cloud scale / shift table (ss_table_rows() > 0): ss_table_kernel fills it, behind
// the hand-off granules of the workspace (gldm_r1d_workspace_bytes), and the engine is pointed at it.  false: the launch failed.
bool launch_ss_table(RunArgs &a, hipStream_t s) {
  const int rows = ss_table_rows(&a.d);
  if (rows <= 0) return true;
  float *tab = reinterpret_cast<float *>(reinterpret_cast<char *>(a.ws) + ws_layout(&a.d, a.n_samples).ss_off);
  const int n_cond = (a.n_samples + a.samples_per_cond - 1) / a.samples_per_cond;
  hipLaunchKernelGGL(ss_table_kernel, dim3(n_cond), dim3(256), 0, s, a.d, a.weights, a.cemb, rows, tab);
  if (hipGetLastError() != hipSuccess) return false;
  a.ss_tab = tab;
  a.ss_stride = rows;
  return true;
}
}  // namespace

GLDM_API int gldm_r1d_cond_embed(const float *z_cond, const float *w, const float *b, int n_cond, int rows, int dc,
                                 int e, float *cemb, gldm_stream_t stream) {
  if (!z_cond || !w || !b || !cemb || n_cond <= 0 || rows <= 0 || dc <= 0 || e <= 0) return GLDM_ERR_INVALID_ARG;
  const int total = n_cond * rows * e;
  hipLaunchKernelGGL(cond_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     z_cond, w, b, n_cond * rows, dc, e, cemb);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API long long gldm_r1d_workspace_bytes(const gldm_r1d_desc *desc, int n_samples) {
  if (validate(desc) != GLDM_OK || n_samples <= 0) return -1;
  // header + one 8-byte hand-off granule per activation column of every tile (see ChainHdr) + table + park scratch
  return ws_layout(desc, n_samples).total;
}

GLDM_API int gldm_r1d_tile_columns(const gldm_r1d_desc *desc) {
  const int st = validate(desc);
  if (st != GLDM_OK) return st;
  return wide_engine(desc) ? 64 : engine_nc();
}

GLDM_API int gldm_denoise(const gldm_r1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                          int samples_per_cond, const float *x_in, int n_samples, const int32_t *timesteps,
                          const int32_t *sample_t, int n_steps, int sched_kind, int clip_sample,
                          const float *sched_coef, const float *step_noise, const float *sample_emb, float *x_out,
                          void *workspace, gldm_stream_t stream) {
  int st = validate(desc);
  if (st != GLDM_OK) return st;
  if (!weights || !cemb || !x_in || !x_out || !workspace || n_samples <= 0 || n_steps <= 0 || samples_per_cond <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (desc->latent_dim != 0) return GLDM_ERR_INVALID_ARG;
  if (temb && !timesteps && !sample_t) return GLDM_ERR_INVALID_ARG;
  if (sched_kind != GLDM_SCHED_NONE && (!sched_coef || ((unsigned long long)sched_coef & 15))) return GLDM_ERR_INVALID_ARG;  // rows are read as 16-byte loads
  if (sched_kind == GLDM_SCHED_NONE && n_steps != 1) return GLDM_ERR_INVALID_ARG;
  RunArgs a{};
  a.d = *desc;
  a.weights = weights; a.temb = temb; a.cemb = cemb; a.semb = sample_emb; a.samples_per_cond = samples_per_cond;
  a.x_in = x_in; a.n_samples = n_samples; a.timesteps = timesteps; a.sample_t = sample_t; a.n_steps = n_steps;
  a.sched_kind = sched_kind; a.clip_sample = clip_sample; a.sched_coef = sched_coef; a.step_noise = step_noise;
  a.out0 = x_out; a.out1 = nullptr; a.ws = reinterpret_cast<float *>(workspace);
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_denoise_rng(const gldm_r1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                              int samples_per_cond, const float *x_in, int n_samples, const int32_t *timesteps, int n_steps,
                              int clip_sample, const float *sched_coef, unsigned long long noise_seed,
                              long long noise_base, const float *sample_emb, float *x_out, void *workspace,
                              gldm_stream_t stream) {
  int st = validate(desc);
  if (st != GLDM_OK) return st;
  if (!weights || !cemb || !x_in || !x_out || !workspace || n_samples <= 0 || n_steps <= 0 || samples_per_cond <= 0 ||
      noise_base < 0)
    return GLDM_ERR_INVALID_ARG;
  if (desc->latent_dim != 0 || (temb && !timesteps)) return GLDM_ERR_INVALID_ARG;
  if (!sched_coef || ((unsigned long long)sched_coef & 15)) return GLDM_ERR_INVALID_ARG;
  RunArgs a{};
  a.d = *desc;
  a.weights = weights; a.temb = temb; a.cemb = cemb; a.semb = sample_emb; a.samples_per_cond = samples_per_cond;
  a.x_in = x_in; a.n_samples = n_samples; a.timesteps = timesteps; a.sample_t = nullptr; a.n_steps = n_steps;
  a.sched_kind = GLDM_SCHED_DDPM; a.clip_sample = clip_sample; a.sched_coef = sched_coef; a.step_noise = nullptr;
  a.noise_seed = noise_seed; a.noise_base = noise_base; a.noise_on = 1;
  a.out0 = x_out; a.out1 = nullptr; a.ws = reinterpret_cast<float *>(workspace);
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_step_noise_rng(unsigned long long noise_seed, long long noise_base, int step, int n_samples, int seq_len,
                                 float *out, gldm_stream_t stream) {
  if (!out || n_samples <= 0 || seq_len <= 0 || step < 0 || noise_base < 0) return GLDM_ERR_INVALID_ARG;
  const int total = n_samples * seq_len;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), noise_seed,
                     noise_base, step, n_samples, seq_len, out);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_decode(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond,
                         const float *z_h, int n_samples, float *tmrp, float *logit, void *workspace,
                         gldm_stream_t stream) {
  int st = validate(desc);
  if (st != GLDM_OK) return st;
  if (!weights || !cemb || !z_h || !tmrp || !logit || !workspace || n_samples <= 0 || samples_per_cond <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (desc->latent_dim <= 0 || desc->n_head != 7 || desc->head_kind != GLDM_HEAD_DECODER) return GLDM_ERR_INVALID_ARG;
  RunArgs a{};
  a.d = *desc;
  a.weights = weights; a.temb = nullptr; a.cemb = cemb; a.samples_per_cond = samples_per_cond;
  a.x_in = z_h; a.n_samples = n_samples; a.n_steps = 1; a.sched_kind = GLDM_SCHED_NONE;
  a.out0 = tmrp; a.out1 = logit; a.ws = reinterpret_cast<float *>(workspace);
  if (!launch_ss_table(a, reinterpret_cast<hipStream_t>(stream))) return GLDM_ERR_LAUNCH;
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_encode(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond,
                         const float *h, int n_samples, const float *eps, float mix_mu, float mix_eps, int eps_times_std,
                         float *mu, float *logvar, float *z, void *workspace, gldm_stream_t stream) {
  int st = validate(desc);
  if (st != GLDM_OK) return st;
  if (!weights || !cemb || !h || !mu || !logvar || !workspace || n_samples <= 0 || samples_per_cond <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (desc->latent_dim <= 0 || desc->head_kind != GLDM_HEAD_ENCODER || desc->n_head < 2 || (desc->n_head & 1) ||
      desc->n_head > 2 * GLDM_R1D_MAX_LATENT)
    return GLDM_ERR_INVALID_ARG;
  if (desc->seq_len != 16) return GLDM_ERR_UNSUPPORTED;   // the encoder head is compiled into the 16-position engines only
  RunArgs a{};
  a.d = *desc;
  a.weights = weights; a.temb = nullptr; a.cemb = cemb; a.samples_per_cond = samples_per_cond;
  a.x_in = h; a.n_samples = n_samples; a.n_steps = 1; a.sched_kind = GLDM_SCHED_NONE;
  a.out0 = mu; a.out1 = logvar; a.out2 = z; a.eps = eps; a.mix_mu = mix_mu; a.mix_eps = mix_eps;
  a.eps_times_std = eps_times_std; a.ws = reinterpret_cast<float *>(workspace);
  if (!launch_ss_table(a, reinterpret_cast<hipStream_t>(stream))) return GLDM_ERR_LAUNCH;
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_pose_prologue(const float *H, const float *label, const float *grasp_mean, const float *grasp_std, int n,
                                int grasps_per_cloud, int n_clouds, float *h, gldm_stream_t stream) {
  if (!H || !grasp_mean || !grasp_std || !h || n <= 0 || grasps_per_cloud <= 0 || n_clouds <= 0) return GLDM_ERR_INVALID_ARG;
  if ((long long)n_clouds * grasps_per_cloud < (long long)n) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pose_prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H,
                     label, grasp_mean, grasp_std, n, grasps_per_cloud, h);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_pose_epilogue(const float *tmrp, const float *logit, const float *grasp_mean,
                                const float *grasp_std, int n, int grasps_per_cloud, int n_clouds, float *H,
                                float *tmrp_unnorm, float *confidence, gldm_stream_t stream) {
  if (!tmrp || !grasp_mean || !grasp_std || !H || !tmrp_unnorm || n <= 0 || grasps_per_cloud <= 0 || n_clouds <= 0)
    return GLDM_ERR_INVALID_ARG;
  // every grasp's cloud row (i / grasps_per_cloud) must exist in mean/std [n_clouds, 6]
  if ((long long)n_clouds * grasps_per_cloud < (long long)n) return GLDM_ERR_INVALID_ARG;
  if (confidence && !logit) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pose_epilogue_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     tmrp, logit, grasp_mean, grasp_std, n, grasps_per_cloud, H, tmrp_unnorm, confidence);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
