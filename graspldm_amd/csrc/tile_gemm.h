// tile_gemm.h -- the tile GEMMs: a workgroup's activation tile in LDS times weights streamed L2 -> VGPR as whole fragments.
// The middle of three layers: on mfma_prims.h (the only header it may include), under r1d_gemm.h (the ResNet1D engine's own
// part).  Included by sa_mlp.hip, pointwise_mlp.hip and resnet1d.hip, and by the probes tools/micro/gemm_rate.hip and
// vmem_interference.hip.  Device code only, __forceinline__ in an anonymous namespace: nothing here is a symbol.
//   * Geo<NC> (a workgroup's NC activation columns as [channel][column] f32 rows in two buffers X and H, XOR-swizzled: swz),
//     PG<LL> (the same tensors as pre-split f16 planes in B-fragment order, store_planes4), Ctx (what a wave knows of its launch);
//   * f32 pipe (v_mfma_f32_16x16x4_f32): gemm_fast_pf / gemm_fast_tap3 / gemm_fast / gemm_small, store_tiles; gemm_passes
//     (bias, one k-sweep per pass, store) is one wave's share of a layer, GLDM_DEAL_1X1 deals a 1x1 layer's output tiles over
//     the waves, conv_gemm is a whole 1x1 layer;
//   * split-f16 pipe: gemm1_pl (1x1, B from planes).
// Nothing of one kernel family lives here: the engine's misc region, its scale / shift tables, the GroupNorm epilogue and
// the k = 3 convs with their dealing are r1d_gemm.h's, r1d_wide.h's and resnet1d.hip's.
#pragma once
#include "mfma_prims.h"

namespace {

constexpr int kMaxC = 256;

// Geometry of one workgroup and its two activation buffers (floats).  X: block input / residual stream, H: scratch.
// (The ResNet1D engine's map goes on behind them: R1dGeo, r1d_gemm.h.)
template <int NC>
struct Geo {
  static constexpr int kWaves = NC / 8;           // 8 waves at 64 columns, 4 at 32
  static constexpr int kThreads = kWaves * 64;
  static constexpr int kNT = NC / 16;             // 16-column n-tiles
  static constexpr int kRP = 64 / NC;             // rows a wave touches per pass: lane = (sub, column)
  static constexpr int kSlots = kWaves * kRP;     // row slots of the norm passes
  static constexpr int kBufX = 0;
  static constexpr int kBufH = kMaxC * NC;
};

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

// Pre-split activation planes of the 64-column engines.  A tensor that is only ever read as a GEMM B operand is kept
// in LDS already split into its two f16 planes, in B-fragment order:
//   [32-channel block kb][plane hi|lo][g = 0..3][column 0..63][8 f16 = channels 32 kb + 8 g + 0..7]
// (8 KiB per 32 channels).  The producer's epilogue splits each element ONCE (its accumulators hold 4 consecutive
// channels of a column: one ds_write_b64 per plane); the eight consumer waves read a whole fragment plane with one
// ds_read_b128 per lane and their k-loops are loads + MFMA only.
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
  // rows 128 .. 255 lie over the first blocks: the residual stream is parked in global scratch, R1dCtx::park)
  static constexpr int kW = LL == 16 ? kH : 256 * 64;
  static constexpr int kEnd = kW + 8 * kBlockFloats;
};
static_assert(PG<4>::kEnd <= 512 * 64, "position-major planes end in front of the attention exchange slots");
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

struct Ctx {
  const float *w;   // packed weights
  float *lds;
  int tid, wave, lane;
  int nta;         // live 16-column n-tiles of this workgroup (kNT = full tile, 1 = tail tile)
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

// One wave's share of a GEMM: PASSES x MT m-tiles by NT n-tiles, one k-sweep per pass.  Passes keep
// the register footprint of a sweep small (MT * TAPS <= 6 fragments per block) so that every variant
// fits beside the other phases of the kernel without spilling; the extra cost of a pass is one
// pipeline fill.  The bias is folded into the accumulator start value.
// (The engine's gemm3_gn, r1d_gemm.h, repeats the sweep in front of its GroupNorm epilogue: shared through a helper that
// takes the accumulators by reference, both came out as different machine code -- the start values as single moves.)
template <int NC, int L, int TAPS, int MT, int NT, int PASSES>
__device__ __forceinline__ void gemm_passes(const Ctx &c, const float *wp, int mt0, int nt0, bool active,
                                            const float *src, int cin, float *dst, int cout, const float *bias,
                                            bool alias, int act) {
  f32x4 acc[PASSES][MT][NT];
  const int kq = c.lane >> 4;
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
  if (alias) __syncthreads();
  if (active) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) store_tiles<NC, MT, NT>(c, acc[p], mt0 + p * MT, nt0, dst, cout, act);
  }
}

// A 1x1 layer's output tiles dealt over the waves (all n-tiles each, or the two halves of the tile at 64 columns), where
// G1(MT, NT, PASSES, mt0, nt0, active) is the user's gemm_passes call; w: the wave, nta: Ctx::nta.  Output widths are
// 16 x {1, 2, 4, 8, 12, 16} rows (the callers' validation enforces it).  A macro because its two users, conv_gemm below and
// the ResNet1D engine's conv_op (resnet1d.hip), must expand it in place: behind one more level of calls both kernels come out
// as different machine code.
#define GLDM_DEAL_1X1(NC, nta, mtiles, w, G1)                                                \
  if constexpr (NC == 64) { /* layout agnostic: 8 waves x 4 n-tiles */                       \
    if (mtiles == 16) G1(2, 4, 1, 2 * w, 0, true);                                           \
    else if (mtiles == 12) G1(3, 2, 1, 3 * (w & 3), 2 * (w >> 2), true);                     \
    else if (mtiles == 8) G1(1, 4, 1, w, 0, true);                                           \
    else if (mtiles == 4) G1(1, 2, 1, w & 3, 2 * (w >> 2), true);                            \
    else if (mtiles == 2) G1(1, 1, 1, w & 1, w >> 1, true);                                  \
    else G1(1, 1, 1, 0, w & 3, w < 4);                                                       \
  } else if (nta == 1) { /* tail workgroup: only columns 0..15 are live */                   \
    if (mtiles == 16) G1(4, 1, 1, 4 * w, 0, true);                                           \
    else if (mtiles == 12) G1(3, 1, 1, 3 * w, 0, true);                                      \
    else if (mtiles == 8) G1(2, 1, 1, 2 * w, 0, true);                                       \
    else G1(1, 1, 1, w < mtiles ? w : 0, 0, w < mtiles);                                     \
  } else if (mtiles == 16) G1(4, 2, 1, 4 * w, 0, true);                                      \
  else if (mtiles == 12) G1(3, 2, 1, 3 * w, 0, true);                                        \
  else if (mtiles == 8) G1(2, 2, 1, 2 * w, 0, true);                                         \
  else if (mtiles == 4) G1(1, 2, 1, w, 0, true);                                             \
  else if (mtiles == 2) G1(1, 1, 1, w & 1, w >> 1, true);                                    \
  else G1(1, 1, 1, 0, w & 1, w < 2);

// A whole 1x1 layer: dst[cout][NC] = act(W * src[cin][NC] + bias), the waves splitting the output rows; b_off < 0: no bias.
// Ends with a barrier.  alias: dst overlaps src -> all reads complete (barrier) before any store.
// (The k = 3 convs are the ResNet1D engine's, and their dealing with them: conv_op of resnet1d.hip.)
template <int NC, int L>
__device__ __forceinline__ void conv_gemm(const Ctx &c, int w_off, int b_off, const float *src, int cin, float *dst, int cout,
                                          bool alias, int act = 0) {
  const float *wp = c.w + w_off;
  const float *bias = b_off >= 0 ? c.w + b_off : nullptr;
  const int mtiles = (cout + 15) >> 4;
  const int w = c.wave;
#define GLDM_G1(MT, NT, P, mt0, nt0, on) gemm_passes<NC, L, 1, MT, NT, P>(c, wp, mt0, nt0, on, src, cin, dst, cout, bias, alias, act)
  GLDM_DEAL_1X1(NC, c.nta, mtiles, w, GLDM_G1)
#undef GLDM_G1
  __syncthreads();
}

}  // namespace
