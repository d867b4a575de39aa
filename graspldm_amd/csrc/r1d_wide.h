// r1d_wide.h -- the wide-level phases of the 64-column engines r1d_kernel<64, 4> and <64, 16> (resnet1d.hip is the map of the
// family): position-major / zero-padded-row columns, GEMMs on the f16 matrix pipe through the hi + lo split with the B operands
// in LDS as pre-split planes.  k = 3 convs (gemm_pm3_pl, gemm_sm3_pl) under the GroupNorm / scale-shift / SiLU / residual
// epilogue (conv_pm3_wave), the 4-channel first level on the VALU (conv_pm3_cin4, resblock4_pm), to_out + LayerNorm + residual
// (out_ln_*), PreNorm + to_qkv + attention as one op (column_stats8, qkv_att_pm, qkv_att16_pm), the fused ResnetBlock op
// (resblock_pm).  Included by resnet1d.hip inside its anonymous
// namespace, behind r1d_gemm.h (R1dGeo, R1dCtx, GnEpilogue), r1d_tape.h (kOpInts) and r1d_debug.h (GLDM_WV_STAMP) and in front of
// quad_narrow.h / quad16_narrow.h (sqrt_up).

constexpr int kPlaneH = PG<4>::kH, kPlaneX = PG<4>::kX;   // H planes: floats [8192, 16384), X planes: [16384, 24576) (tile_gemm.h)
constexpr int kPlaneMaxC = 128;
// The 256-channel level (only ever the last one: a down conv into it and one ResnetBlock) keeps ONE tensor in LDS as
// planes (8 blocks x 8 KiB = 64 KiB, floats [16384, 32768): behind the level's f32 residual stream X, rows 0..255 =
// floats [0, 16384)): the down conv writes the planes of the new residual stream X there (and X itself as f32 rows);
// conv1 reads the planes and, behind its GroupNorm exchange barrier (every wave is past its k-loop), overwrites them with
// the planes of H; conv2 reads those and adds act(GN(conv)) to the f32 rows for the final 1x1.

// PRE of the k = 3 convs: NoPreA, or PreA (first weight fragments requested by the caller); HOOK of conv_pm3_wave: NoHook, or
// work to run in the shadow of its epilogue
struct NoPreA { static constexpr bool on = false; };
struct NoHook { __device__ __forceinline__ void operator()() const {} };

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

// Position-major k = 3 conv on split-f16 operands.  wp3: split fragments
// of [Cout x 3 Cin], k = tap * Cin + ci, 32-deep k-blocks (Cin % 32 == 0).  One set of A registers per tap: the
// moment a tap's MFMAs have issued, its registers are refilled with the next channel block's fragments of that tap,
// which then have the two other taps' MFMAs (and the partner wave's) to arrive.  The raw f32 B values of the next
// block are read from LDS while the current block's MFMAs run and split at the top of the next trip.
// The conv with the B operand read from pre-split planes: ds_read_b128 per (tile, plane), no VALU.
// B planes of the next channel block are requested while the current block's MFMAs run (second register set).
template <int MT, int P0, int NP, class PRE = NoPreA>
__device__ __forceinline__ void gemm_pm3_pl(const R1dCtx &c, const float *__restrict__ wp3, int cin, int mt0,
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
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl)
        a[buf][mi][pl] = wv.raw_at(((mt0 + mi) * kblocks + t * kb32 + kb) * kFragBytes, pl * 1024);
  };
  auto load_b = [&](int buf, int kb) {
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
__device__ __forceinline__ void gemm_sm3_pl(const R1dCtx &c, const float *__restrict__ wp3, int cin, int mt0,
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
    for (int kb0 = 0; kb0 < kb32; kb0 += 2) {   // 4 or 8 blocks, or one (a 16- or 32-channel level in front of the 256-channel one)
#pragma unroll
      for (int st = 0; st < 3; ++st) step(st, kb0);
      if (kb0 == last) break;   // an odd block count: the trip's second block does not exist (its steps would multiply block 0 again)
#pragma unroll
      for (int st = 3; st < 6; ++st) step(st, kb0);
    }
  }
}

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
__device__ __forceinline__ void conv_pm3_wave(const R1dCtx &c, const float *wp, const float *bias, int mt0,
                                              const float *src, int cin, float *dst, int cout, bool alias,
                                              const GnEpilogue &g, const PRE &pre = PRE(), const HOOK &hook = HOOK(),
                                              bool live = true) {
  using GG = R1dGeo<64>;
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
  if (has_ss && !ss_tab) {
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
__device__ __forceinline__ void conv_pm3_cin4_rounds(const R1dCtx &c, const float *wp, const float *bias, const float *src,
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
__device__ __forceinline__ void conv_pm3_cin4_any(const R1dCtx &c, const float *wp, const float *bias, const float *src,
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
    // the new residual stream's planes (a wave's 4 channels are one half of an 8-group; cout % 32 == 0).  A 256-channel
    // level behind the first one keeps them in its one plane set, which starts where the X planes do
    static_assert(PG<4>::kW == kPlaneX, "the 256-channel level's planes start at the X planes");
    if (rd * 32 < cout)
      store_planes4(c.lds + kPlaneX, rd * 32 + c.wave * 4, n, out[rd][0], out[rd][1], out[rd][2], out[rd][3]);
  }
}

__device__ __forceinline__ void conv_pm3_cin4(const R1dCtx &c, const float *wp, const float *bias, const float *src,
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
__device__ __forceinline__ void resblock4_pm(const R1dCtx &c, const int (&o)[kOpInts], int E) {
  using GG = R1dGeo<64>;
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
__device__ __forceinline__ void out_ln_wave(const R1dCtx &c, const float *wp, const float *bias, int mt0, int nt0,
                                            bool active, int p0, const float *src, int cin, float *xres, int C,
                                            const float *gain, const FIRST &first = FIRST()) {
  using GG = R1dGeo<64>;
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
__device__ __forceinline__ Frag3 out_ln_request(const R1dCtx &c, int w_off) {
  const WStream wv(c.w + w_off, c.lane);
  Frag3 f;
#pragma unroll
  for (int pl = 0; pl < kSplit; ++pl) f.p[pl] = wv.raw_at((c.wave * (kHidden / 32)) * kFragBytes, pl * 1024);   // m-tile = wave, block 0
  return f;
}
template <int LL = 4>
__device__ __forceinline__ void out_ln_pm128(const R1dCtx &c, int w_off, int b_off, const float *src, int cin, float *xres, int g_off,
                                             const Frag3 &first) {
  out_ln_wave<4, 8, true, LL, Frag3>(c, c.w + w_off, c.w + b_off, c.wave, 0, true, 0, src, cin, xres, 128, c.w + g_off, first);
}
template <int LL = 4>
__device__ __forceinline__ void out_ln_pm(const R1dCtx &c, int w_off, int b_off, const float *src, int cin, float *xres,
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
__device__ __forceinline__ void column_stats8(const R1dCtx &c, const float *src, float inv_c) {
  constexpr int NC = 64;
  using GG = R1dGeo<NC>;
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
static_assert(kAttExch + 8 * 24 * 16 <= R1dGeo<64>::kArena, "attention exchange slots");
template <int KB32>   // C / 32 (0: the 4-channel level)
__device__ __forceinline__ void qkv_att_pm(const R1dCtx &c, int w_off, int s_off, const float *src, int C) {
  constexpr int NC = 64;
  using GG = R1dGeo<NC>;
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
// (quad16_narrow.h, included behind this header, defines the attention core this op shares with the wave-local levels)
__device__ __forceinline__ void quad16_attention_head(const f32x4 (&qa)[2], const f32x4 (&ka)[2], const f32x4 (&vt)[2], f32x4 (&out)[2]);
template <int KB32>   // ceil(C / 32): a 16-channel level is one zero-padded block
__device__ __forceinline__ void qkv_att16_pm(const R1dCtx &c, int w_off, int s_off, const float *src, int C) {
  using GG = R1dGeo<64>;
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
__device__ __forceinline__ void resblock_pm_wave(const R1dCtx &c, const float *wp1, const float *b1, const float *wp2,
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
__device__ __forceinline__ void resblock_pm(const R1dCtx &c, int w1, int b1, int w2, int b2, float *X, float *H, int C,
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
