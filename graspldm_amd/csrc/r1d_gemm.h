// r1d_gemm.h -- what the ResNet1D engine (resnet1d.hip is the map of the family) adds to the tile GEMMs of tile_gemm.h: the
// top of the three layers mfma_prims.h <- tile_gemm.h <- this.
//   * GLDM_SKIP / GLDM_STAMPS, the hooks of -DGLDM_DEBUG_KNOBS diagnostic builds;
//   * R1dGeo<NC>: the engine's LDS map behind Geo<NC>'s X and H (attention buffers, the misc region: latent rows, embedding
//     sums, exchange slots, tape, segments, hand-shake words, the narrow chain's offset table) and the LDS budget;
//   * R1dCtx: Ctx + the phase-skip mask, the per-cloud scale / shift rows and the parked residual stream;
//   * GnEpilogue, gemm3_gn (one wave's share of an f32 k = 3 conv under the GroupNorm + scale/shift + SiLU + residual
//     epilogue) and conv3_f32, which deals such a conv over the waves of the 32-column engine.
// Included by resnet1d.hip inside its anonymous namespace, behind tile_gemm.h and in front of every other r1d_*.h (the
// 64-column engines' k = 3 convs are r1d_wide.h's, their dealing conv_op's in resnet1d.hip).  It needs nothing but
// tile_gemm.h, so the probes under tools/micro that time the f32 k = 3 conv include it the same way.

// Diagnostic knobs (phase skipping, per-op cycle stamps, workgroup stagger) exist only in builds made
// with -DGLDM_DEBUG_KNOBS (make EXTRA=-DGLDM_DEBUG_KNOBS); the shipped kernels contain none of them.
#ifdef GLDM_DEBUG_KNOBS
#define GLDM_SKIP(c, bit) ((c).skip & (bit))
#define GLDM_STAMPS(p) (p)
#else
#define GLDM_SKIP(c, bit) false
#define GLDM_STAMPS(p) ((long long *)nullptr)
#endif

// The engine's LDS map (floats) behind the two activation buffers of Geo<NC>.
template <int NC>
struct R1dGeo : Geo<NC> {
  using Geo<NC>::kWaves;
  using Geo<NC>::kBufH;
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
static_assert(R1dGeo<64>::kLdsFloats * 4 <= 160 * 1024, "LDS budget (1 WG/CU)");
static_assert(R1dGeo<32>::kLdsFloats * 4 * 2 <= 160 * 1024, "LDS budget (2 WG/CU)");
static_assert(PG<16>::kEnd <= R1dGeo<64>::kArena, "padded planes fit the arena");

struct R1dCtx : Ctx {
  int skip;         // diagnostic phase-skip mask (GLDM_R1D_SKIP), 0 in production
  // scale / shift rows precomputed per conditioning cloud (pose decoder: ss_table_kernel), for the tile's samples 0 and
  // 1 (16-position engine: a 16-column n-tile is one sample), or null: computed in the epilogue
  const float *ss_row[2] = {nullptr, nullptr};
  const float *ss_lane = nullptr;   // 16-position 64-column engine: the same rows for THIS LANE's sample (lane & 3), or null
  // position-major engine, 256-channel level: this workgroup's 64 KiB of global scratch where the residual stream is
  // parked (f32) between the level's down conv and the end of its ResnetBlock, while LDS holds the split planes
  float *park = nullptr;
};

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
  int tab_off = 0;     // this ResnetBlock's rows in the per-cloud scale/shift table (R1dCtx::ss_row)
};

// One wave's share of an f32 k = 3 conv under that epilogue: gemm_passes of tile_gemm.h with the parameter loads in front
// of the sweeps and the epilogue in place of the store (g.mode == 0: stored as it is).
template <int NC, int L, int MT, int NT, int PASSES>
__device__ __forceinline__ void gemm3_gn(const R1dCtx &c, const float *wp, int mt0, int nt0, bool active,
                                         const float *src, int cin, float *dst, int cout, const float *bias,
                                         bool alias, const GnEpilogue &g) {
  using GG = R1dGeo<NC>;
  f32x4 acc[PASSES][MT][NT];
  const int kq = c.lane >> 4, col = c.lane & 15;
  // ---- parameters of the GroupNorm epilogue.  Every load goes out in one batch: before the k-sweep when the
  // variant is a single pass (registers to spare: the round trip hides behind the GEMM), else at the start of
  // the epilogue, in the shadow of the statistics.
  constexpr bool kEarlyParams = PASSES == 1;
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
  for (int p = 0; p < PASSES; ++p) {   // the sweeps of gemm_passes (tile_gemm.h)
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
      if ((cin & 15) == 0) gemm_fast<NC, L, 3, MT, NT>(c, wp, cin >> 4, mt0 + p * MT, nt0, src, acc[p]);
      else gemm_small<NC, L, MT, NT>(c, wp, (3 * cin + 15) >> 4, mt0 + p * MT, nt0, src, cin, 3, acc[p]);
    }
  }
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
  if (alias) __syncthreads();
  if (active) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) store_tiles<NC, MT, NT>(c, acc[p], mt0 + p * MT, nt0, dst, cout, 0);
  }
}

#undef GLDM_LOAD_GN_PARAMS

// An f32 k = 3 conv of the 32-column engine dealt over its 4 waves (<= 2 m-tiles per sweep).  No barrier behind it.
template <int NC, int L>
__device__ __forceinline__ void conv3_f32(const R1dCtx &c, const float *wp, const float *bias, const float *src, int cin,
                                          float *dst, int cout, bool alias, const GnEpilogue &g) {
  const int mtiles = (cout + 15) >> 4;
  const int w = c.wave;
#define GLDM_G3(MT, NT, P, mt0, nt0, on) gemm3_gn<NC, L, MT, NT, P>(c, wp, mt0, nt0, on, src, cin, dst, cout, bias, alias, g)
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
#undef GLDM_G3
}
