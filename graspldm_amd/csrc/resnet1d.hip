// resnet1d.hip -- the fused 1-D ResNet engine of GraspLDM on gfx950:
//   * gldm_denoise[_rng] : the whole reverse-diffusion loop (T steps of TimeConditionedResNet1D.forward + the scheduler
//                          update) in ONE launch; the latent never leaves the chip between steps;
//   * gldm_decode        : ConditionalGraspPoseDecoder.forward (in_layer, ResNet1D, tmrp / class_logits heads);
//   * gldm_encode        : GraspCVAE.encode (in_layer, ResNet1D, out_layer folded into mu / logvar, reparameterisation);
//   * ss_table_kernel (the per-cloud scale / shift table of nets without a time embedding) runs in front of decode / encode.
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
//             two workgroups per CU, sample-major columns, v_mfma_f32_16x16x4_f32 through tile_gemm.h's f32 cores.
// The step is a tape of ops built on the host (build_tape) and interpreted by run_tape with every phase inlined: in the
// kernel arguments (RunArgs::pm_tape) for the 64-column engines, built in LDS by the 32-column one.
// The family, every header included below inside this file's anonymous namespace:
//   tile_gemm.h       (on mfma_prims.h) types, split-f16 arithmetic, reductions; X / H buffers, planes, the tile GEMMs, 1x1 layers:
//                     shared with the other kernel sources, included at file scope
//   r1d_gemm.h        the engine's LDS map and launch context (R1dGeo, R1dCtx), GLDM_SKIP, the GroupNorm epilogue, f32 k = 3 convs
//   r1d_tape.h        the step program: op codes and layout, quad_levels / quad16_levels, build_tape, read_op
//   r1d_debug.h       diagnostic builds only: wave stamps, environment knobs, the stamp report (included twice: device part, host hooks)
//   r1d_wide.h        wide-level phases of the 64-column engines: conv_pm3_wave, out_ln_*, qkv_att_pm, qkv_att16_pm, resblock_pm
//   r1d_rows.h        phases of the 32-column f32 engine: layer_norm_*, attention_pair, resblock4_valu
//   quad_narrow.h, quad16_narrow.h   the wave-local narrow levels of the 4- and the 16-position engine
//   r1d_chain.h       the hand-off between workgroups: ChainHdr, chain_give, chain_take
//   diffusion_step.h  Philox normals and the scheduler updates (shared with unet1d.hip and pose_ops.hip)
// Here: RunArgs, conv_op, run_tape, r1d_kernel, ss_table_kernel; the host side (validation, engine selection, workspace layout, work
// plan, launch); the entry points.  The small ops either side of the engine (cond-embed, pose prologue / epilogue, step noise)
// are pose_ops.hip.
#include "tile_gemm.h"

namespace {

constexpr int kMaxSegs = 64;  // tiles (+ one spliced step segment) a persistent workgroup can be given

#include "r1d_gemm.h"
#include "r1d_tape.h"
#include "r1d_debug.h"   // the device part
#include "r1d_wide.h"
#include "r1d_rows.h"
#include "quad_narrow.h"
#include "quad16_narrow.h"
#include "r1d_chain.h"
#include "diffusion_step.h"

// ---------------------------------------------------------- the network ----
constexpr int kParkBytes = 256 * 64 * 4;   // one [256][64] f32 tile per workgroup (R1dCtx::park)

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
  float *park;            // position-major engine with a 256-channel last level: 64 KiB of scratch per workgroup (R1dCtx::park)
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

// A conv op of the tape: dst[cout][NC] = W * im2col(src[cin][NC]) + bias under g's epilogue, the waves splitting the output
// rows.  Ends with a barrier.  alias: dst overlaps src -> all reads complete (barrier) before any store.
// Output widths are 16 x {1, 2, 4, 8, 12, 16} rows (validate() enforces it).
// (Tried and dropped: running the <= 64-channel levels column-parallel, one wave per n-tile with no
// barriers inside the level: those phases are bound by per-wave issue, not by the barriers, and with
// half the waves active every op took 1.7-2x longer.  And the opposite, 8 waves per 32-column tile
// with the statistics of a wide group exchanged between wave pairs: correct, but at 128 VGPRs per
// wave the k-loops spill and the launch was 5-7 % slower than with 4 waves.)
template <int NC, int L>
__device__ __forceinline__ void conv_op(const R1dCtx &c, int w_off, int b_off, const float *src, int cin, int ktaps,
                                        float *dst, int cout, bool alias, const GnEpilogue &g) {
  if (GLDM_SKIP(c, 8)) return;
  const float *wp = c.w + w_off;
  const float *bias = b_off >= 0 ? c.w + b_off : nullptr;
  const int mtiles = (cout + 15) >> 4;
  const int w = c.wave;
  if (ktaps == 3) {
    if constexpr (NC == 64) {
      // 64-column engines: 8 waves share the m-tiles (L = 4: the three taps tie the 4 position tiles together; L = 16:
      // tiles of 4 positions x 4 samples, taps by shifted plane reads).  Only the levels' down convs come this way.
      // (Dealt here and not in a function of r1d_wide.h: one more level of calls changes the kernels' machine code.)
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
    } else {
      conv3_f32<NC, L>(c, wp, bias, src, cin, dst, cout, alias, g);
    }
  } else {
#define GLDM_G1(MT, NT, P, mt0, nt0, on) gemm_passes<NC, L, 1, MT, NT, P>(c, wp, mt0, nt0, on, src, cin, dst, cout, bias, alias, 0)
    GLDM_DEAL_1X1(NC, c.nta, mtiles, w, GLDM_G1)
#undef GLDM_G1
  }
  __syncthreads();
}

template <int NC, int L>
__device__ __forceinline__ void run_tape(const R1dCtx &c0, const gldm_r1d_desc &d, const int *tape, kernarg_int *ktape, int n_ops, int E, long long *stamps) {
  constexpr bool KARG = NC == 64;
  for (int op = 0; op < n_ops; ++op) {
    if (stamps && c0.tid == 0) stamps[op] = (long long)__builtin_readcyclecounter();
    // the lane ids are laundered per op: otherwise every variant's lane-derived LDS offsets are
    // hoisted out of the step loop as invariants and live (spilled) across the whole kernel
    R1dCtx c = c0;
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
        conv_op<NC, L>(c, o[1], o[2], c.lds + o[3], o[5], o[7] & 255, c.lds + o[4], o[6], (o[7] & kFlagAlias) != 0, g);
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
          if (c.ss_lane) {   // pose decoder: the per-cloud table (wave uniform: the launch has one or not); R1dCtx::ss_lane of a
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

template <int NC, int L>
__global__ __launch_bounds__(R1dGeo<NC>::kThreads, 2) void r1d_kernel(const RunArgs a) {
  using GG = R1dGeo<NC>;
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
  R1dCtx c{{a.weights, lds, (int)threadIdx.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), (int)threadIdx.x & 63,
            GG::kNT}, a.skip};
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
    tape[1023] = PM ? a.pm_nops : build_tape<NC>(d, tape);
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
  constexpr bool kCeLds = PM;
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

// ---------------------------------------------------------- the host side ----
bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

constexpr int kEngineNC = 32;  // denoiser / decoder geometry: 32 columns, two workgroups per CU
int engine_nc() { return kEngineNC; }

#include "r1d_debug.h"   // the host hooks (dbg_*): empty unless built with -DGLDM_DEBUG_KNOBS

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

// Level widths of the 64-column engines: 32 / 64 / 128 / 256 channels behind the first level, at most 128 below the last
// one (attention levels)
bool wide_widths(const gldm_r1d_desc *d) {
  for (int i = 1; i <= d->n_levels; ++i) {
    const int C = d->dims[i];
    if (!(C == 32 || C == 64 || C == 128 || C == 256)) return false;
    if (i < d->n_levels && C > 128) return false;
  }
  return true;
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
  return wide_widths(d);
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
  return wide_widths(d);
}
bool wide_engine(const gldm_r1d_desc *d) { return pm_supported(d) || pm16_supported(d); }   // 64-column tiles

using gldm_dev::cu_count;

// header | hand-off granules | (256-byte aligned) the decoder's scale/shift table | (256-byte aligned) park scratch
// Park scratch: where the 16-position 64-column engine parks the residual stream of a 256-channel last level (PG<16>::kW):
// 64 KiB per workgroup of the launch (at most one per CU); the 4-position engine keeps it in LDS.  Offsets are -1 where the
// descriptor has no such region.
struct WsLayout { long long tiles, ss_off, park_off, total; int nc; };
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
  w.park_off = -1;
  if (!pm_supported(d) && pm16_supported(d) && d->dims[d->n_levels] == 256) {
    bytes = (bytes + 255) & ~255LL;
    w.park_off = bytes;
    bytes += (w.tiles < cu_count() ? w.tiles : cu_count()) * kParkBytes;
  }
  w.total = bytes;
  return w;
}

// Work plan of one launch.  `slots` = workgroups resident at once (two 32-column tiles per CU).  A batch of
// up to `slots` tiles is one workgroup per tile.  A larger one runs `slots` persistent workgroups: each owns
// `rounds` whole tiles, and the `left` tiles beyond the whole rounds are NOT run as a last, partly empty
// round (5120 latents = 640 tiles on 512 slots would take two rounds for 1.25 rounds of work): each is cut
// along the step axis into `chain` segments that a group of `chain` consecutive slots runs in turn, so every
// slot ends up with (nearly) the same number of tile-steps.
struct Plan { int grid, slots, rounds, left, chain, seglen; };

Plan make_plan(int n_samples, int n_steps, int L, int nc, bool allow_chain = true) {
  const int slots = dbg_slots(cu_count() * (nc == 32 ? 2 : 1));
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
  const size_t lds_bytes = dbg_lds_bytes((size_t)R1dGeo<NC>::kLdsFloats * sizeof(float));
  gldm_dev::launch_dynamic_lds<r1d_kernel<NC, L>>(dim3(tiles), dim3(R1dGeo<NC>::kThreads), (int)lds_bytes, lds_bytes, s, a);
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
  a.n_cus = cu_count();
  a.park = nullptr;
  a.pm_nops = 0;
  if (pm) {
    static_assert(8 * GLDM_R1D_MAX_LEVELS + 2 <= kPmMaxOps && sizeof(RunArgs) <= 4096, "64-column tape in the kernel arguments");
    // 16-position nets: the wave-local levels take their scale / shift rows from the per-cloud table or a 64-wide embedding
    const bool use_quad = !dbg_noquad() && !(pm16 && !(a_in.ss_tab != nullptr || a_in.d.emb_dim == 64));
    a.pm_nops = build_tape<64>(a_in.d, a.pm_tape, use_quad);
    const WsLayout wl = ws_layout(&a_in.d, a_in.n_samples);
    if (wl.park_off >= 0) a.park = reinterpret_cast<float *>(reinterpret_cast<char *>(a_in.ws) + wl.park_off);
  }
  dbg_arm(a);   // diagnostic builds only (r1d_debug.h); the shipped library reads no environment
  const int rc = pm4 ? launch_one<64, 4>(a, tiles, s)
                     : (pm16 ? launch_one<64, 16>(a, tiles, s)
                             : (L == 4 ? launch_one<kEngineNC, 4>(a, tiles, s) : launch_one<kEngineNC, 16>(a, tiles, s)));
  dbg_report(a, pm, pm16);
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

// What every engine entry point fills of RunArgs: the net, its inputs and outputs, one pass with no scheduler.  Everything
// else starts at zero (no time embedding, no noise, no table); gldm_denoise[_rng] add the loop, gldm_encode the mixing.
RunArgs engine_args(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond, const float *x_in,
                    int n_samples, float *out0, float *out1, void *workspace) {
  RunArgs a{};
  a.d = *desc;
  a.weights = weights; a.cemb = cemb; a.samples_per_cond = samples_per_cond;
  a.x_in = x_in; a.n_samples = n_samples; a.n_steps = 1; a.sched_kind = GLDM_SCHED_NONE;
  a.out0 = out0; a.out1 = out1; a.ws = reinterpret_cast<float *>(workspace);
  return a;
}
}  // namespace

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
  RunArgs a = engine_args(desc, weights, cemb, samples_per_cond, x_in, n_samples, x_out, nullptr, workspace);
  a.temb = temb; a.semb = sample_emb; a.timesteps = timesteps; a.sample_t = sample_t; a.n_steps = n_steps;
  a.sched_kind = sched_kind; a.clip_sample = clip_sample; a.sched_coef = sched_coef; a.step_noise = step_noise;
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
  RunArgs a = engine_args(desc, weights, cemb, samples_per_cond, x_in, n_samples, x_out, nullptr, workspace);
  a.temb = temb; a.semb = sample_emb; a.timesteps = timesteps; a.n_steps = n_steps;
  a.sched_kind = GLDM_SCHED_DDPM; a.clip_sample = clip_sample; a.sched_coef = sched_coef;
  a.noise_seed = noise_seed; a.noise_base = noise_base; a.noise_on = 1;
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_decode(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond,
                         const float *z_h, int n_samples, float *tmrp, float *logit, void *workspace,
                         gldm_stream_t stream) {
  int st = validate(desc);
  if (st != GLDM_OK) return st;
  if (!weights || !cemb || !z_h || !tmrp || !logit || !workspace || n_samples <= 0 || samples_per_cond <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (desc->latent_dim <= 0 || desc->n_head != 7 || desc->head_kind != GLDM_HEAD_DECODER) return GLDM_ERR_INVALID_ARG;
  RunArgs a = engine_args(desc, weights, cemb, samples_per_cond, z_h, n_samples, tmrp, logit, workspace);
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
  RunArgs a = engine_args(desc, weights, cemb, samples_per_cond, h, n_samples, mu, logvar, workspace);
  a.out2 = z; a.eps = eps; a.mix_mu = mix_mu; a.mix_eps = mix_eps; a.eps_times_std = eps_times_std;
  if (!launch_ss_table(a, reinterpret_cast<hipStream_t>(stream))) return GLDM_ERR_LAUNCH;
  return launch_r1d(a, reinterpret_cast<hipStream_t>(stream));
}
