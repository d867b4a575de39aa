// conv3d.hip -- the Conv3d(k = 3, p = 1) of PVConv's voxel branch (ext/pvcnn/modules/pvconv.py:47-84) on gfx950:
//   conv3d_k3_kernel            implicit GEMM on v_mfma_f32_16x16x4_f32                     (gldm_conv3d_k3[_cl])
//   conv3d_k3_pl_kernel         the same conv on split-f16 operands, brick pre-split in LDS  (gldm_conv3d_k3_f16x2[_gn])
//   conv3d_k3_fewch_sp_kernel   split-f16, a few input channels (3 -> 48 at 24^3)            (gldm_conv3d_k3_f16x2)
//   conv3d_k3_generic_kernel    any shape, direct form on the VALU                           (gldm_conv3d_k3_generic)
// What follows the convs (GroupNorm, SE gate, devoxelize) is voxel_norm.hip.
//
// Mapping of the f32 kernel: a workgroup (4 waves) owns a 4 x 4 x r brick of output voxels (16 r outputs =
// r n-tiles of 16) for ALL output channels.  Per 16-input-channel block the input brick with
// its one-voxel halo (6 x 6 x (r+2), zero padded at the grid border) is staged in LDS once and
// serves all 27 taps: a tap is a constant LDS offset, so the k-loop is LDS reads + MFMA only.
// Weights (fragment order, k = tap * Cin_pad + ci) stream from L2 one tap ahead.  The LDS row
// stride is = 16 (mod 32) dwords so the 4-row x 16-voxel B-fragment reads are conflict free.
// Two workgroups fit per CU (62 KiB LDS each): one stages while the other computes.
// Every conv's epilogue also emits per-brick per-channel (sum, sum of squares) (voxel_geom.h) so GroupNorm needs
// no extra pass over the tensor for its statistics (combined in f64, fixed order).
#include "mfma_prims.h"
#include "voxel_geom.h"

namespace {

#ifdef GLDM_DEBUG_KNOBS
__device__ long long g_c3_stamp[32];
#define GLDM_C3_STAMP(i) \
  do { if (blockIdx.x == 5 && blockIdx.y == (gridDim.y >> 1) && threadIdx.x == 0) g_c3_stamp[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define GLDM_C3_STAMP(i) do {} while (0)
#endif

// Not mfma_prims.h's dpp_mov: that one is __builtin_amdgcn_mov_dpp, this one update_dpp(0, ...), which has the compiler clear
// the destination with a v_mov_b32 in front of each.  Swapping it in changes the code of every conv kernel (fewer
// v_mov_b32, more s_nop around the epilogue's DPP adds); whether that is faster has not been measured, so the form the
// convs were tuned with stays.
template <int CTRL>
__device__ __forceinline__ float c3_dpp_mov(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float x) {  // every lane of a 16-lane DPP row ends with the row's sum
  x += c3_dpp_mov<0xB1>(x);   // quad_perm [1,0,3,2]
  x += c3_dpp_mov<0x4E>(x);   // quad_perm [2,3,0,1]
  x += c3_dpp_mov<0x141>(x);  // row_half_mirror
  x += c3_dpp_mov<0x140>(x);  // row_mirror
  return x;
}

constexpr int kConvThreads = 256;

// z extent of a brick row in LDS: r + 2, or, where the brick is staged four z at a time, r + 8: float4 slots aligned with
// the grid's own z (slot k = z 4 k - 4 .. 4 k - 1), so that every load is a 16-byte aligned dwordx4 inside the grid and
// the two end slots of a row are all zero padding, written once (resolutions up to 24: the wider bricks would lose
// their second workgroup per CU to the padding)
__host__ __device__ constexpr bool brick_vec4(int r) { return r <= 24; }
__host__ __device__ constexpr int brick_zp(int r) { return brick_vec4(r) ? r + 8 : r + 2; }  // vec4: z = -4 .. r + 3
__host__ __device__ constexpr int brick_row_stride(int r) {  // dwords per channel row in LDS, = 16 mod 32
  return ((6 * 6 * brick_zp(r) + 31) / 32 * 32 + 16) - 32 >= 6 * 6 * brick_zp(r) ? (6 * 6 * brick_zp(r) + 31) / 32 * 32 - 16
                                                                                 : (6 * 6 * brick_zp(r) + 31) / 32 * 32 + 16;
}

// JN: k-steps of 4 input channels per tap and 16-channel block that hold real channels (Cin <= 4: 1, else 4)
template <int MT, int NTW, int JN>
__global__ __launch_bounds__(kConvThreads, 2) void conv3d_k3_kernel(const float *__restrict__ x,
                                                                    const float *__restrict__ wp,
                                                                    const float *__restrict__ bias, int cin, int cout,
                                                                    int r_arg, float *__restrict__ y,
                                                                    float *__restrict__ partial, int cout_total, int co0,
                                                                    int out_cl) {
  // out_cl: y is written channel-last, [b][r^3][cout_total] (see conv3d_k3_pl_kernel); cout % 4 == 0 then
  // cout output channels starting at channel co0 of a cout_total-channel conv (wp / bias already point at the slice):
  // wide convs (256 ch @ 8^3, 128 ch @ 16^3: PVCNN2's feature propagation) run as two launches of half the m-tiles
  constexpr int r = 4 * NTW;  // the instantiation fixes the resolution: every division below is by a constant (with a
  (void)r_arg;                // run-time r the index maps of a workgroup cost 8 k cycles before its first load)
  extern __shared__ float lds[];
  // Everything outside the tap loops (index maps, staging, barriers, epilogue) is short latency-bound work that shares
  // its SIMD with the other workgroups' MFMA streams: it gets issue priority (the streams need one slot per 32 cycles
  // and lose nothing); measured on the 48 -> 96 conv at 12^3, its epilogue took 70 k cycles without.
  __builtin_amdgcn_s_setprio(3);
  GLDM_C3_STAMP(0);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kq = lane >> 4;
  const int bpr = r / kBrick;                       // bricks per axis
  const int bx0 = (blockIdx.x / bpr) * kBrick, by0 = (blockIdx.x % bpr) * kBrick;
  const int b = blockIdx.y;
  constexpr bool kVec = brick_vec4(r);
  constexpr int r3 = r * r * r, zp = brick_zp(r), bv = 36 * zp, bvp = brick_row_stride(r);
  const int cblocks = (cin + 15) >> 4, kblocks = 27 * cblocks;
  x += (size_t)b * cin * r3;
  y += out_cl ? (size_t)b * cout_total * r3 + co0 : ((size_t)b * cout_total + co0) * r3;
  const WStream wv(wp, lane);  // weight fragments: buffer loads, scalar offsets (see wstream.h)
  const lds_f *l3 = (const lds_f *)lds;

  // output voxel of (n-tile, lane column) in brick coordinates; LDS base of its (0,0,0) tap
  int obase[NTW], gvox[NTW];
#pragma unroll
  for (int ni = 0; ni < NTW; ++ni) {
    const int o = 16 * (wave * NTW + ni) + col;       // 0 .. 16 r - 1
    const int iz = o % r, ixy = o / r, ix = ixy >> 2, iy = ixy & 3;
    obase[ni] = (ix * 6 + iy) * zp + iz + (kVec ? 3 : 0) + kq * bvp;  // + row kq of each 4-row k-step (vec4: z = -1 sits at 3)
    gvox[ni] = ((bx0 + ix) * r + by0 + iy) * r + iz;
  }
  f32x4 acc[MT][NTW];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    f32x4 bvv;
#pragma unroll
    for (int q = 0; q < 4; ++q) bvv[q] = bias[min(16 * mi + 4 * kq + q, cout - 1)];
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] = bvv;
  }

  // Staging map, computed once.  Scalar form: thread t copies brick elements t, t + 256, ... (SQ of them) of every
  // channel.  Vector form (kVec): a brick row is r / 4 + 2 float4 slots aligned with the grid's z; thread t owns the
  // interior slot t (36 rows x r / 4 of them, at most one per thread): ONE aligned dwordx4 load per channel and ONE
  // ds_write_b128 -- 16 + 16 instructions per thread and block at r = 24 instead of 64 + 64 -- and nothing else: the
  // end slots of every row and the rows outside the grid are zero for the whole life of the workgroup and are written
  // once, before the first block.  That matters because every instruction of these phases waits for a slot between
  // the co-resident workgroup's MFMAs (45-90 cycles each): the staging is priced by its instruction count.
  constexpr int kSlotsRow = r / 4, kSlots = 36 * kSlotsRow;
  static_assert(!kVec || kSlots <= kConvThreads, "one interior slot per thread");
  constexpr int SQ = kVec ? 1 : (36 * (4 * NTW + 2) + kConvThreads - 1) / kConvThreads;  // scalar: 4 at r = 24, 2 at r = 12
  constexpr int kStageCh = JN == 1 ? 4 : 16;  // a <= 4-channel input only ever reads LDS rows 0..3 (one k-step per tap)
  int s_lds[SQ], s_glb[SQ];
#pragma unroll
  for (int q = 0; q < SQ; ++q) {
    const int rem = tid + q * kConvThreads;
    s_lds[q] = -1;
    s_glb[q] = -1;
    if (kVec) {
      if (rem < kSlots) {
        const int ixy = rem / kSlotsRow, k = rem - ixy * kSlotsRow;
        const int gx = bx0 + ixy / 6 - 1, gy = by0 + ixy % 6 - 1;
        s_lds[q] = ixy * zp + 4 * (k + 1);
        if ((unsigned)gx < (unsigned)r && (unsigned)gy < (unsigned)r) s_glb[q] = (gx * r + gy) * r + 4 * k;
      }
    } else if (rem < bv) {
      s_lds[q] = rem;
      const int ixy = rem / zp, izp = rem - ixy * zp;
      const int gx = bx0 + ixy / 6 - 1, gy = by0 + ixy % 6 - 1, gz = izp - 1;
      if ((unsigned)gx < (unsigned)r && (unsigned)gy < (unsigned)r && (unsigned)gz < (unsigned)r)
        s_glb[q] = (gx * r + gy) * r + gz;
    }
  }
  if constexpr (kVec) {  // the zero padding of the brick, once: both end slots of every row, interior slots of outside rows
    const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tid < 72) {
      float *lc = lds + (tid >> 1) * zp + ((tid & 1) ? 4 * (kSlotsRow + 1) : 0);
#pragma unroll
      for (int ci = 0; ci < kStageCh; ++ci) *reinterpret_cast<f32x4 *>(lc + ci * bvp) = z4;
    }
    if (s_lds[0] >= 0 && s_glb[0] < 0) {
      float *lc = lds + s_lds[0];
#pragma unroll
      for (int ci = 0; ci < kStageCh; ++ci) *reinterpret_cast<f32x4 *>(lc + ci * bvp) = z4;
    }
  }
  // The staging is a latency problem (60 KB per block and workgroup, every load a memory round trip), so the NEXT
  // block's 16 channels are requested before the current block's MFMA loop and only written to LDS after it: the
  // round trips hide behind 1944 MFMAs per wave.
  float stg[kVec ? 1 : SQ][kVec ? 1 : kStageCh];
  f32x4 stv[kVec ? kStageCh : 1];
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, cin * r3 * 4, 0x00020000);
  auto stage_load = [&](int cb) {
    if constexpr (kVec) {
      // unconditional (threads without a slot read slot 0 and drop it); a channel past cin lies beyond the cloud's
      // slice and reads 0 by the buffer rule
      const int g0 = s_glb[0] >= 0 ? s_glb[0] : 0;
#pragma unroll
      for (int ci = 0; ci < kStageCh; ++ci)
        stv[ci] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, ((cb * 16 + ci) * r3 + g0) * 4, 0, 0));
    } else {
      const float *xc = x + (size_t)(cb * 16) * r3;
#pragma unroll
      for (int q = 0; q < SQ; ++q)
#pragma unroll
        for (int ci = 0; ci < kStageCh; ++ci) {
          stg[q][ci] = 0.f;
          if (s_glb[q] >= 0 && cb * 16 + ci < cin) stg[q][ci] = xc[(size_t)ci * r3 + s_glb[q]];
        }
    }
  };
  auto stage_store = [&]() {
    if constexpr (kVec) {
      if (s_glb[0] >= 0) {
        float *lc = lds + s_lds[0];
#pragma unroll
        for (int ci = 0; ci < kStageCh; ++ci) *reinterpret_cast<f32x4 *>(lc + ci * bvp) = stv[ci];
      }
    } else {
#pragma unroll
      for (int q = 0; q < SQ; ++q)
        if (s_lds[q] >= 0) {
          float *lc = lds + s_lds[q];
#pragma unroll
          for (int ci = 0; ci < kStageCh; ++ci) lc[ci * bvp] = stg[q][ci];
        }
    }
  };
  constexpr int kStageLoads = SQ * kStageCh;  // load instructions per thread and block
  constexpr bool kLate = r <= 12 && kStageLoads <= 32;  // measured per resolution (see the tap loop)
  constexpr bool kPipe = SQ <= 4;  // 64 staged registers beside the accumulators; wider bricks (r = 32) stage in place
  GLDM_C3_STAMP(1);
  if (kPipe) stage_load(0);
  GLDM_C3_STAMP(2);
  for (int cb = 0; cb < cblocks; ++cb) {
    __syncthreads();  // previous block's reads are done
    if (cb < 3) GLDM_C3_STAMP(3 + 4 * cb);
    if (!kPipe) stage_load(cb);
    stage_store();
    if (cb < 3) GLDM_C3_STAMP(4 + 4 * cb);
    if (kPipe && !kLate && cb + 1 < cblocks) stage_load(cb + 1);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (cb < 3) GLDM_C3_STAMP(5 + 4 * cb);
    // ---- 27 taps x JN k-steps of MFMA; weights one tap ahead, B fragments (LDS) one k-step ahead
    f32x4 a_cur[MT], a_nxt[MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) a_cur[mi] = wv[((size_t)mi * kblocks + cb) * 64];
    float bf[NTW], bn[NTW];
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) bf[ni] = l3[obase[ni]];  // tap 0, k-step 0
    __builtin_amdgcn_s_setprio(0);
    for (int tap = 0; tap < 27; ++tap) {
      // vmcnt is in order: staged loads requested before the weight loads make the first fragment wait for them.
      // Small bricks (r = 12: 32 loads per thread) are requested behind the LAST weight load of the block instead, with
      // only the last taps' MFMAs in front (8-9 % faster there; for r = 24, 64 loads inside the tap loop, 14 % slower).
#ifdef GLDM_DEBUG_KNOBS
      if (cb < 2 && (tap == 1 || tap == 2 || tap == 14)) GLDM_C3_STAMP(14 + 3 * cb + (tap == 1 ? 0 : (tap == 2 ? 1 : 2)));
#endif
      if (kLate && tap == 25 && cb + 1 < cblocks) stage_load(cb + 1);
      const int tn = tap + 1 < 27 ? tap + 1 : tap;
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) a_nxt[mi] = wv[((size_t)mi * kblocks + tn * cblocks + cb) * 64];
      __builtin_amdgcn_sched_barrier(0);   // pinned in front of this tap's MFMAs: the scheduler sinks the request to its use
      const int toff = ((tap / 9) * 6 + (tap / 3) % 3) * zp + tap % 3;
      const int tnoff = ((tn / 9) * 6 + (tn / 3) % 3) * zp + tn % 3;
#pragma unroll
      for (int j = 0; j < JN; ++j) {
        const int noff = j + 1 < JN ? toff + 4 * (j + 1) * bvp : tnoff;  // the read after the last one is redundant
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) bn[ni] = l3[obase[ni] + noff];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int ni = 0; ni < NTW; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[mi][j], bf[ni], acc[mi][ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) bf[ni] = bn[ni];
      }
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) a_cur[mi] = a_nxt[mi];
    }
    __builtin_amdgcn_s_setprio(3);
    if (cb < 3) GLDM_C3_STAMP(6 + 4 * cb);
  }
  // ---- epilogue: per-channel partial statistics of this brick, then the stores.  The stores come LAST: a barrier
  // behind them waits for every one of them to be written (vmcnt(0): 70 k cycles per workgroup at r = 12).
  __syncthreads();
  GLDM_C3_STAMP(20);
  float *s_part = lds;  // [4 waves][MT*16][2]
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 16 * mi + 4 * kq + q;
      float s = 0.f, s2 = 0.f;
#pragma unroll
      for (int ni = 0; ni < NTW; ++ni) {
        const float v = acc[mi][ni][q];
        s += v;
        s2 += v * v;
      }
      s = row16_sum(s);   // over the 16 columns of the tile: DPP (a __shfl_xor is an LDS round trip, 8 per row here)
      s2 = row16_sum(s2);
      if (col == 0 && co < cout) {
        s_part[(wave * MT * 16 + co) * 2] = s;
        s_part[(wave * MT * 16 + co) * 2 + 1] = s2;
      }
    }
  }
  GLDM_C3_STAMP(24);
  __syncthreads();
  GLDM_C3_STAMP(25);
  if (tid < cout) {
    float s = 0.f, s2 = 0.f;
    for (int w = 0; w < 4; ++w) {
      s += s_part[(w * MT * 16 + tid) * 2];
      s2 += s_part[(w * MT * 16 + tid) * 2 + 1];
    }
    float *p = partial + (((size_t)b * gridDim.x + blockIdx.x) * cout_total + co0 + tid) * 2;
    p[0] = s;
    p[1] = s2;
  }
  GLDM_C3_STAMP(26);
  if (out_cl) {
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
        if (16 * mi + 4 * kq < cout) *reinterpret_cast<f32x4 *>(y + (size_t)gvox[ni] * cout_total + 16 * mi + 4 * kq) = acc[mi][ni];
  } else {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 16 * mi + 4 * kq + q;
        if (co < cout) {
#pragma unroll
          for (int ni = 0; ni < NTW; ++ni) y[(size_t)co * r3 + gvox[ni]] = acc[mi][ni][q];
        }
      }
  }
  GLDM_C3_STAMP(21);
}

// ---- the same conv on split-f16 operands (the shipped encoder's two shapes: 48 ch @ 24^3 and 96 ch @ 12^3) ------------
// v_mfma_f32_16x16x32_f16 with every f32 operand written as hi + lo (two f16 numbers, x = hi + lo up to 2^-22 |x|) and
// the three partial products a_hi b_lo + a_lo b_hi + a_hi b_hi accumulated in f32 (mfma_split): 3/16 of the
// f32-MFMA time (csrc/mfma_prims.h, "split-f16 products": the measured accuracy is recorded there).  K is walked as (16-channel block, PAIR of taps):
// lane group g of a fragment = (tap 2 p + (g >> 1), channels 8 (g & 1) .. + 7); 27 taps = 13 pairs + one half-empty
// (zero weights).  Work is walked in groups of 3 m-tiles x 3 n-tiles so that the A sets (double buffered), the B planes
// and the accumulators fit 256 registers.  Weights: graspldm_amd/voxel.py: pack_conv3d_f16x2.
// (First form, measured and replaced: the brick kept f32 in LDS, every lane splitting its 8 channels of a voxel again
// for each (tap pair, n-tile): 2.4 / 0.9 ms per launch at 256 clouds against 2.1 / 0.8 with the pre-split planes below,
// 3.55 / 1.25 on the f32 pipe.)

constexpr int kPairs = 14;  // tap pairs per 16-channel block (the last one holds tap 26 and zeros)

// Not mfma_prims.h's wave_max: this one walks the offsets 32 .. 1, the shared one 1 .. 32 -- the same value, but the
// shared one reorders instructions in the twelve kernels that range a brick, and their code is to stay as measured.
__device__ __forceinline__ float c3_wave_max(float x) {   // x >= 0: every lane ends with the wave's maximum
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// ---- split-f16 conv with the brick PRE-SPLIT in LDS --------------------------------------------------------------------
// Splitting a lane's 8 channels of a voxel for every (tap pair, n-tile) that touches it means ~27 splits per element
// and wave, 36 VALU instructions per 18-36 MFMAs, with the two waves of a SIMD doing it in lock step.  Here the
// staging threads split each brick element ONCE and keep the two f16 planes in LDS, channel-minor:
//   [plane hi|lo][channel half][voxel of the 6 x 6 x (r + 2) haloed brick][8 channels]   (16 B per voxel, half and plane)
// so a B fragment plane is ONE ds_read_b128 per lane (voxel of its column + the tap of its lane group, channel half)
// and the tap loop is LDS reads + buffer loads + MFMA.  64 B per voxel and 16-channel block, what the f32 brick takes: the
// 24^3 brick is 59 KiB a plane set and keeps two sets (kDB below), one workgroup of 8 waves per CU (3 n-tiles each); the
// 12^3 brick 32 KiB, 4 waves.
// Staging: an item = (voxel, 8-channel half): 8 dword loads one channel apart (coalesced along z), the split
// (split_planes8), two ds_write_b128; the next block's raw values are requested before the tap loop and split / stored
// after it.
// R: grid resolution; ZB: z extent of the brick (R, or a divisor of it: the 24^3 grid can run as two 4 x 4 x 12 half bricks
// per (x, y) -- 32 KiB of planes, several workgroups of 4 waves per CU instead of one of 8, so that one brick's
// staging, barriers and epilogue run under another's MFMAs, like the 12^3 conv always did; the two halves of a brick add
// their GroupNorm partials into one zeroed slot with atomics: two addends, so the sum does not depend on their order).
// ACT: the input is the RAW output of the previous conv and GroupNorm + Swish are applied while the brick is staged:
// x' = swish(a[b][ch] x + s[b][ch]) per in-grid element, (a, s) = in_coef (gldm_groupnorm_coef: the previous conv's partial
// statistics folded with the norm's affine).  The zero padding outside the grid is the activated tensor's padding and stays
// zero.  Replaces a read + write pass of groupnorm_swish_kernel over the tensor (0.26 ms at 48 ch @ 24^3 per 256 clouds) by
// ~9 VALU instructions per staged element under the co-resident waves' MFMAs.
template <int MT, int R, int ZB, int WAVES, bool ACT = false>
__global__ __launch_bounds__(64 * WAVES, (ZB * 16 / WAVES / 16 >= 6) ? 1 : 2) void conv3d_k3_pl_kernel(const float *__restrict__ x,
                                                                                      const float *__restrict__ wp3,
                                                                                      const float *__restrict__ bias, int cin,
                                                                                      int cout, float *__restrict__ y,
                                                                                      float *__restrict__ partial,
                                                                                      const float *__restrict__ in_coef,
                                                                                      int out_cl) {
  // out_cl: y is written channel-LAST, [b][r^3][cout] (one 16-byte store per accumulator instead of four 4-byte ones):
  // the layout of a PVConv's last conv, whose readers (SE squeeze, devoxelize) then take a voxel's channels as one run
  constexpr int r = R, NTW = ZB / WAVES, kThreads = 64 * WAVES, kZParts = R / ZB;
  // tiles walked in GM x GN groups: 3 x 3 for the shipped encoder's 48 / 96 channels on 24^3 / 12^3 bricks; the power-of-two
  // widths and grids of PVCNN2 (32 / 64 / 128 channels at 32^3 .. 4^3) in groups of 4, 2 or 1
  constexpr int GM = MT % 3 == 0 ? 3 : (MT % 4 == 0 ? 4 : (MT % 2 == 0 ? 2 : 1));
  constexpr int GN = NTW % 3 == 0 ? 3 : (NTW % 2 == 0 ? 2 : 1);
  static_assert(R % ZB == 0 && ZB % WAVES == 0, "whole n-tiles per wave");
  constexpr int MG = MT / GM, NG = NTW / GN;
  // (Measured and kept out: 4 waves x 6 n-tiles on the 24^3 brick -- half the weight-fragment deliveries, but more than
  // 256 registers, hence one wave per SIMD -- 0.74 ms per launch against 0.67 for 8 waves x 3 n-tiles.)
  constexpr int zp = ZB + 2, nvox = 36 * zp, r3 = r * r * r;
  constexpr int hs = (nvox + 15) & ~15;   // units between the two channel halves of a plane: a multiple of the 16-unit bank row
  constexpr int kItems = 2 * nvox, kRounds = (kItems + kThreads - 1) / kThreads;
  // Two plane sets where the brick leaves room for them and the workgroup has the CU to itself anyway (24^3: 2 x 60 KiB): a
  // wave that is through the tap loop of block cb writes the planes of block cb + 1 into the OTHER set at once instead of
  // waiting at a barrier for the slowest wave's last reads (phase stamps: 2-5 k cycles of such waits per block, then the
  // stores, then a second barrier); one barrier per block is left.
  constexpr bool kDB = R == 24 && ZB == 24;
  // Range scale (raw input only: an activated one is bounded by the norm's affine).  Every 16-channel block is split as
  // x / s_run, s_run the largest power-of-two scale any block so far has asked for (range_pow2 of the block's largest
  // staged magnitude: the waves publish theirs in front of the block's first barrier); when it grows the accumulators --
  // bias included -- are rescaled, and the epilogue multiplies them back.  Ordinary data: s_run = 1 throughout.
  constexpr bool kRanged = !ACT;
  extern __shared__ float lds[];
  GLDM_C3_STAMP(0);
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, kq = lane >> 4;
  const int bpr = r / kBrick;
  const int bxy = blockIdx.x / kZParts, bz0 = (blockIdx.x % kZParts) * ZB;
  const int bx0 = (bxy / bpr) * kBrick, by0 = (bxy % bpr) * kBrick;
  const int b = blockIdx.y;
  const int cblocks = (cin + 15) >> 4, kblocks = kPairs * cblocks;
  x += (size_t)b * cin * r3;
  y += (size_t)b * cout * r3;
  const WStream wv(wp3, lane);
  constexpr int kSet = kSplit * 2 * hs;   // 16-byte units of one plane set
  lds_u4 *pl0 = (lds_u4 *)lds;   // 16-byte units: plane * 2 hs + half * hs + voxel.  A ds_read_b128 is served in 16-lane groups
                                // that mix columns 0-3, 12-15 of one lane row with columns 4-11 of the next (the other channel
                                // half): with hs a multiple of 16 units the two sets fall on disjoint banks

  // fragment read base of (n-tile, lane column): voxel (0,0,0)-tap of the column, this lane's channel half
  int vb[NTW];
#pragma unroll
  for (int ni = 0; ni < NTW; ++ni) {
    const int o = 16 * (wave * NTW + ni) + col;
    const int iz = o % ZB, ixy = o / ZB, ix = ixy >> 2, iy = ixy & 3;
    vb[ni] = (ix * 6 + iy) * zp + iz + (kq & 1) * hs;
  }
  f32x4 acc[MT][NTW];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    f32x4 bvv;
#pragma unroll
    for (int q = 0; q < 4; ++q) bvv[q] = bias[16 * mi + 4 * kq + q];   // cout == 16 MT (the launcher checks)
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] = bvv;
  }
  // ---- staging map: item i = (voxel i >> 1 ... ) ordered so that consecutive threads take consecutive z of one half
  int s_lds[kRounds], s_glb[kRounds];
#pragma unroll
  for (int q = 0; q < kRounds; ++q) {
    const int it = tid + q * kThreads;
    s_lds[q] = -1;
    s_glb[q] = -1;
    if (it < kItems) {
      const int h = it / nvox, v = it - h * nvox;       // half-major: a wave's loads run along z
      const int ixy = v / zp, izp = v - ixy * zp;
      const int gx = bx0 + ixy / 6 - 1, gy = by0 + ixy % 6 - 1, gz = bz0 + izp - 1;
      s_lds[q] = h * hs + v;
      if ((unsigned)gx < (unsigned)r && (unsigned)gy < (unsigned)r && (unsigned)gz < (unsigned)r)
        s_glb[q] = (gx * r + gy) * r + gz + 8 * h * r3;
    }
  }
  // halo voxels outside the grid stay zero for the whole kernel: written once, both planes
  {
    const u32x4 z4 = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < kRounds; ++q)
      if (s_lds[q] >= 0 && s_glb[q] < 0) {
#pragma unroll
        for (int k = 0; k < kSplit; ++k) {
          pl0[k * 2 * hs + s_lds[q]] = z4;
          if constexpr (kDB) pl0[kSet + k * 2 * hs + s_lds[q]] = z4;
        }
      }
  }
  float stg[kRounds][8];
  auto stage_load = [&](int cb) {
    const float *xc = x + (size_t)(cb * 16) * r3;
#pragma unroll
    for (int q = 0; q < kRounds; ++q) {
      const int g0 = s_glb[q] >= 0 ? s_glb[q] : 0;   // unconditional loads on a clamped address
#pragma unroll
      for (int j = 0; j < 8; ++j) stg[q][j] = xc[(size_t)j * r3 + g0];
    }
  };
  // ACT: (a, s) of every input channel of this cloud, behind the planes (the launcher adds the room): read back as
  // wave-wide broadcasts of four 16-byte pairs-of-pairs per staged item
  float *s_coef = lds + (kDB ? 2 : 1) * kSet * 4;   // [cin][2]
  if constexpr (ACT) {
    for (int i = tid; i < 2 * cin; i += kThreads) s_coef[i] = in_coef[(size_t)b * cin * 2 + i];
  }
  unsigned s_run_u = 0x3f800000u;   // s_run's bits, kept on the scalar side
  float *rng = s_coef;   // [WAVES] (raw input: no coefficients there; the launcher adds the room)
  auto stage_store = [&](int cb) {
    lds_u4 *pl = pl0 + (kDB ? (cb & 1) * kSet : 0);
#pragma unroll
    for (int q = 0; q < kRounds; ++q)
      if (s_glb[q] >= 0) {
        if constexpr (kRanged) {
          const float inv_run = __uint_as_float((254u << 23) - s_run_u);
#pragma unroll
          for (int j = 0; j < 8; ++j) stg[q][j] *= inv_run;
        }
        if constexpr (ACT) {
          const int h = (tid + q * kThreads) / nvox;
          const f32x4 *cf = reinterpret_cast<const f32x4 *>(s_coef + 2 * (16 * cb + 8 * h));   // (a, s) x 8 channels
#pragma unroll
          for (int j2 = 0; j2 < 4; ++j2) {
            const f32x4 c4 = cf[j2];
            const float t0 = fmaf(stg[q][2 * j2], c4[0], c4[1]), t1 = fmaf(stg[q][2 * j2 + 1], c4[2], c4[3]);
            stg[q][2 * j2] = t0 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * t0));
            stg[q][2 * j2 + 1] = t1 * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * t1));
          }
        }
        u32x4 planes[kSplit];
        split_planes8(stg[q], planes);
#pragma unroll
        for (int k = 0; k < kSplit; ++k) pl[k * 2 * hs + s_lds[q]] = planes[k];
      }
  };
  GLDM_C3_STAMP(1);
  stage_load(0);
  GLDM_C3_STAMP(2);
  for (int cb = 0; cb < cblocks; ++cb) {
    if constexpr (kRanged) {
      float mx = 0.f;
#pragma unroll
      for (int q = 0; q < kRounds; ++q)
        if (s_glb[q] >= 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(stg[q][j]));
        }
      mx = c3_wave_max(mx);
      if (lane == 0) rng[wave] = mx;
    }
    if (!kDB || kRanged || cb == 0) __syncthreads();   // the previous block's readers are done (two sets: its planes are not touched)
    if constexpr (kRanged) {
      float mx = 0.f;
#pragma unroll
      for (int w8 = 0; w8 < WAVES; ++w8) mx = fmaxf(mx, rng[w8]);
      const unsigned need = __builtin_amdgcn_readfirstlane(__float_as_uint(range_pow2(mx)));
      const unsigned s_new = (cb == 0 || need > s_run_u) ? need : s_run_u;   // positive floats order like their bits
      if (s_new != s_run_u) {   // wave uniform, never taken on ordinary data
        const float f = __uint_as_float(s_run_u) * pow2_inv(__uint_as_float(s_new));
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] *= f;
        s_run_u = s_new;
      }
    }
    if (cb < 3) GLDM_C3_STAMP(3 + 4 * cb);
    stage_store(cb);
    if (cb + 1 < cblocks) stage_load(cb + 1);
    __builtin_amdgcn_sched_barrier(0);
    if (cb < 3) GLDM_C3_STAMP(4 + 4 * cb);
    __syncthreads();   // two sets: also "everyone is through block cb - 1's taps", so block cb + 1 may overwrite its set
    if (cb < 3) GLDM_C3_STAMP(5 + 4 * cb);
    const lds_u4 *pl = pl0 + (kDB ? (cb & 1) * kSet : 0);
    u32x4 a[2][GM][kSplit];
    auto load_a = [&](int buf, int step) {   // step = pair * MG + mg
      const int p = step / MG, mg = step - p * MG;
#pragma unroll
      for (int mi = 0; mi < GM; ++mi)
#pragma unroll
        for (int k = 0; k < kSplit; ++k)
          a[buf][mi][k] = wv.raw_at((((GM * mg + mi) * kblocks + cb * kPairs + p) * kSplit) * 1024, k * 1024);
    };
    load_a(0, 0);
    __builtin_amdgcn_s_setprio(0);
    constexpr int kSteps = kPairs * MG;
    constexpr int kUnits = kPairs * NG;   // (pair, n-group) units: the B planes of unit u + 1 are requested during unit u
    constexpr bool kBPre = NG > 1;   // a second B set costs 36 registers: only where a wave has two n-groups
    u32x4 bs[kBPre ? 2 : 1][GN][kSplit];
    auto load_b = [&](int buf, int unit) {
      const int p = unit / NG, ng = unit - p * NG;
      const int ta = 2 * p, tb = 2 * p + 1 < 27 ? 2 * p + 1 : 26;
      const int offa = ((ta / 9) * 6 + (ta / 3) % 3) * zp + ta % 3, offb = ((tb / 9) * 6 + (tb / 3) % 3) * zp + tb % 3;
      const int toff = (kq >> 1) ? offb : offa;
#pragma unroll
      for (int q = 0; q < GN; ++q)
#pragma unroll
        for (int k = 0; k < kSplit; ++k) bs[buf][q][k] = pl[k * 2 * hs + vb[GN * ng + q] + toff];
    };
    if (kBPre) load_b(0, 0);
    for (int p0 = 0; p0 < kPairs; p0 += 2) {
#pragma unroll
      for (int pu = 0; pu < 2; ++pu) {
        const int p = p0 + pu;
#pragma unroll
        for (int ng = 0; ng < NG; ++ng) {
          const int unit = p * NG + ng;
          const int bcur = kBPre ? ((pu * NG + ng) & 1) : 0;   // p0 * NG is even
          if (kBPre) load_b(bcur ^ 1, unit + 1 < kUnits ? unit + 1 : unit);
          else load_b(0, unit);
#pragma unroll
          for (int mg = 0; mg < MG; ++mg) {
            const int step = p * MG + mg;
            const int cur = (pu * MG + mg) & 1;
            // the A set of the next (pair, m-group); with two n-groups a set serves both (requested in the first)
            if (ng == 0) load_a(cur ^ 1, step + 1 < kSteps ? step + 1 : step);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mi = 0; mi < GM; ++mi)
#pragma unroll
              for (int q = 0; q < GN; ++q)
                acc[GM * mg + mi][GN * ng + q] = mfma_split(a[cur][mi], bs[bcur][q], acc[GM * mg + mi][GN * ng + q]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    if (cb < 3) GLDM_C3_STAMP(6 + 4 * cb);
    __builtin_amdgcn_s_setprio(3);
  }
  // ---- epilogue: per-channel partial statistics of this brick, then the stores
  __syncthreads();
  GLDM_C3_STAMP(20);
  if constexpr (kRanged) {
    if (s_run_u != 0x3f800000u) {
      const float s_run = __uint_as_float(s_run_u);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] *= s_run;
    }
  }
  float *s_part = lds;  // [WAVES][MT * 16][2]
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 16 * mi + 4 * kq + q;
      float s = 0.f, s2 = 0.f;
#pragma unroll
      for (int ni = 0; ni < NTW; ++ni) {
        const float v = acc[mi][ni][q];
        s += v;
        s2 += v * v;
      }
      s = row16_sum(s);
      s2 = row16_sum(s2);
      if (col == 0) {
        s_part[(wave * MT * 16 + co) * 2] = s;
        s_part[(wave * MT * 16 + co) * 2 + 1] = s2;
      }
    }
  }
  __syncthreads();
  if (tid < cout) {
    float s = 0.f, s2 = 0.f;
    for (int w = 0; w < WAVES; ++w) {
      s += s_part[(w * MT * 16 + tid) * 2];
      s2 += s_part[(w * MT * 16 + tid) * 2 + 1];
    }
    float *p = partial + (((size_t)b * (gridDim.x / kZParts) + bxy) * cout + tid) * 2;
    if constexpr (kZParts == 1) {
      p[0] = s;
      p[1] = s2;
    } else {   // the slot was zeroed by the launcher; two addends: order independent
      atomicAdd(p, s);
      atomicAdd(p + 1, s2);
    }
  }
  // the output voxels of (n-tile, lane column), derived here from an opaque copy of the lane id: computed in front of
  // the block loop they were NTW more registers alive across it (one instantiation spilled)
  int gvox[NTW];
  {
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) {
      const int o = 16 * (wave * NTW + ni) + (lane_o & 15);
      const int iz = o % ZB, ixy = o / ZB, ix = ixy >> 2, iy = ixy & 3;
      gvox[ni] = ((bx0 + ix) * r + by0 + iy) * r + bz0 + iz;
    }
  }
  if (out_cl) {
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
        *reinterpret_cast<f32x4 *>(y + (size_t)gvox[ni] * cout + 16 * mi + 4 * kq) = acc[mi][ni];
  } else {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = 16 * mi + 4 * kq + q;
#pragma unroll
        for (int ni = 0; ni < NTW; ++ni) y[(size_t)co * r3 + gvox[ni]] = acc[mi][ni][q];
      }
  }
  GLDM_C3_STAMP(21);
}

// ---- split-f16 conv of a FEW input channels (the encoder's first voxel conv: 3 -> 48 at 24^3) ------------------------
// With k = tap * 16 + ci (conv3d_k3_kernel, JN = 1) a 3-channel input pays 27 k-steps of 4 on the f32 pipe for 81 real
// products per output: 0.49 ms per 256 clouds at 0.55 matrix-pipe occupancy, for a tensor whose store takes 0.1 ms.  Here
// K is packed tap-major, channel-minor without padding between taps: k = tap * CIN + ci < 27 CIN, rounded up ONCE to a
// multiple of 32 (CIN = 3: 81 -> 96 = three k-blocks of v_mfma_f32_16x16x32_f16), three f16 partial products per f32
// product as everywhere else.  Lane (g, col) of a B fragment gathers its 8 consecutive k = (tap, ci) pairs of its voxel
// from the f32 brick in LDS (8 ds_read_b32 at per-lane offsets, one n-tile ahead of their use) and splits them; the A
// planes of a k-block (MT m-tiles x 2 planes) are read once per wave.  A workgroup of 8 waves owns a 4 x 4 x R
// brick, R / 8 n-tiles per wave, 117 registers: two workgroups per CU; the haloed input brick is CIN x 6 x 6 x (R + 2)
// floats (11 KiB at R = 24).  0.32 ms.  (Measured and dropped: persistent workgroups with the weight planes in LDS and the
// next brick's input requested under the current k-loop -- 216 registers, one workgroup per CU: 0.41 ms; the same with
// two 4-wave workgroups per CU spills: 0.59 ms.)  Weights: graspldm_amd/voxel.py: pack_conv3d_fewch_f16x2.
template <int MT, int R, int CIN, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 4) void conv3d_k3_fewch_sp_kernel(const float *__restrict__ x,
                                                                           const float *__restrict__ wp3,
                                                                           const float *__restrict__ bias,
                                                                           float *__restrict__ y,
                                                                           float *__restrict__ partial) {
  constexpr int r = R, NTW = R / WAVES, kThreads = 64 * WAVES, zp = R + 2, nvox = 36 * zp, r3 = r * r * r;
  static_assert(R % WAVES == 0, "whole n-tiles per wave");
  constexpr int K = 27 * CIN, KB = (K + 31) / 32, cout = 16 * MT;
  constexpr int cs = nvox + ((nvox & 31) == 0 ? 8 : 0);   // channel stride in LDS
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int col = lane & 15, g = lane >> 4;
  const int bpr = r / kBrick;
  const int bx0 = (blockIdx.x / bpr) * kBrick, by0 = (blockIdx.x % bpr) * kBrick;
  const int b = blockIdx.y;
  x += (size_t)b * CIN * r3;
  y += (size_t)b * cout * r3;
  // ---- the haloed brick, f32, zero outside the grid; its largest magnitude for the range scale (range_pow2: the
  // grid holds voxel averages of raw coordinates / features)
  float mx = 0.f;
  for (int i = tid; i < CIN * nvox; i += kThreads) {
    const int ci = i / nvox, v = i - ci * nvox;
    const int ixy = v / zp, izp = v - ixy * zp;
    const int gx = bx0 + ixy / 6 - 1, gy = by0 + ixy % 6 - 1, gz = izp - 1;
    float val = 0.f;
    if ((unsigned)gx < (unsigned)r && (unsigned)gy < (unsigned)r && (unsigned)gz < (unsigned)r)
      val = x[(size_t)ci * r3 + (gx * r + gy) * r + gz];
    lds[ci * cs + v] = val;
    mx = fmaxf(mx, fabsf(val));
  }
  float *rng = lds + CIN * cs;   // [WAVES], behind the brick (the launcher adds the room)
  mx = c3_wave_max(mx);
  if (lane == 0) rng[wave] = mx;
  int vb[NTW], gvox[NTW];
#pragma unroll
  for (int ni = 0; ni < NTW; ++ni) {
    const int o = 16 * (wave * NTW + ni) + col;
    const int iz = o % r, ixy = o / r, ix = ixy >> 2, iy = ixy & 3;
    vb[ni] = (ix * 6 + iy) * zp + iz;
    gvox[ni] = ((bx0 + ix) * r + by0 + iy) * r + iz;
  }
  const WStream wv(wp3, lane);
  const lds_f *l3 = (const lds_f *)lds;
  __syncthreads();
  float s_in;
  {
    float m8 = 0.f;
#pragma unroll
    for (int w8 = 0; w8 < WAVES; ++w8) m8 = fmaxf(m8, rng[w8]);
    s_in = range_pow2(__uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(m8))));
  }
  const float inv_in = pow2_inv(s_in);
  f32x4 acc[MT][NTW];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const f32x4 bvv = *reinterpret_cast<const f32x4 *>(bias + 16 * mi + 4 * g) * inv_in;
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] = bvv;
  }
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    u32x4 a[MT][kSplit];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int pl = 0; pl < kSplit; ++pl) a[mi][pl] = wv.raw_at(((mi * KB + kb) * kSplit) * 1024, pl * 1024);
    int off[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * kb + 8 * g + j;
      const int tap = k / CIN, ci = k - tap * CIN;
      // k >= K: zero weights; any finite brick element serves
      off[j] = k < K ? ci * cs + ((tap / 9) * 6 + (tap / 3) % 3) * zp + tap % 3 : 0;
    }
    // the gathers run one n-tile ahead of the split + MFMAs that use them
    float v[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[0][j] = l3[vb[0] + off[j]];
#pragma unroll
    for (int ni = 0; ni < NTW; ++ni) {
      if (ni + 1 < NTW) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[(ni + 1) & 1][j] = l3[vb[ni + 1] + off[j]];
      }
      u32x4 b3[kSplit];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[ni & 1][j] *= inv_in;
      split_planes8(v[ni & 1], b3);
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) acc[mi][ni] = mfma_split(a[mi], b3, acc[mi][ni]);
    }
  }
  if (s_in != 1.0f) {   // wave uniform
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NTW; ++ni) acc[mi][ni] *= s_in;
  }
  // ---- epilogue: per-channel partial statistics of this brick, then the stores (as in conv3d_k3_pl_kernel)
  __syncthreads();
  float *s_part = lds;  // [WAVES][MT * 16][2]
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 16 * mi + 4 * g + q;
      float s = 0.f, s2 = 0.f;
#pragma unroll
      for (int ni = 0; ni < NTW; ++ni) {
        const float v = acc[mi][ni][q];
        s += v;
        s2 += v * v;
      }
      s = row16_sum(s);
      s2 = row16_sum(s2);
      if (col == 0) {
        s_part[(wave * MT * 16 + co) * 2] = s;
        s_part[(wave * MT * 16 + co) * 2 + 1] = s2;
      }
    }
  }
  __syncthreads();
  if (tid < cout) {
    float s = 0.f, s2 = 0.f;
    for (int w = 0; w < WAVES; ++w) {
      s += s_part[(w * MT * 16 + tid) * 2];
      s2 += s_part[(w * MT * 16 + tid) * 2 + 1];
    }
    float *p = partial + (((size_t)b * gridDim.x + blockIdx.x) * cout + tid) * 2;
    p[0] = s;
    p[1] = s2;
  }
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = 16 * mi + 4 * g + q;
#pragma unroll
      for (int ni = 0; ni < NTW; ++ni) y[(size_t)co * r3 + gvox[ni]] = acc[mi][ni][q];
    }
}

template <int MT, int NTW, int JN>
int launch_conv_jn(const float *x, const float *wp, const float *bias, int b, int cin, int cout, int r, float *y,
                float *partial, hipStream_t s, int cout_total, int co0, int out_cl) {
  const size_t lds_bytes = (size_t)16 * brick_row_stride(r) * sizeof(float);
  struct Tag {};  // one flag array per instantiation
  gldm_dev::allow_dynamic_lds<Tag>(reinterpret_cast<const void *>(&conv3d_k3_kernel<MT, NTW, JN>), (int)lds_bytes);
  const int bpr = r / kBrick;
  hipLaunchKernelGGL((conv3d_k3_kernel<MT, NTW, JN>), dim3(bpr * bpr, b), dim3(kConvThreads), lds_bytes, s, x, wp, bias,
                     cin, cout, r, y, partial, cout_total, co0, out_cl);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

// ---- any-shape Conv3d(k = 3, p = 1) for voxel shapes without an MFMA instantiation (PVCNN2's 256 ch @ 8^3 and
// 128 ch @ 16^3 feature-propagation convs: 16 m-tiles of accumulators do not fit a wave).  Direct form on the VALU: a
// workgroup owns a 4 x 4 x r brick like the MFMA kernels (so the GroupNorm partials have the same layout), a thread a
// voxel, weights [cout][cin][27] as stored by nn.Conv3d, wave-uniform on the scalar path.  Correctness path, not a fast
// one: these shapes are outside the shipped encoder.
__global__ __launch_bounds__(256) void conv3d_k3_generic_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const float *__restrict__ bias, int cin, int cout, int r,
                                                                float *__restrict__ y, float *__restrict__ partial) {
  __shared__ float s_red[2][4];
  const int bpr = bricks_per_axis(r), r3 = r * r * r, nvox = 16 * r;   // any r: the last brick row / column may be partial
  const int bx0 = (blockIdx.x / bpr) * kBrick, by0 = (blockIdx.x % bpr) * kBrick, b = blockIdx.y;
  x += (size_t)b * cin * r3;
  y += (size_t)b * cout * r3;
  const int tid = threadIdx.x;
  for (int co = 0; co < cout; ++co) {
    float s = 0.f, s2 = 0.f;
    for (int v = tid; v < nvox; v += 256) {
      const int iz = v % r, ixy = v / r, gx = bx0 + (ixy >> 2), gy = by0 + (ixy & 3);
      if (gx >= r || gy >= r) continue;
      float acc = bias[co];
      for (int ci = 0; ci < cin; ++ci) {
        const float *xc = x + (size_t)ci * r3;
        const float *wc = w + ((size_t)co * cin + ci) * 27;
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
          const int nx = gx + tap / 9 - 1, ny = gy + (tap / 3) % 3 - 1, nz = iz + tap % 3 - 1;
          if ((unsigned)nx < (unsigned)r && (unsigned)ny < (unsigned)r && (unsigned)nz < (unsigned)r)
            acc = fmaf(wc[tap], xc[(nx * r + ny) * r + nz], acc);
        }
      }
      y[(size_t)co * r3 + (gx * r + gy) * r + iz] = acc;
      s += acc;
      s2 += acc * acc;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    __syncthreads();
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = s; s_red[1][tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
      float *p = partial + (((size_t)b * gridDim.x + blockIdx.x) * cout + co) * 2;
      p[0] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
      p[1] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
    }
  }
}

}  // namespace

GLDM_API long long gldm_conv3d_partial_floats(int b, int cout, int r) {
  if (b <= 0 || cout <= 0 || r <= 0) return -1;
  const long long bpr = bricks_per_axis(r);
  return (long long)b * bpr * bpr * cout * 2;
}

template <int MT, int NTW>
int launch_conv(const float *x, const float *wp, const float *bias, int b, int cin, int cout, int r, float *y,
                float *partial, hipStream_t s, int out_cl, int cout_total = -1, int co0 = 0) {
  if (cout_total < 0) cout_total = cout;
  // a 3-channel input (the first voxel conv) has one real k-step per tap: skip the three of padding
  return cin <= 4 ? launch_conv_jn<MT, NTW, 1>(x, wp, bias, b, cin, cout, r, y, partial, s, cout_total, co0, out_cl)
                  : launch_conv_jn<MT, NTW, 4>(x, wp, bias, b, cin, cout, r, y, partial, s, cout_total, co0, out_cl);
}

// a conv of 2 MH m-tiles as two launches of MH (the accumulators of 16 m-tiles do not fit a wave)
template <int MH, int NTW>
int launch_conv_halves(const float *x, const float *wp, const float *bias, int b, int cin, int cout, int r, float *y,
                       float *partial, hipStream_t s, int out_cl) {
  const size_t kblocks = 27 * (size_t)((cin + 15) >> 4);
  const int half = 16 * MH;
  const int rc = launch_conv<MH, NTW>(x, wp, bias, b, cin, half, r, y, partial, s, out_cl, cout, 0);
  if (rc != GLDM_OK) return rc;
  return launch_conv<MH, NTW>(x, wp + (size_t)MH * kblocks * 256, bias + half, b, cin, cout - half, r, y, partial, s, out_cl, cout, half);
}

// The f32-MFMA instantiations, once: X(MT, NTW) for cout in (16 (MT - 1), 16 MT] at r = 4 NTW as one launch, H(MT, NTW, MH) as
// two launches of MH m-tiles.  conv_f32_plan (the shape query) and conv3d_k3_impl (the dispatch) both read this list.
#define GLDM_CONV_F32_LIST(X, H)                                                                                          \
  X(3, 6)   /* 48 ch @ 24^3  (shipped fpc/ppc PVCNN encoder) */                                                            \
  X(6, 3)   /* 96 ch @ 12^3 */                                                                                             \
  X(2, 8)   /* 32 ch @ 32^3  (PVCNN2) */                                                                                   \
  X(3, 8)   /* 33 .. 48 ch @ 32^3 */                                                                                       \
  X(4, 4)   /* 64 ch @ 16^3 */                                                                                             \
  X(8, 2)   /* 128 ch @ 8^3 */                                                                                             \
  /* half-width / half-resolution variants (the reference's encoder benchmark runs PVCNN / PVCNN2 at 0.5 / 0.5) */       \
  X(2, 4)   /* 32 ch @ 16^3 */                                                                                             \
  X(4, 2)   /* 64 ch @ 8^3 */                                                                                              \
  X(1, 4)   /* 16 ch @ 16^3 */                                                                                             \
  X(2, 2)   /* 32 ch @ 8^3 */                                                                                              \
  X(4, 1)   /* 64 ch @ 4^3 */                                                                                              \
  X(8, 1)   /* 128 ch @ 4^3 */                                                                                             \
  /* 64 ch @ 32^3 (PVCNN2 at full width under numerics.f32_only(): the split kernel serves it otherwise): 4 m-tiles x 8   \
     n-tiles of accumulators spilled 58-70 registers as one launch -- two launches of the 32-channel instantiation instead */ \
  H(4, 8, 2)                                                                                                               \
  H(16, 2, 8)   /* 256 ch @ 8^3 */                                                                                         \
  H(8, 4, 4)    /* 128 ch @ 16^3 */

// The shape part of conv3d_k3_impl: a pure function of (cout, r) (every cin >= 1 runs).  GLDM_OK or GLDM_ERR_UNSUPPORTED.
static int conv_f32_plan(int cin, int cout, int r) {
  if (cin <= 0 || cout <= 0 || r <= 0) return GLDM_ERR_UNSUPPORTED;
  if (r % 4 || (size_t)16 * brick_row_stride(r) * 4 > 160 * 1024) return GLDM_ERR_UNSUPPORTED;
  const int mt = (cout + 15) / 16, ntw = r / 4;
#define GLDM_CONV_CASE(M, N) if (mt == M && ntw == N) return GLDM_OK;
#define GLDM_CONV_HALVES(M, N, MH) GLDM_CONV_CASE(M, N)
  GLDM_CONV_F32_LIST(GLDM_CONV_CASE, GLDM_CONV_HALVES)
#undef GLDM_CONV_CASE
#undef GLDM_CONV_HALVES
  return GLDM_ERR_UNSUPPORTED;
}

static int conv3d_k3_impl(const float *x, const float *w_packed, const float *bias, int b, int cin, int cout, int r,
                          float *y, float *partial, int out_cl, gldm_stream_t stream) {
  if (!x || !w_packed || !bias || !y || !partial || b <= 0 || cin <= 0 || cout <= 0 || r <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (out_cl && cout % 4) return GLDM_ERR_UNSUPPORTED;
  if (conv_f32_plan(cin, cout, r) != GLDM_OK) return GLDM_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int mt = (cout + 15) / 16, ntw = r / 4;
#ifdef GLDM_DEBUG_KNOBS
  struct StampDump {  // diagnostic builds: GLDM_C3_STAMP=1 prints the phase clocks of one mid-grid workgroup per call
    hipStream_t s; int cin, cout, r;
    ~StampDump() {
      if (!getenv("GLDM_C3_STAMP")) return;
      long long h[32];
      (void)hipStreamSynchronize(s);
      (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_c3_stamp), sizeof(h));
      printf("conv3d %d->%d @%d: setup %lld, stage0 issue %lld", cin, cout, r, h[1] - h[0], h[2] - h[1]);
      for (int cb = 0; cb < (cin + 15) / 16 && cb < 3; ++cb)
        printf(" | cb%d: wait %lld store %lld barrier %lld taps %lld", cb, h[3 + 4 * cb] - (cb ? h[2 + 4 * cb] : h[2]),
               h[4 + 4 * cb] - h[3 + 4 * cb], h[5 + 4 * cb] - h[4 + 4 * cb], h[6 + 4 * cb] - h[5 + 4 * cb]);
      printf(" | epilogue %lld (stats %lld, barrier %lld, partials %lld, stores %lld), total %lld", h[21] - h[20], h[24] - h[20],
             h[25] - h[24], h[26] - h[25], h[21] - h[26], h[21] - h[0]);
      for (int cb = 0; cb < 2; ++cb)
        printf(" | cb%d taps: first %lld, second %lld, 2..13 %lld", cb, h[14 + 3 * cb] - h[5 + 4 * cb],
               h[15 + 3 * cb] - h[14 + 3 * cb], h[16 + 3 * cb] - h[15 + 3 * cb]);
      printf("\n");
    }
  } dump{s, cin, cout, r};
#endif
#define GLDM_CONV_CASE(M, N) \
  if (mt == M && ntw == N) return launch_conv<M, N>(x, w_packed, bias, b, cin, cout, r, y, partial, s, out_cl);
#define GLDM_CONV_HALVES(M, N, MH) \
  if (mt == M && ntw == N) return launch_conv_halves<MH, N>(x, w_packed, bias, b, cin, cout, r, y, partial, s, out_cl);
  GLDM_CONV_F32_LIST(GLDM_CONV_CASE, GLDM_CONV_HALVES)
#undef GLDM_CONV_CASE
#undef GLDM_CONV_HALVES
  return GLDM_ERR_UNSUPPORTED;
}

GLDM_API int gldm_conv3d_k3(const float *x, const float *w_packed, const float *bias, int b, int cin, int cout, int r,
                            float *y, float *partial, gldm_stream_t stream) {
  return conv3d_k3_impl(x, w_packed, bias, b, cin, cout, r, y, partial, 0, stream);
}

GLDM_API int gldm_conv3d_k3_cl(const float *x, const float *w_packed, const float *bias, int b, int cin, int cout, int r,
                               float *y_cl, float *partial, gldm_stream_t stream) {
  return conv3d_k3_impl(x, w_packed, bias, b, cin, cout, r, y_cl, partial, 1, stream);
}

template <int MT, int R, int ZB, int WAVES, bool ACT>
int launch_conv_pl_act(const float *x, const float *wp3, const float *bias, int b, int cin, int cout, float *y, float *partial,
                       const float *in_coef, int out_cl, hipStream_t s) {
  const size_t lds_bytes = (size_t)(R == 24 && ZB == 24 ? 2 : 1) * kSplit * 2 * ((36 * (ZB + 2) + 15) & ~15) * 16 +
                           (ACT ? (size_t)2 * cin * sizeof(float) : 64 /* the waves' range words */);
  struct Tag {};
  gldm_dev::allow_dynamic_lds<Tag>(reinterpret_cast<const void *>(&conv3d_k3_pl_kernel<MT, R, ZB, WAVES, ACT>), (int)lds_bytes);
  const int bpr = R / kBrick;
  if (R != ZB) {   // the halves of a brick add their partials into one slot
    if (hipMemsetAsync(partial, 0, (size_t)b * bpr * bpr * cout * 2 * sizeof(float), s) != hipSuccess) return GLDM_ERR_LAUNCH;
  }
  hipLaunchKernelGGL((conv3d_k3_pl_kernel<MT, R, ZB, WAVES, ACT>), dim3(bpr * bpr * (R / ZB), b), dim3(64 * WAVES), lds_bytes,
                     s, x, wp3, bias, cin, cout, y, partial, in_coef, out_cl);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
template <int MT, int R, int ZB, int WAVES>
int launch_conv_pl(const float *x, const float *wp3, const float *bias, int b, int cin, int cout, float *y, float *partial,
                   const float *in_coef, int out_cl, hipStream_t s) {
  return in_coef ? launch_conv_pl_act<MT, R, ZB, WAVES, true>(x, wp3, bias, b, cin, cout, y, partial, in_coef, out_cl, s)
                 : launch_conv_pl_act<MT, R, ZB, WAVES, false>(x, wp3, bias, b, cin, cout, y, partial, nullptr, out_cl, s);
}

// (4 x 4 x 12 half bricks at 24^3 -- <3, 24, 12, 4>, two co-resident workgroups of 4 waves -- measured before round 6, on three
// bf16 planes (48 KiB a half brick), 2.12 ms against 2.05 for the full-z brick: the kernel's 220 registers allow two waves per SIMD either way, and the
// halves pay a z halo and the weight stream twice.  Kept as an instantiable option, not used.  Round 6, with three f16
// products instead of six bf16 ones: A/B of the whole encoder on one box 4.69 / 4.72 ms (full brick) against 4.63 / 4.84
// (halves) -- inside the run-to-run spread, still not used.)
// Round 6, two more forms of the 24^3 conv measured on one box against this one (whole shipped encoder, 256 clouds, A/B by an
// environment switch of the diagnostic build; phase stamps of a mid-grid workgroup: taps 31 k of a brick's 70 k cycles,
// store phases 2.4-5.2 k and barrier waits 2.9-3.8 k per 16-channel block, epilogue 5.4 k):
//  * block cb + 1 split and stored INSIDE block cb's tap loop, one staging round behind every second tap pair (the other
//    plane set is free there): the store phases shrank to 0.3-1.1 k, the taps grew 10.4 -> 12.2 k and the barrier waits
//    3.5 -> 6-7 k -- 4.49-4.50 ms against 4.48: nothing.  The staging VALU work does not hide under the other wave's MFMAs;
//  * <3, 24, 24, 4>: four waves x six n-tiles (half the weight-fragment deliveries per MFMA), two workgroups per CU, no
//    staging prefetch across the tap loop (64 registers): 18-24 spilled registers, 4.58 against 4.63 ms: 1 %, not kept.
//
// The plane-staging split-f16 instantiations, once: X(cout, r, MT, R, ZB, WAVES), cin % 16 == 0.  conv_split_plan (the shape
// query) and conv3d_k3_f16x2_impl (the dispatch) both read this list; the few-channel form 3 -> 48 @ 24^3 stands in front of it.
#define GLDM_CONV_SPLIT_LIST(X)                                                                 \
  X(48, 24, 3, 24, 24, 8)                                                                        \
  X(96, 12, 6, 12, 12, 4)                                                                        \
  /* PVCNN2's power-of-two shapes (round 5; f32-MFMA kernels before) */                          \
  X(32, 32, 2, 32, 32, 8)                                                                        \
  X(64, 32, 4, 32, 32, 8)                                                                        \
  X(32, 16, 2, 16, 16, 4)                                                                        \
  X(64, 16, 4, 16, 16, 4)                                                                        \
  X(128, 16, 8, 16, 16, 8)                                                                       \
  X(64, 8, 4, 8, 8, 4)                                                                           \
  X(128, 8, 8, 8, 8, 4)                                                                          \
  X(256, 8, 16, 8, 8, 8)                                                                         \
  X(128, 4, 8, 4, 4, 4)

constexpr bool conv_split_fewch(int cin, int cout, int r) { return cin == 3 && cout == 48 && r == 24; }   // the first voxel conv

// The shape part of conv3d_k3_f16x2_impl: a pure function of (cin, cout, r).  GLDM_OK or GLDM_ERR_UNSUPPORTED.
static int conv_split_plan(int cin, int cout, int r) {
  if (cin <= 0 || cout <= 0 || r <= 0) return GLDM_ERR_UNSUPPORTED;
  if (conv_split_fewch(cin, cout, r)) return GLDM_OK;
  if (cin % 16) return GLDM_ERR_UNSUPPORTED;   // the listed kernels: cout == 16 MT exactly, no row guards
#define GLDM_CONV_CASE(C, RR, MT, R, ZB, WAVES) if (cout == C && r == RR) return GLDM_OK;
  GLDM_CONV_SPLIT_LIST(GLDM_CONV_CASE)
#undef GLDM_CONV_CASE
  return GLDM_ERR_UNSUPPORTED;
}

static int conv3d_k3_f16x2_impl(const float *x, const float *in_coef, const float *w_split, const float *bias, int b, int cin,
                                 int cout, int r, float *y, float *partial, int out_cl, gldm_stream_t stream) {
  if (!x || !w_split || !bias || !y || !partial || b <= 0 || cin <= 0 || cout <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  if ((in_coef || out_cl) && cin % 16) return GLDM_ERR_UNSUPPORTED;   // both live in the plane-staging kernels
  if (conv_split_plan(cin, cout, r) != GLDM_OK) return GLDM_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (conv_split_fewch(cin, cout, r)) {   // K = 81 packed into three k-blocks
    constexpr int kZp = 26, kNvox = 36 * kZp;
    const size_t lds_bytes = (size_t)3 * (kNvox + ((kNvox & 31) == 0 ? 8 : 0)) * sizeof(float) + 64;   // + the waves' range words
    hipLaunchKernelGGL((conv3d_k3_fewch_sp_kernel<3, 24, 3, 8>), dim3(36, b), dim3(512), lds_bytes, s, x, w_split, bias, y, partial);
    return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
  }
#ifdef GLDM_DEBUG_KNOBS
  struct StampDump {  // diagnostic builds: GLDM_C3_STAMP=1 prints the phase clocks of one mid-grid workgroup per call
    hipStream_t s; int cin, cout, r, b;
    ~StampDump() {
      if (!getenv("GLDM_C3_STAMP")) return;
      long long h[32];
      (void)hipStreamSynchronize(s);
      (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_c3_stamp), sizeof(h));
      printf("conv3d split %d->%d @%d b=%d: setup %lld, stage0 issue %lld", cin, cout, r, b, h[1] - h[0], h[2] - h[1]);
      for (int cb = 0; cb < cin / 16 && cb < 3; ++cb)
        printf(" | cb%d: wait %lld store %lld barrier %lld taps %lld", cb, h[3 + 4 * cb] - (cb ? h[2 + 4 * cb] : h[2]),
               h[4 + 4 * cb] - h[3 + 4 * cb], h[5 + 4 * cb] - h[4 + 4 * cb], h[6 + 4 * cb] - h[5 + 4 * cb]);
      printf(" | epilogue %lld, total %lld\n", h[21] - h[20], h[21] - h[0]);
    }
  } dump{s, cin, cout, r, b};
#endif
#define GLDM_CONV_CASE(C, RR, MT, R, ZB, WAVES) \
  if (cout == C && r == RR) return launch_conv_pl<MT, R, ZB, WAVES>(x, w_split, bias, b, cin, cout, y, partial, in_coef, out_cl, s);
  GLDM_CONV_SPLIT_LIST(GLDM_CONV_CASE)
#undef GLDM_CONV_CASE
  return GLDM_ERR_UNSUPPORTED;
}

GLDM_API int gldm_conv3d_k3_supported(int kind, int cin, int cout, int r) {
  if (kind == GLDM_CONV3D_F32) return conv_f32_plan(cin, cout, r);
  if (kind == GLDM_CONV3D_F16X2) return conv_split_plan(cin, cout, r);
  return GLDM_ERR_INVALID_ARG;
}

GLDM_API int gldm_conv3d_k3_f16x2(const float *x, const float *w_split, const float *bias, int b, int cin, int cout, int r,
                                   float *y, float *partial, gldm_stream_t stream) {
  return conv3d_k3_f16x2_impl(x, nullptr, w_split, bias, b, cin, cout, r, y, partial, 0, stream);
}

GLDM_API int gldm_conv3d_k3_f16x2_gn(const float *x, const float *in_coef, const float *w_split, const float *bias, int b,
                                      int cin, int cout, int r, float *y, float *partial, int out_channel_last,
                                      gldm_stream_t stream) {
  return conv3d_k3_f16x2_impl(x, in_coef, w_split, bias, b, cin, cout, r, y, partial, out_channel_last ? 1 : 0, stream);
}

GLDM_API int gldm_conv3d_k3_generic(const float *x, const float *w, const float *bias, int b, int cin, int cout, int r,
                                    float *y, float *partial, gldm_stream_t stream) {
  if (!x || !w || !bias || !y || !partial || b <= 0 || cin <= 0 || cout <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(conv3d_k3_generic_kernel, dim3(bricks_per_cloud(r), b), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, w,
                     bias, cin, cout, r, y, partial);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
