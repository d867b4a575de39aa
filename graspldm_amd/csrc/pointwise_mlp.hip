// pointwise_mlp.hip -- fused pointwise MLP layers on the tile GEMMs of tile_gemm.h.
// y[b, :, cols] = act(W x[b, :, cols] + bias) for a k = 1 Conv1d + folded BatchNorm + ReLU of SharedMLP
// (ext/pvcnn/modules/shared_mlp.py:6-35) in the native [B, C, N] layout, and optionally, on the accumulators
// before they are stored, the head  z[b, :, cols] = Wh y + bh  (PVCNNEncoder: conv_downscale + out_layer[0]
// folded, pc_encoders.py:104-111).  With the head fused `y` may be NULL: the encoder's [B, 1536, N] tensor
// (1.6 GB per 256 clouds) then never reaches HBM.  Two kernels:
//   * pointwise_mlp_sp_kernel<ADD, NT, MU> = gldm_pointwise_mlp*_f16x2*, the shipped path: weights as split-f16 fragments,
//     the staged tile as f16 planes, products on the f16 matrix pipe through the hi + lo split; 32- or 48-point tiles (NT),
//     output rows dealt in units of MU m-tiles, ADD: an addend in front of the activation;
//   * pointwise_mlp_kernel = gldm_pointwise_mlp[2], the same layer on the f32 matrix pipe (numerics.f32_only()).
//     A persistent workgroup of 8 waves takes 32 points of one cloud at a time: the [cin][32] input tile is staged
//     once in LDS (swizzled like the engine's activations) and every wave sweeps its share of the output rows over it
//     with gemm_fast_pf, weights streamed as buffer-load fragments.  The head product uses each 16-row
//     block of y straight from the accumulators as the B operand (lane (kq, col) register r = row 4 kq + r = k-step
//     r of a 16x16x4 MFMA), against head weights packed in that k order; the waves' partial z tiles meet in LDS.
// Device code first, then launch_pointwise and the entry points.
#include "tile_gemm.h"

namespace {

struct PwArgs {
  const float *x, *w, *bias, *head_w, *head_b;
  float *y, *z;
  int cin, cout, n, relu, hout, tiles_per_cloud, total_tiles;
  // optional layer in front (x [b, cin0, n] -> relu(W0 x + b0) = the [cin][32] tile of the main layer, never in HBM)
  const float *w0, *bias0;
  int cin0;
  int dyn_first;   // split-f16 kernel: units (pairs of m-tiles) >= dyn_first are handed out at run time
  int ticket_off;  // ... from a ticket at this float index of the LDS plan
  int x0_in_planes; // 48-column tiles: the front layer's f32 tile lies under the planes (see pointwise_mlp_sp_kernel)
  // split-f16 kernel, ADD instantiation: an addend in front of the activation, add[cloud * add_bs + row * add_rs + col * add_cs]
  // (a per-cloud bias: bs = cout, rs = 1, cs = 0; a [b, cout, n] tensor: bs = cout * n, rs = n, cs = 1)
  const float *add;
  long long add_bs, add_rs, add_cs;
  // split-f16 kernel: range scales (range_pow2).  The staged input tile's is measured; the front layer's output planes take
  // theirs from the bound gain0_r * max |x| + gain0_b (largest row sum of |W0|, largest |bias0|).  rng_off: float index of the
  // eight per-wave range words in the LDS plan.  ranged == 0: operands are split as they are.
  int ranged, rng_off;
  float gain0_r, gain0_b;
  int y_point_major;   // split-f16 kernel: y is [b, n, cout] (a lane's four consecutive rows of a column: one 16-byte store)
  int cin_rows;        // split-f16 kernel without a front layer: rows x really has (cin = that padded to whole 128-deep trips
                       // of the weight ring: the planes of the rows beyond are zero, like the weights' columns there)
};

__global__ __launch_bounds__(512, 2) void pointwise_mlp_kernel(const PwArgs a) {
  constexpr int NC = 32;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Ctx c{a.w, lds, tid, wave, lane, 2};
  const int col = lane & 15, kq = lane >> 4;
  const int cblocks = a.cin >> 4, mtiles = a.cout >> 4, mt_per_wave = mtiles >> 3;
  float *zpart = lds + a.cin * NC;  // [8 waves][16 rows][32 cols]
  const WStream hw(a.head_w ? a.head_w : a.w, lane);
  for (int tile = blockIdx.x; tile < a.total_tiles; tile += gridDim.x) {
    const int b = tile / a.tiles_per_cloud, c0 = (tile - b * a.tiles_per_cloud) * NC;
    __syncthreads();  // the previous tile's readers are done
    if (a.w0) {
      // layer in front: stage its [cin0][32] input tile behind the z partials, sweep its output rows (= the main
      // layer's input rows) with the same GEMM core and leave them in LDS as the main layer's tile
      float *x0 = zpart + 8 * 16 * NC;
      const float *xb0 = a.x + (size_t)b * a.cin0 * a.n + c0;
      for (int i = tid; i < a.cin0 * 8; i += 512) {
        const int row = i >> 3, q = i & 7;
        *reinterpret_cast<f32x4 *>(x0 + swz<NC>(row, 4 * q)) = *reinterpret_cast<const f32x4 *>(xb0 + (size_t)row * a.n + 4 * q);
      }
      __syncthreads();
      const int cb0 = a.cin0 >> 4, mt_per_wave0 = a.cin >> 7;  // cin output rows = cin / 16 m-tiles over 8 waves
      for (int ps = 0; ps < mt_per_wave0; ps += 2) {
        const int mt0 = wave * mt_per_wave0 + ps;
        f32x4 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const f32x4 bv = *reinterpret_cast<const f32x4 *>(a.bias0 + 16 * (mt0 + mi) + 4 * kq);
          acc[mi][0] = bv;
          acc[mi][1] = bv;
        }
        gemm_fast_pf<NC, 4, 1, 2, 2, 2>(c, a.w0, cb0, mt0, 0, x0, acc);
        lds_f *d3 = (lds_f *)lds;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              d3[swz<NC>(16 * (mt0 + mi) + 4 * kq + r, 16 * ni + col)] = fmaxf(acc[mi][ni][r], 0.f);
      }
    } else {
      const float *xb = a.x + (size_t)b * a.cin * a.n + c0;
      for (int i = tid; i < a.cin * 8; i += 512) {
        const int row = i >> 3, q = i & 7;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + (size_t)row * a.n + 4 * q);
        *reinterpret_cast<f32x4 *>(lds + swz<NC>(row, 4 * q)) = v;
      }
    }
    __syncthreads();
    f32x4 zacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int ps = 0; ps < mt_per_wave; ps += 2) {
      const int mt0 = wave * mt_per_wave + ps;
      f32x4 acc[2][2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(a.bias + 16 * (mt0 + mi) + 4 * kq);
        acc[mi][0] = bv;
        acc[mi][1] = bv;
      }
      if ((cblocks & 3) == 0) gemm_fast_pf<NC, 4, 1, 2, 2, 4>(c, a.w, cblocks, mt0, 0, lds, acc);
      else gemm_fast_pf<NC, 4, 1, 2, 2, 2>(c, a.w, cblocks, mt0, 0, lds, acc);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        if (a.relu) {
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mi][ni][r] = fmaxf(acc[mi][ni][r], 0.f);
        }
        if (a.y) {
          float *yb = a.y + ((size_t)b * a.cout + 16 * (mt0 + mi) + 4 * kq) * a.n + c0 + col;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) __builtin_nontemporal_store(acc[mi][ni][r], yb + (size_t)r * a.n + 16 * ni);
        }
        if (a.head_w) {
          const f32x4 ah = hw[(size_t)(mt0 + mi) * 64];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
              zacc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[r], acc[mi][ni][r], zacc[ni], 0, 0, 0);
        }
      }
    }
    if (a.head_w) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) zpart[(wave * 16 + 4 * kq + r) * NC + 16 * ni + col] = zacc[ni][r];
      __syncthreads();
      for (int i = tid; i < a.hout * NC; i += 512) {
        const int row = i / NC, cc = i - row * NC;
        float v = a.head_b ? a.head_b[row] : 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) v += zpart[(w8 * 16 + row) * NC + cc];
        a.z[((size_t)b * a.hout + row) * a.n + c0 + cc] = v;
      }
    }
  }
}

// ---- the same layer(s) on split-f16 operands -------------------------------------------------------------------------
// pointwise_mlp_kernel with the main GEMM on v_mfma_f32_16x16x32_bf16 (6 partial products per f32 product, see the
// split-f16 core of the position-major engine): weights pre-split on the host (mfma_a_fragments_f16x2), the [cin][32]
// input tile split ONCE while it is staged and kept in LDS as B-fragment planes
//   [32-channel block][plane hi|mid|lo][g][32 columns][8 bf16]      (6 KiB per block; cin = 768: 144 KiB)
// so the eight waves' k-loops are ds_read_b128 + buffer loads + MFMA.  A 32-column tile re-uses a weight fragment
// for two n-tiles only: 7 MB of fragments per tile, 62 B/clk if the MFMAs were never to wait -- above the 50 B/clk a CU
// draws from L2 (tools/micro/l2_stream), so fragments are requested four blocks ahead (ring of four register sets: 24 KiB
// in flight per wave) and the ring is kept full across the units of output rows.
// (Measured and dropped: 64-column tiles with K walked in 256-channel chunks -- planes of a chunk in LDS, accumulators of
// half the output rows kept across the chunks, two passes, front layer recomputed per pass on the bf16 pipe: half the
// weight bytes per column, yet the same 0.97-1.04 ms per 329 clouds as this kernel's 1.04: the stream is not what it
// waits for in the end.)
// The optional layer in front (96 -> 768: an eighth of the FLOPs) runs on the same pipe (pw_front_split: 20-25 k cycles
// per tile on the f32 pipe before) and writes its ReLU output straight into those planes; the head product is taken on the
// accumulators exactly as in the f32 kernel (the C layout of the two MFMA shapes is the same).
// f32 [row][NC] tile of the front layer: swz<32> on the first 32 columns (the two n-tiles trade places on odd rows), any
// further n-tile in place
template <int NC>
__device__ __forceinline__ int pw_swz(int row, int col) { return row * NC + (col < 32 ? (col ^ ((row & 1) << 4)) : col); }
template <int NC>   // columns of the tile: 32 or 48
__device__ __forceinline__ void store_planes4_pw(float *planes, int c0, int n, float v0, float v1, float v2, float v3) {
  unsigned h0, h1, l0, l1;
  split_f16x2(v0, v1, h0, l0);
  split_f16x2(v2, v3, h1, l1);
  const int a = ((((c0 >> 5) * kSplit) * 4 + ((c0 >> 3) & 3)) * NC + n) * 4 + ((c0 >> 2) & 1) * 2;   // dwords
  lds_u2 *d = (lds_u2 *)(planes + a);
  d[0] = u32x2_t{h0, h1};
  d[8 * NC] = u32x2_t{l0, l1};   // next plane: 4 * NC * 4 dwords
}

// The layer in front of the split-f16 main layer, on the same pipe: x0 = the f32 [cin0][32] tile (swizzled), w0s =
// split fragments of W0 [cin x cin0], KB0 = cin0 / 32.  A wave splits the whole tile ONCE into registers (its B planes
// serve all of the wave's m-tiles) and walks its m-tiles in pairs; the A registers of a (m-tile, block) are refilled
// with the next pair's fragments as soon as its MFMAs have issued.  Output: ReLU, split, into the main layer's planes.
// bsc = 1 / (range scale of the input tile), osc = that scale / the scale of the output planes (range_pow2; 1 and 1 for
// ordinary data)
template <int KB0, int NT>
__device__ __forceinline__ void pw_front_split(const WStream &w0s, const float *bias0, const float *x0, float *planes,
                                               int wave, int lane, int mt_per_wave0, bool x0_in_planes, float bsc, float osc) {
  constexpr int NC = 16 * NT;
  const int col = lane & 15, kq = lane >> 4;
  u32x4 bp[KB0][NT][kSplit];
#pragma unroll
  for (int kb = 0; kb < KB0; ++kb)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = x0[pw_swz<NC>(32 * kb + 8 * kq + j, 16 * ni + col)] * bsc;
      split_planes8(v, bp[kb][ni]);
    }
  if (x0_in_planes) __syncthreads();   // 48-column tiles: the f32 tile lies under the planes this layer is about to write
  u32x4 af[2][KB0][kSplit];
  const int mt_first = wave * mt_per_wave0, mt_last = mt_first + mt_per_wave0 - 2;
  auto load_a = [&](int mi, int kb, int mt0) {
#pragma unroll
    for (int pl = 0; pl < kSplit; ++pl) af[mi][kb][pl] = w0s.raw_at(((mt0 + mi) * KB0 + kb) * kFragBytes, pl * 1024);
  };
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int kb = 0; kb < KB0; ++kb) load_a(mi, kb, mt_first);
  for (int mt0 = mt_first; mt0 <= mt_last; mt0 += 2) {
    const int mtn = mt0 + 2 <= mt_last ? mt0 + 2 : mt_last;
    f32x4 acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias0 + 16 * (mt0 + mi) + 4 * kq) * bsc;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = bv;
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int kb = 0; kb < KB0; ++kb) {
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = mfma_split(af[mi][kb], bp[kb][ni], acc[mi][ni]);
        __builtin_amdgcn_sched_barrier(0);
        load_a(mi, kb, mtn);   // pinned here: the scheduler sinks such requests to their first use otherwise
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        store_planes4_pw<NC>(planes, 16 * (mt0 + mi) + 4 * kq, 16 * ni + col, fmaxf(acc[mi][ni][0], 0.f) * osc,
                             fmaxf(acc[mi][ni][1], 0.f) * osc, fmaxf(acc[mi][ni][2], 0.f) * osc, fmaxf(acc[mi][ni][3], 0.f) * osc);
  }
}

#ifdef GLDM_DEBUG_KNOBS
__device__ long long g_pw_stamp[64];
#define GLDM_PW_STAMP(i) \
  do { if (blockIdx.x == 5 && tile == 5 + 2 * (int)gridDim.x && (threadIdx.x & 63) == 0 && (wave == 0 || wave == 7)) \
         g_pw_stamp[(wave ? 32 : 0) + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define GLDM_PW_STAMP(i) do {} while (0)
#endif
// NT: n-tiles per tile.  2 = 32 points (96 KiB of planes at cin = 768).  3 = 48 points (144 KiB): a weight fragment then
// serves three n-tiles -- with three f16 products per block the kernel is bound by the CU's L2 rate (5 MB of fragments per
// tile at 52 B/clk = 96 k cycles against 59 k of MFMAs at 32 points), so bytes per POINT are what counts.  n % 16 == 0: a
// cloud's last tile holds 1-3 whole n-tiles (`ntv`); the others are computed on zeros and never stored.
// MU: m-tiles per unit of output rows (2; 1 for layers of fewer than 256 rows, whose 4-7 two-tile units left waves idle:
// the 128-row feature-propagation layers and the set-abstraction first layer per point)
// (Tried for MU = 1: a 128-register bound, two workgroups per CU -- these launches are short tiles whose staging -> barrier
// -> k-loop -> store chain is latency -- 96 spilled registers: the ring of four A sets and two B sets does not fit.)
template <bool ADD, int NT, int MU = 2>
__global__ __launch_bounds__(512, 2) void pointwise_mlp_sp_kernel(const PwArgs a) {
  constexpr int NC = 16 * NT;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kq = lane >> 4;
  const int kb32 = a.cin >> 5, mtiles = a.cout >> 4;
  float *planes = lds;                       // [kb32][kSplit][4][NC][4 dwords]
  float *zpart = lds;                        // [8 waves][16 rows][NC cols], over the planes once they are dead
  float *zdyn = lds + a.cin * (NC / 2) * kSplit;   // behind the planes: head products of the drawn units [unit - dyn_first][hout][NC]
  // front layer's f32 input tile [cin0][NC]: behind the planes, under zdyn (dead by then); 48-column tiles have no room
  // there -- it lies UNDER the planes and the front layer takes it into registers, then a barrier, before it writes them
  float *x0 = a.x0_in_planes ? lds : zdyn;
  int *ticket = (int *)(lds + a.ticket_off); // next unit of output rows to hand out (main layer)
  const WStream hw(a.head_w ? a.head_w : a.w, lane);
  const WStream wv(a.w, lane);
  const lds_u4 *pl3 = (const lds_u4 *)planes + kq * NC + col;   // + ((kb * kSplit + plane) * 4) * NC + 16 ni
  for (int tile = blockIdx.x; tile < a.total_tiles; tile += gridDim.x) {
    const int b = tile / a.tiles_per_cloud, c0 = (tile - b * a.tiles_per_cloud) * NC;
    const int ntv = min(NT, (a.n - c0) >> 4);   // whole n-tiles of this tile that exist
    __syncthreads();  // the previous tile's readers are done
    GLDM_PW_STAMP(0);
    if (tid == 0) *ticket = a.dyn_first;
    // range scale of the main layer's planes (range_pow2): the accumulators run in its units, `v = acc * s_main + bias` below
    float s_main = 1.0f;
    float *rng = lds + a.rng_off;   // [8]: the waves' largest staged magnitudes
    auto range_publish = [&](float mx) {
      mx = half_max(row_pair_max(row16_max(mx)));
      if (lane == 0) rng[wave] = mx;
    };
    auto range_read = [&]() {
      const f32x4 r0 = *reinterpret_cast<const f32x4 *>(rng), r1 = *reinterpret_cast<const f32x4 *>(rng + 4);
      const float mx = fmaxf(fmaxf(fmaxf(r0[0], r0[1]), fmaxf(r0[2], r0[3])), fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3])));
      return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(mx)));
    };
    if (a.w0) {
      const float *xb0 = a.x + (size_t)b * a.cin0 * a.n + c0;
      float mx = 0.f;
      for (int i = tid; i < a.cin0 * (NC / 4); i += 512) {
        const int row = i / (NC / 4), q = i - row * (NC / 4);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (4 * q < 16 * ntv) v = *reinterpret_cast<const f32x4 *>(xb0 + (size_t)row * a.n + 4 * q);
        *reinterpret_cast<f32x4 *>(x0 + pw_swz<NC>(row, 4 * q)) = v;
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
      }
      if (a.ranged) range_publish(mx);
      __syncthreads();
      GLDM_PW_STAMP(1);
      float bsc = 1.0f, osc = 1.0f;
      if (a.ranged) {
        const float m0 = range_read(), s0 = range_pow2(m0);
        s_main = range_pow2(a.gain0_r * m0 + a.gain0_b);
        bsc = pow2_inv(s0);
        osc = s0 * pow2_inv(s_main);
      }
      const int mt_per_wave0 = a.cin >> 7;   // cin / 16 m-tiles over 8 waves
      const WStream w0s(a.w0, lane);
      switch (a.cin0 >> 5) {
        case 1: pw_front_split<1, NT>(w0s, a.bias0, x0, planes, wave, lane, mt_per_wave0, a.x0_in_planes != 0, bsc, osc); break;
        case 2: pw_front_split<2, NT>(w0s, a.bias0, x0, planes, wave, lane, mt_per_wave0, a.x0_in_planes != 0, bsc, osc); break;
        default: pw_front_split<3, NT>(w0s, a.bias0, x0, planes, wave, lane, mt_per_wave0, a.x0_in_planes != 0, bsc, osc); break;
      }
    } else {
      // stage + split: item = (8-channel group, column)
      const float *xb = a.x + (size_t)b * a.cin_rows * a.n + c0;
      // The tile's range scale needs its largest magnitude before anything is split.  Up to kHold items per thread (cin <=
      // 256 at 32 points: the feature-propagation and per-point layers of the set-abstraction backbones) the staged values
      // wait in registers across the exchange barrier: ONE pass over the input.  Wider tiles take a first pass for the maximum
      // and read the tile again (from L2): measured on the feature-propagation layers of PointNet2SSG, the two-pass form alone
      // cost 60-90 % of a launch.
      constexpr int kHold = 2;
      const int items = (a.cin >> 3) * NC;
      auto stage_store = [&](int i, float (&v)[8], float inv) {
        const int kg = i / NC, scol = i - kg * NC, row = 8 * kg;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= inv;
        u32x4 pl[kSplit];
        split_planes8(v, pl);
        lds_u4 *d = (lds_u4 *)planes + (((row >> 5) * kSplit) * 4 + ((row >> 3) & 3)) * NC + scol;
        d[0] = pl[0];
        d[4 * NC] = pl[1];
      };
      auto stage_load = [&](int i, float (&v)[8]) {
        const int kg = i / NC, scol = i - kg * NC, row = 8 * kg;
        const bool in = scol < 16 * ntv && row < a.cin_rows;   // (cin_rows % 8 == 0: whole groups)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = in ? xb[(size_t)(row + j) * a.n + scol] : 0.f;
      };
      if (NT == 2 && a.ranged && items <= kHold * 512) {   // (48-point tiles exist for inputs of 640 rows and more only)
        float hv[kHold][8];
        float mx = 0.f;
#pragma unroll
        for (int q = 0; q < kHold; ++q) {
          const int i = tid + 512 * q;
          if (i < items) {
            stage_load(i, hv[q]);
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(hv[q][j]));
          }
        }
        range_publish(mx);
        __syncthreads();
        s_main = range_pow2(range_read());
        const float inv = pow2_inv(s_main);
#pragma unroll
        for (int q = 0; q < kHold; ++q) {
          const int i = tid + 512 * q;
          if (i < items) stage_store(i, hv[q], inv);
        }
      } else {
        float inv = 1.0f;
        if (a.ranged) {
          float mx = 0.f;
          for (int i = tid; i < items; i += 512) {
            float v[8];
            stage_load(i, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(v[j]));
          }
          range_publish(mx);
          __syncthreads();
          s_main = range_pow2(range_read());
          inv = pow2_inv(s_main);
        }
        for (int i = tid; i < items; i += 512) {
          float v[8];
          stage_load(i, v);
          stage_store(i, v, inv);
        }
      }
    }
    GLDM_PW_STAMP(2);
    __syncthreads();
    GLDM_PW_STAMP(3);
    f32x4 zacc[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) zacc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ---- the output rows in units of two m-tiles, handed out at run time.  With a fixed share per wave the older wave
    // of a SIMD gets the matrix pipe whenever it wants it, finishes its share at 95 % of the pair's rate and then idles
    // at the tile's last barrier while its partner, alone, cannot hide its own LDS / weight latencies (stamps: wave 0
    // done after 131 k cycles, wave 7 after 166 k, a lone wave at 58 % of the pipe).  A wave that is done takes the next
    // unit off an LDS ticket instead; the unit after the current one is drawn before the current k-loop so that its
    // first weight fragments are requested from inside that loop (the ring of four A sets never drains), and the B
    // planes of block k + 1 are read in front of the MFMAs of block k.
    const int units = mtiles / MU;
    u32x4 af[4][MU][kSplit];
    auto load_a = [&](int buf, int mt0, int kb) {
#pragma unroll
      for (int mi = 0; mi < MU; ++mi)
#pragma unroll
        for (int pl = 0; pl < kSplit; ++pl) af[buf][mi][pl] = wv.raw_at(((mt0 + mi) * kb32 + kb) * kFragBytes, pl * 1024);
    };
    u32x4 bs[2][NT][kSplit];
    auto load_b = [&](int buf, int kb) {
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int pl = 0; pl < kSplit; ++pl) bs[buf][ni][pl] = pl3[(kb * kSplit + pl) * 4 * NC + 16 * ni];
    };
    auto draw = [&]() {
      int t = 0;
      if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return __builtin_amdgcn_readfirstlane(t);
    };
    // Units below dyn_first are dealt round robin (wave w: w, w + 8, ...), the rest drawn.  The head sum must not depend
    // on who drew what: a drawn unit's head product goes to its own LDS slot (zdyn, over the dead front-layer tile), only
    // the dealt ones accumulate in the wave's zacc, and the final sum walks waves, then slots, in index order.
    const int dyn_first = a.dyn_first;
    int unit = wave;
#pragma unroll
    for (int u = 0; u < 4; ++u) load_a(u, MU * (unit < units ? unit : 0), u);   // a wave without a unit requests unit 0's (unused)
    load_b(0, 0);
    while (unit < units) {
      const int mt0 = MU * unit;
      const int nxt = unit + 8 < dyn_first ? unit + 8 : draw();
      const int mtn = MU * (nxt < units ? nxt : unit);   // past the end: harmless re-reads of this unit's fragments
      // bias and head fragments of this unit: requested now, used behind the k-loop (the bias is added last)
      f32x4 acc[MU][NT], bv[MU], ah[MU];
#pragma unroll
      for (int mi = 0; mi < MU; ++mi) {
        bv[mi] = *reinterpret_cast<const f32x4 *>(a.bias + 16 * (mt0 + mi) + 4 * kq);
        ah[mi] = hw[(size_t)(a.head_w ? mt0 + mi : 0) * 64];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      for (int kb0 = 0; kb0 < kb32; kb0 += 4) {
        const bool tail = kb0 + 4 >= kb32;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kb = kb0 + u;
          load_b((u + 1) & 1, kb + 1 < kb32 ? kb + 1 : 0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mi = 0; mi < MU; ++mi)
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = mfma_split(af[u][mi], bs[u & 1][ni], acc[mi][ni]);
          __builtin_amdgcn_sched_barrier(0);
          load_a(u, tail ? mtn : mt0, tail ? u : kb + 4);
        }
      }
#pragma unroll
      for (int mi = 0; mi < MU; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = __builtin_fmaf(acc[mi][ni][r], s_main, bv[mi][r]);   // s_main = 1: the plain sum, bit for bit
            if constexpr (ADD)
              v += a.add[(long long)b * a.add_bs + (long long)(16 * (mt0 + mi) + 4 * kq + r) * a.add_rs +
                         (long long)(c0 + (ni < ntv ? 16 * ni + col : col)) * a.add_cs];
            acc[mi][ni][r] = a.relu ? fmaxf(v, 0.f) : v;
          }
        if (a.y && a.y_point_major) {
          float *yb = a.y + ((size_t)b * a.n + c0 + col) * a.cout + 16 * (mt0 + mi) + 4 * kq;
#pragma unroll
          for (int ni = 0; ni < NT; ++ni)
            if (ni < ntv) *reinterpret_cast<f32x4 *>(yb + (size_t)16 * ni * a.cout) = acc[mi][ni];
        } else if (a.y) {
          float *yb = a.y + ((size_t)b * a.cout + 16 * (mt0 + mi) + 4 * kq) * a.n + c0 + col;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ni = 0; ni < NT; ++ni)
              if (ni < ntv) __builtin_nontemporal_store(acc[mi][ni][r], yb + (size_t)r * a.n + 16 * ni);
        }
      }
      if (a.head_w) {
        const bool drawn = unit >= dyn_first;
        f32x4 zu[NT];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) zu[ni] = drawn ? f32x4{0.f, 0.f, 0.f, 0.f} : zacc[ni];
#pragma unroll
        for (int mi = 0; mi < MU; ++mi) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int ni = 0; ni < NT; ++ni)
              zu[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[mi][r], acc[mi][ni][r], zu[ni], 0, 0, 0);
        }
        if (drawn) {
          float *slot = zdyn + (unit - dyn_first) * a.hout * NC;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (4 * kq + r < a.hout) {
#pragma unroll
              for (int ni = 0; ni < NT; ++ni) slot[(4 * kq + r) * NC + 16 * ni + col] = zu[ni][r];
            }
        } else {
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) zacc[ni] = zu[ni];
        }
      }
      unit = nxt;
    }
    GLDM_PW_STAMP(16);
    if (a.head_w) {
      __syncthreads();  // every wave is done with the planes: the z partials go over them
      GLDM_PW_STAMP(17);
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) zpart[(wave * 16 + 4 * kq + r) * NC + 16 * ni + col] = zacc[ni][r];
      __syncthreads();
      // fixed summation tree: four lanes per output (waves 2p, 2p + 1 and every fourth slot from p), then the quad
      const int nd = units - dyn_first;
      for (int i0 = 0; i0 < a.hout * NC * 4; i0 += 512) {
        const int i = i0 + tid, o = i >> 2, p = i & 3;
        const bool live = o < a.hout * NC;
        const int row = live ? o / NC : 0, cc = live ? o - row * NC : 0;
        float v = zpart[((2 * p) * 16 + row) * NC + cc] + zpart[((2 * p + 1) * 16 + row) * NC + cc];
        for (int d = p; d < nd; d += 4) v += zdyn[(d * a.hout + row) * NC + cc];
        v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
        v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
        if (live && p == 0 && cc < 16 * ntv) a.z[((size_t)b * a.hout + row) * a.n + c0 + cc] = v + (a.head_b ? a.head_b[row] : 0.f);
      }
    }
    GLDM_PW_STAMP(18);
  }
}

using gldm_dev::cu_count;

// What launch_pointwise makes of a shape: K as the kernel walks it, the unit and tile widths, and the split form's LDS plan.
struct PwPlan {
  int cin;            // K: cin_arg, or (split form without a front layer) padded to whole 128-deep trips of the weight ring
  int mu, nt;         // m-tiles per unit, 16-point n-tiles per tile
  int dyn_first, ticket_off, x0_in_planes;
  size_t lds_bytes;
};

// The shape part of launch_pointwise: a pure function of the sizes and the form flags (no pointer, no HIP call, no CU
// count).  cin0 = 0: no front layer; hout = 0: no head.  GLDM_OK and the plan, or GLDM_ERR_UNSUPPORTED.
int plan_pointwise(bool split_f16, int cin0, int cin_arg, int cout, int n, int hout, bool add, bool y_point_major, PwPlan &p) {
  if (cin0 < 0 || cin_arg <= 0 || cout <= 0 || n <= 0 || hout < 0 || hout > 16) return GLDM_ERR_UNSUPPORTED;
  if ((y_point_major || add) && !split_f16) return GLDM_ERR_UNSUPPORTED;
  const bool front = cin0 > 0, head = hout > 0;
  // The split launch without a front layer takes any multiple of 8 input rows: K is padded to whole 128-deep trips of its
  // weight ring (the caller's fragments carry zero columns there: r1d_pack.mfma_a_fragments_f16x2 of the padded matrix)
  const int cin = (split_f16 && !front && (cin_arg & 7) == 0) ? (cin_arg + 127) & ~127 : cin_arg;
  // k-blocks in pairs, 32-point tiles; output rows: 2 m-tiles x 8 waves per round on the f32 kernel, units of two m-tiles on
  // the split one (fewer than eight units -- 64 .. 224 output rows -- leave waves without a unit idle)
  // the split launch hands out its output rows in units of two m-tiles, or of one where two would leave waves idle (fewer
  // than 256 rows, no front layer / head): then any multiple of 16 rows
  // (narrow inputs only: 32-point planes within half a CU's LDS, i.e. the 32-point tile form stays)
  const int mu = (split_f16 && !front && !head && cout < 256 && ((size_t)cin * 32 * 2 * kSplit + 64) * 2 <= (size_t)160 * 1024) ? 1 : 2;
  if ((cin & 31) || (split_f16 ? (n & 15) : (n & 31)) || (split_f16 ? (cout & (16 * mu - 1)) : (cout & 255))) return GLDM_ERR_UNSUPPORTED;
  if ((front || head) && (cout & 255)) return GLDM_ERR_UNSUPPORTED;   // front layer / head: whole rounds of units only
  if (front && ((cin0 & 31) || (cin & 255))) return GLDM_ERR_UNSUPPORTED;
  size_t lds_bytes = ((size_t)cin * 32 + 8 * 16 * 32 + (size_t)cin0 * 32) * sizeof(float);
  if (split_f16) {  // `w` and `w0` hold split-f16 fragments: planes of the tile + the front layer's f32 tile
    if (cin & 127) return GLDM_ERR_UNSUPPORTED;  // the A ring walks four 32-deep blocks per trip
    if (cin0 > 96) return GLDM_ERR_UNSUPPORTED;  // the front layer keeps its whole split tile in registers (72)
  }
  int dyn_first = 0, ticket_off = 0, nt = 2, x0_in_planes = 0;
  if (split_f16) {
    // LDS plan: planes | head products of the drawn units (the front layer's f32 tile lies under them: dead by then) |
    // ticket.  As many units are drawn as have room for their head slot (all but the first round when there is no head).
    // Tile width: 48 points where 32-point planes already take more than half a CU's LDS (one workgroup per CU either way)
    // and the 48-point plan fits; the front tile then goes UNDER the planes (x0_in_planes).
    const size_t cap = (size_t)160 * 1024 - 64;   // ticket + range words
    const int units = cout / (16 * mu);
    auto plan = [&](int ncol, bool x0_under, size_t &planes, size_t &region, int &first) {
      planes = (size_t)cin * ncol * 2 * kSplit;   // bytes: cin x ncol x kSplit f16
      region = (front && !x0_under) ? (size_t)cin0 * ncol * sizeof(float) : 0;
      if (planes + region > cap) return false;
      if (x0_under && (size_t)cin0 * ncol * sizeof(float) > planes) return false;
      int drawn = units > 8 ? units - 8 : 0;
      if (head) {
        const size_t slot = (size_t)hout * ncol * sizeof(float);
        const int room = (int)((cap - planes) / slot);
        if (drawn > room) drawn = room;
        if (planes < (size_t)8 * 16 * ncol * sizeof(float)) drawn = 0;   // z partials need the planes' space
      }
      first = (units - drawn + 7) & ~7;   // whole rounds are dealt
      if (head && (size_t)(units - first) * hout * ncol * sizeof(float) > region)
        region = (size_t)(units - first) * hout * ncol * sizeof(float);
      return planes + region <= cap;
    };
    size_t planes = 0, region = 0;
    if (!plan(32, false, planes, region, dyn_first)) return GLDM_ERR_UNSUPPORTED;
    if ((planes + region + 64) * 2 > (size_t)160 * 1024 && n >= 48) {
      size_t p3 = 0, r3 = 0;
      int f3 = 0;
      if (plan(48, front, p3, r3, f3)) {
        nt = 3; planes = p3; region = r3; dyn_first = f3; x0_in_planes = front ? 1 : 0;
      }
    }
    ticket_off = (int)((planes + region) / sizeof(float));
    lds_bytes = planes + region + 64;   // ticket (16 B) + the eight range words
  }
  if (lds_bytes > 160 * 1024) return GLDM_ERR_UNSUPPORTED;
  p = PwPlan{cin, mu, nt, dyn_first, ticket_off, x0_in_planes, lds_bytes};
  return GLDM_OK;
}

int launch_pointwise(const float *x, const float *w0, const float *b0, int cin0, const float *w, const float *bias, int b,
                     int cin_arg, int cout, int n, int relu, const float *head_w, const float *head_b, int hout, float *y,
                     float *z, hipStream_t stream, bool split_f16 = false, const float *add = nullptr, long long add_bs = 0,
                     long long add_rs = 0, long long add_cs = 0, const float *front_gain = nullptr, bool y_point_major = false) {
  if (y_point_major && !y) return GLDM_ERR_UNSUPPORTED;
  if (!x || !w || !bias || b <= 0 || cin_arg <= 0 || cout <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (!y && !head_w) return GLDM_ERR_INVALID_ARG;
  if (head_w && (!z || hout <= 0 || hout > 16)) return GLDM_ERR_INVALID_ARG;
  if (w0 && (!b0 || cin0 <= 0)) return GLDM_ERR_UNSUPPORTED;
  PwPlan p{};
  const int rc = plan_pointwise(split_f16, w0 ? cin0 : 0, cin_arg, cout, n, head_w ? hout : 0, add != nullptr, y_point_major, p);
  if (rc != GLDM_OK) return rc;
  const int cin_rows = cin_arg, cin = p.cin, mu = p.mu, nt = p.nt;
  const size_t lds_bytes = p.lds_bytes;
  PwArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.head_w = head_w; a.head_b = head_b; a.y = y; a.z = z;
  a.cin = cin; a.cout = cout; a.n = n; a.relu = relu; a.hout = hout;
  a.w0 = w0; a.bias0 = b0; a.cin0 = cin0;
  a.dyn_first = p.dyn_first; a.ticket_off = p.ticket_off; a.x0_in_planes = p.x0_in_planes;
  a.add = add; a.add_bs = add_bs; a.add_rs = add_rs; a.add_cs = add_cs;
  // range scales: a lone layer measures its input tile; with a layer in front the caller's gain bounds its output
  a.y_point_major = y_point_major ? 1 : 0;
  a.cin_rows = cin_rows;
  a.rng_off = p.ticket_off + 4;
  a.ranged = split_f16 && (!w0 || front_gain);
  if (w0 && front_gain) {
    a.gain0_r = front_gain[0]; a.gain0_b = front_gain[1];
    if (!(a.gain0_r >= 0.f) || !(a.gain0_b >= 0.f)) return GLDM_ERR_INVALID_ARG;
  }
  a.tiles_per_cloud = (n + 16 * nt - 1) / (16 * nt);
  a.total_tiles = b * a.tiles_per_cloud;
  const int per_cu = lds_bytes * 2 <= 160 * 1024 ? 2 : 1;
  int grid = cu_count() * per_cu;
  if (grid > a.total_tiles) grid = a.total_tiles;
  const dim3 g(grid), t(512);
  constexpr int kLim = 160 * 1024;   // every kernel's dynamic-LDS limit: the CU's LDS
  using gldm_dev::launch_dynamic_lds;
  if (split_f16 && mu == 1 && nt == 2) {
    if (add) launch_dynamic_lds<pointwise_mlp_sp_kernel<true, 2, 1>>(g, t, kLim, lds_bytes, stream, a);
    else launch_dynamic_lds<pointwise_mlp_sp_kernel<false, 2, 1>>(g, t, kLim, lds_bytes, stream, a);
  } else if (split_f16 && add && nt == 3) launch_dynamic_lds<pointwise_mlp_sp_kernel<true, 3>>(g, t, kLim, lds_bytes, stream, a);
  else if (split_f16 && nt == 3) launch_dynamic_lds<pointwise_mlp_sp_kernel<false, 3>>(g, t, kLim, lds_bytes, stream, a);
  else if (split_f16 && add) launch_dynamic_lds<pointwise_mlp_sp_kernel<true, 2>>(g, t, kLim, lds_bytes, stream, a);
  else if (split_f16) launch_dynamic_lds<pointwise_mlp_sp_kernel<false, 2>>(g, t, kLim, lds_bytes, stream, a);
  else launch_dynamic_lds<pointwise_mlp_kernel>(g, t, kLim, lds_bytes, stream, a);
#ifdef GLDM_DEBUG_KNOBS
  if (split_f16 && getenv("GLDM_PW_STAMP")) {   // diagnostic builds: phase clocks of one steady-state tile (waves 0 and 7)
    long long h[64];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_pw_stamp), sizeof(h));
    for (int w = 0; w < 2; ++w) {
      const long long *q = h + 32 * w;
      printf("pointwise split %d(%d)->%d b=%d wave %d: stage %lld front %lld barrier %lld |", cin, cin0, cout, b, w ? 7 : 0,
             q[1] - q[0], q[2] - q[1], q[3] - q[2]);
      printf(" main %lld wait %lld head %lld total %lld\n", q[16] - q[3], q[17] - q[16], q[18] - q[17], q[18] - q[0]);
    }
  }
#endif
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
}  // namespace

GLDM_API int gldm_pointwise_mlp_supported(int split_f16, int cin0, int cin, int cout, int n, int hout, int with_addend,
                                          int point_major) {
  PwPlan p{};
  return plan_pointwise(split_f16 != 0, cin0, cin, cout, n, hout, with_addend != 0, point_major != 0, p);
}

GLDM_API int gldm_pointwise_mlp(const float *x, const float *w_packed, const float *bias, int b, int cin, int cout,
                                int n, int relu, const float *head_w_packed, const float *head_bias, int hout,
                                float *y, float *z, gldm_stream_t stream) {
  return launch_pointwise(x, nullptr, nullptr, 0, w_packed, bias, b, cin, cout, n, relu, head_w_packed, head_bias, hout,
                          y, z, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_pointwise_mlp2(const float *x, const float *w0_packed, const float *bias0, int cin0,
                                 const float *w_packed, const float *bias, int b, int cin, int cout, int n,
                                 const float *head_w_packed, const float *head_bias, int hout, float *y, float *z,
                                 gldm_stream_t stream) {
  if (!w0_packed) return GLDM_ERR_INVALID_ARG;
  return launch_pointwise(x, w0_packed, bias0, cin0, w_packed, bias, b, cin, cout, n, 1, head_w_packed, head_bias,
                          hout, y, z, reinterpret_cast<hipStream_t>(stream));
}

GLDM_API int gldm_pointwise_mlp_f16x2(const float *x, const float *w_split, const float *bias, int b, int cin, int cout,
                                       int n, int relu, const float *head_w_packed, const float *head_bias, int hout,
                                       float *y, float *z, gldm_stream_t stream) {
  return launch_pointwise(x, nullptr, nullptr, 0, w_split, bias, b, cin, cout, n, relu, head_w_packed, head_bias, hout,
                          y, z, reinterpret_cast<hipStream_t>(stream), true);
}

GLDM_API int gldm_pointwise_mlp_f16x2_pm(const float *x, const float *w_split, const float *bias, int b, int cin, int cout,
                                          int n, int relu, float *y_point_major, gldm_stream_t stream) {
  return launch_pointwise(x, nullptr, nullptr, 0, w_split, bias, b, cin, cout, n, relu, nullptr, nullptr, 0, y_point_major,
                          nullptr, reinterpret_cast<hipStream_t>(stream), true, nullptr, 0, 0, 0, nullptr, true);
}

GLDM_API int gldm_pointwise_mlp_f16x2_add(const float *x, const float *w_split, const float *bias, const float *add,
                                           long long add_cloud_stride, long long add_row_stride, long long add_col_stride, int b,
                                           int cin, int cout, int n, int relu, float *y, gldm_stream_t stream) {
  if (!add) return GLDM_ERR_INVALID_ARG;
  return launch_pointwise(x, nullptr, nullptr, 0, w_split, bias, b, cin, cout, n, relu, nullptr, nullptr, 0, y, nullptr,
                          reinterpret_cast<hipStream_t>(stream), true, add, add_cloud_stride, add_row_stride, add_col_stride);
}

GLDM_API int gldm_pointwise_mlp2_f16x2(const float *x, const float *w0_packed, const float *bias0, int cin0,
                                        const float *w_split, const float *bias, int b, int cin, int cout, int n,
                                        const float *head_w_packed, const float *head_bias, int hout,
                                        const float *front_gain, float *y, float *z, gldm_stream_t stream) {
  if (!w0_packed) return GLDM_ERR_INVALID_ARG;
  return launch_pointwise(x, w0_packed, bias0, cin0, w_split, bias, b, cin, cout, n, 1, head_w_packed, head_bias,
                          hout, y, z, reinterpret_cast<hipStream_t>(stream), true, nullptr, 0, 0, 0, front_gain);
}
