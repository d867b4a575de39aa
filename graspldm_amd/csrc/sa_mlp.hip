// sa_mlp.hip -- the fused set-abstraction core on the tile GEMMs of tile_gemm.h.
// PointNetSAModule (ext/pvcnn/modules/pointnet.py:100-111) without the FPS:
//   grouped = cat(p[idx] - centre, f[idx])          (BallQuery.forward)
//   out[b, :, j] = max_k  SharedMLP2d(grouped)[b, :, j, k]
// The grouped tensor ([B, 3+C, M, U], 4.3 MB per cloud at SSG-SA2) never exists in HBM: a workgroup gathers its tile of
// (centre, neighbour) columns straight into LDS, runs the MLP layers (BatchNorm folded, ReLU) with weights streamed from L2
// and takes the max over the U neighbours on chip.  Three kernels:
//   * sa_mlp3_kernel<SUBMAX, QUADS, PRE> = gldm_sa_mlp_forward_f16x2[_pre], the shipped path: 64-column tiles as pre-split
//     f16 planes, layers on the f16 matrix pipe through the hi + lo split (gemm1_pl), range-scaled operands; PRE: the first
//     layer hoisted into a per-point term; SUBMAX > 1: several tiles per workgroup pass for narrow nets;
//   * sa_mlp2_kernel = gldm_sa_mlp_forward where the layer plan fits: 128-column f32 tiles, max taken on the accumulators;
//   * sa_mlp_kernel  = gldm_sa_mlp_forward otherwise: one 64-column f32 tile = 64/U centres x U neighbours on conv_gemm (1x1 layers).
//     HBM traffic: 12N + 4CN + 12M + 4MU (idx) in, 4 Cout M out per cloud.
// Device code first, then launch_sa3 and the entry points.
#include "tile_gemm.h"

namespace {

struct SaArgs {
  const float *points, *centers, *feat;
  const int32_t *idx;
  const float *weights;
  float *out;
  int c, n, m, u, n_layers;
  int cin_pad[4], cout[4], w_off[4], b_off[4];
  // split-f16 kernel: range scales on (range_pow2).  gain_r / gain_b: per layer, the largest row sum of |W| and the largest
  // |bias| (BatchNorm folded), from the packer: |layer output| <= gain_r * max |input| + gain_b
  int ranged;
  float gain_r[4], gain_b[4];
  // split-f16 kernel, first layer hoisted (gldm_sa_mlp_forward_f16x2_pre): pre [b][n][c1] = W1b f + b1 per POINT (one
  // pointwise GEMM per cloud instead of one per (centre, neighbour) pair: every point sits in ~16 balls), wa_off: float
  // index in `weights` of W1a [c1][4] (the coordinate columns x, y, z, 0).  The MFMA layers are then layers 2.. of the module.
  const float *pre;
  int c1, wa_off;
  int pre_bcast;   // pre is ONE row [c1] for every point (a module without features: the row is the folded bias b1)
};

__global__ __launch_bounds__(Geo<64>::kThreads, 2) void sa_mlp_kernel(const SaArgs a) {
  using GG = Geo<64>;
  constexpr int NC = 64;
  extern __shared__ float lds[];
  Ctx c{a.weights, lds, (int)threadIdx.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), (int)threadIdx.x & 63,
        GG::kNT};
  const int b = blockIdx.y, tile = blockIdx.x;
  const int cpt = NC / a.u;                 // centres per tile
  const int j0 = tile * cpt;
  const float *pts = a.points + (size_t)b * 3 * a.n;
  const float *ctr = a.centers + (size_t)b * 3 * a.m;
  const float *feat = a.feat ? a.feat + (size_t)b * a.c * a.n : nullptr;
  const int32_t *idx = a.idx + ((size_t)b * a.m + j0) * a.u;
  float *X = lds + GG::kBufX, *H = lds + GG::kBufH;
  // ---- gather the neighbour tile: rows 0..2 relative coords, 3..3+C features, zero pad
  {
    const int col = c.lane, jj = col / a.u;
    const bool live = j0 + jj < a.m;
    const int id = live ? idx[col] : 0;
    const int rows = a.cin_pad[0];
    // six rows per wave in flight at a time: every element is a scattered memory round trip, and issued one by one
    // (load, wait, store) the gather took as long as the tile's MFMAs.  (Requesting the NEXT tile's rows before the
    // MLP from a persistent workgroup was slower: the in-order vmcnt makes the first weight fragment wait for them.)
    for (int r0 = c.wave; r0 < rows; r0 += 6 * GG::kWaves) {
      float v[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int r = r0 + q * GG::kWaves;
        v[q] = 0.f;
        if (live && r < rows) {
          if (r < 3) v[q] = pts[r * a.n + id] - ctr[r * a.m + j0 + jj];
          else if (r < 3 + a.c) v[q] = feat[(size_t)(r - 3) * a.n + id];
        }
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int r = r0 + q * GG::kWaves;
        if (r < rows) X[swz<NC>(r, col)] = v[q];
      }
    }
  }
  __syncthreads();
  // ---- grouped MLP (1x1 convs + folded BN + ReLU), ping-pong X <-> H
  float *src = X, *dst = H;
  for (int l = 0; l < a.n_layers; ++l) {
    conv_gemm<NC, 4>(c, a.w_off[l], a.b_off[l], src, a.cin_pad[l], dst, a.cout[l], false, 1);   // (L is the k = 3 convs' layout: any)
    float *t = src; src = dst; dst = t;
  }
  // ---- max over the U neighbours of each centre
  const int cout = a.cout[a.n_layers - 1];
  float *out = a.out + (size_t)b * cout * a.m;
  for (int i = c.tid; i < cout * cpt; i += GG::kThreads) {
    const int row = i / cpt, jj = i - row * cpt;
    if (j0 + jj >= a.m) continue;
    float mx = -3.0e38f;
    for (int k = 0; k < a.u; ++k) mx = fmaxf(mx, src[swz<NC>(row, jj * a.u + k)]);
    out[(size_t)row * a.m + j0 + jj] = mx;
  }
}

// ======================================================== fused set abstraction, 128-column tiles ==
// sa_mlp_kernel at twice the tile: 128 columns = 128 / U centres x U neighbours per workgroup (8 waves, one workgroup
// per CU).  Every weight fragment then serves 8 n-tiles, a layer's fill / epilogue / barrier is paid once per 128
// columns, and the last layer's output is never stored: max over a centre's neighbours is taken on the accumulators
// (in-lane over the centre's n-tiles, DPP over the 16 columns of a tile; ReLU after the max, it is monotone) and only
// [cout][centres] leaves the CU.  LDS: region A [max(cin_pad0, cout1)][128] (the gathered tile, later layer 2's
// output) + region B [cout0][128] (+ [cout2] for 4 layers).  Shapes outside this plan run on sa_mlp_kernel.

template <int MT, int NT>
__device__ __forceinline__ void sa2_tiles(const Ctx &c, const SaArgs &a, int l, int mt0, int nt0, const float *src,
                                          float *dst, bool last, int j0, float *outb) {
  constexpr int NC = 128;
  const int col = c.lane & 15, kq = c.lane >> 4;
  const float *wp = a.weights + a.w_off[l], *bias = a.weights + a.b_off[l];
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 16 * (mt0 + mi) + 4 * kq);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = bv;
  }
  const int cblocks = a.cin_pad[l] >> 4;
  if ((cblocks & 3) == 0) gemm_fast_pf<NC, 16, 1, MT, NT, 4>(c, wp, cblocks, mt0, nt0, src, acc);
  else gemm_fast_pf<NC, 16, 1, MT, NT, 2>(c, wp, cblocks, mt0, nt0, src, acc);  // the launcher checked: even
  if (!last) {
    lds_f *d3 = (lds_f *)dst;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          d3[swz<NC>(16 * (mt0 + mi) + 4 * kq + r, 16 * (nt0 + ni) + col)] = fmaxf(acc[mi][ni][r], 0.f);
    return;
  }
  // max over each centre's U columns: tpc = U / 16 n-tiles per centre (1, 2 or 4; NT is a multiple of it)
  const int tpc = a.u >> 4;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m[NT];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) m[ni] = acc[mi][ni][r];
      if (tpc >= 2) {
#pragma unroll
        for (int ni = 0; ni < NT; ni += 2) m[ni] = fmaxf(m[ni], m[ni + 1 < NT ? ni + 1 : ni]);
      }
      if (tpc >= 4) {
#pragma unroll
        for (int ni = 0; ni < NT; ni += 4) m[ni] = fmaxf(m[ni], m[ni + 2 < NT ? ni + 2 : ni]);
      }
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        if (ni % tpc) continue;  // wave uniform
        const float v = fmaxf(row16_max(m[ni]), 0.f);
        const int jj = (nt0 + ni) / tpc;  // centre of the tile
        if (col == 0 && j0 + jj < a.m) outb[(size_t)(16 * (mt0 + mi) + 4 * kq + r) * a.m + j0 + jj] = v;
      }
    }
}

// The gather of tile t + 1 is requested in front of tile t's last layer and stored after it: its scattered round
// trips (12 k cycles exposed per tile before) run under the longest GEMM of the tile.  Everything about it is
// UNCONDITIONAL -- clamped tile index, clamped addresses, the store of a last redundant tile -- because a load behind a
// branch, or one whose only consumer is behind a branch, is waited for on the spot.  (The in-order vmcnt makes the
// layer's first weight fragment wait for the gather's loads: a few hundred cycles once per tile, measured.)
constexpr int kSaFly = 32;  // feature rows per thread in flight: 4 row quarters x 32 = 128 feature channels

struct SaTile {
  const float *pts, *ctr, *feat;
  int id, jj, j0;
  bool live;
};

__device__ __forceinline__ SaTile sa2_tile(const SaArgs &a, int t, int tiles_per_cloud, int cpt, int col) {
  const int b = t / tiles_per_cloud, tile = t - b * tiles_per_cloud;
  SaTile s;
  s.j0 = tile * cpt;
  s.jj = col / a.u;
  s.live = s.j0 + s.jj < a.m;
  s.pts = a.points + (size_t)b * 3 * a.n;
  s.ctr = a.centers + (size_t)b * 3 * a.m;
  s.feat = a.feat ? a.feat + (size_t)b * a.c * a.n : a.points;
  const int32_t *idx = a.idx + ((size_t)b * a.m + s.j0) * a.u;
  s.id = idx[s.live ? col : 0];
  s.id = s.live ? s.id : 0;
  return s;
}

__device__ __forceinline__ void sa2_gather_load(const SaArgs &a, const SaTile &s, int rq, float &xyz, float (&v)[kSaFly]) {
  const int r3 = rq < 3 ? rq : 0;
  xyz = s.pts[r3 * a.n + s.id] - s.ctr[r3 * a.m + (s.live ? s.j0 + s.jj : 0)];
  const int cmax = a.c > 0 ? a.c - 1 : 0;
#pragma unroll
  for (int q = 0; q < kSaFly; ++q) {
    const int f = rq + 4 * q;
    v[q] = s.feat[(size_t)(f < cmax ? f : cmax) * a.n + s.id];
  }
}

__device__ __forceinline__ void sa2_gather_store(const SaArgs &a, const SaTile &s, int rq, int col, float xyz,
                                                 const float (&v)[kSaFly], float *A) {
  constexpr int NC = 128;
  lds_f *A3 = (lds_f *)A;
  const int rows = a.cin_pad[0];
  if (rq < 3) A3[swz<NC>(rq, col)] = s.live ? xyz : 0.f;
#pragma unroll
  for (int q = 0; q < kSaFly; ++q) {
    const int f = rq + 4 * q;
    if (3 + f < rows) A3[swz<NC>(3 + f, col)] = (s.live && f < a.c) ? v[q] : 0.f;
  }
  for (int r = 3 + 4 * kSaFly + rq; r < rows; r += 4) A3[swz<NC>(r, col)] = 0.f;  // zero pad beyond 131 rows
}

__global__ __launch_bounds__(512, 1) void sa_mlp2_kernel(const SaArgs a, int rows_a, int tiles_per_cloud, int total_tiles) {
  constexpr int NC = 128;
  extern __shared__ float lds[];
  Ctx c{a.weights, lds, (int)threadIdx.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), (int)threadIdx.x & 63,
        8};
  const int cpt = NC / a.u;  // centres per tile
  float *A = lds, *B = lds + (size_t)rows_a * NC;
  const int w = c.wave, col = c.tid & (NC - 1), rq = c.tid >> 7;
  auto layer = [&](int l, const float *src, float *dst, int j0, float *outb) {
    const bool last = l == a.n_layers - 1;
    const int mtiles = a.cout[l] >> 4;
    // the lane ids are laundered per call: otherwise every variant's lane-derived LDS offsets are hoisted out of the
    // tile loop as invariants and live (spilled) across the whole kernel
    Ctx cl = c;
    asm volatile("" : "+v"(cl.tid), "+v"(cl.lane));
    if (mtiles >= 8) {  // one m-tile x all 8 n-tiles per pass: every weight fragment serves 128 columns
      for (int p = 0; p < (mtiles >> 3); ++p) sa2_tiles<1, 8>(cl, a, l, w + 8 * p, 0, src, dst, last, j0, outb);
    } else if (mtiles == 4) sa2_tiles<1, 4>(cl, a, l, w & 3, 4 * (w >> 2), src, dst, last, j0, outb);
    else sa2_tiles<1, 2>(cl, a, l, w & 1, 2 * (w >> 1), src, dst, last, j0, outb);
  };
  // persistent workgroups (a tile is 45 us of work and a workgroup launch several)
  int t = blockIdx.x;
  {
    const SaTile s = sa2_tile(a, t, tiles_per_cloud, cpt, col);
    float xyz, v[kSaFly];
    sa2_gather_load(a, s, rq, xyz, v);
    sa2_gather_store(a, s, rq, col, xyz, v, A);
  }
  __syncthreads();
  for (; t < total_tiles; t += gridDim.x) {
    const int b = t / tiles_per_cloud, j0 = (t - b * tiles_per_cloud) * cpt;
    float *outb = a.out + (size_t)b * a.cout[a.n_layers - 1] * a.m;
    float *src = A, *dst = B;
    for (int l = 0; l + 1 < a.n_layers; ++l) {
      layer(l, src, dst, j0, outb);
      __syncthreads();
      float *tsw = src; src = dst; dst = tsw;
    }
    const int tn = t + (int)gridDim.x < total_tiles ? t + (int)gridDim.x : t;
    const SaTile s = sa2_tile(a, tn, tiles_per_cloud, cpt, col);
    float xyz, v[kSaFly];
    sa2_gather_load(a, s, rq, xyz, v);
    layer(a.n_layers - 1, src, dst, j0, outb);
    __syncthreads();  // the last layer may have been reading region A
    sa2_gather_store(a, s, rq, col, xyz, v, A);
    __syncthreads();
  }
}

// ======================================================== fused set abstraction on split-f16 planes ==
// The same module core (gather + grouped MLP + max over the neighbours, ext/pvcnn/modules/pointnet.py:100-111) with the
// GEMMs on the bf16 matrix pipe: every f32 product as six bf16 partial products (hi / mid / lo splits of both operands,
// f32 accumulation: see the split-f16 core above), 6/16 of the f32-MFMA time.  A tile is 64 columns = 64 / U centres x U
// neighbours; the gathered tile and every hidden layer's output live in LDS as pre-split planes in B-fragment order
// (the position-major engine's geometry: 12 KiB per 32 channels), written once by their producer (the gather threads hold
// four consecutive channels of a column; a layer's epilogue its accumulators' four consecutive rows), so the k-loops are
// ds_read_b128 + buffer loads + MFMA (gemm1_pl).  Region A: the gathered tile, later the odd hidden layers' outputs;
// region B: the even ones'.  The last layer is never stored: max over a centre's neighbours on the accumulators.
// Persistent workgroups; the next tile's gather is requested in front of the last layer and stored behind it.
// Shapes: cin_pad a multiple of 32 (zero weights beyond the real rows), hidden widths multiples of 32 up to 256, U in
// {16, 32, 64}; anything else runs on the f32 kernels above.
constexpr int kSaBlockFloats = PG<4>::kBlockFloats;   // one 32-channel block of a 64-column tile's planes
constexpr int kSa3Quads = 9;   // row quads per gather thread: 8 threads per column x 9 x 4 rows >= 259 + padding
template <int NT, class FIRST>
__device__ __forceinline__ void sa3_gemm(const Ctx &c, const float *wp, int kb, int mt, int nt0, const float *planes,
                                         f32x4 (&acc)[1][NT], const FIRST &first) {
  switch (kb) {
    case 1: gemm1_pl<1, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 2: gemm1_pl<2, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 3: gemm1_pl<3, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 4: gemm1_pl<4, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 5: gemm1_pl<5, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 6: gemm1_pl<6, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
    case 9: gemm1_pl<9, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;   // 259 + 3 -> 288 rows (PVCNN2 SA4)
    default: gemm1_pl<8, 1, NT, NoPre, 1, 4, FIRST>(c, wp, mt, nt0, planes, acc, NoPre(), first); break;
  }
}
// The wave's first m-tile of layer l (the mapping of sa_mlp3_kernel) and the request for its block-0 fragments: issued
// right behind the previous layer's k-loop, in flight under its epilogue and the barrier (each layer of a tile used to
// start with a cold L2 round trip: ~1.9 k cycles against 2-5 k of MFMAs).
__device__ __forceinline__ int sa3_first_mt(const SaArgs &a, int l, int w) {
  const int mtiles = a.cout[l] >> 4;
  return (l + 1 < a.n_layers && mtiles < 8) ? (mtiles == 4 ? (w & 3) : (w & 1)) : w;
}
__device__ __forceinline__ Frag3 sa3_request(const Ctx &c, const SaArgs &a, int l) {
  const WStream wv(a.weights + a.w_off[l], c.lane);
  const int mt = sa3_first_mt(a, l, c.wave), kb = a.cin_pad[l] >> 5;
  const int mtc = mt < (a.cout[l] >> 4) ? mt : 0;   // waves beyond a narrow last layer: any valid fragment
  Frag3 f;
#pragma unroll
  for (int pl = 0; pl < kSplit; ++pl) f.p[pl] = wv.raw_at(mtc * kb * kFragBytes, pl * 1024);
  return f;
}
// REQ: request the next layer's first fragments right behind this k-loop (in flight under the epilogue and the barrier)
// bsc = 1 / (scale of the input planes): the accumulators run in the input's units; osc = that scale / the scale of the
// output planes (both 1 for ordinary data: range_pow2)
template <int NT, class FIRST, bool REQ>
__device__ __forceinline__ Frag3 sa3_hidden(const Ctx &c, const SaArgs &a, int l, int mt, int nt0, const float *src, float *dst,
                                            const FIRST &first, float bsc, float osc) {
  const int col = c.lane & 15, kq = c.lane >> 4;
  f32x4 acc[1][NT];
  const f32x4 bv = *reinterpret_cast<const f32x4 *>(a.weights + a.b_off[l] + 16 * mt + 4 * kq) * bsc;
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) acc[0][ni] = bv;
  sa3_gemm<NT, FIRST>(c, a.weights + a.w_off[l], a.cin_pad[l] >> 5, mt, nt0, src, acc, first);
  Frag3 nxt{};
  if constexpr (REQ) nxt = sa3_request(c, a, l + 1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ni = 0; ni < NT; ++ni)
    store_planes4(dst, 16 * mt + 4 * kq, 16 * (nt0 + ni) + col, fmaxf(acc[0][ni][0], 0.f) * osc, fmaxf(acc[0][ni][1], 0.f) * osc,
                  fmaxf(acc[0][ni][2], 0.f) * osc, fmaxf(acc[0][ni][3], 0.f) * osc);
  return nxt;
}
// last layer: m-tile mt over all four n-tiles, max over each centre's U / 16 tiles and 16 columns, ReLU, one value per row
// STAGED (the single-tile kernels): the pooled values are not stored here.  A workgroup walks RUNS of consecutive tiles,
// i.e. 8 consecutive centres of a cloud; the pooled value of (row, centre s of the run) goes to stage[row][s] in LDS and,
// at the end of the run, all threads write the rows' 32-byte runs (sa3_flush) -- where the unstaged form wrote every (row,
// centre) as a 4-byte store of its own into its own 32-byte sector (268 MB of HBM writes per launch at SSG-SA2 for a
// 33.5 MB tensor).  LDS, not registers, carries the run: values kept in registers across tiles were spilled to scratch, and
// a scratch reload queues behind the next tile's gather in the in-order vmcnt (measured: 1.02 -> 1.26 ms).
constexpr int kSaRun = 8;   // centres per staged run
template <class FIRST, bool STAGED = false>
__device__ __forceinline__ void sa3_last(const Ctx &c, const SaArgs &a, int l, int mt, const float *src, int j0, float *outb,
                                         const FIRST &first, float bsc, float osc, float *stage = nullptr, int slot0 = 0) {
  const int col = c.lane & 15, kq = c.lane >> 4;
  f32x4 acc[1][4];
  const f32x4 bv = *reinterpret_cast<const f32x4 *>(a.weights + a.b_off[l] + 16 * mt + 4 * kq) * bsc;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[0][ni] = bv;
  sa3_gemm<4, FIRST>(c, a.weights + a.w_off[l], a.cin_pad[l] >> 5, mt, 0, src, acc, first);
  const int tpc = a.u >> 4;   // n-tiles per centre: 1, 2 or 4
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float m[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) m[ni] = acc[0][ni][r];
    if (tpc >= 2) { m[0] = fmaxf(m[0], m[1]); m[2] = fmaxf(m[2], m[3]); }
    if (tpc >= 4) m[0] = fmaxf(m[0], m[2]);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      if (ni % tpc) continue;  // wave uniform
      const float v = fmaxf(row16_max(m[ni]), 0.f) * osc;
      const int jj = ni / tpc;
      if constexpr (STAGED) {
        if (col == 0 && j0 + jj < a.m) ((lds_f *)stage)[(16 * mt + 4 * kq + r) * kSaRun + slot0 + jj] = v;
      } else {
        if (col == 0 && j0 + jj < a.m) outb[(size_t)(16 * mt + 4 * kq + r) * a.m + j0 + jj] = v;
      }
    }
  }
}
// the staged run -> out[b][row][jbase .. jbase + count) for every row of the last layer: thread = (row, half of the run)
__device__ __forceinline__ void sa3_flush(const SaArgs &a, const float *stage, int tid, int b, int jbase, int count) {
  const int rows = a.cout[a.n_layers - 1];
  for (int i = tid; i < 2 * rows; i += 512) {
    const int row = i >> 1, h4 = 4 * (i & 1), left = count - h4;
    if (left <= 0) continue;
    const f32x4 v = *reinterpret_cast<const lds_f4 *>((const lds_f *)stage + row * kSaRun + h4);
    float *o = a.out + ((size_t)b * rows + row) * a.m + jbase + h4;
    if (left >= 4 && (((size_t)o & 15) == 0)) *reinterpret_cast<f32x4 *>(o) = v;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < left) o[e] = v[e];
    }
  }
}

// One layer of the multi-tile form over all `sub` tiles of a workgroup pass: the m-tile's weight fragments (KB blocks x 3
// planes) are requested ONCE and stay in registers while the tiles' planes stream through -- per tile only LDS reads,
// MFMAs and the epilogue remain (through gemm1_pl every tile paid the fragments' round trip again: latency bound at 24-96
// MFMAs per call).  LAST: max over the neighbours instead of the plane stores.
template <int KB, int NT, bool LAST>
__device__ __forceinline__ void sa3_layer_multi(const Ctx &c, const SaArgs &a, int l, int mt, int nt0, int sub, int per,
                                                int src_off, int dst_off, int T, int tiles_per_cloud, int total_tiles,
                                                float bsc, float osc) {
  const int col = c.lane & 15, kq = c.lane >> 4, g = kq;
  const WStream wv(a.weights + a.w_off[l], c.lane);
  u32x4 af[KB][kSplit];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int pl = 0; pl < kSplit; ++pl) af[kb][pl] = wv.raw_at((mt * KB + kb) * kFragBytes, pl * 1024);
  const f32x4 bv = *reinterpret_cast<const f32x4 *>(a.weights + a.b_off[l] + 16 * mt + 4 * kq) * bsc;
  const int cpt = 64 / a.u, tpc = a.u >> 4;
  for (int st = 0; st < sub; ++st) {
    const lds_u4 *pl3 = (const lds_u4 *)(c.lds + st * per + src_off) + g * 64 + 16 * nt0 + col;
    f32x4 acc[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[ni] = bv;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      u32x4 bs[NT][kSplit];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int pl = 0; pl < kSplit; ++pl) bs[ni][pl] = pl3[(kb * kSplit + pl) * 256 + 16 * ni];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) acc[ni] = mfma_split(af[kb], bs[ni], acc[ni]);
    }
    if constexpr (!LAST) {
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        store_planes4(c.lds + st * per + dst_off, 16 * mt + 4 * kq, 16 * (nt0 + ni) + col, fmaxf(acc[ni][0], 0.f) * osc,
                      fmaxf(acc[ni][1], 0.f) * osc, fmaxf(acc[ni][2], 0.f) * osc, fmaxf(acc[ni][3], 0.f) * osc);
    } else {
      static_assert(!LAST || NT == 4, "the max runs over all four n-tiles of a tile");
      const int t = T * sub + st;
      if (t < total_tiles) {   // wave uniform
        const int b = t / tiles_per_cloud, j0 = (t - b * tiles_per_cloud) * cpt;
        float *outb = a.out + (size_t)b * a.cout[l] * a.m;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m[4];
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) m[ni] = acc[ni < NT ? ni : 0][r];
          if (tpc >= 2) { m[0] = fmaxf(m[0], m[1]); m[2] = fmaxf(m[2], m[3]); }
          if (tpc >= 4) m[0] = fmaxf(m[0], m[2]);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            if (ni % tpc) continue;  // wave uniform
            const float v = fmaxf(row16_max(m[ni]), 0.f) * osc;
            const int jj = ni / tpc;
            if (col == 0 && j0 + jj < a.m) outb[(size_t)(16 * mt + 4 * kq + r) * a.m + j0 + jj] = v;
          }
        }
      }
    }
  }
}
template <int NT, bool LAST>
__device__ __forceinline__ void sa3_layer_multi_kb(const Ctx &c, const SaArgs &a, int l, int mt, int nt0, int sub, int per,
                                                   int src_off, int dst_off, int T, int tiles_per_cloud, int total_tiles,
                                                   float bsc, float osc) {
  switch (a.cin_pad[l] >> 5) {
    case 1: sa3_layer_multi<1, NT, LAST>(c, a, l, mt, nt0, sub, per, src_off, dst_off, T, tiles_per_cloud, total_tiles, bsc, osc); break;
    case 2: sa3_layer_multi<2, NT, LAST>(c, a, l, mt, nt0, sub, per, src_off, dst_off, T, tiles_per_cloud, total_tiles, bsc, osc); break;
    default: sa3_layer_multi<4, NT, LAST>(c, a, l, mt, nt0, sub, per, src_off, dst_off, T, tiles_per_cloud, total_tiles, bsc, osc); break;
  }
}

// SUBMAX > 1: narrow nets (SSG SA1: 3 -> 64 -> 64 -> 128 over 512 centres per cloud) have 1.3 k cycles of MFMAs per
// 64-column tile against ~13 k of per-tile cost (four barriers, three cold layer starts, the gather's round trip): a
// workgroup then takes `sub` consecutive tiles at once -- their planes side by side in LDS, every layer swept over all of
// them between two barriers, the weight fragments of the later ones coming from L1.  QUADS: row quads a gather thread
// holds per tile (9 covers 288 input rows; the multi-tile form takes 32-row inputs: one quad).
// PRE: the module's first layer is not a GEMM here.  W1 [x - c; f] = W1a (x - c) + W1b f, and W1b f + b1 depends on the
// POINT only: the caller computes it once per cloud (a.pre), the gather threads fetch a neighbour's 4 rows of it instead of
// 4 feature rows, add the three coordinate products and apply the ReLU -- the tile that goes into LDS is the first
// layer's OUTPUT.  One k-loop, one plane-writing epilogue and one barrier per tile less, 29 % fewer MFMAs at SSG-SA2.
// (The second launch bound is waves per SIMD: 4 = two co-resident workgroups, i.e. 128 registers.  The hoisted form with
// up to four row quads per gather thread fits them; the general one holds nine quads and runs one workgroup per CU.)
template <int SUBMAX, int QUADS, bool PRE = false>
__global__ __launch_bounds__(512, (PRE && QUADS <= 4) ? 4 : 2) void sa_mlp3_kernel(const SaArgs a, int blocks_a, int blocks_b, int sub,
                                                         int tiles_per_cloud, int total_tiles) {
  extern __shared__ float lds[];
  Ctx c{a.weights, lds, (int)threadIdx.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), (int)threadIdx.x & 63,
        4};
  const int cpt = 64 / a.u;  // centres per tile
  const int per = (blocks_a + blocks_b) * kSaBlockFloats;   // floats of one tile's two plane regions
  const int w = c.wave, col = c.lane, qg = c.wave;   // gather: thread = (column, row-quad group)
  const int nquads = a.cin_pad[0] >> 2;
  const int supers = (total_tiles + sub - 1) / sub;
  float gv[SUBMAX][QUADS][4];
  float dxyz[SUBMAX][PRE ? 4 : 1];   // PRE: the column's x - c (3) and its live mask
  // The neighbour index of a column is requested a tile ahead of the gather that dereferences it (idx_request at the end
  // of the previous gather_load): read where it is used, every tile began with an exposed round trip for the index in
  // front of the gather's own.
  int id_pf[SUBMAX];
  auto idx_request = [&](int T) {
#pragma unroll
    for (int st = 0; st < SUBMAX; ++st) {
      const int t0 = T * sub + (st < sub ? st : 0);
      const int t = t0 < total_tiles ? t0 : total_tiles - 1;
      const int b = t / tiles_per_cloud, tile = t - b * tiles_per_cloud, j0 = tile * cpt, jj = col / a.u;
      const bool live = j0 + jj < a.m;
      id_pf[st] = (a.idx + ((size_t)b * a.m + j0) * a.u)[live ? col : 0];
    }
  };
  auto gather_load = [&](int T) {   // idx_request(T) went before
#pragma unroll
    for (int st = 0; st < SUBMAX; ++st) {
      const int t0 = T * sub + (st < sub ? st : 0);
      const int t = t0 < total_tiles ? t0 : total_tiles - 1;   // clamped: every load stays unconditional
      const int b = t / tiles_per_cloud, tile = t - b * tiles_per_cloud, j0 = tile * cpt, jj = col / a.u;
      const bool live = j0 + jj < a.m;
      const float *pts = a.points + (size_t)b * 3 * a.n, *ctr = a.centers + (size_t)b * 3 * a.m;
      const float *feat = a.feat ? a.feat + (size_t)b * a.c * a.n : a.points;
      const int id = live ? id_pf[st] : 0;
      const int jc = live ? j0 + jj : 0, cmax = a.c > 0 ? a.c - 1 : 0;
      if constexpr (PRE) {
        // pre is POINT-major, [b][n][c1]: a neighbour's rows are one run of c1 floats, a thread's row quad one 16-byte load
        // (channel-major, the 4-byte gathers of a tile were 8192 cache-line requests: the texture addresser, not the
        // matrix pipe, bounded the kernel -- a layer less changed nothing)
        const f32x4 *prow = reinterpret_cast<const f32x4 *>(a.pre + (a.pre_bcast ? (size_t)0 : ((size_t)b * a.n + id) * a.c1));
#pragma unroll
        for (int e = 0; e < 3; ++e) dxyz[st][e] = pts[e * a.n + id] - ctr[e * a.m + jc];
        dxyz[st][3] = live ? 1.0f : 0.0f;
        const int qmax = (a.c1 >> 2) - 1;
#pragma unroll
        for (int i = 0; i < QUADS; ++i) {
          const int rq = qg + 8 * i;
          const f32x4 v4 = prow[rq < qmax ? rq : qmax];
#pragma unroll
          for (int e = 0; e < 4; ++e) gv[st][i][e] = v4[e];
        }
        continue;
      }
#pragma unroll
      for (int i = 0; i < QUADS; ++i) {
        const int rq = qg + 8 * i;   // rows 4 rq .. 4 rq + 3: [x y z f0] for quad 0, f[4 rq - 3 ..] after it
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ch = 4 * rq + e;
          float v;
          if (ch < 3) v = pts[ch * a.n + id] - ctr[ch * a.m + jc];
          else { const int f = ch - 3; v = feat[(size_t)(f < cmax ? f : cmax) * a.n + id]; v = f < a.c ? v : 0.f; }
          gv[st][i][e] = live ? v : 0.f;
        }
      }
    }
  };
  // PRE: gv holds the neighbours' rows of W1b f + b1; add W1a (x - c), ReLU -> the first layer's output (dead columns and
  // rows beyond c1: zero).  W1a's rows are wave uniform (a wave's threads share their row quads).
  auto gather_finish = [&]() {
    if constexpr (PRE) {
      const f32x4 *wa = reinterpret_cast<const f32x4 *>(a.weights + a.wa_off);
#pragma unroll
      for (int i = 0; i < QUADS; ++i) {
        const int rq = qg + 8 * i;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 4 * rq + e;
          const f32x4 w4 = wa[row < a.c1 ? row : 0];
#pragma unroll
          for (int st = 0; st < SUBMAX; ++st) {
            float h = gv[st][i][e];
            h = __builtin_fmaf(w4[0], dxyz[st][0], h);
            h = __builtin_fmaf(w4[1], dxyz[st][1], h);
            h = __builtin_fmaf(w4[2], dxyz[st][2], h);
            gv[st][i][e] = row < a.c1 ? fmaxf(h, 0.f) * dxyz[st][3] : 0.f;
          }
        }
      }
    }
  };
  // Range scale of the gathered tile(s) (range_pow2): every wave publishes the largest magnitude it holds in front of a
  // barrier the tile needs anyway, all read the eight words behind it.  m_in / s_in: of the tile(s) about to be stored.
  float *rng = lds + (size_t)sub * per;   // [8], behind the planes (the launcher adds the room)
  float m_in = 0.f, s_in = 1.f;
  auto range_publish = [&]() {
    float mx = 0.f;
#pragma unroll
    for (int st = 0; st < SUBMAX; ++st)
#pragma unroll
      for (int i = 0; i < QUADS; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(gv[st][i][e]));
    mx = half_max(row_pair_max(row16_max(mx)));
    if (c.lane == 0) rng[c.wave] = mx;
  };
  auto range_read = [&]() {
    const f32x4 r0 = *reinterpret_cast<const f32x4 *>(rng), r1 = *reinterpret_cast<const f32x4 *>(rng + 4);
    const float mx = fmaxf(fmaxf(fmaxf(r0[0], r0[1]), fmaxf(r0[2], r0[3])), fmaxf(fmaxf(r1[0], r1[1]), fmaxf(r1[2], r1[3])));
    m_in = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(mx)));
    s_in = range_pow2(m_in);
  };
  auto gather_store = [&]() {
    const float inv = pow2_inv(s_in);
#pragma unroll
    for (int st = 0; st < SUBMAX; ++st) {
      if (st < sub) {
#pragma unroll
        for (int i = 0; i < QUADS; ++i) {
          const int rq = qg + 8 * i;
          if (rq < nquads)
            store_planes4(lds + st * per, 4 * rq, col, gv[st][i][0] * inv, gv[st][i][1] * inv, gv[st][i][2] * inv, gv[st][i][3] * inv);
        }
      }
    }
  };
  Frag3 frag;   // block-0 fragments of the wave's first m-tile of the NEXT layer to run
  // The request for the next layer's first fragments sits behind this layer's (first) k-loop, in front of its stores: in
  // flight under the epilogue and the barrier.  Straight-line code: the fragments travel by value.
  auto hidden = [&](int l, bool a_to_b, float bsc, float osc) {
    const int mtiles = a.cout[l] >> 4;
    Ctx cl = c;
    asm volatile("" : "+v"(cl.tid), "+v"(cl.lane));
    if constexpr (SUBMAX > 1) {   // weights once per layer, the tiles stream through (sa3_layer_multi)
      const int so = a_to_b ? 0 : blocks_a * kSaBlockFloats, dof = a_to_b ? blocks_a * kSaBlockFloats : 0;
      if (mtiles >= 8) {
        for (int p = 0; p < (mtiles >> 3); ++p) sa3_layer_multi_kb<4, false>(cl, a, l, w + 8 * p, 0, sub, per, so, dof, 0, 1, 0, bsc, osc);
      } else if (mtiles == 4) sa3_layer_multi_kb<2, false>(cl, a, l, w & 3, 2 * (w >> 2), sub, per, so, dof, 0, 1, 0, bsc, osc);
      else sa3_layer_multi_kb<1, false>(cl, a, l, w & 1, w >> 1, sub, per, so, dof, 0, 1, 0, bsc, osc);
      return;
    }
    const Frag3 cur = frag;
    for (int st = 0; st < sub; ++st) {
      const float *src = lds + st * per + (a_to_b ? 0 : blocks_a * kSaBlockFloats);
      float *dst = lds + st * per + (a_to_b ? blocks_a * kSaBlockFloats : 0);
      if (st == 0) {
        if (mtiles == 8) frag = sa3_hidden<4, Frag3, true>(cl, a, l, w, 0, src, dst, cur, bsc, osc);
        else if (mtiles == 16) {
          sa3_hidden<4, Frag3, false>(cl, a, l, w, 0, src, dst, cur, bsc, osc);
          frag = sa3_hidden<4, NoFirst, true>(cl, a, l, w + 8, 0, src, dst, NoFirst(), bsc, osc);
        } else if (mtiles == 4) frag = sa3_hidden<2, Frag3, true>(cl, a, l, w & 3, 2 * (w >> 2), src, dst, cur, bsc, osc);
        else frag = sa3_hidden<1, Frag3, true>(cl, a, l, w & 1, w >> 1, src, dst, cur, bsc, osc);
      } else if constexpr (SUBMAX > 1) {
        if (mtiles == 8) sa3_hidden<4, NoFirst, false>(cl, a, l, w, 0, src, dst, NoFirst(), bsc, osc);
        else if (mtiles == 16) {
          sa3_hidden<4, NoFirst, false>(cl, a, l, w, 0, src, dst, NoFirst(), bsc, osc);
          sa3_hidden<4, NoFirst, false>(cl, a, l, w + 8, 0, src, dst, NoFirst(), bsc, osc);
        } else if (mtiles == 4) sa3_hidden<2, NoFirst, false>(cl, a, l, w & 3, 2 * (w >> 2), src, dst, NoFirst(), bsc, osc);
        else sa3_hidden<1, NoFirst, false>(cl, a, l, w & 1, w >> 1, src, dst, NoFirst(), bsc, osc);
      }
    }
  };
  // Tile order.  SUBMAX > 1: workgroup w takes super-tiles w, w + grid, ...  SUBMAX == 1: RUNS of consecutive tiles = 8
  // consecutive centres of a cloud, so that the pooled rows leave as 32-byte runs (SaOutStage); the runs are dealt
  // w, w + grid, ... in an order that gives the workgroups of one XCD (blockIdx % 8: the dispatcher's round robin)
  // neighbouring runs: at any time the chip works on ~32 clouds and an XCD on four of them, whose features stay in its L2.
  // (Measured and dropped: one contiguous range of 64 tiles per workgroup, 16-centre runs -- every workgroup on a cloud of
  // its own, 256 clouds live at once: 1.02 -> 1.31 ms at SSG-SA2, the gathers miss L2.)
  constexpr bool kRuns = SUBMAX == 1;
  const int grid = gridDim.x;
  const int run = !kRuns ? 1 : (supers < 8 * grid ? 1 : (cpt >= kSaRun ? 1 : kSaRun / cpt));   // small launches: a tile per workgroup at a time
  const int w8 = !kRuns ? (int)blockIdx.x
                        : ((grid & 7) == 0 ? ((int)blockIdx.x & 7) * (grid >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x);
  auto tile_of = [&](int q) { return (w8 + (q / run) * grid) * run + q % run; };   // this workgroup's q-th (super-)tile
  int q = 0, T = tile_of(0);
  if (T >= supers) return;   // (whole workgroup: no barrier has been reached yet)
  float *stage = rng + 16;   // [rows of the last layer][kSaRun] (kRuns; the launcher adds the room)
  int st_count = 0, st_b = 0, st_jbase = 0;
  idx_request(T);
  gather_load(T);
  {
    const int T1 = tile_of(1);
    idx_request(T1 < supers ? T1 : T);
  }
  frag = sa3_request(c, a, 0);
  gather_finish();
  if (a.ranged) {
    range_publish();
    __syncthreads();
    range_read();
  }
  gather_store();
  __syncthreads();
  for (; T < supers; T = tile_of(++q)) {
    bool a_to_b = true;
    // scales of this tile's planes, layer by layer: the input's is measured, a hidden layer's follows from the bound
    // |out| <= gain_r * max |in| + gain_b (true units)
    float bnd = m_in, s_cur = s_in;
    for (int l = 0; l + 1 < a.n_layers; ++l) {
      bnd = a.gain_r[l] * bnd + a.gain_b[l];
      const float s_nxt = a.ranged ? range_pow2(bnd) : 1.0f;
      hidden(l, a_to_b, pow2_inv(s_cur), s_cur * pow2_inv(s_nxt));
      s_cur = s_nxt;
      __syncthreads();
      a_to_b = !a_to_b;
    }
    const int Tq = tile_of(q + 1), Tn = Tq < supers ? Tq : T;
    gather_load(Tn);
    {
      const int T2 = tile_of(q + 2);
      idx_request(T2 < supers ? T2 : Tn);   // for the gather of the tile after next
    }
    {
      const int l = a.n_layers - 1, mtiles = a.cout[l] >> 4;
      const float bsc = pow2_inv(s_cur), osc = s_cur;
      Ctx cl = c;
      asm volatile("" : "+v"(cl.tid), "+v"(cl.lane));
      if constexpr (SUBMAX > 1) {
        const int so = a_to_b ? 0 : blocks_a * kSaBlockFloats;
        for (int mt = w; mt < mtiles; mt += 8)
          sa3_layer_multi_kb<4, true>(cl, a, l, mt, 0, sub, per, so, 0, T, tiles_per_cloud, total_tiles, bsc, osc);
      }
      const Frag3 cur = frag;
      for (int st = 0; st < (SUBMAX > 1 ? 0 : sub); ++st) {
        const int t = T * sub + st;
        if (t >= total_tiles) break;   // wave uniform
        const int b = t / tiles_per_cloud, j0 = (t - b * tiles_per_cloud) * cpt;
        float *outb = a.out + (size_t)b * a.cout[l] * a.m;
        const float *src = lds + st * per + (a_to_b ? 0 : blocks_a * kSaBlockFloats);
        if constexpr (kRuns) {
          const int live = a.m - j0 < cpt ? a.m - j0 : cpt;          // centres of this tile that exist
          if (st_count == 0) { st_b = b; st_jbase = j0; }
          if (w < mtiles) sa3_last<Frag3, true>(cl, a, l, w, src, j0, outb, cur, bsc, osc, stage, st_count);
          for (int mt = w + 8; mt < mtiles; mt += 8) sa3_last<NoFirst, true>(cl, a, l, mt, src, j0, outb, NoFirst(), bsc, osc, stage, st_count);
          st_count += live;
        } else {
        if (st == 0) {
          if (w < mtiles) sa3_last<Frag3>(cl, a, l, w, src, j0, outb, cur, bsc, osc);
        } else {
          if (w < mtiles) sa3_last<NoFirst>(cl, a, l, w, src, j0, outb, NoFirst(), bsc, osc);
        }
        for (int mt = w + 8; mt < mtiles; mt += 8) sa3_last<NoFirst>(cl, a, l, mt, src, j0, outb, NoFirst(), bsc, osc);
        }
      }
      frag = sa3_request(c, a, 0);   // the next tile's first layer
    }
    gather_finish();                 // the next tile's gathered values have long landed
    if (a.ranged) range_publish();
    __syncthreads();  // the last layer may have been reading region A
    if constexpr (kRuns) {
      // the run ends here unless the next tile continues it (same cloud, the next centres, room in the stage)
      bool more = Tq < supers;
      if (more) {
        const int bn = Tq / tiles_per_cloud, jn = (Tq - bn * tiles_per_cloud) * cpt;
        const int liven = a.m - jn < cpt ? a.m - jn : cpt;
        more = bn == st_b && jn == st_jbase + st_count && st_count + liven <= kSaRun;
      }
      if (!more) {
        sa3_flush(a, stage, c.tid, st_b, st_jbase, st_count);
        st_count = 0;
      }
    }
    if (a.ranged) range_read();
    gather_store();
    __syncthreads();
  }
}

using gldm_dev::cu_count;

// What launch_sa3 makes of a layer plan: the two plane regions and the bytes of one tile.
struct Sa3Plan {
  int blocks_a, blocks_b;   // 32-row plane blocks of regions A (the gathered rows, odd hidden layers) and B (even hidden layers)
  size_t tile_bytes;        // one tile's two plane regions
  size_t behind_bytes;      // behind the planes: the eight range words and (single-tile kernels) the staged output rows of a run
};

// The shape part of launch_sa3: a pure function of the sizes and the host tables (no device pointer, no HIP call, no CU
// count).  pre: the hoisted form (c = 0, cin_pad[0] = rows of pre).  GLDM_OK and the plan, or the launch's status.
int plan_sa3(bool pre, int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout, Sa3Plan &p) {
  if (n_layers < 1 || n_layers > 4 || !(u == 16 || u == 32 || u == 64)) return GLDM_ERR_UNSUPPORTED;
  int blocks_a = 0, blocks_b = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int kb = cin_pad[l] >> 5, mt = cout[l] >> 4;
    if (cin_pad[l] <= 0 || (cin_pad[l] & 31) || !(kb <= 6 || kb == 8 || kb == 9) || cout[l] <= 0 || (cout[l] & 15)) return GLDM_ERR_UNSUPPORTED;
    if (l > 0 && cin_pad[l] != cout[l - 1]) return GLDM_ERR_INVALID_ARG;
    if (l + 1 < n_layers) {   // hidden layer: its output is the next layer's planes
      if ((cout[l] & 31) || !(mt == 2 || mt == 4 || mt == 8 || mt == 16)) return GLDM_ERR_UNSUPPORTED;
      int &blk = (l & 1) ? blocks_a : blocks_b;
      blk = blk > (cout[l] >> 5) ? blk : (cout[l] >> 5);
    }
  }
  if (!pre && (cin_pad[0] < 3 + c || cin_pad[0] > 32 * kSa3Quads)) return GLDM_ERR_UNSUPPORTED;
  if (pre && cin_pad[0] > 256) return GLDM_ERR_UNSUPPORTED;
  blocks_a = blocks_a > (cin_pad[0] >> 5) ? blocks_a : (cin_pad[0] >> 5);
  const size_t tile_bytes = (size_t)(blocks_a + blocks_b) * kSaBlockFloats * sizeof(float);
  const size_t behind_bytes = 64 + (size_t)cout[n_layers - 1] * kSaRun * sizeof(float);
  if (tile_bytes + behind_bytes > 160 * 1024) return GLDM_ERR_UNSUPPORTED;
  p = Sa3Plan{blocks_a, blocks_b, tile_bytes, behind_bytes};
  return GLDM_OK;
}

// pre != nullptr: the first layer hoisted (sa_mlp3_kernel<.., PRE>): `features` unused, c = 0, cin_pad[0] = rows of pre
int launch_sa3(const float *points, const float *centers, const float *features, const float *pre, int wa_off, int pre_bcast,
               const int32_t *idx, const float *weights, int b, int c, int n, int m, int u,
               int n_layers, const int32_t *cin_pad, const int32_t *cout, const int32_t *w3_off,
               const int32_t *b_off, const float *range_gain, float *out, gldm_stream_t stream) {
  if (!points || !centers || !idx || !weights || !out || !cin_pad || !cout || !w3_off || !b_off || b <= 0 || c < 0 ||
      n <= 0 || m <= 0 || u <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (c > 0 && !features) return GLDM_ERR_INVALID_ARG;
  if (pre && (c != 0 || wa_off < 0 || (wa_off & 3))) return GLDM_ERR_INVALID_ARG;
  Sa3Plan p{};
  const int rc = plan_sa3(pre != nullptr, c, u, n_layers, cin_pad, cout, p);
  if (rc != GLDM_OK) return rc;
  SaArgs a{};
  a.points = points; a.centers = centers; a.feat = c > 0 ? features : nullptr; a.idx = idx; a.weights = weights;
  a.out = out; a.c = c; a.n = n; a.m = m; a.u = u; a.n_layers = n_layers;
  a.ranged = range_gain != nullptr;
  a.pre = pre; a.c1 = pre ? cin_pad[0] : 0; a.wa_off = wa_off; a.pre_bcast = pre_bcast ? 1 : 0;
  for (int l = 0; l < n_layers; ++l) {
    a.cin_pad[l] = cin_pad[l]; a.cout[l] = cout[l]; a.w_off[l] = w3_off[l]; a.b_off[l] = b_off[l];
    if (!range_gain) continue;
    a.gain_r[l] = range_gain[2 * l];
    a.gain_b[l] = range_gain[2 * l + 1];
    if (!(a.gain_r[l] >= 0.f) || !(a.gain_b[l] >= 0.f)) return GLDM_ERR_INVALID_ARG;
  }
  const int blocks_a = p.blocks_a, blocks_b = p.blocks_b;
  const size_t tile_bytes = p.tile_bytes, kRngBytes = p.behind_bytes;
  const int cpt = 64 / u, tpc = (m + cpt - 1) / cpt, total = tpc * b;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // narrow nets (32-row inputs, every K in {32, 64, 128}): the multi-tile kernel -- the layer's weights once per
  // workgroup pass, `sub` tiles' planes side by side in LDS (SSG SA1: three 48 KiB tiles, 2.52 -> 2.07 ms).  Two
  // co-resident workgroups of one tile each (the kernel fits 128 registers) measured slower: 2.40 ms.
  // one or two row quads per gather thread; the hoisted form (pre): the multi-tile kernel with two tiles per pass
  bool kb_ok = cin_pad[0] == 32 || cin_pad[0] == 64;
  for (int l = 0; l < n_layers; ++l) kb_ok = kb_ok && (cin_pad[l] == 32 || cin_pad[l] == 64 || cin_pad[l] == 128);
  int sub = kb_ok ? (int)(((size_t)160 * 1024 - kRngBytes) / tile_bytes) : 1;
  if (sub > 4) sub = 4;
  // two workgroups of two tiles each rather than one of four where LDS allows (the kernel fits 128 registers): the phases of
  // one overlap the other's (SSG-SA1 at 256 clouds: 1.55 -> 1.47 ms)
  if (sub > 2 && (tile_bytes * 2 + kRngBytes) * 2 <= (size_t)160 * 1024) sub = 2;
  if (pre && sub > 2) sub = 2;
  while (sub > 1 && (total + sub - 1) / sub < 2 * cu_count()) --sub;
  const dim3 t(512);
  constexpr int kLim = 160 * 1024;   // every kernel's dynamic-LDS limit: the CU's LDS
  using gldm_dev::launch_dynamic_lds;
  if (sub > 1) {
    const int supers = (total + sub - 1) / sub;
    const int per_cu_m = (tile_bytes * sub + kRngBytes) * 2 <= (size_t)160 * 1024 ? 2 : 1;
    const dim3 g(supers < cu_count() * per_cu_m ? supers : cu_count() * per_cu_m);
    const size_t lds = tile_bytes * sub + kRngBytes;
    if (pre) launch_dynamic_lds<sa_mlp3_kernel<2, 2, true>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, sub, tpc, total);
    else if (cin_pad[0] == 32) launch_dynamic_lds<sa_mlp3_kernel<4, 1>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, sub, tpc, total);
    else launch_dynamic_lds<sa_mlp3_kernel<4, 2>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, sub, tpc, total);
  } else {
    const int per_cu = (tile_bytes + kRngBytes) * 2 <= 160 * 1024 ? 2 : 1;
    const dim3 g(cu_count() * per_cu < total ? cu_count() * per_cu : total);
    const size_t lds = tile_bytes + kRngBytes;
    if (pre && cin_pad[0] <= 128) launch_dynamic_lds<sa_mlp3_kernel<1, 4, true>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, 1, tpc, total);
    else if (pre) launch_dynamic_lds<sa_mlp3_kernel<1, 8, true>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, 1, tpc, total);
    else launch_dynamic_lds<sa_mlp3_kernel<1, kSa3Quads>>(g, t, kLim, lds, s, a, blocks_a, blocks_b, 1, tpc, total);
  }
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
}  // namespace

GLDM_API int gldm_sa_mlp_forward_f16x2(const float *points, const float *centers, const float *features,
                                        const int32_t *idx, const float *weights, int b, int c, int n, int m, int u,
                                        int n_layers, const int32_t *cin_pad, const int32_t *cout, const int32_t *w3_off,
                                        const int32_t *b_off, const float *range_gain, float *out, gldm_stream_t stream) {
  return launch_sa3(points, centers, features, nullptr, 0, 0, idx, weights, b, c, n, m, u, n_layers, cin_pad, cout, w3_off, b_off,
                    range_gain, out, stream);
}

GLDM_API int gldm_sa_mlp_forward_f16x2_pre(const float *points, const float *centers, const float *pre, int pre_broadcast,
                                            const int32_t *idx, const float *weights, int wa_off, int b, int n, int m, int u, int n_layers,
                                            const int32_t *cin_pad, const int32_t *cout, const int32_t *w3_off,
                                            const int32_t *b_off, const float *range_gain, float *out, gldm_stream_t stream) {
  if (!pre) return GLDM_ERR_INVALID_ARG;
  return launch_sa3(points, centers, nullptr, pre, wa_off, pre_broadcast, idx, weights, b, 0, n, m, u, n_layers, cin_pad, cout, w3_off,
                    b_off, range_gain, out, stream);
}

namespace {
// What gldm_sa_mlp_forward makes of a layer plan: the 128-column kernel where it fits, else the 64-column one.
struct SaF32Plan {
  bool wide;          // 128-column tiles (sa_mlp2_kernel)
  int rows_a;         // its region A
  size_t lds_bytes;   // its two regions
};

// The shape part of gldm_sa_mlp_forward: a pure function of the sizes and the host tables, as plan_sa3.
int plan_sa_f32(int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout, SaF32Plan &p) {
  if (n_layers < 1 || n_layers > 4) return GLDM_ERR_UNSUPPORTED;
  if (u > 64 || (64 % u) != 0) return GLDM_ERR_UNSUPPORTED;
  for (int l = 0; l < n_layers; ++l) {
    const int mt = (cout[l] + 15) >> 4;
    if (cin_pad[l] <= 0 || (cin_pad[l] & 15) || cin_pad[l] > kMaxC || cout[l] > kMaxC ||
        !(mt == 1 || mt == 2 || mt == 4 || mt == 8 || mt == 12 || mt == 16) || (cout[l] & 15))
      return GLDM_ERR_UNSUPPORTED;
    if (l > 0 && cin_pad[l] != cout[l - 1]) return GLDM_ERR_INVALID_ARG;
  }
  if (cin_pad[0] < 3 + c) return GLDM_ERR_INVALID_ARG;
  // 128-column tiles when the layer plan fits: widths 32 / 64 / 128 / 256 k, U a multiple of 16, both regions in LDS
  bool ok = (u == 16 || u == 32 || u == 64) && c <= 4 * kSaFly;
  int rows_a = cin_pad[0], rows_b = 0;
  for (int l = 0; l < n_layers && ok; ++l) {
    const int mt = cout[l] >> 4;
    ok = (mt == 2 || mt == 4 || (mt >= 8 && (mt & 7) == 0)) && (cin_pad[l] & 31) == 0;
    if (l + 1 < n_layers) {  // stored outputs: even layers -> B, odd layers -> A
      if (l & 1) rows_a = rows_a > cout[l] ? rows_a : cout[l];
      else rows_b = rows_b > cout[l] ? rows_b : cout[l];
    } else if (ok) {  // the max runs on one wave's n-tiles: a centre's U / 16 tiles must not straddle two waves
      const int nt = mt >= 8 ? 8 : (mt == 4 ? 4 : 2);
      ok = (u >> 4) <= nt;
    }
  }
  const size_t lds2 = (size_t)(rows_a + rows_b) * 128 * sizeof(float);
  p = SaF32Plan{ok && lds2 <= 160 * 1024, rows_a, lds2};
  return GLDM_OK;
}
}  // namespace

GLDM_API int gldm_sa_mlp_supported(int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout) {
  if (!cin_pad || !cout || c < 0 || u <= 0) return GLDM_ERR_INVALID_ARG;
  SaF32Plan p{};
  return plan_sa_f32(c, u, n_layers, cin_pad, cout, p);
}

GLDM_API long long gldm_sa_mlp_f16x2_lds_bytes(int pre, int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout,
                                                long long *plane_bytes) {
  if (!cin_pad || !cout || c < 0 || u <= 0 || (pre && c != 0)) return GLDM_ERR_INVALID_ARG;
  Sa3Plan p{};
  const int rc = plan_sa3(pre != 0, c, u, n_layers, cin_pad, cout, p);
  if (rc != GLDM_OK) return rc;
  if (plane_bytes) *plane_bytes = (long long)p.tile_bytes;
  return (long long)(p.tile_bytes + p.behind_bytes);
}

GLDM_API int gldm_sa_mlp_forward(const float *points, const float *centers, const float *features,
                                 const int32_t *idx, const float *weights, int b, int c, int n, int m, int u,
                                 int n_layers, const int32_t *cin_pad, const int32_t *cout, const int32_t *w_off,
                                 const int32_t *b_off, float *out, gldm_stream_t stream) {
  if (!points || !centers || !idx || !weights || !out || !cin_pad || !cout || !w_off || !b_off || b <= 0 || c < 0 ||
      n <= 0 || m <= 0 || u <= 0)
    return GLDM_ERR_INVALID_ARG;
  if (c > 0 && !features) return GLDM_ERR_INVALID_ARG;
  SaF32Plan p{};
  const int rc = plan_sa_f32(c, u, n_layers, cin_pad, cout, p);
  if (rc != GLDM_OK) return rc;
  SaArgs a{};
  a.points = points; a.centers = centers; a.feat = c > 0 ? features : nullptr; a.idx = idx; a.weights = weights;
  a.out = out; a.c = c; a.n = n; a.m = m; a.u = u; a.n_layers = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    a.cin_pad[l] = cin_pad[l]; a.cout[l] = cout[l]; a.w_off[l] = w_off[l]; a.b_off[l] = b_off[l];
  }
#ifdef GLDM_DEBUG_KNOBS
  static const bool tile64 = getenv("GLDM_SA_TILE64") != nullptr;  // diagnostic builds: force the 64-column kernel
#else
  constexpr bool tile64 = false;  // the shipped library reads no environment
#endif
  if (p.wide && !tile64) {
    const int cpt2 = 128 / u, tpc = (m + cpt2 - 1) / cpt2, total = tpc * b;
    const int grid = total < cu_count() ? total : cu_count();
    gldm_dev::launch_dynamic_lds<sa_mlp2_kernel>(dim3(grid), dim3(512), 160 * 1024, p.lds_bytes, reinterpret_cast<hipStream_t>(stream),
                                                 a, p.rows_a, tpc, total);
    return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
  }
  const size_t lds_bytes = (size_t)(Geo<64>::kBufH + kMaxC * 64) * sizeof(float);
  const int cpt = 64 / u;
  gldm_dev::launch_dynamic_lds<sa_mlp_kernel>(dim3((m + cpt - 1) / cpt, b), dim3(Geo<64>::kThreads), (int)lds_bytes, lds_bytes,
                                              reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
