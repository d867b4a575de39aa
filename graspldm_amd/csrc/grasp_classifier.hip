// grasp_classifier.hip -- the two ends of PointsBasedGraspClassifier (grasp_ldm/models/grasp_classifier.py:13-143) around
// its PVCNN / PVCNN2 backbone.
//
//   gldm_grasp_scene   the network input of every (cloud, pose) scene in one pass: the gripper's control points placed at
//                      the pose and brought into the cloud's normalised frame (acronym_grasp_points.py:25-28,107,117),
//                      the label channel and the channel-first merge (grasp_classifier.py:71-80).
//   gldm_cls_head      the `classifier` Sequential + sigmoid on the backbone's features x [b, c, n]:
//                        logit_b = c0 + sum_n l_n (w2 . relu(W1' x_{b,n} + b1')),   c0 = lb + b2 sum_n l_n   (host, f64)
//                      W1', b1' = classifier.0 with its BatchNorm folded, w2 = classifier.2, l = classifier.3.
//
// Head structure.  A workgroup owns 64 points of one scene and 128 rows of W1' per pass (four waves, two 16-row tiles x
// four 16-point tiles each).  Per 32-channel block the 256 threads stage the [32][64] slab of x ONCE (coalesced rows of
// 64 points, the next slab's loads in flight while this one multiplies), split it into the two f16 planes in B-fragment
// order in LDS, and every wave reads whole fragments from there; the weights arrive as pre-packed A fragments (16-byte
// loads, L2 -> VGPR).  ReLU, the dot with w2 and the weight l_n run on the accumulators: neither [b, 128, n] nor
// [b, 1, n] exists.  Range: x is data, so the 64-point tile is split as x / s with s a power of two from the tile's
// largest magnitude over all channels (head_pow2: the tile's maximum always lands in [2^13, 2^14)), measured in a first
// pass over the tile and folded back on the accumulators.  exact_f32: the same walk with f32 slabs on v_mfma_f32_16x16x4_f32, no scale.
// Sum over points: rows inside a lane (fixed order), lanes 16 / 32 apart, the four waves, the 64 columns (fixed tree),
// one partial per workgroup in the workspace; a second launch adds a scene's partials in tile order.  No atomics, nothing
// waits on another workgroup: a scene's logit does not depend on its place in the batch, on b or on any chunking.
// Tail columns (n % 64) are staged as zeros and carry weight 0.
#include "mfma_prims.h"

namespace {

constexpr int kHeadCols = 64;      // points per workgroup
constexpr int kHeadRowsPass = 128; // rows of W1' per pass: 4 waves x 2 m-tiles
constexpr int kHeadFoldKb = 4;     // exact_f32: 32-deep K blocks per partial sum
constexpr int kHeadMaxRows = 512, kHeadMaxC = 2048, kHeadMaxN = 1 << 20;

inline bool head_shape_ok(int c, int rows, int n) {
  return c % 16 == 0 && c >= 16 && c <= kHeadMaxC && rows % 16 == 0 && rows >= 16 && rows <= kHeadMaxRows && n >= 1 && n <= kHeadMaxN;
}
inline long long head_tiles(int n) { return (n + kHeadCols - 1) / kHeadCols; }

// The tile's scale: ALWAYS the power of two that brings its largest magnitude m into [2^13, 2^14) -- range_pow2 leaves
// 2^-8 <= m < 2^14 unscaled (for the bits of kernels older than the scales), where the lo pieces of a tile of a few 1e-3
// are f16 subnormals and a logit loses 1e-5 of itself; nothing here has older bits to keep.  1 for an empty or non-finite tile.
__device__ __forceinline__ float head_pow2(float m) {
  int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - 127;
  if (e < -100 || e > 100) return 1.0f;
  e = e < -40 ? -40 : e;
  return __uint_as_float((unsigned)(e - 13 + 127) << 23);
}

// ---- scene assembly -----------------------------------------------------------------------------------------------------
// A thread per (scene, column): four stores, each coalesced along the columns.
__global__ __launch_bounds__(256) void grasp_scene_kernel(const float *__restrict__ pc, const float *__restrict__ H,
                                                          const float *__restrict__ grip, const float *__restrict__ pc_mean,
                                                          float shift, float scale, int G, int np, int ng, long long total,
                                                          float *__restrict__ x) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = np + ng;
  const long long s = i / n;
  const int j = (int)(i - s * n);
  const long long cloud = s / G;
  float v[3], label;
  if (j < np) {
    const float *p = pc + (cloud * np + j) * 3;
    v[0] = p[0], v[1] = p[1], v[2] = p[2];
    label = 0.f;
  } else {
    const float *h = H + s * 16, *g = grip + (size_t)(j - np) * 3;
    const float *m = pc_mean ? pc_mean + cloud * 3 : nullptr;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // the reference's own order (H @ [p; 1] as a k-ordered fma chain, the translation its last term, then the two
      // subtractions and ONE division): PVCNN2 selects points (FPS, ball queries), and a coordinate one ulp away from the
      // reference's can flip a selection and move the logit by 1e-4
      float a = h[4 * r] * g[0];
      a = __builtin_fmaf(h[4 * r + 1], g[1], a);
      a = __builtin_fmaf(h[4 * r + 2], g[2], a);
      a += h[4 * r + 3];
      if (m) a -= m[r];
      v[r] = (a - shift) / scale;
    }
    label = 1.f;
  }
  float *o = x + s * 4 * n + j;
  o[0] = v[0];
  o[n] = v[1];
  o[2 * (size_t)n] = v[2];
  o[3 * (size_t)n] = label;
}

// ---- head: GEMM + ReLU + w2 + l_n, one partial per (scene, 64-point tile) ---------------------------------------------
// w: !EX split-f16 A fragments [rows/16][kb32][plane][lane 64][8 f16] (K zero-padded to 32), EX f32 A fragments
// [rows/16][c/16][lane 64][4].  part [b][tiles].
template <bool EX>
__global__ __launch_bounds__(256) void cls_head_kernel(const float *__restrict__ x, const u32x4 *__restrict__ w,
                                                       const float *__restrict__ b1, const float *__restrict__ w2,
                                                       const float *__restrict__ l, int c, int rows, int n, int tiles,
                                                       float *__restrict__ part) {
  constexpr int MT = 2, NT = 4;
  // !EX: [plane][g][col] 16-byte entries; EX: [32 channels][64 cols] floats.  8 KiB either way.
  __shared__ u32x4 slab[2 * 4 * kHeadCols];
  __shared__ float red[4][kHeadCols];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, r16 = lane & 15;
  const int scene = blockIdx.x / tiles, tile = blockIdx.x - scene * tiles, n0 = tile * kHeadCols;
  const int sg = tid >> 6, scol = tid & 63;                      // staging role: channel octet, column
  const bool live = n0 + scol < n;
  const float *xs = x + (size_t)scene * c * n + n0 + (live ? scol : 0);
  const int kb32 = (c + 31) / 32, kb16 = c / 16, mtiles = rows / 16;

  // pass 1: the tile's largest magnitude (the staging roles' columns, every fourth channel per octet role)
  float scale = 1.f, inv = 1.f;
  if constexpr (!EX) {
    float m = 0.f;
#pragma unroll 8
    for (int ch = sg; ch < c; ch += 4) m = fmaxf(m, fabsf(xs[(size_t)ch * n]));
    m = live ? m : 0.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[0][wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    __syncthreads();
    scale = head_pow2(m);
    inv = pow2_inv(scale);
  }

  auto fetch = [&](int kb, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ch = 32 * kb + 8 * sg + j;
      const float t = xs[(size_t)min(ch, c - 1) * n];   // unconditional (address clamped): a branch around a load is waited for at the join
      v[j] = (live && ch < c) ? t * inv : 0.f;
    }
  };
  auto stage = [&](const float (&v)[8]) {
    if constexpr (EX) {
      float *sf = (float *)slab;
#pragma unroll
      for (int j = 0; j < 8; ++j) sf[(8 * sg + j) * kHeadCols + scol] = v[j];
    } else {
      u32x4 pl[kSplit];
      split_planes8(v, pl);
      slab[sg * kHeadCols + scol] = pl[0];
      slab[(4 + sg) * kHeadCols + scol] = pl[1];
    }
  };

  float colsum[NT] = {0.f, 0.f, 0.f, 0.f};   // this wave's rows of  w2 . relu(..)  per column, all passes
  for (int mt0 = 0; mt0 < mtiles; mt0 += kHeadRowsPass / 16) {
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    int mt[MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) mt[mi] = min(mt0 + MT * wave + mi, mtiles - 1);   // clamped for the loads, masked below

    // EX: folded into a total every kHeadFoldKb K blocks.  One f32 chain over c = 2048 is 512 dependent roundings at the
    // magnitude of the finished row: 1.6 times the bar on a logit whose terms cancel.  Folded: 32 steps and c / 128 totals.
    [[maybe_unused]] f32x4 total[EX ? MT : 1][EX ? NT : 1];
    if constexpr (EX) {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) total[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto fold = [&]() {
      if constexpr (EX) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) {
            total[mi][ni] += acc[mi][ni];
            acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    };

    float v[8];
    fetch(0, v);
    for (int kb = 0; kb < kb32; ++kb) {
      if (EX && kb && kb % kHeadFoldKb == 0) fold();
      stage(v);
      __syncthreads();
      if (kb + 1 < kb32) fetch(kb + 1, v);   // in flight while this slab multiplies
      if constexpr (EX) {
        const float *sf = (const float *)slab;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (2 * kb + h < kb16) {
            f32x4 a[MT];
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
              a[mi] = __builtin_bit_cast(f32x4, w[((size_t)mt[mi] * kb16 + 2 * kb + h) * 64 + lane]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int ni = 0; ni < NT; ++ni) {
                const float bv = sf[(16 * h + 4 * j + g) * kHeadCols + 16 * ni + r16];
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
                  acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][j], bv, acc[mi][ni], 0, 0, 0);
              }
          }
        }
      } else {
        u32x4 a[MT][kSplit], b[NT][kSplit];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int pl = 0; pl < kSplit; ++pl) a[mi][pl] = w[(((size_t)mt[mi] * kb32 + kb) * kSplit + pl) * 64 + lane];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
          for (int pl = 0; pl < kSplit; ++pl) b[ni][pl] = slab[(4 * pl + g) * kHeadCols + 16 * ni + r16];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = mfma_split(a[mi], b[ni], acc[mi][ni]);
      }
      __syncthreads();
    }
    if constexpr (EX) {
      fold();
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = total[mi][ni];
    }

    // epilogue on the accumulators: acc[mi][ni][r] = row 16 mt + 4 g + r, column 16 ni + r16
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      if (mt0 + MT * wave + mi < mtiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * mt[mi] + 4 * g + r;
          const float bias = b1[row], wr = w2[row];
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) {
            const float y = __builtin_fmaf(acc[mi][ni][r], scale, bias);
            colsum[ni] = __builtin_fmaf(wr, fmaxf(y, 0.f), colsum[ni]);
          }
        }
      }
    }
  }
  // rows of the other lane groups, then of the other waves
#pragma unroll
  for (int ni = 0; ni < NT; ++ni) {
    float s = colsum[ni];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0) red[wave][16 * ni + r16] = s;
  }
  __syncthreads();
  if (wave == 0) {
    float s = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    s = n0 + lane < n ? s * l[n0 + lane] : 0.f;
    s = wave_sum(s);
    if (lane == 0) part[(size_t)scene * tiles + tile] = s;
  }
}

// a thread per scene: its partials in tile order, the constant, the sigmoid
__global__ __launch_bounds__(256) void cls_head_finish_kernel(const float *__restrict__ part, int b, int tiles, float c0,
                                                              float *__restrict__ logit, float *__restrict__ prob) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= b) return;
  const float *p = part + (size_t)s * tiles;
  float a = 0.f;
  for (int t = 0; t < tiles; ++t) a += p[t];
  a += c0;
  logit[s] = a;
  prob[s] = 1.0f / (1.0f + expf(-a));
}

}  // namespace

GLDM_API int gldm_grasp_scene(const float *pc, const float *H, const float *gripper, const float *pc_mean, float pc_shift,
                              float pc_scale, int bc, int g, int np, int ng, float *x, gldm_stream_t stream) {
  if (!pc || !H || !gripper || !x || bc <= 0 || g <= 0 || np <= 0 || ng <= 0) return GLDM_ERR_INVALID_ARG;
  if (!(pc_scale > 0.f) && !(pc_scale < 0.f)) return GLDM_ERR_INVALID_ARG;   // zero or NaN
  const long long total = (long long)bc * g * (np + ng);
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(grasp_scene_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pc, H,
                     gripper, pc_mean, pc_shift, pc_scale, g, np, ng, total, x);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API long long gldm_cls_head_workspace_bytes(int b, int c, int rows, int n) {
  if (b <= 0 || !head_shape_ok(c, rows, n)) return -1;
  return (4ll * b * head_tiles(n) + 255) / 256 * 256;
}

GLDM_API int gldm_cls_head(const float *x, const void *w1, const float *b1, const float *w2, const float *l, float c0, int b,
                           int c, int rows, int n, int exact_f32, void *workspace, long long workspace_bytes, float *logit,
                           float *prob, gldm_stream_t stream) {
  if (!x || !w1 || !b1 || !w2 || !l || !logit || !prob || b <= 0 || c <= 0 || rows <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (!head_shape_ok(c, rows, n)) return GLDM_ERR_UNSUPPORTED;
  const long long tiles = head_tiles(n);
  if (b * tiles > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  if (!workspace || ((size_t)w1 & 15) || ((size_t)workspace & 3)) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_cls_head_workspace_bytes(b, c, rows, n)) return GLDM_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float *part = (float *)workspace;
  if (exact_f32)
    hipLaunchKernelGGL(cls_head_kernel<true>, dim3((unsigned)(b * tiles)), dim3(256), 0, st, x, (const u32x4 *)w1, b1, w2, l, c,
                       rows, n, (int)tiles, part);
  else
    hipLaunchKernelGGL(cls_head_kernel<false>, dim3((unsigned)(b * tiles)), dim3(256), 0, st, x, (const u32x4 *)w1, b1, w2, l, c,
                       rows, n, (int)tiles, part);
  if (hipGetLastError() != hipSuccess) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(cls_head_finish_kernel, dim3((b + 255) / 256), dim3(256), 0, st, part, b, (int)tiles, c0, logit, prob);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
