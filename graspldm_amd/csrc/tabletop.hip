// tabletop.hip -- geometric tabletop segmentation on gfx950 (include/gldm.h: gldm_plane_ransac, gldm_plane_moments,
// gldm_segment_tabletop).  The reference has no counterpart: its pipeline starts from one object's cloud.
// Compiled with -ffp-contract=off (csrc/Makefile, SRCS_STRICT): every product, difference, sum, quotient and square root
// rounds once per written operation, so a numpy restatement in f32 decides every inlier, every foreground pixel and every
// link exactly like these kernels.
//
//   gldm_plane_ransac      T hypotheses x N points.  One launch turns the triples into planes; the count launch gives each
//                          thread kPerThread points in registers, reads the (wave-uniform) planes through scalar loads,
//                          and turns one compare per (point, hypothesis) into a ballot + popcount.  Counts gather in LDS
//                          and are flushed once per workgroup with integer atomics (order-free, so bit-deterministic).
//   gldm_plane_moments     per-tile f64 partial sums in a fixed tree, then one workgroup over the tiles in a fixed order.
//   gldm_segment_tabletop  connected components of the pixels above the plane, by union-find.  Every union hangs the
//                          higher root under the lower with atomicMin, so parents only ever decrease: every find / union
//                          loop terminates on its own data, the final root of a component is its lowest pixel index
//                          whatever the execution order, and no workgroup waits for another.  Six launches on one stream:
//                            tile     one deprojection per pixel, union-find in LDS inside a kTw x kTh tile; parent[] = the
//                                     tile-local root (global index)
//                            border   unions across tile edges on the global parent[]
//                            flatten  parent[p] = root(p); size[root] += 1 (one atomic per distinct root of a wave)
//                            gather   roots with size >= min_pixels -> 64-bit keys (size, ~root)
//                            select   one workgroup: the max_labels largest keys, in order
//                            write    labels[p] = rank of root(p) among the selected, else 0
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "components.h"
#include "depth_deproject.h"
#include "host_util.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kPerThread = 8;
constexpr int kTile = kBlock * kPerThread;   // 2048 points per workgroup (ransac, moments)
constexpr int kMaxPoints = 1 << 24;
constexpr int kMaxHyp = 4096;
constexpr int kHypChunk = 64;                // hypotheses per workgroup of the count launch (grid.y = chunks): at T = 512 and
                                             // 126 point tiles that is 1008 workgroups, four per CU, enough waves per SIMD
                                             // to cover the scalar load in front of every hypothesis (256: one wave per SIMD)
constexpr int kMoments = 10;

__device__ __forceinline__ bool plane_inlier(float nx, float ny, float nz, float d, float tol, float x, float y, float z) {
  return fabsf(((nx * x + ny * y) + nz * z) + d) <= tol;   // NaN never passes
}

// ---------------------------------------------------------------------------------------------------- plane ransac --
// One thread per hypothesis: the plane through points i, j, k, or plane 0 / count -1 / flag 1 for a degenerate one.
__global__ __launch_bounds__(kBlock) void ransac_planes_kernel(const float *__restrict__ pts, int n,
                                                               const int32_t *__restrict__ triples, int t, float min_cross2,
                                                               float *__restrict__ out_plane, int32_t *__restrict__ out_count,
                                                               int32_t *__restrict__ degenerate) {
  const int h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= t) return;
  const int i = triples[3 * h], j = triples[3 * h + 1], k = triples[3 * h + 2];
  float nx = 0.f, ny = 0.f, nz = 0.f, d = 0.f;
  bool ok = i >= 0 && i < n && j >= 0 && j < n && k >= 0 && k < n && i != j && i != k && j != k;
  if (ok) {
    const float p0x = pts[3 * (size_t)i], p0y = pts[3 * (size_t)i + 1], p0z = pts[3 * (size_t)i + 2];
    const float e1x = pts[3 * (size_t)j] - p0x, e1y = pts[3 * (size_t)j + 1] - p0y, e1z = pts[3 * (size_t)j + 2] - p0z;
    const float e2x = pts[3 * (size_t)k] - p0x, e2y = pts[3 * (size_t)k + 1] - p0y, e2z = pts[3 * (size_t)k + 2] - p0z;
    const float cx = e1y * e2z - e1z * e2y;
    const float cy = e1z * e2x - e1x * e2z;
    const float cz = e1x * e2y - e1y * e2x;
    const float l2 = (cx * cx + cy * cy) + cz * cz;
    ok = l2 >= min_cross2;
    if (ok) {
      const float l = sqrtf(l2);   // IEEE: hipcc rounds sqrtf correctly by default (__fsqrt_rn is the 1-ulp native one)
      nx = __fdiv_rn(cx, l);
      ny = __fdiv_rn(cy, l);
      nz = __fdiv_rn(cz, l);
      d = -((nx * p0x + ny * p0y) + nz * p0z);
    }
  }
  out_plane[4 * h] = nx;
  out_plane[4 * h + 1] = ny;
  out_plane[4 * h + 2] = nz;
  out_plane[4 * h + 3] = d;
  out_count[h] = ok ? 0 : -1;
  degenerate[h] = ok ? 0 : 1;
}

// grid (point tiles, hypothesis chunks).  planes / degenerate are indexed by a wave-uniform h: scalar loads.
__global__ __launch_bounds__(kBlock) void ransac_count_kernel(const float *__restrict__ pts, int n,
                                                              const float4 *__restrict__ planes,
                                                              const int32_t *__restrict__ degenerate, int t, float tol,
                                                              int32_t *__restrict__ out_count) {
  __shared__ int s_cnt[kHypChunk];
  const int tid = threadIdx.x, lane = tid & 63;
  const int h0 = blockIdx.y * kHypChunk;
  const int hn = min(kHypChunk, t - h0);
  float x[kPerThread], y[kPerThread], z[kPerThread];
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int idx = blockIdx.x * kTile + q * kBlock + tid;
    x[q] = y[q] = z[q] = __builtin_nanf("");   // rows past n: never inliers
    if (idx < n) {
      x[q] = pts[3 * (size_t)idx];
      y[q] = pts[3 * (size_t)idx + 1];
      z[q] = pts[3 * (size_t)idx + 2];
    }
  }
  for (int i = tid; i < kHypChunk; i += kBlock) s_cnt[i] = 0;
  __syncthreads();
  for (int hh = 0; hh < hn; ++hh) {
    if (degenerate[h0 + hh]) continue;   // uniform
    const float4 pl = planes[h0 + hh];
    int c = 0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) c += __popcll(__ballot(plane_inlier(pl.x, pl.y, pl.z, pl.w, tol, x[q], y[q], z[q])));
    if (lane == 0 && c) atomicAdd(&s_cnt[hh], c);
  }
  __syncthreads();
  for (int i = tid; i < hn; i += kBlock) {
    const int c = s_cnt[i];
    if (c) atomicAdd(&out_count[h0 + i], c);   // a degenerate hypothesis has c == 0: its -1 stays
  }
}

// --------------------------------------------------------------------------------------------------- plane moments --
// Sum of v[0..10) over the workgroup in a fixed tree (xor shuffles inside a wave, then the waves in ascending order);
// the result is valid in thread 0.
__device__ __forceinline__ void block_sum10(double *v, double (*s_red)[kMoments]) {
#pragma unroll
  for (int m = 0; m < kMoments; ++m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[m] += __shfl_xor(v[m], off, kWave);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) s_red[threadIdx.x >> 6][m] = v[m];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) {
      double a = s_red[0][m];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) a += s_red[w][m];
      v[m] = a;
    }
  }
}

__global__ __launch_bounds__(kBlock) void moments_tile_kernel(const float *__restrict__ pts, int n, float nx, float ny, float nz,
                                                              float d, float tol, double *__restrict__ partial) {
  __shared__ double s_red[kWaves][kMoments];
  const int tid = threadIdx.x;
  double v[kMoments];
#pragma unroll
  for (int m = 0; m < kMoments; ++m) v[m] = 0.0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int idx = blockIdx.x * kTile + q * kBlock + tid;
    if (idx < n) {
      const float fx = pts[3 * (size_t)idx], fy = pts[3 * (size_t)idx + 1], fz = pts[3 * (size_t)idx + 2];
      if (plane_inlier(nx, ny, nz, d, tol, fx, fy, fz)) {
        const double x = fx, y = fy, z = fz;
        v[0] += 1.0; v[1] += x; v[2] += y; v[3] += z;
        v[4] += x * x; v[5] += x * y; v[6] += x * z; v[7] += y * y; v[8] += y * z; v[9] += z * z;
      }
    }
  }
  block_sum10(v, s_red);
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) partial[(size_t)blockIdx.x * kMoments + m] = v[m];
  }
}

// One workgroup: thread i adds tiles i, i + kBlock, ... in ascending order, then the same tree.
__global__ __launch_bounds__(kBlock) void moments_reduce_kernel(const double *__restrict__ partial, int tiles,
                                                                double *__restrict__ out) {
  __shared__ double s_red[kWaves][kMoments];
  double v[kMoments];
#pragma unroll
  for (int m = 0; m < kMoments; ++m) v[m] = 0.0;
  for (int tl = threadIdx.x; tl < tiles; tl += kBlock) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) v[m] += partial[(size_t)tl * kMoments + m];
  }
  block_sum10(v, s_red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < kMoments; ++m) out[m] = v[m];
  }
}

int check_points(int n) {
  if (n < 1) return GLDM_ERR_INVALID_ARG;
  if (n > kMaxPoints) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

int check_ransac(int n, int t) {
  const int st = check_points(n);
  if (st != GLDM_OK) return st;
  if (t < 1) return GLDM_ERR_INVALID_ARG;
  if (t > kMaxHyp) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

// ------------------------------------------------------------------------------------------------------- segmenter --
constexpr int kTw = 64, kTh = 16;            // tile: one wave per row, kSegPer rows per wave (a 480 x 640 frame: 300 tiles)
constexpr int kSegPer = kTh / kWaves;
constexpr int kTilePix = kTw * kTh;
constexpr int kMaxLabels = 64;
constexpr int kBorderBlock = 128;            // >= kTw + kTh border pixels of a tile
static_assert(kTw == kWave && kTh % kWaves == 0, "one wave per tile row");
static_assert(kTw + kTh <= kBorderBlock, "one thread per border pixel");

struct SegParams {
  DepthParams P;
  float a, b, c, d, h_min, h_max, link2;
  int h, tiles_x;
};

// Foreground: `deproject` keeps the pixel and its height over the plane lies in (h_min, h_max].
template <typename T>
__device__ __forceinline__ bool foreground(const T *__restrict__ depth, const uint8_t *__restrict__ mask, const SegParams &S,
                                           int pix, float &x, float &y, float &z) {
  const float dv = load_depth(depth, (size_t)pix, S.P.depth_scale);
  const unsigned m = mask ? mask[pix] : 1u;
  if (!deproject(S.P, pix, dv, m, x, y, z)) return false;
  const float hgt = ((S.a * x + S.b * y) + S.c * z) + S.d;
  return hgt > S.h_min && hgt <= S.h_max;
}

__device__ __forceinline__ bool close_enough(const SegParams &S, float x0, float y0, float z0, float x1, float y1, float z1) {
  const float dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
  return ((dx * dx + dy * dy) + dz * dz) <= S.link2;
}

// One tile: local union-find in LDS over the links inside the tile.  parent[p] = global index of the tile-local root, -1 for
// background; size[p] = 0.  Local index l = ly * kTw + lx grows with the global pixel index inside a tile, so the lowest
// local root is the lowest pixel.  Every pixel is deprojected once; its right and lower neighbours inside the tile are read
// back from LDS (the border launch deprojects the pairs that straddle two tiles with the same inlined code).
template <typename T>
__global__ __launch_bounds__(kBlock) void seg_tile_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                          SegParams S, int32_t *__restrict__ parent, int32_t *__restrict__ size,
                                                          int32_t *__restrict__ cand_count) {
  __shared__ int s_par[kTilePix];
  __shared__ float s_x[kTilePix], s_y[kTilePix], s_z[kTilePix];
  const int tid = threadIdx.x, lx = tid & 63;
  const int ty = blockIdx.x / S.tiles_x, tx = blockIdx.x - ty * S.tiles_x;
  const int w = S.P.w, u = tx * kTw + lx;
  if (blockIdx.x == 0 && tid == 0) *cand_count = 0;
#pragma unroll
  for (int q = 0; q < kSegPer; ++q) {
    const int ly = q * kWaves + (tid >> 6), v = ty * kTh + ly, l = ly * kTw + lx;
    int par = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (u < w && v < S.h && foreground(depth, mask, S, v * w + u, x, y, z)) par = l;
    s_par[l] = par;
    s_x[l] = x;
    s_y[l] = y;
    s_z[l] = z;
  }
  __syncthreads();
  unsigned right = 0u, down = 0u;   // bit q: linked to the neighbour inside the tile
#pragma unroll
  for (int q = 0; q < kSegPer; ++q) {
    const int ly = q * kWaves + (tid >> 6), l = ly * kTw + lx;
    if (s_par[l] >= 0) {   // the initial values: nothing is united before the barrier below
      if (lx + 1 < kTw && s_par[l + 1] >= 0 && close_enough(S, s_x[l], s_y[l], s_z[l], s_x[l + 1], s_y[l + 1], s_z[l + 1]))
        right |= 1u << q;
      if (ly + 1 < kTh && s_par[l + kTw] >= 0 &&
          close_enough(S, s_x[l], s_y[l], s_z[l], s_x[l + kTw], s_y[l + kTw], s_z[l + kTw]))
        down |= 1u << q;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kSegPer; ++q) {
    const int l = (q * kWaves + (tid >> 6)) * kTw + lx;
    if (right & (1u << q)) uf_union(s_par, l, l + 1);
    if (down & (1u << q)) uf_union(s_par, l, l + kTw);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kSegPer; ++q) {
    const int ly = q * kWaves + (tid >> 6), v = ty * kTh + ly, l = ly * kTw + lx;
    if (u < w && v < S.h) {
      const int pix = v * w + u;
      int root = -1;
      if (s_par[l] >= 0) {
        const int r = uf_find(s_par, l);
        root = (ty * kTh + r / kTw) * w + tx * kTw + (r % kTw);
      }
      parent[pix] = root;
      size[pix] = 0;
    }
  }
}

// Links across tile edges: thread i < kTw looks down from the tile's last row, kTw <= i < kTw + kTh right from its last column.
template <typename T>
__global__ __launch_bounds__(kBorderBlock) void seg_border_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                  SegParams S, int32_t *__restrict__ parent) {
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / S.tiles_x, tx = blockIdx.x - ty * S.tiles_x;
  const int w = S.P.w;
  int u, v, step;
  if (tid < kTw) {
    u = tx * kTw + tid; v = ty * kTh + kTh - 1; step = w;
    if (u >= w || v + 1 >= S.h) return;
  } else if (tid < kTw + kTh) {
    u = tx * kTw + kTw - 1; v = ty * kTh + (tid - kTw); step = 1;
    if (u + 1 >= w || v >= S.h) return;
  } else {
    return;
  }
  const int pix = v * w + u;
  float x, y, z, xn, yn, zn;
  if (foreground(depth, mask, S, pix, x, y, z) && foreground(depth, mask, S, pix + step, xn, yn, zn) &&
      close_enough(S, x, y, z, xn, yn, zn))
    uf_union(parent, pix, pix + step);
}

// parent[p] = root(p) (a racing reader sees an ancestor either way), and one atomic per distinct root of a wave onto size[].
__global__ __launch_bounds__(kBlock) void seg_flatten_kernel(int32_t *__restrict__ parent, int32_t *__restrict__ size, int hw) {
  const int pix = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63;
  int r = -1;
  if (pix < hw && __atomic_load_n(&parent[pix], __ATOMIC_RELAXED) >= 0) {
    r = uf_find(parent, pix);
    __atomic_store_n(&parent[pix], r, __ATOMIC_RELAXED);
  }
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {   // uniform: todo is a ballot
    const int lead = __ffsll((long long)todo) - 1;
    const int rr = __shfl(r, lead, kWave);
    const unsigned long long same = __ballot(r == rr);
    if (lane == lead) atomicAdd(&size[rr], __popcll(same));
    todo &= ~same;
  }
}

// Roots of at least min_pixels pixels -> cand[0 .. *cand_count), in any order (the selection does not depend on it).
__global__ __launch_bounds__(kBlock) void seg_gather_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size,
                                                            int hw, int min_pixels, unsigned long long *__restrict__ cand,
                                                            int32_t *__restrict__ cand_count) {
  const int pix = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63;
  int sz = 0;
  const bool is = pix < hw && parent[pix] == pix && (sz = size[pix]) >= min_pixels;
  const unsigned long long bal = __ballot(is);
  if (!bal) return;
  int base = 0;
  if (lane == __ffsll((long long)bal) - 1) base = atomicAdd(cand_count, __popcll(bal));   // at most hw roots in all
  base = __shfl(base, __ffsll((long long)bal) - 1, kWave);
  if (is) cand[base + __popcll(bal & ((1ull << lane) - 1ull))] = seg_key(sz, pix);
}

// One workgroup: components.h's select_largest over the candidates.
__global__ __launch_bounds__(kSelectBlock) void seg_select_kernel(const unsigned long long *__restrict__ cand,
                                                                  const int32_t *__restrict__ cand_count, int max_labels,
                                                                  int32_t *__restrict__ num_labels,
                                                                  int32_t *__restrict__ label_pixels,
                                                                  int32_t *__restrict__ label_root) {
  __shared__ unsigned long long s_key[kSelectBlock];
  __shared__ unsigned long long s_best;
  select_largest(cand, *cand_count, max_labels, num_labels, label_pixels, label_root, s_key, &s_best);
}

__global__ __launch_bounds__(kBlock) void seg_write_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size,
                                                           int hw, int min_pixels, const int32_t *__restrict__ num_labels,
                                                           const int32_t *__restrict__ label_root,
                                                           int32_t *__restrict__ labels) {
  __shared__ int s_root[kMaxLabels];
  const int k = *num_labels;   // <= max_labels <= kMaxLabels
  if ((int)threadIdx.x < k) s_root[threadIdx.x] = label_root[threadIdx.x];
  __syncthreads();
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= hw) return;
  const int r = parent[pix];
  int lab = 0;
  if (r >= 0 && size[r] >= min_pixels) {
    for (int i = 0; i < k; ++i) lab = s_root[i] == r ? i + 1 : lab;
  }
  labels[pix] = lab;
}

// workspace: parent [hw] int32 | size [hw] int32 | cand [hw] u64 | cand_count (8 bytes)
long long seg_bytes(long long hw) { return hw * 16ll + 8ll; }

int check_frame(int h, int w) {
  if (h < 1 || w < 1) return GLDM_ERR_INVALID_ARG;
  if ((long long)h * w > kMaxPoints) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

int check_segment(int h, int w, int min_pixels, int max_labels) {
  const int st = check_frame(h, w);
  if (st != GLDM_OK) return st;
  if (min_pixels < 1 || max_labels < 1) return GLDM_ERR_INVALID_ARG;
  if (max_labels > kMaxLabels) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

template <typename T>
int run_segment(const T *depth, const uint8_t *mask, const SegParams &S, int min_pixels, int max_labels, void *workspace,
                int32_t *labels, int32_t *num_labels, int32_t *label_pixels, int32_t *label_root, hipStream_t s) {
  const int hw = S.P.hw;
  int32_t *parent = static_cast<int32_t *>(workspace);
  int32_t *size = parent + hw;
  unsigned long long *cand = reinterpret_cast<unsigned long long *>(size + hw);   // byte offset 8 * hw: aligned
  int32_t *cand_count = reinterpret_cast<int32_t *>(cand + hw);
  const int tiles = S.tiles_x * ((S.h + kTh - 1) / kTh);
  const int blocks = (hw + kBlock - 1) / kBlock;
  int st;
  hipLaunchKernelGGL((seg_tile_kernel<T>), dim3(tiles), dim3(kBlock), 0, s, depth, mask, S, parent, size, cand_count);
  if ((st = launch_status()) != GLDM_OK) return st;
  hipLaunchKernelGGL((seg_border_kernel<T>), dim3(tiles), dim3(kBorderBlock), 0, s, depth, mask, S, parent);
  if ((st = launch_status()) != GLDM_OK) return st;
  hipLaunchKernelGGL(seg_flatten_kernel, dim3(blocks), dim3(kBlock), 0, s, parent, size, hw);
  if ((st = launch_status()) != GLDM_OK) return st;
  hipLaunchKernelGGL(seg_gather_kernel, dim3(blocks), dim3(kBlock), 0, s, parent, size, hw, min_pixels, cand, cand_count);
  if ((st = launch_status()) != GLDM_OK) return st;
  hipLaunchKernelGGL(seg_select_kernel, dim3(1), dim3(kSelectBlock), 0, s, cand, cand_count, max_labels, num_labels,
                     label_pixels, label_root);
  if ((st = launch_status()) != GLDM_OK) return st;
  hipLaunchKernelGGL(seg_write_kernel, dim3(blocks), dim3(kBlock), 0, s, parent, size, hw, min_pixels, num_labels, label_root,
                     labels);
  return launch_status();
}

}  // namespace

GLDM_API int gldm_plane_ransac_tile_points(void) { return kTile; }

GLDM_API long long gldm_plane_ransac_workspace_bytes(int n, int t) {
  const int st = check_ransac(n, t);
  if (st != GLDM_OK) return st;
  return (long long)t * (long long)sizeof(int32_t);
}

GLDM_API int gldm_plane_ransac(const float *points, int n, const int32_t *triples, int t, float tol, float min_cross2,
                               void *workspace, long long workspace_bytes, float *out_plane, int32_t *out_count,
                               gldm_stream_t stream) {
  // the envelope first: nothing below touches a pointer or the device before it holds
  const int st = check_ransac(n, t);
  if (st != GLDM_OK) return st;
  if (tol != tol || min_cross2 != min_cross2) return GLDM_ERR_INVALID_ARG;
  if (!points || !triples || !workspace || !out_plane || !out_count) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_plane_ransac_workspace_bytes(n, t)) return GLDM_ERR_WORKSPACE;
  int32_t *degenerate = static_cast<int32_t *>(workspace);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(ransac_planes_kernel, dim3((t + kBlock - 1) / kBlock), dim3(kBlock), 0, s, points, n, triples, t,
                     min_cross2, out_plane, out_count, degenerate);
  const int st2 = launch_status();
  if (st2 != GLDM_OK) return st2;
  hipLaunchKernelGGL(ransac_count_kernel, dim3((n + kTile - 1) / kTile, (t + kHypChunk - 1) / kHypChunk), dim3(kBlock), 0, s,
                     points, n, reinterpret_cast<const float4 *>(out_plane), degenerate, t, tol, out_count);
  return launch_status();
}

GLDM_API long long gldm_plane_moments_workspace_bytes(int n) {
  const int st = check_points(n);
  if (st != GLDM_OK) return st;
  return (long long)((n + kTile - 1) / kTile) * kMoments * (long long)sizeof(double);
}

GLDM_API int gldm_plane_moments(const float *points, int n, const float *plane, float tol, void *workspace,
                                long long workspace_bytes, double *out, gldm_stream_t stream) {
  const int st = check_points(n);
  if (st != GLDM_OK) return st;
  if (tol != tol || !points || !plane || !workspace || !out) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_plane_moments_workspace_bytes(n)) return GLDM_ERR_WORKSPACE;
  const int tiles = (n + kTile - 1) / kTile;
  double *partial = static_cast<double *>(workspace);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(moments_tile_kernel, dim3(tiles), dim3(kBlock), 0, s, points, n, plane[0], plane[1], plane[2], plane[3],
                     tol, partial);
  const int st2 = launch_status();
  if (st2 != GLDM_OK) return st2;
  hipLaunchKernelGGL(moments_reduce_kernel, dim3(1), dim3(kBlock), 0, s, partial, tiles, out);
  return launch_status();
}

GLDM_API int gldm_segment_tile_shape(int *tw, int *th) {
  if (!tw || !th) return GLDM_ERR_INVALID_ARG;
  *tw = kTw;
  *th = kTh;
  return GLDM_OK;
}

GLDM_API long long gldm_segment_tabletop_workspace_bytes(int h, int w) {
  const int st = check_frame(h, w);
  if (st != GLDM_OK) return st;
  return seg_bytes((long long)h * w);
}

GLDM_API int gldm_segment_tabletop(const void *depth, int depth_is_u16, float depth_scale, const uint8_t *mask, int h, int w,
                                   float fx, float fy, float cx, float cy, float z_min, float z_max,
                                   const float *cam_to_world, const float *box_lo, const float *box_hi, const float *plane,
                                   float h_min, float h_max, float link_dist, int min_pixels, int max_labels, void *workspace,
                                   long long workspace_bytes, int32_t *labels, int32_t *num_labels, int32_t *label_pixels,
                                   int32_t *label_root, gldm_stream_t stream) {
  // the envelope first: nothing below touches a pointer or the device before it holds
  const int st = check_segment(h, w, min_pixels, max_labels);
  if (st != GLDM_OK) return st;
  if (!(fx != 0.f) || !(fy != 0.f) || !(z_min < z_max) || fx != fx || fy != fy || cx != cx || cy != cy)
    return GLDM_ERR_INVALID_ARG;
  if (!(h_min < h_max) || !(link_dist >= 0.f)) return GLDM_ERR_INVALID_ARG;
  if (!depth || !plane || !workspace || !labels || !num_labels || !label_pixels || !label_root ||
      (box_lo == nullptr) != (box_hi == nullptr))
    return GLDM_ERR_INVALID_ARG;
  if (depth_is_u16 != 0 && depth_is_u16 != 1) return GLDM_ERR_INVALID_ARG;
  if (plane[0] != plane[0] || plane[1] != plane[1] || plane[2] != plane[2] || plane[3] != plane[3]) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_segment_tabletop_workspace_bytes(h, w)) return GLDM_ERR_WORKSPACE;
  SegParams S;
  S.P = make_params(depth_is_u16, depth_scale, h, w, fx, fy, cx, cy, z_min, z_max, cam_to_world, box_lo, box_hi);
  S.a = plane[0]; S.b = plane[1]; S.c = plane[2]; S.d = plane[3];
  S.h_min = h_min; S.h_max = h_max;
  S.link2 = link_dist * link_dist;   // formed once, in f32
  S.h = h;
  S.tiles_x = (w + kTw - 1) / kTw;
  hipStream_t s = as_stream(stream);
  if (depth_is_u16)
    return run_segment(static_cast<const uint16_t *>(depth), mask, S, min_pixels, max_labels, workspace, labels, num_labels,
                       label_pixels, label_root, s);
  return run_segment(static_cast<const float *>(depth), mask, S, min_pixels, max_labels, workspace, labels, num_labels,
                     label_pixels, label_root, s);
}
