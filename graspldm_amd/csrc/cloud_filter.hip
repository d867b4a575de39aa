// cloud_filter.hip -- outlier removal on ragged sensor clouds (include/gldm.h, "sensor-cloud cleanup"):
//
//   gldm_neighbor_stats   for every point the number of other points of its cloud within a radius (capped at k) and the mean
//                         distance to the up to k nearest of them: ONE scan, the broad phase of knn_kernel (normals.hip) with
//                         32-bit keys (the bits of d2) and no index list.
//   gldm_filter_outliers  the keep rule (a neighbour count, and optionally mean distance <= mu + std_ratio * sigma of the
//                         cloud, Open3D's radius and statistical filters) and the ordered compaction of the kept rows.
//
// Clouds are ragged: cloud i is rows start[i] .. start[i] + count[i] of points [rows,3]; its 256-row chunks are counted from
// its own start.  Compiled with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): every f32 and f64 operation below rounds
// once, as tests/cloud_filter_ref.py restates it.
#include <math.h>
#include <stdint.h>

#include "knn_scan.h"
#include "ragged_compact.h"   // Range, cloud_range, chunk_count, scan_kernel: shared with cloud_downsample.hip

namespace {

// boxes [b, chunks_max, 6]: lo xyz, hi xyz of every 256-row chunk of every cloud (chunks past a cloud's end: not written).
__global__ __launch_bounds__(kChunk) void ragged_box_kernel(const float *__restrict__ pts, const int32_t *__restrict__ start,
                                                            const int32_t *__restrict__ count, int n_max, int rows,
                                                            int chunks_max, float *__restrict__ boxes) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int p0 = ch * kChunk;
  if (p0 >= rg.n) return;   // uniform over the workgroup
  chunk_box_body(pts + (rg.s + p0) * 3, min(kChunk, rg.n - p0), boxes + ((long long)cloud * chunks_max + ch) * 6);
}

// knn_kernel's scan (normals.hip) for the filter: a workgroup's 256 lanes are the query points of one chunk, every lane
// keeps the KT smallest d2 among the OTHER points (j != i by index) within r2, sorted in registers as 32-bit patterns; the
// candidate chunks come through LDS outward from the own chunk; the same two exact skips (box_d2).  Only the multiset of
// the k smallest d2 leaves the kernel, so a candidate that ties the k-th changes nothing and equal keys need no index.
template <int KT>
__global__ __launch_bounds__(kChunk) void stats_kernel(const float *__restrict__ all_pts, const int32_t *__restrict__ start,
                                                       const int32_t *__restrict__ count, const float *__restrict__ boxes,
                                                       int n_max, int rows, int k, int chunks_max, float r2,
                                                       int32_t *__restrict__ neighbors, float *__restrict__ score) {
  __shared__ float pts[kChunk * 3];
  const int tid = threadIdx.x;
  const int own = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int n = rg.n;
  if (own * kChunk >= n) return;   // uniform over the workgroup
  const int chunks = chunks_of(n);
  const float *cloud_pts = all_pts + rg.s * 3;
  const float *cloud_boxes = boxes + (long long)cloud * chunks_max * 6;
  const int qi = own * kChunk + tid;
  const bool live = qi < n;
  const int qs = live ? qi : n - 1;
  const float qx = cloud_pts[(long long)qs * 3 + 0], qy = cloud_pts[(long long)qs * 3 + 1], qz = cloud_pts[(long long)qs * 3 + 2];

  uint32_t key[KT];
#pragma unroll
  for (int s = 0; s < KT; ++s) key[s] = kInfBits;

  const Box own_box = load_box(cloud_boxes, own);
  const Box wave_box = wave_query_box(qx, qy, qz);   // dead lanes repeat the cloud's last point, which is in the chunk
  float bound = r2;                                  // wave-uniform

  const int reach = max(own, chunks - 1 - own);
  for (int step = 0; step <= reach; ++step) {
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const int ch = side == 0 ? own + step : own - step;
      if (ch < 0 || ch >= chunks || (side == 1 && step == 0)) continue;   // uniform over the workgroup
      const Box cb = load_box(cloud_boxes, ch);
      if (box_d2(own_box, cb) > r2) continue;                             // uniform over the workgroup
      const int p0 = ch * kChunk;
      const int cnt = min(kChunk, n - p0);
      stage_chunk(pts, cloud_pts + (long long)p0 * 3, cnt);
      if (box_d2(wave_box, cb) > bound) continue;   // wave-uniform; the barriers above are behind this wave already
      for (int c = 0; c < cnt; ++c) {
        const float dx = pts[c * 3 + 0] - qx, dy = pts[c * 3 + 1] - qy, dz = pts[c * 3 + 2] - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const uint32_t cand = __float_as_uint(d2);
        insert_key<uint32_t, KT>(key, cand, live && p0 + c != qi && d2 <= r2 && cand < key[KT - 1]);
      }
      // the wave's largest k-th squared distance: +inf while a live lane's list is short
      uint32_t kth = 0u;
#pragma unroll
      for (int s = 0; s < KT; ++s)
        if (s == k - 1) kth = key[s];
      bound = fminf(r2, __uint_as_float(wave_max_bits(live ? kth : 0u)));
    }
  }

  if (live) {
    int found = 0;
    double sum = 0.0;   // ascending d2
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      if (s < k && key[s] != kInfBits) {
        ++found;
        sum += (double)sqrtf(__uint_as_float(key[s]));   // IEEE: hipcc rounds sqrtf correctly by default
      }
    }
    neighbors[rg.s + qi] = found;
    score[rg.s + qi] = found ? (float)(sum / (double)found) : __uint_as_float(kInfBits);
  }
}

template <int KT>
void launch_stats(hipStream_t st, unsigned blocks, const float *pts, const int32_t *start, const int32_t *count,
                  const float *boxes, int n_max, int rows, int k, int chunks_max, float r2, int32_t *neighbors, float *score) {
  hipLaunchKernelGGL(stats_kernel<KT>, dim3(blocks), dim3(kChunk), 0, st, pts, start, count, boxes, n_max, rows, k, chunks_max,
                     r2, neighbors, score);
}

// ------------------------------------------------------------------------------------------- keep rule and compaction --

// The fixed tree of a 256-row chunk: a butterfly over each wave's 64 lanes (offsets 32, 16, .. 1; a + b = b + a, so every
// lane holds the same bits), then (w0 + w1) + (w2 + w3).  Returned in every lane.
__device__ __forceinline__ double chunk_tree_sum(double v, double *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();   // red is free again
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// PASS 0: per chunk the number of points with neighbors >= need and the sum of their scores; PASS 1: the sum of their
// (score - mu)^2.  f64, fixed tree.  tile_cnt / partial [b, chunks_max].
template <int PASS>
__global__ __launch_bounds__(kChunk) void moment_tile_kernel(const int32_t *__restrict__ neighbors,
                                                             const float *__restrict__ score,
                                                             const int32_t *__restrict__ start,
                                                             const int32_t *__restrict__ count, int n_max, int rows,
                                                             int chunks_max, int need, const double *__restrict__ stats,
                                                             int32_t *__restrict__ tile_cnt, double *__restrict__ partial) {
  __shared__ double red[kChunk / 64];
  __shared__ int redi[kChunk / 64];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const bool valid = qi < rg.n && neighbors[rg.s + qi] >= need;
  double v = 0.0;
  if (valid) {
    const double sc = (double)score[rg.s + qi];
    if (PASS == 0) {
      v = sc;
    } else {
      const double d = sc - stats[cloud * 2];
      v = d * d;
    }
  }
  const double sum = chunk_tree_sum(v, red);
  int before;
  const int cnt = PASS == 0 ? chunk_count(valid, redi, before) : 0;
  if (threadIdx.x == 0) {
    partial[(long long)cloud * chunks_max + ch] = sum;
    if (PASS == 0) tile_cnt[(long long)cloud * chunks_max + ch] = cnt;
  }
}

// One lane per cloud, its chunks in ascending order.  PASS 0: N and mu = S1 / N (0 for N = 0); PASS 1: sigma =
// sqrt(S2 / (N - 1)) (0 for N < 2) and the threshold mu + std_ratio * sigma.  stats [b,2] = mu, sigma.
template <int PASS>
__global__ __launch_bounds__(256) void moment_cloud_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                           int b, int n_max, int rows, int chunks_max,
                                                           const int32_t *__restrict__ tile_cnt,
                                                           const double *__restrict__ partial, float std_ratio,
                                                           int32_t *__restrict__ valid_n, double *__restrict__ stats,
                                                           double *__restrict__ thr) {
  const int cloud = blockIdx.x * 256 + threadIdx.x;
  if (cloud >= b) return;
  const int chunks = chunks_of(cloud_range(start, count, cloud, n_max, rows).n);
  const long long at = (long long)cloud * chunks_max;
  double sum = 0.0;
  for (int ch = 0; ch < chunks; ++ch) sum += partial[at + ch];
  if (PASS == 0) {
    int n = 0;
    for (int ch = 0; ch < chunks; ++ch) n += tile_cnt[at + ch];
    valid_n[cloud] = n;
    stats[cloud * 2] = n > 0 ? sum / (double)n : 0.0;
  } else {
    const int n = valid_n[cloud];
    const double mu = stats[cloud * 2];
    const double sigma = n >= 2 ? sqrt(sum / (double)(n - 1)) : 0.0;
    stats[cloud * 2 + 1] = sigma;
    thr[cloud] = mu + (double)std_ratio * sigma;
  }
}

// neighbors >= min_neighbors and, with the statistical rule, at least one neighbour and score <= the cloud's threshold.
__device__ __forceinline__ bool keep_point(int nb, float sc, int min_neighbors, bool stat, double thr) {
  return nb >= min_neighbors && (!stat || (nb >= 1 && (double)sc <= thr));
}

// WRITE 0: the kept rows of every chunk -> tile_cnt.  WRITE 1 (after scan_kernel): the kept rows, packed in ascending row
// order behind out_start[cloud] + the chunk's offset; rows copied bit for bit, kept = the source row relative to the start.
template <int WRITE>
__global__ __launch_bounds__(kChunk) void keep_kernel(const float *__restrict__ pts, const int32_t *__restrict__ neighbors,
                                                      const float *__restrict__ score, const int32_t *__restrict__ start,
                                                      const int32_t *__restrict__ count, int n_max, int rows, int chunks_max,
                                                      int min_neighbors, int stat, const double *__restrict__ thr,
                                                      int32_t *__restrict__ tile_cnt, const int32_t *__restrict__ out_start,
                                                      float *__restrict__ out_points, int32_t *__restrict__ kept) {
  __shared__ int redi[kChunk / 64];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int qi = ch * kChunk + (int)threadIdx.x;
  const long long row = rg.s + qi;
  const bool keep = qi < rg.n && keep_point(neighbors[row], score[row], min_neighbors, stat != 0, thr[cloud]);
  int before;
  const int total = chunk_count(keep, redi, before);
  const long long tile = (long long)cloud * chunks_max + ch;
  if (WRITE == 0) {
    if (threadIdx.x == 0) tile_cnt[tile] = total;
  } else if (keep) {
    const long long dst = (long long)out_start[cloud] + tile_cnt[tile] + before;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(pts) + row * 3;
    uint32_t *o = reinterpret_cast<uint32_t *>(out_points) + dst * 3;
    o[0] = src[0], o[1] = src[1], o[2] = src[2];
    kept[dst] = qi;
  }
}

// The envelope the two entries share; no pointer is read and the device is not touched outside it.
int check_envelope(int b, int n_max, int rows, int k) {
  if (b < 1 || n_max < 0 || rows < 0) return GLDM_ERR_INVALID_ARG;
  if (b > kMaxClouds || n_max > kMaxN || k < 1 || k > kMaxK) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

}  // namespace

GLDM_API long long gldm_neighbor_stats_workspace_bytes(int b, int n_max) {
  const int st = check_envelope(b, n_max, 0, 1);
  if (st != GLDM_OK) return st;
  return (long long)b * ceil_div(n_max, kChunk) * 6 * (long long)sizeof(float);
}

GLDM_API int gldm_neighbor_stats(const float *points, const int32_t *start, const int32_t *count, int b, int n_max, int rows,
                                 int k, float max_radius, void *workspace, long long workspace_bytes, int32_t *neighbors,
                                 float *score, gldm_stream_t stream) {
  const int env = check_envelope(b, n_max, rows, k);
  if (env != GLDM_OK) return env;
  if (!(max_radius >= 0.f) || !isfinite(max_radius * max_radius)) return GLDM_ERR_INVALID_ARG;   // r2 must be finite
  if (n_max == 0 || rows == 0) return GLDM_OK;   // every cloud is empty
  const long long need = gldm_neighbor_stats_workspace_bytes(b, n_max);
  if (!points || !start || !count || !neighbors || !score || !workspace) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < need) return GLDM_ERR_WORKSPACE;
  const int chunks_max = ceil_div(n_max, kChunk);
  const unsigned blocks = (unsigned)((long long)b * chunks_max);   // <= 65535 * 4096
  const float r2 = max_radius * max_radius;
  float *boxes = static_cast<float *>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ragged_box_kernel, dim3(blocks), dim3(kChunk), 0, st, points, start, count, n_max, rows, chunks_max, boxes);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  if (k <= 4)
    launch_stats<4>(st, blocks, points, start, count, boxes, n_max, rows, k, chunks_max, r2, neighbors, score);
  else if (k <= 8)
    launch_stats<8>(st, blocks, points, start, count, boxes, n_max, rows, k, chunks_max, r2, neighbors, score);
  else if (k <= 12)
    launch_stats<12>(st, blocks, points, start, count, boxes, n_max, rows, k, chunks_max, r2, neighbors, score);
  else
    launch_stats<16>(st, blocks, points, start, count, boxes, n_max, rows, k, chunks_max, r2, neighbors, score);
  return launch_status();
}

// workspace: partial f64 [tiles], thr f64 [b], tile_cnt int32 [tiles], valid_n int32 [b]
GLDM_API long long gldm_filter_outliers_workspace_bytes(int b, int n_max) {
  const int st = check_envelope(b, n_max, 0, 1);
  if (st != GLDM_OK) return st;
  const long long tiles = (long long)b * ceil_div(n_max, kChunk);
  return (tiles + b) * (long long)sizeof(double) + align8((tiles + b) * (long long)sizeof(int32_t));
}

GLDM_API int gldm_filter_outliers(const float *points, const int32_t *neighbors, const float *score, const int32_t *start,
                                  const int32_t *count, int b, int n_max, int rows, int k, int min_neighbors, float std_ratio,
                                  void *workspace, long long workspace_bytes, float *out_points, int32_t *out_start,
                                  int32_t *out_count, int32_t *kept, double *stats, gldm_stream_t stream) {
  const int env = check_envelope(b, n_max, rows, k);
  if (env != GLDM_OK) return env;
  if (min_neighbors < 0 || min_neighbors > k || std_ratio != std_ratio) return GLDM_ERR_INVALID_ARG;
  const bool empty = n_max == 0 || rows == 0;   // every cloud is empty: counts and statistics are still written
  if (!start || !count || !out_start || !out_count || !stats || !workspace) return GLDM_ERR_INVALID_ARG;
  if (!empty && (!points || !neighbors || !score || !out_points || !kept)) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_filter_outliers_workspace_bytes(b, n_max)) return GLDM_ERR_WORKSPACE;
  const int chunks_max = ceil_div(n_max, kChunk);
  const long long tiles = (long long)b * chunks_max;
  double *partial = static_cast<double *>(workspace);
  double *thr = partial + tiles;
  int32_t *tile_cnt = reinterpret_cast<int32_t *>(thr + b);
  int32_t *valid_n = tile_cnt + tiles;
  const int need = max(min_neighbors, 1);
  const int stat = std_ratio >= 0.f ? 1 : 0;
  const unsigned blocks = empty ? 0u : (unsigned)tiles, cloud_blocks = (unsigned)ceil_div(b, 256);
  const int nm = empty ? 0 : n_max;   // the per-cloud kernels then see empty clouds and read no tile
  hipStream_t st = as_stream(stream);
  if (blocks)
    hipLaunchKernelGGL(moment_tile_kernel<0>, dim3(blocks), dim3(kChunk), 0, st, neighbors, score, start, count, n_max, rows,
                       chunks_max, need, stats, tile_cnt, partial);
  hipLaunchKernelGGL(moment_cloud_kernel<0>, dim3(cloud_blocks), dim3(256), 0, st, start, count, b, nm, rows, chunks_max, tile_cnt,
                     partial, std_ratio, valid_n, stats, thr);
  if (blocks)
    hipLaunchKernelGGL(moment_tile_kernel<1>, dim3(blocks), dim3(kChunk), 0, st, neighbors, score, start, count, n_max, rows,
                       chunks_max, need, stats, tile_cnt, partial);
  hipLaunchKernelGGL(moment_cloud_kernel<1>, dim3(cloud_blocks), dim3(256), 0, st, start, count, b, nm, rows, chunks_max, tile_cnt,
                     partial, std_ratio, valid_n, stats, thr);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  if (blocks)
    hipLaunchKernelGGL(keep_kernel<0>, dim3(blocks), dim3(kChunk), 0, st, points, neighbors, score, start, count, n_max, rows,
                       chunks_max, min_neighbors, stat, thr, tile_cnt, out_start, out_points, kept);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, start, count, b, nm, rows, chunks_max, tile_cnt, out_start,
                     out_count);
  if (blocks)
    hipLaunchKernelGGL(keep_kernel<1>, dim3(blocks), dim3(kChunk), 0, st, points, neighbors, score, start, count, n_max, rows,
                       chunks_max, min_neighbors, stat, thr, tile_cnt, out_start, out_points, kept);
  return launch_status();
}
