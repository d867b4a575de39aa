// ragged_compact.h -- the ragged layout and the ordered compaction that cloud_filter.hip (gldm_filter_outliers) and
// cloud_downsample.hip (gldm_voxel_downsample) share: cloud i is rows start[i] .. start[i] + count[i] of points [rows,3];
// its 256-row chunks are counted from its own start; flagged rows go out in ascending row order through per-chunk counts,
// one scan launch and a ballot + popcount rank.  No atomics, no workgroup waits for another.
#pragma once
#include <stdint.h>

#include "knn_scan.h"   // kChunk

namespace {

constexpr int kMaxClouds = 65535;

__host__ __device__ constexpr int chunks_of(int n) { return (n + kChunk - 1) / kChunk; }

struct Range {
  long long s;   // first row
  int n;         // rows
};

// The rows of one cloud: count clamped to [0, n_max]; a range that leaves [0, rows) is empty (nothing outside the array is
// ever addressed).
__device__ __forceinline__ Range cloud_range(const int32_t *__restrict__ start, const int32_t *__restrict__ count, int cloud,
                                             int n_max, int rows) {
  const long long s = start[cloud];
  int n = max(0, min(count[cloud], n_max));
  if (s < 0 || s + n > (long long)rows) n = 0;
  return {s, n};
}

// The number of set flags in the chunk (every lane) and, in `before`, the number set in lower lanes of the workgroup.
__device__ __forceinline__ int chunk_count(bool flag, int *red, int &before) {
  const unsigned long long bal = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();   // red is free again
  if (lane == 0) red[wave] = __popcll(bal);
  __syncthreads();
  before = __popcll(bal & ((1ull << lane) - 1ull));
  int total = 0;
#pragma unroll
  for (int w = 0; w < kChunk / 64; ++w) {
    before += w < wave ? red[w] : 0;
    total += red[w];
  }
  return total;
}

// One workgroup: every cloud's tile counts -> exclusive offsets inside the cloud (in place) and out_count; then the exclusive
// sum of out_count over the clouds -> out_start.  Lane t owns the clouds t*per .. (t+1)*per - 1.
__global__ __launch_bounds__(256) void scan_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count, int b,
                                                   int n_max, int rows, int chunks_max, int32_t *__restrict__ tile_cnt,
                                                   int32_t *__restrict__ out_start, int32_t *__restrict__ out_count) {
  __shared__ int sums[256];
  const int tid = threadIdx.x;
  const int per = (b + 255) / 256;
  const int c0 = min(b, tid * per), c1 = min(b, c0 + per);
  int mine = 0;
  for (int cloud = c0; cloud < c1; ++cloud) {
    const int chunks = chunks_of(cloud_range(start, count, cloud, n_max, rows).n);
    const long long at = (long long)cloud * chunks_max;
    int run = 0;
    for (int ch = 0; ch < chunks; ++ch) {
      const int c = tile_cnt[at + ch];
      tile_cnt[at + ch] = run;
      run += c;
    }
    out_count[cloud] = run;
    mine += run;
  }
  sums[tid] = mine;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += sums[t];
  for (int cloud = c0; cloud < c1; ++cloud) {
    out_start[cloud] = base;
    base += out_count[cloud];
  }
}

inline long long align8(long long v) { return (v + 7) & ~7ll; }

}  // namespace
