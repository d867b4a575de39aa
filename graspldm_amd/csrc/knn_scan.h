// knn_scan.h -- the pieces the two radius-bounded neighbour scans share: knn_kernel (normals.hip: 64-bit (d2, index) keys,
// index lists out) and stats_kernel (cloud_filter.hip: 32-bit d2 keys, count and mean distance out).  Both sources are built
// with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): a squared distance is (dx*dx + dy*dy) + dz*dz with one rounding per
// written operation, and the broad phase below is exact only on such values.
#pragma once
#include <stdint.h>

#include "host_util.h"

namespace {

constexpr int kChunk = 256;        // points staged per step = threads per workgroup = query points per workgroup
constexpr int kMaxK = 16;
constexpr int kMaxN = 1 << 20;
constexpr uint32_t kInfBits = 0x7f800000u;

struct Box {
  float lo[3], hi[3];
};

// Squared distance between two boxes in the arithmetic of a point pair: per axis the gap g = max(0, alo - bhi, blo - ahi)
// is a rounded difference of two coordinates that bracket every pair's, and rounding is monotone, so |fl(xi - xj)| >= g for
// every point i of one box and j of the other; squares and the two sums are monotone as well.  Hence the value returned is
// <= the d2 the scan computes for ANY such pair: a chunk with box_d2 > bound holds no candidate with d2 <= bound, not even
// one that ties.  No margin is needed and no bit of the result depends on the skip.
__device__ __forceinline__ float box_d2(const Box &a, const Box &b) {
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = fmaxf(0.f, fmaxf(a.lo[c] - b.hi[c], b.lo[c] - a.hi[c]));
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

__device__ __forceinline__ Box load_box(const float *__restrict__ boxes, long long at) {
  Box b;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b.lo[c] = boxes[at * 6 + c];
    b.hi[c] = boxes[at * 6 + 3 + c];
  }
  return b;
}

// v[0..2] / v[3..5] -> the minimum / maximum over the wave, in every lane.
__device__ __forceinline__ void wave_minmax(float (&v)[6]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = fminf(v[c], __shfl_xor(v[c], off));
      v[c + 3] = fmaxf(v[c + 3], __shfl_xor(v[c + 3], off));
    }
  }
}

// The box (lo xyz, hi xyz -> out[6]) of the cnt >= 1 rows at src, by one workgroup of kChunk lanes.
__device__ __forceinline__ void chunk_box_body(const float *__restrict__ src, int cnt, float *__restrict__ out) {
  __shared__ float red[kChunk / 64][6];
  const int tid = threadIdx.x;
  const int i = min(tid, cnt - 1);   // a lane past the end repeats the last point
  float v[6];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = v[c + 3] = src[i * 3 + c];
  wave_minmax(v);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) red[tid >> 6][c] = v[c];
  }
  __syncthreads();
  if (tid < 6) {
    float r = red[0][tid];
#pragma unroll
    for (int w = 1; w < kChunk / 64; ++w) r = tid < 3 ? fminf(r, red[w][tid]) : fmaxf(r, red[w][tid]);
    out[tid] = r;
  }
}

// The box of the wave's query points.
__device__ __forceinline__ Box wave_query_box(float qx, float qy, float qz) {
  float v[6] = {qx, qy, qz, qx, qy, qz};
  wave_minmax(v);
  Box b;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b.lo[c] = v[c];
    b.hi[c] = v[c + 3];
  }
  return b;
}

// Stage the cnt rows at src into LDS (coalesced dword loads of the [n,3] rows), between two barriers: the previous chunk
// has been read by every wave before, the new one is visible to every wave after.
__device__ __forceinline__ void stage_chunk(float *__restrict__ pts, const float *__restrict__ src, int cnt) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int f = tid + c * kChunk;
    if (f < cnt * 3) pts[f] = src[f];
  }
  __syncthreads();
}

// One candidate against every lane's KT smallest keys, sorted in registers (fully unrolled: no run-time register index).
// `in`: this lane offers cand and cand < key[KT - 1].  Most candidates end at the ballot: one compare.
template <typename Key, int KT>
__device__ __forceinline__ void insert_key(Key (&key)[KT], Key cand, bool in) {
  if (__ballot(in) != 0ull) {
    Key carry = in ? cand : ~(Key)0;
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      const bool lt = carry < key[s];
      const Key lo = lt ? carry : key[s];
      carry = lt ? key[s] : carry;
      key[s] = lo;
    }
  }
}

// The largest value over the wave of a per-lane d2 bit pattern (non-negative floats order like their bits).
__device__ __forceinline__ uint32_t wave_max_bits(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
  return v;
}

}  // namespace
