// ball_query.h -- the ball-query scan of neighbors.hip, once: ball_query_multi_kernel (gldm_ball_query is its one-scale
// launch) and sa_group_kernel run this body, so they cannot decide differently about a point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kWave = 64;
constexpr int kBqBlock = 256;             // one wave per centre, kBqBlock / kWave centres at a time
constexpr int kBqCentresPerBlock = 16;
constexpr int kBqMaxLdsPoints = 5120;     // 60 KiB of coordinates
constexpr int kBqLdsBytes = 64 * 1024;    // what a launch gets without raising the kernel's dynamic-LDS limit
constexpr int kMaxScales = 4;

// Whether a block stages its cloud's coordinates in LDS, given the dynamic LDS its kernel needs for everything else.
// False sends the launch to the form that reads the points through L2: a request past 64 KiB is never made.
inline bool bq_stage_points(int n, size_t other_lds_bytes) {
  return n <= kBqMaxLdsPoints && other_lds_bytes + (size_t)3 * n * sizeof(float) <= (size_t)kBqLdsBytes;
}

// The cloud's [3][n] coordinates: copied into `lds` by the block's kBqBlock threads (kStage; the caller's barrier
// follows), or left where they are.
struct BqPoints {
  const float *x, *y, *z;
};

template <bool kStage>
__device__ __forceinline__ BqPoints bq_points(const float *points, int n, float *lds) {
  if (kStage) {
    for (int i = threadIdx.x; i < 3 * n; i += kBqBlock) lds[i] = points[i];
    points = lds;
  }
  return {points, points + n, points + 2 * n};
}

// One wave scans the cloud for one centre and S radii, 64 candidates per step.  The squared distance
// (cx - x)^2 + (cy - y)^2 + (cz - z)^2 is computed once per point, products and sums rounding once each in this order
// (-ffp-contract=off), and a point is inside a ball when it is strictly '<' r2[s].  Each scale keeps its own ballot,
// prefix popcount and count: o[s] receives the first u[s] hits in index order, and the slots that are left are filled
// with the first hit (0 for an empty ball).  The scan ends when every scale is full.
template <int S>
__device__ __forceinline__ void ball_query_scan(const BqPoints p, int n, float cx, float cy, float cz, const float *r2,
                                                const int *u, int32_t *const *o, int lane) {
  int cnt[S], first[S];
#pragma unroll
  for (int s = 0; s < S; ++s) cnt[s] = first[s] = 0;
  auto open = [&] {   // wave-uniform: some scale still has room
    bool any = cnt[0] < u[0];
#pragma unroll
    for (int s = 1; s < S; ++s) any |= cnt[s] < u[s];
    return any;
  };
  for (int base = 0; base < n && open(); base += kWave) {
    const int k = base + lane;
    bool hit[S] = {};
    if (k < n) {
      const float dx = cx - p.x[k];
      const float dy = cy - p.y[k];
      const float dz = cz - p.z[k];
      const float d2 = dx * dx + dy * dy + dz * dz;
#pragma unroll
      for (int s = 0; s < S; ++s) hit[s] = d2 < r2[s];
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (S == 1 || cnt[s] < u[s]) {   // a full scale has ended its scan (at one scale that is the loop's own test)
        const unsigned long long mask = __ballot(hit[s]);
        if (mask != 0ull) {
          if (cnt[s] == 0) first[s] = base + __ffsll((long long)mask) - 1;
          const int slot = cnt[s] + __popcll(mask & ((1ull << lane) - 1ull));
          if (hit[s] && slot < u[s]) o[s][slot] = k;
          cnt[s] += __popcll(mask);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int c = cnt[s] < u[s] ? cnt[s] : u[s];
    const int fill = first[s];  // 0 when the ball is empty
    for (int v = c + lane; v < u[s]; v += kWave) o[s][v] = fill;
  }
}

// The scan at one scale.
__device__ __forceinline__ void ball_query_one(const BqPoints p, int n, float cx, float cy, float cz, float r2, int u,
                                               int32_t *o, int lane) {
  ball_query_scan<1>(p, n, cx, cy, cz, &r2, &u, &o, lane);
}

}  // namespace
