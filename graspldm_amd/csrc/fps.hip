// fps.hip -- the farthest-point family for gfx950, behind the C ABI declared in include/gldm.h: the reference's CUDA sampler
// (gldm_furthest_point_sampling), its host-side greedy sampler (gldm_farthest_points_euclid), the same on clouds beyond
// one workgroup's registers (gldm_farthest_points_euclid_large) and on clouds of different sizes packed in one array
// (gldm_farthest_points_euclid_ragged).
//
// Three forms, ONE key and one arithmetic, so that a cloud gets the same picks from every form:
//  * fps_wave_kernel   one wave per cloud (n <= 1024), no LDS exchange and no barrier in the round;
//  * fps_block_rounds  one workgroup per cloud (n <= 8192): coordinates and running distances in registers/LDS for all M
//                      rounds, one barrier per round (fps_kernel, fps_ragged_block_kernel);
//  * fps_round         one launch per round over slices of the cloud (fps_large_round_kernel, fps_ragged_round_kernel).
// Compiled with -ffp-contract=off: the picks depend on every product and every sum of a distance rounding once, like the
// scalar oracle's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_util.h"

namespace {

constexpr int kWave = 64;

// ------------------------------------------------------- the key, the rules --
// Round winner = arg-max of a 64-bit key: high word = distance bits (distances are >= +0 so the bit pattern is monotone),
// low word = the tie word of the rule.  The low word of a real key is never 0, so key 0 is below every real key.
// kRule 0: the reference's CUDA kernel (sampling.cu:86-167): coords [3][n], squared distances, start 1e38; tie word
//          ~((k mod 512) << 22 | k), which reproduces the reference's tie resolution (strict '>' inside a 512-stride scan,
//          strict '<' in the shared-memory tree -> lowest slot, then lowest k).
// kRule 1: the reference's host-side greedy sampler PointCloudHelpers.farthest_points
//          (grasp_ldm/utils/pointcloud_helpers.py:160-217, used by regularize_pc_point_count :124-158):
//          points [n][3], EUCLIDEAN distance sqrt((dx^2 + dy^2) + dz^2) in f32 (numpy's summation order),
//          start 1e7, tie word ~k: np.argmax's tie rule = lowest index.
constexpr int kFpsMaxPerThread = 8;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// ------------------------------------------------- one workgroup per cloud --
// Thread t owns points t, t+T, t+2T, ... (kept in registers together with their running min-distance); the previous
// winner's coordinates come from LDS.  `coords` is the cloud's base, `out` its row of m picks.
template <int kThreads, int kPerThread, int kRule>
__device__ __forceinline__ void fps_block_rounds(const float *coords, int n, int m, int32_t *out, float *s_xyz,
                                                 unsigned long long (*s_part)[kThreads / kWave]) {
  const int tid = threadIdx.x;
  if (kRule == 0) {
    for (int i = tid; i < 3 * n; i += kThreads) s_xyz[i] = coords[i];
  } else {
    for (int i = tid; i < 3 * n; i += kThreads) s_xyz[(i % 3) * n + i / 3] = coords[i];
  }
  float x[kPerThread], y[kPerThread], z[kPerThread], dist[kPerThread];
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int k = tid + q * kThreads;
    const bool ok = k < n;
    x[q] = ok ? coords[kRule == 0 ? k : 3 * k] : 0.f;
    y[q] = ok ? coords[kRule == 0 ? k + n : 3 * k + 1] : 0.f;
    z[q] = ok ? coords[kRule == 0 ? k + 2 * n : 3 * k + 2] : 0.f;
    dist[q] = kRule == 0 ? 1e38f : 1e7f;
  }
  if (tid == 0) out[0] = 0;
  __syncthreads();
  int old = 0;
  const int wave = tid >> 6, lane = tid & 63;
  constexpr int kWaves = kThreads / kWave;
  for (int j = 1; j < m; ++j) {
    const float x1 = s_xyz[old], y1 = s_xyz[old + n], z1 = s_xyz[old + 2 * n];
    unsigned long long best = 0ull;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int k = tid + q * kThreads;
      if (k < n) {
        float d = (x[q] - x1) * (x[q] - x1) + (y[q] - y1) * (y[q] - y1) + (z[q] - z1) * (z[q] - z1);
        if (kRule == 1) d = __fsqrt_rn(d);
        const float d2 = d < dist[q] ? d : dist[q];
        dist[q] = d2;
        const unsigned int tie = kRule == 0 ? ~(((unsigned int)(k & 511) << 22) | (unsigned int)k) : ~(unsigned int)k;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | tie;
        best = key > best ? key : best;
      }
    }
    best = wave_max_u64(best);
    if (kWaves > 1) {
      if (lane == 0) s_part[j & 1][wave] = best;
      __syncthreads();
      unsigned long long v = lane < kWaves ? s_part[j & 1][lane] : 0ull;
#pragma unroll
      for (int off = kWaves / 2; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, kWave);
        v = o > v ? o : v;
      }
      best = __shfl(v, 0, kWave);
    }
    old = (int)((~(unsigned int)best) & 0x3FFFFFu);
    if (tid == 0) out[j] = old;
  }
}

template <int kThreads, int kPerThread, int kRule>
__global__ __launch_bounds__(kThreads) void fps_kernel(const float *__restrict__ coords, int n, int m,
                                                       int32_t *__restrict__ out) {
  extern __shared__ float s_xyz[];  // [3][n]
  __shared__ unsigned long long s_part[2][kThreads / kWave];
  const int b = blockIdx.x;
  fps_block_rounds<kThreads, kPerThread, kRule>(coords + (size_t)b * 3 * n, n, m, out + (size_t)b * m, s_xyz, s_part);
}

// ------------------------------------------------------ one wave per cloud --
// n <= 1024: lane l owns points l, l + 64, ... (kPer of them, in registers with their running min-distances), so a round
// is 10 VALU instructions per point, an in-lane arg-max and ONE wave reduction -- no LDS exchange, no barrier (the 16-wave
// form above spends most of a round's 1.2 us in its two reductions and the barrier between them: 0.62 ms per 1024 -> 512
// sampling whatever the batch).  The reduction runs on the two 32-bit halves of the key one after the other (distance
// bits, then the tie word among the lanes that hold the maximal distance): four DPP row steps + four v_readlane each.  The
// previous winner's coordinates come from LDS (a broadcast read).
template <int CTRL>
__device__ __forceinline__ unsigned dpp_shr_u32(unsigned v) {   // lanes without a source read 0 (the identity of max)
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  v = max(v, dpp_shr_u32<0x111>(v));   // row_shr:1
  v = max(v, dpp_shr_u32<0x112>(v));   // row_shr:2
  v = max(v, dpp_shr_u32<0x114>(v));   // row_shr:4
  v = max(v, dpp_shr_u32<0x118>(v));   // row_shr:8: lane 15 of every row holds the row's maximum
  const unsigned a = __builtin_amdgcn_readlane(v, 15), b = __builtin_amdgcn_readlane(v, 31);
  const unsigned c = __builtin_amdgcn_readlane(v, 47), d = __builtin_amdgcn_readlane(v, 63);
  return max(max(a, b), max(c, d));
}
template <int kPer, int kRule>
__global__ __launch_bounds__(64) void fps_wave_kernel(const float *__restrict__ coords, int n, int m,
                                                      int32_t *__restrict__ out) {
  extern __shared__ float s_xyz[];  // [3][n]
  const int b = blockIdx.x, lane = threadIdx.x;
  coords += (size_t)b * 3 * n;
  out += (size_t)b * m;
  // Slots beyond n: distance 0 for ever (min(d, 0) = 0) and tie word 0, i.e. key 0: the round needs no per-point test
  // (16 exec-masked branches per round otherwise).
  float x[kPer], y[kPer], z[kPer], dist[kPer];
  unsigned tiew[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int k = lane + 64 * q;
    const bool ok = k < n;
    x[q] = ok ? coords[kRule == 0 ? k : 3 * k] : 0.f;
    y[q] = ok ? coords[kRule == 0 ? k + n : 3 * k + 1] : 0.f;
    z[q] = ok ? coords[kRule == 0 ? k + 2 * n : 3 * k + 2] : 0.f;
    dist[q] = ok ? (kRule == 0 ? 1e38f : 1e7f) : 0.f;
    const unsigned int tie = kRule == 0 ? ~(((unsigned int)(k & 511) << 22) | (unsigned int)k) : ~(unsigned int)k;
    tiew[q] = ok ? tie : 0u;
    if (ok) {
      s_xyz[k] = x[q];
      s_xyz[k + n] = y[q];
      s_xyz[k + 2 * n] = z[q];
    }
  }
  if (lane == 0) out[0] = 0;
  __syncthreads();
  int old = 0;
  for (int j = 1; j < m; ++j) {
    const float x1 = s_xyz[old], y1 = s_xyz[old + n], z1 = s_xyz[old + 2 * n];
    unsigned long long best = 0ull;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      float d = (x[q] - x1) * (x[q] - x1) + (y[q] - y1) * (y[q] - y1) + (z[q] - z1) * (z[q] - z1);
      if (kRule == 1) d = __fsqrt_rn(d);
      const float d2 = d < dist[q] ? d : dist[q];
      dist[q] = d2;
      const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | tiew[q];
      best = key > best ? key : best;
    }
    const unsigned hi = (unsigned)(best >> 32), lo = (unsigned)best;
    const unsigned hmax = wave_max_u32(hi);
    const unsigned lmax = wave_max_u32(hi == hmax ? lo : 0u);
    old = (int)((~lmax) & 0x3FFFFFu);
    if (lane == 0) out[j] = old;
  }
}

// --------------------------------------------------- one launch per round --
// Rule-1 selection on clouds beyond one workgroup's registers (8192 < n <= 2^22): a cloud is cut into runs of `slice`
// consecutive points, one workgroup each, and a round is ONE LAUNCH over (slices, b) -- the grid-wide decision of a round
// happens at the launch boundary, no workgroup ever waits for another.  Launch r, in the workgroup of slice s (fps_round):
//   1. it reduces the `live` partial keys that launch r-1 left (one per slice, at most kFpsLargeMaxSlices; exact:
//      the key above) to pick r (r = 0: index 0) -- every workgroup redundantly, which costs a few hundred L2 reads and
//      saves a launch; slice 0 writes out[r];
//   2. unless r is the last round, it updates its slice's running minima `mind` (global workspace, start 1e7 taken as a
//      constant in launch 0, so the workspace needs no initialisation) with the distance to pick r and leaves its own
//      partial key in the other half of the double-buffered partials.
// Slice i is workgroup i in every round, so a slice's points and minima are re-read by the same XCD's L2 each round.
// `points` is the cloud's base, `cnt` (> m) its live rows: rows past it are never read, and a slice that starts at or past
// it leaves key 0.
constexpr int kFpsLargeBlock = 256;
constexpr int kFpsLargeMinSlice = 1024;
constexpr int kFpsLargeMaxSlices = 512;
constexpr int kFpsLargeMaxN = 1 << 22;   // the index field of the key
constexpr int kFpsLargeMaxM = 8192;

__device__ __forceinline__ void fps_round(const float *points, int cnt, int live, int slice, float *mind,
                                          unsigned long long *partials, int r, int m, int32_t *out,
                                          unsigned long long *s_part) {
  const int s = blockIdx.x, slices = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  const unsigned long long *prev = partials + ((size_t)((r + 1) & 1) * gridDim.y + b) * slices;   // [2][clouds][slices]
  unsigned long long *mine = partials + ((size_t)(r & 1) * gridDim.y + b) * slices;
  int pick = 0;
  if (r > 0) {
    unsigned long long v = 0ull;
    for (int i = tid; i < live; i += kFpsLargeBlock) {
      const unsigned long long o = prev[i];
      v = o > v ? o : v;
    }
    v = wave_max_u64(v);
    if ((tid & 63) == 0) s_part[tid >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kFpsLargeBlock / kWave; ++w) v = s_part[w] > v ? s_part[w] : v;
    pick = (int)((~(unsigned int)v) & 0x3FFFFFu);   // < cnt: only live rows ever left a non-zero key
    __syncthreads();
  }
  if (s == 0 && tid == 0) out[r] = pick;
  if (r == m - 1) return;
  const float x1 = points[3 * (size_t)pick], y1 = points[3 * (size_t)pick + 1], z1 = points[3 * (size_t)pick + 2];
  const int k0 = s * slice;
  const int k1 = (k0 + slice < cnt) ? k0 + slice : cnt;
  unsigned long long best = 0ull;
  for (int k = k0 + tid; k < k1; k += kFpsLargeBlock) {
    const float x = points[3 * (size_t)k], y = points[3 * (size_t)k + 1], z = points[3 * (size_t)k + 2];
    const float d = __fsqrt_rn((x - x1) * (x - x1) + (y - y1) * (y - y1) + (z - z1) * (z - z1));
    const float old = r == 0 ? 1e7f : mind[k];
    const float d2 = d < old ? d : old;
    mind[k] = d2;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | ~(unsigned int)k;
    best = key > best ? key : best;
  }
  best = wave_max_u64(best);
  if ((tid & 63) == 0) s_part[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kFpsLargeBlock / kWave; ++w) best = s_part[w] > best ? s_part[w] : best;
    mine[s] = best;
  }
}

// Clouds of one row stride n.  `counts` (optional): the live rows of each cloud; a cloud with counts[b] <= m gets
// 0 .. counts[b]-1 then -1 (the reference's nclusters >= N -> arange case).
__global__ __launch_bounds__(kFpsLargeBlock) void fps_large_round_kernel(const float *__restrict__ points, int n, int m,
                                                                         int slice, const int32_t *__restrict__ counts,
                                                                         float *__restrict__ mind,
                                                                         unsigned long long *__restrict__ partials, int r,
                                                                         int32_t *__restrict__ out) {
  __shared__ unsigned long long s_part[kFpsLargeBlock / kWave];
  const int s = blockIdx.x, slices = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  int cnt = counts ? counts[b] : n;
  cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
  out += (size_t)b * m;
  if (cnt <= m) {
    if (s == 0 && tid == 0) out[r] = r < cnt ? r : -1;
    return;
  }
  fps_round(points + (size_t)b * 3 * n, cnt, slices, slice, mind + (size_t)b * n, partials, r, m, out, s_part);
}

// Clouds of DIFFERENT sizes packed in one [rows, 3] array (gldm_farthest_points_euclid_ragged): cloud b is rows
// start[b] .. start[b] + min(count[b], n_max), and every cloud gets the picks it would get alone:
//   fps_ragged_block_kernel  one workgroup per cloud for counts <= 8192 (fps_block_rounds<1024, 8, 1> with the live row
//                            count read per cloud, LDS sized for min(n_max, 8192) rows); also writes the 0 .. count-1, -1
//                            rows of the clouds with count <= m.  Workgroups of larger clouds leave at once.
//   fps_ragged_round_kernel  fps_round over (slices(n_max), b) for counts > 8192 (> m, always); minima [b, n_max];
//                            workgroups of smaller clouds and of slices past the count leave at once, and the partials of
//                            those slices are never read.
constexpr int kFpsRaggedThreads = 1024;
constexpr int kFpsBlockMaxN = kFpsRaggedThreads * kFpsMaxPerThread;   // 8192

__device__ __forceinline__ int ragged_count(const int32_t *__restrict__ count, int b, int n_max) {
  const int c = count[b];
  return c < 0 ? 0 : (c > n_max ? n_max : c);
}

__global__ __launch_bounds__(kFpsRaggedThreads) void fps_ragged_block_kernel(const float *__restrict__ points,
                                                                             const int32_t *__restrict__ start,
                                                                             const int32_t *__restrict__ count, int n_max,
                                                                             int m, int32_t *__restrict__ out) {
  extern __shared__ float s_xyz[];  // [3][n], n <= min(n_max, 8192)
  __shared__ unsigned long long s_part[2][kFpsRaggedThreads / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = ragged_count(count, b, n_max);
  if (n > kFpsBlockMaxN) return;   // the round launches serve it
  out += (size_t)b * m;
  if (n <= m) {
    for (int j = tid; j < m; j += kFpsRaggedThreads) out[j] = j < n ? j : -1;
    return;
  }
  fps_block_rounds<kFpsRaggedThreads, kFpsMaxPerThread, 1>(points + 3 * (size_t)start[b], n, m, out, s_xyz, s_part);
}

__global__ __launch_bounds__(kFpsLargeBlock) void fps_ragged_round_kernel(const float *__restrict__ points,
                                                                          const int32_t *__restrict__ start,
                                                                          const int32_t *__restrict__ count, int n_max, int m,
                                                                          int slice, float *__restrict__ mind,
                                                                          unsigned long long *__restrict__ partials, int r,
                                                                          int32_t *__restrict__ out) {
  __shared__ unsigned long long s_part[kFpsLargeBlock / kWave];
  const int s = blockIdx.x, b = blockIdx.y;
  const int cnt = ragged_count(count, b, n_max);
  if (cnt <= kFpsBlockMaxN) return;   // the one-workgroup form served it
  const int live = (cnt + slice - 1) / slice;   // slices that hold rows
  if (s >= live) return;
  fps_round(points + 3 * (size_t)start[b], cnt, live, slice, mind + (size_t)b * n_max, partials, r, m,
            out + (size_t)b * m, s_part);
}

// ------------------------------------------------------------ host side ----
template <int kThreads, int kPerThread, int kRule>
int launch_fps(const float *coords, int b, int n, int m, int32_t *out, hipStream_t s) {
  hipLaunchKernelGGL((fps_kernel<kThreads, kPerThread, kRule>), dim3(b), dim3(kThreads), (size_t)3 * n * sizeof(float),
                     s, coords, n, m, out);
  return launch_status();
}
template <int kPer, int kRule>
int launch_fps_wave(const float *coords, int b, int n, int m, int32_t *out, hipStream_t s) {
  hipLaunchKernelGGL((fps_wave_kernel<kPer, kRule>), dim3(b), dim3(64), (size_t)3 * n * sizeof(float), s, coords, n, m, out);
  return launch_status();
}
template <int kRule>
int dispatch_fps(const float *coords, int b, int n, int m, int32_t *out_idx, hipStream_t s) {
  // up to 1024 points: one wave per cloud, no barrier in the round (fps_wave_kernel)
  if (n <= 64) return launch_fps_wave<1, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 128) return launch_fps_wave<2, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 256) return launch_fps_wave<4, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 512) return launch_fps_wave<8, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 1024) return launch_fps_wave<16, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 2048) return launch_fps<1024, 2, kRule>(coords, b, n, m, out_idx, s);
  if (n <= 4096) return launch_fps<1024, 4, kRule>(coords, b, n, m, out_idx, s);
  return launch_fps<1024, 8, kRule>(coords, b, n, m, out_idx, s);
}

// 0, or the status of a shape outside the envelope of the round launches; n_min: the smallest row stride the entry takes
int fps_rounds_check(int b, int n, int m, int n_min) {
  if (b <= 0 || n <= 0 || m < 0) return GLDM_ERR_INVALID_ARG;
  if (n < n_min || n > kFpsLargeMaxN || m > kFpsLargeMaxM || b > 65535) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}
int fps_large_slice(int n) {
  int slice = kFpsLargeMinSlice;
  while (ceil_div(n, slice) > kFpsLargeMaxSlices) slice *= 2;
  return slice;
}
// The workspace of the round launches over b clouds of row stride n: minima [b][n] f32, padded to 8 bytes, then the
// partials [2][b][slices] u64.
long long fps_minima_bytes(int b, int n) { return (((long long)b * n * 4) + 7) / 8 * 8; }
long long fps_rounds_workspace_bytes(int b, int n) {
  return fps_minima_bytes(b, n) + 2ll * b * ceil_div(n, fps_large_slice(n)) * (long long)sizeof(unsigned long long);
}
// Carve the workspace and enqueue the m round launches back to back (no synchronisation here); launch(grid, slice,
// minima, partials, r) enqueues round r.
template <typename Launch>
int fps_enqueue_rounds(int b, int n, int m, void *workspace, Launch launch) {
  const int slice = fps_large_slice(n);
  const dim3 grid(ceil_div(n, slice), b);
  float *mind = static_cast<float *>(workspace);
  unsigned long long *partials = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + fps_minima_bytes(b, n));
  for (int r = 0; r < m; ++r) {
    launch(grid, slice, mind, partials, r);
    const int ls = launch_status();
    if (ls != GLDM_OK) return ls;
  }
  return GLDM_OK;
}

}  // namespace

// =========================================================== C ABI =========

GLDM_API int gldm_furthest_point_sampling(const float *coords, int b, int n, int m, int32_t *out_idx,
                                          gldm_stream_t stream) {
  if (!coords || !out_idx || b <= 0 || n <= 0 || m < 0) return GLDM_ERR_INVALID_ARG;
  if (m == 0) return GLDM_OK;
  if (n > kFpsBlockMaxN) return GLDM_ERR_UNSUPPORTED;
  return dispatch_fps<0>(coords, b, n, m, out_idx, as_stream(stream));
}

GLDM_API int gldm_farthest_points_euclid(const float *points, int b, int n, int m, int32_t *out_idx,
                                         gldm_stream_t stream) {
  if (!points || !out_idx || b <= 0 || n <= 0 || m < 0 || m > n) return GLDM_ERR_INVALID_ARG;
  if (m == 0) return GLDM_OK;
  if (n > kFpsBlockMaxN) return GLDM_ERR_UNSUPPORTED;
  return dispatch_fps<1>(points, b, n, m, out_idx, as_stream(stream));
}

GLDM_API int gldm_farthest_points_euclid_large_slice(int n) {
  if (n <= kFpsBlockMaxN || n > kFpsLargeMaxN) return GLDM_ERR_UNSUPPORTED;
  return fps_large_slice(n);
}

GLDM_API long long gldm_farthest_points_euclid_large_workspace_bytes(int b, int n) {
  const int st = fps_rounds_check(b, n, 1, kFpsBlockMaxN + 1);
  return st != GLDM_OK ? st : fps_rounds_workspace_bytes(b, n);
}

GLDM_API int gldm_farthest_points_euclid_large(const float *points, const int32_t *counts, int b, int n, int m,
                                               void *workspace, long long workspace_bytes, int32_t *out_idx,
                                               gldm_stream_t stream) {
  const int st = fps_rounds_check(b, n, m, kFpsBlockMaxN + 1);   // the envelope before any pointer
  if (st != GLDM_OK) return st;
  if (m > n) return GLDM_ERR_INVALID_ARG;
  if (!points || !out_idx || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return GLDM_ERR_INVALID_ARG;
  if (m == 0) return GLDM_OK;
  if (workspace_bytes < fps_rounds_workspace_bytes(b, n)) return GLDM_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  return fps_enqueue_rounds(b, n, m, workspace, [&](dim3 grid, int slice, float *mind, unsigned long long *partials, int r) {
    hipLaunchKernelGGL(fps_large_round_kernel, grid, dim3(kFpsLargeBlock), 0, s, points, n, m, slice, counts, mind,
                       partials, r, out_idx);
  });
}

GLDM_API long long gldm_farthest_points_euclid_ragged_workspace_bytes(int b, int n_max) {
  const int st = fps_rounds_check(b, n_max, 1, 1);
  if (st != GLDM_OK) return st;
  return n_max <= kFpsBlockMaxN ? 0 : fps_rounds_workspace_bytes(b, n_max);
}

GLDM_API int gldm_farthest_points_euclid_ragged(const float *points, const int32_t *start, const int32_t *count, int b,
                                                int n_max, int m, void *workspace, long long workspace_bytes,
                                                int32_t *out_idx, gldm_stream_t stream) {
  const int st = fps_rounds_check(b, n_max, m, 1);   // the envelope before any pointer
  if (st != GLDM_OK) return st;
  const bool large = n_max > kFpsBlockMaxN;
  if (!points || !start || !count || !out_idx) return GLDM_ERR_INVALID_ARG;
  if (large && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u))) return GLDM_ERR_INVALID_ARG;
  if (m == 0) return GLDM_OK;
  if (large && workspace_bytes < fps_rounds_workspace_bytes(b, n_max)) return GLDM_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  const int lds_rows = large ? kFpsBlockMaxN : n_max;
  hipLaunchKernelGGL(fps_ragged_block_kernel, dim3(b), dim3(kFpsRaggedThreads), (size_t)3 * lds_rows * sizeof(float), s,
                     points, start, count, n_max, m, out_idx);
  const int ls = launch_status();
  if (ls != GLDM_OK || !large) return ls;
  return fps_enqueue_rounds(b, n_max, m, workspace, [&](dim3 grid, int slice, float *mind, unsigned long long *partials, int r) {
    hipLaunchKernelGGL(fps_ragged_round_kernel, grid, dim3(kFpsLargeBlock), 0, s, points, start, count, n_max, m, slice,
                       mind, partials, r, out_idx);
  });
}
