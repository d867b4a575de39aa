// sa_msg.hip -- gfx950 kernels of the multi-scale set-abstraction module (PointNetSAModule with more than one radius:
// pointnet.py:49-114), behind the C ABI declared in include/gldm.h.
//
//  * gldm_ball_query_multi: ONE scan of a cloud's points per centre for up to four radii.  One wave per centre as in
//    point_ops.hip's ball_query_kernel; the squared distance is computed once per point, each scale keeps its own ballot,
//    prefix popcount and count, and the scan ends when every scale is full.  Same expression, same strict '<', same fill
//    rule: bit-identical to one gldm_ball_query per radius.  Compiled with -ffp-contract=off like point_ops.hip.
//  * gldm_group_max_concat: the maximum over h consecutive columns, written into a row range of the module's
//    concatenated output.  h > 1 folds the sub-centres of a U = 64 h neighbourhood that ran on the 64-column fused
//    kernels as h centres; h = 1 is the strided copy that stands in for torch.cat.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gldm.h"

#define GLDM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kWave = 64;
constexpr int kBqBlock = 256;
constexpr int kBqMaxLdsPoints = 5120;  // 60 KiB: the staging limit of ball_query_kernel
constexpr int kBqCentresPerBlock = 16;
constexpr int kMaxScales = 4;

inline int launch_status() { return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH; }
inline hipStream_t as_stream(gldm_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

struct BqScales {
  float r2[kMaxScales];
  int u[kMaxScales];
  int32_t *out[kMaxScales];  // [b, m, u_s]
};

template <int S>
__device__ __forceinline__ void ball_query_multi_wave(const float *px, const float *py, const float *pz, int n, float cx,
                                                      float cy, float cz, const BqScales &a, size_t centre, int lane) {
  int cnt[S], first[S];
  int32_t *o[S];
  bool open = false;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    cnt[s] = 0;
    first[s] = 0;
    o[s] = a.out[s] + centre * (size_t)a.u[s];
    open = open || a.u[s] > 0;
  }
  for (int base = 0; base < n && open; base += kWave) {
    const int k = base + lane;
    float d2 = 0.f;
    if (k < n) {
      const float dx = cx - px[k];
      const float dy = cy - py[k];
      const float dz = cz - pz[k];
      d2 = dx * dx + dy * dy + dz * dz;
    }
    open = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      if (cnt[s] < a.u[s]) {   // wave-uniform: a full scale has ended its scan, as the single-radius loop does
        const bool hit = k < n && d2 < a.r2[s];
        const unsigned long long mask = __ballot(hit);
        if (mask != 0ull) {
          if (cnt[s] == 0) first[s] = base + __ffsll((long long)mask) - 1;
          const int slot = cnt[s] + __popcll(mask & ((1ull << lane) - 1ull));
          if (hit && slot < a.u[s]) o[s][slot] = k;
          cnt[s] += __popcll(mask);
        }
        open = open || cnt[s] < a.u[s];
      }
    }
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int c = cnt[s] < a.u[s] ? cnt[s] : a.u[s];
    const int fill = first[s];  // 0 when the ball is empty
    for (int v = c + lane; v < a.u[s]; v += kWave) o[s][v] = fill;
  }
}

template <bool kUseLds, int S>
__global__ __launch_bounds__(kBqBlock) void ball_query_multi_kernel(const float *__restrict__ centers,
                                                                    const float *__restrict__ points, int n, int m,
                                                                    BqScales a) {
  extern __shared__ float s_pts[];
  const int b = blockIdx.y;
  points += (size_t)b * 3 * n;
  centers += (size_t)b * 3 * m;
  const float *px = points, *py = points + n, *pz = points + 2 * n;
  if (kUseLds) {
    for (int i = threadIdx.x; i < 3 * n; i += kBqBlock) s_pts[i] = points[i];
    __syncthreads();
    px = s_pts;
    py = s_pts + n;
    pz = s_pts + 2 * n;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * kBqCentresPerBlock;
  const int j1 = min(j0 + kBqCentresPerBlock, m);
  for (int j = j0 + wave; j < j1; j += kBqBlock / kWave) {
    ball_query_multi_wave<S>(px, py, pz, n, centers[j], centers[j + m], centers[j + 2 * m], a, (size_t)b * m + j, lane);
  }
}

template <int S>
void launch_ball_query_multi(const float *centers, const float *points, int b, int n, int m, const BqScales &a,
                             hipStream_t s) {
  dim3 grid(ceil_div(m, kBqCentresPerBlock), b);
  if (n <= kBqMaxLdsPoints) {
    hipLaunchKernelGGL((ball_query_multi_kernel<true, S>), grid, dim3(kBqBlock), (size_t)3 * n * sizeof(float), s, centers,
                       points, n, m, a);
  } else {
    hipLaunchKernelGGL((ball_query_multi_kernel<false, S>), grid, dim3(kBqBlock), 0, s, centers, points, n, m, a);
  }
}

// ------------------------------------------------------- fold + concatenate --
// Thread = 4 consecutive output columns of one (cloud, row): 4 H input floats; a block's 256 threads run over the
// flattened (row, column quad) items of a cloud, so short rows (M = 128: 32 quads) still fill it.  16-byte loads when the
// input rows are 16-byte aligned (m h a multiple of 4), 16-byte stores when the output rows are (m a multiple of 4).
constexpr int kFoldBlock = 256;

__device__ __forceinline__ float max4(const float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }

template <int H>
__global__ __launch_bounds__(kFoldBlock) void group_max_concat_kernel(const float *__restrict__ part, int c, int m,
                                                                      float *__restrict__ out, int c0, int ctot,
                                                                      int in_vec, int out_vec) {
  const int quads = (m + 3) >> 2;
  const long long item = (long long)blockIdx.x * kFoldBlock + threadIdx.x;
  if (item >= (long long)c * quads) return;
  const int row = (int)(item / quads), j = (int)(item % quads) * 4, b = blockIdx.y;
  const float *src = part + ((size_t)b * c + row) * ((size_t)m * H) + (size_t)j * H;
  float *dst = out + ((size_t)b * ctot + c0 + row) * (size_t)m + j;
  const bool whole = j + 3 < m;
  float r[4];
  if (whole && in_vec) {
    if (H == 1) {
      const float4 v = *reinterpret_cast<const float4 *>(src);
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else if (H == 2) {
      const float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 4);
      r[0] = fmaxf(v0.x, v0.y); r[1] = fmaxf(v0.z, v0.w); r[2] = fmaxf(v1.x, v1.y); r[3] = fmaxf(v1.z, v1.w);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] = max4(*reinterpret_cast<const float4 *>(src + 4 * q));
    }
  } else {
    const int live = whole ? 4 : m - j;
    for (int q = 0; q < live; ++q) {
      float v = src[q * H];
#pragma unroll
      for (int t = 1; t < H; ++t) v = fmaxf(v, src[q * H + t]);
      r[q] = v;
    }
  }
  if (whole && out_vec) {
    *reinterpret_cast<float4 *>(dst) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    const int live = whole ? 4 : m - j;
    for (int q = 0; q < live; ++q) dst[q] = r[q];
  }
}

}  // namespace

GLDM_API int gldm_ball_query_multi(const float *centers, const float *points, int b, int n, int m, int n_scales,
                                   const float *radius, const int32_t *u, int32_t *const *out, gldm_stream_t stream) {
  if (!centers || !points || !radius || !u || !out || b <= 0 || n <= 0 || m <= 0) return GLDM_ERR_INVALID_ARG;
  if (n_scales < 1 || n_scales > kMaxScales) return GLDM_ERR_UNSUPPORTED;
  if (b > 65535) return GLDM_ERR_UNSUPPORTED;
  BqScales a{};
  for (int s = 0; s < n_scales; ++s) {
    if (!out[s] || u[s] <= 0) return GLDM_ERR_INVALID_ARG;
    a.r2[s] = radius[s] * radius[s];
    a.u[s] = u[s];
    a.out[s] = out[s];
  }
  const hipStream_t st = as_stream(stream);
  switch (n_scales) {
    case 1: launch_ball_query_multi<1>(centers, points, b, n, m, a, st); break;
    case 2: launch_ball_query_multi<2>(centers, points, b, n, m, a, st); break;
    case 3: launch_ball_query_multi<3>(centers, points, b, n, m, a, st); break;
    default: launch_ball_query_multi<4>(centers, points, b, n, m, a, st); break;
  }
  return launch_status();
}

GLDM_API int gldm_group_max_concat(const float *part, int b, int c, int m, int h, float *out, int c0, int ctot,
                                   gldm_stream_t stream) {
  if (!part || !out || b <= 0 || c <= 0 || m <= 0 || c0 < 0 || c0 + c > ctot) return GLDM_ERR_INVALID_ARG;
  if (!(h == 1 || h == 2 || h == 4) || b > 65535) return GLDM_ERR_UNSUPPORTED;
  const int in_vec = ((size_t)m * h) % 4 == 0 && (reinterpret_cast<uintptr_t>(part) & 15) == 0;
  const int out_vec = m % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const long long items = (long long)c * ceil_div(m, 4);
  if ((items + kFoldBlock - 1) / kFoldBlock > 0x7fffffffLL) return GLDM_ERR_UNSUPPORTED;
  dim3 grid((unsigned)((items + kFoldBlock - 1) / kFoldBlock), b);
  const hipStream_t st = as_stream(stream);
  if (h == 1) hipLaunchKernelGGL(group_max_concat_kernel<1>, grid, dim3(kFoldBlock), 0, st, part, c, m, out, c0, ctot, in_vec, out_vec);
  else if (h == 2) hipLaunchKernelGGL(group_max_concat_kernel<2>, grid, dim3(kFoldBlock), 0, st, part, c, m, out, c0, ctot, in_vec, out_vec);
  else hipLaunchKernelGGL(group_max_concat_kernel<4>, grid, dim3(kFoldBlock), 0, st, part, c, m, out, c0, ctot, in_vec, out_vec);
  return launch_status();
}
