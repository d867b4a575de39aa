// sa_msg.hip -- the two max pools of the set-abstraction modules (pointnet.py:40-114) for gfx950, behind the C ABI
// declared in include/gldm.h.
//
//  * gldm_group_max_concat: the maximum over h consecutive columns, written into a row range of the module's
//    concatenated output.  h > 1 folds the sub-centres of a U = 64 h neighbourhood that ran on the 64-column fused
//    kernels as h centres; h = 1 is the strided copy that stands in for torch.cat.
//  * gldm_row_max: the maximum over a whole row, the global pooling of PointNetAModule.
// (The multi-radius ball query of the multi-scale module is in neighbors.hip, beside the single-radius one.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_util.h"

namespace {

constexpr int kWave = 64;

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

// ---------------------------------------------------------------- row max --
// out[row] = max over n of x[row][0..n): the global pooling of PointNetAModule (pointnet.py:40-44, `.max(dim=-1)`) over
// [b * c] rows.  One wave per row, 16-byte loads where the row allows, DPP-free shuffle reduction (a row is a few hundred
// floats: the launch is one pass over x).  NaN propagates as in torch.max (a NaN in the row -> NaN).
__global__ __launch_bounds__(256) void row_max_kernel(const float *__restrict__ x, long long rows, int n, float *__restrict__ out) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float *p = x + row * n;
  float m = -__builtin_inff();
  bool nan = false;
  if ((n & 3) == 0 && (((size_t)p & 15) == 0)) {
    for (int i = lane; i < (n >> 2); i += 64) {
      const float4 v = reinterpret_cast<const float4 *>(p)[i];
      nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
      m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const float v = p[i];
      nan |= v != v;
      m = fmaxf(m, v);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
  const bool any_nan = __ballot(nan) != 0ull;
  if (lane == 0) out[row] = any_nan ? __builtin_nanf("") : m;
}

}  // namespace

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

GLDM_API int gldm_row_max(const float *x, long long rows, int n, float *out, gldm_stream_t stream) {
  if (!x || !out || rows <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(row_max_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, as_stream(stream), x, rows, n, out);
  return launch_status();
}
