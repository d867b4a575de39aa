// point_ops.hip -- what is left once every kernel family has a source of its own: the sensor-cloud front end
// (gldm_normalize_cloud, gldm_gather_points) and the library's own two entries, gldm_abi_version and gldm_status_string,
// behind the C ABI declared in include/gldm.h.  The neighbourhood operators are in neighbors.hip, the point <-> voxel
// operators in voxel_points.hip, farthest-point sampling in fps.hip, the max pools of the set-abstraction modules in
// sa_msg.hip.  Compiled with -ffp-contract=off: (pc - mean - shift) / scale rounds once per written operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_util.h"

GLDM_API int gldm_abi_version(void) { return GLDM_ABI_VERSION; }

GLDM_API const char *gldm_status_string(int status) {
  switch (status) {
    case GLDM_OK: return "ok";
    case GLDM_ERR_INVALID_ARG: return "invalid argument (null pointer or non-positive size)";
    case GLDM_ERR_LAUNCH: return "HIP kernel launch failed";
    case GLDM_ERR_UNSUPPORTED: return "shape not supported by the gfx950 kernels";
    case GLDM_ERR_WORKSPACE: return "workspace too small";
    default: return "unknown gldm status";
  }
}

namespace {
// Raw-cloud front end: centre + scale a sensor cloud [n][3] (tools/inference.py:570-591 normalize_input) and
// gather rows of it by index (point-count regularisation).  The mean is accumulated in f64 in a fixed tree.
constexpr int kWave = 64;
constexpr int kNcBlock = 256;
struct Vec3 { float v[3]; };
__global__ __launch_bounds__(kNcBlock) void normalize_cloud_kernel(const float *__restrict__ pc, int n, Vec3 shift,
                                                                   Vec3 scale, float *__restrict__ out,
                                                                   float *__restrict__ mean_out) {
  __shared__ double s_sum[3][kNcBlock / kWave];
  __shared__ float s_mean[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  pc += (size_t)b * 3 * n;
  out += (size_t)b * 3 * n;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int k = tid; k < n; k += kNcBlock)
#pragma unroll
    for (int a = 0; a < 3; ++a) acc[a] += (double)pc[3 * k + a];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double v = acc[a];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    if ((tid & 63) == 0) s_sum[a][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < 3) {
    double v = 0.0;
    for (int w = 0; w < kNcBlock / kWave; ++w) v += s_sum[tid][w];
    const float m = (float)(v / (double)n);
    s_mean[tid] = m;
    mean_out[(size_t)b * 3 + tid] = m;
  }
  __syncthreads();
  for (int i = tid; i < 3 * n; i += kNcBlock) {
    const int a = i % 3;
    const float sh = a == 0 ? shift.v[0] : (a == 1 ? shift.v[1] : shift.v[2]);
    const float sc = a == 0 ? scale.v[0] : (a == 1 ? scale.v[1] : scale.v[2]);
    out[i] = ((pc[i] - s_mean[a]) - sh) / sc;
  }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ pc, const int32_t *__restrict__ idx,
                                                          int n, int m, float *__restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * m) return;
  const int j = i / 3, a = i - 3 * j;
  out[(size_t)b * 3 * m + i] = pc[((size_t)b * n + idx[(size_t)b * m + j]) * 3 + a];
}
}  // namespace

GLDM_API int gldm_normalize_cloud(const float *pc, int b, int n, float shift_x, float shift_y, float shift_z,
                                  float scale_x, float scale_y, float scale_z, float *pc_out, float *mean_out,
                                  gldm_stream_t stream) {
  if (!pc || !pc_out || !mean_out || b <= 0 || n <= 0 || scale_x == 0.f || scale_y == 0.f || scale_z == 0.f)
    return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(normalize_cloud_kernel, dim3(b), dim3(kNcBlock), 0, as_stream(stream), pc, n,
                     Vec3{{shift_x, shift_y, shift_z}}, Vec3{{scale_x, scale_y, scale_z}}, pc_out, mean_out);
  return launch_status();
}

GLDM_API int gldm_gather_points(const float *pc, const int32_t *idx, int b, int n, int m, float *out,
                                gldm_stream_t stream) {
  if (!pc || !idx || !out || b <= 0 || n <= 0 || m <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div(3 * m, 256), b), dim3(256), 0, as_stream(stream), pc, idx, n,
                     m, out);
  return launch_status();
}
