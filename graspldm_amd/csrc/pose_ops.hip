// pose_ops.hip -- the small element-wise ops either side of the 1-D engines (resnet1d.hip), one thread per output:
//   * gldm_r1d_cond_embed : SiLU(Linear(z_cond)), the conditioning rows of the embedding sum;
//   * gldm_pose_prologue  : 4x4 poses -> normalised (t, mrp[, label]) rows for the grasp encoder;
//   * gldm_pose_epilogue  : decoder heads -> un-normalised (t, mrp), 4x4 poses, confidence;
//   * gldm_step_noise_rng : the in-kernel DDPM noise of gldm_denoise_rng on its own, for the statistical tests.
// The two pose kernels follow the reference's operation order with no contraction (the pragmas around them).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gldm.h"

#define GLDM_API extern "C" __attribute__((visibility("default")))

namespace {

#include "diffusion_step.h"

__global__ void cond_embed_kernel(const float *__restrict__ z, const float *__restrict__ w,
                                  const float *__restrict__ b, int rows_total, int dc, int e, float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows_total * e) return;
  const int row = i / e, col = i - row * e;
  const float *zr = z + (size_t)row * dc, *wr = w + (size_t)col * dc;
  float acc = b[col];
  for (int q = 0; q < dc; ++q) acc += wr[q] * zr[q];
  out[i] = acc / (1.0f + expf(-acc));
}

#pragma clang fp contract(off)
__global__ void pose_epilogue_kernel(const float *__restrict__ tmrp, const float *__restrict__ logit,
                                     const float *__restrict__ mean, const float *__restrict__ stdv, int n, int gpc,
                                     float *__restrict__ H, float *__restrict__ un, float *__restrict__ conf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cl = i / gpc;
  float v[6];
  for (int q = 0; q < 6; ++q) {
    v[q] = tmrp[(size_t)i * 6 + q] * stdv[cl * 6 + q] + mean[cl * 6 + q];
    un[(size_t)i * 6 + q] = v[q];
  }
  // rotations.py:218-252 (mrp -> quat) and :171-215 (quat -> rotmat, SciPy convention)
  const float magsq = v[3] * v[3] + v[4] * v[4] + v[5] * v[5];
  const float den = 1.0f + magsq;
  const float x = (2.0f * v[3]) / den, y = (2.0f * v[4]) / den, z = (2.0f * v[5]) / den;
  const float w = (1.0f - magsq) / den;
  const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const float xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  float *h = H + (size_t)i * 16;
  h[0] = x2 - y2 - z2 + w2;  h[1] = 2.0f * (xy - zw);     h[2] = 2.0f * (xz + yw);      h[3] = v[0];
  h[4] = 2.0f * (xy + zw);   h[5] = -x2 + y2 - z2 + w2;   h[6] = 2.0f * (yz - xw);      h[7] = v[1];
  h[8] = 2.0f * (xz - yw);   h[9] = 2.0f * (yz + xw);     h[10] = -x2 - y2 + z2 + w2;   h[11] = v[2];
  h[12] = 0.f; h[13] = 0.f; h[14] = 0.f; h[15] = 1.0f;
  if (conf) conf[i] = 1.0f / (1.0f + expf(-logit[i]));
}

// The way back (rotations.py:305-309,115-163): arg-max over (R00, R11, R22, trace) with the first maximum winning (torch
// argmax), the SciPy branch formulas, normalise, q.xyz / (1 + q.w), then the dataset's (x - mean) / std.  Same operation
// order as the reference on the same f32 values (no contraction), so the branch is the reference's.
__global__ void pose_prologue_kernel(const float *__restrict__ H, const float *__restrict__ label,
                                     const float *__restrict__ mean, const float *__restrict__ stdv, int n, int gpc,
                                     float *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cl = i / gpc;
  const float *h = H + (size_t)i * 16;
  float m[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[r][c] = h[4 * r + c];
  const float dg[4] = {m[0][0], m[1][1], m[2][2], (m[0][0] + m[1][1]) + m[2][2]};
  int ch = 0;
  for (int q = 1; q < 4; ++q) ch = dg[q] > dg[ch] ? q : ch;
  float q4[4];
  if (ch == 3) {
    q4[0] = m[2][1] - m[1][2];
    q4[1] = m[0][2] - m[2][0];
    q4[2] = m[1][0] - m[0][1];
    q4[3] = 1.0f + dg[3];
  } else {
    // constant indices only (a runtime-indexed register array would go to scratch)
    const float mii = ch == 0 ? m[0][0] : (ch == 1 ? m[1][1] : m[2][2]);
    const float mji = ch == 0 ? m[1][0] : (ch == 1 ? m[2][1] : m[0][2]), mij = ch == 0 ? m[0][1] : (ch == 1 ? m[1][2] : m[2][0]);
    const float mki = ch == 0 ? m[2][0] : (ch == 1 ? m[0][1] : m[1][2]), mik = ch == 0 ? m[0][2] : (ch == 1 ? m[1][0] : m[2][1]);
    const float mkj = ch == 0 ? m[2][1] : (ch == 1 ? m[0][2] : m[1][0]), mjk = ch == 0 ? m[1][2] : (ch == 1 ? m[2][0] : m[0][1]);
    const float qi = (1.0f - dg[3]) + 2.0f * mii, qj = mji + mij, qk = mki + mik;
    q4[0] = ch == 0 ? qi : (ch == 1 ? qk : qj);
    q4[1] = ch == 0 ? qj : (ch == 1 ? qi : qk);
    q4[2] = ch == 0 ? qk : (ch == 1 ? qj : qi);
    q4[3] = mkj - mjk;
  }
  const float nrm = sqrtf(((q4[0] * q4[0] + q4[1] * q4[1]) + q4[2] * q4[2]) + q4[3] * q4[3]);
  const float den = 1.0f + q4[3] / nrm;
  const float v[6] = {h[3], h[7], h[11], (q4[0] / nrm) / den, (q4[1] / nrm) / den, (q4[2] / nrm) / den};
  const int w = label ? 7 : 6;
  for (int q = 0; q < 6; ++q) out[(size_t)i * w + q] = (v[q] - mean[cl * 6 + q]) / stdv[cl * 6 + q];
  if (label) out[(size_t)i * 7 + 6] = label[i];
}
#pragma clang fp contract(fast)

}  // namespace

// The generator on its own (n latents x L positions of one step), for the statistical tests: out [n][L]
__global__ void philox_normal_kernel(unsigned long long seed, long long base, int step, int n, int L, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * L) return;
  const int gi = i / L, l = i - gi * L;
  const unsigned long long g = (unsigned long long)(base + gi);
  float z4[4];
  philox_normal4(seed, (unsigned)g, (unsigned)(g >> 32), (unsigned)(l >> 2), (unsigned)step, z4);
  out[i] = z4[l & 3];
}

GLDM_API int gldm_r1d_cond_embed(const float *z_cond, const float *w, const float *b, int n_cond, int rows, int dc,
                                 int e, float *cemb, gldm_stream_t stream) {
  if (!z_cond || !w || !b || !cemb || n_cond <= 0 || rows <= 0 || dc <= 0 || e <= 0) return GLDM_ERR_INVALID_ARG;
  const int total = n_cond * rows * e;
  hipLaunchKernelGGL(cond_embed_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     z_cond, w, b, n_cond * rows, dc, e, cemb);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_step_noise_rng(unsigned long long noise_seed, long long noise_base, int step, int n_samples, int seq_len,
                                 float *out, gldm_stream_t stream) {
  if (!out || n_samples <= 0 || seq_len <= 0 || step < 0 || noise_base < 0) return GLDM_ERR_INVALID_ARG;
  const int total = n_samples * seq_len;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), noise_seed,
                     noise_base, step, n_samples, seq_len, out);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_pose_prologue(const float *H, const float *label, const float *grasp_mean, const float *grasp_std, int n,
                                int grasps_per_cloud, int n_clouds, float *h, gldm_stream_t stream) {
  if (!H || !grasp_mean || !grasp_std || !h || n <= 0 || grasps_per_cloud <= 0 || n_clouds <= 0) return GLDM_ERR_INVALID_ARG;
  if ((long long)n_clouds * grasps_per_cloud < (long long)n) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pose_prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), H,
                     label, grasp_mean, grasp_std, n, grasps_per_cloud, h);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_pose_epilogue(const float *tmrp, const float *logit, const float *grasp_mean,
                                const float *grasp_std, int n, int grasps_per_cloud, int n_clouds, float *H,
                                float *tmrp_unnorm, float *confidence, gldm_stream_t stream) {
  if (!tmrp || !grasp_mean || !grasp_std || !H || !tmrp_unnorm || n <= 0 || grasps_per_cloud <= 0 || n_clouds <= 0)
    return GLDM_ERR_INVALID_ARG;
  // every grasp's cloud row (i / grasps_per_cloud) must exist in mean/std [n_clouds, 6]
  if ((long long)n_clouds * grasps_per_cloud < (long long)n) return GLDM_ERR_INVALID_ARG;
  if (confidence && !logit) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pose_epilogue_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     tmrp, logit, grasp_mean, grasp_std, n, grasps_per_cloud, H, tmrp_unnorm, confidence);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
