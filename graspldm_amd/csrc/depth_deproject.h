// depth_deproject.h -- "is this pixel valid and where is its point": the one predicate + pinhole deprojection shared by
// depth_cloud.hip (gldm_depth_to_cloud, gldm_depth_to_objects) and tabletop.hip (gldm_segment_tabletop).  Both sources are
// compiled with -ffp-contract=off (csrc/Makefile, SRCS_STRICT), so every product, quotient and sum below rounds once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct DepthParams {
  float fx, fy, cx, cy, z_min, z_max, depth_scale;
  float xf[12];          // cam_to_world, 3 x 4 row major
  float lo[3], hi[3];    // box in the output frame
  int has_xf, has_box;
  int w, hw;
};

__device__ __forceinline__ float load_depth(const float *d, size_t i, float) { return d[i]; }
__device__ __forceinline__ float load_depth(const uint16_t *d, size_t i, float scale) { return (float)d[i] * scale; }

// The one predicate + point of a pixel; `d` and `m` are the loaded depth (metres) and mask byte (1 without a mask).
__device__ __forceinline__ bool deproject(const DepthParams &P, int pix, float d, unsigned m, float &ox, float &oy, float &oz) {
  if (!(d > P.z_min && d <= P.z_max) || m == 0u) return false;
  const int v = pix / P.w, u = pix - v * P.w;
  const float x = __fdiv_rn(((float)u - P.cx) * d, P.fx);
  const float y = __fdiv_rn(((float)v - P.cy) * d, P.fy);
  const float z = d;
  if (!P.has_xf) {
    ox = x; oy = y; oz = z;
  } else {
    ox = ((P.xf[0] * x + P.xf[1] * y) + P.xf[2] * z) + P.xf[3];
    oy = ((P.xf[4] * x + P.xf[5] * y) + P.xf[6] * z) + P.xf[7];
    oz = ((P.xf[8] * x + P.xf[9] * y) + P.xf[10] * z) + P.xf[11];
  }
  if (P.has_box) {
    if (!(ox >= P.lo[0] && ox <= P.hi[0] && oy >= P.lo[1] && oy <= P.hi[1] && oz >= P.lo[2] && oz <= P.hi[2])) return false;
  }
  return true;
}

// The host side of DepthParams: the arguments of gldm_depth_to_cloud for frames of h x w.
inline DepthParams make_params(int depth_is_u16, float depth_scale, int h, int w, float fx, float fy, float cx, float cy,
                               float z_min, float z_max, const float *cam_to_world, const float *box_lo,
                               const float *box_hi) {
  DepthParams P;
  P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.z_min = z_min; P.z_max = z_max;
  P.depth_scale = depth_is_u16 ? depth_scale : 1.f;
  P.has_xf = cam_to_world != nullptr;
  P.has_box = box_lo != nullptr;
  for (int i = 0; i < 12; ++i) P.xf[i] = cam_to_world ? cam_to_world[i] : 0.f;
  for (int i = 0; i < 3; ++i) {
    P.lo[i] = box_lo ? box_lo[i] : 0.f;
    P.hi[i] = box_hi ? box_hi[i] : 0.f;
  }
  P.w = w;
  P.hw = h * w;
  return P;
}

}  // namespace
