// oracle/ref_shim/entry.hip -- TEST INFRASTRUCTURE.  C entry points over the
// reference's seven forward launchers, for ctypes (oracle/ref_backend.py).  The
// launcher declarations are read from the reference tree at build time (-I its
// functional/src); every pointer is a raw device pointer and nothing is
// validated here -- ref_backend.py checks index ranges before it calls.
#include <hip/hip_runtime.h>

#include "ATen/cuda/CUDAContext.h"
#include "ball_query/ball_query.cuh"
#include "grouping/grouping.cuh"
#include "interpolate/neighbor_interpolate.cuh"
#include "interpolate/trilinear_devox.cuh"
#include "sampling/sampling.cuh"
#include "voxelization/vox.cuh"

static hipStream_t g_stream = nullptr;

namespace at {
namespace cuda {
hipStream_t getCurrentCUDAStream() { return g_stream; }
}
}

#define REF_API extern "C" __attribute__((visibility("default")))

// furthest_point_sampling and avg_voxelize launch on the legacy default stream
// whatever is set here (sampling.cu:169-174, vox.cu:114-120).
REF_API void ref_set_stream(void *stream) { g_stream = (hipStream_t)stream; }

REF_API void ref_ball_query(int b, int n, int m, float r2, int u, const float *centers, const float *points,
                            int *out) {
  ball_query(b, n, m, r2, u, centers, points, out);
}

REF_API void ref_grouping(int b, int c, int n, int m, int u, const float *feat, const int *idx, float *out) {
  grouping(b, c, n, m, u, feat, idx, out);
}

REF_API void ref_gather_features(int b, int c, int n, int m, const float *feat, const int *idx, float *out) {
  gather_features(b, c, n, m, feat, idx, out);
}

REF_API void ref_furthest_point_sampling(int b, int n, int m, const float *coords, float *dist, int *out) {
  furthest_point_sampling(b, n, m, coords, dist, out);
}

REF_API void ref_three_nearest_neighbors_interpolate(int b, int c, int m, int n, const float *points,
                                                     const float *centers, const float *cfeat, int *idx,
                                                     float *wgt, float *out) {
  three_nearest_neighbors_interpolate(b, c, m, n, points, centers, cfeat, idx, wgt, out);
}

REF_API void ref_trilinear_devoxelize(int b, int c, int n, int r, int is_training, const float *coords,
                                      const float *feat, int *inds, float *wgts, float *outs) {
  trilinear_devoxelize(b, c, n, r, r * r, r * r * r, is_training != 0, coords, feat, inds, wgts, outs);
}

REF_API void ref_avg_voxelize(int b, int c, int n, int r, const int *coords, const float *feat, int *ind, int *cnt,
                              float *out) {
  avg_voxelize(b, c, n, r, r * r, r * r * r, coords, feat, ind, cnt, out);
}
