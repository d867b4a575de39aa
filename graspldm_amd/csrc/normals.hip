// normals.hip -- surface normals of sensor clouds (include/gldm.h, "surface normals"):
//
//   gldm_knn_radius     the up to k nearest neighbours of every point within a radius, ordered by (d2, index): the search of
//                       estimate_normals_cam_from_pc (grasp_ldm/utils/pointcloud_helpers.py:74-97: cKDTree.query with
//                       distance_upper_bound).
//   gldm_point_normals  the eigenvector of the smallest eigenvalue of every point's neighbourhood scatter matrix, turned
//                       towards a view point (vectorized_normal_computation, :99-122).
//
// Compiled with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): a squared distance is (dx*dx + dy*dy) + dz*dz with one
// rounding per written operation, and the broad phase below relies on exactly that.  Nothing here uses the matrix pipe.
#include <math.h>
#include <stdint.h>

#include "knn_scan.h"

namespace {

constexpr int kSweeps = 8;         // cyclic Jacobi sweeps over a 3 x 3 matrix in f64 (quadratic convergence: 5 suffice)

// A neighbour is one 64-bit key: the bits of d2 (a non-negative float orders like its bit pattern) above the index.  Keys
// order exactly like (d2, index), so the k smallest keys are the answer whatever order the candidates arrive in.
__device__ __forceinline__ uint64_t make_key(float d2, int j) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)j; }

// boxes [b, chunks, 6]: lo xyz, hi xyz of every 256-point chunk (Box, box_d2 and the body: knn_scan.h).
__global__ __launch_bounds__(kChunk) void chunk_box_kernel(const float *__restrict__ pc, int n, int chunks,
                                                           float *__restrict__ boxes) {
  const int ch = blockIdx.x % chunks;
  const int cloud = blockIdx.x / chunks;
  const int p0 = ch * kChunk;
  chunk_box_body(pc + ((long long)cloud * n + p0) * 3, min(kChunk, n - p0), boxes + ((long long)cloud * chunks + ch) * 6);
}

// Grid: clouds x chunks.  A workgroup's 256 lanes are the query points of one chunk; every lane keeps its KT smallest keys
// sorted in registers (fully unrolled: no run-time register index).  Candidate chunks come through LDS (coalesced dword
// loads of the [n,3] rows; a candidate is one broadcast read) in the order own chunk, +1, -1, +2, ...: on a cloud in pixel
// order the lists fill with near points at once and the bound below tightens early.
// Broad phase, two levels, both exact (box_d2): the workgroup skips a chunk whose box lies farther than r2 from its own
// chunk's box (uniform over the workgroup: no load, no barrier); a wave skips the scan of a staged chunk that lies farther
// from the box of its own 64 points than min(r2, the wave's largest k-th d2) -- +inf until every lane's list holds k.
template <int KT>
__global__ __launch_bounds__(kChunk) void knn_kernel(const float *__restrict__ pc, const float *__restrict__ boxes, int n,
                                                     int k, int chunks, float r2, int32_t *__restrict__ idx,
                                                     float *__restrict__ d2out, int32_t *__restrict__ found) {
  __shared__ float pts[kChunk * 3];
  const int tid = threadIdx.x;
  const int own = blockIdx.x % chunks;
  const int cloud = blockIdx.x / chunks;
  const float *cloud_pts = pc + (long long)cloud * n * 3;
  const float *cloud_boxes = boxes + (long long)cloud * chunks * 6;
  const int qi = own * kChunk + tid;
  const bool live = qi < n;
  const int qs = live ? qi : n - 1;
  const float qx = cloud_pts[(long long)qs * 3 + 0], qy = cloud_pts[(long long)qs * 3 + 1], qz = cloud_pts[(long long)qs * 3 + 2];

  const uint64_t empty = ((uint64_t)kInfBits << 32) | (uint32_t)n;
  uint64_t key[KT];
#pragma unroll
  for (int s = 0; s < KT; ++s) key[s] = empty;

  const Box own_box = load_box(cloud_boxes, own);
  const Box wave_box = wave_query_box(qx, qy, qz);   // dead lanes repeat the cloud's last point, which is in the chunk
  float bound = r2;   // wave-uniform

  const int reach = max(own, chunks - 1 - own);
  for (int step = 0; step <= reach; ++step) {
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
      const int ch = side == 0 ? own + step : own - step;
      if (ch < 0 || ch >= chunks || (side == 1 && step == 0)) continue;   // uniform over the workgroup
      const Box cb = load_box(cloud_boxes, ch);
      if (box_d2(own_box, cb) > r2) continue;                             // uniform over the workgroup
      const int p0 = ch * kChunk;
      const int cnt = min(kChunk, n - p0);
      stage_chunk(pts, cloud_pts + (long long)p0 * 3, cnt);
      if (box_d2(wave_box, cb) > bound) continue;   // wave-uniform; the barriers above are behind this wave already
      for (int c = 0; c < cnt; ++c) {
        const float dx = pts[c * 3 + 0] - qx, dy = pts[c * 3 + 1] - qy, dz = pts[c * 3 + 2] - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const uint64_t cand = make_key(d2, p0 + c);
        insert_key<uint64_t, KT>(key, cand, live && d2 <= r2 && cand < key[KT - 1]);
      }
      // the wave's largest k-th squared distance: +inf while a live lane's list is short
      uint32_t kth = 0u;
#pragma unroll
      for (int s = 0; s < KT; ++s)
        if (s == k - 1) kth = (uint32_t)(key[s] >> 32);
      bound = fminf(r2, __uint_as_float(wave_max_bits(live ? kth : 0u)));
    }
  }

  if (live) {
    const long long row = ((long long)cloud * n + qi) * k;
    int cntf = 0;
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      if (s < k) {
        const int j = (int)(uint32_t)key[s];
        idx[row + s] = j;
        if (d2out) d2out[row + s] = __uint_as_float((uint32_t)(key[s] >> 32));
        cntf += j != n ? 1 : 0;
      }
    }
    found[(long long)cloud * n + qi] = cntf;
  }
}

// One Jacobi rotation of the symmetric 3 x 3 matrix in the plane (p, q), r the third axis; v*p, v*q the two columns of
// the accumulated eigenvector matrix.  Skipped where the off-diagonal is exactly 0.
__device__ __forceinline__ void rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                       double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // |theta| huge: t -> 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0, v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1, v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2, v2q = s * a2 + c * b2;
}

// One lane per point.  diffs in f32 as the reference forms them; the six sums of products in f64 (a product of two f32 is
// exact there); cyclic Jacobi with a fixed trip count; the column of the smallest diagonal entry (lowest index on a tie).
__global__ __launch_bounds__(256) void normals_kernel(const float *__restrict__ pc, const int32_t *__restrict__ idx,
                                                      const float *__restrict__ neighbors, int n, int k, long long total,
                                                      float vx, float vy, float vz, float *__restrict__ normals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long cloud = i / n;
  const float px = pc[i * 3 + 0], py = pc[i * 3 + 1], pz = pc[i * 3 + 2];
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
  int alive = 0;
  for (int s = 0; s < k; ++s) {
    float x, y, z;
    if (idx) {
      const int j = idx[i * k + s];
      const bool ok = j >= 0 && j < n;   // a missing slot (n) counts as the point itself
      alive += ok ? 1 : 0;
      const long long at = ok ? cloud * n + j : i;
      x = pc[at * 3 + 0], y = pc[at * 3 + 1], z = pc[at * 3 + 2];
    } else {
      const float *nb = neighbors + (i * k + s) * 3;
      x = nb[0], y = nb[1], z = nb[2];
      ++alive;
    }
    const float fx = x - px, fy = y - py, fz = z - pz;
    const double dx = fx, dy = fy, dz = fz;
    a00 += dx * dx, a01 += dx * dy, a02 += dx * dz, a11 += dy * dy, a12 += dy * dz, a22 += dz * dz;
  }
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll 1
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
    rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
    rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
  }
  const bool c1 = a11 < a00;
  const bool c2 = a22 < (c1 ? a11 : a00);
  double ex = c2 ? v02 : (c1 ? v01 : v00);
  double ey = c2 ? v12 : (c1 ? v11 : v10);
  double ez = c2 ? v22 : (c1 ? v21 : v20);
  const double inv = 1.0 / sqrt(ex * ex + ey * ey + ez * ez);
  ex *= inv, ey *= inv, ez *= inv;
  const float wx = px - vx, wy = py - vy, wz = pz - vz;
  const double dot = ex * (double)wx + ey * (double)wy + ez * (double)wz;
  if (dot >= 0.0) ex = -ex, ey = -ey, ez = -ez;   // pointcloud_helpers.py:120-121
  const bool plane = alive >= 3;
  normals[i * 3 + 0] = plane ? (float)ex : 0.f;
  normals[i * 3 + 1] = plane ? (float)ey : 0.f;
  normals[i * 3 + 2] = plane ? (float)ez : 0.f;
}

template <int KT>
void launch_knn(hipStream_t st, unsigned blocks, const float *pc, const float *boxes, int n, int k, int chunks, float r2,
                int32_t *idx, float *d2, int32_t *found) {
  hipLaunchKernelGGL(knn_kernel<KT>, dim3(blocks), dim3(kChunk), 0, st, pc, boxes, n, k, chunks, r2, idx, d2, found);
}

}  // namespace

GLDM_API long long gldm_knn_radius_workspace_bytes(int b, int n) {
  if (b <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (n > kMaxN || (long long)b * ceil_div(n, kChunk) > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  return (long long)b * ceil_div(n, kChunk) * 6 * (long long)sizeof(float);
}

GLDM_API int gldm_knn_radius(const float *pc, int b, int n, int k, float max_radius, void *workspace, long long workspace_bytes,
                             int32_t *idx, float *d2, int32_t *found, gldm_stream_t stream) {
  // the envelope first: no pointer is read and the device is not touched outside it
  if (b <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (k < 1 || k > kMaxK || n > kMaxN) return GLDM_ERR_UNSUPPORTED;
  const long long need = gldm_knn_radius_workspace_bytes(b, n);
  if (need < 0) return (int)need;
  if (!(max_radius >= 0.f) || !isfinite(max_radius * max_radius)) return GLDM_ERR_INVALID_ARG;   // r2 must be finite
  if (!pc || !idx || !found || !workspace) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < need) return GLDM_ERR_WORKSPACE;
  const int chunks = ceil_div(n, kChunk);
  const unsigned blocks = (unsigned)((long long)b * chunks);
  const float r2 = max_radius * max_radius;
  float *boxes = static_cast<float *>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(chunk_box_kernel, dim3(blocks), dim3(kChunk), 0, st, pc, n, chunks, boxes);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  if (k <= 4)
    launch_knn<4>(st, blocks, pc, boxes, n, k, chunks, r2, idx, d2, found);
  else if (k <= 8)
    launch_knn<8>(st, blocks, pc, boxes, n, k, chunks, r2, idx, d2, found);
  else if (k <= 12)
    launch_knn<12>(st, blocks, pc, boxes, n, k, chunks, r2, idx, d2, found);
  else
    launch_knn<16>(st, blocks, pc, boxes, n, k, chunks, r2, idx, d2, found);
  return launch_status();
}

GLDM_API int gldm_point_normals(const float *pc, const int32_t *idx, const float *neighbors, int b, int n, int k,
                                const float *view, float *normals, gldm_stream_t stream) {
  if (b <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (k < 1 || k > kMaxK || n > kMaxN) return GLDM_ERR_UNSUPPORTED;
  if (!pc || !view || !normals || (idx == nullptr) == (neighbors == nullptr)) return GLDM_ERR_INVALID_ARG;
  if (!isfinite(view[0]) || !isfinite(view[1]) || !isfinite(view[2])) return GLDM_ERR_INVALID_ARG;
  const long long total = (long long)b * n;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(normals_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), pc, idx, neighbors, n, k, total,
                     view[0], view[1], view[2], normals);
  return launch_status();
}
