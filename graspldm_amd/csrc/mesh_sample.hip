// mesh_sample.hip -- area-weighted surface sampling of a ragged batch of triangle meshes (include/gldm.h, "meshes";
// DESIGN.md 4.17):
//
//   gldm_mesh_sample_surface  n points on the surface of every mesh, each on a face drawn with probability proportional
//                             to its area; the face's row and, optionally, its unit normal.
//
// The face areas are f64; they become integer weights at a per-mesh power-of-two scale, so that the running sum a sample
// searches is an integer scan and no scan order changes a bit.  Four launches: the per-mesh largest area (an exact maximum,
// vector atomicMax on the bits of non-negative doubles, behind a clearing launch), the weights and their inclusive scan
// (one workgroup per mesh), the samples.  Compiled with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): every f64 and
// f32 operation below rounds once, as tests/mesh_ref.py restates it.
#include <math.h>
#include <stdint.h>

#include "host_util.h"
#include "mesh_range.h"

namespace {

#include "diffusion_step.h"   // philox4x32_10
#pragma clang fp contract(off)   // the header ends by handing contraction back to its fast-math users: off again, as built

constexpr int kMaxSamples = 1 << 24;        // per mesh
constexpr long long kMaxSampleRows = 1ll << 28;   // b * n

// e1 = v1 - v0, e2 = v2 - v0 and c = e1 x e2 in f64; n2 = (cx cx + cy cy) + cz cz.
__device__ __forceinline__ double cross_f64(const Tri &t, double (&c)[3]) {
  double e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e1[k] = (double)t.v[1][k] - (double)t.v[0][k];
    e2[k] = (double)t.v[2][k] - (double)t.v[0][k];
  }
  c[0] = e1[1] * e2[2] - e1[2] * e2[1];
  c[1] = e1[2] * e2[0] - e1[0] * e2[2];
  c[2] = e1[0] * e2[1] - e1[1] * e2[0];
  return (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
}

__global__ void amax_clear_kernel(int b, unsigned long long *__restrict__ amax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b) amax[i] = 0ull;
}

// A = 0.5 sqrt(n2); 0 for a face with an index outside its mesh and for an area that is not a positive finite number.
__global__ __launch_bounds__(kMeshChunk) void area_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                          MeshArrays ma, int chunks_max, double *__restrict__ area,
                                                          unsigned long long *__restrict__ amax) {
  const int ch = blockIdx.x % chunks_max;
  const int mesh = blockIdx.x / chunks_max;
  const MeshRange mr = mesh_range(ma, mesh);
  const int f = ch * kMeshChunk + (int)threadIdx.x;
  if (f >= mr.fn) return;
  const Tri t = load_tri(verts, faces, mr, mr.fs + f);
  double c[3];
  double a = 0.5 * sqrt(cross_f64(t, c));
  if (!t.ok || !(a > 0.0) || !(a < INFINITY)) a = 0.0;
  area[mr.fs + f] = a;
  if (a > 0.0) atomicMax(&amax[mesh], (unsigned long long)__double_as_longlong(a));
}

// One workgroup per mesh: q = rint(A 2^(40 - e)), Amax = m 2^e with m in [0.5, 1), and the inclusive sum of q in face order.
__global__ __launch_bounds__(kMeshChunk) void weight_scan_kernel(MeshArrays ma, const double *__restrict__ area,
                                                                 const unsigned long long *__restrict__ amax,
                                                                 unsigned long long *__restrict__ cum,
                                                                 unsigned long long *__restrict__ total) {
  __shared__ unsigned long long wsum[kMeshChunk / 64];
  const int mesh = blockIdx.x;
  const MeshRange mr = mesh_range(ma, mesh);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double top = __longlong_as_double((long long)amax[mesh]);
  int e = 0;
  if (top > 0.0) frexp(top, &e);
  unsigned long long run = 0ull;
  for (int f0 = 0; f0 < mr.fn; f0 += kMeshChunk) {
    const int f = f0 + tid;
    unsigned long long q = 0ull;
    if (f < mr.fn && top > 0.0) q = (unsigned long long)rint(ldexp(area[mr.fs + f], 40 - e));
    unsigned long long x = q;   // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    __syncthreads();   // wsum is free again
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    unsigned long long before = run, all = 0ull;
#pragma unroll
    for (int w = 0; w < kMeshChunk / 64; ++w) {
      before += w < wave ? wsum[w] : 0ull;
      all += wsum[w];
    }
    if (f < mr.fn) cum[mr.fs + f] = before + x;
    run += all;
  }
  if (tid == 0) total[mesh] = run;
}

template <int RNG>
__global__ __launch_bounds__(256) void sample_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                     MeshArrays ma, int n, int chunks_n, const float *__restrict__ rand,
                                                     unsigned long long seed, const unsigned long long *__restrict__ cum,
                                                     const unsigned long long *__restrict__ total,
                                                     float *__restrict__ points, int32_t *__restrict__ face,
                                                     float *__restrict__ normals) {
  const int mesh = blockIdx.x / chunks_n;
  const int i = (blockIdx.x % chunks_n) * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const MeshRange mr = mesh_range(ma, mesh);
  const long long at = (long long)mesh * n + i;
  const unsigned long long tot = mr.fn > 0 ? total[mesh] : 0ull;
  float out[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
  int row = -1;
  if (tot > 0ull) {
    unsigned k0;      // u0 2^24 as an integer
    float u1, u2;
    if (RNG) {
      unsigned x[4];
      philox4x32_10(seed, (unsigned)i, (unsigned)mesh, 0u, 0u, x);
      k0 = x[0] >> 8;
      u1 = (float)(x[1] >> 8) * 5.9604644775390625e-08f;
      u2 = (float)(x[2] >> 8) * 5.9604644775390625e-08f;
    } else {
      // anything the tensor holds is brought into [0, 1) first: fmax / fmin return the other operand for a NaN
      const float top = 0.99999994f;
      const float u0 = fminf(fmaxf(rand[at * 3 + 0], 0.f), top);
      u1 = fminf(fmaxf(rand[at * 3 + 1], 0.f), top);
      u2 = fminf(fmaxf(rand[at * 3 + 2], 0.f), top);
      k0 = (unsigned)(u0 * 16777216.0f);
    }
    // t = (k0 * total) >> 24 without a 128-bit product: total = hi 2^32 + lo, k0 hi < 2^54, k0 lo < 2^56
    const unsigned long long hi = tot >> 32, lo = tot & 0xffffffffull;
    const unsigned long long t = ((k0 * hi) << 8) + ((k0 * lo) >> 24);
    int a = 0, z = mr.fn - 1;   // the first face with cum > t; t < total = cum[fn - 1]
    while (a < z) {
      const int mid = a + (z - a) / 2;
      if (cum[mr.fs + mid] > t) z = mid; else a = mid + 1;
    }
    row = (int)(mr.fs + a);
    const Tri tr = load_tri(verts, faces, mr, row);   // ok: the face has a weight
    if (u1 + u2 > 1.0f) {
      u1 = 1.0f - u1;
      u2 = 1.0f - u2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float e1 = tr.v[1][c] - tr.v[0][c], e2 = tr.v[2][c] - tr.v[0][c];
      out[c] = tr.v[0][c] + (e1 * u1 + e2 * u2);
    }
    if (normals) {
      double cr[3];
      const double len = sqrt(cross_f64(tr, cr));
#pragma unroll
      for (int c = 0; c < 3; ++c) nrm[c] = (float)(cr[c] / len);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) points[at * 3 + c] = out[c];
  if (face) face[at] = row;
  if (normals)
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[at * 3 + c] = nrm[c];
}

// No pointer is read and the device is not touched outside it.
int check_envelope(int b, int f_max, int n_verts, int n_faces, int n) {
  if (b < 1 || f_max < 0 || n_verts < 0 || n_faces < 0 || n < 0) return GLDM_ERR_INVALID_ARG;
  if (b > kMaxMeshes || f_max > kMaxMeshFaces || n_verts > kMaxMeshRows || n_faces > kMaxMeshRows || n > kMaxSamples ||
      (long long)b * n > kMaxSampleRows)
    return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

inline long long align8(long long v) { return (v + 7) & ~7ll; }

}  // namespace

// workspace: area f64 [n_faces], cum u64 [n_faces], amax u64 [b], total u64 [b]
GLDM_API long long gldm_mesh_sample_surface_workspace_bytes(int b, int f_max, int n_verts, int n_faces, int n) {
  const int st = check_envelope(b, f_max, n_verts, n_faces, n);
  if (st != GLDM_OK) return st;
  return 16ll * n_faces + 16ll * b;
}

GLDM_API int gldm_mesh_sample_surface(const float *vertices, const int32_t *faces, const int32_t *vert_start,
                                      const int32_t *vert_count, const int32_t *face_start, const int32_t *face_count, int b,
                                      int f_max, int n_verts, int n_faces, int n, const float *rand, unsigned long long seed,
                                      void *workspace, long long workspace_bytes, float *points, int32_t *face, float *normals,
                                      gldm_stream_t stream) {
  const int env = check_envelope(b, f_max, n_verts, n_faces, n);
  if (env != GLDM_OK) return env;
  if (n == 0) return GLDM_OK;
  if (!vert_start || !vert_count || !face_start || !face_count || !points || !workspace) return GLDM_ERR_INVALID_ARG;
  if ((n_faces > 0 && !faces) || (n_verts > 0 && !vertices)) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_mesh_sample_surface_workspace_bytes(b, f_max, n_verts, n_faces, n)) return GLDM_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  double *area = static_cast<double *>(workspace);
  unsigned long long *cum = reinterpret_cast<unsigned long long *>(area + n_faces);
  unsigned long long *amax = cum + n_faces, *total = amax + b;
  const MeshArrays ma = {vert_start, vert_count, face_start, face_count, f_max, n_verts, n_faces};
  hipLaunchKernelGGL(amax_clear_kernel, dim3(ceil_div(b, 256)), dim3(256), 0, st, b, amax);
  if (f_max > 0 && n_faces > 0) {
    const int chunks_max = ceil_div(f_max, kMeshChunk);
    hipLaunchKernelGGL(area_kernel, dim3((unsigned)((long long)b * chunks_max)), dim3(kMeshChunk), 0, st, vertices, faces, ma,
                       chunks_max, area, amax);
  }
  hipLaunchKernelGGL(weight_scan_kernel, dim3(b), dim3(kMeshChunk), 0, st, ma, area, amax, cum, total);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  const int chunks_n = ceil_div(n, 256);
  const dim3 grid((unsigned)((long long)b * chunks_n));   // <= 2^28 / 256 + 65535
  if (rand)
    hipLaunchKernelGGL(sample_kernel<0>, grid, dim3(256), 0, st, vertices, faces, ma, n, chunks_n, rand, seed, cum, total, points,
                       face, normals);
  else
    hipLaunchKernelGGL(sample_kernel<1>, grid, dim3(256), 0, st, vertices, faces, ma, n, chunks_n, rand, seed, cum, total, points,
                       face, normals);
  return launch_status();
}
