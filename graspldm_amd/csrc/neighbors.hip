// neighbors.hip -- gfx950 kernels of the neighbourhood operators of the PointNet++ modules, behind the C ABI declared in
// include/gldm.h: ball query for one radius and for up to four (gldm_ball_query, gldm_ball_query_multi), the fused
// set-abstraction gather (gldm_sa_group), grouping, gather, and 3-NN with interpolation.
//
// Design notes (CDNA4, wave64):
//  * every launch spreads one cloud over many workgroups (the reference launches ONE block per cloud for all of these);
//  * ball query is a wave-per-centre ordered compaction: 64 candidates per step, __ballot + prefix popcount keep the
//    reference's "first U in index order" semantics exactly.  The scan is ball_query.h's, for every kernel that needs one;
//  * compiled with -ffp-contract=off so that the strict-inequality decisions on distances and the 3-term interpolation
//    sums match the scalar oracle bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "ball_query.h"
#include "host_util.h"

namespace {

// ------------------------------------------------------------ ball query --
// One wave per centre, kBqCentresPerBlock centres per 256-thread block, ONE scan of the cloud per centre for all radii.
// Point coordinates are staged once per block in LDS when they fit (bq_stage_points), otherwise read through L2.
struct BqScales {
  float r2[kMaxScales];
  int u[kMaxScales];
  int32_t *out[kMaxScales];  // [b, m, u_s]
};

template <bool kUseLds, int S>
__global__ __launch_bounds__(kBqBlock) void ball_query_multi_kernel(const float *__restrict__ centers,
                                                                    const float *__restrict__ points, int n, int m,
                                                                    BqScales a) {
  extern __shared__ float s_pts[];
  const int b = blockIdx.y;
  points += (size_t)b * 3 * n;
  centers += (size_t)b * 3 * m;
  const BqPoints p = bq_points<kUseLds>(points, n, s_pts);
  if (kUseLds) __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * kBqCentresPerBlock;
  const int j1 = min(j0 + kBqCentresPerBlock, m);
  for (int j = j0 + wave; j < j1; j += kBqBlock / kWave) {
    int32_t *o[S];
#pragma unroll
    for (int s = 0; s < S; ++s) o[s] = a.out[s] + ((size_t)b * m + j) * (size_t)a.u[s];
    ball_query_scan<S>(p, n, centers[j], centers[j + m], centers[j + 2 * m], a.r2, a.u, o, lane);
  }
}

template <int S>
void launch_ball_query_multi(const float *centers, const float *points, int b, int n, int m, const BqScales &a,
                             hipStream_t s) {
  dim3 grid(ceil_div(m, kBqCentresPerBlock), b);
  if (bq_stage_points(n, 0)) {
    hipLaunchKernelGGL((ball_query_multi_kernel<true, S>), grid, dim3(kBqBlock), (size_t)3 * n * sizeof(float), s, centers,
                       points, n, m, a);
  } else {
    hipLaunchKernelGGL((ball_query_multi_kernel<false, S>), grid, dim3(kBqBlock), 0, s, centers, points, n, m, a);
  }
}

// -------------------------------------------------------------- grouping --
// Thread = 4 consecutive (centre, neighbour) slots; the 4 indices are loaded
// once and reused for a chunk of channels.  Stores are 16 B per lane.
constexpr int kGrpBlock = 256;
constexpr int kGrpChannelsPerBlock = 16;

__global__ __launch_bounds__(kGrpBlock) void grouping_kernel(const float *__restrict__ feat,
                                                             const int32_t *__restrict__ idx, int c, int n,
                                                             int mu, float *__restrict__ out) {
  const int b = blockIdx.z;
  feat += (size_t)b * c * n;
  idx += (size_t)b * mu;
  out += (size_t)b * c * mu;
  const int c0 = blockIdx.y * kGrpChannelsPerBlock;
  const int c1 = min(c0 + kGrpChannelsPerBlock, c);
  const int p = (blockIdx.x * kGrpBlock + threadIdx.x) * 4;
  if (p >= mu) return;
  if (p + 3 < mu && (mu & 3) == 0) {
    const int4 id = *reinterpret_cast<const int4 *>(idx + p);
    for (int l = c0; l < c1; ++l) {
      const float *f = feat + (size_t)l * n;
      float4 v = make_float4(f[id.x], f[id.y], f[id.z], f[id.w]);
      *reinterpret_cast<float4 *>(out + (size_t)l * mu + p) = v;
    }
  } else {
    for (int q = p; q < min(p + 4, mu); ++q) {
      const int id = idx[q];
      for (int l = c0; l < c1; ++l) out[(size_t)l * mu + q] = feat[(size_t)l * n + id];
    }
  }
}

__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ feat,
                                                     const int32_t *__restrict__ idx, int c, int n, int m,
                                                     float *__restrict__ out) {
  const int b = blockIdx.z, l = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  out[((size_t)b * c + l) * m + j] = feat[((size_t)b * c + l) * n + idx[(size_t)b * m + j]];
}

// -------------------------------------------------- 3-NN + interpolation --
__global__ __launch_bounds__(256) void three_nn_kernel(const float *__restrict__ points,
                                                       const float *__restrict__ centers, int n, int m,
                                                       int32_t *__restrict__ idx, float *__restrict__ wgt) {
  extern __shared__ float s_c[];  // [3][m]
  const int b = blockIdx.y;
  points += (size_t)b * 3 * n;
  centers += (size_t)b * 3 * m;
  idx += (size_t)b * 3 * n;
  wgt += (size_t)b * 3 * n;
  for (int i = threadIdx.x; i < 3 * m; i += 256) s_c[i] = centers[i];
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float ux = points[j], uy = points[j + n], uz = points[j + 2 * n];
  double best0 = 1e40, best1 = 1e40, best2 = 1e40;
  int i0 = 0, i1 = 0, i2 = 0;
  for (int k = 0; k < m; ++k) {
    const float cx = s_c[k], cy = s_c[k + m], cz = s_c[k + 2 * m];
    const float d = (ux - cx) * (ux - cx) + (uy - cy) * (uy - cy) + (uz - cz) * (uz - cz);
    if (d < best2) {
      best2 = d; i2 = k;
      if (d < best1) {
        best2 = best1; i2 = i1;
        best1 = d; i1 = k;
        if (d < best0) {
          best1 = best0; i1 = i0;
          best0 = d; i0 = k;
        }
      }
    }
  }
  best0 = fmax(fmin((double)1e10f, best0), (double)1e-10f);
  best1 = fmax(fmin((double)1e10f, best1), (double)1e-10f);
  best2 = fmax(fmin((double)1e10f, best2), (double)1e-10f);
  const float d0d1 = (float)(best0 * best1);
  const float d0d2 = (float)(best0 * best2);
  const float d1d2 = (float)(best1 * best2);
  const float inv = 1.0f / (d0d1 + d0d2 + d1d2);
  wgt[j] = d1d2 * inv;
  idx[j] = i0;
  wgt[j + n] = d0d2 * inv;
  idx[j + n] = i1;
  wgt[j + 2 * n] = d0d1 * inv;
  idx[j + 2 * n] = i2;
}

__global__ __launch_bounds__(256) void three_interp_kernel(const float *__restrict__ cfeat,
                                                           const int32_t *__restrict__ idx,
                                                           const float *__restrict__ wgt, int c, int m, int n,
                                                           float *__restrict__ out) {
  const int b = blockIdx.z;
  cfeat += (size_t)b * c * m;
  idx += (size_t)b * 3 * n;
  wgt += (size_t)b * 3 * n;
  out += (size_t)b * c * n;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float w1 = wgt[j], w2 = wgt[j + n], w3 = wgt[j + 2 * n];
  const int a1 = idx[j], a2 = idx[j + n], a3 = idx[j + 2 * n];
  const int c0 = blockIdx.y * 16, c1 = min(c0 + 16, c);
  for (int l = c0; l < c1; ++l) {
    const float *f = cfeat + (size_t)l * m;
    out[(size_t)l * n + j] = f[a1] * w1 + f[a2] * w2 + f[a3] * w3;
  }
}

// ------------------------------------------------- fused SA gather ---------
// BallQuery.forward as one kernel.  Block = centres_per_block centres of one cloud:
//   phase 1: wave-per-centre ordered ball query (ball_query_scan at one scale; points staged in LDS when
//            bq_stage_points allows), centres and neighbour indices stay in LDS;
//   phase 2: every channel row of the grouped tensor for these centres is a
//            contiguous run of centres_per_block*u floats in HBM -> 16-byte coalesced
//            stores; reads are index gathers served from L2 (the per-cloud
//            feature slab is <= 512 KiB and shared by all blocks of the cloud).
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <bool kUseLds>
__global__ __launch_bounds__(kBqBlock) void sa_group_kernel(const float *__restrict__ points,
                                                            const float *__restrict__ centers,
                                                            const float *__restrict__ feat, int c, int n, int m,
                                                            float r2, int u, int centres_per_block,
                                                            float *__restrict__ out,
                                                            int32_t *__restrict__ idx_out) {
  extern __shared__ float s_mem[];
  const int b = blockIdx.y;
  points += (size_t)b * 3 * n;
  centers += (size_t)b * 3 * m;
  if (feat) feat += (size_t)b * c * n;
  out += (size_t)b * (3 + c) * m * u;
  const int j0 = blockIdx.x * centres_per_block;
  const int nj = min(centres_per_block, m - j0);
  int32_t *s_idx = reinterpret_cast<int32_t *>(s_mem);       // [centres_per_block*u]
  float *s_ctr = s_mem + centres_per_block * u;              // [3][centres_per_block]
  float *s_pts = s_ctr + 3 * centres_per_block;              // [3][n] (kUseLds)
  const BqPoints pt = bq_points<kUseLds>(points, n, s_pts);
  for (int i = threadIdx.x; i < 3 * nj; i += kBqBlock) {
    const int a = i / nj, jj = i - a * nj;
    s_ctr[a * centres_per_block + jj] = centers[a * m + j0 + jj];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int jj = wave; jj < nj; jj += kBqBlock / kWave) {
    ball_query_one(pt, n, s_ctr[jj], s_ctr[centres_per_block + jj], s_ctr[2 * centres_per_block + jj], r2, u,
                   s_idx + jj * u, lane);
  }
  __syncthreads();
  const int run = nj * u;  // contiguous floats per channel row for this block
  if (idx_out) {
    int32_t *io = idx_out + ((size_t)b * m + j0) * u;
    for (int p = threadIdx.x; p < run; p += kBqBlock) io[p] = s_idx[p];
  }
  const size_t mu = (size_t)m * u;
  float *obase = out + (size_t)j0 * u;
  // coordinate rows: neighbour minus centre
  for (int p = threadIdx.x; p < 3 * run; p += kBqBlock) {
    const int a = p / run, q = p - a * run;
    const int id = s_idx[q];
    const int jj = q / u;
    const float v = (a == 0 ? pt.x[id] : (a == 1 ? pt.y[id] : pt.z[id])) - s_ctr[a * centres_per_block + jj];
    obase[(size_t)a * mu + q] = v;
  }
  // feature rows
  if (feat) {
    if ((run & 3) == 0 && (mu & 3) == 0) {
      const int run4 = run >> 2;
      for (int p = threadIdx.x; p < run4; p += kBqBlock) {
        const int4 id = *reinterpret_cast<const int4 *>(s_idx + 4 * p);
        float *o = obase + 3 * mu + 4 * p;
#pragma unroll 4
        for (int l = 0; l < c; ++l) {
          const float *f = feat + (size_t)l * n;
          f32x4_t v = {f[id.x], f[id.y], f[id.z], f[id.w]};
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t *>(o + (size_t)l * mu));  // streamed once
        }
      }
    } else {
      for (int p = threadIdx.x; p < run; p += kBqBlock) {
        const int id = s_idx[p];
        for (int l = 0; l < c; ++l) obase[(3 + (size_t)l) * mu + p] = feat[(size_t)l * n + id];
      }
    }
  }
}

}  // namespace

// =========================================================== C ABI =========

GLDM_API int gldm_ball_query(const float *centers, const float *points, int b, int n, int m, float radius, int u,
                             int32_t *out, gldm_stream_t stream) {
  if (!centers || !points || !out || b <= 0 || n <= 0 || m <= 0 || u <= 0) return GLDM_ERR_INVALID_ARG;
  BqScales a{};
  a.r2[0] = radius * radius;
  a.u[0] = u;
  a.out[0] = out;
  launch_ball_query_multi<1>(centers, points, b, n, m, a, as_stream(stream));
  return launch_status();
}

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

GLDM_API int gldm_sa_group(const float *points, const float *centers, const float *features, int b, int c, int n,
                           int m, float radius, int u, float *out, int32_t *idx_out, gldm_stream_t stream) {
  if (!points || !centers || !out || b <= 0 || c < 0 || n <= 0 || m <= 0 || u <= 0) return GLDM_ERR_INVALID_ARG;
  if (c > 0 && !features) return GLDM_ERR_INVALID_ARG;
  const float r2 = radius * radius;
  // 16 centres per block: every thread owns one 16-byte slot of each channel row's 4 KiB run
  // (u = 64); measured best of {4, 8, 16, 32} on MI355X (tools/bench_point_ops.py).
  int cpb = 16;
#ifdef GLDM_DEBUG_KNOBS
  {
    const char *e = getenv("GLDM_SA_CPB");  // tuning knob (diagnostic builds only)
    if (e) cpb = atoi(e);
  }
#endif
  while (cpb > 1 && (size_t)cpb * u * sizeof(int32_t) > 32 * 1024) cpb >>= 1;
  const size_t fixed = (size_t)cpb * u * sizeof(int32_t) + (size_t)3 * cpb * sizeof(float);
  dim3 grid(ceil_div(m, cpb), b);
  const float *f = c > 0 ? features : nullptr;
  if (bq_stage_points(n, fixed)) {
    hipLaunchKernelGGL(sa_group_kernel<true>, grid, dim3(kBqBlock), fixed + (size_t)3 * n * sizeof(float),
                       as_stream(stream), points, centers, f, c, n, m, r2, u, cpb, out, idx_out);
  } else {
    hipLaunchKernelGGL(sa_group_kernel<false>, grid, dim3(kBqBlock), fixed, as_stream(stream), points, centers, f,
                       c, n, m, r2, u, cpb, out, idx_out);
  }
  return launch_status();
}

GLDM_API int gldm_grouping_forward(const float *features, const int32_t *idx, int b, int c, int n, int m, int u,
                                   float *out, gldm_stream_t stream) {
  if (!features || !idx || !out || b <= 0 || c <= 0 || n <= 0 || m <= 0 || u <= 0) return GLDM_ERR_INVALID_ARG;
  const int mu = m * u;
  dim3 grid(ceil_div(ceil_div(mu, 4), kGrpBlock), ceil_div(c, kGrpChannelsPerBlock), b);
  hipLaunchKernelGGL(grouping_kernel, grid, dim3(kGrpBlock), 0, as_stream(stream), features, idx, c, n, mu, out);
  return launch_status();
}

GLDM_API int gldm_gather_features_forward(const float *features, const int32_t *idx, int b, int c, int n, int m,
                                          float *out, gldm_stream_t stream) {
  if (!features || !idx || !out || b <= 0 || c <= 0 || n <= 0 || m <= 0) return GLDM_ERR_INVALID_ARG;
  dim3 grid(ceil_div(m, 256), c, b);
  hipLaunchKernelGGL(gather_kernel, grid, dim3(256), 0, as_stream(stream), features, idx, c, n, m, out);
  return launch_status();
}

GLDM_API int gldm_three_nn_interpolate_forward(const float *points, const float *centers,
                                               const float *center_features, int b, int c, int m, int n,
                                               float *out, int32_t *idx, float *wgt, gldm_stream_t stream) {
  if (!points || !centers || !center_features || !out || !idx || !wgt || b <= 0 || c <= 0 || m <= 0 || n <= 0)
    return GLDM_ERR_INVALID_ARG;
  if ((size_t)3 * m * sizeof(float) > 64 * 1024) return GLDM_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(three_nn_kernel, dim3(ceil_div(n, 256), b), dim3(256), (size_t)3 * m * sizeof(float), s,
                     points, centers, n, m, idx, wgt);
  int st = launch_status();
  if (st != GLDM_OK) return st;
  hipLaunchKernelGGL(three_interp_kernel, dim3(ceil_div(n, 256), ceil_div(c, 16), b), dim3(256), 0, s,
                     center_features, idx, wgt, c, m, n, out);
  return launch_status();
}
