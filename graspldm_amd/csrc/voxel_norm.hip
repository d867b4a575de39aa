// voxel_norm.hip -- what follows the voxel convs of PVConv (ext/pvcnn/modules/pvconv.py:47-84), and the GroupNorm family:
//   gldm_groupnorm_swish                GroupNorm(8) + Swish in place, statistics from the convs' per-brick partials (voxel_geom.h)
//   gldm_groupnorm_coef                 the same norm as coefficients (a, s) per (cloud, channel), applied by whoever reads the
//                                       raw conv output: the next conv's staging (conv3d.hip) and the three below
//   gldm_gn_swish_chan_sum[_cl]         the SE squeeze of swish(a x + s), never written
//   gldm_se_gate[_parts]                SE gate (se.py:12-25)
//   gldm_devoxelize_[gn_[cl_]]fused     trilinear devoxelize x gate + point-branch features
//   gldm_groupnorm_affine               x = a y + s over the grid: the norm without the activation
//   gldm_groupnorm_swish_points[_sum]   GroupNorm + Swish over point features [b, c, n] (+ residual, + per-channel sums):
//                                       the norms of the attention blocks
#include "mfma_prims.h"
#include "voxel_geom.h"

namespace {

// GroupNorm(groups) + Swish over [B, C, r^3]; statistics from the conv's per-brick partials.
// grid = (groups, B); optional per-channel sum of the OUTPUT (for the SE squeeze).
__global__ __launch_bounds__(512) void groupnorm_swish_kernel(float *__restrict__ y, const float *__restrict__ partial,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, int c, int r3,
                                                              int nbricks, int groups, float eps,
                                                              float *__restrict__ chan_sum) {
  __shared__ double s_stat[2];
  __shared__ float s_red[8];
  const int g = blockIdx.x, b = blockIdx.y, cpg = c / groups;
  const int tid = threadIdx.x;
  if (tid < 64) {
    double s = 0.0, s2 = 0.0;
    for (int i = tid; i < nbricks * cpg; i += 64) {
      const int br = i / cpg, ch = g * cpg + i % cpg;
      const float *p = partial + (((size_t)b * nbricks + br) * c + ch) * 2;
      s += (double)p[0];
      s2 += (double)p[1];
    }
    for (int off = 32; off >= 1; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    if (tid == 0) {
      const double n = (double)cpg * r3, mean = s / n;
      s_stat[0] = mean;
      s_stat[1] = 1.0 / sqrt(fmax(s2 / n - mean * mean, 0.0) + (double)eps);
    }
  }
  __syncthreads();
  const float mean = (float)s_stat[0], rstd = (float)s_stat[1];
  for (int cc = 0; cc < cpg; ++cc) {
    const int ch = g * cpg + cc;
    float *row = y + ((size_t)b * c + ch) * r3;
    const float ga = gamma[ch] * rstd, be = beta[ch] - mean * rstd * gamma[ch];
    float acc = 0.f;
    const int n4 = (r3 & 3) ? 0 : r3 >> 2;   // rows are 16-byte aligned only when r^3 is a multiple of 4
    if (r3 & 3) {
      for (int i = tid; i < r3; i += 512) {
        const float t = row[i] * ga + be;
        const float o = t / (1.0f + __expf(-t));
        acc += o;
        row[i] = o;
      }
    }
    for (int i = tid; i < n4; i += 512) {
      float4 v = reinterpret_cast<float4 *>(row)[i];
      float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float t = o[q] * ga + be;
        o[q] = t / (1.0f + __expf(-t));
        acc += o[q];
      }
      reinterpret_cast<float4 *>(row)[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (chan_sum) {
      for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
      __syncthreads();
      if ((tid & 63) == 0) s_red[tid >> 6] = acc;
      __syncthreads();
      if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < 8; ++w) t += s_red[w];
        chan_sum[(size_t)b * c + ch] = t;
      }
    }
  }
}

// SE gate: gate = sigmoid(W2 act(W1 mean)), W1 [c/red, c], W2 [c, c/red]; one block per cloud.
__global__ void se_gate_kernel(const float *__restrict__ chan_sum, const float *__restrict__ w1,
                               const float *__restrict__ w2, int c, int hid, int r3, int use_relu,
                               float *__restrict__ gate, int parts) {
  extern __shared__ float s[];  // mean[c], h[hid]
  const int b = blockIdx.x, tid = threadIdx.x;
  float *mean = s, *h = s + c;
  // chan_sum [b][parts][c]: partial sums of the squeeze, added in index order
  for (int i = tid; i < c; i += blockDim.x) {
    float t = chan_sum[(size_t)b * parts * c + i];
    for (int p = 1; p < parts; ++p) t += chan_sum[((size_t)b * parts + p) * c + i];
    mean[i] = t / (float)r3;
  }
  __syncthreads();
  for (int i = tid; i < hid; i += blockDim.x) {
    float a = 0.f;
    for (int q = 0; q < c; ++q) a += w1[i * c + q] * mean[q];
    h[i] = use_relu ? fmaxf(a, 0.f) : a / (1.0f + expf(-a));
  }
  __syncthreads();
  for (int i = tid; i < c; i += blockDim.x) {
    float a = 0.f;
    for (int q = 0; q < hid; ++q) a += w2[i * hid + q] * h[q];
    gate[(size_t)b * c + i] = 1.0f / (1.0f + expf(-a));
  }
}

// GroupNorm as per-(cloud, channel) coefficients: y = a x + s with a = gamma rstd, s = beta - mean a; statistics from the
// conv's per-brick partials, combined in f64 in a fixed order exactly as groupnorm_swish_kernel does.  grid = (groups, B).
__global__ __launch_bounds__(64) void groupnorm_coef_kernel(const float *__restrict__ partial, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, int c, int r3, int nbricks,
                                                            int groups, float eps, float *__restrict__ coef) {
  const int g = blockIdx.x, b = blockIdx.y, cpg = c / groups, tid = threadIdx.x;
  double s = 0.0, s2 = 0.0;
  for (int i = tid; i < nbricks * cpg; i += 64) {
    const int br = i / cpg, ch = g * cpg + i % cpg;
    const float *p = partial + (((size_t)b * nbricks + br) * c + ch) * 2;
    s += (double)p[0];
    s2 += (double)p[1];
  }
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
  const double n = (double)cpg * r3, mean_d = s / n;
  const float mean = (float)mean_d, rstd = (float)(1.0 / sqrt(fmax(s2 / n - mean_d * mean_d, 0.0) + (double)eps));
  for (int i = tid; i < cpg; i += 64) {   // one trip up to 64 channels per group; the voxel attention stack goes to 128
    const int ch = g * cpg + i;
    const float a = gamma[ch] * rstd;
    coef[((size_t)b * c + ch) * 2] = a;
    coef[((size_t)b * c + ch) * 2 + 1] = beta[ch] - mean * rstd * gamma[ch];
  }
}

__device__ __forceinline__ float swish_fast(float t) {
  return t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * t));
}

// chan_sum[b][ch] = sum over the voxels of swish(a x + s): the SE squeeze of a GroupNorm + Swish output that is never
// written (read-only pass; the consumers apply the same map on the fly).  grid = (C, B), rows of r^3 floats.
__global__ __launch_bounds__(256) void gn_swish_sum_kernel(const float *__restrict__ y, const float *__restrict__ coef, int c,
                                                           int r3, float *__restrict__ chan_sum) {
  __shared__ float s_red[4];
  const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float *row = y + ((size_t)b * c + ch) * r3;
  const float a = coef[((size_t)b * c + ch) * 2], s = coef[((size_t)b * c + ch) * 2 + 1];
  float acc = 0.f;
  if ((r3 & 3) == 0) {
    const float4 *row4 = reinterpret_cast<const float4 *>(row);
    for (int i = tid; i < (r3 >> 2); i += 256) {
      const float4 v = row4[i];
      acc += swish_fast(fmaf(v.x, a, s)) + swish_fast(fmaf(v.y, a, s)) + swish_fast(fmaf(v.z, a, s)) + swish_fast(fmaf(v.w, a, s));
    }
  } else {
    for (int i = tid; i < r3; i += 256) acc += swish_fast(fmaf(row[i], a, s));
  }
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) chan_sum[(size_t)b * c + ch] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// The same squeeze over a channel-LAST tensor [b][r^3][c]: block (part, b) sums its share of the voxels for every channel
// (thread = (voxel stripe, channel quad), 16-byte loads), parts[b][part][c] leaves; se_gate_kernel adds the parts in order.
__global__ __launch_bounds__(256) void gn_swish_sum_cl_kernel(const float *__restrict__ y, const float *__restrict__ coef, int c,
                                                              int r3, float *__restrict__ parts) {
  __shared__ f32x4 s_acc[256];
  const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int quads = c >> 2, stripes = 256 / quads;          // threads beyond stripes * quads idle
  const int qd = tid % quads, stripe = tid / quads;
  const int v0 = (int)((long long)r3 * part / kSumParts), v1 = (int)((long long)r3 * (part + 1) / kSumParts);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (stripe < stripes) {
    const f32x4 *cf = reinterpret_cast<const f32x4 *>(coef + ((size_t)b * c + 4 * qd) * 2);
    const f32x4 c01 = cf[0], c23 = cf[1];   // (a0, s0, a1, s1), (a2, s2, a3, s3)
    const f32x4 *row = reinterpret_cast<const f32x4 *>(y + (size_t)b * r3 * c) + qd;
    for (int v = v0 + stripe; v < v1; v += stripes) {
      const f32x4 x = row[(size_t)v * quads];
      acc[0] += swish_fast(fmaf(x[0], c01[0], c01[1]));
      acc[1] += swish_fast(fmaf(x[1], c01[2], c01[3]));
      acc[2] += swish_fast(fmaf(x[2], c23[0], c23[1]));
      acc[3] += swish_fast(fmaf(x[3], c23[2], c23[3]));
    }
  }
  s_acc[tid] = acc;
  __syncthreads();
  if (tid < quads) {
    f32x4 t = s_acc[tid];
    for (int st = 1; st < stripes; ++st) {
      const f32x4 o = s_acc[st * quads + tid];
      t[0] += o[0]; t[1] += o[1]; t[2] += o[2]; t[3] += o[3];
    }
    *reinterpret_cast<f32x4 *>(parts + ((size_t)b * kSumParts + part) * c + 4 * tid) = t;
  }
}

// devoxelize_fused_kernel over a channel-LAST raw conv output [b][r^3][c] (coef required): a point's corner is ONE run of
// c floats, read as 16-byte loads by c / 4 neighbouring lanes, instead of c dword gathers from c cache lines (the
// channel-major form is bound by the address path: 64 lines per wave instruction, 0.24 ms per 48 x 24^3 x 256 clouds).
// Block = 64 points; item = (point, channel quad); the results cross LDS so that the stores (and the reads of `add`) run
// along the points.  c % 4 == 0, c <= 256.
__global__ __launch_bounds__(256) void devoxelize_cl_kernel(const float *__restrict__ coords, const float *__restrict__ feat,
                                                            const float *__restrict__ coef, const float *__restrict__ gate,
                                                            const float *__restrict__ add, int c, int n, int r,
                                                            float *__restrict__ outs) {
  extern __shared__ float s_tile[];   // [c][65]
  const int b = blockIdx.y, p0 = blockIdx.x * 64, tid = threadIdx.x;
  const int r2 = r * r, r3 = r2 * r, quads = c >> 2;
  coords += (size_t)b * 3 * n;
  const f32x4 *f4 = reinterpret_cast<const f32x4 *>(feat + (size_t)b * r3 * c);
  for (int it = tid; it < 64 * quads; it += 256) {
    const int pt = it / quads, qd = it - pt * quads;
    const int i = min(p0 + pt, n - 1);
    float w[8];
    int idx[8];
    trilinear_corners(coords[i], coords[i + n], coords[i + 2 * n], r, w, idx);
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = f4[(size_t)idx[k] * quads + qd];
    const f32x4 *cf = reinterpret_cast<const f32x4 *>(coef + ((size_t)b * c + 4 * qd) * 2);
    const f32x4 c01 = cf[0], c23 = cf[1];
    const float ca[4] = {c01[0], c01[2], c23[0], c23[2]}, cs[4] = {c01[1], c01[3], c23[1], c23[3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) o += w[k] * swish_fast(fmaf(v[k][q], ca[q], cs[q]));
      s_tile[(4 * qd + q) * 65 + pt] = o;
    }
  }
  __syncthreads();
  for (int e = tid; e < c * 64; e += 256) {
    const int ch = e >> 6, pt = e & 63;
    if (p0 + pt < n) {
      const float gt = gate ? gate[(size_t)b * c + ch] : 1.0f;
      const size_t o = ((size_t)b * c + ch) * n + p0 + pt;
      outs[o] = gt * s_tile[ch * 65 + pt] + (add ? add[o] : 0.f);
    }
  }
}

// out[b,c,i] = gate[b,c] * trilinear(V[b,c], coords[b,:,i]) + add[b,c,i]
__global__ __launch_bounds__(256) void devoxelize_fused_kernel(const float *__restrict__ coords,
                                                               const float *__restrict__ feat,
                                                               const float *__restrict__ gate,
                                                               const float *__restrict__ add, int c, int n, int r,
                                                               float *__restrict__ outs,
                                                               const float *__restrict__ coef) {
  // coef != NULL: `feat` is a raw conv output and GroupNorm + Swish are applied to the 8 corners on the fly
  // (swish(a f + s), (a, s) per cloud and channel: groupnorm_coef_kernel)
  const int b = blockIdx.z;
  const int r2 = r * r, r3 = r2 * r;
  coords += (size_t)b * 3 * n;
  feat += (size_t)b * c * r3;
  outs += (size_t)b * c * n;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float w[8];
  int id[8];
  trilinear_corners(coords[i], coords[i + n], coords[i + 2 * n], r, w, id);
  const int c0 = blockIdx.y * 16, c1 = min(c0 + 16, c);
  for (int l = c0; l < c1; ++l) {
    const float *f = feat + (size_t)l * r3;
    float f0 = f[id[0]], f1 = f[id[1]], f2 = f[id[2]], f3 = f[id[3]], f4 = f[id[4]], f5 = f[id[5]], f6 = f[id[6]], f7 = f[id[7]];
    if (coef) {
      const float a = coef[((size_t)b * c + l) * 2], s = coef[((size_t)b * c + l) * 2 + 1];
      f0 = swish_fast(fmaf(f0, a, s)); f1 = swish_fast(fmaf(f1, a, s)); f2 = swish_fast(fmaf(f2, a, s));
      f3 = swish_fast(fmaf(f3, a, s)); f4 = swish_fast(fmaf(f4, a, s)); f5 = swish_fast(fmaf(f5, a, s));
      f6 = swish_fast(fmaf(f6, a, s)); f7 = swish_fast(fmaf(f7, a, s));
    }
    const float v = w[0] * f0 + w[1] * f1 + w[2] * f2 + w[3] * f3 + w[4] * f4 + w[5] * f5 + w[6] * f6 + w[7] * f7;
    const float gt = gate ? gate[(size_t)b * c + l] : 1.0f;
    const float ad = add ? add[((size_t)b * c + l) * n + i] : 0.f;
    outs[(size_t)l * n + i] = gt * v + ad;
  }
}

// ---- x = a y + s per (cloud, channel) over a voxel grid: GroupNorm WITHOUT the activation ---------------------------------
__global__ __launch_bounds__(256) void gn_affine_kernel(const float *__restrict__ y, const float *__restrict__ coef, int quads,
                                                        float *__restrict__ x) {
  const size_t row = blockIdx.x;   // cloud * c + channel
  const float a = coef[2 * row], s = coef[2 * row + 1];
  const f32x4 *y4 = (const f32x4 *)y + row * quads;
  f32x4 *x4 = (f32x4 *)x + row * quads;
  for (int i = blockIdx.y * 256 + threadIdx.x; i < quads; i += gridDim.y * 256) {
    f32x4 t = y4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = __builtin_fmaf(a, t[e], s);
    x4[i] = t;
  }
}

// ---- GroupNorm + Swish over [b, c, n] (+ a residual in front) -----------------------------------------------------------
// A workgroup per (cloud, group): the group's channels are one contiguous run of (c / groups) n floats.  Statistics of
// x (+ add) in f64, per-thread partial sums in index order and a fixed tree over the threads.
// gn_points_stats is that pass, for both kernels below (256 threads; red is the calling kernel's): what makes
// gldm_groupnorm_swish_points_sum's output the bits of gldm_groupnorm_swish_points'.
__device__ __forceinline__ void gn_points_stats(const f32x4 *x4, const f32x4 *a4, int quads, double cnt, float eps,
                                                double (&red)[2][256], double &mean, double &rstd) {
  const int tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < quads; i += 256) {
    f32x4 v = x4[i];
    if (a4) v += a4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s1 += (double)v[e];
      s2 += (double)v[e] * (double)v[e];
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  mean = red[0][0] / cnt;
  double var = red[1][0] / cnt - mean * mean;
  var = var > 0.0 ? var : 0.0;
  rstd = 1.0 / sqrt(var + (double)eps);
}

__global__ __launch_bounds__(256) void gn_swish_points_kernel(const float *x, const float *add, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, int c, int n, int groups, float eps,
                                                              float *out) {
  __shared__ double red[2][256];
  const int cg = c / groups, tid = threadIdx.x;
  const size_t base = ((size_t)blockIdx.y * c + (size_t)blockIdx.x * cg) * n;
  const int quads = cg * (n / 4);
  const f32x4 *x4 = (const f32x4 *)(x + base), *a4 = add ? (const f32x4 *)(add + base) : nullptr;
  double mean, rstd;
  gn_points_stats(x4, a4, quads, (double)cg * n, eps, red, mean, rstd);
  f32x4 *o4 = (f32x4 *)(out + base);
  const int qpc = n / 4;   // a 16-byte run stays inside one channel
  for (int i = tid; i < quads; i += 256) {
    const int ch = blockIdx.x * cg + i / qpc;
    const float a = (float)((double)gamma[ch] * rstd), s = (float)((double)beta[ch] - mean * (double)gamma[ch] * rstd);
    f32x4 v = x4[i];
    if (a4) v += a4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = __builtin_fmaf(a, v[e], s);
      v[e] = t / (1.0f + expf(-t));
    }
    o4[i] = v;
  }
}

// ---- GroupNorm + Swish over [b, c, n] (+ a residual in front) with the per-channel sums of the OUTPUT ------------------------
// The same statistics (gn_points_stats: a workgroup per (cloud, group), f64, fixed tree); the second pass is a wave per
// channel, so that a channel's sum is one wave's: lanes add their quads in index order (f64), then a fixed shuffle tree.
__global__ __launch_bounds__(256) void gn_swish_points_sum_kernel(const float *x, const float *add, const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, int c, int n, int groups, float eps,
                                                                  float *out, float *__restrict__ chan_sum) {
  __shared__ double red[2][256];
  const int cg = c / groups, tid = threadIdx.x;
  const size_t base = ((size_t)blockIdx.y * c + (size_t)blockIdx.x * cg) * n;
  const int quads = cg * (n / 4);
  const f32x4 *x4 = (const f32x4 *)(x + base), *a4 = add ? (const f32x4 *)(add + base) : nullptr;
  double mean, rstd;
  gn_points_stats(x4, a4, quads, (double)cg * n, eps, red, mean, rstd);
  f32x4 *o4 = (f32x4 *)(out + base);
  const int qpc = n / 4, wave = tid >> 6, lane = tid & 63;
  for (int cl = wave; cl < cg; cl += 4) {
    const int ch = blockIdx.x * cg + cl;
    const float a = (float)((double)gamma[ch] * rstd), s = (float)((double)beta[ch] - mean * (double)gamma[ch] * rstd);
    double sum = 0.0;
    for (int i = lane; i < qpc; i += 64) {
      f32x4 v = x4[cl * qpc + i];
      if (a4) v += a4[cl * qpc + i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = __builtin_fmaf(a, v[e], s);
        v[e] = t / (1.0f + expf(-t));
        sum += (double)v[e];
      }
      o4[cl * qpc + i] = v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) chan_sum[(size_t)blockIdx.y * c + ch] = (float)sum;
  }
}

}  // namespace

GLDM_API int gldm_groupnorm_coef(const float *partial, const float *gamma, const float *beta, int b, int c, int r, int groups,
                                 float eps, float *coef, gldm_stream_t stream) {
  if (!partial || !gamma || !beta || !coef || b <= 0 || c <= 0 || r <= 0 || groups <= 0 || c % groups || c / groups > 128)
    return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(groupnorm_coef_kernel, dim3(groups, b), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), partial, gamma,
                     beta, c, r * r * r, bricks_per_cloud(r), groups, eps, coef);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_gn_swish_chan_sum(const float *y, const float *coef, int b, int c, int r, float *chan_sum,
                                    gldm_stream_t stream) {
  if (!y || !coef || !chan_sum || b <= 0 || c <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(gn_swish_sum_kernel, dim3(c, b), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, coef, c,
                     r * r * r, chan_sum);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_groupnorm_swish(float *y, const float *partial, const float *gamma, const float *beta, int b, int c,
                                  int r, int groups, float eps, float *chan_sum, gldm_stream_t stream) {
  if (!y || !partial || !gamma || !beta || b <= 0 || c <= 0 || r <= 0 || groups <= 0 || c % groups)
    return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(groupnorm_swish_kernel, dim3(groups, b), dim3(512), 0, reinterpret_cast<hipStream_t>(stream), y,
                     partial, gamma, beta, c, r * r * r, bricks_per_cloud(r), groups, eps, chan_sum);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_se_gate(const float *chan_sum, const float *w1, const float *w2, int b, int c, int hidden, int r,
                          int use_relu, float *gate, gldm_stream_t stream) {
  if (!chan_sum || !w1 || !w2 || !gate || b <= 0 || c <= 0 || hidden <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(se_gate_kernel, dim3(b), dim3(128), (size_t)(c + hidden) * sizeof(float),
                     reinterpret_cast<hipStream_t>(stream), chan_sum, w1, w2, c, hidden, r * r * r, use_relu, gate, 1);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_se_gate_parts(const float *chan_parts, int parts, const float *w1, const float *w2, int b, int c, int hidden,
                                int r, int use_relu, float *gate, gldm_stream_t stream) {
  if (!chan_parts || !w1 || !w2 || !gate || b <= 0 || c <= 0 || hidden <= 0 || r <= 0 || parts <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(se_gate_kernel, dim3(b), dim3(128), (size_t)(c + hidden) * sizeof(float),
                     reinterpret_cast<hipStream_t>(stream), chan_parts, w1, w2, c, hidden, r * r * r, use_relu, gate, parts);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_squeeze_parts(void) { return kSumParts; }

GLDM_API int gldm_gn_swish_chan_sum_cl(const float *y, const float *coef, int b, int c, int r, float *chan_parts,
                                       gldm_stream_t stream) {
  if (!y || !coef || !chan_parts || b <= 0 || c <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  if (c % 4 || c > 1024) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gn_swish_sum_cl_kernel, dim3(kSumParts, b), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, coef, c,
                     r * r * r, chan_parts);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_devoxelize_gn_cl_fused(const float *coords, const float *features_cl, const float *coef, const float *gate,
                                         const float *add, int b, int c, int n, int r, float *out, gldm_stream_t stream) {
  if (!coords || !features_cl || !coef || !out || b <= 0 || c <= 0 || n <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  if (c % 4 || c > 256) return GLDM_ERR_UNSUPPORTED;
  struct DevoxClTag { int site; };
  gldm_dev::allow_dynamic_lds<DevoxClTag>(reinterpret_cast<const void *>(&devoxelize_cl_kernel), 256 * 65 * (int)sizeof(float));
  hipLaunchKernelGGL(devoxelize_cl_kernel, dim3((n + 63) / 64, b), dim3(256), (size_t)c * 65 * sizeof(float),
                     reinterpret_cast<hipStream_t>(stream), coords, features_cl, coef, gate, add, c, n, r, out);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_devoxelize_fused(const float *coords, const float *features, const float *gate, const float *add,
                                   int b, int c, int n, int r, float *out, gldm_stream_t stream) {
  if (!coords || !features || !out || b <= 0 || c <= 0 || n <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(devoxelize_fused_kernel, dim3((n + 255) / 256, (c + 15) / 16, b), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), coords, features, gate, add, c, n, r, out, nullptr);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_devoxelize_gn_fused(const float *coords, const float *features, const float *coef, const float *gate,
                                      const float *add, int b, int c, int n, int r, float *out, gldm_stream_t stream) {
  if (!coords || !features || !coef || !out || b <= 0 || c <= 0 || n <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(devoxelize_fused_kernel, dim3((n + 255) / 256, (c + 15) / 16, b), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), coords, features, gate, add, c, n, r, out, coef);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_groupnorm_affine(const float *y, const float *coef, int b, int c, int r, float *x, gldm_stream_t stream) {
  if (!y || !coef || !x || b <= 0 || c <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  if ((((size_t)y | (size_t)x) & 15)) return GLDM_ERR_INVALID_ARG;
  const long long vox = (long long)r * r * r;
  if (vox % 4 || r > 64 || (long long)b * c > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  const int quads = (int)(vox / 4);
  const int gx = quads >= 4096 ? 4 : 1;
  hipLaunchKernelGGL(gn_affine_kernel, dim3(b * c, gx), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, coef, quads, x);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_groupnorm_swish_points(const float *x, const float *add, const float *gamma, const float *beta, int b, int c,
                                         int n, int groups, float eps, float *out, gldm_stream_t stream) {
  if (!x || !gamma || !beta || !out || b <= 0 || c <= 0 || n <= 0 || groups <= 0) return GLDM_ERR_INVALID_ARG;
  if ((((size_t)x | (size_t)add | (size_t)out) & 15)) return GLDM_ERR_INVALID_ARG;   // 16-byte vector accesses
  if (c % groups || c / groups > 128 || n % 4 || b > 65535) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gn_swish_points_kernel, dim3(groups, b), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, add, gamma,
                     beta, c, n, groups, eps, out);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_groupnorm_swish_points_sum(const float *x, const float *add, const float *gamma, const float *beta, int b, int c,
                                             int n, int groups, float eps, float *out, float *chan_sum, gldm_stream_t stream) {
  if (!x || !gamma || !beta || !out || !chan_sum || b <= 0 || c <= 0 || n <= 0 || groups <= 0) return GLDM_ERR_INVALID_ARG;
  if ((((size_t)x | (size_t)add | (size_t)out) & 15)) return GLDM_ERR_INVALID_ARG;   // 16-byte vector accesses
  if (c % groups || c / groups > 128 || n % 4 || b > 65535) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gn_swish_points_sum_kernel, dim3(groups, b), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, add,
                     gamma, beta, c, n, groups, eps, out, chan_sum);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
