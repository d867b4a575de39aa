// voxel_points.hip -- gfx950 kernels of the point <-> voxel operators of PVConv's voxel branch, behind the C ABI declared
// in include/gldm.h: voxel coordinates of a cloud (gldm_voxel_coords), the scatter-mean of point features onto the grid
// (gldm_avg_voxelize_forward) and the trilinear read back (gldm_trilinear_devoxelize_forward).
//
//  * the voxel scatter-mean is deterministic: points are bitonic-sorted by (voxel, index) in LDS and each voxel is summed in
//    ascending point index;
//  * compiled with -ffp-contract=off so that the 8-corner sums and the means match the scalar oracle bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devstate.h"
#include "host_util.h"
#include "voxel_geom.h"

namespace {

constexpr int kWave = 64;

// -------------------------------------------------------- voxel coords ----
// One block per cloud: f64 tree mean per axis, optional max-norm scaling,
// clamp, round-half-even (rintf == torch.round).
constexpr int kVcBlock = 256;

__device__ __forceinline__ double block_sum_f64(double v, double *s_red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kVcBlock / kWave; ++w) t += s_red[w];
  return t;
}

__global__ __launch_bounds__(kVcBlock) void voxel_coords_kernel(const float *__restrict__ coords, int n, int r,
                                                                int normalize, float eps,
                                                                float *__restrict__ norm_coords,
                                                                int32_t *__restrict__ vox) {
  __shared__ double s_red[kVcBlock / kWave];
  __shared__ float s_max[kVcBlock / kWave];
  const int b = blockIdx.x;
  coords += (size_t)b * 3 * n;
  norm_coords += (size_t)b * 3 * n;
  vox += (size_t)b * 3 * n;
  float mean[3];
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kVcBlock) s += (double)coords[a * n + i];
    mean[a] = (float)(block_sum_f64(s, s_red) / (double)n);
  }
  float denom = 1.f;
  if (normalize) {
    float mx = 0.f;
    for (int i = threadIdx.x; i < n; i += kVcBlock) {
      const float x = coords[i] - mean[0], y = coords[n + i] - mean[1], z = coords[2 * n + i] - mean[2];
      mx = fmaxf(mx, sqrtf(x * x + y * y + z * z));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = 0.f;
    for (int w = 0; w < kVcBlock / kWave; ++w) mx = fmaxf(mx, s_max[w]);
    denom = mx * 2.0f + eps;
  }
  const float rf = (float)r, hi = (float)(r - 1);
  for (int i = threadIdx.x; i < 3 * n; i += kVcBlock) {
    const int a = i / n;
    float v = coords[i] - mean[a];
    v = normalize ? (v / denom + 0.5f) : ((v + 1.f) / 2.0f);
    v = fminf(fmaxf(v * rf, 0.f), hi);
    norm_coords[i] = v;
    vox[i] = (int32_t)rintf(v);
  }
}

// --------------------------------------------------------- avg voxelize ---
// grid = (channel chunks, clouds).  Each block sorts (voxel, point) keys in LDS, then every segment leader sums its
// voxel's points in ascending point index for the block's channels.
constexpr int kVoxBlock = 1024;
constexpr int kVoxChannelsPerBlock = 8;

// s_key[0..np2) = (voxel << log_np2) | point for the cloud's n points, all ones beyond them; the cloud's first block also
// writes each point's flat voxel index.  A barrier ends it.
__device__ __forceinline__ void vox_build_keys(const int32_t *vc, int n, int np2, int log_np2, int r, int r2,
                                               unsigned int *s_key, int32_t *ind) {
  for (int i = threadIdx.x; i < np2; i += kVoxBlock) {
    unsigned int key = 0xFFFFFFFFu;
    if (i < n) {
      const int v = vc[i] * r2 + vc[i + n] * r + vc[i + 2 * n];
      key = ((unsigned int)v << log_np2) | (unsigned int)i;
      if (blockIdx.x == 0) ind[i] = v;
    }
    s_key[i] = key;
  }
  __syncthreads();
}

// Ascending bitonic network over s_key[0..np2) in LDS, one barrier per stage; any np2.
__device__ __forceinline__ void vox_sort_keys_lds(unsigned int *s_key, int np2) {
  for (int size = 2; size <= np2; size <<= 1) {
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      for (int t = threadIdx.x; t < np2 / 2; t += kVoxBlock) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned int a = s_key[lo], bb = s_key[hi];
        if ((a > bb) == up) {
          s_key[lo] = bb;
          s_key[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// The segment-leader scan over the sorted keys: f(p, v, len) for every voxel v that holds points, p the position of its
// first key and len its points (their indices ascend with the position).
template <class F>
__device__ __forceinline__ void vox_for_each_voxel(const unsigned int *s_key, int n, int log_np2, F f) {
  for (int p = threadIdx.x; p < n; p += kVoxBlock) {
    const unsigned int v = s_key[p] >> log_np2;
    if (p > 0 && (s_key[p - 1] >> log_np2) == v) continue;  // not a segment leader
    int len = 1;
    while (p + len < n && (s_key[p + len] >> log_np2) == v) ++len;
    f(p, v, len);
  }
}

template <int kPerThread>
__global__ __launch_bounds__(kVoxBlock) void avg_voxelize_kernel(const float *__restrict__ feat,
                                                                 const int32_t *__restrict__ vc, int c, int n,
                                                                 int np2, int log_np2, int r,
                                                                 float *__restrict__ out,
                                                                 int32_t *__restrict__ ind,
                                                                 int32_t *__restrict__ cnt) {
  extern __shared__ unsigned int s_key[];  // [np2]
  const int b = blockIdx.y;
  const int r2 = r * r, r3 = r2 * r;
  feat += (size_t)b * c * n;
  vc += (size_t)b * 3 * n;
  out += (size_t)b * c * r3;
  ind += (size_t)b * n;
  cnt += (size_t)b * r3;
  vox_build_keys(vc, n, np2, log_np2, r, r2, s_key, ind);
  vox_sort_keys_lds(s_key, np2);
  const unsigned int imask = (1u << log_np2) - 1u;
  const int c0 = blockIdx.x * kVoxChannelsPerBlock, c1 = min(c0 + kVoxChannelsPerBlock, c);
  vox_for_each_voxel(s_key, n, log_np2, [&](int p, unsigned int v, int len) {
    if (blockIdx.x == 0) cnt[v] = len;
    const float div = (float)(1.0 / (double)(float)len);
    for (int l = c0; l < c1; ++l) {
      const float *f = feat + (size_t)l * n;
      float acc = 0.f;
      for (int q = 0; q < len; ++q) acc += f[s_key[p + q] & imask] * div;
      out[(size_t)l * r3 + v] = acc;
    }
  });
}

// The same scatter-mean with the grid assembled in LDS and written out DENSE: a block sorts its cloud's keys once,
// then walks its channels in rounds of G: zero a [G][r^3] grid in LDS, every segment leader puts its voxel's means
// there (the same sums in the same order as above), and the block writes the rows out with coalesced 16-byte stores.
// The output needs no memset and no scattered 4-byte stores: 0.157 -> see profiles (the 24^3 x 3 and 12^3 x 48 grids of the
// shipped encoder).  Block (0, b) also writes the dense count grid.  r^3 % 4 == 0, keys + one grid row within LDS.
__global__ __launch_bounds__(kVoxBlock) void avg_voxelize_dense_kernel(const float *__restrict__ feat,
                                                                       const int32_t *__restrict__ vc, int c, int n,
                                                                       int np2, int log_np2, int r, int chunk, int g_rows,
                                                                       int stage_feat, float *__restrict__ out,
                                                                       int32_t *__restrict__ ind,
                                                                       int32_t *__restrict__ cnt) {
  extern __shared__ unsigned int s_key[];  // [np2] keys, [np2] occupied-voxel list, a counter, then [g_rows][r^3] floats (+ features)
  const int b = blockIdx.y;
  const int r2 = r * r, r3 = r2 * r;
  feat += (size_t)b * c * n;
  vc += (size_t)b * 3 * n;
  out += (size_t)b * c * r3;
  ind += (size_t)b * n;
  cnt += (size_t)b * r3;
  const int tid = threadIdx.x;
  vox_build_keys(vc, n, np2, log_np2, r, r2, s_key, ind);
  if (np2 <= kVoxBlock) {
    // one key per thread, in a register: strides below the wave width are exchanged with shuffles (no barrier), the
    // others through LDS -- 10 barrier-separated stages instead of 55 for 1024 points
    unsigned int key = tid < np2 ? s_key[tid] : 0xFFFFFFFFu;
    for (int size = 2; size <= np2; size <<= 1) {
      const bool up = (tid & size) == 0;
      for (int stride = size >> 1; stride >= 1; stride >>= 1) {
        unsigned int other;
        if (stride >= kWave) {
          __syncthreads();   // the previous exchange's readers are done
          if (tid < np2) s_key[tid] = key;
          __syncthreads();
          other = tid < np2 ? s_key[tid ^ stride] : 0xFFFFFFFFu;
        } else {
          other = (unsigned int)__shfl_xor((int)key, stride, kWave);
        }
        const bool lower = (tid & stride) == 0;
        const unsigned int mn = key < other ? key : other, mx = key < other ? other : key;
        key = (lower == up) ? mn : mx;
      }
    }
    __syncthreads();
    if (tid < np2) s_key[tid] = key;
    __syncthreads();
  } else {
    vox_sort_keys_lds(s_key, np2);
  }
  const unsigned int imask = (1u << log_np2) - 1u;
  const int c0 = blockIdx.x * chunk, c1 = min(c0 + chunk, c);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // ---- the occupied voxels as a list (leader position | points << 16), once per block.  A voxel's sum is a serial
  // chain (ascending point index: the order the result is defined in), but the chains of different channels and voxels
  // are independent: the rounds below deal (voxel, channel) pairs to the threads, so that a crowded voxel (70 points in
  // one 12^3 voxel of an unnormalised cloud) costs 70 steps on a handful of threads, not 70 x channels on one.
  unsigned int *s_lead = s_key + np2;            // [n]
  int *s_count = reinterpret_cast<int *>(s_lead + np2);
  float *grid = reinterpret_cast<float *>(s_count + 4);
  if (tid == 0) *s_count = 0;
  __syncthreads();
  vox_for_each_voxel(s_key, n, log_np2, [&](int p, unsigned int, int len) {
    s_lead[atomicAdd(s_count, 1)] = (unsigned int)p | ((unsigned int)len << 16);
  });
  __syncthreads();
  const int n_lead = *s_count;
  // the count grid: one round of its own, by the cloud's first block
  if (blockIdx.x == 0) {
    for (int i = tid; i < r3 / 4; i += kVoxBlock) reinterpret_cast<float4 *>(grid)[i] = z4;
    __syncthreads();
    for (int i = tid; i < n_lead; i += kVoxBlock) {
      const unsigned int e = s_lead[i];
      reinterpret_cast<int *>(grid)[s_key[e & 0xFFFFu] >> log_np2] = (int)(e >> 16);
    }
    __syncthreads();
    for (int i = tid; i < r3 / 4; i += kVoxBlock)
      reinterpret_cast<float4 *>(cnt)[i] = reinterpret_cast<const float4 *>(grid)[i];
    __syncthreads();
  }
  // feature rows of the round: staged in LDS behind the grid when they fit (coalesced loads once, instead of global
  // round trips inside the chains).  stage_feat == 2: fetched as 16-byte loads into registers a round AHEAD (requested
  // before the previous round's chains, stored after them): with one block per CU nothing else hides those round trips
  float *sf = grid + (size_t)g_rows * r3;
  // four named registers (an indexed float4[4] behind the lambda and the data-dependent round loop was kept in scratch:
  // 96 B per lane of private memory in a latency-bound kernel)
  float4 pre0 = z4, pre1 = z4, pre2 = z4, pre3 = z4;
  auto fetch = [&](int l0, int rows) {
    const float4 *src = reinterpret_cast<const float4 *>(feat + (size_t)l0 * n);
    const int cnt4 = (rows * n) >> 2;
    // unconditional loads on clamped addresses; lanes beyond the rows keep a value nobody stores
    const int last = cnt4 > 0 ? cnt4 - 1 : 0;
    pre0 = src[min(tid, last)];
    pre1 = src[min(tid + kVoxBlock, last)];
    pre2 = src[min(tid + 2 * kVoxBlock, last)];
    pre3 = src[min(tid + 3 * kVoxBlock, last)];
  };
  if (stage_feat == 2) fetch(c0, min(g_rows, c1 - c0));
  for (int l0 = c0; l0 < c1; l0 += g_rows) {
    const int rows = min(g_rows, c1 - l0);
    for (int i = tid; i < rows * (r3 / 4); i += kVoxBlock) reinterpret_cast<float4 *>(grid)[i] = z4;
    if (stage_feat == 2) {
      const int cnt4 = (rows * n) >> 2;
      float4 *sf4 = reinterpret_cast<float4 *>(sf);
      if (tid < cnt4) sf4[tid] = pre0;
      if (tid + kVoxBlock < cnt4) sf4[tid + kVoxBlock] = pre1;
      if (tid + 2 * kVoxBlock < cnt4) sf4[tid + 2 * kVoxBlock] = pre2;
      if (tid + 3 * kVoxBlock < cnt4) sf4[tid + 3 * kVoxBlock] = pre3;
    } else if (stage_feat) {
      for (int i = tid; i < rows * n; i += kVoxBlock) sf[i] = feat[(size_t)l0 * n + i];
    }
    __syncthreads();
    if (stage_feat == 2 && l0 + g_rows < c1) fetch(l0 + g_rows, min(g_rows, c1 - l0 - g_rows));
    // (voxel, channel) pairs, voxel-minor: neighbouring lanes read different points of one row
    for (int w = tid; w < n_lead * rows; w += kVoxBlock) {
      const int l = w / n_lead, id = w - l * n_lead;
      const unsigned int e = s_lead[id];
      const int p = (int)(e & 0xFFFFu), len = (int)(e >> 16);
      const float div = (float)(1.0 / (double)(float)len);
      const float *f = stage_feat ? sf + (size_t)l * n : feat + (size_t)(l0 + l) * n;
      float acc = 0.f;
      for (int q = 0; q < len; ++q) acc += f[s_key[p + q] & imask] * div;
      grid[(size_t)l * r3 + (s_key[p] >> log_np2)] = acc;
    }
    __syncthreads();
    float4 *o4 = reinterpret_cast<float4 *>(out + (size_t)l0 * r3);
    for (int i = tid; i < rows * (r3 / 4); i += kVoxBlock) o4[i] = reinterpret_cast<const float4 *>(grid)[i];
    __syncthreads();
  }
}

// ------------------------------------------------------ devoxelize ---------
constexpr int kDevBlock = 256;
constexpr int kDevChannelsPerBlock = 16;

__global__ __launch_bounds__(kDevBlock) void trilinear_devoxelize_kernel(const float *__restrict__ coords,
                                                                         const float *__restrict__ feat, int c,
                                                                         int n, int r, int is_training,
                                                                         float *__restrict__ outs,
                                                                         int32_t *__restrict__ inds,
                                                                         float *__restrict__ wgts) {
  const int b = blockIdx.z;
  const int r3 = r * r * r;
  coords += (size_t)b * 3 * n;
  feat += (size_t)b * c * r3;
  outs += (size_t)b * c * n;
  const int i = blockIdx.x * kDevBlock + threadIdx.x;
  if (i >= n) return;
  float w[8];
  int id[8];
  trilinear_corners(coords[i], coords[i + n], coords[i + 2 * n], r, w, id);
  if (is_training && blockIdx.y == 0) {
    float *wo = wgts + (size_t)b * 8 * n;
    int32_t *io = inds + (size_t)b * 8 * n;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      wo[i + k * n] = w[k];
      io[i + k * n] = id[k];
    }
  }
  const int c0 = blockIdx.y * kDevChannelsPerBlock, c1 = min(c0 + kDevChannelsPerBlock, c);
  for (int l = c0; l < c1; ++l) {
    const float *f = feat + (size_t)l * r3;
    outs[(size_t)l * n + i] = w[0] * f[id[0]] + w[1] * f[id[1]] + w[2] * f[id[2]] + w[3] * f[id[3]] +
                              w[4] * f[id[4]] + w[5] * f[id[5]] + w[6] * f[id[6]] + w[7] * f[id[7]];
  }
}

int ilog2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

}  // namespace

// =========================================================== C ABI =========

GLDM_API int gldm_voxel_coords(const float *coords, int b, int n, int r, int normalize, float eps,
                               float *norm_coords, int32_t *vox_coords, gldm_stream_t stream) {
  if (!coords || !norm_coords || !vox_coords || b <= 0 || n <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(voxel_coords_kernel, dim3(b), dim3(kVcBlock), 0, as_stream(stream), coords, n, r, normalize,
                     eps, norm_coords, vox_coords);
  return launch_status();
}

GLDM_API int gldm_avg_voxelize_forward(const float *features, const int32_t *vox_coords, int b, int c, int n,
                                       int r, float *out, int32_t *ind, int32_t *cnt, gldm_stream_t stream) {
  if (!features || !vox_coords || !out || !ind || !cnt || b <= 0 || c <= 0 || n <= 0 || r <= 0)
    return GLDM_ERR_INVALID_ARG;
  const int log_np2 = ilog2_ceil(n);
  const int np2 = 1 << log_np2;
  if (n > 8192 || r > 64 || (long long)r * r * r * np2 > (1ll << 32)) return GLDM_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  const size_t r3 = (size_t)r * r * r;
  // grids whose rows fit LDS beside the keys: assembled on chip and written dense (no memsets, no scattered stores)
  {
    const size_t key_bytes = (size_t)2 * np2 * sizeof(unsigned int) + 16, row_bytes = r3 * sizeof(float);
    const size_t room = (size_t)150 * 1024 - key_bytes;
    if (r3 % 4 == 0 && row_bytes <= room) {
      // rows per round: grid row + (when it fits) the row's features, both in LDS
      const size_t both = row_bytes + (size_t)n * sizeof(float);
      int stage_feat = both <= room ? 1 : 0;
      int g_rows = (int)(room / (stage_feat ? both : row_bytes));
      if (g_rows > 16) g_rows = 16;
      if (g_rows > c) g_rows = c;
      if (stage_feat && n % 4 == 0 && (size_t)g_rows * n <= (size_t)4 * 4 * kVoxBlock) stage_feat = 2;   // register prefetch form
      // A block sorts its cloud's keys once and then walks `chunk` channels in rounds of g_rows: a cloud is split over
      // several blocks only while the launch would otherwise leave compute units idle
      auto lds_of = [&](int rows) { return key_bytes + (size_t)rows * (stage_feat ? both : row_bytes); };
      const int rounds = ceil_div(c, g_rows);
      int parts = gldm_dev::cu_count() / b;   // (measured: more, smaller blocks per cloud re-sort more than they overlap)
      parts = parts < 1 ? 1 : (parts > rounds ? rounds : parts);
      const int chunk = ceil_div(rounds, parts) * g_rows;
      const size_t lds_bytes = lds_of(g_rows);
      struct VoxDenseTag { int site; };
      gldm_dev::allow_dynamic_lds<VoxDenseTag>(reinterpret_cast<const void *>(&avg_voxelize_dense_kernel), 160 * 1024);
      hipLaunchKernelGGL(avg_voxelize_dense_kernel, dim3(ceil_div(c, chunk), b), dim3(kVoxBlock), lds_bytes, s, features,
                         vox_coords, c, n, np2, log_np2, r, chunk, g_rows, stage_feat, out, ind, cnt);
      return launch_status();
    }
  }
  if (hipMemsetAsync(out, 0, (size_t)b * c * r3 * sizeof(float), s) != hipSuccess) return GLDM_ERR_LAUNCH;
  if (hipMemsetAsync(cnt, 0, (size_t)b * r3 * sizeof(int32_t), s) != hipSuccess) return GLDM_ERR_LAUNCH;
  dim3 grid(ceil_div(c, kVoxChannelsPerBlock), b);
  hipLaunchKernelGGL(avg_voxelize_kernel<1>, grid, dim3(kVoxBlock), (size_t)np2 * sizeof(unsigned int), s,
                     features, vox_coords, c, n, np2, log_np2, r, out, ind, cnt);
  return launch_status();
}

GLDM_API int gldm_trilinear_devoxelize_forward(const float *coords, const float *features, int b, int c, int n,
                                               int r, int is_training, float *out, int32_t *inds, float *wgts,
                                               gldm_stream_t stream) {
  if (!coords || !features || !out || b <= 0 || c <= 0 || n <= 0 || r <= 0) return GLDM_ERR_INVALID_ARG;
  if (is_training && (!inds || !wgts)) return GLDM_ERR_INVALID_ARG;
  dim3 grid(ceil_div(n, kDevBlock), ceil_div(c, kDevChannelsPerBlock), b);
  hipLaunchKernelGGL(trilinear_devoxelize_kernel, grid, dim3(kDevBlock), 0, as_stream(stream), coords, features,
                     c, n, r, is_training, out, inds, wgts);
  return launch_status();
}
