// depth_cloud.hip -- depth frames to ordered point clouds on gfx950 (gldm_depth_to_cloud, include/gldm.h).
//
// ref: grasp_ldm/utils/camera.py:176-215 (Camera.depth_to_pointcloud_torch): the pinhole deprojection in front of
// regularize_pc_point_count and normalize_input.  Compiled with -ffp-contract=off (csrc/Makefile, SRCS_STRICT): the keep
// predicates and every product, quotient and sum round once per written operation, which is what the reference's torch
// expression computes on f32 tensors with its f64 intrinsics cast to f32.
//
// Layout: a frame's H*W pixels are cut into tiles of kTile = kBlock * kPerThread consecutive pixels, one workgroup per
// (tile, frame).  Thread t of a tile looks at pixels base + q * kBlock + t, q = 0 .. kPerThread - 1 (coalesced loads), so
// ascending pixel order is (q, wave, lane) order.
//
// Ordered compaction without any workgroup waiting for another: two launches.
//   pass 1  every tile counts its kept pixels -> tile_count[f][tile]                      (caller workspace)
//   pass 2  every tile sums the counts of the tiles in front of it in its frame (at most 8191 ints, one strided read +
//           one workgroup reduction), predicates again, and writes its points at that offset; inside the tile the slot
//           of a pixel is the exclusive prefix over the (q, wave) ballot counts plus the popcount of the lower lanes.
//           The last tile of a frame writes count[f].
// Both passes call the same inlined `deproject` on the same loaded values, so they cannot disagree about a pixel.
//
// gldm_depth_to_objects (further down): the same tiles and the same `deproject` with an instance-label image, one ordered
// compaction per label in three launches.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "depth_deproject.h"   // DepthParams, load_depth, deproject, make_params: shared with tabletop.hip
#include "host_util.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kPerThread = 8;
constexpr int kTile = kBlock * kPerThread;   // 2048 pixels
constexpr int kMaxPixels = 1 << 24;
constexpr int kMaxFrames = 65535;            // grid.y

// Sum of v over the workgroup, in every thread (s_red: kWaves ints).
__device__ __forceinline__ int block_sum(int v, int *s_red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += s_red[w];
  return t;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void depth_count_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                             DepthParams P, int tiles, int32_t *__restrict__ tile_count) {
  __shared__ int s_red[kWaves];
  const int tile = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const size_t fbase = (size_t)f * P.hw;
  int kept = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int pix = tile * kTile + q * kBlock + tid;
    if (pix < P.hw) {
      const float d = load_depth(depth, fbase + pix, P.depth_scale);
      const unsigned m = mask ? mask[fbase + pix] : 1u;
      float x, y, z;
      kept += deproject(P, pix, d, m, x, y, z) ? 1 : 0;
    }
  }
  const int total = block_sum(kept, s_red);
  if (tid == 0) tile_count[(size_t)f * tiles + tile] = total;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void depth_write_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                             DepthParams P, int tiles, const int32_t *__restrict__ tile_count,
                                                             float *__restrict__ points, int32_t *__restrict__ count,
                                                             int32_t *__restrict__ pixel) {
  __shared__ int s_red[kWaves];
  __shared__ int s_cnt[kPerThread * kWaves + 1];
  const int tile = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const size_t fbase = (size_t)f * P.hw;
  // offset of this tile: the counts of the tiles in front of it in this frame
  int front = 0;
  for (int t = tid; t < tile; t += kBlock) front += tile_count[(size_t)f * tiles + t];
  const int offset = block_sum(front, s_red);
  float x[kPerThread], y[kPerThread], z[kPerThread];
  unsigned keepbits = 0u;
  int below[kPerThread];
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int pix = tile * kTile + q * kBlock + tid;
    bool k = false;
    x[q] = y[q] = z[q] = 0.f;
    if (pix < P.hw) {
      const float d = load_depth(depth, fbase + pix, P.depth_scale);
      const unsigned m = mask ? mask[fbase + pix] : 1u;
      k = deproject(P, pix, d, m, x[q], y[q], z[q]);
    }
    const unsigned long long bal = __ballot(k);
    below[q] = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[q * kWaves + wave] = __popcll(bal);
    keepbits |= k ? (1u << q) : 0u;
  }
  __syncthreads();
  if (tid == 0) {   // exclusive prefix over the 32 (q, wave) counts, in place; the total behind them
    int run = 0;
    for (int i = 0; i < kPerThread * kWaves; ++i) {
      const int c = s_cnt[i];
      s_cnt[i] = run;
      run += c;
    }
    s_cnt[kPerThread * kWaves] = run;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    if (keepbits & (1u << q)) {
      const size_t row = fbase + (size_t)(offset + s_cnt[q * kWaves + wave] + below[q]);   // < fbase + hw: at most hw pixels are kept
      points[3 * row] = x[q];
      points[3 * row + 1] = y[q];
      points[3 * row + 2] = z[q];
      if (pixel) pixel[row] = tile * kTile + q * kBlock + tid;
    }
  }
  if (tile == tiles - 1 && tid == 0) count[f] = offset + s_cnt[kPerThread * kWaves];
}

template <typename T>
int run(const T *depth, const uint8_t *mask, const DepthParams &P, int frames, int tiles, int32_t *ws, float *points,
        int32_t *count, int32_t *pixel, hipStream_t s) {
  hipLaunchKernelGGL((depth_count_kernel<T>), dim3(tiles, frames), dim3(kBlock), 0, s, depth, mask, P, tiles, ws);
  int st = launch_status();
  if (st != GLDM_OK) return st;
  hipLaunchKernelGGL((depth_write_kernel<T>), dim3(tiles, frames), dim3(kBlock), 0, s, depth, mask, P, tiles, ws, points,
                     count, pixel);
  return launch_status();
}

// 0, or the status of a shape outside the envelope
int check_shape(int frames, int h, int w) {
  if (frames < 1 || h < 1 || w < 1) return GLDM_ERR_INVALID_ARG;
  if ((long long)h * w > kMaxPixels || frames > kMaxFrames) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

// ------------------------------------------------------------------------------------------------ labelled frames --
// gldm_depth_to_objects: the same tiles, one compaction per label 1 .. K in one pass over the frame.  Three launches,
// no workgroup waits for another:
//   count  every tile counts its kept pixels per label         -> ws[f][k][tile]
//   scan   one workgroup per (label, frame): exclusive prefix over the tiles, in place; the total is count[f][k]
//   write  every tile turns count[f][0..K) into start[f][k] (K <= 64 values: one wave scan), adds its own ws[f][k][tile],
//          predicates again and writes; tile 0 writes start[f][..]
// Slot of a pixel among the pixels of its label inside a tile: its rank in its wave (a loop over the distinct labels that
// the wave holds) plus the exclusive prefix of that label over the 32 (q, wave) groups in front of it, kept in LDS
// (s_cnt[group][label], 8 KiB).  Count and write run the same `label_ranks` on the same loaded values.
constexpr int kMaxLabels = 64;
constexpr int kGroups = kPerThread * kWaves;   // 32 (q, wave) groups of 64 consecutive pixels

// Rank of this lane among the lanes of the wave that carry the same label (lab 0: none), and how many they are.  Every
// lane of the wave must call it.
__device__ __forceinline__ int wave_label_rank(int lab, int lane, int &same_count) {
  unsigned long long todo = __ballot(lab != 0);
  int rank = 0;
  same_count = 0;
  while (todo) {   // uniform: todo is a ballot
    const int l = __shfl(lab, __ffsll((long long)todo) - 1, kWave);   // the first live lane's label
    const unsigned long long same = __ballot(lab == l);
    if (lab == l) {
      rank = __popcll(same & ((1ull << lane) - 1ull));
      same_count = __popcll(same);
    }
    todo &= ~same;
  }
  return rank;
}

// The tile's pixels of this thread: label (0 = dropped or background) and rank inside the wave per q, the points when
// kPoints, and the per-(group, label) counts in s_cnt (synchronised on return).
template <typename T, bool kPoints>
__device__ __forceinline__ void label_ranks(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                            const int32_t *__restrict__ labels, const DepthParams &P, int num_labels,
                                            int tile, size_t fbase, int (*s_cnt)[kMaxLabels], int *lab, int *rank, float *x,
                                            float *y, float *z) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kGroups * kMaxLabels; i += kBlock) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int pix = tile * kTile + q * kBlock + tid;
    int l = 0;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (pix < P.hw) {
      const float d = load_depth(depth, fbase + pix, P.depth_scale);
      const unsigned m = mask ? mask[fbase + pix] : 1u;
      const int32_t raw = labels[fbase + pix];
      const bool k = deproject(P, pix, d, m, px, py, pz);
      l = (k && raw >= 1 && raw <= num_labels) ? raw : 0;
    }
    int same;
    rank[q] = wave_label_rank(l, lane, same);
    lab[q] = l;
    if (kPoints) {
      x[q] = px; y[q] = py; z[q] = pz;
    }
    if (l != 0 && rank[q] == 0) s_cnt[q * kWaves + wave][l - 1] = same;   // 1 <= l <= num_labels <= kMaxLabels
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kBlock) void objects_count_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                               const int32_t *__restrict__ labels, DepthParams P,
                                                               int num_labels, int tiles, int32_t *__restrict__ ws) {
  __shared__ int s_cnt[kGroups][kMaxLabels];
  const int tile = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  int lab[kPerThread], rank[kPerThread];
  label_ranks<T, false>(depth, mask, labels, P, num_labels, tile, (size_t)f * P.hw, s_cnt, lab, rank, nullptr, nullptr,
                        nullptr);
  if (tid < num_labels) {
    int total = 0;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) total += s_cnt[g][tid];
    ws[((size_t)f * num_labels + tid) * tiles + tile] = total;
  }
}

// grid (num_labels, frames): ws[f][k][0 .. tiles) from counts to their exclusive prefix; count[f][k] = the total.
__global__ __launch_bounds__(kBlock) void objects_scan_kernel(int32_t *__restrict__ ws, int tiles, int32_t *__restrict__ count) {
  __shared__ int s_w[kWaves];
  const int k = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int32_t *row = ws + ((size_t)f * gridDim.x + k) * tiles;
  int run = 0;
  for (int t0 = 0; t0 < tiles; t0 += kBlock) {
    const int t = t0 + tid;
    const int c = t < tiles ? row[t] : 0;
    int inc = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(inc, off, kWave);
      if (lane >= off) inc += o;
    }
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int v = s_w[w];
      before += w < wave ? v : 0;
      total += v;
    }
    if (t < tiles) row[t] = run + before + inc - c;
    run += total;
    __syncthreads();
  }
  if (tid == 0) count[(size_t)f * gridDim.x + k] = run;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void objects_write_kernel(const T *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                               const int32_t *__restrict__ labels, DepthParams P,
                                                               int num_labels, int tiles, const int32_t *__restrict__ ws,
                                                               const int32_t *__restrict__ count, float *__restrict__ points,
                                                               int32_t *__restrict__ start, int32_t *__restrict__ pixel) {
  __shared__ int s_cnt[kGroups][kMaxLabels];
  __shared__ int s_base[kMaxLabels];
  const int tile = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
  const size_t fbase = (size_t)f * P.hw;
  if (tid < kWave) {   // wave 0: start[f][k] = the counts of the labels in front of k; base = start + this tile's offset
    const int c = tid < num_labels ? count[(size_t)f * num_labels + tid] : 0;
    int inc = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(inc, off, kWave);
      if (tid >= off) inc += o;
    }
    if (tid < num_labels) {
      const int st = inc - c;
      s_base[tid] = st + ws[((size_t)f * num_labels + tid) * tiles + tile];
      if (tile == 0) start[(size_t)f * num_labels + tid] = st;
    }
  }
  int lab[kPerThread], rank[kPerThread];
  float x[kPerThread], y[kPerThread], z[kPerThread];
  label_ranks<T, true>(depth, mask, labels, P, num_labels, tile, fbase, s_cnt, lab, rank, x, y, z);   // (orders s_base too)
  if (tid < num_labels) {   // exclusive prefix over the 32 groups of label tid, in place
    int run = 0;
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
      const int c = s_cnt[g][tid];
      s_cnt[g][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    if (lab[q] != 0) {
      // < fbase + hw: the frame keeps at most hw pixels over all labels
      const size_t row = fbase + (size_t)(s_base[lab[q] - 1] + s_cnt[q * kWaves + wave][lab[q] - 1] + rank[q]);
      points[3 * row] = x[q];
      points[3 * row + 1] = y[q];
      points[3 * row + 2] = z[q];
      if (pixel) pixel[row] = tile * kTile + q * kBlock + tid;
    }
  }
}

template <typename T>
int run_objects(const T *depth, const uint8_t *mask, const int32_t *labels, const DepthParams &P, int num_labels, int frames,
                int tiles, int32_t *ws, float *points, int32_t *start, int32_t *count, int32_t *pixel, hipStream_t s) {
  hipLaunchKernelGGL((objects_count_kernel<T>), dim3(tiles, frames), dim3(kBlock), 0, s, depth, mask, labels, P, num_labels,
                     tiles, ws);
  int st = launch_status();
  if (st != GLDM_OK) return st;
  hipLaunchKernelGGL(objects_scan_kernel, dim3(num_labels, frames), dim3(kBlock), 0, s, ws, tiles, count);
  st = launch_status();
  if (st != GLDM_OK) return st;
  hipLaunchKernelGGL((objects_write_kernel<T>), dim3(tiles, frames), dim3(kBlock), 0, s, depth, mask, labels, P, num_labels,
                     tiles, ws, count, points, start, pixel);
  return launch_status();
}

int check_objects_shape(int frames, int h, int w, int num_labels) {
  const int st = check_shape(frames, h, w);
  if (st != GLDM_OK) return st;
  if (num_labels < 1) return GLDM_ERR_INVALID_ARG;
  if (num_labels > kMaxLabels) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

}  // namespace

GLDM_API int gldm_depth_to_cloud_tile_pixels(void) { return kTile; }

GLDM_API long long gldm_depth_to_cloud_workspace_bytes(int frames, int h, int w) {
  const int st = check_shape(frames, h, w);
  if (st != GLDM_OK) return st;
  const long long tiles = ((long long)h * w + kTile - 1) / kTile;
  return (long long)frames * tiles * (long long)sizeof(int32_t);
}

GLDM_API int gldm_depth_to_cloud(const void *depth, int depth_is_u16, float depth_scale, const uint8_t *mask, int frames,
                                 int h, int w, float fx, float fy, float cx, float cy, float z_min, float z_max,
                                 const float *cam_to_world, const float *box_lo, const float *box_hi, void *workspace,
                                 long long workspace_bytes, float *points, int32_t *count, int32_t *pixel,
                                 gldm_stream_t stream) {
  // the envelope first: nothing below touches a pointer or the device before it holds
  const int st = check_shape(frames, h, w);
  if (st != GLDM_OK) return st;
  if (!(fx != 0.f) || !(fy != 0.f) || !(z_min < z_max) || fx != fx || fy != fy || cx != cx || cy != cy)
    return GLDM_ERR_INVALID_ARG;
  if (!depth || !workspace || !points || !count || (box_lo == nullptr) != (box_hi == nullptr)) return GLDM_ERR_INVALID_ARG;
  if (depth_is_u16 != 0 && depth_is_u16 != 1) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_depth_to_cloud_workspace_bytes(frames, h, w)) return GLDM_ERR_WORKSPACE;
  const DepthParams P = make_params(depth_is_u16, depth_scale, h, w, fx, fy, cx, cy, z_min, z_max, cam_to_world, box_lo, box_hi);
  const int tiles = (P.hw + kTile - 1) / kTile;
  int32_t *ws = static_cast<int32_t *>(workspace);
  hipStream_t s = as_stream(stream);
  if (depth_is_u16)
    return run(static_cast<const uint16_t *>(depth), mask, P, frames, tiles, ws, points, count, pixel, s);
  return run(static_cast<const float *>(depth), mask, P, frames, tiles, ws, points, count, pixel, s);
}

GLDM_API long long gldm_depth_to_objects_workspace_bytes(int frames, int h, int w, int num_labels) {
  const int st = check_objects_shape(frames, h, w, num_labels);
  if (st != GLDM_OK) return st;
  const long long tiles = ((long long)h * w + kTile - 1) / kTile;
  return (long long)frames * num_labels * tiles * (long long)sizeof(int32_t);
}

GLDM_API int gldm_depth_to_objects(const void *depth, int depth_is_u16, float depth_scale, const uint8_t *mask,
                                   const int32_t *labels, int num_labels, int frames, int h, int w, float fx, float fy,
                                   float cx, float cy, float z_min, float z_max, const float *cam_to_world,
                                   const float *box_lo, const float *box_hi, void *workspace, long long workspace_bytes,
                                   float *points, int32_t *start, int32_t *count, int32_t *pixel, gldm_stream_t stream) {
  // the envelope first: nothing below touches a pointer or the device before it holds
  const int st = check_objects_shape(frames, h, w, num_labels);
  if (st != GLDM_OK) return st;
  if (!(fx != 0.f) || !(fy != 0.f) || !(z_min < z_max) || fx != fx || fy != fy || cx != cx || cy != cy)
    return GLDM_ERR_INVALID_ARG;
  if (!depth || !labels || !workspace || !points || !start || !count || (box_lo == nullptr) != (box_hi == nullptr))
    return GLDM_ERR_INVALID_ARG;
  if (depth_is_u16 != 0 && depth_is_u16 != 1) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_depth_to_objects_workspace_bytes(frames, h, w, num_labels)) return GLDM_ERR_WORKSPACE;
  const DepthParams P = make_params(depth_is_u16, depth_scale, h, w, fx, fy, cx, cy, z_min, z_max, cam_to_world, box_lo, box_hi);
  const int tiles = (P.hw + kTile - 1) / kTile;
  int32_t *ws = static_cast<int32_t *>(workspace);
  hipStream_t s = as_stream(stream);
  if (depth_is_u16)
    return run_objects(static_cast<const uint16_t *>(depth), mask, labels, P, num_labels, frames, tiles, ws, points, start,
                       count, pixel, s);
  return run_objects(static_cast<const float *>(depth), mask, labels, P, num_labels, frames, tiles, ws, points, start, count,
                     pixel, s);
}
