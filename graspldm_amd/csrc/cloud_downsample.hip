// cloud_downsample.hip -- voxel-grid downsampling of ragged sensor clouds (include/gldm.h, "voxel-grid downsampling";
// DESIGN.md 4.15):
//
//   gldm_voxel_downsample  one output row per occupied voxel of every cloud: the centroid of its points, their number and
//                          the lowest source row among them; the voxels of a cloud in order of first appearance.
//
// A hash build (one table region per cloud, linear probing, vector atomics) followed by the ordered compaction of
// ragged_compact.h.  Every quantity an output depends on is a count, a minimum or an exact integer sum, so the race between
// lanes for slots and the order of the atomics change no bit.  Compiled with -ffp-contract=off (csrc/Makefile:
// SRCS_STRICT): every f64 operation below rounds once, as tests/cloud_downsample_ref.py restates it.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ragged_compact.h"
#include "voxel_hash.h"

namespace {

constexpr int kMaxVoxelN = 1 << 22;      // points of one cloud
constexpr int kMaxVoxelRows = 1 << 24;   // rows of one call: slot indices (2 per row) stay below 2^25
constexpr double kQLimit = 68719476736.0;           // 2^36 = 2^20 * 2^16
constexpr double kQScale = 65536.0;

// 48 bytes, 8-byte aligned.  key: voxel_hash.h's cell_key, all-ones = empty.
struct Slot {
  unsigned long long key;
  unsigned long long sum[3];   // int64 sums of q, two's complement
  int32_t members;
  int32_t first;               // lowest source row, relative to the cloud's start
  int32_t out;                 // the voxel's output row, relative to the cloud's out_start (write pass)
  int32_t pad;
};
static_assert(sizeof(Slot) == 48, "workspace layout");

// Per axis, in f64: t = p / v; cell = floor(t) clamped to [-2^20, 2^20 - 1]; q = rint(t * 2^16) clamped to [-2^36, 2^36].
// fmax / fmin return the other operand for a NaN, so whatever the data holds both conversions are defined.
__device__ __forceinline__ void quantise(float p, double v, long long &cell, long long &q) {
  const double t = (double)p / v;
  cell = (long long)fmin(fmax(floor(t), -kCellLimit), kCellLimit - 1.0);
  q = (long long)fmin(fmax(rint(t * kQScale), -kQLimit), kQLimit);
}

// Cloud i owns the slots 2 * start[i] .. 2 * (start[i] + count[i]); a workgroup clears those of its chunk's rows.
__global__ __launch_bounds__(kChunk) void table_init_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                            int n_max, int rows, int chunks_max, Slot *__restrict__ table) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int p0 = ch * kChunk;
  if (p0 >= rg.n) return;   // uniform over the workgroup
  const int cnt = min(kChunk, rg.n - p0);
  Slot *base = table + 2 * (rg.s + p0);
  for (int i = threadIdx.x; i < 2 * cnt; i += kChunk) {
    Slot e;
    e.key = kEmptyKey;
    e.sum[0] = e.sum[1] = e.sum[2] = 0ull;
    e.members = 0;
    e.first = INT_MAX;
    e.out = -1;
    e.pad = 0;
    base[i] = e;
  }
}

// One lane per point: find the slot of its voxel in the cloud's region (voxel_hash.h: linear probing from a hash of the key; a
// slot is taken when the compare-and-swap returns empty or the own key), add the point to it and remember the slot.  The region holds
// two slots per point, so an empty slot always exists and the loop ends within `len` probes; it is bounded by `len` all the
// same and a row that found none (impossible) carries slot -1, which every later pass skips.
__global__ __launch_bounds__(kChunk) void table_insert_kernel(const float *__restrict__ pts, const int32_t *__restrict__ start,
                                                              const int32_t *__restrict__ count, int n_max, int rows,
                                                              int chunks_max, double voxel, Slot *__restrict__ table,
                                                              int32_t *__restrict__ slot_of) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (qi >= rg.n) return;
  const long long row = rg.s + qi;
  long long cell[3], q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) quantise(pts[row * 3 + c], voxel, cell[c], q[c]);
  const unsigned long long key = cell_key(cell[0], cell[1], cell[2]);
  const long long base = 2 * rg.s;
  const long long at = hash_insert(table + base, 2u * (unsigned)rg.n, key);
  const long long slot = at < 0 ? -1 : base + at;
  slot_of[row] = (int32_t)slot;
  if (slot < 0) return;
  Slot *s = table + slot;
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(&s->sum[c], (unsigned long long)q[c]);
  atomicAdd(&s->members, 1);
  atomicMin(&s->first, qi);
}

// A row opens an output row iff it is the lowest row of its voxel.  WRITE 0: their number per chunk -> tile_cnt.  WRITE 1
// (after scan_kernel): the voxels, packed in ascending `first` behind out_start[cloud] + the chunk's offset.
template <int WRITE>
__global__ __launch_bounds__(kChunk) void voxel_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                       int n_max, int rows, int chunks_max, double voxel,
                                                       Slot *__restrict__ table, const int32_t *__restrict__ slot_of,
                                                       int32_t *__restrict__ tile_cnt, const int32_t *__restrict__ out_start,
                                                       float *__restrict__ out_points, int32_t *__restrict__ first,
                                                       int32_t *__restrict__ members) {
  __shared__ int redi[kChunk / 64];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int qi = ch * kChunk + (int)threadIdx.x;
  const int slot = qi < rg.n ? slot_of[rg.s + qi] : -1;
  const bool opens = slot >= 0 && table[slot].first == qi;
  int before;
  const int total = chunk_count(opens, redi, before);
  const long long tile = (long long)cloud * chunks_max + ch;
  if (WRITE == 0) {
    if (threadIdx.x == 0) tile_cnt[tile] = total;
  } else if (opens) {
    Slot *s = table + slot;
    const int rel = tile_cnt[tile] + before;
    const long long dst = (long long)out_start[cloud] + rel;
    const int m = s->members;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out_points[dst * 3 + c] = (float)(((double)(long long)s->sum[c] / (double)m) / kQScale * voxel);
    first[dst] = qi;
    members[dst] = m;
    s->out = rel;
  }
}

__global__ __launch_bounds__(kChunk) void voxel_map_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                           int n_max, int rows, int chunks_max, const Slot *__restrict__ table,
                                                           const int32_t *__restrict__ slot_of, int32_t *__restrict__ voxel_of) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (qi >= rg.n) return;
  const int slot = slot_of[rg.s + qi];
  voxel_of[rg.s + qi] = slot >= 0 ? table[slot].out : -1;
}

// No pointer is read and the device is not touched outside it.
int check_envelope(int b, int n_max, int rows) {
  if (b < 1 || n_max < 0 || rows < 0) return GLDM_ERR_INVALID_ARG;
  if (b > kMaxClouds || n_max > kMaxVoxelN || rows > kMaxVoxelRows) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

}  // namespace

// workspace: table Slot [2 rows], slot_of int32 [rows], tile_cnt int32 [tiles]
GLDM_API long long gldm_voxel_downsample_workspace_bytes(int b, int n_max, int rows) {
  const int st = check_envelope(b, n_max, rows);
  if (st != GLDM_OK) return st;
  const long long tiles = (long long)b * ceil_div(n_max, kChunk);
  return 2ll * rows * (long long)sizeof(Slot) + align8((long long)rows * (long long)sizeof(int32_t)) +
         align8(tiles * (long long)sizeof(int32_t));
}

GLDM_API int gldm_voxel_downsample(const float *points, const int32_t *start, const int32_t *count, int b, int n_max, int rows,
                                   float voxel_size, void *workspace, long long workspace_bytes, float *out_points,
                                   int32_t *out_start, int32_t *out_count, int32_t *first, int32_t *members, int32_t *voxel,
                                   gldm_stream_t stream) {
  if (b < 1 || n_max < 0 || rows < 0 || !(voxel_size > 0.f) || !isfinite(voxel_size)) return GLDM_ERR_INVALID_ARG;
  const int env = check_envelope(b, n_max, rows);
  if (env != GLDM_OK) return env;
  const bool empty = n_max == 0 || rows == 0;   // every cloud is empty: the counts are still written
  if (!start || !count || !out_start || !out_count) return GLDM_ERR_INVALID_ARG;
  if (!empty && (!points || !out_points || !first || !members || !workspace)) return GLDM_ERR_INVALID_ARG;
  if (!empty && workspace_bytes < gldm_voxel_downsample_workspace_bytes(b, n_max, rows)) return GLDM_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  if (empty) {   // the scan sees empty clouds and reads no tile
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, start, count, b, 0, rows, 0, (int32_t *)nullptr, out_start,
                       out_count);
    return launch_status();
  }
  const int chunks_max = ceil_div(n_max, kChunk);
  const unsigned blocks = (unsigned)((long long)b * chunks_max);   // <= 65535 * 16384
  Slot *table = static_cast<Slot *>(workspace);
  int32_t *slot_of = reinterpret_cast<int32_t *>(table + 2ll * rows);
  int32_t *tile_cnt = slot_of + align8((long long)rows * (long long)sizeof(int32_t)) / (long long)sizeof(int32_t);
  const double v = (double)voxel_size;
  hipLaunchKernelGGL(table_init_kernel, dim3(blocks), dim3(kChunk), 0, st, start, count, n_max, rows, chunks_max, table);
  hipLaunchKernelGGL(table_insert_kernel, dim3(blocks), dim3(kChunk), 0, st, points, start, count, n_max, rows, chunks_max, v,
                     table, slot_of);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(voxel_kernel<0>, dim3(blocks), dim3(kChunk), 0, st, start, count, n_max, rows, chunks_max, v, table,
                     slot_of, tile_cnt, out_start, out_points, first, members);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, start, count, b, n_max, rows, chunks_max, tile_cnt, out_start,
                     out_count);
  hipLaunchKernelGGL(voxel_kernel<1>, dim3(blocks), dim3(kChunk), 0, st, start, count, n_max, rows, chunks_max, v, table,
                     slot_of, tile_cnt, out_start, out_points, first, members);
  if (voxel)
    hipLaunchKernelGGL(voxel_map_kernel, dim3(blocks), dim3(kChunk), 0, st, start, count, n_max, rows, chunks_max, table, slot_of,
                       voxel);
  return launch_status();
}
