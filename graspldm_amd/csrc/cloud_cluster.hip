// cloud_cluster.hip -- Euclidean clustering of unorganised, ragged clouds and the ordered split of a labelled cloud into its
// objects (include/gldm.h, "Euclidean clustering"):
//
//   gldm_cluster_cloud  connected components of the graph "two active rows of a cloud closer than link_dist": PCL's
//                       EuclideanClusterExtraction.  A per-cloud hash grid (voxel_hash.h) of cell size link_dist * (1 + 2^-10)
//                       makes the 27 neighbouring cells a complete search (the argument stands in gldm.h); the components
//                       come from the lock-free union-find of components.h, whose result -- the lowest row of a component
//                       as its root -- does not depend on the execution order.  Eleven launches on one stream:
//                         init     clear the cloud regions of the table
//                         insert   active test, cell, compare-and-swap on the key, members += 1; parent[] = self / -1
//                         count    members per 256-row chunk of slots          } a counting sort of the rows by cell:
//                         scan     ragged_compact.h's scan over the chunks     } offset of every cell, then the rows
//                         offsets  exclusive offsets of the slots of a chunk   } (x, y, z, row) behind it, in whatever
//                         scatter  member records into cell order              } order the atomics give -- no output sees it
//                         union    the hot one: a lane per record IN CELL ORDER against the records of the 27 cells
//                         flatten  parent[] = root; size[root] += 1 (one atomic per distinct root of a wave)
//                         gather   roots of at least min_points rows -> keys (size, ~root), per cloud
//                         select   one workgroup per cloud: the max_labels largest keys, in order
//                         write    labels[row] = rank of its root among the selected, else 0
//   gldm_split_labels   rows with label 1 .. max_labels packed cloud-major, by label, by row: per-chunk per-label counts, two
//                       scans, a write pass that ranks by ballot + popcount.  No atomics.
//
// No workgroup waits for another; every loop is bounded by the data it walks (probe loops by the region length, find loops
// because parents only decrease, member loops by the cell's count).  Compiled with -ffp-contract=off (csrc/Makefile,
// SRCS_STRICT): the f64 quotient and floor, the height over the plane and the squared distance round once per written
// operation, as tests/cloud_cluster_ref.py restates them.
#include <math.h>
#include <stdint.h>

#include "components.h"
#include "ragged_compact.h"
#include "voxel_hash.h"

namespace {

constexpr int kMaxClusterN = 1 << 22;      // points of one cloud
constexpr int kMaxClusterRows = 1 << 24;   // rows of one call
constexpr int kMaxLabels = 64;
constexpr long long kMaxSplitCounters = 1ll << 24;   // b * chunks * max_labels of gldm_split_labels
constexpr float kMinLink = 0x1p-60f, kMaxLink = 0x1p60f;

// 24 bytes, 8-byte aligned.
struct CSlot {
  unsigned long long key;   // voxel_hash.h's cell_key, all-ones = empty
  int32_t members;          // rows of the cell
  int32_t offset;           // of the cell's first record in the cloud's part of `sorted`
  int32_t fill;             // records written so far (scatter)
  int32_t pad;
};
static_assert(sizeof(CSlot) == 24, "workspace layout");

struct __attribute__((aligned(16))) Member {
  float x, y, z;
  int32_t row;   // relative to the cloud's start
};
static_assert(sizeof(Member) == 16, "workspace layout");

struct ClusterParams {
  double cs;                 // cell size
  float link2;               // link_dist^2, formed once in f32 on the host
  float a, b, c, d, h_min, h_max;
  int use_plane;
};

// floor((double)p / cs); `ok` is cleared unless it lies strictly inside (-2^20, 2^20 - 1) (NaN and inf fail): the 26
// neighbours of an active row's cell are cells of the lattice too.
__device__ __forceinline__ long long cell_of(float p, double cs, bool &ok) {
  const double c = floor((double)p / cs);
  ok = ok && c > -kCellLimit && c < kCellLimit - 1.0;
  return ok ? (long long)c : 0ll;
}

__device__ __forceinline__ bool active_row(const ClusterParams &P, float x, float y, float z, long long cell[3]) {
  bool ok = true;
  cell[0] = cell_of(x, P.cs, ok);
  cell[1] = cell_of(y, P.cs, ok);
  cell[2] = cell_of(z, P.cs, ok);
  if (ok && P.use_plane) {
    const float hgt = ((P.a * x + P.b * y) + P.c * z) + P.d;
    ok = hgt > P.h_min && hgt <= P.h_max;
  }
  return ok;
}

// Inclusive scan over the workgroup: `before` = the sum over lower threads, the return value the sum over all.
__device__ __forceinline__ int chunk_scan(int v, int *red, int &before) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    inc += lane >= off ? t : 0;
  }
  __syncthreads();   // red is free again
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  before = inc - v;
  int total = 0;
#pragma unroll
  for (int w = 0; w < kChunk / 64; ++w) {
    before += w < wave ? red[w] : 0;
    total += red[w];
  }
  return total;
}

// Cloud i owns the slots 2 * start[i] .. 2 * (start[i] + count[i]); a workgroup clears those of its chunk's rows.
__global__ __launch_bounds__(kChunk) void cl_init_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                         int n_max, int rows, int chunks_max, CSlot *__restrict__ table,
                                                         int32_t *__restrict__ cand_count) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  if (ch == 0 && threadIdx.x == 0) cand_count[cloud] = 0;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int p0 = ch * kChunk;
  if (p0 >= rg.n) return;   // uniform over the workgroup
  const int cnt = min(kChunk, rg.n - p0);
  CSlot *base = table + 2 * (rg.s + p0);
  for (int i = threadIdx.x; i < 2 * cnt; i += kChunk) {
    CSlot e;
    e.key = kEmptyKey;
    e.members = 0;
    e.offset = 0;
    e.fill = 0;
    e.pad = 0;
    base[i] = e;
  }
}

// One lane per row.  An active row takes the slot of its cell and counts itself there; parent = itself.  Every other row
// (and one that found no slot: impossible at 2 slots per row) has slot -1 and parent -1 and is skipped from here on.
__global__ __launch_bounds__(kChunk) void cl_insert_kernel(const float *__restrict__ pts, const int32_t *__restrict__ start,
                                                           const int32_t *__restrict__ count, int n_max, int rows,
                                                           int chunks_max, ClusterParams P, CSlot *__restrict__ table,
                                                           int32_t *__restrict__ slot_of, int32_t *__restrict__ parent,
                                                           int32_t *__restrict__ size) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (qi >= rg.n) return;
  const long long row = rg.s + qi;
  long long cell[3];
  long long slot = -1;
  if (active_row(P, pts[row * 3], pts[row * 3 + 1], pts[row * 3 + 2], cell)) {
    const long long base = 2 * rg.s;
    const long long at = hash_insert(table + base, 2u * (unsigned)rg.n, cell_key(cell[0], cell[1], cell[2]));
    if (at >= 0) {
      slot = base + at;
      atomicAdd(&table[slot].members, 1);
    }
  }
  slot_of[row] = (int32_t)slot;
  parent[row] = slot >= 0 ? qi : -1;
  size[row] = 0;
}

// The slots of a chunk (2 per row; the chunks of a cloud tile its region).  WRITE 0: the sum of their members -> tile_cnt.
// WRITE 1 (after scan_kernel): offset of every slot = the chunk's offset + the members of the lower slots of the chunk.
template <int WRITE>
__global__ __launch_bounds__(kChunk) void cl_offsets_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                            int n_max, int rows, int chunks_max, CSlot *__restrict__ table,
                                                            int32_t *__restrict__ tile_cnt) {
  __shared__ int red[kChunk / 64];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int p0 = ch * kChunk;
  if (p0 >= rg.n) return;   // uniform over the workgroup
  const int cnt = min(kChunk, rg.n - p0);
  CSlot *base = table + 2 * (rg.s + p0);
  const int i0 = 2 * (int)threadIdx.x;
  const bool in = i0 < 2 * cnt;   // then i0 + 1 < 2 * cnt as well
  const int m0 = in ? base[i0].members : 0, m1 = in ? base[i0 + 1].members : 0;
  int before;
  const int total = chunk_scan(m0 + m1, red, before);
  const long long tile = (long long)cloud * chunks_max + ch;
  if (WRITE == 0) {
    if (threadIdx.x == 0) tile_cnt[tile] = total;
  } else if (in) {
    const int o = tile_cnt[tile] + before;
    base[i0].offset = o;
    base[i0 + 1].offset = o + m0;
  }
}

// Every active row writes its record behind its cell's offset; the place inside the cell is whatever the atomic hands out.
__global__ __launch_bounds__(kChunk) void cl_scatter_kernel(const float *__restrict__ pts, const int32_t *__restrict__ start,
                                                            const int32_t *__restrict__ count, int n_max, int rows,
                                                            int chunks_max, CSlot *__restrict__ table,
                                                            const int32_t *__restrict__ slot_of, Member *__restrict__ sorted) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (qi >= rg.n) return;
  const long long row = rg.s + qi;
  const int slot = slot_of[row];
  if (slot < 0) return;
  CSlot *s = table + slot;
  const int pos = s->offset + atomicAdd(&s->fill, 1);   // < the cloud's active rows <= rg.n
  if (pos < 0 || pos >= rg.n) return;   // only if the ranges overlap, against the contract: stay inside the cloud
  Member m;
  m.x = pts[row * 3];
  m.y = pts[row * 3 + 1];
  m.z = pts[row * 3 + 2];
  m.row = qi;
  sorted[rg.s + pos] = m;
}

// The hot launch.  A LANE PER RECORD, taken in cell order: the lanes of a wave then sit in the same or in adjacent cells, so
// their 27 probes hit the same few slots and their member loops have similar lengths.  (A wave per cell would leave most
// lanes idle on the clouds this is made for: after a voxel downsample a cell holds a handful of rows.)  Each unordered pair is
// tested once, by its higher row.  `cur` follows the row's root, so the walk up the tree is not repeated per neighbour.
__global__ __launch_bounds__(kChunk) void cl_union_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                          int n_max, int rows, int chunks_max, ClusterParams P,
                                                          const CSlot *__restrict__ table, const Member *__restrict__ sorted,
                                                          const int32_t *__restrict__ act_count, int32_t *__restrict__ parent) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int i = ch * kChunk + (int)threadIdx.x;
  if (i >= min(act_count[cloud], rg.n)) return;
  const Member *recs = sorted + rg.s;
  const CSlot *region = table + 2 * rg.s;
  const unsigned len = 2u * (unsigned)rg.n;
  int *par = parent + rg.s;
  const Member me = recs[i];
  if ((unsigned)me.row >= (unsigned)rg.n) return;   // as in the scatter: never with ranges that keep the contract
  bool ok = true;
  const long long cx = cell_of(me.x, P.cs, ok), cy = cell_of(me.y, P.cs, ok), cz = cell_of(me.z, P.cs, ok);
  int cur = me.row;
  for (int k = 0; k < 27; ++k) {
    const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;
    const long long at = hash_find(region, len, cell_key(cx + ox, cy + oy, cz + oz));
    if (at < 0) continue;
    const int off = region[at].offset, m = region[at].members;
    if (off < 0 || m < 0 || off + m > rg.n) continue;
    for (int j = 0; j < m; ++j) {
      const Member q = recs[off + j];
      if ((unsigned)q.row >= (unsigned)me.row) continue;
      const float dx = me.x - q.x, dy = me.y - q.y, dz = me.z - q.z;
      if (((dx * dx + dy * dy) + dz * dz) <= P.link2) {
        cur = uf_find(par, cur);
        const int r = uf_find(par, q.row);
        if (r != cur) uf_union(par, cur, r);
      }
    }
  }
}

// parent[p] = root(p) (a racing reader sees an ancestor either way), and one atomic per distinct root of a wave onto size[].
__global__ __launch_bounds__(kChunk) void cl_flatten_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                            int n_max, int rows, int chunks_max, int32_t *__restrict__ parent,
                                                            int32_t *__restrict__ size) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int qi = ch * kChunk + (int)threadIdx.x, lane = threadIdx.x & 63;
  int *par = parent + rg.s;
  int r = -1;
  if (qi < rg.n && __atomic_load_n(&par[qi], __ATOMIC_RELAXED) >= 0) {
    r = uf_find(par, qi);
    __atomic_store_n(&par[qi], r, __ATOMIC_RELAXED);
  }
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {   // uniform: todo is a ballot
    const int lead = __ffsll((long long)todo) - 1;
    const int rr = __shfl(r, lead, 64);
    const unsigned long long same = __ballot(r == rr);
    if (lane == lead) atomicAdd(&size[rg.s + rr], __popcll(same));
    todo &= ~same;
  }
}

// Roots of at least min_points rows -> the cloud's part of cand, in any order (the selection does not depend on it).
__global__ __launch_bounds__(kChunk) void cl_gather_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                           int n_max, int rows, int chunks_max,
                                                           const int32_t *__restrict__ parent, const int32_t *__restrict__ size,
                                                           int min_points, unsigned long long *__restrict__ cand,
                                                           int32_t *__restrict__ cand_count) {
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int qi = ch * kChunk + (int)threadIdx.x, lane = threadIdx.x & 63;
  int sz = 0;
  const bool is = qi < rg.n && parent[rg.s + qi] == qi && (sz = size[rg.s + qi]) >= min_points;
  const unsigned long long bal = __ballot(is);
  if (!bal) return;
  const int lead = __ffsll((long long)bal) - 1;
  int base = 0;
  if (lane == lead) base = atomicAdd(&cand_count[cloud], __popcll(bal));   // at most rg.n roots in all
  base = __shfl(base, lead, 64);
  if (is) cand[rg.s + base + __popcll(bal & ((1ull << lane) - 1ull))] = seg_key(sz, qi);
}

// One workgroup per cloud: components.h's select_largest over the cloud's candidates.
__global__ __launch_bounds__(kSelectBlock) void cl_select_kernel(const int32_t *__restrict__ start,
                                                                 const int32_t *__restrict__ count, int n_max, int rows,
                                                                 const unsigned long long *__restrict__ cand,
                                                                 const int32_t *__restrict__ cand_count, int max_labels,
                                                                 int32_t *__restrict__ num_labels,
                                                                 int32_t *__restrict__ label_points,
                                                                 int32_t *__restrict__ label_root) {
  __shared__ unsigned long long s_key[kSelectBlock];
  __shared__ unsigned long long s_best;
  const int cloud = blockIdx.x;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  const int m = min(cand_count[cloud], rg.n);   // 0 for an empty cloud, whose rg.s may point anywhere
  select_largest(cand + (m ? rg.s : 0), m, max_labels, num_labels + cloud, label_points + (long long)cloud * max_labels,
                 label_root + (long long)cloud * max_labels, s_key, &s_best);
}

__global__ __launch_bounds__(kChunk) void cl_write_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                          int n_max, int rows, int chunks_max, int max_labels,
                                                          const int32_t *__restrict__ parent,
                                                          const int32_t *__restrict__ num_labels,
                                                          const int32_t *__restrict__ label_root,
                                                          int32_t *__restrict__ labels) {
  __shared__ int s_root[kMaxLabels];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int k = num_labels[cloud];   // <= max_labels <= kMaxLabels
  if ((int)threadIdx.x < k) s_root[threadIdx.x] = label_root[(long long)cloud * max_labels + threadIdx.x];
  __syncthreads();
  const int qi = ch * kChunk + (int)threadIdx.x;
  if (qi >= rg.n) return;
  const int r = parent[rg.s + qi];
  int lab = 0;
  if (r >= 0) {
    for (int i = 0; i < k; ++i) lab = s_root[i] == r ? i + 1 : lab;
  }
  labels[rg.s + qi] = lab;
}

// Every cloud is empty: no label, the tables in their "nothing found" state.
__global__ __launch_bounds__(kChunk) void cl_nothing_kernel(int b, int max_labels, int32_t *__restrict__ num_labels,
                                                            int32_t *__restrict__ label_points,
                                                            int32_t *__restrict__ label_root) {
  const long long i = (long long)blockIdx.x * kChunk + threadIdx.x;
  if (i < b) num_labels[i] = 0;
  if (i < (long long)b * max_labels) {
    label_points[i] = 0;
    label_root[i] = -1;
  }
}

// ------------------------------------------------------------------------------------------------------------ split --
// The label of the lane's row if it is one of 1 .. max_labels, else 0; the counts of every label per wave -> s_cnt[wave][.]
// (each wave writes its own row: no atomics); `before` = the rows of the same label in lower lanes of the wave.
__device__ __forceinline__ int split_rank(const int32_t *__restrict__ labels, const Range &rg, int qi, int max_labels,
                                          int (*s_cnt)[kMaxLabels], int &before) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lab = qi < rg.n ? labels[rg.s + qi] : 0;
  if (lab < 1 || lab > max_labels) lab = 0;
  s_cnt[wave][lane] = 0;   // kMaxLabels == 64 lanes
  before = 0;
  unsigned long long todo = __ballot(lab > 0);
  while (todo) {   // uniform: todo is a ballot
    const int lead = __ffsll((long long)todo) - 1;
    const int l = __shfl(lab, lead, 64);
    const unsigned long long same = __ballot(lab == l);
    if (lane == lead) s_cnt[wave][l - 1] = __popcll(same);
    if (lab == l) before = __popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  __syncthreads();
  return lab;
}
static_assert(kMaxLabels == 64, "one lane clears one counter");

// WRITE 0: rows per label of the chunk -> cnt[tile][label].  WRITE 1 (after the two scans): the rows go out.
template <int WRITE>
__global__ __launch_bounds__(kChunk) void split_kernel(const float *__restrict__ pts, const int32_t *__restrict__ labels,
                                                       const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                       int n_max, int rows, int chunks_max, int max_labels,
                                                       int32_t *__restrict__ cnt, const int32_t *__restrict__ obj_start,
                                                       float *__restrict__ out_points, int32_t *__restrict__ out_row) {
  __shared__ int s_cnt[kChunk / 64][kMaxLabels];
  const int ch = blockIdx.x % chunks_max;
  const int cloud = blockIdx.x / chunks_max;
  const Range rg = cloud_range(start, count, cloud, n_max, rows);
  if (ch * kChunk >= rg.n) return;   // uniform over the workgroup
  const int qi = ch * kChunk + (int)threadIdx.x, wave = threadIdx.x >> 6;
  int before;
  const int lab = split_rank(labels, rg, qi, max_labels, s_cnt, before);
  const long long tile = (long long)cloud * chunks_max + ch;
  if (WRITE == 0) {
    if ((int)threadIdx.x < max_labels) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kChunk / 64; ++w) c += s_cnt[w][threadIdx.x];
      cnt[tile * max_labels + threadIdx.x] = c;
    }
  } else if (lab > 0) {
#pragma unroll
    for (int w = 0; w < kChunk / 64; ++w) before += w < wave ? s_cnt[w][lab - 1] : 0;
    const long long dst = (long long)obj_start[(long long)cloud * max_labels + lab - 1] + cnt[tile * max_labels + lab - 1] + before;
    const long long src = rg.s + qi;
    if (dst >= rows) return;   // only if the ranges overlap, against the contract
#pragma unroll
    for (int c = 0; c < 3; ++c) out_points[dst * 3 + c] = pts[src * 3 + c];
    out_row[dst] = qi;
  }
}

// One workgroup of 64 per cloud, lane l owns label l + 1: the chunk counts -> exclusive offsets (in place), the sum ->
// obj_count.  The reads of a step are one coalesced row of cnt.
__global__ __launch_bounds__(64) void split_scan_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ count,
                                                        int n_max, int rows, int chunks_max, int max_labels,
                                                        int32_t *__restrict__ cnt, int32_t *__restrict__ obj_count) {
  const int cloud = blockIdx.x, l = threadIdx.x;
  if (l >= max_labels) return;
  const int chunks = chunks_of(cloud_range(start, count, cloud, n_max, rows).n);
  int32_t *c = cnt + (long long)cloud * chunks_max * max_labels + l;
  int run = 0;
  for (int ch = 0; ch < chunks; ++ch) {
    const int v = c[(long long)ch * max_labels];
    c[(long long)ch * max_labels] = run;
    run += v;
  }
  obj_count[(long long)cloud * max_labels + l] = run;
}

// One workgroup: obj_start = the exclusive sum of obj_count over (cloud, label); out_total = the sum.  Thread t owns the
// entries t*per .. (t+1)*per - 1.
__global__ __launch_bounds__(256) void split_starts_kernel(long long entries, const int32_t *__restrict__ obj_count,
                                                           int32_t *__restrict__ obj_start, int32_t *__restrict__ out_total) {
  __shared__ int sums[256];
  const int tid = threadIdx.x;
  const long long per = (entries + 255) / 256;
  const long long e0 = min(entries, tid * per), e1 = min(entries, e0 + per);
  int mine = 0;
  for (long long e = e0; e < e1; ++e) mine += obj_count[e];
  sums[tid] = mine;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += sums[t];
  for (long long e = e0; e < e1; ++e) {
    obj_start[e] = base;
    base += obj_count[e];
  }
  if (tid == 255) *out_total = base;   // its range is the last (possibly empty): base = the sum of all
}

// No pointer is read and the device is not touched outside these.
int check_layout(int b, int n_max, int rows) {
  if (b < 1 || n_max < 0 || rows < 0) return GLDM_ERR_INVALID_ARG;
  if (b > kMaxClouds || n_max > kMaxClusterN || rows > kMaxClusterRows) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

int check_split(int b, int n_max, int rows, int max_labels) {
  if (b < 1 || n_max < 0 || rows < 0 || max_labels < 1) return GLDM_ERR_INVALID_ARG;
  if (b > kMaxClouds || n_max > kMaxClusterN || rows > kMaxClusterRows || max_labels > kMaxLabels) return GLDM_ERR_UNSUPPORTED;
  if ((long long)b * chunks_of(n_max) * max_labels > kMaxSplitCounters) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

inline long long align16(long long v) { return (v + 15) & ~15ll; }

struct ClusterSpace {
  long long sorted, table, cand, slot_of, parent, size, tile_cnt, act_start, act_count, cand_count, bytes;
};

ClusterSpace cluster_space(int b, int n_max, int rows) {
  ClusterSpace w;
  const long long r = rows, per_cloud = align8((long long)b * (long long)sizeof(int32_t));
  long long at = 0;
  w.sorted = at;     at += r * (long long)sizeof(Member);
  w.table = at;      at += 2 * r * (long long)sizeof(CSlot);
  w.cand = at;       at += r * 8;
  w.slot_of = at;    at += align8(r * 4);
  w.parent = at;     at += align8(r * 4);
  w.size = at;       at += align8(r * 4);
  w.tile_cnt = at;   at += align8((long long)b * chunks_of(n_max) * 4);
  w.act_start = at;  at += per_cloud;
  w.act_count = at;  at += per_cloud;
  w.cand_count = at; at += per_cloud;
  w.bytes = align16(at);
  return w;
}

}  // namespace

GLDM_API long long gldm_cluster_cloud_workspace_bytes(int b, int n_max, int rows) {
  const int st = check_layout(b, n_max, rows);
  if (st != GLDM_OK) return st;
  return cluster_space(b, n_max, rows).bytes;
}

GLDM_API int gldm_cluster_cloud(const float *points, const int32_t *start, const int32_t *count, int b, int n_max, int rows,
                                float link_dist, const float *plane, float h_min, float h_max, int min_points, int max_labels,
                                void *workspace, long long workspace_bytes, int32_t *labels, int32_t *num_labels,
                                int32_t *label_points, int32_t *label_root, gldm_stream_t stream) {
  // the envelope first: nothing below touches a pointer or the device before it holds
  if (b < 1 || n_max < 0 || rows < 0 || min_points < 1 || max_labels < 1) return GLDM_ERR_INVALID_ARG;
  if (!(link_dist >= kMinLink && link_dist <= kMaxLink)) return GLDM_ERR_INVALID_ARG;   // NaN, inf, <= 0 fail as well
  const int env = check_layout(b, n_max, rows);
  if (env != GLDM_OK) return env;
  if (max_labels > kMaxLabels) return GLDM_ERR_UNSUPPORTED;
  if (!start || !count || !num_labels || !label_points || !label_root) return GLDM_ERR_INVALID_ARG;
  ClusterParams P;
  P.cs = (double)link_dist * (1.0 + 0x1p-10);
  P.link2 = link_dist * link_dist;   // formed once, in f32
  P.a = P.b = P.c = P.d = 0.f;
  P.h_min = h_min;
  P.h_max = h_max;
  P.use_plane = plane != nullptr;
  if (plane) {
    if (plane[0] != plane[0] || plane[1] != plane[1] || plane[2] != plane[2] || plane[3] != plane[3] || !(h_min < h_max))
      return GLDM_ERR_INVALID_ARG;
    P.a = plane[0]; P.b = plane[1]; P.c = plane[2]; P.d = plane[3];
  }
  hipStream_t st = as_stream(stream);
  if (n_max == 0 || rows == 0) {   // every cloud is empty: the tables are still written
    const long long cells = (long long)b * max_labels;
    hipLaunchKernelGGL(cl_nothing_kernel, dim3((unsigned)((cells + kChunk - 1) / kChunk)), dim3(kChunk), 0, st, b, max_labels,
                       num_labels, label_points, label_root);
    return launch_status();
  }
  if (!points || !labels || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return GLDM_ERR_INVALID_ARG;
  const ClusterSpace w = cluster_space(b, n_max, rows);
  if (workspace_bytes < w.bytes) return GLDM_ERR_WORKSPACE;
  char *ws = static_cast<char *>(workspace);
  Member *sorted = reinterpret_cast<Member *>(ws + w.sorted);
  CSlot *table = reinterpret_cast<CSlot *>(ws + w.table);
  unsigned long long *cand = reinterpret_cast<unsigned long long *>(ws + w.cand);
  int32_t *slot_of = reinterpret_cast<int32_t *>(ws + w.slot_of);
  int32_t *parent = reinterpret_cast<int32_t *>(ws + w.parent);
  int32_t *size = reinterpret_cast<int32_t *>(ws + w.size);
  int32_t *tile_cnt = reinterpret_cast<int32_t *>(ws + w.tile_cnt);
  int32_t *act_start = reinterpret_cast<int32_t *>(ws + w.act_start);
  int32_t *act_count = reinterpret_cast<int32_t *>(ws + w.act_count);
  int32_t *cand_count = reinterpret_cast<int32_t *>(ws + w.cand_count);
  const int chunks_max = chunks_of(n_max);
  const dim3 grid((unsigned)((long long)b * chunks_max)), block(kChunk);   // <= 65535 * 16384
  hipLaunchKernelGGL(cl_init_kernel, grid, block, 0, st, start, count, n_max, rows, chunks_max, table, cand_count);
  hipLaunchKernelGGL(cl_insert_kernel, grid, block, 0, st, points, start, count, n_max, rows, chunks_max, P, table, slot_of,
                     parent, size);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(cl_offsets_kernel<0>, grid, block, 0, st, start, count, n_max, rows, chunks_max, table, tile_cnt);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(256), 0, st, start, count, b, n_max, rows, chunks_max, tile_cnt, act_start,
                     act_count);
  hipLaunchKernelGGL(cl_offsets_kernel<1>, grid, block, 0, st, start, count, n_max, rows, chunks_max, table, tile_cnt);
  hipLaunchKernelGGL(cl_scatter_kernel, grid, block, 0, st, points, start, count, n_max, rows, chunks_max, table, slot_of, sorted);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(cl_union_kernel, grid, block, 0, st, start, count, n_max, rows, chunks_max, P, table, sorted, act_count,
                     parent);
  hipLaunchKernelGGL(cl_flatten_kernel, grid, block, 0, st, start, count, n_max, rows, chunks_max, parent, size);
  hipLaunchKernelGGL(cl_gather_kernel, grid, block, 0, st, start, count, n_max, rows, chunks_max, parent, size, min_points, cand,
                     cand_count);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(cl_select_kernel, dim3(b), dim3(kSelectBlock), 0, st, start, count, n_max, rows, cand, cand_count,
                     max_labels, num_labels, label_points, label_root);
  hipLaunchKernelGGL(cl_write_kernel, grid, block, 0, st, start, count, n_max, rows, chunks_max, max_labels, parent, num_labels,
                     label_root, labels);
  return launch_status();
}

// workspace: cnt int32 [b, chunks, max_labels]
GLDM_API long long gldm_split_labels_workspace_bytes(int b, int n_max, int rows, int max_labels) {
  const int st = check_split(b, n_max, rows, max_labels);
  if (st != GLDM_OK) return st;
  return align8((long long)b * chunks_of(n_max) * max_labels * (long long)sizeof(int32_t));
}

GLDM_API int gldm_split_labels(const float *points, const int32_t *labels, const int32_t *start, const int32_t *count, int b,
                               int n_max, int rows, int max_labels, void *workspace, long long workspace_bytes,
                               float *out_points, int32_t *out_row, int32_t *obj_start, int32_t *obj_count, int32_t *out_total,
                               gldm_stream_t stream) {
  const int env = check_split(b, n_max, rows, max_labels);
  if (env != GLDM_OK) return env;
  const bool empty = n_max == 0 || rows == 0;   // every cloud is empty: the tables are still written
  if (!start || !count || !obj_start || !obj_count || !out_total) return GLDM_ERR_INVALID_ARG;
  if (!empty && (!points || !labels || !out_points || !out_row || !workspace)) return GLDM_ERR_INVALID_ARG;
  if (!empty && workspace_bytes < gldm_split_labels_workspace_bytes(b, n_max, rows, max_labels)) return GLDM_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const int chunks_max = empty ? 0 : chunks_of(n_max);
  const int n_eff = empty ? 0 : n_max;   // the scans then see empty clouds and read no counter
  int32_t *cnt = static_cast<int32_t *>(workspace);
  const dim3 grid((unsigned)((long long)b * chunks_max)), block(kChunk);
  if (!empty)
    hipLaunchKernelGGL(split_kernel<0>, grid, block, 0, st, points, labels, start, count, n_max, rows, chunks_max, max_labels,
                       cnt, obj_start, out_points, out_row);
  hipLaunchKernelGGL(split_scan_kernel, dim3(b), dim3(64), 0, st, start, count, n_eff, rows, chunks_max, max_labels, cnt,
                     obj_count);
  hipLaunchKernelGGL(split_starts_kernel, dim3(1), dim3(256), 0, st, (long long)b * max_labels, obj_count, obj_start, out_total);
  if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  if (!empty)
    hipLaunchKernelGGL(split_kernel<1>, grid, block, 0, st, points, labels, start, count, n_max, rows, chunks_max, max_labels,
                       cnt, obj_start, out_points, out_row);
  return launch_status();
}
