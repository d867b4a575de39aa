// grasp_select.hip -- geometric filtering and selection of grasp poses (include/gldm.h, "grasp selection"):
//
//   gldm_grasp_clearance  distance of the open gripper's segments (grasp_ldm/utils/gripper.py:26-31) to a whole scene cloud,
//                         and the number of scene points inside the finger-sweep tubes (:33-47, :80-103), per pose.
//   gldm_grasp_contact_normals  the same contact set split by finger, and how many of each side's contacts have their
//                         surface normal inside the friction cone around the pose's closing axis.
//   gldm_select_grasps    top-k or greedy farthest-pose ("diverse") selection per cloud, under the control-point distance of
//                         grasp_ldm/losses/loss.py:77-127.
//
// Compiled with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): every decision below (broad phase, contact test, argmax)
// is taken on values rounded once per written operation, so a pose decides the same in every launch shape.  Nothing here
// uses the matrix pipe; the reductions are this file's own.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gldm.h"

#define GLDM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kMaxSeg = 8;          // segments per family (body, sweep)
constexpr int kChunk = 256;         // scene points staged per step = threads per workgroup (gldm_grasp_clearance_chunk)
constexpr int kPoseTile = 4;        // poses a workgroup carries through its share of the scene: 48 scalar registers
constexpr int kMaxNs = 1 << 24;
constexpr int kSelThreads = 256, kSelPer = 8;
constexpr int kSelMaxG = kSelThreads * kSelPer;   // 2048 candidates per cloud, twelve floats each in registers
constexpr int kSelMaxNp = 64;

// One segment family by value, in the kernel-argument segment: a, ab = b - a, inv = 1 / |ab|^2 (0 for a point).  A
// segment is one 32-byte scalar load at a wave-uniform index; only the narrow phase reads it, so the families stay out
// of the scalar registers that the tile's poses need.
struct Seg {
  float ax, ay, az, dx, dy, dz, inv, pad;
};
struct SegSet {
  Seg s[kMaxSeg];
  int n, pad[7];
};

struct alignas(32) ClearArgs {
  SegSet body, sweep;
  float cx, cy, cz;   // bounding-sphere centre of both families
  float reach2;       // (rho + max(cap, r_sweep))^2 with a margin: the broad phase keeps |q - c|^2 <= reach2
  float r2;           // r_sweep^2
  float cap;
};

// A pointer whose loads at a wave-uniform address are scalar loads (the constant address space): for inputs that no launch
// of this file writes.
typedef const float __attribute__((address_space(4))) *scalar_ptr;
__device__ __forceinline__ scalar_ptr as_scalar(const float *p) { return (scalar_ptr)(uintptr_t)p; }

// Squared distance of q to the set's nearest segment (+inf for an empty set).
__device__ __forceinline__ float seg_min_d2(const SegSet &s, float qx, float qy, float qz) {
  float best = __builtin_inff();
#pragma clang loop unroll(disable) vectorize(disable)
  for (int i = 0; i < s.n; ++i) {   // wave-uniform
    const Seg g = s.s[i];
    const float px = qx - g.ax, py = qy - g.ay, pz = qz - g.az;
    float u = (px * g.dx + py * g.dy + pz * g.dz) * g.inv;
    u = fminf(fmaxf(u, 0.f), 1.f);
    const float wx = px - u * g.dx, wy = py - u * g.dy, wz = pz - u * g.dz;
    best = fminf(best, wx * wx + wy * wy + wz * wz);
  }
  return best;
}

__global__ __launch_bounds__(256) void clearance_init_kernel(float *__restrict__ clearance, int32_t *__restrict__ contacts,
                                                             long long poses, float cap) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < poses) {
    clearance[i] = cap;
    contacts[i] = 0;
  }
}

// Grid: slices x pose tiles x clouds, flattened.  A workgroup walks every `slices`-th chunk of its cloud: the chunk goes
// through LDS once (coalesced dword loads of the [n,3] rows, stride-3 reads: no bank conflict) and meets the tile's poses,
// whose sixteen floats are wave-uniform scalar loads.  Lanes are points.  Per pose a lane keeps the smallest squared body
// distance and its contact count; they meet across lanes, waves and workgroups as a min of non-negative floats (ordered
// like their bit patterns) and an integer sum: exact, so no bit depends on the split.  sqrt is monotone and correctly
// rounded, hence min(cap, sqrt(min d2)) is the same number wherever the sqrt is taken.
// kNormals (gldm_grasp_contact_normals): the same scan, broad phase and contact test; instead of the body distance a lane
// keeps four counts per pose -- contacts of side 0 (q.x > 0) and side 1, and those of each side whose normal satisfies
// |(R00*nx + R10*ny) + R20*nz| >= cos_friction (a zero normal never does) -- written to side[pose][2] and aligned[pose][2].
template <bool kNormals>
__global__ __launch_bounds__(kChunk) void clearance_kernel(const float *__restrict__ scene, const float *__restrict__ H,
                                                           int ns, int g, int slices, int tiles, ClearArgs a,
                                                           float *__restrict__ clearance, int32_t *__restrict__ contacts,
                                                           const float *__restrict__ normals, float cos_friction,
                                                           int32_t *__restrict__ side, int32_t *__restrict__ aligned) {
  constexpr int kCounts = kNormals ? 4 : 1;
  __shared__ float pts[kChunk * 3];
  __shared__ float nrm[kNormals ? kChunk * 3 : 1];           // the chunk's normals, staged like its points
  __shared__ float red_d[kChunk / 64][kNormals ? 1 : kPoseTile];
  __shared__ int red_c[kChunk / 64][kPoseTile * kCounts];
  const int tid = threadIdx.x;
  const unsigned bid = blockIdx.x;
  const int slice = bid % slices;
  const int tile = (bid / slices) % tiles;
  const int cloud = bid / slices / tiles;
  const int g0 = tile * kPoseTile;
  const int gn = min(kPoseTile, g - g0);
  const float *cloud_pts = scene + (long long)cloud * ns * 3;
  const float *poses = H + ((long long)cloud * g + g0) * 16;

  [[maybe_unused]] float best[kPoseTile];   // the body distance: not kept under kNormals
  int hits[kPoseTile][kCounts];
#pragma unroll
  for (int p = 0; p < kPoseTile; ++p) {
    if constexpr (!kNormals) best[p] = __builtin_inff();
#pragma unroll
    for (int c = 0; c < kCounts; ++c) hits[p][c] = 0;
  }

  const int chunks = (ns + kChunk - 1) / kChunk;
  for (int ch = slice; ch < chunks; ch += slices) {
    const int p0 = ch * kChunk;
    const int cnt = min(kChunk, ns - p0);
    const float *src = cloud_pts + (long long)p0 * 3;
    __syncthreads();   // the previous chunk has been read
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int f = tid + k * kChunk;
      if (f < cnt * 3) {
        pts[f] = src[f];
        if constexpr (kNormals) nrm[f] = normals[((long long)cloud * ns + p0) * 3 + f];
      }
    }
    __syncthreads();
    const bool live = tid < cnt;
    const float x = live ? pts[tid * 3 + 0] : 0.f, y = live ? pts[tid * 3 + 1] : 0.f, z = live ? pts[tid * 3 + 2] : 0.f;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if constexpr (kNormals) {
      if (live) nx = nrm[tid * 3 + 0], ny = nrm[tid * 3 + 1], nz = nrm[tid * 3 + 2];
    }
#pragma unroll
    for (int p = 0; p < kPoseTile; ++p) {
      if (p < gn) {   // wave-uniform
        const scalar_ptr hp = as_scalar(poses + p * 16);
        const float vx = x - hp[3], vy = y - hp[7], vz = z - hp[11];
        // q = R^T (p - t)
        const float qx = hp[0] * vx + hp[4] * vy + hp[8] * vz;
        const float qy = hp[1] * vx + hp[5] * vy + hp[9] * vz;
        const float qz = hp[2] * vx + hp[6] * vy + hp[10] * vz;
        const float ex = qx - a.cx, ey = qy - a.cy, ez = qz - a.cz;
        const bool near = live && (ex * ex + ey * ey + ez * ez <= a.reach2);
        if (__ballot(near) != 0ull) {   // a chunk nowhere near this pose costs nine multiplies per lane
          // every lane of the wave walks the segments (uniform control flow: scalar loop, scalar segment loads);
          // `near` only selects what is kept
          const float dsw = seg_min_d2(a.sweep, qx, qy, qz);
          const bool hit = near && dsw <= a.r2;   // an empty sweep family gives +inf: no contact
          if constexpr (kNormals) {
            const bool left = qx > 0.f;
            const bool cone = fabsf((hp[0] * nx + hp[4] * ny) + hp[8] * nz) >= cos_friction && (nx != 0.f || ny != 0.f || nz != 0.f);
            hits[p][0] += (hit && left) ? 1 : 0;
            hits[p][1] += (hit && !left) ? 1 : 0;
            hits[p][2] += (hit && left && cone) ? 1 : 0;
            hits[p][3] += (hit && !left && cone) ? 1 : 0;
          } else {
            const float db = seg_min_d2(a.body, qx, qy, qz);
            best[p] = near ? fminf(best[p], db) : best[p];
            hits[p][0] += hit ? 1 : 0;
          }
        }
      }
    }
  }

  // lanes -> waves -> workgroup -> the pose's words
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int p = 0; p < kPoseTile; ++p) {
    if constexpr (!kNormals) {
      float d = best[p];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) d = fminf(d, __shfl_xor(d, off));
      if (lane == 0) red_d[wave][p] = d;
    }
#pragma unroll
    for (int k = 0; k < kCounts; ++k) {
      int c = hits[p][k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
      if (lane == 0) red_c[wave][p * kCounts + k] = c;
    }
  }
  __syncthreads();
  if constexpr (kNormals) {
    if (tid < gn * 4) {   // thread = (pose of the tile, count)
      int c = red_c[0][tid];
#pragma unroll
      for (int w = 1; w < kChunk / 64; ++w) c += red_c[w][tid];
      const long long row = (long long)cloud * g + g0 + (tid >> 2);
      int32_t *out = (tid & 2) ? aligned : side;
      if (c != 0) atomicAdd(out + row * 2 + (tid & 1), c);
    }
  } else if (tid < gn) {
    float d = red_d[0][tid];
    int c = red_c[0][tid];
#pragma unroll
    for (int w = 1; w < kChunk / 64; ++w) {
      d = fminf(d, red_d[w][tid]);
      c += red_c[w][tid];
    }
    const long long row = (long long)cloud * g + g0 + tid;
    const float cl = __fsqrt_rn(d);
    if (cl < a.cap) atomicMin(reinterpret_cast<int *>(clearance) + row, __float_as_int(cl));   // cl >= 0: int order = float order
    if (c != 0) atomicAdd(contacts + row, c);
  }
}

// ------------------------------------------------------------------------------------------------------ selection --

struct SelArgs {
  float cbx, cby, cbz;                       // centroid of the control points
  float m00, m01, m02, m11, m12, m22;        // (1/Np) sum e e^T of the centred points e = c - centroid
  float min_sep2;
  int mode;
};

struct Best {
  float v;
  int i;
};
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// argmax over the workgroup of (v, lowest i); entries that do not take part carry (-inf, INT_MAX).  Every thread returns it.
__device__ __forceinline__ Best block_argmax(float v, int i, float *sv, int *si) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();   // the previous round's readers are done
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  Best b{sv[0], si[0]};
#pragma unroll
  for (int w = 1; w < kSelThreads / 64; ++w)
    if (better(sv[w], si[w], b.v, b.i)) {
      b.v = sv[w];
      b.i = si[w];
    }
  return b;
}

// One workgroup per cloud.  Thread t owns candidates t, t + 256, ... (at most eight) and keeps their poses and running
// minima in registers; the rounds of the greedy run inside the launch, each one an argmax over the workgroup.
//
// D(i, j) = (1/Np) sum_k |H_i c_k - H_j c_k|^2 with c_k = cb + e_k, sum e_k = 0:
//   D = |dt + dR cb|^2 + tr(dR Me dR^T),  dt = t_j - t_i, dR = R_j - R_i, Me = (1/Np) sum e e^T
// (the cross term of the general closed form vanishes around the centroid).  Both terms are sums of squares up to the
// rounding of Me, the differences are formed first, and an exact duplicate of a pose is at distance exactly 0.
__global__ __launch_bounds__(kSelThreads) void select_kernel(const float *__restrict__ H, const float *__restrict__ score,
                                                             const uint8_t *__restrict__ keep, int g, int k, SelArgs a,
                                                             int32_t *__restrict__ index, int32_t *__restrict__ count,
                                                             float *__restrict__ gap) {
  __shared__ float sv[kSelThreads / 64];
  __shared__ int si[kSelThreads / 64];
  __shared__ float s_score[kSelMaxG];
  __shared__ int s_total;
  const int tid = threadIdx.x;
  const int cloud = blockIdx.x;
  const float *Hc = H + (long long)cloud * g * 16;
  const float *sc = score + (long long)cloud * g;
  const uint8_t *kp = keep ? keep + (long long)cloud * g : nullptr;
  int32_t *idx_out = index + (long long)cloud * k;
  float *gap_out = gap + (long long)cloud * k;
  const float ninf = -__builtin_inff();

  if (a.mode == 0) {
    // rank of a kept candidate = kept candidates in front of it in (score falling, index rising)
    if (tid == 0) s_total = 0;
    for (int j = tid; j < g; j += kSelThreads) s_score[j] = (!kp || kp[j]) ? sc[j] : ninf;   // scores are finite: -inf = dropped
    __syncthreads();
    int kept = 0;
    for (int j = tid; j < g; j += kSelThreads) {
      const float v = s_score[j];
      if (v == ninf) continue;
      ++kept;
      int rank = 0;
      for (int i = 0; i < g; ++i) {
        const float o = s_score[i];
        rank += (o > v || (o == v && i < j)) ? 1 : 0;
      }
      if (rank < k) idx_out[rank] = j;   // ranks are distinct: one writer per slot
    }
    if (kept) atomicAdd(&s_total, kept);
    __syncthreads();
    const int n = min(s_total, k);
    for (int s = tid; s < k; s += kSelThreads) {
      if (s >= n) idx_out[s] = -1;
      gap_out[s] = 0.f;
    }
    if (tid == 0) count[cloud] = n;
    return;
  }

  float r[kSelPer][9], t[kSelPer][3], m[kSelPer], sco[kSelPer];
  bool alive[kSelPer];
#pragma unroll
  for (int c = 0; c < kSelPer; ++c) {
    const int j = tid + c * kSelThreads;
    alive[c] = j < g && (!kp || kp[j] != 0);
    m[c] = __builtin_inff();
    sco[c] = alive[c] ? sc[j] : ninf;
    const float *h = Hc + (long long)(j < g ? j : 0) * 16;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      r[c][u * 3 + 0] = h[u * 4 + 0];
      r[c][u * 3 + 1] = h[u * 4 + 1];
      r[c][u * 3 + 2] = h[u * 4 + 2];
      t[c][u] = h[u * 4 + 3];
    }
  }

  int picked = 0;
  for (int round = 0; round < k; ++round) {
    float v = ninf;
    int vi = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < kSelPer; ++c) {
      const float cand = round == 0 ? sco[c] : m[c];
      const int j = tid + c * kSelThreads;
      if (alive[c] && better(cand, j, v, vi)) {
        v = cand;
        vi = j;
      }
    }
    const Best b = block_argmax(v, vi, sv, si);
    if (b.i == 0x7fffffff) break;                          // no candidate left
    if (round > 0 && b.v < a.min_sep2) break;              // the farthest one is too close to a pick
    const int p = __builtin_amdgcn_readfirstlane(b.i);     // the same in every thread: the pick's pose is a scalar load
    if (tid == 0) {
      idx_out[round] = p;
      gap_out[round] = round == 0 ? __builtin_inff() : __fsqrt_rn(b.v);
    }
    picked = round + 1;
    const scalar_ptr hp = as_scalar(Hc + (long long)p * 16);
#pragma unroll
    for (int c = 0; c < kSelPer; ++c) {
      const int j = tid + c * kSelThreads;
      if (j == p) alive[c] = false;
      float d[9];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        d[u * 3 + 0] = r[c][u * 3 + 0] - hp[u * 4 + 0];
        d[u * 3 + 1] = r[c][u * 3 + 1] - hp[u * 4 + 1];
        d[u * 3 + 2] = r[c][u * 3 + 2] - hp[u * 4 + 2];
      }
      float D = 0.f;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const float dx = d[u * 3], dy = d[u * 3 + 1], dz = d[u * 3 + 2];
        const float w = (t[c][u] - hp[u * 4 + 3]) + (dx * a.cbx + dy * a.cby + dz * a.cbz);
        // row u of dR against Me: dR_u Me dR_u^T
        const float q = dx * (a.m00 * dx + a.m01 * dy + a.m02 * dz) + dy * (a.m01 * dx + a.m11 * dy + a.m12 * dz) +
                        dz * (a.m02 * dx + a.m12 * dy + a.m22 * dz);
        D += w * w + q;
      }
      m[c] = fminf(m[c], fmaxf(D, 0.f));
    }
  }
  for (int s = picked + tid; s < k; s += kSelThreads) {
    idx_out[s] = -1;
    gap_out[s] = 0.f;
  }
  if (tid == 0) count[cloud] = picked;
}

bool fill_segments(const float *seg, int n, SegSet *out) {
  out->n = n;
  for (int i = 0; i < kMaxSeg; ++i) {
    const bool on = i < n;
    Seg &o = out->s[i];
    o.ax = o.ay = o.az = o.dx = o.dy = o.dz = 0.f;
    if (on) {   // seg may be null for an empty family: no pointer is formed from it then
      const float *a = seg + i * 6, *b = seg + i * 6 + 3;
      for (int c = 0; c < 6; ++c)
        if (!isfinite(a[c])) return false;
      o.ax = a[0], o.ay = a[1], o.az = a[2];
      o.dx = b[0] - a[0], o.dy = b[1] - a[1], o.dz = b[2] - a[2];
    }
    const float len2 = o.dx * o.dx + o.dy * o.dy + o.dz * o.dz;
    o.inv = len2 > 0.f ? 1.f / len2 : 0.f;
    o.pad = 0.f;
  }
  for (int i = 0; i < 7; ++i) out->pad[i] = 0;
  return true;
}

// The kernel's arguments from the two segment families (host arrays; body may be empty: sb = 0): false for a non-finite
// segment or reach.
bool fill_clear_args(const float *body, int sb, const float *sweep, int ss, float r_sweep, float cap, ClearArgs *a) {
  if (!fill_segments(body, sb, &a->body) || !fill_segments(sweep, ss, &a->sweep)) return false;
  // bounding sphere of all end points (segments are convex: the end points suffice), centred on their box
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int fam = 0; fam < 2; ++fam) {
    const float *seg = fam ? sweep : body;
    for (int i = 0; i < (fam ? ss : sb) * 2; ++i)
      for (int c = 0; c < 3; ++c) {
        lo[c] = fmin(lo[c], (double)seg[i * 3 + c]);
        hi[c] = fmax(hi[c], (double)seg[i * 3 + c]);
      }
  }
  const double ctr[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
  double rho = 0.0;
  for (int fam = 0; fam < 2; ++fam) {
    const float *seg = fam ? sweep : body;
    for (int i = 0; i < (fam ? ss : sb) * 2; ++i) {
      double d2 = 0.0;
      for (int c = 0; c < 3; ++c) d2 += ((double)seg[i * 3 + c] - ctr[c]) * ((double)seg[i * 3 + c] - ctr[c]);
      rho = fmax(rho, sqrt(d2));
    }
  }
  // A skipped point must be unable to change either output AS THE KERNEL COMPUTES THEM: both phases start from the same
  // f32 q, so their disagreement is the rounding of a dozen operations on magnitudes <= reach: the 1e-3 margin is
  // four orders of magnitude above it.
  const double reach = (rho + fmax((double)cap, (double)r_sweep)) * 1.001;
  a->cx = (float)ctr[0], a->cy = (float)ctr[1], a->cz = (float)ctr[2];
  a->reach2 = (float)(reach * reach);
  a->r2 = r_sweep * r_sweep;
  a->cap = cap;
  return isfinite(a->reach2);
}

// The launch shape both entries share: slices x pose tiles x clouds workgroups.
struct ClearGrid {
  long long poses, blocks;
  int slices, tiles;
};
bool clear_grid(int b, int g, int ns, ClearGrid *gr) {
  const long long tiles = (g + kPoseTile - 1) / kPoseTile;
  const int chunks = (ns + kChunk - 1) / kChunk;
  // enough workgroups to fill the chip, no more slices than chunks
  long long slices = 4096 / (b * tiles);
  slices = slices < 1 ? 1 : (slices > chunks ? chunks : slices);
  gr->poses = (long long)b * g;
  gr->blocks = slices * tiles * b;
  gr->slices = (int)slices;
  gr->tiles = (int)tiles;
  return gr->poses <= 0x7fffffffll && gr->blocks <= 0x7fffffffll;
}

}  // namespace

GLDM_API int gldm_grasp_clearance_chunk(void) { return kChunk; }

GLDM_API int gldm_grasp_clearance(const float *scene, const float *H, int b, int g, int ns, const float *body, int sb,
                                  const float *sweep, int ss, float r_sweep, float cap, float *clearance, int32_t *contacts,
                                  gldm_stream_t stream) {
  // the envelope first: no pointer is read and the device is not touched outside it
  if (b <= 0 || g <= 0 || ns <= 0 || sb < 0 || ss < 0) return GLDM_ERR_INVALID_ARG;
  if (ns > kMaxNs || sb < 1 || sb > kMaxSeg || ss > kMaxSeg) return GLDM_ERR_UNSUPPORTED;
  if (!scene || !H || !body || (ss > 0 && !sweep) || !clearance || !contacts) return GLDM_ERR_INVALID_ARG;
  if (!(cap > 0.f) || !isfinite(cap) || !(r_sweep >= 0.f) || !isfinite(r_sweep)) return GLDM_ERR_INVALID_ARG;
  ClearGrid gr;
  if (!clear_grid(b, g, ns, &gr)) return GLDM_ERR_UNSUPPORTED;

  ClearArgs a;
  if (!fill_clear_args(body, sb, sweep, ss, r_sweep, cap, &a)) return GLDM_ERR_INVALID_ARG;

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(clearance_init_kernel, dim3((unsigned)((gr.poses + 255) / 256)), dim3(256), 0, st, clearance, contacts,
                     gr.poses, cap);
  if (hipGetLastError() != hipSuccess) return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(clearance_kernel<false>, dim3((unsigned)gr.blocks), dim3(kChunk), 0, st, scene, H, ns, g, gr.slices, gr.tiles,
                     a, clearance, contacts, nullptr, 0.f, nullptr, nullptr);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_grasp_contact_normals(const float *scene, const float *normals, const float *H, int b, int g, int ns,
                                        const float *sweep, int ss, float r_sweep, float cos_friction, int32_t *contacts_side,
                                        int32_t *aligned, gldm_stream_t stream) {
  // the envelope of gldm_grasp_clearance, checked first in the same way
  if (b <= 0 || g <= 0 || ns <= 0 || ss < 0) return GLDM_ERR_INVALID_ARG;
  if (ns > kMaxNs || ss > kMaxSeg) return GLDM_ERR_UNSUPPORTED;
  if (!scene || !normals || !H || (ss > 0 && !sweep) || !contacts_side || !aligned) return GLDM_ERR_INVALID_ARG;
  if (!(r_sweep >= 0.f) || !isfinite(r_sweep) || !(cos_friction >= 0.f) || !(cos_friction <= 1.f)) return GLDM_ERR_INVALID_ARG;
  ClearGrid gr;
  if (!clear_grid(b, g, ns, &gr) || gr.poses * 2 > 0x7fffffffll) return GLDM_ERR_UNSUPPORTED;
  // the sweep family alone: its bounding sphere plus r_sweep is the reach; every contact lies inside it, as it lies inside
  // the larger sphere of gldm_grasp_clearance, so both entries count the same points
  ClearArgs a;
  if (!fill_clear_args(nullptr, 0, sweep, ss, r_sweep, 0.f, &a)) return GLDM_ERR_INVALID_ARG;

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t bytes = (size_t)gr.poses * 2 * sizeof(int32_t);
  if (hipMemsetAsync(contacts_side, 0, bytes, st) != hipSuccess || hipMemsetAsync(aligned, 0, bytes, st) != hipSuccess)
    return GLDM_ERR_LAUNCH;
  hipLaunchKernelGGL(clearance_kernel<true>, dim3((unsigned)gr.blocks), dim3(kChunk), 0, st, scene, H, ns, g, gr.slices, gr.tiles,
                     a, nullptr, nullptr, normals, cos_friction, contacts_side, aligned);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_select_grasps(const float *H, const float *score, const uint8_t *keep, int b, int g, const float *ctrl,
                                int np, int k, int mode, float min_separation, int32_t *index, int32_t *count, float *gap,
                                gldm_stream_t stream) {
  if (b <= 0 || g <= 0 || np <= 0 || k <= 0 || (mode != 0 && mode != 1)) return GLDM_ERR_INVALID_ARG;
  if (g > kSelMaxG || np > kSelMaxNp || k > g) return GLDM_ERR_UNSUPPORTED;
  if (!H || !score || !ctrl || !index || !count || !gap) return GLDM_ERR_INVALID_ARG;
  if (!(min_separation >= 0.f) || !isfinite(min_separation)) return GLDM_ERR_INVALID_ARG;
  double cb[3] = {0, 0, 0}, me[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < np * 3; ++i) {
    if (!isfinite(ctrl[i])) return GLDM_ERR_INVALID_ARG;
    cb[i % 3] += ctrl[i];
  }
  for (int c = 0; c < 3; ++c) cb[c] /= np;
  for (int i = 0; i < np; ++i) {
    const double e0 = ctrl[i * 3] - cb[0], e1 = ctrl[i * 3 + 1] - cb[1], e2 = ctrl[i * 3 + 2] - cb[2];
    me[0] += e0 * e0, me[1] += e0 * e1, me[2] += e0 * e2, me[3] += e1 * e1, me[4] += e1 * e2, me[5] += e2 * e2;
  }
  SelArgs a;
  a.cbx = (float)cb[0], a.cby = (float)cb[1], a.cbz = (float)cb[2];
  a.m00 = (float)(me[0] / np), a.m01 = (float)(me[1] / np), a.m02 = (float)(me[2] / np);
  a.m11 = (float)(me[3] / np), a.m12 = (float)(me[4] / np), a.m22 = (float)(me[5] / np);
  a.min_sep2 = min_separation * min_separation;
  a.mode = mode;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)b), dim3(kSelThreads), 0, st, H, score, keep, g, k, a, index, count, gap);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
