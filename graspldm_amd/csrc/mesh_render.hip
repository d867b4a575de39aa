// mesh_render.hip -- depth, instance-label and face-index frames of triangle meshes seen by a pinhole camera
// (include/gldm.h, "meshes"):
//
//   gldm_render_depth  frames of h x w pixels; frame r draws a range of an instance table whose rows place a mesh of the
//                      batch in front of the camera.
//
// Two launches.  setup_kernel writes one record per (instance, face): the projected vertices, their depths, the label and
// the face row, and beside it the integer pixel box of the triangle.  tile_kernel runs one workgroup per 16 x 16 pixel tile:
// it walks the boxes of its frame 256 at a time, stages the records whose box meets the tile in LDS (ballot + popcount
// compaction) and every thread tests its own pixel against them, keeping the minimum of (depth bits << 32 | record) in
// registers.  No atomics, no initialising pass, no workgroup waits for another: every pixel is a pure function of the inputs.
// Compiled with -ffp-contract=off (csrc/Makefile: SRCS_STRICT): every operation below rounds once, as tests/mesh_ref.py
// restates it.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "host_util.h"
#include "mesh_range.h"

namespace {

constexpr int kTile = 16;                  // pixels per tile side; kTile * kTile threads
constexpr int kMaxFrames = 65535;
constexpr int kMaxInstances = 65535;
constexpr int kMaxTris = 1 << 24;          // records of one call: the low word of a pixel's key
constexpr int kMaxPixels = 1 << 24;
constexpr unsigned long long kEmpty = ~0ull;

struct Rec {
  float px[3], py[3], z[3];
  int32_t label, face, pad;
};
static_assert(sizeof(Rec) == 48, "workspace layout");

// The pixels a triangle can cover: x0 <= u <= x1, y0 <= v <= y1.  A record that draws nothing has x0 > x1; y0 = 1 then
// marks a triangle that was dropped (and is counted), y0 = 0 one that was skipped.
struct Box {
  int32_t x0, y0, x1, y1;
};

struct Optics {
  float fx, fy, cx, cy, z_near, z_far;
};

struct Instances {
  const int32_t *mesh;    // [n_inst]
  const float *xf;        // [n_inst, 12]: obj_to_cam, 3 x 4 row major
  const int32_t *label;   // [n_inst]
  const int32_t *tri;     // [n_inst]: first record
  int n_inst, n_tris, b;
};

// ceil of the smallest / floor of the largest coordinate as pixel indices; -1 and 2^24 stand for everything outside.
__device__ __forceinline__ int pixel_of(float x) { return (int)fminf(fmaxf(x, -1.f), 16777216.f); }

__global__ __launch_bounds__(256) void setup_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                    MeshArrays ma, Instances in, Optics o, Rec *__restrict__ recs,
                                                    Box *__restrict__ boxes) {
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= in.n_tris) return;
  Box box = {1, 0, 0, 0};
  Rec rec = {};
  // the last instance whose first record is not behind r
  int lo = 0, hi = in.n_inst;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (in.tri[mid] <= r) lo = mid + 1; else hi = mid;
  }
  const int inst = lo - 1;
  const int mesh = inst >= 0 ? in.mesh[inst] : -1;
  if (mesh >= 0 && mesh < in.b) {
    const MeshRange mr = mesh_range(ma, mesh);
    const long long local = (long long)r - in.tri[inst];
    if (local >= 0 && local < mr.fn) {
      const Tri t = load_tri(verts, faces, mr, mr.fs + local);
      if (t.ok) {
        const float *m = in.xf + (long long)inst * 12;
        bool draw = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float x = t.v[k][0], y = t.v[k][1], z = t.v[k][2];
          const float X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
          const float Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
          const float Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
          draw = draw && Z >= o.z_near;   // false for a NaN
          rec.px[k] = __fdiv_rn(X * o.fx, Z) + o.cx;
          rec.py[k] = __fdiv_rn(Y * o.fy, Z) + o.cy;
          rec.z[k] = Z;
          draw = draw && fabsf(rec.px[k]) < INFINITY && fabsf(rec.py[k]) < INFINITY;
        }
        rec.label = in.label[inst];
        rec.face = (int32_t)(mr.fs + local);
        if (draw) {
          box.x0 = pixel_of(ceilf(fminf(fminf(rec.px[0], rec.px[1]), rec.px[2])));
          box.x1 = pixel_of(floorf(fmaxf(fmaxf(rec.px[0], rec.px[1]), rec.px[2])));
          box.y0 = pixel_of(ceilf(fminf(fminf(rec.py[0], rec.py[1]), rec.py[2])));
          box.y1 = pixel_of(floorf(fmaxf(fmaxf(rec.py[0], rec.py[1]), rec.py[2])));
          if (box.x0 > box.x1) box = {1, 0, 0, 0};   // between two pixel columns
        } else {
          box.y0 = 1;
        }
      }
    }
  }
  recs[r] = rec;
  boxes[r] = box;
}

// (bx - ax)(py - ay) - (by - ay)(px - ax) in f64, evaluated from the lexicographically lower endpoint of the edge and
// negated when that is b: the two triangles on a shared edge get bitwise opposite values.
__device__ __forceinline__ double edge_fn(float ax, float ay, float bx, float by, double px, double py) {
  const bool fwd = ax < bx || (ax == bx && ay <= by);
  const double ox = fwd ? ax : bx, oy = fwd ? ay : by, tx = fwd ? bx : ax, ty = fwd ? by : ay;
  const double e = (tx - ox) * (py - oy) - (ty - oy) * (px - ox);
  return fwd ? e : -e;
}

__global__ __launch_bounds__(kTile * kTile) void tile_kernel(const Rec *__restrict__ recs, const Box *__restrict__ boxes,
                                                             Instances in, const int32_t *__restrict__ frame_start,
                                                             const int32_t *__restrict__ frame_count, int h, int w, int tiles_x,
                                                             Optics o, float *__restrict__ depth, int32_t *__restrict__ label,
                                                             int32_t *__restrict__ face, int32_t *__restrict__ dropped) {
  constexpr int kThreads = kTile * kTile;
  __shared__ Rec srec[kThreads];
  __shared__ int sidx[kThreads];
  __shared__ int wcnt[kThreads / 64];
  __shared__ int sdrop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frame = blockIdx.y;
  const int tx0 = (int)(blockIdx.x % tiles_x) * kTile, ty0 = (int)(blockIdx.x / tiles_x) * kTile;
  const int u = tx0 + (tid & (kTile - 1)), v = ty0 + tid / kTile;
  // the records of the frame: from the first record of its first instance to the first record behind its last
  int lo = 0, hi = 0;
  {
    const long long is = frame_start[frame], ic = frame_count[frame];
    if (is >= 0 && ic > 0 && is + ic <= in.n_inst) {
      lo = in.tri[is];
      hi = is + ic < in.n_inst ? in.tri[is + ic] : in.n_tris;
      lo = max(0, min(lo, in.n_tris));
      hi = max(lo, min(hi, in.n_tris));
    }
  }
  if (tid == 0) sdrop = 0;
  unsigned long long best = kEmpty;
  int ndrop = 0;
  const double px = (double)u, py = (double)v;
  for (int base = lo; base < hi; base += kThreads) {
    const int r = base + tid;
    Box bx = {1, 0, 0, 0};
    if (r < hi) bx = boxes[r];
    const bool draws = bx.x0 <= bx.x1;
    ndrop += (!draws && bx.y0 == 1) ? 1 : 0;
    const bool hit = draws && bx.x0 <= tx0 + kTile - 1 && bx.x1 >= tx0 && bx.y0 <= ty0 + kTile - 1 && bx.y1 >= ty0;
    const unsigned long long bal = __ballot(hit);
    __syncthreads();   // wcnt, srec and sidx are free again
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int slot = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
      slot += k < wave ? wcnt[k] : 0;
      total += wcnt[k];
    }
    if (hit) {
      srec[slot] = recs[r];
      sidx[slot] = r;
    }
    __syncthreads();
    for (int j = 0; j < total; ++j) {
      const Rec &t = srec[j];
      // inside the triangle's own pixel box: a consequence of the edge test in exact arithmetic, part of the rule here
      const float x_lo = fminf(fminf(t.px[0], t.px[1]), t.px[2]), x_hi = fmaxf(fmaxf(t.px[0], t.px[1]), t.px[2]);
      const float y_lo = fminf(fminf(t.py[0], t.py[1]), t.py[2]), y_hi = fmaxf(fmaxf(t.py[0], t.py[1]), t.py[2]);
      if (!((float)u >= x_lo && (float)u <= x_hi && (float)v >= y_lo && (float)v <= y_hi)) continue;
      const double w0 = edge_fn(t.px[1], t.py[1], t.px[2], t.py[2], px, py);
      const double w1 = edge_fn(t.px[2], t.py[2], t.px[0], t.py[0], px, py);
      const double w2 = edge_fn(t.px[0], t.py[0], t.px[1], t.py[1], px, py);
      const double s = (w0 + w1) + w2;
      const bool in_tri = ((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0)) && s != 0.0;
      if (!in_tri) continue;
      const double q = ((w0 / (double)t.z[0] + w1 / (double)t.z[1]) + w2 / (double)t.z[2]) / s;
      const float z = (float)(1.0 / q);
      if (!(z >= o.z_near && z <= o.z_far)) continue;
      const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)sidx[j];
      best = key < best ? key : best;
    }
  }
  if (blockIdx.x == 0) {   // the frame's first tile has seen every box of the frame
    if (ndrop) atomicAdd(&sdrop, ndrop);
    __syncthreads();
    if (tid == 0) dropped[frame] = sdrop;
  }
  if (u >= w || v >= h) return;
  const long long at = ((long long)frame * h + v) * w + u;
  const bool empty = best == kEmpty;
  const int r = (int)(best & 0xffffffffull);
  depth[at] = empty ? 0.f : __uint_as_float((unsigned)(best >> 32));
  if (label) label[at] = empty ? 0 : recs[r].label;
  if (face) face[at] = empty ? -1 : recs[r].face;
}

// No pointer is read and the device is not touched outside it.
int check_envelope(int b, int n_verts, int n_faces, int n_inst, int n_tris, int frames, int h, int w) {
  if (b < 1 || n_verts < 0 || n_faces < 0 || n_inst < 0 || n_tris < 0 || frames < 1 || h < 1 || w < 1)
    return GLDM_ERR_INVALID_ARG;
  if (b > kMaxMeshes || n_verts > kMaxMeshRows || n_faces > kMaxMeshRows || n_inst > kMaxInstances || n_tris > kMaxTris ||
      frames > kMaxFrames || (long long)h * w > kMaxPixels)
    return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

}  // namespace

// workspace: Rec [n_tris], Box [n_tris]
GLDM_API long long gldm_render_depth_workspace_bytes(int b, int n_verts, int n_faces, int n_inst, int n_tris, int frames, int h,
                                                     int w) {
  const int st = check_envelope(b, n_verts, n_faces, n_inst, n_tris, frames, h, w);
  if (st != GLDM_OK) return st;
  return (long long)n_tris * (long long)(sizeof(Rec) + sizeof(Box));
}

GLDM_API int gldm_render_depth(const float *vertices, const int32_t *faces, const int32_t *vert_start, const int32_t *vert_count,
                               const int32_t *face_start, const int32_t *face_count, int b, int n_verts, int n_faces,
                               const int32_t *inst_mesh, const float *inst_xf, const int32_t *inst_label,
                               const int32_t *inst_tri, int n_inst, int n_tris, const int32_t *frame_start,
                               const int32_t *frame_count, int frames, int h, int w, float fx, float fy, float cx, float cy,
                               float z_near, float z_far, void *workspace, long long workspace_bytes, float *depth,
                               int32_t *label, int32_t *face, int32_t *dropped, gldm_stream_t stream) {
  const int env = check_envelope(b, n_verts, n_faces, n_inst, n_tris, frames, h, w);
  if (env != GLDM_OK) return env;
  if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f || !isfinite(cx) || !isfinite(cy) || !(z_near > 0.f) ||
      !(z_near < z_far) || !isfinite(z_far))
    return GLDM_ERR_INVALID_ARG;
  if (!vert_start || !vert_count || !face_start || !face_count || !frame_start || !frame_count || !depth || !dropped)
    return GLDM_ERR_INVALID_ARG;
  if (n_inst > 0 && (!inst_mesh || !inst_xf || !inst_label || !inst_tri)) return GLDM_ERR_INVALID_ARG;
  if (n_tris > 0 && (!workspace || !vertices || !faces || n_inst == 0)) return GLDM_ERR_INVALID_ARG;
  if (workspace_bytes < gldm_render_depth_workspace_bytes(b, n_verts, n_faces, n_inst, n_tris, frames, h, w))
    return GLDM_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  Rec *recs = static_cast<Rec *>(workspace);
  Box *boxes = reinterpret_cast<Box *>(recs + n_tris);
  const MeshArrays ma = {vert_start, vert_count, face_start, face_count, kMaxMeshFaces, n_verts, n_faces};
  const Instances in = {inst_mesh, inst_xf, inst_label, inst_tri, n_tris > 0 ? n_inst : 0, n_tris, b};
  const Optics o = {fx, fy, cx, cy, z_near, z_far};
  if (n_tris > 0) {
    hipLaunchKernelGGL(setup_kernel, dim3(ceil_div(n_tris, 256)), dim3(256), 0, st, vertices, faces, ma, in, o, recs, boxes);
    if (launch_status() != GLDM_OK) return GLDM_ERR_LAUNCH;
  }
  const int tiles_x = ceil_div(w, kTile), tiles_y = ceil_div(h, kTile);
  hipLaunchKernelGGL(tile_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)frames), dim3(kTile * kTile), 0, st, recs, boxes,
                     in, frame_start, frame_count, h, w, tiles_x, o, depth, label, face, dropped);
  return launch_status();
}
