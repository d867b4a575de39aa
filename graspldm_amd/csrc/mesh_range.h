// mesh_range.h -- the packed layout of a ragged batch of triangle meshes that mesh_sample.hip and mesh_render.hip share:
// mesh i owns the rows vert_start[i] .. + vert_count[i] of vertices [n_verts,3] and face_start[i] .. + face_count[i] of
// faces [n_faces,3]; a face's indices are local to its mesh.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kMeshChunk = 256;
constexpr int kMaxMeshes = 65535;
constexpr int kMaxMeshFaces = 1 << 22;   // faces of one mesh: their integer weights (40 bits each) sum below 2^62
constexpr int kMaxMeshRows = 1 << 24;    // rows of the packed vertex and face arrays

struct MeshArrays {
  const int32_t *vert_start, *vert_count, *face_start, *face_count;
  int f_max, n_verts, n_faces;
};

struct MeshRange {
  long long vs, fs;   // first vertex row, first face row
  int vn, fn;         // vertices, faces
};

// The rows of one mesh: the face count clamped to [0, f_max]; a range that leaves its array is empty, so nothing outside the
// arrays is ever addressed.  A mesh without vertices keeps its faces: every one of them then has an index out of range.
__device__ __forceinline__ MeshRange mesh_range(const MeshArrays &m, int mesh) {
  MeshRange r;
  r.vs = m.vert_start[mesh];
  r.fs = m.face_start[mesh];
  r.vn = max(0, m.vert_count[mesh]);
  r.fn = max(0, min(m.face_count[mesh], m.f_max));
  if (r.vs < 0 || r.vs + r.vn > (long long)m.n_verts) r.vn = 0;
  if (r.fs < 0 || r.fs + r.fn > (long long)m.n_faces) r.fn = 0;
  return r;
}

struct Tri {
  float v[3][3];
  bool ok;
};

// The vertices of packed face `row` of a mesh; not ok (and nothing read past the index row) when an index leaves the mesh.
__device__ __forceinline__ Tri load_tri(const float *__restrict__ verts, const int32_t *__restrict__ faces, const MeshRange &mr,
                                        long long row) {
  Tri t;
  int idx[3];
  t.ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k] = faces[row * 3 + k];
    t.ok = t.ok && idx[k] >= 0 && idx[k] < mr.vn;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) t.v[k][c] = t.ok ? verts[(mr.vs + idx[k]) * 3 + c] : 0.f;
  return t;
}

}  // namespace
