"""Triangle meshes on the host: the packed batch that `pointcloud.sample_mesh_surface` and `pointcloud.render_depth` take
(include/gldm.h, "meshes"), readers for the formats object models come in, and a few primitives.

The reference reads its objects with trimesh (grasp_ldm/dataset/acronym/acronym_pointclouds.py:173-176, 402); nothing of
trimesh is needed here: Wavefront OBJ, STL (binary and ASCII) and .npz are read with numpy alone.  No torch import until a
batch goes to a device.
"""
import os
import struct

import numpy as np

MAX_MESHES = 65535        # gldm.h: b
MAX_MESH_FACES = 1 << 22  # faces of one mesh
MAX_ROWS = 1 << 24        # rows of the packed vertex / face arrays


class Mesh:
    """One mesh: vertices [V, 3] f32, faces [F, 3] int32 (indices into its own vertices)."""

    def __init__(self, vertices, faces):
        self.vertices = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
        self.faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
        _validate(self.vertices, self.faces, "mesh")
        self.faces = self.faces.astype(np.int32)

    def scaled(self, scale):
        return Mesh(self.vertices * np.float32(scale), self.faces)

    def transformed(self, matrix):
        """Vertices under a 4 x 4 (or 3 x 4) rigid transform, composed in f64 and rounded once."""
        m = np.asarray(matrix, dtype=np.float64)
        v = self.vertices.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        return Mesh(v.astype(np.float32), self.faces)

    @property
    def bounds(self):
        return self.vertices.min(axis=0), self.vertices.max(axis=0)


def _validate(vertices, faces, what):
    if not np.isfinite(vertices).all():
        raise ValueError(f"{what}: vertices must be finite")
    if faces.size and (faces.min() < 0 or faces.max() >= vertices.shape[0]):
        raise ValueError(f"{what}: face indices must lie in [0, {vertices.shape[0]}), found {int(faces.min())} .. "
                         f"{int(faces.max())}")


class MeshBatch:
    """A ragged batch of meshes in the layout of gldm.h: `vertices` [V, 3] f32 and `faces` [F, 3] int32 packed, mesh i
    owning `vert_start[i] .. + vert_count[i]` and `face_start[i] .. + face_count[i]`; face indices local to their mesh.
    Built from Mesh objects (or (vertices, faces) pairs); validated on the host: finite vertices and indices in range are
    ValueErrors, the size limits of the kernels NotImplementedErrors, before any HIP call."""

    def __init__(self, meshes):
        meshes = [m if isinstance(m, Mesh) else Mesh(*m) for m in meshes]
        if not meshes:
            raise ValueError("MeshBatch needs at least one mesh")
        self.vert_count = np.array([m.vertices.shape[0] for m in meshes], dtype=np.int32)
        self.face_count = np.array([m.faces.shape[0] for m in meshes], dtype=np.int32)
        self.vert_start = (np.cumsum(self.vert_count) - self.vert_count).astype(np.int32)
        self.face_start = (np.cumsum(self.face_count) - self.face_count).astype(np.int32)
        self.vertices = np.concatenate([m.vertices for m in meshes]).reshape(-1, 3)
        self.faces = np.concatenate([m.faces for m in meshes]).reshape(-1, 3)
        check_envelope(len(meshes), int(self.face_count.max()), self.vertices.shape[0], self.faces.shape[0])
        self._device = {}

    @classmethod
    def from_packed(cls, vertices, faces, vert_start, vert_count, face_start, face_count):
        """A batch from arrays that are packed already; every mesh's range and indices are checked."""
        vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        ranges = [np.asarray(a, dtype=np.int64).reshape(-1) for a in (vert_start, vert_count, face_start, face_count)]
        if len({a.size for a in ranges}) != 1:
            raise ValueError("vert_start, vert_count, face_start and face_count must have one length")
        meshes = []
        for i, (vs, vc, fs, fc) in enumerate(zip(*ranges)):
            if min(vs, vc, fs, fc) < 0 or vs + vc > vertices.shape[0] or fs + fc > faces.shape[0]:
                raise ValueError(f"mesh {i}: its vertex or face range leaves the packed arrays")
            try:
                meshes.append(Mesh(vertices[vs:vs + vc], faces[fs:fs + fc]))
            except ValueError as e:
                raise ValueError(f"mesh {i}: {e}") from e
        return cls(meshes)

    @classmethod
    def of(cls, meshes):
        """meshes: a MeshBatch (returned as it is), a Mesh, or a sequence of meshes."""
        if isinstance(meshes, cls):
            return meshes
        return cls([meshes] if isinstance(meshes, Mesh) else meshes)

    def __len__(self):
        return len(self.vert_count)

    def mesh(self, i):
        vs, vc, fs, fc = (int(a[i]) for a in (self.vert_start, self.vert_count, self.face_start, self.face_count))
        return Mesh(self.vertices[vs:vs + vc], self.faces[fs:fs + fc])

    @property
    def f_max(self):
        return int(self.face_count.max())

    def on(self, device):
        """The six arrays as tensors on `device` (cached): (vertices, faces, ranges [4, B] int32: vert_start, vert_count,
        face_start, face_count)."""
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("meshes go to a CUDA device (graspldm_amd has no CPU path)")
        key = str(device)
        if key not in self._device:
            ranges = np.stack([self.vert_start, self.vert_count, self.face_start, self.face_count])
            self._device[key] = (torch.from_numpy(self.vertices).to(device), torch.from_numpy(self.faces).to(device),
                                 torch.from_numpy(ranges).to(device))
        return self._device[key]


def check_envelope(b, f_max, n_verts, n_faces):
    """The limits every mesh entry of gldm.h shares, named."""
    if b > MAX_MESHES:
        raise NotImplementedError(f"{b} meshes: a batch holds at most {MAX_MESHES}")
    if f_max > MAX_MESH_FACES:
        raise NotImplementedError(f"a mesh of {f_max} faces: at most 2^22 = {MAX_MESH_FACES} faces per mesh")
    if n_verts > MAX_ROWS or n_faces > MAX_ROWS:
        raise NotImplementedError(f"{n_verts} vertices and {n_faces} faces: at most 2^24 = {MAX_ROWS} packed rows of each")


# ---------------------------------------------------------------------------------------------------------------- readers

def load_mesh(path, scale=1.0):
    """Read a Wavefront OBJ, an STL (binary or ASCII) or an .npz with `vertices` and `faces` -> Mesh, vertices times `scale`.
    OBJ: `v` and `f` lines; `a/b/c` index forms (the vertex index is the part before the first slash); negative indices count
    back from the vertices read so far; polygons are fan-triangulated.  STL: vertices with the same three bit patterns are
    merged, in order of first appearance."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        mesh = _read_obj(path)
    elif ext == ".stl":
        mesh = _read_stl(path)
    elif ext == ".npz":
        with np.load(path) as z:
            if "vertices" not in z or "faces" not in z:
                raise ValueError(f"{path}: an .npz mesh holds `vertices` and `faces`")
            mesh = Mesh(z["vertices"], z["faces"])
    else:
        raise ValueError(f"{path}: unknown mesh format '{ext}' (.obj, .stl and .npz are read)")
    return mesh if scale == 1.0 else mesh.scaled(scale)


def _read_obj(path):
    verts, faces = [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            words = line.split("#", 1)[0].split()
            if not words:
                continue
            if words[0] == "v":
                if len(words) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                verts.append([float(w) for w in words[1:4]])
            elif words[0] == "f":
                idx = []
                for w in words[1:]:
                    i = int(w.split("/", 1)[0])
                    if i == 0:
                        raise ValueError(f"{path}:{ln}: OBJ indices start at 1")
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs three vertices")
                faces.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
    try:
        return Mesh(np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from e


def _read_stl(path):
    with open(path, "rb") as f:
        data = f.read()
    tri = None
    if len(data) >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if len(data) == 84 + 50 * n:   # the size decides: a binary header may begin with "solid" too
            rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
            tri = rec["v"].reshape(-1, 3).astype(np.float32)
    if tri is None:
        words = data.decode("ascii", errors="replace").split()
        if not words or words[0] != "solid":
            raise ValueError(f"{path}: neither a binary STL of the size its header states nor an ASCII one")
        at = [i for i, w in enumerate(words) if w == "vertex"]
        if len(at) % 3:
            raise ValueError(f"{path}: {len(at)} vertices are no whole number of facets")
        tri = np.array([[float(words[i + 1]), float(words[i + 2]), float(words[i + 3])] for i in at],
                       dtype=np.float64).reshape(-1, 3).astype(np.float32)
    return Mesh(*merge_vertices(tri))


def merge_vertices(corners):
    """corners [3 F, 3] f32 (a triangle soup) -> (vertices, faces): corners with the same three bit patterns become one
    vertex; the vertices keep the order of first appearance."""
    corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 3)
    keys = corners.view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")           # unique rows by first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return corners[first[order]], rank[inverse.reshape(-1)].reshape(-1, 3)


def save_obj(path, mesh):
    with open(path, "w") as f:
        for v in mesh.vertices:
            f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in v))
        for t in mesh.faces:
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def save_stl(path, mesh, ascii=False):
    tri = mesh.vertices[mesh.faces]   # [F, 3, 3]
    if ascii:
        with open(path, "w") as f:
            f.write("solid mesh\n")
            for t in tri:
                f.write(" facet normal 0 0 0\n  outer loop\n")
                for v in t:
                    f.write("   vertex %.9g %.9g %.9g\n" % tuple(float(x) for x in v))
                f.write("  endloop\n endfacet\n")
            f.write("endsolid mesh\n")
        return
    rec = np.zeros(tri.shape[0], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["v"] = tri
    with open(path, "wb") as f:
        f.write(b"binary stl".ljust(80, b" ") + struct.pack("<I", tri.shape[0]) + rec.tobytes())


# ------------------------------------------------------------------------------------------------------------- primitives

def box(extents, center=(0.0, 0.0, 0.0)):
    """An axis-aligned box of the given edge lengths: 8 vertices, 12 faces, outward winding."""
    e = np.asarray(extents, dtype=np.float64).reshape(3) / 2
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * e + np.asarray(center)
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
         [1, 5, 7], [1, 7, 3]]
    return Mesh(v, f)


def icosphere(subdivisions=2, radius=1.0):
    """An icosahedron subdivided `subdivisions` times, vertices pushed to the sphere: 20 * 4^s faces, closed and convex."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(subdivisions)):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return Mesh(np.array(v) * float(radius), f)


def cylinder(radius, height, sections=32):
    """A closed cylinder around z, centred on the origin: 2 * sections + 2 vertices, 4 * sections faces."""
    n = int(sections)
    if n < 3:
        raise ValueError("a cylinder needs at least 3 sections")
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)
    v = np.concatenate([np.column_stack([ring, np.full(n, -height / 2)]), np.column_stack([ring, np.full(n, height / 2)]),
                        [[0, 0, -height / 2], [0, 0, height / 2]]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, n + j], [i, n + j, n + i], [2 * n, j, i], [2 * n + 1, n + i, n + j]]
    return Mesh(v, f)
