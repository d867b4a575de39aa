"""numpy restatement of gldm_mesh_sample_surface and gldm_render_depth (include/gldm.h, "meshes"): every output bit, written
from the header's rules with one numpy operation per written operation (numpy never contracts a product and a sum).  The
arrays are the raw packed ones of the C entry, so that ranges and indices a MeshBatch would refuse can be restated too."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.philox import philox4x32_10  # noqa: E402

MAX_FACES = 1 << 22
F32, F64 = np.float32, np.float64


def mesh_ranges(vert_start, vert_count, face_start, face_count, n_verts, n_faces, f_max=MAX_FACES):
    """[(vs, vn, fs, fn)] per mesh: counts clamped, a range that leaves its array empty."""
    out = []
    for vs, vc, fs, fc in zip(vert_start, vert_count, face_start, face_count):
        vs, fs = int(vs), int(fs)
        vn, fn = max(0, int(vc)), max(0, min(int(fc), int(f_max)))
        if vs < 0 or vs + vn > n_verts:
            vn = 0
        if fs < 0 or fs + fn > n_faces:
            fn = 0
        out.append((vs, vn, fs, fn))
    return out


def _tris(vertices, faces, rg):
    """(v [fn, 3, 3] f32, ok [fn]) of one mesh: the vertices of a face with an index outside the mesh are zeros."""
    vs, vn, fs, fn = rg
    idx = faces[fs:fs + fn].astype(np.int64)
    ok = np.all((idx >= 0) & (idx < vn), axis=1) if fn else np.zeros(0, bool)
    v = np.zeros((fn, 3, 3), F32)
    v[ok] = vertices[vs + idx[ok]]
    return v, ok


def _cross(v):
    """c [F, 3] and n2 [F] in f64 of triangles v [F, 3, 3] f32."""
    d = v.astype(F64)
    e1, e2 = d[:, 1] - d[:, 0], d[:, 2] - d[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return c, (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]


def face_weights(vertices, faces, rg):
    """q [fn] uint64 of one mesh."""
    v, ok = _tris(vertices, faces, rg)
    with np.errstate(all="ignore"):
        _, n2 = _cross(v)
        a = 0.5 * np.sqrt(n2)
    a[~(ok & (a > 0) & (a < np.inf))] = 0.0
    if a.size == 0 or a.max() == 0:
        return np.zeros(a.size, np.uint64)
    _, e = np.frexp(a.max())
    return np.rint(np.ldexp(a, 40 - int(e))).astype(np.uint64)


def uniforms(seed, mesh, n):
    """(k0 [n] uint64, u1, u2 [n] f32) of the in-kernel generator for one mesh."""
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = np.arange(n, dtype=np.uint32), np.uint32(mesh)
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)) >> np.uint32(8)
    s = F32(2.0 ** -24)
    return x[:, 0].astype(np.uint64), x[:, 1].astype(F32) * s, x[:, 2].astype(F32) * s


def sample_surface(vertices, faces, vert_start, vert_count, face_start, face_count, n, rand=None, seed=0, f_max=MAX_FACES):
    """-> dict(points [B, n, 3] f32, face [B, n] int32, normals [B, n, 3] f32)."""
    vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    ranges = mesh_ranges(vert_start, vert_count, face_start, face_count, vertices.shape[0], faces.shape[0], f_max)
    b = len(ranges)
    points, face, normals = np.zeros((b, n, 3), F32), np.full((b, n), -1, np.int32), np.zeros((b, n, 3), F32)
    for j, rg in enumerate(ranges):
        q = face_weights(vertices, faces, rg)
        cum = np.cumsum(q, dtype=np.uint64)
        total = int(cum[-1]) if q.size else 0
        if total == 0 or n == 0:
            continue
        if rand is None:
            k0, u1, u2 = uniforms(seed, j, n)
        else:
            with np.errstate(invalid="ignore"):
                u = np.fmin(np.fmax(np.asarray(rand, F32)[j], F32(0)), F32(1 - 2.0 ** -24))
            k0, u1, u2 = (u[:, 0] * F32(2.0 ** 24)).astype(np.uint64), u[:, 1].copy(), u[:, 2].copy()
        hi, lo = np.uint64(total >> 32), np.uint64(total & 0xFFFFFFFF)
        t = ((k0 * hi) << np.uint64(8)) + ((k0 * lo) >> np.uint64(24))
        assert all(int(a) == (int(k) * total) >> 24 for a, k in zip(t[:64], k0[:64]))   # the 88-bit product, in Python ints
        pick = np.searchsorted(cum, t, side="right")   # the first face with cum > t
        v, ok = _tris(vertices, faces, rg)
        v = v[pick]
        assert ok[pick].all()
        flip = u1 + u2 > F32(1)
        u1 = np.where(flip, F32(1) - u1, u1)[:, None]
        u2 = np.where(flip, F32(1) - u2, u2)[:, None]
        points[j] = v[:, 0] + ((v[:, 1] - v[:, 0]) * u1 + (v[:, 2] - v[:, 0]) * u2)
        face[j] = (rg[2] + pick).astype(np.int32)
        c, n2 = _cross(v)
        normals[j] = (c / np.sqrt(n2)[:, None]).astype(F32)
    return dict(points=points, face=face, normals=normals)


# ---------------------------------------------------------------------------------------------------------------- render

def _edge(ax, ay, bx, by, px, py):
    """E_ab at the pixels (px, py: f64 arrays) from f32 endpoints, evaluated from the lexicographically lower one."""
    fwd = ax < bx or (ax == bx and ay <= by)
    ox, oy, tx, ty = (F64(ax), F64(ay), F64(bx), F64(by)) if fwd else (F64(bx), F64(by), F64(ax), F64(ay))
    e = (tx - ox) * (py - oy) - (ty - oy) * (px - ox)
    return e if fwd else -e


def records(vertices, faces, ranges, inst_mesh, inst_xf, inst_label, inst_tri, n_tris, optics):
    """One record per r in [0, n_tris): None (draws nothing), "dropped", or (px [3], py [3], z [3] f32, label, face row)."""
    fx, fy, cx, cy, z_near, _ = (F32(v) for v in optics)
    b, out = len(ranges), []
    tri = np.asarray(inst_tri, dtype=np.int64)
    for r in range(n_tris):
        lo, hi = 0, len(tri)
        while lo < hi:   # the last instance with tri <= r
            mid = lo + (hi - lo) // 2
            lo, hi = (mid + 1, hi) if tri[mid] <= r else (lo, mid)
        inst = lo - 1
        mesh = int(inst_mesh[inst]) if inst >= 0 else -1
        rec = None
        if 0 <= mesh < b:
            vs, vn, fs, fn = ranges[mesh]
            local = r - int(tri[inst])
            if 0 <= local < fn:
                idx = faces[fs + local].astype(np.int64)
                if np.all((idx >= 0) & (idx < vn)):
                    v = vertices[vs + idx]   # [3, 3] f32
                    m = np.asarray(inst_xf[inst], F32).reshape(3, 4)
                    with np.errstate(all="ignore"):
                        cam = [((m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2]) + m[i, 3] for i in range(3)]
                        px = (cam[0] * fx) / cam[2] + cx
                        py = (cam[1] * fy) / cam[2] + cy
                    draw = np.all(cam[2] >= z_near) and np.isfinite(px).all() and np.isfinite(py).all()
                    rec = (px, py, cam[2], int(inst_label[inst]), fs + local) if draw else "dropped"
        out.append(rec)
    return out


def render(vertices, faces, vert_start, vert_count, face_start, face_count, inst_mesh, inst_xf, inst_label, inst_tri, n_tris,
           frame_start, frame_count, h, w, optics, return_cover=False):
    """-> dict(depth [R, h, w] f32, label, face [R, h, w] int32, dropped [R] int32); with return_cover also cover [R, h, w]:
    how many records pass the coverage rule at each pixel (the depth window not applied)."""
    vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    ranges = mesh_ranges(vert_start, vert_count, face_start, face_count, vertices.shape[0], faces.shape[0])
    n_inst, frames = len(inst_mesh), len(frame_start)
    recs = records(vertices, faces, ranges, inst_mesh, inst_xf, inst_label, inst_tri, n_tris, optics) if n_inst else []
    z_near, z_far = F32(optics[4]), F32(optics[5])
    empty = np.uint64(2 ** 64 - 1)
    key = np.full((frames, h, w), empty, np.uint64)
    cover = np.zeros((frames, h, w), np.int32)
    dropped = np.zeros(frames, np.int32)
    for f in range(frames):
        s, c = int(frame_start[f]), int(frame_count[f])
        if s < 0 or c <= 0 or s + c > n_inst or n_tris == 0:
            continue
        lo = int(inst_tri[s])
        hi = int(inst_tri[s + c]) if s + c < n_inst else n_tris
        lo = max(0, min(lo, n_tris))
        hi = max(lo, min(hi, n_tris))
        for r in range(lo, hi):
            rec = recs[r]
            if rec is None:
                continue
            if isinstance(rec, str):
                dropped[f] += 1
                continue
            px, py, z, _, _ = rec
            u0, u1 = int(max(np.ceil(px.min()), 0)), int(min(np.floor(px.max()), w - 1))
            v0, v1 = int(max(np.ceil(py.min()), 0)), int(min(np.floor(py.max()), h - 1))
            if u0 > u1 or v0 > v1:
                continue
            gu, gv = np.meshgrid(np.arange(u0, u1 + 1, dtype=F64), np.arange(v0, v1 + 1, dtype=F64))
            w0 = _edge(px[1], py[1], px[2], py[2], gu, gv)
            w1 = _edge(px[2], py[2], px[0], py[0], gu, gv)
            w2 = _edge(px[0], py[0], px[1], py[1], gu, gv)
            s_ = (w0 + w1) + w2
            inside = (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))) & (s_ != 0)
            cover[f, v0:v1 + 1, u0:u1 + 1] += inside
            with np.errstate(all="ignore"):
                q = ((w0 / F64(z[0]) + w1 / F64(z[1])) + w2 / F64(z[2])) / s_
                zz = (1.0 / q).astype(F32)
            keep = inside & (zz >= z_near) & (zz <= z_far)
            k = (zz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(r)
            view = key[f, v0:v1 + 1, u0:u1 + 1]
            view[keep] = np.minimum(view[keep], k[keep])
    hit = key != empty
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32).view(F32), F32(0)).astype(F32)
    rec_of = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    lab_of = np.array([r[3] if isinstance(r, tuple) else 0 for r in recs] + [0], dtype=np.int32)
    face_of = np.array([r[4] if isinstance(r, tuple) else -1 for r in recs] + [-1], dtype=np.int32)
    rec_of[~hit] = len(recs)
    out = dict(depth=depth, label=lab_of[rec_of], face=face_of[rec_of], dropped=dropped)
    if return_cover:
        out["cover"] = cover
    return out


def render_plan_arrays(mb, plan):
    """The positional arguments of render() from a MeshBatch and pointcloud.render_plan's dict."""
    return (mb.vertices, mb.faces, mb.vert_start, mb.vert_count, mb.face_start, mb.face_count, plan["mesh"], plan["xf"],
            plan["label"], plan["tri"], plan["n_tris"], plan["frame_start"], plan["frame_count"], plan["h"], plan["w"],
            plan["optics"])
