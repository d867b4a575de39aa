"""CPU: the host layer of the mesh front end (graspldm_amd/mesh.py, camera.look_at, the envelope of
pointcloud.sample_mesh_surface / render_depth, the C entries' argument checks) and the properties of the numpy restatement
(tests/mesh_ref.py) that the GPU tests then hold the kernels to, bit for bit."""
import ctypes
import re

import numpy as np
import pytest

import mesh_ref as ref
from graspldm_amd import mesh as M
from graspldm_amd.camera import Camera, look_at, views_on_sphere

NEW = ("gldm_mesh_sample_surface", "gldm_mesh_sample_surface_workspace_bytes", "gldm_render_depth",
       "gldm_render_depth_workspace_bytes")


def batch_args(mb):
    return mb.vertices, mb.faces, mb.vert_start, mb.vert_count, mb.face_start, mb.face_count


def camera(w=96, h=64, f=80.0, z_near=0.05, z_far=20.0):
    return Camera.from_intrinsics(f, f, (w - 1) / 2, (h - 1) / 2, w, h, z_near=z_near, z_far=z_far)


# ------------------------------------------------------------------------------------------------------------- loaders

def test_obj_with_quads_slashes_and_negative_indices(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# a unit square and a triangle\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\nv 0.5 0.5 1\nf -1 1//1 2//1\nf 1/1 3/1 -1/1\n")
    m = M.load_mesh(str(p))
    assert m.vertices.shape == (5, 3) and m.vertices.dtype == np.float32
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 2, 4]] and m.faces.dtype == np.int32
    assert np.array_equal(M.load_mesh(str(p), scale=0.5).vertices, m.vertices * np.float32(0.5))
    q = tmp_path / "round.obj"
    M.save_obj(str(q), m)
    back = M.load_mesh(str(q))
    assert back.vertices.tobytes() == m.vertices.tobytes() and np.array_equal(back.faces, m.faces)
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="indices"):
        M.load_mesh(str(bad))


@pytest.mark.parametrize("ascii_", [False, True])
def test_stl_round_trip_merges_vertices_bitwise(tmp_path, ascii_):
    m = M.icosphere(1, 0.3)
    p = tmp_path / "m.stl"
    M.save_stl(str(p), m, ascii=ascii_)
    back = M.load_mesh(str(p))
    assert back.vertices.shape == m.vertices.shape and back.faces.shape == m.faces.shape   # 42 vertices, not 3 * 80
    assert back.vertices[back.faces].tobytes() == m.vertices[m.faces].tobytes()
    # -0.0 and 0.0 are different bit patterns: not merged
    v, f = M.merge_vertices(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32))
    assert v.shape == (4, 3) and f.tolist() == [[0, 1, 2], [3, 1, 2]]


def test_npz_and_unknown_formats(tmp_path):
    m = M.cylinder(0.1, 0.3, 7)
    assert m.vertices.shape == (16, 3) and m.faces.shape == (28, 3)
    p = tmp_path / "m.npz"
    np.savez(str(p), vertices=m.vertices, faces=m.faces)
    back = M.load_mesh(str(p), scale=2.0)
    assert np.array_equal(back.vertices, m.vertices * np.float32(2)) and np.array_equal(back.faces, m.faces)
    np.savez(str(tmp_path / "no.npz"), points=m.vertices)
    with pytest.raises(ValueError, match="vertices"):
        M.load_mesh(str(tmp_path / "no.npz"))
    with pytest.raises(ValueError, match="unknown mesh format"):
        M.load_mesh(str(tmp_path / "m.ply"))


def test_primitives_are_closed_and_outward():
    for m, volume in ((M.box((0.2, 0.3, 0.4)), 0.024), (M.icosphere(3, 0.5), 4 / 3 * np.pi * 0.125),
                      (M.cylinder(0.1, 0.5, 64), np.pi * 0.01 * 0.5)):
        edges = np.concatenate([m.faces[:, [0, 1]], m.faces[:, [1, 2]], m.faces[:, [2, 0]]])
        both = {tuple(e) for e in edges.tolist()}
        assert len(both) == len(edges) and all((b, a) in both for a, b in both)   # every edge once in each direction
        v = m.vertices[m.faces].astype(np.float64)
        signed = np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6
        assert abs(signed - volume) < 0.01 * volume, (signed, volume)
    assert M.icosphere(3).faces.shape == (1280, 3)


def test_meshbatch_layout_and_validation():
    a, b = M.box((1, 1, 1)), M.icosphere(0)
    mb = M.MeshBatch([a, (np.zeros((0, 3)), np.zeros((0, 3))), b])
    assert len(mb) == 3 and mb.vert_start.tolist() == [0, 8, 8] and mb.face_count.tolist() == [12, 0, 20]
    assert mb.faces.max() == 11 and mb.f_max == 20 and mb.faces.dtype == np.int32 and mb.vertices.dtype == np.float32
    assert np.array_equal(mb.mesh(2).faces, b.faces)
    assert M.MeshBatch.of(mb) is mb and len(M.MeshBatch.of(a)) == 1
    with pytest.raises(ValueError, match="indices"):
        M.MeshBatch([(a.vertices, [[0, 1, 8]])])
    with pytest.raises(ValueError, match="indices"):
        M.MeshBatch([(a.vertices, [[0, -1, 2]])])
    with pytest.raises(ValueError, match="finite"):
        M.MeshBatch([(np.array([[0, 0, 0], [1, 0, np.inf], [0, 1, 0]]), [[0, 1, 2]])])
    with pytest.raises(ValueError, match="mesh 1"):
        M.MeshBatch.from_packed(mb.vertices, mb.faces, [0, 8], [8, 3], [0, 12], [12, 20])   # the sphere's faces, 3 vertices
    with pytest.raises(ValueError, match="range"):
        M.MeshBatch.from_packed(mb.vertices, mb.faces, [0], [99], [0], [12])
    with pytest.raises(NotImplementedError, match="2\\^22"):
        M.check_envelope(1, (1 << 22) + 1, 10, (1 << 22) + 1)
    with pytest.raises(NotImplementedError, match="65535"):
        M.check_envelope(65536, 1, 10, 10)
    with pytest.raises(RuntimeError, match="CUDA"):
        mb.on("cpu")


# ------------------------------------------------------------------------------------------------- envelope and the ABI

def test_header_exports_and_binding_agree_and_the_abi_is_15():
    from graspldm_amd import _abi, _lib
    text = open(_abi.HEADER).read()
    assert re.search(r"#define GLDM_ABI_VERSION 15\b", text) and _lib.ABI_VERSION == 15
    h = _lib.lib()
    assert h.gldm_abi_version() == 15
    for name in NEW:
        assert name in _abi.PROTOTYPES and hasattr(h, name), name
    vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _abi.PROTOTYPES["gldm_mesh_sample_surface"] == (i, [vp] * 6 + [i] * 5 + [vp, ctypes.c_ulonglong, vp, ll] + [vp] * 4)
    assert _abi.PROTOTYPES["gldm_render_depth_workspace_bytes"] == (ll, [i] * 8)
    assert _abi.PROTOTYPES["gldm_render_depth"] == (i, [vp] * 6 + [i] * 3 + [vp] * 4 + [i] * 2 + [vp] * 2 + [i] * 3
                                                   + [ctypes.c_float] * 6 + [vp, ll] + [vp] * 5)
    assert list(_abi.STRUCTS) == ["gldm_r1d_resblock", "gldm_r1d_level", "gldm_r1d_desc", "gldm_unet1d_desc"]


def test_c_entries_check_the_envelope_before_any_pointer():
    from graspldm_amd import _lib
    h = _lib.lib()
    inv, uns = -1, -3
    ws = h.gldm_mesh_sample_surface_workspace_bytes
    assert ws(3, 100, 1000, 500, 64) == 16 * 500 + 16 * 3
    for args, st in (((0, 1, 1, 1, 1), inv), ((1, -1, 1, 1, 1), inv), ((1, 1, 1, 1, -1), inv), ((65536, 1, 1, 1, 1), uns),
                     ((1, (1 << 22) + 1, 1, 1, 1), uns), ((1, 1, (1 << 24) + 1, 1, 1), uns), ((1, 1, 1, (1 << 24) + 1, 1), uns),
                     ((1, 1, 1, 1, (1 << 24) + 1), uns), ((32, 1, 1, 1, 1 << 24), uns)):
        assert ws(*args) == st, args
        assert h.gldm_mesh_sample_surface(None, None, None, None, None, None, *args, None, 0, None, 0, None, None, None,
                                          None) == st, args
    assert h.gldm_mesh_sample_surface(*[None] * 6, 1, 1, 3, 1, 8, None, 0, None, 0, None, None, None, None) == inv   # nulls
    rw = h.gldm_render_depth_workspace_bytes
    assert rw(2, 100, 50, 3, 150, 4, 480, 640) == 64 * 150
    good = (1, 8, 12, 1, 12, 1, 48, 64)

    def render(sizes, optics=(50.0, 50.0, 32.0, 24.0, 0.05, 20.0)):
        b, nv, nf, ni, nt, fr, hh, ww = sizes
        return h.gldm_render_depth(*[None] * 6, b, nv, nf, *[None] * 4, ni, nt, None, None, fr, hh, ww, *optics, None, 0,
                                   *[None] * 4, None)

    for at, value, st in ((0, 0, inv), (5, 0, inv), (6, 0, inv), (3, -1, inv), (0, 65536, uns), (1, (1 << 24) + 1, uns),
                          (3, 65536, uns), (4, (1 << 24) + 1, uns), (5, 65536, uns), (6, 1 << 20, uns)):
        sizes = list(good)
        sizes[at] = value
        assert rw(*sizes) == st and render(sizes) == st, (at, value)
    assert rw(1, 8, 12, 1, 12, 1, 4096, 4096) == 64 * 12 and rw(1, 8, 12, 1, 12, 1, 4096, 4097) == uns   # h w <= 2^24
    for optics in ((0.0, 50, 32, 24, 0.05, 20), (50, float("nan"), 32, 24, 0.05, 20), (50, 50, float("inf"), 24, 0.05, 20),
                   (50, 50, 32, 24, 0.0, 20), (50, 50, 32, 24, 1.0, 1.0), (50, 50, 32, 24, 0.05, float("inf")),
                   (50, 50, 32, 24, float("nan"), 20)):
        assert render(good, optics) == inv, optics
    assert render(good) == inv   # a valid shape with null pointers


def test_python_entries_name_the_limit_before_any_hip_call():
    """No GPU is needed: every one of these raises before a tensor or the device is touched."""
    from graspldm_amd import pointcloud as P
    tri = M.Mesh([[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[0, 1, 2]])
    with pytest.raises(NotImplementedError, match="2\\^24 samples"):
        P.sample_mesh_surface(tri, (1 << 24) + 1, seed=0)
    with pytest.raises(NotImplementedError, match="2\\^28"):
        P.sample_mesh_surface([tri] * 32, 1 << 24, seed=0)
    with pytest.raises(ValueError, match="negative"):
        P.sample_mesh_surface(tri, -1, seed=0)
    with pytest.raises(ValueError, match="not both"):
        P.sample_mesh_surface(tri, 4, rand=np.zeros((1, 4, 3)), seed=1)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        import torch
        P.sample_mesh_surface(tri, 4, rand=torch.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="64 unsigned bits"):
        P.sample_mesh_surface(tri, 4, seed=-1)
    pose = np.eye(4)
    with pytest.raises(NotImplementedError, match="2\\^24 pixels"):
        P.render_depth(tri, camera(4097, 4096), pose)
    with pytest.raises(NotImplementedError, match="65535"):
        P.render_depth(tri, camera(8, 8), np.tile(pose, (65536, 1, 1)))
    with pytest.raises(NotImplementedError, match="instances"):
        P.render_depth(tri, camera(8, 8), pose, instances=[[(0, pose, 1)] * 65536])
    big = M.MeshBatch([M.Mesh(np.zeros((3, 3)), np.zeros((1 << 19, 3), np.int64))])
    with pytest.raises(NotImplementedError, match="triangles"):
        P.render_depth(big, camera(8, 8), pose, instances=[[(0, pose, 1)] * 33])
    with pytest.raises(ValueError, match="z_near"):
        P.render_depth(tri, camera(8, 8, z_near=0.0), pose)
    with pytest.raises(ValueError, match="z_near"):
        P.render_depth(tri, camera(8, 8, z_near=2.0, z_far=1.0), pose)
    with pytest.raises(ValueError, match="label"):
        P.render_depth(tri, camera(8, 8), pose, instances=[[(0, pose, 0)]])
    with pytest.raises(ValueError, match="holds 1 meshes"):
        P.render_depth(tri, camera(8, 8), pose, instances=[[(1, pose, 1)]])
    with pytest.raises(ValueError, match="camera poses"):
        P.render_depth(tri, camera(8, 8), np.tile(pose, (2, 1, 1)), instances=[[(0, pose, 1)]] * 3)
    with pytest.raises(ValueError, match="finite"):
        P.render_depth(tri, camera(8, 8), pose * np.nan)
    with pytest.raises(NotImplementedError, match="pyrender"):
        camera().to_pyrender_camera()


def test_render_plan_composes_in_f64_and_lays_out_the_table():
    from graspldm_amd.pointcloud import render_plan
    mb = M.MeshBatch([M.box((1, 1, 1)), M.icosphere(0)])
    poses = views_on_sphere(3, 2.0, rng=np.random.default_rng(0))
    plan = render_plan(mb, camera(), poses, None)
    assert plan["mesh"].tolist() == [0, 0, 0, 1, 1, 1] and plan["tri"].tolist() == [0, 12, 24, 36, 56, 76]
    assert plan["n_tris"] == 96 and plan["frame_start"].tolist() == list(range(6)) and plan["frame_count"].tolist() == [1] * 6
    assert plan["xf"].dtype == np.float32 and np.array_equal(plan["xf"][4], poses[1][:3].astype(np.float32).reshape(12))
    o2w = np.eye(4)
    o2w[:3, 3] = (0.1, 0.2, 0.3)
    plan = render_plan(mb, camera(), poses[0], [[(1, o2w), (0, np.eye(4))], [], [(0, o2w, 7)]])
    assert plan["label"].tolist() == [1, 2, 7] and plan["frame_start"].tolist() == [0, 2, 2]
    assert plan["frame_count"].tolist() == [2, 0, 1] and plan["tri"].tolist() == [0, 20, 32]
    assert plan["xf"][0].tobytes() == (poses[0] @ o2w)[:3].astype(np.float32).tobytes()


# ------------------------------------------------------------------------------------------------------ camera helpers

def test_look_at_is_orthonormal_and_puts_the_target_on_the_axis():
    rng = np.random.default_rng(3)
    cases = [(rng.normal(size=3), rng.normal(size=3), (0, 0, 1)) for _ in range(20)]
    cases += [((0, 0, 2), (0, 0, 0), (0, 0, 1)), ((0, 0, -2), (0, 0, 0), (0, 0, 1))]   # looking along `up`
    for eye, target, up in cases:
        m = look_at(eye, target, up)
        r = m[:3, :3]
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(r) - 1) < 1e-12
        assert np.array_equal(m[3], [0, 0, 0, 1])
        t = m @ np.append(np.asarray(target, float), 1)
        dist = np.linalg.norm(np.asarray(target, float) - np.asarray(eye, float))
        assert np.allclose(t[:3], [0, 0, dist], atol=1e-12)                     # on the optical axis, in front
        assert np.allclose(m @ np.append(np.asarray(eye, float), 1), [0, 0, 0, 1], atol=1e-12)
    m = look_at((0, -2, 0), (0, 0, 0), (0, 0, 1))   # looking along +y with z up: +x stays right, world up is image -y
    assert np.allclose(m[:3, :3] @ [1, 0, 0], [1, 0, 0]) and np.allclose(m[:3, :3] @ [0, 0, 1], [0, -1, 0])
    with pytest.raises(ValueError):
        look_at((1, 1, 1), (1, 1, 1))
    poses = views_on_sphere(16, 0.7, target=(0.1, 0.2, 0.3), rng=np.random.default_rng(1))
    assert poses.shape == (16, 4, 4)
    for m in poses:
        assert np.allclose(m @ [0.1, 0.2, 0.3, 1], [0, 0, 0.7, 1], atol=1e-12)
    assert views_on_sphere(0, 1.0).shape == (0, 4, 4)


# ------------------------------------------------------------------------------------- properties of the restatement

def sliver_mesh():
    """Faces with areas from 1e-6 to 1, one with zero area and one repeated vertex."""
    v = [[0, 0, 0], [1, 0, 0], [0, 2, 0]]
    f = [[0, 1, 2]]
    for k, a in enumerate((1e-6, 1e-4, 1e-2, 0.3)):
        v += [[2 + k, 0, 0], [2 + k + 2 * a, 0, 0], [2 + k, 1, 1]]   # 0.5 * 2a * sqrt(2)
        f.append([3 * k + 3, 3 * k + 4, 3 * k + 5])
    v += [[0, 0, 5], [1, 1, 6], [2, 2, 7]]   # collinear: zero area
    f += [[15, 16, 17], [0, 0, 1]]
    return M.Mesh(v, f)


def test_stratified_u0_picks_every_face_in_proportion():
    for mesh in (sliver_mesh(), M.icosphere(2, 0.4), M.box((0.1, 0.2, 0.7))):
        mb = M.MeshBatch([mesh])
        q = ref.face_weights(mb.vertices, mb.faces, (0, int(mb.vert_count[0]), 0, int(mb.face_count[0])))
        assert q.max() >= 2 ** 39 and q.max() <= 2 ** 40
        for n in (1000, 4096):
            rand = np.zeros((1, n, 3), np.float32)
            rand[0, :, 0] = (np.arange(n) + 0.5) / n
            rand[0, :, 0] = np.floor(rand[0, :, 0] * 2 ** 24) / 2 ** 24
            got = ref.sample_surface(*batch_args(mb), n, rand=rand)
            counts = np.bincount(got["face"][0], minlength=q.size)
            want = n * q.astype(np.float64) / float(q.sum())
            assert np.all(np.abs(counts - want) <= 2), np.abs(counts - want).max()
            assert np.all(counts[q == 0] == 0)


def test_restated_samples_lie_on_their_faces_and_normals_are_unit():
    mb = M.MeshBatch([M.icosphere(1, 0.5), sliver_mesh()])
    got = ref.sample_surface(*batch_args(mb), 500, seed=12345)
    for j in range(2):
        tri = mb.vertices[mb.faces[got["face"][j] - mb.face_start[j]] + mb.vert_start[j]].astype(np.float64)
        p, nrm = got["points"][j].astype(np.float64), got["normals"][j].astype(np.float64)
        scale = np.abs(tri).max()
        assert np.all(np.abs(np.einsum("ij,ij->i", p - tri[:, 0], nrm)) < 8 * 2.0 ** -24 * scale)   # in the face's plane
        assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1) < 4 * 2.0 ** -24)
    # a seed is a pure function; another seed is another draw
    again = ref.sample_surface(*batch_args(mb), 500, seed=12345)
    other = ref.sample_surface(*batch_args(mb), 500, seed=12346)
    assert again["points"].tobytes() == got["points"].tobytes() and other["points"].tobytes() != got["points"].tobytes()


def sphere_scene(w=96, h=64):
    from graspldm_amd.pointcloud import render_plan
    mb = M.MeshBatch([M.icosphere(3, 0.4)])
    cam = camera(w, h, f=70.0)
    plan = render_plan(mb, cam, look_at((0.9, -0.5, 0.6), (0, 0, 0)), None)
    return mb, plan


def test_convex_mesh_is_covered_an_even_number_of_times_and_in_one_run_per_row():
    mb, plan = sphere_scene()
    out = ref.render(*ref.render_plan_arrays(mb, plan), return_cover=True)
    cover, depth = out["cover"][0], out["depth"][0]
    assert out["dropped"].tolist() == [0]
    n_cov = int((cover > 0).sum())
    assert n_cov > 1500                                   # the sphere fills a good part of the 96 x 64 frame
    assert np.all(cover % 2 == 0), np.unique(cover)       # front and back, a shared edge exactly once per side
    assert np.array_equal(cover > 0, depth > 0)
    for row in cover > 0:
        at = np.flatnonzero(row)
        assert at.size == 0 or at[-1] - at[0] + 1 == at.size   # one run: no holes
    # the nearest of the two surfaces: every depth is the distance of the front of the sphere along the pixel's ray
    d = np.linalg.norm([0.9, -0.5, 0.6])
    assert depth[depth > 0].min() > d - 0.4 - 1e-3 and depth[depth > 0].max() < d


# ------------------------------------------------------------------------------------------------------------------ CLI

def _cli():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(root, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_mesh_flags_and_their_exclusions(capsys):
    cli = _cli()
    base = ["--synthetic", "64", "--mode", "LDM"]
    old = cli.parse_args(base)
    assert old.mesh_file is None and all(getattr(old, f) is None for f in cli.MESH_FLAGS)
    a = cli.parse_args(base + ["--mesh_file", "part.obj", "--mesh_scale", "0.001", "--mesh_seed", "3"])
    assert (a.mesh_file, a.mesh_scale, a.mesh_seed, a.mesh_views, a.mesh_view, a.camera_json) == ("part.obj", 0.001, 3, None,
                                                                                                None, None)
    a = cli.parse_args(base + ["--mesh_file", "part.stl", "--mesh_views", "4", "--view_radius", "0.6", "--camera_json", "c.json"])
    assert (a.mesh_views, a.view_radius, a.camera_json) == (4, 0.6, "c.json")
    a = cli.parse_args(base + ["--mesh_file", "part.npz", "--mesh_view", "0.3", "-0.2", "0.4", "--camera_json", "c.json"])
    assert a.mesh_view == [0.3, -0.2, 0.4]
    for argv, words in (
            (["--mesh_scale", "2"], "--mesh_scale goes with --mesh_file"),
            (["--mesh_views", "2"], "--mesh_views goes with --mesh_file"),
            (["--mesh_seed", "2"], "--mesh_seed goes with --mesh_file"),
            (["--mesh_file", "m.obj", "--pc_file", "c.npy"], "exclude each other"),
            (["--mesh_file", "m.obj", "--depth_file", "d.npy", "--camera_json", "c.json"], "exclude each other"),
            (["--mesh_file", "m.obj", "--mesh_views", "2"], "need --camera_json"),
            (["--mesh_file", "m.obj", "--mesh_view", "1", "0", "0"], "need --camera_json"),
            (["--mesh_file", "m.obj", "--camera_json", "c.json"], "--camera_json goes with --mesh_views"),
            (["--mesh_file", "m.obj", "--mesh_views", "2", "--mesh_view", "1", "0", "0", "--camera_json", "c.json"],
             "--mesh_views and --mesh_view exclude"),
            (["--mesh_file", "m.obj", "--view_radius", "1", "--mesh_view", "1", "0", "0", "--camera_json", "c.json"],
             "--view_radius goes with --mesh_views"),
            (["--mesh_file", "m.obj", "--mesh_views", "0", "--camera_json", "c.json"], "at least 1"),
            (["--mesh_file", "m.obj", "--mesh_scale", "0"], "must be positive"),
            (["--mesh_file", "m.obj", "--voxel_size", "0.01"], "excludes --refine_from")):
        with pytest.raises(SystemExit):
            cli.parse_args(base + argv)
        assert words in capsys.readouterr().err, argv
    with pytest.raises(SystemExit, match="--camera_json goes with --depth_file"):   # what it said before, without a mesh
        cli.parse_args(base + ["--camera_json", "c.json"])
