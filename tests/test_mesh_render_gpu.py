"""GPU: gldm_render_depth against the numpy restatement (tests/mesh_ref.py): exact equality of depth, labels, face rows and
the dropped counts.  Every call goes through the C ABI TWICE, each time with the outputs poisoned and the workspace filled
with other garbage, and the two results are compared bitwise.  No tolerance: a pixel is the minimum of integer keys over
triangles whose coverage and depth are restated operation by operation."""
import warnings

import numpy as np
import pytest
import torch

import mesh_ref as ref
from graspldm_amd import mesh as M
from graspldm_amd.camera import look_at
from graspldm_amd.pointcloud import render_plan
from test_mesh_cpu import camera, sphere_scene
from test_mesh_sample_gpu import _garbage, _twice

pytestmark = pytest.mark.gpu

POISON = -7
KEYS = ("depth", "label", "face", "dropped")


def _render(vertices, faces, vs, vc, fs, fc, inst_mesh, inst_xf, inst_label, inst_tri, n_tris, frame_start, frame_count, h, w,
            optics):
    from graspldm_amd import _lib as L
    lib = L.lib()
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).cuda()
    rg = torch.tensor(np.stack([vs, vc, fs, fc]).astype(np.int32)).cuda()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1)).cuda()
    im, il, it, f0, f1 = i32(inst_mesh), i32(inst_label), i32(inst_tri), i32(frame_start), i32(frame_count)
    xf = torch.from_numpy(np.ascontiguousarray(inst_xf, np.float32).reshape(-1, 12)).cuda()
    n_inst, frames = im.numel(), f0.numel()
    sizes = (rg.shape[1], v.shape[0], f.shape[0], n_inst, n_tris, frames, h, w)
    nbytes = lib.gldm_render_depth_workspace_bytes(*sizes)
    assert nbytes == 64 * n_tris
    p = lambda t: L.ptr(t) if t.numel() else None

    def run(k):
        ws = _garbage(nbytes, k)
        assert ws.data_ptr() % 16 == 0
        depth = torch.full((frames, h, w), float("nan"), dtype=torch.float32).cuda()
        label = torch.full((frames, h, w), POISON, dtype=torch.int32).cuda()
        face = torch.full((frames, h, w), POISON, dtype=torch.int32).cuda()
        dropped = torch.full((frames,), POISON, dtype=torch.int32).cuda()
        L.call("gldm_render_depth", p(v), p(f), L.ptr(rg[0]), L.ptr(rg[1]), L.ptr(rg[2]), L.ptr(rg[3]), *sizes[:3], p(im), p(xf),
               p(il), p(it), n_inst, n_tris, L.ptr(f0), L.ptr(f1), frames, h, w, *[float(x) for x in optics],
               L.ptr(ws) if n_tris else None, nbytes, L.ptr(depth), L.ptr(label), L.ptr(face), L.ptr(dropped),
               L.current_stream())
        torch.cuda.synchronize()
        return dict(depth=depth.cpu().numpy(), label=label.cpu().numpy(), face=face.cpu().numpy(),
                    dropped=dropped.cpu().numpy())

    return _twice(run)


def _check(args, exp=None):
    got = _render(*args)
    exp = ref.render(*args) if exp is None else exp
    for key in KEYS:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert got[key].tobytes() == exp[key].tobytes(), key
    assert np.array_equal(got["depth"] > 0, got["label"] > 0) and np.array_equal(got["depth"] > 0, got["face"] >= 0)
    return got


def _scene(meshes, cam, world_to_cam, instances=None):
    mb = M.MeshBatch.of(meshes)
    return ref.render_plan_arrays(mb, render_plan(mb, cam, world_to_cam, instances))


def _shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


TRI = M.Mesh([[-0.3, -0.2, 1.0], [0.35, -0.1, 1.2], [-0.05, 0.3, 0.9]], [[0, 1, 2]])


def test_one_triangle_in_an_8_by_8_frame():
    got = _check(_scene(TRI, camera(8, 8, f=6.0), np.eye(4)))
    n = int((got["depth"] > 0).sum())
    assert 4 <= n <= 16 and got["dropped"].tolist() == [0] and set(np.unique(got["face"])) == {-1, 0}
    assert got["depth"][got["depth"] > 0].min() > 0.9 and got["depth"].max() < 1.2
    # no instance at all, and an instance of a mesh without faces: empty frames, still written
    got = _check(_scene(TRI, camera(8, 8, f=6.0), np.eye(4), instances=[[]]))
    assert not got["depth"].any() and np.all(got["face"] == -1) and not got["label"].any()
    empty = M.MeshBatch([(np.zeros((0, 3)), np.zeros((0, 3)))])
    got = _check(_scene(empty, camera(8, 8, f=6.0), np.eye(4)))
    assert not got["depth"].any()


@pytest.mark.parametrize("size", [(64, 48), (37, 53)])
def test_a_box_also_where_the_frame_is_no_multiple_of_the_tile(size):
    w, h = size
    cam = camera(w, h, f=1.3 * w)
    got = _check(_scene(M.box((0.3, 0.2, 0.25)), cam, look_at((0.5, -0.6, 0.45), (0, 0, 0))))
    assert (got["depth"] > 0).mean() > 0.15 and len(np.unique(got["face"])) == 7   # -1 and three faces, two triangles each
    assert got["depth"][0, 0, 0] == 0 and got["depth"][0, h // 2, w // 2] > 0


def test_the_icosphere_has_no_cracks():
    mb, plan = sphere_scene()
    args = ref.render_plan_arrays(mb, plan)
    exp = ref.render(*args, return_cover=True)
    got = _check(args, exp)
    covered = got["depth"][0] > 0
    assert np.array_equal(covered, exp["cover"][0] > 0) and covered.sum() > 1500
    for row in covered:
        at = np.flatnonzero(row)
        assert at.size == 0 or at[-1] - at[0] + 1 == at.size   # one run per image row


def test_off_screen_behind_the_camera_and_coincident_triangles():
    cam = camera(40, 24, f=30.0)
    # partly off screen: the triangle reaches past the left and the top edge
    got = _check(_scene(TRI, cam, _shift(-0.5, -0.3, 0.0)))
    assert got["depth"][0, 0, 0] > 0 and got["dropped"].tolist() == [0]
    # one vertex behind the near plane, and one triangle wholly behind the camera: dropped whole and counted
    poke = M.Mesh([[-0.3, -0.2, 1.0], [0.35, -0.1, 0.01], [-0.05, 0.3, 0.9], [0, 0, -1], [1, 0, -1], [0, 1, -2]],
                  [[0, 1, 2], [3, 4, 5]])
    got = _check(_scene([TRI, poke], cam, np.eye(4), instances=[[(0, np.eye(4), 1), (1, np.eye(4), 2)], [(1, np.eye(4), 2)]]))
    assert got["dropped"].tolist() == [2, 2] and not got["depth"][1].any() and set(np.unique(got["label"][0])) == {0, 1}
    # two coincident triangles: the lower record wins, whichever mesh or label it carries
    got = _check(_scene([TRI, TRI], cam, np.eye(4), instances=[[(1, np.eye(4), 5), (0, np.eye(4), 3)]]))
    assert set(np.unique(got["label"])) == {0, 5} and set(np.unique(got["face"])) == {-1, 1}
    # outside the depth window: nothing is drawn, nothing is counted
    got = _check(_scene(TRI, camera(40, 24, f=30.0, z_near=0.05, z_far=0.8), np.eye(4)))
    assert not got["depth"].any() and got["dropped"].tolist() == [0]


def test_two_labelled_instances_occlude_each_other():
    cam = camera(64, 48, f=90.0)
    pose = look_at((0, -1.2, 0.5), (0, 0, 0))
    meshes = [M.box((0.3, 0.3, 0.3)), M.cylinder(0.1, 0.5, 24)]
    inst = [[(0, _shift(0.0, 0.25, 0.0), 1), (1, _shift(0.12, -0.15, 0.0), 2)]]   # the cylinder stands in front of the box
    got = _check(_scene(meshes, cam, pose, inst))
    lab = got["label"][0]
    assert (lab == 1).sum() > 100 and (lab == 2).sum() > 100
    assert np.all(got["face"][0][lab == 1] < 12) and np.all(got["face"][0][lab == 2] >= 12)
    alone = _check(_scene(meshes, cam, pose, [[inst[0][0]]]))
    hidden = (alone["label"][0] == 1) & (lab == 2)
    assert hidden.sum() > 50 and np.all(got["depth"][0][hidden] < alone["depth"][0][hidden])   # nearer wins where they overlap


def test_three_frames_with_their_own_instance_ranges_and_a_face_that_leaves_its_mesh():
    cam = camera(37, 53, f=40.0)
    meshes = [M.box((0.2, 0.2, 0.2)), M.icosphere(1, 0.15), M.cylinder(0.08, 0.3, 12)]
    poses = np.stack([look_at(e, (0, 0, 0)) for e in ((0.8, 0.1, 0.3), (-0.2, 0.9, 0.4), (0.1, -0.3, 1.0))])
    inst = [[(0, _shift(0, 0, 0), 1), (1, _shift(0.3, 0, 0), 2), (2, _shift(-0.3, 0, 0), 3)], [(2, _shift(0, 0, 0), 9)],
            [(1, _shift(0, 0.1, 0), 4), (1, _shift(0, -0.25, 0), 4)]]
    args = list(_scene(meshes, cam, poses, inst))
    got = _check(args)
    assert [set(np.unique(l)) for l in got["label"]] == [{0, 1, 2, 3}, {0, 9}, {0, 4}]
    faces = args[1].copy()
    faces[3] = (0, 1, 8)   # the box has 8 vertices: index 8 is the sphere's first -- skipped, not read, not counted
    faces[15] = (-1, 0, 1)
    args[1] = faces
    cut = _check(args)
    assert cut["dropped"].tolist() == [0, 0, 0] and not np.isin(cut["face"], (3, 15)).any() and np.isin(got["face"], (3, 15)).any()
    # frame ranges that leave the table, and first-record offsets that leave the records: empty or cut, never read outside
    args[11], args[12] = np.array([0, 5, -1], np.int32), np.array([3, 2, 1], np.int32)
    cut = _check(args)
    assert not cut["depth"][1:].any() and cut["depth"][0].any()


def test_a_frame_filling_pair_under_a_thousand_small_triangles():
    """More records than one staged chunk in every tile (the pair) and in the tiles the small ones fall into."""
    rng = np.random.default_rng(11)
    w, h = 80, 56
    cam = camera(w, h, f=50.0)
    wall = M.Mesh([[-3, -3, 2], [3, -3, 2], [3, 3, 2], [-3, 3, 2]], [[0, 1, 2], [0, 2, 3]])
    c = np.stack([rng.uniform(-0.9, 0.9, 1000), rng.uniform(-0.6, 0.6, 1000), rng.uniform(0.8, 1.9, 1000)], axis=1)
    v = (c[:, None, :] + rng.uniform(-0.06, 0.06, (1000, 3, 3))).reshape(-1, 3)
    small = M.Mesh(v, np.arange(3000).reshape(-1, 3))
    got = _check(_scene([wall, small], cam, np.eye(4), instances=[[(0, np.eye(4), 1), (1, np.eye(4), 2)]]))
    assert np.all(got["depth"] > 0) and (got["label"] == 2).mean() > 0.2 and (got["label"] == 1).mean() > 0.2
    assert len(np.unique(got["face"][got["label"] == 2])) > 500 and got["depth"][got["label"] == 1].tobytes() == \
        np.full(int((got["label"] == 1).sum()), 2.0, np.float32).tobytes()


def test_deprojecting_a_rendered_box_lands_on_its_surface():
    """render_depth -> depth_to_cloud: every point lies within 64 ulp of its depth of the box's surface."""
    from graspldm_amd.pointcloud import depth_to_cloud, render_depth
    cam = camera(64, 48, f=55.0)
    ext = np.array([0.3, 0.2, 0.25])
    pose = look_at((0.5, -0.6, 0.45), (0, 0, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        depth, label, face = render_depth(M.box(ext), cam, pose, return_labels=True, return_faces=True)
    assert depth.shape == (1, 48, 64) and label.dtype == torch.int32 and int(label.max()) == 1 and int(face.max()) < 12
    pts, pix = depth_to_cloud(depth[0], cam, return_pixels=True)
    assert pts.shape[0] == int((depth > 0).sum()) > 300
    p = pts.cpu().numpy().astype(np.float64)
    obj = (p - pose[:3, 3]) @ pose[:3, :3]                    # R^T (p - t)
    q = np.abs(obj) - ext / 2
    dist = np.where((q > 0).any(axis=1), np.linalg.norm(np.maximum(q, 0), axis=1), -q.max(axis=1))
    assert np.all(dist <= 64 * 2.0 ** -23 * p[:, 2]), (dist / (2.0 ** -23 * p[:, 2])).max()
    # a triangle in front of the near plane: dropped with a warning
    with pytest.warns(RuntimeWarning, match="dropped"):
        d = cam.render_depth(M.box(ext), look_at((0.2, 0, 0), (0, 0, 0)))
    assert d.shape == (1, 48, 64)
