"""GPU: from an object model to grasps -- infer_on_mesh against infer_on_pointcloud on the sampled surface and against
infer_on_depth on the rendered frame (bitwise), a rendered table-and-three-objects scene through segment_tabletop against
the renderer's own ground-truth labels, and the CLI's --mesh_file path.  Model fixture and recipe of
tests/test_tabletop_e2e_gpu.py: 10 DDIM steps, 4 grasps, num_points = 1024."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_ref as ref
import tabletop_ref as R
from graspldm_amd import mesh as M
from graspldm_amd.camera import Camera, look_at

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 96
H_MIN, H_MAX, LINK, MIN_PIXELS = 0.01, 0.5, 0.04, 32


@pytest.fixture(scope="module")
def inf(fpc_state_dict):
    from graspldm_amd.inference import InferenceLDM
    from test_modules_cpu import build_fpc
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return InferenceLDM(model=m.cuda().eval(), num_inference_steps=10, device="cuda:0")


def _seed(s=4):
    torch.manual_seed(s)
    np.random.seed(s)


def _same(got, exp):
    for k, v in exp.items():
        if isinstance(v, torch.Tensor):
            same = torch.equal(got[k].view(torch.int32), v.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(got[k], v)
            assert same, k


def _camera(w=W, h=H, f=110.0):
    return Camera.from_intrinsics(f, f, (w - 1) / 2, (h - 1) / 2, w, h)


def test_infer_on_mesh_is_infer_on_pointcloud_on_the_sampled_surface(inf):
    from graspldm_amd.grasp_select import GraspSelection
    from graspldm_amd.pointcloud import sample_mesh_surface
    mesh = M.cylinder(0.03, 0.12, 32)
    pts, face = sample_mesh_surface(mesh, 1024, seed=7, return_faces=True)
    _seed()
    exp = inf.infer_on_pointcloud(pts[0], num_grasps=4)
    _seed()
    got = inf.infer_on_mesh(mesh, num_grasps=4, seed=7)   # num_points: the encoder's 1024
    assert got["grasps"].shape == (1, 4, 4, 4) and got["cam_pose"] is None
    _same(got, exp)
    assert torch.equal(got["mesh_face"], face) and got["mesh_face"].shape == (1, 1024)
    # every input point lies on the face it is said to come from
    tri = torch.from_numpy(mesh.vertices[mesh.faces]).cuda()[face[0].long()].double()
    nrm = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    off = ((pts[0].double() - tri[:, 0]) * nrm).sum(dim=1).abs() / nrm.norm(dim=1)
    assert float(off.max()) < 1e-7
    # a selection that asks for a scene: the scene is a denser sample of the same surface, drawn with seed + 1
    sel = GraspSelection(collision_free=True, top_k=2)
    scene = sample_mesh_surface(mesh, 8192, seed=8)[0]
    _seed()
    exp = inf.infer_on_pointcloud(pts[0], num_grasps=4, selection=sel, scene_pc=scene)
    _seed()
    got = inf.infer_on_mesh(mesh, num_grasps=4, seed=7, selection=sel)
    assert got["grasps"].shape == (1, 2, 4, 4)
    _same(got, exp)
    with pytest.raises(ValueError, match="needs a camera"):
        inf.infer_on_mesh(mesh, view=2)
    with pytest.raises(ValueError, match="go with a view"):
        inf.infer_on_mesh(mesh, camera=_camera())
    with pytest.raises(TypeError):
        inf.infer_on_mesh(M.MeshBatch([mesh]))


def test_infer_on_mesh_with_a_view_is_infer_on_depth_on_the_rendered_frame(inf):
    from graspldm_amd.pointcloud import render_depth
    mesh, cam = M.box((0.08, 0.05, 0.12)), _camera()
    pose = look_at((0.17, -0.2, 0.14), (0, 0, 0))
    depth, face = render_depth(mesh, cam, pose, return_faces=True)
    assert int((depth > 0).sum()) == 1622   # more than the encoder's 1024: the farthest-point selection runs
    _seed()
    exp = inf.infer_on_depth(depth[0], cam, num_grasps=4, num_points=1024)
    _seed()
    got = inf.infer_on_mesh(mesh, num_grasps=4, view=pose, camera=cam)
    assert got["grasps"].shape == (1, 4, 4, 4)
    _same(got, exp)
    assert np.array_equal(got["cam_pose"].numpy(), pose[None]) and len(got["mesh_face"]) == 1
    assert torch.equal(got["mesh_face"][0], face[0][depth[0] > 0])
    # a number of views: views_on_sphere under the seed, one result per view
    _seed()
    got = inf.infer_on_mesh(mesh, num_grasps=4, view=3, camera=cam, seed=11, view_radius=0.45)
    from graspldm_amd.camera import views_on_sphere
    poses = views_on_sphere(3, 0.45, (0, 0, 0), np.random.default_rng(11))
    assert got["grasps"].shape == (3, 4, 4, 4) and np.array_equal(got["cam_pose"].numpy(), poses)
    _seed()
    _same(got, inf.infer_on_depth(render_depth(mesh, cam, poses), cam, num_grasps=4, num_points=1024))


# --------------------------------------------------------------------------------------------------- the tabletop scene

def _table_scene():
    """A table top at z = 0 and three objects standing on it, seen from above and in front: (MeshBatch, instances, camera,
    pose, the table plane in the camera frame with the camera on its positive side)."""
    def at(x, y, z):
        m = np.eye(4)
        m[:3, 3] = (x, y, z)
        return m
    meshes = M.MeshBatch([M.box((1.2, 1.2, 0.04)), M.box((0.1, 0.1, 0.12)), M.cylinder(0.05, 0.16, 24), M.icosphere(2, 0.06)])
    inst = [[(0, at(0, 0, -0.02), 1), (1, at(-0.25, 0.0, 0.06), 2), (2, at(0.05, 0.1, 0.08), 3), (3, at(0.3, -0.1, 0.06), 4)]]
    pose = look_at((0.0, -0.9, 0.9), (0, 0, 0))
    normal = pose[:3, :3] @ np.array([0.0, 0.0, 1.0])
    plane = np.append(normal, -normal @ pose[:3, 3]).astype(np.float32)
    assert plane[3] > 0
    return meshes, inst, _camera(), pose, plane


def _judge(labels, num, truth, depth, cam, plane):
    """Every segmenter label lies inside exactly one ground-truth object; every object with at least MIN_PIXELS pixels higher
    than H_MIN over the table is found."""
    assert num >= 1
    for k in range(1, num + 1):
        under = np.unique(truth[labels == k])
        assert under.size == 1 and under[0] >= 2, (k, under)
    fx, fy, cx, cy = cam.intrinsics
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = depth.astype(np.float64)
    hgt = plane[0] * (u - cx) * d / fx + plane[1] * (v - cy) * d / fy + plane[2] * d + plane[3]
    found = 0
    for obj in (2, 3, 4):
        tall = (truth == obj) & (hgt > H_MIN + 1e-4)
        if tall.sum() >= MIN_PIXELS:
            assert (labels[truth == obj] > 0).any(), obj
            found += 1
    return found


@pytest.fixture(scope="module")
def table_restated():
    """On the CPU, once: the restated render, and tabletop_ref on it already satisfies what the GPU test asks."""
    from graspldm_amd.pointcloud import render_plan
    meshes, inst, cam, pose, plane = _table_scene()
    out = ref.render(*ref.render_plan_arrays(meshes, render_plan(meshes, cam, pose, inst)))
    depth, truth = out["depth"][0], out["label"][0]
    assert out["dropped"].tolist() == [0] and set(np.unique(truth)) == {0, 1, 2, 3, 4}
    labels, num, pixels, _ = R.segment(torch.from_numpy(depth), cam.K, plane, H_MIN, H_MAX, LINK, MIN_PIXELS, 64)
    assert _judge(labels, num, truth, depth, cam, plane) == 3 and num == 3
    return dict(depth=depth, truth=truth, labels=labels, num=num)


def test_rendered_tabletop_scene_through_the_segmenter(table_restated):
    from graspldm_amd.pointcloud import TablePlane, render_depth, segment_tabletop
    meshes, inst, cam, pose, plane = _table_scene()
    depth, truth, face = render_depth(meshes, cam, pose, instances=inst, return_labels=True, return_faces=True)
    assert depth.cpu().numpy().tobytes() == table_restated["depth"].tobytes()
    assert np.array_equal(truth[0].cpu().numpy(), table_restated["truth"])
    labels, num, _ = segment_tabletop(depth[0], cam, plane=TablePlane(plane[:3], plane[3]), height_range=(H_MIN, H_MAX),
                                      link_dist=LINK, min_pixels=MIN_PIXELS)
    lab = labels.cpu().numpy()
    assert _judge(lab, num, truth[0].cpu().numpy(), depth[0].cpu().numpy(), cam, plane) == 3
    assert num == table_restated["num"] and np.array_equal(lab, table_restated["labels"])
    # the face rows agree with the labels: each instance's faces lie in its mesh's range of the packed array
    f, t = face[0].cpu().numpy(), truth[0].cpu().numpy()
    for k in range(4):
        rows = f[t == k + 1]
        assert rows.size and rows.min() >= meshes.face_start[k] and rows.max() < meshes.face_start[k] + meshes.face_count[k]


def test_cli_mesh_file(tmp_path):
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    path, out = str(tmp_path / "part.obj"), str(tmp_path / "o.npz")
    M.save_obj(path, M.cylinder(30.0, 120.0, 32))   # millimetres
    res = cli.main(["--synthetic", "1024", "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "5", "--mesh_file", path,
                    "--mesh_scale", "0.001", "--mesh_seed", "3", "--seed", "1", "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (1, 4, 4, 4) and bool(torch.isfinite(res[0]["grasps"]).all())
    z = np.load(out)
    assert z["grasps"].shape == (1, 4, 4, 4) and z["mesh_face"].shape == (1, 1024) and z["mesh_face"].min() >= 0
    assert z["mesh_face"].max() < 128 and "cam_pose" not in z.files
    assert float(res[0]["pc"].abs().max()) < 0.07   # the scale was applied: metres
