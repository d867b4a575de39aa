"""GPU: from a labelled depth frame to the grasps of every object -- infer_on_scene against infer_on_pointcloud on the
stacked, per-object regularised clouds of the restatement (tests/depth_ref.py), with and without a selection, and the
CLI's --labels_file path against the API.  Model fixture and recipe of tests/test_depth_e2e_gpu.py: 96 x 128, 10 DDIM
steps, 4 grasps, num_points = 1024.  The frame holds a plane and three objects: 70 x 120 px (more than 8192 points: the
round-launch selection), 1600 px (the 26 rows that the first leaves free hold no 40 x 40 square, so 20 x 80: the
one-workgroup selection), 15 x 20 px (fewer than 1024: resampled), and a 3-pixel label that min_object_points drops."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from depth_ref import deproject

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 128
INTR = (400.0, 401.5, 63.25881958, 47.5)


def _scene():
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.0 + 0.0004 * u + 0.0002 * v
    labels = torch.zeros(H, W, dtype=torch.int32)
    labels[2:72, 4:124] = 1
    labels[74:94, 2:82] = 2
    labels[76:91, 90:110] = 3
    labels[94, 120:123] = 4
    bump = 0.03 * torch.sin(u / 9.0) * torch.cos(v / 7.0) + 0.0003 * v
    for k, z in ((1, 0.8), (2, 0.7), (3, 0.75), (4, 0.9)):
        depth = torch.where(labels == k, z + bump, depth)
    depth[0, :5] = 0.0
    depth[50, 60] = float("nan")   # inside object 1
    return depth.contiguous(), labels


def _camera():
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(*INTR, W, H)


@pytest.fixture(scope="module")
def inf(fpc_state_dict):
    from graspldm_amd.inference import InferenceLDM
    from test_modules_cpu import build_fpc
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return InferenceLDM(model=m.cuda().eval(), num_inference_steps=10, device="cuda:0")


@pytest.fixture(scope="module")
def objects():
    depth, labels = _scene()
    cam = _camera()
    objs = [deproject(depth, cam.K, mask=labels == k)[0] for k in (1, 2, 3)]
    assert [o.shape[0] for o in objs] == [70 * 120 - 1, 1600, 300] and objs[0].shape[0] > 8192
    return objs


def _seed(s=4):
    torch.manual_seed(s)
    np.random.seed(s)


def _stack(objects):
    from graspldm_amd.pointcloud import PointCloudHelpers
    return torch.stack([PointCloudHelpers.regularize_pc_point_count(o.cuda(), 1024, True) for o in objects])


def test_infer_on_scene_equals_infer_on_pointcloud_on_the_stacked_restated_clouds(inf, objects):
    depth, labels = _scene()
    cam = _camera()
    _seed()
    inf.infer_on_pointcloud(_stack(objects), num_grasps=4)   # first call of the process: library warm-up
    _seed()
    exp = inf.infer_on_pointcloud(_stack(objects), num_grasps=4)
    _seed()
    got = inf.infer_on_scene(depth.cuda(), cam, labels.cuda(), num_grasps=4, num_points=1024)
    assert got["grasps"].shape == (3, 4, 4, 4)
    for k in ("grasps", "grasp_tmrp", "confidence", "pc"):
        assert torch.equal(got[k], exp[k]), k
    assert got["object_label"].tolist() == [1, 2, 3] and got["object_points"].tolist() == [o.shape[0] for o in objects]
    # scene_rank: every pose, by falling confidence, ties to the lower object, then the lower slot
    conf = got["confidence"].reshape(3, 4).cpu()
    want = sorted(((b, g) for b in range(3) for g in range(4)), key=lambda p: (-float(conf[p]), p[0], p[1]))
    rank = got["scene_rank"]
    assert rank.dtype == torch.int64 and rank.cpu().tolist() == [list(p) for p in want]
    # min_object_points between the sizes drops the smaller objects; num_labels below a label makes it background
    _seed()
    two = inf.infer_on_scene(depth.cuda(), cam, labels.cuda(), num_grasps=4, num_points=1024, min_object_points=1000)
    assert two["object_label"].tolist() == [1, 2] and two["grasps"].shape == (2, 4, 4, 4)
    _seed()
    one = inf.infer_on_scene(depth.cuda(), cam, labels.cuda(), num_grasps=4, num_points=1024, num_labels=1)
    assert one["object_label"].tolist() == [1]


def test_infer_on_scene_takes_the_unlabelled_frame_as_the_scene(inf, objects):
    from graspldm_amd.grasp_select import GraspSelection
    depth, labels = _scene()
    cam = _camera()
    scene, _ = deproject(depth, cam.K)
    assert scene.shape[0] == H * W - 6
    sel = GraspSelection(collision_free=True, top_k=2)
    _seed(6)
    exp = inf.infer_on_pointcloud(_stack(objects), num_grasps=4, selection=sel, scene_pc=scene.cuda())
    _seed(6)
    got = inf.infer_on_scene(depth.cuda(), cam, labels.cuda(), num_grasps=4, num_points=1024, selection=sel)
    assert got["grasps"].shape == (3, 2, 4, 4)
    for k in ("selected_index", "selected_count", "clearance"):
        assert torch.equal(got[k], exp[k]), k
    for k in ("grasps", "confidence"):   # NaN in the slots behind selected_count
        assert torch.equal(got[k].view(torch.int32), exp[k].view(torch.int32)), k
    conf = got["confidence"].reshape(3, 2).cpu()
    live = [(b, g) for b in range(3) for g in range(2) if g < int(got["selected_count"][b])]
    want = sorted(live, key=lambda p: (-float(conf[p]), p[0], p[1]))
    assert got["scene_rank"].cpu().tolist() == [list(p) for p in want]


def test_no_object_of_the_asked_size_raises_before_generation(inf, monkeypatch):
    depth, labels = _scene()

    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    with pytest.raises(ValueError, match="no object has at least 9000 points"):
        inf.infer_on_scene(depth.cuda(), _camera(), labels.cuda(), num_grasps=4, num_points=1024, min_object_points=9000)
    with pytest.raises(ValueError, match="differ in size"):
        inf.infer_on_scene(depth.cuda(), _camera(), labels.cuda(), num_grasps=4)
    with pytest.raises(ValueError, match=r"one frame \[H, W\]"):
        inf.infer_on_scene(depth.cuda().unsqueeze(0), _camera(), labels.cuda().unsqueeze(0), num_grasps=4, num_points=1024)


def test_cli_labels_file_equals_the_api(tmp_path, fpc_state_dict):
    from test_checkpoint import _write_experiment
    from graspldm_amd.camera import Camera
    from graspldm_amd.inference import InferenceLDM
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ema = {k: (v + 0.01 if v.is_floating_point() else v) for k, v in fpc_state_dict.items()}
    _write_experiment(str(tmp_path), "exp_scene", fpc_state_dict, ema)
    depth, labels = _scene()
    np.save(tmp_path / "depth.npy", depth.numpy())
    np.save(tmp_path / "labels.npy", labels.numpy())
    cam_path = str(tmp_path / "cam.json")
    fx, fy, cx, cy = INTR
    with open(cam_path, "w") as f:
        json.dump(dict(cameraMatrix=[[fx, 0, cx], [0, fy, cy], [0, 0, 1]], distCoeffs=[], width=W, height=H, hfov=18.2,
                       vfov=13.6), f)
    out = str(tmp_path / "o.npz")
    res = cli.main(["--exp_path", str(tmp_path / "exp_scene"), "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "10",
                    "--depth_file", str(tmp_path / "depth.npy"), "--camera_json", cam_path, "--labels_file",
                    str(tmp_path / "labels.npy"), "--min_object_points", "200", "--num_points", "1024", "--seed", "5",
                    "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (3, 4, 4, 4)
    _seed(5)   # where the CLI seeds: in front of building the model, whose initialisers draw from the same generator
    api = InferenceLDM(exp_name="exp_scene", exp_out_root=str(tmp_path), num_inference_steps=10, use_fast_sampler=True)
    exp = api.infer_on_scene(depth.cuda(), Camera(cam_path), labels.cuda(), num_grasps=4, num_points=1024,
                             min_object_points=200)
    z = np.load(out)
    for k in ("grasps", "confidence", "object_label", "object_points", "scene_rank"):
        assert np.array_equal(z[k], exp[k].cpu().numpy()), k
    assert z["object_label"].tolist() == [1, 2, 3]
