"""GPU: from a depth frame to grasps -- infer_on_depth against infer_on_pointcloud on the restatement's cloud
(tests/depth_ref.py), with and without a selection, and the CLI's --depth_file path against the API.  Synthetic-recipe
weights, a 96 x 128 frame of a box on a plane whose 9120 object pixels put the large farthest-point selection on the path."""
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
    """depth [96,128] f32 (a tilted plane at about 1 m, a bumpy box 0.2 m in front of it, a few dead pixels), mask."""
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.0 + 0.0004 * u + 0.0002 * v
    mask = torch.zeros(H, W, dtype=torch.uint8)
    mask[8:88, 8:122] = 1
    box = 0.8 + 0.03 * torch.sin(u / 9.0) * torch.cos(v / 7.0) + 0.0003 * v
    depth = torch.where(mask.bool(), box, depth)
    depth[0, :5] = 0.0
    depth[50, 60] = float("nan")
    return depth.contiguous(), mask


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


def _seed(s=4):
    torch.manual_seed(s)
    np.random.seed(s)


def test_infer_on_depth_equals_infer_on_pointcloud_on_the_restated_cloud(inf):
    depth, mask = _scene()
    cam = _camera()
    obj, _ = deproject(depth, cam.K, mask=mask)
    assert 8192 < obj.shape[0] == 80 * 114 - 1
    _seed()
    inf.infer_on_pointcloud(obj.cuda(), num_grasps=4, num_points=1024)   # first call of the process: library warm-up
    _seed()
    exp = inf.infer_on_pointcloud(obj.cuda(), num_grasps=4, num_points=1024)
    _seed()
    got = inf.infer_on_depth(depth.cuda(), cam, mask=mask.cuda(), num_grasps=4, num_points=1024)
    assert got["grasps"].shape == (1, 4, 4, 4)
    for k in ("grasps", "grasp_tmrp", "confidence", "pc"):
        assert torch.equal(got[k], exp[k]), k


def test_infer_on_depth_takes_the_unmasked_frame_as_the_scene(inf):
    from graspldm_amd.grasp_select import GraspSelection
    depth, mask = _scene()
    cam = _camera()
    obj, _ = deproject(depth, cam.K, mask=mask)
    scene, _ = deproject(depth, cam.K)
    assert scene.shape[0] == H * W - 6
    sel = GraspSelection(collision_free=True, top_k=2)
    _seed(6)
    exp = inf.infer_on_pointcloud(obj.cuda(), num_grasps=4, num_points=1024, selection=sel, scene_pc=scene.cuda())
    _seed(6)
    got = inf.infer_on_depth(depth.cuda(), cam, mask=mask.cuda(), num_grasps=4, num_points=1024, selection=sel)
    assert got["grasps"].shape == (1, 2, 4, 4)
    for k in ("selected_index", "selected_count", "clearance"):
        assert torch.equal(got[k], exp[k]), k
    for k in ("grasps", "confidence"):   # NaN in the slots behind selected_count
        assert torch.equal(got[k].view(torch.int32), exp[k].view(torch.int32)), k


def test_an_empty_object_cloud_raises_before_generation(inf, monkeypatch):
    depth, mask = _scene()

    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    monkeypatch.setattr(inf, "prepare_pointcloud", boom)
    with pytest.raises(ValueError, match="frame 0"):
        inf.infer_on_depth(depth.cuda(), _camera(), mask=torch.zeros_like(mask).cuda(), num_grasps=4, num_points=1024)
    both = torch.stack([depth, depth]).cuda()
    masks = torch.stack([mask, torch.zeros_like(mask)]).cuda()
    with pytest.raises(ValueError, match="frame 1"):
        inf.infer_on_depth(both, _camera(), mask=masks, num_grasps=4, num_points=1024)


def test_cli_depth_file_equals_the_api(tmp_path, fpc_state_dict):
    from test_checkpoint import _write_experiment
    from graspldm_amd.camera import Camera
    from graspldm_amd.inference import InferenceLDM
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ema = {k: (v + 0.01 if v.is_floating_point() else v) for k, v in fpc_state_dict.items()}
    _write_experiment(str(tmp_path), "exp_depth", fpc_state_dict, ema)
    depth, mask = _scene()
    np.save(tmp_path / "depth.npy", depth.numpy())
    np.save(tmp_path / "mask.npy", mask.numpy())
    cam_path = str(tmp_path / "cam.json")
    fx, fy, cx, cy = INTR
    with open(cam_path, "w") as f:
        json.dump(dict(cameraMatrix=[[fx, 0, cx], [0, fy, cy], [0, 0, 1]], distCoeffs=[], width=W, height=H, hfov=18.2,
                       vfov=13.6), f)
    out = str(tmp_path / "o.npz")
    res = cli.main(["--exp_path", str(tmp_path / "exp_depth"), "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "10",
                    "--depth_file", str(tmp_path / "depth.npy"), "--camera_json", cam_path, "--mask_file",
                    str(tmp_path / "mask.npy"), "--num_points", "1024", "--seed", "5", "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (1, 4, 4, 4)
    _seed(5)   # where the CLI seeds: in front of building the model, whose initialisers draw from the same generator
    api = InferenceLDM(exp_name="exp_depth", exp_out_root=str(tmp_path), num_inference_steps=10, use_fast_sampler=True)
    exp = api.infer_on_depth(depth.cuda(), Camera(cam_path), mask=mask.cuda(), num_grasps=4, num_points=1024)
    z = np.load(out)
    assert np.array_equal(z["grasps"], exp["grasps"].cpu().numpy())
    assert np.array_equal(z["confidence"], exp["confidence"].cpu().numpy())
