"""GPU: voxel-grid downsampling inside the entry points, on the 96 x 128 frame, the synthetic-recipe weights and the 10 DDIM
steps of test_depth_e2e_gpu.py.  With a CloudDownsample the depth entry points give bit for bit what infer_on_pointcloud
gives on the restated downsampled cloud (tests/cloud_downsample_ref.py, then tests/cloud_filter_ref.py where a cleanup
follows); without one nothing changes; the CLI's --voxel_size equals the API."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cloud_downsample_ref as ref
import cloud_filter_ref
from depth_ref import deproject
from test_depth_e2e_gpu import H, INTR, ROOT, W, _camera, _scene, _seed

pytestmark = pytest.mark.gpu

VOXEL = 0.004   # the object's pixels lie 2 mm apart: about four of them share a voxel


@pytest.fixture(scope="module")
def inf(fpc_state_dict):
    from graspldm_amd.inference import InferenceLDM
    from test_modules_cpu import build_fpc
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return InferenceLDM(model=m.cuda().eval(), num_inference_steps=10, device="cuda:0")


@pytest.fixture(scope="module")
def restated():
    """The object cloud and its two halves (labels 1 / 2), deprojected, downsampled and -- the halves -- filtered on the CPU,
    once.  The preconditions that make the tests mean something are asserted here."""
    from graspldm_amd.grasp_select import CloudCleanup
    depth, mask = _scene()
    K = _camera().K
    obj, _ = deproject(depth, K, mask=mask)
    down = ref.downsample_cloud(obj.numpy(), VOXEL)
    assert 1024 < down["points"].shape[0] < 8192 < obj.shape[0]     # still above num_points, now below the large selection
    u = torch.arange(W).expand(H, W)
    labels = torch.where(mask.bool(), torch.where(u < 64, 1, 2), 0).to(torch.int32).contiguous()
    cleanup = CloudCleanup(k=8, max_radius=0.006, min_neighbors=4)
    halves = []
    for lab in (1, 2):
        raw, _ = deproject(depth, K, mask=(labels == lab).to(torch.uint8))
        d = ref.downsample_cloud(raw.numpy(), VOXEL)["points"]
        f = cloud_filter_ref.filter_outliers(d, [0], [d.shape[0]], cleanup.k, cleanup.max_radius, cleanup.min_neighbors)
        swapped = cloud_filter_ref.filter_outliers(raw.numpy()[:2048], [0], [2048], cleanup.k, cleanup.max_radius,
                                                   cleanup.min_neighbors)
        assert 1024 < f["out_count"][0] < d.shape[0]                # the filter bites on the downsampled cloud ...
        assert swapped["out_count"][0] == 2048                      # ... and not at raw density: the order matters
        halves.append(dict(raw=raw.shape[0], down=d.shape[0], clean=f["out_points"]))
    return dict(depth=depth, mask=mask, labels=labels, obj=obj, down=down, cleanup=cleanup, halves=halves)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_infer_on_depth_with_downsample_equals_infer_on_pointcloud_on_the_restated_cloud(inf, restated):
    from graspldm_amd.grasp_select import CloudDownsample
    cam = _camera()
    cloud = torch.from_numpy(restated["down"]["points"]).cuda()
    _seed()
    exp = inf.infer_on_pointcloud(cloud, num_grasps=4, num_points=1024)
    _seed()
    got = inf.infer_on_depth(restated["depth"].cuda(), cam, mask=restated["mask"].cuda(), num_grasps=4, num_points=1024,
                             downsample=CloudDownsample(VOXEL))
    assert got["grasps"].shape == (1, 4, 4, 4)
    for k in ("grasps", "grasp_tmrp", "confidence", "pc"):
        assert _bits_equal(got[k], exp[k]), k
    assert got["voxel_size"] == float(np.float32(VOXEL))
    assert got["object_points"].tolist() == [cloud.shape[0]] and got["object_points_raw"].tolist() == [restated["obj"].shape[0]]
    _seed()
    same = inf.infer_on_pointcloud(restated["obj"].cuda(), num_grasps=4, num_points=1024, downsample=CloudDownsample(VOXEL))
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(same[k], exp[k]), k
    assert same["voxel_size"] == got["voxel_size"] and torch.equal(same["object_points"], got["object_points"])


def test_max_points_is_reported_through_infer_on_depth(inf, restated):
    from graspldm_amd.grasp_select import CloudDownsample
    size = VOXEL
    while ref.downsample_cloud(restated["obj"].numpy(), size)["first"].shape[0] > 1500:
        size *= 1.25
    assert size > VOXEL
    cloud = torch.from_numpy(ref.downsample_cloud(restated["obj"].numpy(), size)["points"]).cuda()
    _seed(8)
    exp = inf.infer_on_pointcloud(cloud, num_grasps=4, num_points=1024)
    _seed(8)
    got = inf.infer_on_depth(restated["depth"].cuda(), _camera(), mask=restated["mask"].cuda(), num_grasps=4, num_points=1024,
                             downsample=CloudDownsample(VOXEL, max_points=1500))
    assert got["voxel_size"] == float(np.float32(size)) and got["object_points"].tolist() == [cloud.shape[0]]
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(got[k], exp[k]), k


def test_infer_on_scene_downsamples_first_and_cleans_up_second(inf, restated):
    from graspldm_amd.grasp_select import CloudDownsample
    from graspldm_amd.pointcloud import regularize_objects
    halves = restated["halves"]
    counts = [h["clean"].shape[0] for h in halves]
    packed = torch.from_numpy(np.concatenate([h["clean"] for h in halves])).cuda()
    _seed(5)
    batch = regularize_objects(packed, [0, counts[0]], counts, 1024)
    exp = inf.infer_on_pointcloud(batch, num_grasps=4)
    _seed(5)
    got = inf.infer_on_scene(restated["depth"].cuda(), _camera(), restated["labels"].cuda(), num_grasps=4, num_points=1024,
                             cleanup=restated["cleanup"], downsample=CloudDownsample(VOXEL))
    assert got["grasps"].shape == (2, 4, 4, 4)
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(got[k], exp[k]), k
    assert got["object_label"].tolist() == [1, 2] and got["voxel_size"] == float(np.float32(VOXEL))
    assert got["object_points"].tolist() == counts and got["object_points_raw"].tolist() == [h["raw"] for h in halves]


def test_downsample_none_is_the_plain_call(inf, restated):
    cam = _camera()
    depth, mask, labels = restated["depth"].cuda(), restated["mask"].cuda(), restated["labels"].cuda()
    _seed(6)
    plain = inf.infer_on_depth(depth, cam, mask=mask, num_grasps=4, num_points=1024)
    _seed(6)
    none = inf.infer_on_depth(depth, cam, mask=mask, num_grasps=4, num_points=1024, downsample=None)
    assert set(none) == set(plain) and "voxel_size" not in none and "object_points_raw" not in none
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert _bits_equal(none[k], plain[k]), k
    _seed(7)
    plain = inf.infer_on_scene(depth, cam, labels, num_grasps=4, num_points=1024, cleanup=restated["cleanup"])
    _seed(7)
    none = inf.infer_on_scene(depth, cam, labels, num_grasps=4, num_points=1024, cleanup=restated["cleanup"], downsample=None)
    assert set(none) == set(plain) and "voxel_size" not in none
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert _bits_equal(none[k], plain[k]), k
    assert plain["object_points_raw"].tolist() == [h["raw"] for h in restated["halves"]]   # its meaning with cleanup alone


def test_downsample_must_be_a_cloud_downsample(inf, restated, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    with pytest.raises(TypeError, match="CloudDownsample"):
        inf.infer_on_depth(restated["depth"].cuda(), _camera(), mask=restated["mask"].cuda(), num_grasps=4, num_points=1024,
                           downsample=dict(voxel_size=VOXEL))


def test_cli_voxel_size_equals_the_api(tmp_path, fpc_state_dict, restated):
    from test_checkpoint import _write_experiment
    from graspldm_amd.camera import Camera
    from graspldm_amd.grasp_select import CloudDownsample
    from graspldm_amd.inference import InferenceLDM
    spec = importlib.util.spec_from_file_location("generate_grasps_cli_voxel", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ema = {k: (v + 0.01 if v.is_floating_point() else v) for k, v in fpc_state_dict.items()}
    _write_experiment(str(tmp_path), "exp_voxel", fpc_state_dict, ema)
    depth, mask = restated["depth"], restated["mask"]
    np.save(tmp_path / "depth.npy", depth.numpy())
    np.save(tmp_path / "mask.npy", mask.numpy())
    cam_path = str(tmp_path / "cam.json")
    fx, fy, cx, cy = INTR
    with open(cam_path, "w") as f:
        json.dump(dict(cameraMatrix=[[fx, 0, cx], [0, fy, cy], [0, 0, 1]], distCoeffs=[], width=W, height=H, hfov=18.2,
                       vfov=13.6), f)
    out = str(tmp_path / "o.npz")
    res = cli.main(["--exp_path", str(tmp_path / "exp_voxel"), "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "10",
                    "--depth_file", str(tmp_path / "depth.npy"), "--camera_json", cam_path, "--mask_file",
                    str(tmp_path / "mask.npy"), "--num_points", "1024", "--seed", "5", "--voxel_size", str(VOXEL),
                    "--voxel_max_points", "4000", "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (1, 4, 4, 4)
    _seed(5)   # where the CLI seeds: in front of building the model, whose initialisers draw from the same generator
    api = InferenceLDM(exp_name="exp_voxel", exp_out_root=str(tmp_path), num_inference_steps=10, use_fast_sampler=True)
    exp = api.infer_on_depth(depth.cuda(), Camera(cam_path), mask=mask.cuda(), num_grasps=4, num_points=1024,
                             downsample=CloudDownsample(VOXEL, max_points=4000))
    z = np.load(out)
    assert np.array_equal(z["grasps"], exp["grasps"].cpu().numpy())
    assert np.array_equal(z["confidence"], exp["confidence"].cpu().numpy())
    assert restated["down"]["points"].shape[0] > 4000               # so the voxel grows once: 5 mm
    grown = ref.downsample_cloud(restated["obj"].numpy(), VOXEL * 1.25)["first"].shape[0]
    assert z["voxel_size"].tolist() == [exp["voxel_size"]] == [float(np.float32(VOXEL * 1.25))]
    assert z["object_points"].tolist() == exp["object_points"].tolist() == [grown] and grown <= 4000
    assert z["object_points_raw"].tolist() == [restated["obj"].shape[0]]
