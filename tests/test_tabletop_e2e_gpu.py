"""GPU: from a bare depth frame to the grasps of every object on the table -- fit_table_plane and segment_tabletop against
the restatement (tests/tabletop_ref.py), infer_on_tabletop against infer_on_scene given the restated labels, the
ValueErrors, and the CLI's --segment_tabletop path against the API.  Model fixture and recipe of
tests/test_scene_e2e_gpu.py: 96 x 128, 10 DDIM steps, 4 grasps, num_points = 1024.  The frame: a tilted table with
millimetre noise and 15 % dead pixels, three boxes standing on it (two of them adjacent in the image, 0.1 m apart in
depth), a 3-pixel speck and a far wall."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import tabletop_ref as R
from depth_ref import deproject

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 128
INTR = (400.0, 401.5, 63.25881958, 47.5)
TOL, T = 0.005, 512


def _scene():
    g = np.random.default_rng(42)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 1.0 + 0.0004 * u + 0.0002 * v + g.normal(0.0, 0.001, (H, W))
    d[10:60, 10:50] = 0.85 + g.normal(0.0, 0.0005, (50, 40))
    d[10:60, 50:90] = 0.75 + g.normal(0.0, 0.0005, (50, 40))   # touches the first box in the image, 0.1 m in front of it
    d[68:90, 30:62] = 0.90 + g.normal(0.0, 0.0005, (22, 32))
    d[80, 100:103] = 0.95                                       # a speck
    d[0:4, :] = 3.0                                             # a far wall
    d[g.random((H, W)) < 0.15] = 0.0
    return torch.from_numpy(d.astype(np.float32)).contiguous()


def _camera():
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(*INTR, W, H)


@pytest.fixture(scope="module")
def restated():
    """The restatement, once: cloud, triples, (normal, offset, inliers, hypothesis) and the labels under that plane."""
    depth, cam = _scene(), _camera()
    cloud = deproject(depth, cam.K)[0].numpy()
    triples = np.random.default_rng(0).integers(0, cloud.shape[0], (T, 3))
    fit = R.fit_plane(cloud, triples, TOL, 1e-8)
    seg = R.segment(depth, cam.K, np.append(fit[0], fit[1]), 0.01, 0.5, 0.01, 32, 64)
    assert seg[1] == 3 and fit[2] > 0.4 * cloud.shape[0]
    return dict(cloud=cloud, triples=triples, fit=fit, seg=seg)


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


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return [0 if x == y else (1 if y in (np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))) else 99)
            for x, y in zip(a, b)]


def test_fit_table_plane_equals_the_restatement(restated):
    from graspldm_amd.pointcloud import fit_table_plane
    depth, cam = _scene().cuda(), _camera()
    normal, offset, inl, hyp = restated["fit"]
    raw = fit_table_plane(depth, cam, tol=TOL, hypotheses=T, refit=False)
    e_n, e_o, _, _ = R.fit_plane(restated["cloud"], restated["triples"], TOL, 1e-8, refit=False)
    assert (raw.hypothesis, raw.inliers) == (hyp, inl)
    assert np.array_equal(raw.normal.view(np.int32), e_n.view(np.int32)) and np.float32(raw.offset) == e_o
    got = fit_table_plane(depth, cam, tol=TOL, hypotheses=T)
    assert (got.hypothesis, got.inliers) == (hyp, inl)
    assert max(_ulps(got.normal, normal)) <= 1 and max(_ulps([got.offset], [offset])) <= 1, (got, normal, offset)
    assert got.offset > 0 and got.normal[2] < -0.9   # the camera looks along +z: it sits on the positive side
    # an explicit generator draws the same triples as the default
    same = fit_table_plane(depth, cam, tol=TOL, hypotheses=T, rng=np.random.default_rng(0))
    assert same.hypothesis == got.hypothesis and np.array_equal(same.as_array(), got.as_array())


def test_segment_tabletop_equals_the_restated_labels(restated):
    from graspldm_amd.pointcloud import TablePlane, segment_tabletop
    depth, cam = _scene().cuda(), _camera()
    normal, offset, inl, hyp = restated["fit"]
    e_labels, e_num, e_pixels, e_root = restated["seg"]
    labels, num, plane, pixels, root = segment_tabletop(depth, cam, plane=TablePlane(normal, offset, inl, hyp),
                                                        return_stats=True)
    assert num == e_num == 3 and labels.dtype == torch.int32 and labels.is_cuda
    assert np.array_equal(labels.cpu().numpy(), e_labels)
    assert pixels == e_pixels.tolist() and root == e_root.tolist()
    # the two boxes that touch in the image are two labels; the speck and the wall are background
    lab = labels.cpu().numpy()
    assert set(np.unique(lab[10:60, 10:50])) <= {0, 1, 2} and set(np.unique(lab[10:60, 50:90])) <= {0, 1, 2}
    assert lab[10:60, 10:50].max() != lab[10:60, 50:90].max() and not lab[80, 100:103].any() and not lab[0:4].any()
    # plane=None fits one first: the same labels when the fitted plane is the restated one bit for bit
    labels2, num2, plane2 = segment_tabletop(depth, cam, tol=TOL, hypotheses=T)
    assert num2 == 3 and plane2.hypothesis == hyp
    if np.array_equal(plane2.as_array(), np.append(normal, offset).astype(np.float32)):
        assert torch.equal(labels2, labels)


def test_infer_on_tabletop_equals_infer_on_scene_on_the_restated_labels(inf, restated):
    from graspldm_amd.grasp_select import GraspSelection
    from graspldm_amd.pointcloud import TablePlane
    depth, cam = _scene().cuda(), _camera()
    normal, offset, inl, hyp = restated["fit"]
    plane = TablePlane(normal, offset, inl, hyp)
    e_labels = torch.from_numpy(restated["seg"][0]).cuda()
    for sel, seed in ((None, 4), (GraspSelection(collision_free=True, top_k=2), 6)):
        extra = {} if sel is None else dict(selection=sel)
        _seed(seed)
        exp = inf.infer_on_scene(depth, cam, e_labels, num_grasps=4, num_points=1024, num_labels=3, **extra)
        _seed(seed)
        got = inf.infer_on_tabletop(depth, cam, num_grasps=4, num_points=1024, segmentation=dict(plane=plane), **extra)
        assert got["grasps"].shape == ((3, 4, 4, 4) if sel is None else (3, 2, 4, 4))
        for k, v in exp.items():
            if isinstance(v, torch.Tensor):
                same = torch.equal(got[k].view(torch.int32), v.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(got[k], v)
                assert same, k
        assert torch.equal(got["labels"], e_labels) and got["table_plane"] is plane
        assert got["object_label"].tolist() == [1, 2, 3] and got["object_points"].tolist() == restated["seg"][2][:3].tolist()


def test_value_errors(inf, monkeypatch):
    from graspldm_amd.pointcloud import fit_table_plane, segment_tabletop
    cam = _camera()
    dead = torch.zeros(H, W, device="cuda")
    with pytest.raises(ValueError, match="a plane needs 3"):
        fit_table_plane(dead, cam)
    line = dead.clone()
    line[47, 10:15] = 1.0   # five collinear points
    with pytest.raises(ValueError, match="degenerate"):
        fit_table_plane(line, cam, hypotheses=64)
    with pytest.raises(ValueError, match="hypotheses must be"):
        fit_table_plane(line, cam, hypotheses=4097)
    with pytest.raises(ValueError, match="max_objects"):
        segment_tabletop(line, cam, plane=(0, 0, -1, 1), max_objects=65)
    with pytest.raises(ValueError, match=r"one frame \[H, W\]"):
        segment_tabletop(line.unsqueeze(0), cam, plane=(0, 0, -1, 1))

    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    bare = torch.ones(H, W, device="cuda")   # a table and nothing on it
    with pytest.raises(ValueError, match="no object found"):
        inf.infer_on_tabletop(bare, cam, num_grasps=4, num_points=1024, segmentation=dict(plane=(0, 0, -1, 1)))
    with pytest.raises(ValueError, match=r"one frame \[H, W\]"):
        inf.infer_on_tabletop(bare.unsqueeze(0), cam, num_grasps=4)


def test_cli_segment_tabletop_equals_the_api(tmp_path, fpc_state_dict, restated):
    from test_checkpoint import _write_experiment
    from graspldm_amd.camera import Camera
    from graspldm_amd.inference import InferenceLDM
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ema = {k: (v + 0.01 if v.is_floating_point() else v) for k, v in fpc_state_dict.items()}
    _write_experiment(str(tmp_path), "exp_table", fpc_state_dict, ema)
    depth = _scene()
    np.save(tmp_path / "depth.npy", depth.numpy())
    cam_path = str(tmp_path / "cam.json")
    fx, fy, cx, cy = INTR
    with open(cam_path, "w") as f:
        json.dump(dict(cameraMatrix=[[fx, 0, cx], [0, fy, cy], [0, 0, 1]], distCoeffs=[], width=W, height=H, hfov=18.2,
                       vfov=13.6), f)
    out = str(tmp_path / "o.npz")
    res = cli.main(["--exp_path", str(tmp_path / "exp_table"), "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "10",
                    "--depth_file", str(tmp_path / "depth.npy"), "--camera_json", cam_path, "--segment_tabletop",
                    "--table_tol", str(TOL), "--ransac_hypotheses", str(T), "--segment_seed", "0", "--min_object_pixels", "40",
                    "--num_points", "1024", "--seed", "5", "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (3, 4, 4, 4)
    _seed(5)   # where the CLI seeds: in front of building the model, whose initialisers draw from the same generator
    api = InferenceLDM(exp_name="exp_table", exp_out_root=str(tmp_path), num_inference_steps=10, use_fast_sampler=True)
    exp = api.infer_on_tabletop(depth.cuda(), Camera(cam_path), num_grasps=4, num_points=1024,
                                segmentation=dict(tol=TOL, hypotheses=T, rng=np.random.default_rng(0), min_pixels=40))
    z = np.load(out)
    for k in ("grasps", "confidence", "object_label", "object_points", "scene_rank"):
        assert np.array_equal(z[k], exp[k].cpu().numpy()), k
    assert np.array_equal(z["labels"][0], exp["labels"].cpu().numpy()) and z["labels"].dtype == np.int32
    assert np.array_equal(z["table_plane"][0], exp["table_plane"].as_array())
    assert exp["table_plane"].hypothesis == restated["fit"][3] and z["object_label"].tolist() == [1, 2, 3]
