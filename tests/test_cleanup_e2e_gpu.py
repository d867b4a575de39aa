"""GPU: sensor-cloud cleanup inside the depth entry points.  A 48 x 64 frame of a plane with a bump, and a dirty copy with 25
flying pixels, each farther than max_radius from every other deprojected point: with a CloudCleanup the dirty frame gives
bit for bit the grasps of the clean one (the dirty frame with those pixels set to 0), through infer_on_depth and through
infer_on_scene; without one nothing changes.  Synthetic-recipe weights, as in test_depth_e2e_gpu.py."""
import numpy as np
import pytest
import torch

import cloud_filter_ref as ref
from depth_ref import deproject

pytestmark = pytest.mark.gpu

H, W = 48, 64
INTR = (600.0, 600.0, 31.5, 23.5)
N_FLY = 25


def _camera():
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(*INTR, W, H)


def _frames():
    """(clean, dirty, labels, flying pixel indices): depth [48,64] f32 at about 0.6 m (1 mm between pixels), a two-label
    image (left / right half), 25 flying pixels between 0.25 m and 0.54 m, 12 mm apart in depth."""
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rr = ((u - 30.0) ** 2 + (v - 22.0) ** 2) * 1e-6
    dirty = 0.6 - torch.sqrt(torch.clamp(0.02 ** 2 - rr, min=0.0)) + 0.00002 * u + 0.00001 * v
    rng = np.random.default_rng(9)
    fly = np.sort(rng.choice(H * W, N_FLY, replace=False))
    dirty.view(-1)[torch.from_numpy(fly)] = torch.tensor(0.25 + 0.012 * np.arange(N_FLY), dtype=torch.float32)
    clean = dirty.clone()
    clean.view(-1)[torch.from_numpy(fly)] = 0.0
    labels = torch.where(u < W // 2, 1, 2).to(torch.int32)
    return clean.contiguous(), dirty.contiguous(), labels.contiguous(), fly


@pytest.fixture(scope="module")
def inf(fpc_state_dict):
    from graspldm_amd.inference import InferenceLDM
    from test_modules_cpu import build_fpc
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return InferenceLDM(model=m.cuda().eval(), num_inference_steps=10, device="cuda:0")


@pytest.fixture(scope="module")
def scene():
    """The frames and the preconditions, asserted on the CPU with the restatement before any GPU run."""
    from graspldm_amd.grasp_select import CloudCleanup
    clean, dirty, labels, fly = _frames()
    cleanup = CloudCleanup()
    K = _camera().K
    injected = []
    for lab in (None, 1, 2):
        mask = None if lab is None else (labels == lab).to(torch.uint8)
        cloud, pix = deproject(dirty, K, mask=mask)
        is_fly = np.isin(pix.numpy(), fly)
        nb, _ = ref.neighbor_stats(cloud.numpy(), cleanup.k, cleanup.max_radius)
        assert nb[~is_fly].min() >= cleanup.min_neighbors      # every clean point has enough neighbours ...
        assert nb[is_fly].max() == 0                           # ... and no flying pixel has any
        injected.append(int(is_fly.sum()))
    assert injected[0] == N_FLY == injected[1] + injected[2] and min(injected) > 0
    return dict(clean=clean.cuda(), dirty=dirty.cuda(), labels=labels.cuda(), cleanup=cleanup, injected=injected)


def _seed(s=4):
    torch.manual_seed(s)
    np.random.seed(s)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_infer_on_depth_with_cleanup_equals_the_clean_frame(inf, scene):
    cam = _camera()
    _seed()
    exp = inf.infer_on_depth(scene["clean"], cam, num_grasps=4, num_points=1024)
    _seed()
    got = inf.infer_on_depth(scene["dirty"], cam, num_grasps=4, num_points=1024, cleanup=scene["cleanup"])
    assert got["grasps"].shape == (1, 4, 4, 4)
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(got[k], exp[k]), k
    assert got["object_points_raw"].tolist() == [H * W] and got["object_points"].tolist() == [H * W - N_FLY]
    assert "object_points_raw" not in exp


def test_infer_on_scene_with_cleanup_equals_the_clean_frame(inf, scene):
    cam = _camera()
    _seed(5)
    exp = inf.infer_on_scene(scene["clean"], cam, scene["labels"], num_grasps=4, num_points=1024)
    _seed(5)
    got = inf.infer_on_scene(scene["dirty"], cam, scene["labels"], num_grasps=4, num_points=1024, cleanup=scene["cleanup"])
    assert got["grasps"].shape == (2, 4, 4, 4)
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(got[k], exp[k]), k
    assert torch.equal(got["object_label"], exp["object_label"]) and torch.equal(got["scene_rank"], exp["scene_rank"])
    assert torch.equal(got["object_points"], exp["object_points"])
    assert (got["object_points_raw"] - got["object_points"]).tolist() == scene["injected"][1:]
    assert "object_points_raw" not in exp


def test_flying_pixels_change_the_result_without_cleanup_and_none_is_the_plain_call(inf, scene):
    cam = _camera()
    _seed(6)
    plain = inf.infer_on_depth(scene["dirty"], cam, num_grasps=4, num_points=1024)
    _seed(6)
    none = inf.infer_on_depth(scene["dirty"], cam, num_grasps=4, num_points=1024, cleanup=None)
    assert set(none) == set(plain)
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(none[k], plain[k]), k
    _seed(6)
    clean = inf.infer_on_depth(scene["clean"], cam, num_grasps=4, num_points=1024)
    assert not _bits_equal(plain["pc"], clean["pc"])           # the outliers do reach the encoder when nothing removes them
    _seed(7)
    plain = inf.infer_on_scene(scene["dirty"], cam, scene["labels"], num_grasps=4, num_points=1024)
    _seed(7)
    none = inf.infer_on_scene(scene["dirty"], cam, scene["labels"], num_grasps=4, num_points=1024, cleanup=None)
    assert set(none) == set(plain)
    for k in ("grasps", "confidence", "pc"):
        assert _bits_equal(none[k], plain[k]), k


def test_cleanup_must_be_a_cloud_cleanup_and_an_emptied_cloud_raises(inf, scene, monkeypatch):
    from graspldm_amd.grasp_select import CloudCleanup
    cam = _camera()

    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    with pytest.raises(TypeError, match="CloudCleanup"):
        inf.infer_on_depth(scene["dirty"], cam, num_grasps=4, num_points=1024, cleanup=dict(k=8))
    nothing = CloudCleanup(k=8, max_radius=1e-5, min_neighbors=8)   # no point has 8 neighbours within 10 um
    with pytest.raises(ValueError, match="frame 0"):
        inf.infer_on_depth(scene["dirty"], cam, num_grasps=4, num_points=1024, cleanup=nothing)
    with pytest.raises(ValueError, match="no object has at least"):
        inf.infer_on_scene(scene["dirty"], cam, scene["labels"], num_grasps=4, num_points=1024, cleanup=nothing)
