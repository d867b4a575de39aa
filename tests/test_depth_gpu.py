"""GPU: gldm_depth_to_cloud (csrc/depth_cloud.hip) through graspldm_amd.pointcloud.depth_to_cloud against the torch
restatement tests/depth_ref.py, which tests/test_depth_cpu.py pins to the reference.  Everything is bit-exact: points,
counts, order and pixel indices."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from depth_ref import deproject

pytestmark = pytest.mark.gpu

K = [[61.537128448486328, 0.0, 31.025881958], [0.0, 61.3391, 23.774318695], [0.0, 0.0, 1.0]]


def _cam(h, w, k=K):
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(k[0][0], k[1][1], k[0][2], k[1][2], w, h)


def _frame(h, w, seed, holes=0.3):
    g = torch.Generator().manual_seed(seed)
    d = 0.3 + 1.2 * torch.rand(h, w, generator=g)
    d[torch.rand(h, w, generator=g) < holes] = 0.0
    return d


def _same(got, exp):
    return got.shape == exp.shape and got.dtype == exp.dtype and torch.equal(
        got.cpu().contiguous().view(torch.int32), exp.contiguous().view(torch.int32))


def _check(depth, cam, **kw):
    from graspldm_amd.pointcloud import depth_to_cloud
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    pts, pix = depth_to_cloud(depth.cuda(), cam, return_pixels=True, **dev)
    exp_pts, exp_pix = deproject(depth, cam.K, **kw)
    assert _same(pts, exp_pts), (pts.shape, exp_pts.shape)
    assert pix.dtype == torch.int32 and torch.equal(pix.cpu(), exp_pix)
    return pts


def _tile():
    from graspldm_amd.pointcloud import depth_tile_pixels
    return depth_tile_pixels()


def test_pixel_counts_around_the_tile_size():
    t = _tile()
    for h, w in ((1, 1), (7, 9), (1, t - 1), (1, t), (1, t + 1), (1, 3 * t + 37)):
        for holes in (0.3, 0.0):
            n = _check(_frame(h, w, seed=h * 131 + w, holes=holes), _cam(h, w)).shape[0]
            assert holes > 0 or n == h * w
    # more than three tiles as a frame with rows (u and v both move), H*W no multiple of the tile
    h, w = 3 * t // 61 + 2, 61
    assert h * w > 3 * t and (h * w) % t != 0
    _check(_frame(h, w, seed=5), _cam(h, w))


def test_three_frames_in_one_call_full_sparse_empty():
    from graspldm_amd.pointcloud import depth_to_cloud
    from graspldm_amd import _lib as L
    t = _tile()
    h, w = 3, t + 5
    frames = torch.stack([_frame(h, w, 1, holes=0.0), _frame(h, w, 2, holes=0.9), torch.zeros(h, w)])
    cam = _cam(h, w)
    clouds, pixels = depth_to_cloud(frames.cuda(), cam, return_pixels=True)
    assert [c.shape[0] for c in clouds][0] == h * w and clouds[2].shape[0] == 0
    for f in range(3):
        exp_pts, exp_pix = deproject(frames[f], cam.K)
        assert _same(clouds[f], exp_pts) and torch.equal(pixels[f].cpu(), exp_pix)
    # a frame alone equals the same frame at position 1 of 3
    alone = depth_to_cloud(frames[1].cuda(), cam)
    assert _same(alone, clouds[1].cpu())
    # rows past count[f] are not written, nothing at all for the empty frame: call the entry on poisoned buffers
    lib = L.lib()
    d = frames.cuda()
    nbytes = lib.gldm_depth_to_cloud_workspace_bytes(3, h, w)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    pts = torch.full((3, h * w, 3), -77.0, device="cuda")
    pix = torch.full((3, h * w), -5, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    fx, fy, cx, cy = cam.intrinsics
    L.call("gldm_depth_to_cloud", L.ptr(d), 0, 1.0, None, 3, h, w, fx, fy, cx, cy, 0.0, 3.4028234663852886e38, None, None, None,
           L.ptr(ws), nbytes, L.ptr(pts), L.ptr(cnt), L.ptr(pix), L.current_stream())
    c = cnt.tolist()
    assert c == [x.shape[0] for x in clouds] and c[2] == 0
    for f in range(3):
        assert bool((pts[f, c[f]:] == -77.0).all()) and bool((pix[f, c[f]:] == -5).all())
        assert _same(pts[f, :c[f]], clouds[f].cpu())


def test_bad_depth_values_are_dropped():
    d = _frame(7, 9, 3, holes=0.0)
    d[0, 0], d[1, 1], d[2, 2], d[3, 3], d[4, 4] = float("nan"), float("inf"), -float("inf"), -0.5, 0.0
    d[6, 8] = -0.0
    pts = _check(d, _cam(7, 9))
    assert pts.shape[0] == 63 - 6 and bool(torch.isfinite(pts).all())


def test_u16_path_equals_f32_path_on_the_same_metres():
    from graspldm_amd.pointcloud import depth_to_cloud
    t = _tile()
    h, w = 5, t // 4 + 3
    g = torch.Generator().manual_seed(9)
    raw = torch.randint(0, 4000, (h, w), generator=g).to(torch.int32)
    raw[torch.rand(h, w, generator=g) < 0.2] = 0
    raw[0, 1] = 65535
    metres = raw.to(torch.float32) * torch.tensor(0.001, dtype=torch.float32)
    cam = _cam(h, w)
    u16 = torch.from_numpy(raw.numpy().astype(np.uint16))
    a, pa = depth_to_cloud(u16.cuda(), cam, depth_scale=0.001, return_pixels=True)
    b, pb = depth_to_cloud(metres.cuda(), cam, return_pixels=True)
    assert _same(a, b.cpu()) and torch.equal(pa, pb)
    exp, _ = deproject(raw, cam.K, depth_scale=0.001)
    assert _same(a, exp)
    as_i16 = torch.from_numpy(raw.numpy().astype(np.uint16).view(np.int16))   # the same bits where uint16 is unavailable
    assert _same(depth_to_cloud(as_i16.cuda(), cam, depth_scale=0.001), exp)
    with pytest.raises(ValueError, match="depth_scale"):
        depth_to_cloud(u16.cuda(), cam)


def test_mask_alone():
    d = _frame(48, 64, 4)
    mask = torch.zeros(48, 64, dtype=torch.uint8)
    mask[10:30, 20:50] = 255
    mask[40, 3] = 1
    _check(d, _cam(48, 64), mask=mask)
    _check(d, _cam(48, 64), mask=mask.bool())


def test_window_edges_on_exact_pixel_values():
    d = _frame(48, 64, 6)
    lo, hi = 0.5, 1.25
    d[5, 5], d[5, 6], d[6, 5], d[6, 6] = lo, hi, float(np.nextafter(np.float32(lo), np.float32(2))), float(
        np.nextafter(np.float32(hi), np.float32(2)))
    from graspldm_amd.pointcloud import depth_to_cloud
    cam = _cam(48, 64)
    _check(d, cam, z_range=(lo, hi))
    _, pix = depth_to_cloud(d.cuda(), cam, z_range=(lo, hi), return_pixels=True)
    kept = set(pix.tolist())
    assert 5 * 64 + 5 not in kept and 5 * 64 + 6 in kept and 6 * 64 + 5 in kept and 6 * 64 + 6 not in kept


def test_transform_and_box_with_points_on_a_face():
    d = _frame(48, 64, 7, holes=0.1)
    cam = _cam(48, 64)
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    T = [[c, -s, 0.0, 0.11], [s, c, 0.0, -0.07], [0.0, 0.0, 1.0, 0.5]]
    free, _ = deproject(d, cam.K, cam_to_world=T)
    # box faces through coordinates that points really have: those points lie exactly on a face and are kept
    order = free[:, 0].sort().values
    lo = (float(order[len(order) // 4]), float(free[:, 1].min()), float(free[:, 2].sort().values[10]))
    hi = (float(order[3 * len(order) // 4]), float(free[:, 1].max()), float(free[:, 2].max()))
    pts = _check(d, cam, cam_to_world=T, crop_box=(lo, hi))
    assert 0 < pts.shape[0] < free.shape[0]
    assert bool((pts[:, 0] == lo[0]).any()) and bool((pts[:, 0] == hi[0]).any()) and bool((pts[:, 2] == lo[2]).any())
    T4 = torch.tensor(T + [[0.0, 0.0, 0.0, 1.0]])
    from graspldm_amd.pointcloud import depth_to_cloud
    assert _same(depth_to_cloud(d.cuda(), cam, cam_to_world=T4.cuda(), crop_box=(lo, hi)), pts.cpu())
    _check(d, cam, cam_to_world=T)
    _check(d, cam, crop_box=((-0.2, -0.2, 0.4), (0.2, 0.2, 1.0)))


def test_camera_method_equals_the_reference_golden(tmp_path):
    from graspldm_amd.camera import Camera
    g = load_golden("depth_cloud.npz")
    path = str(tmp_path / "cam.json")
    with open(path, "w") as f:
        json.dump(dict(cameraMatrix=g["K"].tolist(), distCoeffs=[], width=64, height=48, hfov=55.0, vfov=42.7), f)
    cam = Camera(path)
    for name in ("sparse", "full", "empty"):
        depth = g[f"depth_{name}"].cuda()
        assert _same(cam.depth_to_pointcloud_torch(depth), g[f"points_{name}"]), name
    depth = g["depth_sparse"]
    rgb = torch.randint(0, 255, (48, 64, 3), generator=torch.Generator().manual_seed(1)).to(torch.uint8)
    pc, col = cam.depth_to_pointcloud_torch(depth.cuda(), rgb.cuda())
    where = torch.where(depth > 0)
    assert torch.equal(col.cpu(), rgb[where[0], where[1], :]) and _same(pc, g["points_sparse"])


def test_two_calls_are_bitwise_equal():
    from graspldm_amd.pointcloud import depth_to_cloud
    t = _tile()
    d = torch.stack([_frame(9, t // 2 + 1, s) for s in (11, 12)]).cuda()
    cam = _cam(9, t // 2 + 1)
    a = depth_to_cloud(d, cam)
    b = depth_to_cloud(d, cam)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
