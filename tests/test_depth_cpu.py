"""CPU: the depth front end without a device -- the torch restatement (tests/depth_ref.py) against the golden captured
from the reference's Camera.depth_to_pointcloud_torch, the envelopes of gldm_depth_to_cloud and
gldm_farthest_points_euclid_large, the Camera model, the depth file reader and the CLI's flag checks."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from depth_ref import deproject

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3


def _cli():
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _camera_json(tmp_path, g=None, **over):
    g = load_golden("depth_cloud.npz") if g is None else g
    data = dict(cameraMatrix=g["K"].tolist(), distCoeffs=[], width=int(g["width"]), height=int(g["height"]), hfov=55.0,
                vfov=42.7)
    data.update(over)
    path = str(tmp_path / "cam.json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path


@pytest.mark.parametrize("name", ["sparse", "full", "empty"])
def test_restatement_equals_the_reference_bit_for_bit(name):
    g = load_golden("depth_cloud.npz")
    pts, pix = deproject(g[f"depth_{name}"], g["K"])
    ref = g[f"points_{name}"]
    assert pts.shape == ref.shape and pts.dtype == torch.float32
    assert torch.equal(pts.view(torch.int32), ref.view(torch.int32))
    w = int(g["width"])
    where = torch.where(g[f"depth_{name}"] > 0)
    assert torch.equal(pix.long(), where[0] * w + where[1])
    assert {"sparse": 0 < pts.shape[0] < 48 * 64, "full": pts.shape[0] == 48 * 64, "empty": pts.shape[0] == 0}[name]


def test_restatement_options():
    """mask, window edges, transform and box act in the contract's order on the restatement itself."""
    g = load_golden("depth_cloud.npz")
    d, K = g["depth_full"], g["K"]
    mask = torch.zeros(48, 64, dtype=torch.uint8)
    mask[5:9, 7:11] = 3
    pts, pix = deproject(d, K, mask=mask)
    assert pts.shape[0] == 16 and pix[0] == 5 * 64 + 7
    lo, hi = float(d[3, 3]), float(d[4, 4])
    lo, hi = min(lo, hi), max(lo, hi)
    _, pix = deproject(d, K, z_range=(lo, hi))
    kept = torch.zeros(48 * 64, dtype=torch.bool)
    kept[pix.long()] = True
    flat = d.reshape(-1)
    assert not kept[flat == lo].any() and kept[flat == hi].all()
    T = [[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 2.0]]
    p0, _ = deproject(d, K)
    p1, _ = deproject(d, K, cam_to_world=T)
    assert torch.equal(p1[:, 2], p0[:, 2] + 2.0) and torch.equal(p1[:, 1], p0[:, 0] - 0.25)


def test_depth_to_cloud_envelope_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    ws = h.gldm_depth_to_cloud_workspace_bytes
    tile = h.gldm_depth_to_cloud_tile_pixels()
    assert tile > 0 and ws(1, 1, 1) == 4 and ws(3, 1, tile + 1) == 3 * 2 * 4 and ws(1, 4096, 4096) == (1 << 24) // tile * 4
    assert ws(1, 4097, 4096) == UNSUPPORTED and ws(1, 1, (1 << 24) + 1) == UNSUPPORTED
    assert ws(0, 4, 4) == INVALID and ws(1, 0, 4) == INVALID and ws(1, 4, -1) == INVALID
    one = ctypes.c_void_p(16)   # a non-null pointer that must never be dereferenced

    def call(depth=one, frames=1, hh=4, ww=4, fx=1.0, fy=1.0, zmin=0.0, zmax=1.0, work=one, nbytes=1 << 20, points=one,
             count=one, lo=None, hi=None):
        return h.gldm_depth_to_cloud(depth, 0, 1.0, None, frames, hh, ww, fx, fy, 0.0, 0.0, zmin, zmax, None, lo, hi, work,
                                     nbytes, points, count, None, None)

    assert call(hh=1, ww=(1 << 24) + 1) == UNSUPPORTED
    assert call(hh=4097, ww=4096) == UNSUPPORTED
    assert call(frames=0) == INVALID and call(hh=0) == INVALID
    assert call(fx=0.0) == INVALID and call(fy=0.0) == INVALID
    assert call(zmin=1.0, zmax=1.0) == INVALID and call(zmin=2.0, zmax=1.0) == INVALID and call(zmax=float("nan")) == INVALID
    assert call(depth=None) == INVALID and call(work=None) == INVALID and call(points=None) == INVALID
    assert call(count=None) == INVALID
    box = (ctypes.c_float * 3)(0, 0, 0)
    assert call(lo=box, hi=None) == INVALID
    assert call(nbytes=3) == -4   # GLDM_ERR_WORKSPACE


def test_fps_large_envelope_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    ws = h.gldm_farthest_points_euclid_large_workspace_bytes
    one = ctypes.c_void_p(16)

    def call(n, m, b=1, points=one, work=one, out=one, nbytes=1 << 40):
        return h.gldm_farthest_points_euclid_large(points, None, b, n, m, work, nbytes, out, None)

    assert call(8192, 4) == UNSUPPORTED and ws(1, 8192) == UNSUPPORTED
    assert call((1 << 22) + 1, 4) == UNSUPPORTED and ws(1, (1 << 22) + 1) == UNSUPPORTED
    assert call(20000, 8193) == UNSUPPORTED
    assert call(5000, 4) == UNSUPPORTED
    assert call(20000, 4, b=0) == INVALID and call(0, 1) == INVALID and call(20000, -1) == INVALID
    assert call(20000, 4, points=None) == INVALID and call(20000, 4, work=None) == INVALID and call(20000, 4, out=None) == INVALID
    assert call(20000, 4, work=ctypes.c_void_p(20)) == INVALID   # not 8-byte aligned
    assert call(20000, 4, nbytes=20000 * 4) == -4
    assert call(20000, 0) == 0   # nothing to select: no launch
    slice_of = h.gldm_farthest_points_euclid_large_slice
    assert slice_of(8193) == slice_of(1 << 19) == 1024 and slice_of((1 << 19) + 1) == 2048 and slice_of(1 << 22) == 8192
    assert slice_of(8192) == UNSUPPORTED
    for n in (8193, 20011, (1 << 19) + 7, 1 << 22):
        slices = -(-n // slice_of(n))
        assert slices <= 512 and ws(2, n) == (2 * n * 4 + 7) // 8 * 8 + 2 * 2 * slices * 8


def test_camera_model(tmp_path):
    from graspldm_amd.camera import Camera
    g = load_golden("depth_cloud.npz")
    cam = Camera(_camera_json(tmp_path, g))
    assert (cam.width, cam.height) == (64, 48) and cam.z_near == 0.05 and cam.z_far == 20
    K = g["K"].numpy()
    assert cam.intrinsics == (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) and cam.xfov == 55.0 and cam.yfov == 42.7
    with pytest.raises(NotImplementedError):
        cam.to_pyrender_camera()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        cam.depth_to_pointcloud_torch(torch.zeros(48, 64))
    c2 = Camera.from_intrinsics(600.0, 601.0, 320.5, 239.5, 640, 480)
    assert c2.intrinsics == (600.0, 601.0, 320.5, 239.5) and (c2.width, c2.height) == (640, 480)
    assert abs(c2.xfov - 2 * np.degrees(np.arctan(640 / 1200.0))) < 1e-9
    with pytest.raises(KeyError):
        Camera(_bad_json(tmp_path))


def _bad_json(tmp_path):
    path = str(tmp_path / "bad.json")
    with open(path, "w") as f:
        json.dump(dict(width=4, height=4), f)
    return path


def test_camera_rejects_a_frame_of_the_wrong_size(tmp_path):
    """The reference's shape asserts come first, in front of the device check."""
    from graspldm_amd.camera import Camera
    cam = Camera(_camera_json(tmp_path))
    with pytest.raises(AssertionError, match="width"):
        cam.depth_to_pointcloud_torch(torch.zeros(48, 63))
    with pytest.raises(AssertionError, match="height"):
        cam.depth_to_pointcloud_torch(torch.zeros(47, 64))


def test_read_depth_file_round_trips(tmp_path):
    from graspldm_amd.pointcloud import read_depth_file
    rng = np.random.RandomState(1)
    d = rng.rand(6, 9).astype(np.float32)
    raw = rng.randint(0, 65535, size=(6, 9)).astype(np.uint16)
    np.save(tmp_path / "d.npy", d)
    np.save(tmp_path / "d64.npy", d.astype(np.float64))
    np.save(tmp_path / "r.npy", raw)
    np.savez(tmp_path / "d.npz", depth=d)
    np.savez(tmp_path / "a.npz", raw)
    for name, want in (("d.npy", d), ("d64.npy", d), ("r.npy", raw), ("d.npz", d), ("a.npz", raw)):
        got = read_depth_file(str(tmp_path / name))
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    np.savez(tmp_path / "x.npz", other=d)
    with pytest.raises(ValueError, match="depth / arr_0"):
        read_depth_file(str(tmp_path / "x.npz"))
    np.save(tmp_path / "v.npy", d.reshape(-1))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        read_depth_file(str(tmp_path / "v.npy"))
    with pytest.raises(ValueError, match="unknown depth format"):
        read_depth_file(str(tmp_path / "d.exr"))


def test_cli_depth_flag_checks():
    cli = _cli()
    a = cli.parse_args(["--exp_path", "x", "--mode", "LDM", "--depth_file", "d.npy", "--camera_json", "c.json", "--mask_file",
                        "m.npy", "--depth_scale", "0.001", "--z_range", "0.2", "1.5", "--crop_box", "0", "0", "0", "1", "1",
                        "1", "--collision_free", "--top_k", "3"])
    assert a.depth_file == "d.npy" and a.z_range == [0.2, 1.5] and a.crop_box == [0, 0, 0, 1, 1, 1] and a.depth_scale == 0.001
    with pytest.raises(SystemExit, match="exclude"):
        cli.main(["--exp_path", "x", "--depth_file", "d.npy", "--camera_json", "c.json", "--pc_file", "a.npy"])
    with pytest.raises(SystemExit, match="exclude"):
        cli.main(["--synthetic", "1024", "--depth_file", "d.npy", "--camera_json", "c.json"])
    with pytest.raises(SystemExit, match="needs --camera_json"):
        cli.main(["--exp_path", "x", "--depth_file", "d.npy"])
    with pytest.raises(SystemExit, match="goes with --depth_file"):
        cli.main(["--exp_path", "x", "--pc_file", "a.npy", "--mask_file", "m.npy"])
    d = cli.parse_args(["--exp_path", "x"])   # without the flags nothing changes
    assert d.depth_file is None and d.camera_json is None and d.crop_box is None
