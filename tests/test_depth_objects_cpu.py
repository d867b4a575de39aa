"""CPU: labelled depth frames without a device -- the restatement (tests/scene_ref.py) on a hand-made frame, the
envelopes of gldm_depth_to_objects and gldm_farthest_points_euclid_ragged through the C ABI, their bytes queries, and
the CLI's --labels_file flag checks."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from depth_ref import deproject
from scene_ref import deproject_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
K3 = [[2.0, 0.0, 2.0], [0.0, 2.0, 1.5], [0.0, 0.0, 1.0]]


def _cli():
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_order_and_counts_on_a_hand_made_frame():
    depth = torch.ones(4, 5)
    depth[0, 0] = 0.0          # dead pixel inside label 2
    depth[3, 4] = float("nan")  # dead pixel inside label 1
    labels = torch.tensor([[2, 2, 0, 1, 1],
                           [2, -3, 0, 1, 4],
                           [3, 3, 3, 0, 1],
                           [0, 2, 5, 1, 1]])
    mask = torch.ones(4, 5, dtype=torch.uint8)
    mask[2, 1] = 0             # masked pixel inside label 3
    pts, pix, start, count = deproject_objects(depth, K3, labels, 4, mask=mask)
    # label 1: pixels 3 4 8 14 18 (19 is NaN); label 2: 1 5 16 (0 is dead); label 3: 10 12 (11 masked); label 4: 9; 5 > K
    assert pix.tolist() == [3, 4, 8, 14, 18, 1, 5, 16, 10, 12, 9]
    assert count == [5, 3, 2, 1] and start == [0, 5, 8, 10]
    whole, whole_pix = deproject(depth, K3)
    lookup = {int(p): whole[i] for i, p in enumerate(whole_pix)}
    assert all(torch.equal(pts[i], lookup[int(p)]) for i, p in enumerate(pix))
    # an absent label keeps its place with count 0
    _, _, start, count = deproject_objects(depth, K3, torch.where(labels == 2, 0, labels), 4, mask=mask)
    assert count == [5, 0, 2, 1] and start == [0, 5, 5, 7]


def test_depth_to_objects_envelope_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    ws = h.gldm_depth_to_objects_workspace_bytes
    tile = h.gldm_depth_to_cloud_tile_pixels()
    assert ws(1, 1, 1, 1) == 4 and ws(3, 1, tile + 1, 5) == 3 * 5 * 2 * 4
    assert ws(1, 4096, 4096, 64) == 64 * ((1 << 24) // tile) * 4
    assert ws(1, 4, 4, 0) == INVALID and ws(1, 4, 4, -2) == INVALID and ws(1, 4, 4, 65) == UNSUPPORTED
    assert ws(0, 4, 4, 2) == INVALID and ws(1, 0, 4, 2) == INVALID
    assert ws(1, 4097, 4096, 2) == UNSUPPORTED and ws(1, 1, (1 << 24) + 1, 2) == UNSUPPORTED
    one = ctypes.c_void_p(16)   # a non-null pointer that must never be dereferenced

    def call(depth=one, labels=one, k=2, frames=1, hh=4, ww=4, fx=1.0, zmin=0.0, zmax=1.0, work=one, nbytes=1 << 20,
             points=one, start=one, count=one):
        return h.gldm_depth_to_objects(depth, 0, 1.0, None, labels, k, frames, hh, ww, fx, 1.0, 0.0, 0.0, zmin, zmax, None,
                                       None, None, work, nbytes, points, start, count, None, None)

    assert call(k=0) == INVALID and call(k=65) == UNSUPPORTED
    assert call(frames=0) == INVALID and call(hh=0) == INVALID
    assert call(hh=1, ww=(1 << 24) + 1) == UNSUPPORTED and call(hh=4097, ww=4096) == UNSUPPORTED
    # the envelope comes before the pointers: null pointers and a shape outside it give the shape's status
    assert h.gldm_depth_to_objects(None, 0, 1.0, None, None, 65, 1, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None, None, None, 0,
                                   None, None, None, None, None) == UNSUPPORTED
    assert h.gldm_depth_to_objects(None, 0, 1.0, None, None, 0, 1, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None, None, None, 0,
                                   None, None, None, None, None) == INVALID
    assert call(fx=0.0) == INVALID and call(zmin=1.0, zmax=1.0) == INVALID
    assert call(depth=None) == INVALID and call(labels=None) == INVALID and call(work=None) == INVALID
    assert call(points=None) == INVALID and call(start=None) == INVALID and call(count=None) == INVALID
    assert call(nbytes=7) == WORKSPACE
    assert h.gldm_abi_version() == 15


def test_fps_ragged_envelope_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    ws = h.gldm_farthest_points_euclid_ragged_workspace_bytes
    large_ws = h.gldm_farthest_points_euclid_large_workspace_bytes
    one = ctypes.c_void_p(16)

    def call(n_max, m, b=1, points=one, start=one, count=one, work=one, out=one, nbytes=1 << 40):
        return h.gldm_farthest_points_euclid_ragged(points, start, count, b, n_max, m, work, nbytes, out, None)

    assert call(20000, 8193) == UNSUPPORTED and call(100, 8193) == UNSUPPORTED
    assert call((1 << 22) + 1, 4) == UNSUPPORTED and ws(1, (1 << 22) + 1) == UNSUPPORTED
    assert call(100, 4, b=65536) == UNSUPPORTED and ws(65536, 100) == UNSUPPORTED
    assert h.gldm_farthest_points_euclid_ragged(None, None, None, 1, 100, 8193, None, 0, None, None) == UNSUPPORTED
    assert h.gldm_farthest_points_euclid_ragged(None, None, None, 1, (1 << 22) + 1, 4, None, 0, None, None) == UNSUPPORTED
    assert call(100, 4, b=0) == INVALID and call(0, 4) == INVALID and call(100, -1) == INVALID
    assert ws(0, 100) == INVALID and ws(1, 0) == INVALID
    assert call(100, 4, points=None) == INVALID and call(100, 4, start=None) == INVALID
    assert call(100, 4, count=None) == INVALID and call(100, 4, out=None) == INVALID
    assert call(20000, 4, work=None) == INVALID and call(20000, 4, work=ctypes.c_void_p(20)) == INVALID
    assert call(20000, 4, nbytes=20000 * 4) == WORKSPACE
    assert call(100, 0) == 0 and call(20000, 0) == 0   # nothing to select: no launch
    # bytes: nothing up to 8192 rows, beyond that what the large entry needs for b clouds of n_max rows
    assert ws(1, 1) == 0 and ws(7, 8192) == 0
    for b, n in ((1, 8193), (3, 20011), (2, 1 << 22)):
        assert ws(b, n) == large_ws(b, n) > 0


def test_python_entry_points_reject_what_the_kernel_cannot_take():
    from graspldm_amd import pointcloud as P
    assert P.MAX_LABELS == 64
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.depth_to_objects(torch.zeros(4, 4), None, torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.regularize_objects(torch.zeros(4, 3), [0], [4], 2)


def test_cli_labels_flag_checks(tmp_path):
    cli = _cli()
    a = cli.parse_args(["--exp_path", "x", "--mode", "LDM", "--depth_file", "d.npy", "--camera_json", "c.json", "--labels_file",
                        "l.npy", "--mask_file", "m.npy", "--min_object_points", "50"])
    assert a.labels_file == "l.npy" and a.mask_file == "m.npy" and a.min_object_points == 50
    with pytest.raises(SystemExit, match="--labels_file goes with --depth_file"):
        cli.main(["--exp_path", "x", "--pc_file", "a.npy", "--labels_file", "l.npy"])
    with pytest.raises(SystemExit, match="--min_object_points goes with --depth_file"):
        cli.main(["--exp_path", "x", "--pc_file", "a.npy", "--min_object_points", "5"])
    with pytest.raises(SystemExit, match="--min_object_points goes with --labels_file"):
        cli.main(["--exp_path", "x", "--depth_file", "d.npy", "--camera_json", "c.json", "--min_object_points", "5"])
    d = cli.parse_args(["--exp_path", "x"])   # without the flags nothing changes
    assert d.labels_file is None and d.min_object_points is None
    lab = np.arange(12, dtype=np.int64).reshape(3, 4)
    np.save(tmp_path / "l.npy", lab)
    np.savez(tmp_path / "l.npz", labels=lab.astype(np.uint8))
    np.savez(tmp_path / "a.npz", lab)
    for name in ("l.npy", "l.npz", "a.npz"):
        got = cli.read_labels_file(str(tmp_path / name))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), lab), name
    np.save(tmp_path / "f.npy", lab.astype(np.float32))
    with pytest.raises(SystemExit, match="integer"):
        cli.read_labels_file(str(tmp_path / "f.npy"))
    np.save(tmp_path / "v.npy", lab.reshape(-1))
    with pytest.raises(SystemExit, match=r"\[H, W\]"):
        cli.read_labels_file(str(tmp_path / "v.npy"))
    np.savez(tmp_path / "x.npz", other=lab)
    with pytest.raises(SystemExit, match="labels / arr_0"):
        cli.read_labels_file(str(tmp_path / "x.npz"))
