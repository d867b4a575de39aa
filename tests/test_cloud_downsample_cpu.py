"""CPU: the restatement of the voxel-grid downsampling (tests/cloud_downsample_ref.py) against an independent formulation,
the cell-face lattice, the CloudDownsample dataclass, the Python layer's envelope (every error raised before the library is
touched), the CLI flags and the header."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import cloud_downsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def face_lattice():
    """Points exactly on cell faces: p = k * v for v = 0.5, k = -4 .. 4 per axis (exact in f32), each twice -> [1458, 3]."""
    k = np.arange(-4, 5, dtype=np.float32)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * np.float32(0.5)
    return np.concatenate([g, g[::-1]]).astype(np.float32)


@pytest.mark.parametrize("n,v,seed", [(2000, 0.004, 0), (777, 0.01, 1), (300, 0.002, 2)])
def test_restatement_agrees_with_the_plain_f64_mean(n, v, seed):
    rng = np.random.default_rng(seed)
    pc = (rng.uniform(-0.05, 0.05, (n, 3)) + np.array([0.1, -0.2, 0.6])).astype(np.float32)
    got = ref.downsample_cloud(pc, v)
    v32 = np.float64(np.float32(v))
    p64 = pc.astype(np.float64)
    cell = np.floor(p64 / v32).astype(np.int64)
    seen, means, firsts, members = {}, [], [], []
    for i, c in enumerate(map(tuple, cell)):   # independent: a dict in order of first appearance, plain f64 means
        if c not in seen:
            seen[c] = len(means)
            means.append([])
            firsts.append(i)
        means[seen[c]].append(p64[i])
    members = np.array([len(m) for m in means], dtype=np.int32)
    mean = np.array([np.mean(m, axis=0) for m in means])
    assert 1 < len(means) < n and members.max() > 1
    assert np.array_equal(got["first"], np.array(firsts, dtype=np.int32))
    assert np.array_equal(got["members"], members)
    assert np.array_equal(got["voxel"], np.array([seen[tuple(c)] for c in cell], dtype=np.int32))
    # the bar is derived: every point moves by at most half a quantum (v * 2^-16; a whole one bounds mean and f64 noise
    # generously), then the centroid is rounded to f32 once
    bar = v32 * 2.0 ** -16 + np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got["points"].astype(np.float64) - mean) <= bar)
    assert got["members"].sum() == n and np.all(np.diff(got["first"]) > 0)


def test_points_on_cell_faces_land_by_floor_not_truncation():
    pc = face_lattice()
    cell, q = ref.quantise(pc, 0.5)
    k = np.rint(pc / 0.5).astype(np.int64)
    assert np.array_equal(cell, k)                      # p = k v lies in cell k, for negative k too (truncation: k + 1)
    assert np.array_equal(q, k * 65536)
    d = ref.downsample_cloud(pc, 0.5)
    assert d["points"].shape == (729, 3) and np.all(d["members"] == 2)
    assert np.array_equal(d["points"], pc[:729])        # both members of a voxel are the same point: the centroid is exact
    just_below = np.nextafter(np.float32(-1.0), np.float32(-2.0))
    assert ref.quantise(np.array([[just_below, -0.0, 0.0]], np.float32), 0.5)[0].tolist() == [[-3, 0, 0]]


def test_cloud_downsample_defaults_and_validation():
    from graspldm_amd.grasp_select import CloudDownsample
    c = CloudDownsample()
    assert (c.voxel_size, c.max_points, c.apply_to_scene) == (0.003, None, False)
    assert c.options == dict(voxel_size=0.003, max_points=None)
    assert CloudDownsample(0.005, 2048, True).options == dict(voxel_size=0.005, max_points=2048)
    with pytest.raises(Exception):
        c.voxel_size = 1.0   # frozen
    for bad in (dict(voxel_size=0.0), dict(voxel_size=-0.001), dict(voxel_size=float("inf")), dict(voxel_size=float("nan")),
                dict(voxel_size="3mm"), dict(voxel_size=True), dict(max_points=0), dict(max_points=-5), dict(max_points=10.0),
                dict(max_points=True), dict(apply_to_scene=1)):
        with pytest.raises(ValueError):
            CloudDownsample(**bad)


@pytest.fixture
def no_library(monkeypatch):
    """The Python layer with CPU tensors let through and every door to the library shut."""
    from graspldm_amd import _lib, pointcloud

    def shut(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("lib", "call", "workspace", "current_stream"):
        monkeypatch.setattr(_lib, name, shut)
    monkeypatch.setattr(pointcloud, "_need_cuda", lambda *a, **k: None)
    return pointcloud


def test_envelope_errors_come_before_the_library(no_library):
    P = no_library
    pts = torch.zeros(10, 3)
    for v in (0.0, -1.0, float("inf"), float("nan"), 1e-50, 1e39, None, "x"):
        with pytest.raises(ValueError, match="voxel_size"):
            P.voxel_downsample(pts, v)
    fn = lambda **kw: P.voxel_downsample(pts, 0.01, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="go together"):
        fn(start=[0])
    with pytest.raises(ValueError, match="leave points"):
        fn(start=[4], count=[7])
    with pytest.raises(ValueError, match="negative"):
        fn(start=[0], count=[-3])
    with pytest.raises(ValueError, match="overlap"):
        fn(start=[0, 3], count=[4, 4])
    with pytest.raises(NotImplementedError, match="65535"):
        fn(start=[0] * 65536, count=[0] * 65536)
    with pytest.raises(ValueError, match="shape"):
        P.voxel_downsample(torch.zeros(10, 2), 0.01)
    big = torch.zeros(1, 3).expand((1 << 22) + 1, 3)   # no memory behind it
    with pytest.raises(NotImplementedError, match=r"gldm_voxel_downsample takes at most 2\^22"):
        P.voxel_downsample(big, 0.01, start=[0], count=[(1 << 22) + 1])
    big = torch.zeros(1, 3).expand((1 << 24) + 1, 3)
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        P.voxel_downsample(big, 0.01, start=[0], count=[5])
    with pytest.raises(AssertionError, match="library was touched"):   # inside the envelope the call goes on
        fn()


def test_non_finite_and_out_of_range_points_raise_before_the_library(no_library):
    from graspldm_amd._lib import GldmError
    P = no_library
    pts = torch.zeros(12, 3)
    pts[5, 1] = float("nan")
    with pytest.raises(GldmError, match="non-finite"):
        P.voxel_downsample(pts, 0.01, start=[0, 6], count=[6, 6])
    with pytest.raises(GldmError, match="non-finite"):
        P.voxel_downsample(pts.reshape(2, 6, 3), 0.01)
    with pytest.raises(AssertionError, match="library was touched"):   # row 5 lies in a gap
        P.voxel_downsample(pts, 0.01, start=[0, 6], count=[5, 6])
    far = torch.zeros(12, 3)
    far[7, 2] = -float(1 << 19)   # |p| / v = 2^20 exactly at v = 0.5: the first value outside
    with pytest.raises(ValueError, match=r"2\^20"):
        P.voxel_downsample(far, 0.5)
    with pytest.raises(ValueError, match=r"2\^20"):
        P.voxel_downsample(far, 0.5, start=[0, 6], count=[6, 6])
    with pytest.raises(AssertionError, match="library was touched"):   # row 7 lies in a gap
        P.voxel_downsample(far, 0.5, start=[0, 8], count=[7, 4])
    far[7, 2] = np.nextafter(np.float32(-(1 << 19)), np.float32(0.0)).item()
    with pytest.raises(AssertionError, match="library was touched"):   # the last value inside
        P.voxel_downsample(far, 0.5)


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_grasps_cli_downsample", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        spec.loader.exec_module(cli)
    finally:
        sys.path.pop(0)
    return cli


def test_cli_flags_parse_and_their_exclusions():
    from graspldm_amd.grasp_select import CloudDownsample
    cli = _cli()
    depth = ["--exp_path", "x", "--depth_file", "d.npy", "--camera_json", "c.json"]
    cloud = ["--exp_path", "x", "--pc_file", "c.npy", "--num_points", "1024"]
    for base in (depth, cloud):
        assert cli.downsample_options(cli.parse_args(base)) == {}
        args = cli.parse_args(base + ["--voxel_size", "0.004"])
        assert cli.downsample_options(args) == dict(downsample=CloudDownsample(voxel_size=0.004))
        args = cli.parse_args(base + ["--voxel_size", "0.002", "--voxel_max_points", "4096", "--downsample_scene"])
        assert cli.downsample_options(args) == dict(downsample=CloudDownsample(0.002, 4096, True))
    for argv in (["--exp_path", "x", "--synthetic", "1", "--voxel_size", "0.003"],          # neither kind of input
                 ["--exp_path", "x", "--pc_file", "c.npy", "--voxel_size", "0.003"],        # --pc_file without --num_points
                 depth + ["--voxel_max_points", "100"], depth + ["--downsample_scene"],     # companions without --voxel_size
                 cloud + ["--downsample_scene"],
                 depth + ["--voxel_size", "0"], depth + ["--voxel_size", "-0.01"], depth + ["--voxel_size", "inf"],
                 depth + ["--voxel_size", "0.003", "--voxel_max_points", "0"]):
        with pytest.raises(SystemExit) as e:   # argparse's error: exit status 2
            cli.parse_args(argv)
        assert e.value.code == 2, argv


def test_header_declares_the_entry_and_the_abi_stays_15():
    from graspldm_amd import _abi
    protos, _, consts = _abi.parse(open(os.path.join(ROOT, "include", "gldm.h")).read())
    assert consts["GLDM_ABI_VERSION"] == 15
    import ctypes
    ret, args = protos["gldm_voxel_downsample"]
    assert ret is ctypes.c_int and len(args) == 16 and args[6] is ctypes.c_float and args[3:6] == [ctypes.c_int] * 3
    ret, args = protos["gldm_voxel_downsample_workspace_bytes"]
    assert ret is ctypes.c_longlong and args == [ctypes.c_int] * 3
    text = open(os.path.join(ROOT, "include", "gldm.h")).read()
    section = text[text.index("voxel-grid downsampling"):text.index("gldm_voxel_downsample_workspace_bytes(int b")]
    assert re.search(r"anchored at the ORIGIN, not at the cloud's min bound as in Open3D", section)
    src = open(os.path.join(ROOT, "graspldm_amd", "csrc", "Makefile")).read()
    strict = re.search(r"^SRCS_STRICT := (.*)$", src, re.M).group(1).split()
    assert "cloud_downsample.hip" in strict
