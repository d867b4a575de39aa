"""CPU: the restatement of the sensor-cloud cleanup (tests/cloud_filter_ref.py) against scipy and numpy, the Python layer's
envelope (every error raised before the library is touched), the CLI flags and the CloudCleanup defaults."""
import os
import sys

import numpy as np
import pytest
import torch

import cloud_filter_ref as ref
import normals_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,k,r", [(700, 8, 0.012), (300, 16, 0.03), (257, 4, 0.006)])
def test_restated_scan_agrees_with_ckdtree(n, k, r):
    spatial = pytest.importorskip("scipy.spatial")
    pc = normals_ref.half_sphere(n, seed=n)
    nb, sc = ref.neighbor_stats(pc, k, r)
    r32 = float(np.sqrt(np.float32(r) * np.float32(r), dtype=np.float32))
    tree = spatial.cKDTree(pc.astype(np.float64))
    dist, _ = tree.query(pc.astype(np.float64), k=k + 1, distance_upper_bound=r32)   # the point itself comes first
    dist = dist[:, 1:]
    live = np.isfinite(dist)
    # tie-free precondition: no f64 distance within rounding of the radius or of the k-th / (k+1)-th boundary
    full = np.sort(np.linalg.norm(pc[None].astype(np.float64) - pc[:, None].astype(np.float64), axis=-1), axis=-1)[:, 1:]
    assert np.abs(full - r32).min() > 1e-6 * r32
    assert np.array_equal(nb, live.sum(-1).astype(np.int32))
    mean = np.where(nb > 0, np.where(live, dist, 0.0).sum(-1) / np.maximum(nb, 1), np.inf)
    has = nb > 0
    assert np.all(np.isinf(sc[~has]))
    assert np.allclose(sc[has].astype(np.float64), mean[has], rtol=4 * np.finfo(np.float32).eps, atol=0.0)


def test_restated_moments_agree_with_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 255, 256, 257, 1000):
        nb = rng.integers(0, 9, n).astype(np.int32)
        sc = np.where(nb > 0, rng.uniform(0.001, 0.01, n), np.inf).astype(np.float32)
        for need in (0, 1, 3):
            valid = nb >= max(need, 1)
            cnt, mu, sigma = ref.cloud_moments(nb, sc, need)
            assert cnt == valid.sum()
            v = sc[valid].astype(np.float64)
            if cnt == 0:
                assert mu == 0.0 and sigma == 0.0
                continue
            assert abs(mu - np.mean(v)) <= 1e-12 * abs(np.mean(v))
            if cnt < 2:
                assert sigma == 0.0
            else:
                assert abs(sigma - np.std(v, ddof=1)) <= 1e-12 * np.std(v, ddof=1)


def test_tree_sum_is_the_documented_order():
    v = np.random.default_rng(0).uniform(0, 1, 256)
    w = [None] * 4
    for q in range(4):
        a = list(v[q * 64:(q + 1) * 64])
        for off in (32, 16, 8, 4, 2, 1):
            a = [a[i] + a[i + off] for i in range(off)]
        w[q] = a[0]
    assert ref.chunk_tree_sum(v) == (w[0] + w[1]) + (w[2] + w[3])


def test_restated_filter_packs_in_row_order():
    pc = np.concatenate([normals_ref.half_sphere(300, seed=1), np.array([[1, 1, 1], [2, 2, 2]], dtype=np.float32)])
    pc = pc[np.random.default_rng(1).permutation(pc.shape[0])]
    out = ref.filter_outliers(pc, [0], [pc.shape[0]], 8, 0.03, 2)
    assert out["out_count"][0] == out["kept"].shape[0] <= 300
    assert np.all(np.diff(out["kept"]) > 0)
    assert np.array_equal(out["out_points"], pc[out["kept"]])
    far = np.nonzero(pc[:, 0] >= 1)[0]
    assert not np.isin(far, out["kept"]).any() and np.all(out["neighbors"][far] == 0) and np.all(np.isinf(out["score"][far]))


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
    for fn in (lambda **kw: P.neighbor_stats(pts, **{"k": 8, "max_radius": 0.01, **kw}),
               lambda **kw: P.remove_outliers(pts, **kw)):
        with pytest.raises(NotImplementedError, match="1 .. 16"):
            fn(k=0)
        with pytest.raises(NotImplementedError, match="1 .. 16"):
            fn(k=17)
        for r in (-1.0, float("nan"), 1e20, float("inf")):
            with pytest.raises(ValueError, match="max_radius"):
                fn(max_radius=r)
        with pytest.raises(ValueError, match="go together"):
            fn(start=[0])
        with pytest.raises(ValueError, match="leave points"):
            fn(start=[4], count=[7])
        with pytest.raises(ValueError, match="leave points"):
            fn(start=[-1], count=[3])
        with pytest.raises(ValueError, match="negative"):
            fn(start=[0], count=[-3])
        with pytest.raises(ValueError, match="overlap"):
            fn(start=[0, 3], count=[4, 4])
        with pytest.raises(ValueError, match="clouds"):
            fn(start=[0, 3], count=[3])
        with pytest.raises(NotImplementedError, match="65535"):
            fn(start=[0] * 65536, count=[0] * 65536)
        with pytest.raises(NotImplementedError, match="65535"):
            fn(start=[], count=[])
    with pytest.raises(ValueError, match="min_neighbors"):
        P.remove_outliers(pts, k=4, min_neighbors=5)
    with pytest.raises(ValueError, match="min_neighbors"):
        P.remove_outliers(pts, min_neighbors=-1)
    with pytest.raises(ValueError, match="std_ratio"):
        P.remove_outliers(pts, std_ratio=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        P.remove_outliers(torch.zeros(10, 2))
    with pytest.raises(ValueError, match=r"\[rows, 3\]"):
        P.remove_outliers(torch.zeros(2, 5, 3), start=[0], count=[2])
    big = torch.zeros(1, 3).expand((1 << 20) + 1, 3)   # no memory behind it
    with pytest.raises(NotImplementedError, match="2\\^20"):
        P.remove_outliers(big, start=[0], count=[(1 << 20) + 1])
    with pytest.raises(NotImplementedError, match="2\\^20"):
        P.neighbor_stats(big, 8, 0.01, start=[0], count=[(1 << 20) + 1])


def test_non_finite_points_inside_a_cloud_raise_gldm_error(no_library):
    from graspldm_amd._lib import GldmError
    P = no_library
    pts = torch.zeros(12, 3)
    pts[5, 1] = float("nan")
    with pytest.raises(GldmError, match="non-finite"):
        P.remove_outliers(pts, start=[0, 6], count=[6, 6])
    with pytest.raises(GldmError, match="non-finite"):
        P.neighbor_stats(pts.reshape(2, 6, 3), 4, 0.1)
    with pytest.raises(AssertionError, match="library was touched"):   # row 5 lies in a gap: the call goes on to the library
        P.remove_outliers(pts, start=[0, 6], count=[5, 6])


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_grasps_cli_cleanup", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        spec.loader.exec_module(cli)
    finally:
        sys.path.pop(0)
    return cli


def test_cli_flags_parse_and_need_a_depth_file():
    from graspldm_amd.grasp_select import CloudCleanup
    cli = _cli()
    base = ["--exp_path", "x", "--depth_file", "d.npy", "--camera_json", "c.json"]
    args = cli.parse_args(base)
    assert not args.remove_outliers and cli.cleanup_options(args) == {}
    args = cli.parse_args(base + ["--remove_outliers"])
    assert cli.cleanup_options(args) == dict(cleanup=CloudCleanup())
    args = cli.parse_args(base + ["--remove_outliers", "--outlier_k", "12", "--outlier_radius", "0.02", "--outlier_min_neighbors",
                                  "5", "--outlier_std_ratio", "2.0", "--clean_scene"])
    assert cli.cleanup_options(args) == dict(cleanup=CloudCleanup(k=12, max_radius=0.02, min_neighbors=5, std_ratio=2.0,
                                                                  apply_to_scene=True))
    with pytest.raises(SystemExit, match="1 .. 16"):
        cli.cleanup_options(cli.parse_args(base + ["--remove_outliers", "--outlier_k", "17"]))
    for flags in (["--remove_outliers"], ["--outlier_k", "4"], ["--outlier_radius", "0.1"], ["--outlier_min_neighbors", "1"],
                  ["--outlier_std_ratio", "1"], ["--clean_scene"]):
        with pytest.raises(SystemExit, match="depth_file"):
            cli.parse_args(["--exp_path", "x", "--synthetic", "1"] + flags)
    for flags in (["--outlier_k", "4"], ["--clean_scene"], ["--outlier_std_ratio", "1"]):
        with pytest.raises(SystemExit, match="remove_outliers"):
            cli.parse_args(base + flags)


def test_cloud_cleanup_defaults_and_validation():
    from graspldm_amd.grasp_select import CloudCleanup
    c = CloudCleanup()
    assert (c.k, c.max_radius, c.min_neighbors, c.std_ratio, c.apply_to_scene) == (8, 0.01, 3, None, False)
    assert c.options == dict(k=8, max_radius=0.01, min_neighbors=3, std_ratio=None)
    for bad in (dict(k=0), dict(k=17), dict(max_radius=-1.0), dict(max_radius=float("nan")), dict(min_neighbors=9),
                dict(min_neighbors=-1), dict(std_ratio=float("nan")), dict(apply_to_scene=1), dict(k=2.0)):
        with pytest.raises(ValueError):
            CloudCleanup(**bad)
