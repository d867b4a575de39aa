"""CPU: tabletop segmentation without a device -- the restatement (tests/tabletop_ref.py) on a hand-made frame and against
scipy's connected components, the envelopes of gldm_plane_ransac / gldm_plane_moments / gldm_segment_tabletop through the
C ABI with pointers that must never be read, their bytes queries, and the CLI's --segment_tabletop flag checks."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import tabletop_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
K1 = [[100.0, 0.0, 3.5], [0.0, 100.0, 2.5], [0.0, 0.0, 1.0]]
TABLE = (0.0, 0.0, -1.0, 1.0)   # height = 1 - z: the table is the plane z = 1 seen from the origin


def _cli():
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_on_a_hand_made_frame():
    """6 x 8, table at z = 1.  A: 2 x 3 block at z = 0.9 (6 px, root 1).  B: an L of 5 px at z = 0.8 touching A in the image
    (0.1 m behind: not linked at link_dist 0.05).  C: 2 px at z = 0.9.  One pixel at 0.995 is below h_min, one at 0.4 above
    h_max, one NaN inside A."""
    d = np.ones((6, 8), dtype=np.float32)
    d[0:2, 1:4] = 0.9
    d[1, 2] = np.nan
    d[2:5, 1] = 0.8
    d[4, 2:4] = 0.8
    d[3, 6] = d[4, 6] = 0.9
    d[0, 6] = 0.995
    d[5, 7] = 0.4
    want = np.zeros((6, 8), dtype=np.int32)
    want[0:2, 1:4] = 1
    want[1, 2] = 0
    want[2:5, 1] = 1
    want[4, 2:4] = 1
    want[3, 6] = want[4, 6] = 2
    # with a generous link distance A and B are one component of 10 pixels
    labels, num, pixels, root = R.segment(torch.from_numpy(d), K1, TABLE, 0.01, 0.5, 0.2, 2, 4)
    assert num == 2 and np.array_equal(labels, want)
    assert pixels.tolist() == [10, 2, 0, 0] and root.tolist() == [1, 3 * 8 + 6, -1, -1]
    # at 0.05 the depth step separates them: A (5 px, root 1), B (5 px, root 17) tie -> lower root first; C third
    want[2:5, 1] = 2
    want[4, 2:4] = 2
    want[3, 6] = want[4, 6] = 3
    labels, num, pixels, root = R.segment(torch.from_numpy(d), K1, TABLE, 0.01, 0.5, 0.05, 2, 4)
    assert num == 3 and np.array_equal(labels, want)
    assert pixels.tolist() == [5, 5, 2, 0] and root.tolist() == [1, 17, 30, -1]
    # min_pixels drops C, max_labels = 1 keeps only the first of the tie
    labels, num, pixels, root = R.segment(torch.from_numpy(d), K1, TABLE, 0.01, 0.5, 0.05, 3, 1)
    assert num == 1 and np.array_equal(labels, (want == 1).astype(np.int32)) and root.tolist() == [1]


def test_restatement_equals_scipy_components_without_a_distance_rule():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(3)
    fg = g.random((37, 53)) < 0.55
    d = np.where(fg, 0.9, 1.0).astype(np.float32)
    labels, num, pixels, _ = R.segment(torch.from_numpy(d), K1, TABLE, 0.01, 0.5, float("inf"), 1, 64)
    ref, n = ndi.label(fg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    sizes = np.bincount(ref.reshape(-1))[1:]
    assert n > 64 and num == 64
    assert sorted(pixels.tolist(), reverse=True) == pixels.tolist() == sorted(sizes.tolist(), reverse=True)[:64]
    for k in range(1, 65):   # every label is exactly one scipy component, of the recorded size
        inside = np.unique(ref[labels == k])
        assert inside.size == 1 and inside[0] > 0 and (ref == inside[0]).sum() == pixels[k - 1] == (labels == k).sum()
    # unlimited: the partition is the same up to relabelling
    root = R.components(fg, R._links(fg, np.zeros(fg.shape + (3,), np.float32), float("inf"), 1),
                        R._links(fg, np.zeros(fg.shape + (3,), np.float32), float("inf"), 0))
    pairs = {(int(a), int(b)) for a, b in zip(root[fg].reshape(-1), ref[fg].reshape(-1))}
    assert len(pairs) == n == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def test_ransac_restatement_on_known_planes():
    pts = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 1.004], [0.3, 0.2, 2], [2, 0, 1], [0, 0, 1]],
                   dtype=np.float32)
    tri = [[0, 1, 2], [0, 1, 6], [0, 0, 2], [0, 1, 8], [-1, 1, 2], [0, 7, 2], [2, 1, 0]]
    planes, counts = R.ransac(pts, tri, 0.005, 1e-8)
    assert counts.tolist() == [7, -1, -1, -1, -1, -1, 7]   # collinear, repeated, out of range x 2, coincident
    assert planes[0].tolist() == [0.0, 0.0, 1.0, -1.0] and planes[6].tolist() == [0.0, 0.0, -1.0, 1.0]
    assert not planes[1:6].any()
    n, o, inl, hyp = R.fit_plane(pts, tri, 0.005, 1e-8, refit=False)
    assert hyp == 0 and inl == 7 and n.tolist() == [0.0, 0.0, -1.0] and o == 1.0   # the origin has positive height
    s, a = R.moments(pts, planes[0], 0.005)
    assert s[0] == 7 and abs(s[3] - (6 + 1.004)) < 1e-6 and np.all(a >= np.abs(s))


def test_ransac_and_moments_envelopes_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(16)   # a non-null pointer that must never be dereferenced
    tile = h.gldm_plane_ransac_tile_points()
    assert tile > 0 and tile % 64 == 0
    ws = h.gldm_plane_ransac_workspace_bytes
    assert ws(3, 1) == 4 and ws(1 << 24, 4096) == 4096 * 4
    assert ws(0, 1) == INVALID and ws(3, 0) == INVALID and ws((1 << 24) + 1, 1) == UNSUPPORTED and ws(3, 4097) == UNSUPPORTED

    def ransac(n=100, t=8, tol=0.01, mc=1e-8, points=one, tri=one, work=one, nbytes=1 << 20, plane=one, count=one):
        return h.gldm_plane_ransac(points, n, tri, t, tol, mc, work, nbytes, plane, count, None)

    assert ransac(n=0) == INVALID and ransac(t=0) == INVALID and ransac(n=-5) == INVALID
    assert ransac(n=(1 << 24) + 1) == UNSUPPORTED and ransac(t=4097) == UNSUPPORTED
    assert h.gldm_plane_ransac(None, 3, None, 4097, 0.01, 1e-8, None, 0, None, None, None) == UNSUPPORTED
    assert h.gldm_plane_ransac(None, 0, None, 8, 0.01, 1e-8, None, 0, None, None, None) == INVALID
    assert ransac(tol=float("nan")) == INVALID and ransac(mc=float("nan")) == INVALID
    assert ransac(points=None) == INVALID and ransac(tri=None) == INVALID and ransac(work=None) == INVALID
    assert ransac(plane=None) == INVALID and ransac(count=None) == INVALID
    assert ransac(nbytes=8 * 4 - 1) == WORKSPACE

    mws = h.gldm_plane_moments_workspace_bytes
    assert mws(1) == 80 and mws(tile) == 80 and mws(tile + 1) == 160 and mws(1 << 24) == ((1 << 24) // tile) * 80
    assert mws(0) == INVALID and mws((1 << 24) + 1) == UNSUPPORTED
    pl = (ctypes.c_float * 4)(0.0, 0.0, 1.0, -1.0)

    def moments(n=100, tol=0.01, points=one, plane=pl, work=one, nbytes=1 << 20, out=one):
        return h.gldm_plane_moments(points, n, plane, tol, work, nbytes, out, None)

    assert moments(n=0) == INVALID and moments(n=(1 << 24) + 1) == UNSUPPORTED
    assert h.gldm_plane_moments(None, (1 << 24) + 1, None, 0.01, None, 0, None, None) == UNSUPPORTED
    assert moments(tol=float("nan")) == INVALID and moments(points=None) == INVALID and moments(plane=None) == INVALID
    assert moments(work=None) == INVALID and moments(out=None) == INVALID and moments(nbytes=79) == WORKSPACE


def test_segment_tabletop_envelope_without_a_device():
    from graspldm_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(16)
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    assert h.gldm_segment_tile_shape(ctypes.byref(tw), ctypes.byref(th)) == 0 and tw.value >= 1 and th.value >= 1
    assert h.gldm_segment_tile_shape(None, ctypes.byref(th)) == INVALID
    ws = h.gldm_segment_tabletop_workspace_bytes
    assert ws(1, 1) == 24 and ws(480, 640) == 480 * 640 * 16 + 8 and ws(4096, 4096) == (1 << 28) + 8
    assert ws(0, 4) == INVALID and ws(4, 0) == INVALID and ws(4097, 4096) == UNSUPPORTED and ws(1, (1 << 24) + 1) == UNSUPPORTED
    pl = (ctypes.c_float * 4)(0.0, 0.0, -1.0, 1.0)

    def call(depth=one, u16=0, hh=4, ww=4, fx=1.0, zmin=0.0, zmax=1.0, lo=None, hi=None, plane=pl, hmin=0.01, hmax=0.5,
             link=0.01, minpix=1, k=4, work=one, nbytes=1 << 20, labels=one, num=one, pixels=one, root=one):
        return h.gldm_segment_tabletop(depth, u16, 1.0, None, hh, ww, fx, 1.0, 0.0, 0.0, zmin, zmax, None, lo, hi, plane, hmin,
                                       hmax, link, minpix, k, work, nbytes, labels, num, pixels, root, None)

    assert call(hh=0) == INVALID and call(ww=-1) == INVALID
    assert call(hh=4097, ww=4096) == UNSUPPORTED and call(hh=1, ww=(1 << 24) + 1) == UNSUPPORTED
    assert call(minpix=0) == INVALID and call(k=0) == INVALID and call(k=65) == UNSUPPORTED
    # the envelope comes before the pointers: null pointers and a shape outside it give the shape's status
    assert h.gldm_segment_tabletop(None, 0, 1.0, None, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None, None, None, 0.01, 0.5,
                                   0.01, 1, 65, None, 0, None, None, None, None, None) == UNSUPPORTED
    assert h.gldm_segment_tabletop(None, 0, 1.0, None, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None, None, None, 0.01, 0.5,
                                   0.01, 0, 4, None, 0, None, None, None, None, None) == INVALID
    assert call(fx=0.0) == INVALID and call(zmin=1.0, zmax=1.0) == INVALID and call(u16=2) == INVALID
    assert call(hmin=0.5, hmax=0.5) == INVALID and call(hmin=float("nan")) == INVALID
    assert call(link=-0.01) == INVALID and call(link=float("nan")) == INVALID
    bad = (ctypes.c_float * 4)(0.0, float("nan"), -1.0, 1.0)
    assert call(plane=bad) == INVALID and call(plane=None) == INVALID
    box = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    assert call(lo=box) == INVALID and call(hi=box) == INVALID
    assert call(depth=None) == INVALID and call(work=None) == INVALID and call(labels=None) == INVALID
    assert call(num=None) == INVALID and call(pixels=None) == INVALID and call(root=None) == INVALID
    assert call(nbytes=4 * 4 * 16 + 7) == WORKSPACE
    assert h.gldm_abi_version() == 15   # 14 -> 15 added the encoder shape queries: no existing signature changed


def test_python_entry_points_reject_what_the_kernels_cannot_take():
    from graspldm_amd import pointcloud as P
    from graspldm_amd.inference import _InferenceBase
    assert callable(_InferenceBase.infer_on_tabletop) and P.RANSAC_MAX_HYPOTHESES == 4096
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.fit_table_plane(torch.zeros(4, 4), None)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.segment_tabletop(torch.zeros(4, 4), None)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.plane_ransac(torch.zeros(4, 3), [[0, 1, 2]], 0.01)
    # orientation: the camera centre gets positive height; on the plane, the first non-zero component is positive
    n, o = P.orient_plane([0.0, 0.0, 1.0], -1.0, np.zeros(3))
    assert n.tolist() == [0.0, 0.0, -1.0] and o == 1.0
    n, o = P.orient_plane([0.0, -1.0, 0.0], 0.0, np.zeros(3))
    assert n.tolist() == [0.0, 1.0, 0.0] and o == 0.0
    n, o = P.orient_plane([0.0, 0.0, 1.0], -1.0, np.array([0.0, 0.0, 3.0]))
    assert n.tolist() == [0.0, 0.0, 1.0] and o == -1.0
    m = R.moments(np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1.5]], np.float32), (0, 0, 1, -1), 0.01)[0]
    pn, po = P.plane_from_moments(m)
    rn, ro = R.plane_from_moments(m)
    assert np.array_equal(pn, rn) and po == ro and abs(abs(pn[2]) - 1) < 1e-6
    tp = P.TablePlane([0, 0, -1], 1.0, 7, 3)
    assert tp.as_array().tolist() == [0.0, 0.0, -1.0, 1.0] and tp.as_array().dtype == np.float32 and tp.inliers == 7


def test_cli_segment_tabletop_flag_checks():
    cli = _cli()
    base = ["--exp_path", "x", "--mode", "LDM", "--depth_file", "d.npy", "--camera_json", "c.json"]
    a = cli.parse_args(base + ["--segment_tabletop", "--table_tol", "0.004", "--object_height", "0.02", "0.3", "--link_dist",
                               "0.02", "--min_object_pixels", "40", "--ransac_hypotheses", "256", "--segment_seed", "9",
                               "--min_object_points", "50"])
    assert a.segment_tabletop and a.table_tol == 0.004 and a.object_height == [0.02, 0.3] and a.min_object_points == 50
    opts = cli.segmentation_options(a)
    assert {k: v for k, v in opts.items() if k != "rng"} == dict(tol=0.004, height_range=(0.02, 0.3), link_dist=0.02,
                                                                  min_pixels=40, hypotheses=256)
    assert opts["rng"].integers(0, 100, 3).tolist() == np.random.default_rng(9).integers(0, 100, 3).tolist()
    assert cli.segmentation_options(cli.parse_args(base + ["--segment_tabletop"])) == {}
    with pytest.raises(SystemExit, match="excludes --labels_file"):
        cli.main(base + ["--segment_tabletop", "--labels_file", "l.npy"])
    with pytest.raises(SystemExit, match="--segment_tabletop goes with --depth_file"):
        cli.main(["--exp_path", "x", "--pc_file", "a.npy", "--segment_tabletop"])
    with pytest.raises(SystemExit, match="--link_dist goes with --segment_tabletop"):
        cli.main(base + ["--link_dist", "0.02"])
    with pytest.raises(SystemExit, match="--table_tol goes with --segment_tabletop"):
        cli.main(["--exp_path", "x", "--pc_file", "a.npy", "--table_tol", "0.02"])
    d = cli.parse_args(["--exp_path", "x"])   # without the flags nothing changes
    assert not d.segment_tabletop and all(getattr(d, f) is None for f in cli.SEGMENT_FLAGS)
