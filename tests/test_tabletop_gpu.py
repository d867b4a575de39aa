"""GPU: gldm_plane_ransac, gldm_plane_moments and gldm_segment_tabletop (csrc/tabletop.hip) against the restatement
tests/tabletop_ref.py.  Every case runs the C entry on poisoned outputs and a garbage workspace; integer outputs and
planes are compared without tolerance, the f64 moments within the worst-case bound of re-ordered f64 addition."""
import ctypes

import numpy as np
import pytest
import torch

import tabletop_ref as R

pytestmark = pytest.mark.gpu

K = [[61.537128448486328, 0.0, 31.025881958], [0.0, 61.3391, 23.774318695], [0.0, 0.0, 1.0]]
FLT_MAX = 3.4028234663852886e38
TABLE = (0.0, 0.0, -1.0, 1.0)   # height = 1 - z
GARBAGE = 0x5A5A5A5A


def _cam(h, w):
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(K[0][0], K[1][1], K[0][2], K[1][2], w, h)


def _lib():
    from graspldm_amd import _lib as L
    return L, L.lib()


def _tile():
    return _lib()[1].gldm_plane_ransac_tile_points()


def _shape():
    from graspldm_amd.pointcloud import segment_tile_shape
    return segment_tile_shape()


def _floats(v, n):
    return None if v is None else (ctypes.c_float * n)(*np.asarray(v, dtype=np.float32).reshape(-1)[:n])


# ------------------------------------------------------------------------------------------------------------ ransac --
def _cloud(n, seed):
    """A noisy plane z = 1 + 0.1 x - 0.05 y with 30 % outliers; rows 5 .. 7 collinear and row 9 = row 8 where they exist."""
    g = np.random.default_rng(seed)
    xy = g.uniform(-0.5, 0.5, (n, 2))
    z = 1.0 + 0.1 * xy[:, 0] - 0.05 * xy[:, 1] + g.normal(0, 0.001, n)
    out = g.random(n) < 0.3
    z[out] = g.uniform(0.5, 1.5, int(out.sum()))
    p = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
    if n >= 16:
        p[6] = p[5] + np.float32(0.25) * np.array([1, 2, -1], np.float32)
        p[7] = p[5] + np.float32(0.5) * np.array([1, 2, -1], np.float32)
        p[9] = p[8]
    return p


def _triples(n, t, seed):
    g = np.random.default_rng(seed)
    tri = g.integers(0, n, (t, 3)).astype(np.int32)
    if t >= 65 and n >= 16:
        tri[3] = (4, 4, 11)      # repeated index
        tri[10] = (5, 6, 7)      # collinear
        tri[20] = (8, 9, 12)     # coincident points
        tri[30] = (1, n, 2)      # out of range
        tri[40] = (-1, 3, 2)
        tri[64] = (12, 13, 14)
    return tri


def _raw_ransac(pts, tri, tol, min_cross2):
    L, lib = _lib()
    n, t = pts.shape[0], tri.shape[0]
    d_pts, d_tri = torch.from_numpy(pts).cuda(), torch.from_numpy(tri).cuda()
    nbytes = lib.gldm_plane_ransac_workspace_bytes(n, t)
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), GARBAGE, dtype=torch.int32, device="cuda")
    planes = torch.full((t, 4), -77.0, device="cuda")
    counts = torch.full((t,), 123456, dtype=torch.int32, device="cuda")
    L.call("gldm_plane_ransac", L.ptr(d_pts), n, L.ptr(d_tri), t, tol, min_cross2, L.ptr(ws), nbytes, L.ptr(planes), L.ptr(counts),
           L.current_stream())
    torch.cuda.synchronize()
    return planes.cpu().numpy(), counts.cpu().numpy()


def _sizes():
    tile = _tile()
    return [3, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 37]


@pytest.mark.parametrize("which", range(8))
def test_ransac_counts_and_planes_equal_the_restatement(which):
    n = _sizes()[which]
    pts = _cloud(n, 100 + which)
    for t in (1, 2, 65, 4096):
        tri = _triples(n, t, 7 * which + t)
        planes, counts = _raw_ransac(pts, tri, 0.004, 1e-8)
        e_planes, e_counts = R.ransac(pts, tri, 0.004, 1e-8)
        assert np.array_equal(counts, e_counts), (n, t, np.nonzero(counts != e_counts)[0][:8])
        assert np.array_equal(planes.view(np.int32), e_planes.view(np.int32)), (n, t)
        if t >= 65 and n >= 16:
            assert [int(counts[i]) for i in (3, 10, 20, 30, 40)] == [-1] * 5 and not planes[[3, 10, 20, 30, 40]].any()
            assert counts[64] >= 3
        again = _raw_ransac(pts, tri, 0.004, 1e-8)
        assert np.array_equal(again[1], counts) and np.array_equal(again[0].view(np.int32), planes.view(np.int32))
    if n >= 64:
        assert counts.max() > 0.5 * n   # the noisy plane is found


def test_ransac_nan_points_never_count_and_python_entry_agrees():
    from graspldm_amd.pointcloud import plane_ransac
    pts = _cloud(700, 5)
    pts[100:140, 2] = np.nan
    pts[200, 0] = np.inf
    tri = _triples(700, 65, 9)
    planes, counts = _raw_ransac(pts, tri, 0.004, 1e-8)
    e_planes, e_counts = R.ransac(pts, tri, 0.004, 1e-8)
    assert np.array_equal(counts, e_counts) and np.array_equal(planes.view(np.int32), e_planes.view(np.int32))
    p2, c2 = plane_ransac(torch.from_numpy(pts).cuda(), tri, 0.004, 1e-8)
    assert np.array_equal(c2.cpu().numpy(), counts) and np.array_equal(p2.cpu().numpy().view(np.int32), planes.view(np.int32))


# ----------------------------------------------------------------------------------------------------------- moments --
def _raw_moments(pts, plane, tol):
    L, lib = _lib()
    n = pts.shape[0]
    d_pts = torch.from_numpy(pts).cuda()
    nbytes = lib.gldm_plane_moments_workspace_bytes(n)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((10,), -77.0, dtype=torch.float64, device="cuda")
    L.call("gldm_plane_moments", L.ptr(d_pts), n, _floats(plane, 4), tol, L.ptr(ws), nbytes, L.ptr(out), L.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("which", range(8))
def test_moments_within_the_reordering_bound_and_repeatable(which):
    n = _sizes()[which]
    pts = _cloud(n, 300 + which)
    plane = np.array([-0.1, 0.05, 1.0, -1.0], np.float32) / np.float32(np.sqrt(1.0125))
    for tol in (0.004, 10.0):   # the plane's inliers; every point
        got = _raw_moments(pts, plane, tol)
        want, mag = R.moments(pts, plane, tol)
        assert got[0] == want[0]
        assert tol < 1 or got[0] == n
        bound = n * 2.0 ** -52 * mag
        assert np.all(np.abs(got - want) <= bound), (n, tol, np.abs(got - want), bound)
        assert np.array_equal(_raw_moments(pts, plane, tol).view(np.int64), got.view(np.int64))


# ----------------------------------------------------------------------------------------------------------- segment --
def _raw_segment(depth, cam, plane=TABLE, h_min=0.01, h_max=0.5, link_dist=0.05, min_pixels=1, max_labels=64, mask=None,
                 z_range=None, depth_scale=None, cam_to_world=None, crop_box=None):
    """The C entry on poisoned buffers -> (labels [h, w], num, label_pixels, label_root) numpy."""
    L, lib = _lib()
    h, w = depth.shape
    d = depth.cuda().contiguous()
    m8 = None if mask is None else (torch.as_tensor(mask) != 0).to(torch.uint8).cuda().contiguous()
    nbytes = lib.gldm_segment_tabletop_workspace_bytes(h, w)
    assert nbytes == 16 * h * w + 8
    ws = torch.full((nbytes // 4,), GARBAGE, dtype=torch.int32, device="cuda")   # uninitialised means anything
    labels = torch.full((h, w), -9, dtype=torch.int32, device="cuda")
    stats = torch.full((1 + 2 * max_labels,), -9, dtype=torch.int32, device="cuda")
    fx, fy, cx, cy = cam.intrinsics
    z_min, z_max = (0.0, FLT_MAX) if z_range is None else z_range
    xf = _floats(None if cam_to_world is None else np.asarray(cam_to_world, dtype=np.float32)[:3], 12)
    lo, hi = (None, None) if crop_box is None else (_floats(crop_box[0], 3), _floats(crop_box[1], 3))
    L.call("gldm_segment_tabletop", L.ptr(d), int(d.dtype != torch.float32), float(depth_scale or 1.0), L.ptr(m8), h, w, fx, fy,
           cx, cy, z_min, z_max, xf, lo, hi, _floats(plane, 4), h_min, h_max, link_dist, min_pixels, max_labels, L.ptr(ws), nbytes,
           L.ptr(labels), L.ptr(stats[0:1]), L.ptr(stats[1:1 + max_labels]), L.ptr(stats[1 + max_labels:]), L.current_stream())
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    return labels.cpu().numpy(), int(s[0]), s[1:1 + max_labels], s[1 + max_labels:]


def _check(depth, ref_depth=None, **kw):
    """depth: what the device reads; ref_depth: what the restatement reads (raw units as int32 for 16-bit frames)."""
    h, w = depth.shape
    cam = _cam(h, w)
    got = _raw_segment(depth, cam, **kw)
    rk = {("max_labels" if k == "max_labels" else k): v for k, v in kw.items()}
    want = R.segment(depth if ref_depth is None else ref_depth, cam.K, rk.pop("plane", TABLE), rk.pop("h_min", 0.01),
                     rk.pop("h_max", 0.5), rk.pop("link_dist", 0.05), rk.pop("min_pixels", 1), rk.pop("max_labels", 64), **rk)
    assert got[1] == want[1], (got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (got[2], want[2], got[3], want[3])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:8]
    again = _raw_segment(depth, cam, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    return got


def _frame(fg, z_obj=0.9):
    return torch.from_numpy(np.where(fg, np.float32(z_obj), np.float32(1.0)).astype(np.float32))


def _serpentine(h, w):
    fg = np.zeros((h, w), bool)
    fg[0::2] = True
    for i, r in enumerate(range(1, h, 2)):
        fg[r, w - 1 if i % 2 == 0 else 0] = True
    return fg


def _spiral(h, w):
    """Rings on the even levels, each cut open at one pixel and bridged to the next: one long winding chain."""
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    level = np.minimum(np.minimum(r, c), np.minimum(h - 1 - r, w - 1 - c))
    fg = level % 2 == 0
    for k in range(0, (min(h, w) - 1) // 2 - 2, 2):
        if k + 4 < w - 1 - (k + 2):
            fg[k, k + 2] = False
            fg[k + 1, k + 3] = True
    return fg


def _comb(h, w):
    fg = np.zeros((h, w), bool)
    fg[:, 0::2] = True
    fg[h - 1] = True
    return fg


def _shapes():
    tw, th = _shape()
    return [(1, 1), (1, tw + 1), (th + 1, 1), (2 * th + 3, 2 * tw + 5), (200, 300)]


@pytest.mark.parametrize("which", range(5))
def test_segment_chains_across_every_tile_border(which):
    h, w = _shapes()[which]
    for make in (_serpentine, _spiral, _comb):
        fg = make(h, w)
        labels, num, pixels, root = _check(_frame(fg), link_dist=0.05)
        if make is not _spiral:
            assert num == 1 and pixels[0] == fg.sum() and root[0] == 0   # one component, rooted at its lowest pixel
            assert np.array_equal(labels != 0, fg)
    full = np.ones((h, w), bool)
    labels, num, pixels, root = _check(_frame(full))
    assert num == 1 and pixels[0] == h * w


@pytest.mark.parametrize("which", range(5))
def test_segment_checkerboard_every_pixel_its_own_component(which):
    h, w = _shapes()[which]
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    fg = (r + c) % 2 == 0
    labels, num, _, _ = _check(_frame(fg), min_pixels=2)
    assert num == 0 and not labels.any()
    labels, num, pixels, root = _check(_frame(fg), min_pixels=1)
    k = min(64, int(fg.sum()))
    assert num == k and pixels[:k].tolist() == [1] * k
    assert root[:k].tolist() == np.nonzero(fg.reshape(-1))[0][:k].tolist()   # the tie rule: the lowest roots, in order


@pytest.mark.parametrize("blobs", [63, 64, 65])
def test_segment_equal_blobs_ties_and_the_cap(blobs):
    tw, th = _shape()
    h, w = 2 * th + 3, 2 * tw + 5
    fg = np.zeros((h, w), bool)
    per_row = (w - 1) // 5
    for b in range(blobs):
        r, c = 1 + 5 * (b // per_row), 1 + 5 * (b % per_row)
        fg[r:r + 3, c:c + 3] = True
    assert 1 + 5 * ((blobs - 1) // per_row) + 3 <= h
    labels, num, pixels, root = _check(_frame(fg), min_pixels=9)
    assert num == min(blobs, 64) and pixels[:num].tolist() == [9] * num and sorted(root[:num].tolist()) == root[:num].tolist()
    assert (labels != 0).sum() == 9 * num
    _, num, _, _ = _check(_frame(fg), min_pixels=10)
    assert num == 0
    _, num, pixels, _ = _check(_frame(fg), min_pixels=9, max_labels=5)
    assert num == 5 and pixels.shape == (5,)


def test_segment_depth_step_between_touching_blobs():
    h, w = 40, 90
    d = np.ones((h, w), np.float32)
    d[5:30, 10:40] = 0.9
    d[5:30, 40:70] = 0.88
    cam = _cam(h, w)
    _, xyz = R.foreground(torch.from_numpy(d), cam.K, TABLE, 0.01, 0.5)
    gap = np.sqrt(((xyz[5:30, 40] - xyz[5:30, 39]).astype(np.float64) ** 2).sum(axis=1))
    side = np.sqrt(((xyz[5:30, 11:40] - xyz[5:30, 10:39]).astype(np.float64) ** 2).sum(axis=2)).max()
    assert side < gap.min() * 0.9
    below, above = float(gap.min()) * 0.999, float(gap.max()) * 1.001
    labels, num, pixels, _ = _check(torch.from_numpy(d), link_dist=below, min_pixels=10)
    assert num == 2 and pixels[:2].tolist() == [750, 750] and labels[10, 39] == 1 and labels[10, 40] == 2
    labels, num, pixels, _ = _check(torch.from_numpy(d), link_dist=above, min_pixels=10)
    assert num == 1 and pixels[0] == 1500
    _, num, _, _ = _check(torch.from_numpy(d), link_dist=float("inf"), min_pixels=10)
    assert num == 1
    _, num, pixels, _ = _check(torch.from_numpy(d), link_dist=0.0, min_pixels=1, max_labels=3)
    assert num == 3 and pixels.tolist() == [1, 1, 1]


def test_segment_height_window_and_dead_pixels():
    tw, th = _shape()
    h, w = th + 9, 2 * tw + 20
    ramp = np.linspace(0.998, 0.45, w, dtype=np.float32)   # heights 0.002 .. 0.55: straddles h_min and h_max
    d = np.ones((h, w), np.float32)
    d[4:h - 4] = ramp[None, :]
    g = np.random.default_rng(11)
    for bad in (np.nan, 0.0, np.inf, -0.5):
        d[g.random((h, w)) < 0.04] = bad
    labels, num, pixels, _ = _check(torch.from_numpy(d), link_dist=0.05, min_pixels=3)
    assert num >= 1
    hgt = 1.0 - d
    with np.errstate(invalid="ignore"):
        assert not labels[~((hgt > 0.01) & (hgt <= 0.5))].any()
    # the window's edges, exactly: a row of pixels at heights around both thresholds
    e = np.ones((1, 8), np.float32)
    hmin, hmax = np.float32(0.01), np.float32(0.5)
    e[0, :8] = np.float32(1.0) - np.array([np.nextafter(hmin, np.float32(0)), hmin, np.nextafter(hmin, np.float32(1)), 0.2,
                                           np.nextafter(hmax, np.float32(0)), hmax, np.nextafter(hmax, np.float32(1)), 0.2],
                                          dtype=np.float32)
    _check(torch.from_numpy(e), link_dist=float("inf"), min_pixels=1)


def test_segment_u16_mask_window_transform_box():
    tw, th = _shape()
    h, w = th + 13, tw + 29
    g = np.random.default_rng(21)
    raw = np.full((h, w), 1000, np.int32)
    raw[3:20, 5:40] = 900
    raw[25:40, 30:80] = 850
    raw[10:35, 60:70] = 700
    raw[g.random((h, w)) < 0.05] = 0
    dev = torch.from_numpy(raw.astype(np.int16))   # the 16 bits of the raw units
    ref = torch.from_numpy(raw)
    mask = torch.from_numpy((g.random((h, w)) < 0.9).astype(np.uint8))
    _, num, _, _ = _check(dev, ref_depth=ref, depth_scale=0.001, link_dist=0.05, min_pixels=4)
    assert num >= 3
    _check(dev, ref_depth=ref, depth_scale=0.001, mask=mask, link_dist=0.05, min_pixels=2)
    _check(dev, ref_depth=ref, depth_scale=0.001, mask=mask, z_range=(0.75, 0.95), link_dist=0.05, min_pixels=2)
    # a camera looking down at a table in the world frame: z_world = 1.2 - z_cam, table at z_world = 0.2
    xf = np.array([[1, 0, 0, 0.1], [0, -1, 0, 0.2], [0, 0, -1, 1.2]], np.float32)
    plane = (0.0, 0.0, 1.0, -0.2)
    _, num, _, _ = _check(dev, ref_depth=ref, depth_scale=0.001, cam_to_world=xf, plane=plane, link_dist=0.05, min_pixels=4)
    assert num >= 3
    box = ((-0.2, -0.3, 0.0), (0.45, 0.5, 0.48))
    _, num, _, _ = _check(dev, ref_depth=ref, depth_scale=0.001, mask=mask, z_range=(0.6, 0.95), cam_to_world=xf, plane=plane,
                          crop_box=box, link_dist=0.05, min_pixels=2)
    assert num >= 1
    f32 = torch.from_numpy(raw.astype(np.float32) * np.float32(0.001))
    _check(f32, mask=mask, cam_to_world=xf, plane=plane, crop_box=box, link_dist=0.02, min_pixels=2, max_labels=7)


def test_python_entry_and_depth_to_objects_on_its_labels():
    from graspldm_amd.pointcloud import depth_to_objects, segment_tabletop
    h, w = 70, 150
    d = np.ones((h, w), np.float32)
    d[5:30, 10:40] = 0.9
    d[5:30, 40:70] = 0.8
    d[40:60, 20:120] = 0.85
    d[62:64, 5:7] = 0.9
    d[12, 20] = np.nan
    cam = _cam(h, w)
    depth = torch.from_numpy(d).cuda()
    labels, num, plane, pixels, root = segment_tabletop(depth, cam, plane=TABLE, link_dist=0.05, min_pixels=10,
                                                        return_stats=True)
    want = R.segment(torch.from_numpy(d), cam.K, TABLE, 0.01, 0.5, 0.05, 10, 64)
    assert num == want[1] == 3 and np.array_equal(labels.cpu().numpy(), want[0])
    assert pixels == want[2].tolist() and root == want[3].tolist() and pixels[:3] == [2000, 750, 749]
    assert plane.as_array().tolist() == list(TABLE)
    clouds = depth_to_objects(depth, cam, labels, num_labels=num)
    assert [c.shape[0] for c in clouds] == pixels[:num]
