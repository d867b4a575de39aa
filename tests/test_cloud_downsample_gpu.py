"""GPU: gldm_voxel_downsample (through pointcloud.voxel_downsample) against the numpy restatement
(tests/cloud_downsample_ref.py): exact equality of every output, bit for bit where it is a float.  No tolerance: counts,
minima and integer sums do not depend on the order of the atomics, and the f64 expressions are restated operation by
operation."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_downsample_ref as ref
import normals_ref
from test_cloud_downsample_cpu import face_lattice

pytestmark = pytest.mark.gpu

KEYS = ("out_points", "out_start", "out_count", "first", "members", "voxel")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _gpu(points, start, count, v, return_map=True):
    from graspldm_amd.pointcloud import voxel_downsample
    res = voxel_downsample(torch.from_numpy(points).cuda(), v, start=start, count=count, return_map=return_map)
    out = dict(out_points=res[0].cpu().numpy(), out_start=np.asarray(res[1], dtype=np.int32),
               out_count=np.asarray(res[2], dtype=np.int32), first=res[3].cpu().numpy(), members=res[4].cpu().numpy())
    if return_map:
        out["voxel"] = res[5].cpu().numpy()
    return out


def _same(got, exp, keys=KEYS):
    for key in keys:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert np.array_equal(_bits(got[key]), _bits(exp[key])), key


def _check(points, start, count, v):
    got, exp = _gpu(points, start, count, v), ref.voxel_downsample(points, start, count, v)
    _same(got, exp)
    return got, exp


def _ragged(clouds, gap=5, first=3):
    """The clouds packed with NaN-filled gaps; no start is a multiple of 256."""
    start, at = [], first
    for c in clouds:
        assert at % 256 != 0
        start.append(at)
        at += c.shape[0] + gap
        at += 1 if at % 256 == 0 else 0
    points = np.full((at + 7, 3), np.nan, dtype=np.float32)
    for s, c in zip(start, clouds):
        points[s:s + c.shape[0]] = c
    return points, start, [c.shape[0] for c in clouds]


def _cube(n, seed, side=0.05, centre=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-side / 2, side / 2, (n, 3)) + np.asarray(centre)).astype(np.float32)


def test_ragged_call_over_every_size_class():
    points, start, count = _ragged([_cube(n, seed=n, centre=(0.01, -0.02, 0.6)) for n in (0, 1, 2, 255, 256, 257, 600)])
    got, _ = _check(points, start, count, 0.004)
    assert got["out_count"][:3].tolist() == [0, 1, 2] and 300 < got["out_count"][-1] < 600   # voxels of one and of many points
    assert got["members"].max() > 1 and got["members"].sum() == sum(count)
    gaps = np.ones(points.shape[0], dtype=bool)
    for s, c in zip(start, count):
        gaps[s:s + c] = False
    assert np.all(got["voxel"][gaps] == -1) and np.all(got["voxel"][~gaps] >= 0)


def test_all_points_in_one_voxel_every_atomic_contends():
    pc = _cube(600, seed=1, side=0.008, centre=(0.105, -0.095, 0.605))
    got, _ = _check(pc, [0], [600], 0.01)
    assert got["out_count"].tolist() == [1] and got["members"].tolist() == [600] and got["first"].tolist() == [0]
    assert np.all(got["voxel"] == 0)


def test_every_point_in_its_own_voxel_table_at_its_maximum_load():
    rng = np.random.default_rng(2)
    cells = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-5, 5), np.arange(-3, 3), indexing="ij"), -1).reshape(-1, 3)
    cells = cells[rng.permutation(600)]
    pc = ((cells + rng.uniform(0.1, 0.9, (600, 3))) * 0.01).astype(np.float32)
    got, _ = _check(pc, [0], [600], 0.01)
    assert got["out_count"].tolist() == [600] and np.all(got["members"] == 1)
    assert np.array_equal(got["first"], np.arange(600)) and np.array_equal(got["voxel"], np.arange(600))


def test_duplicated_points():
    p = normals_ref.half_sphere(300, seed=2)
    both = np.concatenate([p, p])[np.random.default_rng(2).permutation(600)]
    got, _ = _check(both, [0], [600], 0.0005)
    assert np.all(got["members"] % 2 == 0)
    single = got["members"] == 2                 # twice the same point: the centroid is the quantised point itself
    assert single.sum() > 100
    src = both[got["first"][single]].astype(np.float64)
    v = np.float64(np.float32(0.0005))
    assert np.all(np.abs(got["out_points"][single] - src) <= v * 2.0 ** -17 + np.spacing(np.abs(src).astype(np.float32)))


def test_points_on_cell_faces():
    pc = face_lattice()
    got, _ = _check(pc, [0], [pc.shape[0]], 0.5)
    assert got["out_count"].tolist() == [729] and np.all(got["members"] == 2)
    assert np.array_equal(got["out_points"], pc[:729])


def test_two_hundred_small_clouds_probing_wraps_round_the_regions():
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 41, 200)
    clouds = [_cube(int(n), seed=100 + i, side=0.02, centre=rng.uniform(-0.3, 0.3, 3)) for i, n in enumerate(sizes)]
    points, start, count = _ragged(clouds, gap=2)
    got, _ = _check(points, start, count, 0.006)
    assert got["out_count"].min() >= 1 and (got["members"] > 1).any() and (got["out_count"] == np.asarray(count)).any()


def test_a_shuffled_cloud_gives_the_same_voxels_and_first_follows_the_shuffle():
    pc = normals_ref.organised_patch()
    n = pc.shape[0]
    perm = np.random.default_rng(6).permutation(n)
    o, eo = _check(pc, [0], [n], 0.003)
    s, es = _check(pc[perm], [0], [n], 0.003)

    def voxels(got, exp):
        rows = np.concatenate([exp["cell"], _bits(got["out_points"]).astype(np.int64), got["members"][:, None]], axis=1)
        return rows[np.lexsort(rows.T[::-1])]

    assert np.array_equal(voxels(o, eo), voxels(s, es))          # the same multiset of (cell, centroid, members)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)                                     # source row -> its row in the shuffled cloud
    cells = ref.quantise(pc, 0.003)[0]
    for j in range(0, s["first"].shape[0], 7):                   # first = the lowest shuffled row among the voxel's points
        members_o = np.nonzero(np.all(cells == es["cell"][j], axis=1))[0]
        assert s["first"][j] == inv[members_o].min()
    assert np.all(np.diff(s["first"]) > 0) and np.all(np.diff(o["first"]) > 0)


def test_voxel_maps_every_row_to_the_output_row_of_its_cell():
    points, start, count = _ragged([_cube(700, seed=8, centre=(0.0, 0.0, 0.5)), _cube(300, seed=9)])
    got, exp = _check(points, start, count, 0.005)
    for i, (s, c) in enumerate(zip(start, count)):
        cell, _ = ref.quantise(points[s:s + c], 0.005)
        rows = got["out_start"][i] + got["voxel"][s:s + c]
        assert np.all((0 <= got["voxel"][s:s + c]) & (got["voxel"][s:s + c] < got["out_count"][i]))
        assert np.array_equal(exp["cell"][rows], cell)
        assert np.array_equal(np.bincount(got["voxel"][s:s + c], minlength=got["out_count"][i]),
                              got["members"][got["out_start"][i]:got["out_start"][i] + got["out_count"][i]])


def test_dense_batch_equals_its_ragged_call_and_a_cloud_alone_equals_it_at_position_two_of_three():
    from graspldm_amd.pointcloud import voxel_downsample
    b, n = 3, 300
    pc = np.stack([normals_ref.half_sphere(n, seed=20 + i) for i in range(b)])
    flat = pc.reshape(b * n, 3)
    start, count = [i * n for i in range(b)], [n] * b
    rag, _ = _check(flat, start, count, 0.01)
    out, ostart, ocount, first, members, vox = voxel_downsample(torch.from_numpy(pc).cuda(), 0.01, return_map=True)
    assert ostart == rag["out_start"].tolist() and ocount == rag["out_count"].tolist() and vox.shape == (b, n)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(rag["out_points"]))
    assert np.array_equal(first.cpu().numpy(), rag["first"]) and np.array_equal(members.cpu().numpy(), rag["members"])
    assert np.array_equal(vox.cpu().numpy().reshape(-1), rag["voxel"])
    one, s0, c0, first0, members0, vox0 = voxel_downsample(torch.from_numpy(pc[1]).cuda(), 0.01, return_map=True)
    lo, hi = ostart[1], ostart[1] + ocount[1]
    assert (s0, c0) == (0, ocount[1]) and torch.equal(one.view(torch.int32), out[lo:hi].view(torch.int32))
    assert torch.equal(first0, first[lo:hi]) and torch.equal(members0, members[lo:hi]) and torch.equal(vox0, vox[1])


def test_two_calls_are_bitwise_equal_and_voxel_may_be_null():
    points, start, count = _ragged([_cube(700, seed=17), _cube(33, seed=18), _cube(1025, seed=19)])
    a = _gpu(points, start, count, 0.004)
    b = _gpu(points, start, count, 0.004)
    for key in a:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    c = _gpu(points, start, count, 0.004, return_map=False)      # voxel = NULL: the map pass is skipped, nothing else moves
    assert "voxel" not in c
    _same(c, ref.voxel_downsample(points, start, count, 0.004), keys=KEYS[:-1])


def test_max_points_grows_the_voxel_until_the_patch_fits_and_reports_the_size():
    from graspldm_amd.pointcloud import voxel_downsample_capped
    pc = normals_ref.organised_patch()            # 48 x 64 points, 1 mm apart
    (out, _, m, first, members), used = voxel_downsample_capped(torch.from_numpy(pc).cuda(), 0.001, max_points=500)
    size, grows = 0.001, 0
    while ref.downsample_cloud(pc, size)["first"].shape[0] > 500:
        size, grows = size * 1.25, grows + 1
    exp = ref.downsample_cloud(pc, size)
    assert 2 <= grows <= 16 and used == float(np.float32(size)) and used > 0.001
    assert m == exp["first"].shape[0] <= 500 and out.shape == (m, 3)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(exp["points"]))
    assert np.array_equal(first.cpu().numpy(), exp["first"]) and np.array_equal(members.cpu().numpy(), exp["members"])
    (_, _, m0, _, _), used0 = voxel_downsample_capped(torch.from_numpy(pc).cuda(), 0.001, max_points=None)
    assert used0 == float(np.float32(0.001)) and m0 > 500
    with pytest.raises(ValueError, match="max_points"):
        voxel_downsample_capped(torch.from_numpy(pc).cuda(), 1e-4, max_points=1)   # 1.25^16 = 36: 3.6 mm voxels at the end


def test_the_entry_refuses_what_lies_outside_its_envelope_before_any_pointer():
    from graspldm_amd import _abi, _lib
    h = _lib.lib()
    bad, unsupported = _abi.CONSTANTS["GLDM_ERR_INVALID_ARG"], _abi.CONSTANTS["GLDM_ERR_UNSUPPORTED"]
    null = ctypes.c_void_p(None)

    def entry(b=1, n_max=10, rows=10, v=0.01):
        return h.gldm_voxel_downsample(null, null, null, b, n_max, rows, v, null, 0, null, null, null, null, null, null, null)

    for v in (0.0, float("inf"), -0.01, float("nan")):
        assert entry(v=v) == bad, v
    assert entry(b=0) == bad and entry(n_max=-1) == bad and entry(rows=-1) == bad
    assert entry(n_max=(1 << 22) + 1) == unsupported
    assert entry(rows=(1 << 24) + 1) == unsupported and entry(b=65536) == unsupported
    assert h.gldm_voxel_downsample_workspace_bytes(1, (1 << 22) + 1, 10) == unsupported
    assert h.gldm_voxel_downsample_workspace_bytes(0, 10, 10) == bad
    assert h.gldm_voxel_downsample_workspace_bytes(2, 300, 1000) >= 2 * 1000 * 48 + 4 * 1000 + 4 * 2 * 2
    assert entry() == bad   # inside the envelope, the null pointers are refused, still before the device
