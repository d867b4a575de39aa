"""GPU: gldm_neighbor_stats and gldm_filter_outliers (through pointcloud.neighbor_stats / remove_outliers) against the numpy
restatement (tests/cloud_filter_ref.py): exact equality of every output, bit for bit where it is a float.  No tolerance: the
scan's d2 is restated operation by operation, the f64 sums in the kernel's fixed order."""
import numpy as np
import pytest
import torch

import cloud_filter_ref as ref
import normals_ref

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _gpu(points, start, count, k, r, mn, std):
    from graspldm_amd.pointcloud import remove_outliers
    out, ostart, ocount, kept, stats = remove_outliers(torch.from_numpy(points).cuda(), k=k, max_radius=r, min_neighbors=mn,
                                                       std_ratio=std, start=start, count=count)
    return dict(neighbors=stats["neighbors"].cpu().numpy(), score=stats["score"].cpu().numpy(),
                stats=torch.stack([stats["mu"], stats["sigma"]], dim=1).cpu().numpy(), out_points=out.cpu().numpy(),
                out_start=np.asarray(ostart, dtype=np.int32), out_count=np.asarray(ocount, dtype=np.int32),
                kept=kept.cpu().numpy())


def _same(got, exp):
    for key in ("neighbors", "out_start", "out_count", "kept"):
        assert got[key].dtype == exp[key].dtype and np.array_equal(got[key], exp[key]), key
    for key in ("score", "stats", "out_points"):
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert np.array_equal(_bits(got[key]), _bits(exp[key])), key


def _check(points, start, count, k, r, mn, std=None):
    got, exp = _gpu(points, start, count, k, r, mn, std), ref.filter_outliers(points, start, count, k, r, mn, std)
    _same(got, exp)
    return got


def _ragged(counts, seed, gap=5, first=3, side=0.05):
    """Clouds of the given sizes, uniform in a cube, packed with NaN-filled gaps; no start is a multiple of 256."""
    rng = np.random.default_rng(seed)
    start, at = [], first
    for c in counts:
        assert at % 256 != 0
        start.append(at)
        at += c + gap
        at += 1 if at % 256 == 0 else 0
    points = np.full((at + 7, 3), np.nan, dtype=np.float32)
    for s, c in zip(start, counts):
        points[s:s + c] = rng.uniform(0.0, side, (c, 3)).astype(np.float32)
    return points, start, list(counts)


@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("std", [None, 1.5])
def test_ragged_call_over_every_size_class(k, std):
    points, start, count = _ragged([0, 1, 2, k, k + 1, 255, 256, 257, 600], seed=k)
    got = _check(points, start, count, k, 0.012, 2, std)
    assert got["out_count"][0] == got["out_count"][1] == 0 and got["out_count"][-1] > 300
    assert got["neighbors"].max() == k                       # the cap is reached, so the k-th distance bound is in play


def test_neighbor_stats_alone_equals_the_restatement():
    from graspldm_amd.pointcloud import neighbor_stats
    points, start, count = _ragged([300, 0, 513], seed=7)
    exp = ref.filter_outliers(points, start, count, 12, 0.01, 0)
    nb, sc = neighbor_stats(torch.from_numpy(points).cuda(), 12, 0.01, start=start, count=count)
    assert np.array_equal(nb.cpu().numpy(), exp["neighbors"])
    assert np.array_equal(_bits(sc.cpu().numpy()), _bits(exp["score"]))


def _doubled(n=300, seed=2):
    p = normals_ref.half_sphere(n, seed=seed)
    both = np.concatenate([p, p])
    return both[np.random.default_rng(seed).permutation(2 * n)]


def test_duplicates_are_neighbours_and_the_point_itself_is_not():
    points = _doubled()
    got = _check(points, [0], [600], 8, 0.01, 1, 2.0)
    assert got["neighbors"].min() >= 1                       # the twin, at d2 = 0
    one = _check(points, [0], [600], 1, 0.01, 1)
    assert np.all(one["neighbors"] == 1) and np.all(one["score"] == 0.0)


def test_radius_zero():
    points = _doubled()
    got = _check(points, [0], [600], 4, 0.0, 1)
    assert np.all(got["neighbors"] == 1) and got["out_count"][0] == 600
    alone = normals_ref.half_sphere(300, seed=3)
    got = _check(alone, [0], [300], 4, 0.0, 1, 1.0)
    assert np.all(got["neighbors"] == 0) and got["out_count"][0] == 0 and np.all(got["stats"] == 0.0)


@pytest.mark.parametrize("k", [4, 6, 8, 16])
def test_lattice_with_ties_at_every_kth_distance(k):
    g = np.arange(6, dtype=np.float32) * np.float32(0.25)    # exact in f32: 6 neighbours tie at 0.25, 12 at 0.25 * sqrt(2)
    points = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    got = _check(points, [0], [216], k, 0.36, 4, 0.5)
    assert got["neighbors"].min() == min(k, 6)               # a corner: 3 + 3 within the radius


def test_min_neighbors_zero_without_the_statistical_rule_keeps_everything():
    points, start, count = _ragged([40, 300, 1, 257], seed=11, side=0.2)
    got = _check(points, start, count, 8, 0.01, 0)
    assert (got["neighbors"] == 0).any()
    assert got["out_count"].tolist() == count and np.array_equal(got["kept"], np.concatenate([np.arange(c) for c in count]))
    assert np.array_equal(_bits(got["out_points"]), _bits(np.concatenate([points[s:s + c] for s, c in zip(start, count)])))


def test_min_neighbors_k_on_a_sparse_cloud_drops_everything():
    points, start, count = _ragged([300, 257], seed=13, side=1.0)
    got = _check(points, start, count, 8, 0.01, 8)
    assert got["out_count"].tolist() == [0, 0] and got["out_start"].tolist() == [0, 0] and got["kept"].shape == (0,)
    assert got["out_points"].shape == (0, 3)


K_PATCH, R_PATCH, MIN_PATCH = 8, 0.003, 2


@pytest.fixture(scope="module")
def patch():
    """The 48 x 64 organised patch with 40 isolated points mixed in, in pixel order and under a fixed shuffle, each with its
    restated scan (computed once)."""
    base = normals_ref.organised_patch()
    rng = np.random.default_rng(5)
    iso = np.stack([rng.uniform(-0.03, 0.03, 40), rng.uniform(-0.02, 0.02, 40), 0.2 + 0.008 * np.arange(40)], axis=1)
    at = np.sort(rng.choice(base.shape[0], 40, replace=False))
    ordered = np.insert(base, at, iso.astype(np.float32), axis=0)
    n = ordered.shape[0]
    is_iso = np.zeros(n, dtype=bool)
    is_iso[at + np.arange(40)] = True
    assert np.array_equal(ordered[is_iso], iso.astype(np.float32))
    perm = np.random.default_rng(6).permutation(n)
    scans = {name: ref.neighbor_stats(p, K_PATCH, R_PATCH) for name, p in (("ordered", ordered), ("shuffled", ordered[perm]))}
    return dict(ordered=ordered, shuffled=ordered[perm], perm=perm, is_iso=is_iso, scans=scans, n=n)


def _patch_expected(patch, name, std):
    """ref.filter_outliers for the one cloud, from the scan computed once."""
    points = patch[name]
    nb, sc = patch["scans"][name]
    _, mu, sigma = ref.cloud_moments(nb, sc, MIN_PATCH)
    keep = np.nonzero(ref.keep_mask(nb, sc, MIN_PATCH, std, mu, sigma))[0].astype(np.int32)
    return dict(neighbors=nb, score=sc, stats=np.array([[mu, sigma]]), out_points=points[keep],
                out_start=np.zeros(1, dtype=np.int32), out_count=np.array([keep.shape[0]], dtype=np.int32), kept=keep)


def test_broad_phase_changes_no_bit_pixel_order_against_shuffle(patch):
    n, perm = patch["n"], patch["perm"]
    got = {}
    for name in ("ordered", "shuffled"):
        got[name] = _gpu(patch[name], [0], [n], K_PATCH, R_PATCH, MIN_PATCH, None)
        _same(got[name], _patch_expected(patch, name, None))
    o, s = got["ordered"], got["shuffled"]
    assert np.array_equal(_bits(s["score"]), _bits(o["score"][perm])) and np.array_equal(s["neighbors"], o["neighbors"][perm])
    assert np.array_equal(np.sort(perm[s["kept"]]), o["kept"])                     # the same kept set
    assert np.array_equal(o["kept"], np.nonzero(~patch["is_iso"])[0])              # exactly the injected points went
    assert np.all(o["neighbors"][patch["is_iso"]] == 0)


@pytest.mark.parametrize("std", [1.0, 2.0])
def test_statistical_rule_on_the_patch(patch, std):
    got = _gpu(patch["ordered"], [0], [patch["n"]], K_PATCH, R_PATCH, MIN_PATCH, std)
    _same(got, _patch_expected(patch, "ordered", std))
    kept = got["out_count"][0]
    assert 0 < kept < patch["n"] - 40                                              # the rule bites beyond the radius rule
    if std == 2.0:
        assert kept > _gpu(patch["ordered"], [0], [patch["n"]], K_PATCH, R_PATCH, MIN_PATCH, 1.0)["out_count"][0]


def test_dense_batch_equals_its_ragged_call():
    from graspldm_amd.pointcloud import neighbor_stats, remove_outliers
    b, n = 3, 300
    pc = np.stack([normals_ref.half_sphere(n, seed=20 + i) for i in range(b)])
    flat = pc.reshape(b * n, 3)
    start, count = [i * n for i in range(b)], [n] * b
    rag = _check(flat, start, count, 8, 0.012, 3, 1.0)
    out, ostart, ocount, kept, stats = remove_outliers(torch.from_numpy(pc).cuda(), k=8, max_radius=0.012, min_neighbors=3,
                                                       std_ratio=1.0)
    assert ostart == rag["out_start"].tolist() and ocount == rag["out_count"].tolist()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(rag["out_points"])) and np.array_equal(kept.cpu().numpy(), rag["kept"])
    assert stats["neighbors"].shape == (b, n) and np.array_equal(stats["neighbors"].cpu().numpy().reshape(-1), rag["neighbors"])
    assert np.array_equal(_bits(stats["score"].cpu().numpy().reshape(-1)), _bits(rag["score"]))
    nb, sc = neighbor_stats(torch.from_numpy(pc).cuda(), 8, 0.012)
    assert nb.shape == (b, n) and torch.equal(nb, stats["neighbors"]) and torch.equal(sc.view(torch.int32),
                                                                                      stats["score"].view(torch.int32))
    one, s0, c0, kept0, _ = remove_outliers(torch.from_numpy(pc[1]).cuda(), k=8, max_radius=0.012, min_neighbors=3, std_ratio=1.0)
    lo, hi = ostart[1], ostart[1] + ocount[1]
    assert (s0, c0) == (0, ocount[1]) and torch.equal(one, out[lo:hi]) and torch.equal(kept0, kept[lo:hi])


def test_two_calls_are_bitwise_equal():
    points, start, count = _ragged([700, 33, 1025], seed=17)
    a = _gpu(points, start, count, 12, 0.012, 3, 1.0)
    b = _gpu(points, start, count, 12, 0.012, 3, 1.0)
    for key in a:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
