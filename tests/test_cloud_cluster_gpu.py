"""GPU: gldm_cluster_cloud and gldm_split_labels against the numpy restatement (tests/cloud_cluster_ref.py, the brute-force
all-pairs search): exact equality of every output.  Every call goes through the C ABI TWICE, each time with the outputs
poisoned and the workspace filled with other garbage, and the two results are compared bitwise.  No tolerance: the
components are a property of the link graph, the roots are minima, the sizes are counts."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_cluster_ref as ref
from test_cloud_cluster_cpu import LINKS, blobs, serpentine, straddling_cloud, threshold_pairs

pytestmark = pytest.mark.gpu

POISON = -7
CKEYS = ("labels", "num_labels", "label_points", "label_root")
SKEYS = ("out_points", "out_row", "obj_start", "obj_count", "out_total")


def _garbage(nbytes, seed):
    """A 16-byte aligned device buffer of nbytes filled with noise."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, ((nbytes + 7) // 8 + 2,), generator=g, dtype=torch.int64).cuda()


def _twice(run):
    a, b = run(1), run(2)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), f"two calls differ in {key}"
    return a


def _cluster(points, start, count, link, plane=None, h=(0.0, 0.0), min_points=1, max_labels=64, n_max=None):
    from graspldm_amd import _lib as L
    lib = L.lib()
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).cuda()
    rows, b = pts.shape[0], len(start)
    n_max = max(count) if n_max is None else n_max
    sc = torch.tensor([start, count], dtype=torch.int32).cuda()
    nbytes = lib.gldm_cluster_cloud_workspace_bytes(b, n_max, rows)
    assert nbytes >= 0
    pl = None if plane is None else np.ascontiguousarray(plane, dtype=np.float32)

    def run(seed):
        ws = _garbage(nbytes, seed)
        assert ws.data_ptr() % 16 == 0
        labels = torch.full((max(rows, 1),), POISON, dtype=torch.int32).cuda()
        tabs = torch.full((b * (1 + 2 * max_labels),), POISON, dtype=torch.int32).cuda()
        L.call("gldm_cluster_cloud", L.ptr(pts) if rows else None, L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, float(link),
               None if pl is None else pl.ctypes.data_as(ctypes.c_void_p), float(h[0]), float(h[1]), min_points, max_labels,
               L.ptr(ws), nbytes, L.ptr(labels), L.ptr(tabs[:b]), L.ptr(tabs[b:b + b * max_labels]),
               L.ptr(tabs[b + b * max_labels:]), L.current_stream())
        torch.cuda.synchronize()
        t = tabs.cpu().numpy()
        return dict(labels=labels[:rows].cpu().numpy(), num_labels=t[:b].copy(),
                    label_points=t[b:b + b * max_labels].reshape(b, max_labels).copy(),
                    label_root=t[b + b * max_labels:].reshape(b, max_labels).copy())

    return _twice(run)


def _check_cluster(points, start, count, link, **kw):
    got = _cluster(points, start, count, link, **kw)
    h = kw.pop("h", (0.0, 0.0))
    exp = ref.cluster_cloud(points, start, count, link, h_min=h[0], h_max=h[1], poison=POISON, **kw)
    for key in CKEYS:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert np.array_equal(got[key], exp[key]), key
    return got


def _split(points, labels, start, count, max_labels, n_max=None):
    from graspldm_amd import _lib as L
    lib = L.lib()
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    rows, b = pts.shape[0], len(start)
    n_max = max(count) if n_max is None else n_max
    sc = torch.tensor([start, count], dtype=torch.int32).cuda()
    nbytes = lib.gldm_split_labels_workspace_bytes(b, n_max, rows, max_labels)
    assert nbytes >= 0

    def run(seed):
        ws = _garbage(nbytes, seed)
        out = torch.full((max(rows, 1), 3), float("nan"), dtype=torch.float32).cuda()
        src = torch.full((max(rows, 1),), POISON, dtype=torch.int32).cuda()
        tabs = torch.full((2 * b * max_labels + 1,), POISON, dtype=torch.int32).cuda()
        m = b * max_labels
        L.call("gldm_split_labels", L.ptr(pts) if rows else None, L.ptr(lab) if rows else None, L.ptr(sc[0]), L.ptr(sc[1]), b,
               n_max, rows, max_labels, L.ptr(ws), nbytes, L.ptr(out), L.ptr(src), L.ptr(tabs[:m]), L.ptr(tabs[m:2 * m]),
               L.ptr(tabs[2 * m:]), L.current_stream())
        torch.cuda.synchronize()
        t = tabs.cpu().numpy()
        total = int(t[-1])
        assert 0 <= total <= rows
        rest = src[total:rows].cpu().numpy()
        assert np.all(rest == POISON) and bool(torch.isnan(out[total:rows]).all())   # nothing past the total is written
        return dict(out_points=out[:total].cpu().numpy(), out_row=src[:total].cpu().numpy(),
                    obj_start=t[:m].reshape(b, max_labels).copy(), obj_count=t[m:2 * m].reshape(b, max_labels).copy(),
                    out_total=t[-1].copy())

    return _twice(run)


def _check_split(points, labels, start, count, max_labels, **kw):
    got, exp = _split(points, labels, start, count, max_labels, **kw), ref.split_labels(points, labels, start, count, max_labels, **kw)
    for key in SKEYS:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert got[key].tobytes() == exp[key].tobytes(), key
    # the properties, whatever the restatement says
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    b = len(start)
    flat_s, flat_c = got["obj_start"].reshape(-1), got["obj_count"].reshape(-1)
    assert np.array_equal(flat_s, np.cumsum(flat_c) - flat_c) and flat_c.sum() == got["out_total"]   # dense starts
    ranges = ref.cloud_ranges(start, count, max(count) if kw.get("n_max") is None else kw["n_max"], p.shape[0])
    for i in range(b):
        for k in range(max_labels):
            s, c = got["obj_start"][i, k], got["obj_count"][i, k]
            src = got["out_row"][s:s + c]
            assert np.all(np.diff(src) > 0)                                                    # ascending inside an object
            assert np.all(np.asarray(labels)[ranges[i][0] + src] == k + 1)
            assert got["out_points"][s:s + c].tobytes() == p[ranges[i][0] + src].tobytes()    # bit copies
    return got


def _ragged(clouds, gap=5, first=3, fill=np.nan):
    """The clouds packed with gaps; no start is a multiple of 256."""
    start, at = [], first
    for c in clouds:
        assert at % 256 != 0
        start.append(at)
        at += c.shape[0] + gap
        at += 1 if at % 256 == 0 else 0
    points = np.full((at + 7, 3), fill, dtype=np.float32)
    for s, c in zip(start, clouds):
        points[s:s + c.shape[0]] = c
    return points, start, [c.shape[0] for c in clouds]


def _cube(n, seed, link=0.01, fill=1.1):
    """n random rows in a cube sized so that a row has about `fill` others within link: many components of many sizes."""
    rng = np.random.default_rng(seed)
    side = link * max(n / fill * 4.19, 1.0) ** (1 / 3)
    return (rng.uniform(-side / 2, side / 2, (n, 3)) + np.array([0.1, -0.2, 0.6])).astype(np.float32)


SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 3 * 256 + 37)


def test_every_size_class_alone():
    for n in SIZES:
        pc = _cube(n, seed=n)
        got = _check_cluster(pc, [0], [n], 0.01, min_points=1, max_labels=64)
        if n >= 63:
            assert got["num_labels"][0] > 8 and got["label_points"][0, 0] >= 2
        _check_split(pc, got["labels"], [0], [n], 64)


def test_ragged_batch_with_empty_and_invalid_clouds_and_unowned_rows():
    clouds = [_cube(n, seed=100 + n) for n in SIZES]
    points, start, count = _ragged(clouds)
    rows = points.shape[0]
    # two more clouds whose ranges leave [0, rows): treated as empty, nothing of them is read or written
    start, count = start + [rows - 5, -2], count + [40, 30]
    got = _check_cluster(points, start, count, 0.01, min_points=2, max_labels=16)
    assert got["num_labels"][0] == 0 and got["num_labels"][-1] == 0 and got["num_labels"][-2] == 0
    assert got["num_labels"][-3] == 16 and np.all(got["label_root"][0] == -1) and np.all(got["label_points"][-1] == 0)
    owned = np.zeros(rows, dtype=bool)
    for s, c in zip(start[:-2], count[:-2]):
        owned[s:s + c] = True
    assert np.all(got["labels"][~owned] == POISON) and np.all(got["labels"][owned] >= 0)
    _check_split(points, got["labels"], start, count, 16)
    # n_max below a cloud's count: the count is clamped
    _check_cluster(points, start, count, 0.01, min_points=1, max_labels=8, n_max=300)
    # every cloud empty: the tables are written, nothing else is touched
    got = _check_cluster(points, [3, 9], [0, 0], 0.01, max_labels=5)
    assert np.all(got["labels"] == POISON) and got["num_labels"].tolist() == [0, 0] and np.all(got["label_root"] == -1)
    got = _check_cluster(np.zeros((0, 3), np.float32), [0], [0], 0.01, max_labels=64)
    assert got["num_labels"].tolist() == [0]


def test_serpentine_is_one_component_and_a_gap_makes_two():
    link, n = 0.01, 1500   # 6 chunks; about 35 turns through some 1400 cells
    chain = serpentine(n, link)
    got = _check_cluster(chain, [0], [n], link, min_points=1, max_labels=4)
    assert got["num_labels"].tolist() == [1] and got["label_points"][0].tolist() == [n, 0, 0, 0]
    assert got["label_root"][0].tolist() == [0, -1, -1, -1] and np.all(got["labels"] == 1)
    cells = ref.cells_of(chain, link)
    assert len({tuple(c) for c in cells.tolist()}) > 1000
    cut = serpentine(n, link, gap_at=900)
    got = _check_cluster(cut, [0], [n], link, min_points=1, max_labels=4)
    assert got["num_labels"].tolist() == [2] and got["label_points"][0].tolist() == [900, 600, 0, 0]
    assert got["label_root"][0].tolist() == [0, 900, -1, -1]
    assert np.all(got["labels"][:900] == 1) and np.all(got["labels"][900:] == 2)
    # the chain walked from its far end, and in random order: the root is still the lowest row
    back = chain[::-1].copy()
    got = _check_cluster(back, [0], [n], link, min_points=1, max_labels=2)
    assert got["label_root"][0].tolist() == [0, -1] and got["label_points"][0, 0] == n
    mixed = chain[np.random.default_rng(5).permutation(n)]
    got = _check_cluster(mixed, [0], [n], link, min_points=1, max_labels=2)
    assert got["label_root"][0].tolist() == [0, -1] and got["label_points"][0, 0] == n


@pytest.mark.parametrize("link", LINKS)
def test_threshold_pairs_and_straddling_clouds(link):
    pts = threshold_pairs(link)
    got = _check_cluster(pts, [0], [pts.shape[0]], link, min_points=2, max_labels=64)
    assert 0 < got["num_labels"][0] and np.all(got["label_points"][0][:got["num_labels"][0]] == 2)
    clouds = [straddling_cloud(link, 300, seed) for seed in range(4)]
    points, start, count = _ragged(clouds)
    _check_cluster(points, start, count, link, min_points=1, max_labels=64)


def test_identical_points_nan_rows_inf_rows_and_rows_beyond_the_lattice():
    same = np.tile(np.array([[0.25, -0.125, 0.5]], dtype=np.float32), (300, 1))
    got = _check_cluster(same, [0], [300], 0.01, min_points=1, max_labels=3)
    assert got["label_points"][0].tolist() == [300, 0, 0] and got["label_root"][0].tolist() == [0, -1, -1]
    holed = same.copy()
    holed[0, 1] = np.nan          # the root moves to row 1
    holed[137, 2] = np.nan
    got = _check_cluster(holed, [0], [300], 0.01, min_points=1, max_labels=3)
    assert got["label_points"][0].tolist() == [298, 0, 0] and got["label_root"][0].tolist() == [1, -1, -1]
    assert got["labels"][0] == 0 and got["labels"][137] == 0 and got["labels"].sum() == 298
    # inf rows and rows beyond the lattice limit are inactive: never linked, not even two identical ones
    link = 0.5
    far = float(np.float32(ref.cell_size(link) * (2 ** 20 - 1) * (1 + 2e-7)))
    edge = float(np.float32(ref.cell_size(link) * (2 ** 20 - 1) * (1 - 2e-7)))
    pts = np.array([[far, 0, 0], [far, 0, 0], [0, np.inf, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 3e38, 3e38],
                    [edge, 0, 0], [edge, 0, 0], [0, -far, 0], [0, -far, 0], [0, 0, 0], [0, 0.3, 0]], dtype=np.float32)
    got = _check_cluster(pts, [0], [12], link, min_points=1, max_labels=4)
    assert got["labels"].tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 2, 2] and got["num_labels"].tolist() == [2]


@pytest.mark.parametrize("clusters", [63, 64, 65])
def test_equal_clusters_around_the_label_ceiling(clusters):
    pts, owner = blobs([3] * clusters, 0.01, seed=clusters)
    got = _check_cluster(pts, [0], [pts.shape[0]], 0.01, min_points=1, max_labels=64)
    k = min(clusters, 64)
    assert got["num_labels"].tolist() == [k] and np.all(got["label_points"][0, :k] == 3)
    firsts = sorted(int(np.flatnonzero(owner == c)[0]) for c in range(clusters))
    assert got["label_root"][0, :k].tolist() == firsts[:k]            # ties: the lower roots win and come first
    if clusters == 65:
        loser = owner[firsts[64]]
        assert np.all(got["labels"][owner == loser] == 0) and (got["labels"] == 0).sum() == 3


def test_size_ties_min_points_and_one_label():
    sizes = [5, 3, 5, 2, 3, 1, 4]
    pts, owner = blobs(sizes, 0.01, seed=3)
    n = pts.shape[0]
    for min_points in (2, 3, 4):          # size - 1, size, size + 1 around the blobs of 3
        got = _check_cluster(pts, [0], [n], 0.01, min_points=min_points, max_labels=64)
        assert got["num_labels"][0] == sum(s >= min_points for s in sizes)
    for min_points in (4, 5, 6):          # ... and around the two largest
        got = _check_cluster(pts, [0], [n], 0.01, min_points=min_points, max_labels=64)
        assert got["num_labels"][0] == sum(s >= min_points for s in sizes)
    got = _check_cluster(pts, [0], [n], 0.01, min_points=1, max_labels=1)
    first5 = min(int(np.flatnonzero(owner == c)[0]) for c in (0, 2))
    assert got["num_labels"].tolist() == [1] and got["label_points"].tolist() == [[5]] and got["label_root"].tolist() == [[first5]]
    assert (got["labels"] == 1).sum() == 5


def test_more_than_1024_candidate_components():
    rng = np.random.default_rng(11)
    cells = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(11), indexing="ij"), -1).reshape(-1, 3)[:1500]
    pts = (cells[rng.permutation(1500)] * 0.03).astype(np.float32)        # 1500 isolated rows, 3 link_dists apart
    pts = np.concatenate([pts, pts[[700, 20, 1333]] + np.float32(0.004)])  # three of them get a partner: size 2
    got = _check_cluster(pts, [0], [1503], 0.01, min_points=1, max_labels=64)
    assert got["num_labels"].tolist() == [64] and got["label_points"][0].tolist() == [2, 2, 2] + [1] * 61
    assert got["label_root"][0, :3].tolist() == [20, 700, 1333]
    singles = [i for i in range(80) if i != 20][:61]
    assert got["label_root"][0, 3:].tolist() == singles
    got = _check_cluster(pts, [0], [1503], 0.01, min_points=2, max_labels=64)
    assert got["num_labels"].tolist() == [3]
    # two such clouds and an ordinary one in one call: the selection is per cloud
    points, start, count = _ragged([pts, _cube(500, seed=9), pts[::-1].copy()])
    _check_cluster(points, start, count, 0.01, min_points=1, max_labels=7)


def test_plane_and_height_window_edges_to_the_ulp():
    h0, h1 = np.float32(0.01), np.float32(0.5)
    up = lambda v: np.nextafter(np.float32(v), np.float32(10))   # noqa: E731
    z = np.array([h0, up(h0), up(h0), h1, h1, up(h1), 0.2, 0.2, -0.2, 0.0], dtype=np.float32)
    pts = np.stack([np.arange(10) // 2 * 0.001, np.zeros(10), z], axis=1).astype(np.float32)
    flat = (0.0, 0.0, 1.0, 0.0)    # hgt = z exactly
    got = _check_cluster(pts, [0], [10], 0.01, plane=flat, h=(h0, h1), min_points=1, max_labels=8)
    assert (got["labels"] > 0).tolist() == [False, True, True, True, True, False, True, True, False, False]
    got = _check_cluster(pts, [0], [10], 0.01, plane=None, min_points=1, max_labels=8)
    assert np.all(got["labels"] > 0)
    # a tilted table under random rows: every rounding of the height expression counts
    rng = np.random.default_rng(4)
    nrm = np.array([0.12, -0.35, 0.93])
    nrm /= np.linalg.norm(nrm)
    plane = np.append(nrm, -0.31).astype(np.float32)
    cloud = (rng.uniform(-0.06, 0.06, (1200, 3)) + nrm * 0.31).astype(np.float32)
    hgt = ref.height(cloud, plane)
    edges = (np.float32(np.sort(hgt)[400]), np.float32(np.sort(hgt)[900]))   # both edges ARE heights of rows
    got = _check_cluster(cloud, [0], [1200], 0.012, plane=plane, h=edges, min_points=1, max_labels=64)
    order = np.argsort(hgt, kind="stable")
    assert got["labels"][order[400]] == 0 or hgt[order[401]] == hgt[order[400]]   # hgt == h_min: outside
    inside = (hgt > edges[0]) & (hgt <= edges[1])
    assert inside[order[900]] and 400 < inside.sum() <= 500 and np.all(got["labels"][~inside] == 0)
    assert got["label_points"][0].sum() <= inside.sum() and got["num_labels"][0] > 3


def test_shuffled_copy_gives_the_same_partition():
    # 48 components, so every one of them gets a label (past the ceiling the ties between equal sizes go to the lower
    # root, which a shuffle moves), on top of a random cube's worth of irregular ones
    sizes = np.random.default_rng(20).integers(2, 40, 40).tolist()
    pc = np.concatenate([blobs(sizes, 0.01, seed=21)[0], serpentine(150, 0.01) + np.float32([0, 0.2, 0]),
                         _cube(7, seed=21, fill=0.01)])
    n = pc.shape[0]
    perm = np.random.default_rng(22).permutation(n)
    a = _check_cluster(pc, [0], [n], 0.01, min_points=1, max_labels=64)
    b = _check_cluster(pc[perm], [0], [n], 0.01, min_points=1, max_labels=64)
    assert a["num_labels"][0] == 48
    back = {frozenset(perm[list(rows)].tolist()) for rows in ref.partition(b["labels"])}   # as sets of SOURCE rows
    assert back == ref.partition(a["labels"]) and len(back) == a["num_labels"][0] > 5
    assert not np.array_equal(a["label_root"], b["label_root"])      # the labels follow the new lowest rows
    assert np.array_equal(a["label_points"], b["label_points"])


def test_split_labels_on_hand_written_labels():
    rng = np.random.default_rng(31)
    clouds = [rng.normal(size=(n, 3)).astype(np.float32) for n in (0, 1, 255, 256, 257, 1000)]
    points, start, count = _ragged(clouds, fill=7.0)
    rows = points.shape[0]
    labels = rng.integers(-2, 9, rows).astype(np.int32)        # -2 .. 8: 0, negatives and values above max_labels = 5
    labels[rng.integers(0, rows, 20)] = np.iinfo(np.int32).min
    labels[rng.integers(0, rows, 20)] = np.iinfo(np.int32).max
    got = _check_split(points, labels, start, count, 5)
    assert got["obj_count"][0].tolist() == [0] * 5 and got["obj_count"][-1].min() > 50
    assert got["out_total"] == sum(((labels[s:s + c] >= 1) & (labels[s:s + c] <= 5)).sum() for s, c in zip(start, count))
    _check_split(points, labels, start + [rows - 3], count + [10], 8)          # a range that leaves the array: empty
    _check_split(points, labels, start, count, 64)
    _check_split(points, labels, start, count, 1)
    one = np.full(rows, 3, dtype=np.int32)                                         # one label everywhere: every rank is used
    got = _check_split(points, one, start, count, 4)
    assert np.array_equal(got["obj_count"][:, 2], np.asarray(count)) and got["obj_count"][:, [0, 1, 3]].sum() == 0
    got = _check_split(points, np.zeros(rows, np.int32), start, count, 4)
    assert got["out_total"] == 0 and got["obj_start"].sum() == 0
    got = _check_split(points, labels, [3, 9], [0, 0], 4)                          # every cloud empty
    assert got["out_total"] == 0 and got["obj_count"].sum() == 0


def test_python_layer_dense_batches_and_the_hand_over_to_the_ragged_entries():
    from graspldm_amd.pointcloud import cluster_cloud, regularize_objects, split_labels
    pts, owner = blobs([40, 25, 60, 3], 0.01, seed=8)
    dev = torch.from_numpy(pts).cuda()
    labels, num, sizes, roots = cluster_cloud(dev, link_dist=0.01, min_points=10, max_objects=5, return_stats=True)
    exp = ref.cluster_one(pts, 0.01, min_points=10, max_labels=5)
    assert labels.dtype == torch.int32 and labels.shape == (128,) and np.array_equal(labels.cpu().numpy(), exp[0])
    assert (num, sizes, roots) == (3, exp[2].tolist(), exp[3].tolist()) and sizes[:3] == [60, 40, 25]
    both = torch.stack([dev, dev.flip(0)])
    lab2, num2 = cluster_cloud(both, link_dist=0.01, min_points=10, max_objects=5)
    assert lab2.shape == (2, 128) and num2 == [3, 3] and np.array_equal(lab2[0].cpu().numpy(), exp[0])
    assert np.array_equal(lab2[1].cpu().numpy(), ref.cluster_one(pts[::-1], 0.01, min_points=10, max_labels=5)[0])
    packed, ostart, ocount, src = split_labels(dev, labels, max_objects=5)
    want = ref.split_labels(pts, exp[0], [0], [128], 5)
    assert packed.cpu().numpy().tobytes() == want["out_points"].tobytes() and np.array_equal(src.cpu().numpy(), want["out_row"])
    assert ostart == want["obj_start"].reshape(-1).tolist() and ocount == want["obj_count"].reshape(-1).tolist()
    assert ocount == [60, 40, 25, 0, 0] and ostart == [0, 60, 100, 125, 125]
    batch = regularize_objects(packed, ostart[:num], ocount[:num], 16)            # straight into the ragged entries
    assert batch.shape == (3, 16, 3)
    for k in range(num):
        obj = set(map(bytes, pts[exp[0] == k + 1].view(np.uint8).reshape(-1, 12)))
        assert all(bytes(r) in obj for r in batch[k].cpu().numpy().view(np.uint8).reshape(-1, 12))
    lab_all, num_all = cluster_cloud(torch.full((10, 3), float("nan")).cuda(), min_points=1)
    assert num_all == 0 and int(lab_all.abs().sum()) == 0
