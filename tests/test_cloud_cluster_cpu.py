"""CPU: the restatement of the Euclidean clustering (tests/cloud_cluster_ref.py) on a hand-made case and against scipy, the
completeness of the 27-cell grid search on adversarial inputs, every envelope of gldm_cluster_cloud and gldm_split_labels
through the C ABI (with pointers that must not be read), the bytes queries, the Python layer's argument errors and the
header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_cluster_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINKS = (1e-3, 0.01, 0.3, 0.0123456789)   # the last: a value not representable in few bits


def _status(name):
    from graspldm_amd import _abi
    return _abi.CONSTANTS[name]


INVALID, UNSUPPORTED, WORKSPACE = (_status("GLDM_ERR_" + n) for n in ("INVALID_ARG", "UNSUPPORTED", "WORKSPACE"))


# ---------------------------------------------------------------------------------------------------- generators --
def _ulps(v, k):
    """v moved by k ulp (f32)."""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def threshold_pairs(link_dist, spacing=8.0):
    """Pairs at f32 distance exactly link_dist, one ulp below and one ulp above, on each axis and on the diagonal, from
    bases at the origin, at exact multiples of the cell size (both signs) and just beside them; the pairs stand `spacing`
    link_dists apart, so only the two rows of a pair can be linked.  -> [2 m, 3] f32: rows 2 i and 2 i + 1 are pair i."""
    link = np.float32(link_dist)
    cs = ref.cell_size(link)
    dirs = [np.array(d, dtype=np.float64) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1))]
    diag = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    bases = [0.0, cs * 3, -cs * 3, float(_ulps(cs * 5, -1)), float(_ulps(-cs * 5, 1)), cs * 2.5, -cs * 7.5]
    pts, at = [], 0
    for base in bases:
        for k in (-1, 0, 1):
            d = np.float64(_ulps(link, k))
            for u in dirs + [diag, -diag]:
                origin = np.zeros(3)   # along an axis the direction has no part in: on an axis the difference stays exact
                origin[int(np.argmin(np.abs(u)))] = at * spacing * float(link)
                a = (origin + base).astype(np.float32)
                b = (a.astype(np.float64) + u * d).astype(np.float32)
                pts += [a, b]
                at += 1
    return np.stack(pts).astype(np.float32)


def straddling_cloud(link_dist, n, seed):
    """Random rows on and beside cell boundaries: lattice nodes k * cs (negative k too) plus offsets of 0, a few ulp and
    fractions of link_dist, so that most linked pairs sit in different cells."""
    rng = np.random.default_rng(seed)
    cs = ref.cell_size(link_dist)
    node = rng.integers(-3, 4, (n, 3)).astype(np.float64) * cs
    frac = rng.choice([0.0, 0.0, 1.0, -1.0, 0.5, -0.5, 0.999, -0.999, 1.0005, -1.0005], (n, 3)) * float(np.float32(link_dist))
    p = (node + frac).astype(np.float32)
    nudge = rng.integers(-2, 3, (n, 3))
    for k in (-2, -1, 1, 2):
        moved = p.copy()
        for _ in range(abs(k)):
            moved = np.nextafter(moved, np.float32(np.inf if k > 0 else -np.inf))
        p = np.where(nudge == k, moved, p)
    return p.astype(np.float32)


def serpentine(n, link_dist, run=40, turn=3, gap_at=None, step=0.95, gap=1.05):
    """A chain of n points `step` link_dists apart, `run` steps along +-x, then `turn` steps along +y, and so on: it winds
    through many cells and its rows are 3 steps (2.85 link_dists) apart, so only chain neighbours are linked.  gap_at: the
    step in front of that point is `gap` link_dists long."""
    link = float(np.float32(link_dist))
    p, pos, direction, left = [], np.zeros(3), 1.0, run
    for i in range(n):
        if i:
            length = (gap if i == gap_at else step) * link
            if left > 0:
                pos = pos + np.array([direction * length, 0.0, 0.0])
                left -= 1
            else:
                pos = pos + np.array([0.0, length, 0.0])
                left -= 1
                if left == -turn:
                    direction, left = -direction, run
        p.append(pos.copy())
    return np.asarray(p).astype(np.float32)


def blobs(sizes, link_dist, seed=0, spacing=5.0):
    """One tight blob per entry of sizes (all its rows within link_dist / 4 of its centre, so it is one component), the
    centres `spacing` link_dists apart on a line, rows of the blobs interleaved at random.  -> (points, blob of every row)."""
    rng = np.random.default_rng(seed)
    link = float(np.float32(link_dist))
    owner = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    centre = np.stack([np.arange(len(sizes)) * spacing * link, np.zeros(len(sizes)), np.zeros(len(sizes))], axis=1)
    p = centre[owner] + rng.uniform(-link / 8, link / 8, (owner.size, 3))
    return p.astype(np.float32), owner


# --------------------------------------------------------------------------------------------------- restatement --
def test_hand_made_dozen_points():
    L = 0.01
    pts = np.array([[0.000, 0, 0], [0.009, 0, 0], [0.018, 0, 0],           # a chain of three: rows 0 1 2
                    [0.100, 0, 0], [0.100, 0.010, 0],                     # a pair exactly link_dist apart (f32: equal squares)
                    [0.200, 0, 0],                                        # alone
                    [0.027, 0, 0],                                        # joins the chain through row 2
                    [0.300, 0, 0], [0.300, 0, 0.0101],                    # just too far: two singles
                    [np.nan, 0, 0],                                       # inactive
                    [0.100, 0.005, 0.002],                                # joins the pair
                    [0.200, 0.0, 0.004]], dtype=np.float32)               # joins row 5
    for search in ("brute", "grid"):
        labels, k, sizes, roots = ref.cluster_one(pts, L, min_points=1, max_labels=8, search=search)
        assert labels.tolist() == [1, 1, 1, 2, 2, 3, 1, 4, 5, 0, 2, 3]
        assert k == 5 and sizes.tolist() == [4, 3, 2, 1, 1, 0, 0, 0] and roots.tolist() == [0, 3, 5, 7, 8, -1, -1, -1]
        labels, k, sizes, roots = ref.cluster_one(pts, L, min_points=2, max_labels=2, search=search)
        assert labels.tolist() == [1, 1, 1, 2, 2, 0, 1, 0, 0, 0, 2, 0] and k == 2 and roots.tolist() == [0, 3]
    out = ref.split_labels(pts, [1, 1, 1, 2, 2, 3, 1, 4, 5, 0, 2, 3], [0], [12], 4)
    assert out["out_row"].tolist() == [0, 1, 2, 6, 3, 4, 10, 5, 11, 7]
    assert out["obj_start"].tolist() == [[0, 4, 7, 9]] and out["obj_count"].tolist() == [[4, 3, 2, 1]] and out["out_total"] == 10


@pytest.mark.parametrize("n,link,seed", [(400, 0.01, 0), (1500, 0.004, 1), (700, 0.3, 2)])
def test_restatement_agrees_with_scipy(n, link, seed):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(seed)
    pc = (rng.uniform(-0.5, 0.5, (n, 3)) * link * n ** (1 / 3) * 1.2).astype(np.float32)
    act = np.ones(n, dtype=bool)
    pairs = ref.pairs_brute(pc, act, ref.link2_of(link))
    graph = sparse.coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    ncomp, comp = csgraph.connected_components(graph, directed=False)
    root = ref.roots_of(n, act, pairs)
    assert 1 < ncomp < n and len(np.unique(root)) == ncomp
    for c in range(ncomp):   # a component of scipy's = the rows of one root, and the root is the lowest of them
        rows = np.flatnonzero(comp == c)
        assert np.all(root[rows] == rows.min())
    labels, k, sizes, roots = ref.rank_components(root, 1, 64)
    order = sorted((-np.sum(comp == c), np.flatnonzero(comp == c).min()) for c in range(ncomp))[:64]
    assert k == min(ncomp, 64) and [(-s, r) for s, r in zip(sizes[:k], roots[:k])] == order


# --------------------------------------------------------------------------------------------- grid completeness --
@pytest.mark.parametrize("link", LINKS)
def test_grid_search_finds_every_threshold_pair(link):
    pts = threshold_pairs(link)
    act = ref.active_rows(pts, link)
    assert act.all()
    link2 = ref.link2_of(link)
    brute, grid = ref.pairs_brute(pts, act, link2), ref.pairs_grid(pts, act, link, link2)
    assert sorted(map(tuple, brute.tolist())) == sorted(map(tuple, grid.tolist()))
    hit = set(map(tuple, brute.tolist()))
    assert all(i == j + 1 and j % 2 == 0 for i, j in hit)             # only the two rows of a pair
    m = pts.shape[0] // 2
    assert m / 4 < len(hit) < m                                        # both sides of the threshold are populated
    origin_axis = [(2 * i + 1, 2 * i) in hit for i in range(24)]       # base 0: k = -1, 0, +1 ulp, 8 directions each
    assert origin_axis[:6] == [True] * 6 and origin_axis[8:14] == [True] * 6 and origin_axis[16:22] == [False] * 6


@pytest.mark.parametrize("link", LINKS)
def test_grid_search_equals_brute_force_on_straddling_clouds(link):
    linked = cross = 0
    for seed in range(12):   # 12 clouds x 300 rows: about 10^5 near pairs per link_dist
        pts = straddling_cloud(link, 300, seed)
        act = ref.active_rows(pts, link)
        link2 = ref.link2_of(link)
        brute, grid = ref.pairs_brute(pts, act, link2), ref.pairs_grid(pts, act, link, link2)
        assert sorted(map(tuple, brute.tolist())) == sorted(map(tuple, grid.tolist()))
        cells = ref.cells_of(pts, link)
        linked += len(brute)
        cross += int(np.any(cells[brute[:, 0]] != cells[brute[:, 1]], axis=1).sum())
        assert np.all(np.abs(cells[brute[:, 0]] - cells[brute[:, 1]]) <= 1)
    assert linked > 2000 and cross > linked // 2   # the generator does its job


@pytest.mark.parametrize("link", LINKS)
def test_random_near_threshold_pairs_never_sit_two_cells_apart(link):
    rng = np.random.default_rng(7)
    n = 4000
    cs = ref.cell_size(link)
    a = (rng.integers(-50, 50, (n, 3)) * cs + rng.uniform(-1, 1, (n, 3)) * float(np.float32(link))).astype(np.float32)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[: n // 2] = np.eye(3)[rng.integers(0, 3, n // 2)] * rng.choice([-1.0, 1.0], (n // 2, 1))   # half of them on an axis
    b = (a.astype(np.float64) + u * float(np.float32(link)) * (1 + rng.integers(-4, 5, (n, 1)) * 2.0 ** -23)).astype(np.float32)
    hit = ref.linked(a, b, ref.link2_of(link))
    assert n / 5 < hit.sum() < n * 4 / 5
    ca, cb = ref.cells_of(a, link), ref.cells_of(b, link)
    assert np.all(np.abs(ca - cb)[hit] <= 1)
    assert np.any(np.abs(ca - cb)[hit] == 1)


def test_active_rule_at_the_lattice_limit_and_the_height_window():
    link = 0.5
    cs = ref.cell_size(link)
    edge_hi, edge_lo = (2 ** 20 - 1) * cs, (-(2 ** 20) + 1) * cs
    pts = np.zeros((8, 3), dtype=np.float32)
    pts[0, 0] = np.float32(edge_hi * (1 - 2e-7))      # cell 2^20 - 2: the last one inside
    pts[1, 1] = np.float32(edge_hi * (1 + 2e-7))      # cell 2^20 - 1: outside
    pts[2, 2] = np.float32(edge_lo * (1 - 2e-7))      # cell -2^20 + 1: the first one inside
    pts[3, 0] = np.float32(edge_lo * (1 + 2e-7))      # cell -2^20: outside
    pts[4, 1] = np.inf
    pts[5, 2] = np.nan
    pts[6, 0] = np.float32(3e38)
    cells = ref.cells_of(pts, link)
    assert cells[0, 0] == 2 ** 20 - 2 and cells[1, 1] >= 2 ** 20 - 1 and cells[2, 2] == -2 ** 20 + 1 and cells[3, 0] <= -2 ** 20
    assert ref.active_rows(pts, link).tolist() == [True, False, True, False, False, False, False, True]
    plane, h0, h1 = (0.0, 0.0, 1.0, 0.0), np.float32(0.01), np.float32(0.5)
    z = np.array([h0, np.nextafter(h0, np.float32(1)), h1, np.nextafter(h1, np.float32(1)), 0.2, -0.2], dtype=np.float32)
    pts = np.stack([np.zeros(6), np.zeros(6), z], axis=1).astype(np.float32)
    assert ref.active_rows(pts, link, plane, h0, h1).tolist() == [False, True, True, False, True, False]
    assert ref.active_rows(pts, link).all()


# ------------------------------------------------------------------------------------------------------ the C ABI --
@pytest.fixture(scope="module")
def lib():
    from graspldm_amd import _lib
    return _lib.lib()


BAD = ctypes.c_void_p(0x10)   # a pointer that must not be read (16-byte aligned, like a workspace)


def _cluster(lib, b=1, n_max=10, rows=10, link=0.01, plane=None, h=(0.0, 1.0), min_points=1, max_labels=4, ws=BAD,
             ws_bytes=1 << 40, ptr=BAD):
    return lib.gldm_cluster_cloud(ptr, ptr, ptr, b, n_max, rows, link, plane, h[0], h[1], min_points, max_labels, ws, ws_bytes,
                                  ptr, ptr, ptr, ptr, None)


def _split(lib, b=1, n_max=10, rows=10, max_labels=4, ws=BAD, ws_bytes=1 << 40, ptr=BAD):
    return lib.gldm_split_labels(ptr, ptr, ptr, ptr, b, n_max, rows, max_labels, ws, ws_bytes, ptr, ptr, ptr, ptr, ptr, None)


def test_cluster_cloud_refuses_every_envelope_before_any_pointer(lib):
    for kw in (dict(b=0), dict(b=-1), dict(n_max=-1), dict(rows=-1), dict(min_points=0), dict(min_points=-3),
               dict(max_labels=0), dict(max_labels=-1), dict(link=0.0), dict(link=-0.01), dict(link=float("inf")),
               dict(link=float("nan")), dict(link=2.0 ** -61), dict(link=2.0 ** 61)):
        assert _cluster(lib, **kw) == INVALID, kw
    for kw in (dict(b=65536), dict(n_max=(1 << 22) + 1), dict(rows=(1 << 24) + 1), dict(max_labels=65)):
        assert _cluster(lib, **kw) == UNSUPPORTED, kw
    nan_plane = (ctypes.c_float * 4)(0.0, float("nan"), 1.0, 0.0)
    good_plane = (ctypes.c_float * 4)(0.0, 0.0, 1.0, 0.0)
    assert _cluster(lib, plane=nan_plane) == INVALID
    assert _cluster(lib, plane=good_plane, h=(0.5, 0.5)) == INVALID
    assert _cluster(lib, plane=good_plane, h=(0.5, float("nan"))) == INVALID
    assert _cluster(lib, ptr=None) == INVALID                                   # null pointers
    assert _cluster(lib, ws=None) == INVALID
    assert _cluster(lib, ws=ctypes.c_void_p(0x18)) == INVALID                   # not 16-byte aligned
    need = lib.gldm_cluster_cloud_workspace_bytes(1, 10, 10)
    assert need > 0 and _cluster(lib, ws_bytes=need - 1) == WORKSPACE
    assert _cluster(lib, b=65535, n_max=1 << 22, rows=1 << 24, link=2.0 ** -60, max_labels=64, ws_bytes=0) == WORKSPACE


def test_split_labels_refuses_every_envelope_before_any_pointer(lib):
    for kw in (dict(b=0), dict(b=-1), dict(n_max=-1), dict(rows=-1), dict(max_labels=0), dict(max_labels=-2)):
        assert _split(lib, **kw) == INVALID, kw
    for kw in (dict(b=65536), dict(n_max=(1 << 22) + 1), dict(rows=(1 << 24) + 1), dict(max_labels=65),
               dict(b=17, n_max=1 << 22, rows=1 << 24, max_labels=64),         # 17 * 16384 * 64 > 2^24 counters
               dict(b=65535, n_max=1025, max_labels=64, rows=1 << 20)):        # 65535 * 5 * 64 > 2^24
        assert _split(lib, **kw) == UNSUPPORTED, kw
    assert _split(lib, ptr=None) == INVALID
    assert _split(lib, ws=None) == INVALID
    need = lib.gldm_split_labels_workspace_bytes(1, 10, 10, 4)
    assert need > 0 and _split(lib, ws_bytes=need - 1) == WORKSPACE
    assert _split(lib, b=1, n_max=1 << 22, rows=1 << 22, max_labels=64, ws_bytes=0) == WORKSPACE    # inside the envelope
    assert _split(lib, b=256, n_max=8192, rows=1 << 21, max_labels=64, ws_bytes=0) == WORKSPACE
    assert _split(lib, b=65535, n_max=256, rows=1 << 24, max_labels=4, ws_bytes=0) == WORKSPACE


def test_bytes_queries_grow_with_every_argument_and_refuse_the_envelopes(lib):
    cb, sb = lib.gldm_cluster_cloud_workspace_bytes, lib.gldm_split_labels_workspace_bytes
    assert cb(0, 10, 10) == INVALID and cb(1, -1, 10) == INVALID and cb(1, 10, -1) == INVALID
    assert cb(65536, 10, 10) == UNSUPPORTED and cb(1, (1 << 22) + 1, 10) == UNSUPPORTED and cb(1, 10, (1 << 24) + 1) == UNSUPPORTED
    assert sb(0, 10, 10, 4) == INVALID and sb(1, 10, 10, 0) == INVALID and sb(1, 10, 10, 65) == UNSUPPORTED
    assert sb(17, 1 << 22, 1 << 24, 64) == UNSUPPORTED and sb(16, 1 << 22, 1 << 24, 64) == 1 << 26
    last = 0
    for rows in (0, 1, 255, 256, 257, 10000, 1 << 20, 1 << 24):
        now = cb(1, min(rows, 1 << 22), rows)
        assert now > last and now % 16 == 0 and now >= 84 * rows
        last = now
    assert cb(2, 1000, 5000) > cb(1, 1000, 5000) and cb(1, 2000, 5000) > cb(1, 1000, 5000)
    assert cb(65535, 1 << 22, 1 << 24) > (1 << 32)          # long long, no overflow
    assert sb(1, 0, 0, 4) == 0
    for args, counters in (((1, 1 << 22, 1 << 22, 64), 1 << 20), ((256, 8192, 1 << 21, 64), 1 << 19), ((3, 257, 900, 5), 30)):
        assert sb(*args) == 4 * counters
    assert sb(2, 300, 600, 8) > sb(1, 300, 600, 8) and sb(1, 600, 600, 8) > sb(1, 300, 600, 8) and sb(1, 300, 600, 9) > sb(1, 300, 600, 8)


# ------------------------------------------------------------------------------------------------ the Python layer --
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


def test_cluster_cloud_argument_errors_come_before_the_library(no_library):
    P = no_library
    pts = torch.zeros(10, 3)
    for v in (0.0, -1.0, float("inf"), float("nan"), 1e-50, 1e39, 2.0 ** -61, None, "x", True):
        with pytest.raises(ValueError, match="link_dist"):
            P.cluster_cloud(pts, link_dist=v)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="max_objects"):
            P.cluster_cloud(pts, max_objects=k)
    with pytest.raises(ValueError, match="min_points"):
        P.cluster_cloud(pts, min_points=0)
    with pytest.raises(ValueError, match="plane must hold 4"):
        P.cluster_cloud(pts, plane=[0, 0, 1])
    with pytest.raises(ValueError, match="height_range"):
        P.cluster_cloud(pts, plane=[0, 0, 1, 0], height_range=(0.5, 0.1))
    with pytest.raises(ValueError, match="finite"):
        P.cluster_cloud(pts, plane=[0, float("nan"), 1, 0])
    with pytest.raises(ValueError, match="go together"):
        P.cluster_cloud(pts, start=[0])
    with pytest.raises(ValueError, match="overlap"):
        P.cluster_cloud(pts, start=[0, 3], count=[4, 4])
    with pytest.raises(ValueError, match="leave points"):
        P.cluster_cloud(pts, start=[4], count=[7])
    with pytest.raises(NotImplementedError, match="65535"):
        P.cluster_cloud(pts, start=[0] * 65536, count=[0] * 65536)
    big = torch.zeros(1, 3).expand((1 << 22) + 1, 3)   # no memory behind it
    with pytest.raises(NotImplementedError, match=r"gldm_cluster_cloud takes at most 2\^22"):
        P.cluster_cloud(big, start=[0], count=[(1 << 22) + 1])
    big = torch.zeros(1, 3).expand((1 << 24) + 1, 3)
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        P.cluster_cloud(big, start=[0], count=[5])
    with pytest.raises(AssertionError, match="library was touched"):   # inside the envelope the call goes on
        P.cluster_cloud(pts)
    nan = torch.full((10, 3), float("nan"))
    with pytest.raises(AssertionError, match="library was touched"):   # non-finite rows are inactive, not an error
        P.cluster_cloud(nan)


def test_split_labels_segment_cloud_and_fit_plane_argument_errors(no_library):
    P = no_library
    pts = torch.zeros(10, 3)
    lab = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(ValueError, match="max_objects"):
        P.split_labels(pts, lab, max_objects=65)
    with pytest.raises(ValueError, match="integer tensor of 10"):
        P.split_labels(pts, lab[:9])
    with pytest.raises(ValueError, match="integer tensor"):
        P.split_labels(pts, lab.float())
    rows = (1 << 24) + 1   # no memory behind either tensor
    with pytest.raises(NotImplementedError, match=r"gldm_split_labels takes at most 2\^24"):
        P.split_labels(torch.zeros(1, 3).expand(rows, 3), torch.zeros(1, dtype=torch.int32).expand(rows), start=[0], count=[5])
    rows = (1 << 22) + 16   # one cloud of 2^22 rows and 16 of one: 17 * 16384 * 64 counters
    with pytest.raises(NotImplementedError, match=r"max_objects <= 2\^24"):
        P.split_labels(torch.zeros(1, 3).expand(rows, 3), torch.zeros(1, dtype=torch.int32).expand(rows),
                       start=[0] + [(1 << 22) + i for i in range(16)], count=[1 << 22] + [1] * 16)
    with pytest.raises(AssertionError, match="library was touched"):
        P.split_labels(pts, lab)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        P.segment_cloud(torch.zeros(2, 10, 3))
    with pytest.raises(ValueError, match="takes no plane"):
        P.segment_cloud(pts, plane=[0, 0, 1, 0], table=False)
    with pytest.raises(ValueError, match="link_dist"):
        P.segment_cloud(pts, link_dist=0.0)
    with pytest.raises(ValueError, match="max_objects"):
        P.segment_cloud(pts, max_objects=0)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        P.fit_plane(torch.zeros(10, 2))
    with pytest.raises(ValueError, match="hypotheses"):
        P.fit_plane(pts, hypotheses=0)
    with pytest.raises(ValueError, match="hypotheses"):
        P.fit_plane(pts, hypotheses=4097)
    with pytest.raises(ValueError, match="needs 3"):
        P.fit_plane(pts[:2])
    with pytest.raises(ValueError, match="view_point"):
        P.fit_plane(pts, view_point=[0, 0])
    with pytest.raises(ValueError, match="view_point"):
        P.fit_plane(pts, view_point=[0, float("inf"), 0])


def test_header_states_the_contract_and_the_abi_stays_15():
    from graspldm_amd import _abi
    text = open(os.path.join(ROOT, "include", "gldm.h")).read()
    protos, _, consts = _abi.parse(text)
    assert consts["GLDM_ABI_VERSION"] == 15
    ret, args = protos["gldm_cluster_cloud"]
    assert ret is ctypes.c_int and len(args) == 19 and args[6] is ctypes.c_float and args[3:6] == [ctypes.c_int] * 3
    assert args[8:10] == [ctypes.c_float] * 2 and args[10:12] == [ctypes.c_int] * 2 and args[13] is ctypes.c_longlong
    assert protos["gldm_cluster_cloud_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    ret, args = protos["gldm_split_labels"]
    assert ret is ctypes.c_int and len(args) == 16 and args[4:8] == [ctypes.c_int] * 4
    assert protos["gldm_split_labels_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 4)
    section = text[text.index("Euclidean clustering"):text.index("gldm_split_labels_workspace_bytes(int b")]
    for words in (r"cs = \(double\)link_dist \* \(1 \+ 2\^-10\)", r"strictly inside \(-2\^20, 2\^20 - 1\)",
                  r"hgt > h_min && hgt <= h_max", r"\(\(dx\*dx \+ dy\*dy\) \+ dz\*dz\) <= link2",
                  r"root of a component is its lowest row", r"falling size, ties to the lower root",
                  r"Why the grid may not lose a link", r"\|D\| < cs \* \(1 - 2\^-11\)", r"at most 2\^-33 absolute error",
                  r"floors differ by at most 1", r"downsample first", r"cloud-major, then by ascending label, then by ascending row",
                  r"count of 0 keeps the running start"):
        assert re.search(words, section), words
    src = open(os.path.join(ROOT, "graspldm_amd", "csrc", "Makefile")).read()
    assert "cloud_cluster.hip" in re.search(r"^SRCS_STRICT := (.*)$", src, re.M).group(1).split()
    for name in ("cloud_downsample.hip", "cloud_cluster.hip"):   # the shared hash lives in one place
        body = open(os.path.join(ROOT, "graspldm_amd", "csrc", name)).read()
        assert '#include "voxel_hash.h"' in body and "0xbf58476d1ce4e5b9" not in body
    for name in ("tabletop.hip", "cloud_cluster.hip"):            # ... and so does the union-find
        body = open(os.path.join(ROOT, "graspldm_amd", "csrc", name)).read()
        assert '#include "components.h"' in body and "atomicMin(&par[" not in body


# ---------------------------------------------------------------------------------------------------------- the CLI --
def _cli():
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("generate_grasps_cli_cluster", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        spec.loader.exec_module(cli)
    finally:
        sys.path.pop(0)
    return cli


def test_cli_segment_cloud_flags_and_their_exclusions():
    from graspldm_amd.grasp_select import CloudCleanup, CloudDownsample
    cli = _cli()
    scene = ["--exp_path", "x", "--pc_file", "scene.npy", "--num_points", "1024", "--segment_cloud"]
    args = cli.parse_args(scene)
    assert args.segment_cloud and cli.cloud_segmentation_options(args) == {}
    assert cli.cleanup_options(args) == {} and cli.downsample_options(args) == {}
    args = cli.parse_args(scene + ["--table_tol", "0.004", "--object_height", "0.02", "0.3", "--link_dist", "0.008",
                                   "--ransac_hypotheses", "256", "--segment_seed", "5", "--min_cluster_points", "20",
                                   "--min_object_points", "64", "--voxel_size", "0.003", "--voxel_max_points", "50000",
                                   "--downsample_scene", "--remove_outliers", "--outlier_k", "6", "--clean_scene"])
    opts = cli.cloud_segmentation_options(args)
    rng = opts.pop("rng")
    assert opts == dict(tol=0.004, height_range=(0.02, 0.3), link_dist=0.008, hypotheses=256, min_points=20)
    assert rng.integers(0, 1000, 4).tolist() == np.random.default_rng(5).integers(0, 1000, 4).tolist()
    assert cli.downsample_options(args) == dict(downsample=CloudDownsample(0.003, 50000, True))
    assert cli.cleanup_options(args) == dict(cleanup=CloudCleanup(k=6, apply_to_scene=True))
    assert args.min_object_points == 64
    args = cli.parse_args(scene + ["--no_table_plane", "--link_dist", "0.02"])
    assert cli.cloud_segmentation_options(args) == dict(table=False, link_dist=0.02)
    cloud = ["--exp_path", "x", "--pc_file", "c.npy", "--num_points", "1024"]
    depth = ["--exp_path", "x", "--depth_file", "d.npy", "--camera_json", "c.json"]
    for argv in (["--exp_path", "x", "--pc_file", "c.npy", "--segment_cloud"],                       # no --num_points
                 ["--exp_path", "x", "--num_points", "64", "--segment_cloud"],                       # no --pc_file
                 cloud + ["--pc_file", "d.npy", "--segment_cloud"],                                   # two files
                 depth + ["--segment_cloud"], depth + ["--num_points", "64", "--segment_cloud"],      # a depth frame
                 ["--exp_path", "x", "--synthetic", "64", "--segment_cloud"],
                 scene + ["--synthetic", "64"], scene + ["--refine_from", "g.npy"],
                 cloud + ["--min_cluster_points", "5"], cloud + ["--no_table_plane"],                 # companions alone
                 depth + ["--segment_tabletop", "--min_cluster_points", "5"], depth + ["--no_table_plane"],
                 scene + ["--min_cluster_points", "0"],
                 scene + ["--no_table_plane", "--table_tol", "0.01"], scene + ["--no_table_plane", "--object_height", "0", "1"],
                 scene + ["--no_table_plane", "--segment_seed", "1"], scene + ["--scene_file", "a.npy", "--scene_file", "b.npy"]):
        with pytest.raises(SystemExit) as e:   # argparse's error: exit status 2
            cli.parse_args(argv)
        assert e.value.code == 2, argv
    # what the parser refused before, it still refuses -- with and without the new switch
    for argv in (cloud + ["--remove_outliers"], cloud + ["--outlier_k", "4"], cloud + ["--link_dist", "0.01"],
                 cloud + ["--table_tol", "0.01"], cloud + ["--min_object_points", "5"], cloud + ["--segment_tabletop"],
                 scene + ["--segment_tabletop"], scene + ["--min_object_pixels", "10"], scene + ["--outlier_k", "4"],
                 scene + ["--clean_scene"], scene + ["--camera_json", "c.json"], scene + ["--labels_file", "l.npy"],
                 scene + ["--mask_file", "m.npy"], scene + ["--z_range", "0", "1"], scene + ["--voxel_max_points", "5"],
                 scene + ["--voxel_size", "0"], depth + ["--link_dist", "0.01"], depth + ["--pc_file", "c.npy"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code not in (0, None), argv
