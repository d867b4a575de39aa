"""The contracts of gldm_cluster_cloud and gldm_split_labels (include/gldm.h, "Euclidean clustering") in numpy, one f32 (or
f64) operation per step as csrc/cloud_cluster.hip writes them: the active rule, brute-force all-pairs links, a plain
union-find, the ranking by (-size, root), the split by a stable sort on (label, row) -- and, beside the brute-force search,
the GRID search the kernels use (cells by the f64 rule, 27 neighbours), so that its completeness can be put to the test."""
import numpy as np

CELL_LIMIT = float(1 << 20)
MARGIN = 1.0 + 2.0 ** -10


def cell_size(link_dist):
    return np.float64(np.float32(link_dist)) * np.float64(MARGIN)


def link2_of(link_dist):
    return np.float32(link_dist) * np.float32(link_dist)


def cells_of(points, link_dist):
    """floor((double)p / cs) per axis as f64 [n, 3] (NaN / inf stay what they are)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(points, dtype=np.float32).astype(np.float64) / cell_size(link_dist))


def height(points, plane):
    p = np.asarray(points, dtype=np.float32)
    a, b, c, d = (np.float32(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d


def active_rows(points, link_dist, plane=None, h_min=0.0, h_max=0.0):
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    c = cells_of(p, link_dist)
    with np.errstate(invalid="ignore"):
        act = np.isfinite(p).all(axis=1) & ((c > -CELL_LIMIT) & (c < CELL_LIMIT - 1.0)).all(axis=1)
        if plane is not None:
            hgt = height(p, plane)
            act &= (hgt > np.float32(h_min)) & (hgt <= np.float32(h_max))
    return act


def linked(pi, pj, link2):
    """The link test of rows pi [.., 3] against pj [.., 3] (broadcast), f32 op by op."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = pi - pj
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return ((dx * dx + dy * dy) + dz * dz) <= link2


class UnionFind:
    def __init__(self, n):
        self.par = list(range(n))

    def find(self, x):
        root = x
        while self.par[root] != root:
            root = self.par[root]
        while self.par[x] != root:
            self.par[x], x = root, self.par[x]
        return root

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.par[max(a, b)] = min(a, b)   # the lower row stays the root


def pairs_brute(p, act, link2):
    """Every linked pair (i > j) of active rows, by the all-pairs test."""
    idx = np.flatnonzero(act)
    q = p[idx]
    out = []
    for lo in range(0, len(idx), 512):   # blocks of rows: memory stays at 512 x n
        hit = linked(q[lo:lo + 512, None, :], q[None, :, :], link2)
        i, j = np.nonzero(hit)
        keep = (i + lo) > j
        out.append(np.stack([idx[i[keep] + lo], idx[j[keep]]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def pairs_grid(p, act, link_dist, link2):
    """The same pairs as the kernels find them: rows binned by cell, every row against the rows of the 27 cells around it."""
    cells = cells_of(p, link_dist)
    idx = np.flatnonzero(act)
    bins = {}
    for i in idx:
        bins.setdefault(tuple(int(v) for v in cells[i]), []).append(int(i))
    out = []
    offsets = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    for (cx, cy, cz), rows in bins.items():
        near = [j for ox, oy, oz in offsets for j in bins.get((cx + ox, cy + oy, cz + oz), ())]
        near = np.asarray(near, dtype=np.int64)
        mine = np.asarray(rows, dtype=np.int64)
        hit = linked(p[mine][:, None, :], p[near][None, :, :], link2)
        i, j = np.nonzero(hit)
        keep = mine[i] > near[j]
        out.append(np.stack([mine[i[keep]], near[j[keep]]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def roots_of(n, act, pairs):
    """root [n]: the lowest row of every active row's component, -1 for inactive rows."""
    uf = UnionFind(n)
    for i, j in pairs.tolist():
        uf.union(i, j)
    return np.array([uf.find(i) if act[i] else -1 for i in range(n)], dtype=np.int64)


def rank_components(root, min_points, max_labels):
    """-> (labels [n] int32, K, sizes [max_labels] int32, roots [max_labels] int32)."""
    r, size = np.unique(root[root >= 0], return_counts=True)
    order = sorted((int(-s), int(q)) for q, s in zip(r, size) if s >= min_points)[:max_labels]
    labels = np.zeros(root.shape[0], dtype=np.int32)
    sizes = np.zeros(max_labels, dtype=np.int32)
    roots = np.full(max_labels, -1, dtype=np.int32)
    for k, (neg, q) in enumerate(order):
        labels[root == q] = k + 1
        sizes[k], roots[k] = -neg, q
    return labels, len(order), sizes, roots


def cluster_one(points, link_dist, plane=None, h_min=0.0, h_max=0.0, min_points=1, max_labels=64, search="brute"):
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    act = active_rows(p, link_dist, plane, h_min, h_max)
    link2 = link2_of(link_dist)
    pairs = pairs_brute(p, act, link2) if search == "brute" else pairs_grid(p, act, link_dist, link2)
    return rank_components(roots_of(p.shape[0], act, pairs), min_points, max_labels)


def cloud_ranges(start, count, n_max, rows):
    """cloud_range of csrc/ragged_compact.h for every cloud."""
    out = []
    for s, c in zip(start, count):
        n = max(0, min(int(c), n_max))
        if s < 0 or s + n > rows:
            n = 0
        out.append((int(s), n))
    return out


def cluster_cloud(points, start, count, link_dist, plane=None, h_min=0.0, h_max=0.0, min_points=1, max_labels=64,
                  poison=-7, search="brute", n_max=None):
    """The whole entry on a ragged batch -> dict(labels [rows] (poison outside every cloud), num_labels [b], label_points,
    label_root [b, max_labels])."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    rows, b = p.shape[0], len(start)
    n_max = max(count) if n_max is None else n_max
    labels = np.full(rows, poison, dtype=np.int32)
    num = np.zeros(b, dtype=np.int32)
    sizes = np.zeros((b, max_labels), dtype=np.int32)
    roots = np.full((b, max_labels), -1, dtype=np.int32)
    for i, (s, n) in enumerate(cloud_ranges(start, count, n_max, rows)):
        if n:
            labels[s:s + n], num[i], sizes[i], roots[i] = cluster_one(p[s:s + n], link_dist, plane, h_min, h_max, min_points,
                                                                     max_labels, search)
    return dict(labels=labels, num_labels=num, label_points=sizes, label_root=roots)


def split_labels(points, labels, start, count, max_labels, n_max=None):
    """-> dict(out_points [total, 3], out_row [total], obj_start, obj_count [b, max_labels], out_total)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    lab = np.asarray(labels, dtype=np.int32)
    rows, b = p.shape[0], len(start)
    n_max = max(count) if n_max is None else n_max
    pts, src = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.int32)]
    cnt = np.zeros((b, max_labels), dtype=np.int32)
    for i, (s, n) in enumerate(cloud_ranges(start, count, n_max, rows)):
        l = lab[s:s + n]
        keep = np.flatnonzero((l >= 1) & (l <= max_labels))
        order = keep[np.argsort(l[keep], kind="stable")]   # by label, rows ascending inside a label
        pts.append(p[s + order])
        src.append(order.astype(np.int32))
        cnt[i] = np.bincount(l[keep] - 1, minlength=max_labels)
    flat = cnt.reshape(-1).astype(np.int64)
    start_out = (np.cumsum(flat) - flat).astype(np.int32).reshape(b, max_labels)
    return dict(out_points=np.concatenate(pts), out_row=np.concatenate(src), obj_start=start_out, obj_count=cnt,
                out_total=np.int32(flat.sum()))


def partition(labels):
    """The labelled rows as a set of frozensets of rows (label 0 left out): what must survive a shuffle."""
    lab = np.asarray(labels)
    return {frozenset(np.flatnonzero(lab == k).tolist()) for k in np.unique(lab) if k > 0}
