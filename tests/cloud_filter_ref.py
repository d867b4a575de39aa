"""Restatement of the definitions of csrc/cloud_filter.hip (include/gldm.h, "sensor-cloud cleanup"), point by point and with
none of the kernels' shortcuts (no chunks of candidates, no boxes, no sorted registers, no scan).  A helper for
test_cloud_filter_cpu.py / test_cloud_filter_gpu.py / test_cleanup_e2e_gpu.py, like normals_ref.py.

  neighbor_stats   full pairwise d2 in f32 in the header's operation order, a sort, the f64 sum in ascending d2
  cloud_moments    N, mu, sigma over the points with enough neighbours: f64, the fixed tree inside every 256-row chunk, then
                   the chunks in ascending order, two passes
  filter_outliers  the mask and the ordered compaction of every cloud of a ragged batch; everything the entries return
"""
import numpy as np

CHUNK = 256


def neighbor_stats(pc, k, max_radius, rows=512):
    """One cloud pc [n,3] -> (neighbors int32 [n], score f32 [n]): gldm_neighbor_stats' definition."""
    pc = np.ascontiguousarray(np.asarray(pc, dtype=np.float32)).reshape(-1, 3)
    n = pc.shape[0]
    r2 = np.float32(max_radius) * np.float32(max_radius)
    neighbors = np.zeros(n, dtype=np.int32)
    score = np.full(n, np.inf, dtype=np.float32)
    for r0 in range(0, n, rows):
        q = pc[r0:r0 + rows]
        d = pc[None, :, :] - q[:, None, :]                                             # f32, differences first
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]   # one f32 rounding per operation
        assert d2.dtype == np.float32
        inside = d2 <= r2
        inside[np.arange(q.shape[0]), r0 + np.arange(q.shape[0])] = False              # j != i by index
        s = np.sort(np.where(inside, d2, np.float32(np.inf)), axis=-1)[:, :k]          # ascending d2
        cnt = np.minimum(inside.sum(-1), k).astype(np.int32)
        neighbors[r0:r0 + q.shape[0]] = cnt
        for i in range(q.shape[0]):
            if cnt[i]:
                total = np.float64(0.0)
                for v in s[i, :cnt[i]]:
                    total = total + np.float64(np.sqrt(v, dtype=np.float32))           # sqrtf, then widened
                score[r0 + i] = np.float32(total / np.float64(cnt[i]))
    return neighbors, score


def chunk_tree_sum(v):
    """v f64 [256] -> the sum in the kernel's fixed tree: a fold of each 64 values with offsets 32, 16, .. 1 (what the
    butterfly leaves in lane 0; a + b = b + a), then (w0 + w1) + (w2 + w3)."""
    a = np.asarray(v, dtype=np.float64).reshape(4, 64)
    off = 32
    while off:
        a = a[:, :off] + a[:, off:2 * off]
        off //= 2
    w = a[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def _chunked_sum(values, valid):
    """values f64 [n], valid bool [n]: the invalid rows count as +0.0; tree inside every chunk, chunks ascending."""
    n = values.shape[0]
    total = np.float64(0.0)
    for p0 in range(0, n, CHUNK):
        v = np.zeros(CHUNK, dtype=np.float64)
        m = min(CHUNK, n - p0)
        v[:m] = np.where(valid[p0:p0 + m], values[p0:p0 + m], 0.0)
        total = total + chunk_tree_sum(v)
    return total


def cloud_moments(neighbors, score, min_neighbors):
    """-> (N, mu, sigma) of one cloud over the points with neighbors >= max(min_neighbors, 1)."""
    valid = neighbors >= max(int(min_neighbors), 1)
    n = int(valid.sum())
    sc = score.astype(np.float64)
    sc = np.where(valid, sc, 0.0)   # +inf of a point without neighbours never enters
    mu = _chunked_sum(sc, valid) / np.float64(n) if n > 0 else np.float64(0.0)
    d = sc - mu
    sigma = np.sqrt(_chunked_sum(d * d, valid) / np.float64(n - 1)) if n >= 2 else np.float64(0.0)
    return n, np.float64(mu), np.float64(sigma)


def keep_mask(neighbors, score, min_neighbors, std_ratio, mu, sigma):
    keep = neighbors >= int(min_neighbors)
    if std_ratio is not None and std_ratio >= 0:
        thr = mu + np.float64(np.float32(std_ratio)) * sigma   # the entry takes std_ratio as f32
        keep &= (neighbors >= 1) & (score.astype(np.float64) <= thr)
    return keep


def filter_outliers(points, start, count, k, max_radius, min_neighbors, std_ratio=None):
    """The ragged batch: points [rows,3], start / count: b ints.  -> dict: neighbors int32 [rows] and score f32 [rows] (0 /
    +inf outside every cloud), stats f64 [b,2], out_points f32 [total,3], out_start / out_count int32 [b], kept int32 [total]."""
    points = np.asarray(points, dtype=np.float32)
    rows, b = points.shape[0], len(start)
    neighbors = np.zeros(rows, dtype=np.int32)
    score = np.full(rows, np.inf, dtype=np.float32)
    stats = np.zeros((b, 2), dtype=np.float64)
    out, kept, ocount = [], [], []
    for i, (s, c) in enumerate(zip(start, count)):
        nb, sc = neighbor_stats(points[s:s + c], k, max_radius)
        neighbors[s:s + c], score[s:s + c] = nb, sc
        _, mu, sigma = cloud_moments(nb, sc, min_neighbors)
        stats[i] = mu, sigma
        keep = np.nonzero(keep_mask(nb, sc, min_neighbors, std_ratio, mu, sigma))[0]
        out.append(points[s:s + c][keep])
        kept.append(keep.astype(np.int32))
        ocount.append(keep.shape[0])
    ocount = np.asarray(ocount, dtype=np.int32)
    ostart = (np.cumsum(ocount) - ocount).astype(np.int32)
    return dict(neighbors=neighbors, score=score, stats=stats, out_points=np.concatenate(out).reshape(-1, 3),
                out_start=ostart, out_count=ocount, kept=np.concatenate(kept))
