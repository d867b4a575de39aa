"""Restatement of the definition of csrc/cloud_downsample.hip (include/gldm.h, "voxel-grid downsampling"), with none of the
kernels' machinery (no hash table, no atomics, no chunks, no scan).  A helper for test_cloud_downsample_cpu.py /
test_cloud_downsample_gpu.py / test_downsample_e2e_gpu.py, like cloud_filter_ref.py.

  quantise          per point and axis in f64: t = p / voxel_size, cell = floor(t), q = rint(t * 65536) (round-half-even)
  downsample_cloud  one cloud: np.unique on the cell triples, exact int64 sums of q, the voxels ordered by `first`, the
                    header's centroid expression
  voxel_downsample  every cloud of a ragged batch; everything the entry returns
"""
import numpy as np

Q_SCALE = np.float64(65536.0)
CELL_LIMIT = 1 << 20


def quantise(pc, voxel_size):
    """pc f32 [n,3] -> (cell int64 [n,3], q int64 [n,3]); the entry takes voxel_size as f32 and widens it."""
    v = np.float64(np.float32(voxel_size))
    t = np.asarray(pc, dtype=np.float32).astype(np.float64) / v          # IEEE division
    assert np.all(np.abs(t) < CELL_LIMIT), "the precondition |p| / voxel_size < 2^20"
    return np.floor(t).astype(np.int64), np.rint(t * Q_SCALE).astype(np.int64)


def downsample_cloud(pc, voxel_size):
    """One cloud pc [n,3] -> dict: points f32 [m,3], first int32 [m], members int32 [m], voxel int32 [n], cell int64 [m,3]."""
    pc = np.ascontiguousarray(np.asarray(pc, dtype=np.float32)).reshape(-1, 3)
    n = pc.shape[0]
    if n == 0:
        return dict(points=np.zeros((0, 3), np.float32), first=np.zeros(0, np.int32), members=np.zeros(0, np.int32),
                    voxel=np.zeros(0, np.int32), cell=np.zeros((0, 3), np.int64))
    v = np.float64(np.float32(voxel_size))
    cell, q = quantise(pc, voxel_size)
    uniq, first, inverse, members = np.unique(cell, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")                # ascending `first` = order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    sum_q = np.zeros((uniq.shape[0], 3), dtype=np.int64)
    np.add.at(sum_q, inverse, q)                            # exact integer sums
    m = members.astype(np.float64)[:, None]
    centroid = ((sum_q.astype(np.float64) / m) / Q_SCALE * v).astype(np.float32)
    return dict(points=centroid[order], first=first[order].astype(np.int32), members=members[order].astype(np.int32),
                voxel=rank[inverse].astype(np.int32), cell=uniq[order])


def voxel_downsample(points, start, count, voxel_size):
    """The ragged batch: points [rows,3], start / count: b ints.  -> dict: out_points f32 [total,3], out_start / out_count
    int32 [b], first / members int32 [total], voxel int32 [rows] (-1 outside every cloud), cell int64 [total,3]."""
    points = np.asarray(points, dtype=np.float32)
    rows = points.shape[0]
    voxel = np.full(rows, -1, dtype=np.int32)
    parts = []
    for s, c in zip(start, count):
        d = downsample_cloud(points[s:s + c], voxel_size)
        voxel[s:s + c] = d["voxel"]
        parts.append(d)
    ocount = np.asarray([d["first"].shape[0] for d in parts], dtype=np.int32)
    ostart = (np.cumsum(ocount) - ocount).astype(np.int32)
    cat = lambda key, shape: np.concatenate([d[key] for d in parts]).reshape(shape)   # noqa: E731
    return dict(out_points=cat("points", (-1, 3)), out_start=ostart, out_count=ocount, first=cat("first", -1),
                members=cat("members", -1), voxel=voxel, cell=cat("cell", (-1, 3)))
