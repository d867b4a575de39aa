#!/usr/bin/env python3
"""Timing of the sensor-cloud cleanup (gldm_neighbor_stats, gldm_filter_outliers in csrc/cloud_filter.hip;
pointcloud.remove_outliers) on one MI355X.  HIP events around warmed calls, medians of --iterations with min-max, as
tools/bench_tabletop.py.  The frame is tools/bench_scene.py's 480 x 640 one: 8 objects of 28800 .. 400 pixels; 1 % of the
object pixels are made flying pixels (a seeded draw, depth 0.4 .. 0.7 m in front of objects at 0.8 m and beyond).  All
three routes filter the same ragged batch (gldm_depth_to_objects' layout) with the same k, radius and min_neighbors.

  gpu       the two bare entries with preallocated buffers: one call per event window, and 50 calls in one window; then
            pointcloud.remove_outliers end to end (allocations, the finite check, the read-back of the counts)
  compose   the route without the new entries that stays on the GPU: per object the existing gldm_knn_radius at k + 1 (it
            returns the point itself), then torch ops for the count, the mean distance, the mask and the compaction
  scan      the two scans alone on the largest object, alternated windows: gldm_neighbor_stats (32-bit keys, no index list)
            against gldm_knn_radius at k + 1 (64-bit keys, idx and d2 out)
  host      read back, scipy cKDTree.query(k + 1, distance_upper_bound), numpy mask, upload -- where scipy is installed

    python tools/bench_cleanup.py --out profiles/cleanup_bench.json"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_scene import H, K, W, make_scene, timed  # noqa: E402
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import _depth_to_objects_packed, knn_radius, remove_outliers  # noqa: E402

FX, FY, CX, CY = 615.3, 615.7, 319.5, 239.5
KNN, RADIUS, MIN_NB = 8, 0.005, 3
BATCH = 50


def make_dirty_scene():
    depth, labels = make_scene()
    rng = np.random.default_rng(2)
    obj = torch.nonzero(labels.reshape(-1) > 0).reshape(-1).numpy()
    fly = rng.choice(obj, obj.shape[0] // 100, replace=False)
    depth.view(-1)[torch.from_numpy(fly)] = torch.from_numpy(rng.uniform(0.4, 0.7, fly.shape[0]).astype(np.float32))
    return depth.contiguous(), labels, int(fly.shape[0])


def per_call(fn, iterations, warmup):
    def many():
        for _ in range(BATCH):
            fn()
    return tuple(v / BATCH for v in timed(many, iterations, warmup))


def bench_gpu(args, out, packed, start, count):
    lib = L.lib()
    dev, rows, b, n_max, total = packed.device, packed.shape[0], len(start), max(count), sum(count)
    sc = torch.tensor([start, count], dtype=torch.int32, device=dev)
    nb1 = lib.gldm_neighbor_stats_workspace_bytes(b, n_max)
    nb2 = lib.gldm_filter_outliers_workspace_bytes(b, n_max)
    ws1 = torch.empty(nb1 // 4 + 1, dtype=torch.float32, device=dev)
    ws2 = torch.empty(nb2 // 8 + 1, dtype=torch.float64, device=dev)
    neighbors = torch.zeros(rows, dtype=torch.int32, device=dev)
    score = torch.zeros(rows, dtype=torch.float32, device=dev)
    outp = torch.empty(total, 3, device=dev)
    kept = torch.empty(total, dtype=torch.int32, device=dev)
    osc = torch.empty(2, b, dtype=torch.int32, device=dev)
    mom = torch.empty(b, 2, dtype=torch.float64, device=dev)
    s = L.current_stream()

    def scan():
        L.call("gldm_neighbor_stats", L.ptr(packed), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, KNN, RADIUS, L.ptr(ws1), nb1,
               L.ptr(neighbors), L.ptr(score), s)

    def filt():
        L.call("gldm_filter_outliers", L.ptr(packed), L.ptr(neighbors), L.ptr(score), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows,
               KNN, MIN_NB, -1.0, L.ptr(ws2), nb2, L.ptr(outp), L.ptr(osc[0]), L.ptr(osc[1]), L.ptr(kept), L.ptr(mom), s)

    res = {}
    for name, fn in (("neighbor_stats", scan), ("filter_outliers", filt)):
        res[name] = dict(one_call_ms=timed(fn, args.iterations, args.warmup),
                         back_to_back_ms_per_call=per_call(fn, args.iterations, args.warmup))
    api = lambda: remove_outliers(packed, k=KNN, max_radius=RADIUS, min_neighbors=MIN_NB, start=start, count=count)   # noqa: E731
    res["remove_outliers_ms"] = [timed(api, args.iterations, args.warmup)]
    out["gpu"] = res
    return api


def compose_route(packed, start, count):
    """The same filter from the existing entry and torch ops -> (points, counts)."""
    outs, counts = [], []
    for s0, c in zip(start, count):
        obj = packed[s0:s0 + c]
        _, d2, found = knn_radius(obj, KNN + 1, RADIUS)
        nb = found - 1                                              # the point itself comes first, at d2 = 0
        dist = torch.sqrt(d2[:, 1:])
        live = torch.arange(KNN, device=obj.device)[None, :] < nb[:, None]
        score = torch.where(live, dist, torch.zeros_like(dist)).double().sum(1) / nb.clamp(min=1)   # noqa: F841 (the scan's second output)
        keep = nb >= MIN_NB
        outs.append(obj[keep])
        counts.append(keep.sum())
    return torch.cat(outs), torch.stack(counts).tolist()


def bench_compose(args, out, packed, start, count, api):
    pts, counts = compose_route(packed, start, count)
    ref_pts, _, ref_counts, _, _ = api()
    assert counts == ref_counts and torch.equal(pts, ref_pts), "the two GPU routes disagree"
    fn = lambda: compose_route(packed, start, count)   # noqa: E731
    a1 = timed(fn, args.iterations, args.warmup)
    b1 = timed(api, args.iterations, args.warmup)
    a2 = timed(fn, args.iterations, 1)
    b2 = timed(api, args.iterations, 1)
    out["compose"] = dict(route="per object gldm_knn_radius at k + 1, torch ops for count, mean, mask, compaction",
                          ms=[a1, a2], remove_outliers_ms_alternated=[b1, b2])


def bench_scan(args, out, packed, start, count):
    lib = L.lib()
    i = int(np.argmax(count))
    obj = packed[start[i]:start[i] + count[i]].contiguous()
    n, dev = obj.shape[0], obj.device
    sc = torch.tensor([[0], [n]], dtype=torch.int32, device=dev)
    nb1 = lib.gldm_neighbor_stats_workspace_bytes(1, n)
    nb2 = lib.gldm_knn_radius_workspace_bytes(1, n)
    ws1 = torch.empty(nb1 // 4 + 1, dtype=torch.float32, device=dev)
    ws2 = torch.empty(nb2 // 4 + 1, dtype=torch.float32, device=dev)
    neighbors = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, KNN + 1, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, KNN + 1, dtype=torch.float32, device=dev)
    found = torch.empty(n, dtype=torch.int32, device=dev)
    s = L.current_stream()

    def stats():
        L.call("gldm_neighbor_stats", L.ptr(obj), L.ptr(sc[0]), L.ptr(sc[1]), 1, n, n, KNN, RADIUS, L.ptr(ws1), nb1,
               L.ptr(neighbors), L.ptr(score), s)

    def knn():
        L.call("gldm_knn_radius", L.ptr(obj), 1, n, KNN + 1, RADIUS, L.ptr(ws2), nb2, L.ptr(idx), L.ptr(d2), L.ptr(found), s)

    stats()
    knn()
    assert torch.equal(neighbors, found - 1), "the two scans disagree on the counts"
    windows = []
    for w in range(3):   # alternated: the spread between windows of the same kernel is the noise floor of the comparison
        windows.append(dict(neighbor_stats_ms_per_call=per_call(stats, args.iterations, args.warmup if w == 0 else 1),
                            knn_radius_ms_per_call=per_call(knn, args.iterations, args.warmup if w == 0 else 1)))
    out["scan"] = dict(points=n, k=KNN, knn_k=KNN + 1, calls_per_window=BATCH, windows=windows)


def host_route(packed, start, count):
    from scipy.spatial import cKDTree
    p = packed.cpu().numpy()   # read back
    outs = []
    for s0, c in zip(start, count):
        obj = p[s0:s0 + c]
        dist, _ = cKDTree(obj).query(obj, k=KNN + 1, distance_upper_bound=RADIUS)
        nb = np.isfinite(dist[:, 1:]).sum(1)
        outs.append(obj[nb >= MIN_NB])
    return torch.from_numpy(np.concatenate(outs)).cuda()   # upload


def bench_host(args, out, packed, start, count, api):
    try:
        import scipy.spatial  # noqa: F401
    except ImportError:
        out["host"] = "not measured: scipy is not installed"
        return
    got = host_route(packed, start, count)
    same = bool(got.shape == api()[0].shape)
    t = []
    for _ in range(max(3, args.iterations // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(packed, start, count)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    out["host"] = dict(route="read back, scipy cKDTree.query(k + 1, distance_upper_bound) per object, numpy mask, upload; "
                             "host clock around a synchronise", same_row_count_as_gpu=same,
                       ms=(float(np.median(t)), float(min(t)), float(max(t))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip", type=str, default="", help="comma list of compose,scan,host")
    ap.add_argument("--time_limit", type=int, default=300, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    cam = Camera.from_intrinsics(FX, FY, CX, CY, W, H)
    depth, labels, flying = make_dirty_scene()
    points, _, starts, counts = _depth_to_objects_packed(depth.cuda(), cam, labels.cuda(), num_labels=K)
    packed, start, count = points[0], starts[0], counts[0]
    out = dict(gpu_name=torch.cuda.get_device_name(), frame=[H, W], objects=K, object_points=count, flying_pixels=flying,
               k=KNN, max_radius=RADIUS, min_neighbors=MIN_NB, iterations=args.iterations)
    skip = set(args.skip.split(","))
    api = bench_gpu(args, out, packed, start, count)
    out["kept_points"] = api()[2]
    if "compose" not in skip:
        bench_compose(args, out, packed, start, count, api)
    if "scan" not in skip:
        bench_scan(args, out, packed, start, count)
    if "host" not in skip:
        bench_host(args, out, packed, start, count, api)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
