#!/usr/bin/env python3
"""Timing of the Euclidean clustering (gldm_cluster_cloud, gldm_split_labels in csrc/cloud_cluster.hip;
pointcloud.cluster_cloud / split_labels / segment_cloud) on one MI355X.  HIP events around warmed calls, medians of
--iterations with min-max, as tools/bench_tabletop.py, whose 480 x 640 table scene it uses -- seen twice: camera A is that
frame; camera B is the same surfaces with its own millimetre of seeded depth noise from a pose 1.1 mm beside A's, so that
its points fall between A's.  Both go through depth_to_cloud with their cam_to_world, are concatenated and shuffled: a
fused scene without a pixel grid, twice the density of one frame.

  raw       the fused cloud as it is (about 5 * 10^5 rows, some 40 of them per 1 cm cell)
  voxel3mm  the same after pointcloud.voxel_downsample at 3 mm, the advised order
  per variant:
    entry   the bare gldm_cluster_cloud under the fitted table plane (eleven launches), preallocated buffers: one call per
            event window, and 20 calls in one window (per call: the kernels without the launch gaps of a lone call)
    split   the bare gldm_split_labels on those labels, the same two ways
    api     cluster_cloud and segment_cloud(plane=None) end to end (allocations, the fit, the read-backs)
    host    the route without these entries: read the cloud back, height mask, scipy.spatial.cKDTree.query_pairs,
            scipy.sparse.csgraph.connected_components, size ranking, upload -- where scipy is installed; its partition is
            checked against the entry's

    python tools/bench_cluster.py --out profiles/cluster_bench.json"""
import argparse
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_scene import H, W, timed  # noqa: E402
from bench_tabletop import CX, CY, FX, FY, make_table_scene  # noqa: E402
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import (cluster_cloud, depth_to_cloud, fit_plane, segment_cloud,  # noqa: E402
                                     voxel_downsample)

T, TOL = 512, 0.005
LINK, HEIGHT, MIN_POINTS, MAX_LABELS = 0.01, (0.01, 0.8), 32, 64
VOXEL = 0.003
BATCH = 20


def make_fused_scene():
    """-> the fused, shuffled cloud [n, 3] on the device."""
    cam = Camera.from_intrinsics(FX, FY, CX, CY, W, H)
    depth_a, _ = make_table_scene()
    noise = torch.from_numpy(np.random.default_rng(7).normal(0.0, 0.001, (H, W)).astype(np.float32))
    depth_b = torch.where(depth_a > 0, depth_a + noise, depth_a)
    pose_b = torch.eye(4)
    pose_b[0, 3], pose_b[1, 3] = 0.0011, 0.0011
    a = depth_to_cloud(depth_a.cuda(), cam, cam_to_world=torch.eye(4))
    b = depth_to_cloud(depth_b.cuda().contiguous(), cam, cam_to_world=pose_b)
    cloud = torch.cat([a, b])
    perm = torch.from_numpy(np.random.default_rng(8).permutation(cloud.shape[0])).cuda()
    return cloud[perm].contiguous()


def per_call(fn, iterations, warmup):
    """BATCH calls back to back inside one event window -> (median, min, max) ms per call."""
    def many():
        for _ in range(BATCH):
            fn()
    return tuple(v / BATCH for v in timed(many, iterations, warmup))


def bench_entry(args, cloud, plane):
    lib = L.lib()
    n = cloud.shape[0]
    sc = torch.tensor([[0], [n]], dtype=torch.int32, device="cuda")
    nb = lib.gldm_cluster_cloud_workspace_bytes(1, n, n)
    ws = torch.empty(nb // 8 + 2, dtype=torch.int64, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    stats = torch.empty(1 + 2 * MAX_LABELS, dtype=torch.int32, device="cuda")
    pl = (ctypes.c_float * 4)(*plane.as_array())
    s = L.current_stream()

    def entry():
        L.call("gldm_cluster_cloud", L.ptr(cloud), L.ptr(sc[0]), L.ptr(sc[1]), 1, n, n, LINK, pl, HEIGHT[0], HEIGHT[1], MIN_POINTS,
               MAX_LABELS, L.ptr(ws), nb, L.ptr(labels), L.ptr(stats[0:1]), L.ptr(stats[1:1 + MAX_LABELS]),
               L.ptr(stats[1 + MAX_LABELS:]), s)

    t_one = timed(entry, args.iterations, args.warmup)
    t_many = per_call(entry, args.iterations, args.warmup)
    host = stats.tolist()
    k = host[0]
    nbs = lib.gldm_split_labels_workspace_bytes(1, n, n, MAX_LABELS)
    wss = torch.empty(nbs // 8 + 2, dtype=torch.int64, device="cuda")
    packed = torch.empty(n, 3, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    tab = torch.empty(2 * MAX_LABELS + 1, dtype=torch.int32, device="cuda")

    def split():
        L.call("gldm_split_labels", L.ptr(cloud), L.ptr(labels), L.ptr(sc[0]), L.ptr(sc[1]), 1, n, n, MAX_LABELS, L.ptr(wss), nbs,
               L.ptr(packed), L.ptr(src), L.ptr(tab[:MAX_LABELS]), L.ptr(tab[MAX_LABELS:2 * MAX_LABELS]),
               L.ptr(tab[2 * MAX_LABELS:]), s)

    s_one = timed(split, args.iterations, args.warmup)
    s_many = per_call(split, args.iterations, args.warmup)
    assert tab.tolist()[-1] == sum(host[1:1 + k])
    res = dict(points=n, active_rows_labelled=sum(host[1:1 + k]), launches=11, num_labels=k, label_points=host[1:1 + k],
               workspace_bytes=nb, one_call_ms=t_one, back_to_back_ms_per_call=t_many,
               split=dict(launches=4, one_call_ms=s_one, back_to_back_ms_per_call=s_many))
    return res, labels


def bench_api(args, cloud, plane):
    kw = dict(link_dist=LINK, min_points=MIN_POINTS, height_range=HEIGHT)
    t_cluster = timed(lambda: cluster_cloud(cloud, plane=plane, **kw), args.iterations, args.warmup)
    t_segment = timed(lambda: segment_cloud(cloud, tol=TOL, hypotheses=T, **kw), args.iterations, args.warmup)
    return dict(cluster_cloud_ms=t_cluster, segment_cloud_with_the_fit_ms=t_segment)


def host_route(cloud, plane):
    """What a user without these entries does with a cloud on the device: -> (labels on the device, K)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p = cloud.cpu().numpy()   # read back
    nrm, d = plane.normal, np.float32(plane.offset)
    hgt = p @ nrm + d
    act = np.flatnonzero((hgt > HEIGHT[0]) & (hgt <= HEIGHT[1]))
    q = p[act]
    pairs = cKDTree(q).query_pairs(LINK, output_type="ndarray")
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(q), len(q)))
    ncomp, comp = connected_components(graph, directed=False)
    sizes = np.bincount(comp, minlength=ncomp)
    first = np.full(ncomp, len(q), dtype=np.int64)
    np.minimum.at(first, comp, np.arange(len(q)))
    order = sorted((-int(sizes[c]), int(first[c]), c) for c in range(ncomp) if sizes[c] >= MIN_POINTS)[:MAX_LABELS]
    remap = np.zeros(ncomp, dtype=np.int32)
    for k, (_, _, c) in enumerate(order):
        remap[c] = k + 1
    labels = np.zeros(p.shape[0], dtype=np.int32)
    labels[act] = remap[comp]
    return torch.from_numpy(labels).cuda(), len(order)   # upload


def bench_host(args, cloud, plane, labels):
    try:
        import scipy.sparse.csgraph  # noqa: F401
        import scipy.spatial  # noqa: F401
    except ImportError:
        return "not measured: scipy is not installed"
    got, num = host_route(cloud, plane)
    # cKDTree measures in f64 and the plane test is numpy's dot: a pair or a row within an ulp of a threshold may differ,
    # so the figure reported is the share of rows that carry the same label
    agree = float((got == labels).float().mean())
    t = []
    for _ in range(max(2, args.iterations // 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(cloud, plane)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(route="read back, height mask, cKDTree.query_pairs, connected_components, ranking, upload; host clock around "
                      "a synchronise", num_labels=num, rows_with_the_entrys_label=agree,
                ms=(float(np.median(t)), float(min(t)), float(max(t))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip", type=str, default="", help="comma list of raw,voxel3mm,api,host")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    skip = set(args.skip.split(","))
    out = dict(gpu=torch.cuda.get_device_name(), frames=2, frame=[H, W], iterations=args.iterations, link_dist=LINK,
               height_range=HEIGHT, min_points=MIN_POINTS)
    fused = make_fused_scene()
    plane = fit_plane(fused, tol=TOL, hypotheses=T)
    out["plane"] = dict(normal=plane.normal.tolist(), offset=plane.offset, inliers=plane.inliers, points=int(fused.shape[0]))
    t_down = timed(lambda: voxel_downsample(fused, VOXEL), args.iterations, args.warmup)
    small = voxel_downsample(fused, VOXEL)[0].contiguous()
    out["voxel_downsample_3mm_ms"] = t_down
    for name, cloud in (("raw", fused), ("voxel3mm", small)):
        if name in skip:
            continue
        res, labels = bench_entry(args, cloud, plane)
        if "api" not in skip:
            res["api"] = bench_api(args, cloud, plane)
        if "host" not in skip:
            res["host"] = bench_host(args, cloud, plane, labels)
        out[name] = res
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
