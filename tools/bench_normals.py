#!/usr/bin/env python3
"""Timing of the surface-normal front end (gldm_knn_radius, gldm_point_normals in csrc/normals.hip; pointcloud.knn_radius /
estimate_normals) on one MI355X.  HIP events around warmed calls, medians of --iterations with min-max, as
tools/bench_tabletop.py, whose 480 x 640 frame (8 objects on a tilted table, 20 % of the table's pixels dead) it uses.

  ordered   the frame's cloud in pixel order (gldm_depth_to_cloud's order), r = 0.05, k = 12: the bare gldm_knn_radius
            (two launches, preallocated buffers), the bare gldm_point_normals, and pointcloud.estimate_normals end to end
  shuffled  the same points under a fixed permutation: every 256-point chunk spans the frame, no chunk is skipped and the
            search is the full scan; candidate pairs per second against the VALU ceiling (9 lane-operations per pair:
            3 sub, 3 mul, 2 add, 1 compare; 256 CUs x 64 lanes per clock x 2.4 GHz)
  host      the route without these entries: read the cloud back, cKDTree(...).query(k, distance_upper_bound, workers=16),
            numpy eigh of the f64 scatter matrices, orientation, upload -- where scipy is installed

    python tools/bench_normals.py --out profiles/normals_bench.json"""
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
from bench_scene import H, W, timed  # noqa: E402
from bench_tabletop import CX, CY, FX, FY, make_table_scene  # noqa: E402
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import depth_to_cloud, estimate_normals  # noqa: E402

RADIUS, K = 0.05, 12
VALU_LANE_OPS_PER_S = 256 * 64 * 2.4e9
OPS_PER_PAIR = 9


def bench_gpu(args, cloud):
    lib = L.lib()
    n = cloud.shape[0]
    nb = lib.gldm_knn_radius_workspace_bytes(1, n)
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device="cuda")
    idx = torch.empty(n, K, dtype=torch.int32, device="cuda")
    d2 = torch.empty(n, K, dtype=torch.float32, device="cuda")
    found = torch.empty(n, dtype=torch.int32, device="cuda")
    normals = torch.empty(n, 3, device="cuda")
    view = np.zeros(3, dtype=np.float32)
    s = L.current_stream()

    def search():
        L.call("gldm_knn_radius", L.ptr(cloud), 1, n, K, RADIUS, L.ptr(ws), nb, L.ptr(idx), L.ptr(d2), L.ptr(found), s)

    def eigen():
        L.call("gldm_point_normals", L.ptr(cloud), L.ptr(idx), None, 1, n, K, view.ctypes.data, L.ptr(normals), s)

    t_search = timed(search, args.iterations, args.warmup)
    t_eigen = timed(eigen, args.iterations, args.warmup)
    t_api = timed(lambda: estimate_normals(cloud, max_radius=RADIUS, k=K), args.iterations, args.warmup)
    return dict(points=n, knn_radius_ms=t_search, point_normals_ms=t_eigen, estimate_normals_ms=t_api,
                found_min=int(found.min()), found_max=int(found.max())), normals.clone()


def host_route(cloud):
    """What a user without these entries does with a cloud on the device: -> normals on the device."""
    from scipy.spatial import cKDTree
    p = cloud.cpu().numpy()   # read back
    n = p.shape[0]
    _, ndx = cKDTree(p).query(p, k=K, distance_upper_bound=RADIUS, workers=16)
    ndx = np.where(ndx == n, np.arange(n)[:, None], ndx)
    diffs = (p[ndx] - p[:, None, :]).astype(np.float64)
    _, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", diffs, diffs))
    nrm = vec[:, :, 0]
    nrm[(nrm * p).sum(-1) >= 0] *= -1.0
    return torch.from_numpy(nrm.astype(np.float32)).cuda()   # upload


def bench_host(args, out, cloud, normals):
    try:
        import scipy.spatial  # noqa: F401
    except ImportError:
        out["host"] = "not measured: scipy is not installed"
        return
    got = host_route(cloud)
    agree = float(((got * normals).sum(-1).abs() > 0.999).float().mean())
    t = []
    for _ in range(max(3, args.iterations // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(cloud)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    out["host"] = dict(route="read back, cKDTree query workers=16, numpy eigh (f64), upload; host clock around a synchronise",
                       ms=(float(np.median(t)), float(min(t)), float(max(t))), share_of_normals_within_2_6_degrees=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip", type=str, default="", help="comma list of ordered,shuffled,host")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    out = dict(gpu=torch.cuda.get_device_name(), frame=[H, W], radius=RADIUS, k=K, iterations=args.iterations)
    cam = Camera.from_intrinsics(FX, FY, CX, CY, W, H)
    depth, _ = make_table_scene()
    cloud = depth_to_cloud(depth.cuda(), cam).contiguous()
    skip = set(args.skip.split(","))
    normals = None
    if "ordered" not in skip:
        out["ordered"], normals = bench_gpu(args, cloud)
    if "shuffled" not in skip:
        perm = torch.from_numpy(np.random.default_rng(0).permutation(cloud.shape[0])).cuda()
        res, shuffled_normals = bench_gpu(args, cloud[perm].contiguous())
        pairs = float(cloud.shape[0]) ** 2
        rate = pairs / (res["knn_radius_ms"][0] * 1e-3)
        res.update(candidate_pairs_per_s=rate, share_of_valu_ceiling=rate * OPS_PER_PAIR / VALU_LANE_OPS_PER_S)
        if normals is not None:
            res["normals_equal_ordered_bitwise"] = bool(torch.equal(shuffled_normals, normals[perm]))
        out["shuffled"] = res
    if "host" not in skip and normals is not None:
        bench_host(args, out, cloud, normals)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
