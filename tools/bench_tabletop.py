#!/usr/bin/env python3
"""Timing of the tabletop segmenter (gldm_plane_ransac, gldm_plane_moments, gldm_segment_tabletop in csrc/tabletop.hip;
pointcloud.fit_table_plane / segment_tabletop; InferenceLDM.infer_on_tabletop) on one MI355X.  HIP events around warmed
calls, medians of --iterations with min-max, as tools/bench_scene.py, whose 480 x 640 frame it uses with a table under it:
the 8 objects of 28800 .. 400 pixels keep their depth, the background becomes a tilted plane in 3-D (bench_scene's is
linear in the pixel coordinates, which is a curved surface) with 1 mm of seeded noise; 20 % of the table's pixels are dead.

  ransac    the bare gldm_plane_ransac at T = 512 on the frame's cloud, preallocated buffers: one call per event window,
            and 50 calls in one window (per call: the kernels without the launch gaps of a lone call); achieved
            point-hypothesis evaluations per second against the VALU ceiling (7 lane-operations per evaluation: 3 mul,
            3 add, 1 compare; 256 CUs x 64 lanes per clock x 2.4 GHz)
  segment   the bare gldm_segment_tabletop (six launches) the same two ways
  api       fit_table_plane and segment_tabletop(plane=None) end to end (allocations, the draws, the read-backs, the eigen-solve)
  host      the route without these entries: read the cloud and the frame back, numpy RANSAC at the same T (the same
            triples, the same f32 test), height mask, scipy.ndimage.label, size filter, upload -- where scipy is installed
  e2e       infer_on_tabletop against infer_on_scene with ready labels, --steps DDIM steps, 10 grasps per object

    python tools/bench_tabletop.py --out profiles/tabletop_bench.json"""
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
from bench_scene import BOXES, H, K, W, make_scene, timed  # noqa: E402
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import FLT_MAX, depth_to_cloud, fit_table_plane, segment_tabletop  # noqa: E402

T, TOL = 512, 0.005
SEG = dict(height_range=(0.01, 0.8), link_dist=0.01, min_pixels=32)
SIZES = [(v1 - v0) * (u1 - u0) for v0, v1, u0, u1 in BOXES]
VALU_LANE_OPS_PER_S = 256 * 64 * 2.4e9
OPS_PER_EVAL = 7
BATCH = 50


FX, FY, CX, CY = 615.3, 615.7, 319.5, 239.5
TABLE_N, TABLE_Z0 = (0.13, 0.09, -0.987), 1.3   # direction of the table's normal, its depth on the optical axis


def make_table_scene():
    """bench_scene's objects on a planar table: -> (depth [H, W] f32, labels [H, W] int32)."""
    depth, labels = make_scene()
    n = np.asarray(TABLE_N, dtype=np.float64)
    n /= np.linalg.norm(n)
    d = -n[2] * TABLE_Z0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = -d / (n[0] * (u - CX) / FX + n[1] * (v - CY) / FY + n[2])
    z += np.random.default_rng(1).normal(0.0, 0.001, (H, W))
    table = torch.from_numpy(z.astype(np.float32))
    table[depth == 0.0] = 0.0   # bench_scene's dead pixels (on the background only)
    return torch.where(labels > 0, depth, table).contiguous(), labels


def per_call(fn, iterations, warmup):
    """BATCH calls back to back inside one event window -> (median, min, max) ms per call."""
    def many():
        for _ in range(BATCH):
            fn()
    return tuple(v / BATCH for v in timed(many, iterations, warmup))


def bench_ransac(args, out, cloud):
    lib = L.lib()
    n = cloud.shape[0]
    tri = torch.from_numpy(np.random.default_rng(0).integers(0, n, (T, 3)).astype(np.int32)).cuda()
    nb = lib.gldm_plane_ransac_workspace_bytes(n, T)
    ws = torch.empty(nb // 4 + 1, dtype=torch.int32, device="cuda")
    planes = torch.empty(T, 4, device="cuda")
    counts = torch.empty(T, dtype=torch.int32, device="cuda")
    s = L.current_stream()

    def entry():
        L.call("gldm_plane_ransac", L.ptr(cloud), n, L.ptr(tri), T, TOL, 1e-8, L.ptr(ws), nb, L.ptr(planes), L.ptr(counts), s)

    t_one = timed(entry, args.iterations, args.warmup)
    t_many = per_call(entry, args.iterations, args.warmup)
    evals = float(n) * T
    rate = evals / (t_many[0] * 1e-3)
    out["ransac"] = dict(points=n, hypotheses=T, best_count=int(counts.max()), one_call_ms=t_one, back_to_back_ms_per_call=t_many,
                         evaluations_per_s=rate, valu_ceiling_evaluations_per_s=VALU_LANE_OPS_PER_S / OPS_PER_EVAL,
                         share_of_valu_ceiling=rate * OPS_PER_EVAL / VALU_LANE_OPS_PER_S)


def bench_segment(args, out, depth, cam, plane):
    lib = L.lib()
    fx, fy, cx, cy = cam.intrinsics
    nb = lib.gldm_segment_tabletop_workspace_bytes(H, W)
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device="cuda")
    labels = torch.empty(H, W, dtype=torch.int32, device="cuda")
    stats = torch.empty(1 + 2 * 64, dtype=torch.int32, device="cuda")
    pl = (ctypes.c_float * 4)(*plane.as_array())
    s = L.current_stream()

    def entry():
        L.call("gldm_segment_tabletop", L.ptr(depth), 0, 1.0, None, H, W, fx, fy, cx, cy, 0.0, FLT_MAX, None, None, None, pl,
               SEG["height_range"][0], SEG["height_range"][1], SEG["link_dist"], SEG["min_pixels"], 64, L.ptr(ws), nb,
               L.ptr(labels), L.ptr(stats[0:1]), L.ptr(stats[1:65]), L.ptr(stats[65:]), s)

    t_one = timed(entry, args.iterations, args.warmup)
    t_many = per_call(entry, args.iterations, args.warmup)
    host = stats.tolist()
    assert host[0] == K and host[1:1 + K] == SIZES, host[:1 + K]   # the eight boxes, largest first
    out["segment"] = dict(pixels=H * W, launches=6, num_labels=host[0], label_pixels=host[1:1 + K], one_call_ms=t_one,
                          back_to_back_ms_per_call=t_many)


def bench_api(args, out, depth, cam):
    t_fit = timed(lambda: fit_table_plane(depth, cam, tol=TOL, hypotheses=T), args.iterations, args.warmup)
    t_seg = timed(lambda: segment_tabletop(depth, cam, tol=TOL, hypotheses=T, **SEG), args.iterations, args.warmup)
    out["api"] = dict(fit_table_plane_ms=t_fit, segment_tabletop_ms=t_seg)


def host_route(depth, cam, triples):
    """What a user without these entries does with a frame on the device: -> labels on the device."""
    import scipy.ndimage as ndi
    cloud, pix = depth_to_cloud(depth, cam, return_pixels=True)
    p, pix = cloud.cpu().numpy(), pix.cpu().numpy()   # read back
    best, best_n = None, -1
    for i, j, k in triples:
        c = np.cross(p[j] - p[i], p[k] - p[i])
        l2 = float(c @ c)
        if i == j or i == k or j == k or not l2 >= 1e-8:
            continue
        nrm = (c / np.float32(np.sqrt(l2))).astype(np.float32)
        d = -np.float32(nrm @ p[i])
        cnt = int((np.abs(p @ nrm + d) <= np.float32(TOL)).sum())
        if cnt > best_n:
            best, best_n = (nrm, d), cnt
    nrm, d = best
    if d < 0:
        nrm, d = -nrm, -d
    hgt = p @ nrm + d
    fg = np.zeros(H * W, dtype=bool)
    fg[pix[(hgt > SEG["height_range"][0]) & (hgt <= SEG["height_range"][1])]] = True
    lab, n = ndi.label(fg.reshape(H, W))
    sizes = np.bincount(lab.reshape(-1))
    order = [k for k in np.argsort(-sizes[1:], kind="stable") + 1 if sizes[k] >= SEG["min_pixels"]][:64]
    remap = np.zeros(n + 1, dtype=np.int32)
    remap[order] = np.arange(1, len(order) + 1)
    return torch.from_numpy(remap[lab]).cuda(), len(order)   # upload


def bench_host(args, out, depth, cam):
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        out["host"] = "not measured: scipy is not installed"
        return
    n = depth_to_cloud(depth, cam).shape[0]
    triples = np.random.default_rng(0).integers(0, n, (T, 3))
    labels, num = host_route(depth, cam, triples)
    assert num == K and [int((labels == k + 1).sum()) for k in range(K)] == SIZES
    t = []
    for _ in range(max(3, args.iterations // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(depth, cam, triples)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    out["host"] = dict(route="read back, numpy RANSAC T=512, scipy.ndimage.label, upload; host clock around a synchronise",
                       ms=(float(np.median(t)), float(min(t)), float(max(t))))


def bench_e2e(args, out, depth, labels, cam):
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_fpc_ldm
    inf = InferenceLDM(model=build_fpc_ldm(n_points=1024, scheduler="ddim"), num_inference_steps=args.steps, device="cuda:0")
    n_it = max(3, args.iterations // 2)
    seg = dict(tol=TOL, hypotheses=T, **SEG)
    table = lambda: inf.infer_on_tabletop(depth, cam, num_grasps=10, num_points=1024, segmentation=seg)   # noqa: E731
    scene = lambda: inf.infer_on_scene(depth, cam, labels, num_grasps=10, num_points=1024, num_labels=K)   # noqa: E731
    got = table()
    assert got["grasps"].shape == (K, 10, 4, 4) and torch.equal(got["labels"], labels)   # the labels a user would have passed
    t_scene, t_table = timed(scene, n_it, 2), timed(table, n_it, 2)
    t_scene2, t_table2 = timed(scene, n_it, 1), timed(table, n_it, 1)   # alternated: the spread between two windows
    out["e2e"] = dict(steps=args.steps, grasps_per_object=10, infer_on_scene_ready_labels_ms=[t_scene, t_scene2],
                      infer_on_tabletop_ms=[t_table, t_table2], added_ms=t_table[0] - t_scene[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="DDIM steps of the e2e part")
    ap.add_argument("--skip", type=str, default="", help="comma list of ransac,segment,api,host,e2e")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    out = dict(gpu=torch.cuda.get_device_name(), frame=[H, W], objects_in_frame=K, iterations=args.iterations)
    cam = Camera.from_intrinsics(FX, FY, CX, CY, W, H)
    depth, labels = make_table_scene()
    depth, labels = depth.cuda(), labels.cuda()
    skip = set(args.skip.split(","))
    cloud = depth_to_cloud(depth, cam)
    plane = fit_table_plane(depth, cam, tol=TOL, hypotheses=T)
    out["plane"] = dict(normal=plane.normal.tolist(), offset=plane.offset, inliers=plane.inliers, points=int(cloud.shape[0]))
    if "ransac" not in skip:
        bench_ransac(args, out, cloud)
    if "segment" not in skip:
        bench_segment(args, out, depth, cam, plane)
    if "api" not in skip:
        bench_api(args, out, depth, cam)
    if "host" not in skip:
        bench_host(args, out, depth, cam)
    if "e2e" not in skip:
        bench_e2e(args, out, depth, labels, cam)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
