#!/usr/bin/env python3
"""Timing of the labelled-frame front end (gldm_depth_to_objects in csrc/depth_cloud.hip, gldm_farthest_points_euclid_ragged
in csrc/fps.hip, InferenceLDM.infer_on_scene) on one MI355X.  HIP events around warmed calls, medians of --iterations
with min-max, as tools/bench_depth.py.  One 480 x 640 frame, a plane with 8 objects of 28800, 12000, 8100, 4800, 2000,
1200, 750 and 400 pixels (two above 8192: the round launches; 750 and 400 are resampled up to 1024).

  objects     the bare gldm_depth_to_objects (three launches) on preallocated buffers against 8 calls of the bare
              gldm_depth_to_cloud with mask = (labels == k) (two launches each; the masks are built outside the window),
              and the two Python calls (allocations + read-backs) the same way
  regularize  regularize_objects (one ragged selection + one gather) against 8 calls of
              PointCloudHelpers.regularize_pc_point_count, on the same device clouds, to 1024 points
  e2e         infer_on_scene against the loop of 8 infer_on_depth(mask = labels == k) calls, --steps DDIM steps, 10 grasps
              per object: the loop is what the code before this entry could do

    python tools/bench_scene.py --out profiles/scene_bench.json"""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import (FLT_MAX, PointCloudHelpers, _depth_to_objects_packed, depth_to_cloud,  # noqa: E402
                                     depth_to_objects, regularize_objects)

H, W = 480, 640
BOXES = [(20, 180, 20, 200), (20, 140, 230, 330), (200, 290, 20, 110), (200, 260, 140, 220), (300, 340, 20, 70),
         (300, 330, 100, 140), (300, 325, 170, 200), (300, 320, 230, 250)]   # (v0, v1, u0, u1) of labels 1 .. 8
K = len(BOXES)


def timed(fn, iterations, warmup):
    with torch.inference_mode():
        for _ in range(warmup):
            fn()
            torch.cuda.synchronize()
        t = []
        for _ in range(iterations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(min(t)), float(max(t))


def make_scene():
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.2 + 0.0003 * u + 0.0002 * v
    labels = torch.zeros(H, W, dtype=torch.int32)
    for k, (v0, v1, u0, u1) in enumerate(BOXES):
        labels[v0:v1, u0:u1] = k + 1
    bump = 0.04 * torch.sin(u / 23.0) * torch.cos(v / 17.0) + 0.0002 * v
    depth = torch.where(labels > 0, 0.8 + 0.01 * labels + bump, depth)
    dead = torch.rand(H, W, generator=torch.Generator().manual_seed(0)) < 0.2
    depth[dead & (labels == 0)] = 0.0   # dead pixels on the plane only: the objects keep their sizes
    return depth.contiguous(), labels


def bench_objects(args, out, depth, labels, cam):
    fx, fy, cx, cy = cam.intrinsics
    lib = L.lib()
    masks = [(labels == k).to(torch.uint8).contiguous() for k in range(1, K + 1)]
    nb_o = lib.gldm_depth_to_objects_workspace_bytes(1, H, W, K)
    nb_c = lib.gldm_depth_to_cloud_workspace_bytes(1, H, W)
    ws = torch.empty(max(nb_o, nb_c) // 4 + 1, dtype=torch.int32, device="cuda")
    pts = torch.empty(1, H * W, 3, device="cuda")
    each = [torch.empty(1, H * W, 3, device="cuda") for _ in range(K)]
    sc = torch.empty(2, 1, K, dtype=torch.int32, device="cuda")
    cnt = torch.empty(K, dtype=torch.int32, device="cuda")
    s = L.current_stream()

    def entry():
        L.call("gldm_depth_to_objects", L.ptr(depth), 0, 1.0, None, L.ptr(labels), K, 1, H, W, fx, fy, cx, cy, 0.0, FLT_MAX,
               None, None, None, L.ptr(ws), nb_o, L.ptr(pts), L.ptr(sc[0]), L.ptr(sc[1]), None, s)

    def loop():
        for k in range(K):
            L.call("gldm_depth_to_cloud", L.ptr(depth), 0, 1.0, L.ptr(masks[k]), 1, H, W, fx, fy, cx, cy, 0.0, FLT_MAX, None,
                   None, None, L.ptr(ws), nb_c, L.ptr(each[k]), L.ptr(cnt[k:]), None, s)

    t_entry = timed(entry, args.iterations, args.warmup)
    t_loop = timed(loop, args.iterations, args.warmup)
    start, count = sc.tolist()
    for k in range(K):   # the two routes agree, bit for bit
        a, b = pts[0, start[0][k]:start[0][k] + count[0][k]], each[k][0, :int(cnt[k])]
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    t_api = timed(lambda: depth_to_objects(depth, cam, labels, num_labels=K), args.iterations, args.warmup)
    t_api_loop = timed(lambda: [depth_to_cloud(depth, cam, mask=m) for m in masks], args.iterations, args.warmup)
    out["objects"] = dict(counts=count[0], entry_ms=t_entry, loop_of_8_entries_ms=t_loop, api_ms=t_api,
                          loop_of_8_api_ms=t_api_loop, ratio_loop_over_entry=t_loop[0] / t_entry[0],
                          ratio_api_loop_over_api=t_api_loop[0] / t_api[0])


def bench_regularize(args, out, depth, labels, cam):
    points, _, starts, counts = _depth_to_objects_packed(depth, cam, labels, num_labels=K)
    packed, starts, counts = points[0], starts[0], counts[0]
    clouds = [packed[s:s + c] for s, c in zip(starts, counts)]
    np.random.seed(1)
    exp = torch.stack([PointCloudHelpers.regularize_pc_point_count(c, 1024, True) for c in clouds])
    np.random.seed(1)
    assert torch.equal(regularize_objects(packed, starts, counts, 1024), exp)
    t_one = timed(lambda: regularize_objects(packed, starts, counts, 1024), args.iterations, args.warmup)
    t_loop = timed(lambda: [PointCloudHelpers.regularize_pc_point_count(c, 1024, True) for c in clouds], args.iterations,
                   args.warmup)
    out["regularize"] = dict(counts=counts, regularize_objects_ms=t_one, loop_of_8_ms=t_loop,
                             ratio_loop_over_one=t_loop[0] / t_one[0])


def bench_e2e(args, out, depth, labels, cam):
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_fpc_ldm
    inf = InferenceLDM(model=build_fpc_ldm(n_points=1024, scheduler="ddim"), num_inference_steps=args.steps, device="cuda:0")
    masks = [labels == k for k in range(1, K + 1)]
    n_it = max(3, args.iterations // 2)
    scene = lambda: inf.infer_on_scene(depth, cam, labels, num_grasps=10, num_points=1024, num_labels=K)   # noqa: E731
    loop = lambda: [inf.infer_on_depth(depth, cam, mask=m, num_grasps=10, num_points=1024) for m in masks]   # noqa: E731
    assert scene()["grasps"].shape == (K, 10, 4, 4)
    t_scene = timed(scene, n_it, 2)
    t_loop = timed(loop, n_it, 2)
    out["e2e"] = dict(steps=args.steps, grasps_per_object=10, infer_on_scene_ms=t_scene, loop_of_8_infer_on_depth_ms=t_loop,
                      ratio_loop_over_scene=t_loop[0] / t_scene[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100, help="DDIM steps of the e2e part")
    ap.add_argument("--skip", type=str, default="", help="comma list of objects,regularize,e2e")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    out = dict(gpu=torch.cuda.get_device_name(), frame=[H, W], objects_in_frame=K, iterations=args.iterations)
    cam = Camera.from_intrinsics(615.3, 615.7, 319.5, 239.5, W, H)
    depth, labels = make_scene()
    depth, labels = depth.cuda(), labels.cuda()
    skip = set(args.skip.split(","))
    if "objects" not in skip:
        bench_objects(args, out, depth, labels, cam)
    if "regularize" not in skip:
        bench_regularize(args, out, depth, labels, cam)
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
