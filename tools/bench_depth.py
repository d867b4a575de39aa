#!/usr/bin/env python3
"""Timing of the depth front end (csrc/depth_cloud.hip, the large farthest-point selection of csrc/fps.hip,
InferenceLDM.infer_on_depth) on one MI355X.  HIP events around warmed calls, medians of --iterations with min-max, as
tools/bench_grasp_select.py.

  deproject   gldm_depth_to_cloud at 480 x 640, f32 and u16, 1 and 16 frames: the bare entry on preallocated buffers
              (two launches), the Python call (allocations + the read-back of the counts), and the plain torch expression
              on the same GPU (torch.where, index math, vstack) per frame.  `frac_of_copy`: the time a float4 copy of the
              same bytes would take (depth read once + 12 B per kept pixel, at COPY_TBPS measured copy bandwidth) over the
              entry's time.
  fps         gldm_farthest_points_euclid_large 3e5 -> 1024 and -> 4096 for 1 and 16 clouds: time per call and per round,
              bytes per round (20 B per point: 12 read, minimum read and written) and the bandwidth that makes.  Yardstick:
              the reference's numpy routine (oracle.front_end.farthest_points) on this job's CPUs for --cpu_rounds rounds,
              per-round time EXTRAPOLATED to the full m (the routine's cost per round does not depend on the round).
  e2e         infer_on_depth on one 480 x 640 frame with a mask (object of about 6e4 pixels -> 1024 points, 10 DDIM steps)
              beside infer_on_pointcloud on the ready 1024-point cloud: the front end's share.

    python tools/bench_depth.py --out profiles/depth_bench.json"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import FLT_MAX, depth_to_cloud, farthest_point_indices, gather_points  # noqa: E402

COPY_TBPS = 6.29
H, W = 480, 640


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


def make_depth(frames, seed=0):
    """A tilted plane with a bumpy object and 20 % dead pixels: metres f32 and the same in millimetres u16."""
    g = torch.Generator().manual_seed(seed)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = (1.2 + 0.0003 * u + 0.0002 * v).repeat(frames, 1, 1)
    mask = torch.zeros(frames, H, W, dtype=torch.uint8)
    mask[:, 120:360, 200:460] = 1
    d = torch.where(mask.bool(), 0.8 + 0.04 * torch.sin(u / 23.0) * torch.cos(v / 17.0) + 0.0002 * v, d)
    d[torch.rand(frames, H, W, generator=g) < 0.2] = 0.0
    raw = (d * 1000.0).round().to(torch.int32).numpy().astype(np.uint16)
    return d.contiguous(), torch.from_numpy(raw), mask


def torch_deproject(depth, fx, fy, cx, cy):
    where = torch.where(depth > 0)
    x, y = where[1], where[0]
    z = depth[y, x]
    return torch.vstack(((x.to(torch.float32) - cx) * z / fx, (y.to(torch.float32) - cy) * z / fy, z)).T


def bench_deproject(args, out):
    cam = Camera.from_intrinsics(615.3, 615.7, 319.5, 239.5, W, H)
    fx, fy, cx, cy = cam.intrinsics
    lib = L.lib()
    for frames in (1, 16):
        d32, d16, _ = make_depth(frames)
        for name, d, scale in (("f32", d32.cuda(), None), ("u16", d16.cuda(), 0.001)):
            nbytes = lib.gldm_depth_to_cloud_workspace_bytes(frames, H, W)
            ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device="cuda")
            pts = torch.empty(frames, H * W, 3, device="cuda")
            cnt = torch.empty(frames, dtype=torch.int32, device="cuda")
            entry = lambda: L.call("gldm_depth_to_cloud", L.ptr(d), int(scale is not None), float(scale or 1.0), None, frames,  # noqa: E731
                                   H, W, fx, fy, cx, cy, 0.0, FLT_MAX, None, None, None, L.ptr(ws), nbytes, L.ptr(pts),
                                   L.ptr(cnt), None, L.current_stream())
            api = lambda: depth_to_cloud(d, cam, depth_scale=scale)   # noqa: E731
            metres = d if scale is None else d.to(torch.int32).to(torch.float32) * scale
            plain = lambda: [torch_deproject(metres[f], fx, fy, cx, cy) for f in range(frames)]   # noqa: E731
            t_entry = timed(entry, args.iterations, args.warmup)
            t_api = timed(api, args.iterations, args.warmup)
            t_plain = timed(plain, args.iterations, args.warmup)
            kept = int(cnt.sum())
            ideal_bytes = frames * H * W * d.element_size() + 12 * kept
            out[f"deproject_{name}_f{frames}"] = dict(
                entry_ms=t_entry, api_ms=t_api, torch_ms=t_plain, ratio_torch_over_api=t_plain[0] / t_api[0], kept=kept,
                ideal_bytes=ideal_bytes, frac_of_copy=ideal_bytes / (COPY_TBPS * 1e12) / (t_entry[0] * 1e-3))


def bench_fps(args, out):
    from oracle import front_end as F
    n = 300000
    g = torch.Generator().manual_seed(1)
    clouds = (torch.randn(16, n, 3, generator=g) * torch.tensor([0.3, 0.2, 0.05]) + torch.tensor([0.0, 0.0, 1.0])).contiguous()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    t0 = time.perf_counter()
    ref = F.farthest_points(clouds[0].numpy(), args.cpu_rounds)
    cpu_round_ms = (time.perf_counter() - t0) * 1e3 / args.cpu_rounds
    out["fps_cpu_numpy"] = dict(n=n, rounds_run=args.cpu_rounds, per_round_ms=cpu_round_ms,
                                extrapolated_ms={"1024": cpu_round_ms * 1024, "4096": cpu_round_ms * 4096},
                                note="per cloud; the full-m times are extrapolated from rounds_run rounds")
    for b in (1, 16):
        pc = clouds[:b].cuda()
        for m in (1024, 4096):
            t = timed(lambda: farthest_point_indices(pc, m), args.iterations, args.warmup)
            idx = farthest_point_indices(pc, m)
            assert np.array_equal(idx[0, :args.cpu_rounds].cpu().numpy(), ref)
            bytes_round = b * n * 20
            out[f"fps_n{n}_m{m}_b{b}"] = dict(call_ms=t, per_round_us=t[0] * 1e3 / m, bytes_per_round=bytes_round,
                                              tbps=bytes_round / (t[0] * 1e-3 / m) / 1e12,
                                              speedup_vs_numpy_extrapolated=cpu_round_ms * m * b / t[0])


def bench_e2e(args, out):
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_fpc_ldm
    inf = InferenceLDM(model=build_fpc_ldm(n_points=1024, scheduler="ddim"), num_inference_steps=10, device="cuda:0")
    cam = Camera.from_intrinsics(615.3, 615.7, 319.5, 239.5, W, H)
    d32, _, mask = make_depth(1)
    depth, mask = d32[0].cuda(), mask[0].cuda()
    obj = depth_to_cloud(depth, cam, mask=mask)
    ready = gather_points(obj, farthest_point_indices(obj, 1024))[0]
    n_it = max(3, args.iterations // 2)
    t_depth = timed(lambda: inf.infer_on_depth(depth, cam, mask=mask, num_grasps=10, num_points=1024), n_it, 2)
    t_ready = timed(lambda: inf.infer_on_pointcloud(ready, num_grasps=10), n_it, 2)
    t_front = timed(lambda: gather_points(depth_to_cloud(depth, cam, mask=mask), farthest_point_indices(
        depth_to_cloud(depth, cam, mask=mask), 1024)), n_it, 2)
    out["e2e"] = dict(object_points=int(obj.shape[0]), infer_on_depth_ms=t_depth, infer_on_ready_cloud_ms=t_ready,
                      front_end_share=1.0 - t_ready[0] / t_depth[0], deproject_twice_fps_gather_ms=t_front)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu_rounds", type=int, default=16, help="rounds of the numpy routine that are really run")
    ap.add_argument("--skip", type=str, default="", help="comma list of deproject,fps,e2e")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    out = dict(gpu=torch.cuda.get_device_name(), frame=[H, W], copy_tbps=COPY_TBPS, iterations=args.iterations)
    skip = set(args.skip.split(","))
    if "deproject" not in skip:
        bench_deproject(args, out)
    if "fps" not in skip:
        bench_fps(args, out)
    if "e2e" not in skip:
        bench_e2e(args, out)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
