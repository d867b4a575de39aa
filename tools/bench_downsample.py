#!/usr/bin/env python3
"""Timing of the voxel-grid downsampling (gldm_voxel_downsample in csrc/cloud_downsample.hip; pointcloud.voxel_downsample;
the `downsample=` argument of the entry points) on one MI355X.  HIP events around warmed calls, medians of --iterations
with min-max, alternated windows where two routes are compared, as tools/bench_cleanup.py.  The frame is
tools/bench_depth.py's 480 x 640 one: an object of 49,993 pixels at about 0.8 m (1.3 mm between pixels).

  gpu       at 2, 3 and 5 mm: the bare entry with preallocated buffers (one call per event window, and 50 calls in one
            window), then pointcloud.voxel_downsample end to end (allocations, the finite / range check, both read-backs)
  compose   the route without the entry that stays on the GPU: cell keys packed into int64, torch.unique(return_inverse,
            return_counts), index_add_ of the f64 coordinates, a division.  Asserted to give the same voxels and members, and
            centroids within voxel_size * 2^-16 + one f32 ulp of the entry's (the derived bar of
            tests/test_cloud_downsample_cpu.py).  Alternated with voxel_downsample.
  alt       with --alt_lib: the bare entry of another build of the library (make EXTRA=... OUT=...) on the same buffers,
            alternated with this build's, and its outputs compared bit for bit
  e2e       infer_on_depth on the frame (-> 1024 points, 10 grasps, 10 DDIM steps) with and without CloudDownsample(0.003),
            and both again with a CloudCleanup; alternated windows

    python tools/bench_downsample.py --out profiles/downsample_bench.json"""
import argparse
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_depth import H, W, make_depth, timed  # noqa: E402
from graspldm_amd import _abi, _lib as L  # noqa: E402
from graspldm_amd.camera import Camera  # noqa: E402
from graspldm_amd.pointcloud import depth_to_cloud, voxel_downsample  # noqa: E402

FX, FY, CX, CY = 615.3, 615.7, 319.5, 239.5
SIZES = (0.002, 0.003, 0.005)
BATCH = 50


def per_call(fn, iterations, warmup):
    def many():
        for _ in range(BATCH):
            fn()
    return tuple(v / BATCH for v in timed(many, iterations, warmup))


class Entry:
    """The bare gldm_voxel_downsample of one library on preallocated buffers, one cloud."""

    def __init__(self, fn, ws_bytes, obj):
        n, dev = obj.shape[0], obj.device
        self.fn, self.obj, self.n = fn, obj, n
        self.sc = torch.tensor([[0], [n]], dtype=torch.int32, device=dev)
        self.nbytes = ws_bytes(1, n, n)
        self.ws = torch.empty(self.nbytes // 8 + 1, dtype=torch.int64, device=dev)
        self.out = torch.zeros(n, 3, device=dev)
        self.fm = torch.zeros(2, n, dtype=torch.int32, device=dev)
        self.osc = torch.zeros(2, 1, dtype=torch.int32, device=dev)
        self.vox = torch.zeros(n, dtype=torch.int32, device=dev)
        self.stream = L.current_stream()

    def __call__(self, v, with_map=True):
        st = self.fn(L.ptr(self.obj), L.ptr(self.sc[0]), L.ptr(self.sc[1]), 1, self.n, self.n, v, L.ptr(self.ws), self.nbytes,
                     L.ptr(self.out), L.ptr(self.osc[0]), L.ptr(self.osc[1]), L.ptr(self.fm[0]), L.ptr(self.fm[1]),
                     L.ptr(self.vox if with_map else None), self.stream)
        assert st == 0, st

    def outputs(self):
        m = int(self.osc[1, 0])
        return self.out[:m].clone(), self.fm[:, :m].clone(), self.vox.clone()


def bench_gpu(args, out, obj):
    lib = L.lib()
    entry = Entry(lib.gldm_voxel_downsample, lib.gldm_voxel_downsample_workspace_bytes, obj)
    res = {}
    for v in SIZES:
        one = timed(lambda: entry(v), args.iterations, args.warmup)
        many = per_call(lambda: entry(v), args.iterations, args.warmup)
        no_map = per_call(lambda: entry(v, with_map=False), args.iterations, 1)
        api = timed(lambda: voxel_downsample(obj, v), args.iterations, args.warmup)
        res[f"{v * 1e3:g}mm"] = dict(voxels=int(entry.osc[1, 0]), one_call_ms=one, back_to_back_ms_per_call=many,
                                     back_to_back_without_map_ms_per_call=no_map, voxel_downsample_ms=api)
    out["gpu"] = res
    return entry


def compose_route(obj, v):
    """The same voxels from torch ops -> (centroids f32 [m,3] in ascending key order, keys int64 [m], members int64 [m])."""
    cell = torch.floor(obj.double() / v).to(torch.int64) + (1 << 20)
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    keys, inverse, members = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros(keys.shape[0], 3, dtype=torch.float64, device=obj.device).index_add_(0, inverse, obj.double())
    return (sums / members[:, None]).float(), keys, members


def bench_compose(args, out, obj):
    res = {}
    for v in SIZES:
        v32 = float(np.float32(v))
        cen, keys, members = compose_route(obj, v32)
        pts, _, m, first, mem = voxel_downsample(obj, v)
        cell = torch.floor(obj[first.long()].double() / v32).to(torch.int64) + (1 << 20)
        mine = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
        order = torch.argsort(mine)
        assert torch.equal(mine[order], keys) and torch.equal(mem.long()[order], members), "the two GPU routes disagree"
        bar = v32 * 2.0 ** -16 + torch.from_numpy(np.spacing(np.abs(cen.cpu().numpy()))).to(obj.device).double()
        worst = (pts[order].double() - cen.double()).abs()
        assert bool((worst <= bar).all()), "centroids beyond voxel_size * 2^-16 + one f32 ulp"
        fn = lambda: compose_route(obj, v32)          # noqa: E731
        api = lambda: voxel_downsample(obj, v)        # noqa: E731
        a1 = timed(fn, args.iterations, args.warmup)
        b1 = timed(api, args.iterations, args.warmup)
        a2 = timed(fn, args.iterations, 1)
        b2 = timed(api, args.iterations, 1)
        res[f"{v * 1e3:g}mm"] = dict(voxels=m, max_centroid_difference_m=float(worst.max()), ms=[a1, a2],
                                     voxel_downsample_ms_alternated=[b1, b2])
    out["compose"] = dict(route="int64 cell keys, torch.unique(return_inverse, return_counts), index_add_ in f64, division; "
                                "the voxels come in key order, without first / the row map", sizes=res)


def bench_alt(args, out, obj, entry):
    h = ctypes.CDLL(args.alt_lib)
    for name in ("gldm_voxel_downsample", "gldm_voxel_downsample_workspace_bytes"):
        getattr(h, name).restype, getattr(h, name).argtypes = _abi.PROTOTYPES[name]
    alt = Entry(h.gldm_voxel_downsample, h.gldm_voxel_downsample_workspace_bytes, obj)
    res = {}
    for v in SIZES:
        entry(v)
        alt(v)
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(entry.outputs(), alt.outputs()))
        windows = []
        for w in range(3):   # alternated: the spread between windows of the same build is the noise floor of the comparison
            windows.append(dict(this_ms_per_call=per_call(lambda: entry(v), args.iterations, args.warmup if w == 0 else 1),
                                alt_ms_per_call=per_call(lambda: alt(v), args.iterations, args.warmup if w == 0 else 1)))
        res[f"{v * 1e3:g}mm"] = dict(outputs_bit_equal=same, windows=windows)
    out["alt"] = dict(alt_lib=os.path.basename(args.alt_lib), note=args.alt_note, calls_per_window=BATCH, sizes=res)


def bench_e2e(args, out, depth, mask, cam):
    from graspldm_amd.grasp_select import CloudCleanup, CloudDownsample
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_fpc_ldm
    inf = InferenceLDM(model=build_fpc_ldm(n_points=1024, scheduler="ddim"), num_inference_steps=10, device="cuda:0")
    down, clean = CloudDownsample(0.003), CloudCleanup()
    routes = dict(plain={}, downsample=dict(downsample=down), cleanup=dict(cleanup=clean),
                  downsample_cleanup=dict(downsample=down, cleanup=clean))
    n_it = max(3, args.iterations // 2)
    res = {name: [] for name in routes}
    points = {}
    for w in range(2):   # alternated windows
        for name, kw in routes.items():
            fn = lambda: inf.infer_on_depth(depth, cam, mask=mask, num_grasps=10, num_points=1024, **kw)   # noqa: E731
            res[name].append(timed(fn, n_it, 2 if w == 0 else 1))
            with torch.inference_mode():   # as timed() runs it: the engines' buffers were made there
                r = fn()
            points[name] = [int(r[k][0]) for k in ("object_points_raw", "object_points") if k in r]
    out["e2e"] = dict(infer_on_depth_ms=res, object_points_raw_and_kept=points, voxel_size=down.voxel_size,
                      cleanup=clean.options, grasps=10, ddim_steps=10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip", type=str, default="", help="comma list of compose,e2e")
    ap.add_argument("--alt_lib", type=str, default=None, help="another build of libgldm_hip.so whose bare entry is alternated "
                                                              "with this build's")
    ap.add_argument("--alt_note", type=str, default="", help="what the other build changes (recorded)")
    ap.add_argument("--time_limit", type=int, default=300, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    cam = Camera.from_intrinsics(FX, FY, CX, CY, W, H)
    d32, _, mask = make_depth(1)
    depth, mask = d32[0].cuda(), mask[0].cuda()
    obj = depth_to_cloud(depth, cam, mask=mask).contiguous()
    out = dict(gpu_name=torch.cuda.get_device_name(), frame=[H, W], object_points=int(obj.shape[0]), iterations=args.iterations)
    skip = set(args.skip.split(","))
    entry = bench_gpu(args, out, obj)
    if "compose" not in skip:
        bench_compose(args, out, obj)
    if args.alt_lib:
        bench_alt(args, out, obj, entry)
    if "e2e" not in skip:
        bench_e2e(args, out, depth, mask, cam)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
