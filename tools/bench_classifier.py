#!/usr/bin/env python3
"""Timing of the grasp success classifier on one MI355X: 256 synthetic clouds x 20 poses = 5,120 scenes of 1024 + 64 points
through PointsBasedGraspClassifier.score_poses (PVCNN backbone, scale_channels 0.25, scale_voxel_resolution 0.75), and
its three stages on one chunk of scenes: the scene kernel, the backbone, the head.  The head launch (gldm_cls_head) is
timed alternately with the three layer launches it replaces (pointwise_conv_bn_relu, pointwise_rows, dense.linear) on the
same features.  HIP events around warmed calls, medians of --iterations.

    python tools/bench_classifier.py --out profiles/classifier_bench.json

FLOP of the head per scene: 2 C rows N for the GEMM (the 128 -> 1 row and the point weights are 2 rows N more, counted);
rated against the split-f16 ceiling (2500 / 3 TFLOP/s: three f16 products per f32 product) and, as bytes, against one read
of the features."""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import dense, numerics  # noqa: E402
from graspldm_amd.grasp_classifier import grasp_scene  # noqa: E402
from graspldm_amd.gripper import control_points  # noqa: E402
from graspldm_amd.pipeline import build_classifier  # noqa: E402
from graspldm_amd.synthetic import PC_STD, _random_rotation, synthetic_batch  # noqa: E402

PEAK_SPLIT = 2500.0 / 3


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


def alternate(fa, fb, iterations, warmup):
    """Two callables timed in turns (a b a b ...), so that both see the same clocks and neighbours."""
    ta, tb = [], []
    with torch.inference_mode():
        for i in range(warmup + iterations):
            for fn, t in ((fa, ta), (fb, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    t.append(e0.elapsed_time(e1))
    stat = lambda t: (float(np.median(t)), float(min(t)), float(max(t)))   # noqa: E731
    return stat(ta), stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--gripper_points", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=160, help="scenes of the per-stage timings")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    bc, g, n_cloud, n_grip = args.clouds, args.poses, args.points, args.gripper_points
    n = n_cloud + n_grip
    out = dict(clouds=bc, poses=g, scenes=bc * g, points=n, arithmetic="f32_only" if args.f32_only else "split",
               gpu=torch.cuda.get_device_name())
    with numerics.f32_only(args.f32_only):
        model = build_classifier(n_cloud, n_grip, "PVCNN").cuda()
        pcs, metas = synthetic_batch(bc, n_cloud)
        gen = torch.Generator().manual_seed(0)
        H = torch.zeros(bc * g, 4, 4)
        for i in range(bc * g):
            H[i, :3, :3] = _random_rotation(gen).float()
        H[:, :3, 3] = metas["pc_mean"].repeat_interleave(g, 0) + 0.06 * torch.randn(bc * g, 3, generator=gen)
        H[:, 3, 3] = 1.0
        pc, Hc, mean, gp = pcs.cuda(), H.cuda(), metas["pc_mean"].cuda(), control_points(n_grip).cuda()
        score = lambda: model.score_poses(pc, Hc, gripper_points=gp, pc_mean=mean, pc_scale=PC_STD)   # noqa: E731
        out["score_poses_ms"] = timed(score, max(3, args.iterations // 3), 1)
        out["scenes_per_s"] = bc * g / (out["score_poses_ms"][0] * 1e-3)
        out["chunk_scenes_default"] = max(1, (2 << 30) // model._scene_bytes(n))
        # the stages on one chunk of whole clouds
        cc = max(1, args.chunk // g)
        s = cc * g
        out["stage_scenes"] = s
        scene = lambda: grasp_scene(pc[:cc], Hc[:s], gp, mean[:cc], 0.0, PC_STD)   # noqa: E731
        out["scene_kernel_ms"] = timed(scene, args.iterations, args.warmup)
        x = scene()
        out["backbone_ms"] = timed(lambda: model.base_network(x), args.iterations, args.warmup)
        feats = model.base_network(x)
        conv, bn, conv2, lin = model._head_layers()
        c, rows = feats.shape[1], conv.weight.shape[0]
        fallback = lambda: dense.linear(dense.pointwise_rows(dense.pointwise_conv_bn_relu(feats, conv, bn), conv2), lin)   # noqa: E731
        head = lambda: model.head(feats)   # noqa: E731
        out["head_ms"], out["head_three_launch_fallback_ms"] = alternate(head, fallback, args.iterations, args.warmup)
        lo = model.head(feats)[0]
        out["head_vs_fallback_max_abs_diff"] = float((lo - fallback().reshape(-1)).abs().max())
    flop = (2.0 * c * rows + 2.0 * rows + 2.0) * n * s
    out["head_tflops"] = flop / (out["head_ms"][0] * 1e-3) / 1e12
    out["head_read_GBps"] = 4.0 * c * n * s / (out["head_ms"][0] * 1e-3) / 1e9
    if not args.f32_only:
        out["head_frac_of_split_ceiling"] = out["head_tflops"] / PEAK_SPLIT
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
