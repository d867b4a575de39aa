#!/usr/bin/env python3
"""Timing of voxel attention inside PVConv on one MI355X -- HIP events around warmed launches, medians, as
tools/bench_attention.py measures.

    python tools/bench_voxel_attention.py                 # JSON on the last line
    python tools/bench_voxel_attention.py --skip-encoders  # the two cores only

  cores      the fused core (gldm_point_attention_fused) against the materialised core (gldm_point_attention) on the SAME
             tensors, launches alternating in one process, at (C, n) = (64, 4096), (32, 1728), (128, 512): time, TFLOP/s of
             4 n^2 C per cloud and the fraction of the split-f16 ceiling (2500 / 3 TFLOP/s)
  encoders   PVCNN2Encoder at scale 0.5 and 1.0 for a batch of clouds with use_local_attention off and on
  launches   the launches the attention adds to that encoder's PVConv, each alone at its shape: the affine GroupNorm, the
             folded q' conv, the core, the folded out conv, GroupNorm + Swish with the squeeze sums
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import _lib as L  # noqa: E402
from graspldm_amd import attention as A  # noqa: E402
from graspldm_amd import numerics  # noqa: E402
from graspldm_amd.pc_encoders import PVCNN2Encoder  # noqa: E402
from graspldm_amd.synthetic import load_synthetic_weights  # noqa: E402

PEAK_SPLIT = 2500.0 / 3
CORE_SHAPES = [(16, 64, 4096), (64, 32, 1728), (256, 128, 512)]   # (clouds, C, n): seconds of the materialised core at most


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fns, iterations, warmup):
    """Median / min / max ms of every callable, their launches alternating (the same clocks and cache state for all)."""
    with torch.inference_mode():
        for _ in range(warmup):
            for fn in fns:
                fn()
                torch.cuda.synchronize()
        t = [[] for _ in fns]
        for _ in range(iterations):
            for i, fn in enumerate(fns):
                t[i].append(event_ms(fn))
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in t]


def bench_cores(args, out):
    rows = []
    for b, c, n in CORE_SHAPES:
        q, x = torch.randn(b, c, n, device="cuda") * c ** -0.25, torch.randn(b, c, n, device="cuda") * c ** -0.25
        fused, mat = timed([lambda: A.point_attention_fused(q, x, x), lambda: A.point_attention(q, x, x)], args.iterations, args.warmup)
        flop = 4.0 * c * n * n * b
        row = dict(clouds=b, c=c, n=n, fused_ms=fused, materialised_ms=mat)
        for name, t in (("fused", fused), ("materialised", mat)):
            row[name + "_tflops"] = flop / (t[0] * 1e-3) / 1e12
            if not args.f32_only:
                row[name + "_frac_of_split_ceiling"] = row[name + "_tflops"] / PEAK_SPLIT
        rows.append(row)
    out["cores"] = rows


def bench_encoders(args, out):
    b, n = args.clouds, args.points
    pcs = torch.randn(b, n, 3, device="cuda")
    enc_rows, launch_rows = [], []
    for scale in (0.5, 1.0):
        row = dict(scale=scale)
        for on in (False, True):
            enc = PVCNN2Encoder(in_features=3, out_features=64, n_points=n, scale_channels=scale, scale_voxel_resolution=scale,
                                out_channels=3, use_local_attention=on)
            enc = load_synthetic_weights(enc, seed=0).cuda().eval()
            row["on_ms" if on else "off_ms"] = timed([lambda: enc(pcs)], args.iterations, args.warmup)[0]
        enc_rows.append(row)
        block = enc.pvcnn_modules.sa_layers[1][0]
        att, c, r = block.voxel_layers[6], block.out_channels, block.resolution
        y, coef = torch.randn(b, c, r ** 3, device="cuda"), torch.rand(b, c, 2, device="cuda")
        xa, st = torch.empty_like(y), L.current_stream(y.device)
        pq, po = att._packed(y.device)
        L.call("gldm_groupnorm_affine", L.ptr(y), L.ptr(coef), b, c, r, L.ptr(xa), st)
        qp = A.run_conv(xa, pq)
        h = A.attention_core(qp, xa, xa)
        o = A.run_conv(h, po)
        names = ["groupnorm_affine", "q_conv", "core", "out_conv", "groupnorm_swish_sum"]
        t = timed([lambda: L.call("gldm_groupnorm_affine", L.ptr(y), L.ptr(coef), b, c, r, L.ptr(xa), st),
                   lambda: A.run_conv(xa, pq), lambda: A.attention_core(qp, xa, xa), lambda: A.run_conv(h, po),
                   lambda: A.groupnorm_swish_sum(o, att.norm, add=xa)], args.iterations, args.warmup)
        launch_rows.append(dict(scale=scale, c=c, r=r, clouds=b, **{k + "_ms": v for k, v in zip(names, t)}))
    out["encoders"], out["launches"] = enc_rows, launch_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--skip-encoders", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.manual_seed(0)
    out = dict(arithmetic="f32_only" if args.f32_only else "split", gpu=torch.cuda.get_device_name(), clouds=args.clouds,
               points=args.points)
    with numerics.f32_only(args.f32_only):
        bench_cores(args, out)
        if not args.skip_encoders:
            bench_encoders(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
