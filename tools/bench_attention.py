#!/usr/bin/env python3
"""Timing of the global-attention path on one MI355X: the shipped encoder (PVCNNEncoder, fpc arguments) for a batch of
clouds with use_global_attention off and on, the attention core alone (gldm_point_attention at the encoder's width) and
the Attention block alone -- HIP events around warmed forwards, as tools/bench_encoders.py measures.

    python tools/bench_attention.py                      # 256 clouds x 1024 points, JSON on the last line
    bash tools/prof_kernels.sh attn tools/bench_attention.py --iterations 3     # per-kernel times (scores / softmax / apply)

FLOP of the core per cloud: 2 c n^2 for the scores and 2 c n^2 for the apply product; rated against the split-f16 ceiling
(2500 / 3 TFLOP/s: three f16 products per f32 product)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import numerics  # noqa: E402
from graspldm_amd.attention import Attention, point_attention  # noqa: E402
from graspldm_amd.pc_encoders import PVCNNEncoder  # noqa: E402
from graspldm_amd.synthetic import load_synthetic_weights  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--f32-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.manual_seed(0)
    b, n = args.clouds, args.points
    out = dict(clouds=b, points=n, arithmetic="f32_only" if args.f32_only else "split", gpu=torch.cuda.get_device_name())
    with numerics.f32_only(args.f32_only):
        pcs = torch.randn(b, n, 3, device="cuda")
        for on in (False, True):
            enc = PVCNNEncoder(in_features=3, out_features=64, n_points=n, scale_channels=0.75, scale_voxel_resolution=0.75,
                               num_blocks=(1, 1, 1, 1), out_channels=3, use_global_attention=on)
            enc = load_synthetic_weights(enc, seed=0).cuda().eval()
            out["encoder_attention_on_ms" if on else "encoder_attention_off_ms"] = timed(lambda: enc(pcs), args.iterations, args.warmup)
        c = enc.global_attention.q.weight.shape[0]
        x = torch.randn(b, c, n, device="cuda")
        q = torch.randn(b, c, n, device="cuda")
        out["core_ms"] = timed(lambda: point_attention(q, x, x), args.iterations, args.warmup)
        att = enc.global_attention
        out["block_ms"] = timed(lambda: att(x), args.iterations, args.warmup)
    flop = 4.0 * c * n * n * b
    out["core_tflops"] = flop / (out["core_ms"][0] * 1e-3) / 1e12
    if not args.f32_only:
        out["core_frac_of_split_ceiling"] = out["core_tflops"] / PEAK_SPLIT
    print(json.dumps(out))


if __name__ == "__main__":
    main()
