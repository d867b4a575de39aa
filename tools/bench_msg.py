#!/usr/bin/env python3
"""Multi-scale set abstraction against the path it replaces, on one MI355X: the PointNet2 with the MSG tables (whole
net), its two set-abstraction modules alone, and gldm_ball_query_multi against one gldm_ball_query per radius.  Inputs
and timing as tools/bench_encoders.py (randn [B, 10, 1024], device events around one call, warm-up first).

`--package-root DIR` imports graspldm_amd from another checkout that holds a built library: the commit before the
multi-scale path has no PointNet2MSG, and its time is that of PointNet2(sa_blocks=MSG tables, ...,
with_one_hot_shape_id=True, num_shapes=4), which this tool builds whenever the package lacks the class.  One process
times one package; alternate the two in one session and compare the medians of the rounds against their spread:

    for r in 1 2 3; do
      python tools/bench_msg.py --package-root ../parent --batch 16 >> profiles/msg_bench_raw.txt
      python tools/bench_msg.py --batch 16 >> profiles/msg_bench_raw.txt
    done
    python tools/bench_msg.py --batch 256 >> profiles/msg_bench_raw.txt
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

SA = [(None, (512, [0.1, 0.2, 0.4], [32, 64, 128], [(32, 32, 64), (64, 64, 128), (64, 96, 128)])),
      (None, (128, [0.4, 0.8], [64, 128], [(128, 128, 256), (128, 196, 256)])),
      (None, (None, None, None, (256, 512, 1024)))]
FP = [((256, 256), None), ((256, 128), None), ((128, 128, 128), None)]


def timed(fn, iters, warm, rounds):
    """Median of `iters` device-event timings (ms), `rounds` times: the spread of the rounds is the noise floor."""
    out = []
    with torch.inference_mode():
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            t = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
            out.append(round(float(np.median(t)), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, nargs="+", default=[16])
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    sys.path.insert(0, os.path.abspath(args.package_root))
    from graspldm_amd import pvcnn
    from graspldm_amd.backend import _backend
    from graspldm_amd.synthetic import load_synthetic_weights
    fused = hasattr(pvcnn, "PointNet2MSG")
    net = pvcnn.PointNet2MSG(num_shapes=4) if fused else \
        pvcnn.PointNet2(sa_blocks=SA, fp_blocks=FP, with_one_hot_shape_id=True, num_shapes=4)
    net = load_synthetic_weights(net, seed=0).cuda().eval()
    t = lambda fn, it=args.iterations: timed(fn, it, args.warmup, args.rounds)
    for b in args.batch:
        torch.manual_seed(0)
        x = torch.randn(b, 10, 1024, device="cuda")
        coords, feats = x[:, :3].contiguous(), x[:, 3:6].contiguous()
        with torch.inference_mode():
            f1, c1 = net.sa_layers[0]((feats, coords))
            c2 = pvcnn.furthest_point_sample(c1, 128)
            out = net(x)
        r = dict(path="multi-scale fused" if fused else "per-scale (grouped tensor, cat)", clouds=b, unit="ms, median per round",
                 net=t(lambda: net(x)), sa1=t(lambda: net.sa_layers[0]((feats, coords))),
                 sa2=t(lambda: net.sa_layers[1]((f1, c1))), checksum=float(out.double().abs().sum()))
        for name, pts, ctr, radii, us in (("bq_sa1", coords, c1, SA[0][1][1], SA[0][1][2]), ("bq_sa2", c1, c2, SA[1][1][1], SA[1][1][2])):
            r[name + "_per_radius"] = t(lambda: [_backend.ball_query(ctr, pts, rr, u) for rr, u in zip(radii, us)], 2 * args.iterations)
            if fused:
                r[name + "_multi"] = t(lambda: _backend.ball_query_multi(ctr, pts, radii, us), 2 * args.iterations)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
