#!/usr/bin/env python3
"""Timing of grasp selection (graspldm_amd/grasp_select.py, csrc/grasp_select.hip) on one MI355X.  HIP events around warmed
calls, medians of --iterations, as tools/bench_classifier.py.

  clearance   gldm_grasp_clearance at 256 clouds x 20 poses, for a scene of 1024 points (the object cloud alone) and of
              65,536 points (object + table + clutter), beside the plain torch expression for the same numbers on the same
              GPU, chunked over poses so that its [poses, Ns, segments] temporaries fit in --torch_bytes.  Reported: both
              times, their ratio, (pose, point) pairs per second and that rate against the f32 VALU peak at
              FLOP_PER_PAIR flop per pair (a pair that reaches the narrow phase: 26 flop to place the point and test the
              bounding sphere + 23 per segment, six segments; a skipped pair costs the 26 only, so for the large scene the
              figure is an effective rate).
  diverse     gldm_select_grasps mode 1 at 256 clouds x 200 candidates -> 20, and mode 0 on the same candidates.
  end to end  on --e2e_clouds clouds x 20 poses: clearance + diverse selection of --e2e_keep poses + score_poses on those,
              against score_poses on all 20.

    python tools/bench_grasp_select.py --out profiles/grasp_select_bench.json"""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import gripper  # noqa: E402
from graspldm_amd.grasp_select import grasp_clearance, select_grasps  # noqa: E402
from graspldm_amd.synthetic import PC_STD, _random_rotation  # noqa: E402

PEAK_VALU_TFLOPS = 157.3
FLOP_PER_PAIR = 26 + 23 * 6


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


def torch_clearance(scene, H, body, sweep, r_sweep, cap, max_bytes):
    """The same two numbers as one torch expression per chunk of poses (f32)."""
    b, g = H.shape[:2]
    ns = scene.shape[1]
    seg = torch.cat([body, sweep])
    a, ab = seg[:, 0], seg[:, 1] - seg[:, 0]
    inv = 1.0 / (ab * ab).sum(-1)
    per_pose = ns * seg.shape[0] * 4 * 8            # qa, u, w and their products: about eight [Ns, S(,3)] f32 temporaries
    step = max(1, int(max_bytes // (per_pose * 3)))
    clear = torch.empty(b, g, device=H.device)
    contacts = torch.empty(b, g, dtype=torch.int32, device=H.device)
    for c in range(b):
        for g0 in range(0, g, step):
            Hc = H[c, g0:g0 + step]
            q = torch.einsum("gji,gnj->gni", Hc[:, :3, :3], scene[c][None] - Hc[:, None, :3, 3])
            qa = q[:, :, None, :] - a
            u = ((qa * ab).sum(-1) * inv).clamp(0.0, 1.0)
            w = qa - u[..., None] * ab
            d2 = (w * w).sum(-1)
            clear[c, g0:g0 + step] = d2[..., :body.shape[0]].amin(dim=(1, 2)).sqrt().clamp(max=cap)
            contacts[c, g0:g0 + step] = (d2[..., body.shape[0]:].amin(-1) <= r_sweep * r_sweep).sum(-1)
    return clear, contacts


def make_inputs(bc, g, ns, seed=0):
    """Object clouds of 1024 points (0.05 randn + offset); beyond that a 1 m x 1 m table under the object and clutter blobs.
    Poses at the object's mean + 0.06 randn with random rotations."""
    gen = torch.Generator().manual_seed(seed)
    n_obj = min(ns, 1024)
    obj = 0.05 * torch.randn(bc, n_obj, 3, generator=gen) + 0.2 * torch.rand(bc, 1, 3, generator=gen)
    parts = [obj]
    if ns > n_obj:
        n_table = (ns - n_obj) // 2
        table = torch.rand(bc, n_table, 3, generator=gen) - 0.5
        table[..., 2] = 0.002 * torch.randn(bc, n_table, generator=gen) - 0.15
        n_cl = ns - n_obj - n_table
        centres = torch.rand(bc, 16, 3, generator=gen) - 0.5
        clutter = centres[:, torch.arange(n_cl) % 16] + 0.04 * torch.randn(bc, n_cl, 3, generator=gen)
        parts += [table + obj.mean(1, keepdim=True), clutter + obj.mean(1, keepdim=True)]
    scene = torch.cat(parts, dim=1)
    H = torch.zeros(bc, g, 4, 4)
    for c in range(bc):
        for i in range(g):
            H[c, i, :3, :3] = _random_rotation(gen).float()
    H[:, :, :3, 3] = obj.mean(1)[:, None] + 0.06 * torch.randn(bc, g, 3, generator=gen)
    H[:, :, 3, 3] = 1.0
    return scene, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=256)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--candidates", type=int, default=200)
    ap.add_argument("--e2e_clouds", type=int, default=32)
    ap.add_argument("--e2e_keep", type=int, default=5)
    ap.add_argument("--torch_bytes", type=float, default=2e9)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--time_limit", type=int, default=420, help="seconds after which the run aborts itself")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    signal.alarm(args.time_limit)
    bc, g = args.clouds, args.poses
    out = dict(clouds=bc, poses=g, gpu=torch.cuda.get_device_name(), flop_per_pair=FLOP_PER_PAIR)
    body = torch.tensor(gripper.OPEN_SEGMENTS).cuda()
    sweep = torch.tensor(gripper.SWEEP_SEGMENTS).cuda()
    for ns in (1024, 65536):
        scene, H = make_inputs(bc, g, ns)
        scene, H = scene.cuda(), H.cuda()
        ours = lambda: grasp_clearance(scene, H)   # noqa: E731
        plain = lambda: torch_clearance(scene, H, body, sweep, 0.006, 0.05, args.torch_bytes)   # noqa: E731
        t_ours = timed(ours, args.iterations, args.warmup)
        t_plain = timed(plain, max(2, args.iterations // 5), 1)
        a, b = ours(), plain()
        pairs = bc * g * ns
        out[f"clearance_ns{ns}"] = dict(
            kernel_ms=t_ours, torch_ms=t_plain, ratio=t_plain[0] / t_ours[0], pairs_per_s=pairs / (t_ours[0] * 1e-3),
            frac_of_valu_peak=pairs * FLOP_PER_PAIR / (t_ours[0] * 1e-3) / (PEAK_VALU_TFLOPS * 1e12),
            max_abs_diff_vs_torch=float((a[0] - b[0]).abs().max()), contacts_differ=int((a[1] != b[1]).sum()),
            colliding=int((a[0] <= 0.006).sum()), capped=int((a[0] == 0.05).sum()))
    # selection launches
    _, Hs = make_inputs(bc, args.candidates, 1024, seed=1)
    Hs = Hs.cuda()
    score = torch.rand(bc, args.candidates, generator=torch.Generator().manual_seed(2)).cuda()
    out["diverse_ms"] = timed(lambda: select_grasps(Hs, score, k=g, diverse=True), args.iterations, args.warmup)
    out["topk_ms"] = timed(lambda: select_grasps(Hs, score, k=g), args.iterations, args.warmup)
    out["candidates"] = args.candidates
    # selection in front of the classifier
    from graspldm_amd.pipeline import build_classifier
    ec, keep_n = args.e2e_clouds, args.e2e_keep
    model = build_classifier(1024, 64, "PVCNN").cuda()
    scene, H = make_inputs(ec, g, 1024, seed=3)
    scene, H = scene.cuda(), H.cuda()
    mean = scene.mean(1)
    pc = (scene - mean[:, None]) / PC_STD
    conf = torch.rand(ec, g, generator=torch.Generator().manual_seed(4)).cuda()
    score_all = lambda: model.score_poses(pc, H, pc_mean=mean, pc_scale=PC_STD)   # noqa: E731

    def selected():
        clear, contacts = grasp_clearance(scene, H)
        index, count, _ = select_grasps(H, conf, keep=clear > 0.006, k=keep_n, diverse=True)
        idx = index.long().clamp(min=0)
        return model.score_poses(pc, H.gather(1, idx.view(ec, keep_n, 1, 1).expand(-1, -1, 4, 4)), pc_mean=mean, pc_scale=PC_STD)

    n_it = max(3, args.iterations // 3)
    out["e2e"] = dict(clouds=ec, poses=g, kept=keep_n, score_all_ms=timed(score_all, n_it, 1), select_then_score_ms=timed(selected, n_it, 1))
    out["e2e"]["ratio"] = out["e2e"]["score_all_ms"][0] / out["e2e"]["select_then_score_ms"][0]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
