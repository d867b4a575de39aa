"""Unet1D on the fused kernel against the same net as eager torch ops on the same GPU (tests/unet1d_ref.py: one launch per
op), with the shipped ResNet1D engines at the same batch as context.  HIP events, warm-up first, median of the repeats.

    python tools/bench_unet1d.py [--n 5120] [--steps 100] [--repeats 5]

Case B (dim 16, (1, 2, 4), L 16, time + z_cond) as a DDIM launch of --steps steps; case A (dim 16, (1, 2, 4, 8), L 16,
z_cond [n, 3, 64]) as one decoder-core pass.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unet1d_ref as U  # noqa: E402
from graspldm_amd.diffusion import GaussianDiffusion1D  # noqa: E402
from graspldm_amd.resnets import Unet1D  # noqa: E402
from graspldm_amd.synthetic import load_synthetic_weights  # noqa: E402
from graspldm_amd.unet1d_pack import OP_ATT, OP_CONV  # noqa: E402

SPLIT_F16_PEAK = 2.5e15 / 3   # dense f16 matrix peak of an MI355X over the three partial products of a split product


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def program_flop(plan, n):
    """Executed matrix-pipe FLOP of one pass over n samples: 2 M K_padded columns_padded per conv op, padding included."""
    d, prog = plan["desc"], plan["ops"]
    s = d.tile_samples
    tiles = (n + s - 1) // s
    flop = 0
    for r in prog:
        if r[0] == OP_CONV:
            kb = r[10] * ((r[2] + 31) // 32 + ((r[5] + 31) // 32 if r[5] > 0 else 0))
            flop += 2 * r[8] * kb * 32 * ((s * r[12] + 15) // 16 * 16)
        elif r[0] == OP_ATT:
            cols = (s * r[4] + 15) // 16 * 16
            flop += 2 * cols * (384 * ((r[2] + 31) // 32) * 32 + r[2] * 128)
    return flop * tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5120)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, steps in (("B", a.steps), ("A", 1)):
        c = U.CASES[name]
        net = load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"]).to(dev)
        sd = {k: v.detach() for k, v in net.state_dict().items()}
        x, z, t = U.case_inputs(name, min(a.n, 4096))
        reps = (a.n + x.shape[0] - 1) // x.shape[0]
        x = x.repeat(reps, 1, 1)[:a.n].to(dev)
        z = z.repeat(reps, *([1] * (z.ndim - 1)))[:a.n].to(dev)
        groups = c["args"]["resnet_block_groups"]
        if steps > 1:
            ddm = GaussianDiffusion1D(net, n_dims=c["L"], noise_scheduler_type="ddim", beta_start=5e-5, beta_end=1e-3)
            ddm.set_inference_timesteps(steps)
            fused = lambda: ddm.sample(z_cond=z, batch_size=a.n, x_T=x)   # noqa: E731
            tb = torch.full((a.n,), 500, dtype=torch.long, device=dev)
            eager_one = lambda: U.unet1d_forward(sd, "", x, z, tb, groups=groups)   # noqa: E731
        else:
            fused = lambda: net(x, z_cond=z)   # noqa: E731
            eager_one = lambda: U.unet1d_forward(sd, "", x, z, None, groups=groups)   # noqa: E731
        with torch.no_grad():
            f_ms = timed(fused, a.repeats)
            e_ms = timed(eager_one, a.repeats) * steps     # the eager sampler is `steps` such passes plus its scheduler ops
        from graspldm_amd.unet1d_pack import pack_unet1d
        rows = 0 if z is None else (1 if z.ndim == 2 else z.shape[1])
        plan = pack_unet1d({k: v.cpu() for k, v in sd.items()}, "", groups, c["L"], cond_rows=rows,
                           time_cond=c["args"]["is_time_conditioned"], num_steps=1000)
        flop = program_flop(plan, a.n) * steps
        print(json.dumps(dict(case=name, n=a.n, steps=steps, fused_ms=round(f_ms, 3), eager_ms=round(e_ms, 3),
                              eager_over_fused=round(e_ms / f_ms, 2), tile_samples=plan["desc"].tile_samples,
                              lds_kib=plan["desc"].lds_floats * 4 / 1024, gflop=round(flop / 1e9, 2),
                              frac_of_split_f16_peak=round(flop / (f_ms * 1e-3) / SPLIT_F16_PEAK, 4))), flush=True)
    # context: the shipped ResNet1D engines at the same batch
    from graspldm_amd.pipeline import build_fpc_ldm
    ldm = build_fpc_ldm(device=dev)
    ldm.set_inference_timesteps(a.steps)
    zc = torch.randn(a.n, 3, 64, device=dev)
    xt = torch.randn(a.n, 1, 4)
    zh = torch.randn(a.n, 4, device=dev)
    with torch.no_grad():
        d_ms = timed(lambda: ldm.diffusion_model.sample(z_cond=zc, batch_size=a.n, x_T=xt), a.repeats)
        v_ms = timed(lambda: ldm.vae_model.decoder(zh, zc), a.repeats)
    print(json.dumps(dict(context="ResNet1D engines", n=a.n, gldm_denoise_ms=round(d_ms, 3), steps=a.steps,
                          gldm_decode_ms=round(v_ms, 3))), flush=True)


if __name__ == "__main__":
    main()
