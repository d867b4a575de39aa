"""Capture the golden vectors of Unet1D from the reference's own Python.  CONTAINER-ONLY (needs the reference checkout,
like tools/make_golden_msg.py); run from the repo root:

    python tools/make_golden_unet1d.py

  schema_unet1d.json   per golden configuration (tests/unet1d_ref.py: CASES) the reference module's state-dict key -> shape
  unet1d.npz           per configuration X: X_out = the reference module's output on the first GOLDEN_ROWS rows of
                       case_inputs(X, .) (recipe weights, seed = the case's), X_d = max |restatement f32 - restatement f64|
                       on the same rows, the f64 copy fed the f32 time-embedding rows (both implementations take those from the
                       same f32 host computation; without this the sin / cos of t * w * 2 pi dominates: 1e-5 .. 3e-5)

  unet1d_vae.npz       the reference's GraspCVAE of the shipped fpc config with a Unet1D pose decoder and grasp encoder
                       (dim_mults (1, 2, 4, 8), no time conditioning, groups 4; recipe weights, seed 0) on 2 synthetic clouds
                       x 4 grasps: mu, logvar, eps, z of encode(); tmrp, logit of forward(compute_loss=False) under the same
                       seed; gen_tmrp, gen_logit = decoder(z_h, cond) for the stored z_h; the grasp rows h.  Its decoder /
                       encoder state-dict keys are the schema's "VAE" entry.

Inputs are not stored: tests/unet1d_ref.case_inputs draws them.  The reference's own .double() copy is NOT the yardstick: its
weight-standardisation and LayerNorm eps switch from 1e-5 to 1e-3 off f32 (resnets.py:86,110).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from graspldm_amd import synthetic  # noqa: E402
from oracle import ref_import  # noqa: E402
import unet1d_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


@torch.no_grad()
def unet_golden(vae_keys):
    from grasp_ldm.models.modules.resnets import Unet1D
    schema, arrays = {}, {}
    for name, c in unet1d_ref.CASES.items():
        net = synthetic.load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"]).eval()
        sd = {k: v.detach() for k, v in net.state_dict().items()}
        schema[name] = {k: list(v.shape) for k, v in sd.items()}
        x, z, t = unet1d_ref.case_inputs(name, unet1d_ref.GOLDEN_ROWS)
        out = net(x, time=t, z_cond=z)
        groups = c["args"]["resnet_block_groups"]
        r32 = unet1d_ref.unet1d_forward(sd, "", x, z, t, groups=groups)
        temb = unet1d_ref.unet_time_embedding(sd, "", t).double() if t is not None else None
        r64 = unet1d_ref.unet1d_forward({k: v.double() for k, v in sd.items()}, "", x.double(),
                                        z.double() if z is not None else None, t, groups=groups, temb=temb)
        d = float((r32.double() - r64).abs().max())
        print(f"  case {name}: out {tuple(out.shape)}, max |out| {float(out.abs().max()):.3f}, "
              f"|reference - restatement| {float((out - r32).abs().max()):.1e}, d = {d:.2e}")
        arrays[name + "_out"], arrays[name + "_d"] = out.numpy(), np.float64(d)
    schema["VAE"] = vae_keys
    with open(os.path.join(OUT, "schema_unet1d.json"), "w") as f:
        json.dump(schema, f, indent=0)
    np.savez_compressed(os.path.join(OUT, "unet1d.npz"), **arrays)


VAE_CORE = dict(dim_mults=(1, 2, 4, 8), input_conditioning_dims=64, is_time_conditioned=False, resnet_block_groups=4)
VAE_SEED = 1234


@torch.no_grad()
def vae_golden():
    from grasp_ldm.models.builder import build_model_from_cfg
    cfg = ref_import.load_reference_config("configs/generation/fpc/fpc_1a_latentc3_z4_pc64_180k.py")
    a = cfg.model.vae.model.args
    a.grasp_encoder_config = dict(type="Unet1D", args=dict(in_features=7, **VAE_CORE))
    a.decoder_config = dict(type="Unet1D", args=dict(**VAE_CORE))
    vae = synthetic.load_synthetic_weights(build_model_from_cfg(cfg.model.vae), seed=0).eval()
    keys = {k: list(v.shape) for k, v in vae.state_dict().items() if k.startswith(("decoder.", "encoder.grasp_encoder."))}
    pcs, _ = synthetic.synthetic_batch(2, 1024)
    g = torch.Generator().manual_seed(41)
    h = torch.randn(8, 7, generator=g)
    h[:, 6] = (torch.rand(8, generator=g) < 0.75).float()
    z_h = torch.randn(8, 4, generator=g)
    torch.manual_seed(VAE_SEED)
    (mu, logvar, z), (_, _, z_pc) = vae.encode(pcs, h)
    torch.manual_seed(VAE_SEED)
    eps = torch.randn(8, 4)
    assert torch.equal(mu + eps * torch.exp(0.5 * logvar), z), "eps is not the reference's draw"
    torch.manual_seed(VAE_SEED)
    tmrp, logit = vae(pcs, h, compute_loss=False)
    gen_tmrp, gen_logit = vae.decoder(z_h, cond=z_pc)
    np.savez_compressed(os.path.join(OUT, "unet1d_vae.npz"), h=h.numpy(), z_h=z_h.numpy(), mu=mu.numpy(), logvar=logvar.numpy(),
                        eps=eps.numpy(), z=z.numpy(), tmrp=tmrp.numpy(), logit=logit.numpy(), gen_tmrp=gen_tmrp.numpy(),
                        gen_logit=gen_logit.numpy())
    print(f"  VAE with Unet1D cores: {len(keys)} decoder / grasp-encoder keys, max |tmrp| {float(tmrp.abs().max()):.3f}")
    return keys


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    unet_golden(vae_golden())
