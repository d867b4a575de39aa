"""Capture the golden vectors of the global-attention path from the reference's own Python.  CONTAINER-ONLY (needs the
reference checkout, like oracle/make_golden.py whose shims and weight recipe it uses); run from the repo root:

    python tools/make_golden_attention.py

  schema_pvcnn_encoder_attn.json   state-dict key -> (shape, dtype) of PVCNNEncoder(fpc args, use_global_attention=True)
  attention_block.npz              modules.Attention(64, 8, D=1) on x1 (2, 64, 192) and Attention(32, 8, D=3) on x3
                                   (2, 32, 4, 4, 4): recipe weights (seed 0) under the keys `global_attention.*`, inputs
                                   from torch.Generator seeds 41 / 43 (not stored), the f32 outputs y1 / y3
  pvcnn_encoder_attn.npz           the encoder's latent z [2, 3, 64] on synthetic clouds 0 and 1 (recipe weights, seed 0) at
                                   n_points = 1024 and 64; z_f64tail: everything behind the reference's f32 conv_downscale
                                   output re-evaluated in f64 by .double() copies of its own modules; d = max|z - z_f64tail|
                                   (d is the f32 rounding of the reference's own tail: it moves with the BLAS thread count
                                   and blocking, 0.7e-6 .. 1.4e-6 seen; captured with 8 threads)

Fixtures hold inputs and expected outputs only (data, no reference source).
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graspldm_amd import synthetic  # noqa: E402
from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FPC = dict(in_features=3, out_features=64, scale_channels=0.75, scale_voxel_resolution=0.75, num_blocks=(1, 1, 1, 1),
           out_channels=3, use_global_attention=True)


def _save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrays.items()})
    print(f"  {name:32s} {os.path.getsize(path) / 1024:8.1f} KiB")


def attention_weights(module, seed=0):
    """Recipe weights for an Attention block, drawn under the keys it has inside an encoder."""
    sd = {k: synthetic.synthetic_tensor("global_attention." + k, v.shape, seed=seed) for k, v in module.state_dict().items()}
    module.load_state_dict(sd, strict=True)
    return module.eval()


def block_inputs():
    """x1 (2, 64, 192) and x3 (2, 32, 4, 4, 4) of attention_block.npz (the test draws the same)."""
    return (torch.randn(2, 64, 192, generator=torch.Generator().manual_seed(41)),
            torch.randn(2, 32, 4, 4, 4, generator=torch.Generator().manual_seed(43)))


@torch.no_grad()
def block_golden():
    from grasp_ldm.models.modules.modules import Attention
    x1, x3 = block_inputs()
    y1 = attention_weights(Attention(64, 8, D=1))(x1)
    y3 = attention_weights(Attention(32, 8, D=3))(x3)
    _save("attention_block.npz", y1=y1, y3=y3)   # the inputs are their seeds: block_inputs() regenerates them bit for bit


@torch.no_grad()
def encoder_golden():
    from grasp_ldm.models.modules.pc_encoders import PVCNNEncoder
    out = {}
    for n in (1024, 64):
        enc = PVCNNEncoder(n_points=n, **FPC)
        synthetic.load_synthetic_weights(enc, seed=0)
        enc.eval()
        if n == 1024:
            with open(os.path.join(OUT, "schema_pvcnn_encoder_attn.json"), "w") as f:
                json.dump({k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in enc.state_dict().items()}, f,
                          indent=0)
        pcs, _ = synthetic.synthetic_batch(2, n)
        z = enc(pcs)
        feats = enc.conv_downscale(enc.pvcnn_modules(pcs.transpose(1, 2).contiguous()))
        att, tail = copy.deepcopy(enc.global_attention).double(), copy.deepcopy(enc.out_layer).double()
        z64 = tail(att(feats.double()))
        out[f"z_{n}"], out[f"z_f64tail_{n}"] = z, z64
        out[f"d_{n}"] = float((z.double() - z64).abs().max())
        print(f"  n_points {n}: d = max|z - z_f64tail| = {out[f'd_{n}']:.3e}")
    _save("pvcnn_encoder_attn.npz", **out)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    block_golden()
    encoder_golden()
