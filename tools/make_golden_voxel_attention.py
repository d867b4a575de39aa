"""Capture the golden vectors of voxel attention inside PVConv from the reference's own Python.  CONTAINER-ONLY (needs the
reference checkout, like tools/make_golden_attention.py whose shims and weight recipe it shares); run from the repo root:

    python tools/make_golden_voxel_attention.py

  schema_pvcnn2_attn.json   state-dict key -> (shape, dtype) of PVCNN2(use_attention=True, width_multiplier=0.5,
                            voxel_resolution_multiplier=0.5)
  pvconv_attn.npz           PVConv(32, 32, 3, resolution=r, use_attention=True, with_se=True, with_se_relu=True).eval() for
                            r = 4 and 8, recipe weights (seed 0), on 2 clouds x 256 points: features from
                            torch.Generator seed 47 (not stored), coords = synthetic clouds 0 and 1 (not stored).
                            y_r4 / y_r8: the f32 output, every 8th point; d_r4 / d_r8: the reference's f32 voxel stack
                            against a .double() copy of it on the same (f32) voxel grid, max abs over the grid
  pvcnn2_attn.npz           the PVCNN2 of the schema (recipe weights, seed 0) on synthetic clouds 0 and 1 (1024 points,
                            as the encoder sees them): out = its features, every 16th point; d = the f32 voxel stack of
                            its attention PVConv (sa_layers.1.0: C = 32, r = 8, 512 tokens) against a .double() copy on the
                            voxel grid it saw in that forward

Fixtures hold expected outputs only; the inputs are their seeds (data, no reference source).
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
FEATURE_SEED, N_POINTS = 47, 256


def _save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrays.items()})
    print(f"  {name:32s} {os.path.getsize(path) / 1024:8.1f} KiB")


def pvconv_inputs():
    """(features [2, 32, 256], coords [2, 3, 256]) of pvconv_attn.npz (the test draws the same)."""
    feats = torch.randn(2, 32, N_POINTS, generator=torch.Generator().manual_seed(FEATURE_SEED))
    pcs, _ = synthetic.synthetic_batch(2, N_POINTS)
    return feats, pcs.transpose(1, 2).contiguous()


def stack_error(pvconv, features, coords):
    """max |voxel_layers(vox) - voxel_layers.double()(vox.double())| on the module's own f32 voxel grid."""
    vox, _ = pvconv.voxelization(features, coords)
    y32 = pvconv.voxel_layers(vox)
    y64 = copy.deepcopy(pvconv.voxel_layers).double()(vox.double())
    return float((y32.double() - y64).abs().max())


@torch.no_grad()
def pvconv_golden():
    from grasp_ldm.models.modules.ext.pvcnn.modules.pvconv import PVConv
    feats, coords = pvconv_inputs()
    out = {}
    for r in (4, 8):
        m = PVConv(32, 32, 3, resolution=r, use_attention=True, with_se=True, with_se_relu=True)
        synthetic.load_synthetic_weights(m, seed=0)
        m.eval()
        y, _ = m((feats, coords))
        out[f"y_r{r}"], out[f"d_r{r}"] = y[:, :, ::8], stack_error(m, feats, coords)
        print(f"  PVConv r = {r}: d = {out[f'd_r{r}']:.3e}")
    _save("pvconv_attn.npz", **out)


@torch.no_grad()
def pvcnn2_golden():
    from grasp_ldm.models.modules.ext.pvcnn.pvcnn_base import PVCNN2
    net = PVCNN2(use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    synthetic.load_synthetic_weights(net, seed=0)
    net.eval()
    with open(os.path.join(OUT, "schema_pvcnn2_attn.json"), "w") as f:
        json.dump({k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()}, f, indent=0)
    seen = []
    block = net.sa_layers[1][0]
    hook = block.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    pcs, _ = synthetic.synthetic_batch(2, 1024)
    out = net(pcs.transpose(1, 2).contiguous())
    hook.remove()
    d = stack_error(block, *seen[0])
    print(f"  PVCNN2 attention PVConv {tuple(seen[0][0].shape)} at r = {block.resolution}: d = {d:.3e}")
    _save("pvcnn2_attn.npz", out=out[:, :, ::16], d=d)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    pvconv_golden()
    pvcnn2_golden()
