"""Capture the golden vectors of the grasp success classifier from the reference's own Python.  CONTAINER-ONLY (needs the
reference checkout, like oracle/make_golden.py whose shims and weight recipe it uses); run from the repo root:

    python tools/make_golden_classifier.py

  schema_grasp_classifier.json   {"PVCNN" | "PVCNN2": state-dict key -> (shape, dtype)} of PointsBasedGraspClassifier with the
                                 backbones of cases a / c
  grasp_classifier.npz           the reference model with recipe weights (seed 0) on synthetic clouds 0, 1 (not stored:
                                 synthetic.synthetic_batch regenerates them), cloud c repeated for its G poses:
      a  PVCNN (0.25 / 0.75, blocks (1,1,1,1), 1 extra channel)  N = 1024 + 64, 2 clouds x 2 poses
      b  the same                                                N =   64 + 12, 2 x 2   (tail columns, N % 32 != 0)
      c  PVCNN2 (1 extra channel)                                N = 1024 + 64, 2 x 1
    per case X: X_H [Bc*G,4,4] poses in the un-normalised cloud frame (random rotations, translations near the cloud;
    X_seed is the generator seed that passed the two conditions below), X_gripper [Ng,3], X_grasp_points [Bc*G,Ng,3] (f32,
    normalised frame), X_logit, X_prob [Bc*G], X_logit_f64tail (the reference's f32 backbone output through .double()
    copies of its own `classifier`), X_d = max|logit - logit_f64tail| (the f32 rounding of the reference's own tail).

Conditions on the INPUTS, asserted here (the seed is redrawn until both hold): no point of a merged scene lies within 1e-4
of a voxel rounding boundary in any Voxelization of the backbone (two f32 implementations may then round it to different
voxels), and every |logit| <= 20 (prob is not saturated).

Reported and stored, not a condition: X_sens, the largest move of the reference's OWN logit when the gripper points are
rounded differently (evaluated in f64 and rounded once; three random +-1 ulp perturbations).  PVCNN: 5e-7 / 1e-6.  PVCNN2:
1.2e-4 at the seed kept, 4e-5 .. 2e-4 at every seed of 100..199 that passes the two conditions -- farthest-point sampling
and ball queries SELECT points, evenly spaced gripper points make near-ties, and the selection flips with the last bit of
a coordinate.  Two f32 evaluations of the points that differ in one rounding do not agree on such a scene to better than
that: gldm_grasp_scene therefore walks the order used here (products in k order, then the translation, the mean, the
scale), and tests/test_classifier_gpu.py checks its points against the stored grasp_points bit for bit.

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

from graspldm_amd import gripper, synthetic  # noqa: E402
from graspldm_amd.pipeline import classifier_model_config  # noqa: E402
from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = (("a", "PVCNN", 1024, 64, 2, 2), ("b", "PVCNN", 64, 12, 2, 2), ("c", "PVCNN2", 1024, 64, 2, 1))
TIE_MARGIN, LOGIT_MAX = 1e-4, 20.0


def draw_poses(seed, clouds_raw, g):
    """[Bc*G, 4, 4] f32: uniform random rotations, translations = a point 0.06 m (normal, per axis) around the cloud's mean."""
    gen = torch.Generator().manual_seed(seed)
    H = torch.zeros(clouds_raw.shape[0] * g, 4, 4, dtype=torch.float64)
    for i in range(H.shape[0]):
        H[i, :3, :3] = synthetic._random_rotation(gen)
        H[i, :3, 3] = clouds_raw[i // g].double().mean(0) + 0.06 * torch.randn(3, generator=gen, dtype=torch.float64)
        H[i, 3, 3] = 1.0
    return H.float()


def reference_model(backbone, n_cloud, n_grip):
    from grasp_ldm.models.builder import build_model_from_cfg
    from grasp_ldm.utils.config import ConfigDict
    cfg = ConfigDict(classifier_model_config(n_cloud, n_grip, backbone))
    model = build_model_from_cfg(cfg)
    model = model["model"] if isinstance(model, dict) else model
    synthetic.load_synthetic_weights(model, seed=0)
    return model.eval()


def scene_logit(model, pc_rep, pts):
    x = torch.cat((torch.cat((pc_rep, torch.zeros_like(pc_rep[..., :1])), -1),
                   torch.cat((pts, torch.ones_like(pts[..., :1])), -1)), -2).transpose(1, 2).contiguous()
    return model.classifier(model.base_network(x)).reshape(-1)


def sensitivity(model, pc_rep, pts, H, gp, mean, logit, seed):
    """Largest move of the reference's logit under other roundings of the gripper points (see the module docstring)."""
    exact = torch.einsum("bij,nj->bni", H[:, :3, :3].double(), gp.double()) + H[:, None, :3, 3].double()
    exact = ((exact - mean.double()[:, None]) / float(np.float32(synthetic.PC_STD))).float()
    worst = float((scene_logit(model, pc_rep, exact) - logit).abs().max())
    gen = torch.Generator().manual_seed(seed)
    up, down = torch.full_like(pts, float("inf")), torch.full_like(pts, -float("inf"))
    for _ in range(3):
        sgn = torch.randint(0, 3, pts.shape, generator=gen) - 1
        pert = torch.where(sgn > 0, torch.nextafter(pts, up), torch.where(sgn < 0, torch.nextafter(pts, down), pts))
        worst = max(worst, float((scene_logit(model, pc_rep, pert) - logit).abs().max()))
    return worst


@torch.no_grad()
def run_case(model, n_cloud, n_grip, g):
    from grasp_ldm.models.modules.ext.pvcnn.modules.voxelization import Voxelization
    pcs, metas = synthetic.synthetic_batch(2, n_cloud)
    raw = pcs * synthetic.PC_STD + metas["pc_mean"].unsqueeze(1)
    gp = gripper.control_points(n_grip)
    margins = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: margins.append(float(((out[1] - torch.floor(out[1])) - 0.5).abs().min())))
             for m in model.modules() if isinstance(m, Voxelization)]
    try:
        for seed in range(100, 200):
            del margins[:]
            H = draw_poses(seed, raw, g)
            mean = metas["pc_mean"].repeat_interleave(g, 0)
            pts = torch.einsum("bij,nj->bni", H[:, :3, :3], gp) + H[:, None, :3, 3]
            pts = (pts - mean[:, None] - 0.0) / synthetic.PC_STD
            pc_rep = pcs.repeat_interleave(g, 0)
            _, prob = model(pc_rep, pts, compute_loss=False)
            x = torch.cat((torch.cat((pc_rep, torch.zeros_like(pc_rep[..., :1])), -1),
                           torch.cat((pts, torch.ones_like(pts[..., :1])), -1)), -2).transpose(1, 2).contiguous()
            feats = model.base_network(x)
            logit = model.classifier(feats).reshape(-1)
            assert torch.equal(torch.sigmoid(logit), prob.reshape(-1))
            margin = min(margins)
            if margin >= TIE_MARGIN and float(logit.abs().max()) <= LOGIT_MAX:
                break
            print(f"    seed {seed}: margin {margin:.2e}, max|logit| {float(logit.abs().max()):.2f}: redrawn")
        else:
            raise AssertionError("no seed in 100..199 satisfies the tie / saturation conditions")
    finally:
        for h in hooks:
            h.remove()
    assert margin >= TIE_MARGIN and float(logit.abs().max()) <= LOGIT_MAX
    sens = sensitivity(model, pc_rep, pts, H, gp, mean, logit, seed)
    l64 = copy.deepcopy(model.classifier).double()(feats.double()).reshape(-1)
    d = float((logit.double() - l64).abs().max())
    print(f"    seed {seed}: voxel margin {margin:.2e}, sens {sens:.2e}, logit {logit.tolist()}, d = {d:.3e}")
    return dict(seed=seed, sens=sens, H=H, gripper=gp, grasp_points=pts, logit=logit, prob=prob.reshape(-1), logit_f64tail=l64, d=d)


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    schema, out = {}, {}
    for name, backbone, n_cloud, n_grip, _, g in CASES:
        print(f"  case {name}: {backbone} at {n_cloud} + {n_grip}")
        model = reference_model(backbone, n_cloud, n_grip)
        if n_cloud == 1024:
            schema[backbone] = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
        for k, v in run_case(model, n_cloud, n_grip, g).items():
            out[f"{name}_{k}"] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    with open(os.path.join(OUT, "schema_grasp_classifier.json"), "w") as f:
        json.dump(schema, f, indent=0)
    path = os.path.join(OUT, "grasp_classifier.npz")
    np.savez_compressed(path, **out)
    print(f"  grasp_classifier.npz {os.path.getsize(path) / 1024:8.1f} KiB")


if __name__ == "__main__":
    main()
