"""Capture the golden vectors of the grasp-encoder path from the reference's own Python.  CONTAINER-ONLY (needs the
reference checkout, like oracle/make_golden.py whose shims and weight recipe it uses); run from the repo root:

    python tools/make_golden_encode.py            # writes tests/golden/vae_encode.npz and H_to_tmrp.npz

  vae_encode.npz   fpc config, synthetic seed-0 weights, synthetic_batch(2, 1024), 8 grasps per cloud:
                   GraspCVAE.encode (mu, logvar, z and the eps it drew) and GraspCVAE.forward(compute_loss=False)
                   (tmrp, logit), both under torch.manual_seed(1234)
  H_to_tmrp.npz    utils/rotations.H_to_tmrp on 96 poses: 64 from tmrp_to_H of seeded tmrp, 16 within 1e-3 rad of a
                   half turn (all three `choice != 3` branches), 8 identities / half turns about the axes, and LAST the
                   8 poses of the tie group (trace equal to the largest diagonal entry up to f32 rounding).  Every pose
                   of the first 88 has an arg-max margin (largest minus second largest of R00, R11, R22, trace on the
                   f32 matrix) of at least 1e-3, so f32 rounding cannot move it to another branch; margins are stored.

Fixtures hold inputs and expected outputs only (data, no reference source).
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graspldm_amd import synthetic  # noqa: E402
from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 1234
MARGIN = 1e-3


def _save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrays.items()})
    print(f"  {name:22s} {os.path.getsize(path) / 1024:8.1f} KiB")


def _margin(H):
    R = H[..., :3, :3]
    d = torch.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2], R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]], -1)
    top = d.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def _axis_angle_H(axis, angle, t):
    """Rodrigues in f64, rounded once to f32: [n,3] unit axes, [n] angles, [n,3] translations -> [n,4,4]."""
    axis, angle = axis.double(), angle.double()
    K = torch.zeros(axis.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2] = -axis[:, 2], axis[:, 1]
    K[:, 1, 0], K[:, 1, 2] = axis[:, 2], -axis[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -axis[:, 1], axis[:, 0]
    s, c = angle.sin().reshape(-1, 1, 1), angle.cos().reshape(-1, 1, 1)
    R = torch.eye(3, dtype=torch.float64) + s * K + (1 - c) * (K @ K)
    H = torch.eye(4, dtype=torch.float64).repeat(axis.shape[0], 1, 1)
    H[:, :3, :3] = R
    H[:, :3, 3] = t.double()
    return H.float()


def _redraw(draw, n):
    """n poses from draw(k) -> [k,4,4], re-drawing every one whose arg-max margin is below MARGIN."""
    H = draw(n)
    for _ in range(100):
        bad = _margin(H) < MARGIN
        if not bad.any():
            return H
        H[bad] = draw(int(bad.sum()))
    raise RuntimeError("margin re-draw did not converge")


@torch.no_grad()
def h_to_tmrp_golden():
    from grasp_ldm.utils.rotations import H_to_tmrp, tmrp_to_H
    g = torch.Generator().manual_seed(11)

    def seeded(k):
        return tmrp_to_H(torch.randn(k, 6, generator=g)).float()

    def half_turn(k):
        ax = torch.randn(k, 3, generator=g, dtype=torch.float64)
        ax = ax / ax.norm(dim=-1, keepdim=True)
        # the largest component decides the branch: rotate it through x, y, z
        big = ax.abs().argmax(dim=-1)
        want = torch.arange(k) % 3
        ax = torch.stack([ax[i].roll(int(want[i] - big[i])) for i in range(k)])
        ang = math.pi - 1e-3 * torch.rand(k, generator=g, dtype=torch.float64)
        return _axis_angle_H(ax, ang, 0.2 * torch.randn(k, 3, generator=g))

    def tie(k):
        # R_ii == trace  <=>  n_i^2 = (1 + cos) / (1 - cos); angles between 90 and 108 degrees keep n_i^2 above 1/2, so
        # that R_ii is the largest diagonal entry
        ang = math.pi * (0.5 + 0.1 * torch.rand(k, generator=g, dtype=torch.float64))
        c = ang.cos()
        ni = ((1 + c) / (1 - c)).sqrt()
        phi = 2 * math.pi * torch.rand(k, generator=g, dtype=torch.float64)
        rest = (1 - ni * ni).sqrt()
        ax = torch.stack([ni, rest * phi.cos(), rest * phi.sin()], -1)
        ax = torch.stack([ax[i].roll(i % 3) for i in range(k)])
        return _axis_angle_H(ax, ang, 0.2 * torch.randn(k, 3, generator=g))

    a = _redraw(seeded, 64)
    b = _redraw(half_turn, 16)
    e = torch.eye(3)
    axes = torch.cat([e[:1], e, e[:1], e])                        # identity (angle 0), three half turns, twice
    angs = torch.tensor([0.0, math.pi, math.pi, math.pi] * 2)
    c = _axis_angle_H(axes, angs, 0.2 * torch.randn(8, 3, generator=g))
    c[:, :3, :3] = c[:, :3, :3].round()                           # exact signed identities
    d = tie(8)
    H = torch.cat([a, b, c, d])
    m = _margin(H)
    assert (m[:88] >= MARGIN).all() and (m[88:] < 1e-6).all(), m
    tmrp = H_to_tmrp(H)
    assert tmrp.dtype == torch.float32 and torch.isfinite(tmrp).all()
    _save("H_to_tmrp.npz", H=H, tmrp=tmrp, margin=m, n_tie=np.array(8))


@torch.no_grad()
def vae_encode_golden():
    ldm = ref_import.build_reference_ldm(noise_scheduler_type="ddim")
    synthetic.load_synthetic_weights(ldm, seed=0)
    vae = ldm.vae_model.eval()
    pcs, _ = synthetic.synthetic_batch(2, 1024)
    g = torch.Generator().manual_seed(31)
    h = torch.randn(16, 7, generator=g)
    h[:, 6] = (torch.rand(16, generator=g) < 0.75).float()
    torch.manual_seed(SEED)
    (mu, logvar, z), (_, _, z_pc) = vae.encode(pcs, h)
    torch.manual_seed(SEED)
    eps = torch.randn(16, 4)                                       # the randn_like(std) of reparameterize
    assert torch.equal(mu + eps * torch.exp(0.5 * logvar), z), "eps is not the reference's draw"
    torch.manual_seed(SEED)
    tmrp, logit = vae(pcs, h, compute_loss=False)
    _save("vae_encode.npz", pc=pcs, h=h, z_pc=z_pc[::8].contiguous(), mu=mu, logvar=logvar, eps=eps, z=z,
          tmrp=tmrp, logit=logit, seed=SEED)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    h_to_tmrp_golden()
    vae_encode_golden()
