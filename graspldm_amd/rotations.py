"""`tmrp_to_H` (grasp_ldm/utils/rotations.py:298-302: MRP -> quaternion -> SciPy-convention
rotation matrix -> 4x4) on the GPU via gldm_pose_epilogue, and its inverse `H_to_tmrp` (:305-309 with rotmat_to_mrp
:115-163) via gldm_pose_prologue."""
import torch

from .r1d import pose_epilogue, pose_prologue


def tmrp_to_H(tmrp):
    if not tmrp.is_cuda:
        raise RuntimeError("tmrp must be a CUDA tensor (graspldm_amd has no CPU path)")
    shape = tmrp.shape[:-1]
    flat = tmrp.reshape(-1, tmrp.shape[-1])[:, :6].contiguous().float()
    n = flat.shape[0]
    zeros = torch.zeros(1, 6, device=tmrp.device)
    ones = torch.ones(1, 6, device=tmrp.device)
    H, _, _ = pose_epilogue(flat, None, zeros, ones, max(n, 1))
    return H.view(*shape, 4, 4)


def H_to_tmrp(H):
    """[..., 4, 4] -> [..., 6] = (t, mrp).  Like the reference not canonicalised: the shadow set (|m| > 1) comes back when
    the chosen branch of rotmat_to_mrp gives a negative w."""
    if not H.is_cuda:
        raise RuntimeError("H must be a CUDA tensor (graspldm_amd has no CPU path)")
    shape = H.shape[:-2]
    flat = H.reshape(-1, 4, 4)
    n = flat.shape[0]
    if n == 0:
        return torch.empty(*shape, 6, dtype=torch.float32, device=H.device)
    zeros = torch.zeros(1, 6, device=H.device)
    ones = torch.ones(1, 6, device=H.device)
    return pose_prologue(flat, None, zeros, ones, n).view(*shape, 6)
