"""TEST INFRASTRUCTURE: the deprojection of a depth frame restated in torch (CPU, f32), written from the arithmetic
contract of gldm_depth_to_cloud (include/gldm.h) and pinned to the reference's Camera.depth_to_pointcloud_torch by
tests/golden/depth_cloud.npz (tests/test_depth_cpu.py).  Every step is one elementwise f32 op, in the order of the
contract: window, mask, x / y / z, transform, box; kept pixels in ascending pixel index."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def deproject(depth, K, mask=None, z_range=None, depth_scale=None, cam_to_world=None, crop_box=None):
    """depth [H, W] (f32 metres, or integer raw units with depth_scale) -> (points [n, 3] f32, pixel [n] int32)."""
    depth = torch.as_tensor(depth)
    h, w = depth.shape
    d = depth.to(torch.float32)
    if depth_scale is not None:
        d = d * _f32(depth_scale)
    z_min, z_max = (0.0, FLT_MAX) if z_range is None else z_range
    keep = (d > _f32(z_min)) & (d <= _f32(z_max))
    if mask is not None:
        keep = keep & (torch.as_tensor(mask) != 0)
    fx, fy, cx, cy = (_f32(K[0][0]), _f32(K[1][1]), _f32(K[0][2]), _f32(K[1][2]))
    u = torch.arange(w, dtype=torch.float32).expand(h, w)
    v = torch.arange(h, dtype=torch.float32).unsqueeze(1).expand(h, w)
    x = ((u - cx) * d) / fx
    y = ((v - cy) * d) / fy
    z = d
    if cam_to_world is not None:
        T = torch.as_tensor(np.asarray(cam_to_world, dtype=np.float32))[:3]
        x, y, z = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
    if crop_box is not None:
        lo, hi = [[_f32(c) for c in side] for side in crop_box]
        for p, a, b in zip((x, y, z), lo, hi):
            keep = keep & (p >= a) & (p <= b)
    flat = keep.reshape(-1)
    pix = torch.nonzero(flat).reshape(-1)
    pts = torch.stack([x.reshape(-1)[pix], y.reshape(-1)[pix], z.reshape(-1)[pix]], dim=1)
    return pts.contiguous(), pix.to(torch.int32)
