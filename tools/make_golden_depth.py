#!/usr/bin/env python3
"""Capture tests/golden/depth_cloud.npz from the reference's own Camera.depth_to_pointcloud_torch
(grasp_ldm/utils/camera.py:176-215).  CONTAINER-ONLY (needs the reference checkout; shims of oracle/ref_import.py);
no test imports this file.

    python tools/make_golden_depth.py

Three 48 x 64 f32 frames under one camera whose intrinsics are not representable in f32 (the reference casts its f64
scalars where they meet the f32 tensors): `sparse` (zeros, a band and scattered holes), `full` (every pixel valid) and
`empty` (all zero).  Stored: K (f64, as in the camera json), width, height, depth_<name>, points_<name>."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

H, W = 48, 64
K = [[61.537128448486328 + 1e-9, 0.0, 31.025881958 + 3e-9], [0.0, 61.3391 + 1e-7 / 3, 23.774318695 + 1e-9 / 7], [0.0, 0.0, 1.0]]


def frames():
    g = torch.Generator().manual_seed(20)
    full = 0.4 + 0.8 * torch.rand(H, W, generator=g)
    sparse = 0.3 + 1.2 * torch.rand(H, W, generator=g)
    sparse[torch.rand(H, W, generator=g) < 0.35] = 0.0   # holes
    sparse[10:14] = 0.0                                   # a band of invalid rows
    sparse[:, 0] = 0.0
    sparse[H - 1, W - 1] = 0.731                          # the last pixel is valid
    return dict(sparse=sparse, full=full, empty=torch.zeros(H, W))


def main():
    ref_import.install_shims()
    from grasp_ldm.utils.camera import Camera
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cam.json")
        with open(path, "w") as f:
            json.dump(dict(cameraMatrix=K, distCoeffs=[], width=W, height=H, hfov=55.0, vfov=42.7), f)
        cam = Camera(path)
        out = dict(K=np.asarray(K, dtype=np.float64), width=np.int32(W), height=np.int32(H))
        for name, depth in frames().items():
            pts = cam.depth_to_pointcloud_torch(depth)
            assert pts.dtype == torch.float32
            out[f"depth_{name}"] = depth.numpy()
            out[f"points_{name}"] = pts.contiguous().numpy().reshape(-1, 3)
            print(name, tuple(pts.shape))
    dst = os.path.join(ROOT, "tests", "golden", "depth_cloud.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
