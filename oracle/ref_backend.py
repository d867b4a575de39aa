"""ctypes front end of the reference's own point-op kernels, compiled for gfx950
by oracle/ref_build.py (oracle/_ref/libpvcnn_ref*.so).  TEST INFRASTRUCTURE: see
oracle/__init__.py; nothing under graspldm_amd/ may import this module.

Same seven forward names and signatures as oracle.cpu_backend._backend, on CUDA
tensors.  Two instances, one per library:

  default   the compiler's default contraction (the analogue of nvcc's fmad)
  strict    -ffp-contract=off, the arithmetic oracle/point_ops.c restates

Outputs are allocated as the reference's C++ wrappers do (zero-filled:
ball_query.cpp:20-22, vox.cpp:31-36, ...; distances = full(1e38f):
sampling.cpp:51-54).  The reference kernels index unchecked, so every index
tensor and every voxel coordinate is range-checked on the host BEFORE a launch,
and the device is synchronised before and after each call (two launchers use the
legacy default stream whatever the caller's stream is: sampling.cu:169-174,
vox.cu:114-120).
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
LIBS = {"default": "libpvcnn_ref.so", "strict": "libpvcnn_ref_strict.so"}

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_ARGTYPES = {
    "ref_set_stream": [_vp],
    "ref_ball_query": [_i, _i, _i, _f, _i, _vp, _vp, _vp],
    "ref_grouping": [_i, _i, _i, _i, _i, _vp, _vp, _vp],
    "ref_gather_features": [_i, _i, _i, _i, _vp, _vp, _vp],
    "ref_furthest_point_sampling": [_i, _i, _i, _vp, _vp, _vp],
    "ref_three_nearest_neighbors_interpolate": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "ref_trilinear_devoxelize": [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "ref_avg_voxelize": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
}


def available(ref_dir=REF_DIR):
    """True when both reference libraries have been built."""
    return all(os.path.exists(os.path.join(ref_dir, f)) for f in LIBS.values())


def load_library(path):
    """dlopen one reference library and bind the C entry points of ref_shim/entry.hip."""
    lib = ctypes.CDLL(path)
    for name, args in _ARGTYPES.items():
        fn = getattr(lib, name)   # AttributeError: the library does not export the entry
        fn.argtypes, fn.restype = args, None
    return lib


def _chk(t, dtype, name, ndim):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be a {'float' if dtype == torch.float32 else 'int'} tensor")
    if t.dim() != ndim:
        raise RuntimeError(f"{name} must have {ndim} dimensions")


def _chk_range(t, hi, name):
    """Raise unless every element of the int tensor lies in [0, hi): the reference kernels would read or write outside
    their tensors otherwise."""
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= hi):
        raise RuntimeError(f"{name} outside [0, {hi}): refusing to launch an unchecked reference kernel")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class _RefBackend:
    """One reference library behind the reference pybind module's forward names."""

    def __init__(self, kind):
        self.kind = kind
        self._lib = None

    def _call(self, name, dev, *args):
        if self._lib is None:
            self._lib = load_library(os.path.join(REF_DIR, LIBS[self.kind]))
        with torch.cuda.device(dev):
            torch.cuda.synchronize()
            self._lib.ref_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            getattr(self._lib, name)(*args)
            torch.cuda.synchronize()

    def ball_query(self, centers_coords, points_coords, radius, num_neighbors):
        _chk(centers_coords, torch.float32, "centers_coords", 3)
        _chk(points_coords, torch.float32, "points_coords", 3)
        b, _, m = centers_coords.shape
        n = points_coords.shape[2]
        if points_coords.shape[:2] != (b, 3) or centers_coords.shape[1] != 3 or num_neighbors < 1:
            raise RuntimeError("ball_query: expects [b,3,m] centres, [b,3,n] points, num_neighbors >= 1")
        out = torch.zeros((b, m, num_neighbors), dtype=torch.int32, device=points_coords.device)
        r = np.float32(radius)  # `const float radius`; radius * radius in f32 (ball_query.cpp:24)
        self._call("ref_ball_query", out.device, b, n, m, float(np.float32(r * r)), num_neighbors,
                   _p(centers_coords), _p(points_coords), _p(out))
        return out

    def grouping_forward(self, features, indices):
        _chk(features, torch.float32, "features", 3)
        _chk(indices, torch.int32, "indices", 3)
        b, c, n = features.shape
        _, m, u = indices.shape
        if indices.shape[0] != b:
            raise RuntimeError("grouping_forward: batch sizes differ")
        _chk_range(indices, n, "indices")
        out = torch.zeros((b, c, m, u), dtype=torch.float32, device=features.device)
        self._call("ref_grouping", out.device, b, c, n, m, u, _p(features), _p(indices), _p(out))
        return out

    def gather_features_forward(self, features, indices):
        _chk(features, torch.float32, "features", 3)
        _chk(indices, torch.int32, "indices", 2)
        b, c, n = features.shape
        m = indices.shape[1]
        if indices.shape[0] != b:
            raise RuntimeError("gather_features_forward: batch sizes differ")
        _chk_range(indices, n, "indices")
        out = torch.zeros((b, c, m), dtype=torch.float32, device=features.device)
        self._call("ref_gather_features", out.device, b, c, n, m, _p(features), _p(indices), _p(out))
        return out

    def furthest_point_sampling(self, coords, num_samples):
        _chk(coords, torch.float32, "coords", 3)
        b, three, n = coords.shape
        if three != 3 or n < 1:
            raise RuntimeError("furthest_point_sampling: expects [b,3,n] coords, n >= 1")
        out = torch.zeros((b, num_samples), dtype=torch.int32, device=coords.device)
        dist = torch.full((b, n), 1e38, dtype=torch.float32, device=coords.device)
        self._call("ref_furthest_point_sampling", out.device, b, n, num_samples, _p(coords), _p(dist), _p(out))
        return out

    def three_nearest_neighbors_interpolate_forward(self, points_coords, centers_coords, centers_features):
        _chk(points_coords, torch.float32, "points_coords", 3)
        _chk(centers_coords, torch.float32, "centers_coords", 3)
        _chk(centers_features, torch.float32, "centers_features", 3)
        b, c, m = centers_features.shape
        n = points_coords.shape[2]
        if points_coords.shape[:2] != (b, 3) or tuple(centers_coords.shape) != (b, 3, m) or m < 1:
            raise RuntimeError("three_nn: expects [b,3,n] points, [b,3,m] centres, [b,c,m] features, m >= 1")
        dev = points_coords.device
        idx = torch.zeros((b, 3, n), dtype=torch.int32, device=dev)
        wgt = torch.zeros((b, 3, n), dtype=torch.float32, device=dev)
        out = torch.zeros((b, c, n), dtype=torch.float32, device=dev)
        self._call("ref_three_nearest_neighbors_interpolate", dev, b, c, m, n, _p(points_coords), _p(centers_coords),
                   _p(centers_features), _p(idx), _p(wgt), _p(out))
        return [out, idx, wgt]

    def avg_voxelize_forward(self, features, coords, resolution):
        _chk(features, torch.float32, "features", 3)
        _chk(coords, torch.int32, "coords", 3)
        b, c, n = features.shape
        if tuple(coords.shape) != (b, 3, n) or resolution < 1:
            raise RuntimeError("avg_voxelize_forward: expects [b,c,n] features, [b,3,n] coords, resolution >= 1")
        _chk_range(coords, resolution, "voxel coordinates")
        r3 = resolution ** 3
        dev = features.device
        ind = torch.zeros((b, n), dtype=torch.int32, device=dev)
        out = torch.zeros((b, c, r3), dtype=torch.float32, device=dev)
        cnt = torch.zeros((b, r3), dtype=torch.int32, device=dev)
        self._call("ref_avg_voxelize", dev, b, c, n, resolution, _p(coords), _p(features), _p(ind), _p(cnt), _p(out))
        return [out, ind, cnt]

    def trilinear_devoxelize_forward(self, r, is_training, coords, features):
        _chk(features, torch.float32, "features", 3)
        _chk(coords, torch.float32, "coords", 3)
        b, c, s = features.shape
        n = coords.shape[2]
        if coords.shape[:2] != (b, 3) or s != r ** 3:
            raise RuntimeError("trilinear_devoxelize_forward: expects [b,3,n] coords and [b,c,r^3] features")
        # every corner the kernel reads lies in the grid iff 0 <= coordinate <= r - 1 (trilinear_devox.cu:41-75: the high
        # corner is taken only where the fractional part is positive)
        if n and not bool(((coords >= 0) & (coords <= r - 1)).all()):
            raise RuntimeError(f"coords outside [0, {r - 1}]: refusing to launch an unchecked reference kernel")
        dev = features.device
        outs = torch.zeros((b, c, n), dtype=torch.float32, device=dev)
        shape = (b, 8, n) if is_training else (1,)
        inds = torch.zeros(shape, dtype=torch.int32, device=dev)
        wgts = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._call("ref_trilinear_devoxelize", dev, b, c, n, r, 1 if is_training else 0, _p(coords), _p(features),
                   _p(inds), _p(wgts), _p(outs))
        return [outs, inds, wgts]


default = _RefBackend("default")
strict = _RefBackend("strict")
__all__ = ["available", "default", "strict", "load_library", "REF_DIR", "LIBS"]
