"""ctypes binding of libgldm_hip.so (C ABI: include/gldm.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If
the shared object is missing or a kernel launch fails, callers get an exception.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# GLDM_LIB: another build of the same library (diagnostic builds: make -C graspldm_amd/csrc EXTRA=... OUT=...)
LIB_PATH = os.environ.get("GLDM_LIB") or os.path.join(_PKG, "libgldm_hip.so")

ABI_VERSION = 15


class GldmError(RuntimeError):
    pass


_lib = None

_ll = ctypes.c_longlong
_ull = ctypes.c_ulonglong
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float

_SIGNATURES = {
    # name: argtypes  (all return int, but the *_workspace_bytes / *_lds_bytes entries: long long)
    "gldm_ball_query": [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp],
    "gldm_grouping_forward": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "gldm_gather_features_forward": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_furthest_point_sampling": [_vp, _i, _i, _i, _vp, _vp],
    "gldm_three_nn_interpolate_forward": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_avg_voxelize_forward": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_trilinear_devoxelize_forward": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_voxel_coords": [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp],
    "gldm_farthest_points_euclid": [_vp, _i, _i, _i, _vp, _vp],
    "gldm_normalize_cloud": [_vp, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp],
    "gldm_gather_points": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_sa_group": [_vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp],
    "gldm_r1d_cond_embed": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_denoise": [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "gldm_denoise_rng": [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _ull, _ll, _vp, _vp, _vp, _vp],
    "gldm_step_noise_rng": [_ull, _ll, _i, _i, _i, _vp, _vp],
    "gldm_decode": [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "gldm_pose_epilogue": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_encode": [_vp, _vp, _vp, _i, _vp, _i, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _vp],
    "gldm_pose_prologue": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_conv3d_k3": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "gldm_conv3d_k3_cl": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "gldm_conv3d_k3_generic": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "gldm_conv3d_k3_f16x2": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "gldm_conv3d_k3_f16x2_gn": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "gldm_groupnorm_coef": [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp],
    "gldm_gn_swish_chan_sum": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_gn_swish_chan_sum_cl": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_se_gate_parts": [_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "gldm_groupnorm_swish": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp],
    "gldm_se_gate": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "gldm_bias_act": [_vp, _vp, _i, _i, ctypes.c_longlong, _i, _vp],
    "gldm_devoxelize_fused": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_devoxelize_gn_fused": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_devoxelize_gn_cl_fused": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_pointwise_mlp": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "gldm_pointwise_mlp2": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "gldm_pointwise_small": [_vp, _vp, _vp, _i, _i, _i, ctypes.c_longlong, _i, _vp, _vp],
    "gldm_pointwise_any": [_vp, _vp, _vp, _i, _i, _i, ctypes.c_longlong, _i, _vp, _vp],
    "gldm_linear_rows": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_pointwise_mlp_f16x2": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "gldm_row_max": [_vp, _ll, _i, _vp, _vp],
    "gldm_pointwise_mlp_f16x2_pm": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "gldm_pointwise_mlp_f16x2_add": [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _i, _i, _i, _i, _i, _vp, _vp],
    "gldm_pointwise_mlp2_f16x2": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "gldm_point_attention": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _ll, _vp, _vp],
    "gldm_point_attention_workspace_bytes": [_i, _i, _i],   # returns long long
    "gldm_groupnorm_swish_points": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp],
    "gldm_pointwise_rows": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_point_attention_fused": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "gldm_groupnorm_affine": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "gldm_groupnorm_swish_points_sum": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp],
    "gldm_grasp_scene": [_vp, _vp, _vp, _vp, _f, _f, _i, _i, _i, _i, _vp, _vp],
    "gldm_cls_head_workspace_bytes": [_i, _i, _i, _i],   # returns long long
    "gldm_cls_head": [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _vp, _ll, _vp, _vp, _vp],
    "gldm_sa_mlp_forward": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "gldm_sa_mlp_forward_f16x2": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gldm_sa_mlp_forward_f16x2_pre": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # the shape queries of the three MFMA families of the encoders (ABI 15): the launchers' own planners
    "gldm_pointwise_mlp_supported": [_i, _i, _i, _i, _i, _i, _i, _i],
    "gldm_conv3d_k3_supported": [_i, _i, _i, _i],
    "gldm_sa_mlp_supported": [_i, _i, _i, _vp, _vp],
    "gldm_sa_mlp_f16x2_lds_bytes": [_i, _i, _i, _i, _vp, _vp, ctypes.POINTER(_ll)],   # returns long long
    "gldm_ball_query_multi": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_group_max_concat": [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp],
    "gldm_unet1d_supported": [_vp, _i],
    "gldm_grasp_clearance_chunk": [],
    "gldm_grasp_clearance": [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _i, _f, _f, _vp, _vp, _vp],
    "gldm_grasp_contact_normals": [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _f, _f, _vp, _vp, _vp],
    "gldm_knn_radius_workspace_bytes": [_i, _i],   # returns long long
    "gldm_knn_radius": [_vp, _i, _i, _i, _f, _vp, _ll, _vp, _vp, _vp, _vp],
    "gldm_point_normals": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp],
    "gldm_select_grasps": [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "gldm_farthest_points_euclid_large_workspace_bytes": [_i, _i],   # returns long long
    "gldm_farthest_points_euclid_large_slice": [_i],
    "gldm_farthest_points_euclid_large": [_vp, _vp, _i, _i, _i, _vp, _ll, _vp, _vp],
    "gldm_depth_to_cloud_workspace_bytes": [_i, _i, _i],   # returns long long
    "gldm_depth_to_cloud_tile_pixels": [],
    "gldm_depth_to_cloud": [_vp, _i, _f, _vp, _i, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp],
    "gldm_unet1d": [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "gldm_depth_to_objects_workspace_bytes": [_i, _i, _i, _i],   # returns long long
    "gldm_depth_to_objects": [_vp, _i, _f, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _ll, _vp, _vp,
                              _vp, _vp, _vp],
    "gldm_farthest_points_euclid_ragged_workspace_bytes": [_i, _i],   # returns long long
    "gldm_farthest_points_euclid_ragged": [_vp, _vp, _vp, _i, _i, _i, _vp, _ll, _vp, _vp],
    "gldm_plane_ransac_workspace_bytes": [_i, _i],   # returns long long
    "gldm_plane_ransac_tile_points": [],
    "gldm_plane_ransac": [_vp, _i, _vp, _i, _f, _f, _vp, _ll, _vp, _vp, _vp],
    "gldm_plane_moments_workspace_bytes": [_i],   # returns long long
    "gldm_plane_moments": [_vp, _i, _vp, _f, _vp, _ll, _vp, _vp],
    "gldm_segment_tabletop_workspace_bytes": [_i, _i],   # returns long long
    "gldm_segment_tile_shape": [ctypes.POINTER(_i), ctypes.POINTER(_i)],
    "gldm_segment_tabletop": [_vp, _i, _f, _vp, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _i, _vp,
                              _ll, _vp, _vp, _vp, _vp, _vp],
}


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libgldm_hip.so (hipcc cross-compiles
    without a GPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise GldmError("building libgldm_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """The loaded library; raises GldmError loudly when it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GldmError(
            f"{LIB_PATH} is missing: the gfx950 HIP library is required (no fallback path). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C graspldm_amd/csrc`.")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7, and whichever copy is mapped first
    # serves both.  Loaded in front of torch, this library would bring /opt/rocm's copy in, and launches then fail once torch
    # initialises the device on it (seen as GLDM_ERR_LAUNCH from the first kernel of `python __graft_entry__.py smoke`).
    # The package plumbs torch tensors and streams anyway: import it first.
    import torch  # noqa: F401
    try:
        h = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise GldmError(f"cannot load {LIB_PATH}: {e}") from e
    h.gldm_abi_version.restype = _i
    h.gldm_abi_version.argtypes = []
    h.gldm_status_string.restype = ctypes.c_char_p
    h.gldm_status_string.argtypes = [_i]
    if h.gldm_abi_version() != ABI_VERSION:
        raise GldmError(f"libgldm_hip.so ABI {h.gldm_abi_version()} != expected {ABI_VERSION}; rebuild it")
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(h, name)
        fn.argtypes = argtypes
        fn.restype = _ll if name.endswith(("_workspace_bytes", "_lds_bytes")) else _i
    h.gldm_r1d_workspace_bytes.argtypes = [_vp, _i]
    h.gldm_r1d_workspace_bytes.restype = ctypes.c_longlong
    h.gldm_r1d_tile_columns.argtypes = [_vp]
    h.gldm_r1d_tile_columns.restype = _i
    h.gldm_conv3d_partial_floats.argtypes = [_i, _i, _i]
    h.gldm_conv3d_partial_floats.restype = ctypes.c_longlong
    h.gldm_squeeze_parts.argtypes = []
    h.gldm_squeeze_parts.restype = _i
    _lib = h
    return h


def call(name, *args):
    h = lib()
    status = getattr(h, name)(*args)
    if status != 0:
        raise GldmError(f"{name} failed: {h.gldm_status_string(status).decode()} (status {status})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def workspace(name, sizes, dtype, device, envelope):
    """The workspace of entry `name` for the shape `sizes` (the arguments of `name`_workspace_bytes): (an uninitialised
    tensor of `dtype` covering the bytes, the bytes); (None, 0) where the entry needs none.  A shape outside the entry's
    envelope raises GldmError with the status string and `envelope`, the caller's words for shape and limits."""
    import torch
    h = lib()
    nbytes = getattr(h, name + "_workspace_bytes")(*sizes)
    if nbytes < 0:
        raise GldmError(f"{name}: {h.gldm_status_string(int(nbytes)).decode()} ({envelope})")
    if nbytes == 0:
        return None, 0
    item = torch.empty((), dtype=dtype).element_size()
    return torch.empty((nbytes + item - 1) // item, dtype=dtype, device=device), nbytes


def current_stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
