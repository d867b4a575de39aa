"""Raw-cloud front end on the GPU: what a sensor cloud goes through before
`generate_grasps` -- point-count regularisation and dataset-statistics normalisation.

Mirrors `PointCloudHelpers` (grasp_ldm/utils/pointcloud_helpers.py: regularize_pointcloud :40-71,
regularize_pc_point_count :124-158, farthest_points :160-217) and `normalize_input`
(tools/inference.py:570-591).  The point arithmetic (greedy farthest-point selection, row gathers,
centring/scaling) runs in libgldm_hip.so; the RANDOM index draws stay on the host and use exactly
the generator calls the reference makes (np.random.choice / torch.randperm), so a seeded run picks
the same points.  CPU tensors are rejected like everywhere else in this package.

In front of that, from a depth camera: `depth_to_cloud` deprojects depth frames on the GPU
(gldm_depth_to_cloud; Camera.depth_to_pointcloud_torch, grasp_ldm/utils/camera.py:176-215), `read_depth_file` reads them
from disk, and clouds of more than 8192 points take gldm_farthest_points_euclid_large.  With an instance-label image
 `depth_to_objects` cuts the frame into every object's cloud in one pass (gldm_depth_to_objects) and
`regularize_objects` brings clouds of different sizes to one point count with one ragged selection
(gldm_farthest_points_euclid_ragged) and one gather.  Without a label image `fit_table_plane` finds the
table (gldm_plane_ransac, gldm_plane_moments) and `segment_tabletop` labels the objects standing on it
(gldm_segment_tabletop).  `estimate_normals` gives a sensor cloud its surface normals (gldm_knn_radius,
gldm_point_normals; estimate_normals_cam_from_pc, pointcloud_helpers.py:74-122).  `remove_outliers` drops
the isolated points of sensor clouds before any of that sees them (gldm_neighbor_stats, gldm_filter_outliers), and
`voxel_downsample` brings raw sensor density down to one point per voxel in front of both
(gldm_voxel_downsample).  From an object model instead of a sensor: `sample_mesh_surface` draws the full cloud
the reference takes from trimesh (gldm_mesh_sample_surface) and `render_depth` the depth frames it takes from pyrender
(gldm_render_depth), with ground-truth labels and face indices.
"""
import ctypes
import math
import typing

import numpy as np
import torch

from . import _lib as L

PC_SHIFT, PC_SCALE, MRP_SCALE = 0.0, 0.05, 0.5


def _need_cuda(t, name="pc"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (graspldm_amd has no CPU path)")


def _as_batch(pc):
    _need_cuda(pc)
    if pc.ndim not in (2, 3) or pc.shape[-1] != 3:
        raise ValueError(f"Expected point cloud to have shape (N, 3) or (B, N, 3), got {tuple(pc.shape)}.")
    return (pc.unsqueeze(0) if pc.ndim == 2 else pc).contiguous().float()


def gather_points(pc, idx):
    """pc [B,N,3], idx int [B,M] -> [B,M,3]."""
    pcb = _as_batch(pc)
    idx = idx.to(device=pcb.device, dtype=torch.int32).reshape(pcb.shape[0], -1).contiguous()
    b, n, _ = pcb.shape
    m = idx.shape[1]
    out = torch.empty((b, m, 3), dtype=torch.float32, device=pcb.device)
    if m:
        with torch.cuda.device(pcb.device):
            L.call("gldm_gather_points", L.ptr(pcb), L.ptr(idx), b, n, m, L.ptr(out), L.current_stream(pcb.device))
    return out


FPS_SMALL_MAX = 8192   # gldm_farthest_points_euclid's ceiling; larger clouds take gldm_farthest_points_euclid_large


def farthest_point_indices(pc, nclusters):
    """Centre indices of PointCloudHelpers.farthest_points(pc, nclusters, distance_by_translation_point,
    return_center_indexes=True) (pointcloud_helpers.py:160-223) for every cloud of pc [B,N,3] / [N,3]:
    int32 [B, min(nclusters, N)]; `nclusters >= N` returns arange(N) like the reference (:185-191)."""
    pcb = _as_batch(pc)
    b, n, _ = pcb.shape
    if nclusters >= n:
        return torch.arange(n, dtype=torch.int32, device=pcb.device).unsqueeze(0).repeat(b, 1)
    idx = torch.empty((b, int(nclusters)), dtype=torch.int32, device=pcb.device)
    if n > FPS_SMALL_MAX:
        return farthest_point_indices_large(pcb, int(nclusters), out=idx)
    with torch.cuda.device(pcb.device):
        L.call("gldm_farthest_points_euclid", L.ptr(pcb), b, n, int(nclusters), L.ptr(idx), L.current_stream(pcb.device))
    return idx


def farthest_point_indices_large(pc, nclusters, counts=None, out=None):
    """gldm_farthest_points_euclid_large on pc [B,N,3] with 8192 < N <= 2^22: the same indices as
    farthest_point_indices, one launch per round over many workgroups.  counts (int32 [B] on the device, optional): the
    live rows of each cloud -- rows past them are never read, and a cloud with counts[b] <= nclusters gets
    0 .. counts[b]-1 followed by -1.  -> int32 [B, nclusters]."""
    pcb = _as_batch(pc)
    b, n, _ = pcb.shape
    m = int(nclusters)
    ws, nbytes = L.workspace("gldm_farthest_points_euclid_large", (b, n), torch.int64, pcb.device,
                             f"b = {b}, n = {n}; 8192 < n <= 2^22")
    if counts is not None:
        _need_cuda(counts, "counts")
        counts = counts.to(device=pcb.device, dtype=torch.int32).reshape(b).contiguous()
    idx = torch.empty((b, m), dtype=torch.int32, device=pcb.device) if out is None else out
    with torch.cuda.device(pcb.device):
        L.call("gldm_farthest_points_euclid_large", L.ptr(pcb), L.ptr(counts), b, n, m, L.ptr(ws), nbytes, L.ptr(idx),
               L.current_stream(pcb.device))
    return idx


def _drawn_rows(n, num_points, use_farthest_point, rng):
    """The rows (int64 [num_points]) that bring one cloud of n rows to num_points, drawn on the host with the generator
    calls of pointcloud_helpers.py:124-158 (`rng`: a np.random.RandomState / Generator-like object with `.choice`; None =
    the global np.random the reference draws from): n > num_points: num_points of them without replacement; n <
    num_points: all of them, then num_points - n drawn with replacement.  None where n > num_points and
    use_farthest_point: take the farthest-point selection (no draw)."""
    rng = np.random if rng is None else rng
    if n > num_points:
        if use_farthest_point:
            return None
        return torch.from_numpy(np.asarray(rng.choice(range(n), size=num_points, replace=False))).long()
    if n < num_points:
        extra = torch.from_numpy(np.asarray(rng.choice(range(n), size=num_points - n)))
        return torch.cat([torch.arange(n), extra.long()])
    return torch.arange(n)


class PointCloudHelpers:
    """The point-count helpers of the reference class of the same name, on CUDA tensors."""

    @staticmethod
    def farthest_points(data, nclusters, dist_func=None, return_center_indexes=True, **_):
        if dist_func is not None and getattr(dist_func, "__name__", "") != "distance_by_translation_point":
            raise NotImplementedError("only the Euclidean point distance (distance_by_translation_point) is built")
        if not return_center_indexes:
            raise NotImplementedError("cluster labels are not on the generation path; ask for the centre indexes")
        idx = farthest_point_indices(data, nclusters)
        return idx[0] if data.ndim == 2 else idx

    @staticmethod
    def regularize_pc_point_count(pc, npoints, use_farthest_point=False, rng=None):
        """pointcloud_helpers.py:124-158 on one cloud [N,3] -> [npoints,3].  `rng`: a np.random.RandomState /
        Generator-like object with `.choice`; default = the global np.random the reference draws from."""
        _need_cuda(pc)
        assert pc.ndim == 2
        if pc.shape[0] == npoints:
            return pc.contiguous().float()
        idx = _drawn_rows(pc.shape[0], npoints, use_farthest_point, rng)
        idx = farthest_point_indices(pc, npoints) if idx is None else idx.unsqueeze(0)
        return gather_points(pc, idx)[0]

    @staticmethod
    def regularize_pointcloud(pc, num_points):
        """pointcloud_helpers.py:40-71 on one cloud [N,3] -> [1,num_points,3]; draws torch.randperm on the
        CPU generator exactly where the reference does."""
        _need_cuda(pc)
        assert pc.ndim == 2
        n = pc.shape[0]
        if n < num_points:
            mult = max(num_points // n, 1)
            base = torch.arange(n).repeat(mult)              # pc.repeat(multiplier, 1)
            extra = num_points - base.shape[0]
            idx = torch.cat([base, base[torch.randperm(base.shape[0])[:extra]]])
        elif n > num_points:
            idx = torch.randperm(n)[:num_points]
        else:
            return pc.contiguous().float().unsqueeze(0)
        return gather_points(pc, idx.unsqueeze(0))

    @staticmethod
    def estimate_normals_cam_from_pc(pc_cam, max_radius=0.05, k=12):
        """pointcloud_helpers.py:74-97 on one cloud [N,3] in camera coordinates -> [N,3] normals towards the camera
        (estimate_normals below; the zero vector where fewer than 3 neighbours lie within max_radius)."""
        _need_cuda(pc_cam, "pc_cam")
        if pc_cam.ndim != 2:
            raise ValueError(f"pc_cam must be [N, 3], not {tuple(pc_cam.shape)}")
        return estimate_normals(pc_cam, max_radius=max_radius, k=k)[0]

    @staticmethod
    def vectorized_normal_computation(pc, neighbors):
        """pointcloud_helpers.py:99-122: pc [N,3], neighbors [N,k,3] -> [N,3] (the `neighbors` form of gldm_point_normals)."""
        pcb = _as_batch(pc)
        _need_cuda(neighbors, "neighbors")
        nb = neighbors.to(pcb.device).float().contiguous()
        if pc.ndim != 2 or nb.ndim != 3 or nb.shape[0] != pcb.shape[1] or nb.shape[2] != 3:
            raise ValueError(f"pc must be [N, 3] and neighbors [N, k, 3], not {tuple(pc.shape)} and {tuple(neighbors.shape)}")
        k = nb.shape[1]
        _check_knn_envelope(pcb.shape[1], k)
        _finite_cloud(pcb)
        _finite_cloud(nb)
        return _point_normals(pcb, None, nb, k, None)[0]


def _vec(v, n, device):
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    return (t.expand(n) if t.numel() == 1 else t).to(device).contiguous()


def normalize_input(pc, pc_shift=PC_SHIFT, pc_scale=PC_SCALE, mrp_scale=MRP_SCALE, grasp_shift=None):
    """Centre every cloud on its mean, normalise with the dataset statistics, build the metas that
    `unnormalize_grasps` / `unnormalize_pc` need -- `normalize_input` of grasp_ldm/inference/inference_base.py:
    181-212 (statistics from set_normalization_params :103-130) and of tools/inference.py:570-591 (which reads
    class constants PC_MEAN / PC_STD / GRASP_MEAN / GRASP_STD that that file never defines; the values are the
    dataset's: shift 0, translation scale 0.05, rotation scale 0.5, acronym_pointclouds.py:15-16).  One launch.
    pc [N,3] or [B,N,3] (not modified; the reference subtracts in place) -> (pc_norm of the same rank, metas)
    with grasp_mean [B,6] and grasp_std [1,6] as in tools/inference.py:581-588.  A single [N,3] cloud counts as
    B = 1 (the reference repeats grasp_mean N times there, :581, which its unnormalize_grasps then broadcasts
    into N copies of every grasp)."""
    _need_cuda(pc)
    assert pc.ndim in (2, 3)
    pcb = _as_batch(pc)
    b, n, _ = pcb.shape
    dev = pcb.device
    sh, sc = _vec(pc_shift, 3, "cpu"), _vec(pc_scale, 3, "cpu")
    out = torch.empty_like(pcb)
    mean = torch.empty((b, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_normalize_cloud", L.ptr(pcb), b, n, float(sh[0]), float(sh[1]), float(sh[2]), float(sc[0]),
               float(sc[1]), float(sc[2]), L.ptr(out), L.ptr(mean), L.current_stream(dev))
    gm = (torch.zeros(6) if grasp_shift is None else _vec(grasp_shift, 6, "cpu")).to(dev).unsqueeze(0).repeat(b, 1)
    gm[:, :3] += mean
    gstd = torch.cat([sc, _vec(mrp_scale, 3, "cpu")]).to(dev).unsqueeze(0)
    pc_mean = sh.to(dev) + mean
    metas = dict(pc_mean=pc_mean if pc.ndim == 3 else pc_mean[0], pc_std=sc.to(dev).unsqueeze(0),
                 grasp_mean=gm, grasp_std=gstd, dataset_normalized=True, use_dataset_statistics=False)
    return (out if pc.ndim == 3 else out[0]), metas


FLT_MAX = 3.4028234663852886e38


def depth_tile_pixels():
    """Pixels per tile (= per workgroup) of gldm_depth_to_cloud."""
    return int(L.lib().gldm_depth_to_cloud_tile_pixels())


def _host_floats(v, n, name):
    a = np.ascontiguousarray(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(-1))
    if a.size != n:
        raise ValueError(f"{name} must hold {n} numbers, not {a.size}")
    return a


def depth_to_cloud(depth, camera, mask=None, z_range=None, depth_scale=None, cam_to_world=None, crop_box=None,
                   return_pixels=False):
    """Depth frame(s) -> cloud(s), one HIP entry (gldm_depth_to_cloud): the deprojection of
    Camera.depth_to_pointcloud_torch (grasp_ldm/utils/camera.py:176-215) with a mask, a depth window, a rigid transform
    and a crop box folded in.
      depth         CUDA [H, W] or [F, H, W]: float32 metres, or raw sensor units as torch.uint16 (or int16 holding the
                    same bits) together with depth_scale (metres per unit, e.g. 0.001)
      camera        graspldm_amd.camera.Camera (fx, fy, cx, cy; its width / height must match)
      mask          CUDA bool / uint8 of depth's shape, nonzero = keep
      z_range       (z_min, z_max): kept iff z_min < d <= z_max; default (0, FLT_MAX): NaN, inf, zero and negative
                    depth are dropped
      cam_to_world  3 x 4 or 4 x 4 (host or device; read on the host): points come out as R p + t
      crop_box      ((x0, y0, z0), (x1, y1, z1)) in the output frame, faces included
    Kept pixels come in ascending pixel index v * W + u (the order of torch.where(depth > 0)).
    -> [n, 3] for an [H, W] input, a list of F clouds [n_f, 3] for [F, H, W] (views of one buffer, cut after ONE
    read-back of the counts); with return_pixels also the int32 source pixel indices in the same form."""
    fr = _depth_frames(depth, camera, mask, z_range, depth_scale, cam_to_world, crop_box)
    f, h, w, dev, single = fr.f, fr.h, fr.w, fr.device, fr.single
    ws, nbytes = L.workspace("gldm_depth_to_cloud", (f, h, w), torch.int32, dev, f"frames {f}, {h} x {w}; 1 <= H*W <= 2^24")
    points = torch.empty((f, h * w, 3), dtype=torch.float32, device=dev)
    count = torch.empty(f, dtype=torch.int32, device=dev)
    pixel = torch.empty((f, h * w), dtype=torch.int32, device=dev) if return_pixels else None
    with torch.cuda.device(dev):
        L.call("gldm_depth_to_cloud", *fr.source, f, h, w, *fr.optics, L.ptr(ws), nbytes, L.ptr(points), L.ptr(count),
               L.ptr(pixel), L.current_stream(dev))
    counts = count.tolist()   # the one read-back
    clouds = [points[i, :c] for i, c in enumerate(counts)]
    if not return_pixels:
        return clouds[0] if single else clouds
    pixels = [pixel[i, :c] for i, c in enumerate(counts)]
    return (clouds[0], pixels[0]) if single else (clouds, pixels)


MAX_LABELS = 64   # gldm_depth_to_objects' ceiling on num_labels


def depth_to_objects(depth, camera, labels, num_labels=None, mask=None, z_range=None, depth_scale=None, cam_to_world=None,
                     crop_box=None, return_pixels=False):
    """Depth frame(s) + instance labels -> every object's cloud, one HIP entry (gldm_depth_to_objects).
    Arguments as depth_to_cloud, plus
      labels      CUDA integer tensor of depth's shape: pixel of object k = label k (1 .. num_labels); labels <= 0 or
                  > num_labels are background
      num_labels  K (1 .. 64); default int(labels.max()) (one more read-back), at least 1
    The cloud of object k is bit-identical to depth_to_cloud(depth, camera, mask=(labels == k) & mask, ...).
    -> a list of K clouds [count_k, 3] (empty ones included) for an [H, W] input, a list of F such lists for [F, H, W]:
    views of one buffer, cut after ONE read-back of start / count; with return_pixels also the int32 source pixel indices
    in the same form."""
    points, pixel, starts, counts = _depth_to_objects_packed(depth, camera, labels, num_labels, mask, z_range, depth_scale,
                                                             cam_to_world, crop_box, return_pixels)
    single = depth.ndim == 2
    clouds = [[points[i, s:s + c] for s, c in zip(st, ct)] for i, (st, ct) in enumerate(zip(starts, counts))]
    if not return_pixels:
        return clouds[0] if single else clouds
    pixels = [[pixel[i, s:s + c] for s, c in zip(st, ct)] for i, (st, ct) in enumerate(zip(starts, counts))]
    return (clouds[0], pixels[0]) if single else (clouds, pixels)


def _depth_to_objects_packed(depth, camera, labels, num_labels=None, mask=None, z_range=None, depth_scale=None,
                             cam_to_world=None, crop_box=None, return_pixels=False):
    """depth_to_objects before the cut: (points [F, H*W, 3], pixel [F, H*W] or None, start, count); start / count are host
    lists [F][K] from the one read-back, start relative to the frame's row 0."""
    _need_cuda(depth, "depth")
    _need_cuda(labels, "labels")
    if tuple(labels.shape) != tuple(depth.shape):
        raise ValueError(f"labels {tuple(labels.shape)} do not match depth {tuple(depth.shape)}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must be an integer tensor, not {labels.dtype}")
    fr = _depth_frames(depth, camera, mask, z_range, depth_scale, cam_to_world, crop_box)
    f, h, w, dev = fr.f, fr.h, fr.w, fr.device
    lab = labels.reshape(f, h, w).to(device=dev, dtype=torch.int32).contiguous()
    k = max(int(lab.max()), 1) if num_labels is None else int(num_labels)
    if k > MAX_LABELS:
        raise NotImplementedError(f"num_labels = {k}: gldm_depth_to_objects takes at most {MAX_LABELS} labels per call")
    if k < 1:
        raise ValueError(f"num_labels must be at least 1, not {k}")
    ws, nbytes = L.workspace("gldm_depth_to_objects", (f, h, w, k), torch.int32, dev,
                             f"frames {f}, {h} x {w}, {k} labels; 1 <= H*W <= 2^24")
    points = torch.empty((f, h * w, 3), dtype=torch.float32, device=dev)
    sc = torch.empty((2, f, k), dtype=torch.int32, device=dev)   # start, count: one buffer, one read-back
    pixel = torch.empty((f, h * w), dtype=torch.int32, device=dev) if return_pixels else None
    with torch.cuda.device(dev):
        L.call("gldm_depth_to_objects", *fr.source, L.ptr(lab), k, f, h, w, *fr.optics, L.ptr(ws), nbytes, L.ptr(points),
               L.ptr(sc[0]), L.ptr(sc[1]), L.ptr(pixel), L.current_stream(dev))
    starts, counts = sc.tolist()   # the one read-back
    return points, pixel, starts, counts


def _host_ptr(a):
    """Pointer to a host numpy array (None -> NULL); the array must outlive the call it is passed to."""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class _DepthFrames(typing.NamedTuple):
    """What the depth entries (gldm_depth_to_cloud, gldm_depth_to_objects, gldm_segment_tabletop) share."""
    frames: torch.Tensor   # [F, H, W], contiguous
    single: bool           # the caller gave one frame [H, W]
    f: int
    h: int
    w: int
    device: torch.device
    source: tuple          # the entries' leading arguments, in gldm.h's order: depth, is_u16, depth_scale, mask
    optics: tuple          # those behind the shape: fx, fy, cx, cy, z_min, z_max, cam_to_world, crop_lo, crop_hi
    alive: tuple           # the mask and the host arrays behind the pointers above: they live as long as the record


def _depth_frames(depth, camera, mask, z_range, depth_scale, cam_to_world, crop_box):
    """The checks and conversions in front of every depth entry: depth [H, W] or [F, H, W] against the camera model, the
    optional arguments through _depth_options -> _DepthFrames."""
    _need_cuda(depth, "depth")
    if depth.ndim not in (2, 3):
        raise ValueError(f"depth must be [H, W] or [F, H, W], not {tuple(depth.shape)}")
    single = depth.ndim == 2
    d = (depth.unsqueeze(0) if single else depth).contiguous()
    f, h, w = d.shape
    if (h, w) != (camera.height, camera.width):
        raise ValueError(f"depth frames are {h} x {w}, the camera model is {camera.height} x {camera.width}")
    is_u16, m8, z_min, z_max, xf, lo, hi = _depth_options(d, depth, mask, z_range, depth_scale, cam_to_world, crop_box)
    fx, fy, cx, cy = camera.intrinsics
    return _DepthFrames(d, single, f, h, w, d.device, (L.ptr(d), int(is_u16), float(depth_scale or 1.0), L.ptr(m8)),
                        (fx, fy, cx, cy, z_min, z_max, _host_ptr(xf), _host_ptr(lo), _host_ptr(hi)), (m8, xf, lo, hi))


def _depth_options(d, depth, mask, z_range, depth_scale, cam_to_world, crop_box):
    """The checks and host-side conversions depth_to_cloud makes on its optional arguments, for frames d [F,H,W]:
    -> (is_u16, mask u8 or None, z_min, z_max, xf, lo, hi)."""
    f, h, w = d.shape
    raw_types = tuple(t for t in (getattr(torch, "uint16", None), torch.int16) if t is not None)
    is_u16 = d.dtype in raw_types
    if is_u16:
        if depth_scale is None:
            raise ValueError("raw 16-bit depth needs depth_scale (metres per unit)")
    elif d.dtype == torch.float32:
        if depth_scale is not None:
            raise ValueError("depth_scale goes with raw 16-bit depth; float32 depth is in metres")
    else:
        raise ValueError(f"depth must be float32 (metres) or 16-bit raw units, not {d.dtype}")
    m8 = None
    if mask is not None:
        _need_cuda(mask, "mask")
        m8 = (mask.unsqueeze(0) if mask.ndim == 2 else mask)
        if tuple(m8.shape) != (f, h, w):
            raise ValueError(f"mask {tuple(mask.shape)} does not match depth {tuple(depth.shape)}")
        m8 = (m8 if m8.dtype == torch.uint8 else (m8 != 0).to(torch.uint8)).to(d.device).contiguous()
    z_min, z_max = (0.0, FLT_MAX) if z_range is None else (float(z_range[0]), float(z_range[1]))
    xf = lo = hi = None
    if cam_to_world is not None:
        t = np.asarray(cam_to_world.detach().cpu() if isinstance(cam_to_world, torch.Tensor) else cam_to_world, dtype=np.float32)
        if t.shape not in ((3, 4), (4, 4)):
            raise ValueError(f"cam_to_world must be 3 x 4 or 4 x 4, not {t.shape}")
        xf = np.ascontiguousarray(t[:3].reshape(-1))
    if crop_box is not None:
        lo, hi = _host_floats(crop_box[0], 3, "crop_box[0]"), _host_floats(crop_box[1], 3, "crop_box[1]")
    return is_u16, m8, z_min, z_max, xf, lo, hi


def farthest_point_indices_ragged(packed, start, count, n_max, nclusters):
    """gldm_farthest_points_euclid_ragged: farthest-point selection over B clouds of different sizes packed in
    `packed` [rows, 3]; start / count: int32 [B] on the device, n_max: a host upper bound of the counts.  -> int32
    [B, nclusters], relative to each cloud's start: what farthest_point_indices returns for that cloud alone; a cloud with
    count <= nclusters gets 0 .. count-1 followed by -1."""
    _need_cuda(packed, "packed")
    if packed.ndim != 2 or packed.shape[1] != 3:
        raise ValueError(f"packed must be [rows, 3], not {tuple(packed.shape)}")
    pts = packed.contiguous().float()
    dev = pts.device
    start = start.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    count = count.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    b, m, n_max = start.shape[0], int(nclusters), int(n_max)
    if count.shape[0] != b:
        raise ValueError(f"start holds {b} clouds, count {count.shape[0]}")
    ws, nbytes = L.workspace("gldm_farthest_points_euclid_ragged", (b, n_max), torch.int64, dev,
                             f"b = {b}, n_max = {n_max}; 1 <= n_max <= 2^22")
    idx = torch.empty((b, m), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_farthest_points_euclid_ragged", L.ptr(pts), L.ptr(start), L.ptr(count), b, n_max, m, L.ptr(ws), nbytes,
               L.ptr(idx), L.current_stream(dev))
    return idx


def regularize_objects(packed, start, count, num_points, use_farthest_point=True, rng=None):
    """B clouds of different sizes -> [B, num_points, 3]: row i equals
    PointCloudHelpers.regularize_pc_point_count(packed[start[i]:start[i] + count[i]], num_points, use_farthest_point, rng),
    called in ascending i (the order of the draws of rng / np.random).  packed [rows, 3] on the device; start / count:
    host sequences of ints.  Clouds above num_points with use_farthest_point go through ONE ragged selection
    (gldm_farthest_points_euclid_ragged); the others get the host-drawn indices of that function; then one
    gldm_gather_points over the packed rows."""
    _need_cuda(packed, "packed")
    if packed.ndim != 2 or packed.shape[1] != 3:
        raise ValueError(f"packed must be [rows, 3], not {tuple(packed.shape)}")
    start, count = [int(s) for s in start], [int(c) for c in count]
    if len(start) != len(count) or not start:
        raise ValueError(f"start holds {len(start)} clouds, count {len(count)}; at least one is needed")
    num_points = int(num_points)
    for i, (s, c) in enumerate(zip(start, count)):
        if c <= 0:
            raise ValueError(f"cloud {i} is empty")
        if s < 0 or s + c > packed.shape[0]:
            raise ValueError(f"cloud {i}: rows {s} .. {s + c} leave packed [{packed.shape[0]}, 3]")
    pts = packed.contiguous().float()
    dev = pts.device
    b = len(start)
    idx = torch.zeros((b, num_points), dtype=torch.int64)
    far = []
    for i, n in enumerate(count):   # the draws, in the order the per-cloud function makes them
        drawn = _drawn_rows(n, num_points, use_farthest_point, rng)
        if drawn is None:
            far.append(i)
        else:
            idx[i] = drawn
    rows = (idx + torch.tensor(start, dtype=torch.int64).unsqueeze(1)).to(device=dev, dtype=torch.int32)
    if far:
        fs = torch.tensor([start[i] for i in far], dtype=torch.int32, device=dev)
        fc = torch.tensor([count[i] for i in far], dtype=torch.int32, device=dev)
        sel = farthest_point_indices_ragged(pts, fs, fc, max(count[i] for i in far), num_points)
        rows[torch.tensor(far, device=dev)] = sel + fs.unsqueeze(1)
    return gather_points(pts.unsqueeze(0), rows.reshape(1, -1)).reshape(b, num_points, 3)


def read_depth_file(path):
    """A depth image from disk -> numpy [H, W]: float32 (metres) or uint16 (raw units: pass depth_scale on).  `.npy`,
    `.npz` (key depth, else arr_0) and 16-bit `.png` (only where PIL is installed)."""
    ext = path.rsplit(".", 1)[-1].lower() if "." in path else ""
    if ext == "npy":
        a = np.load(path)
    elif ext == "npz":
        with np.load(path) as z:
            key = next((k for k in ("depth", "arr_0") if k in z.files), None)
            if key is None:
                raise ValueError(f"{path}: none of the arrays depth / arr_0 found (has {z.files})")
            a = z[key]
    elif ext == "png":
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f"{path}: reading .png depth needs PIL (Pillow), which is not installed; convert the "
                               "image to .npy / .npz") from e
        a = np.asarray(Image.open(path))
        if a.dtype != np.uint16:
            raise ValueError(f"{path}: expected a 16-bit single-channel depth image, got {a.dtype} {a.shape}")
    else:
        raise ValueError(f"{path}: unknown depth format (.npy .npz .png)")
    a = np.asarray(a)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"{path}: expected an [H, W] depth image, got {a.shape}")
    if a.dtype == np.uint16:
        return np.ascontiguousarray(a)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{path}: depth must be numeric, got {a.dtype}")
    return np.ascontiguousarray(a.astype(np.float32))


def depth_to_tensor(a, device):
    """read_depth_file's array on the device: float32, or the uint16 bits (as int16 where torch has no uint16)."""
    if a.dtype == np.uint16:
        if hasattr(torch, "uint16"):
            return torch.from_numpy(a).to(device)
        return torch.from_numpy(a.view(np.int16)).to(device)
    return torch.from_numpy(a).to(device)


def read_cloud_file(path):
    """A sensor cloud from disk -> float32 numpy [N, 3] (metres, sensor / world frame).  `.npy` ([N,3] or [N,>=3]),
    `.npz` (first of the keys pc / points / xyz / arr_0), `.ply` (ascii or binary_little_endian, vertex x y z) and
    whitespace-separated text (`.xyz`, `.txt`, `.pts`).  The reference's CLI only iterates dataset items
    (tools/generate_grasps.py:109-131); `generate_on_pointcloud` (inference_base.py:161-212) is its entry point for
    such clouds, this is the file front of it."""
    ext = path.rsplit(".", 1)[-1].lower() if "." in path else ""
    if ext == "npy":
        a = np.load(path)
    elif ext == "npz":
        with np.load(path) as z:
            key = next((k for k in ("pc", "points", "xyz", "arr_0") if k in z.files), None)
            if key is None:
                raise ValueError(f"{path}: none of the arrays pc / points / xyz / arr_0 found (has {z.files})")
            a = z[key]
    elif ext == "ply":
        a = _read_ply_vertices(path)
    elif ext in ("xyz", "txt", "pts", "csv"):
        a = np.loadtxt(path, delimiter="," if ext == "csv" else None, ndmin=2)
    else:
        raise ValueError(f"{path}: unknown cloud format (.npy .npz .ply .xyz .txt .pts .csv)")
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] < 3 or a.shape[0] == 0:
        raise ValueError(f"{path}: expected an [N, 3] array of points, got {a.shape}")
    a = a[:, :3].astype(np.float32)
    if not np.isfinite(a).all():
        a = a[np.isfinite(a).all(axis=1)]   # depth cameras mark invalid pixels with NaN / inf
    return np.ascontiguousarray(a)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _read_ply_vertices(path):
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n_vert, props, in_vertex = None, 0, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header has no end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n_vert = int(tok[2])
                elif not props:
                    raise ValueError(f"{path}: an element precedes `vertex`; not supported")
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list property on vertices is not supported")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in ("x", "y", "z")):
            raise ValueError(f"{path}: vertex element has no x / y / z")
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=n_vert, ndmin=2)
            return np.stack([rows[:, names.index(k)] for k in ("x", "y", "z")], axis=1)
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
        dt = np.dtype([(n, "<" + t) for n, t in props])
        v = np.frombuffer(f.read(dt.itemsize * n_vert), dtype=dt, count=n_vert)
        return np.stack([v["x"], v["y"], v["z"]], axis=1)


# ------------------------------------------------------------------------------------------ tabletop segmentation --
# a RANSAC table plane (gldm_plane_ransac, gldm_plane_moments) and the objects above it as connected
# components of the depth image (gldm_segment_tabletop).  The draws and the 3 x 3 eigen-solve stay on the host.
RANSAC_MAX_HYPOTHESES = 4096   # gldm_plane_ransac's ceiling on t


class TablePlane:
    """A plane n . p + offset = 0 (f32): `normal` numpy [3], `offset` float, `inliers` (points within tol of the winning
    hypothesis) and `hypothesis` (its index among the draws).  The camera centre has positive height."""

    def __init__(self, normal, offset, inliers=0, hypothesis=-1):
        self.normal = np.asarray(normal, dtype=np.float32).reshape(3)
        self.offset = float(np.float32(offset))
        self.inliers = int(inliers)
        self.hypothesis = int(hypothesis)

    def as_array(self):
        return np.ascontiguousarray(np.append(self.normal, np.float32(self.offset)).astype(np.float32))

    def __repr__(self):
        return f"TablePlane(normal={self.normal.tolist()}, offset={self.offset}, inliers={self.inliers}, hypothesis={self.hypothesis})"


def segment_tile_shape():
    """(tile width, tile height) in pixels of gldm_segment_tabletop's first launch."""
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    L.call("gldm_segment_tile_shape", ctypes.byref(tw), ctypes.byref(th))
    return tw.value, th.value


def plane_ransac(points, triples, tol, min_cross2=1e-8):
    """gldm_plane_ransac: points CUDA [n, 3] f32, triples integer [T, 3] (host or device) -> (planes [T, 4] f32,
    counts [T] int32) on the device; a degenerate hypothesis has plane 0 and count -1."""
    _need_cuda(points, "points")
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], not {tuple(points.shape)}")
    pts = points.contiguous().float()
    dev = pts.device
    tri = torch.as_tensor(triples).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    n, t = pts.shape[0], tri.shape[0]
    ws, nbytes = L.workspace("gldm_plane_ransac", (n, t), torch.int32, dev,
                             f"n = {n}, t = {t}; 1 <= n <= 2^24, 1 <= t <= {RANSAC_MAX_HYPOTHESES}")
    planes = torch.empty((t, 4), dtype=torch.float32, device=dev)
    counts = torch.empty(t, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_plane_ransac", L.ptr(pts), n, L.ptr(tri), t, float(tol), float(min_cross2), L.ptr(ws), nbytes,
               L.ptr(planes), L.ptr(counts), L.current_stream(dev))
    return planes, counts


def plane_moments(points, plane, tol):
    """gldm_plane_moments: points CUDA [n, 3], plane 4 host floats -> f64 [10] on the device: count, the three sums and the
    six second moments of the points within tol of the plane."""
    _need_cuda(points, "points")
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [n, 3], not {tuple(points.shape)}")
    pts = points.contiguous().float()
    dev = pts.device
    pl = _host_floats(plane, 4, "plane")
    n = pts.shape[0]
    ws, nbytes = L.workspace("gldm_plane_moments", (n,), torch.float64, dev, f"n = {n}; 1 <= n <= 2^24")
    out = torch.empty(10, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_plane_moments", L.ptr(pts), n, _host_ptr(pl), float(tol), L.ptr(ws), nbytes,
               L.ptr(out), L.current_stream(dev))
    return out


def _camera_centre(cam_to_world):
    if cam_to_world is None:
        return np.zeros(3, dtype=np.float64)
    t = np.asarray(cam_to_world.detach().cpu() if isinstance(cam_to_world, torch.Tensor) else cam_to_world, dtype=np.float32)
    return t[:3, 3].astype(np.float64)


def orient_plane(normal, offset, centre):
    """(normal, offset) f32 with the sign that gives `centre` positive height; a centre on the plane: the first non-zero
    component of the normal positive."""
    n = np.asarray(normal, dtype=np.float32)
    o = np.float32(offset)
    hgt = float(np.dot(n.astype(np.float64), centre) + np.float64(o))
    if hgt == 0.0:
        nz = n[n != 0]
        flip = nz.size > 0 and nz[0] < 0
    else:
        flip = hgt < 0.0
    return (-n, -o) if flip else (n, o)


def plane_from_moments(m):
    """Least-squares plane of the moments (f64 [10]: count, sums, second moments): the eigenvector of the smallest eigenvalue
    of the covariance (numpy.linalg.eigh, f64), offset = -n . mean, both rounded to f32."""
    m = np.asarray(m, dtype=np.float64)
    cnt = m[0]
    mean = m[1:4] / cnt
    sec = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]], dtype=np.float64) / cnt
    cov = sec - np.outer(mean, mean)
    _, vec = np.linalg.eigh(cov)
    n = vec[:, 0]
    return n.astype(np.float32), np.float32(-np.dot(n, mean))


def fit_table_plane(depth, camera, tol=0.005, hypotheses=512, rng=None, refit=True, min_cross2=1e-8, mask=None, z_range=None,
                    depth_scale=None, cam_to_world=None, crop_box=None):
    """The dominant plane of one depth frame [H, W] by RANSAC on the GPU -> TablePlane.
    depth_to_cloud (its options: mask, z_range, depth_scale, cam_to_world, crop_box) gives the n points; the triples are
    rng.integers(0, n, (hypotheses, 3)) drawn on the host (rng=None: np.random.default_rng(0)); ONE gldm_plane_ransac call
    scores them and ONE read-back brings the counts; the best is the highest count, ties to the lowest index.  With refit,
    one gldm_plane_moments call over its inliers and the smallest eigenvector of their f64 covariance replace it.  The
    camera centre (translation of cam_to_world, else the origin) gets positive height.  Fewer than 3 points, or every
    hypothesis degenerate: ValueError."""
    _need_cuda(depth, "depth")
    if depth.ndim != 2:
        raise ValueError(f"fit_table_plane takes one frame [H, W], not {tuple(depth.shape)}")
    t = int(hypotheses)
    if not 1 <= t <= RANSAC_MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be 1 .. {RANSAC_MAX_HYPOTHESES}, not {t}")
    cloud = depth_to_cloud(depth, camera, mask=mask, z_range=z_range, depth_scale=depth_scale, cam_to_world=cam_to_world,
                           crop_box=crop_box)
    n = cloud.shape[0]
    if n < 3:
        raise ValueError(f"the frame keeps {n} points; a plane needs 3")
    rng = np.random.default_rng(0) if rng is None else rng
    triples = np.asarray(rng.integers(0, n, (t, 3)), dtype=np.int32)
    planes, counts = plane_ransac(cloud, torch.from_numpy(triples), tol, min_cross2)
    host = counts.cpu().numpy()   # the one read-back of the T counts
    best = int(np.argmax(host))   # the first of the highest
    if host[best] < 0:
        raise ValueError(f"all {t} hypotheses are degenerate (repeated or collinear points); no plane")
    plane = planes[best].cpu().numpy()
    normal, offset = plane[:3], plane[3]
    if refit:
        normal, offset = plane_from_moments(plane_moments(cloud, plane, tol).cpu().numpy())
    normal, offset = orient_plane(normal, offset, _camera_centre(cam_to_world))
    return TablePlane(normal, offset, inliers=int(host[best]), hypothesis=best)


def segment_tabletop(depth, camera, plane=None, height_range=(0.01, 0.5), link_dist=0.01, min_pixels=32, max_objects=64,
                     mask=None, z_range=None, depth_scale=None, cam_to_world=None, crop_box=None, tol=0.005, hypotheses=512,
                     rng=None, refit=True, min_cross2=1e-8, return_stats=False):
    """One depth frame [H, W] -> an instance-label image of the objects on the table, one HIP entry (gldm_segment_tabletop,
    DESIGN.md 4.12).  plane: a TablePlane or 4 numbers (a, b, c, d); None fits one with fit_table_plane (tol, hypotheses, rng,
    refit, min_cross2).  Foreground = pixels depth_to_cloud keeps (same options) whose height over the plane lies in
    (height_range[0], height_range[1]]; 4-neighbours closer than link_dist in 3-D are linked; components of at least
    min_pixels pixels are labelled 1 .. K (K <= max_objects <= 64) by falling pixel count, ties to the lower first pixel.
    -> (labels [H, W] int32 on the device, num_labels, plane); with return_stats also (label_pixels, label_root) host lists."""
    _need_cuda(depth, "depth")
    if depth.ndim != 2:
        raise ValueError(f"segment_tabletop takes one frame [H, W], not {tuple(depth.shape)}")
    fr = _depth_frames(depth, camera, mask, z_range, depth_scale, cam_to_world, crop_box)
    h, w, dev = fr.h, fr.w, fr.device
    if plane is None:
        plane = fit_table_plane(depth, camera, tol=tol, hypotheses=hypotheses, rng=rng, refit=refit, min_cross2=min_cross2,
                                mask=mask, z_range=z_range, depth_scale=depth_scale, cam_to_world=cam_to_world,
                                crop_box=crop_box)
    pl = plane.as_array() if isinstance(plane, TablePlane) else _host_floats(plane, 4, "plane")
    k = int(max_objects)
    if not 1 <= k <= MAX_LABELS:
        raise ValueError(f"max_objects must be 1 .. {MAX_LABELS}, not {k}")
    if int(min_pixels) < 1:
        raise ValueError(f"min_pixels must be at least 1, not {min_pixels}")
    ws, nbytes = L.workspace("gldm_segment_tabletop", (h, w), torch.int64, dev, f"{h} x {w}; 1 <= H*W <= 2^24")
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    stats = torch.empty(1 + 2 * k, dtype=torch.int32, device=dev)   # num_labels, label_pixels, label_root: one read-back
    with torch.cuda.device(dev):
        L.call("gldm_segment_tabletop", *fr.source, h, w, *fr.optics, _host_ptr(pl), float(height_range[0]),
               float(height_range[1]), float(link_dist), int(min_pixels), k, L.ptr(ws), nbytes, L.ptr(labels),
               L.ptr(stats[0:1]), L.ptr(stats[1:1 + k]), L.ptr(stats[1 + k:]), L.current_stream(dev))
    host = stats.tolist()   # the one read-back
    num = host[0]
    if not isinstance(plane, TablePlane):
        plane = TablePlane(pl[:3], pl[3])
    if return_stats:
        return labels, num, plane, host[1:1 + k], host[1 + k:]
    return labels, num, plane


# ------------------------------------------------------------------------------------------------ surface normals --
# the k nearest neighbours within a radius (gldm_knn_radius) and the smallest eigenvector of every
# neighbourhood (gldm_point_normals): estimate_normals_cam_from_pc / vectorized_normal_computation of
# grasp_ldm/utils/pointcloud_helpers.py:74-122 without the round trip through scipy and numpy.
KNN_MAX_K = 16          # gldm_knn_radius' ceiling on k
KNN_MAX_POINTS = 1 << 20   # ... and on the points of one cloud


def _check_knn_envelope(n, k):
    if not 1 <= int(k) <= KNN_MAX_K:
        raise NotImplementedError(f"k = {k}: gldm_knn_radius keeps 1 .. {KNN_MAX_K} neighbours per point")
    if not 1 <= n <= KNN_MAX_POINTS:
        raise NotImplementedError(f"n = {n}: gldm_knn_radius takes 1 .. 2^20 = {KNN_MAX_POINTS} points per cloud")


def _finite_cloud(pcb):
    if not bool(torch.isfinite(pcb).all()):
        raise L.GldmError("the points hold non-finite values")


def knn_radius(pc, k, max_radius):
    """gldm_knn_radius on pc [N,3] or [B,N,3]: for every point the up to k nearest points of its cloud within max_radius,
    itself included, ordered by (squared distance, index) -> (idx int32 [..,N,k], d2 f32 [..,N,k], found int32 [..,N]);
    slots behind found carry idx = N and d2 = +inf (cKDTree.query's convention).  d2 = (dx*dx + dy*dy) + dz*dz in f32."""
    pcb = _as_batch(pc)
    b, n, _ = pcb.shape
    k = int(k)
    _check_knn_envelope(n, k)
    r = float(max_radius)
    if not (r >= 0.0 and r * r <= FLT_MAX):   # r2 finite in f32 (NaN fails both): +inf is the padding of d2
        raise ValueError(f"max_radius must be >= 0 with a finite square in f32, not {max_radius!r}")
    _finite_cloud(pcb)
    dev = pcb.device
    ws, nbytes = L.workspace("gldm_knn_radius", (b, n), torch.float32, dev, f"b = {b}, n = {n}; 1 <= n <= 2^20")
    idx = torch.empty((b, n, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((b, n, k), dtype=torch.float32, device=dev)
    found = torch.empty((b, n), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_knn_radius", L.ptr(pcb), b, n, k, float(max_radius), L.ptr(ws), nbytes, L.ptr(idx), L.ptr(d2),
               L.ptr(found), L.current_stream(dev))
    if pc.ndim == 2:
        return idx[0], d2[0], found[0]
    return idx, d2, found


def _point_normals(pcb, idx, neighbors, k, view_point):
    b, n, _ = pcb.shape
    view = _host_floats(np.zeros(3, dtype=np.float32) if view_point is None else view_point, 3, "view_point")
    if not np.isfinite(view).all():
        raise ValueError("view_point must be finite")
    normals = torch.empty((b, n, 3), dtype=torch.float32, device=pcb.device)
    with torch.cuda.device(pcb.device):
        L.call("gldm_point_normals", L.ptr(pcb), L.ptr(idx), L.ptr(neighbors), b, n, k, _host_ptr(view), L.ptr(normals),
               L.current_stream(pcb.device))
    return normals


def estimate_normals(pc, max_radius=0.05, k=12, view_point=None):
    """Surface normals of pc [N,3] or [B,N,3] -> (normals f32 of pc's shape, found int32 [..,N]): per point the
    eigenvector of the smallest eigenvalue of sum (q - p)(q - p)^T over its up to k nearest neighbours q within max_radius
    (knn_radius), unit length, turned so that dot(normal, p - view_point) < 0 (view_point: 3 numbers, default the origin:
    towards the camera).  Points with found < 3 get the zero vector."""
    pcb = _as_batch(pc)
    idx, _, found = knn_radius(pcb, k, max_radius)
    normals = _point_normals(pcb, idx.contiguous(), None, int(k), view_point)
    if pc.ndim == 2:
        return normals[0], found[0]
    return normals, found


# ----------------------------------------------------------------------------------------------- sensor-cloud cleanup --
# outlier removal between deprojection and farthest-point selection (gldm_neighbor_stats,
# gldm_filter_outliers): Open3D's remove_radius_outlier / remove_statistical_outlier on ragged batches, without the round
# trip through scipy.
CLEANUP_MAX_K = 16              # gldm_neighbor_stats' ceiling on k
CLEANUP_MAX_POINTS = 1 << 20    # ... on the points of one cloud
CLEANUP_MAX_CLOUDS = 65535      # ... and on the clouds of one call


def _check_cleanup_envelope(k, max_radius, min_neighbors=0, std_ratio=None):
    if not 1 <= int(k) <= CLEANUP_MAX_K:
        raise NotImplementedError(f"k = {k}: gldm_neighbor_stats keeps 1 .. {CLEANUP_MAX_K} neighbours per point")
    r = float(max_radius)
    if not (r >= 0.0 and float(np.float32(r)) ** 2 <= FLT_MAX):   # r2 finite in f32 (NaN fails both)
        raise ValueError(f"max_radius must be >= 0 with a finite square in f32, not {max_radius!r}")
    if not 0 <= int(min_neighbors) <= int(k):
        raise ValueError(f"min_neighbors must be 0 .. k = {int(k)}, not {min_neighbors}")
    if std_ratio is not None and float(std_ratio) != float(std_ratio):
        raise ValueError("std_ratio must not be NaN (None or a negative value switches the statistical rule off)")


def _ragged_layout(points, start, count, entry="gldm_neighbor_stats", max_points=CLEANUP_MAX_POINTS):
    """The checks in front of the ragged entries: points [n,3] / [b,n,3] dense, or [rows,3] with start / count (host
    sequences or tensors: one read-back) -> (pts [rows,3] f32 contiguous, start, count as host lists, dense shape or None).
    Raises before any library call.  entry / max_points: the entry named in the messages and its ceiling on the points of
    one cloud (a power of two)."""
    _need_cuda(points, "points")
    if (start is None) != (count is None):
        raise ValueError("start and count go together")
    if start is None:
        pcb = _as_batch(points)
        b, n, _ = pcb.shape
        pts, start, count, dense = pcb.reshape(b * n, 3), [i * n for i in range(b)], [n] * b, tuple(points.shape[:-1])
    else:
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"with start / count, points must be [rows, 3], not {tuple(points.shape)}")
        pts, dense = points.contiguous().float(), None
        start = [int(s) for s in (start.tolist() if isinstance(start, torch.Tensor) else start)]
        count = [int(c) for c in (count.tolist() if isinstance(count, torch.Tensor) else count)]
    b, rows = len(start), pts.shape[0]
    if len(count) != b:
        raise ValueError(f"start holds {b} clouds, count {len(count)}")
    if not 1 <= b <= CLEANUP_MAX_CLOUDS:
        raise NotImplementedError(f"{b} clouds: {entry} takes 1 .. {CLEANUP_MAX_CLOUDS} clouds per call")
    if rows > 0x7fffffff:
        raise NotImplementedError(f"{rows} rows: {entry} takes at most 2^31 - 1 rows per call")
    end = 0
    for i, (s, c) in sorted(enumerate(zip(start, count)), key=lambda t: t[1][0]):
        if c < 0:
            raise ValueError(f"cloud {i}: count {c} is negative")
        if c > max_points:
            raise NotImplementedError(f"cloud {i} has {c} points: {entry} takes at most 2^{max_points.bit_length() - 1} = "
                                      f"{max_points} points per cloud")
        if c and (s < 0 or s + c > rows):
            raise ValueError(f"cloud {i}: rows {s} .. {s + c} leave points [{rows}, 3]")
        if c and s < end:
            raise ValueError(f"cloud {i}: rows {s} .. {s + c} overlap another cloud")
        end = s + c if c else end
    return pts, start, count, dense


def _finite_rows(pts, start, count, dense):
    """Non-finite values inside a cloud's rows raise GldmError; the gaps between the clouds may hold anything."""
    if dense is not None:
        return _finite_cloud(pts)
    bad = (~torch.isfinite(pts)).any(dim=1).to(torch.int32)
    run = torch.cat([torch.zeros(1, dtype=torch.int64, device=pts.device), torch.cumsum(bad, 0)])
    s = torch.tensor(start, dtype=torch.int64, device=pts.device).clamp(0, pts.shape[0])
    e = (s + torch.tensor(count, dtype=torch.int64, device=pts.device)).clamp(0, pts.shape[0])
    if bool((run[e] - run[s]).ne(0).any()):
        raise L.GldmError("the points hold non-finite values")


def _neighbor_stats(pts, sc, b, n_max, k, max_radius):
    """gldm_neighbor_stats on checked arguments; sc int32 [2, b] on the device (start, count) -> (neighbors, score) [rows]."""
    dev, rows = pts.device, pts.shape[0]
    ws, nbytes = L.workspace("gldm_neighbor_stats", (b, n_max), torch.float32, dev,
                             f"b = {b}, n_max = {n_max}; b <= {CLEANUP_MAX_CLOUDS}, n_max <= 2^20")
    neighbors = torch.zeros(rows, dtype=torch.int32, device=dev)
    score = torch.full((rows,), float("inf"), dtype=torch.float32, device=dev)
    if ws is not None and rows:
        with torch.cuda.device(dev):
            L.call("gldm_neighbor_stats", L.ptr(pts), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, int(k), float(max_radius),
                   L.ptr(ws), nbytes, L.ptr(neighbors), L.ptr(score), L.current_stream(dev))
    return neighbors, score


def neighbor_stats(points, k, max_radius, start=None, count=None):
    """gldm_neighbor_stats: for every point the number of OTHER points of its cloud within max_radius, capped at k, and the
    mean distance to the up to k nearest of them (+inf where there is none).  points [n,3] or [b,n,3]; or [rows,3] with
    start / count (host sequences or tensors of b ints): cloud i = rows start[i] .. start[i] + count[i], rows outside every
    cloud are never read.  -> (neighbors int32, score f32) of points' leading shape; rows outside every cloud carry 0 / +inf.
    d2 = (dx*dx + dy*dy) + dz*dz in f32 as in knn_radius; a duplicate of a point is its neighbour at distance 0."""
    _check_cleanup_envelope(k, max_radius)
    pts, start, count, dense = _ragged_layout(points, start, count)
    _finite_rows(pts, start, count, dense)
    sc = torch.tensor([start, count], dtype=torch.int32, device=pts.device)
    neighbors, score = _neighbor_stats(pts, sc, len(start), max(count), k, max_radius)
    if dense is not None:
        return neighbors.reshape(dense), score.reshape(dense)
    return neighbors, score


def remove_outliers(points, k=8, max_radius=0.01, min_neighbors=3, std_ratio=None, start=None, count=None):
    """Outlier removal on the GPU (gldm_neighbor_stats + gldm_filter_outliers).  A point is kept iff it has at
    least min_neighbors other points of its cloud within max_radius (counted up to k: Open3D's remove_radius_outlier) and,
    with std_ratio (None or negative: off), at least one and a mean distance to its up to k nearest of them of at most
    mu + std_ratio * sigma, mean and sample deviation of that figure over the cloud's points with at least
    max(min_neighbors, 1) neighbours (remove_statistical_outlier, bounded by the radius).
    points / start / count as neighbor_stats.  The kept rows keep their order.
    -> (points, start, count, kept, stats): the packed kept rows [total, 3] (bit copies), start / count host lists of b ints
    (ONE read-back), kept int32 [total]: the source row of every output row relative to its cloud's start; stats: dict of
    mu, sigma (f64 [b] on the device), neighbors, score (neighbor_stats' outputs).  For one cloud [n,3]: (points [m,3], 0, m,
    kept [m], stats)."""
    _check_cleanup_envelope(k, max_radius, min_neighbors, std_ratio)
    pts, start, count, dense = _ragged_layout(points, start, count)
    total_in = sum(count)
    if total_in > 0x7fffffff:
        raise NotImplementedError(f"{total_in} points in all: gldm_filter_outliers packs at most 2^31 - 1 rows")
    _finite_rows(pts, start, count, dense)
    dev, rows, b, n_max = pts.device, pts.shape[0], len(start), max(count)
    ratio = -1.0 if std_ratio is None else float(std_ratio)
    sc = torch.tensor([start, count], dtype=torch.int32, device=dev)
    neighbors, score = _neighbor_stats(pts, sc, b, n_max, k, max_radius)
    ws, nbytes = L.workspace("gldm_filter_outliers", (b, n_max), torch.float64, dev,
                             f"b = {b}, n_max = {n_max}; b <= {CLEANUP_MAX_CLOUDS}, n_max <= 2^20")
    out = torch.empty((total_in, 3), dtype=torch.float32, device=dev)
    kept = torch.empty(total_in, dtype=torch.int32, device=dev)
    osc = torch.empty((2, b), dtype=torch.int32, device=dev)   # out_start, out_count: one buffer, one read-back
    mom = torch.empty((b, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_filter_outliers", L.ptr(pts), L.ptr(neighbors), L.ptr(score), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows,
               int(k), int(min_neighbors), ratio, L.ptr(ws), nbytes, L.ptr(out), L.ptr(osc[0]), L.ptr(osc[1]), L.ptr(kept),
               L.ptr(mom), L.current_stream(dev))
    ostart, ocount = osc.tolist()   # the one read-back
    total = sum(ocount)
    stats = dict(mu=mom[:, 0], sigma=mom[:, 1], neighbors=neighbors, score=score)
    if dense is not None:
        stats["neighbors"], stats["score"] = neighbors.reshape(dense), score.reshape(dense)
        if len(dense) == 1:
            return out[:total], 0, total, kept[:total], stats
    return out[:total], ostart, ocount, kept[:total], stats


# ------------------------------------------------------------------------------------------ voxel-grid downsampling --
# one point per occupied voxel between deprojection and everything else (gldm_voxel_downsample): Open3D's
# voxel_down_sample / PCL's VoxelGrid on ragged batches, on a lattice anchored at the origin.
VOXEL_MAX_POINTS = 1 << 22      # gldm_voxel_downsample's ceiling on the points of one cloud
VOXEL_MAX_ROWS = 1 << 24        # ... on the rows of one call
VOXEL_MAX_CELL = 1 << 20        # ... and on |coordinate| / voxel_size
VOXEL_GROW = 1.25               # voxel_downsample_capped: the factor between two attempts
VOXEL_MAX_GROWS = 16            # ... and how often it is applied


def _voxel_size_f32(voxel_size):
    """voxel_size as the f32 value the entry receives; anything but a finite positive number raises ValueError."""
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(voxel_size))
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(voxel_size, bool) or not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"voxel_size must be finite and > 0 in f32, not {voxel_size!r}")
    return v


def _voxel_rows(pts, start, count, dense, v):
    """ONE device reduction and read-back for both conditions on the rows inside the clouds: non-finite values raise
    GldmError, a coordinate with |p| / voxel_size >= 2^20 (in f64, as the kernel divides) raises ValueError.  The gaps
    between the clouds may hold anything."""
    nonfinite = (~torch.isfinite(pts)).any(dim=1)
    far = (~(pts.double().abs() / v < float(VOXEL_MAX_CELL))).any(dim=1) & ~nonfinite
    bad = torch.stack([nonfinite, far]).to(torch.int32)   # [2, rows]
    if dense is not None:
        hit = bad.any(dim=1)
    else:
        run = torch.cat([torch.zeros((2, 1), dtype=torch.int64, device=pts.device), torch.cumsum(bad, 1)], dim=1)
        s = torch.tensor(start, dtype=torch.int64, device=pts.device).clamp(0, pts.shape[0])
        e = (s + torch.tensor(count, dtype=torch.int64, device=pts.device)).clamp(0, pts.shape[0])
        hit = (run[:, e] - run[:, s]).ne(0).any(dim=1)
    hit_nonfinite, hit_far = hit.tolist()   # the one read-back
    if hit_nonfinite:
        raise L.GldmError("the points hold non-finite values")
    if hit_far:
        raise ValueError(f"a coordinate has |p| / voxel_size >= 2^20 = {VOXEL_MAX_CELL} (voxel_size = {v!r}): "
                         "gldm_voxel_downsample's lattice ends there")


def voxel_downsample(points, voxel_size, start=None, count=None, return_map=False):
    """Voxel-grid downsampling on the GPU (gldm_voxel_downsample): one output point per occupied voxel of
    every cloud, the centroid of the voxel's points.  The lattice is anchored at the ORIGIN (cell = floor(p / voxel_size) per
    axis, in f64), not at the cloud's min bound as in Open3D: a voxel means the same place in every frame.  The centroid is
    the mean of the coordinates quantised to voxel_size * 2^-16, summed exactly, so every output bit is independent of the
    execution order (tests/cloud_downsample_ref.py restates it in numpy).  A cloud's voxels come in order of first
    appearance.  points / start / count as neighbor_stats (at most 2^22 points per cloud, 2^24 rows, 65535 clouds per
    call); voxel_size: finite and > 0 as f32; |p| / voxel_size < 2^20 for every coordinate.
    -> (points, start, count, first, members): the packed centroids [total, 3], start / count host lists of b ints (the
    second read-back; the first brings the finite / range check), first int32 [total]: the lowest source row of every
    voxel relative to its cloud's start, members int32 [total]: its number of points.  With return_map also voxel int32
    of points' leading shape: the output row of every source row, relative to its cloud's start in the output (-1 outside
    every cloud): labels, pixels or normals can be carried over with it.  For one cloud [n,3]: (points [m,3], 0, m, first [m],
    members [m][, voxel [n]])."""
    v = _voxel_size_f32(voxel_size)
    pts, start, count, dense = _ragged_layout(points, start, count, "gldm_voxel_downsample", VOXEL_MAX_POINTS)
    rows, b, n_max, total_in = pts.shape[0], len(start), max(count), sum(count)
    if rows > VOXEL_MAX_ROWS:
        raise NotImplementedError(f"{rows} rows: gldm_voxel_downsample takes at most 2^24 = {VOXEL_MAX_ROWS} rows per call")
    _voxel_rows(pts, start, count, dense, v)
    dev = pts.device
    sc = torch.tensor([start, count], dtype=torch.int32, device=dev)
    ws, nbytes = L.workspace("gldm_voxel_downsample", (b, n_max, rows), torch.int64, dev,
                             f"b = {b}, n_max = {n_max}, rows = {rows}; b <= {CLEANUP_MAX_CLOUDS}, n_max <= 2^22, rows <= 2^24")
    out = torch.empty((total_in, 3), dtype=torch.float32, device=dev)
    fm = torch.empty((2, total_in), dtype=torch.int32, device=dev)   # first, members
    osc = torch.empty((2, b), dtype=torch.int32, device=dev)         # out_start, out_count: one buffer, one read-back
    vox = torch.full((rows,), -1, dtype=torch.int32, device=dev) if return_map else None
    with torch.cuda.device(dev):
        L.call("gldm_voxel_downsample", L.ptr(pts), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, v, L.ptr(ws), nbytes,
               L.ptr(out), L.ptr(osc[0]), L.ptr(osc[1]), L.ptr(fm[0]), L.ptr(fm[1]), L.ptr(vox), L.current_stream(dev))
    ostart, ocount = osc.tolist()   # the second read-back
    total = sum(ocount)
    res = (out[:total], ostart, ocount, fm[0, :total], fm[1, :total])
    if dense is not None and len(dense) == 1:
        res = (out[:total], 0, total, fm[0, :total], fm[1, :total])
    if return_map:
        res += (vox.reshape(dense) if dense is not None else vox,)
    return res


def voxel_downsample_capped(points, voxel_size, max_points=None, start=None, count=None, return_map=False):
    """voxel_downsample with a ceiling on the points of every cloud: while any cloud's output count exceeds max_points
    (None: no ceiling) the WHOLE call is repeated with voxel_size * 1.25, at most 16 times, then ValueError.  One size holds
    for all clouds of the call.  -> (voxel_downsample's result, the voxel size used, as the f32 value the entry received)."""
    size = float(voxel_size)
    for _ in range(VOXEL_MAX_GROWS + 1):
        res = voxel_downsample(points, size, start=start, count=count, return_map=return_map)
        most = res[2] if isinstance(res[2], int) else max(res[2])
        if max_points is None or most <= int(max_points):
            return res, _voxel_size_f32(size)
        size *= VOXEL_GROW
    raise ValueError(f"a cloud still holds {most} voxels, above max_points = {max_points}, after voxel_size grew "
                     f"{VOXEL_MAX_GROWS} times by {VOXEL_GROW} from {voxel_size!r}")


# --------------------------------------------------------------------------------------------- Euclidean clustering --
# the objects of a cloud that has no pixel grid (several cameras fused, a downsampled or filtered cloud, a
# file): connected components under "closer than link_dist" (gldm_cluster_cloud: PCL's EuclideanClusterExtraction) and the
# ordered split of the labelled cloud into its objects (gldm_split_labels), without the round trip through cKDTree.
CLUSTER_MAX_POINTS = 1 << 22    # gldm_cluster_cloud's ceiling on the points of one cloud
CLUSTER_MAX_ROWS = 1 << 24      # ... and on the rows of one call
CLUSTER_MIN_LINK = 2.0 ** -60   # link_dist lies in [2^-60, 2^60]
CLUSTER_MAX_LINK = 2.0 ** 60
SPLIT_MAX_COUNTERS = 1 << 24    # gldm_split_labels: clouds * ceil(n_max / 256) * max_objects


def _link_dist_f32(link_dist):
    """link_dist as the f32 value the entry receives; anything outside [2^-60, 2^60] raises ValueError."""
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(link_dist))
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(link_dist, bool) or not CLUSTER_MIN_LINK <= v <= CLUSTER_MAX_LINK:
        raise ValueError(f"link_dist must lie in [2^-60, 2^60] as f32, not {link_dist!r}")
    return v


def _max_objects(max_objects):
    k = int(max_objects)
    if not 1 <= k <= MAX_LABELS:
        raise ValueError(f"max_objects must be 1 .. {MAX_LABELS}, not {max_objects}")
    return k


def _cluster_layout(points, start, count, entry):
    pts, start, count, dense = _ragged_layout(points, start, count, entry, CLUSTER_MAX_POINTS)
    if pts.shape[0] > CLUSTER_MAX_ROWS:
        raise NotImplementedError(f"{pts.shape[0]} rows: {entry} takes at most 2^24 = {CLUSTER_MAX_ROWS} rows per call")
    return pts, start, count, dense


def cluster_cloud(points, link_dist=0.01, min_points=32, max_objects=64, plane=None, height_range=(0.01, 0.5), start=None,
                  count=None, return_stats=False):
    """Euclidean clustering on the GPU (gldm_cluster_cloud): the connected components of every cloud under
    "two rows are linked iff (dx*dx + dy*dy) + dz*dz <= link_dist^2 in f32" -- PCL's EuclideanClusterExtraction, Open3D's
    cluster_dbscan(min_points=1) -- exact, independent of the execution order and restated bit for bit in numpy
    (tests/cloud_cluster_ref.py).  points / start / count as voxel_downsample (at most 2^22 points per cloud, 2^24 rows,
    65535 clouds per call); the points may hold anything: a row with a non-finite coordinate, or with |p| / link_dist
    beyond 2^20, is inactive (label 0, linked to nothing).  plane: a TablePlane or 4 numbers; then only the rows whose
    height over it lies in (height_range[0], height_range[1]] are active (segment_tabletop's rule).  Components of at least
    min_points rows are labelled 1 .. K (K <= max_objects <= 64) by falling size, ties to the lower first row.
    The cost per row is the number of rows in the 27 cells of size link_dist around it; a cloud with all its points within
    link_dist of each other costs n^2: downsample first (voxel_downsample at a voxel below link_dist).
    -> (labels int32 of points' leading shape on the device -- rows outside every cloud carry 0 --, num_labels); with
    return_stats also (label_points, label_root): the sizes and the lowest rows (relative to the cloud's start) of the
    labels.  For one cloud [n,3] num_labels is an int and the stats are lists of max_objects ints; otherwise lists per
    cloud.  ONE read-back (the small tables)."""
    link = _link_dist_f32(link_dist)
    k = _max_objects(max_objects)
    if int(min_points) < 1:
        raise ValueError(f"min_points must be at least 1, not {min_points}")
    pl = None
    if plane is not None:
        pl = plane.as_array() if isinstance(plane, TablePlane) else _host_floats(plane, 4, "plane")
        h0, h1 = float(height_range[0]), float(height_range[1])
        if not np.isfinite(pl).all() or not h0 < h1:
            raise ValueError(f"the plane must be finite and height_range rising, not {pl.tolist()}, {height_range!r}")
    else:
        h0, h1 = 0.0, 0.0
    pts, start, count, dense = _cluster_layout(points, start, count, "gldm_cluster_cloud")
    dev, rows, b, n_max = pts.device, pts.shape[0], len(start), max(count)
    sc = torch.tensor([start, count], dtype=torch.int32, device=dev)
    ws, nbytes = L.workspace("gldm_cluster_cloud", (b, n_max, rows), torch.int64, dev,
                             f"b = {b}, n_max = {n_max}, rows = {rows}; b <= {CLEANUP_MAX_CLOUDS}, n_max <= 2^22, rows <= 2^24")
    labels = torch.zeros(rows, dtype=torch.int32, device=dev)
    stats = torch.empty(b * (1 + 2 * k), dtype=torch.int32, device=dev)   # num_labels, label_points, label_root
    with torch.cuda.device(dev):
        L.call("gldm_cluster_cloud", L.ptr(pts), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, link,
               None if pl is None else _host_ptr(pl), h0, h1, int(min_points), k, L.ptr(ws), nbytes, L.ptr(labels),
               L.ptr(stats[:b]), L.ptr(stats[b:b + b * k]), L.ptr(stats[b + b * k:]), L.current_stream(dev))
    host = stats.tolist()   # the one read-back
    num = host[:b]
    sizes = [host[b + i * k:b + (i + 1) * k] for i in range(b)]
    roots = [host[b + b * k + i * k:b + b * k + (i + 1) * k] for i in range(b)]
    if dense is not None:
        labels = labels.reshape(dense)
        if len(dense) == 1:
            num, sizes, roots = num[0], sizes[0], roots[0]
    if return_stats:
        return labels, num, sizes, roots
    return labels, num


def split_labels(points, labels, max_objects=64, start=None, count=None):
    """The rows of a labelled cloud packed object by object (gldm_split_labels): the rows with label 1 ..
    max_objects go out cloud-major, then by ascending label, then by ascending row; every other label is dropped.
    points / start / count as cluster_cloud; labels: an integer tensor of points' leading shape.
    -> (packed [total, 3] -- bit copies --, obj_start, obj_count, src_row): obj_start / obj_count are host lists of
    clouds * max_objects ints in (cloud, label) order (ONE read-back), obj_start absolute in packed and running on over
    empty objects; src_row int32 [total] is every output row's source row relative to its cloud.  (packed, obj_start,
    obj_count) with the empty objects left out is what regularize_objects, remove_outliers and voxel_downsample take."""
    k = _max_objects(max_objects)
    pts, start, count, dense = _cluster_layout(points, start, count, "gldm_split_labels")
    dev, rows, b, n_max = pts.device, pts.shape[0], len(start), max(count)
    if not isinstance(labels, torch.Tensor) or labels.dtype.is_floating_point or labels.numel() != rows:
        raise ValueError(f"labels must be an integer tensor of {rows} entries, one per row of points")
    if b * ((n_max + 255) // 256) * k > SPLIT_MAX_COUNTERS:
        raise NotImplementedError(f"{b} clouds of up to {n_max} points at {k} objects: gldm_split_labels keeps clouds * "
                                  f"ceil(n_max / 256) * max_objects <= 2^24 = {SPLIT_MAX_COUNTERS}")
    lab = labels.to(device=dev, dtype=torch.int32).reshape(rows).contiguous()
    sc = torch.tensor([start, count], dtype=torch.int32, device=dev)
    ws, nbytes = L.workspace("gldm_split_labels", (b, n_max, rows, k), torch.int64, dev,
                             f"b = {b}, n_max = {n_max}, rows = {rows}, max_objects = {k}")
    out = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    src = torch.empty(rows, dtype=torch.int32, device=dev)
    tab = torch.empty(2 * b * k + 1, dtype=torch.int32, device=dev)   # obj_start, obj_count, out_total: one read-back
    with torch.cuda.device(dev):
        L.call("gldm_split_labels", L.ptr(pts), L.ptr(lab), L.ptr(sc[0]), L.ptr(sc[1]), b, n_max, rows, k, L.ptr(ws), nbytes,
               L.ptr(out), L.ptr(src), L.ptr(tab[:b * k]), L.ptr(tab[b * k:2 * b * k]), L.ptr(tab[2 * b * k:]),
               L.current_stream(dev))
    host = tab.tolist()   # the one read-back
    total = host[-1]
    return out[:total], host[:b * k], host[b * k:2 * b * k], src[:total]


def fit_plane(points, tol=0.005, hypotheses=512, rng=None, refit=True, min_cross2=1e-8, view_point=None):
    """The dominant plane of a cloud [n, 3] by RANSAC on the GPU -> TablePlane: everything fit_table_plane does after its
    deprojection, on a given cloud.  The triples are rng.integers(0, n, (hypotheses, 3)) drawn on the host (rng=None:
    np.random.default_rng(0)); ONE gldm_plane_ransac call scores them and ONE read-back brings the counts; the best is the
    highest count, ties to the lowest index.  With refit, one gldm_plane_moments call over its inliers and the smallest
    eigenvector of their f64 covariance replace it.  view_point (3 numbers, default the origin) gets positive height: it plays
    the camera centre's part.  Fewer than 3 points, or every hypothesis degenerate: ValueError."""
    _need_cuda(points, "points")
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"fit_plane takes one cloud [n, 3], not {tuple(points.shape)}")
    t = int(hypotheses)
    if not 1 <= t <= RANSAC_MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be 1 .. {RANSAC_MAX_HYPOTHESES}, not {t}")
    view = np.zeros(3, dtype=np.float64) if view_point is None else _host_floats(view_point, 3, "view_point").astype(np.float64)
    if not np.isfinite(view).all():
        raise ValueError("view_point must be finite")
    n = points.shape[0]
    if n < 3:
        raise ValueError(f"the cloud holds {n} points; a plane needs 3")
    rng = np.random.default_rng(0) if rng is None else rng
    triples = np.asarray(rng.integers(0, n, (t, 3)), dtype=np.int32)
    planes, counts = plane_ransac(points, torch.from_numpy(triples), tol, min_cross2)
    host = counts.cpu().numpy()   # the one read-back of the T counts
    best = int(np.argmax(host))   # the first of the highest
    if host[best] < 0:
        raise ValueError(f"all {t} hypotheses are degenerate (repeated or collinear points); no plane")
    plane = planes[best].cpu().numpy()
    normal, offset = plane[:3], plane[3]
    if refit:
        normal, offset = plane_from_moments(plane_moments(points, plane, tol).cpu().numpy())
    normal, offset = orient_plane(normal, offset, view)
    return TablePlane(normal, offset, inliers=int(host[best]), hypothesis=best)


def segment_cloud(points, plane=None, table=True, height_range=(0.01, 0.5), link_dist=0.01, min_points=32, max_objects=64,
                  tol=0.005, hypotheses=512, rng=None, refit=True, min_cross2=1e-8, view_point=None):
    """One unorganised cloud [n, 3] -> the labels of the objects in it, segment_tabletop without a pixel
    grid.  table=True: the rows whose height over the table plane lies in (height_range[0], height_range[1]] are clustered
    (cluster_cloud); plane: a TablePlane or 4 numbers, None fits one with fit_plane (tol, hypotheses, rng, refit, min_cross2,
    view_point).  table=False: plain clustering of every row, and the plane returned is None (a plane given with it is an
    error).  -> (labels [n] int32 on the device, num_labels, plane)."""
    _need_cuda(points, "points")
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"segment_cloud takes one cloud [n, 3], not {tuple(points.shape)}")
    if not table:
        if plane is not None:
            raise ValueError("table=False clusters every row: it takes no plane")
        labels, num = cluster_cloud(points, link_dist=link_dist, min_points=min_points, max_objects=max_objects)
        return labels, num, None
    _link_dist_f32(link_dist), _max_objects(max_objects)   # before the fit's launches
    if plane is None:
        plane = fit_plane(points, tol=tol, hypotheses=hypotheses, rng=rng, refit=refit, min_cross2=min_cross2,
                          view_point=view_point)
    elif not isinstance(plane, TablePlane):
        pl = _host_floats(plane, 4, "plane")
        plane = TablePlane(pl[:3], pl[3])
    labels, num = cluster_cloud(points, link_dist=link_dist, min_points=min_points, max_objects=max_objects, plane=plane,
                                height_range=height_range)
    return labels, num, plane


# ------------------------------------------------------------------------------------------------ meshes

MESH_MAX_SAMPLES = 1 << 24       # gldm_mesh_sample_surface: n
MESH_MAX_SAMPLE_ROWS = 1 << 28   # b * n
RENDER_MAX_PIXELS = 1 << 24      # gldm_render_depth: h * w
RENDER_MAX_FRAMES = 65535
RENDER_MAX_INSTANCES = 65535
RENDER_MAX_TRIANGLES = 1 << 24


def _mesh_device(device, *tensors):
    for t in tensors:
        if t is not None:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def sample_mesh_surface(meshes, n, rand=None, seed=None, return_faces=False, return_normals=False, device=None):
    """n points on the surface of every mesh, faces drawn by area: trimesh's `mesh.sample(n)` (acronym_pointclouds.py:
    173-176, 402) as one HIP entry (gldm_mesh_sample_surface; the exact rule is in include/gldm.h).
      meshes   a graspldm_amd.mesh.MeshBatch, a Mesh or a sequence of meshes (B of them)
      rand     CUDA f32 [B, n, 3] uniforms in [0, 1), multiples of 2^-24 (torch.rand gives such); or
      seed     int: the uniforms are drawn in the kernel (Philox4x32-10 keyed on (seed, mesh, sample)); with neither, a seed
               is drawn from torch's CPU generator, so torch.manual_seed makes a run repeatable
    -> points [B, n, 3]; with return_faces also face [B, n] int32 (the row of the batch's packed face array, -1 for a mesh
    without area, whose points are zero); with return_normals also the unit face normals [B, n, 3]."""
    from .mesh import MeshBatch
    mb = MeshBatch.of(meshes)
    b, n = len(mb), int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, not {n}")
    if n > MESH_MAX_SAMPLES or b * n > MESH_MAX_SAMPLE_ROWS:
        raise NotImplementedError(f"{b} meshes x {n} samples: gldm_mesh_sample_surface takes at most 2^24 samples per mesh "
                                  f"and 2^28 per call")
    if rand is not None and seed is not None:
        raise ValueError("give the uniforms (rand) or a seed for the in-kernel generator, not both")
    if rand is not None:
        _need_cuda(rand, "rand")
        if tuple(rand.shape) != (b, n, 3) or rand.dtype != torch.float32:
            raise ValueError(f"rand must be f32 [{b}, {n}, 3], not {rand.dtype} {tuple(rand.shape)}")
        rand = rand.contiguous()
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, ()))
    seed = 0 if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must fit 64 unsigned bits, not {seed}")
    dev = _mesh_device(device, rand)
    verts, faces, rg = mb.on(dev)
    sizes = (b, mb.f_max, verts.shape[0], faces.shape[0], n)
    points = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    face = torch.empty((b, n), dtype=torch.int32, device=dev) if return_faces else None
    normals = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if return_normals else None
    if n:
        ws, nbytes = L.workspace("gldm_mesh_sample_surface", sizes, torch.int64, dev, f"{b} meshes, {n} samples")
        with torch.cuda.device(dev):
            L.call("gldm_mesh_sample_surface", L.ptr(verts), L.ptr(faces), L.ptr(rg[0]), L.ptr(rg[1]), L.ptr(rg[2]),
                   L.ptr(rg[3]), *sizes, L.ptr(rand), seed, L.ptr(ws), nbytes, L.ptr(points), L.ptr(face), L.ptr(normals),
                   L.current_stream(dev))
    out = (points,) + ((face,) if return_faces else ()) + ((normals,) if return_normals else ())
    return out[0] if len(out) == 1 else out


def _poses(m, name):
    a = np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float64)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError(f"{name} must be 4 x 4 (or 3 x 4) or a stack of such, not {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} must be finite")
    full = np.tile(np.eye(4), (a.shape[0], 1, 1))
    full[:, :a.shape[1]] = a
    return full


def render_plan(mb, camera, world_to_cam, instances):
    """The host half of render_depth, without a HIP call: the instance table and the frame ranges of gldm_render_depth as
    numpy arrays, every limit checked.  -> dict(mesh, xf [I, 12] f32, label, tri [I], n_tris, frame_start, frame_count,
    h, w, optics (fx, fy, cx, cy, z_near, z_far))."""
    b = len(mb)
    poses = _poses(world_to_cam, "world_to_cam")
    if instances is None:   # one frame per (mesh, pose) pair, mesh-major
        frames = [[(i, np.eye(4), 1)] for i in range(b) for _ in range(poses.shape[0])]
        poses = np.tile(poses, (b, 1, 1))
    else:
        frames = [list(f) for f in instances]
        if poses.shape[0] == 1:
            poses = np.tile(poses, (len(frames), 1, 1))
        if poses.shape[0] != len(frames):
            raise ValueError(f"{len(frames)} frames of instances but {poses.shape[0]} camera poses")
    h, w = int(camera.height), int(camera.width)
    fx, fy, cx, cy = camera.intrinsics
    z_near, z_far = float(np.float32(camera.z_near)), float(np.float32(camera.z_far))
    if h < 1 or w < 1 or not frames:
        raise ValueError(f"render_depth needs at least one frame of at least one pixel, not {len(frames)} of {h} x {w}")
    if h * w > RENDER_MAX_PIXELS:
        raise NotImplementedError(f"frames of {h} x {w}: gldm_render_depth takes at most 2^24 pixels per frame")
    if len(frames) > RENDER_MAX_FRAMES:
        raise NotImplementedError(f"{len(frames)} frames: gldm_render_depth takes at most {RENDER_MAX_FRAMES} per call")
    if not (np.isfinite([fx, fy, cx, cy]).all() and np.float32(fx) != 0 and np.float32(fy) != 0):
        raise ValueError(f"the camera needs finite intrinsics and fx, fy != 0, not {(fx, fy, cx, cy)}")
    if not 0 < z_near < z_far < float("inf"):
        raise ValueError(f"the camera needs 0 < z_near < z_far, not {camera.z_near}, {camera.z_far}")
    mesh, xf, label, fstart, fcount = [], [], [], [], []
    for pose, frame in zip(poses, frames):
        fstart.append(len(mesh))
        fcount.append(len(frame))
        for inst in frame:
            inst = tuple(inst)
            if len(inst) not in (2, 3):
                raise ValueError("an instance is (mesh id, obj_to_world) or (mesh id, obj_to_world, label)")
            m, obj_to_world = inst[:2]
            lab = inst[2] if len(inst) == 3 else len(mesh) - fstart[-1] + 1
            if not 0 <= int(m) < b:
                raise ValueError(f"instance of mesh {m}: the batch holds {b} meshes")
            if int(lab) < 1 or int(lab) > 2 ** 31 - 1:
                raise ValueError(f"an instance label must be an int32 >= 1, not {lab}")
            mesh.append(int(m))
            label.append(int(lab))
            xf.append((pose @ _poses(obj_to_world, "obj_to_world")[0])[:3].astype(np.float32).reshape(12))
    if len(mesh) > RENDER_MAX_INSTANCES:
        raise NotImplementedError(f"{len(mesh)} instances: gldm_render_depth takes at most {RENDER_MAX_INSTANCES} per call")
    tris = mb.face_count.astype(np.int64)[np.asarray(mesh, dtype=np.int64)] if mesh else np.zeros(0, np.int64)
    n_tris = int(tris.sum())
    if n_tris > RENDER_MAX_TRIANGLES:
        raise NotImplementedError(f"{n_tris} triangles: gldm_render_depth takes at most 2^24 per call")
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)
    return dict(mesh=i32(mesh), xf=np.asarray(xf, dtype=np.float32).reshape(-1, 12), label=i32(label),
                tri=i32(np.cumsum(tris) - tris), n_tris=n_tris, frame_start=i32(fstart), frame_count=i32(fcount), h=h, w=w,
                optics=tuple(float(np.float32(v)) for v in (fx, fy, cx, cy, z_near, z_far)))


def render_depth(meshes, camera, world_to_cam, instances=None, return_labels=False, return_faces=False, device=None):
    """Depth frames of meshes seen by a pinhole camera, one HIP entry (gldm_render_depth; the exact rule is in
    include/gldm.h): what the reference takes from pyrender (acronym_partial_pointclouds.py:521-581).  The frames follow the
    deprojection's conventions -- +z forward, +x right, +y down, pixel (u, v) sampled at its integer coordinates -- so
    depth_to_cloud(render_depth(...)) lies on the surface.  (An OpenGL renderer samples pixel centres, half a pixel further.)
      meshes        a MeshBatch, a Mesh or a sequence of meshes
      camera        graspldm_amd.camera.Camera: intrinsics, image size, z_near / z_far
      world_to_cam  4 x 4, or [P, 4, 4] (camera.look_at / views_on_sphere); host or device, read on the host
      instances     None: every mesh at its own coordinates, one frame per (mesh, pose) pair, mesh-major, label 1.
                    Otherwise one list per frame of (mesh id, obj_to_world 4 x 4, label >= 1) (without a label: 1, 2, .. in
                    the frame's order); world_to_cam then holds one pose, or one per frame.  obj_to_cam = world_to_cam
                    obj_to_world is composed in f64 and rounded once.
    A triangle with a vertex in front of z_near is dropped whole (no clipping), with a warning.
    -> depth [R, h, w] f32, 0 where empty; with return_labels also the labels [R, h, w] int32 (0 = background); with
    return_faces also the rows of the batch's packed face array [R, h, w] int32 (-1 where empty)."""
    from .mesh import MeshBatch
    mb = MeshBatch.of(meshes)
    plan = render_plan(mb, camera, world_to_cam, instances)
    dev = _mesh_device(device)
    verts, faces, rg = mb.on(dev)
    r, h, w, n_inst, n_tris = plan["frame_start"].size, plan["h"], plan["w"], plan["mesh"].size, plan["n_tris"]
    table = torch.from_numpy(np.concatenate([plan["mesh"], plan["label"], plan["tri"], plan["frame_start"],
                                             plan["frame_count"]])).to(dev)
    i_mesh, i_label, i_tri, f_start, f_count = torch.split(table, [n_inst] * 3 + [r] * 2)
    xf = torch.from_numpy(plan["xf"]).to(dev)
    sizes = (len(mb), verts.shape[0], faces.shape[0], n_inst, n_tris, r, h, w)
    ws, nbytes = L.workspace("gldm_render_depth", sizes, torch.int64, dev, f"{r} frames of {h} x {w}, {n_tris} triangles")
    ws = None if ws is None else ws[(-ws.data_ptr() // 8) % 2:]   # 16-byte aligned (torch's allocations are, anyway)
    depth = torch.empty((r, h, w), dtype=torch.float32, device=dev)
    label = torch.empty((r, h, w), dtype=torch.int32, device=dev) if return_labels else None
    face = torch.empty((r, h, w), dtype=torch.int32, device=dev) if return_faces else None
    dropped = torch.empty(r, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("gldm_render_depth", L.ptr(verts), L.ptr(faces), L.ptr(rg[0]), L.ptr(rg[1]), L.ptr(rg[2]), L.ptr(rg[3]),
               sizes[0], sizes[1], sizes[2], L.ptr(i_mesh), L.ptr(xf), L.ptr(i_label), L.ptr(i_tri), n_inst, n_tris,
               L.ptr(f_start), L.ptr(f_count), r, h, w, *plan["optics"], L.ptr(ws), nbytes, L.ptr(depth), L.ptr(label),
               L.ptr(face), L.ptr(dropped), L.current_stream(dev))
    n_dropped = int(dropped.sum())   # the one read-back
    if n_dropped:
        import warnings
        warnings.warn(f"render_depth: {n_dropped} triangles reach in front of z_near = {camera.z_near} and were dropped whole "
                      f"(there is no clipping): move the camera back or lower z_near", RuntimeWarning, stacklevel=2)
    out = (depth,) + ((label,) if return_labels else ()) + ((face,) if return_faces else ())
    return out[0] if len(out) == 1 else out
