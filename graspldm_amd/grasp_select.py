"""Geometric filtering and selection of grasp poses (csrc/grasp_select.hip).

  grasp_clearance   gldm_grasp_clearance: how far the open gripper's segments stay from a WHOLE scene cloud (table and
                    clutter included, 10^5 .. 10^6 points) and how many scene points lie inside the finger-sweep tubes,
                    per pose.  The geometry is the reference's marker geometry (grasp_ldm/utils/gripper.py:26-47, :80-128),
                    which the reference only draws.
  select_grasps     gldm_select_grasps: the best k of a cloud's candidates, or k diverse ones (greedy farthest pose under
                    the control-point distance of grasp_ldm/losses/loss.py:77-127), one workgroup per cloud.
  contact_normals   gldm_grasp_contact_normals: those contacts split by finger, and how many of each side face the fingers
                    (surface normal inside the friction cone around the pose's closing axis).
  GraspSelection    what a caller asks of `_InferenceBase.select_grasps` (inference.py).
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import gripper
from ._lib import GldmError
from .dense import _need_cuda

# the envelope of the two entries (csrc/grasp_select.hip; GLDM_ERR_UNSUPPORTED outside it)
MAX_SCENE_POINTS = 1 << 24
MAX_SEGMENTS = 8
MAX_CANDIDATES = 2048
MAX_CONTROL_POINTS = 64
CHUNK = 256   # scene points staged per step (gldm_grasp_clearance_chunk)
SCORE_BY = ("confidence", "success", "product")


def clearance_supported(ns, sb, ss):
    """The shape limits of gldm_grasp_clearance: ns scene points per cloud, sb body and ss sweep segments."""
    return 1 <= ns <= MAX_SCENE_POINTS and 1 <= sb <= MAX_SEGMENTS and 0 <= ss <= MAX_SEGMENTS


def select_supported(g, k, np_):
    """The shape limits of gldm_select_grasps: g candidates per cloud, k picks, np_ control points."""
    return 1 <= k <= g <= MAX_CANDIDATES and 1 <= np_ <= MAX_CONTROL_POINTS


def _check_finite(named):
    """One device reduction and one read-back for all tensors: GldmError naming the first that holds a non-finite value."""
    flags = torch.stack([torch.isfinite(t).all() for _, t in named]).cpu()
    for (name, _), ok in zip(named, flags.tolist()):
        if not ok:
            raise GldmError(f"{name} hold non-finite values")


def _host_floats(x, name, cols):
    """A small tensor / nested sequence -> (ctypes float array, rows); the segment and control-point arguments of the two
    entries are host arrays (they travel as kernel arguments)."""
    t = torch.as_tensor(x, dtype=torch.float32).detach().cpu().reshape(-1)
    if t.numel() % cols:
        raise RuntimeError(f"{name} must be [n,{cols // 3},3]" if cols == 6 else f"{name} must be [n,3]")
    if not bool(torch.isfinite(t).all()):
        raise GldmError(f"{name} hold non-finite values")
    return (ctypes.c_float * max(1, t.numel()))(*t.tolist()), t.numel() // cols


def _poses(H, name="H"):
    _need_cuda(H, name)
    if H.ndim == 3:
        H = H.unsqueeze(0)
    if H.ndim != 4 or H.shape[-2:] != (4, 4) or H.shape[0] < 1 or H.shape[1] < 1:
        raise RuntimeError(f"{name} must be [B,G,4,4] (or [G,4,4] for one cloud), not {tuple(H.shape)}")
    return H.contiguous().float()


def grasp_clearance(scene, H, *, body_segments=None, sweep_segments=None, sweep_radius=gripper.SWEEP_RADIUS,
                    max_clearance=0.05):
    """scene [B, Ns, 3] (or [Ns, 3]) in the frame of the poses H [B, G, 4, 4] (or [G, 4, 4]) -> (clearance [B, G] f32,
    contacts [B, G] int32).  clearance = min(max_clearance, distance of the nearest scene point to the nearest body segment)
    with the point taken into the gripper frame, q = R^T (p - t); contacts = scene points within sweep_radius of a sweep
    segment.  body_segments [Sb, 2, 3] default to gripper.OPEN_SEGMENTS, sweep_segments [Ss, 2, 3] to gripper.SWEEP_SEGMENTS
    (an empty list: no contact test).  max_clearance is what makes the broad phase possible: a point farther than the
    gripper's bounding sphere plus max_clearance is skipped, so it also bounds what a caller can ask of the result."""
    from . import _lib as L
    _need_cuda(scene, "scene")
    H = _poses(H)
    if scene.ndim == 2:
        scene = scene.unsqueeze(0)
    if scene.ndim != 3 or scene.shape[-1] != 3 or scene.shape[0] != H.shape[0]:
        raise RuntimeError(f"scene must be [B,Ns,3] with B = {H.shape[0]} clouds (or [Ns,3] for one), not {tuple(scene.shape)}")
    if scene.device != H.device:
        raise RuntimeError("scene and H must live on the same device")
    body, sb = _host_floats(gripper.OPEN_SEGMENTS if body_segments is None else body_segments, "body_segments", 6)
    sweep, ss = _host_floats(gripper.SWEEP_SEGMENTS if sweep_segments is None else sweep_segments, "sweep_segments", 6)
    b, g = H.shape[:2]
    ns = scene.shape[1]
    if not clearance_supported(ns, sb, ss):
        raise NotImplementedError(f"gldm_grasp_clearance takes 1..{MAX_SCENE_POINTS} scene points per cloud, 1..{MAX_SEGMENTS} "
                                  f"body and 0..{MAX_SEGMENTS} sweep segments, not Ns={ns}, Sb={sb}, Ss={ss}")
    if not (math.isfinite(max_clearance) and max_clearance > 0) or not (math.isfinite(sweep_radius) and sweep_radius >= 0):
        raise ValueError("max_clearance must be > 0 and sweep_radius >= 0")
    scene = scene.contiguous().float()
    _check_finite((("the scene points", scene), ("the grasp poses", H)))
    clearance = torch.empty(b, g, dtype=torch.float32, device=H.device)
    contacts = torch.empty(b, g, dtype=torch.int32, device=H.device)
    with torch.cuda.device(H.device):
        L.call("gldm_grasp_clearance", L.ptr(scene), L.ptr(H), b, g, ns, body, sb, sweep if ss else None, ss,
               ctypes.c_float(sweep_radius), ctypes.c_float(max_clearance), L.ptr(clearance), L.ptr(contacts),
               L.current_stream(H.device))
    return clearance, contacts


def contact_normals(scene, normals, H, *, sweep_segments=None, sweep_radius=gripper.SWEEP_RADIUS, friction_angle_deg=30.0):
    """gldm_grasp_contact_normals: scene and its unit normals [B, Ns, 3] (or [Ns, 3]; pointcloud.estimate_normals), poses H
    [B, G, 4, 4] (or [G, 4, 4]) -> (contacts_side [B, G, 2], aligned [B, G, 2]) int32.  contacts_side: grasp_clearance's
    contacts split by finger (side 0: q.x > 0, the left finger of gripper.OPEN_SEGMENTS; side 1: the rest); aligned: those
    whose normal lies within friction_angle_deg of the pose's closing axis (first column of R), either way round.  A zero
    normal is never aligned."""
    from . import _lib as L
    _need_cuda(scene, "scene")
    _need_cuda(normals, "normals")
    H = _poses(H)
    if scene.ndim == 2:
        scene = scene.unsqueeze(0)
    if normals.ndim == 2:
        normals = normals.unsqueeze(0)
    if scene.ndim != 3 or scene.shape[-1] != 3 or scene.shape[0] != H.shape[0]:
        raise RuntimeError(f"scene must be [B,Ns,3] with B = {H.shape[0]} clouds (or [Ns,3] for one), not {tuple(scene.shape)}")
    if tuple(normals.shape) != tuple(scene.shape):
        raise RuntimeError(f"normals {tuple(normals.shape)} do not match the scene {tuple(scene.shape)}")
    if scene.device != H.device or normals.device != H.device:
        raise RuntimeError("scene, normals and H must live on the same device")
    sweep, ss = _host_floats(gripper.SWEEP_SEGMENTS if sweep_segments is None else sweep_segments, "sweep_segments", 6)
    b, g = H.shape[:2]
    ns = scene.shape[1]
    if not clearance_supported(ns, 1, ss):
        raise NotImplementedError(f"gldm_grasp_contact_normals takes 1..{MAX_SCENE_POINTS} scene points per cloud and "
                                  f"0..{MAX_SEGMENTS} sweep segments, not Ns={ns}, Ss={ss}")
    if not (math.isfinite(sweep_radius) and sweep_radius >= 0):
        raise ValueError("sweep_radius must be >= 0")
    if not (math.isfinite(friction_angle_deg) and 0.0 < friction_angle_deg <= 90.0):
        raise ValueError(f"friction_angle_deg must lie in (0, 90], not {friction_angle_deg!r}")
    scene, normals = scene.contiguous().float(), normals.contiguous().float()
    _check_finite((("the scene points", scene), ("the scene normals", normals), ("the grasp poses", H)))
    side = torch.empty(b, g, 2, dtype=torch.int32, device=H.device)
    aligned = torch.empty(b, g, 2, dtype=torch.int32, device=H.device)
    with torch.cuda.device(H.device):
        L.call("gldm_grasp_contact_normals", L.ptr(scene), L.ptr(normals), L.ptr(H), b, g, ns, sweep if ss else None, ss,
               ctypes.c_float(sweep_radius), ctypes.c_float(friction_cos(friction_angle_deg)), L.ptr(side), L.ptr(aligned),
               L.current_stream(H.device))
    return side, aligned


def friction_cos(friction_angle_deg):
    """cos of the friction angle as gldm_grasp_contact_normals takes it: formed in f64, rounded once to f32."""
    return float(torch.tensor(math.cos(math.radians(friction_angle_deg)), dtype=torch.float64).float())


def select_grasps(H, score, keep=None, k=None, diverse=False, control_points=None, min_separation=0.0):
    """Which k of each cloud's candidates to hand on: H [B, G, 4, 4] (or [G, 4, 4]), score [B, G], keep [B, G] bool or None
    -> (index [B, k] int32, -1 behind the last pick; count [B] int32; gap [B, k] f32).
    diverse=False: the kept candidates by falling score (lowest index first on a tie); gap is 0.
    diverse=True: the best-scored kept candidate first, then repeatedly the one whose control points lie farthest (mean
    squared distance, the reference's pose metric) from every pick so far; stops early once that distance falls below
    min_separation^2.  gap = RMS control-point distance (metres) of a pick to the nearest earlier one, +inf for the first.
    k defaults to G; control_points [Np, 3] to gripper.control_points(16)."""
    from . import _lib as L
    H = _poses(H)
    b, g = H.shape[:2]
    _need_cuda(score, "score")
    score = score.reshape(b, g).contiguous().float()
    k = g if k is None else int(k)
    ctrl, np_ = _host_floats(gripper.control_points(16) if control_points is None else control_points, "control_points", 3)
    if not select_supported(g, k, np_):
        raise NotImplementedError(f"gldm_select_grasps takes 1 <= k <= G <= {MAX_CANDIDATES} candidates per cloud and "
                                  f"1..{MAX_CONTROL_POINTS} control points, not k={k}, G={g}, Np={np_}")
    if not (math.isfinite(min_separation) and min_separation >= 0):
        raise ValueError("min_separation must be >= 0")
    if keep is not None:
        _need_cuda(keep, "keep")
        keep = keep.reshape(b, g).to(torch.uint8).contiguous()
    _check_finite((("the grasp poses", H), ("the scores", score)))
    index = torch.empty(b, k, dtype=torch.int32, device=H.device)
    count = torch.empty(b, dtype=torch.int32, device=H.device)
    gap = torch.empty(b, k, dtype=torch.float32, device=H.device)
    with torch.cuda.device(H.device):
        L.call("gldm_select_grasps", L.ptr(H), L.ptr(score), L.ptr(keep), b, g, ctrl, np_, k, int(bool(diverse)),
               ctypes.c_float(min_separation), L.ptr(index), L.ptr(count), L.ptr(gap), L.current_stream(H.device))
    return index, count, gap


@dataclass(frozen=True)
class GraspSelection:
    """What to keep of a result dict (`_InferenceBase.select_grasps`).  Filters, cheapest first: min_confidence on the
    decoder's confidence; collision_free (clearance of the open gripper to the scene > body_radius) and min_contacts (scene
    points between the fingers) from one clearance launch; min_success on the classifier's probability, scored for the
    survivors only.  Then top_k (None: every survivor) by `score_by`, or `diverse` ones at least min_separation apart.
    min_aligned_contacts (after the clearance filter, one contact_normals launch): at least that many contacts whose surface
    normal lies within friction_angle_deg of the closing axis -- in total, or with both_fingers on each finger's side; the
    scene's normals are estimated from normals_k neighbours within normals_radius where the caller gives none."""
    min_confidence: Optional[float] = None
    min_success: Optional[float] = None
    collision_free: bool = False
    body_radius: float = gripper.BODY_RADIUS
    min_contacts: int = 0
    top_k: Optional[int] = None
    diverse: bool = False
    min_separation: float = 0.0
    score_by: str = "confidence"
    min_aligned_contacts: int = 0
    friction_angle_deg: float = 30.0
    both_fingers: bool = False
    normals_k: int = 12
    normals_radius: float = 0.05

    def __post_init__(self):
        for name in ("min_confidence", "min_success"):
            v = getattr(self, name)
            if v is not None and not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
                raise ValueError(f"{name} must lie in [0, 1] (or be None), not {v!r}")
        if not (isinstance(self.body_radius, (int, float)) and math.isfinite(self.body_radius) and self.body_radius >= 0):
            raise ValueError(f"body_radius must be >= 0, not {self.body_radius!r}")
        if not (isinstance(self.min_contacts, int) and not isinstance(self.min_contacts, bool) and self.min_contacts >= 0):
            raise ValueError(f"min_contacts must be an integer >= 0, not {self.min_contacts!r}")
        if self.top_k is not None and not (isinstance(self.top_k, int) and not isinstance(self.top_k, bool) and self.top_k >= 1):
            raise ValueError(f"top_k must be an integer >= 1 (or None), not {self.top_k!r}")
        if not (isinstance(self.min_separation, (int, float)) and math.isfinite(self.min_separation) and self.min_separation >= 0):
            raise ValueError(f"min_separation must be >= 0, not {self.min_separation!r}")
        if self.score_by not in SCORE_BY:
            raise ValueError(f"score_by must be one of {SCORE_BY}, not {self.score_by!r}")
        if not (isinstance(self.min_aligned_contacts, int) and not isinstance(self.min_aligned_contacts, bool)
                and self.min_aligned_contacts >= 0):
            raise ValueError(f"min_aligned_contacts must be an integer >= 0, not {self.min_aligned_contacts!r}")
        if not (isinstance(self.friction_angle_deg, (int, float)) and not isinstance(self.friction_angle_deg, bool)
                and math.isfinite(self.friction_angle_deg) and 0.0 < self.friction_angle_deg <= 90.0):
            raise ValueError(f"friction_angle_deg must lie in (0, 90], not {self.friction_angle_deg!r}")
        if not isinstance(self.both_fingers, bool):
            raise ValueError(f"both_fingers must be a bool, not {self.both_fingers!r}")
        if not (isinstance(self.normals_k, int) and not isinstance(self.normals_k, bool) and 3 <= self.normals_k <= 16):
            raise ValueError(f"normals_k must be an integer in 3 .. 16 (a plane needs 3 neighbours), not {self.normals_k!r}")
        if not (isinstance(self.normals_radius, (int, float)) and not isinstance(self.normals_radius, bool)
                and math.isfinite(self.normals_radius) and self.normals_radius > 0):
            raise ValueError(f"normals_radius must be > 0, not {self.normals_radius!r}")

    @property
    def needs_clearance(self):
        return bool(self.collision_free) or self.min_contacts > 0

    @property
    def needs_normals(self):
        return self.min_aligned_contacts > 0

    @property
    def needs_scene(self):
        return self.needs_clearance or self.needs_normals

    @property
    def needs_success(self):
        return self.min_success is not None or self.score_by in ("success", "product")


@dataclass(frozen=True)
class CloudCleanup:
    """Outlier removal on the object clouds of a depth frame, between deprojection and point-count regularisation
    (pointcloud.remove_outliers): keep a point iff at least min_neighbors other points of its cloud lie
    within max_radius (counted up to k) and, with std_ratio (None: off), its mean distance to them is at most mu + std_ratio
    * sigma of its cloud.  apply_to_scene: filter the scene cloud a GraspSelection is checked against as well."""
    k: int = 8
    max_radius: float = 0.01
    min_neighbors: int = 3
    std_ratio: Optional[float] = None
    apply_to_scene: bool = False

    def __post_init__(self):
        if not (isinstance(self.k, int) and not isinstance(self.k, bool) and 1 <= self.k <= 16):
            raise ValueError(f"k must be an integer in 1 .. 16, not {self.k!r}")
        if not (isinstance(self.max_radius, (int, float)) and not isinstance(self.max_radius, bool)
                and math.isfinite(self.max_radius) and self.max_radius >= 0):
            raise ValueError(f"max_radius must be >= 0, not {self.max_radius!r}")
        if not (isinstance(self.min_neighbors, int) and not isinstance(self.min_neighbors, bool)
                and 0 <= self.min_neighbors <= self.k):
            raise ValueError(f"min_neighbors must be an integer in 0 .. k = {self.k}, not {self.min_neighbors!r}")
        if self.std_ratio is not None and not (isinstance(self.std_ratio, (int, float)) and not isinstance(self.std_ratio, bool)
                                               and not math.isnan(self.std_ratio)):
            raise ValueError(f"std_ratio must be a number (or None), not {self.std_ratio!r}")
        if not isinstance(self.apply_to_scene, bool):
            raise ValueError(f"apply_to_scene must be a bool, not {self.apply_to_scene!r}")

    @property
    def options(self):
        """The keyword arguments of pointcloud.remove_outliers."""
        return dict(k=self.k, max_radius=self.max_radius, min_neighbors=self.min_neighbors, std_ratio=self.std_ratio)


@dataclass(frozen=True)
class CloudDownsample:
    """Voxel-grid downsampling of the object clouds of a depth frame or of a sensor cloud, in front of `CloudCleanup` and of
    the point-count regularisation (pointcloud.voxel_downsample): one point per occupied voxel of
    voxel_size metres, the centroid of the voxel's points, on a lattice anchored at the origin.  max_points (None: no
    ceiling): while any cloud of the call keeps more points, the whole call is repeated with voxel_size * 1.25, at most 16
    times (then ValueError); one size holds for all clouds and the results report it.  apply_to_scene: downsample the scene
    cloud a GraspSelection is checked against as well."""
    voxel_size: float = 0.003
    max_points: Optional[int] = None
    apply_to_scene: bool = False

    def __post_init__(self):
        if not (isinstance(self.voxel_size, (int, float)) and not isinstance(self.voxel_size, bool)
                and math.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError(f"voxel_size must be finite and > 0, not {self.voxel_size!r}")
        if self.max_points is not None and not (isinstance(self.max_points, int) and not isinstance(self.max_points, bool)
                                                and self.max_points >= 1):
            raise ValueError(f"max_points must be an integer >= 1 (or None), not {self.max_points!r}")
        if not isinstance(self.apply_to_scene, bool):
            raise ValueError(f"apply_to_scene must be a bool, not {self.apply_to_scene!r}")

    @property
    def options(self):
        """The keyword arguments of pointcloud.voxel_downsample_capped."""
        return dict(voxel_size=self.voxel_size, max_points=self.max_points)
