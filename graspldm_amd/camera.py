"""Pinhole camera model: mirror of `Camera` (grasp_ldm/utils/camera.py:89-223) for the path from a depth frame to a
cloud.  The deprojection itself is one HIP entry (gldm_depth_to_cloud, csrc/depth_cloud.hip) behind
`graspldm_amd.pointcloud.depth_to_cloud`; this class carries the intrinsics and keeps the reference's method names.
Lens distortion is read and ignored, as in the reference."""
import json
import os

import numpy as np


class Camera:
    """Camera model from a user json file (keys cameraMatrix, distCoeffs, width, height, hfov, vfov)."""

    def __init__(self, camera_json_path, z_near=0.05, z_far=20):
        self.name = os.path.basename(camera_json_path)
        with open(camera_json_path) as f:
            self.data = json.load(f)
        self._setup(z_near, z_far)

    @classmethod
    def from_intrinsics(cls, fx, fy, cx, cy, width, height, z_near=0.05, z_far=20):
        """A camera without a file: the same object from the four intrinsics and the image size."""
        self = cls.__new__(cls)
        self.name = "intrinsics"
        hfov = float(2 * np.arctan2(width, 2 * fx) * 180 / np.pi)
        vfov = float(2 * np.arctan2(height, 2 * fy) * 180 / np.pi)
        self.data = dict(cameraMatrix=[[float(fx), 0.0, float(cx)], [0.0, float(fy), float(cy)], [0.0, 0.0, 1.0]],
                         distCoeffs=[], width=int(width), height=int(height), hfov=hfov, vfov=vfov)
        self._setup(z_near, z_far)
        return self

    def _setup(self, z_near, z_far):
        for key in ("cameraMatrix", "width", "height"):
            if key not in self.data:
                raise KeyError(f"camera json {self.name}: no `{key}`")
        self.K = np.array(self.data["cameraMatrix"], dtype=np.float64)
        if self.K.shape != (3, 3):
            raise ValueError(f"camera json {self.name}: cameraMatrix must be 3 x 3, not {self.K.shape}")
        self.dists = np.array(self.data.get("distCoeffs", []))
        self._fx, self._fy = self.K[0, 0], self.K[1, 1]
        self._cx, self._cy = self.K[0, 2], self.K[1, 2]
        if self._fx == 0 or self._fy == 0:
            raise ValueError(f"camera json {self.name}: zero focal length")
        self.z_near, self.z_far = z_near, z_far
        self.width, self.height = int(self.data["width"]), int(self.data["height"])
        self.xfov, self.yfov = self.data.get("hfov"), self.data.get("vfov")

    @property
    def intrinsics(self):
        """(fx, fy, cx, cy) as Python floats (cast to f32 where they enter the arithmetic, as torch does with the
        reference's f64 scalars)."""
        return float(self._fx), float(self._fy), float(self._cx), float(self._cy)

    def to_pyrender_camera(self):
        raise NotImplementedError("rendering (pyrender) is out of scope on this path")

    def depth_to_pointcloud_torch(self, depth, rgb=None):
        """camera.py:176-215 on a CUDA depth image [H, W] (f32, metres) -> [n, 3] points in the camera frame, in the
        row-major order of torch.where(depth > 0); with rgb [H, W, C] also rgb[v, u, :] of the kept pixels (indexed
        once: the reference indexes it a second time with the same coordinates, which cannot run).
        The predicate is `depth > 0` like the reference's, and NON-FINITE depth is dropped too (the reference would
        carry +inf through as inf / NaN coordinates); z_near / z_far are not applied here, as in the reference.
        CPU tensors are rejected."""
        from .pointcloud import _need_cuda, depth_to_cloud
        assert depth.ndim == 2, f"depth must be [H, W], not {tuple(depth.shape)}"
        height, width = depth.shape[0], depth.shape[1]
        assert height == self.height, "Something went wrong. height of the depth image does not match the camera model."
        assert width == self.width, "Something went wrong. width of the depth image does not match the camera model."
        _need_cuda(depth, "depth")
        if rgb is None:
            return depth_to_cloud(depth, self)
        _need_cuda(rgb, "rgb")
        assert rgb.ndim == 3 and rgb.shape[0] == height and rgb.shape[1] == width, "rgb must be [H, W, C] of the depth's size"
        pc, pix = depth_to_cloud(depth, self, return_pixels=True)
        return pc, rgb.reshape(height * width, -1)[pix.long()]

    def render_depth(self, meshes, world_to_cam, instances=None, return_labels=False, return_faces=False):
        """Depth frames of meshes seen by this camera (graspldm_amd.pointcloud.render_depth: one HIP entry,
        gldm_render_depth), in the conventions of depth_to_pointcloud_torch: what the reference asks pyrender for."""
        from .pointcloud import render_depth
        return render_depth(meshes, self, world_to_cam, instances=instances, return_labels=return_labels,
                            return_faces=return_faces)

    def write_to_dir(self, out_dir):
        json_fp = os.path.join(out_dir, f"camera_{self.name}.json")
        with open(json_fp, "w") as f:
            json.dump(self.data, f)
        return json_fp


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera 4 x 4 (f64) of a camera at `eye` looking at `target`, in the frame of the deprojection: +z forward,
    +x right, +y down.  `up` only has to be no multiple of the viewing direction; where it is, another axis takes its place."""
    eye, target = np.asarray(eye, dtype=np.float64).reshape(3), np.asarray(target, dtype=np.float64).reshape(3)
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise ValueError("look_at: eye and target coincide")
    z = z / np.linalg.norm(z)
    up = np.asarray(up, dtype=np.float64).reshape(3)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9 * max(np.linalg.norm(up), 1e-300):
        x = np.cross(z, np.eye(3)[np.argmin(np.abs(z))])
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, :3] = np.stack([x, y, z])
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def views_on_sphere(n, radius, target=(0.0, 0.0, 0.0), rng=None):
    """n world-to-camera poses [n, 4, 4] (look_at) from eyes drawn uniformly on the sphere of `radius` around `target`, as
    the partial-cloud renders of the reference are taken (acronym_partial_pointclouds.py:521-581).  rng: a
    np.random.Generator / RandomState (with .normal); default np.random."""
    rng = np.random if rng is None else rng
    d = np.asarray(rng.normal(size=(int(n), 3)), dtype=np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    target = np.asarray(target, dtype=np.float64).reshape(3)
    return np.stack([look_at(target + float(radius) * v, target) for v in d]) if n else np.zeros((0, 4, 4))
