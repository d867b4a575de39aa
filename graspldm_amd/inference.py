"""Inference harness: mirror of `tools/inference.py` (Experiment :97-158, InferenceLDM
:401-666, InferenceVAE :669-815, unnormalize_* :31-94) for the generation path.

Differences, all additive or documented:
  * a model can be injected directly (`model=`) so the path runs without an experiment
    directory (no ACRONYM data / checkpoints exist offline); datasets are out of scope,
    inputs follow the dataset item contract produced by graspldm_amd.synthetic;
  * `num_inference_steps` is honoured (the reference's CLI ignores `--inference_steps`
    because it passes use_fast_sampler=False: tools/generate_grasps.py:69-79);
  * unnormalise + tmrp_to_H + sigmoid are one HIP launch (gldm_pose_epilogue).
"""
import glob
import os
import warnings
from enum import Enum

import numpy as np
import torch

from .builder import build_model_from_cfg
from .checkpoint import Experiment, fix_state_dict_prefix, load_weights as _load_weights, model_section  # noqa: F401
from .r1d import pose_epilogue, pose_prologue

PC_STD, MRP_STD = 0.05, 0.5


class Conditioning(Enum):
    UNCONDITIONAL = "NORMAL"
    CLASS_CONDITIONED = "CLASS_CONDITIONED"
    REGION_CONDITIONED = "REGION_CONDITIONED"


class ModelType(Enum):
    LDM = "LDM"
    VAE = "VAE"


def unnormalize_pc(pc, metas):
    if pc.ndim == 2:
        return pc * metas["pc_std"].to(pc.device) + metas["pc_mean"].to(pc.device)
    return pc * metas["pc_std"].unsqueeze(-2).to(pc.device) + metas["pc_mean"].unsqueeze(-2).to(pc.device)


class _InferenceBase:
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("graspldm_amd runs on the GPU only (no CPU path)")
        self.model = None
        self.dataset = None
        self.classifier = None
        self.gripper_points = None

    def _results(self, pc, metas, tmrp, cls_logit, num_pcs, num_grasps, all_steps=(), score=True):
        # before anything leaves the device: a lost hand-off inside the fused sampling launch raises here
        # (status, not silent garbage: the reference exits the process on a CUDA error, cuda_utils.cuh:28-37)
        from ._cache import cached_value
        for m in self.model.modules():
            eng = cached_value(m, "_engine")
            if eng is not None:
                eng.check()
        if not bool(torch.isfinite(pc).all()):
            # (ReLU as max(x, 0) drops a NaN where torch.relu keeps it: a NaN point would come out as plausible-looking grasps)
            from ._lib import GldmError
            raise GldmError("the input point cloud holds non-finite coordinates")
        metas = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in metas.items()}
        # mean [B,6] and std [1,6] (normalize_input and the dataset both build them so) broadcast independently
        mean, std = metas["grasp_mean"], metas["grasp_std"]
        H, un, conf = pose_epilogue(tmrp, cls_logit, mean, std, num_grasps)
        # ... and so does a pose that is not a number: the GEMMs multiply f16 pieces -- operands whose size the
        # data sets carry range scales, and anything that still leaves the range must not reach the caller as a grasp
        if not bool(torch.isfinite(H).all()) or (conf is not None and not bool(torch.isfinite(conf).all())):
            from ._lib import GldmError
            bad = int((~torch.isfinite(H.view(-1, 16)).all(dim=1)).sum())
            raise GldmError(f"{bad} of {H.numel() // 16} generated poses are not finite (input cloud / metas out of range, "
                            "or weights whose activations leave the f16 range: rerun under graspldm_amd.numerics.f32_only())")
        steps_H = []
        if all_steps:
            if num_pcs > 1:  # tools/inference.py:631-634
                raise NotImplementedError("Batched grasps for all diffusion steps are not implemented")
            for step in all_steps:  # [tmrp [G,6], logit [G,1]] on the CPU (grasp_ldm.py:223-227)
                Hs, _, _ = pose_epilogue(step[0].to(self.device), None, mean, std, num_grasps)
                steps_H.append(Hs.view(1, num_grasps, 4, 4).cpu())
        out = dict(grasps=H.view(num_pcs, num_grasps, 4, 4), grasp_tmrp=un.view(num_pcs, num_grasps, 6),
                   confidence=conf.view(num_pcs, num_grasps, 1), qualities=None, pc=unnormalize_pc(pc, metas),
                   all_steps_grasps=steps_H)
        if self.classifier is not None and score:   # additive: the key exists only with a classifier set
            out["success"] = self.score_grasps(pc, metas, out["grasps"]).unsqueeze(-1)
        return out

    def _finish(self, out, pc, metas, selection, scene_pc):
        """The tail of every generation entry: with a selection the classifier has not run yet (select_grasps scores the
        poses that the cheap filters leave, or the selected ones)."""
        if selection is None:
            return out
        return self.select_grasps(out, selection, scene_pc=scene_pc, pc=pc, metas=metas)

    @torch.no_grad()
    def select_grasps(self, results, selection, scene_pc=None, pc=None, metas=None, scene_normals=None):
        """Filter and select the poses of a result dict (graspldm_amd.grasp_select.GraspSelection) -> a NEW dict; `results`
        is not modified.  scene_pc [B, Ns, 3] (or [Ns, 3]): the whole scene in the frame of results["pc"] -- table and
        clutter included --, default results["pc"] itself.  pc / metas: the normalised cloud(s) and metas the results were
        generated from; needed only where the classifier has to run (generate_grasps(..., selection=) passes them).
        Cheap first: confidence mask -> one clearance launch (only if collision_free / min_contacts ask for it) -> one
        contact-normals launch (only if min_aligned_contacts asks for it; scene_normals [B, Ns, 3]: the scene's unit
        normals, estimated here with pointcloud.estimate_normals when None; adds aligned_contacts [B, G, 2]) -> the
        classifier on the survivors (only if min_success / score_by need it) -> top-k or diverse launch -> with a classifier
        attached and not yet run, the classifier on the k selected poses.
        grasps, grasp_tmrp, confidence (success, latent_* when present) come back gathered to [B, K, ...], NaN in the slots
        behind selected_count; added keys: selected_index [B, K] (-1 padded), selected_count [B], selected_gap [B, K],
        clearance / contacts [B, G] (None when no filter asked for them)."""
        from . import grasp_select as gs
        if not isinstance(selection, gs.GraspSelection):
            raise TypeError("selection must be a graspldm_amd.grasp_select.GraspSelection")
        H = results["grasps"].to(self.device)
        b, g = H.shape[:2]
        conf = results["confidence"].to(self.device).reshape(b, g)
        keep = torch.ones(b, g, dtype=torch.bool, device=self.device)
        if selection.min_confidence is not None:
            keep &= conf >= selection.min_confidence
        clearance = contacts = aligned = None
        if selection.needs_scene:
            scene = results["pc"] if scene_pc is None else scene_pc
            scene = (scene.unsqueeze(0) if scene.ndim == 2 else scene).to(self.device)
            shared = scene.shape[0] == 1 and b > 1   # one scene for every cloud of the batch
            if shared:
                scene = scene.expand(b, -1, -1)
        if selection.needs_clearance:
            clearance, contacts = gs.grasp_clearance(scene, H, max_clearance=max(0.05, 2.0 * selection.body_radius))
            if selection.collision_free:
                keep &= clearance > selection.body_radius
            if selection.min_contacts > 0:
                keep &= contacts >= selection.min_contacts
        if selection.needs_normals:
            if scene_normals is None:
                from .pointcloud import estimate_normals
                src = scene[:1] if shared else scene
                normals = estimate_normals(src, max_radius=selection.normals_radius, k=selection.normals_k)[0]
            else:
                normals = (scene_normals.unsqueeze(0) if scene_normals.ndim == 2 else scene_normals).to(self.device)
            if normals.shape[0] == 1 and b > 1:
                normals = normals.expand(b, -1, -1)
            _, aligned = gs.contact_normals(scene, normals, H, friction_angle_deg=selection.friction_angle_deg)
            if selection.both_fingers:
                keep &= (aligned >= selection.min_aligned_contacts).all(dim=-1)
            else:
                keep &= aligned.sum(dim=-1) >= selection.min_aligned_contacts
        success = results.get("success")
        success = None if success is None else success.to(self.device).reshape(b, g)

        def score(Hsel):   # [B, n, 4, 4] -> [B, n]
            if self.classifier is None:
                raise RuntimeError("the selection needs success probabilities (min_success / score_by) but no classifier is "
                                   "attached: call set_classifier(model) first")
            if pc is None or metas is None:
                raise RuntimeError("scoring needs the normalised cloud and its metas: pass pc= and metas= (generate_grasps("
                                   "..., selection=) does)")
            return self.score_grasps(pc, metas, Hsel)

        def pad_gather(index, count, n):   # poses at index[:, :n], the slots behind count filled with the cloud's first one
            idx = index[:, :n].long()
            first = idx[:, :1].clamp(min=0)
            valid = torch.arange(n, device=self.device)[None, :] < count[:, None]
            idx = torch.where(valid, idx, first.expand(-1, n))
            return H.gather(1, idx.view(b, n, 1, 1).expand(-1, -1, 4, 4)), idx, valid

        if selection.needs_success and success is None:
            # compact the survivors (top-k mode: kept candidates in front), score them, scatter back; the rest stay NaN
            index, count, _ = gs.select_grasps(H, conf, keep=keep, k=g)
            success = torch.full((b, g), float("nan"), device=self.device)
            n = int(count.max())
            if n > 0:
                Hs, idx, valid = pad_gather(index, count, n)
                s = score(Hs).reshape(b, n)
                rows = torch.arange(b, device=self.device)[:, None].expand(-1, n)
                success[rows[valid], idx[valid]] = s[valid]
        if selection.min_success is not None:
            keep &= success >= selection.min_success   # NaN (unscored) compares false
        by = {"confidence": conf, "success": success, "product": None if success is None else conf * success}[selection.score_by]
        by = torch.where(keep, by, torch.zeros_like(conf))   # dropped poses may carry NaN
        k = g if selection.top_k is None else min(selection.top_k, g)
        index, count, gap = gs.select_grasps(H, by, keep=keep, k=k, diverse=selection.diverse,
                                             min_separation=selection.min_separation)
        valid = torch.arange(k, device=self.device)[None, :] < count[:, None]
        idx = index.long().clamp(min=0)
        out = dict(results)
        per_pose = {key: out[key] for key in ("grasps", "grasp_tmrp", "confidence", "latent_mu", "latent_logvar")
                    if out.get(key) is not None}
        if success is not None:
            per_pose["success"] = success.unsqueeze(-1)
        for key, t in per_pose.items():
            t = t.to(self.device)
            tail = t.shape[2:]
            ix = idx.view(b, k, *([1] * len(tail))).expand(-1, -1, *tail)
            vm = valid.view(b, k, *([1] * len(tail)))
            out[key] = torch.where(vm, t.gather(1, ix), torch.full((), float("nan"), dtype=t.dtype, device=self.device))
        if success is None and self.classifier is not None:   # the classifier has not run: the k selected poses only
            n = int(count.max())
            sel = torch.full((b, k), float("nan"), device=self.device)
            if n > 0:
                Hs, _, v = pad_gather(index, count, n)
                sel[:, :n] = torch.where(v, score(Hs).reshape(b, n), sel[:, :n])
            out["success"] = sel.unsqueeze(-1)
        out.update(selected_index=index, selected_count=count, selected_gap=gap, clearance=clearance, contacts=contacts)
        if aligned is not None:   # the key exists only where the filter was asked for
            out["aligned_contacts"] = aligned
        return out

    def set_classifier(self, model, gripper_points=None):
        """Attach a PointsBasedGraspClassifier: every result dict then carries `success` [B, G, 1], the classifier's
        probability for each returned pose (score_grasps).  gripper_points [Ng, 3]: the points the classifier was trained
        with (default: gripper.control_points(num_pc_points - N) for a cloud of N points).  None detaches it."""
        self.classifier = None if model is None else model.to(self.device).eval()
        self.gripper_points = None if gripper_points is None else gripper_points.to(self.device).float()

    @torch.no_grad()
    def score_grasps(self, pc, metas, H):
        """Success probability [B, G] of poses H [B, G, 4, 4] (or [G, 4, 4] for one cloud; un-normalised cloud frame, as
        generate_grasps returns them) against the normalised cloud(s) pc: the gripper points go through the cloud's own
        normalisation, (x - metas["pc_mean"]) / pc_scale.  metas["pc_mean"] is the total shift (centring mean + pc_shift,
        acronym_grasp_points.py:121), so the instance's pc_shift is already part of it."""
        if self.classifier is None:
            raise RuntimeError("no classifier attached: call set_classifier(model) first")
        batch = (pc.unsqueeze(0) if pc.ndim == 2 else pc).to(self.device)
        H = H.to(self.device)
        if H.ndim == 3:
            H = H.unsqueeze(0)
        if H.ndim != 4 or H.shape[-2:] != (4, 4) or H.shape[0] != batch.shape[0]:
            raise RuntimeError(f"grasps must be [B,G,4,4] with B = {batch.shape[0]} clouds (or [G,4,4] for one), not {tuple(H.shape)}")
        scale = torch.as_tensor((getattr(self, "_norm", None) or {}).get("pc_scale", PC_STD), dtype=torch.float32).reshape(-1)
        if not bool((scale == scale[0]).all()):
            raise NotImplementedError("the classifier front takes one translation scale for the three axes")
        mean = metas["pc_mean"].to(self.device).float().reshape(-1, 3)
        return self.classifier.score_poses(batch, H, gripper_points=self.gripper_points, pc_mean=mean, pc_shift=0.0,
                                           pc_scale=float(scale[0]))

    def set_normalization_params(self, norm_config):
        """grasp_ldm/inference/inference_base.py:103-130: pc_shift, grasp_shift, translation_scale, rotation_scale."""
        get = (lambda k: norm_config[k]) if isinstance(norm_config, dict) else (lambda k: getattr(norm_config, k))
        for k in ("pc_shift", "grasp_shift", "translation_scale", "rotation_scale"):
            try:
                get(k)
            except (KeyError, AttributeError):
                raise AssertionError(f"norm_config should have `{k}`")
        self._norm = dict(pc_shift=get("pc_shift"), grasp_shift=get("grasp_shift"),
                          pc_scale=get("translation_scale"), mrp_scale=get("rotation_scale"))

    def normalize_input(self, pc):
        """tools/inference.py:570-591 / inference_base.py:181-212: centre on the mean, divide by the translation
        scale (0.05 unless set_normalization_params says otherwise), build metas.  One HIP launch."""
        from .pointcloud import normalize_input
        kw = getattr(self, "_norm", None) or dict(pc_shift=0.0, pc_scale=PC_STD, mrp_scale=MRP_STD, grasp_shift=None)
        return normalize_input(pc.to(self.device), **kw)

    def _grasp_encoder(self):
        vae = getattr(self.model, "vae_model", None) or self.model
        return vae.encoder.grasp_encoder

    def normalize_grasps(self, H, metas, label=None):
        """Poses in the cloud's (un-normalised) frame -> the encoder's input rows: H [B,G,4,4] (or [G,4,4] for one cloud)
        -> [B*G, 6|7] = ((t, mrp) - grasp_mean) / grasp_std, with the label column appended when the encoder's in_layer
        takes 7 features.  label defaults to ones: the success flag the dataset appends to good grasps
        (dataset/acronym/acronym.py:224).  One HIP launch (gldm_pose_prologue)."""
        H = H.to(self.device)
        if H.ndim == 3:
            H = H.unsqueeze(0)
        if H.ndim != 4 or H.shape[-2:] != (4, 4):
            raise RuntimeError(f"grasps must be [B,G,4,4] or [G,4,4], not {tuple(H.shape)}")
        b, g = H.shape[:2]
        lab = None
        if self._grasp_encoder().in_features == 7:
            lab = torch.ones(b * g, device=self.device) if label is None else label.to(self.device).reshape(-1).float()
        return pose_prologue(H.reshape(b * g, 4, 4), lab, metas["grasp_mean"].to(self.device),
                             metas["grasp_std"].to(self.device), g)

    def prepare_pointcloud(self, pc, num_points=None, use_farthest_point=True):
        """The front half of infer_on_pointcloud: bring a raw cloud to the encoder's point count, normalise -> (pc, metas)."""
        pc = pc.to(self.device)
        if num_points is not None and pc.shape[-2] != num_points:
            from .pointcloud import PointCloudHelpers
            clouds = pc.unsqueeze(0) if pc.ndim == 2 else pc
            reg = torch.stack([PointCloudHelpers.regularize_pc_point_count(c, num_points, use_farthest_point)
                               for c in clouds])
            pc = reg[0] if pc.ndim == 2 else reg
        return self.normalize_input(pc)

    def infer_on_pointcloud(self, pc, num_grasps=10, return_intermediate=False, num_points=None,
                            use_farthest_point=True, selection=None, scene_pc=None, downsample=None):
        """tools/inference.py:658-666 (= generate_on_pointcloud, grasp_ldm/inference/inference_base.py:161-179).
        `num_points` (additive): first bring every cloud to the encoder's point count
        (PointCloudHelpers.regularize_pc_point_count; farthest-point selection by default).  `selection` / `scene_pc`
        (additive): filter and select the poses (select_grasps); scene_pc is in the frame of `pc`.
        `downsample` (a graspldm_amd.grasp_select.CloudDownsample; additive): the order is downsample ->
        point-count regularisation: ONE pointcloud.voxel_downsample call over all clouds of pc before num_points is
        applied; the results gain voxel_size (the size used), object_points and object_points_raw [B] (points after / before
        it); with downsample.apply_to_scene a given scene_pc is downsampled too.  A cloud left empty raises ValueError."""
        if downsample is not None:
            pc = pc.to(self.device)
            single = pc.ndim == 2
            raw = list(pc.unsqueeze(0) if single else pc)
            clouds, size = self._downsample_clouds(raw, downsample)
            for i, c in enumerate(clouds):
                if c.shape[0] == 0:
                    raise ValueError(f"cloud {i} is empty")
            if selection is not None and scene_pc is not None and downsample.apply_to_scene:
                scene_pc = self._downsample_scene(scene_pc.to(self.device), size)
            extra = {} if selection is None else dict(selection=selection, scene_pc=scene_pc)
            out = self._infer_on_clouds(clouds, single, num_grasps, num_points, use_farthest_point, return_intermediate, extra)
            return self._downsample_keys(out, size, clouds, [c.shape[0] for c in raw])
        pcn, metas = self.prepare_pointcloud(pc, num_points, use_farthest_point)
        if selection is None:
            return self.generate_grasps(pcn, metas, num_grasps=num_grasps, return_intermediate=return_intermediate)
        return self.generate_grasps(pcn, metas, num_grasps=num_grasps, return_intermediate=return_intermediate,
                                    selection=selection, scene_pc=scene_pc)

    generate_on_pointcloud = infer_on_pointcloud

    def infer_on_depth(self, depth, camera, mask=None, num_grasps=10, num_points=None, use_farthest_point=True,
                       z_range=None, depth_scale=None, cam_to_world=None, crop_box=None, selection=None, scene_pc=None,
                       return_intermediate=False, cleanup=None, downsample=None):
        """From a depth frame to grasps without leaving the GPU (additive; the reference stops at
        Camera.depth_to_pointcloud_torch, grasp_ldm/utils/camera.py:176-215, and leaves the rest to the caller).
        depth [H, W] or [F, H, W] (CUDA; float32 metres or raw 16-bit units with depth_scale), camera: a
        graspldm_amd.camera.Camera.  Object cloud of every frame = the deprojection under `mask` / `crop_box` inside
        `z_range` (pointcloud.depth_to_cloud), then prepare_pointcloud (num_points, farthest-point selection by default),
        then generate_grasps: exactly infer_on_pointcloud on that cloud.  When `selection` asks for collision_free,
        min_contacts or min_aligned_contacts and no scene_pc is given, the scene is the same frame without mask and crop,
        inside z_range.
        Poses are in the camera frame, or in the world frame with cam_to_world (3 x 4 / 4 x 4).  A frame whose object
        cloud is empty raises ValueError before anything is generated.  F frames -> results of batch F.
        `cleanup` (a graspldm_amd.grasp_select.CloudCleanup): the object clouds of all frames lose their
        outliers in one pointcloud.remove_outliers call before anything else sees them; the empty-cloud check refers to the
        filtered clouds, the results gain object_points and object_points_raw [F] (points after / before the filter), and
        with cleanup.apply_to_scene the scene cloud taken from the frame is filtered too.
        `downsample` (a graspldm_amd.grasp_select.CloudDownsample): the order is deprojection ->
        downsample -> cleanup (if given) -> point-count regularisation.  The object clouds of all frames go through ONE
        pointcloud.voxel_downsample call first, so cleanup sees uniform density and fewer points; the empty-cloud check and
        object_points refer to the counts after both steps, object_points_raw [F] to the deprojected counts, and the
        results gain voxel_size (the size used).  With downsample.apply_to_scene the scene cloud taken from the frame is
        downsampled (before cleanup.apply_to_scene filters it)."""
        from .pointcloud import depth_to_cloud
        depth = depth.to(self.device) if isinstance(depth, torch.Tensor) else depth
        mask = mask.to(self.device) if isinstance(mask, torch.Tensor) else mask
        kw = dict(z_range=z_range, depth_scale=depth_scale, cam_to_world=cam_to_world)
        clouds = depth_to_cloud(depth, camera, mask=mask, crop_box=crop_box, **kw)
        single = depth.ndim == 2
        clouds = [clouds] if single else clouds
        if downsample is not None:
            raw_counts = [c.shape[0] for c in clouds]
            clouds, voxel_size = self._downsample_clouds(clouds, downsample)
        if cleanup is not None:
            if downsample is None:
                raw_counts = [c.shape[0] for c in clouds]
            clouds = self._clean_clouds(clouds, cleanup)
        for f, c in enumerate(clouds):
            if c.shape[0] == 0:
                raise ValueError(f"frame {f}: the object cloud is empty (no pixel passes the mask, the depth window "
                                 "and the crop box)")
        if selection is not None and scene_pc is None and selection.needs_scene:
            scenes = depth_to_cloud(depth, camera, **kw)
            if downsample is not None and downsample.apply_to_scene:
                scenes = [self._downsample_scene(s, voxel_size) for s in ([scenes] if single else scenes)]
                scenes = scenes[0] if single else scenes
            if cleanup is not None and cleanup.apply_to_scene:
                scenes = self._clean_clouds([scenes] if single else scenes, cleanup)
                scenes = scenes[0] if single else scenes
            if single:
                scene_pc = scenes
            elif len({s.shape[0] for s in scenes}) == 1:
                scene_pc = torch.stack(scenes)
            else:
                raise ValueError("the frames' scene clouds differ in size and cannot form one batch: pass scene_pc "
                                 "[F, Ns, 3], or call infer_on_depth frame by frame")
        extra = {} if selection is None else dict(selection=selection, scene_pc=scene_pc)
        out = self._infer_on_clouds(clouds, single, num_grasps, num_points, use_farthest_point, return_intermediate, extra)
        if downsample is not None:
            return self._downsample_keys(out, voxel_size, clouds, raw_counts)
        if cleanup is not None:
            out["object_points"] = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64, device=self.device)
            out["object_points_raw"] = torch.tensor(raw_counts, dtype=torch.int64, device=self.device)
        return out

    def _infer_on_clouds(self, clouds, single, num_grasps, num_points, use_farthest_point, return_intermediate, extra):
        """The back half of infer_on_depth: the frames' object clouds -> results of batch F."""
        from .pointcloud import PointCloudHelpers
        if single:
            return self.infer_on_pointcloud(clouds[0], num_grasps=num_grasps, return_intermediate=return_intermediate,
                                            num_points=num_points, use_farthest_point=use_farthest_point, **extra)
        if num_points is None:
            if len({c.shape[0] for c in clouds}) != 1:
                raise ValueError("the frames' object clouds differ in size: pass num_points")
            batch = torch.stack(clouds)
        else:
            batch = torch.stack([c if c.shape[0] == num_points else
                                 PointCloudHelpers.regularize_pc_point_count(c, num_points, use_farthest_point)
                                 for c in clouds])
        pcn, metas = self.normalize_input(batch)
        return self.generate_grasps(pcn, metas, num_grasps=num_grasps, return_intermediate=return_intermediate, **extra)

    def _encoder_points(self):
        """n_points of the model's cloud encoder (its out_layer[1] is a Linear over the point axis: N is fixed)."""
        vae = getattr(self.model, "vae_model", self.model)
        try:
            enc = vae.encoder.pc_encoder if hasattr(vae, "encoder") else vae.pc_encoder
            return int(enc.out_layer[1].in_features)
        except (AttributeError, IndexError, TypeError):
            raise ValueError("cannot infer the encoder's point count: pass num_points") from None

    def infer_on_mesh(self, mesh, num_grasps=10, num_points=None, view=None, camera=None, seed=None, selection=None,
                      scene_points=None, view_radius=None, use_farthest_point=True, return_intermediate=False):
        """From an object model to grasps without leaving the GPU (additive): the two inputs the reference's
        experiments read from ACRONYM meshes -- `mesh.sample(n)` for the full-cloud model (acronym_pointclouds.py:173-176,
        402) and rendered depth frames for the partial-cloud model (acronym_partial_pointclouds.py:521-581).
        mesh: a graspldm_amd.mesh.Mesh (load_mesh reads OBJ / STL / npz).  num_points: default the encoder's point count.
        view=None: pointcloud.sample_mesh_surface draws num_points surface points (seed: the in-kernel generator's; None
        draws one from torch's CPU generator) and the rest is exactly infer_on_pointcloud on them.  When `selection` asks for
        a scene (collision_free, min_contacts, min_aligned_contacts) the scene is a denser sample of the same surface:
        scene_points of them (default 8 num_points), drawn with seed + 1.
        view = a world-to-camera pose [4, 4] or [F, 4, 4] (camera.look_at), or an int F for camera.views_on_sphere(F,
        view_radius, centre of the mesh's bounding box, np.random.default_rng(seed)); view_radius defaults to 4 times the
        bounding sphere's radius.  `camera` (a graspldm_amd.camera.Camera) is then required: pointcloud.render_depth renders
        the frames and the rest is exactly infer_on_depth on them, one result per view, poses in each view's camera frame.
        The results gain mesh_face -- the mesh face under every input point: [1, num_points] int32 without a view; with
        views a list of F tensors, one entry per deprojected point in pixel order -- and cam_pose (the world-to-camera
        poses [F, 4, 4] float64 on the host; None without a view)."""
        from .camera import views_on_sphere
        from .mesh import Mesh
        from .pointcloud import depth_to_cloud, render_depth, sample_mesh_surface
        if not isinstance(mesh, Mesh):
            raise TypeError("infer_on_mesh takes one graspldm_amd.mesh.Mesh (mesh.load_mesh reads OBJ, STL and npz files)")
        if mesh.faces.shape[0] == 0:
            raise ValueError("the mesh has no faces")
        n = self._encoder_points() if num_points is None else int(num_points)
        extra = {} if selection is None else dict(selection=selection)
        if view is None:
            if camera is not None or view_radius is not None:
                raise ValueError("camera and view_radius go with a view")
            seed = int(torch.randint(0, 2 ** 62, ())) if seed is None else int(seed)
            pts, face = sample_mesh_surface(mesh, n, seed=seed, return_faces=True, device=self.device)
            if bool((face < 0).any()):
                raise ValueError("the mesh has no surface area")
            if selection is not None and selection.needs_scene:
                m = 8 * n if scene_points is None else int(scene_points)
                extra["scene_pc"] = sample_mesh_surface(mesh, m, seed=(seed + 1) % 2 ** 64, device=self.device)[0]
            out = self.infer_on_pointcloud(pts[0], num_grasps=num_grasps, return_intermediate=return_intermediate, **extra)
            out["mesh_face"], out["cam_pose"] = face, None
            return out
        if camera is None:
            raise ValueError("a view needs a camera (graspldm_amd.camera.Camera: intrinsics and image size)")
        lo, hi = mesh.bounds
        centre = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
        if isinstance(view, (int, np.integer)) and not isinstance(view, bool):
            if view < 1:
                raise ValueError(f"view = {view}: at least one view")
            radius = 4 * float(np.linalg.norm(mesh.vertices.astype(np.float64) - centre, axis=1).max())
            radius = radius if view_radius is None else float(view_radius)
            poses = views_on_sphere(int(view), radius, centre, np.random.default_rng(seed))
            single = False
        else:
            if view_radius is not None:
                raise ValueError("view_radius goes with a number of views")
            poses = np.asarray(view.detach().cpu() if isinstance(view, torch.Tensor) else view, dtype=np.float64)
            single = poses.ndim == 2
            poses = poses.reshape(-1, 4, 4)
        depth, face = render_depth(mesh, camera, poses, return_faces=True, device=self.device)
        out = self.infer_on_depth(depth[0] if single else depth, camera, num_grasps=num_grasps, num_points=n,
                                  use_farthest_point=use_farthest_point, return_intermediate=return_intermediate, **extra)
        _, pix = depth_to_cloud(depth, camera, return_pixels=True)
        out["mesh_face"] = [face[f].reshape(-1)[p.long()] for f, p in enumerate(pix)]
        out["cam_pose"] = torch.from_numpy(poses.copy())
        return out

    @staticmethod
    def _clean_objects(packed, starts, counts, cleanup):
        """The objects of one frame (rows starts[k] .. + counts[k] of packed) through ONE ragged pointcloud.remove_outliers
        call -> (packed, starts, counts) of the filtered objects."""
        from .grasp_select import CloudCleanup
        from .pointcloud import remove_outliers
        if not isinstance(cleanup, CloudCleanup):
            raise TypeError("cleanup must be a graspldm_amd.grasp_select.CloudCleanup")
        out, ostart, ocount, _, _ = remove_outliers(packed, start=starts, count=counts, **cleanup.options)
        return out, ostart, ocount

    @staticmethod
    def _clean_clouds(clouds, cleanup):
        """A list of clouds [n_i, 3] through ONE pointcloud.remove_outliers call -> the list of the filtered clouds."""
        counts = [c.shape[0] for c in clouds]
        starts = [sum(counts[:i]) for i in range(len(counts))]
        packed = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
        out, ostart, ocount = _InferenceBase._clean_objects(packed, starts, counts, cleanup)
        return [out[s:s + c] for s, c in zip(ostart, ocount)]

    @staticmethod
    def _downsample_objects(packed, starts, counts, downsample):
        """The objects of one frame (rows starts[k] .. + counts[k] of packed) through ONE ragged
        pointcloud.voxel_downsample_capped call -> (packed, starts, counts, voxel size used)."""
        from .grasp_select import CloudDownsample
        from .pointcloud import voxel_downsample_capped
        if not isinstance(downsample, CloudDownsample):
            raise TypeError("downsample must be a graspldm_amd.grasp_select.CloudDownsample")
        (out, ostart, ocount, _, _), size = voxel_downsample_capped(packed, start=starts, count=counts, **downsample.options)
        return out, ostart, ocount, size

    @staticmethod
    def _downsample_clouds(clouds, downsample):
        """A list of clouds [n_i, 3] through ONE pointcloud.voxel_downsample_capped call -> (the list of the downsampled
        clouds, voxel size used)."""
        counts = [c.shape[0] for c in clouds]
        starts = [sum(counts[:i]) for i in range(len(counts))]
        packed = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
        out, ostart, ocount, size = _InferenceBase._downsample_objects(packed, starts, counts, downsample)
        return [out[s:s + c] for s, c in zip(ostart, ocount)], size

    @staticmethod
    def _downsample_scene(scene, voxel_size):
        """A scene cloud [Ns, 3] or [B, Ns, 3] at the voxel size the objects ended with (no ceiling on its points).  A batch
        must keep one size per cloud to stay a batch."""
        from .pointcloud import voxel_downsample
        if scene.ndim == 2:
            return voxel_downsample(scene, voxel_size)[0]
        out, ostart, ocount, _, _ = voxel_downsample(scene, voxel_size)
        if len(set(ocount)) != 1:
            raise ValueError("the downsampled scene clouds differ in size and cannot form one batch: pass one scene "
                             "[Ns, 3], or downsample.apply_to_scene=False")
        return torch.stack([out[s:s + c] for s, c in zip(ostart, ocount)])

    def _downsample_keys(self, out, voxel_size, clouds, raw_counts):
        out["voxel_size"] = voxel_size
        out["object_points"] = torch.tensor([c.shape[0] for c in clouds], dtype=torch.int64, device=self.device)
        out["object_points_raw"] = torch.tensor(raw_counts, dtype=torch.int64, device=self.device)
        return out

    def infer_on_scene(self, depth, camera, labels, num_grasps=10, num_points=None, num_labels=None, min_object_points=32,
                       use_farthest_point=True, mask=None, z_range=None, depth_scale=None, cam_to_world=None, crop_box=None,
                       selection=None, scene_pc=None, cleanup=None, downsample=None):
        """One depth frame [H, W] with an instance-label image -> the grasps of every object, as ONE batch (additive,
        DESIGN.md 4.11).  labels: integer tensor of depth's shape, object k = label k (1 .. num_labels, at most 64; default
        labels.max()); the other arguments as infer_on_depth.  Objects with fewer than min_object_points points are skipped;
        the kept ones (ascending label) go through pointcloud.regularize_objects (num_points; None only if they all have
        the same size), normalize_input and generate_grasps: exactly generate_grasps on the stacked clouds.  When
        `selection` asks for collision_free, min_contacts or min_aligned_contacts and no scene_pc is given, the scene is the
        same frame without labels, mask and crop, inside z_range, as one [1, Ns, 3] cloud for every object.
        Added keys: object_label [B] and object_points [B] (label and raw point count of every row of the batch),
        scene_rank [n, 2] int64: (object row, slot) of every pose that is not NaN, by falling score (selection.score_by;
        confidence without a selection), ties to the lower object, then the lower slot.
        `cleanup` (a graspldm_amd.grasp_select.CloudCleanup): ONE ragged pointcloud.remove_outliers call over
        all objects of the frame, between the deprojection and regularize_objects; min_object_points, the error above and
        object_points then refer to the filtered counts and object_points_raw [B] holds the unfiltered ones; with
        cleanup.apply_to_scene the scene cloud taken from the frame is filtered too.
        `downsample` (a graspldm_amd.grasp_select.CloudDownsample): the order is deprojection ->
        downsample -> cleanup (if given) -> regularize_objects.  ONE ragged pointcloud.voxel_downsample call over all objects
        of the frame comes first, so cleanup sees uniform density and fewer points; min_object_points, the error above and
        object_points refer to the counts after both steps, object_points_raw [B] holds the deprojected ones, and the result
        gains voxel_size (the size used).  With downsample.apply_to_scene the scene cloud taken from the frame is
        downsampled (before cleanup.apply_to_scene filters it)."""
        from .pointcloud import _depth_to_objects_packed, depth_to_cloud, regularize_objects
        depth = depth.to(self.device) if isinstance(depth, torch.Tensor) else depth
        labels = labels.to(self.device) if isinstance(labels, torch.Tensor) else labels
        mask = mask.to(self.device) if isinstance(mask, torch.Tensor) else mask
        if not isinstance(depth, torch.Tensor) or depth.ndim != 2:
            raise ValueError("infer_on_scene takes one frame [H, W]")
        kw = dict(z_range=z_range, depth_scale=depth_scale, cam_to_world=cam_to_world)
        points, _, starts, counts = _depth_to_objects_packed(depth, camera, labels, num_labels=num_labels, mask=mask,
                                                             crop_box=crop_box, **kw)
        packed, starts, counts = points[0], starts[0], counts[0]
        if downsample is not None:
            raw_counts = counts
            packed, starts, counts, voxel_size = self._downsample_objects(packed, starts, counts, downsample)
        if cleanup is not None:
            if downsample is None:
                raw_counts = counts
            packed, starts, counts = self._clean_objects(packed, starts, counts, cleanup)
        kept = [k for k, c in enumerate(counts) if c >= max(int(min_object_points), 1)]
        if not kept:
            raise ValueError(f"no object has at least {min_object_points} points (labels 1 .. {len(counts)} hold "
                             f"{counts} after the mask, the depth window and the crop box)")
        ks, kc = [starts[k] for k in kept], [counts[k] for k in kept]
        if num_points is None:
            if len(set(kc)) != 1:
                raise ValueError("the objects' clouds differ in size: pass num_points")
            batch = torch.stack([packed[s:s + c] for s, c in zip(ks, kc)])
        else:
            batch = regularize_objects(packed, ks, kc, num_points, use_farthest_point)
        if selection is not None and scene_pc is None and selection.needs_scene:
            scene_pc = depth_to_cloud(depth, camera, **kw)
            if downsample is not None and downsample.apply_to_scene:
                scene_pc = self._downsample_scene(scene_pc, voxel_size)
            if cleanup is not None and cleanup.apply_to_scene:
                scene_pc = self._clean_clouds([scene_pc], cleanup)[0]
            scene_pc = scene_pc.unsqueeze(0)
        extra = {} if selection is None else dict(selection=selection, scene_pc=scene_pc)
        pcn, metas = self.normalize_input(batch)
        out = self.generate_grasps(pcn, metas, num_grasps=num_grasps, **extra)
        out["object_label"] = torch.tensor([k + 1 for k in kept], dtype=torch.int64, device=self.device)
        out["object_points"] = torch.tensor(kc, dtype=torch.int64, device=self.device)
        if cleanup is not None or downsample is not None:
            out["object_points_raw"] = torch.tensor([raw_counts[k] for k in kept], dtype=torch.int64, device=self.device)
        if downsample is not None:
            out["voxel_size"] = voxel_size
        out["scene_rank"] = self._scene_rank(out, selection)
        return out

    def infer_on_tabletop(self, depth, camera, num_grasps=10, num_points=None, segmentation=None, min_object_points=32,
                          use_farthest_point=True, mask=None, z_range=None, depth_scale=None, cam_to_world=None,
                          crop_box=None, selection=None, scene_pc=None, cleanup=None, downsample=None):
        """One depth frame [H, W] of objects standing on a table -> the grasps of every object, without a label image
        (additive): pointcloud.segment_tabletop makes the labels on the GPU (a RANSAC table plane, then the
        connected components above it), infer_on_scene does the rest with them.  segmentation: a dict of
        segment_tabletop's own options (plane, height_range, link_dist, min_pixels, max_objects, tol, hypotheses, rng,
        refit, min_cross2); the depth options go to both.  The result of infer_on_scene gains `labels` ([H, W] int32) and
        `table_plane` (pointcloud.TablePlane).  No object found: ValueError.  `cleanup`: as in infer_on_scene (the labels are made
        from the unfiltered frame).  `downsample`: as in infer_on_scene as well (deprojection -> downsample -> cleanup ->
        regularisation; the labels are made from the full frame)."""
        from .pointcloud import segment_tabletop
        depth = depth.to(self.device) if isinstance(depth, torch.Tensor) else depth
        mask = mask.to(self.device) if isinstance(mask, torch.Tensor) else mask
        if not isinstance(depth, torch.Tensor) or depth.ndim != 2:
            raise ValueError("infer_on_tabletop takes one frame [H, W]")
        kw = dict(mask=mask, z_range=z_range, depth_scale=depth_scale, cam_to_world=cam_to_world, crop_box=crop_box)
        labels, num, plane = segment_tabletop(depth, camera, **dict(segmentation or {}), **kw)
        if num < 1:
            raise ValueError("no object found on the table (no component of enough pixels inside the height range)")
        out = self.infer_on_scene(depth, camera, labels, num_grasps=num_grasps, num_points=num_points, num_labels=num,
                                  min_object_points=min_object_points, use_farthest_point=use_farthest_point,
                                  selection=selection, scene_pc=scene_pc, **kw, **({} if cleanup is None else
                                                                                   dict(cleanup=cleanup)),
                                  **({} if downsample is None else dict(downsample=downsample)))
        out["labels"] = labels
        out["table_plane"] = plane
        return out

    def infer_on_cloud_scene(self, pc, num_grasps=10, num_points=None, segmentation=None, min_object_points=32,
                             use_farthest_point=True, selection=None, scene_pc=None, cleanup=None, downsample=None,
                             view_point=None):
        """One unorganised scene cloud [N, 3] -- several cameras fused, a downsampled or filtered cloud, a file -- -> the
        grasps of every object in it, as ONE batch (additive): infer_on_tabletop without a pixel grid.
        The order of the steps:
          1. `downsample` (a graspldm_amd.grasp_select.CloudDownsample): pointcloud.voxel_downsample_capped of the WHOLE
             cloud first, because the clustering costs (points within link_dist) per point;
          2. pointcloud.segment_cloud (segmentation: a dict of its own options -- plane, table, height_range, link_dist,
             min_points, max_objects, tol, hypotheses, rng, refit, min_cross2; view_point goes to it too): a RANSAC table
             plane, then the Euclidean clusters above it;
          3. pointcloud.split_labels: the objects packed in label order;
          4. `cleanup` (a graspldm_amd.grasp_select.CloudCleanup): ONE ragged pointcloud.remove_outliers call over them;
          5. pointcloud.regularize_objects (num_points; None only if they all have the same size);
          6. normalize_input;  7. generate_grasps on every object at once, exactly as infer_on_scene ends.
        A voxel size (the one actually used) above link_dist raises ValueError: nothing would link.  When `selection` needs
        a scene and no scene_pc is given, the scene is the input cloud as [1, Ns, 3], downsampled under
        downsample.apply_to_scene and then filtered under cleanup.apply_to_scene.
        Added keys: object_label, object_points, scene_rank (as infer_on_scene), object_points_raw (the counts before
        cleanup, when it ran), labels [n] int32 and segmented_points [n, 3] (the cloud the labels refer to: the input, or its
        downsampled copy), table_plane (a pointcloud.TablePlane, None with table=False), voxel_size (when downsampled).
        No object, or none with min_object_points points: ValueError with the counts."""
        from .pointcloud import _link_dist_f32, regularize_objects, segment_cloud, split_labels, voxel_downsample_capped
        if not isinstance(pc, torch.Tensor) or pc.ndim != 2 or pc.shape[1] != 3:
            raise ValueError("infer_on_cloud_scene takes one cloud [N, 3]")
        pc = pc.to(self.device).contiguous().float()
        seg = dict(segmentation or {})
        if view_point is not None:
            if "view_point" in seg:
                raise ValueError("view_point was given twice: as an argument and inside segmentation")
            seg["view_point"] = view_point
        link = _link_dist_f32(seg.get("link_dist", 0.01))
        cloud, voxel_size = pc, None
        if downsample is not None:
            from .grasp_select import CloudDownsample
            if not isinstance(downsample, CloudDownsample):
                raise TypeError("downsample must be a graspldm_amd.grasp_select.CloudDownsample")
            res, voxel_size = voxel_downsample_capped(pc, **downsample.options)
            cloud = res[0]
            if voxel_size > link:
                raise ValueError(f"the voxel size used, {voxel_size!r}, exceeds link_dist = {link!r}: neighbouring voxels "
                                 "would not be linked and every point would be its own cluster")
        labels, num, plane = segment_cloud(cloud, **seg)
        if num < 1:
            raise ValueError(f"no object found in the cloud: no cluster of at least {seg.get('min_points', 32)} points among "
                             f"the {cloud.shape[0]} points (link_dist = {link!r})")
        packed, starts, counts, _ = split_labels(cloud, labels, max_objects=seg.get("max_objects", 64))
        starts, counts = starts[:num], counts[:num]
        if cleanup is not None:
            raw_counts = counts
            packed, starts, counts = self._clean_objects(packed, starts, counts, cleanup)
        kept = [k for k, c in enumerate(counts) if c >= max(int(min_object_points), 1)]
        if not kept:
            raise ValueError(f"no object has at least {min_object_points} points (labels 1 .. {len(counts)} hold {counts})")
        ks, kc = [starts[k] for k in kept], [counts[k] for k in kept]
        if num_points is None:
            if len(set(kc)) != 1:
                raise ValueError("the objects' clouds differ in size: pass num_points")
            batch = torch.stack([packed[s:s + c] for s, c in zip(ks, kc)])
        else:
            batch = regularize_objects(packed, ks, kc, num_points, use_farthest_point)
        if selection is not None and scene_pc is None and selection.needs_scene:
            scene_pc = pc
            if downsample is not None and downsample.apply_to_scene:
                scene_pc = self._downsample_scene(scene_pc, voxel_size)
            if cleanup is not None and cleanup.apply_to_scene:
                scene_pc = self._clean_clouds([scene_pc], cleanup)[0]
            scene_pc = scene_pc.unsqueeze(0)
        extra = {} if selection is None else dict(selection=selection, scene_pc=scene_pc)
        pcn, metas = self.normalize_input(batch)
        out = self.generate_grasps(pcn, metas, num_grasps=num_grasps, **extra)
        out["object_label"] = torch.tensor([k + 1 for k in kept], dtype=torch.int64, device=self.device)
        out["object_points"] = torch.tensor(kc, dtype=torch.int64, device=self.device)
        if cleanup is not None:
            out["object_points_raw"] = torch.tensor([raw_counts[k] for k in kept], dtype=torch.int64, device=self.device)
        if downsample is not None:
            out["voxel_size"] = voxel_size
        out["labels"] = labels
        out["segmented_points"] = cloud
        out["table_plane"] = plane
        out["scene_rank"] = self._scene_rank(out, selection)
        return out

    @staticmethod
    def _scene_rank(out, selection):
        """(object row, slot) [n, 2] of the poses of a result dict that are not NaN, by falling score; ties keep the
        row-major order."""
        H = out["grasps"]
        b, g = H.shape[:2]
        conf = out["confidence"].reshape(b, g)
        by = "confidence" if selection is None else selection.score_by
        if by != "confidence":
            success = out["success"].reshape(b, g)
            score = success if by == "success" else conf * success
        else:
            score = conf
        valid = ~torch.isnan(H.reshape(b, g, 16)).any(dim=2)
        flat = torch.nonzero(valid.reshape(-1)).reshape(-1)
        s = torch.nan_to_num(score.reshape(-1)[flat], nan=float("-inf"))
        order = flat[torch.sort(s, descending=True, stable=True).indices]
        return torch.stack([order // g, order % g], dim=1)

    def generate_class_conditioned_grasps(self, pc, num_grasps=10, metas=None, data_idx=None, class_label=0, **kwargs):
        """tools/inference.py:330-364: the label, repeated per grasp, travels in metas["mode_cls"] to the
        class-conditioned denoiser (ClassTimeConditionedResNet1D).  One cloud, like the reference."""
        metas = dict(metas)
        metas["mode_cls"] = torch.LongTensor([class_label]).unsqueeze(0).repeat((num_grasps, 1)).to(
            self.device, dtype=torch.float32)
        return self.generate_grasps(pc, metas=metas, num_grasps=num_grasps, **kwargs)

    def infer(self, data_idx=None, num_grasps=10, visualize=False, condition_type=Conditioning.UNCONDITIONAL,
              conditioning=None, **kwargs):
        if self.dataset is None:
            raise RuntimeError("no dataset attached: ACRONYM loading is out of scope; call generate_grasps(pc, metas) "
                               "with a dataset-contract item (graspldm_amd.synthetic.normalize_cloud)")
        if condition_type == Conditioning.REGION_CONDITIONED:
            raise NotImplementedError("region conditioned denoisers are not shipped (out of scope)")
        item = self.dataset[data_idx if data_idx is not None else 0]
        if condition_type == Conditioning.CLASS_CONDITIONED:
            res = self.generate_class_conditioned_grasps(item["pc"], num_grasps=num_grasps, metas=item["metas"],
                                                         class_label=conditioning, **kwargs)
        else:
            res = self.generate_grasps(item["pc"], item["metas"], num_grasps=num_grasps, **kwargs)
        res["inputs"] = dict(item)
        return res


class InferenceLDM(_InferenceBase):
    def __init__(self, exp_name=None, exp_out_root=None, data_root=None, data_split="test", use_ema_model=True,
                 ddm_ckpt_path=None, vae_ckpt_path=None, elucidated_ckpt_path=None, use_elucidated=False,
                 use_fast_sampler=True, num_inference_steps=None, augment_pc=False, load_dataset=False,
                 device="cuda:0", model=None):
        super().__init__(device)
        self.use_ema_model = use_ema_model
        self.ddm_mode = "ddm" if not use_elucidated else "elucidated_ddm"
        # _setup_ldm_sampler, tools/inference.py:463-490
        if use_fast_sampler:
            self.fast_sampler = "DDIM" if not use_elucidated else "DPMPP"
            default_steps = 100 if not use_elucidated else 32
            self.num_inference_steps = default_steps if num_inference_steps is None else num_inference_steps
        else:
            # elucidated + no fast sampler: ElucidatedDiffusion.sample(use_dpmpp=False) = the stochastic Heun sampler
            # (elucidated_diffusion.py:177-257), one network launch per evaluation
            self.fast_sampler, self.num_inference_steps = ("HEUN" if use_elucidated else None), num_inference_steps
        if model is not None:
            self.model = model.to(self.device).eval()
        else:
            from .checkpoint import load_ldm_from_experiment
            m, self.config, self.experiment = load_ldm_from_experiment(
                exp_name, exp_out_root, use_ema_model, ddm_ckpt_path if not use_elucidated else elucidated_ckpt_path,
                use_fast_sampler and not use_elucidated, mode=self.ddm_mode)
            self.model = m.to(self.device).eval()
        if load_dataset:
            warnings.warn("ACRONYM dataset loading is out of scope; use generate_grasps(pc, metas)")

    @torch.no_grad()
    def generate_grasps(self, pc, metas, num_grasps=10, return_intermediate=False, x_T=None, selection=None, scene_pc=None,
                        **kwargs):
        batch = (pc.unsqueeze(0) if pc.ndim == 2 else pc).to(self.device)
        extra_sampler = {}
        if self.fast_sampler == "DPMPP":  # tools/inference.py:607-609
            extra_sampler = dict(use_dpmpp=True, num_sample_steps=self.num_inference_steps)
            if "noise" in kwargs:
                extra_sampler["noise"] = kwargs["noise"]
        elif self.fast_sampler == "HEUN":
            extra_sampler = dict(use_dpmpp=False)
            if self.num_inference_steps is not None:
                extra_sampler["num_sample_steps"] = self.num_inference_steps
            extra_sampler.update({k: kwargs[k] for k in ("noise",) if k in kwargs})
        elif self.num_inference_steps is not None:
            self.model.set_inference_timesteps(self.num_inference_steps)
        if return_intermediate and batch.shape[0] > 1:  # the reference raises after sampling; fail before the work
            raise NotImplementedError("Batched grasps for all diffusion steps are not implemented")
        # noise_source="kernel" (+ noise_seed / noise_base): DDPM step noise drawn inside the fused launch (diffusion.py)
        extra = {k: kwargs[k] for k in ("step_noise", "cls_cond", "noise_source", "noise_seed", "noise_base") if k in kwargs}
        extra.update(extra_sampler)
        denoiser = getattr(self.model.diffusion_model, "model", None) or getattr(self.model.diffusion_model, "net")
        if hasattr(denoiser, "class_embedding"):
            extra["metas"] = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in metas.items()}
        (tmrp, logit), steps = self.model.generate_grasps(batch, num_grasps=num_grasps,
                                                          return_intermediate=return_intermediate, x_T=x_T, **extra)
        out = self._results(batch, metas, tmrp, logit, batch.shape[0], num_grasps, all_steps=steps, score=selection is None)
        return self._finish(out, batch, metas, selection, scene_pc)

    @torch.no_grad()
    def refine_grasps(self, pc, metas, H, strength=0.3, noise=None, selection=None, scene_pc=None, **kwargs):
        """Reverse diffusion started from given grasps H [B,G,4,4] (cloud frame, un-normalised) instead of from noise
        (GraspLatentDDM.refine_grasps).  Same result dict as generate_grasps, plus latent_mu / latent_logvar [B,G,L]."""
        batch = (pc.unsqueeze(0) if pc.ndim == 2 else pc).to(self.device)
        if self.fast_sampler in ("DPMPP", "HEUN"):
            raise NotImplementedError("refine_grasps runs the DDIM / DDPM samplers only")
        if self.num_inference_steps is not None:
            self.model.set_inference_timesteps(self.num_inference_steps)
        h = self.normalize_grasps(H, metas, label=kwargs.pop("label", None))
        g = h.shape[0] // batch.shape[0]
        extra = {k: kwargs[k] for k in ("step_noise", "cls_cond", "noise_source", "noise_seed", "noise_base") if k in kwargs}
        if hasattr(self.model.diffusion_model.model, "class_embedding"):
            extra["metas"] = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in metas.items()}
        (tmrp, logit), lat = self.model._refine(batch, h, strength, noise=noise, **extra)
        out = self._results(batch, metas, tmrp, logit, batch.shape[0], g, score=selection is None)
        out["latent_mu"], out["latent_logvar"] = lat["mu"].view(batch.shape[0], g, -1), lat["logvar"].view(batch.shape[0], g, -1)
        return self._finish(out, batch, metas, selection, scene_pc)


class InferenceVAE(_InferenceBase):
    def __init__(self, exp_name=None, exp_out_root=None, use_ema_model=True, data_root=None, data_split="test",
                 ddm_ckpt_path=None, vae_ckpt_path=None, augment_pc=False, load_dataset=False, device="cuda:0",
                 model=None):
        super().__init__(device)
        self.use_ema_model = use_ema_model
        if model is not None:
            self.model = model.to(self.device).eval()
        else:
            from .checkpoint import load_vae_from_experiment
            m, self.config, self.experiment = load_vae_from_experiment(exp_name, exp_out_root, use_ema_model,
                                                                        vae_ckpt_path)
            self.model = m.to(self.device).eval()

    @torch.no_grad()
    def generate_grasps(self, pc, metas, num_grasps=10, z_h=None, selection=None, scene_pc=None, **kwargs):
        batch = (pc.unsqueeze(0) if pc.ndim == 2 else pc).to(self.device)
        tmrp, logit = self.model.generate_grasps(batch, num_grasps, z_h=z_h)
        out = self._results(batch, metas, tmrp, logit, batch.shape[0], num_grasps, score=selection is None)
        out.pop("all_steps_grasps")
        return self._finish(out, batch, metas, selection, scene_pc)

    @torch.no_grad()
    def reconstruct_grasps(self, pc, metas, H, eps=None, selection=None, scene_pc=None, **kwargs):
        """Given grasps H [B,G,4,4] (cloud frame, un-normalised) through the VAE: normalise -> encode -> decode
        (GraspCVAE.forward(compute_loss=False)).  eps [B*G, L]: the normals of the reparameterisation; None decodes the
        mean (z = mu).  Same result dict as generate_grasps, plus latent_mu / latent_logvar [B,G,L]."""
        batch = (pc.unsqueeze(0) if pc.ndim == 2 else pc).to(self.device)
        h = self.normalize_grasps(H, metas, label=kwargs.pop("label", None))
        vae = getattr(self.model, "vae_model", None) or self.model
        mu, logvar, z, z_pc, g = vae._encode(batch, h, eps=None if eps is None else eps.to(self.device))
        tmrp, logit = vae.decoder(z, z_pc, samples_per_cond=g)
        out = self._results(batch, metas, tmrp, logit, batch.shape[0], g, score=selection is None)
        out.pop("all_steps_grasps")
        out["latent_mu"], out["latent_logvar"] = mu.view(batch.shape[0], g, -1), logvar.view(batch.shape[0], g, -1)
        return self._finish(out, batch, metas, selection, scene_pc)
