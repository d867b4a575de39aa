#!/usr/bin/env python3
"""Grasp generation CLI: same flags as the reference's `tools/generate_grasps.py:14-61`
(--exp_path --data_root --mode --split --num_grasps --visualize --no_ema --num_samples
--conditioning --condition_value --inference_steps) on the MI355X path.

Additive flags: --pc_file FILE [--num_points N] (generate on a sensor cloud read from .npy / .npz / .ply / .xyz:
the reference's `generate_on_pointcloud`, grasp_ldm/inference/inference_base.py:161-212, which its own CLI does not
reach -- it only iterates ACRONYM items, tools/generate_grasps.py:109-131), --device, --seed, --synthetic N (run on N-point synthetic object clouds with
the synthetic weight recipe when no experiment directory / ACRONYM data is available; there is
no network here for either), --out FILE.npz, --classifier_config FILE [--classifier_ckpt FILE] [--sort_by_success] (score every
generated grasp with a PointsBasedGraspClassifier: the results and the written file gain `success`), --refine_from FILE [--refine_strength S] (start from given grasps instead of
from noise: with --mode VAE the file's grasps are reconstructed through the VAE, with --mode LDM they are encoded, diffused
forward to `S` of the schedule and denoised again; FILE is .npy / .npz key `grasps`, [G,4,4] or [B,G,4,4] -- one set per
sample / cloud file in order --, un-normalised, in the cloud's frame; --num_grasps is taken from the file then),
--collision_free / --min_contacts N [--scene_file FILE] / --min_confidence X / --min_success X / --top_k K / --diverse
[--min_separation M] (geometric filtering and selection of the generated poses, graspldm_amd/grasp_select.py: the gripper
must clear the scene, N scene points must lie between the fingers, thresholds on confidence and on the classifier's
success, the best K or K diverse ones; --out gains selected_index, selected_count, selected_gap, clearance, contacts;
without any of these flags nothing changes), --min_aligned_contacts N [--friction_angle DEG] [--both_fingers] [--normals_k K]
[--normals_radius R] (friction-cone contact filter: at least N contacts between the fingers whose surface normal lies within
DEG of the closing axis, with --both_fingers on each finger's side; the scene's normals are estimated on the GPU from K
neighbours within R metres; --out gains aligned_contacts), --depth_file FILE --camera_json FILE [--mask_file FILE] [--depth_scale S]
[--z_range MIN MAX] [--crop_box x0 y0 z0 x1 y1 z1] (generate on a depth frame: deprojected on the GPU, the masked / cropped
pixels are the object, and for --collision_free / --min_contacts / --min_aligned_contacts without --scene_file the whole
frame is the scene;
exclusive with --pc_file and --synthetic), --labels_file FILE [--min_object_points N] (with --depth_file: an instance-label
image, object k = label k; every object with at least N points gets its grasps in one batch, infer_on_scene; --out gains
object_label, object_points, scene_rank), --segment_tabletop [--table_tol T] [--object_height MIN MAX] [--link_dist D]
[--min_object_pixels N] [--ransac_hypotheses T] [--segment_seed S] (with --depth_file, instead of --labels_file: the labels
are made on the GPU from the frame itself -- a RANSAC table plane, then the connected components above it,
infer_on_tabletop; --out gains labels, table_plane and the --labels_file keys), --remove_outliers [--outlier_k K]
[--outlier_radius R] [--outlier_min_neighbors N] [--outlier_std_ratio S] [--clean_scene] (with --depth_file: every object
cloud loses its isolated points on the GPU before the farthest-point selection, pointcloud.remove_outliers; --out gains
object_points_raw), --voxel_size V [--voxel_max_points N] [--downsample_scene] (with --depth_file, or with --pc_file
--num_points: every cloud is downsampled on a voxel grid of V metres on the GPU first, one centroid per occupied voxel,
pointcloud.voxel_downsample; the order is deprojection -> downsample -> --remove_outliers -> point-count regularisation;
with N the size grows by 1.25 until no cloud keeps more than N points; --out gains voxel_size, object_points,
object_points_raw), --segment_cloud [--min_cluster_points N] [--no_table_plane] (with exactly one --pc_file and
--num_points: the file is a whole scene without a pixel grid -- several cameras fused, a downsampled cloud --; the table plane
is fitted and the points above it are split into objects by Euclidean clustering on the GPU, infer_on_cloud_scene; --table_tol,
--object_height, --link_dist, --ransac_hypotheses, --segment_seed, --min_object_points, --voxel_size and --remove_outliers
with their families keep their meaning; --no_table_plane clusters every point; --out gains labels, segmented_points,
table_plane and the --labels_file keys), --mesh_file FILE [--mesh_scale S] [--mesh_views N | --mesh_view EX EY EZ]
[--view_radius R] [--camera_json FILE] [--mesh_seed S] (generate on an object model read from .obj / .stl / .npz,
infer_on_mesh: its surface sampled on the GPU into the encoder's point count, or -- with a view, which needs --camera_json --
depth frames of it rendered on the GPU and deprojected, one result per view; excludes --pc_file and --depth_file; --out gains
mesh_face without a view and cam_pose with one).  `--inference_steps` is honoured (the reference
silently ignores it: it passes use_fast_sampler=False, tools/generate_grasps.py:69-79).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graspldm_amd.inference import Conditioning, InferenceLDM, InferenceVAE  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Grasp Generation Script (MI355X)")
    p.add_argument("--exp_path", type=str, default=None, help="Path to experiment checkpoint")
    p.add_argument("--data_root", type=str, default="data/ACRONYM", help="Root directory for data")
    p.add_argument("--mode", type=str, choices=["VAE", "LDM"], default="VAE", help="Model type to use")
    p.add_argument("--split", type=str, default="test", help="Data split to use")
    p.add_argument("--num_grasps", type=int, default=20, help="Number of grasps to generate")
    p.add_argument("--visualize", action="store_true", help="Enable visualization")
    p.add_argument("--no_ema", action="store_false", dest="use_ema_model", help="Disable EMA model usage")
    p.add_argument("--num_samples", type=int, default=11, help="Number of samples to generate")
    p.add_argument("--conditioning", type=str, choices=["unconditional", "class", "region"], default="unconditional")
    p.add_argument("--condition_value", type=int, help="Value for conditioning (class label or region ID)")
    p.add_argument("--inference_steps", type=int, default=100, help="Number of inference steps for LDM")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--synthetic", type=int, default=0, metavar="N",
                   help="use N-point synthetic clouds and synthetic weights (no experiment dir needed)")
    p.add_argument("--pc_file", type=str, action="append", default=None, metavar="FILE",
                   help="generate on this raw cloud ([N,3], metres; .npy .npz .ply .xyz); may be repeated. The cloud is "
                        "brought to the encoder's point count and normalised like generate_on_pointcloud does")
    p.add_argument("--num_points", type=int, default=None,
                   help="encoder point count for --pc_file (default: the model's pc encoder n_points)")
    p.add_argument("--random_resample", action="store_true",
                   help="with --pc_file: random subsampling instead of farthest-point selection")
    p.add_argument("--refine_from", type=str, default=None, metavar="FILE",
                   help="grasps to start from ([G,4,4] or [B,G,4,4], .npy or .npz key `grasps`; cloud frame, un-normalised): "
                        "reconstructed (--mode VAE) or refined by partial reverse diffusion (--mode LDM)")
    p.add_argument("--refine_strength", type=float, default=0.3,
                   help="with --refine_from and --mode LDM: the share of the schedule to diffuse forward and denoise again "
                        "(0 = decode the encoder's mean, 1 = the whole schedule)")
    p.add_argument("--classifier_config", type=str, default=None, metavar="FILE",
                   help="reference-style config whose `model` is a PointsBasedGraspClassifier: every generated grasp is "
                        "scored against its cloud and the results gain `success`")
    p.add_argument("--classifier_ckpt", type=str, default=None, metavar="FILE",
                   help="the classifier's checkpoint (optional with --synthetic: the synthetic weight recipe is used)")
    p.add_argument("--sort_by_success", action="store_true",
                   help="with --classifier_config: order each cloud's grasps by falling success probability in --out")
    p.add_argument("--scene_file", type=str, action="append", default=None, metavar="FILE",
                   help="the whole scene (table, clutter) for --collision_free / --min_contacts / --min_aligned_contacts, read "
                        "like --pc_file and in the frame of the --pc_file cloud: one file, or one per cloud (default: the "
                        "cloud itself)")
    p.add_argument("--collision_free", action="store_true",
                   help="keep only poses whose open gripper stays clear of every scene point")
    p.add_argument("--min_contacts", type=int, default=0, metavar="N",
                   help="keep only poses with at least N scene points between the fingers")
    p.add_argument("--min_aligned_contacts", type=int, default=0, metavar="N",
                   help="keep only poses with at least N contacts whose surface normal lies inside the friction cone around "
                        "the closing axis (the scene's normals are estimated on the GPU)")
    p.add_argument("--friction_angle", type=float, default=30.0, metavar="DEG",
                   help="with --min_aligned_contacts: half-angle of the friction cone in degrees, in (0, 90]")
    p.add_argument("--both_fingers", action="store_true",
                   help="with --min_aligned_contacts: require the N aligned contacts on each finger's side, not in total")
    p.add_argument("--normals_k", type=int, default=12, metavar="K",
                   help="with --min_aligned_contacts: neighbours per scene point for the normal estimate (3 .. 16)")
    p.add_argument("--normals_radius", type=float, default=0.05, metavar="R",
                   help="with --min_aligned_contacts: search radius of those neighbours in metres")
    p.add_argument("--min_confidence", type=float, default=None, metavar="X", help="keep only poses with confidence >= X")
    p.add_argument("--min_success", type=float, default=None, metavar="X",
                   help="with --classifier_config: keep only poses with success probability >= X (only the poses that "
                        "pass the cheaper filters are scored)")
    p.add_argument("--top_k", type=int, default=None, metavar="K", help="return the best K surviving poses of each cloud")
    p.add_argument("--diverse", action="store_true",
                   help="with --top_k: K poses spread over the survivors (greedy farthest pose) instead of the K best")
    p.add_argument("--min_separation", type=float, default=0.0, metavar="M",
                   help="with --diverse: stop once no survivor is at least M metres (RMS control-point distance) from every pick")
    p.add_argument("--depth_file", type=str, default=None, metavar="FILE",
                   help="generate on a depth frame ([H,W]; .npy / .npz float metres or uint16 raw units, 16-bit .png where "
                        "PIL is installed): deprojected on the GPU with --camera_json, then as --pc_file")
    p.add_argument("--camera_json", type=str, default=None, metavar="FILE",
                   help="camera model of --depth_file (keys cameraMatrix, width, height, ...)")
    p.add_argument("--mask_file", type=str, default=None, metavar="FILE",
                   help="with --depth_file: object mask [H,W] (.npy / .npz key mask or arr_0), nonzero = object pixel")
    p.add_argument("--labels_file", type=str, default=None, metavar="FILE",
                   help="with --depth_file: instance labels [H,W] (integer; .npy / .npz key labels or arr_0), object k = "
                        "label k >= 1: grasps for every object of the frame in one batch")
    p.add_argument("--min_object_points", type=int, default=None, metavar="N",
                   help="with --labels_file: skip objects with fewer than N points (default 32)")
    p.add_argument("--segment_tabletop", action="store_true",
                   help="with --depth_file: find the table plane and the objects standing on it on the GPU and generate "
                        "grasps for every object (excludes --labels_file)")
    p.add_argument("--table_tol", type=float, default=None, metavar="T",
                   help="with --segment_tabletop: inlier distance of the table plane fit, metres (default 0.005)")
    p.add_argument("--object_height", type=float, nargs=2, default=None, metavar=("MIN", "MAX"),
                   help="with --segment_tabletop: object pixels lie MIN < height <= MAX metres over the table (default 0.01 0.5)")
    p.add_argument("--link_dist", type=float, default=None, metavar="D",
                   help="with --segment_tabletop: neighbouring pixels at most D metres apart belong together (default 0.01)")
    p.add_argument("--min_object_pixels", type=int, default=None, metavar="N",
                   help="with --segment_tabletop: drop components of fewer than N pixels (default 32)")
    p.add_argument("--ransac_hypotheses", type=int, default=None, metavar="T",
                   help="with --segment_tabletop: plane hypotheses to score, 1 .. 4096 (default 512)")
    p.add_argument("--segment_seed", type=int, default=None, metavar="S",
                   help="with --segment_tabletop: seed of the hypothesis draws (default 0)")
    p.add_argument("--segment_cloud", action="store_true",
                   help="with one --pc_file and --num_points: the file is a whole scene; find the table plane and split the "
                        "points above it into objects by Euclidean clustering on the GPU, grasps for every object (excludes "
                        "--depth_file)")
    p.add_argument("--min_cluster_points", type=int, default=None, metavar="N",
                   help="with --segment_cloud: drop clusters of fewer than N points (default 32)")
    p.add_argument("--no_table_plane", action="store_true",
                   help="with --segment_cloud: no plane fit and no height window, every point is clustered")
    p.add_argument("--depth_scale", type=float, default=None, metavar="S",
                   help="with --depth_file of raw 16-bit units: metres per unit (e.g. 0.001)")
    p.add_argument("--z_range", type=float, nargs=2, default=None, metavar=("MIN", "MAX"),
                   help="with --depth_file: keep MIN < depth <= MAX metres (default: every finite depth > 0)")
    p.add_argument("--crop_box", type=float, nargs=6, default=None, metavar=("x0", "y0", "z0", "x1", "y1", "z1"),
                   help="with --depth_file: keep object points inside this box (camera frame, metres)")
    p.add_argument("--remove_outliers", action="store_true",
                   help="with --depth_file: drop the isolated points (flying pixels) of every object cloud on the GPU before "
                        "the farthest-point selection")
    p.add_argument("--outlier_k", type=int, default=None, metavar="K",
                   help="with --remove_outliers: neighbours counted per point, 1 .. 16 (default 8)")
    p.add_argument("--outlier_radius", type=float, default=None, metavar="R",
                   help="with --remove_outliers: neighbours lie within R metres (default 0.01)")
    p.add_argument("--outlier_min_neighbors", type=int, default=None, metavar="N",
                   help="with --remove_outliers: keep points with at least N neighbours, 0 .. K (default 3)")
    p.add_argument("--outlier_std_ratio", type=float, default=None, metavar="S",
                   help="with --remove_outliers: also drop points whose mean neighbour distance exceeds the cloud's mean + S "
                        "standard deviations (default: off)")
    p.add_argument("--clean_scene", action="store_true",
                   help="with --remove_outliers: filter the scene cloud the selection is checked against as well")
    p.add_argument("--voxel_size", type=float, default=None, metavar="V",
                   help="with --depth_file, or --pc_file --num_points: downsample every cloud on a voxel grid of V metres on "
                        "the GPU (one centroid per occupied voxel) before --remove_outliers and the point-count regularisation")
    p.add_argument("--voxel_max_points", type=int, default=None, metavar="N",
                   help="with --voxel_size: grow the voxel by 1.25 until no cloud keeps more than N points")
    p.add_argument("--downsample_scene", action="store_true",
                   help="with --voxel_size: downsample the scene cloud the selection is checked against as well")
    p.add_argument("--mesh_file", type=str, default=None, metavar="FILE",
                   help="generate on an object model (.obj, .stl, .npz with vertices and faces): its surface is sampled on the "
                        "GPU into the encoder's point count (--num_points), or with --mesh_views / --mesh_view depth frames "
                        "of it are rendered on the GPU and deprojected, as --depth_file")
    p.add_argument("--mesh_scale", type=float, default=None, metavar="S", help="with --mesh_file: multiply the vertices by S")
    p.add_argument("--mesh_views", type=int, default=None, metavar="N",
                   help="with --mesh_file and --camera_json: render N views from random eyes on a sphere around the object")
    p.add_argument("--mesh_view", type=float, nargs=3, default=None, metavar=("EX", "EY", "EZ"),
                   help="with --mesh_file and --camera_json: render one view from this eye, looking at the object's centre")
    p.add_argument("--view_radius", type=float, default=None, metavar="R",
                   help="with --mesh_views: the sphere's radius in metres (default: 4 times the object's bounding radius)")
    p.add_argument("--mesh_seed", type=int, default=None, metavar="S",
                   help="with --mesh_file: seed of the surface samples / of the random views (default: drawn from --seed)")
    p.add_argument("--out", type=str, default=None, help="write results of all samples to this .npz")
    args = p.parse_args(argv)
    check_mesh_flags(p, args)
    check_cloud_scene_flags(p, args)
    check_depth_flags(args)
    check_downsample_flags(p, args)
    return args


MESH_FLAGS = ("mesh_scale", "mesh_views", "mesh_view", "view_radius", "mesh_seed")


def check_mesh_flags(p, args):
    """--mesh_file excludes --pc_file / --depth_file / --synthetic clouds; a view needs --camera_json; its companions need it."""
    if not args.mesh_file:
        for flag in MESH_FLAGS:
            if getattr(args, flag) is not None:
                p.error(f"--{flag} goes with --mesh_file")
        return
    if args.pc_file or args.depth_file:
        p.error("--mesh_file, --pc_file and --depth_file exclude each other")
    if args.mesh_views is not None and args.mesh_view is not None:
        p.error("--mesh_views and --mesh_view exclude each other")
    view = args.mesh_views is not None or args.mesh_view is not None
    if view and not args.camera_json:
        p.error("--mesh_views / --mesh_view need --camera_json")
    if not view and args.camera_json:
        p.error("--camera_json goes with --mesh_views / --mesh_view (or with --depth_file)")
    if args.view_radius is not None and args.mesh_views is None:
        p.error("--view_radius goes with --mesh_views")
    if args.mesh_views is not None and args.mesh_views < 1:
        p.error("--mesh_views must be at least 1")
    if args.mesh_scale is not None and not args.mesh_scale > 0:
        p.error("--mesh_scale must be positive")
    if args.refine_from or args.segment_cloud or args.voxel_size is not None:
        p.error("--mesh_file generates on the sampled or rendered cloud as it is: it excludes --refine_from, "
                "--segment_cloud and --voxel_size")


def check_downsample_flags(p, args):
    """--voxel_size goes with --depth_file, or with --pc_file --num_points; its companions need it."""
    if args.voxel_size is None:
        for flag in ("voxel_max_points", "downsample_scene"):
            if getattr(args, flag) not in (None, False):
                p.error(f"--{flag} goes with --voxel_size")
        return
    if not (args.depth_file or (args.pc_file and args.num_points is not None)):
        p.error("--voxel_size goes with --depth_file, or with --pc_file --num_points")
    if args.refine_from:
        p.error("--voxel_size does not go with --refine_from")
    try:
        downsample_options(args)
    except SystemExit as e:
        p.error(str(e))


def downsample_options(args):
    """{} without --voxel_size, else the `downsample` argument of the entry points from the --voxel_* flags."""
    if args.voxel_size is None:
        return {}
    from graspldm_amd.grasp_select import CloudDownsample
    try:
        return dict(downsample=CloudDownsample(voxel_size=args.voxel_size, max_points=args.voxel_max_points,
                                               apply_to_scene=bool(args.downsample_scene)))
    except ValueError as e:
        raise SystemExit(f"--voxel_size: {e}")


CLOUD_SCENE_FLAGS = ("min_cluster_points", "no_table_plane")
# the --segment_tabletop flags that --segment_cloud shares (--min_object_pixels counts pixels: it stays with the frame)
CLOUD_SEGMENT_FLAGS = ("table_tol", "object_height", "link_dist", "ransac_hypotheses", "segment_seed")


def check_cloud_scene_flags(p, args):
    """--segment_cloud takes exactly one --pc_file with --num_points and excludes --depth_file; its companions need it."""
    if not args.segment_cloud:
        for flag in CLOUD_SCENE_FLAGS:
            if getattr(args, flag) not in (None, False):
                p.error(f"--{flag} goes with --segment_cloud")
        return
    if args.depth_file:
        p.error("--segment_cloud runs on a --pc_file cloud: it excludes --depth_file (see --segment_tabletop)")
    if not args.pc_file or len(args.pc_file) != 1 or args.num_points is None:
        p.error("--segment_cloud takes exactly one --pc_file, and --num_points")
    if args.synthetic or args.refine_from:
        p.error("--segment_cloud does not go with --synthetic / --refine_from")
    if args.scene_file and len(args.scene_file) != 1:
        p.error("--scene_file: one file for the one --segment_cloud scene")
    if args.min_cluster_points is not None and args.min_cluster_points < 1:
        p.error("--min_cluster_points must be at least 1")
    if args.no_table_plane:
        for flag in ("table_tol", "object_height", "ransac_hypotheses", "segment_seed"):
            if getattr(args, flag) is not None:
                p.error(f"--{flag} fits or uses the table plane: it does not go with --no_table_plane")


def check_depth_flags(args):
    """--depth_file excludes --pc_file / --synthetic and needs --camera_json; its companions need it."""
    if args.depth_file:
        if args.pc_file or args.synthetic:
            raise SystemExit("--depth_file, --pc_file and --synthetic exclude each other")
        if not args.camera_json:
            raise SystemExit("--depth_file needs --camera_json")
        if args.refine_from:
            raise SystemExit("--refine_from runs on --pc_file / --synthetic clouds")
        if args.scene_file and len(args.scene_file) != 1:
            raise SystemExit("--scene_file: one file for the one --depth_file frame")
        if args.segment_tabletop and args.labels_file:
            raise SystemExit("--segment_tabletop makes the labels itself: it excludes --labels_file")
        if args.min_object_points is not None and not (args.labels_file or args.segment_tabletop):
            raise SystemExit("--min_object_points goes with --labels_file")
        for flag in SEGMENT_FLAGS:
            if getattr(args, flag) is not None and not args.segment_tabletop:
                raise SystemExit(f"--{flag} goes with --segment_tabletop")
        for flag in OUTLIER_FLAGS:
            if getattr(args, flag) not in (None, False) and not args.remove_outliers:
                raise SystemExit(f"--{flag} goes with --remove_outliers")
        return
    for flag in ("remove_outliers",) + OUTLIER_FLAGS:
        if getattr(args, flag) not in (None, False) and not args.segment_cloud:
            raise SystemExit(f"--{flag} goes with --depth_file")
    for flag in OUTLIER_FLAGS:
        if getattr(args, flag) not in (None, False) and not args.remove_outliers:
            raise SystemExit(f"--{flag} goes with --remove_outliers")
    if args.segment_tabletop:
        raise SystemExit("--segment_tabletop goes with --depth_file")
    for flag in SEGMENT_FLAGS:
        if getattr(args, flag) is not None and not (args.segment_cloud and flag in CLOUD_SEGMENT_FLAGS):
            raise SystemExit(f"--{flag} goes with --segment_tabletop")
    for flag in ("camera_json", "mask_file", "labels_file", "min_object_points", "depth_scale", "z_range", "crop_box"):
        if getattr(args, flag) is not None and not (args.segment_cloud and flag == "min_object_points") \
                and not (args.mesh_file and flag == "camera_json"):
            raise SystemExit(f"--{flag} goes with --depth_file")


OUTLIER_FLAGS = ("outlier_k", "outlier_radius", "outlier_min_neighbors", "outlier_std_ratio", "clean_scene")
SEGMENT_FLAGS = ("table_tol", "object_height", "link_dist", "min_object_pixels", "ransac_hypotheses", "segment_seed")


def segmentation_options(args):
    """segment_tabletop's options from the --segment_tabletop flags (unset flags keep its defaults)."""
    opts = {}
    if args.table_tol is not None:
        opts["tol"] = args.table_tol
    if args.object_height is not None:
        opts["height_range"] = (args.object_height[0], args.object_height[1])
    if args.link_dist is not None:
        opts["link_dist"] = args.link_dist
    if args.min_object_pixels is not None:
        opts["min_pixels"] = args.min_object_pixels
    if args.ransac_hypotheses is not None:
        opts["hypotheses"] = args.ransac_hypotheses
    if args.segment_seed is not None:
        opts["rng"] = np.random.default_rng(args.segment_seed)
    return opts


def cloud_segmentation_options(args):
    """segment_cloud's options from the --segment_cloud flags (unset flags keep its defaults)."""
    opts = {k: v for k, v in segmentation_options(args).items() if k != "min_pixels"}
    if args.min_cluster_points is not None:
        opts["min_points"] = args.min_cluster_points
    if args.no_table_plane:
        opts["table"] = False
    return opts


def cleanup_options(args):
    """{} without --remove_outliers, else the `cleanup` argument of the depth entry points from the --outlier_* flags (unset
    flags keep CloudCleanup's defaults)."""
    if not args.remove_outliers:
        return {}
    from graspldm_amd.grasp_select import CloudCleanup
    opts = dict(apply_to_scene=bool(args.clean_scene))
    for flag, field in (("outlier_k", "k"), ("outlier_radius", "max_radius"), ("outlier_min_neighbors", "min_neighbors"),
                        ("outlier_std_ratio", "std_ratio")):
        if getattr(args, flag) is not None:
            opts[field] = getattr(args, flag)
    try:
        return dict(cleanup=CloudCleanup(**opts))
    except ValueError as e:
        raise SystemExit(f"--remove_outliers: {e}")


def read_mask_file(path):
    a = np.load(path)
    if hasattr(a, "files"):
        key = next((k for k in ("mask", "arr_0") if k in a.files), None)
        if key is None:
            raise SystemExit(f"{path}: none of the arrays mask / arr_0 found (has {list(a.files)})")
        a = a[key]
    a = np.asarray(a)
    if a.ndim != 2:
        raise SystemExit(f"{path}: the mask must be [H, W], found {a.shape}")
    return torch.from_numpy(np.ascontiguousarray((a != 0).astype(np.uint8)))


def read_labels_file(path):
    a = np.load(path)
    if hasattr(a, "files"):
        key = next((k for k in ("labels", "arr_0") if k in a.files), None)
        if key is None:
            raise SystemExit(f"{path}: none of the arrays labels / arr_0 found (has {list(a.files)})")
        a = a[key]
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype.kind not in "iu":
        raise SystemExit(f"{path}: the labels must be an integer [H, W] image, found {a.dtype} {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))


def run_depth(args, model, selection):
    """--depth_file: one frame through infer_on_depth, or with --labels_file through infer_on_scene."""
    from graspldm_amd.camera import Camera
    from graspldm_amd.pointcloud import depth_to_tensor, read_depth_file
    cam = Camera(args.camera_json)
    depth = depth_to_tensor(read_depth_file(args.depth_file), args.device)
    mask = read_mask_file(args.mask_file).to(args.device) if args.mask_file else None
    n_pts = args.num_points or encoder_points(model.model)
    box = None if args.crop_box is None else (args.crop_box[:3], args.crop_box[3:])
    if args.labels_file or args.segment_tabletop:
        common = dict(num_grasps=args.num_grasps, num_points=n_pts,
                      min_object_points=32 if args.min_object_points is None else args.min_object_points,
                      use_farthest_point=not args.random_resample, mask=mask, z_range=args.z_range,
                      depth_scale=args.depth_scale, crop_box=box, **selection_kwargs(args, selection, 0),
                      **cleanup_options(args), **downsample_options(args))
        if args.segment_tabletop:
            try:
                res = model.infer_on_tabletop(depth, cam, segmentation=segmentation_options(args), **common)
            except ValueError as e:
                raise SystemExit(f"{args.depth_file}: {e}")
            tp = res["table_plane"]
            print(f"{args.depth_file}: table plane n = {tp.normal.tolist()}, d = {tp.offset:.6f} ({tp.inliers} inliers)")
        else:
            labels = read_labels_file(args.labels_file).to(args.device)
            res = model.infer_on_scene(depth, cam, labels, **common)
        conf = res["confidence"].flatten()
        conf = conf[~torch.isnan(conf)]
        print(f"{args.depth_file}: {tuple(depth.shape)} depth, objects {res['object_label'].tolist()} with "
              f"{res['object_points'].tolist()} points -> {n_pts} each; grasps {tuple(res['grasps'].shape)}  "
              f"confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
        return [res]
    res = model.infer_on_depth(depth, cam, mask=mask, num_grasps=args.num_grasps, num_points=n_pts,
                               use_farthest_point=not args.random_resample, z_range=args.z_range,
                               depth_scale=args.depth_scale, crop_box=box, **selection_kwargs(args, selection, 0),
                               **cleanup_options(args), **downsample_options(args))
    conf = res["confidence"].flatten()
    print(f"{args.depth_file}: {tuple(depth.shape)} depth -> {n_pts} points; grasps {tuple(res['grasps'].shape)}  "
          f"confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
    return [res]


def run_mesh(args, model, selection):
    """--mesh_file: the object model through infer_on_mesh -- its sampled surface, or rendered views of it."""
    from graspldm_amd.camera import Camera, look_at
    from graspldm_amd.mesh import load_mesh
    try:
        mesh = load_mesh(args.mesh_file, scale=1.0 if args.mesh_scale is None else args.mesh_scale)
    except (OSError, ValueError) as e:
        raise SystemExit(f"{args.mesh_file}: {e}")
    n_pts = args.num_points or encoder_points(model.model)
    seed = int(np.random.randint(0, 1 << 31)) if args.mesh_seed is None else args.mesh_seed
    sel = {} if selection is None else dict(selection=selection)
    view, cam = None, None
    if args.camera_json:
        cam = Camera(args.camera_json)
        lo, hi = mesh.bounds
        view = args.mesh_views if args.mesh_view is None else look_at(args.mesh_view, (lo.astype(float) + hi.astype(float)) / 2)
    try:
        res = model.infer_on_mesh(mesh, num_grasps=args.num_grasps, num_points=n_pts, view=view, camera=cam, seed=seed,
                                  view_radius=args.view_radius, use_farthest_point=not args.random_resample, **sel)
    except ValueError as e:
        raise SystemExit(f"{args.mesh_file}: {e}")
    conf = res["confidence"].flatten()
    conf = conf[~torch.isnan(conf)]
    what = f"{n_pts} surface points" if view is None else f"{res['grasps'].shape[0]} rendered view(s) -> {n_pts} points each"
    print(f"{args.mesh_file}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces -> {what}; grasps "
          f"{tuple(res['grasps'].shape)}  confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
    return [res]


def run_cloud_scene(args, model, selection):
    """--segment_cloud: the one --pc_file scene through infer_on_cloud_scene."""
    from graspldm_amd.pointcloud import read_cloud_file
    path = args.pc_file[0]
    pc = torch.from_numpy(read_cloud_file(path))
    try:
        res = model.infer_on_cloud_scene(pc, num_grasps=args.num_grasps, num_points=args.num_points,
                                         segmentation=cloud_segmentation_options(args),
                                         min_object_points=32 if args.min_object_points is None else args.min_object_points,
                                         use_farthest_point=not args.random_resample, **selection_kwargs(args, selection, 0),
                                         **cleanup_options(args), **downsample_options(args))
    except ValueError as e:
        raise SystemExit(f"{path}: {e}")
    tp = res["table_plane"]
    if tp is not None:
        print(f"{path}: table plane n = {tp.normal.tolist()}, d = {tp.offset:.6f} ({tp.inliers} inliers)")
    conf = res["confidence"].flatten()
    conf = conf[~torch.isnan(conf)]
    print(f"{path}: {pc.shape[0]} points ({res['segmented_points'].shape[0]} clustered), objects "
          f"{res['object_label'].tolist()} with {res['object_points'].tolist()} points -> {args.num_points} each; grasps "
          f"{tuple(res['grasps'].shape)}  confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
    return [res]


def build_selection(args):
    """The GraspSelection of the selection flags, or None when none of them is set (nothing changes then)."""
    if not args.min_aligned_contacts and (args.both_fingers or args.friction_angle != 30.0 or args.normals_k != 12
                                          or args.normals_radius != 0.05):
        raise SystemExit("--friction_angle / --both_fingers / --normals_k / --normals_radius go with --min_aligned_contacts")
    asked = (args.collision_free or args.min_contacts or args.min_confidence is not None or args.min_success is not None
             or args.top_k is not None or args.diverse or args.min_separation or args.scene_file
             or args.min_aligned_contacts)
    if not asked:
        return None
    if args.min_success is not None and not args.classifier_config:
        raise SystemExit("--min_success needs --classifier_config")
    if args.top_k is not None and args.top_k < 1:
        raise SystemExit("--top_k must be at least 1")
    if args.scene_file and not (args.collision_free or args.min_contacts or args.min_aligned_contacts):
        raise SystemExit("--scene_file is read by --collision_free / --min_contacts / --min_aligned_contacts only")
    if args.scene_file and len(args.scene_file) not in (1, len(args.pc_file) if args.pc_file else args.num_samples):
        raise SystemExit("--scene_file: one file, or one per cloud")
    from graspldm_amd.grasp_select import GraspSelection
    try:
        return GraspSelection(min_confidence=args.min_confidence, min_success=args.min_success,
                              collision_free=args.collision_free, min_contacts=args.min_contacts, top_k=args.top_k,
                              diverse=args.diverse, min_separation=args.min_separation,
                              score_by="success" if args.min_success is not None else "confidence",
                              min_aligned_contacts=args.min_aligned_contacts, friction_angle_deg=args.friction_angle,
                              both_fingers=args.both_fingers, normals_k=args.normals_k, normals_radius=args.normals_radius)
    except ValueError as e:
        raise SystemExit(str(e))


def selection_kwargs(args, selection, i):
    """selection= / scene_pc= of the i-th cloud ({} without selection flags: the calls stay what they were)."""
    if selection is None:
        return {}
    scene = None
    if args.scene_file:
        from graspldm_amd.pointcloud import read_cloud_file
        scene = torch.from_numpy(read_cloud_file(args.scene_file[i if len(args.scene_file) > 1 else 0]))
    return dict(selection=selection, scene_pc=scene)


def setup_model(args):
    if args.synthetic:
        from graspldm_amd.pipeline import build_fpc_ldm
        ldm = build_fpc_ldm(n_points=args.synthetic, scheduler="ddim")
        if args.mode == "LDM":
            return InferenceLDM(model=ldm, num_inference_steps=args.inference_steps, device=args.device)
        return InferenceVAE(model=ldm.vae_model, device=args.device)
    if not args.exp_path:
        raise SystemExit("--exp_path is required (or use --synthetic N)")
    exp_name, exp_root = os.path.basename(args.exp_path.rstrip("/")), os.path.dirname(args.exp_path.rstrip("/"))
    if args.mode == "LDM":
        model = InferenceLDM(exp_name=exp_name, exp_out_root=exp_root, data_root=args.data_root,
                             num_inference_steps=args.inference_steps, use_fast_sampler=True,
                             data_split=args.split, use_ema_model=args.use_ema_model, device=args.device)
        dm = model.model.diffusion_model
        print(f"Trained using noise schedule: beta0 = {dm.beta_start} ; betaT = {dm.beta_end}")
        return model
    return InferenceVAE(exp_name=exp_name, exp_out_root=exp_root, data_root=args.data_root, data_split=args.split,
                        use_ema_model=args.use_ema_model, device=args.device)


def find_classifier_section(cfg):
    """The {type, args} dict of the classifier inside a reference-style config: `model` (or `models`) itself, its
    `classifier` entry, or a `model` key below either."""
    for key in ("model", "models"):
        node = cfg.get(key) if isinstance(cfg, dict) else None
        for _ in range(3):
            if not isinstance(node, dict):
                break
            if node.get("type") == "PointsBasedGraspClassifier":
                return node
            node = node.get("classifier", node.get("model"))
    raise SystemExit("--classifier_config: no model of type PointsBasedGraspClassifier under `model` / `models`")


def setup_classifier(args, model):
    """Build the classifier of --classifier_config, load --classifier_ckpt (or recipe weights under --synthetic), attach."""
    if not args.classifier_config:
        if args.classifier_ckpt or args.sort_by_success:
            raise SystemExit("--classifier_ckpt / --sort_by_success need --classifier_config")
        return model
    from graspldm_amd.builder import build_model
    from graspldm_amd.config import Config
    section = find_classifier_section(Config.fromfile(args.classifier_config))
    clf = build_model(section)
    if args.classifier_ckpt:
        from graspldm_amd.checkpoint import load_weights
        load_weights(clf, args.classifier_ckpt, args.use_ema_model)
    elif args.synthetic:
        from graspldm_amd.synthetic import load_synthetic_weights
        load_synthetic_weights(clf, seed=0)
    else:
        raise SystemExit("--classifier_ckpt is required (recipe weights are used under --synthetic only)")
    model.set_classifier(clf.eval())
    return model


def read_grasp_file(path):
    """[G,4,4] or [B,G,4,4] float32 from .npy / .npz (key `grasps`) -> tensor [B,G,4,4] (B = 1 for a single set)."""
    z = np.load(path)
    if hasattr(z, "files"):
        if "grasps" not in z.files:
            raise SystemExit(f"{path}: no array named `grasps` (found {list(z.files)})")
        z = z["grasps"]
    H = np.asarray(z, dtype=np.float32)
    if H.ndim == 3:
        H = H[None]
    if H.ndim != 4 or H.shape[-2:] != (4, 4) or H.shape[1] == 0:
        raise SystemExit(f"{path}: grasps must be [G,4,4] or [B,G,4,4], found {H.shape}")
    if not np.isfinite(H).all():
        raise SystemExit(f"{path}: grasps hold non-finite entries")
    return torch.from_numpy(H)


def run_one(args, model, pcn, metas, start, i, sel=None):
    """One cloud: generation, or reconstruction / refinement of the i-th grasp set of --refine_from."""
    sel = sel or {}
    if start is None:
        return model.generate_grasps(pcn, metas, num_grasps=args.num_grasps, **sel)
    H = start[i if start.shape[0] > 1 else 0].unsqueeze(0)
    if args.mode == "LDM":
        return model.refine_grasps(pcn, metas, H, strength=args.refine_strength, **sel)
    return model.reconstruct_grasps(pcn, metas, H, **sel)


def main(argv=None):
    args = parse_args(argv)
    selection = build_selection(args)
    start = None
    if args.refine_from:
        if not 0.0 <= args.refine_strength <= 1.0:
            raise SystemExit("--refine_strength must lie in [0, 1]")
        start = read_grasp_file(args.refine_from)
        args.num_grasps = int(start.shape[1])
        want = len(args.pc_file) if args.pc_file else args.num_samples
        if start.shape[0] not in (1, want):
            raise SystemExit(f"--refine_from holds {start.shape[0]} grasp sets for {want} clouds (one set, or one per cloud)")
    if args.conditioning != "unconditional":
        raise SystemExit("class / region conditioned models are not shipped with the reference (out of scope)")
    if args.visualize:
        print("visualisation (trimesh/pyrender) is out of scope on this path; ignoring --visualize")
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
    model = setup_classifier(args, setup_model(args))
    from graspldm_amd.synthetic import normalize_cloud, synthetic_cloud
    results = []
    if args.depth_file:
        return finish(args, run_depth(args, model, selection))
    if args.mesh_file:
        return finish(args, run_mesh(args, model, selection))
    if args.segment_cloud:
        return finish(args, run_cloud_scene(args, model, selection))
    if args.pc_file:
        from graspldm_amd.pointcloud import read_cloud_file
        n_pts = args.num_points or encoder_points(model.model)
        for path in args.pc_file:
            pc = torch.from_numpy(read_cloud_file(path))
            if start is None:
                res = model.infer_on_pointcloud(pc, num_grasps=args.num_grasps, num_points=n_pts,
                                                use_farthest_point=not args.random_resample,
                                                **selection_kwargs(args, selection, len(results)),
                                                **downsample_options(args))
            else:
                pcn, metas = model.prepare_pointcloud(pc, num_points=n_pts, use_farthest_point=not args.random_resample)
                res = run_one(args, model, pcn, metas, start, len(results), selection_kwargs(args, selection, len(results)))
            conf = res["confidence"].flatten()
            print(f"{path}: {pc.shape[0]} points -> {n_pts}; grasps {tuple(res['grasps'].shape)}  "
                  f"confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
            results.append(res)
        return finish(args, results)
    for i in range(args.num_samples):
        if args.synthetic:
            idx = int(np.random.randint(0, 1 << 20))
            pc, metas = normalize_cloud(synthetic_cloud(idx, args.synthetic))
            metas = {k: (v.unsqueeze(0) if isinstance(v, torch.Tensor) else v) for k, v in metas.items()}
        else:
            raise SystemExit("ACRONYM dataset loading is out of scope: pass the object's cloud with --pc_file FILE "
                             "(.npy / .ply / ...), or run on synthetic clouds with --synthetic N")
        res = run_one(args, model, pc, metas, start, i, selection_kwargs(args, selection, i))
        conf = res["confidence"].flatten()
        print(f"sample {i}: cloud #{idx}  grasps {tuple(res['grasps'].shape)}  "
              f"confidence mean {conf.mean().item():.3f}  best {conf.max().item():.3f}")
        results.append(res)
    return finish(args, results)


def encoder_points(model):
    """n_points of the model's cloud encoder (its out_layer[1] is a Linear over the point axis: N is fixed)."""
    vae = getattr(model, "vae_model", model)
    enc = vae.encoder.pc_encoder if hasattr(vae, "encoder") else vae.pc_encoder
    try:
        return int(enc.out_layer[1].in_features)
    except (AttributeError, IndexError, TypeError):
        raise SystemExit("cannot infer the encoder's point count; pass --num_points")


def finish(args, results):
    if args.sort_by_success:   # every per-grasp array of a cloud in the order of falling success
        for r in results:
            order = torch.argsort(r["success"][..., 0], dim=1, descending=True, stable=True)
            for k in ("grasps", "grasp_tmrp", "confidence", "success", "latent_mu", "latent_logvar"):
                if k in r:
                    idx = order.view(*order.shape, *([1] * (r[k].ndim - 2))).expand_as(r[k])
                    r[k] = torch.gather(r[k], 1, idx)
    if args.out:
        extra = {k: torch.cat([r[k] for r in results]).cpu().numpy()
                 for k in ("latent_mu", "latent_logvar", "success", "selected_index", "selected_count", "selected_gap",
                           "clearance", "contacts", "aligned_contacts", "object_label", "object_points", "object_points_raw",
                           "scene_rank", "cam_pose")
                 if all(r.get(k) is not None for r in results)}
        if all(isinstance(r.get("mesh_face"), torch.Tensor) for r in results):   # --mesh_file without a view
            extra["mesh_face"] = torch.cat([r["mesh_face"] for r in results]).cpu().numpy()
        if all(r.get("voxel_size") is not None for r in results):   # --voxel_size: the size every result ended with
            extra["voxel_size"] = np.asarray([r["voxel_size"] for r in results], dtype=np.float32)
        if all(r.get("segmented_points") is not None for r in results):   # --segment_cloud: one scene per result
            extra["labels"] = torch.stack([r["labels"] for r in results]).cpu().numpy()
            extra["segmented_points"] = torch.stack([r["segmented_points"] for r in results]).cpu().numpy()
            if all(r.get("table_plane") is not None for r in results):
                extra["table_plane"] = np.stack([r["table_plane"].as_array() for r in results])
        elif all(r.get("table_plane") is not None for r in results):   # --segment_tabletop: one frame per result
            extra["labels"] = torch.stack([r["labels"] for r in results]).cpu().numpy()
            extra["table_plane"] = np.stack([r["table_plane"].as_array() for r in results])
        np.savez_compressed(args.out, grasps=torch.cat([r["grasps"] for r in results]).cpu().numpy(),
                            grasp_tmrp=torch.cat([r["grasp_tmrp"] for r in results]).cpu().numpy(),
                            confidence=torch.cat([r["confidence"] for r in results]).cpu().numpy(), **extra)
        print("wrote", args.out)
    return results


if __name__ == "__main__":
    main()
