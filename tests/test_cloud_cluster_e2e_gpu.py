"""GPU: from a fused, shuffled scene cloud to the grasps of every object in it -- fit_plane and segment_cloud against the
restatements (tests/tabletop_ref.py, tests/cloud_cluster_ref.py), infer_on_cloud_scene against regularize_objects +
normalize_input + generate_grasps on the restated split, the ValueErrors, the CLI's --segment_cloud path against the API,
and infer_on_pointcloud left as it was.  Model fixture and recipe of tests/test_tabletop_e2e_gpu.py: 10 DDIM steps, 4
grasps, num_points = 1024.  The scene (world frame, the origin 0.6 m above the table): a tilted table, three boxes -- two of
them 2 cm apart: less than a finger, twice link_dist --, a speck of a few points; two 96 x 128 cameras look at it from two
sides, millimetre-scale depth noise and 5 % dead pixels each; depth_to_cloud with cam_to_world, concatenated, shuffled."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cloud_cluster_ref as ref
import cloud_downsample_ref as dref
import tabletop_ref as R
from depth_ref import deproject

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 96, 128
INTR = (200.0, 201.5, 63.25881958, 47.5)
TOL, T, LINK = 0.005, 512, 0.01
Z0 = -0.6
TABLE = (0.02, 0.01)   # z = Z0 + 0.02 x + 0.01 y
BOXES = ((-0.12, -0.04, -0.04, 0.04, 0.08), (-0.02, 0.05, -0.04, 0.04, 0.10), (0.10, 0.16, 0.03, 0.10, 0.06),
         (0.0, 0.005, -0.12, -0.115, 0.025))   # x0 x1 y0 y1 top; the last one is the speck
CAMS = (((0.0, -0.45, Z0 + 0.55), (0.0, 0.0, Z0 + 0.03)), ((0.35, 0.40, Z0 + 0.50), (0.0, 0.0, Z0 + 0.03)))


def _look_at(pos, target):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    z = (target - pos) / np.linalg.norm(target - pos)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
    return m.astype(np.float32)


def _render(cam_to_world, rng):
    """The depth frame of one camera: every pixel's ray against the table plane and the boxes, the nearest hit."""
    fx, fy, cx, cy = INTR
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)   # z_cam = 1: the ray parameter is the depth
    rot, o = cam_to_world[:3, :3].astype(np.float64), cam_to_world[:3, 3].astype(np.float64)
    d = rays @ rot.T
    nrm = np.array([-TABLE[0], -TABLE[1], 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (Z0 - o @ nrm) / (d @ nrm)
        t = np.where(t > 0, t, np.inf)
        for x0, x1, y0, y1, top in BOXES:
            lo, hi = np.array([x0, y0, Z0 - 0.05]), np.array([x1, y1, Z0 + top])
            t0, t1 = (lo - o) / d, (hi - o) / d
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            t = np.where((near <= far) & (near > 0), np.minimum(t, near), t)
    depth = t + rng.normal(0.0, 0.0005, t.shape)
    depth[~np.isfinite(depth)] = 0.0
    depth[rng.random(t.shape) < 0.05] = 0.0
    return depth.astype(np.float32)


def _camera():
    from graspldm_amd.camera import Camera
    return Camera.from_intrinsics(*INTR, W, H)


def _frames():
    rng = np.random.default_rng(42)
    poses = [_look_at(*c) for c in CAMS]
    return [(torch.from_numpy(_render(p, rng)), torch.from_numpy(p)) for p in poses]


@pytest.fixture(scope="module")
def restated():
    """The restatement, once: the fused cloud, the triples, the fit, the labels under that plane and their split."""
    cam = _camera()
    clouds = [deproject(depth, cam.K, cam_to_world=pose)[0].numpy() for depth, pose in _frames()]
    cloud = np.concatenate(clouds)
    perm = np.random.default_rng(1).permutation(cloud.shape[0])
    cloud = np.ascontiguousarray(cloud[perm])
    triples = np.random.default_rng(0).integers(0, cloud.shape[0], (T, 3))
    fit = R.fit_plane(cloud, triples, TOL, 1e-8)
    plane = np.append(fit[0], fit[1]).astype(np.float32)
    every = ref.cluster_one(cloud, LINK, plane, 0.01, 0.5, min_points=1, max_labels=64)
    seg = ref.cluster_one(cloud, LINK, plane, 0.01, 0.5, min_points=32, max_labels=64)
    assert seg[1] == 3 and fit[2] > 0.6 * cloud.shape[0] and fit[0][2] > 0.99
    assert every[1] >= 4 and 0 < every[2][3] < 32            # the speck is a component, below min_points
    centre = [cloud[seg[0] == k].mean(axis=0) for k in (1, 2, 3)]
    gaps = sorted(np.linalg.norm(centre[i] - centre[j]) for i in range(3) for j in range(i))
    assert gaps[0] < 0.11                                     # the two boxes 2 cm apart are two labels
    split = ref.split_labels(cloud, seg[0], [0], [cloud.shape[0]], 64)
    return dict(cloud=cloud, perm=perm, triples=triples, fit=fit, plane=plane, seg=seg, split=split)


@pytest.fixture(scope="module")
def inf(fpc_state_dict):
    from graspldm_amd.inference import InferenceLDM
    from test_modules_cpu import build_fpc
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return InferenceLDM(model=m.cuda().eval(), num_inference_steps=10, device="cuda:0")


def _seed(s=4):
    torch.manual_seed(s)
    np.random.seed(s)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return [0 if x == y else (1 if y in (np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))) else 99)
            for x, y in zip(a, b)]


def _same_tensors(got, exp):
    for k, v in exp.items():
        if isinstance(v, torch.Tensor):
            same = torch.equal(got[k].view(torch.int32), v.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(got[k], v)
            assert same, k


def test_the_fused_cloud_is_the_restated_one(restated):
    from graspldm_amd.pointcloud import depth_to_cloud
    cam = _camera()
    clouds = [depth_to_cloud(depth.cuda(), cam, cam_to_world=pose) for depth, pose in _frames()]
    fused = torch.cat(clouds)[torch.from_numpy(restated["perm"]).cuda()]
    assert fused.cpu().numpy().tobytes() == restated["cloud"].tobytes()


def test_fit_plane_equals_the_restatement(restated):
    from graspldm_amd.pointcloud import fit_plane
    cloud = torch.from_numpy(restated["cloud"]).cuda()
    normal, offset, inl, hyp = restated["fit"]
    raw = fit_plane(cloud, tol=TOL, hypotheses=T, refit=False)
    e_n, e_o, _, _ = R.fit_plane(restated["cloud"], restated["triples"], TOL, 1e-8, refit=False)
    assert (raw.hypothesis, raw.inliers) == (hyp, inl)
    assert np.array_equal(raw.normal.view(np.int32), e_n.view(np.int32)) and np.float32(raw.offset) == e_o
    got = fit_plane(cloud, tol=TOL, hypotheses=T)
    assert (got.hypothesis, got.inliers) == (hyp, inl)
    assert max(_ulps(got.normal, normal)) <= 1 and max(_ulps([got.offset], [offset])) <= 1, (got, normal, offset)
    assert got.normal[2] > 0.99 and got.offset > 0.5          # the origin, 0.6 m above the table, has positive height
    seen = fit_plane(cloud, tol=TOL, hypotheses=T, view_point=CAMS[1][0], rng=np.random.default_rng(0))
    assert np.array_equal(seen.as_array(), got.as_array())    # a camera centre lies on the same side
    below = fit_plane(cloud, tol=TOL, hypotheses=T, view_point=(0.0, 0.0, -2.0))
    assert np.array_equal(below.as_array(), -got.as_array()) and below.inliers == got.inliers


def test_segment_cloud_equals_the_restated_labels(restated):
    from graspldm_amd.pointcloud import TablePlane, cluster_cloud, segment_cloud
    cloud = torch.from_numpy(restated["cloud"]).cuda()
    normal, offset, inl, hyp = restated["fit"]
    e_labels, e_num, e_sizes, e_roots = restated["seg"]
    plane = TablePlane(normal, offset, inl, hyp)
    labels, num, got_plane = segment_cloud(cloud, plane=plane, link_dist=LINK)
    assert num == e_num == 3 and labels.dtype == torch.int32 and labels.is_cuda and got_plane is plane
    assert np.array_equal(labels.cpu().numpy(), e_labels)
    _, _, sizes, roots = cluster_cloud(cloud, link_dist=LINK, plane=plane, return_stats=True)
    assert sizes == e_sizes.tolist() and roots == e_roots.tolist()
    labels2, num2, plane2 = segment_cloud(cloud, tol=TOL, hypotheses=T)      # plane=None fits one first
    assert num2 == 3 and plane2.hypothesis == hyp
    if np.array_equal(plane2.as_array(), restated["plane"]):
        assert torch.equal(labels2, labels)
    labels3, num3, plane3 = segment_cloud(cloud, table=False, link_dist=LINK, min_points=500)   # the table joins everything
    e3 = ref.cluster_one(restated["cloud"], LINK, None, 0, 0, min_points=500, max_labels=64, search="grid")
    assert plane3 is None and num3 == e3[1] >= 1 and np.array_equal(labels3.cpu().numpy(), e3[0])


def _manual(inf, cloud_np, labels_np, num, seed, num_grasps=4, cleanup=None, scene=None, selection=None, min_object_points=32):
    """regularize_objects + normalize_input + generate_grasps on the restated split of (cloud, labels)."""
    from graspldm_amd.pointcloud import regularize_objects, remove_outliers
    split = ref.split_labels(cloud_np, labels_np, [0], [cloud_np.shape[0]], 64)
    packed = torch.from_numpy(split["out_points"]).cuda()
    starts, counts = split["obj_start"][0, :num].tolist(), split["obj_count"][0, :num].tolist()
    raw = counts
    if cleanup is not None:
        packed, starts, counts, _, _ = remove_outliers(packed, start=starts, count=counts, **cleanup.options)
    kept = [k for k, c in enumerate(counts) if c >= min_object_points]
    _seed(seed)   # an object below 1024 points is filled up with rows drawn from numpy's generator
    batch = regularize_objects(packed, [starts[k] for k in kept], [counts[k] for k in kept], 1024)
    pcn, metas = inf.normalize_input(batch)
    extra = {} if selection is None else dict(selection=selection, scene_pc=scene)
    out = inf.generate_grasps(pcn, metas, num_grasps=num_grasps, **extra)
    return out, [k + 1 for k in kept], [counts[k] for k in kept], [raw[k] for k in kept]


def test_infer_on_cloud_scene_equals_the_manual_chain_on_the_restated_split(inf, restated):
    from graspldm_amd.grasp_select import CloudCleanup, CloudDownsample, GraspSelection
    from graspldm_amd.pointcloud import TablePlane, remove_outliers, voxel_downsample
    cloud_np = restated["cloud"]
    cloud = torch.from_numpy(cloud_np).cuda()
    normal, offset, inl, hyp = restated["fit"]
    plane = TablePlane(normal, offset, inl, hyp)
    sel = GraspSelection(collision_free=True, top_k=2)
    down = CloudDownsample(voxel_size=0.004, apply_to_scene=True)
    clean = CloudCleanup(k=8, max_radius=0.012, min_neighbors=4, apply_to_scene=True)
    v = 0.004
    small_np = dref.downsample_cloud(cloud_np, v)["points"]
    small_seg = ref.cluster_one(small_np, LINK, restated["plane"], 0.01, 0.5, min_points=32, max_labels=64, search="grid")
    assert small_seg[1] == 3 and small_np.shape[0] < cloud_np.shape[0]
    for seed, (use_sel, use_down, use_clean) in enumerate([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]):
        kw = {}
        base_np, seg = (small_np, small_seg) if use_down else (cloud_np, restated["seg"])
        scene = None
        if use_sel:
            scene = torch.from_numpy(small_np).cuda() if use_down else cloud     # the input cloud, downsampled, then cleaned
            if use_clean:
                scene = remove_outliers(scene, **clean.options)[0]
            scene = scene.unsqueeze(0)
            kw["selection"] = sel
        if use_down:
            kw["downsample"] = down
        if use_clean:
            kw["cleanup"] = clean
        exp, e_label, e_points, e_raw = _manual(inf, base_np, seg[0], seg[1], seed + 3, cleanup=clean if use_clean else None,
                                                scene=scene, selection=sel if use_sel else None)
        _seed(seed + 3)
        got = inf.infer_on_cloud_scene(cloud, num_grasps=4, num_points=1024, segmentation=dict(plane=plane, link_dist=LINK), **kw)
        assert got["grasps"].shape == ((3, 2, 4, 4) if use_sel else (3, 4, 4, 4))
        _same_tensors(got, exp)
        assert got["object_label"].tolist() == e_label == [1, 2, 3] and got["object_points"].tolist() == e_points
        assert np.array_equal(got["labels"].cpu().numpy(), seg[0]) and got["table_plane"] is plane
        assert got["segmented_points"].cpu().numpy().tobytes() == base_np.tobytes()
        assert ("voxel_size" in got) == bool(use_down) and ("object_points_raw" in got) == bool(use_clean)
        if use_down:
            assert got["voxel_size"] == float(np.float32(v))
            assert torch.equal(voxel_downsample(cloud, v)[0], got["segmented_points"])
        if use_clean:
            assert got["object_points_raw"].tolist() == e_raw and all(a <= b for a, b in zip(e_points, e_raw))
        assert got["scene_rank"].shape[1] == 2 and got["scene_rank"].shape[0] == (6 if use_sel else 12) - int(
            torch.isnan(got["grasps"].reshape(-1, 16)).any(dim=1).sum())


def test_value_errors(inf, restated, monkeypatch):
    from graspldm_amd.grasp_select import CloudDownsample
    cloud = torch.from_numpy(restated["cloud"]).cuda()
    plane = restated["plane"]

    def boom(*a, **k):
        raise AssertionError("generation started")

    monkeypatch.setattr(inf, "generate_grasps", boom)
    with pytest.raises(ValueError, match="exceeds link_dist"):
        inf.infer_on_cloud_scene(cloud, num_points=1024, downsample=CloudDownsample(voxel_size=0.02),
                                 segmentation=dict(plane=plane))
    with pytest.raises(ValueError, match="exceeds link_dist"):      # the size actually used: grown past link_dist by the cap
        inf.infer_on_cloud_scene(cloud, num_points=1024, downsample=CloudDownsample(voxel_size=0.009, max_points=2000),
                                 segmentation=dict(plane=plane))
    with pytest.raises(ValueError, match="no object found in the cloud: no cluster of at least 5000"):
        inf.infer_on_cloud_scene(cloud, num_points=1024, segmentation=dict(plane=plane, min_points=5000))
    with pytest.raises(ValueError, match=r"no object has at least 4000 points \(labels 1 .. 3 hold \["):
        inf.infer_on_cloud_scene(cloud, num_points=1024, segmentation=dict(plane=plane), min_object_points=4000)
    with pytest.raises(ValueError, match="differ in size"):
        inf.infer_on_cloud_scene(cloud, segmentation=dict(plane=plane))
    with pytest.raises(ValueError, match=r"one cloud \[N, 3\]"):
        inf.infer_on_cloud_scene(cloud.unsqueeze(0), num_points=1024)
    with pytest.raises(ValueError, match="view_point was given twice"):
        inf.infer_on_cloud_scene(cloud, num_points=1024, view_point=(0, 0, 0), segmentation=dict(view_point=(0, 0, 1)))
    with pytest.raises(ValueError, match="link_dist"):
        inf.infer_on_cloud_scene(cloud, num_points=1024, segmentation=dict(plane=plane, link_dist=-1.0))
    with pytest.raises(TypeError, match="CloudDownsample"):
        inf.infer_on_cloud_scene(cloud, num_points=1024, downsample=dict(voxel_size=0.003))


def test_cli_segment_cloud_equals_the_api(tmp_path, fpc_state_dict, restated):
    from test_checkpoint import _write_experiment
    from graspldm_amd.grasp_select import CloudCleanup, CloudDownsample
    from graspldm_amd.inference import InferenceLDM
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ema = {k: (v + 0.01 if v.is_floating_point() else v) for k, v in fpc_state_dict.items()}
    _write_experiment(str(tmp_path), "exp_cloud", fpc_state_dict, ema)
    np.save(tmp_path / "scene.npy", restated["cloud"])
    out = str(tmp_path / "o.npz")
    res = cli.main(["--exp_path", str(tmp_path / "exp_cloud"), "--mode", "LDM", "--num_grasps", "4", "--inference_steps", "10",
                    "--pc_file", str(tmp_path / "scene.npy"), "--num_points", "1024", "--segment_cloud", "--table_tol", str(TOL),
                    "--ransac_hypotheses", str(T), "--segment_seed", "0", "--link_dist", str(LINK), "--min_cluster_points", "40",
                    "--min_object_points", "50", "--voxel_size", "0.004", "--remove_outliers", "--outlier_radius", "0.012",
                    "--seed", "5", "--out", out])
    assert len(res) == 1 and res[0]["grasps"].shape == (3, 4, 4, 4)
    _seed(5)   # where the CLI seeds: in front of building the model, whose initialisers draw from the same generator
    api = InferenceLDM(exp_name="exp_cloud", exp_out_root=str(tmp_path), num_inference_steps=10, use_fast_sampler=True)
    exp = api.infer_on_cloud_scene(torch.from_numpy(restated["cloud"]), num_grasps=4, num_points=1024,
                                   segmentation=dict(tol=TOL, hypotheses=T, rng=np.random.default_rng(0), link_dist=LINK,
                                                     min_points=40),
                                   min_object_points=50, downsample=CloudDownsample(voxel_size=0.004),
                                   cleanup=CloudCleanup(max_radius=0.012))
    z = np.load(out)
    for k in ("grasps", "confidence", "object_label", "object_points", "object_points_raw", "scene_rank"):
        assert np.array_equal(z[k], exp[k].cpu().numpy()), k
    assert np.array_equal(z["labels"][0], exp["labels"].cpu().numpy()) and z["labels"].dtype == np.int32
    assert z["segmented_points"][0].tobytes() == exp["segmented_points"].cpu().numpy().tobytes()
    assert np.array_equal(z["table_plane"][0], exp["table_plane"].as_array()) and z["voxel_size"].tolist() == [np.float32(0.004)]
    assert exp["table_plane"].hypothesis >= 0 and z["object_label"].tolist() == [1, 2, 3]
    # --no_table_plane: plain clustering; the table joins everything into one object, and no plane is written
    res = cli.main(["--exp_path", str(tmp_path / "exp_cloud"), "--mode", "LDM", "--num_grasps", "2", "--inference_steps", "10",
                    "--pc_file", str(tmp_path / "scene.npy"), "--num_points", "1024", "--segment_cloud", "--no_table_plane",
                    "--min_cluster_points", "500", "--seed", "5", "--out", out])
    z = np.load(out)
    assert res[0]["table_plane"] is None and "table_plane" not in z.files and z["labels"].shape == (1, restated["cloud"].shape[0])
    assert z["object_label"].tolist() == list(range(1, res[0]["grasps"].shape[0] + 1))


def test_infer_on_pointcloud_without_the_switch_is_what_it_was(inf, restated):
    cloud = torch.from_numpy(restated["cloud"]).cuda()
    _seed(9)
    a = inf.infer_on_pointcloud(cloud, num_grasps=4, num_points=1024)
    _seed(9)
    pcn, metas = inf.prepare_pointcloud(cloud, 1024, True)      # its own two halves, as before this entry existed
    b = inf.generate_grasps(pcn, metas, num_grasps=4)
    assert a["grasps"].shape == (1, 4, 4, 4) and set(a) == set(b)
    _same_tensors(a, b)
    for key in ("labels", "segmented_points", "table_plane", "object_label", "scene_rank", "voxel_size"):
        assert key not in a
