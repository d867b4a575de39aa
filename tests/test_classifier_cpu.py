"""CPU: the grasp success classifier's construction, schema, host-side folds, shape predicate and CLI flags (no compute
calls without a GPU)."""
import ctypes
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT

BACKBONES = ["PVCNN", "PVCNN2"]
_HOST = (ctypes.c_float * 72)()


def _host_ptr():
    """A non-null, 16-byte aligned host pointer for calls that return a status before anything is dereferenced."""
    return ctypes.c_void_p((ctypes.addressof(_HOST) + 15) // 16 * 16)


def _schema(backbone):
    with open(os.path.join(GOLDEN, "schema_grasp_classifier.json")) as f:
        raw = json.load(f)[backbone]
    return {k: (tuple(shape), getattr(torch, dt)) for k, (shape, dt) in raw.items()}


def test_builder_builds_the_registered_model():
    from graspldm_amd.builder import ALL_MODELS, build_model_from_cfg
    from graspldm_amd.grasp_classifier import PointsBasedGraspClassifier
    from graspldm_amd.pipeline import classifier_model_config
    assert ALL_MODELS["PointsBasedGraspClassifier"] is PointsBasedGraspClassifier
    assert set(PointsBasedGraspClassifier.SUPPORTED_BASE_NETWORKS) == {"PVCNN", "PVCNN2"}
    cfg = classifier_model_config(64, 12)
    model = build_model_from_cfg(cfg)
    assert isinstance(model, PointsBasedGraspClassifier) and model.num_pc_points == 76
    assert model.classifier[3].in_features == 76 and isinstance(model.classifier[1], torch.nn.Dropout)
    # loss_config is optional and ignored
    args = dict(cfg["model"]["args"])
    args.pop("loss_config")
    assert isinstance(PointsBasedGraspClassifier(**args), PointsBasedGraspClassifier)
    with pytest.raises(NotImplementedError):
        PointsBasedGraspClassifier(76, dict(type="PointNet2SSG", args={}))


@pytest.mark.parametrize("backbone", BACKBONES)
def test_state_dict_matches_the_reference_schema(backbone):
    from graspldm_amd.pipeline import build_classifier
    from graspldm_amd.synthetic import synthetic_state_dict
    schema = _schema(backbone)
    model = build_classifier(1024, 64, backbone)
    sd = model.state_dict()
    assert set(sd) == set(schema), (sorted(set(sd) - set(schema)), sorted(set(schema) - set(sd)))
    for k, (shape, dtype) in schema.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == dtype, k
    for k in ("classifier.0.layers.0.weight", "classifier.0.layers.1.running_var", "classifier.2.weight", "classifier.3.weight"):
        assert k in sd
    assert not any(k.startswith("classifier.1.") for k in sd)   # the Dropout keeps the numbering
    model.load_state_dict(synthetic_state_dict(schema, seed=0), strict=True)


def test_compute_loss_raises_and_cpu_tensors_raise():
    from graspldm_amd.pipeline import build_classifier
    model = build_classifier(64, 12)
    pc, gp = torch.zeros(2, 64, 3), torch.zeros(2, 12, 3)
    with pytest.raises(NotImplementedError, match="compute_loss=False"):
        model(pc, gp)
    with pytest.raises(NotImplementedError, match="compute_loss=False"):
        model(pc, gp, cls_target=torch.zeros(2), compute_loss=True)
    with pytest.raises(RuntimeError, match="must be CUDA tensors"):
        model(pc, gp, compute_loss=False)
    with pytest.raises(RuntimeError, match="must be CUDA tensors"):
        model.classify_grasps(pc, gp)
    with pytest.raises(RuntimeError, match="must be CUDA tensors"):
        model.score_poses(pc, torch.eye(4).repeat(2, 1, 1, 1))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model.head(torch.zeros(2, 512, 76))


@pytest.mark.parametrize("n", [1, 3, 4, 12, 64, 76])
def test_control_points_lie_on_the_open_gripper(n):
    from graspldm_amd import gripper
    p = gripper.control_points(n)
    assert p.shape == (n, 3) and p.dtype == torch.float32 and torch.isfinite(p).all()
    assert sum(gripper.segment_counts(n)) == n
    seg = torch.tensor(gripper.OPEN_SEGMENTS, dtype=torch.float64)
    a, d = seg[:, 0], seg[:, 1] - seg[:, 0]
    # distance of every point to its nearest segment
    t = (((p.double()[:, None] - a[None]) * d[None]).sum(-1) / (d * d).sum(-1)[None]).clamp(0, 1)
    dist = (p.double()[:, None] - (a[None] + t[..., None] * d[None])).norm(dim=-1).min(dim=1).values
    assert dist.max() < 1e-8
    assert len({tuple(r) for r in p.tolist()}) == n               # no point twice
    if n >= 4:
        assert min(gripper.segment_counts(n)) >= 1


def test_default_point_count_keeps_whole_tiles():
    from graspldm_amd import gripper
    assert (1024 + gripper.DEFAULT_POINTS) % 32 == 0
    assert gripper.control_points().shape == (gripper.DEFAULT_POINTS, 3)


@torch.no_grad()
def test_head_fold_matches_f64():
    from graspldm_amd.grasp_classifier import fold_head
    from graspldm_amd.pipeline import build_classifier
    model = build_classifier(64, 12)
    conv, bn, conv2, lin = model._head_layers()
    w1, b1, w2, l, c0 = fold_head(conv, bn, conv2, lin)
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w64 = conv.weight.double().reshape(128, -1) * s[:, None]
    b64 = (conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()
    assert w1.shape == (128, model.base_network.out_channels) and b1.shape == (128,)
    assert (w1.double() - w64).abs().max() <= 2e-7 * w64.abs().max()
    assert (b1.double() - b64).abs().max() <= 2e-7 * max(1.0, float(b64.abs().max()))
    assert torch.equal(w2, conv2.weight.reshape(-1)) and torch.equal(l, lin.weight.reshape(-1))
    c64 = float(lin.bias.double() + conv2.bias.double() * lin.weight.double().sum())
    assert abs(c0 - c64) <= 1e-12 * max(1.0, abs(c64))


def test_head_pack_takes_the_f32_form_outside_the_f16_range():
    from graspldm_amd import numerics
    from graspldm_amd.grasp_classifier import _pack_head
    from graspldm_amd.pipeline import build_classifier
    model = build_classifier(64, 12)
    conv, bn, conv2, lin = model._head_layers()
    c = model.base_network.out_channels
    p = _pack_head(conv, bn, conv2, lin, "cpu")
    assert not p.exact and p.w1.numel() == 128 * c                 # two f16 planes = one float per element
    with numerics.f32_only():
        q = _pack_head(conv, bn, conv2, lin, "cpu")
    assert q.exact and q.w1.numel() == 128 * c
    with torch.no_grad():
        bn.weight[3] = 1e7                                         # folded |w| beyond 65504
    r = _pack_head(conv, bn, conv2, lin, "cpu")
    assert r.exact and torch.isfinite(r.w1).all()


SHAPE_TABLE = [(64, 128, 96, True), (512, 128, 76, True), (64, 128, 1088, True), (1536, 128, 52, True), (16, 16, 1, True),
               (2048, 512, 1 << 20, True), (48, 16, 7, True),
               (8, 128, 64, False), (24, 128, 64, False), (2064, 128, 64, False), (64, 120, 64, False), (64, 528, 64, False),
               (64, 8, 64, False), (64, 128, (1 << 20) + 1, False)]


@pytest.mark.parametrize("c,rows,n,ok", SHAPE_TABLE)
def test_shape_predicate_agrees_with_the_c_entry(c, rows, n, ok):
    """cls_head_supported (Python) against gldm_cls_head's own answer: the workspace query and the entry's status.  Rejected
    shapes return GLDM_ERR_UNSUPPORTED before anything is launched (non-null dummy pointers, never dereferenced)."""
    from graspldm_amd import _lib as L
    from graspldm_amd.grasp_classifier import cls_head_supported
    h = L.lib()
    assert cls_head_supported(c, rows, n) is ok
    assert (h.gldm_cls_head_workspace_bytes(2, c, rows, n) > 0) is ok
    if not ok:
        p = _host_ptr()
        assert h.gldm_cls_head(p, p, p, p, p, 0.0, 2, c, rows, n, 0, p, 1 << 30, p, p, None) == -3


def test_entries_reject_null_and_non_positive_arguments():
    from graspldm_amd import _lib as L
    h = L.lib()
    p = _host_ptr()
    assert h.gldm_cls_head(None, p, p, p, p, 0.0, 2, 64, 128, 64, 0, p, 1 << 20, p, p, None) == -1
    assert h.gldm_cls_head(p, p, p, p, p, 0.0, 0, 64, 128, 64, 0, p, 1 << 20, p, p, None) == -1
    assert h.gldm_cls_head(p, p, p, p, p, 0.0, 2, 64, 128, 64, 0, None, 1 << 20, p, p, None) == -1
    assert h.gldm_cls_head(p, p, p, p, p, 0.0, 2, 64, 128, 64, 0, p, 4, p, p, None) == -4          # workspace too small
    assert h.gldm_cls_head_workspace_bytes(0, 64, 128, 64) == -1
    assert h.gldm_grasp_scene(None, p, p, None, 0.0, 1.0, 1, 1, 4, 4, p, None) == -1
    assert h.gldm_grasp_scene(p, p, p, None, 0.0, 1.0, 1, 0, 4, 4, p, None) == -1
    assert h.gldm_grasp_scene(p, p, p, None, 0.0, 0.0, 1, 1, 4, 4, p, None) == -1                  # pc_scale = 0
    assert h.gldm_grasp_scene(p, p, p, None, 0.0, float("nan"), 1, 1, 4, 4, p, None) == -1


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_grasps
    return generate_grasps


def test_cli_flags_parse_and_default_to_the_old_behaviour(tmp_path):
    cli = _cli()
    a = cli.parse_args([])
    assert a.classifier_config is None and a.classifier_ckpt is None and a.sort_by_success is False
    sentinel = object()
    assert cli.setup_classifier(a, sentinel) is sentinel           # nothing attached, nothing built
    a = cli.parse_args(["--classifier_config", "c.py", "--classifier_ckpt", "w.ckpt", "--sort_by_success"])
    assert (a.classifier_config, a.classifier_ckpt, a.sort_by_success) == ("c.py", "w.ckpt", True)
    with pytest.raises(SystemExit):
        cli.setup_classifier(cli.parse_args(["--sort_by_success"]), sentinel)
    from graspldm_amd.config import Config
    from graspldm_amd.pipeline import classifier_model_config
    cfg = tmp_path / "cls.py"
    cfg.write_text("model = " + repr(classifier_model_config(64, 12)["model"]) + "\n")
    sec = cli.find_classifier_section(Config.fromfile(str(cfg)))
    assert sec["type"] == "PointsBasedGraspClassifier" and sec["args"]["num_pc_points"] == 76
    nested = tmp_path / "nested.py"
    nested.write_text("model = dict(classifier=" + repr(classifier_model_config(64, 12)) + ")\n")
    assert cli.find_classifier_section(Config.fromfile(str(nested)))["type"] == "PointsBasedGraspClassifier"
