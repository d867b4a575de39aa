"""CPU: the f64 restatements of grasp clearance / contacts / diverse selection on cases derivable by hand, the Python
predicates pinned to the C entries' status codes, GraspSelection's validation and the CLI's selection errors."""
import ctypes
import math
import os
import sys

import pytest
import torch

from conftest import ROOT

import grasp_select_ref as ref

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _identity(n=1):
    return torch.eye(4, dtype=torch.float64).repeat(1, n, 1, 1)


def _geometry():
    from graspldm_amd import gripper
    return gripper.OPEN_SEGMENTS, gripper.SWEEP_SEGMENTS


def test_sweep_segments_are_the_reference_values():
    from graspldm_amd import gripper
    sweep = torch.tensor(gripper.SWEEP_SEGMENTS, dtype=torch.float64)
    assert sweep.shape == (2, 2, 3)
    assert torch.equal(sweep[:, 0, 0], torch.tensor([0.041, 0.041], dtype=torch.float64))
    assert torch.equal(sweep[:, 1, 0], -sweep[:, 0, 0])
    assert torch.allclose(sweep[:, :, 2], torch.tensor([[0.108169998] * 2, [0.098169998] * 2], dtype=torch.float64), atol=0, rtol=0)
    assert gripper.SWEEP_RADIUS == 0.006 and gripper.BODY_RADIUS == 0.006
    assert len(gripper.OPEN_SEGMENTS) == 4                      # untouched


def test_restatement_point_on_the_wrist_axis_has_clearance_zero():
    body, sweep = _geometry()
    scene = torch.tensor([[[0.0, 0.0, 0.03]]], dtype=torch.float64)
    clear, contacts, _, _ = ref.clearance(scene, _identity(), body, sweep, 0.006, 0.05)
    assert float(clear) == 0.0 and int(contacts) == 0


def test_restatement_point_beside_the_left_finger():
    from graspldm_amd import gripper
    body, sweep = _geometry()
    mid_z = 0.5 * (gripper.CENTER_LEFT[2] + gripper.BOTTOM_LEFT[2])
    scene = torch.tensor([[[gripper.CENTER_LEFT[0] + 0.01, 0.0, mid_z]]], dtype=torch.float64)
    clear, contacts, _, _ = ref.clearance(scene, _identity(), body, sweep, 0.006, 0.05)
    assert abs(float(clear) - 0.01) < 1e-15 and int(contacts) == 0
    # the same point seen from a moved and turned gripper: q = R^T (p - t)
    H = _identity()
    H[0, 0, :3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    H[0, 0, :3, 3] = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    moved = scene @ H[0, 0, :3, :3].T + H[0, 0, :3, 3]
    clear, _, _, _ = ref.clearance(moved, H, body, sweep, 0.006, 0.05)
    assert abs(float(clear) - 0.01) < 1e-15
    # and the cap
    far = torch.tensor([[[1.0, 1.0, 1.0]]], dtype=torch.float64)
    clear, contacts, _, _ = ref.clearance(far, _identity(), body, sweep, 0.006, 0.05)
    assert float(clear) == 0.05 and int(contacts) == 0


def test_restatement_point_at_the_fingertip_midline_is_one_contact():
    body, sweep = _geometry()
    scene = torch.tensor([[[0.0, 0.0, 0.108169998], [0.0, 0.02, 0.108169998]]], dtype=torch.float64)
    _, contacts, _, sweep_d = ref.clearance(scene, _identity(), body, sweep, 0.006, 0.05)
    assert int(contacts) == 1
    assert float(sweep_d[0, 0, 0]) < 1e-11 and abs(float(sweep_d[0, 0, 1]) - 0.02) < 1e-9
    _, none, _, no_d = ref.clearance(scene, _identity(), body, [], 0.006, 0.05)            # Ss = 0
    assert int(none) == 0 and no_d is None


def test_restatement_diverse_picks_the_ends_of_three_collinear_poses():
    from graspldm_amd import gripper
    H = torch.eye(4).repeat(3, 1, 1)
    H[:, 0, 3] = torch.tensor([0.0, 0.1, 0.3])
    ctrl = gripper.control_points(16)
    score = torch.tensor([3.0, 2.0, 1.0])
    idx, n, gaps, margins = ref.diverse(H, score, [True] * 3, ctrl, 2)
    assert idx == [0, 2] and n == 2
    assert gaps[0] == math.inf and abs(gaps[1] - 0.3) < 1e-7          # pure translation: D = |dt|^2
    assert len(margins) == 1 and abs(margins[0] - (0.09 - 0.01) / 0.09) < 1e-6
    assert ref.topk(score, [True] * 3, 2) == ([0, 1], 2)
    assert ref.topk(score, [False, True, True], 3) == ([1, 2, -1], 2)
    # min_separation cuts the sequence: nothing is 0.4 m from pose 0
    idx, n, gaps, _ = ref.diverse(H, score, [True] * 3, ctrl, 3, min_separation=0.4)
    assert idx == [0, -1, -1] and n == 1 and gaps == [math.inf, 0.0, 0.0]
    # D of the restatement against the closed form around the centroid (what the kernel evaluates), random poses
    from graspldm_amd.synthetic import _random_rotation
    gen = torch.Generator().manual_seed(3)
    P = torch.eye(4, dtype=torch.float64).repeat(6, 1, 1)
    for i in range(6):
        P[i, :3, :3] = _random_rotation(gen).double()
        P[i, :3, 3] = 0.1 * torch.randn(3, generator=gen, dtype=torch.float64)
    D = ref.pose_distance(P, ctrl)
    c = ctrl.double()
    cb = c.mean(0)
    Me = (c - cb).T @ (c - cb) / c.shape[0]
    dR = P[:, None, :3, :3] - P[None, :, :3, :3]
    dt = P[:, None, :3, 3] - P[None, :, :3, 3]
    w = dt + dR @ cb
    closed = (w * w).sum(-1) + torch.einsum("abij,jk,abik->ab", dR, Me, dR)
    assert torch.allclose(D, closed, rtol=1e-12, atol=1e-18)


def test_predicates_are_pinned_to_the_entries_status():
    """supported() <-> not GLDM_ERR_UNSUPPORTED: the entries check their envelope before any pointer (null pointers inside
    the envelope are GLDM_ERR_INVALID_ARG, so no launch happens here)."""
    from graspldm_amd import _lib as L
    from graspldm_amd import grasp_select as gs
    h = L.lib()
    assert h.gldm_grasp_clearance_chunk() == gs.CHUNK
    f = ctypes.c_float
    for ns, sb, ss in [(1, 1, 0), (1 << 24, 8, 8), ((1 << 24) + 1, 4, 2), (1000, 0, 2), (1000, 9, 2), (1000, 4, 9), (1000, 4, 0)]:
        status = h.gldm_grasp_clearance(None, None, 2, 3, ns, None, sb, None, ss, f(0.006), f(0.05), None, None, None)
        assert (status != -3) == gs.clearance_supported(ns, sb, ss), (ns, sb, ss, status)
        assert status in (-1, -3)
    for g, k, np_ in [(1, 1, 1), (2048, 2048, 64), (2049, 5, 16), (20, 21, 16), (20, 20, 65), (20, 5, 16)]:
        status = h.gldm_select_grasps(None, None, None, 2, g, None, np_, k, 1, f(0.0), None, None, None, None)
        assert (status != -3) == gs.select_supported(g, k, np_), (g, k, np_, status)
        assert status in (-1, -3)
    # non-positive counts are invalid arguments, not unsupported shapes
    assert h.gldm_grasp_clearance(None, None, 0, 3, 10, None, 4, None, 2, f(0.006), f(0.05), None, None, None) == -1
    assert h.gldm_select_grasps(None, None, None, 2, 20, None, 16, 0, 0, f(0.0), None, None, None, None) == -1
    assert h.gldm_select_grasps(None, None, None, 2, 20, None, 16, 5, 2, f(0.0), None, None, None, None) == -1   # mode


def test_python_layer_rejects_cpu_tensors_and_shapes_outside_the_envelope():
    from graspldm_amd import grasp_select as gs
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        gs.grasp_clearance(torch.zeros(1, 8, 3), torch.eye(4).repeat(1, 2, 1, 1))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        gs.select_grasps(torch.eye(4).repeat(1, 2, 1, 1), torch.zeros(1, 2))
    assert not gs.clearance_supported(0, 4, 2) and not gs.select_supported(20, 0, 16)


def test_grasp_selection_validates_its_fields():
    from graspldm_amd.grasp_select import GraspSelection
    s = GraspSelection()
    assert not s.needs_clearance and not s.needs_success and s.body_radius == 0.006 and s.score_by == "confidence"
    assert GraspSelection(collision_free=True).needs_clearance and GraspSelection(min_contacts=1).needs_clearance
    assert GraspSelection(min_success=0.5).needs_success and GraspSelection(score_by="product").needs_success
    for bad in (dict(min_confidence=1.5), dict(min_confidence=-0.1), dict(min_success=2.0), dict(min_success="x"),
                dict(body_radius=-1.0), dict(body_radius=float("nan")), dict(min_contacts=-1), dict(min_contacts=1.5),
                dict(top_k=0), dict(top_k=2.0), dict(min_separation=-0.1), dict(min_separation=float("inf")),
                dict(score_by="quality")):
        with pytest.raises(ValueError):
            GraspSelection(**bad)
    with pytest.raises(Exception):
        s.top_k = 3                                            # frozen


def test_cli_selection_flags_and_errors():
    import generate_grasps as cli
    old = cli.parse_args(["--synthetic", "64", "--mode", "LDM"])
    assert cli.build_selection(old) is None and cli.selection_kwargs(old, None, 0) == {}
    new = cli.parse_args(["--synthetic", "64", "--mode", "LDM", "--collision_free", "--top_k", "4", "--diverse",
                          "--min_separation", "0.02", "--min_confidence", "0.3", "--min_contacts", "2"])
    sel = cli.build_selection(new)
    assert (sel.collision_free, sel.top_k, sel.diverse, sel.min_separation, sel.min_confidence, sel.min_contacts,
            sel.score_by) == (True, 4, True, 0.02, 0.3, 2, "confidence")
    added = {"scene_file", "collision_free", "min_contacts", "min_confidence", "min_success", "top_k", "diverse", "min_separation"}
    for k, v in vars(old).items():
        if k not in added:
            assert getattr(new, k) == v, k
    with pytest.raises(SystemExit, match="classifier_config"):
        cli.main(["--synthetic", "64", "--mode", "LDM", "--min_success", "0.5"])
    with pytest.raises(SystemExit, match="top_k"):
        cli.main(["--synthetic", "64", "--mode", "LDM", "--top_k", "0"])
    with pytest.raises(SystemExit):
        cli.main(["--synthetic", "64", "--mode", "LDM", "--min_confidence", "1.5"])
