"""No device: the documented bounds of the attention cores, the classifier head and the neighbour search pinned from both
sides through the host-only queries, the Python predicates pinned to the same answers on the same rows, and the tables of
tests/additive_envelope_cases.py checked for completeness against the sources (an instantiation without a case fails here).
The rows that need real pointers (the entries without a bytes query) are in tests/test_additive_envelope_gpu.py."""
import inspect
import re

import pytest
import torch

import additive_envelope_cases as C


def _lib():
    from graspldm_amd import _lib as L
    return L.lib()


# ------------------------------------------------------------------------------------------------------------------ bounds
def test_point_attention_bounds_from_both_sides():
    from graspldm_amd import attention
    h = _lib()
    for c, ok in C.ATTN_C_ROWS:
        assert (h.gldm_point_attention_workspace_bytes(1, c, 64) > 0) == ok, c
        assert attention.supported(c) == attention.supported(c, 64) == ok, c
    for n, ok in C.ATTN_N_ROWS:
        assert (h.gldm_point_attention_workspace_bytes(1, 32, n) > 0) == ok, n
        assert attention.supported(32, n) == ok, n
        assert attention.fused_supported(32, n) == ok, n
    for c, n in [(c, n) for c, ok in C.ATTN_C_ROWS if not ok for n in (32, 4096)] + [(16, n) for n, ok in C.ATTN_N_ROWS if not ok]:
        assert h.gldm_point_attention_workspace_bytes(1, c, n) == -1, (c, n)
        with pytest.raises(NotImplementedError):
            attention.check_supported(c, n)
    assert h.gldm_point_attention_workspace_bytes(0, 32, 64) == -1
    # the two maxima together, and the cap: one cloud's need where that is more than 256 MiB would hold
    assert 0 < h.gldm_point_attention_workspace_bytes(1, 1024, 4096) <= 256 << 20
    for c, ok in C.FUSED_C_ROWS:
        assert attention.fused_supported(c, 64) == ok, c
    assert attention.FUSED_MAX_C == 128 and attention.MAX_GROUP_CHANNELS == 128
    attention.check_supported(1024, 32, num_groups=8)              # 128 channels per group: the norm's bound
    with pytest.raises(NotImplementedError):
        attention.check_supported(1024, 32, num_groups=4)


def test_chunk_case_holds_two_clouds_of_three():
    """The chunk loop's case: b = 3 asks for two clouds' blocks, so the launch runs as chunks of 2 and 1."""
    h = _lib()
    b, c, n = C.CORE_CHUNK_CASE
    one = h.gldm_point_attention_workspace_bytes(1, c, n)
    assert one == 89_671_936
    assert h.gldm_point_attention_workspace_bytes(b, c, n) == 2 * one <= 256 << 20 < 3 * one


def test_cls_head_bounds_from_both_sides():
    from graspldm_amd.grasp_classifier import HEAD_MAX_C, HEAD_MAX_N, HEAD_MAX_ROWS, cls_head_supported
    h = _lib()
    assert (HEAD_MAX_C, HEAD_MAX_ROWS, HEAD_MAX_N) == (2048, 512, 1 << 20)
    for c, ok in C.HEAD_C_ROWS:
        assert (h.gldm_cls_head_workspace_bytes(1, c, 128, 64) > 0) == ok, c
        assert cls_head_supported(c, 128, 64) == ok, c
    for rows, ok in C.HEAD_ROWS_ROWS:
        assert (h.gldm_cls_head_workspace_bytes(1, 64, rows, 64) > 0) == ok, rows
        assert cls_head_supported(64, rows, 64) == ok, rows
    for n, ok in C.HEAD_N_ROWS:
        assert (h.gldm_cls_head_workspace_bytes(1, 64, 128, n) > 0) == ok, n
        assert cls_head_supported(64, 128, n) == ok, n
    assert h.gldm_cls_head_workspace_bytes(0, 64, 128, 64) == -1
    assert h.gldm_cls_head_workspace_bytes(1, 2064, 128, 64) == h.gldm_cls_head_workspace_bytes(1, 64, 528, 64) == -1
    # one f32 partial per (scene, 64-point tile), rounded up to 256 bytes
    for b, c, rows, n in C.HEAD_CASES:
        assert cls_head_supported(c, rows, n)
        assert h.gldm_cls_head_workspace_bytes(b, c, rows, n) == (4 * b * ((n + 63) // 64) + 255) // 256 * 256
    assert h.gldm_cls_head_workspace_bytes(1, 2048, 512, 1 << 20) == 4 * (1 << 14)


def test_knn_radius_bounds_from_both_sides():
    h = _lib()
    for n, ok in C.KNN_N_ROWS:
        assert (h.gldm_knn_radius_workspace_bytes(1, n) >= 0) == ok, n
    assert h.gldm_knn_radius_workspace_bytes(1, 0) == h.gldm_knn_radius_workspace_bytes(0, 64) == -1     # GLDM_ERR_INVALID_ARG
    assert h.gldm_knn_radius_workspace_bytes(1, (1 << 20) + 1) == -3                                        # GLDM_ERR_UNSUPPORTED


def test_every_case_lies_inside_the_predicates():
    from graspldm_amd import attention
    from graspldm_amd.grasp_select import clearance_supported, select_supported
    for b, c, n in C.FUSED_CASES + [C.FUSED_RANGE_CASE]:
        assert attention.fused_supported(c, n) and attention.supported(c, n), (c, n)      # both entries take them
    for (b, c, n), _, _ in C.CORE_CASES:
        assert attention.supported(c, n) and not attention.fused_supported(c, n), (c, n)
    assert attention.supported(*C.CORE_CHUNK_CASE[1:])
    for sb, ss in C.CLEARANCE_SEGMENTS:
        assert clearance_supported(C.CLEARANCE_SHAPE[2], sb, ss)
        assert not clearance_supported(C.CLEARANCE_SHAPE[2], sb + 1, ss) and not clearance_supported(C.CLEARANCE_SHAPE[2], sb, 9)
    for b, g, k, _ in C.SELECT_ENVELOPE_CASES:
        assert select_supported(g, k, C.SELECT_CONTROL_POINTS)
        assert not select_supported(g, k, C.SELECT_CONTROL_POINTS + 1) and not select_supported(g, g + 1, 16)
    assert not select_supported(2049, 9, 16)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_every_instantiation_has_a_case():
    import test_voxel_attention_gpu as voxel
    # gldm_pointwise_small: every cin its dispatch names
    assert C.small_cins() == sorted(C.SMALL_CINS) and len(C.SMALL_CINS) >= 7
    text = (C.CSRC / "pointwise_small.hip").read_text()
    doc = re.search(r"cin in \{([0-9, ]+)\}", (C.CSRC.parents[1] / "include" / "gldm.h").read_text())
    assert doc and sorted(int(v) for v in doc.group(1).split(",")) == C.small_cins()
    # gldm_pointwise_rows: every hout of launch_rows<1 .. 8>
    assert "if constexpr (HO > 8)" in text and "launch_rows<1>" in text
    assert {h for _, _, h, _ in C.ROWS_CASES} == set(range(1, 9))
    # the fused core: attn_fused_kernel<2 .. 8, *>, c = 32 .. 128 in steps of 16, in both forms (the tests run every shape
    # at exact_f32 = 0 and 1)
    fused = (C.CSRC / "point_attention_fused.hip").read_text()
    assert "if constexpr (CT > 8)" in fused and "launch_fused<2, true>" in fused and "launch_fused<2, false>" in fused
    assert {c for _, c, _ in C.FUSED_CASES + voxel.SHAPES} == set(range(32, 129, 16))
    assert {c for _, c, _ in C.FUSED_CASES} >= {80, 96, 112}
    assert any(n == 32 for _, _, n in C.FUSED_CASES) and (1, 128, 4096) in C.FUSED_CASES
    # the head: the pass loop, the masked m-tiles, the half K block and both maxima
    head = C.HEAD_CASES
    assert any(rows < 128 for _, _, rows, _ in head)
    assert any(rows % 128 and rows > 128 for _, _, rows, _ in head)
    assert any(rows == 512 for _, _, rows, _ in head)
    assert any(c % 32 == 16 and c > 16 for _, c, _, _ in head)
    assert any(c == 2048 for _, c, _, _ in head)
    assert any(n % 64 == 1 and n > 64 for _, _, _, n in head)
    assert C.HEAD_BATCH_CASE in head and C.HEAD_BATCH_CASE[0] == 3
    # the materialised core: c above 768 at the smallest n, the largest launch, a chunk of more than one cloud
    shapes = [s for s, _, _ in C.CORE_CASES]
    assert {(2, 1024, 32), (1, 1008, 64), (1, 1024, 4096)} <= set(shapes)
    # the norms: both sides of the grid switch of gldm_groupnorm_affine, the bounds of r; channel counts per group that
    # leave waves of the _sum kernel without a channel; a row of a single quad
    norm = (C.CSRC / "voxel_norm.hip").read_text()
    assert "quads >= 4096 ? 4 : 1" in norm
    quads = {r: r ** 3 // 4 for _, _, r in C.AFFINE_CASES}
    assert any(q >= 4096 for q in quads.values()) and any(q < 4096 for q in quads.values()) and {2, 64} <= set(quads)
    assert {c // g for _, c, _, g in C.SWISH_CASES} >= {1, 3, 128} and any(n == 4 for _, _, n, _ in C.SWISH_CASES)
    # selection: kMaxSeg segments in both families, an empty sweep family, the most control points, k = g above 256
    assert (8, 8) in C.CLEARANCE_SEGMENTS and (8, 0) in C.CLEARANCE_SEGMENTS and C.SELECT_CONTROL_POINTS == 64
    assert any(k == g > 256 for _, g, k, _ in C.SELECT_ENVELOPE_CASES) and any(g == 2048 for _, g, _, _ in C.SELECT_ENVELOPE_CASES)
    assert {n for _, n, _ in C.LINEAR_CASES} >= {4, 16384}


def test_every_table_has_a_gpu_run():
    """Each table of the cases file is named by the GPU file's parametrisation."""
    import test_additive_envelope_gpu as gpu
    src = inspect.getsource(gpu)
    for table in ("HEAD_CASES", "HEAD_KINDS", "HEAD_BATCH_CASE", "HEAD_MODULE_ROWS", "FUSED_CASES", "FUSED_KINDS", "FUSED_RANGE_CASE",
                  "RANGE_SCALES", "CORE_CASES", "CORE_CHUNK_CASE", "ROWS_CASES", "SMALL_CINS", "SMALL_COUTS", "SMALL_NS",
                  "LINEAR_CASES", "AFFINE_CASES", "SWISH_CASES", "CLEARANCE_SEGMENTS", "SELECT_ENVELOPE_CASES"):
        assert f"C.{table}" in src, table


# ------------------------------------------------------------------------------------------------- inputs of the GPU cases
def test_head_kinds_make_the_pass_loop_decide():
    from test_classifier_gpu import head_ref
    f64 = lambda args: [t.double() if torch.is_tensor(t) else t for t in args]   # noqa: E731
    for shape in C.HEAD_CASES:
        rows = shape[2]
        last, first = C.make_head(*shape, kind="last_rows"), C.make_head(*shape, kind="first_rows")
        assert last[1].shape == (rows, shape[1]) and last[3].shape == (rows,)
        assert (last[3][:rows - 16] == 0).all() and (last[3][rows - 16:] != 0).all()
        assert (first[3][16:] == 0).all() and (first[3][:16] != 0).all()
        a, b = head_ref(*f64(first)), head_ref(*f64(C.first_rows_head(first)))       # the 16-row head of the same rows
        assert (a - b).abs().max() <= 1e-12 * max(1.0, float(a.abs().max()))


def test_clearance_case_meets_its_precondition():
    """In f64 no point lies within the bar of a tube radius (allowed count zero), no contact within the bar of the finger
    plane, no normal within 1e-6 of the friction cone; the 8 + 8 case has contacts on both sides."""
    import math

    import grasp_select_ref as ref
    import normals_ref
    import test_grasp_select_gpu as base
    scene, normals, H = C.clearance_inputs()
    bar = base._bar(scene, H)
    for sb, ss in C.CLEARANCE_SEGMENTS:
        body, sweep = C.segments(sb, ss)
        assert len(body) == sb and len(sweep) == ss
        want, contacts, body_d, sweep_d = ref.clearance(scene, H, body, sweep, base.R_SWEEP, base.CAP)
        assert int(((body_d - base.R_BODY).abs() <= bar[..., None]).sum()) == 0
        if ss:
            assert int(((sweep_d - base.R_SWEEP).abs() <= bar[..., None]).sum()) == 0
            cos_f = math.cos(math.radians(30.0))
            w = normals_ref.contact_normals(scene, normals, H, sweep, base.R_SWEEP, cos_f)
            assert int((((w["axis_dot"] - cos_f).abs() <= 1e-6) & w["nonzero"]).sum()) == 0
            assert int((w["hit"] & (w["qx"].abs() <= bar[..., None])).sum()) == 0
            assert int(contacts.sum()) > 0 and (w["side"].sum(dim=(0, 1)) > 0).all()
            # the added segments count: fewer contacts with the gripper's own two
            assert int(ref.clearance(scene, H, body, sweep[:2], base.R_SWEEP, base.CAP)[1].sum()) < int(contacts.sum())
        # the added body segments decide some pose's clearance
        assert (ref.clearance(scene, H, body[:4], sweep, base.R_SWEEP, base.CAP)[0] > want).any()
        assert (want < base.CAP).any()


def test_selection_cases_meet_their_precondition():
    """The f64 greedy's margins (best against second-best m, relative) are >= 1e-4 at every pick, with 64 control points."""
    import grasp_select_ref as ref
    import test_grasp_select_gpu as base
    from graspldm_amd import gripper
    ctrl = gripper.control_points(C.SELECT_CONTROL_POINTS)
    assert ctrl.shape == (64, 3)
    for b, g, k, seed in C.SELECT_ENVELOPE_CASES:
        H, score, keep = base._selection_inputs(b, g, seed)
        for mask in (keep, None):
            for c in range(b):
                kept = [True] * g if mask is None else mask[c].tolist()
                margins = ref.diverse(H[c], score[c], kept, ctrl, k)[3]
                assert min(margins) >= 1e-4, (b, g, k, c, min(margins))
