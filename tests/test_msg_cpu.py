"""CPU: multi-scale set abstraction (PointNet2MSG): the class and its reference-shaped state_dict, the shape predicates
(which branches fuse, and that the single-scale predicates answer as they did), the LDS bound against the C entry, and the
two new entry points of the C ABI."""
import ctypes

import pytest
import torch

from conftest import load_schema

# (rows of the grouped input, SharedMLP widths, neighbours) of the five branches of PointNet2MSG.sa_blocks
MSG_BRANCHES = [(6, (32, 32, 64), 32), (6, (64, 64, 128), 64), (6, (64, 96, 128), 128),
                (323, (128, 128, 256), 64), (323, (128, 196, 256), 128)]

# the single-scale shapes of PointNet2SSG (0 and 3 extra channels) and PVCNN2 (width multiplier 1 and 0.5):
# (cin, widths, U) -> fusable, split_plan_ok, split_plan_ok of the layers behind a hoisted first one, split_plan_ok under
# numerics.f32_only() -- the answers of the code before the multi-scale path existed
SINGLE_SCALE = [
    (3, (64, 64, 128), 64, True, True, True, False),
    (6, (64, 64, 128), 64, True, True, True, False),
    (19, (16, 32), 32, True, True, True, False),
    (35, (32, 64), 32, True, True, True, False),
    (67, (64, 128), 32, True, True, True, False),
    (131, (128, 128, 256), 32, True, True, True, False),
    (131, (128, 128, 256), 64, True, True, True, False),
    (131, (128, 256), 32, True, True, True, False),
    (259, (256, 256, 512), 32, False, False, False, False),
    # the multi-scale shapes themselves: the single-scale predicates keep rejecting what they rejected
    (6, (64, 96, 128), 128, False, False, False, False),
    (6, (64, 96, 128), 64, False, False, False, False),
    (323, (128, 196, 256), 128, False, False, False, False),
    (323, (128, 128, 256), 64, False, False, True, False),
]


def test_pointnet2_msg_constructs_with_the_reference_schema():
    """Fails without the feature (the import).  The schema is the reference's PointNet2 built with the MSG tables,
    with_one_hot_shape_id=True, num_shapes=4; num_classes is accepted and ignored."""
    from graspldm_amd.pvcnn import PointNet2, PointNet2MSG
    m = PointNet2MSG(num_classes=7, num_shapes=4)
    assert isinstance(m, PointNet2) and m.with_one_hot_shape_id and m.num_shapes == 4 and m.in_channels == 6
    schema = load_schema("schema_pointnet2_msg.json")
    sd = m.state_dict()
    assert list(sd) == list(schema)
    for k, (shape, dtype) in schema.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == dtype, k
    from graspldm_amd.synthetic import synthetic_state_dict
    m.load_state_dict(synthetic_state_dict(schema, seed=13), strict=True)
    assert list(PointNet2MSG(num_shapes=4).state_dict()) == list(sd)


def test_registries_stay_as_the_reference_has_them():
    from graspldm_amd.grasp_classifier import PointsBasedGraspClassifier
    assert "PointNet2MSG" not in PointsBasedGraspClassifier.SUPPORTED_BASE_NETWORKS
    assert sorted(PointsBasedGraspClassifier.SUPPORTED_BASE_NETWORKS) == ["PVCNN", "PVCNN2"]
    from graspldm_amd.grasp_vae import PcConditionedGraspEncoder
    assert sorted(PcConditionedGraspEncoder.PC_ENCODERS) == ["PVCNN2Encoder", "PVCNNEncoder"]


def test_a_branch_without_an_f32_route_behind_its_split_route_is_not_fused():
    """323 rows into a 256-wide first layer: the hoisted split launch takes it, but were a folded weight beyond the f16
    range there would be no f32 launch to go to (3 + 256 rows exceed its 256): msg_fusable keeps such a branch grouped."""
    from graspldm_amd import numerics
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.sa_pack import msg_fusable, msg_route
    assert msg_route(323, (256, 128, 256), 64) == "pre"
    with numerics.f32_only():
        assert msg_route(323, (256, 128, 256), 64) is None
    assert not msg_fusable(SharedMLP(323, [256, 128, 256], dim=2), 64)


def test_msg_tables_plan():
    from graspldm_amd.pvcnn import PointNet2MSG, sa_plan
    stages, sa_in, width, centers = sa_plan(PointNet2MSG.sa_blocks, 3)
    assert [sum(w[-1] for w in s["pool"]["out_channels"]) if isinstance(s["pool"]["out_channels"][0], list)
            else s["pool"]["out_channels"][-1] for s in stages] == [320, 512, 1024]
    assert width == 1024 and centers == 1
    # the stage inputs the feature-propagation side is sized from (utils.py:116: the reference appends the FEATURE
    # width) and the rows of every stage's grouped input (+ 3 coordinates): what the branch MLPs see
    assert sa_in == [6, 320, 512]
    assert [s["pool"]["in_channels"] + 3 for s in stages] == [6, 323, 515]
    m = PointNet2MSG(num_shapes=4)
    assert [sa.mlps[0].layers[0].weight.shape[1] for sa in m.sa_layers] == [6, 323, 515]
    assert [sa.out_channels for sa in m.sa_layers] == [320, 512, 1024]


@pytest.mark.parametrize("cin,couts,u", MSG_BRANCHES)
def test_every_msg_branch_fuses_in_both_arithmetic_modes(cin, couts, u):
    from graspldm_amd import numerics
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.sa_pack import msg_fusable, msg_route
    mlp = SharedMLP(cin, list(couts), dim=2)
    assert msg_fusable(mlp, u)
    assert msg_route(cin, couts, u) == "pre"                      # SA1: m u / n = 16 .. 64; SA2: 16 .. 32 -> hoisted
    assert msg_route(cin, couts, u, hoist=False) == ("split" if cin == 6 else "pre")   # 323 rows: only the hoisted form
    with numerics.f32_only():
        assert msg_fusable(mlp, u)
        assert msg_route(cin, couts, u) == ("f32" if cin == 6 else "f32_pre")


def test_msg_route_rejects_what_no_kernel_takes():
    from graspldm_amd.sa_pack import msg_fold, msg_route
    assert msg_fold(128) == (64, 2) and msg_fold(256) == (64, 4) and msg_fold(64) == (64, 1) and msg_fold(32) == (32, 1)
    assert msg_route(6, (64, 96, 128), 96) is None                # 64 % U != 0 and no fold
    assert msg_route(6, (64, 96, 120), 64) is None                # last width: no m-tile count
    assert msg_route(6, (64, 512, 128), 64) is None               # hidden width beyond 256
    assert msg_route(6, (32,) * 5, 64) is None
    assert msg_route(515, (256, 512, 1024), 64) is None


@pytest.mark.parametrize("cin,couts,u,fus,split,pre,split_f32", SINGLE_SCALE)
def test_single_scale_predicates_answer_as_before(cin, couts, u, fus, split, pre, split_f32):
    from graspldm_amd import numerics
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.sa_pack import fusable, split_plan_ok
    couts = list(couts)
    assert fusable(SharedMLP(cin, couts, dim=2), u) is fus
    assert split_plan_ok([cin] + couts[:-1], couts, u) is split
    assert split_plan_ok(couts[:-1], couts[1:], u) is pre
    with numerics.f32_only():
        assert split_plan_ok([cin] + couts[:-1], couts, u) is split_f32


def test_tables_of_the_single_scale_shapes_are_packed_as_before():
    """The wider padding rule (96 -> 128, 196 -> 256) is the identity on every width the kernels took before."""
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.sa_pack import SaMlpPlan, _f32_width, _plane_width
    for c in (32, 64, 128, 256):
        assert _plane_width(c) == c
    assert [_plane_width(c) for c in (16, 48, 96, 196)] == [32, 64, 128, 256]
    for c in (16, 32, 64, 128, 192, 256):
        assert _f32_width(c) == c
    assert _f32_width(96) == 128 and _f32_width(196) == 256
    plan = SaMlpPlan(SharedMLP(131, [128, 128, 256], dim=2).eval(), "cpu")
    assert list(plan.f32.cin_pad) == [160, 128, 128] and list(plan.f32.cout) == [128, 128, 256]
    split = plan._split_plan()
    assert list(split.cin_pad) == [160, 128, 128] and list(split.cout) == [128, 128, 256]
    plan = SaMlpPlan(SharedMLP(19, [16, 32], dim=2).eval(), "cpu")
    assert list(plan.f32.cin_pad) == [32, 16] and list(plan.f32.cout) == [16, 32]
    assert list(plan._split_plan().cin_pad) == [32, 32] and list(plan._split_plan().cout) == [32, 32]
    # the multi-scale widths: zero rows, zero bias behind the real ones
    plan = SaMlpPlan(SharedMLP(6, [64, 96, 128], dim=2).eval(), "cpu")
    assert list(plan.f32.cout) == [64, 128, 128] and list(plan.f32.cin_pad) == [32, 64, 128]
    pre = plan._pre_plan()
    assert list(pre.table.cout) == [128, 128] and list(pre.table.cin_pad) == [64, 128]


def _host_ptr():
    buf = (ctypes.c_float * 16)()
    _host_ptr.keep = getattr(_host_ptr, "keep", []) + [buf]
    return ctypes.cast(buf, ctypes.c_void_p)


def test_lds_bound_agrees_with_the_c_entry():
    """The split routes carry launch_sa3's bound: planes (8192 bytes per 32-row block of hi + lo planes) + 64 +
    cout_last * 8 * 4 bytes <= 160 KiB = 163840.  Plane regions come in sizes of at most 9 + 8 blocks, so the bound bites
    through the bytes behind them: 8 + 8 blocks = 131072 with a 1024-row last layer (+ 32832) is 64 bytes over, with a
    1008-row one 448 under, and one plane region less (4 + 8 blocks) fits.  A shape over the limit is rejected by the
    predicate and by both C entries, which answer GLDM_ERR_UNSUPPORTED before anything is launched (non-null dummy
    pointers, never dereferenced)."""
    from graspldm_amd import _lib as L
    from graspldm_amd.sa_pack import msg_route, sa3_takes
    assert sa3_takes(256, [256, 1008], 64) and not sa3_takes(256, [256, 1024], 64) and sa3_takes(128, [256, 1024], 64)
    assert sa3_takes(256, [256, 1008], 64, pre=True) and not sa3_takes(256, [256, 1024], 64, pre=True)
    # msg_route asks sa3_takes; it also keeps pooled rows to the 256 the fused kernels have run, where the widest plane
    # regions fit: 8 + 8 blocks + 64 + 256 * 32 = 139328 bytes
    assert msg_route(253, (256, 256), 64, hoist=False) == "split" and msg_route(6, (256, 256, 256), 64) == "pre"
    assert msg_route(6, (256, 256, 1008), 64) is None and msg_route(6, (256, 256, 1024), 64) is None
    h = L.lib()
    p = _host_ptr()
    arr = ctypes.c_int32 * 2
    gain = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    args = lambda cin_pad, cout: (2, ctypes.cast(arr(*cin_pad), ctypes.c_void_p), ctypes.cast(arr(*cout), ctypes.c_void_p),
                                  ctypes.cast(arr(0, 0), ctypes.c_void_p), ctypes.cast(arr(0, 0), ctypes.c_void_p),
                                  ctypes.cast(gain, ctypes.c_void_p))
    assert h.gldm_sa_mlp_forward_f16x2(p, p, p, p, p, 1, 253, 64, 8, 64, *args([256, 256], [256, 1024]), p, None) == -3
    assert h.gldm_sa_mlp_forward_f16x2_pre(p, p, p, 0, p, p, 0, 1, 64, 8, 64, *args([256, 256], [256, 1024]), p, None) == -3


def test_new_entry_points_are_exported_and_check_their_arguments():
    """Fails without the feature (the symbol lookup)."""
    from graspldm_amd import _lib as L
    h = L.lib()
    assert "gldm_ball_query_multi" in L._SIGNATURES and "gldm_group_max_concat" in L._SIGNATURES
    p = _host_ptr()
    radius, u = (ctypes.c_float * 4)(0.1, 0.2, 0.3, 0.4), (ctypes.c_int32 * 4)(8, 8, 8, 8)
    outs = (ctypes.c_void_p * 4)(p.value, p.value, p.value, p.value)
    assert h.gldm_ball_query_multi(None, p, 1, 8, 2, 1, radius, u, outs, None) == -1
    assert h.gldm_ball_query_multi(p, p, 1, 0, 2, 1, radius, u, outs, None) == -1
    assert h.gldm_ball_query_multi(p, p, 1, 8, 2, 0, radius, u, outs, None) == -3
    assert h.gldm_ball_query_multi(p, p, 1, 8, 2, 5, radius, u, outs, None) == -3
    u[2] = 0
    assert h.gldm_ball_query_multi(p, p, 1, 8, 2, 3, radius, u, outs, None) == -1
    assert h.gldm_group_max_concat(None, 1, 4, 8, 2, p, 0, 4, None) == -1
    assert h.gldm_group_max_concat(p, 1, 4, 8, 2, p, 1, 4, None) == -1      # rows c0 .. c0 + c beyond ctot
    assert h.gldm_group_max_concat(p, 1, 4, 8, 3, p, 0, 4, None) == -3      # h outside {1, 2, 4}


def test_backend_rejects_cpu_tensors():
    from graspldm_amd.backend import _backend
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _backend.ball_query_multi(torch.zeros(1, 3, 4), torch.zeros(1, 3, 8), [0.1, 0.2], [2, 4])
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _backend.group_max_concat(torch.zeros(1, 4, 8), 2, torch.zeros(1, 4, 4), 0)
