"""CPU: host side of voxel attention inside PVConv -- the state_dict schema of PVCNN2(use_attention=True) against the
reference's (fixture captured from it), where the plans put the block, the one shape gate, the switches of the encoder and
the pipeline config, the status codes of the three new entry points (returned before anything is launched), and the
switch-off modules unchanged."""
import ctypes

import pytest

from conftest import load_schema

_HOST = (ctypes.c_char * 4096)()
ATTN_PREFIX = "sa_layers.1.0.voxel_layers.6."
ATTN_KEYS = {ATTN_PREFIX + f"{m}.{p}" for m in ("q", "k", "v", "out", "norm") for p in ("weight", "bias")}


def _host_ptr(offset=0):
    """A non-null, 16-byte aligned (+ offset) host pointer for calls that return a status before anything is dereferenced."""
    return ctypes.c_void_p((ctypes.addressof(_HOST) + 15) // 16 * 16 + offset)


def test_pvcnn2_schema_with_attention_matches_reference():
    from graspldm_amd.attention import Attention
    from graspldm_amd.pvcnn import PVCNN2, SE3d
    from graspldm_amd.synthetic import synthetic_state_dict
    ref = load_schema("schema_pvcnn2_attn.json")
    net = PVCNN2(use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    sd = net.state_dict()
    assert set(sd) == set(ref), (sorted(set(ref) - set(sd))[:5], sorted(set(sd) - set(ref))[:5])
    assert {(k, tuple(v.shape), v.dtype) for k, v in sd.items()} == {(k, s, d) for k, (s, d) in ref.items()}
    net.load_state_dict(synthetic_state_dict(ref, seed=0), strict=True)
    off = PVCNN2(width_multiplier=0.5, voxel_resolution_multiplier=0.5).state_dict()
    # the block's ten keys are the only difference from the switch-off net (the block replaces a Swish, which has none; SE
    # keeps index 7)
    assert {k for k in sd if any(f".{m}." in k for m in ("q", "k", "v", "out", "norm"))} == ATTN_KEYS
    assert set(sd) - set(off) == ATTN_KEYS and set(off) <= set(sd)
    layers = net.sa_layers[1][0].voxel_layers
    assert isinstance(layers[6], Attention) and isinstance(layers[7], SE3d)
    assert tuple(layers[6].q.weight.shape) == (32, 32, 1, 1, 1) and layers[6].norm.num_groups == 8


def test_plans_put_attention_on_stage_one_block_zero_only():
    from graspldm_amd.attention import Attention
    from graspldm_amd.pvcnn import PVCNN2, fp_plan, sa_plan
    stages, sa_in, width, _ = sa_plan(PVCNN2.sa_blocks, 0, use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    flags = [[c["attention"] for c in st["convs"]] for st in stages]
    assert flags == [[False], [True], [False], []]
    assert (stages[1]["convs"][0]["cout"], stages[1]["convs"][0]["resolution"]) == (32, 8)
    assert not any(c["attention"] for st in sa_plan(PVCNN2.sa_blocks, 0)[0] for c in st["convs"])
    # the reference's rule for the propagation stages reads a shadowed local and is never true (utils.py:217-222)
    fp_stages, _ = fp_plan(PVCNN2.fp_blocks, width, sa_in, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    assert not any(c.get("attention", False) for st in fp_stages for c in st["convs"])
    net = PVCNN2(use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5)
    assert not any(isinstance(m, Attention) for m in net.fp_layers.modules())
    assert sum(isinstance(m, Attention) for m in net.sa_layers.modules()) == 1


def test_the_gate():
    from graspldm_amd.attention import check_voxel_supported, voxel_supported
    from graspldm_amd.pvcnn import PVConv
    for c, r in [(32, 4), (64, 12), (128, 16), (256, 8)]:
        check_voxel_supported(c, r)
        assert voxel_supported(c, r)
    with pytest.raises(NotImplementedError, match=r"\(16, 1728\)"):
        check_voxel_supported(16, 12)
    for r in (6, 10, 14, 20):
        assert not voxel_supported(64, r)
        with pytest.raises(NotImplementedError, match=rf"\(64, {r ** 3}\)"):
            check_voxel_supported(64, r)
    for c in (24, 40, 1040):
        with pytest.raises(NotImplementedError):
            check_voxel_supported(c, 8)
    # PVConv asks the gate, and only with the switch on
    with pytest.raises(NotImplementedError, match=r"\(16, 1728\)"):
        PVConv(16, 16, 3, resolution=12, use_attention=True)
    with pytest.raises(NotImplementedError, match=r"\(64, 216\)"):
        PVConv(64, 64, 3, resolution=6, use_attention=True)
    PVConv(16, 16, 3, resolution=12), PVConv(64, 64, 3, resolution=6), PVConv(16, 256, 3, resolution=8, use_attention=True)


def test_encoder_takes_the_switch_from_half_width():
    from graspldm_amd.attention import Attention
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    enc = PVCNN2Encoder(scale_channels=0.5, use_local_attention=True)
    block = enc.pvcnn_modules.sa_layers[1][0]
    assert isinstance(block.voxel_layers[6], Attention) and (block.out_channels, block.resolution) == (32, 12)
    off = PVCNN2Encoder(scale_channels=0.5)
    assert not any(isinstance(m, Attention) for m in off.modules())
    with pytest.raises(NotImplementedError, match=r"\(16, 1728\).*32\.\.1024"):     # the quarter-width default: C = 16, r = 12
        PVCNN2Encoder(use_local_attention=True)


def test_pipeline_config_takes_the_switch():
    from graspldm_amd.pipeline import fpc_model_config
    enc = lambda **kw: fpc_model_config(**kw)["vae"]["model"]["args"]["pc_encoder_config"]["args"]   # noqa: E731
    assert enc(encoder="PVCNN2Encoder", use_local_attention=True)["use_local_attention"] is True
    assert "use_local_attention" not in enc(encoder="PVCNN2Encoder") and "use_local_attention" not in enc()
    assert "use_local_attention" not in enc(encoder="PVCNN2Encoder", use_global_attention=True)
    with pytest.raises(ValueError):
        enc(use_local_attention=True)


def test_classifier_config_passes_the_switch_through():
    from graspldm_amd.attention import Attention
    from graspldm_amd.builder import build_model_from_cfg
    from graspldm_amd.pipeline import classifier_model_config
    cfg = classifier_model_config(1024, 64, "PVCNN2", dict(use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5))
    model = build_model_from_cfg(cfg)
    assert isinstance(model.base_network.sa_layers[1][0].voxel_layers[6], Attention)


@pytest.mark.parametrize("c,n", [(16, 64), (32, 32), (32, 64), (48, 96), (128, 4096), (144, 64), (64, 48), (64, 4128), (40, 64), (256, 512)])
def test_fused_core_status_agrees_with_the_python_gate(c, n):
    """gldm_point_attention_fused's own answer for a shape against attention.fused_supported: GLDM_ERR_UNSUPPORTED before
    anything is launched (non-null dummy pointers, never dereferenced).  An accepted shape cannot be called without a GPU;
    for those the misaligned-pointer status, which the entry checks after the shape, shows that the shape passed."""
    from graspldm_amd import _lib as L
    from graspldm_amd.attention import fused_supported
    h, p = L.lib(), _host_ptr()
    ok = fused_supported(c, n)
    assert ok is (c % 16 == 0 and 32 <= c <= 128 and n % 32 == 0 and 32 <= n <= 4096)
    assert h.gldm_point_attention_fused(_host_ptr(4), p, p, 2, c, n, 0, p, None) == (-1 if ok else -3)


def test_new_entries_reject_bad_arguments_without_launching():
    from graspldm_amd import _lib as L
    h, p, odd = L.lib(), _host_ptr(), _host_ptr(4)
    # the fused core: null pointers, non-positive sizes, a batch beyond the grid, misaligned pointers
    for bad in range(3):
        args = [p, p, p]
        args[bad] = None
        assert h.gldm_point_attention_fused(*args, 2, 64, 512, 0, p, None) == -1
    assert h.gldm_point_attention_fused(p, p, p, 2, 64, 512, 0, None, None) == -1
    assert h.gldm_point_attention_fused(p, p, p, 0, 64, 512, 0, p, None) == -1
    assert h.gldm_point_attention_fused(p, p, p, 65536, 64, 512, 0, p, None) == -3
    for bad in range(4):
        args = [p, p, p, 2, 64, 512, 1, p]
        args[bad if bad < 3 else 7] = odd
        assert h.gldm_point_attention_fused(*args, None) == -1
    # the affine launch
    assert h.gldm_groupnorm_affine(None, p, 2, 32, 4, p, None) == -1
    assert h.gldm_groupnorm_affine(p, None, 2, 32, 4, p, None) == -1
    assert h.gldm_groupnorm_affine(p, p, 2, 32, 4, None, None) == -1
    assert h.gldm_groupnorm_affine(p, p, 2, 0, 4, p, None) == -1
    assert h.gldm_groupnorm_affine(odd, p, 2, 32, 4, p, None) == -1
    assert h.gldm_groupnorm_affine(p, p, 2, 32, 4, odd, None) == -1
    assert h.gldm_groupnorm_affine(p, p, 2, 32, 3, p, None) == -3          # 27 voxels: no whole 16-byte runs
    assert h.gldm_groupnorm_affine(p, p, 2, 32, 68, p, None) == -3
    # GroupNorm + Swish with the squeeze sums: the statuses of gldm_groupnorm_swish_points, and the sums are not optional
    ok = (p, None, p, p, 2, 64, 512, 8, 1e-5, p, p, None)
    for bad in (0, 2, 3, 9, 10):
        args = list(ok)
        args[bad] = None
        assert h.gldm_groupnorm_swish_points_sum(*args) == -1
    for bad in (0, 1, 9):
        args = list(ok)
        args[bad] = odd
        assert h.gldm_groupnorm_swish_points_sum(*args) == -1
    assert h.gldm_groupnorm_swish_points_sum(p, None, p, p, 2, 64, 512, 0, 1e-5, p, p, None) == -1
    assert h.gldm_groupnorm_swish_points_sum(p, None, p, p, 2, 2048, 512, 8, 1e-5, p, p, None) == -3   # 256 channels per group
    assert h.gldm_groupnorm_swish_points_sum(p, None, p, p, 2, 60, 512, 8, 1e-5, p, p, None) == -3
    assert h.gldm_groupnorm_swish_points_sum(p, None, p, p, 2, 64, 510, 8, 1e-5, p, p, None) == -3
    assert h.gldm_groupnorm_swish_points_sum(p, None, p, p, 65536, 64, 512, 8, 1e-5, p, p, None) == -3
    # gldm_groupnorm_coef serves the gate's widest C: 128 channels per group and no more (8 groups: C = 1024)
    assert h.gldm_groupnorm_coef(p, p, p, 2, 1088, 4, 8, 1e-5, p, None) == -1      # 136 per group
    assert h.gldm_groupnorm_coef(p, p, p, 2, 1032, 4, 8, 1e-5, p, None) == -1      # 129 per group
    assert h.gldm_groupnorm_coef(p, p, p, 2, 60, 4, 8, 1e-5, p, None) == -1        # c % groups
    assert h.gldm_abi_version() == L.ABI_VERSION == 15


def test_switch_off_leaves_the_modules_as_they_were():
    from graspldm_amd.pvcnn import PVCNN2, PVConv, SE3d, Swish
    ref = load_schema("schema_pvcnn2.json")
    for net in (PVCNN2(), PVCNN2(use_attention=False)):
        sd = net.state_dict()
        assert set(sd) == set(ref)
        assert all(tuple(sd[k].shape) == shape for k, (shape, _) in ref.items())
    m = PVConv(32, 32, 3, resolution=8, with_se=True)
    assert isinstance(m.voxel_layers[6], Swish) and isinstance(m.voxel_layers[7], SE3d)
    want = {f"voxel_layers.{i}.{p}" for i in (0, 1, 4, 5) for p in ("weight", "bias")} | {"voxel_layers.7.fc.0.weight", "voxel_layers.7.fc.2.weight"}
    assert {k for k in m.state_dict() if k.startswith("voxel_layers.")} == want
