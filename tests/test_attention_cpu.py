"""CPU: host side of the global-attention path -- state_dict schema of both encoders with use_global_attention=True against
the reference's (fixture captured from it), the two algebraic folds against the unfolded formula in f64, the shape
gate, and the switch-off encoders unchanged."""
import pytest
import torch

from conftest import load_schema

FPC = dict(in_features=3, out_features=64, n_points=1024, scale_channels=0.75, scale_voxel_resolution=0.75,
           num_blocks=(1, 1, 1, 1), out_channels=3)


def test_pvcnn_encoder_schema_with_attention_matches_reference():
    from graspldm_amd.pc_encoders import PVCNNEncoder
    from graspldm_amd.synthetic import synthetic_state_dict
    ref = load_schema("schema_pvcnn_encoder_attn.json")
    enc = PVCNNEncoder(use_global_attention=True, **FPC)
    sd = enc.state_dict()
    assert set(sd) == set(ref), (sorted(set(ref) - set(sd))[:5], sorted(set(sd) - set(ref))[:5])
    for k, (shape, dtype) in ref.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == dtype, k
    enc.load_state_dict(synthetic_state_dict(ref, seed=0), strict=True)
    assert tuple(enc.global_attention.q.weight.shape) == (768, 768, 1)


def test_pvcnn2_encoder_with_attention_has_the_reference_block_keys():
    """PVCNN2Encoder shares the head: the same ten global_attention.* keys (at its own width) on top of its switch-off keys."""
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    kw = dict(in_features=3, out_features=64, n_points=1024, scale_channels=1, scale_voxel_resolution=1, out_channels=3)
    off, on = PVCNN2Encoder(**kw).state_dict(), PVCNN2Encoder(use_global_attention=True, **kw).state_dict()
    ref = load_schema("schema_pvcnn_encoder_attn.json")
    extra = sorted(set(on) - set(off))
    assert extra == sorted(k for k in ref if k.startswith("global_attention.")) and set(off) <= set(on)
    c = on["conv_downscale.weight"].shape[0]
    assert c == 32
    for k in extra:
        assert tuple(on[k].shape) == ((c, c, 1) if k.endswith(".weight") and "norm" not in k else (c,)), k
    on_strict = PVCNN2Encoder(use_global_attention=True, **kw)
    on_strict.load_state_dict({k: torch.zeros_like(v) for k, v in on.items()}, strict=True)


@pytest.mark.parametrize("c,n", [(16, 32), (48, 96), (64, 33)])
def test_folds_equal_the_unfolded_formula_in_f64(c, n):
    from graspldm_amd.attention import fold_attention
    g = torch.Generator().manual_seed(c + n)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    wq, wk, wv, wo = (r(c, c) / c ** 0.5 for _ in range(4))
    bq, bk, bv, bo = (0.3 * r(c) for _ in range(4))
    x = r(2, c, n)
    q, k, v = (w @ x + b[:, None] for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    p = torch.softmax(q.transpose(1, 2) @ k, dim=-1)
    want = wo @ (v @ p.transpose(1, 2)) + bo[:, None]
    wq2, bq2, wo2, bo2 = fold_attention(wq, bq, wk, wv, bv, wo, bo)
    assert all(t.dtype == torch.float64 for t in (wq2, bq2, wo2, bo2))
    p2 = torch.softmax((wq2 @ x + bq2[:, None]).transpose(1, 2) @ x, dim=-1)     # K = x
    got = wo2 @ (x @ p2.transpose(1, 2)) + bo2[:, None]                          # V = x
    assert (p2 - p).abs().max() <= 1e-12
    assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))


def test_unsupported_shapes_raise_at_construction():
    from graspldm_amd.attention import Attention
    from graspldm_amd.pc_encoders import PVCNN2Encoder, PVCNNEncoder
    with pytest.raises(NotImplementedError, match=r"\(24, None\)"):
        Attention(24, 8, D=1)
    with pytest.raises(NotImplementedError, match=r"\(2048, None\)"):
        Attention(2048, 8, D=1)
    with pytest.raises(NotImplementedError, match=r"\(768, 1000\)"):      # N not in whole 32-point tiles
        PVCNNEncoder(use_global_attention=True, **dict(FPC, n_points=1000))
    with pytest.raises(NotImplementedError, match=r"\(768, 8192\)"):
        PVCNNEncoder(use_global_attention=True, **dict(FPC, n_points=8192))
    with pytest.raises(NotImplementedError, match=r"\(8, 1024\)"):        # PVCNN2 at a quarter width: C = 8
        PVCNN2Encoder(n_points=1024, scale_channels=0.25, use_global_attention=True)
    with pytest.raises(NotImplementedError):
        PVCNN2Encoder(use_local_attention=True)
    Attention(64, 8, D=3), Attention(1024, 8, D=1)


def test_switch_off_leaves_the_encoders_as_they_were():
    from graspldm_amd.pc_encoders import PVCNNEncoder
    ref = load_schema("schema_fpc_ldm.json")
    pre = "vae_model.encoder.pc_encoder."
    want = {k[len(pre):] for k in ref if k.startswith(pre)}
    enc = PVCNNEncoder(use_global_attention=False, **FPC)
    assert set(enc.state_dict()) == want and enc.global_attention is None
    assert not any(k.startswith("global_attention") for k in PVCNNEncoder(**FPC).state_dict())


def test_pipeline_config_takes_the_switch():
    from graspldm_amd.pipeline import fpc_model_config
    enc = lambda **kw: fpc_model_config(**kw)["vae"]["model"]["args"]["pc_encoder_config"]["args"]   # noqa: E731
    assert enc()["use_global_attention"] is False and enc(use_global_attention=True)["use_global_attention"] is True
    assert "use_global_attention" not in enc(encoder="PVCNN2Encoder")
    assert enc(encoder="PVCNN2Encoder", use_global_attention=True)["use_global_attention"] is True
