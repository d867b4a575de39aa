"""CPU: the grasp-encoder path (GraspCVAE.encode) below the device -- the fixture against the oracle composition, the
packer's encoder head, the C ABI's argument checks and the Python API's error contract.  Nothing here launches a kernel."""
import ctypes
import hashlib

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, load_schema

ENC = "vae_model.encoder.grasp_encoder."
BOT = "vae_model.bottleneck."
PC = "vae_model.encoder.pc_encoder."


def _encoder_arg(sd, enc=ENC, bot=BOT):
    return dict(in_w=sd[enc + "in_layer.weight"], in_b=sd[enc + "in_layer.bias"], out_w=sd[enc + "out_layer.weight"],
                out_b=sd[enc + "out_layer.bias"], mu_w=sd[bot + "mu.weight"], mu_b=sd[bot + "mu.bias"],
                logvar_w=sd[bot + "logvar.weight"], logvar_b=sd[bot + "logvar.bias"])


def oracle_encode(sd, h, z_cond, enc=ENC, bot=BOT):
    """in_layer -> oracle ResNet1D -> out_layer -> bottleneck (grasp_vae.py:104-117,518-536,563-574); dtype follows sd."""
    from oracle import torch_ref as R
    x = F.linear(h, sd[enc + "in_layer.weight"], sd[enc + "in_layer.bias"]).unsqueeze(-2)
    x = R.resnet1d_forward(sd, enc + "net.", x, z_cond=z_cond).squeeze(-2)
    x = F.linear(x, sd[enc + "out_layer.weight"], sd[enc + "out_layer.bias"])
    return F.linear(x, sd[bot + "mu.weight"], sd[bot + "mu.bias"]), F.linear(x, sd[bot + "logvar.weight"], sd[bot + "logvar.bias"])


def test_vae_encode_fixture_is_the_oracle_composition(fpc_state_dict, fpc_spec):
    """The yardstick: tests/golden/vae_encode.npz (the reference's own GraspCVAE.encode / .forward) equals the oracle
    composition bit for bit in f32, the way tests/test_oracle_golden.py pins the other fixtures."""
    from oracle import torch_ref as R
    g = load_golden("vae_encode.npz")
    sd = fpc_state_dict
    z_pc = R.pvcnn_encoder_forward(sd, PC, g["pc"], fpc_spec)
    assert torch.equal(z_pc, g["z_pc"])
    zc = z_pc.repeat_interleave(8, dim=0)
    mu, logvar = oracle_encode(sd, g["h"], zc)
    assert torch.equal(mu, g["mu"]) and torch.equal(logvar, g["logvar"])
    z = mu + g["eps"] * torch.exp(0.5 * logvar)
    assert torch.equal(z, g["z"])
    tmrp, logit = R.decoder_forward(sd, "vae_model.decoder.", z, zc)
    assert torch.equal(tmrp, g["tmrp"]) and torch.equal(logit, g["logit"])
    assert g["h"].shape == (16, 7) and set(g["h"][:, 6].tolist()) <= {0.0, 1.0}
    torch.manual_seed(int(g["seed"]))
    assert torch.equal(torch.randn(16, 4), g["eps"])       # the eps a caller gets from torch.manual_seed(seed)


def test_h_to_tmrp_fixture_layout():
    g = load_golden("H_to_tmrp.npz")
    n_tie = int(g["n_tie"])
    assert g["H"].shape == (96, 4, 4) and g["tmrp"].shape == (96, 6) and n_tie == 8
    assert (g["margin"][:-n_tie] >= 1e-3).all() and (g["margin"][-n_tie:] < 1e-6).all()
    R = g["H"][:, :3, :3]
    choice = torch.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], -1).argmax(-1)
    assert set(choice[64:80].tolist()) == {0, 1, 2}        # the half turns reach all three `choice != 3` branches
    assert set(choice[:64].tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("schema,lz,dc", [("schema_fpc_ldm.json", 4, 64), ("schema_ppc_ldm.json", 16, 256)])
def test_pack_encoder_head(schema, lz, dc):
    from graspldm_amd.r1d_pack import HEAD_ENCODER, pack_resnet1d
    from graspldm_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(load_schema(schema), seed=0)
    arg = _encoder_arg(sd)
    packed = pack_resnet1d(sd, ENC + "net.", groups=4, seq_len=16, encoder=arg)
    d, w = packed["desc"], packed["weights"]
    assert d.head_kind == HEAD_ENCODER and d.n_head == 2 * lz and d.latent_dim == 7 and d.seq_len == 16
    assert packed["cond_w"].shape[1] == dc
    a = {k: v.double() for k, v in arg.items()}
    head_w = w[d.head_w:d.head_w + 2 * lz * 16].reshape(2 * lz, 16).double()
    head_b = w[d.head_b:d.head_b + 2 * lz].double()
    for rows, name in ((slice(0, lz), "mu"), (slice(lz, 2 * lz), "logvar")):
        ew = a[name + "_w"] @ a["out_w"]
        eb = a[name + "_w"] @ a["out_b"] + a[name + "_b"]
        assert (head_w[rows] - ew).abs().max() <= 1e-7 * ew.abs().max()
        assert (head_b[rows] - eb).abs().max() <= 1e-7 * eb.abs().max()
    assert torch.equal(w[d.in_w:d.in_w + 16 * 7].reshape(16, 7), arg["in_w"])
    p = "vae_model.decoder."
    dec = dict(in_w=sd[p + "in_layer.weight"], in_b=sd[p + "in_layer.bias"], tmrp_w=sd[p + "tmrp.weight"],
               tmrp_b=sd[p + "tmrp.bias"], cls_w=sd[p + "class_logits.weight"], cls_b=sd[p + "class_logits.bias"])
    with pytest.raises(ValueError):
        pack_resnet1d(sd, ENC + "net.", groups=4, seq_len=16, encoder=arg, decoder=dec)


def test_abi_entries_and_argument_checks(fpc_state_dict):
    """gldm_encode / gldm_pose_prologue: declared, exported, bound; bad arguments come back as GLDM_ERR_INVALID_ARG (-1)
    before anything touches the device (this test runs without one)."""
    import os
    import re
    from graspldm_amd import _lib
    from graspldm_amd.r1d_pack import pack_resnet1d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gldm.h")).read(), flags=re.S)
    for name in ("gldm_encode", "gldm_pose_prologue"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib._SIGNATURES
    h = _lib.lib()
    assert h.gldm_abi_version() == _lib.ABI_VERSION >= 11
    sd = fpc_state_dict
    enc = pack_resnet1d(sd, ENC + "net.", groups=4, seq_len=16, encoder=_encoder_arg(sd))
    p = "vae_model.decoder."
    dec = pack_resnet1d(sd, p + "net.", groups=4, seq_len=16, decoder=dict(
        in_w=sd[p + "in_layer.weight"], in_b=sd[p + "in_layer.bias"], tmrp_w=sd[p + "tmrp.weight"],
        tmrp_b=sd[p + "tmrp.bias"], cls_w=sd[p + "class_logits.weight"], cls_b=sd[p + "class_logits.bias"]))
    dp = lambda pk: ctypes.cast(ctypes.pointer(pk["desc"]), ctypes.c_void_p)   # noqa: E731
    buf = (ctypes.c_float * 64)()     # host memory standing in for non-NULL pointers: rejected calls never read it
    q = ctypes.cast(buf, ctypes.c_void_p)
    enc_call = lambda d, *a: h.gldm_encode(d, *a)   # noqa: E731
    # (desc, weights, cemb, spc, h, n, eps, mix_mu, mix_eps, eps_times_std, mu, logvar, z, workspace, stream)
    assert enc_call(dp(enc), None, q, 1, q, 1, None, 1.0, 1.0, 1, q, q, None, q, None) == -1          # weights NULL
    assert enc_call(dp(enc), q, q, 1, q, 1, None, 1.0, 1.0, 1, None, q, None, q, None) == -1          # mu NULL
    assert enc_call(dp(enc), q, q, 1, q, 0, None, 1.0, 1.0, 1, q, q, None, q, None) == -1             # n = 0
    assert enc_call(dp(enc), q, q, 0, q, 1, None, 1.0, 1.0, 1, q, q, None, q, None) == -1             # samples_per_cond
    assert enc_call(dp(enc), q, q, 1, q, 1, None, 1.0, 1.0, 1, q, q, None, None, None) == -1          # workspace NULL
    assert enc_call(dp(dec), q, q, 1, q, 1, None, 1.0, 1.0, 1, q, q, None, q, None) == -1             # decoder descriptor
    assert h.gldm_decode(dp(enc), q, q, 1, q, 1, q, q, q, None) == -1                                 # and the converse
    assert h.gldm_pose_prologue(None, None, q, q, 1, 1, 1, q, None) == -1
    assert h.gldm_pose_prologue(q, None, q, q, 0, 1, 1, q, None) == -1
    assert h.gldm_pose_prologue(q, None, q, q, 4, 1, 2, q, None) == -1                                # 4 grasps, 2 cloud rows
    assert h.gldm_pose_prologue(q, None, q, q, 1, 1, 1, None, None) == -1


def test_python_api_error_contract():
    """On CPU tensors encode / forward(compute_loss=False) raise the package's "CUDA tensor" RuntimeError (they exist
    and reach their device check); the training default keeps raising NotImplementedError."""
    from graspldm_amd.pipeline import build_fpc_ldm
    ldm = build_fpc_ldm()
    vae = ldm.vae_model
    xyz, h = torch.zeros(1, 1024, 3), torch.zeros(2, 7)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        vae.encode(xyz, h)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        vae(xyz, h, compute_loss=False)
    with pytest.raises(NotImplementedError):
        vae(xyz, h)
    with pytest.raises(NotImplementedError):
        vae(xyz, h, compute_loss=True)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        vae.encoder.grasp_encoder(h.unsqueeze(1), torch.zeros(2, 3, 64))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ldm.encode_grasps(xyz, h)
    with pytest.raises(ValueError):
        ldm.refine_grasps(xyz, h, 1.5)
    with pytest.raises(ValueError):
        ldm.refine_grasps(xyz, h, -0.1)
    mu, logvar = vae.bottleneck(torch.zeros(2, 4))          # two tiny Linears: plain torch wherever the tensor lives
    assert mu.shape == logvar.shape == (2, 4)
    assert vae.bottleneck.reparameterize(mu, logvar).shape == (2, 4)


def test_decoder_and_denoiser_pack_to_the_parent_commits_bytes(fpc_state_dict):
    """The encoder head is additive: the fpc pose decoder and latent denoiser pack to the weight buffers of the commit in
    front of this feature, byte for byte (sha256 computed there with that commit's packer)."""
    from graspldm_amd.r1d_pack import HEAD_DECODER, pack_resnet1d
    sd = fpc_state_dict
    p = "vae_model.decoder."
    dec = pack_resnet1d(sd, p + "net.", groups=4, seq_len=16, decoder=dict(
        in_w=sd[p + "in_layer.weight"], in_b=sd[p + "in_layer.bias"], tmrp_w=sd[p + "tmrp.weight"],
        tmrp_b=sd[p + "tmrp.bias"], cls_w=sd[p + "class_logits.weight"], cls_b=sd[p + "class_logits.bias"]))
    den = pack_resnet1d(sd, "diffusion_model.model.", groups=4, seq_len=4, num_steps=1000)
    sha = lambda pk: hashlib.sha256(pk["weights"].numpy().tobytes()).hexdigest()   # noqa: E731
    assert dec["weights"].numel() == 2186748 and den["weights"].numel() == 2068976
    assert sha(dec) == "4980b038449044b2b6029417bc4c74ef71c0b7abe081dc4cfaf1ed77a159d305"
    assert sha(den) == "95a5f4c2e08feb19d67460855305aa382f978990704db06a4366ddbe78eaa746"
    assert dec["desc"].head_kind == HEAD_DECODER and dec["desc"].n_head == 7 and den["desc"].n_head == 0
