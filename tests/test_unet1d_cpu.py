"""CPU: Unet1D's registry entries and state-dict schema, the restatement against the reference's recorded outputs, the
packer (fragments, two-source K padding, time tables, the program on the CPU) and the supported envelope."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import unet1d_ref as U
from conftest import GOLDEN, load_golden

FPC_DEFAULT = {'vae': {'model': {'type': 'GraspCVAE', 'args': {'grasp_latent_size': 4, 'pc_latent_size': 64, 'pc_encoder_config': {'type': 'PVCNNEncoder', 'args': {'in_features': 3, 'n_points': 1024, 'scale_channels': 0.75, 'scale_voxel_resolution': 0.75, 'num_blocks': (1, 1, 1, 1), 'out_channels': 3, 'use_global_attention': False}}, 'grasp_encoder_config': {'type': 'ResNet1D', 'args': {'in_features': 7, 'block_channels': (32, 64, 128, 256), 'input_conditioning_dims': 64, 'resnet_block_groups': 4, 'dropout': 0.1}}, 'decoder_config': {'type': 'ResNet1D', 'args': {'block_channels': (32, 64, 128, 256), 'input_conditioning_dims': 64, 'resnet_block_groups': 4, 'dropout': 0.1}}, 'loss_config': {'reconstruction_loss': {'type': 'GraspReconstructionLoss'}, 'latent_loss': {'type': 'VAELatentLoss'}}, 'num_output_qualities': 0, 'intermediate_feature_resolution': 16}}}, 'ddm': {'model': {'type': 'GraspLatentDDM', 'args': {'model': {'type': 'TimeConditionedResNet1D', 'args': {'dim': 4, 'channels': 1, 'is_time_conditioned': True, 'learned_variance': False, 'learned_sinusoidal_cond': False, 'random_fourier_features': True, 'block_channels': (32, 64, 128, 256), 'input_conditioning_dims': 64, 'resnet_block_groups': 4, 'dropout': 0.1}}, 'latent_in_features': 4, 'diffusion_timesteps': 1000, 'noise_scheduler_type': 'ddim', 'diffusion_loss': 'l2', 'beta_schedule': 'linear', 'is_conditioned': True, 'joint_training': False, 'denoising_loss_weight': 1, 'variance_type': 'fixed_large', 'elucidated_diffusion': False, 'beta_start': 5e-05, 'beta_end': 0.001}}}}


def _schema():
    with open(os.path.join(GOLDEN, "schema_unet1d.json")) as f:
        return json.load(f)


def _net(name):
    from graspldm_amd.resnets import Unet1D
    from graspldm_amd.synthetic import load_synthetic_weights
    c = U.LDS_REFUSED[name] if name in U.LDS_REFUSED else U.config(name)
    return load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"])


def _sd(name):
    return {k: v.detach() for k, v in _net(name).state_dict().items()}


# ---------------------------------------------------------------------------------------------- registry and schema
def test_registry_and_nested_config():
    from graspldm_amd import builder
    from graspldm_amd.resnets import Unet1D
    assert builder.ALL_MODELS["Unet1D"] is Unet1D and builder.STANDARD_MODULES["Unet1D"] is Unet1D
    ddm = builder.build_model_from_cfg(dict(model=dict(type="GaussianDiffusion1D", args=dict(
        model=dict(type="Unet1D", args=dict(U.CASES["B"]["args"])), n_dims=16, noise_scheduler_type="ddim"))))
    assert isinstance(ddm.model, Unet1D) and ddm.model.out_channels == 1 and ddm.model.emb_dim == 64
    assert ddm.model.is_time_conditioned and ddm.model.is_input_conditioned and ddm.model.in_features == 16


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_state_dict_matches_the_reference_schema(name):
    want = _schema()[name]
    got = {k: list(v.shape) for k, v in _net(name).state_dict().items()}
    assert got == want, sorted(set(got) ^ set(want))[:8]


def test_vae_with_unet_cores_builds_and_matches_the_fixture_keys():
    from graspldm_amd.builder import build_model_from_cfg
    from graspldm_amd.pipeline import fpc_model_config
    from graspldm_amd.resnets import Unet1D
    cfg = fpc_model_config(vae_core="Unet1D")
    enc_args = cfg["vae"]["model"]["args"]["grasp_encoder_config"]["args"]
    assert enc_args == dict(in_features=7, dim_mults=(1, 2, 4, 8), input_conditioning_dims=64, is_time_conditioned=False,
                            resnet_block_groups=4)
    vae = build_model_from_cfg(cfg["vae"])
    assert isinstance(vae.decoder.net, Unet1D) and isinstance(vae.encoder.grasp_encoder.net, Unet1D)
    got = {k: list(v.shape) for k, v in vae.state_dict().items() if k.startswith(("decoder.", "encoder.grasp_encoder."))}
    assert got == _schema()["VAE"]


def test_default_fpc_config_is_unchanged():
    from graspldm_amd.pipeline import fpc_model_config
    assert fpc_model_config() == FPC_DEFAULT
    with pytest.raises(ValueError, match="vae_core"):
        fpc_model_config(vae_core="Unet2D")


# ------------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_restatement_equals_the_reference_outputs(name):
    gold = load_golden("unet1d.npz")
    x, z, t = U.case_inputs(name, U.GOLDEN_ROWS)
    out = U.unet1d_forward(_sd(name), "", x, z, t, groups=U.CASES[name]["args"]["resnet_block_groups"])
    err = float((out - gold[name + "_out"]).abs().max())
    print(f"case {name}: |restatement - reference| = {err:.1e} (recorded d = {float(gold[name + '_d']):.2e})")
    assert err <= 1e-6


# ----------------------------------------------------------------------------------------------------------- packer
@pytest.mark.parametrize("exact", [False, True])
def test_fragments_round_trip(exact):
    from graspldm_amd.unet1d_pack import fragments, unpack_fragments
    w = torch.randn(48, 96, generator=torch.Generator().manual_seed(3)) * 3
    back = unpack_fragments(fragments(w, exact), 48, 96, exact)
    err = float(((back - w.double()).abs() / w.double().abs().clamp(min=2.0 ** -3)).max())
    assert err <= (0.0 if exact else 2.0 ** -22), err


def test_two_source_padding_has_zero_columns_where_the_descriptor_says():
    """An up block of case A reads 16 + 16 channels: K = 3 taps x (32 + 32), the upper half of every block zero; every
    other column is the standardised weight."""
    from graspldm_amd.r1d_pack import weight_standardize
    from graspldm_amd.unet1d_pack import OP_CONV, pack_unet1d, source_columns, unpack_fragments
    sd = _sd("A")
    pk = pack_unet1d(sd, "", 4, 16, cond_rows=3)
    ws = weight_standardize(sd["ups.3.0.block1.proj.weight"])     # [16, 32, 3]
    convs = [r for r in pk["ops"] if r[0] == OP_CONV and r[5] == 16 and r[2] == 16 and r[10] == 3 and r[8] == 16]
    assert convs, "no two-source 16 + 16 conv in the program"
    cols = source_columns([16, 16], 3)
    assert len(cols) == 192 and sum(c is None for c in cols) == 96
    hits = 0
    for r in convs:
        w = unpack_fragments(pk["weights"][r[13]:], 16, 192, False)
        ok = all(float(w[:, k].abs().max()) == 0.0 if c is None else
                 float((w[:, k] - ws[:, 16 * c[0] + c[2], c[1]].double()).abs().max()) <= 2.0 ** -22 * 8
                 for k, c in enumerate(cols))
        hits += ok
    assert hits >= 1, "no conv of the program holds ups.3.0.block1 in [source][tap][padded channel] order"
    assert pad_example() == (96, 64)


def pad_example():
    from graspldm_amd.unet1d_pack import pad_sources
    return pad_sources(torch.ones(16, 96, 1), [64, 32]).shape[1], pad_sources(torch.ones(16, 32, 1), [16, 16]).shape[1]


def test_time_tables():
    from graspldm_amd.unet1d_pack import time_table
    from oracle.torch_ref import time_embedding
    sd = _sd("B")
    tab = time_table(sd, "", 1000, 16)
    assert torch.equal(tab, time_embedding(sd, "", torch.arange(1000)))
    sd = _sd("C")
    tab = time_table(sd, "", 1000, 16)
    t = torch.arange(1000)
    half = 8
    e = math.log(10000) / (half - 1)
    e = t[:, None] * torch.exp(torch.arange(half) * -e)[None, :]          # resnets.py:34-41 in f32
    four = torch.cat((e.sin(), e.cos()), dim=-1)
    want = F.linear(F.gelu(F.linear(four, sd["time_mlp.1.weight"], sd["time_mlp.1.bias"])), sd["time_mlp.3.weight"],
                    sd["time_mlp.3.bias"])
    assert tab.shape == (1000, 64) and torch.equal(tab, want)


def _program_vs_restatement(name, exact, n):
    """Packs configuration `name`, checks the program's bounds and interprets it on n samples: (packed, the largest
    difference from the f64 restatement)."""
    from graspldm_amd import numerics
    from graspldm_amd.unet1d_pack import check_program, pack_unet1d, run_program_cpu
    c = U.config(name)
    sd = _sd(name)
    x, z, t = U.case_inputs(name, n)
    rows = 0 if z is None else (1 if z.ndim == 2 else z.shape[1])
    with numerics.f32_only(exact):
        pk = pack_unet1d(sd, "", c["args"]["resnet_block_groups"], c["L"], cond_rows=rows,
                         time_cond=c["args"]["is_time_conditioned"], num_steps=1000)
    assert bool(pk["desc"].exact_f32) == exact and pk["desc"].lds_floats * 4 <= 160 * 1024
    check_program(pk["desc"], pk["ops"])
    n = min(n, pk["desc"].tile_samples)
    x, z, t = x[:n], (z[:n] if z is not None else None), (t[:n] if t is not None else None)
    cemb = None
    if z is not None:
        zz = z if z.ndim == 3 else z[:, None]
        cemb = F.linear(F.silu(F.linear(zz, sd["input_emb_layers.0.weight"], sd["input_emb_layers.0.bias"])),
                        sd["input_emb_layers.2.weight"], sd["input_emb_layers.2.bias"])
    te = pk["temb"][t] if t is not None else None
    out = run_program_cpu(pk, x[:, 0], te, cemb)
    ref = U.unet1d_forward({k: v.double() for k, v in sd.items()}, "", x.double(), z.double() if z is not None else None, t,
                           groups=c["args"]["resnet_block_groups"], temb=te.double() if te is not None else None)
    return pk, float((out - ref[:, 0]).abs().max())


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_program_on_the_cpu_reproduces_the_restatement(name, exact):
    """The packed program (ops, LDS map, fragments) interpreted with torch equals the f64 restatement to the weights'
    rounding: pins the packer and the bounds check without a GPU."""
    pk, err = _program_vs_restatement(name, exact, 3)
    assert pk["desc"].tile_samples >= 3
    print(f"case {name} {'f32' if exact else 'split'}: program vs restatement {err:.2e}")
    assert err <= 2e-6


# --------------------------------------------------------------------------------------------------------- envelope
@pytest.mark.parametrize("kw, word", [
    (dict(dim=16, is_self_conditioned=True), "is_self_conditioned"),
    (dict(dim=16, learned_variance=True), "learned_variance"),
    (dict(dim=16, channels=2), "channels"),
    (dict(dim=16, init_dim=32), "init_dim"),
    (dict(dim=8), "dim must be 16 or 32"),
    (dict(dim=16, dim_mults=(1,)), "2 to 4 dim_mults"),
    (dict(dim=16, dim_mults=(1, 2, 4, 8, 16)), "2 to 4 dim_mults"),
    (dict(dim=32, dim_mults=(1, 2, 4, 16)), "multiple of 16 between 16 and 256"),
    (dict(dim=16, resnet_block_groups=2), "resnet_block_groups must be 4 or 8"),
])
def test_unsupported_arguments_raise_naming_the_limit(kw, word):
    from graspldm_amd.resnets import Unet1D
    with pytest.raises(NotImplementedError, match=word):
        Unet1D(**kw)


def test_conditioning_limits():
    from graspldm_amd.resnets import Unet1D
    net = Unet1D(dim=16, dim_mults=(1, 2), input_conditioning_dims=8)
    with pytest.raises(NotImplementedError, match="816-822"):
        net._cond_rows_of(torch.zeros(2, 3, 8))
    net = Unet1D(dim=16, dim_mults=(1, 2), input_conditioning_dims=8, is_time_conditioned=False)
    assert net._cond_rows_of(torch.zeros(2, 3, 8)) == 3
    with pytest.raises(NotImplementedError, match="at most 4 rows"):
        net._cond_rows_of(torch.zeros(2, 5, 8))


def _desc(**kw):
    from graspldm_amd.unet1d import header_desc
    base = dict(dim=16, dims=[16, 16, 32, 64, 128], groups=4, cond_rows=1, time_cond=False)
    base.update(kw)
    return header_desc(**base)


def test_supported_agrees_with_the_python_envelope():
    from graspldm_amd import _lib as L
    from graspldm_amd.unet1d import check_supported
    h = L.lib()
    p = lambda d: ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)   # noqa: E731
    assert h.gldm_unet1d_supported(p(_desc()), 16) == 0
    assert h.gldm_unet1d_supported(p(_desc()), 12) == -3            # four levels need L % 8 == 0 (resnets.py:843)
    assert h.gldm_unet1d_supported(p(_desc()), 24) == -3
    assert h.gldm_unet1d_supported(p(_desc(dims=[16, 16, 32])), 12) == 0
    for bad in (dict(dim=8, dims=[8, 8, 16]), dict(dims=[16, 16]), dict(dims=[16, 16, 24]), dict(dims=[16, 16, 512]),
                dict(groups=2), dict(cond_rows=5), dict(cond_rows=3, time_cond=True)):
        assert h.gldm_unet1d_supported(p(_desc(**bad)), 16) == -3, bad
        with pytest.raises(NotImplementedError, match="envelope"):
            check_supported(_desc(**bad), 16)
    with pytest.raises(NotImplementedError, match="L=12"):
        check_supported(_desc(), 12)


def _query(c):
    """gldm_unet1d_supported on a configuration of unet1d_ref."""
    from graspldm_amd import _lib as L
    from graspldm_amd.unet1d import header_desc
    a = c["args"]
    rows = 0 if c["z_shape"] is None else (1 if len(c["z_shape"]) == 1 else c["z_shape"][0])
    d = header_desc(a["dim"], [a["dim"]] + [a["dim"] * m for m in a["dim_mults"]], a["resnet_block_groups"], rows,
                    a["is_time_conditioned"])
    return L.lib().gldm_unet1d_supported(ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), c["L"])


_PACKED = {}


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", sorted(U.ENVELOPE))
def test_envelope_row_packs_and_its_program_reproduces_the_restatement(name, exact):
    """Every ENVELOPE row: accepted by the query, packed, bounds-checked, and its program on the CPU (up to 3 samples of a
    tile) within 2e-6 of the f64 restatement."""
    assert _query(U.ENVELOPE[name]) == 0
    pk, err = _program_vs_restatement(name, exact, 3)
    if not exact:
        _PACKED[name] = pk
    d = pk["desc"]
    print(f"row {name} {'f32' if exact else 'split'}: tile {d.tile_samples}, LDS {d.lds_floats * 4 / 1024:.1f} KiB, "
          f"program vs restatement {err:.2e}")
    assert err <= 2e-6


@pytest.mark.parametrize("name", sorted(U.LDS_REFUSED))
def test_shapes_inside_the_envelope_that_the_packer_refuses_for_lds(name):
    """The query's envelope is necessary, not sufficient: these pass it and UnetEngine.plan refuses them, naming LDS, before
    any HIP call (no device is touched: the engine is only given a device's name)."""
    from graspldm_amd.unet1d import UnetEngine
    c = U.LDS_REFUSED[name]
    assert _query(c) == 0
    eng = UnetEngine(_sd(name), c["args"]["resnet_block_groups"], 0, False, None, "cuda:0")
    with pytest.raises(NotImplementedError, match="160 KiB of LDS"):
        eng.plan(c["L"])


def test_check_supported_says_that_lds_can_still_refuse():
    from graspldm_amd.unet1d import check_supported
    assert "LDS" in check_supported.__doc__
    with pytest.raises(NotImplementedError, match="LDS"):
        check_supported(_desc(groups=2), 16)


def _properties(c, pk):
    """What one configuration (and the layout the packer chose for it) contributes to the envelope's coverage."""
    from graspldm_amd.unet1d_pack import level_lengths
    a, d = c["args"], pk["desc"]
    widths = [a["dim"] * m for m in a["dim_mults"]]
    rows = 0 if c["z_shape"] is None else (1 if len(c["z_shape"]) == 1 else c["z_shape"][0])
    deepest = level_lengths(c["L"], len(widths))[-1]
    time = "none" if not a["is_time_conditioned"] else ("fourier" if a.get("learned_sinusoidal_cond") else "plain")
    got = {f"dim {a['dim']}", f"{len(widths)} levels", f"groups {a['resnet_block_groups']}", f"cond rows {rows}",
           f"time {time}", f"deepest length {deepest}", f"L {c['L']}", f"tile {d.tile_samples}"}
    got |= {"width 16 mod 32 above 16" for w in widths if w % 32 == 16 and w > 16}
    got |= {"width 256" for w in widths if w == 256}
    got |= {"decreasing widths" for u, v in zip(widths, widths[1:]) if v < u}
    if d.tile_samples * c["L"] % 16:
        got.add("ragged last column block")
    if d.lds_floats * 4 > 150 * 1024:
        got.add("LDS above 150 KiB")
    return got


REQUIRED = {"dim 16", "dim 32", "2 levels", "3 levels", "4 levels", "groups 4", "groups 8", "cond rows 0", "cond rows 1",
            "cond rows 2", "cond rows 3", "cond rows 4", "time none", "time fourier", "time plain",
            "width 16 mod 32 above 16", "width 256", "decreasing widths", "deepest length 3", "deepest length 5",
            "deepest length 7", "L 2", "L 16", "tile 1", "tile 16", "ragged last column block", "LDS above 150 KiB"}


def test_cases_and_envelope_cover_the_listed_corners():
    """Fails when CASES and ENVELOPE together (with the tile sizes the packer chooses today) lose one of REQUIRED."""
    from graspldm_amd.unet1d_pack import pack_unet1d
    got = set()
    for name in sorted(U.CASES) + sorted(U.ENVELOPE):
        c = U.config(name)
        if name not in _PACKED:
            rows = 0 if c["z_shape"] is None else (1 if len(c["z_shape"]) == 1 else c["z_shape"][0])
            _PACKED[name] = pack_unet1d(_sd(name), "", c["args"]["resnet_block_groups"], c["L"], cond_rows=rows,
                                        time_cond=c["args"]["is_time_conditioned"], num_steps=1000)
        got |= _properties(c, _PACKED[name])
    assert not REQUIRED - got, sorted(REQUIRED - got)


@pytest.mark.parametrize("name, admitted", [("N", (1, 2, 3, 5, 7, 11)), ("O", (1, 2, 3, 5, 7, 11, 16))])
def test_tile_sizes_the_bounds_check_admits(name, admitted):
    """pack_unet1d(tile_samples=S) for S in {1, 2, 3, 5, 7, 11, 16}: the layouts check_program admits are the ones
    tests/test_unet1d_envelope_gpu.py forces (FORCED there); the others exceed the 160 KiB of LDS."""
    from graspldm_amd.unet1d_pack import pack_unet1d
    c = U.ENVELOPE[name]
    rows = 0 if c["z_shape"] is None else (1 if len(c["z_shape"]) == 1 else c["z_shape"][0])
    ok = []
    for s in (1, 2, 3, 5, 7, 11, 16):
        try:
            pk = pack_unet1d(_sd(name), "", c["args"]["resnet_block_groups"], c["L"], cond_rows=rows, tile_samples=s)
        except AssertionError as e:
            assert "LDS over 160 KiB" in str(e)
            continue
        assert pk["desc"].tile_samples == s
        ok.append(s)
    assert tuple(ok) == admitted


def test_null_pointers_return_a_status():
    from graspldm_amd import _lib as L
    h = L.lib()
    assert h.gldm_unet1d_supported(None, 16) == -1
    assert h.gldm_unet1d(None, None, None, None, 1, None, 1, 16, None, None, 1, 0, 1, None, None, None, None) == -1
    d = _desc()
    assert h.gldm_unet1d(ctypes.cast(ctypes.pointer(d), ctypes.c_void_p), None, None, None, 1, None, 1, 16, None, None, 1, 0,
                         1, None, None, None, None) == -1
