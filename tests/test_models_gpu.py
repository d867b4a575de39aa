"""GPU (MI355X): the reference-interface modules (same class names / ctor args /
state_dict keys) running on the HIP path, against the golden vectors captured from
the reference.  Tolerances: encoder latent 5e-5 (8 GFLOP of f32 GEMMs per cloud in a
different summation order), poses / H entries 1e-4 (north-star bound)."""
import pytest
import torch

from conftest import load_golden, load_schema
from test_modules_cpu import build_fpc

pytestmark = pytest.mark.gpu


def _err(a, b):
    return (a.detach().cpu() - b).abs().max().item()


@pytest.fixture(scope="module")
def ldm(fpc_state_dict):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    m = build_fpc(scheduler="ddim")
    m.load_state_dict(fpc_state_dict, strict=True)
    return m.cuda().eval()


def test_g2_pvcnn_encoder_golden(ldm):
    g = load_golden("pvcnn_encoder.npz")
    z = ldm.vae_model.encode_pc(g["pc"].cuda())
    assert z.shape == (2, 3, 64)
    assert _err(z, g["z"]) < 5e-5, _err(z, g["z"])


def test_g3_denoiser_module_forward(ldm):
    g = load_golden("denoiser.npz")
    den = ldm.diffusion_model.model
    for i, t in enumerate(g["t"].tolist()):
        tb = torch.full((8,), t, dtype=torch.long, device="cuda")
        eps = den(g["x"].cuda(), time=tb, z_cond=g["z_cond"].cuda(), metas={"ignored": True})
        assert _err(eps, g["eps"][i]) < 2e-5


def test_g4_decoder_module(ldm):
    g = load_golden("decoder.npz")
    tmrp, logit = ldm.vae_model.decoder(g["z_h"].cuda(), g["z_cond"].cuda())
    assert _err(tmrp, g["tmrp"]) < 2e-5 and _err(logit, g["logit"]) < 2e-5


def test_g5_sample_return_all_matches_fused(ldm):
    g = load_golden("ddim_traj.npz")
    ldm.set_inference_timesteps(100)
    dm = ldm.diffusion_model
    x0, _ = dm.sample(z_cond=g["z_cond"].cuda(), batch_size=8, x_T=g["x_T"], device="cuda")
    x0b, trace = dm.sample(z_cond=g["z_cond"].cuda(), batch_size=8, x_T=g["x_T"], device="cuda", return_all=True)
    assert len(trace) == 101 and torch.equal(x0, x0b)  # per-step launches == one fused launch, bitwise
    assert _err(x0, g["x0"]) < 1e-4
    for j, i in enumerate(g["probes"].tolist()):
        assert _err(trace[i], g["x"][j]) < 1e-4


def test_g7_ldm_end_to_end_golden(ldm):
    from graspldm_amd.r1d import pose_epilogue
    g = load_golden("ldm_e2e.npz")
    ldm.set_inference_timesteps(100)
    torch.manual_seed(int(g["seed"]))
    (tmrp, logit), inter = ldm.generate_grasps(g["pc"].cuda(), num_grasps=20)
    assert inter == [] and tmrp.shape == (40, 6) and logit.shape == (40, 1)
    assert _err(tmrp, g["tmrp"]) < 1e-4, _err(tmrp, g["tmrp"])
    assert _err(logit, g["logit"]) < 1e-4
    H, un, conf = pose_epilogue(tmrp, logit, g["grasp_mean"].cuda(), g["grasp_std"].cuda(), 20)
    assert _err(H.view(2, 20, 4, 4), g["H"]) < 1e-4
    assert _err(conf.view(2, 20, 1), g["confidence"]) < 1e-4


def test_g7_vae_end_to_end_golden(ldm):
    g = load_golden("vae_e2e.npz")
    torch.manual_seed(int(g["seed"]))
    tmrp, logit = ldm.vae_model.generate_grasps(g["pc"].cuda(), num_grasps=20)
    assert _err(tmrp, g["tmrp"]) < 1e-4 and _err(logit, g["logit"]) < 1e-4


def test_g7_vae_n64_golden():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd.synthetic import synthetic_state_dict
    g = load_golden("vae_e2e_n64.npz")
    m = build_fpc(n_points=64)
    m.load_state_dict(synthetic_state_dict(load_schema("schema_fpc_ldm_n64.json"), seed=0), strict=True)
    m = m.cuda().eval()
    torch.manual_seed(int(g["seed"]))
    tmrp, logit = m.vae_model.generate_grasps(g["pc"].cuda(), num_grasps=20)
    assert _err(tmrp, g["tmrp"]) < 1e-4 and _err(logit, g["logit"]) < 1e-4


def test_g8_sa_modules_golden():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd.pvcnn import PointNetSAModule
    from graspldm_amd.synthetic import synthetic_state_dict
    g = load_golden("sa_module.npz")
    sa1 = PointNetSAModule(num_centers=512, radius=0.2, num_neighbors=64, in_channels=0, out_channels=(64, 64, 128))
    sa2 = PointNetSAModule(num_centers=128, radius=0.4, num_neighbors=64, in_channels=128, out_channels=(128, 128, 256))
    sa1.load_state_dict(synthetic_state_dict(load_schema("schema_sa1.json"), seed=1), strict=True)
    sa2.load_state_dict(synthetic_state_dict(load_schema("schema_sa2.json"), seed=2), strict=True)
    sa1, sa2 = sa1.cuda().eval(), sa2.cuda().eval()
    with torch.no_grad():
        f1, c1 = sa1((None, g["coords"].cuda()))
        assert torch.equal(c1.cpu(), g["c1"])
        assert _err(f1[:, :, ::4], g["f1"]) < 2e-5
        f2, c2 = sa2((f1, c1))
    assert torch.equal(c2.cpu(), g["c2"])
    assert _err(f2, g["f2"]) < 5e-5


def test_g8_pointnet2_ssg_golden():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd.pvcnn import PointNet2SSG
    from graspldm_amd.synthetic import synthetic_state_dict
    g = load_golden("pointnet2_ssg.npz")
    m = PointNet2SSG(extra_feature_channels=0)
    m.load_state_dict(synthetic_state_dict(load_schema("schema_pointnet2_ssg.json"), seed=3), strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        out = m(g["coords"].cuda())
    assert _err(out[:, :, ::8], g["out"]) < 1e-4


def test_g8_pvcnn2_golden():
    """PVCNN2 (SA with PVConv voxel branches + feature propagation, pvcnn_base.py:147-279) against the output of the
    reference's own Python graph (oracle/make_golden.py, CPU backend shim)."""
    from graspldm_amd.pvcnn import PVCNN2
    from graspldm_amd.synthetic import synthetic_state_dict
    g = load_golden("pvcnn2.npz")
    m = PVCNN2()
    m.load_state_dict(synthetic_state_dict(load_schema("schema_pvcnn2.json"), seed=4), strict=True)
    m = m.cuda().eval()
    with torch.no_grad():
        out = m(g["coords"].cuda())
    assert out.shape[1] == 64 and _err(out[:, :, ::16], g["out"]) < 1e-4, _err(out[:, :, ::16], g["out"])


def test_tmrp_to_H_module(ldm):
    from graspldm_amd.rotations import tmrp_to_H
    g = load_golden("tmrp_to_H.npz")
    assert _err(tmrp_to_H(g["tmrp"].cuda()), g["H"]) < 1e-6
    assert tmrp_to_H(g["tmrp"].view(8, 8, 6).cuda()).shape == (8, 8, 4, 4)


def test_ddpm_sampler_runs_and_is_seed_reproducible(ldm):
    m = build_fpc(scheduler="ddpm")
    m.load_state_dict(ldm.state_dict(), strict=True)
    m = m.cuda().eval()
    z = torch.randn(2, 3, 64, device="cuda")
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    a, _ = m.diffusion_model.sample(z_cond=z, batch_size=6, samples_per_cond=3, device="cuda")
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    b, _ = m.diffusion_model.sample(z_cond=z, batch_size=6, samples_per_cond=3, device="cuda")
    assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().max() < 10


def test_ddpm_sampler_with_noise_drawn_in_the_kernel(ldm):
    """sample(noise_source="kernel"): torch.manual_seed still fixes the run, the seed decides the result, the [steps, n, 1, D]
    tensor is never allocated, and the samples have the statistics of the tensor-fed sampler (same distribution, another
    stream: 4096 latents of one conditioning row, per-dimension mean and spread)."""
    m = build_fpc(scheduler="ddpm")
    m.load_state_dict(ldm.state_dict(), strict=True)
    m = m.cuda().eval()
    dm = m.diffusion_model
    dm.set_inference_timesteps(40)
    z = torch.randn(1, 3, 64, device="cuda")
    torch.manual_seed(3)
    a, _ = dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", noise_source="kernel")
    torch.manual_seed(3)
    b, _ = dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", noise_source="kernel")
    assert torch.equal(a, b) and torch.isfinite(a).all()
    x_T = torch.randn(4096, 1, 4)
    c, _ = dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", noise_source="kernel", noise_seed=1, x_T=x_T)
    d, _ = dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", noise_source="kernel", noise_seed=2, x_T=x_T)
    assert not torch.equal(c, d)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", noise_source="kernel", noise_seed=1, x_T=x_T)
    assert torch.cuda.max_memory_allocated() - before < 40 * 4096 * 4 * 4   # less than the noise tensor alone would take
    t, _ = dm.sample(z_cond=z, batch_size=4096, samples_per_cond=4096, device="cuda", x_T=x_T)
    se = t.std(0) / 4096 ** 0.5
    assert ((c.mean(0) - t.mean(0)).abs() < 6 * se + 1e-4).all()
    assert ((c.std(0) / t.std(0).clamp_min(1e-6) - 1).abs() < 0.1).all()
    with pytest.raises(ValueError):
        dm.sample(z_cond=z, batch_size=4, samples_per_cond=4, device="cuda", noise_source="philox")


@pytest.mark.parametrize("b,c,n,m,u,chans", [(2, 128, 512, 128, 64, (128, 128, 256)), (3, 0, 1024, 512, 64, (64, 64, 128)),
                                             (2, 32, 1024, 1024, 32, (32, 64)), (1, 5, 300, 37, 16, (16, 32, 32, 64)),
                                             (2, 64, 256, 37, 32, (64, 128)), (300, 16, 128, 5, 16, (32, 64, 128, 256)),
                                             (1, 160, 200, 9, 64, (128, 128)), (2, 16, 1024, 1024, 32, (16, 32)),
                                             (2, 256, 64, 16, 32, (128, 256))])
@pytest.mark.parametrize("split", [True, False])
def test_fused_sa_mlp_equals_unfused_oracle(b, c, n, m, u, chans, split, monkeypatch):
    """gldm_sa_mlp_forward_f16x2 / gldm_sa_mlp_forward (gather + grouped MLP + max, fused) vs the oracle's
    ball_group -> shared_mlp -> max on the same weights.  split=True: every case runs on the split-f16 64-column kernel
    (sa_mlp3_kernel: 1 / 2 / 4 centres per tile, ragged last tiles, more tiles than persistent workgroups, 2-4 layers,
    1-6 and 9 input blocks, 16-wide hidden layers packed as zero-padded 32-wide ones, the narrow-net form with one and
    with two row quads per gather thread); the predicate is asked about the tables the launch gets (the last case's
    259 -> 128 -> 256 fits the CU's LDS only with its first layer hoisted: 9 + 4 plane blocks + the staged output rows).  split=False forces the f32 kernels: cases 1-3, 5, 6 on the
    128-column one (sa_mlp2_kernel), cases 4 and 7 on the 64-column one (sa_mlp_kernel)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import sa_pack
    if not split:
        monkeypatch.setattr(sa_pack, "split_plan_ok", lambda *a, **k: False)
    elif len(chans) >= 2 and (m * u >= 2 * n if c else sa_pack.PRE_WITHOUT_FEATURES):
        assert sa_pack.split_plan_ok(list(chans[:-1]), list(chans[1:]), u)   # first layer hoisted: the tables behind it
    else:
        assert sa_pack.split_plan_ok([c + 3] + list(chans[:-1]), list(chans), u)
    from graspldm_amd.pvcnn import PointNetSAModule
    from graspldm_amd.synthetic import load_synthetic_weights
    from oracle import torch_ref as R
    mod = PointNetSAModule(num_centers=m, radius=0.35, num_neighbors=u, in_channels=c, out_channels=chans).eval()
    load_synthetic_weights(mod, seed=11)
    g = torch.Generator().manual_seed(2)
    coords = (torch.rand(b, 3, n, generator=g) * 2 - 1).contiguous()
    feats = torch.randn(b, c, n, generator=g) if c else None
    sd = {k: v.detach() for k, v in mod.state_dict().items()}
    exp, ectr = R.sa_module(sd, "", feats, coords, m, [0.35], [u])
    mod = mod.cuda()
    with torch.no_grad():
        got, ctr = mod((feats.cuda() if c else None, coords.cuda()))
    assert torch.equal(ctr.cpu(), ectr)
    assert _err(got, exp) < 2e-5, _err(got, exp)


@pytest.mark.parametrize("b,c,n,relu", [(3, 48, 1024, 1), (2, 1536, 512, 1), (4, 3, 64, 0), (1, 7, 20, 1)])
def test_bias_act_epilogue(b, c, n, relu):
    """gldm_bias_act: the one-pass bias + ReLU epilogue of the k = 1 convs (shared_mlp.py:24-36); bit-exact (add, max)."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(b * 100 + c)
    y = torch.randn(b, c, n, generator=g).cuda()
    bias = torch.randn(c, generator=g).cuda()
    want = y + bias.view(1, -1, 1)
    if relu:
        want = torch.relu(want)
    L.call("gldm_bias_act", L.ptr(y), L.ptr(bias), b, c, n, relu, L.current_stream(y.device))
    assert torch.equal(y, want)


def test_bias_act_rejects_unaligned_rows():
    from graspldm_amd import _lib as L
    y = torch.zeros(1, 2, 6).cuda()
    with pytest.raises(L.GldmError):
        L.call("gldm_bias_act", L.ptr(y), L.ptr(torch.zeros(2).cuda()), 1, 2, 6, 1, L.current_stream(y.device))


@pytest.mark.parametrize("cin,cout,r", [(3, 48, 24), (48, 48, 24), (48, 96, 12), (96, 96, 12), (3, 32, 32), (64, 64, 16),
                                        (20, 48, 24), (3, 32, 16), (32, 64, 8), (16, 16, 16), (32, 32, 8), (64, 64, 4),
                                        (128, 128, 4)])
def test_conv3d_groupnorm_swish_kernels(cin, cout, r):
    """gldm_conv3d_k3 + gldm_groupnorm_swish vs torch conv3d / group_norm on the CPU (fp32, 2e-5:
    K = 27 cin products per output in a different summation order)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d
    g = torch.Generator().manual_seed(cin * 100 + cout)
    b = 2
    x = torch.randn(b, cin, r, r, r, generator=g)
    x[:, :, ::3] = 0  # empty voxels, like a real occupancy grid
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias, gamma, beta = (torch.randn(cout, generator=g) * 0.1 for _ in range(3))
    gamma = gamma + 1
    ref = F.conv3d(x, w, bias, padding=1)
    y = torch.empty(b, cout, r, r, r, device="cuda")
    part = torch.empty(int(L.lib().gldm_conv3d_partial_floats(b, cout, r)), device="cuda")
    st = L.current_stream()
    dx, dw, db = x.cuda(), pack_conv3d(w).cuda(), bias.cuda()
    L.call("gldm_conv3d_k3", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(y), L.ptr(part), st)
    assert _err(y, ref) < 2e-5, _err(y, ref)
    gn = F.group_norm(ref, 8, gamma, beta, 1e-5)
    ref2 = gn * torch.sigmoid(gn)
    cs = torch.empty(b, cout, device="cuda")
    dg, dbt = gamma.cuda(), beta.cuda()
    L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(part), L.ptr(dg), L.ptr(dbt), b, cout, r, 8, 1e-5, L.ptr(cs), st)
    assert _err(y, ref2) < 2e-5, _err(y, ref2)
    assert _err(cs / r ** 3, ref2.mean(dim=(2, 3, 4))) < 1e-5


@pytest.mark.parametrize("cin,cout,r", [(3, 48, 24), (48, 48, 24), (48, 96, 12), (96, 96, 12),
                                        (32, 32, 16), (16, 32, 32), (32, 64, 16), (64, 64, 8), (64, 64, 32), (64, 128, 8),
                                        (128, 128, 4), (128, 128, 16), (128, 256, 8)])
def test_conv3d_split_f16_kernels(cin, cout, r):
    """gldm_conv3d_k3_f16x2 (the shipped encoder's four voxel convs; 3 -> 48 with K = 81 packed into three k-blocks; PVCNN2's
    power-of-two widths and grids, tiles walked in 2- and 4-groups) vs
    torch conv3d on the CPU, and its GroupNorm partials through gldm_groupnorm_swish (fp32, 2e-5)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d_f16x2, pack_conv3d_fewch_f16x2, split_conv_supported
    assert split_conv_supported(cin, cout, r)
    g = torch.Generator().manual_seed(cin * 100 + cout + 1)
    b = 3
    x = torch.randn(b, cin, r, r, r, generator=g)
    x[:, :, ::3] = 0
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias, gamma, beta = (torch.randn(cout, generator=g) * 0.1 for _ in range(3))
    gamma = gamma + 1
    ref = F.conv3d(x, w, bias, padding=1)
    y = torch.empty(b, cout, r, r, r, device="cuda")
    part = torch.empty(int(L.lib().gldm_conv3d_partial_floats(b, cout, r)), device="cuda")
    st = L.current_stream()
    dw = (pack_conv3d_fewch_f16x2(w) if cin < 16 else pack_conv3d_f16x2(w)).cuda()
    dx, db = x.cuda(), bias.cuda()
    L.call("gldm_conv3d_k3_f16x2", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(y), L.ptr(part), st)
    assert _err(y, ref) < 2e-5, _err(y, ref)
    gn = F.group_norm(ref, 8, gamma, beta, 1e-5)
    ref2 = gn * torch.sigmoid(gn)
    dg, dbt = gamma.cuda(), beta.cuda()
    L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(part), L.ptr(dg), L.ptr(dbt), b, cout, r, 8, 1e-5, None, st)
    assert _err(y, ref2) < 2e-5, _err(y, ref2)


def test_groupnorm_folded_into_its_consumers():
    """Conv3d -> GroupNorm -> Swish -> Conv3d -> GroupNorm -> Swish -> SE sum -> devoxelize with no GroupNorm pass:
    gldm_groupnorm_coef + gldm_conv3d_k3_f16x2_gn + gldm_gn_swish_chan_sum + gldm_devoxelize_gn_fused against torch on the
    CPU (fp32, 2e-5)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d_f16x2
    g = torch.Generator().manual_seed(77)
    b, c, r, n = 3, 48, 24, 256
    x = torch.randn(b, c, r, r, r, generator=g)
    w1, w2 = (torch.randn(c, c, 3, 3, 3, generator=g) / (27 * c) ** 0.5 for _ in range(2))
    b1, b2, g1, be1, g2, be2 = (torch.randn(c, generator=g) * 0.1 for _ in range(6))
    g1, g2 = g1 + 1, g2 + 1
    h = F.group_norm(F.conv3d(x, w1, b1, padding=1), 8, g1, be1, 1e-5)
    h = h * torch.sigmoid(h)
    z = F.group_norm(F.conv3d(h, w2, b2, padding=1), 8, g2, be2, 1e-5)
    z = z * torch.sigmoid(z)
    st = L.current_stream()
    nf = int(L.lib().gldm_conv3d_partial_floats(b, c, r))
    dx = x.cuda()
    y1, y2 = torch.empty(b, c, r, r, r, device="cuda"), torch.empty(b, c, r, r, r, device="cuda")
    p1, p2 = torch.empty(nf, device="cuda"), torch.empty(nf, device="cuda")
    c1, c2 = torch.empty(b, c, 2, device="cuda"), torch.empty(b, c, 2, device="cuda")
    dw1, dw2 = pack_conv3d_f16x2(w1).cuda(), pack_conv3d_f16x2(w2).cuda()
    d = [t.cuda() for t in (b1, b2, g1, be1, g2, be2)]
    L.call("gldm_conv3d_k3_f16x2", L.ptr(dx), L.ptr(dw1), L.ptr(d[0]), b, c, c, r, L.ptr(y1), L.ptr(p1), st)
    L.call("gldm_groupnorm_coef", L.ptr(p1), L.ptr(d[2]), L.ptr(d[3]), b, c, r, 8, 1e-5, L.ptr(c1), st)
    L.call("gldm_conv3d_k3_f16x2_gn", L.ptr(y1), L.ptr(c1), L.ptr(dw2), L.ptr(d[1]), b, c, c, r, L.ptr(y2), L.ptr(p2), 0, st)
    L.call("gldm_groupnorm_coef", L.ptr(p2), L.ptr(d[4]), L.ptr(d[5]), b, c, r, 8, 1e-5, L.ptr(c2), st)
    cs = torch.empty(b, c, device="cuda")
    L.call("gldm_gn_swish_chan_sum", L.ptr(y2), L.ptr(c2), b, c, r, L.ptr(cs), st)
    assert _err(cs / r ** 3, z.mean(dim=(2, 3, 4))) < 2e-5
    # devoxelize of the activated tensor at random points, gated, plus an addend
    coords = torch.rand(b, 3, n, generator=g) * (r - 1)
    gate, add = torch.rand(b, c, generator=g), torch.randn(b, c, n, generator=g)
    out = torch.empty(b, c, n, device="cuda")
    dc, dg, da = coords.cuda(), gate.cuda(), add.cuda()
    L.call("gldm_devoxelize_gn_fused", L.ptr(dc), L.ptr(y2), L.ptr(c2), L.ptr(dg), L.ptr(da), b, c, n, r, L.ptr(out), st)
    ref = torch.empty(b, c, n, device="cuda")
    dz = z.contiguous().cuda()
    L.call("gldm_devoxelize_fused", L.ptr(dc), L.ptr(dz), L.ptr(dg), L.ptr(da), b, c, n, r, L.ptr(ref), st)
    assert _err(out, ref.cpu()) < 2e-5, _err(out, ref.cpu())
    # the same stack with the last conv writing channel-last, its squeeze as partial sums and the run-per-corner devoxelize
    y2cl, p2cl, c2cl = torch.empty(b, r ** 3, c, device="cuda"), torch.empty(nf, device="cuda"), torch.empty(b, c, 2, device="cuda")
    L.call("gldm_conv3d_k3_f16x2_gn", L.ptr(y1), L.ptr(c1), L.ptr(dw2), L.ptr(d[1]), b, c, c, r, L.ptr(y2cl), L.ptr(p2cl), 1, st)
    assert torch.equal(y2cl.view(b, r ** 3, c).permute(0, 2, 1).reshape(b, c, r, r, r), y2) and torch.equal(p2cl, p2)
    L.call("gldm_groupnorm_coef", L.ptr(p2cl), L.ptr(d[4]), L.ptr(d[5]), b, c, r, 8, 1e-5, L.ptr(c2cl), st)
    parts = int(L.lib().gldm_squeeze_parts())
    csp = torch.empty(b, parts, c, device="cuda")
    L.call("gldm_gn_swish_chan_sum_cl", L.ptr(y2cl), L.ptr(c2cl), b, c, r, L.ptr(csp), st)
    assert _err(csp.sum(1) / r ** 3, z.mean(dim=(2, 3, 4))) < 2e-5
    w1, w2 = torch.randn(6, c, generator=g) * 0.2, torch.randn(c, 6, generator=g) * 0.2
    dw1s, dw2s = w1.cuda(), w2.cuda()
    ga, gb = torch.empty(b, c, device="cuda"), torch.empty(b, c, device="cuda")
    L.call("gldm_se_gate_parts", L.ptr(csp), parts, L.ptr(dw1s), L.ptr(dw2s), b, c, 6, r, 0, L.ptr(ga), st)
    L.call("gldm_se_gate", L.ptr(cs), L.ptr(dw1s), L.ptr(dw2s), b, c, 6, r, 0, L.ptr(gb), st)
    assert _err(ga, gb.cpu()) < 1e-6
    out2 = torch.empty(b, c, n, device="cuda")
    L.call("gldm_devoxelize_gn_cl_fused", L.ptr(dc), L.ptr(y2cl), L.ptr(c2cl), L.ptr(dg), L.ptr(da), b, c, n, r, L.ptr(out2), st)
    assert _err(out2, ref.cpu()) < 2e-5, _err(out2, ref.cpu())


@pytest.mark.parametrize("cin,c,r,n", [(48, 96, 12, 100), (3, 32, 16, 77), (64, 64, 8, 1024), (128, 256, 8, 64)])
def test_channel_last_voxel_stack_tail(cin, c, r, n):
    """A voxel stack's last conv written channel-last by the f32 / split kernels (gldm_conv3d_k3_cl,
    gldm_conv3d_k3_f16x2_gn(out_channel_last)) is the channel-major output transposed, bit for bit, and the squeeze /
    devoxelize passes over it agree with the channel-major ones (ragged point counts, 12 / 16 / 24 / 64 channel quads,
    the two-launch 256-channel conv)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d, pack_conv3d_f16x2, split_conv_supported
    g = torch.Generator().manual_seed(c + r)
    b = 2
    x = torch.randn(b, cin, r, r, r, generator=g).cuda()
    w = torch.randn(c, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias, gamma, beta = (torch.randn(c, generator=g).cuda() * 0.1 for _ in range(3))
    gamma = gamma + 1
    st = L.current_stream()
    nf = int(L.lib().gldm_conv3d_partial_floats(b, c, r))
    y, ycl = torch.empty(b, c, r ** 3, device="cuda"), torch.empty(b, r ** 3, c, device="cuda")
    p, pcl = torch.empty(nf, device="cuda"), torch.empty(nf, device="cuda")
    if split_conv_supported(cin, c, r):
        dw = pack_conv3d_f16x2(w).cuda()
        L.call("gldm_conv3d_k3_f16x2", L.ptr(x), L.ptr(dw), L.ptr(bias), b, cin, c, r, L.ptr(y), L.ptr(p), st)
        L.call("gldm_conv3d_k3_f16x2_gn", L.ptr(x), None, L.ptr(dw), L.ptr(bias), b, cin, c, r, L.ptr(ycl), L.ptr(pcl), 1, st)
    else:
        dw = pack_conv3d(w).cuda()
        L.call("gldm_conv3d_k3", L.ptr(x), L.ptr(dw), L.ptr(bias), b, cin, c, r, L.ptr(y), L.ptr(p), st)
        L.call("gldm_conv3d_k3_cl", L.ptr(x), L.ptr(dw), L.ptr(bias), b, cin, c, r, L.ptr(ycl), L.ptr(pcl), st)
    assert torch.equal(ycl.permute(0, 2, 1), y) and torch.equal(pcl, p)
    coef = torch.empty(b, c, 2, device="cuda")
    L.call("gldm_groupnorm_coef", L.ptr(p), L.ptr(gamma), L.ptr(beta), b, c, r, 8, 1e-5, L.ptr(coef), st)
    cs = torch.empty(b, c, device="cuda")
    L.call("gldm_gn_swish_chan_sum", L.ptr(y), L.ptr(coef), b, c, r, L.ptr(cs), st)
    parts = int(L.lib().gldm_squeeze_parts())
    csp = torch.empty(b, parts, c, device="cuda")
    L.call("gldm_gn_swish_chan_sum_cl", L.ptr(ycl), L.ptr(coef), b, c, r, L.ptr(csp), st)
    assert _err(csp.sum(1), cs.cpu()) < 2e-5 * max(1.0, cs.abs().max().item())
    coords = (torch.rand(b, 3, n, generator=g) * (r - 1)).cuda()
    coords[:, :, 0] = r - 1
    coords[:, :, 1] = 0
    gate, add = torch.rand(b, c, generator=g).cuda(), torch.randn(b, c, n, generator=g).cuda()
    o1, o2 = torch.empty(b, c, n, device="cuda"), torch.empty(b, c, n, device="cuda")
    L.call("gldm_devoxelize_gn_fused", L.ptr(coords), L.ptr(y), L.ptr(coef), L.ptr(gate), L.ptr(add), b, c, n, r, L.ptr(o1), st)
    L.call("gldm_devoxelize_gn_cl_fused", L.ptr(coords), L.ptr(ycl), L.ptr(coef), L.ptr(gate), L.ptr(add), b, c, n, r, L.ptr(o2), st)
    assert _err(o2, o1.cpu()) < 1e-5 * max(1.0, o1.abs().max().item())


def test_ppc_config_z16_latent_against_oracle():
    """Second shipped experiment (configs/generation/partial_pc/ppc_1a_...z16_pc256: grasp latent 16,
    pc latent [3,256], denoiser dim 16 -> the L=16 time-conditioned engine): end-to-end LDM
    generation vs the torch-CPU oracle, 20 DDIM steps, identical weights / inputs / noise."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    from oracle import torch_ref as R
    ldm = build_fpc_ldm(latent=16, pc_latent=256).cuda()
    ldm.set_inference_timesteps(20)
    pcs, _ = synthetic_batch(2, 1024, partial=True)
    x_T = torch.randn(10, 1, 16, generator=torch.Generator().manual_seed(5))
    (tm, lg), _ = ldm.generate_grasps(pcs.cuda(), num_grasps=5, x_T=x_T)
    sd = {k: v.detach().cpu() for k, v in ldm.state_dict().items()}
    sched = R.make_scheduler("ddim")
    sched.set_timesteps(20)
    etm, elg = R.ldm_generate(sd, pcs, 5, sched, R.pvcnn_block_spec(0.75, 0.75), n_dims=16, x_T=x_T)
    assert _err(tm, etm) < 1e-4 and _err(lg, elg) < 1e-4, (_err(tm, etm), _err(lg, elg))


def test_infer_on_pointcloud_batched_metas_contract(ldm):
    """normalize_input (tools/inference.py:570-591) returns grasp_mean [B,6] and grasp_std [1,6]: both must
    broadcast per cloud exactly like unnormalize_grasps' unsqueeze(-2) (tools/inference.py:64-94)."""
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.synthetic import synthetic_batch
    from oracle import torch_ref as R
    pcs, _ = synthetic_batch(2, 1024)
    raw = pcs * 0.05 + torch.tensor([[0.3, -0.2, 0.7], [-0.4, 0.1, 0.2]]).unsqueeze(1)  # metres, off-centre
    inf = InferenceLDM(model=ldm, num_inference_steps=10, device="cuda:0")
    pcn, metas = inf.normalize_input(raw.cuda())
    assert metas["grasp_mean"].shape == (2, 6) and metas["grasp_std"].shape == (1, 6)
    x_T = torch.randn(6, 1, 4, generator=torch.Generator().manual_seed(3))
    out = inf.generate_grasps(pcn, metas, num_grasps=3, x_T=x_T)
    (tm, lg), _ = ldm.generate_grasps(pcn, num_grasps=3, x_T=x_T)
    cpu_metas = {k: v.cpu() for k, v in metas.items() if isinstance(v, torch.Tensor)}
    exp = R.pose_epilogue(tm.cpu(), lg.cpu(), cpu_metas, 2, 3)
    assert _err(out["grasps"], exp["grasps"]) < 1e-6
    assert _err(out["grasp_tmrp"], exp["grasp_tmrp"]) < 1e-6
    assert _err(out["confidence"], exp["confidence"]) < 1e-6
    # cloud 1 really uses ITS mean: translations differ from cloud 0's by about the mean offset
    assert (out["grasps"][1, :, :3, 3].mean(0) - out["grasps"][0, :, :3, 3].mean(0)).abs().max() > 0.2
    assert _err(out["pc"], raw) < 1e-5


def test_pose_epilogue_noncontiguous_and_shape_checks():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd.r1d import pose_epilogue
    from oracle import torch_ref as R
    g = torch.Generator().manual_seed(11)
    tm, lg = torch.randn(8, 6, generator=g), torch.randn(8, 1, generator=g)
    mean = torch.randn(6, 4, generator=g).t()            # [4,6] non-contiguous view
    std = (torch.rand(1, 12, generator=g) + 0.5)[:, ::2]  # [1,6] strided
    H, un, conf = pose_epilogue(tm.cuda(), lg.cuda(), mean.cuda(), std.cuda(), 2)
    exp = R.pose_epilogue(tm, lg, dict(grasp_mean=mean, grasp_std=std), 4, 2)
    assert _err(H.view(4, 2, 4, 4), exp["grasps"]) < 1e-6 and _err(un.view(4, 2, 6), exp["grasp_tmrp"]) < 1e-6
    with pytest.raises(RuntimeError):
        pose_epilogue(tm.cuda(), lg.cuda(), mean[:3].cuda(), std.cuda(), 2)   # 3 rows for 4 clouds
    with pytest.raises(RuntimeError):
        pose_epilogue(tm.cuda(), lg.cuda(), mean.cuda(), std.cuda(), 3)       # 8 grasps do not split by 3


def test_return_intermediate_all_steps(ldm):
    """tools/inference.py:628-641: 50 probes, each tmrp_to_H(unnormalize_grasps(step[0])) -> [1,G,4,4]."""
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.synthetic import synthetic_batch
    pcs, metas = synthetic_batch(1, 1024)
    inf = InferenceLDM(model=ldm, num_inference_steps=10, device="cuda:0")
    x_T = torch.randn(4, 1, 4, generator=torch.Generator().manual_seed(5))
    out = inf.generate_grasps(pcs, metas, num_grasps=4, return_intermediate=True, x_T=x_T)
    steps = out["all_steps_grasps"]
    assert len(steps) == 50 and steps[0].shape == (1, 4, 4, 4) and not steps[0].is_cuda
    assert _err(out["grasps"], steps[-1]) < 1e-6          # last probe = the final latent decoded
    assert (steps[0] - steps[-1]).abs().max() > 1e-3       # first probe decodes x_T
    pcs2, metas2 = synthetic_batch(2, 1024)
    with pytest.raises(NotImplementedError):
        inf.generate_grasps(pcs2, metas2, num_grasps=4, return_intermediate=True)


@pytest.mark.parametrize("b,cin,cout,n,relu,hout", [(3, 96, 768, 1024, True, 0), (2, 768, 1536, 64, True, 3),
                                                     (1, 32, 256, 32, False, 16), (5, 64, 256, 96, True, 1)])
def test_pointwise_mlp_layer_and_fused_head(b, cin, cout, n, relu, hout):
    """gldm_pointwise_mlp (k = 1 conv + folded BN + ReLU, optional head on the accumulators) vs torch-CPU f32 matmul.
    2e-5 relative to the output scale: same k-ordered f32 accumulation, different blocking."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import mfma_a_fragments
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(b, cin, n, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    bias = torch.randn(cout, generator=g)
    y_ref = torch.einsum("oc,bcn->bon", w, x) + bias.view(1, -1, 1)
    if relu:
        y_ref = y_ref.relu()
    head = None
    if hout:
        wh, bh = torch.randn(hout, cout, generator=g) / cout ** 0.5, torch.randn(hout, generator=g)
        z_ref = torch.einsum("oc,bcn->bon", wh, y_ref) + bh.view(1, -1, 1)
        head = (dense.pack_head(wh).cuda(), bh.cuda(), hout)
    assert dense.fused_mlp_supported(x.cuda(), cin, cout)
    y, z = dense.pointwise_mlp(x.cuda(), mfma_a_fragments(w).cuda(), bias.cuda(), cout, relu, head=head, keep_y=True)
    assert _err(y, y_ref) < 2e-5 * max(1.0, y_ref.abs().max().item())
    if hout:
        assert _err(z, z_ref) < 2e-5 * max(1.0, z_ref.abs().max().item())
        _, z2 = dense.pointwise_mlp(x.cuda(), mfma_a_fragments(w).cuda(), bias.cuda(), cout, relu, head=head, keep_y=False)
        assert torch.equal(z, z2)   # the head does not depend on whether y is also written


@pytest.mark.parametrize("b,cin0,cin,cout,n,hout", [(2, 96, 768, 1536, 64, 3), (3, 32, 256, 256, 96, 0),
                                                    (1, 64, 512, 768, 32, 16)])
def test_pointwise_mlp_two_layers_one_launch(b, cin0, cin, cout, n, hout):
    """gldm_pointwise_mlp2: relu(W1 relu(W0 x + b0) + b1) (+ head) with the middle tensor kept in LDS, against the
    same two layers as separate gldm_pointwise_mlp launches (bit-identical: same GEMM core, same k order) and against
    a torch-CPU f32 reference (2e-5 of the output scale)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import mfma_a_fragments
    g = torch.Generator().manual_seed(cin0 + cin + cout)
    x = torch.randn(b, cin0, n, generator=g)
    w0, b0 = torch.randn(cin, cin0, generator=g) / cin0 ** 0.5, torch.randn(cin, generator=g)
    w1, b1 = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    h_ref = (torch.einsum("oc,bcn->bon", w0, x) + b0.view(1, -1, 1)).relu()
    y_ref = (torch.einsum("oc,bcn->bon", w1, h_ref) + b1.view(1, -1, 1)).relu()
    head = None
    if hout:
        wh, bh = torch.randn(hout, cout, generator=g) / cout ** 0.5, torch.randn(hout, generator=g)
        z_ref = torch.einsum("oc,bcn->bon", wh, y_ref) + bh.view(1, -1, 1)
        head = (dense.pack_head(wh).cuda(), bh.cuda(), hout)
    xc, p0, p1 = x.cuda(), mfma_a_fragments(w0).cuda(), mfma_a_fragments(w1).cuda()
    assert dense.fused_mlp2_supported(xc, cin0, cin, cout)
    y, z = dense.pointwise_mlp(xc, p1, b1.cuda(), cout, True, head=head, keep_y=True, front=(p0, b0.cuda(), cin))
    h = dense.pointwise_mlp(xc, p0, b0.cuda(), cin, True)[0]
    y2, z2 = dense.pointwise_mlp(h, p1, b1.cuda(), cout, True, head=head, keep_y=True)
    assert _err(y, y_ref) < 2e-5 * max(1.0, y_ref.abs().max().item())
    assert torch.equal(y, y2)
    if hout:
        assert _err(z, z_ref) < 2e-5 * max(1.0, z_ref.abs().max().item())
        assert torch.equal(z, z2)


@pytest.mark.parametrize("b,cin0,cin,cout,n,hout", [(2, 96, 768, 1536, 64, 3), (3, 32, 256, 256, 96, 0),
                                                    (1, 64, 512, 768, 32, 16), (5, 96, 256, 512, 2048, 3),
                                                    (2, 0, 128, 256, 64, 0), (1, 0, 768, 1536, 96, 3),
                                                    (5, 0, 128, 256, 2048, 0), (5, 32, 256, 256, 2048, 0),
                                                    (3, 0, 128, 128, 1024, 0), (2, 0, 256, 128, 512, 0), (1, 0, 128, 64, 32, 0),
                                                    (2, 0, 256, 224, 64, 0),
                                                    # round 6: K zero-padded to the ring's 128 (cin 48 / 64 / 320), units of
                                                    # one m-tile below 256 rows (cout 96 / 80 / 240)
                                                    (3, 0, 48, 96, 1024, 0), (2, 0, 64, 128, 512, 0), (1, 0, 320, 80, 96, 0),
                                                    (2, 0, 64, 240, 64, 0)])
def test_pointwise_mlp_split_f16(b, cin0, cin, cout, n, hout):
    """gldm_pointwise_mlp_f16x2 / gldm_pointwise_mlp2_f16x2 (both layers on the bf16 matrix pipe, every f32 operand
    split exactly into three bf16 numbers; units of output rows handed out to the waves at run time) against a torch-CPU
    reference computed in f64: 2e-5 of the output scale, like the f32-pipe form.  (5, ..., 2048): 320 tiles on 256
    workgroups, i.e. some workgroups take a second tile.  cout 64 / 128 / 224: fewer units of output rows than waves (the
    128-row feature-propagation layers of the PointNet++-style backbones)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import mfma_a_fragments_f16x2
    g = torch.Generator().manual_seed(7 + cin0 + cin + cout)
    c_in = cin0 if cin0 else cin
    x = torch.randn(b, c_in, n, generator=g)
    w1, b1 = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    front = None
    h_ref = x.double()
    if cin0:
        w0, b0 = torch.randn(cin, cin0, generator=g) / cin0 ** 0.5, torch.randn(cin, generator=g)
        h_ref = (torch.einsum("oc,bcn->bon", w0.double(), h_ref) + b0.double().view(1, -1, 1)).relu().float().double()
        front = (mfma_a_fragments_f16x2(w0).cuda(), b0.cuda(), cin)
    y_ref = (torch.einsum("oc,bcn->bon", w1.double(), h_ref) + b1.double().view(1, -1, 1)).relu()
    head = None
    if hout:
        wh, bh = torch.randn(hout, cout, generator=g) / cout ** 0.5, torch.randn(hout, generator=g)
        z_ref = (torch.einsum("oc,bcn->bon", wh.double(), y_ref) + bh.double().view(1, -1, 1)).float()
        head = (dense.pack_head(wh).cuda(), bh.cuda(), hout)
    assert dense.split_supported(cin, cin0)
    w1s = (dense.split_fragments(w1) if cin0 == 0 else mfma_a_fragments_f16x2(w1)).cuda()   # (K padded where cin % 128 != 0)
    y, z = dense.pointwise_mlp(x.cuda(), w1s, b1.cuda(), cout, True, head=head, keep_y=True,
                               front=front, split=True)
    assert _err(y, y_ref.float()) < 2e-5 * max(1.0, y_ref.abs().max().item())
    if hout:
        assert _err(z, z_ref) < 2e-5 * max(1.0, z_ref.abs().max().item())
        # the head sum does not depend on which wave drew which unit of output rows: bitwise repeatable
        for _ in range(3):
            _, z2 = dense.pointwise_mlp(x.cuda(), w1s, b1.cuda(), cout, True, head=head,
                                        keep_y=False, front=front, split=True)
            assert torch.equal(z2, z)


@pytest.mark.parametrize("b,ca,na,cb,n,cout", [(3, 128, 1024, 3, 1024, 128), (2, 256, 128, 3, 128, 256), (4, 1024, 1, 256, 128, 256),
                                               (2, 128, 64, 6, 64, 64), (2, 256, 512, 128, 512, 256), (3, 128, 96, 128, 96, 64),
                                               (32, 1024, 1, 256, 64, 256)])
def test_first_layer_of_a_concatenation_without_the_concatenation(b, ca, na, cb, n, cout):
    """dense.concat_conv_bn_relu: relu(BN(conv(cat([xa, xb])))) as the split-f16 launch over the wide part with the other
    part as its addend (gldm_pointwise_mlp_f16x2_add) -- a few coordinate rows as a [B, Cout, N] tensor, or ONE centre's
    feature vector as a per-cloud bias (what nearest-neighbour interpolation from a single centre broadcasts) -- against
    torch on the CPU in f64 (2e-5 of the output scale)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import torch.nn as nn
    from graspldm_amd import dense
    g = torch.Generator().manual_seed(ca + cb + cout)
    conv, bn = nn.Conv1d(ca + cb, cout, 1), nn.BatchNorm1d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, ca + cb, 1, generator=g) / (ca + cb) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g) * 0.1)
        bn.weight.copy_(1 + 0.1 * torch.randn(cout, generator=g)); bn.bias.copy_(0.1 * torch.randn(cout, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(cout, generator=g)); bn.running_var.copy_(1 + 0.2 * torch.rand(cout, generator=g))
    conv.eval(); bn.eval()
    xa, xb = torch.randn(b, ca, na, generator=g), torch.randn(b, cb, n, generator=g)
    cat = torch.cat([xa.expand(b, ca, n) if na == 1 else xa, xb], dim=1).double()
    ref = bn.double()(conv.double()(cat)).relu().float()
    conv.float(); bn.float()
    conv, bn = conv.cuda(), bn.cuda()
    y = dense.concat_conv_bn_relu(xa.cuda(), xb.cuda(), conv, bn)
    assert y is not None
    assert _err(y, ref) < 2e-5 * max(1.0, ref.abs().max().item()), _err(y, ref)
    # shapes outside the two forms are declined (the caller concatenates)
    assert dense.concat_conv_bn_relu(xa.cuda()[:, :, : max(1, na // 2)], xb.cuda(), conv, bn) is None or na == 1


def test_pointwise_mlp_rejects_unsupported_shapes():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graspldm_amd import _lib as L
    x = torch.zeros(1, 48, 64, device="cuda")
    w = torch.zeros(256 * 48, device="cuda")
    bias = torch.zeros(256, device="cuda")
    y = torch.zeros(1, 256, 64, device="cuda")
    with pytest.raises(L.GldmError, match="shape not supported"):   # cin % 32 != 0
        L.call("gldm_pointwise_mlp", L.ptr(x), L.ptr(w), L.ptr(bias), 1, 48, 256, 64, 1, None, None, 0, L.ptr(y), None,
               L.current_stream(x.device))
    with pytest.raises(L.GldmError):                           # neither y nor a head
        L.call("gldm_pointwise_mlp", L.ptr(x), L.ptr(w), L.ptr(bias), 1, 64, 256, 64, 1, None, None, 0, None, None,
               L.current_stream(x.device))


def test_pvcnn2_encoder_repaired_form():
    """PVCNN2Encoder (the reference's cannot be constructed: SURVEY F2).  Backbone = PVCNN2 with the golden's weights
    (pinned to the reference's graph by test_g8_pvcnn2_golden), head = conv_downscale -> out_layer (pc_encoders.py:
    104-111) recomputed with torch on the CPU from the backbone's features; scale arguments are honoured or rejected."""
    import torch.nn.functional as F
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    from graspldm_amd.synthetic import synthetic_state_dict, synthetic_tensor
    g = load_golden("pvcnn2.npz")
    enc = PVCNN2Encoder(in_features=3, out_features=64, n_points=1024, scale_channels=1, scale_voxel_resolution=1,
                        out_channels=3)
    bb_sd = synthetic_state_dict(load_schema("schema_pvcnn2.json"), seed=4)
    enc.pvcnn_modules.load_state_dict(bb_sd, strict=True)
    head = {k: synthetic_tensor("enc2." + k, v.shape, seed=6) for k, v in enc.state_dict().items()
            if not k.startswith("pvcnn_modules.")}
    enc.load_state_dict({**{"pvcnn_modules." + k: v for k, v in bb_sd.items()}, **head}, strict=True)
    enc = enc.cuda().eval()
    pc = g["coords"].transpose(1, 2).contiguous()          # [1, N, 3]
    with torch.no_grad():
        z = enc(pc.cuda())
        feat = enc.pvcnn_modules(g["coords"].cuda())
    assert _err(feat[:, :, ::16], g["out"]) < 1e-4         # same backbone as the golden
    f = feat.cpu().double()
    h = F.conv1d(f, head["conv_downscale.weight"].double(), head["conv_downscale.bias"].double())
    h = F.conv1d(h, head["out_layer.0.weight"].double(), head["out_layer.0.bias"].double())
    exp = F.linear(h, head["out_layer.1.weight"].double(), head["out_layer.1.bias"].double()).float()
    assert z.shape == (1, 3, 64) and _err(z, exp) < 5e-5, _err(z, exp)
    # half width / half resolution builds and runs (the reference's benchmark setting); foreign arguments are rejected
    small = PVCNN2Encoder(out_features=16, n_points=1024, scale_channels=0.5, scale_voxel_resolution=0.5).cuda().eval()
    assert small.pvcnn_modules.out_channels == 32
    with torch.no_grad():
        zs = small(pc.cuda())
    assert zs.shape == (1, 16) and torch.isfinite(zs).all()
    with pytest.raises(NotImplementedError):
        PVCNN2Encoder(num_blocks=(2, 1, 1, 1))
    with pytest.raises(NotImplementedError):
        PVCNN2Encoder(is_conditioned=True, cond_dims=8)


@pytest.mark.parametrize("cin,cout,n,relu", [(3, 48, 1024, True), (48, 96, 1024, True), (6, 20, 333, False), (64, 7, 4096, True)])
def test_pointwise_small_kernel(cin, cout, n, relu):
    """gldm_pointwise_small (narrow k = 1 conv: the PVConv point branches) against torch on the CPU: k-ordered fma chain
    vs a BLAS dot product, 2e-6 relative to the row's magnitude."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(cin + cout)
    x, w, b = torch.randn(3, cin, n, generator=g), torch.randn(cout, cin, generator=g), torch.randn(cout, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y = torch.empty(3, cout, n, device="cuda")
    L.call("gldm_pointwise_small", L.ptr(xd), L.ptr(wd), L.ptr(bd), 3, cin, cout, n, int(relu), L.ptr(y), L.current_stream())
    exp = torch.einsum("oc,bcn->bon", w.double(), x.double()) + b.double().view(1, -1, 1)
    exp = exp.clamp_min(0) if relu else exp
    assert _err(y, exp.float()) < 2e-6 * (1 + exp.abs().max().item())


def test_linear_rows_kernel():
    """gldm_linear_rows (out_layer[1]: Linear over the point axis) against torch on the CPU."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    for rows, n, nout in [(6, 1024, 64), (5, 4096, 256), (2, 64, 300)]:
        x, w, b = torch.randn(rows, n, generator=g), torch.randn(nout, n, generator=g) / n ** 0.5, torch.randn(nout, generator=g)
        y = torch.empty(rows, nout, device="cuda")
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        L.call("gldm_linear_rows", L.ptr(xd), L.ptr(wd), L.ptr(bd), rows, n, nout, L.ptr(y), L.current_stream())
        exp = (x.double() @ w.double().T + b.double()).float()
        assert _err(y, exp) < (5e-6 if n <= 1024 else 2e-5), (rows, n, nout, _err(y, exp))


def test_voxel_conv_without_mfma_instantiation_runs_the_direct_kernel():
    """A PVConv whose voxel shape has no MFMA instantiation (40 channels: not a multiple of 16) runs the direct kernel
    (gldm_conv3d_k3_generic), not a library fallback; so does a resolution that is not a multiple of the 4 x 4 x r brick
    (partial edge bricks; r^3 not a multiple of 4 takes GroupNorm's scalar pass)."""
    from graspldm_amd.pvcnn import PVConv
    from graspldm_amd.synthetic import load_synthetic_weights
    m = load_synthetic_weights(PVConv(8, 40, 3, 8, with_se=True), seed=2).cuda().eval()
    g = torch.Generator().manual_seed(4)
    feats, coords = torch.randn(2, 8, 256, generator=g), torch.rand(2, 3, 256, generator=g) * 2 - 1
    with torch.no_grad():
        out, _ = m((feats.cuda(), coords.cuda()))
    assert out.shape == (2, 40, 256) and torch.isfinite(out).all()
    # the voxel branch on the CPU from the module's own pieces
    from oracle import torch_ref as R
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    exp = R.pvconv(sd, "", feats, coords, 8, True, False)
    exp = exp[0] if isinstance(exp, tuple) else exp
    assert _err(out, exp) < 2e-5, _err(out, exp)
    for cout, r, se in ((16, 6, False), (24, 9, True), (48, 18, True)):
        odd = load_synthetic_weights(PVConv(8, cout, 3, r, with_se=se), seed=3).cuda().eval()
        with torch.no_grad():
            out, _ = odd((feats.cuda(), coords.cuda()))
        sd = {k: v.detach().cpu() for k, v in odd.state_dict().items()}
        exp = R.pvconv(sd, "", feats, coords, r, True, False)
        exp = exp[0] if isinstance(exp, tuple) else exp
        assert out.shape == (2, cout, 256) and _err(out, exp) < 2e-5, (cout, r, _err(out, exp))


def test_ldm_end_to_end_with_the_set_abstraction_encoder():
    """GraspLatentDDM.generate_grasps conditioned by the SET-ABSTRACTION encoder family (north star: FPS / ball query /
    grouped set-abstraction MLPs conditioning the VAE): PVCNN2Encoder in its repaired form.  Backbone weights = the golden's,
    which test_g8_pvcnn2_golden pins to the reference's own PVCNN2 graph (checked again here on both clouds of the batch:
    pvcnn2.npz's and, as the encoder sees it, the normalised synthetic one of pvcnn2_b.npz); the expectation continues from the backbone's features on the CPU: the encoder head in f64 (pc_encoders.py:104-111), then
    the oracle's 100 DDIM steps and decoder (grasp_ldm.py:189-233).  Poses 1e-4."""
    import torch.nn.functional as F
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch, synthetic_state_dict
    from oracle import torch_ref as R
    g = load_golden("pvcnn2.npz")
    ldm = build_fpc_ldm(encoder="PVCNN2Encoder")
    enc = ldm.vae_model.encoder.pc_encoder
    enc.pvcnn_modules.load_state_dict(synthetic_state_dict(load_schema("schema_pvcnn2.json"), seed=4), strict=True)
    ldm = ldm.cuda().eval()
    ldm.set_inference_timesteps(100)
    G = 8
    extra, _ = synthetic_batch(1, 1024)
    pc = torch.cat([g["coords"].transpose(1, 2), extra]).contiguous()     # [2, N, 3]: the golden cloud and a synthetic one
    x_T = torch.randn(2 * G, 1, 4, generator=torch.Generator().manual_seed(3))
    (tm, lg), _ = ldm.generate_grasps(pc.cuda(), num_grasps=G, x_T=x_T)
    ldm.check_engines()
    with torch.no_grad():
        feat = enc.pvcnn_modules(pc.transpose(1, 2).contiguous().cuda())
        z_hip = enc(pc.cuda())
    assert _err(feat[:1, :, ::16], g["out"]) < 1e-4                       # the reference's backbone
    gb = load_golden("pvcnn2_b.npz")                                      # ... and on the second cloud, from which the
    assert torch.equal(gb["coords"], pc[1:2].transpose(1, 2))             # expectation below continues
    assert _err(feat[1:2, :, ::16], gb["out"]) < 1e-4, _err(feat[1:2, :, ::16], gb["out"])
    sd = {k: v.detach().cpu() for k, v in ldm.state_dict().items()}
    p = "vae_model.encoder.pc_encoder."
    h = F.conv1d(feat.cpu().double(), sd[p + "conv_downscale.weight"].double(), sd[p + "conv_downscale.bias"].double())
    h = F.conv1d(h, sd[p + "out_layer.0.weight"].double(), sd[p + "out_layer.0.bias"].double())
    z = F.linear(h, sd[p + "out_layer.1.weight"].double(), sd[p + "out_layer.1.bias"].double()).float()
    assert z.shape == (2, 3, 64) and _err(z_hip, z) < 5e-5, _err(z_hip, z)
    zr = z.repeat_interleave(G, dim=0)
    sched = R.make_scheduler("ddim")
    sched.set_timesteps(100)
    x, _ = R.sample_latents(sd, "diffusion_model.model.", zr, sched, 4, x_T=x_T)
    etm, elg = R.decoder_forward(sd, "vae_model.decoder.", x.squeeze(-2), zr)
    assert tm.shape == (2 * G, 6) and _err(tm, etm) < 1e-4 and _err(lg, elg) < 1e-4, (_err(tm, etm), _err(lg, elg))


def test_pvcnn2_encoder_default_constructor_runs():
    """The registry encoder as it is default-constructed (scale_channels 0.25, scale_voxel_resolution 0.75: PVConv
    resolutions 24, 12 and 6 -- 6 is not a multiple of the voxel kernels' 4 x 4 x r brick) builds and runs."""
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    from graspldm_amd.pvcnn import PVConv
    from graspldm_amd.synthetic import load_synthetic_weights, synthetic_batch
    enc = load_synthetic_weights(PVCNN2Encoder(), seed=9).cuda().eval()
    assert sorted({m.resolution for m in enc.modules() if isinstance(m, PVConv)}) == [6, 12, 24]
    pcs, _ = synthetic_batch(2, 1024)
    with torch.no_grad():
        z = enc(pcs.cuda())
    assert z.shape == (2, 32) and torch.isfinite(z).all()


@pytest.mark.parametrize("b,cin,cout,n,relu", [(3, 384, 256, 128, True), (2, 131, 70, 333, False), (1, 5, 130, 64, True),
                                               (2, 640, 256, 1024, True), (4, 17, 16, 50, False)])
def test_pointwise_any_kernel(b, cin, cout, n, relu):
    """gldm_pointwise_any (any-shape k = 1 conv on the f32 matrix pipe: the feature-propagation SharedMLPs of PointNet++ /
    PVCNN2, ragged rows / channels / points) against torch on the CPU: a k-ordered f32 fma chain vs a BLAS dot product."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(cin + cout)
    x, w, bias = torch.randn(b, cin, n, generator=g), torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    y = torch.full((b, cout, n), float("nan"), device="cuda")
    L.call("gldm_pointwise_any", L.ptr(xd), L.ptr(wd), L.ptr(bd), b, cin, cout, n, int(relu), L.ptr(y), L.current_stream())
    exp = torch.einsum("oc,bcn->bon", w.double(), x.double()) + bias.double().view(1, -1, 1)
    exp = exp.clamp_min(0) if relu else exp
    assert _err(y, exp.float()) < 3e-6 * (1 + exp.abs().max().item()), _err(y, exp.float())
    y2 = torch.empty_like(y)
    L.call("gldm_pointwise_any", L.ptr(xd), L.ptr(wd), None, b, cin, cout, n, 0, L.ptr(y2), L.current_stream())
    assert _err(y2, torch.einsum("oc,bcn->bon", w.double(), x.double()).float()) < 3e-6 * (1 + exp.abs().max().item())


@pytest.mark.parametrize("b,c,n", [(3, 1024, 128), (2, 7, 33), (1, 1, 1), (4, 256, 4096)])
def test_row_max_kernel(b, c, n):
    """gldm_row_max = x.max(dim=-1, keepdim=True).values (PointNetAModule's global pooling, pointnet.py:40-44): exact, NaN
    propagating like torch.max."""
    from graspldm_amd import dense
    g = torch.Generator().manual_seed(b + c + n)
    x = torch.randn(b, c, n, generator=g)
    x[0, 0, n // 2] = 1e30
    if c > 1:
        x[-1, 1, 0] = float("nan")
    got = dense.row_max(x.cuda()).cpu()
    exp = x.max(dim=-1, keepdim=True).values
    assert got.shape == exp.shape and torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(exp, nan=-7.0))


def test_dense_layers_make_no_library_call():
    """SharedMLP / Linear shapes outside the fused launches (feature-propagation widths, an odd row length) and SE3d on its
    own run hand-written kernels and agree with torch on the CPU; the package no longer imports torch.nn.functional's conv /
    linear on any device path."""
    import inspect
    import torch.nn as nn
    from graspldm_amd import dense, pvcnn
    assert "F.conv1d" not in inspect.getsource(dense) and "F.linear" not in inspect.getsource(dense)
    assert "TF." not in inspect.getsource(pvcnn)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 384, 128, generator=g)
    conv, bn = nn.Conv1d(384, 256, 1), nn.BatchNorm1d(256)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(256, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(256, generator=g) + 0.5)
    conv.eval(), bn.eval()
    with torch.no_grad():
        exp = torch.relu(bn(conv(x)))
        got = dense.pointwise_conv_bn_relu(x.cuda(), conv.cuda(), bn.cuda())
    assert _err(got, exp) < 2e-5
    lin = nn.Linear(333, 20)
    xr = torch.randn(3, 5, 333, generator=g)
    with torch.no_grad():
        assert _err(dense.linear(xr.cuda(), lin.cuda()), lin.cpu()(xr)) < 2e-5
    se = pvcnn.SE3d(32)
    v = torch.randn(2, 32, 4, 4, 4, generator=g)
    with torch.no_grad():
        m = v.mean(dim=(2, 3, 4))
        h = m @ se.fc[0].weight.T
        h = h * torch.sigmoid(h)
        exp_se = v * torch.sigmoid(h @ se.fc[2].weight.T).view(2, 32, 1, 1, 1)
        assert _err(se.cuda()(v.cuda()), exp_se) < 2e-6


def test_standalone_wide_layer_with_narrow_input_runs_the_f32_launch():
    """A SharedMLP layer with cin % 32 == 0, cin < 128 and cout % 256 == 0 (PVCNN at half width: 64 -> 256) keeps split
    fragments only for use as a FRONT layer; on its own it runs the f32 MFMA launch (the split launch needs cin % 128 == 0)."""
    import torch.nn as nn
    from graspldm_amd import dense
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 1024, generator=g)
    conv, bn = nn.Conv1d(64, 256, 1), nn.BatchNorm1d(256)
    conv.eval(), bn.eval()
    with torch.no_grad():
        exp = torch.relu(bn(conv(x)))
        got = dense.pointwise_conv_bn_relu(x.cuda(), conv.cuda(), bn.cuda())
    assert _err(got, exp) < 2e-5


def test_f32_only_switch_runs_the_exact_f32_kernels(ldm):
    """numerics.f32_only(): the same module API on the f32 matrix pipe everywhere (descriptor without split copies ->
    sample-major engine; SA / pointwise / voxel launches on their f32 forms).  Both paths meet the reference's vectors; they
    differ from each other in the last bits only."""
    from graspldm_amd import numerics
    from graspldm_amd.r1d import R1dEngine, pack_resnet1d
    from graspldm_amd import _lib as L
    g = load_golden("ldm_e2e.npz")
    with numerics.f32_only():
        m = build_fpc(scheduler="ddim")
        m.load_state_dict(ldm.state_dict(), strict=True)
        m = m.cuda().eval()
        m.set_inference_timesteps(100)
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        packed = pack_resnet1d(sd, "diffusion_model.model.", groups=4, seq_len=4, num_steps=1000)
        assert L.lib().gldm_r1d_tile_columns(R1dEngine(packed, "cuda:0")._desc_ptr()) == 32
        torch.manual_seed(int(g["seed"]))
        (tm, lg), _ = m.generate_grasps(g["pc"].cuda(), num_grasps=20)
    assert numerics.split_enabled()
    ldm.set_inference_timesteps(100)
    torch.manual_seed(int(g["seed"]))
    (tm2, lg2), _ = ldm.generate_grasps(g["pc"].cuda(), num_grasps=20)
    assert _err(tm, g["tmrp"]) < 1e-4 and _err(tm2, g["tmrp"]) < 1e-4
    assert (tm - tm2).abs().max().item() < 5e-5
    assert not torch.equal(tm, tm2)   # another summation, not the same bits
