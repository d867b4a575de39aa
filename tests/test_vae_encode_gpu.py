"""GPU (MI355X): the grasp-encoder path -- gldm_pose_prologue, gldm_encode (R1dEngine.encode), GraspCVAE.encode /
.forward(compute_loss=False), GraspLatentDDM.refine_grasps and the harness on top -- against the reference's golden
vectors (tests/golden/vae_encode.npz, H_to_tmrp.npz) and the torch-CPU oracle composition on fresh seeded inputs.
Tolerances are the project's (tests/test_r1d_gpu.py): 2e-5 absolute for one forward of O(1) values, 1e-4 for a
multi-step trajectory and for poses; the rotation prologue's 2e-6 is derived at its test."""
import contextlib

import pytest
import torch

from conftest import load_golden, load_schema
from test_vae_encode_cpu import ENC, PC, _encoder_arg, oracle_encode

pytestmark = pytest.mark.gpu

DEC = "vae_model.decoder."
DEN = "diffusion_model.model."


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _err(a, b):
    return (a.detach().cpu().double() - b.double()).abs().max().item()


def _mode(f32):
    from graspldm_amd import numerics
    return numerics.f32_only() if f32 else contextlib.nullcontext()


def _engine(sd, cond_rows=3):
    from graspldm_amd.r1d import R1dEngine, pack_resnet1d
    return R1dEngine(pack_resnet1d(sd, ENC + "net.", groups=4, seq_len=16, cond_rows=cond_rows,
                                   encoder=_encoder_arg(sd)), "cuda:0")


def _dbl(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ 6. rotations

def _h_to_tmrp_f64(H):
    """rotmat_to_mrp restated in f64 from the published SciPy algorithm (arg-max over the diagonal and the trace, the
    four branch formulas, normalise, q.xyz / (1 + q.w)); the test's own reference for the normalised rows."""
    H = H.double()
    R = H[:, :3, :3]
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    dec = torch.stack([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2], tr], -1)
    ch = dec.argmax(-1)
    q = torch.zeros(H.shape[0], 4, dtype=torch.float64)
    for n in range(H.shape[0]):
        i = int(ch[n])
        if i == 3:
            q[n] = torch.stack([R[n, 2, 1] - R[n, 1, 2], R[n, 0, 2] - R[n, 2, 0], R[n, 1, 0] - R[n, 0, 1], 1 + tr[n]])
        else:
            j, k = (i + 1) % 3, (i + 2) % 3
            q[n, i] = 1 - tr[n] + 2 * R[n, i, i]
            q[n, j] = R[n, j, i] + R[n, i, j]
            q[n, k] = R[n, k, i] + R[n, i, k]
            q[n, 3] = R[n, k, j] - R[n, j, k]
    q = q / q.norm(dim=1, keepdim=True)
    return torch.cat([H[:, :3, 3], q[:, :3] / (1 + q[:, 3:])], -1)


def test_h_to_tmrp_golden_and_round_trip():
    """rotations.H_to_tmrp against the reference's on the 88 poses whose branch f32 rounding cannot move, and the round
    trip through tmrp_to_H on all 96 (at a tie another branch is the same rotation).  2e-6: the reference's own f32
    H_to_tmrp sits 4.3e-7 from its f64 evaluation on 5,116 poses of the fixture's recipe (|m| up to 2.39; round trip
    3.9e-7); two f32 evaluations in different operation order can be twice that apart, and the bar leaves a factor of
    two over that."""
    from graspldm_amd import rotations
    g = load_golden("H_to_tmrp.npz")
    n_tie = int(g["n_tie"])
    got = rotations.H_to_tmrp(g["H"].cuda())
    assert got.shape == (96, 6) and torch.isfinite(got).all()
    e = _err(got[:-n_tie], g["tmrp"][:-n_tie])
    back = rotations.tmrp_to_H(got)
    rt = _err(back, g["H"])
    print(f"H_to_tmrp vs reference {e:.2e}; round trip {rt:.2e}")
    assert e < 2e-6, e
    assert rt < 2e-6, rt
    assert rotations.H_to_tmrp(g["H"].cuda().view(2, 48, 4, 4)).shape == (2, 48, 6)


@pytest.mark.parametrize("with_label", [True, False])
def test_pose_prologue_per_cloud_normalisation(with_label):
    """((t, mrp) - mean) / std with per-cloud rows, label appended or not, against the f64 evaluation: 2e-6 divided by
    the column's std (the bar of the un-normalised row, carried through the division)."""
    from graspldm_amd.r1d import pose_prologue
    g = load_golden("H_to_tmrp.npz")
    H = g["H"][:88]                                   # 8 clouds x 11 grasps, none of the tie group
    gen = torch.Generator().manual_seed(17)
    mean = 0.2 * torch.randn(8, 6, generator=gen)
    std = 0.05 + 0.45 * torch.rand(8, 6, generator=gen)
    label = (torch.rand(88, generator=gen) < 0.5).float() if with_label else None
    got = pose_prologue(H.cuda(), None if label is None else label.cuda(), mean.cuda(), std.cuda(), 11)
    assert got.shape == (88, 7 if with_label else 6)
    ref = (_h_to_tmrp_f64(H).view(8, 11, 6) - mean.double().unsqueeze(1)) / std.double().unsqueeze(1)
    rel = ((got[:, :6].cpu().double().view(8, 11, 6) - ref).abs() * std.double().unsqueeze(1)).max().item()
    print(f"pose_prologue: worst |error| x std = {rel:.2e}")
    assert rel < 2e-6, rel
    if with_label:
        assert torch.equal(got[:, 6].cpu(), label)
    # a [1,6] std broadcasts against a [8,6] mean like pose_epilogue's
    got1 = pose_prologue(H.cuda(), None, mean.cuda(), std[:1].cuda(), 11)
    ref1 = (_h_to_tmrp_f64(H).view(8, 11, 6) - mean.double().unsqueeze(1)) / std[:1].double().unsqueeze(1)
    assert ((got1.cpu().double().view(8, 11, 6) - ref1).abs() * std[:1].double().unsqueeze(1)).max().item() < 2e-6
    with pytest.raises(RuntimeError):
        pose_prologue(H.cuda(), None, mean.cuda(), std.cuda(), 10)


# ------------------------------------------------------------------------------------------------ 7. golden

@pytest.mark.parametrize("f32", [False, True])
def test_vae_encode_golden_engine_and_model(f32, fpc_state_dict):
    g = load_golden("vae_encode.npz")
    with _mode(f32):
        eng = _engine(fpc_state_dict)
        mu, logvar, z = eng.encode(g["h"].cuda(), eng.cond_embed(g["z_pc"].cuda()), 8, eps=g["eps"].cuda())
        errs = (_err(mu, g["mu"]), _err(logvar, g["logvar"]), _err(z, g["z"]))
        print(f"engine f32_only={f32}: mu {errs[0]:.2e} logvar {errs[1]:.2e} z {errs[2]:.2e}")
        assert max(errs) < 2e-5, errs
        mu2, logvar2, z2 = eng.encode(g["h"].cuda(), eng.cond_embed(g["z_pc"].cuda()), 8, want_z=False)
        assert z2 is None and torch.equal(mu2, mu) and torch.equal(logvar2, logvar)
        from graspldm_amd.pipeline import build_fpc_ldm
        vae = build_fpc_ldm(device="cuda:0").vae_model
        (m, lv, zz), (a, b, z_pc) = vae.encode(g["pc"].cuda(), g["h"].cuda(), eps=g["eps"].cuda())
        assert a is None and b is None and z_pc.shape == (16, 3, 64)
        assert _err(z_pc[::8], g["z_pc"]) < 2e-5 and torch.equal(z_pc[0], z_pc[7])
        errs = (_err(m, g["mu"]), _err(lv, g["logvar"]), _err(zz, g["z"]))
        print(f"model  f32_only={f32}: mu {errs[0]:.2e} logvar {errs[1]:.2e} z {errs[2]:.2e}")
        assert max(errs) < 2e-5, errs
        # eps=None draws on the CPU generator: torch.manual_seed reproduces the reference's randn_like stream
        torch.manual_seed(int(g["seed"]))
        (_, _, zs), _ = vae.encode(g["pc"].cuda(), g["h"].cuda())
        assert torch.equal(zs, zz)
        torch.manual_seed(int(g["seed"]))
        tmrp, logit = vae(g["pc"].cuda(), g["h"].cuda(), compute_loss=False)
        errs = (_err(tmrp, g["tmrp"]), _err(logit, g["logit"]))
        print(f"forward f32_only={f32}: tmrp {errs[0]:.2e} logit {errs[1]:.2e}")
        assert max(errs) < 2e-5, errs
        # the pieces on their own (reference shapes)
        zg, zrep = vae.encoder(g["pc"].cuda(), g["h"].cuda())
        assert zg.shape == (16, 1, 4) and zrep.shape == (16, 3, 64)
        m3, lv3 = vae.bottleneck(zg.squeeze(-2))
        assert _err(m3, g["mu"]) < 2e-5 and _err(lv3, g["logvar"]) < 2e-5


# ------------------------------------------------------------------------------------------------ 8. fresh inputs

@pytest.mark.parametrize("spc", [1, 20])
def test_encode_ragged_batch_against_oracle(spc, fpc_state_dict):
    sd = fpc_state_dict
    gen = torch.Generator().manual_seed(8 + spc)
    n = 37                                                   # not a multiple of the 4-sample tile
    n_cond = (n + spc - 1) // spc
    h = torch.randn(n, 7, generator=gen)
    h[:, 6] = (torch.rand(n, generator=gen) < 0.5).float()
    zc = torch.randn(n_cond, 3, 64, generator=gen)
    eps = torch.randn(n, 4, generator=gen)
    mu_e, lv_e = oracle_encode(sd, h, zc.repeat_interleave(spc, dim=0)[:n])
    eng = _engine(sd)
    mu, lv, z = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), spc, eps=eps.cuda())
    errs = (_err(mu, mu_e), _err(lv, lv_e), _err(z, mu_e + eps * torch.exp(0.5 * lv_e)))
    print(f"n=37 spc={spc}: {errs}")
    assert max(errs) < 2e-5, errs
    # add_noise form of the mix: z = a mu + s eps, no std
    mu, lv, z = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), spc, eps=eps.cuda(), mix=(0.8, 0.6), eps_times_std=False)
    assert _err(z, 0.8 * mu_e + 0.6 * eps) < 2e-5
    _, _, z = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), spc, mix=(1.0, 1.0))
    assert torch.equal(z, mu)                                # eps None: z = mix_mu * mu


def test_encode_ppc_schema_against_oracle():
    """The partial-cloud experiment's encoder: latent 16 (a 32-row head), 256-wide cloud latent."""
    from graspldm_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(load_schema("schema_ppc_ldm.json"), seed=0)
    gen = torch.Generator().manual_seed(16)
    n = 37
    h = torch.randn(n, 7, generator=gen)
    zc = torch.randn(n, 3, 256, generator=gen)
    eps = torch.randn(n, 16, generator=gen)
    mu_e, lv_e = oracle_encode(sd, h, zc)
    eng = _engine(sd)
    mu, lv, z = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), 1, eps=eps.cuda())
    errs = (_err(mu, mu_e), _err(lv, lv_e), _err(z, mu_e + eps * torch.exp(0.5 * lv_e)))
    print(f"ppc: {errs}")
    assert mu.shape == (n, 16) and max(errs) < 2e-5, errs


def test_encode_six_column_rows(fpc_state_dict):
    """An encoder without the label column (in_features = 6)."""
    sd = dict(fpc_state_dict)
    sd[ENC + "in_layer.weight"] = sd[ENC + "in_layer.weight"][:, :6].contiguous()
    gen = torch.Generator().manual_seed(6)
    h = torch.randn(12, 6, generator=gen)
    zc = torch.randn(3, 3, 64, generator=gen)
    mu_e, lv_e = oracle_encode(sd, h, zc.repeat_interleave(4, dim=0))
    eng = _engine(sd)
    assert eng.desc.latent_dim == 6
    mu, lv, _ = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), 4, want_z=False)
    assert max(_err(mu, mu_e), _err(lv, lv_e)) < 2e-5
    with pytest.raises(RuntimeError):
        eng.encode(torch.zeros(12, 7).cuda(), eng.cond_embed(zc.cuda()), 4)


# ------------------------------------------------------------------------------------------------ 9. range

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("scale", [50.0, 1e-3])
def test_encode_input_range(scale, f32, fpc_state_dict):
    """h scaled by 50 (a grasp 2.5 m from the cloud centre at the translation scale 0.05: the largest input a caller
    plausibly hands in) and by 1e-3, against the f64 composition: 2e-5 relative to max(1, largest |output|)."""
    sd = fpc_state_dict
    gen = torch.Generator().manual_seed(9)
    h = torch.randn(24, 7, generator=gen) * scale
    zc = torch.randn(6, 3, 64, generator=gen)
    mu_e, lv_e = oracle_encode(_dbl(sd), h.double(), zc.double().repeat_interleave(4, dim=0))
    with _mode(f32):
        eng = _engine(sd)
        mu, lv, _ = eng.encode(h.cuda(), eng.cond_embed(zc.cuda()), 4, want_z=False)
    bar = 2e-5 * max(1.0, mu_e.abs().max().item(), lv_e.abs().max().item())
    errs = (_err(mu, mu_e), _err(lv, lv_e))
    print(f"scale {scale} f32_only={f32}: errors {errs}, bar {bar:.2e}, largest output "
          f"{max(mu_e.abs().max().item(), lv_e.abs().max().item()):.3g}")
    assert torch.isfinite(mu).all() and torch.isfinite(lv).all()
    assert max(errs) < bar, (errs, bar)


# ------------------------------------------------------------------------------------------------ 10. determinism

def test_encode_is_repeatable_and_split_invariant(fpc_state_dict):
    gen = torch.Generator().manual_seed(10)
    h = torch.randn(40, 7, generator=gen)
    zc = torch.randn(10, 3, 64, generator=gen)
    eps = torch.randn(40, 4, generator=gen)
    eng = _engine(fpc_state_dict)
    cemb = eng.cond_embed(zc.cuda())
    a = eng.encode(h.cuda(), cemb, 4, eps=eps.cuda())
    b = eng.encode(h.cuda(), cemb, 4, eps=eps.cuda())
    c = eng.encode(h[:16].cuda(), cemb[:4].contiguous(), 4, eps=eps[:16].cuda())
    for x, y, w in zip(a, b, c):
        assert torch.equal(x, y)
        assert torch.equal(x[:16], w)


# ------------------------------------------------------------------------------------------------ 11 / 12. refinement

def _refine_inputs(seed=21, clouds=2, grasps=20):
    from graspldm_amd.synthetic import synthetic_batch
    pcs, _ = synthetic_batch(clouds, 1024)
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(clouds * grasps, 7, generator=gen)
    h[:, 6] = 1.0
    noise = torch.randn(clouds * grasps, 4, generator=gen)
    return pcs, h, noise, gen


def _oracle_refine(sd, z_pc, h, noise, sched, k, ts, step_noise=None):
    """The loop restated from oracle.torch_ref / oracle.schedulers: add_noise(mu, noise, ts[k]), resnet1d_forward +
    sched.step over ts[k:], decoder_forward.  dtype follows sd / the inputs."""
    from oracle import torch_ref as R
    g = h.shape[0] // z_pc.shape[0]
    zc = z_pc.repeat_interleave(g, dim=0)
    mu, logvar = oracle_encode(sd, h, zc)
    if k >= len(ts):
        x, x_k = mu, None
    else:
        x_k = sched.add_noise(mu, noise, ts[k])
        x = x_k.unsqueeze(1)
        for i, t in enumerate(ts[k:]):
            tb = torch.full((x.shape[0],), t, dtype=torch.long)
            eps = R.resnet1d_forward(sd, DEN, x, z_cond=zc, time=tb)
            if step_noise is not None:
                x = sched.step(eps, t, x, noise=step_noise[i] if t > 0 else None).prev_sample
            else:
                x = sched.step(eps, t, x).prev_sample
        x = x.squeeze(1)
    tmrp, logit = R.decoder_forward(sd, DEC, x, zc)
    return dict(mu=mu, logvar=logvar, x_k=x_k, x0=x, tmrp=tmrp, logit=logit)


def _oracle_pair(sd, pcs, spec, h, noise, kind, S, k, step_noise=None, variance_type="fixed_large"):
    """The restated loop in f32 and in f64 on the same inputs, and the worst distance between the two."""
    from graspldm_amd.diffusion import inference_timesteps
    from oracle import torch_ref as R
    z_pc = R.pvcnn_encoder_forward(sd, PC, pcs, spec)
    ts = inference_timesteps(1000, S)
    out = []
    for dbl in (False, True):
        sched = R.make_scheduler(kind, variance_type=variance_type)
        sched.set_timesteps(S)
        # (the scheduler keeps its f32 coefficient tables in both runs: they are the schedule's definition, evaluated like
        # the scheduler library does; the network and the update arithmetic on the state run in f32 / f64)
        c = (lambda t: t.double()) if dbl else (lambda t: t)
        out.append(_oracle_refine(_dbl(sd) if dbl else sd, c(z_pc), c(h), c(noise), sched, k, ts,
                                  None if step_noise is None else c(step_noise)))
    gap = {key: _err(out[0][key], out[1][key]) for key in ("mu", "logvar", "x0", "tmrp") if out[0][key] is not None}
    return out[0], gap, ts


@pytest.mark.parametrize("strength", [0.0, 0.3])
def test_refine_ddim_against_restated_loop(strength, fpc_state_dict, fpc_spec):
    """DDIM, S = 100, 2 clouds x 20 grasps: latents and tmrp within 1e-4 of the loop restated from the oracle.
    Precondition, asserted before the GPU result is looked at: the same loop in f32 and in f64 agrees within 2e-5 on
    this seed, so the reference's own rounding uses at most a fifth of the bar."""
    from graspldm_amd.pipeline import build_fpc_ldm
    pcs, h, noise, _ = _refine_inputs()
    S = 100
    k = S - int(round(S * strength))
    ref, gap, ts = _oracle_pair(fpc_state_dict, pcs, fpc_spec, h, noise, "ddim", S, k)
    print(f"strength {strength}: f32 vs f64 oracle {gap}")
    assert max(gap.values()) < 2e-5, gap
    ldm = build_fpc_ldm(device="cuda:0")
    ldm.set_inference_timesteps(S)
    (tmrp, logit), lat = ldm._refine(pcs.cuda(), h.cuda(), strength, noise=noise)
    ldm.check_engines()
    errs = dict(mu=_err(lat["mu"], ref["mu"]), logvar=_err(lat["logvar"], ref["logvar"]), x0=_err(lat["x0"], ref["x0"]),
                tmrp=_err(tmrp, ref["tmrp"]), logit=_err(logit, ref["logit"]))
    print(f"strength {strength}: GPU vs f32 oracle {errs}")
    assert lat["start_step"] == k
    assert errs["mu"] < 2e-5 and errs["logvar"] < 2e-5
    assert errs["x0"] < 1e-4 and errs["tmrp"] < 1e-4 and errs["logit"] < 1e-4, errs
    (tm2, lg2), empty = ldm.refine_grasps(pcs.cuda(), h.cuda(), strength, noise=noise)
    assert empty == [] and torch.equal(tm2, tmrp) and torch.equal(lg2, logit)
    m, lv = ldm.encode_grasps(pcs.cuda(), h.cuda())
    assert torch.equal(m, lat["mu"]) and torch.equal(lv, lat["logvar"])


def test_refine_full_strength_first_step_and_finiteness(fpc_state_dict, fpc_spec):
    """strength = 1.0 is not compared at a fixed bar (the f32 and f64 oracles themselves end 100 clipped steps 3.9e-3
    apart in the latents): finite results, and the launch's input x_k = add_noise(mu, noise, ts[0]) within 2e-6."""
    from graspldm_amd.pipeline import build_fpc_ldm
    from oracle import torch_ref as R
    pcs, h, noise, _ = _refine_inputs()
    ldm = build_fpc_ldm(device="cuda:0")
    ldm.set_inference_timesteps(100)
    (tmrp, logit), lat = ldm._refine(pcs.cuda(), h.cuda(), 1.0, noise=noise)
    ldm.check_engines()
    assert lat["start_step"] == 0 and torch.isfinite(tmrp).all() and torch.isfinite(logit).all()
    a, s = ldm.diffusion_model.add_noise_scalars(0)
    mu, _, x_k, _, _ = ldm.vae_model._encode(pcs.cuda(), h.cuda(), eps=noise.cuda(), mix=(a, s), eps_times_std=False)
    sched = R.make_scheduler("ddim")
    sched.set_timesteps(100)
    e = _err(x_k, sched.add_noise(mu.cpu(), noise, 990))
    print(f"x_k at ts[0]: {e:.2e}")
    assert e < 2e-6, e
    with pytest.raises(ValueError):
        ldm.refine_grasps(pcs.cuda(), h.cuda(), 1.01)


def test_refine_ddpm_tensor_and_kernel_noise(fpc_state_dict, fpc_spec):
    """DDPM (fixed_large), S = 1000, strength 0.1: the last 100 steps with `noise` and `step_noise` given, 1e-4 against
    the restated loop under the f32-vs-f64 precondition.  noise_source="kernel": the in-kernel stream is keyed on the
    step's INDEX WITHIN THE LAUNCHED SLICE (the launch that starts at ts[k] draws its first step with step number 0, not
    k): finite, check_engines() clean, and within 1e-6 of the tensor path fed with step_noise_rng(seed, base, i) rows,
    i = 0 .. S - k - 1."""
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.r1d import step_noise_rng
    pcs, h, noise, gen = _refine_inputs()
    S, k = 1000, 900
    step_noise = torch.randn(S - k, 40, 1, 4, generator=gen)
    ref, gap, ts = _oracle_pair(fpc_state_dict, pcs, fpc_spec, h, noise, "ddpm", S, k, step_noise=step_noise)
    print(f"ddpm: f32 vs f64 oracle {gap}")
    assert max(gap.values()) < 2e-5, gap
    ldm = build_fpc_ldm(scheduler="ddpm", device="cuda:0")
    (tmrp, logit), lat = ldm._refine(pcs.cuda(), h.cuda(), 0.1, noise=noise, step_noise=step_noise.cuda())
    ldm.check_engines()
    errs = dict(x0=_err(lat["x0"], ref["x0"]), tmrp=_err(tmrp, ref["tmrp"]), logit=_err(logit, ref["logit"]))
    print(f"ddpm: GPU vs f32 oracle {errs}")
    assert lat["start_step"] == k and max(errs.values()) < 1e-4, errs
    seed, base = 1234567, 3
    (tk, lk), latk = ldm._refine(pcs.cuda(), h.cuda(), 0.1, noise=noise, noise_source="kernel", noise_seed=seed,
                                 noise_base=base)
    ldm.check_engines()
    assert torch.isfinite(tk).all() and torch.isfinite(lk).all()
    rows = torch.stack([step_noise_rng(seed, base, i, 40, 4, "cuda:0") for i in range(S - k)]).view(S - k, 40, 1, 4)
    (tt, lt), latt = ldm._refine(pcs.cuda(), h.cuda(), 0.1, noise=noise, step_noise=rows)
    e = max(_err(latk["x0"], latt["x0"].cpu()), _err(tk, tt.cpu()))
    print(f"kernel noise vs tensor path with the same rows: {e:.2e}")
    assert e < 1e-6, e


def test_refine_rejects_elucidated():
    from graspldm_amd.grasp_ldm import GraspLatentDDM
    ldm = GraspLatentDDM.__new__(GraspLatentDDM)
    torch.nn.Module.__init__(ldm)
    ldm.is_elucidated_diffusion = True
    with pytest.raises(NotImplementedError):
        ldm.refine_grasps(torch.zeros(1, 8, 3).cuda(), torch.zeros(1, 7).cuda(), 0.5)


# ------------------------------------------------------------------------------------------------ 13. harness

def test_inference_harness_reconstruct_and_refine(fpc_state_dict):
    """InferenceVAE.reconstruct_grasps / InferenceLDM.refine_grasps on synthetic clouds: generate grasps, hand them back
    as 4x4 poses, check keys, shapes, finiteness and that latent_mu is the path of the golden test (normalise -> encode)."""
    from graspldm_amd.inference import InferenceLDM, InferenceVAE
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    pcs, metas = synthetic_batch(2, 1024)
    ldm = build_fpc_ldm(device="cuda:0")
    inf = InferenceLDM(model=ldm, num_inference_steps=20, device="cuda:0")
    x_T = torch.randn(12, 1, 4, generator=torch.Generator().manual_seed(13))
    first = inf.generate_grasps(pcs, metas, num_grasps=6, x_T=x_T)
    H = first["grasps"]                                                  # [2,6,4,4], cloud frame, un-normalised
    h = inf.normalize_grasps(H, metas)
    assert h.shape == (12, 7) and torch.equal(h[:, 6], torch.ones(12, device="cuda:0"))
    assert _err(h[:, :6].view(2, 6, 6) * metas["grasp_std"].unsqueeze(1).cuda() + metas["grasp_mean"].unsqueeze(1).cuda(),
                first["grasp_tmrp"].cpu()) < 1e-4                        # the inverse of the epilogue's un-normalisation
    mu, logvar = ldm.encode_grasps(pcs.cuda(), h)
    vinf = InferenceVAE(model=ldm.vae_model, device="cuda:0")
    rec = vinf.reconstruct_grasps(pcs, metas, H)
    assert set(rec) >= {"grasps", "grasp_tmrp", "confidence", "pc", "latent_mu", "latent_logvar"}
    assert rec["grasps"].shape == (2, 6, 4, 4) and rec["latent_mu"].shape == (2, 6, 4) and torch.isfinite(rec["grasps"]).all()
    assert torch.equal(rec["latent_mu"].view(12, 4), mu) and torch.equal(rec["latent_logvar"].view(12, 4), logvar)
    noise = torch.randn(12, 4, generator=torch.Generator().manual_seed(14))
    ref = inf.refine_grasps(pcs, metas, H, strength=0.3, noise=noise)
    assert set(ref) >= {"grasps", "grasp_tmrp", "confidence", "pc", "latent_mu", "latent_logvar", "all_steps_grasps"}
    assert ref["grasps"].shape == (2, 6, 4, 4) and torch.isfinite(ref["grasps"]).all()
    assert ((ref["confidence"] > 0) & (ref["confidence"] < 1)).all()
    assert torch.equal(ref["latent_mu"].view(12, 4), mu)
    # strength 0 is the VAE reconstruction of the mean, exactly
    zero = inf.refine_grasps(pcs, metas, H, strength=0.0)
    assert torch.equal(zero["grasps"], rec["grasps"]) and torch.equal(zero["confidence"], rec["confidence"])
    # eps given: the reparameterised latent is decoded instead of the mean
    rec_eps = vinf.reconstruct_grasps(pcs, metas, H, eps=noise)
    assert not torch.equal(rec_eps["grasps"], rec["grasps"]) and torch.equal(rec_eps["latent_mu"], rec["latent_mu"])
