"""GPU: the fused Unet1D kernel (csrc/unet1d.hip) against the f64 restatement (tests/unet1d_ref.py) on the golden
configurations, under both arithmetics; range, repeatability, tile independence; DDIM / DDPM sampling in one launch.

Bars: one pass of a 1-D net 2e-5 x max(1, max |ref|) (the project's, tests/test_models_gpu.py); sampled latents 1e-4.
The f64 yardstick is fed the f32 time-embedding rows (both implementations take them from the same f32 host computation).
"""
import contextlib

import pytest
import torch

import unet1d_ref as U

pytestmark = pytest.mark.gpu

BAR = 2e-5
MODES = ["split", "f32"]
_NETS, _REFS = {}, {}


def _mode(mode):
    from graspldm_amd import numerics
    return numerics.f32_only() if mode == "f32" else contextlib.nullcontext()


def _net(name):
    if name not in _NETS:
        from graspldm_amd.resnets import Unet1D
        from graspldm_amd.synthetic import load_synthetic_weights
        c = U.CASES[name]
        _NETS[name] = load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"]).cuda()
    return _NETS[name]


def _sd64(name):
    return {k: v.detach().cpu().double() for k, v in _net(name).state_dict().items()}


def _ref(name, n=70, scale=1.0):
    """f64 restatement on case_inputs(name, n), computed once per (case, n, scale) and shared."""
    key = (name, n, scale)
    if key not in _REFS:
        c = U.CASES[name]
        x, z, t = U.case_inputs(name, n)
        sd32 = {k: v.detach().cpu() for k, v in _net(name).state_dict().items()}
        temb = U.unet_time_embedding(sd32, "", t).double() if t is not None else None
        _REFS[key] = U.unet1d_forward(_sd64(name), "", x.double() * scale, z.double() if z is not None else None, t,
                                      groups=c["args"]["resnet_block_groups"], temb=temb)
    return _REFS[key]


def _run(name, n, scale=1.0, rows=None):
    x, z, t = U.case_inputs(name, n)
    sel = slice(None) if rows is None else rows
    return _net(name)(x[sel].cuda() * scale, time=t[sel].cuda() if t is not None else None,
                      z_cond=z[sel].cuda() if z is not None else None).cpu()


def _check(out, ref, what):
    assert torch.isfinite(out).all(), what
    err, bar = float((out.double() - ref).abs().max()), BAR * max(1.0, float(ref.abs().max()))
    print(f"{what}: max err {err:.3e} (bar {bar:.1e}, max |ref| {float(ref.abs().max()):.3f})")
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_forward_parity(name, n, mode):
    with _mode(mode):
        out = _run(name, n)
    _check(out, _ref(name)[:n], f"case {name} n={n} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_samples_per_cond(mode):
    """Four samples share a conditioning row (the VAE's use: one cloud, many grasps)."""
    net = _net("A")
    x, z, _ = U.case_inputs("A", 70, samples_per_cond=4)
    zr = z.repeat_interleave(4, dim=0)[:70]
    ref = U.unet1d_forward(_sd64("A"), "", x.double(), zr.double(), None, groups=4)
    with _mode(mode):
        net._cond_rows_of(z)
        eng = net.engine(torch.device("cuda", torch.cuda.current_device()))
        out = eng.forward(x.cuda(), eng.cond_embed(z.cuda()), samples_per_cond=4).cpu()
    _check(out, ref, f"case A samples_per_cond=4 {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_range_input_times_1024(mode):
    """Case A with x * 1024: finite and within the same relative bar (the restatement alone: d = 6.7e-5 at max |y| = 307)."""
    with _mode(mode):
        out = _run("A", 70, scale=1024.0)
    _check(out, _ref("A", 70, 1024.0), f"case A x1024 {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_range_beyond_f16(mode):
    """Case A with x * 2**17: the stem's output, the residual stream and the skips reach ~4e5, beyond f16 (65504), so the
    split operands only survive through the per-block power-of-two scale.  Same relative bar: the f32 restatement alone
    is 1.8e-7 of max |y| from its f64 run at this scale, as at x * 1024 (2.2e-7), measured on the CPU."""
    with _mode(mode):
        out = _run("A", 70, scale=2.0 ** 17)
    _check(out, _ref("A", 70, 2.0 ** 17), f"case A x2^17 {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_repeatable_and_tile_independent(mode):
    with _mode(mode):
        a, b = _run("B", 70), _run("B", 70)
        assert torch.equal(a, b), "the same launch twice differs"
        for i in (0, 37, 69):   # first tile, a middle one, the ragged last one
            alone = _run("B", 70, rows=slice(i, i + 1))
            assert torch.equal(alone[0], a[i]), f"row {i} alone differs from row {i} of the batch"


def _stepped(kind, x_T, z, step_noise):
    """The restatement stepped with oracle.schedulers, gaussian_diffusion.py:232-277."""
    from oracle import torch_ref as R
    sd = {k: v.detach().cpu() for k, v in _net("B").state_dict().items()}
    sched = R.make_scheduler(kind)
    sched.set_timesteps(20)
    x = x_T.clone()
    for i, t in enumerate(reversed(range(0, 1000, 50))):
        eps = U.unet1d_forward(sd, "", x, z, torch.full((x.shape[0],), t, dtype=torch.long), groups=4)
        if kind == "ddpm":
            x = sched.step(eps, t, x, noise=step_noise[i] if t > 0 else None).prev_sample
        else:
            x = sched.step(eps, t, x).prev_sample
    return x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_sampling_one_launch(kind, mode):
    from graspldm_amd.diffusion import GaussianDiffusion1D
    g = torch.Generator().manual_seed(77)
    x_T, z = torch.randn(24, 1, 16, generator=g), torch.randn(24, 64, generator=g)
    noise = torch.randn(20, 24, 1, 16, generator=g)
    ddm = GaussianDiffusion1D(_net("B"), n_dims=16, noise_scheduler_type=kind, beta_start=5e-5, beta_end=1e-3,
                              variance_type="fixed_large")
    ddm.set_inference_timesteps(20)
    kw = dict(z_cond=z.cuda(), batch_size=24, x_T=x_T, step_noise=noise.cuda() if kind == "ddpm" else None)
    with _mode(mode):
        x, _ = ddm.sample(**kw)
        _, trace = ddm.sample(return_all=True, **kw)
        if mode == "split" and kind == "ddpm":
            with pytest.raises(NotImplementedError, match="noise_source='tensor'"):
                ddm.sample(z_cond=z.cuda(), batch_size=24, x_T=x_T, noise_source="kernel")
    assert len(trace) == 21 and torch.equal(trace[-1], x), "one launch differs from the last entry of return_all=True"
    ref = _stepped(kind, x_T, z, noise)
    err = float((x.cpu() - ref).abs().max())
    print(f"{kind} 20 steps {mode}: max err {err:.3e} (bar 1e-4, max |ref| {float(ref.abs().max()):.3f})")
    assert torch.isfinite(x).all() and err <= 1e-4, err


# ------------------------------------------------------------------------------------------ VAE with Unet1D cores
def _vae():
    if "vae" not in _NETS:
        from graspldm_amd.builder import build_model_from_cfg
        from graspldm_amd.pipeline import fpc_model_config
        from graspldm_amd.synthetic import load_synthetic_weights
        vae = build_model_from_cfg(fpc_model_config(vae_core="Unet1D")["vae"])
        _NETS["vae"] = load_synthetic_weights(vae, seed=0).eval().cuda()
    return _NETS["vae"]


@pytest.mark.parametrize("mode", MODES)
def test_vae_with_unet_cores_against_the_reference(mode):
    """GraspCVAE(vae_core="Unet1D") on the fixture's two clouds x 4 grasps: generate_grasps (given z_h), encode and
    forward(compute_loss=False) against the reference's recorded outputs, 1e-4."""
    from conftest import load_golden
    from graspldm_amd.synthetic import synthetic_batch
    g = load_golden("unet1d_vae.npz")
    pcs, _ = synthetic_batch(2, 1024)
    pcs = pcs.cuda()
    with _mode(mode):
        vae = _vae()
        tm, lg = vae.generate_grasps(pcs, 4, z_h=g["z_h"])
        (mu, logvar, z), (_, _, z_pc) = vae.encode(pcs, g["h"].cuda(), eps=g["eps"])
        rt, rl = vae(pcs, g["h"].cuda(), compute_loss=False, eps=g["eps"])
    assert z_pc.shape[0] == 8
    errs = dict(gen_tmrp=tm, gen_logit=lg, mu=mu, logvar=logvar, z=z, tmrp=rt, logit=rl)
    errs = {k: float((v.cpu() - g[k]).abs().max()) for k, v in errs.items()}
    print(f"VAE with Unet1D cores {mode}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) <= 1e-4, errs


def test_inference_vae_reconstructs_with_unet_cores():
    from graspldm_amd.inference import InferenceVAE
    from graspldm_amd.synthetic import synthetic_batch
    pcs, metas = synthetic_batch(2, 1024)
    vinf = InferenceVAE(model=_vae(), device="cuda:0")
    first = vinf.generate_grasps(pcs, metas, num_grasps=4)
    rec = vinf.reconstruct_grasps(pcs, metas, first["grasps"])
    assert set(rec) >= {"grasps", "grasp_tmrp", "confidence", "pc", "latent_mu", "latent_logvar"}
    assert rec["grasps"].shape == (2, 4, 4, 4) and torch.isfinite(rec["grasps"]).all() and torch.isfinite(rec["confidence"]).all()
