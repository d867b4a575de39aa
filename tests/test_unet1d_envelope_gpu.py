"""GPU: the fused Unet1D kernel (csrc/unet1d.hip) over the shape envelope its query accepts (ENVELOPE of
tests/unet1d_ref.py), against the f64 restatement under both arithmetics: every row at its own tile size, rows N and O at
forced tile sizes through the C entry, three sampling variants no other test sets, and a quiet sample beside a loud one.

Bars: one pass 2e-5 x max(1, max |ref|), sampled latents 1e-4 (the project's, tests/test_unet1d_gpu.py).  The f64 yardstick
is fed the f32 time-embedding rows.  Batches are at most 2 S + 1 samples of a tile of S: two whole tiles and a ragged one.
"""
import contextlib
import ctypes

import pytest
import torch

import unet1d_ref as U

pytestmark = pytest.mark.gpu

BAR = 2e-5
MODES = ["split", "f32"]
_NETS, _REFS, _SD = {}, {}, {}


def _mode(mode):
    from graspldm_amd import numerics
    return numerics.f32_only() if mode == "f32" else contextlib.nullcontext()


def _net(name):
    if name not in _NETS:
        from graspldm_amd.resnets import Unet1D
        from graspldm_amd.synthetic import load_synthetic_weights
        c = U.config(name)
        _NETS[name] = load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"]).cuda()
    return _NETS[name]


def _sd(name, dtype=torch.float32):
    if (name, dtype) not in _SD:
        _SD[name, dtype] = {k: v.detach().cpu().to(dtype) for k, v in _net(name).state_dict().items()}
    return _SD[name, dtype]


def _reference(name, x, z, t):
    """The f64 restatement of configuration `name` on (x, z, t), z already one block per sample."""
    temb = U.unet_time_embedding(_sd(name), "", t).double() if t is not None else None
    return U.unet1d_forward(_sd(name, torch.float64), "", x.double(), z.double() if z is not None else None, t,
                            groups=U.config(name)["args"]["resnet_block_groups"], temb=temb)


def _ref(name, n, samples_per_cond=1):
    """f64 restatement on case_inputs(name, n, samples_per_cond), computed once and shared."""
    key = (name, n, samples_per_cond)
    if key not in _REFS:
        x, z, t = U.case_inputs(name, n, samples_per_cond)
        if z is not None and samples_per_cond > 1:
            z = z.repeat_interleave(samples_per_cond, dim=0)[:n]
        _REFS[key] = _reference(name, x, z, t)
    return _REFS[key]


def _forward(name, x, z, t):
    return _net(name)(x.cuda(), time=t.cuda() if t is not None else None, z_cond=z.cuda() if z is not None else None).cpu()


def _tile(name):
    """The tile size the packer chose for `name` (the LDS map does not depend on the arithmetic)."""
    net, c = _net(name), U.config(name)
    net._cond_rows_of(U.case_inputs(name, 1)[1])
    return net.engine(torch.device("cuda", torch.cuda.current_device())).plan(c["L"])["desc"].tile_samples


def _check(out, ref, what):
    assert torch.isfinite(out).all(), what
    err, bar = float((out.double() - ref).abs().max()), BAR * max(1.0, float(ref.abs().max()))
    print(f"{what}: max err {err:.3e} (bar {bar:.1e}, max |ref| {float(ref.abs().max()):.3f})")
    assert err <= bar, (what, err, bar)


# ------------------------------------------------------------------------------------------------- every row, its tile
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(U.ENVELOPE))
def test_forward_parity(name, mode):
    """2 S + 1 samples (two whole tiles and a one-sample tile) and one sample alone against f64; the sample alone has the
    bits it has as row 0 of the batch."""
    with _mode(mode):
        s = _tile(name)
        n = 2 * s + 1
        x, z, t = U.case_inputs(name, n)
        out = _forward(name, x, z, t)
        one = _forward(name, x[:1], z[:1] if z is not None else None, t[:1] if t is not None else None)
    ref = _ref(name, n)
    _check(out, ref, f"row {name} tile {s} n={n} {mode}")
    _check(one, ref[:1], f"row {name} tile {s} n=1 {mode}")
    assert torch.equal(one[0], out[0]), "row 0 alone differs from row 0 of the batch"


# --------------------------------------------------------------------------------------------------- forced tile sizes
# S in {1, 2, 3, 5, 7, 11, 16} where check_program admits the layout (tests/test_unet1d_cpu.py pins these lists: row N at
# 16 samples of 10 positions exceeds the 160 KiB of LDS)
FORCED = {"N": (1, 2, 3, 5, 7, 11), "O": (1, 2, 3, 5, 7, 11, 16)}
SPC = {"N": 1, "O": 3}
N_MAX = 2 * 16 + 1
_PLANS, _FORCED_OUT = {}, {}


def _launch(name, tile_samples, n, mode):
    """pack_unet1d(tile_samples=S) and gldm_unet1d called as UnetEngine.denoise calls it (one forward, no schedule), on the
    first n samples of case_inputs(name, N_MAX, SPC[name]).  None: the packer's own tile size."""
    from graspldm_amd import _lib as L
    from graspldm_amd.r1d_pack import SCHED_NONE
    from graspldm_amd.unet1d_pack import pack_unet1d
    c, spc = U.config(name), SPC[name]
    x, z, t = U.case_inputs(name, N_MAX, spc)
    assert t is None, "rows without time: the helper passes no time-embedding table"
    rows = 0 if z is None else (1 if z.ndim == 2 else z.shape[1])
    key = (name, tile_samples, mode)
    if key not in _PLANS:
        pk = pack_unet1d(_sd(name), "", c["args"]["resnet_block_groups"], c["L"], cond_rows=rows, tile_samples=tile_samples)
        _PLANS[key] = (pk["desc"], pk["weights"].cuda())
    desc, weights = _PLANS[key]
    assert tile_samples is None or desc.tile_samples == tile_samples
    cemb = None
    if z is not None:
        net = _net(name)
        net._cond_rows_of(z)
        cemb = net.engine(torch.device("cuda", torch.cuda.current_device())).cond_embed(z.cuda()).contiguous()
        assert cemb.shape[0] * spc >= n
    x_in = x[:n].cuda().contiguous()
    out = torch.empty_like(x_in)
    L.call("gldm_unet1d", ctypes.cast(ctypes.pointer(desc), ctypes.c_void_p), L.ptr(weights), None, L.ptr(cemb), spc,
           L.ptr(x_in), n, c["L"], None, None, 1, int(SCHED_NONE), 1, None, None, L.ptr(out), L.current_stream())
    return out.cpu()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name, s", [(name, s) for name in sorted(FORCED) for s in FORCED[name]])
def test_forced_tile_size(name, s, mode):
    """A column's arithmetic does not depend on where it sits in a tile (K order is fixed, wave_sum is a fixed tree over a
    sample's group, both attentions run per column): any tile size gives the bits of the packer's own."""
    n = 2 * s + 1
    with _mode(mode):
        if (name, mode) not in _FORCED_OUT:
            _FORCED_OUT[name, mode] = _launch(name, None, N_MAX, mode)
        out = _launch(name, s, n, mode)
    _check(out, _ref(name, N_MAX, SPC[name])[:n], f"row {name} forced tile {s} n={n} {mode}")
    assert torch.equal(out, _FORCED_OUT[name, mode][:n]), f"tile size {s} differs from the packer's own in some bit"


# ---------------------------------------------------------------------------------------------------- sampling variants
VARIANTS = {"ddim_unclipped": ("ddim", False, "fixed_large"), "ddpm_small_clipped": ("ddpm", True, "fixed_small"),
            "ddpm_large_unclipped": ("ddpm", False, "fixed_large")}
_SAMPLING = {}


def _sampling_inputs():
    g = torch.Generator().manual_seed(78)
    n = 11   # 2 S + 1 of row G's tile of 5; three samples share a conditioning row
    x_T, z = torch.randn(n, 1, 12, generator=g), torch.randn(4, 64, generator=g)
    return x_T, z, torch.randn(20, n, 1, 12, generator=g)


def _stepped(kind, clip, variance_type):
    """Row G's restatement stepped with oracle.schedulers (gaussian_diffusion.py:232-277), once per variant."""
    key = (kind, clip, variance_type if kind == "ddpm" else None)
    if key not in _SAMPLING:
        from oracle import schedulers
        kw = dict(num_train_timesteps=1000, beta_start=5e-5, beta_end=1e-3, beta_schedule="linear", clip_sample=clip)
        sched = schedulers.DDIMScheduler(**kw) if kind == "ddim" else schedulers.DDPMScheduler(variance_type=variance_type, **kw)
        sched.set_timesteps(20)
        x_T, z, noise = _sampling_inputs()
        x, zr = x_T.clone(), z.repeat_interleave(3, dim=0)[:x_T.shape[0]]
        for i, t in enumerate(reversed(range(0, 1000, 50))):
            eps = U.unet1d_forward(_sd("G"), "", x, zr, torch.full((x.shape[0],), t, dtype=torch.long), groups=4)
            x = sched.step(eps, t, x, noise=noise[i] if t > 0 else None).prev_sample if kind == "ddpm" else \
                sched.step(eps, t, x).prev_sample
        _SAMPLING[key] = x
    return _SAMPLING[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_sampling_variants(variant, mode):
    """clip_sample=False (the clip == 0 branch of scheduler_update) and the fixed_small variance table, 20 steps in one
    launch, three samples per conditioning row."""
    from graspldm_amd.diffusion import GaussianDiffusion1D
    kind, clip, variance_type = VARIANTS[variant]
    ref = _stepped(kind, clip, variance_type)
    apart = float((ref - _stepped(kind, not clip, variance_type)).abs().max())
    assert apart > 1e-2, f"clipping changes the reference by {apart:.1e} only: the variant would test nothing"
    if kind == "ddpm":
        other = "fixed_large" if variance_type == "fixed_small" else "fixed_small"
        assert float((ref - _stepped(kind, clip, other)).abs().max()) > 1e-2
    x_T, z, noise = _sampling_inputs()
    ddm = GaussianDiffusion1D(_net("G"), n_dims=12, noise_scheduler_type=kind, beta_start=5e-5, beta_end=1e-3,
                              variance_type=variance_type, clip_sample=clip)
    ddm.set_inference_timesteps(20)
    with _mode(mode):
        x, _ = ddm.sample(z_cond=z.cuda(), batch_size=x_T.shape[0], x_T=x_T, samples_per_cond=3,
                          step_noise=noise.cuda() if kind == "ddpm" else None)
    err = float((x.cpu() - ref).abs().max())
    print(f"row G {variant} 20 steps {mode}: max err {err:.3e} (bar 1e-4, max |ref| {float(ref.abs().max()):.3f}, "
          f"clipped and unclipped references {apart:.2e} apart)")
    assert torch.isfinite(x).all() and err <= 1e-4, err


# -------------------------------------------------------------------------------------------------- a loud neighbour
LOUD = 3e7   # the largest magnitude tests/test_range_gpu.py uses


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["C", "O"])
def test_a_loud_neighbour_does_not_cost_a_quiet_sample_its_accuracy(name, mode):
    """One tile of S samples of 4 positions (a 16-column block of a conv holds four samples), sample 1 times 3e7: every
    sample within the bar of ITS OWN reference, the loud one included.  The split convs therefore take their range scale
    per column: a scale shared by a block's 16 columns splits the quiet samples as x / s with the loud one's s, and their
    planes fall into f16's subnormals (measured with one scale per wave: quiet samples up to 4.7e-5 off in case C and 5.9e-5
    in row O, against 3.6e-7 and 2.1e-7 with one per column).  The quiet samples also keep the bits they have in a batch
    without the loud one."""
    with _mode(mode):
        s = _tile(name)
        x, z, t = U.case_inputs(name, s)
        x = x.clone()
        x[1] *= LOUD
        out = _forward(name, x, z, t)
        quiet = _forward(name, *U.case_inputs(name, s))
    ref = _reference(name, x, z, t)
    worst = []
    for i in range(s):
        err, bar = float((out[i].double() - ref[i]).abs().max()), BAR * max(1.0, float(ref[i].abs().max()))
        print(f"{name} {mode} sample {i}{' (loud)' if i == 1 else ''}: max err {err:.3e} (bar {bar:.1e}, "
              f"max |ref| {float(ref[i].abs().max()):.3e})")
        if not err <= bar:
            worst.append((i, err, bar))
    assert torch.isfinite(out).all() and not worst, worst
    keep = [i for i in range(s) if i != 1]
    assert torch.equal(out[keep], quiet[keep]), "a quiet sample's bits depend on its neighbour"
