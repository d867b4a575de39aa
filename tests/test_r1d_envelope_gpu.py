"""GPU: every descriptor the fused ResNet1D engines accept (the accepted rows of tests/r1d_envelope_cases.py; what the
library answers for each is pinned without a device in tests/test_r1d_envelope_cpu.py) on the engine the library routes it
to, R1dEngine(pack_resnet1d(...)) called directly, against the f64 restatement fed the engine's own f32 time-embedding rows.

Denoiser rows: one forward with a shared timestep table, one with per-sample timesteps (the fast embedding path off) and a
6-step DDIM run over the last 6 of 100 steps with two samples per conditioning row.  Decoder rows: tmrp and logit with 1 and
3 samples per conditioning row (a tile straddles two clouds' table rows).  Encoder rows: mu, logvar and z with eps given,
eps_times_std both ways.  Every row at two batches: one whose last tile holds at most 16 live columns (Ctx::nta == 1) and
one whose last tile is wider.  The wrapper allocates the outputs itself, so there is no guard row behind them to look at.

Bars (the project's: tests/test_r1d_gpu.py, tests/test_envelope_gpu.py): 2e-5 x max(1, max |ref|) for one forward, 1e-4 for
the trajectory and for tmrp, logit, mu, logvar and z.  The f32 torch oracle stays within a quarter of them
(tests/test_r1d_envelope_cpu.py), so a failure is the kernel's.  `test_every_accepted_row_has_a_gpu_run` needs no device.

Worst measured error per kernel (MI355X; one forward | 6-step DDIM | head outputs), and the row it came from:
  r1d_kernel<64,4>    7.7e-07 (d4_rows1)          | 3.0e-07 (d4_rows1)   | --
  r1d_kernel<64,16>   6.7e-07 (d16_six_levels)    | 2.4e-07 (d16_rows1)  | 5.3e-07 (dec16_quad_only, tmrp)
  r1d_kernel<32,4>    9.6e-07 (d4_width4_behind)  | 2.3e-07 (d4_first16) | 2.3e-07 (dec4, tmrp)
  r1d_kernel<32,16>   4.2e-07 (d16_emb160)        | 3.1e-07 (d16_first4) | 4.2e-07 (dec16_emb128, logit)
  ss_table_kernel     (its rows feed the two 16-position engines)        | 5.3e-07 (dec16_quad_only, tmrp)
The first run of the table found d4_emb32 6.8e-2, d4_256_only 1.7e-1, d16_park_no_chain 5.7e-1 and dec16_park_no_chain
1.8e-1 off: three kernel bugs, fixed; d16_256_only was added beside them.
"""
import ctypes

import pytest
import torch

import r1d_envelope_cases as C

gpu = pytest.mark.gpu
BAR = 2e-5
DENOISERS = [n for n in C.ACCEPTED if C.BY_NAME[n].head is None]
DECODERS = [n for n in C.ACCEPTED if C.BY_NAME[n].head == "decoder"]
ENCODERS = [n for n in C.ACCEPTED if C.BY_NAME[n].head not in (None, "decoder")]
_ENG = {}


def _engine(name):
    """R1dEngine of the row, built once; the library's route is asserted first."""
    if name not in _ENG:
        from graspldm_amd import _lib as L
        from graspldm_amd.r1d import R1dEngine
        packed = C.pack(name)
        ptr = ctypes.cast(ctypes.pointer(packed["desc"]), ctypes.c_void_p)
        assert L.lib().gldm_r1d_tile_columns(ptr) == C.BY_NAME[name].expected.cols
        _ENG[name] = (R1dEngine(packed, "cuda:0"), packed)
    return _ENG[name]


def _check(got, ref, bar, what):
    got = got.cpu()
    err = float((got.double() - ref).abs().max())
    print(f"{what}: err {err:.3e} bar {bar:.3e} (max |ref| {float(ref.abs().max()):.3f})")
    assert torch.isfinite(got).all(), what
    assert err <= bar, (what, err, bar)


def _forward_bar(ref):
    return BAR * max(1.0, float(ref.abs().max()))


@gpu
@pytest.mark.parametrize("name", DENOISERS)
def test_denoiser_row(name):
    from graspldm_amd.r1d import SCHED_DDIM
    row = C.BY_NAME[name]
    eng, packed = _engine(name)
    kern = f"r1d_kernel<{row.expected.cols},{row.L}>"
    x, z, t = C.inputs(name)
    n_big = x.shape[0]
    t_shared = int(t[0])
    ref_shared = C.forward(name, x, z, torch.full((n_big,), t_shared), packed["temb"])
    ref_each = C.forward(name, x, z, t, packed["temb"])
    x2, z2, _ = C.inputs(name, spc=2)
    ref_ddim = C.ddim_run(name, x2, C.per_sample(z2, 2, n_big), packed["temb"])
    ts, coef = C.ddim_tables()
    for n in C.batches(row):
        what = f"{name} {kern} n={n}"
        cemb = eng.cond_embed(z[:n].cuda())
        out = eng.denoise(x[:n].cuda(), cemb, 1, timesteps=torch.tensor([t_shared], dtype=torch.int32).cuda())
        _check(out, ref_shared[:n], _forward_bar(ref_shared[:n]), what + " shared t")
        out = eng.denoise(x[:n].cuda(), cemb, 1, sample_t=t[:n].int().cuda())
        _check(out, ref_each[:n], _forward_bar(ref_each[:n]), what + " per-sample t")
        cemb2 = eng.cond_embed(z2[:(n + 1) // 2].cuda())
        out = eng.denoise(x2[:n].cuda(), cemb2, 2, timesteps=ts.cuda(), sched_kind=SCHED_DDIM, coef=coef.cuda())
        _check(out, ref_ddim[:n], 1e-4, what + " ddim6")
    assert eng.workspace_errors() == 0


@gpu
@pytest.mark.parametrize("name", DECODERS)
def test_decoder_row(name):
    row = C.BY_NAME[name]
    eng, _ = _engine(name)
    kern = f"r1d_kernel<{row.expected.cols},{row.L}>" + (" + ss_table_kernel" if row.expected.table else "")
    for spc in (1, 3):
        x, z, _t = C.inputs(name, spc=spc)
        ref_tm, ref_lg = C.forward(name, x, C.per_sample(z, spc, x.shape[0]))
        for n in C.batches(row):
            what = f"{name} {kern} n={n} spc={spc}"
            tm, lg = eng.decode(x[:n].cuda(), eng.cond_embed(z[:-(-n // spc)].cuda()), spc)
            assert tm.shape == (n, 6) and lg.shape == (n, 1)
            _check(tm, ref_tm[:n], 1e-4, what + " tmrp")
            _check(lg, ref_lg[:n], 1e-4, what + " logit")
    assert eng.workspace_errors() == 0


@gpu
@pytest.mark.parametrize("name", ENCODERS)
def test_encoder_row(name):
    row = C.BY_NAME[name]
    eng, _ = _engine(name)
    kern = f"r1d_kernel<{row.expected.cols},{row.L}>" + (" + ss_table_kernel" if row.expected.table else "")
    lz = row.head[1]
    for spc in (1, 3):
        x, z, _t = C.inputs(name, spc=spc)
        n_big = x.shape[0]
        eps = torch.randn(n_big, lz, generator=torch.Generator().manual_seed(91 + spc))
        ref_mu, ref_lv = C.forward(name, x, C.per_sample(z, spc, n_big))
        for n in C.batches(row):
            cemb = eng.cond_embed(z[:-(-n // spc)].cuda())
            for times_std in (True, False):
                what = f"{name} {kern} n={n} spc={spc} eps_times_std={times_std}"
                mu, lv, zz = eng.encode(x[:n].cuda(), cemb, spc, eps=eps[:n].cuda(), mix=(1.0, 0.5), eps_times_std=times_std)
                assert mu.shape == lv.shape == zz.shape == (n, lz)
                _check(mu, ref_mu[:n], 1e-4, what + " mu")
                _check(lv, ref_lv[:n], 1e-4, what + " logvar")
                ref_z = ref_mu[:n] + 0.5 * eps[:n].double() * (torch.exp(0.5 * ref_lv[:n]) if times_std else 1.0)
                _check(zz, ref_z, 1e-4, what + " z")
    assert eng.workspace_errors() == 0


def test_every_accepted_row_has_a_gpu_run():
    """No device needed.  Every row of the case table that the library accepts is a parameter of one of the three GPU tests
    above: a new accepted row without a GPU run fails here."""
    ran = set()
    for fn in (test_denoiser_row, test_decoder_row, test_encoder_row):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and any(m.name == "gpu" for m in fn.pytestmark)
        ran |= set(marks[0].args[1])
    missing = [r.name for r in C.ROWS if isinstance(r.expected, C.Accept) and r.name not in ran]
    assert not missing, missing
    assert len(ran) == len(DENOISERS) + len(DECODERS) + len(ENCODERS) == len(C.ACCEPTED)
