"""GPU (MI355X): every entry of the voxel tail (csrc/voxel_norm.hip: the SE squeeze, the SE gate, the three fused
devoxelize entries) through the C ABI, each against the f64 restatement of tests/voxel_tail_ref.py -- never against
another kernel.  tests/test_voxel_tail_cpu.py pins that restatement to the oracle.

Inputs are made directly: a random raw grid y and random coefficients (a, s) stand in for a conv output and its GroupNorm.
Three clouds per case, each with its own coefficients, gate and coordinates, so that a wrong batch stride shows.  Every
entry is launched twice per case and must return the same bits.

Bars (the project's parity bars, none of them taken from the kernels; each test prints what it measured):
  devoxelize  |got - ref| <= 2e-5 max(1, M), M = the largest |activated grid value| of that (cloud, channel)
  squeeze     2e-5 max(1, M) on the MEAN, sum / r^3
  gate        2e-5 absolute (the output lies in (0, 1))"""
import functools
import math

import pytest
import torch

import voxel_tail_ref as T

pytestmark = pytest.mark.gpu

B = 3
BAR = 2e-5
PARTS = 8          # partial sums handed to gldm_se_gate_parts by these tests (any count is legal there)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _check(what, got, ref, bar):
    """got (CUDA f32) against ref (CPU f64) under bar (a float or a tensor that broadcasts); prints the worst error."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(err)
    worst = (err / bar).max().item()
    print(f"{what}: worst |err| {err.max().item():.2e}, {worst:.3f} of its bar")
    assert worst <= 1.0, (what, err.max().item(), worst)


def _twice(launch, shape):
    """Two launches into two buffers (poisoned first): the same bits."""
    outs = [torch.full(shape, float("nan"), device="cuda") for _ in range(2)]
    for o in outs:
        launch(o)
    assert torch.equal(outs[0], outs[1]), "a repeated launch changed the result"
    return outs[0]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _grid(r, c, seed, wide=False):
    """y [B, c, r, r, r] ~ N(0, 1) and coef [B, c, 2].  Plain: |a| in [0.5, 1.5] with both signs, s ~ 0.5 N(0, 1).
    wide: a = +-200 / max|y| of the (cloud, channel), so that a y + s spans about [-200, 200] and 2^(-t log2 e) leaves the
    f32 range on both sides."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, c, r, r, r, generator=g)
    sign = torch.where(torch.rand(B, c, generator=g) < 0.5, -1.0, 1.0)
    if wide:
        a = sign * 200.0 / y.flatten(2).abs().amax(-1)
        s = torch.randn(B, c, generator=g)
    else:
        a = sign * (0.5 + torch.rand(B, c, generator=g))
        s = 0.5 * torch.randn(B, c, generator=g)
    return y, torch.stack([a, s], dim=-1).contiguous()


def _channel_last(y):
    b, c = y.shape[:2]
    return y.reshape(b, c, -1).permute(0, 2, 1).contiguous()


def _special_points(r):
    """Points ON the grid and next to it, all inside [0, r - 1] (r >= 5).  The fractions 2^-20 and 1 - 2^-20 sit at
    lo = 1 and lo = 0, where f32 holds them exactly."""
    e, t = 2.0 ** -20, float(r - 1)
    return [(2.0, 1.0, 3.0),                       # all three axes on a voxel
            (2.0, 0.37, 2.81), (1.62, 3.0, 0.25), (3.4, 1.7, 1.0),          # exactly one axis
            (0.0, 0.0, 0.0), (t, t, t),
            (t, 1.37, 0.0), (2.62, t, t),          # the last voxel beside a fractional part
            (1.0 + e, 0.5, 2.25), (1.0 - e, 2.75, 0.5), (e, 1.0 - e, 1.0 + e)]


def _coords(r, n, seed):
    """[B, 3, total], total = n x launches: random points of [0, r - 1) and, in EVERY cloud, every special point, at
    places that differ from cloud to cloud (cloud 0 has one in the last slot).  One launch takes n points, so a case with
    fewer points than there are special ones is several launches of n."""
    sp = torch.tensor(_special_points(r), dtype=torch.float32)
    s = sp.shape[0]
    total = n * math.ceil((s + 1) / n)
    g = torch.Generator().manual_seed(seed)
    coords = torch.rand(B, 3, total, generator=g) * (r - 1)
    for k in range(B):
        at = [total - 1 - ((j * total // s + 5 * k) % total) for j in range(s)]
        assert len(set(at)) == s
        coords[k][:, at] = sp.T
    # nothing out of range reaches a kernel: those index outside the grid
    assert torch.isfinite(coords).all() and coords.min().item() >= 0.0 and coords.max().item() <= r - 1
    return coords


@functools.lru_cache(maxsize=None)
def _devox_case(r, c, n, with_gate, with_add, wide=False):
    """Inputs and f64 references of one devoxelize case, made once and shared by the three entries (read-only)."""
    seed = 1000 * r + 10 * c + n + (7 if wide else 0)
    y, coef = _grid(r, c, seed, wide)
    coords = _coords(r, n, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    gate = 0.25 + torch.rand(B, c, generator=g) if with_gate else None
    add = torch.randn(B, c, coords.shape[2], generator=g) if with_add else None
    act = T.swish_affine(y, coef)
    act32 = act.float()                                                    # what gldm_devoxelize_fused is given
    return dict(r=r, c=c, n=n, y=y, coef=coef, coords=coords, gate=gate, add=add, act32=act32,
                ref_raw=T.devoxelize(coords, act, gate, add, r), bar_raw=BAR * act.flatten(2).abs().amax(-1, keepdim=True).clamp(min=1.0),
                ref_act=T.devoxelize(coords, act32, gate, add, r),
                bar_act=BAR * act32.double().flatten(2).abs().amax(-1, keepdim=True).clamp(min=1.0))


def _run_devoxelize(entry, case):
    """One entry over the case's launches of n points; [B, c, total] on the GPU."""
    from graspldm_amd import _lib as L
    r, c, n = case["r"], case["c"], case["n"]
    st = L.current_stream()
    coef = case["coef"].cuda()
    gate = None if case["gate"] is None else case["gate"].cuda()
    if entry == "gldm_devoxelize_fused":
        feat = case["act32"].cuda()
    elif entry == "gldm_devoxelize_gn_fused":
        feat = case["y"].cuda()
    else:
        assert c % 4 == 0
        feat = _channel_last(case["y"]).cuda()
    outs = []
    for p0 in range(0, case["coords"].shape[2], n):
        co = case["coords"][:, :, p0:p0 + n].contiguous().cuda()
        add = None if case["add"] is None else case["add"][:, :, p0:p0 + n].contiguous().cuda()
        if entry == "gldm_devoxelize_fused":
            launch = lambda o: L.call(entry, L.ptr(co), L.ptr(feat), L.ptr(gate), L.ptr(add), B, c, n, r, L.ptr(o), st)   # noqa: E731
        else:
            launch = lambda o: L.call(entry, L.ptr(co), L.ptr(feat), L.ptr(coef), L.ptr(gate), L.ptr(add), B, c, n, r, L.ptr(o), st)   # noqa: E731
        outs.append(_twice(launch, (B, c, n)))
    return torch.cat(outs, dim=2)


# r, c, n, gate, add.  n = 1; the 64-point blocks of the channel-last kernel and the 256-point blocks of the channel-major
# one, one point either side; c below, across and off the 16-channel blocks; 1, 3, 12, 24 and 64 channel quads; the last
# row is the channel-last kernel's 66,560 bytes of LDS, above the 64 KiB a kernel has without asking.
DEVOX = [(5, 7, 1, True, True),
         (5, 20, 65, False, True),
         (8, 4, 63, True, False),
         (8, 12, 64, False, False),
         (12, 96, 257, True, True),
         (24, 48, 300, True, True),
         (8, 256, 130, True, True)]
DEVOX_CL = [s for s in DEVOX if s[1] % 4 == 0]
WIDE = (8, 12, 70, True, True, True)      # the coefficients of _grid(wide=True): swish arguments out to +-200


@pytest.mark.parametrize("shape", DEVOX, ids=lambda s: "r{}-c{}-n{}".format(*s[:3]))
def test_devoxelize_fused(shape):
    """gldm_devoxelize_fused on the activated grid (f32) against ref.devoxelize of the same grid."""
    case = _devox_case(*shape)
    got = _run_devoxelize("gldm_devoxelize_fused", case)
    _check("gldm_devoxelize_fused r={} c={} n={}".format(*shape[:3]), got, case["ref_act"], case["bar_act"])


@pytest.mark.parametrize("shape", DEVOX + [WIDE], ids=lambda s: "r{}-c{}-n{}{}".format(*s[:3], "-wide" if len(s) > 5 else ""))
def test_devoxelize_gn_fused(shape):
    """gldm_devoxelize_gn_fused on the raw grid against ref.devoxelize of ref.swish_affine."""
    case = _devox_case(*shape)
    got = _run_devoxelize("gldm_devoxelize_gn_fused", case)
    _check("gldm_devoxelize_gn_fused r={} c={} n={}".format(*shape[:3]), got, case["ref_raw"], case["bar_raw"])


@pytest.mark.parametrize("shape", DEVOX_CL + [WIDE], ids=lambda s: "r{}-c{}-n{}{}".format(*s[:3], "-wide" if len(s) > 5 else ""))
def test_devoxelize_gn_cl_fused(shape):
    """gldm_devoxelize_gn_cl_fused on the raw grid, channel-last, against the same channel-major reference."""
    case = _devox_case(*shape)
    got = _run_devoxelize("gldm_devoxelize_gn_cl_fused", case)
    _check("gldm_devoxelize_gn_cl_fused r={} c={} n={}".format(*shape[:3]), got, case["ref_raw"], case["bar_raw"])


# ---------------------------------------------------------------------------------------------------------------------
# squeeze
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _squeeze_case(r, c, wide=False):
    y, coef = _grid(r, c, 77 * r + c + (3 if wide else 0), wide)
    act = T.swish_affine(y, coef)
    return y, coef, T.squeeze(y, coef) / r ** 3, BAR * act.flatten(2).abs().amax(-1).clamp(min=1.0)


@pytest.mark.parametrize("r,c,wide", [(3, 5, False), (5, 8, False), (8, 32, False), (24, 48, False), (8, 32, True)])
def test_squeeze_channel_major(r, c, wide):
    """gldm_gn_swish_chan_sum: 27 and 125 voxels (the scalar loop: rows that are not 16-byte runs, fewer voxels than
    threads), 512 and 13,824 (the 16-byte loop, half a trip and 13.5 trips of the 256 threads)."""
    from graspldm_amd import _lib as L
    y, coef, ref, bar = _squeeze_case(r, c, wide)
    dy, dc, st = y.cuda(), coef.cuda(), L.current_stream()
    got = _twice(lambda o: L.call("gldm_gn_swish_chan_sum", L.ptr(dy), L.ptr(dc), B, c, r, L.ptr(o), st), (B, c))
    _check(f"gldm_gn_swish_chan_sum r={r} c={c}{' wide' if wide else ''} (mean)", got / r ** 3, ref, bar)


@pytest.mark.parametrize("r,c,wide", [(3, 4, False), (5, 12, False), (8, 48, False), (8, 1024, False), (24, 48, False), (8, 48, True)])
def test_squeeze_channel_last(r, c, wide):
    """gldm_gn_swish_chan_sum_cl, its gldm_squeeze_parts() parts added: 1 quad (256 stripes), 3 quads (85 stripes and an
    idle thread), 12 quads (21 stripes, 4 idle threads), 256 quads (one stripe); 27 and 125 voxels do not divide by the
    parts."""
    from graspldm_amd import _lib as L
    y, coef, ref, bar = _squeeze_case(r, c, wide)
    parts = int(L.lib().gldm_squeeze_parts())
    dy, dc, st = _channel_last(y).cuda(), coef.cuda(), L.current_stream()
    got = _twice(lambda o: L.call("gldm_gn_swish_chan_sum_cl", L.ptr(dy), L.ptr(dc), B, c, r, L.ptr(o), st), (B, parts, c))
    _check(f"gldm_gn_swish_chan_sum_cl r={r} c={c}{' wide' if wide else ''} (mean)", got.double().sum(1) / r ** 3, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------
# gate
# ---------------------------------------------------------------------------------------------------------------------
def _gate_inputs(c, hidden, r):
    """Partial sums [B, PARTS, c] of unequal size (part p carries p + 1 shares of the voxels) whose mean over the r^3
    voxels is ~ N(0, 1), and weights that make pre-activations of about 2 in both layers: gates all over (0, 1).  f32
    dot products of c <= 1024 such terms in index order leave the hidden layer a few 1e-6 from f64 (c roundings of 2^-24
    of partial sums of a few units, adding as a random walk), the second layer passes that on times its weights and the
    sigmoid takes a quarter of it at most: the 2e-5 bar has room for the arithmetic and none for a wrong element."""
    g = torch.Generator().manual_seed(c * 31 + hidden + r)
    share = torch.arange(1, PARTS + 1, dtype=torch.float32)
    share = share / share.pow(2).sum().sqrt()
    parts = torch.randn(B, PARTS, c, generator=g) * share.view(1, PARTS, 1) * float(r ** 3)
    w1 = torch.randn(hidden, c, generator=g) * (2.0 / c ** 0.5)
    w2 = torch.randn(c, hidden, generator=g) * (2.0 / hidden ** 0.5)
    return parts, w1, w2


@pytest.mark.parametrize("r", [5, 24])
@pytest.mark.parametrize("use_relu", [0, 1])
@pytest.mark.parametrize("c,hidden", [(4, 1), (48, 6), (200, 25), (1024, 130)])
def test_se_gate(c, hidden, use_relu, r):
    """gldm_se_gate on sums and gldm_se_gate_parts on 8 partial sums, each against ref.se_gate of its own input: fewer
    channels than the 128 threads, more (two and eight trips), a hidden width above them, one hidden unit."""
    from graspldm_amd import _lib as L
    parts, w1, w2 = _gate_inputs(c, hidden, r)
    sums = parts.sum(1)                                   # f32: the input of gldm_se_gate, and of its reference
    dp, ds, d1, d2, st = parts.cuda(), sums.cuda(), w1.cuda(), w2.cuda(), L.current_stream()
    ref = T.se_gate(sums, w1, w2, r, use_relu)
    assert 0.05 < ref.std().item()                        # gates that differ
    got = _twice(lambda o: L.call("gldm_se_gate", L.ptr(ds), L.ptr(d1), L.ptr(d2), B, c, hidden, r, use_relu, L.ptr(o), st), (B, c))
    _check(f"gldm_se_gate c={c} hidden={hidden} relu={use_relu} r={r}", got, ref, BAR)
    got = _twice(lambda o: L.call("gldm_se_gate_parts", L.ptr(dp), PARTS, L.ptr(d1), L.ptr(d2), B, c, hidden, r, use_relu, L.ptr(o), st), (B, c))
    _check(f"gldm_se_gate_parts c={c} hidden={hidden} relu={use_relu} r={r}", got, T.se_gate(parts, w1, w2, r, use_relu), BAR)


# ---------------------------------------------------------------------------------------------------------------------
# the pieces together
# ---------------------------------------------------------------------------------------------------------------------
def test_squeeze_gate_devoxelize_chain():
    """Channel-last squeeze -> gate from its parts (ReLU) -> channel-last devoxelize at r = 12, c = 96 against the chained
    reference: the [B, parts, c] layout between the first two, sums against means, the gate's [B, c] into the third.
    The output is held to the devoxelize bar, the gate on the way to its own."""
    from graspldm_amd import _lib as L
    r, c, n, hidden = 12, 96, 100, 12
    y, coef = _grid(r, c, 4242)
    coords = _coords(r, n, 4243)
    g = torch.Generator().manual_seed(4244)
    add = torch.randn(B, c, n, generator=g)
    w1 = torch.randn(hidden, c, generator=g) * (8.0 / c ** 0.5)      # means of swish outputs are small: strong weights
    w2 = torch.randn(c, hidden, generator=g) * (2.0 / hidden ** 0.5)
    act = T.swish_affine(y, coef)
    ref_gate = T.se_gate(T.squeeze(y, coef), w1, w2, r, True)
    assert 0.05 < ref_gate.std().item()
    ref = T.devoxelize(coords, act, ref_gate, add, r)
    parts = int(L.lib().gldm_squeeze_parts())
    dy, dc, d1, d2, dco, da, st = (_channel_last(y).cuda(), coef.cuda(), w1.cuda(), w2.cuda(), coords.cuda(), add.cuda(),
                                   L.current_stream())

    def chain(out):
        csp, gate = torch.empty(B, parts, c, device="cuda"), torch.empty(B, c, device="cuda")
        L.call("gldm_gn_swish_chan_sum_cl", L.ptr(dy), L.ptr(dc), B, c, r, L.ptr(csp), st)
        L.call("gldm_se_gate_parts", L.ptr(csp), parts, L.ptr(d1), L.ptr(d2), B, c, hidden, r, 1, L.ptr(gate), st)
        L.call("gldm_devoxelize_gn_cl_fused", L.ptr(dco), L.ptr(dy), L.ptr(dc), L.ptr(gate), L.ptr(da), B, c, n, r, L.ptr(out), st)
        chain.gate = gate

    got = _twice(chain, (B, c, n))
    _check("chain: gate", chain.gate, ref_gate, BAR)
    _check("chain: squeeze_cl -> se_gate_parts -> devoxelize_gn_cl", got, ref, BAR * act.flatten(2).abs().amax(-1, keepdim=True).clamp(min=1.0))
