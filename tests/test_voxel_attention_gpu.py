"""GPU (MI355X): voxel attention inside PVConv.  The fused attention core (csrc/point_attention_fused.hip) through the C
ABI, the two small launches of the voxel attention stack, and the modules with the switch on against the reference
(pvconv_attn.npz, pvcnn2_attn.npz).

Core tolerance per case = max(2e-5 max(1, max|out|), 4 e32), the rule of tests/test_attention_gpu.py (its helpers are
imported, not restated): e32 is the error of the same formula evaluated by torch on the CPU in f32 against f64 on the same
inputs.  Shapes are the smallest at which each mechanism of the kernel exists: one query tile and one key tile; a K block
and a half with inactive waves; several key tiles on the 8^3 grid; the widest C with an odd number of 32-key tiles and a
half-filled workgroup; the 12^3 grid; the largest n."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_attention_gpu import attention_ref, block_ref, make_qkv, run_core

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 64),      # one query tile, one key tile pair
          (2, 48, 96),      # one and a half K blocks, a key tail when tiles are 64
          (2, 64, 512),     # several key tiles, the 8^3 grid
          (1, 128, 320),    # widest C, odd tile count
          (1, 64, 1728),    # the 12^3 grid
          (1, 32, 4096)]    # largest n
KINDS = ["normal", "last_tile_max", "dominant", "zero_q", "negative", "alias", "ascending"]
KEY_TILE = 32               # keys per staged tile of the fused kernel
# zero_q: the result is the mean of v.  A mean of n unit-normal values accumulated in f32 has running sums of up to 3 sqrt(n)
# and, on the f32 matrix pipe, n / 4 accumulator roundings of 2^-24 of that each: as a random walk that is
# 2^-24 x 3 sqrt(n) x sqrt(n / 4) / n = 1.5 x 2^-24 = 9e-8, whatever n is and however small the mean itself (1 / sqrt(n))
# comes out.  The bound is four of those, or 1e-6 of the mean's magnitude (test_attention_gpu's bound) where that is larger.
MEAN_F32 = 4 * 1.5 * 2.0 ** -24


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def make_case(kind, b, c, n, seed=0):
    if kind != "ascending":
        return make_qkv(kind, b, c, n, seed)
    # every row's largest logit grows from key tile to key tile: an online softmax rescales at every tile.  Channel 0
    # carries a staircase of 6 x 1.5 sqrt(c) per 32 keys on top of logits of sigma sqrt(c - 1)
    q, k, v = make_qkv("normal", b, c, n, seed)
    q[:, 0, :] = 6.0
    k[:, 0, :] = (torch.arange(n) // KEY_TILE).float() * (1.5 * c ** 0.5)
    return q, k, v


def run_fused(q, k, v, exact):
    """gldm_point_attention_fused through the C ABI on CUDA tensors (v may be k)."""
    from graspldm_amd import _lib as L
    out = torch.empty_like(q)
    b, c, n = q.shape
    L.call("gldm_point_attention_fused", L.ptr(q), L.ptr(k), L.ptr(v), b, c, n, int(exact), L.ptr(out), L.current_stream(q.device))
    return out


_REFS = {}


def reference(kind, shape, seed=0):
    """(q, k, v, f64 reference, e32) of a case, computed once and shared by the tests that need it."""
    key = (kind, shape, seed)
    if key not in _REFS:
        q, k, v = make_case(kind, *shape, seed=seed)
        ref = attention_ref(q.double(), k.double(), v.double())
        e32 = (attention_ref(q, k, v).double() - ref).abs().max().item()
        _REFS[key] = (q, k, v, ref, e32)
    return _REFS[key]


def tolerance(ref, e32, relative=False):
    scale = ref.abs().max().item()
    return max(2e-5 * (scale if relative else max(1.0, scale)), 4 * e32)


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_core_against_f64(shape, exact):
    b, c, n = shape
    name = "f32" if exact else "split"
    for kind in KINDS:
        q, k, v, ref, e32 = reference(kind, shape)
        qc, kc = q.cuda(), k.cuda()
        got = run_fused(qc, kc, kc if v is k else v.cuda(), exact).cpu()
        assert torch.isfinite(got).all()
        err, tol = (got.double() - ref).abs().max().item(), tolerance(ref, e32)
        print(f"fused core {name} {shape} {kind}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (kind, err, tol)
        logits = q.double().transpose(1, 2) @ k.double()
        if kind == "last_tile_max":
            assert (logits.argmax(dim=-1) >= n - 5).all()
        elif kind == "ascending" and n > KEY_TILE:
            tile_max = logits.reshape(b, n, n // KEY_TILE, KEY_TILE).max(dim=-1).values
            assert (tile_max[..., 1:] > tile_max[..., :-1]).all()
        elif kind == "dominant":
            col = torch.stack([v[i, :, (n - 3, 17, n // 2)[i % 3]] for i in range(b)])[:, :, None].expand(b, c, n)
            assert (got - col).abs().max() <= 1e-6 * col.abs().max(), (got - col).abs().max()
        elif kind == "zero_q":
            mean = v.double().mean(dim=-1, keepdim=True).expand(b, c, n)
            emean = (got.double() - mean).abs().max().item()
            bound = max(1e-6 * mean.abs().max().item(), MEAN_F32)
            print(f"fused core {name} {shape} zero_q: |out - mean v| {emean:.3e}, bound {bound:.3e}")
            assert emean <= bound, emean
        elif kind == "negative":
            assert logits.max() < -1e3


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_core_against_the_materialised_core(shape, exact):
    """Every shape both kernels accept: within the sum of the two tolerances (each kernel is within its own of f64)."""
    q, k, v, ref, e32 = reference("normal", shape)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    a, m = run_fused(qc, kc, vc, exact), run_core(qc, kc, vc, exact)
    diff, tol = (a - m).abs().max().item(), 2 * tolerance(ref, e32)
    print(f"fused against materialised {'f32' if exact else 'split'} {shape}: diff {diff:.3e} tol {tol:.3e}")
    assert diff <= tol


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("what,scale", [("v", 1e5), ("v", 1e-6), ("qk", 1e2), ("qk", 1e-3)])
@pytest.mark.parametrize("shape", [(2, 48, 96), (1, 128, 320)], ids=lambda s: "x".join(map(str, s)))
def test_fused_core_operand_range(shape, what, scale, exact):
    """As test_core_operand_range: v of 1e5 and 1e-6, q and k of 1e2 and 1e-3; the bar relative to the output's magnitude."""
    b, c, n = shape
    q, k, v = make_qkv("normal", b, c, n, seed=3)
    if what == "v":
        v = v * scale
        v[-1, : c // 2] *= 1e-3
    else:
        q, k = q * scale, k * scale
    ref = attention_ref(q.double(), k.double(), v.double())
    e32 = (attention_ref(q, k, v).double() - ref).abs().max().item()
    got = run_fused(q.cuda(), k.cuda(), v.cuda(), exact).cpu()
    assert torch.isfinite(got).all()
    err, tol = (got.double() - ref).abs().max().item(), tolerance(ref, e32, relative=True)
    print(f"fused range {'f32' if exact else 'split'} {shape} {what} x {scale:g}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
def test_fused_core_bitwise(exact):
    b, c, n = 3, 96, 320
    q, k, v = (t.cuda() for t in make_qkv("normal", b, c, n, seed=5))
    a = run_fused(q, k, v, exact)
    torch.cuda.synchronize()
    assert torch.equal(a, run_fused(q, k, v, exact))                                   # two launches
    alone = run_fused(q[2:3].contiguous(), k[2:3].contiguous(), v[2:3].contiguous(), exact)
    assert torch.equal(alone[0], a[2])                                                  # position 2 of 3 against alone
    torch.cuda.synchronize()
    cur, streams, got = torch.cuda.current_stream(), [torch.cuda.Stream() for _ in range(3)], []
    for st in streams:
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            got.append(run_fused(q, k, v, exact))
    torch.cuda.synchronize()
    for i, o in enumerate(got):
        assert torch.equal(o, a), f"stream {i}: max abs diff {(o - a).abs().max().item():.3e}"


def test_fused_core_launches_nothing_on_a_rejected_call():
    from graspldm_amd import _lib as L
    h = L.lib()
    b, c, n = 2, 32, 64
    q = torch.randn(b, c, n, device="cuda")
    out = torch.full_like(q, 7.0)
    st = L.current_stream(q.device)
    assert h.gldm_point_attention_fused(L.ptr(q), L.ptr(q), L.ptr(q), b, 16, n, 0, L.ptr(out), st) == -3
    assert h.gldm_point_attention_fused(L.ptr(q), L.ptr(q), L.ptr(q), b, c, 48, 0, L.ptr(out), st) == -3
    assert h.gldm_point_attention_fused(ctypes.c_void_p(q.data_ptr() + 4), L.ptr(q), L.ptr(q), 1, c, n, 0, L.ptr(out), st) == -1
    assert h.gldm_point_attention_fused(L.ptr(q), None, L.ptr(q), b, c, n, 0, L.ptr(out), st) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert h.gldm_point_attention_fused(L.ptr(q), L.ptr(q), L.ptr(q), b, c, n, 0, L.ptr(out), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).any()


def test_groupnorm_affine_on_a_voxel_grid():
    """gldm_groupnorm_coef + gldm_groupnorm_affine against F.group_norm in f64 at 2e-5 absolute (no activation), from the statistics
    a conv leaves; 4^3 and 12^3 grids, 4 and 96 channels per group (the coefficient launch's widened range); bitwise
    repeatable."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(12)
    for b, cin, c, r in [(2, 16, 32, 4), (3, 32, 64, 12), (1, 16, 768, 4)]:
        x = torch.randn(b, cin, r, r, r, generator=g)
        w = torch.randn(c, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
        bias, gamma, beta = torch.randn(c, generator=g) + 3.0, 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        st = L.current_stream()
        y = torch.empty(b, c, r, r, r, device="cuda")
        partial = torch.empty(int(L.lib().gldm_conv3d_partial_floats(b, c, r)), device="cuda")
        dx, dw, db, dg, dbe = x.cuda(), w.cuda().contiguous(), bias.cuda(), gamma.cuda(), beta.cuda()
        L.call("gldm_conv3d_k3_generic", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, c, r, L.ptr(y), L.ptr(partial), st)
        coef = torch.empty(b, c, 2, device="cuda")
        L.call("gldm_groupnorm_coef", L.ptr(partial), L.ptr(dg), L.ptr(dbe), b, c, r, 8, 1e-5, L.ptr(coef), st)
        out, again = torch.empty(b, c, r ** 3, device="cuda"), torch.empty(b, c, r ** 3, device="cuda")
        L.call("gldm_groupnorm_affine", L.ptr(y), L.ptr(coef), b, c, r, L.ptr(out), st)
        L.call("gldm_groupnorm_affine", L.ptr(y), L.ptr(coef), b, c, r, L.ptr(again), st)
        ref = F.group_norm(y.cpu().double(), 8, gamma.double(), beta.double(), 1e-5).reshape(b, c, -1)
        err = (out.cpu().double() - ref).abs().max().item()
        print(f"groupnorm affine {(b, c, r)}: err {err:.3e}")
        assert err <= 2e-5, (b, c, r, err)
        assert torch.equal(out, again)


def test_groupnorm_swish_points_with_the_squeeze_sums():
    """gldm_groupnorm_swish_points_sum: the output is gldm_groupnorm_swish_points' within 2e-5 of f64, the sums over n
    against an f64 sum at the bar of gldm_gn_swish_chan_sum's test (2e-5 on the mean); a residual, no residual, 128 channels
    per group, n not a multiple of 256; bitwise repeatable."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(4)
    for b, c, n, groups, res in [(2, 32, 64, 8, True), (3, 64, 1728, 8, True), (1, 1024, 64, 8, False), (2, 48, 36, 4, True)]:
        x, add = torch.randn(b, c, n, generator=g) * 3 + 20.0, torch.randn(b, c, n, generator=g)
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        y = F.group_norm((x + add if res else x).double(), groups, gamma.double(), beta.double(), 1e-5)
        ref = y * torch.sigmoid(y)
        xc, ac, gc, bc = x.cuda(), add.cuda() if res else None, gamma.cuda(), beta.cuda()
        outs = []
        for _ in range(2):
            out, cs = torch.empty(b, c, n, device="cuda"), torch.empty(b, c, device="cuda")
            L.call("gldm_groupnorm_swish_points_sum", L.ptr(xc), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(out),
                   L.ptr(cs), L.current_stream(xc.device))
            outs.append((out, cs))
        (out, cs), (out2, cs2) = outs
        err = (out.cpu().double() - ref).abs().max().item()
        esum = (cs.cpu().double() / n - ref.mean(dim=-1)).abs().max().item()
        print(f"groupnorm swish + sums {(b, c, n, groups)}: err {err:.3e}, mean err {esum:.3e}")
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (b, c, n, err)
        assert esum <= 2e-5, (b, c, n, esum)
        assert torch.equal(out, out2) and torch.equal(cs, cs2)
        plain = torch.empty(b, c, n, device="cuda")
        L.call("gldm_groupnorm_swish_points", L.ptr(xc), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(plain),
               L.current_stream(xc.device))
        assert torch.equal(out, plain)


# ---------------------------------------------------------------------------------------------------------------- modules
# Bars are the files' own, as in tests/test_attention_gpu.py: max(bar, 4 d) with the fixture's d, the reference's own f32
# voxel stack against a .double() copy of it (tools/make_golden_voxel_attention.py).
def pvconv_inputs():
    """The inputs of pvconv_attn.npz are their seeds (tools/make_golden_voxel_attention.py: pvconv_inputs)."""
    from graspldm_amd.synthetic import synthetic_batch
    feats = torch.randn(2, 32, 256, generator=torch.Generator().manual_seed(47))
    return feats, synthetic_batch(2, 256)[0].transpose(1, 2).contiguous()


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
@pytest.mark.parametrize("r", [4, 8])
def test_pvconv_with_attention_against_the_reference(r, f32):
    from graspldm_amd import numerics
    from graspldm_amd.pvcnn import PVConv
    from graspldm_amd.synthetic import load_synthetic_weights
    g = load_golden("pvconv_attn.npz")
    want, d = g[f"y_r{r}"], float(g[f"d_r{r}"])
    feats, coords = pvconv_inputs()
    with numerics.f32_only(f32):
        m = load_synthetic_weights(PVConv(32, 32, 3, resolution=r, use_attention=True, with_se=True, with_se_relu=True), seed=0)
        m = m.cuda().eval()
        with torch.no_grad():
            y, c = m((feats.cuda(), coords.cuda()))
            y2, _ = m((feats.cuda(), coords.cuda()))
    assert y.shape == (2, 32, 256) and torch.equal(c.cpu(), coords) and torch.equal(y, y2)
    err, tol = (y.cpu()[:, :, ::8] - want).abs().max().item(), max(2e-5, 4 * d)
    print(f"PVConv + attention r={r} {'f32_only' if f32 else 'split'}: |y - ref| {err:.3e}, tol {tol:.3e} (d {d:.3e})")
    assert err <= tol, (err, tol)


@pytest.fixture(scope="module")
def pvcnn2_attn():
    from graspldm_amd.synthetic import synthetic_batch
    return load_golden("pvcnn2_attn.npz"), synthetic_batch(2, 1024)[0]


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_pvcnn2_with_attention_against_the_reference(pvcnn2_attn, f32):
    """Backbone features at the bar tests/test_models_gpu.py applies to pvcnn2.npz (1e-4)."""
    from graspldm_amd import numerics
    from graspldm_amd.attention import Attention
    from graspldm_amd.pvcnn import PVCNN2
    from graspldm_amd.synthetic import load_synthetic_weights
    g, pcs = pvcnn2_attn
    d = float(g["d"])
    with numerics.f32_only(f32):
        m = load_synthetic_weights(PVCNN2(use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5), seed=0)
        m = m.cuda().eval()
        assert isinstance(m.sa_layers[1][0].voxel_layers[6], Attention)
        with torch.no_grad():
            out = m(pcs.cuda().transpose(1, 2).contiguous()).cpu()
    err, tol = (out[:, :, ::16] - g["out"]).abs().max().item(), max(1e-4, 4 * d)
    print(f"PVCNN2 + attention {'f32_only' if f32 else 'split'}: |out - ref| {err:.3e}, tol {tol:.3e} (d {d:.3e})")
    assert out.shape == (2, 32, 1024) and err <= tol, (err, tol)


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_pvcnn2_encoder_with_local_attention(pvcnn2_attn, f32):
    """PVCNN2Encoder(scale 0.5, use_local_attention=True): the head (conv_downscale -> out_layer) in f64 on the CPU from
    the GPU backbone's own features, the 5e-5 latent bar + 4 x the error of the same tail in f32 on the CPU."""
    from graspldm_amd import numerics
    from graspldm_amd.attention import Attention
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    from graspldm_amd.synthetic import load_synthetic_weights
    _, pcs = pvcnn2_attn
    with numerics.f32_only(f32):
        enc = load_synthetic_weights(PVCNN2Encoder(in_features=3, out_features=64, n_points=1024, scale_channels=0.5,
                                                   scale_voxel_resolution=0.5, out_channels=3, use_local_attention=True),
                                     seed=0).cuda().eval()
        assert isinstance(enc.pvcnn_modules.sa_layers[1][0].voxel_layers[6], Attention)
        with torch.no_grad():
            feats = enc.pvcnn_modules(pcs.cuda().transpose(1, 2).contiguous()).cpu()
            z = enc(pcs.cuda()).cpu()
    sd = {k: v.cpu() for k, v in enc.state_dict().items()}

    def tail(f):
        dt = f.dtype
        h = F.conv1d(f, sd["conv_downscale.weight"].to(dt), sd["conv_downscale.bias"].to(dt))
        h = F.conv1d(h, sd["out_layer.0.weight"].to(dt), sd["out_layer.0.bias"].to(dt))
        return F.linear(h, sd["out_layer.1.weight"].to(dt), sd["out_layer.1.bias"].to(dt))
    z64 = tail(feats.double())
    d = (tail(feats).double() - z64).abs().max().item()
    e = (z.double() - z64).abs().max().item()
    print(f"PVCNN2Encoder + local attention {'f32_only' if f32 else 'split'}: |z - f64 tail| {e:.3e}, d {d:.3e}")
    assert z.shape == (2, 3, 64) and e <= 5e-5 + 4 * d, (e, d)


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_pvconv_with_attention_on_the_materialised_core(f32):
    """C = 256 at r = 4 (64 tokens): wider than the fused kernel, so attention_core takes gldm_point_attention.  Against an
    f64 restatement of the voxel stack (pvconv.py:57-83 with modules.py:34-54 and se.py:12-25) on the kernel's own voxel
    grid, devoxelized by gldm_devoxelize_fused with the module's own point branch.  Bar: max(2e-5 max(1, |y|), 4 d), d = the
    same restatement in f32 on the CPU against f64."""
    from graspldm_amd import _lib as L
    from graspldm_amd import numerics
    from graspldm_amd.pvcnn import PVConv
    from graspldm_amd.synthetic import load_synthetic_weights
    feats, coords = pvconv_inputs()
    c, r = 256, 4
    with numerics.f32_only(f32):
        m = load_synthetic_weights(PVConv(32, c, 3, resolution=r, use_attention=True, with_se=True, with_se_relu=True), seed=0)
        m = m.cuda().eval()
        with torch.no_grad():
            y, _ = m((feats.cuda(), coords.cuda()))
            vox, norm_coords = m.voxelization(feats.cuda(), coords.cuda())
            pf = m.point_features(feats.cuda()).contiguous()
    sd = {k: v.cpu() for k, v in m.voxel_layers.state_dict().items()}

    def stack(x):
        dt = x.dtype
        p = lambda k: sd[k].to(dt)   # noqa: E731
        h = F.group_norm(F.conv3d(x, p("0.weight"), p("0.bias"), padding=1), 8, p("1.weight"), p("1.bias"), 1e-5)
        h = h * torch.sigmoid(h)
        h = F.group_norm(F.conv3d(h, p("4.weight"), p("4.bias"), padding=1), 8, p("5.weight"), p("5.bias"), 1e-5)
        h = block_ref(h, sd, pre="6.")
        gate = torch.sigmoid(F.linear(torch.relu(F.linear(h.mean(dim=(2, 3, 4)), p("7.fc.0.weight"))), p("7.fc.2.weight")))
        return h * gate[:, :, None, None, None]
    z64 = stack(vox.cpu().double())
    d = (stack(vox.cpu()).double() - z64).abs().max().item()
    want = torch.empty_like(y)
    z = z64.float().contiguous().cuda()
    L.call("gldm_devoxelize_fused", L.ptr(norm_coords), L.ptr(z), None, L.ptr(pf), 2, c, 256, r, L.ptr(want), L.current_stream(y.device))
    err, tol = (y - want).abs().max().item(), max(2e-5 * max(1.0, want.abs().max().item()), 4 * d)
    print(f"PVConv + attention C=256 r=4 {'f32_only' if f32 else 'split'}: err {err:.3e}, tol {tol:.3e} (d {d:.3e})")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_ldm_generates_with_local_attention(f32):
    """build_fpc_ldm(PVCNN2Encoder at half scale, use_local_attention=True): 2 clouds x 4 grasps, 10 DDIM steps; finite
    poses, rotations orthonormal to 1e-5, bitwise repeatable."""
    from graspldm_amd import numerics
    from graspldm_amd.attention import Attention
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.rotations import tmrp_to_H
    from graspldm_amd.synthetic import synthetic_batch
    pcs = synthetic_batch(2, 1024)[0].cuda()
    x_T = torch.randn(8, 1, 4, generator=torch.Generator().manual_seed(3)).cuda()
    runs = []
    with numerics.f32_only(f32):
        ldm = build_fpc_ldm(encoder="PVCNN2Encoder", encoder_scale=(0.5, 0.5), use_local_attention=True).cuda().eval()
        ldm.set_inference_timesteps(10)
        assert isinstance(ldm.vae_model.encoder.pc_encoder.pvcnn_modules.sa_layers[1][0].voxel_layers[6], Attention)
        for _ in range(2):
            (tmrp, logit), _ = ldm.generate_grasps(pcs, num_grasps=4, x_T=x_T.clone())
            ldm.check_engines()
            runs.append((tmrp.clone(), logit.clone()))
    tmrp, logit = runs[0]
    assert tmrp.shape == (8, 6) and torch.isfinite(tmrp).all() and torch.isfinite(logit).all()
    H = tmrp_to_H(tmrp)
    R = H[:, :3, :3].double()
    assert (R @ R.transpose(1, 2) - torch.eye(3, device=R.device, dtype=R.dtype)).abs().max() <= 1e-5
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_classifier_with_voxel_attention_backbone(f32):
    """PointsBasedGraspClassifier over PVCNN2 (0.5, 0.5) with use_attention=True: probabilities in [0, 1], finite, one chunk
    against three chunks bitwise."""
    from graspldm_amd import numerics
    from graspldm_amd.attention import Attention
    from graspldm_amd.pipeline import build_classifier
    from graspldm_amd.synthetic import PC_STD, synthetic_batch
    from test_classifier_gpu import _scene_inputs
    pcs, metas = synthetic_batch(3, 1024)
    _, H, _ = _scene_inputs(3, 1, 1024, 64, seed=9)
    H[:, :3, 3] = (H[:, :3, 3] - H[:, :3, 3].mean(0)) + metas["pc_mean"]
    kw = dict(pc_mean=metas["pc_mean"].cuda(), pc_scale=PC_STD)
    pc, Hc = pcs.cuda(), H.view(3, 1, 4, 4).cuda()
    with numerics.f32_only(f32):
        model = build_classifier(1024, 64, "PVCNN2", seed=0, backbone_args=dict(
            use_attention=True, width_multiplier=0.5, voxel_resolution_multiplier=0.5)).cuda()
        assert isinstance(model.base_network.sa_layers[1][0].voxel_layers[6], Attention)
        full = model.score_poses(pc, Hc, **kw)
        chunked = model.score_poses(pc, Hc, max_bytes=model._scene_bytes(1088), **kw)   # 3 chunks of a scene
    assert full.shape == (3, 1) and torch.isfinite(full).all() and ((full >= 0) & (full <= 1)).all()
    assert torch.equal(full, chunked)
