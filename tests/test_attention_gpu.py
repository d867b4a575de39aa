"""GPU (MI355X): the point-attention kernels (csrc/point_attention.hip) through the C ABI, the Attention module against the
reference's block (attention_block.npz) and the encoders with use_global_attention=True against the reference encoder's
latents (pvcnn_encoder_attn.npz).

Core tolerance per case = max(2e-5 max(1, max|out|), 4 e32): 2e-5 is the project's single-forward bar; e32 is the error of
the SAME formula evaluated by torch on the CPU in f32 against f64 on the same inputs (computed here), and the factor 4
covers a different summation order plus the split products where the f32 evaluation itself exceeds the bar (768-deep logits
of unit-normal data have sigma 28: an f32 rounding of the logit is already 1e-6 of the probabilities)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 32),      # K padded to the MFMA depth, less than one 64-key tile
          (2, 48, 96),      # one and a half K blocks, tail tile
          (2, 96, 320),     # odd tile count
          (1, 768, 128),    # the shipped K depth
          (1, 32, 1024),    # flat rows, P ~ 2^-10
          (1, 64, 1056)]    # more than 1024 keys
KINDS = ["normal", "last_tile_max", "dominant", "zero_q", "negative", "alias"]
WORST = {}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def attention_ref(q, k, v):
    """out[b,c,i] = sum_j v[b,c,j] softmax_j(sum_c' q[b,c',i] k[b,c',j]) in the dtype of the inputs (torch, CPU)."""
    p = torch.softmax(q.transpose(1, 2) @ k, dim=-1)
    return v @ p.transpose(1, 2)


def block_ref(x, sd, groups=8, pre=""):
    """modules.py:34-54 restated: the Attention block from its state dict, in the dtype of x."""
    b, c = x.shape[:2]
    h = x.reshape(b, c, -1)
    w = lambda n: sd[pre + n + ".weight"].reshape(c, c).to(x.dtype)   # noqa: E731
    bias = lambda n: sd[pre + n + ".bias"].to(x.dtype)[None, :, None]   # noqa: E731
    q, k, v = (w(n) @ h + bias(n) for n in "qkv")
    y = w("out") @ attention_ref(q, k, v) + bias("out") + h
    y = F.group_norm(y, groups, sd[pre + "norm.weight"].to(x.dtype), sd[pre + "norm.bias"].to(x.dtype), 1e-5)
    return (y * torch.sigmoid(y)).reshape(x.shape)


def make_qkv(kind, b, c, n, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * c + n)
    q, k, v = (torch.randn(b, c, n, generator=g) for _ in range(3))
    if kind == "last_tile_max":       # every row's largest logit among the last keys (the last key tile of any tiling)
        q[:, 0, :], k[:, 0, :] = 6.0, 0.0
        k[:, 0, n - 5:] = 4.0 * c ** 0.5 + 8.0
    elif kind == "dominant":          # one logit more than 1e3 above the rest of its row: key j0, another tile per cloud
        q[:, 0, :], k[:, 0, :] = 40.0, 0.0
        for i in range(b):
            k[i, 0, (n - 3, 17, n // 2)[i % 3]] = 40.0 + 0.3 * c
    elif kind == "zero_q":
        q.zero_()
    elif kind == "negative":          # every logit below -1e3
        q[:, 0, :] = 40.0
        k[:, 0, :] = -(40.0 + 0.3 * c) * (1.0 + 0.1 * torch.rand(b, n, generator=g))
    elif kind == "alias":
        v = k
    return q, k, v


def run_core(q, k, v, exact):
    """gldm_point_attention through the C ABI on CUDA tensors (v may be k)."""
    from graspldm_amd import _lib as L
    b, c, n = q.shape
    nbytes = L.lib().gldm_point_attention_workspace_bytes(b, c, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    L.call("gldm_point_attention", L.ptr(q), L.ptr(k), L.ptr(v), b, c, n, int(exact), L.ptr(ws), nbytes, L.ptr(out),
           L.current_stream(q.device))
    return out


def core_case(q, k, v, exact, relative=False):
    """-> (error, tolerance, f64 reference) of one launch under the rule in the module docstring."""
    ref = attention_ref(q.double(), k.double(), v.double())
    e32 = (attention_ref(q, k, v).double() - ref).abs().max().item()
    qc, kc = q.cuda(), k.cuda()
    got = run_core(qc, kc, kc if v is k else v.cuda(), exact).cpu()
    assert torch.isfinite(got).all()
    scale = ref.abs().max().item()
    tol = max(2e-5 * (scale if relative else max(1.0, scale)), 4 * e32)
    return (got.double() - ref).abs().max().item(), tol, ref, got


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_core_against_f64(shape, exact):
    b, c, n = shape
    for kind in KINDS:
        q, k, v = make_qkv(kind, b, c, n)
        err, tol, ref, got = core_case(q, k, v, exact)
        ratio = err / tol
        WORST[("f32" if exact else "split", shape, kind)] = ratio
        print(f"attention core {'f32' if exact else 'split'} {shape} {kind}: err {err:.3e} tol {tol:.3e} ratio {ratio:.3f}")
        assert err <= tol, (kind, err, tol)
        logits = q.double().transpose(1, 2) @ k.double()
        if kind == "last_tile_max":
            assert (logits.argmax(dim=-1) >= n - 5).all()
        elif kind == "dominant":          # the result is that key's v column
            top = logits.topk(2, dim=-1).values
            assert ((top[..., 0] - top[..., 1]) > 1e3).all()
            col = torch.stack([v[i, :, (n - 3, 17, n // 2)[i % 3]] for i in range(b)])[:, :, None].expand(b, c, n)
            assert (got - col).abs().max() <= 1e-6 * col.abs().max(), (got - col).abs().max()
        elif kind == "zero_q":            # the result is the mean of v, to 1e-6 of that mean's magnitude
            mean = v.double().mean(dim=-1, keepdim=True).expand(b, c, n)
            emean = (got.double() - mean).abs().max().item()
            print(f"attention core {'f32' if exact else 'split'} {shape} zero_q: |out - mean v| {emean:.3e}, "
                  f"bound {1e-6 * mean.abs().max().item():.3e}")
            assert emean <= 1e-6 * mean.abs().max(), emean
        elif kind == "negative":
            assert logits.max() < -1e3
    worst = max(r for (a, s, _), r in WORST.items() if s == shape and a == ("f32" if exact else "split"))
    print(f"attention core worst ratio {'f32' if exact else 'split'} {shape}: {worst:.3f}")


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("what,scale", [("v", 1e5), ("v", 1e-6), ("qk", 1e2), ("qk", 1e-3)])
@pytest.mark.parametrize("shape", [(2, 48, 96), (1, 128, 320)], ids=lambda s: "x".join(map(str, s)))
def test_core_operand_range(shape, what, scale, exact):
    """v of 1e5 (an f16 hi piece is inf without the group scale) and 1e-6 (a subnormal hi piece), q and k of 1e2 and 1e-3:
    the same bars, relative to the output's magnitude; clouds of different magnitude in one launch."""
    b, c, n = shape
    q, k, v = make_qkv("normal", b, c, n, seed=3)
    if what == "v":
        v = v * scale
        v[-1, : c // 2] *= 1e-3
    else:
        q, k = q * scale, k * scale
    err, tol, ref, got = core_case(q, k, v, exact, relative=True)
    print(f"attention range {'f32' if exact else 'split'} {shape} {what} x {scale:g}: err {err:.3e} tol {tol:.3e} "
          f"ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
def test_core_bitwise(exact):
    b, c, n = 3, 96, 320
    q, k, v = (t.cuda() for t in make_qkv("normal", b, c, n, seed=5))
    a = run_core(q, k, v, exact)
    torch.cuda.synchronize()
    assert torch.equal(a, run_core(q, k, v, exact))                                   # two launches
    alone = run_core(q[2:3].contiguous(), k[2:3].contiguous(), v[2:3].contiguous(), exact)
    assert torch.equal(alone[0], a[2])                                                 # position in the batch, b
    torch.cuda.synchronize()
    cur, streams, got = torch.cuda.current_stream(), [torch.cuda.Stream() for _ in range(3)], []
    for st in streams:                                                                 # three side streams, one workspace each
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            got.append(run_core(q, k, v, exact))
    torch.cuda.synchronize()
    for i, o in enumerate(got):
        assert torch.equal(o, a), f"stream {i}: max abs diff {(o - a).abs().max().item():.3e}"


def test_core_chunks_of_clouds_at_the_largest_n():
    """n = 4096: the scores of ONE cloud fill half the 256 MiB workspace cap, so b = 2 runs as two chunks; each cloud equals
    the same cloud launched alone, and cloud 1 the f64 formula."""
    from graspldm_amd import _lib as L
    b, c, n = 2, 16, 4096
    assert L.lib().gldm_point_attention_workspace_bytes(b, c, n) == L.lib().gldm_point_attention_workspace_bytes(1, c, n) <= 256 << 20
    q, k, v = make_qkv("normal", b, c, n, seed=9)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    both = run_core(qc, kc, vc, 0)
    for i in range(b):
        assert torch.equal(run_core(qc[i:i + 1].contiguous(), kc[i:i + 1].contiguous(), vc[i:i + 1].contiguous(), 0)[0], both[i])
    ref = attention_ref(q[1:].double(), k[1:].double(), v[1:].double())
    e32 = (attention_ref(q[1:], k[1:], v[1:]).double() - ref).abs().max().item()
    err, tol = (both[1:].cpu().double() - ref).abs().max().item(), max(2e-5 * max(1.0, ref.abs().max().item()), 4 * e32)
    print(f"attention core split {(b, c, n)} chunked: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol


def test_core_status_codes_without_launching():
    from graspldm_amd import _lib as L
    h = L.lib()
    b, c, n = 2, 32, 64
    q = torch.randn(b, c, n, device="cuda")
    out = torch.full_like(q, 7.0)
    need = h.gldm_point_attention_workspace_bytes(b, c, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = L.current_stream(q.device)
    args = lambda c_, ws_bytes: (L.ptr(q), L.ptr(q), L.ptr(q), b, c_, n, 0, L.ptr(ws), ctypes.c_longlong(ws_bytes), L.ptr(out), st)   # noqa: E731
    assert h.gldm_point_attention(*args(c, need - 1)) == -1          # GLDM_ERR_INVALID_ARG: workspace too small
    assert h.gldm_point_attention(L.ptr(q), L.ptr(q), L.ptr(q), b, c, n, 0, None, ctypes.c_longlong(need), L.ptr(out), st) == -1
    assert h.gldm_point_attention(*args(24, need)) == -3             # GLDM_ERR_UNSUPPORTED: c % 16
    assert h.gldm_point_attention_workspace_bytes(b, 24, n) == -1 and h.gldm_point_attention_workspace_bytes(b, c, 48) == -1
    assert h.gldm_point_attention_workspace_bytes(b, 1040, n) == -1 and h.gldm_point_attention_workspace_bytes(b, c, 4128) == -1
    assert h.gldm_groupnorm_swish_points(L.ptr(q), None, L.ptr(q), L.ptr(q), b, 2048, n, 8, 1e-5, L.ptr(out), st) == -3
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert h.gldm_point_attention(*args(c, need)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.0).all()


def test_groupnorm_swish_points():
    """gldm_groupnorm_swish_points against torch in f64: 2e-5 (the single-forward bar); 96 channels per group at the shipped
    width, a residual, in-place output, a large mean (statistics in f64)."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(2)
    for b, c, n, groups in [(2, 768, 64, 8), (3, 32, 1024, 8), (1, 64, 36, 4)]:
        x, add = torch.randn(b, c, n, generator=g) * 3 + 50.0, torch.randn(b, c, n, generator=g)
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        y = F.group_norm((x + add).double(), groups, gamma.double(), beta.double(), 1e-5)
        ref = y * torch.sigmoid(y)
        xc, ac, gc, bc = x.cuda(), add.cuda(), gamma.cuda(), beta.cuda()
        L.call("gldm_groupnorm_swish_points", L.ptr(xc), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(xc),
               L.current_stream(xc.device))
        err = (xc.cpu().double() - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (b, c, n, err)


def _recipe(module, prefix, seed=0):
    from graspldm_amd.synthetic import synthetic_tensor
    sd = {k: synthetic_tensor(prefix + k, v.shape, seed=seed) for k, v in module.state_dict().items()}
    module.load_state_dict(sd, strict=True)
    return sd


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
@pytest.mark.parametrize("c,d,xk,yk", [(64, 1, "x1", "y1"), (32, 3, "x3", "y3")])
def test_attention_module_against_the_reference_block(c, d, xk, yk, f32):
    """Attention(64, 8, D=1) on (2, 64, 192) and Attention(32, 8, D=3) on (2, 32, 4, 4, 4) with recipe weights: against the
    f64 restatement under the core's tolerance rule (e32 = the reference's own f32 output against f64), and against the
    reference's f32 output itself at that tolerance plus e32 (the reference is that far from f64)."""
    from graspldm_amd import numerics
    from graspldm_amd.attention import Attention
    # the fixture's inputs are their seeds (tools/make_golden_attention.py: block_inputs)
    x = {"x1": torch.randn(2, 64, 192, generator=torch.Generator().manual_seed(41)),
         "x3": torch.randn(2, 32, 4, 4, 4, generator=torch.Generator().manual_seed(43))}[xk]
    y_ref = load_golden("attention_block.npz")[yk]
    m = Attention(c, 8, D=d)
    sd = _recipe(m, "global_attention.")
    y64 = block_ref(x.double(), sd)
    e32 = (y_ref.double() - y64).abs().max().item()
    tol = max(2e-5 * max(1.0, y64.abs().max().item()), 4 * e32)
    with numerics.f32_only(f32):
        m = m.cuda().eval()
        y = m(x.cuda()).cpu()
    assert y.shape == x.shape and torch.isfinite(y).all()
    err64, err = (y.double() - y64).abs().max().item(), (y - y_ref).abs().max().item()
    print(f"Attention({c}, 8, D={d}) {'f32_only' if f32 else 'split'}: |y - f64| {err64:.3e}, |y - ref| {err:.3e}, "
          f"tol {tol:.3e}, e32 {e32:.3e}, ratio {err64 / tol:.3f}")
    assert err64 <= tol and err <= tol + e32, (err64, err, tol, e32)


FPC = dict(in_features=3, out_features=64, scale_channels=0.75, scale_voxel_resolution=0.75, num_blocks=(1, 1, 1, 1),
           out_channels=3, use_global_attention=True)


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
@pytest.mark.parametrize("n", [1024, 64])
def test_pvcnn_encoder_with_global_attention_reference_golden(n, f32):
    from graspldm_amd import numerics
    from graspldm_amd.pc_encoders import PVCNNEncoder
    from graspldm_amd.synthetic import load_synthetic_weights, synthetic_batch
    g = load_golden("pvcnn_encoder_attn.npz")
    z_ref, z64, d = g[f"z_{n}"], g[f"z_f64tail_{n}"], float(g[f"d_{n}"])
    pcs, _ = synthetic_batch(2, n)
    with numerics.f32_only(f32):
        enc = load_synthetic_weights(PVCNNEncoder(n_points=n, **FPC), seed=0).cuda().eval()
        z = enc(pcs.cuda()).cpu()
    assert z.shape == (2, 3, 64)
    e, e64 = (z - z_ref).abs().max().item(), (z.double() - z64).abs().max().item()
    print(f"PVCNNEncoder + attention n={n} {'f32_only' if f32 else 'split'}: |z - ref| {e:.3e}, |z - f64 tail| {e64:.3e}, d {d:.3e}")
    assert e <= 5e-5 and e64 <= 5e-5 + 4 * d, (e, e64, d)


@pytest.mark.parametrize("f32", [False, True], ids=["split", "f32_only"])
def test_pvcnn2_encoder_with_global_attention(f32):
    """PVCNN2Encoder(use_global_attention=True), C = 32: the tail (conv_downscale -> Attention -> out_layer) in f64 on the
    CPU from the GPU backbone's own features.  Bar: the 5e-5 latent bar + 4 x the error of the same tail evaluated by torch
    on the CPU in f32 against f64."""
    from graspldm_amd import numerics
    from graspldm_amd.pc_encoders import PVCNN2Encoder
    from graspldm_amd.synthetic import load_synthetic_weights, synthetic_batch
    pcs, _ = synthetic_batch(2, 1024)
    with numerics.f32_only(f32):
        enc = load_synthetic_weights(PVCNN2Encoder(in_features=3, out_features=64, n_points=1024, scale_channels=1,
                                                   scale_voxel_resolution=1, out_channels=3, use_global_attention=True),
                                     seed=4).cuda().eval()
        assert enc.global_attention.q.weight.shape[0] == 32
        x = pcs.cuda().transpose(1, 2).contiguous()
        feats = enc._backbone_and_head(x, None, None, None).cpu()
        z = enc(pcs.cuda()).cpu()
    sd = {k: v.cpu() for k, v in enc.state_dict().items()}

    def tail(f):
        dt = f.dtype
        h = F.conv1d(f, sd["conv_downscale.weight"].to(dt), sd["conv_downscale.bias"].to(dt))
        h = block_ref(h, sd, pre="global_attention.")
        h = F.conv1d(h, sd["out_layer.0.weight"].to(dt), sd["out_layer.0.bias"].to(dt))
        return F.linear(h, sd["out_layer.1.weight"].to(dt), sd["out_layer.1.bias"].to(dt))
    z64 = tail(feats.double())
    d = (tail(feats).double() - z64).abs().max().item()
    e = (z.double() - z64).abs().max().item()
    print(f"PVCNN2Encoder + attention {'f32_only' if f32 else 'split'}: |z - f64 tail| {e:.3e}, d {d:.3e}")
    assert z.shape == (2, 3, 64) and e <= 5e-5 + 4 * d, (e, d)


def test_ldm_generates_with_global_attention():
    """build_fpc_ldm(use_global_attention=True): 2 clouds x 4 grasps, 10 DDIM steps; finite poses, the denoiser is
    conditioned by encode_pc's output, and the result differs from the switch-off model's."""
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    pcs = synthetic_batch(2, 1024)[0].cuda()
    x_T = torch.randn(8, 1, 4, generator=torch.Generator().manual_seed(3)).cuda()
    outs = []
    for on in (True, False):
        ldm = build_fpc_ldm(use_global_attention=on).cuda().eval()
        ldm.set_inference_timesteps(10)
        assert (ldm.vae_model.encoder.pc_encoder.global_attention is not None) == on
        seen, sample = [], ldm.diffusion_model.sample

        def spy(*a, _sample=sample, _seen=seen, **kw):
            _seen.append(kw["z_cond"].clone())
            return _sample(*a, **kw)
        ldm.diffusion_model.sample = spy
        (tmrp, logit), _ = ldm.generate_grasps(pcs, num_grasps=4, x_T=x_T.clone())
        ldm.check_engines()
        assert tmrp.shape == (8, 6) and torch.isfinite(tmrp).all() and torch.isfinite(logit).all()
        assert len(seen) == 1 and torch.equal(seen[0], ldm.vae_model.encode_pc(pcs))
        outs.append((tmrp.cpu(), seen[0].cpu()))
    assert (outs[0][1] - outs[1][1]).abs().max() > 1e-3 and (outs[0][0] - outs[1][0]).abs().max() > 1e-4


def test_switch_off_encoder_with_more_than_sixteen_output_channels():
    """use_global_attention=False, out_channels = 32: the folded head has more rows than the fused launches take on their
    accumulators, so the backbone's last layer runs alone and the head as a GEMM of its own -- the path this shape always
    took.  Against conv_downscale -> out_layer in f64 on the CPU from the GPU backbone's features, the 5e-5 latent bar."""
    from graspldm_amd.pc_encoders import PVCNNEncoder
    from graspldm_amd.synthetic import load_synthetic_weights, synthetic_batch
    enc = load_synthetic_weights(PVCNNEncoder(n_points=64, **dict(FPC, out_channels=32, use_global_attention=False)), seed=0)
    enc = enc.cuda().eval()
    pcs = synthetic_batch(2, 64)[0].cuda()
    z = enc(pcs).cpu()
    feats = enc.pvcnn_modules(pcs.transpose(1, 2).contiguous()).cpu().double()
    sd = {k: v.cpu().double() for k, v in enc.state_dict().items()}
    h = F.conv1d(feats, sd["conv_downscale.weight"], sd["conv_downscale.bias"])
    h = F.conv1d(h, sd["out_layer.0.weight"], sd["out_layer.0.bias"])
    want = F.linear(h, sd["out_layer.1.weight"], sd["out_layer.1.bias"])
    assert z.shape == (2, 32, 64) and (z.double() - want).abs().max() <= 5e-5, (z.double() - want).abs().max()


def test_pointwise_rows():
    """gldm_pointwise_rows (out_layer[0] behind the attention block) against f64: 2e-5, the single-forward bar; the shipped
    768 -> 3, an odd width with the most rows, no bias; too many rows and a misaligned pointer return their status codes."""
    from graspldm_amd import _lib as L
    g = torch.Generator().manual_seed(8)
    for b, cin, hout, n, has_bias in [(2, 768, 3, 1024, True), (3, 33, 8, 36, True), (1, 64, 1, 260, False)]:
        x, w, bias = torch.randn(b, cin, n, generator=g), torch.randn(hout, cin, generator=g) / cin ** 0.5, torch.randn(hout, generator=g)
        ref = torch.einsum("oc,bcn->bon", w.double(), x.double()) + (bias.double()[None, :, None] if has_bias else 0.0)
        xc, wc, bc = x.cuda(), w.cuda(), bias.cuda() if has_bias else None
        y = torch.empty(b, hout, n, device="cuda")
        L.call("gldm_pointwise_rows", L.ptr(xc), L.ptr(wc), L.ptr(bc), b, cin, hout, n, L.ptr(y), L.current_stream(xc.device))
        err = (y.cpu().double() - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (b, cin, hout, n, err)
    h, st = L.lib(), L.current_stream(xc.device)
    assert h.gldm_pointwise_rows(L.ptr(xc), L.ptr(wc), None, 1, 64, 9, 260, L.ptr(y), st) == -3
    assert h.gldm_pointwise_rows(ctypes.c_void_p(xc.data_ptr() + 4), L.ptr(wc), None, 1, 64, 1, 256, L.ptr(y), st) == -1
    assert h.gldm_groupnorm_swish_points(ctypes.c_void_p(xc.data_ptr() + 4), None, L.ptr(wc), L.ptr(wc), 1, 8, 32, 8, 1e-5,
                                         L.ptr(y), st) == -1
