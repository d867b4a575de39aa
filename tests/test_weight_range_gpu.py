"""GPU (MI355X): the parity bars across WEIGHT magnitudes.  Every split-f16 GEMM multiplies an f32 weight as two f16 pieces;
below |w| = 2^-3 the lo piece is an f16 subnormal and the weight keeps an absolute 2^-25 (weight side).  The
packers ask r1d_pack.split_fits per matrix and send what does not fit to the f32 form the layer already has for weights
beyond 65504.  Here every family of split kernels runs the patterns of tests/weight_range_cases.py -- the whole tensor at
2^-k for k in {0, k_in, 12, 20} (k_in: the largest k the rule accepts for that shape, computed from split_fits: the split
KERNEL at the inside edge of the rule), quiet rows, matched columns -- against f64 (or the torch-CPU oracle's modules in
double on the same weights and neighbourhoods), at the family's existing bar taken relative to the output's magnitude,
quiet rows against their own.  Biases are zero or scaled with their rows.  Each case asserts the route that ran from the plan
attributes (fragments present, `exact`, `split`, the descriptor's split offsets): split for k in {0, k_in}, the f32 form for
the rest.  One line per case, "WR|family|shape|pattern|route|err|bar", is printed before anything is asserted.
"""
import pytest
import torch
import torch.nn.functional as F

import weight_range_cases as W

pytestmark = pytest.mark.gpu

ENGINE_BAR = 5e-6     # tests/test_range_gpu.py::test_resnet_engines_under_wild_conditioning
NORM_BAR = 5e-5       # GroupNorm + swish behind a voxel conv, tests/test_range_gpu.py::test_conv3d_split_range
KINDS = ["k0", "k_in", "k12", "k20", "rows", "cols"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _pattern(kind, k_in):
    """-> (pattern of weight_range_cases, whether the split route must run it)."""
    return {"k0": (("whole", 0), True), "k_in": (("whole", k_in), True), "k12": (("whole", 12), False),
            "k20": (("whole", 20), False), "rows": ("rows", False), "cols": ("cols", False)}[kind]


def _report(family, shape, kind, pattern, split, errs, bar):
    tag = f"2^-{pattern[1]}" if isinstance(pattern, tuple) else pattern
    print(f"WR|{family}|{shape}|{kind}:{tag}|{'split' if split else 'f32'}|{max(errs):.3e}|{bar:.1e}")


def _judge(family, shape, kind, pattern, split, want_split, errs, bar=W.BAR):
    _report(family, shape, kind, pattern, split, errs, bar)
    assert split == want_split, (family, shape, kind, "split" if split else "f32")
    assert max(errs) < bar, (family, shape, kind, errs, bar)


def _group_errs(got, ref, pattern, dim=1):
    m = ref.shape[dim]
    return [W.rel(got.narrow(dim, g.start, g.stop - g.start), ref.narrow(dim, g.start, g.stop - g.start))
            for g in W.row_groups(m, pattern)]


# ------------------------------------------------------------------------------------------------ gldm_pointwise_mlp_f16x2
def _pointwise(x, w, b, head):
    """One layer through the route its fragments allow, as dense._pack_folded decides it: split fragments, else the f32
    launch where it takes the shape, else the any-shape kernel.  -> (y, z, split)."""
    from graspldm_amd import _lib as L
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import SplitRangeError, mfma_a_fragments, mfma_a_fragments_f16x2
    cout, cin = w.shape
    n, hout = x.shape[-1], (head[2] if head else 0)
    try:
        ws = mfma_a_fragments_f16x2(w).cuda()
    except SplitRangeError:
        ws = None
    if ws is not None:
        return (*dense.pointwise_mlp(x, ws, b.cuda(), cout, True, head=head, split=True), True)
    if L.lib().gldm_pointwise_mlp_supported(0, 0, cin, cout, n, hout, 0, 0) == 0:
        return (*dense.pointwise_mlp(x, mfma_a_fragments(w).cuda(), b.cuda(), cout, True, head=head), False)
    assert head is None
    return dense._gemm_bias_act(x, w.cuda(), b.cuda(), True), None, False


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cin,cout,n,hout", [(128, 64, 48, 0), (128, 256, 96, 0), (256, 512, 96, 3)])
def test_pointwise_one_layer(cin, cout, n, hout, kind):
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import split_fits
    w0 = W.kaiming(cout, cin, seed=cin + cout)
    pattern, want = _pattern(kind, W.k_inside(lambda k: split_fits(w0 * 2.0 ** -k)))
    w = W.apply(w0, pattern)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, cin, n, generator=g) / W.col_scale(cin, pattern)[None, :, None]
    ref = torch.einsum("oc,bcn->bon", w.double(), x.double()).relu()
    head = zref = None
    if hout:
        wh = W.kaiming(hout, cout, seed=5)
        zref = torch.einsum("oc,bcn->bon", wh.double(), ref)
        head = (dense.pack_head(wh).cuda(), torch.zeros(hout).cuda(), hout)
    y, z, split = _pointwise(x.cuda(), w, torch.zeros(cout), head)
    errs = _group_errs(y, ref, pattern) + ([W.rel(z, zref)] if hout else [])
    _judge("pointwise_mlp_f16x2", (cin, cout, n, hout), kind, pattern, split, want, errs)


# ----------------------------------------------------------------------------------------------- gldm_pointwise_mlp2_f16x2
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["front", "second"])
def test_pointwise_two_layers(which, kind):
    """96 -> 768 -> 1536 + head at n = 96 (pc_encoders._backbone_and_head: the split launch when both layers have split
    fragments, else gldm_pointwise_mlp2 on f32 fragments).  The pattern goes on one layer; "cols" on the second layer is
    matched by the front layer's rows at 2^12 (with their bias), so the hidden tile itself carries the other unit and
    range_gain of the scaled front layer has to bound it.  Quiet ROWS of the front layer are not observable behind the
    second GEMM (the loud rows drown them), so "rows" on the front layer checks the route and the output as a whole."""
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import SplitRangeError, mfma_a_fragments, mfma_a_fragments_f16x2, split_fits
    cin0, cin, cout, hout, n = 96, 768, 1536, 3, 96
    w0, w1, wh = W.kaiming(cin, cin0, seed=1), W.kaiming(cout, cin, seed=2), W.kaiming(hout, cout, seed=3)
    g = torch.Generator().manual_seed(4)
    b0, x = 0.1 * torch.randn(cin, generator=g), torch.randn(2, cin0, n, generator=g)
    base = w0 if which == "front" else w1
    pattern, want = _pattern(kind, W.k_inside(lambda k: split_fits(base * 2.0 ** -k)))
    if which == "front":
        w0, b0 = W.apply(w0, pattern), b0 * W.row_scale(cin, pattern)
        x = x / W.col_scale(cin0, pattern)[None, :, None]
    else:
        w1 = W.apply(w1, pattern)
        up = 1.0 / W.col_scale(cin, pattern)
        w0, b0 = w0 * up[:, None], b0 * up
    b1 = torch.zeros(cout)
    h = (torch.einsum("oc,bcn->bon", w0.double(), x.double()) + b0.double().view(1, -1, 1)).relu().float().double()
    yref = torch.einsum("oc,bcn->bon", w1.double(), h).relu()
    zref = torch.einsum("oc,bcn->bon", wh.double(), yref)
    gain = dense.range_gain(w0, b0)
    assert float(h.abs().max()) <= gain[0] * float(x.abs().max()) + gain[1]
    head = (dense.pack_head(wh).cuda(), torch.zeros(hout).cuda(), hout)
    try:
        front = (mfma_a_fragments_f16x2(w0).cuda(), b0.cuda(), cin, gain)
        main, split = mfma_a_fragments_f16x2(w1).cuda(), True
    except SplitRangeError:
        assert dense.fused_mlp2_supported(x.cuda(), cin0, cin, cout)
        front, main, split = (mfma_a_fragments(w0).cuda(), b0.cuda(), cin), mfma_a_fragments(w1).cuda(), False
    y, z = dense.pointwise_mlp(x.cuda(), main, b1.cuda(), cout, True, head=head, keep_y=True, front=front, split=split)
    errs = (_group_errs(y, yref, pattern) if which == "second" else [W.rel(y, yref)]) + [W.rel(z, zref)]
    _judge("pointwise_mlp2_f16x2", which, kind, pattern, split, want, errs)


# ------------------------------------------------------------------------- gldm_sa_mlp_forward_f16x2, _pre; one MSG module
def _shape_last_layer(mlp, pattern):
    """The pattern on the LAST layer of a SharedMLP(dim=2) through its BatchNorm, so that the fold produces it:
    running_var grows by the square of the row factor (the bias beta scales with its row), the conv's columns take the
    column factor and the layer in front answers with rows that much larger (its running_var and beta)."""
    conv, bn, prev = mlp.layers[-3], mlp.layers[-2], mlp.layers[-5]
    rs, cs = W.row_scale(conv.weight.shape[0], pattern), W.col_scale(conv.weight.shape[1], pattern)
    with torch.no_grad():
        bn.running_var.mul_(rs ** -2)
        bn.bias.mul_(rs)
        conv.weight.mul_(cs.view(1, -1, 1, 1))
        prev.running_var.mul_(cs ** 2)
        prev.bias.div_(cs)


def _sa_fits(mod):
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import split_fits
    return all(split_fits(dense.fold_conv_bn(mlp.layers[i], mlp.layers[i + 1])[0])
               for mlp in mod.mlps for i in range(0, len(mlp.layers), 3))


def _sa_case(family, kw, feats, coords, kind, seed):
    """One PointNetSAModule forward against the oracle's module in double on the oracle's own neighbourhoods."""
    from graspldm_amd._cache import cached_value
    from graspldm_amd.pvcnn import PointNetSAModule
    from graspldm_amd.synthetic import load_synthetic_weights
    from oracle import torch_ref as R

    def build(pattern):
        mod = load_synthetic_weights(PointNetSAModule(**kw), seed=seed).eval()
        for mlp in mod.mlps:
            _shape_last_layer(mlp, pattern)
        return mod

    pattern, want = _pattern(kind, W.k_inside(lambda k: _sa_fits(build(("whole", k)))))
    mod = build(pattern)
    sd = {k: v.detach().double() for k, v in mod.state_dict().items()}
    radii, us = [g.radius for g in mod.groupers], [g.num_neighbors for g in mod.groupers]
    centers = R.furthest_point_sample(coords, kw["num_centers"])
    refs = [R.shared_mlp(sd, f"mlps.{i}.", R.ball_group(coords, centers, feats, r, u).double()).max(dim=-1).values
            for i, (r, u) in enumerate(zip(radii, us))]
    mod = mod.cuda()
    with torch.no_grad():
        got, ctr = mod((feats.cuda() if feats is not None else None, coords.cuda()))
    assert torch.equal(ctr.cpu(), centers) and torch.isfinite(got).all()
    plans = [cached_value(mlp, "_sa_plan") for mlp in mod.mlps]
    splits = [cached_value(p, "_pre") is not None or cached_value(p, "_split") is not None for p in plans]
    assert all(splits) or not any(splits), splits
    errs, c0 = [], 0
    for ref in refs:
        errs += _group_errs(got[:, c0:c0 + ref.shape[1]], ref, pattern)
        c0 += ref.shape[1]
    _judge(family, tuple(kw["out_channels"]), kind, pattern, all(splits), want, errs)
    return plans


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,c,n,m,u,chans", [(1, 5, 300, 37, 16, (16, 32, 32, 64)), (2, 128, 512, 128, 64, (128, 128, 256))])
def test_sa_module(b, c, n, m, u, chans, kind):
    """(1, 5, 300, ...): gldm_sa_mlp_forward_f16x2; (2, 128, 512, ...): the hoisted form, gldm_sa_mlp_forward_f16x2_pre."""
    from graspldm_amd._cache import cached_value
    g = torch.Generator().manual_seed(2)
    coords = (torch.rand(b, 3, n, generator=g) * 2 - 1).contiguous()
    feats = torch.randn(b, c, n, generator=g)
    kw = dict(num_centers=m, radius=0.35, num_neighbors=u, in_channels=c, out_channels=chans)
    plans = _sa_case("sa_mlp_forward_f16x2" + ("_pre" if c == 128 else ""), kw, feats, coords, kind, seed=11)
    if _pattern(kind, 0)[1]:
        assert (cached_value(plans[0], "_pre") is not None) == (c == 128)


@pytest.mark.parametrize("kind", KINDS)
def test_msg_module(kind):
    """The first multi-scale module of tests/test_msg_gpu.py (two radii, 32 and 128 neighbours) on its golden clouds."""
    from conftest import load_golden
    from test_msg_gpu import SA1, _cloud
    feats = torch.randn(2, 5, 256, generator=torch.Generator().manual_seed(53))
    coords = torch.stack([_cloud(i, 256) for i in load_golden("sa_msg.npz")["clouds"]])
    _sa_case("sa_msg", SA1, feats, coords, kind, seed=11)


# --------------------------------------------------------------------------------------- gldm_conv3d_k3_f16x2 and _gn
def _swish(t):
    return t * torch.sigmoid(t)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cin,cout,r,staged_norm", [(3, 48, 24, False), (48, 96, 12, False), (48, 96, 12, True),
                                                    (128, 128, 4, False), (128, 128, 4, True)])
def test_conv3d(cin, cout, r, staged_norm, kind):
    """VoxelBranchPlan decides the route of one conv; voxel._launch_conv runs it (gldm_conv3d_k3_f16x2, or with
    staged_norm its _gn form applying swish(a x + s) while it stages; the f32 fallback gets that input from a pass in front,
    as voxel.run gives it).  Then the GroupNorm + swish behind it, the re-amplifier of a quiet conv, from the launch's own
    partial sums.  The 3-channel kernel has no staging form."""
    from torch import nn
    from graspldm_amd import _lib as L
    from graspldm_amd import voxel
    from graspldm_amd.r1d_pack import split_fits
    g = torch.Generator().manual_seed(cin * 100 + cout + 1)
    b = 2
    w0 = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias0 = torch.randn(cout, generator=g) * 0.1
    x = torch.randn(b, cin, r, r, r, generator=g)
    x[:, :, ::3] = 0
    a, s = torch.rand(b, cin, generator=g) + 0.5, 0.1 * torch.randn(b, cin, generator=g)
    pattern, want = _pattern(kind, W.k_inside(lambda k: split_fits(w0.reshape(cout, -1) * 2.0 ** -k)))
    rs, cs = W.row_scale(cout, pattern), W.col_scale(cin, pattern)
    w = w0 * rs.view(-1, 1, 1, 1, 1) * cs.view(1, -1, 1, 1, 1)
    bias = bias0 * rs
    if staged_norm:
        a = a / cs[None, :]          # the matched channels arrive 2^12 larger behind the staged swish(a x + s)
        xin = _swish(a.double()[:, :, None, None, None] * x.double() + s.double()[:, :, None, None, None])
    else:
        x = x / cs.view(1, -1, 1, 1, 1)
        xin = x.double()
    ref = F.conv3d(xin, w.double(), bias.double(), padding=1)
    conv = nn.Conv3d(cin, cout, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias)
    conv = conv.cuda()
    plan = voxel.VoxelBranchPlan([conv], "cuda", r)
    split = bool(plan.split[0])
    dx, st = x.cuda(), L.current_stream()
    coef = None
    if staged_norm and split:
        coef = torch.stack([a, s], dim=-1).contiguous().cuda()
    elif staged_norm:
        dx = xin.float().cuda()
    y, part = voxel._launch_conv(plan, 0, conv, dx, coef, b, r, False, st)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    errs = _group_errs(y, ref, pattern)
    gn = F.group_norm(ref, 8, torch.ones(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64), 1e-5)
    ref2 = _swish(gn)
    dg, dbt = torch.ones(cout).cuda(), torch.zeros(cout).cuda()
    L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(part), L.ptr(dg), L.ptr(dbt), b, cout, r, 8, 1e-5, None, st)
    nerr = (y.cpu().double() - ref2).abs().max().item()
    family = "conv3d_k3_f16x2" + ("_gn" if staged_norm else "")
    _report(family + "+norm", (cin, cout, r), kind, pattern, split, [nerr], NORM_BAR)
    _judge(family, (cin, cout, r), kind, pattern, split, want, errs)
    assert nerr < NORM_BAR, (family, kind, nerr)


# ------------------------------------------------------------------------------------------------------------ gldm_cls_head
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,c,n,rows", [(5, 16, 1, 128), (3, 64, 96, 256)])
def test_cls_head(b, c, n, rows, kind):
    """The smallest shape of tests/test_classifier_gpu.py::HEAD_SHAPES and one of 256 rows.  The logit mixes the rows, so a
    row group is measured with w2 zero on the others."""
    from graspldm_amd.grasp_classifier import cls_head, cls_head_supported, pack_head_weights
    from graspldm_amd.r1d_pack import split_fits
    from test_classifier_gpu import head_ref
    assert cls_head_supported(c, rows, n)
    g = torch.Generator().manual_seed(7 * c + n)
    w0 = W.kaiming(rows, c, seed=c + rows)
    pattern, want = _pattern(kind, W.k_inside(lambda k: split_fits(w0 * 2.0 ** -k)))
    w1 = W.apply(w0, pattern)
    x = torch.randn(b, c, n, generator=g) / W.col_scale(c, pattern)[None, :, None]
    w2, l = torch.randn(rows, generator=g) / rows ** 0.5, torch.randn(n, generator=g) / n ** 0.5
    b1 = torch.zeros(rows)
    errs, exact = [], set()
    for grp in W.row_groups(rows, pattern):
        w2g = torch.zeros(rows)
        w2g[grp] = w2[grp]
        pack = pack_head_weights(w1, b1, w2g, l, 0.0, "cuda")
        exact.add(pack.exact)
        logit, _ = cls_head(x.cuda(), pack, rows)
        errs.append(W.rel(logit, head_ref(x.double(), w1.double(), b1.double(), w2g.double(), l.double(), 0.0, 0.0)))
    assert len(exact) == 1
    _judge("cls_head", (b, c, n, rows), kind, pattern, not exact.pop(), want, errs)


# ---------------------------------------------------------------------------------------------------- attention projections
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c,d,shape", [(32, 3, (2, 32, 4, 4, 4)), (64, 1, (2, 64, 192))])
def test_attention_projections(c, d, shape, kind):
    """Attention._packed folds q with k and out with v (attention.fold_attention) and packs the two [C, C] matrices; the
    pattern goes on the module's convs so that the FOLDED matrices carry it (rows of Wk^T Wq are columns of k).  C = 32, the
    module shape of tests/test_attention_gpu.py, has no split launch (fewer than 64 output rows): both of its routes are
    f32 and the case pins that; C = 64 has one.  The projections are run on their own (the block's residual would hide a
    quiet product), then the whole block against the f64 restatement."""
    from graspldm_amd.attention import Attention, fold_attention, run_conv
    from graspldm_amd.r1d_pack import split_fits
    from test_attention_gpu import _recipe, block_ref

    def build(pattern):
        m = Attention(c, 8, D=d)
        _recipe(m, "global_attention.")
        rs, cs = W.row_scale(c, pattern), W.col_scale(c, pattern)
        whole = rs if isinstance(pattern, tuple) else torch.ones(c)
        with torch.no_grad():
            for conv in (m.q, m.k, m.v, m.out):
                conv.bias.zero_()
            wshape = m.q.weight.shape
            m.q.weight.copy_((m.q.weight.reshape(c, c) * whole[:, None] * cs[None, :]).reshape(wshape))
            m.v.weight.copy_((m.v.weight.reshape(c, c) * cs[None, :]).reshape(wshape))
            m.out.weight.copy_((m.out.weight.reshape(c, c) * rs[:, None]).reshape(wshape))
            if pattern == "rows":
                m.k.weight.copy_((m.k.weight.reshape(c, c) * rs[None, :]).reshape(wshape))
        return m

    def folded(m):
        return fold_attention(*(t.reshape(c, c) if t.ndim > 1 else t for t in
                                (m.q.weight, m.q.bias, m.k.weight, m.v.weight, m.v.bias, m.out.weight, m.out.bias)))

    def fits(k):
        wq, _, wo, _ = folded(build(("whole", k)))
        return split_fits(wq.float()) and split_fits(wo.float())

    pattern, want = _pattern(kind, W.k_inside(fits))
    m = build(pattern)
    wq, bq, wo, bo = folded(m)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(43))
    x3 = x.reshape(shape[0], c, -1)
    xs = (x3 / W.col_scale(c, pattern)[None, :, None]).contiguous()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    pq, po = m._packed(torch.device("cuda", torch.cuda.current_device()))
    has_split = c >= 64
    split = pq.ws is not None and po.ws is not None
    assert (pq.ws is None) == (po.ws is None)
    errs = []
    for p, wf, bf in ((pq, wq, bq), (po, wo, bo)):
        got = run_conv(xs.cuda(), p)
        ref = torch.einsum("oc,bcn->bon", wf.float().double(), xs.double()) + bf.float().double().view(1, -1, 1)
        errs += _group_errs(got, ref, pattern)
    y64 = block_ref(x.double(), sd)
    yerr = (m(x.cuda()).cpu().double() - y64).abs().max().item() / max(1.0, y64.abs().max().item())
    _judge("attention_projections", (c, d), kind, pattern, split, want and has_split, errs + [yerr])


# ---------------------------------------------------------------------------------------------------------------- R1dEngine
def _engine_sd(sd, pattern, level=1):
    """The pattern on a level's downsample conv and its attention's to_qkv / to_out (rows with their biases; "cols" has no
    matched activation inside a network, the columns are simply quiet).  The ResnetBlocks' convs are weight-standardised
    by the packer and so immune to their own magnitude; a small weight on a residual BRANCH leaves the sum to the skip path
    and would show nothing."""
    sd = {k: v.clone() for k, v in sd.items()}
    q = f"blocks.{level}."
    for name, bias in ((q + "3.weight", q + "3.bias"), (q + "2.fn.fn.to_qkv.weight", None),
                       (q + "2.fn.fn.to_out.0.weight", q + "2.fn.fn.to_out.0.bias")):
        w = sd[name]
        rs, cs = W.row_scale(w.shape[0], pattern), W.col_scale(w.shape[1], pattern)
        sd[name] = w * rs.view(-1, 1, 1) * cs.view(1, -1, 1)
        if bias is not None:
            sd[bias] = sd[bias] * rs
    return sd


def _engine_case(family, base_sd, kw, x, z, t, kind):
    from oracle import torch_ref as R
    from graspldm_amd.r1d import R1dEngine, pack_resnet1d

    def fits(k):
        d = pack_resnet1d(_engine_sd(base_sd, ("whole", k)), "", **kw)["desc"]
        return d.lv[1].down_w3 != 0

    pattern, want = _pattern(kind, W.k_inside(fits))
    sd = _engine_sd(base_sd, pattern)
    packed = pack_resnet1d(sd, "", **kw)
    d = packed["desc"]
    split = d.lv[1].down_w3 != 0
    assert all((lv.down_w3 != 0) == split for lv in list(d.lv)[1:d.n_levels])
    exp = R.resnet1d_forward({k: v.double() for k, v in sd.items()}, "", x.double(), z_cond=z.double(), time=t,
                             temb=packed["temb"][t].double())
    eng = R1dEngine(packed, "cuda:0")
    got = eng.denoise(x.cuda(), eng.cond_embed(z.cuda()), 1, sample_t=t.int().cuda())
    assert torch.isfinite(got).all() and eng.workspace_errors() == 0
    _judge(family, kw["seq_len"], kind, pattern, split, want, [W.rel(got, exp)], ENGINE_BAR)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("net", ["shipped4", "d16_quad_only"])
def test_r1d_engines(net, kind, fpc_state_dict):
    """The shipped 4-position denoiser and the 16-position row d16_quad_only of tests/r1d_envelope_cases.py (attention on
    every level).  An engine has one arithmetic per descriptor: where a matrix does not fit, pack_resnet1d names no split
    copy at all (the exact form of numerics.f32_only())."""
    import r1d_envelope_cases as C
    g = torch.Generator().manual_seed(5)
    n = 11
    if net == "shipped4":
        p = "diffusion_model.model."
        sd = {k[len(p):]: v for k, v in fpc_state_dict.items() if k.startswith(p)}
        kw, L = dict(groups=4, seq_len=4, num_steps=1000), 4
    else:
        sd = C.state_dict(net)
        kw, L = dict(groups=4, seq_len=16, num_steps=1000, cond_rows=3), 16
    x, z = torch.randn(n, 1, L, generator=g), torch.randn(n, 3, 64, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    _engine_case("r1d_" + net, sd, kw, x, z, t, kind)


# ------------------------------------------------------------------------------------------------------------------ Unet1D
@pytest.mark.parametrize("kind", KINDS)
def test_unet1d(kind):
    """Case A of tests/unet1d_ref.py with the pattern on one down-path conv (downs.1.3); 2^-12 is the `k12` case.  The kernel
    has one arithmetic per descriptor: where the conv does not fit, the whole network is packed exact_f32."""
    import unet1d_ref as U
    from graspldm_amd.resnets import Unet1D
    from graspldm_amd.synthetic import load_synthetic_weights
    from graspldm_amd.unet1d_pack import pack_unet1d
    c = U.CASES["A"]

    def build(pattern):
        net = load_synthetic_weights(Unet1D(**c["args"]), seed=c["seed"])
        conv = net.downs[1][3]
        rs, cs = W.row_scale(conv.weight.shape[0], pattern), W.col_scale(conv.weight.shape[1], pattern)
        with torch.no_grad():
            conv.weight.mul_(rs.view(-1, 1, 1) * cs.view(1, -1, 1))
            conv.bias.mul_(rs)
        return net

    def fits(k):
        sd = {kk: v.detach() for kk, v in build(("whole", k)).state_dict().items()}
        return not pack_unet1d(sd, "", 4, c["L"], cond_rows=3)["desc"].exact_f32

    pattern, want = _pattern(kind, W.k_inside(fits))
    net = build(pattern)
    x, z, _ = U.case_inputs("A", 20)
    sd64 = {k: v.detach().double() for k, v in net.state_dict().items()}
    ref = U.unet1d_forward(sd64, "", x.double(), z.double(), None, groups=4)
    net = net.cuda()
    out = net(x.cuda(), time=None, z_cond=z.cuda()).cpu()
    split = not net.engine(torch.device("cuda", torch.cuda.current_device())).plan(c["L"])["desc"].exact_f32
    assert torch.isfinite(out).all()
    _judge("unet1d", "A", kind, pattern, split, want, [W.rel(out, ref)])
