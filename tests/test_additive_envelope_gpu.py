"""GPU (MI355X): every accepted corner of the kernel families added behind the encoders and the 1-D engines -- gldm_cls_head,
gldm_point_attention_fused, gldm_point_attention, gldm_pointwise_rows / _small, gldm_linear_rows, gldm_groupnorm_affine,
gldm_groupnorm_swish_points[_sum], gldm_grasp_clearance / _contact_normals, gldm_select_grasps -- launched through the C ABI
at the rows of tests/additive_envelope_cases.py and compared with an f64 torch-CPU restatement of the same formula; the rows
just outside each envelope return their documented status and launch nothing.  tests/test_additive_envelope_cpu.py pins the
bounds and the completeness of the tables without a device.

Bars are the families' own, from the tests whose helpers are imported here:
  head, attention cores, gldm_linear_rows   max(2e-5 max(1, scale), 4 e32), e32 = the same formula evaluated by torch on the
                                            CPU in f32 against f64 (relative form for scaled operands); both terms printed
  gldm_pointwise_rows                       2e-5 max(1, scale)
  gldm_pointwise_small                      2e-6 (1 + scale)
  gldm_groupnorm_affine                     one f32 ulp of the f64 value (x = fma(a, y, s) is one rounding)
  gldm_groupnorm_swish_points[_sum]         2e-5 of the output scale, 2e-5 on the mean, the two entries bitwise equal
  clearance                                 test_grasp_select_gpu._bar; contacts and selections exact under f64 preconditions
Every case prints `family shape form kind: err .. tol .. ratio ..`; the worst ratios measured on an MI355X are in DESIGN.md
4.4 to 4.6 and 4.9.

The first run of the tables found three cases of the exact-f32 forms over their bars -- attention core (1,1008,64) normal
1.3e-4 of 1.1e-4, (1,1024,64) normal 1.9e-4 of 1.2e-4, head (1,2048,512,64) x times 1e5 0.109 of 0.068 -- each a single f32
accumulator chain along a K of 1008 to 2048.  Both kernels now add partial sums of 128 channels: 2.3e-5,
3.0e-5 and 1.5e-3 on the same cases.  Everything else passed as it stood."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import additive_envelope_cases as C
from test_attention_gpu import attention_ref, make_qkv, run_core
from test_classifier_gpu import head_case, run_head
from test_voxel_attention_gpu import MEAN_F32, run_fused

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID_ARG, WORKSPACE = -3, -1, -4
FORMS = pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _form(exact):
    return "f32" if exact else "split"


def _report(family, shape, form, kind, err, tol, extra=""):
    print(f"{family} {shape} {form} {kind}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}{extra}")


# ------------------------------------------------------------------------------------------------------ A. gldm_cls_head
@FORMS
@pytest.mark.parametrize("shape", C.HEAD_CASES, ids=_id)
def test_head_envelope_against_f64(shape, exact):
    for kind in C.HEAD_KINDS:
        args = C.make_head(*shape, kind=kind)
        relative = kind.startswith("scale")
        err, tol, ref, logit, prob = head_case(args, exact, relative=relative)
        scale = ref.abs().max().item()
        first = 2e-5 * (scale if relative else max(1.0, scale))
        _report("cls_head", shape, _form(exact), kind, err, tol, f" ({'4 e32' if tol > first else '2e-5 term'} decides; e32 {'= ' + format(tol / 4, '.3e') if tol > first else '<= ' + format(first / 4, '.3e')})")
        assert err <= tol, (kind, err, tol)
        if kind == "negative":              # every pre-activation below zero: logit = lb + b2 sum(l) exactly
            c0 = args[5] + args[6] * float(args[4].double().sum())
            assert (logit.cpu().double() - c0).abs().max() <= 1e-6 * max(1.0, abs(c0)), (logit, c0)
        elif kind == "first_rows":          # later passes add exactly nothing: the rows = 16 head of rows 0 to 15
            small, _ = run_head(*C.first_rows_head(args), exact)
            d = (logit.double() - small.double()).abs().max().item()
            print(f"cls_head {shape} {_form(exact)} first_rows: |logit - 16-row head| {d:.3e}")
            assert d <= tol, (d, tol)
        want = torch.sigmoid(logit)         # prob = sigmoid(logit) to one ulp of torch's
        ulp = (torch.nextafter(want, torch.full_like(want, 2.0)) - want).abs()
        assert ((prob - want).abs() <= ulp).all(), (prob, want)
        again, pagain = run_head(*args, exact)
        assert torch.equal(again, logit) and torch.equal(pagain, prob)      # bitwise repeatable


@FORMS
def test_head_envelope_scene_bits_do_not_depend_on_the_batch(exact):
    args = C.make_head(*C.HEAD_BATCH_CASE, seed=3)
    full, pfull = run_head(*args, exact)
    one, pone = run_head(args[0][1:2].contiguous(), *args[1:], exact)
    assert torch.equal(one, full[1:2]) and torch.equal(pone, pfull[1:2])


def test_head_module_with_a_wider_classifier(monkeypatch):
    """PointsBasedGraspClassifier.head where classifier.0 has 256 rows (two passes of the kernel) against the layer launches
    the predicate's other side selects, at the bars of test_head_fallback_layers_agree_outside_the_kernel_limits."""
    from torch import nn

    from graspldm_amd import grasp_classifier as gc
    from graspldm_amd.pipeline import build_model_from_cfg, classifier_model_config
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.synthetic import load_synthetic_weights
    rows = C.HEAD_MODULE_ROWS
    model = build_model_from_cfg(classifier_model_config(64, 12))           # build_classifier(64, 12), one width changed
    width = model.base_network.out_channels
    model.classifier = nn.Sequential(SharedMLP(width, rows), nn.Dropout(0.5), nn.Conv1d(rows, 1, 1),
                                     nn.Linear(model.num_pc_points, 1))
    load_synthetic_weights(model, seed=0)
    model = model.eval().cuda()
    assert model._head_layers()[0].weight.shape[0] == rows and gc.cls_head_supported(width, rows, 76)
    x = torch.randn(3, width, 76, generator=torch.Generator().manual_seed(5)).cuda()
    logit, prob = model.head(x)
    monkeypatch.setattr(gc, "cls_head_supported", lambda c, rows, n: False)
    l2, p2 = model.head(x)
    assert l2.shape == logit.shape == (3,)
    err, tol = (l2 - logit).abs().max().item(), 2e-5 * max(1.0, float(logit.abs().max()))
    _report("cls_head module", (3, width, rows, 76), "default", "kernel against layers", err, tol)
    assert err <= tol
    assert (p2 - prob).abs().max() <= 1e-5


# --------------------------------------------------------------------------------------- B. gldm_point_attention_fused
def _attention_side_assertions(family, kind, shape, form, q, k, v, got):
    b, c, n = shape
    if kind == "dominant":                  # the result is the dominant key's v column
        col = torch.stack([v[i, :, j] for i, j in enumerate(C.dominant_keys(b, n))])[:, :, None].expand(b, c, n)
        assert (got - col).abs().max() <= 1e-6 * col.abs().max(), (got - col).abs().max()
    elif kind == "zero_q":                  # the result is the mean of v
        mean = v.double().mean(dim=-1, keepdim=True).expand(b, c, n)
        emean = (got.double() - mean).abs().max().item()
        bound = max(1e-6 * mean.abs().max().item(), MEAN_F32)
        print(f"{family} {shape} {form} zero_q: |out - mean v| {emean:.3e}, bound {bound:.3e}")
        assert emean <= bound, emean


@FORMS
@pytest.mark.parametrize("shape", C.FUSED_CASES, ids=_id)
def test_fused_core_envelope_against_f64(shape, exact):
    for kind in C.FUSED_KINDS:
        q, k, v, ref, e32 = C.attention_reference(kind, shape)      # the kind's promises are asserted there, in f64
        qc, kc = q.cuda(), k.cuda()
        got = run_fused(qc, kc, kc if v is k else v.cuda(), exact).cpu()
        assert torch.isfinite(got).all()
        err, tol = (got.double() - ref).abs().max().item(), C.attention_tolerance(ref, e32)
        _report("fused core", shape, _form(exact), kind, err, tol, f" (4 e32 {4 * e32:.3e})")
        assert err <= tol, (kind, err, tol)
        _attention_side_assertions("fused core", kind, shape, _form(exact), q, k, v, got)


@FORMS
@pytest.mark.parametrize("shape", C.FUSED_CASES, ids=_id)
def test_fused_core_envelope_against_the_materialised_core(shape, exact):
    """Both entries accept these shapes: within the sum of the two tolerances (each kernel is within its own of f64)."""
    q, k, v, ref, e32 = C.attention_reference("normal", shape)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    a, m = run_fused(qc, kc, vc, exact), run_core(qc, kc, vc, exact)
    diff, tol = (a - m).abs().max().item(), 2 * C.attention_tolerance(ref, e32)
    _report("fused against materialised", shape, _form(exact), "normal", diff, tol)
    assert diff <= tol
    b = run_fused(qc, kc, vc, exact)
    assert torch.equal(a, b)                                                    # bitwise repeatable


@FORMS
@pytest.mark.parametrize("what,scale", C.RANGE_SCALES)
def test_fused_core_envelope_operand_range(what, scale, exact):
    """test_fused_core_operand_range at an instantiation it does not reach (c = 112)."""
    b, c, n = shape = C.FUSED_RANGE_CASE
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
    err, tol = (got.double() - ref).abs().max().item(), C.attention_tolerance(ref, e32, relative=True)
    _report("fused range", shape, _form(exact), f"{what} x {scale:g}", err, tol, f" (4 e32 {4 * e32:.3e})")
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------ C. gldm_point_attention
CORE_ROWS = [(shape, exact, kinds) for shape, forms, kinds in C.CORE_CASES for exact in forms]


@pytest.mark.parametrize("shape,exact,kinds", CORE_ROWS, ids=[f"{_id(s)}-{_form(e)}" for s, e, _ in CORE_ROWS])
def test_core_envelope_against_f64(shape, exact, kinds):
    b, c, n = shape
    for kind in kinds:
        q, k, v, ref, e32 = C.attention_reference(kind, shape)
        qc, kc = q.cuda(), k.cuda()
        got = run_core(qc, kc, kc if v is k else v.cuda(), exact).cpu()
        assert torch.isfinite(got).all()
        err, tol = (got.double() - ref).abs().max().item(), C.attention_tolerance(ref, e32)
        _report("attention core", shape, _form(exact), kind, err, tol, f" (4 e32 {4 * e32:.3e})")
        assert err <= tol, (kind, err, tol)
        _attention_side_assertions("attention core", kind, shape, _form(exact), q, k, v, got)


@FORMS
def test_core_envelope_chunks_of_two_clouds_and_one(exact):
    """b = 3 where 256 MiB hold two clouds' blocks: the launch runs as chunks of 2 and 1 (nb < chunk grids, input, output
    and per-cloud workspace offsets).  Every cloud equals the same cloud launched alone, bit for bit, and all three are
    within the bar of f64."""
    from graspldm_amd import _lib as L
    b, c, n = shape = C.CORE_CHUNK_CASE
    h = L.lib()
    assert h.gldm_point_attention_workspace_bytes(b, c, n) == 2 * h.gldm_point_attention_workspace_bytes(1, c, n)
    q, k, v, ref, e32 = C.attention_reference("normal", shape, seed=9)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    full = run_core(qc, kc, vc, exact)
    for i in range(b):
        alone = run_core(qc[i:i + 1].contiguous(), kc[i:i + 1].contiguous(), vc[i:i + 1].contiguous(), exact)
        assert torch.equal(alone[0], full[i]), i
    err, tol = (full.cpu().double() - ref).abs().max().item(), C.attention_tolerance(ref, e32)
    _report("attention core", shape, _form(exact), "normal, chunks of 2 and 1", err, tol, f" (4 e32 {4 * e32:.3e})")
    assert err <= tol


# ------------------------------------------------------------------------------------- D. small dense kernels and norms
@pytest.mark.parametrize("shape", C.ROWS_CASES, ids=_id)
def test_pointwise_rows_every_row_count(shape):
    from graspldm_amd import _lib as L
    b, cin, hout, n = shape
    g = torch.Generator().manual_seed(8 + hout + cin)
    x, w, bias = torch.randn(b, cin, n, generator=g), torch.randn(hout, cin, generator=g) / cin ** 0.5, torch.randn(hout, generator=g)
    xc, wc = x.cuda(), w.cuda()
    for has_bias in (True, False):
        ref = torch.einsum("oc,bcn->bon", w.double(), x.double()) + (bias.double()[None, :, None] if has_bias else 0.0)
        y = torch.full((b * hout * n + 64,), 7.0, device="cuda")          # a guard behind the output
        L.call("gldm_pointwise_rows", L.ptr(xc), L.ptr(wc), L.ptr(bias.cuda() if has_bias else None), b, cin, hout, n, L.ptr(y),
               L.current_stream(xc.device))
        assert (y[b * hout * n:] == 7.0).all()
        out = y[:b * hout * n].view(b, hout, n)
        err, tol = (out.cpu().double() - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
        _report("pointwise_rows", shape, "f32", "bias" if has_bias else "no bias", err, tol)
        assert err <= tol, (shape, has_bias, err)


@pytest.mark.parametrize("cin", C.SMALL_CINS)
def test_pointwise_small_every_width(cin):
    from graspldm_amd import _lib as L
    b = C.SMALL_B
    worst = (0.0, None)
    for cout in C.SMALL_COUTS:
        for n in C.SMALL_NS:
            g = torch.Generator().manual_seed(cin + cout + n)
            x, w, bias = torch.randn(b, cin, n, generator=g), torch.randn(cout, cin, generator=g), torch.randn(cout, generator=g)
            xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
            lin = torch.einsum("oc,bcn->bon", w.double(), x.double())
            for relu in (True, False):
                for has_bias in (True, False):
                    exp = lin + bias.double().view(1, -1, 1) if has_bias else lin
                    exp = exp.clamp_min(0) if relu else exp
                    y = torch.full((b * cout * n + 64,), 7.0, device="cuda")          # a guard behind the output
                    L.call("gldm_pointwise_small", L.ptr(xd), L.ptr(wd), L.ptr(bd if has_bias else None), b, cin, cout, n, int(relu),
                           L.ptr(y), L.current_stream())
                    assert (y[b * cout * n:] == 7.0).all()
                    err = (y[:b * cout * n].view(b, cout, n).cpu().double() - exp).abs().max().item()
                    tol = 2e-6 * (1 + exp.abs().max().item())
                    kind = f"cout {cout} n {n} relu {int(relu)} bias {int(has_bias)}"
                    _report("pointwise_small", (b, cin, cout, n), "f32", kind, err, tol)
                    assert err < tol, (cin, kind, err, tol)
                    worst = max(worst, (err / tol, kind))
    print(f"pointwise_small cin {cin}: worst ratio {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("shape", C.LINEAR_CASES, ids=_id)
def test_linear_rows_at_the_bounds_of_n(shape):
    """n = 16384 is the accepted maximum: exactly 64 KiB of dynamic LDS."""
    from graspldm_amd import _lib as L
    rows, n, nout = shape
    g = torch.Generator().manual_seed(3 + n)
    x, w, bias = torch.randn(rows, n, generator=g), torch.randn(nout, n, generator=g) / n ** 0.5, torch.randn(nout, generator=g)
    ref = F.linear(x.double(), w.double(), bias.double())
    e32 = (F.linear(x, w, bias).double() - ref).abs().max().item()
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    y = torch.full((rows + 1, nout), 7.0, device="cuda")
    L.call("gldm_linear_rows", L.ptr(xd), L.ptr(wd), L.ptr(bd), rows, n, nout, L.ptr(y), L.current_stream())
    assert (y[rows] == 7.0).all()
    err, first = (y[:rows].cpu().double() - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
    tol = max(first, 4 * e32)
    _report("linear_rows", shape, "f32", "bias", err, tol, f" (2e-5 term {first:.3e}, 4 e32 {4 * e32:.3e})")
    assert err <= tol, (shape, err, tol)
    y2 = torch.empty(rows, nout, device="cuda")
    L.call("gldm_linear_rows", L.ptr(xd), L.ptr(wd), None, rows, n, nout, L.ptr(y2), L.current_stream())
    err = (y2.cpu().double() - (ref - bias.double())).abs().max().item()
    _report("linear_rows", shape, "f32", "no bias", err, tol)
    assert err <= tol, (shape, err, tol)


@pytest.mark.parametrize("shape", C.AFFINE_CASES, ids=_id)
def test_groupnorm_affine_from_given_coefficients(shape):
    """x = fma(a, y, s) from random (a, s) fed directly: within one f32 ulp of the f64 value at every element, in place and
    out of place, bitwise repeatable.  r = 24 and r = 26 stand either side of the grid switch (quads >= 4096)."""
    from graspldm_amd import _lib as L
    b, c, r = shape
    vox = r ** 3
    g = torch.Generator().manual_seed(12 + r)
    y, coef = torch.randn(b, c, vox, generator=g) * 2 + 1.0, torch.randn(b, c, 2, generator=g)
    ref = coef[..., :1].double() * y.double() + coef[..., 1:].double()
    yc, cc, st = y.cuda(), coef.cuda(), L.current_stream()
    out = torch.full((b * c * vox + 64,), 7.0, device="cuda")                     # a guard behind the output
    again, inplace = torch.empty(b, c, vox, device="cuda"), yc.clone()
    L.call("gldm_groupnorm_affine", L.ptr(yc), L.ptr(cc), b, c, r, L.ptr(out), st)
    L.call("gldm_groupnorm_affine", L.ptr(yc), L.ptr(cc), b, c, r, L.ptr(again), st)
    L.call("gldm_groupnorm_affine", L.ptr(inplace), L.ptr(cc), b, c, r, L.ptr(inplace), st)
    assert (out[b * c * vox:] == 7.0).all()
    got = out[:b * c * vox].view(b, c, vox)
    assert torch.equal(got, again) and torch.equal(got, inplace)
    got = got.cpu()
    ulp = torch.nextafter(got.abs(), torch.full_like(got, math.inf)) - got.abs()
    ratio = ((got.double() - ref).abs() / ulp.double()).max().item()
    print(f"groupnorm_affine {shape} f32 given coefficients: worst err / ulp {ratio:.3f}")
    assert ratio <= 1.0, (shape, ratio)


@pytest.mark.parametrize("shape", C.SWISH_CASES, ids=_id)
def test_groupnorm_swish_points_few_channels_per_group(shape):
    """The assertions of test_groupnorm_swish_points_with_the_squeeze_sums where c / groups is 1 or 3 (waves of the _sum
    kernel without a channel), at 128 channels per group with rows of a single quad, and at a ragged n."""
    from graspldm_amd import _lib as L
    b, c, n, groups = shape
    g = torch.Generator().manual_seed(4 + c + n)
    x, add = torch.randn(b, c, n, generator=g) * 3 + 20.0, torch.randn(b, c, n, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    for res in (True, False):
        y = F.group_norm((x + add if res else x).double(), groups, gamma.double(), beta.double(), 1e-5)
        ref = y * torch.sigmoid(y)
        xc, ac, gc, bc = x.cuda(), add.cuda() if res else None, gamma.cuda(), beta.cuda()
        st = L.current_stream(xc.device)
        outs = []
        for _ in range(2):
            out, cs = torch.empty(b, c, n, device="cuda"), torch.full((b * c + 16,), 7.0, device="cuda")
            L.call("gldm_groupnorm_swish_points_sum", L.ptr(xc), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(out),
                   L.ptr(cs), st)
            assert (cs[b * c:] == 7.0).all()
            outs.append((out, cs[:b * c].view(b, c)))
        (out, cs), (out2, cs2) = outs
        err, tol = (out.cpu().double() - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
        esum = (cs.cpu().double() / n - ref.mean(dim=-1)).abs().max().item()
        _report("groupnorm_swish_points_sum", shape, "f32", "residual" if res else "no residual", err, tol, f", mean err {esum:.3e}")
        assert err <= tol, (shape, err)
        assert esum <= 2e-5, (shape, esum)
        assert torch.equal(out, out2) and torch.equal(cs, cs2)
        plain, inplace = torch.empty(b, c, n, device="cuda"), xc.clone()
        L.call("gldm_groupnorm_swish_points", L.ptr(xc), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(plain), st)
        L.call("gldm_groupnorm_swish_points", L.ptr(inplace), L.ptr(ac), L.ptr(gc), L.ptr(bc), b, c, n, groups, 1e-5, L.ptr(inplace), st)
        assert torch.equal(out, plain) and torch.equal(out, inplace)


# ------------------------------------------------------------------------------------------------------------ E. selection
@pytest.mark.parametrize("sb,ss", C.CLEARANCE_SEGMENTS, ids=lambda v: str(v))
def test_clearance_and_contacts_with_eight_segments(sb, ss):
    import grasp_select_ref as ref
    import normals_ref
    import test_grasp_select_gpu as base
    from graspldm_amd.grasp_select import contact_normals, grasp_clearance
    b, g, ns = C.CLEARANCE_SHAPE
    scene, normals, H = C.clearance_inputs()
    body, sweep = C.segments(sb, ss)
    want, want_contacts, body_d, sweep_d = ref.clearance(scene, H, body, sweep, base.R_SWEEP, base.CAP)
    bar = base._bar(scene, H)
    # precondition (f64): no point within the bar of a tube's radius -- allowed count: zero
    assert int(((body_d - base.R_BODY).abs() <= bar[..., None]).sum()) == 0
    if sweep_d is not None:
        assert int(((sweep_d - base.R_SWEEP).abs() <= bar[..., None]).sum()) == 0
    kw = dict(body_segments=body, sweep_segments=sweep, sweep_radius=base.R_SWEEP, max_clearance=base.CAP)
    clear, contacts = grasp_clearance(scene.cuda(), H.cuda(), **kw)
    again = grasp_clearance(scene.cuda(), H.cuda(), **kw)
    assert clear.shape == (b, g) and contacts.shape == (b, g)
    assert torch.equal(clear, again[0]) and torch.equal(contacts, again[1])
    ratio = ((clear.cpu().double() - want).abs() / bar).max().item()
    print(f"clearance {(b, g, ns)} f32 sb {sb} ss {ss}: err / bar ratio {ratio:.3f}; capped {int((want == base.CAP).sum())} of {b * g}, "
          f"colliding {int((want <= base.R_BODY).sum())}, contacts {want_contacts.flatten().tolist()}")
    assert ratio <= 1.0, ratio
    assert torch.equal(contacts.cpu().long(), want_contacts)
    assert ((clear.cpu().double() > base.R_BODY) == (want > base.R_BODY)).all()
    # the same contact set split by finger and judged by the friction cone
    cos_f = math.cos(math.radians(30.0))
    side, aligned = contact_normals(scene.cuda(), normals.cuda(), H.cuda(), sweep_segments=sweep, sweep_radius=base.R_SWEEP,
                                    friction_angle_deg=30.0)
    assert torch.equal(side.sum(-1, dtype=torch.int32), contacts) and bool((aligned <= side).all())
    if ss:
        w = normals_ref.contact_normals(scene, normals, H, sweep, base.R_SWEEP, cos_f)
        assert int((((w["axis_dot"] - cos_f).abs() <= 1e-6) & w["nonzero"]).sum()) == 0          # preconditions (f64)
        assert int((w["hit"] & (w["qx"].abs() <= bar[..., None])).sum()) == 0
        print(f"contact normals {(b, g, ns)} ss {ss}: by side {w['side'].flatten().tolist()}, aligned {w['aligned'].flatten().tolist()}")
        assert torch.equal(side.cpu().long(), w["side"]) and torch.equal(aligned.cpu().long(), w["aligned"])
    else:
        assert int(side.sum()) == 0 and int(aligned.sum()) == 0


@pytest.mark.parametrize("case", C.SELECT_ENVELOPE_CASES, ids=_id)
def test_selection_with_the_most_control_points(case):
    """Both modes with gripper.control_points(64) (the bound of np), k = g above 256 and g = 2048: the diverse picks equal
    the f64 greedy's under its margin precondition, top-k equals a stable sort."""
    import grasp_select_ref as ref
    import test_grasp_select_gpu as base
    from graspldm_amd import gripper
    from graspldm_amd.grasp_select import select_grasps
    b, g, k, seed = case
    H, score, keep = base._selection_inputs(b, g, seed)
    ctrl = gripper.control_points(C.SELECT_CONTROL_POINTS)
    worst = 0.0
    for mask in (keep, None):
        dmask = None if mask is None else mask.cuda()
        index, count, gap = select_grasps(H.cuda(), score.cuda(), keep=dmask, k=k, diverse=True, control_points=ctrl)
        again = select_grasps(H.cuda(), score.cuda(), keep=dmask, k=k, diverse=True, control_points=ctrl)
        assert all(torch.equal(a, o) for a, o in zip(again, (index, count, gap)))
        assert index.shape == (b, k) and count.shape == (b,) and gap.shape == (b, k)
        for c in range(b):
            kept = [True] * g if mask is None else mask[c].tolist()
            want, n, gaps, margins = ref.diverse(H[c], score[c], kept, ctrl, k)
            assert min(margins, default=math.inf) >= 1e-4, ("precondition: pick another seed", c, min(margins))
            assert index[c].tolist() == want, (c, index[c].tolist(), want)
            assert int(count[c]) == n == min(k, sum(kept))
            got = gap[c].cpu().double()
            assert got[0] == math.inf and (got[n:] == 0).all()
            w = torch.tensor(gaps[1:n], dtype=torch.float64)
            rel = ((got[1:n] - w).abs() / w).max().item()
            worst = max(worst, rel)
            assert rel <= 1e-5, rel
    _report("select_grasps diverse", case, "f32", "gap, relative", worst, 1e-5)
    tied = score.clone()
    tied[:, g // 2] = tied[:, 0]                                      # an exact tie: the lower index goes first
    tied = (tied * 8).round() / 8 if g == 300 else tied              # and many ties
    for mask in (keep, None):
        index, count, gap = select_grasps(H.cuda(), tied.cuda(), keep=None if mask is None else mask.cuda(), k=k, control_points=ctrl)
        for c in range(b):
            kept = torch.ones(g, dtype=torch.bool) if mask is None else mask[c]
            ids = torch.nonzero(kept).flatten()
            order = ids[torch.sort(tied[c][kept], descending=True, stable=True).indices][:k].tolist()
            assert index[c].tolist() == order + [-1] * (k - len(order))
            assert index[c].tolist() == ref.topk(tied[c], kept.tolist(), k)[0]
            assert int(count[c]) == len(order)
        assert (gap == 0).all()


# ------------------------------------------------------------------------------------------------------------ rejected rows
def test_rejected_rows_return_their_status_and_launch_nothing():
    """Just outside each envelope: the documented status, and the output (filled with a sentinel) untouched after the
    device has drained.  Buffers have the size the rejected shape would need."""
    from graspldm_amd import _lib as L
    h, st = L.lib(), L.current_stream()
    sentinel = 7.0

    def fused(b, c, n):
        q, out = torch.empty(b, c, n, device="cuda"), torch.full((b, c, n), sentinel, device="cuda")
        status = h.gldm_point_attention_fused(L.ptr(q), L.ptr(q), L.ptr(q), b, c, n, 0, L.ptr(out), st)
        torch.cuda.synchronize()
        return status, bool((out == sentinel).all())
    for b, c, n in [(2, 16, 64), (2, 144, 64), (2, 32, 48), (1, 32, 4128), (65536, 32, 32)]:
        assert fused(b, c, n) == (UNSUPPORTED, True), (b, c, n)

    x = torch.randn(1, 64, 264, device="cuda")
    w = torch.randn(9, 64, device="cuda")
    y = torch.full((1, 9, 264), sentinel, device="cuda")
    assert h.gldm_pointwise_rows(L.ptr(x), L.ptr(w), None, 1, 64, 9, 260, L.ptr(y), st) == UNSUPPORTED
    assert h.gldm_pointwise_rows(ctypes.c_void_p(x.data_ptr() + 4), L.ptr(w), None, 1, 64, 1, 260, L.ptr(y), st) == INVALID_ARG
    assert h.gldm_pointwise_rows(L.ptr(x), L.ptr(w), None, 1, 64, 1, 258, L.ptr(y), st) == UNSUPPORTED           # n % 4

    xs, gam = torch.randn(2, 129, 8, device="cuda"), torch.ones(129, device="cuda")
    ys = torch.full((2, 129, 8), sentinel, device="cuda")
    cs = torch.full((2, 129), sentinel, device="cuda")
    assert h.gldm_groupnorm_swish_points(L.ptr(xs), None, L.ptr(gam), L.ptr(gam), 2, 129, 8, 1, 1e-5, L.ptr(ys), st) == UNSUPPORTED
    assert h.gldm_groupnorm_swish_points(L.ptr(xs), None, L.ptr(gam), L.ptr(gam), 2, 128, 6, 1, 1e-5, L.ptr(ys), st) == UNSUPPORTED
    assert h.gldm_groupnorm_swish_points_sum(L.ptr(xs), None, L.ptr(gam), L.ptr(gam), 2, 129, 8, 1, 1e-5, L.ptr(ys), L.ptr(cs),
                                             st) == UNSUPPORTED
    assert h.gldm_groupnorm_swish_points_sum(L.ptr(xs), None, L.ptr(gam), L.ptr(gam), 2, 128, 6, 1, 1e-5, L.ptr(ys), L.ptr(cs),
                                             st) == UNSUPPORTED

    ya, coef = torch.randn(65 ** 3 + 3, device="cuda"), torch.randn(1, 1, 2, device="cuda")
    xa = torch.full((65 ** 3 + 3,), sentinel, device="cuda")
    assert h.gldm_groupnorm_affine(L.ptr(ya), L.ptr(coef), 1, 1, 65, L.ptr(xa), st) == UNSUPPORTED
    assert h.gldm_groupnorm_affine(L.ptr(ya), L.ptr(coef), 1, 1, 3, L.ptr(xa), st) == UNSUPPORTED                # 27 voxels

    b, c, rows, n = 2, 64, 128, 70
    args = C.make_head(b, c, rows, n)
    from graspldm_amd.grasp_classifier import pack_head_weights
    pack = pack_head_weights(args[1], args[2], args[3], args[4], 0.0, "cuda")
    need = h.gldm_cls_head_workspace_bytes(b, c, rows, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    xh = args[0].cuda()
    logit, prob = torch.full((b,), sentinel, device="cuda"), torch.full((b,), sentinel, device="cuda")

    def head(nbytes):
        return h.gldm_cls_head(L.ptr(xh), L.ptr(pack.w1), L.ptr(pack.b1), L.ptr(pack.w2), L.ptr(pack.l), 0.0, b, c, rows, n,
                               int(pack.exact), L.ptr(ws), nbytes, L.ptr(logit), L.ptr(prob), st)
    assert head(need - 1) == WORKSPACE
    torch.cuda.synchronize()
    for t in (y, ys, cs, xa, logit, prob):
        assert (t == sentinel).all()
    assert head(need) == 0                                                        # the same call with the bytes it asked for
    torch.cuda.synchronize()
    assert torch.isfinite(logit).all() and not (logit == sentinel).any()
