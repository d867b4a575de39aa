"""GPU (MI355X): every corner of the encoders' shape envelope that the library accepts, run and compared.

tests/test_envelope_cpu.py pins the planners of the three MFMA launch families from both sides of every bound on the host
and never launches an accepted shape; the other GPU tests start from the routing predicates (dense.split_supported,
voxel.split_conv_supported, sa_pack.split_plan_ok) and so only run what the policy routes.  This file runs the band between
the two: shapes the public C entries take (include/gldm.h) and the policy constants of dense.py / sa_pack.py / voxel.py keep
the routes away from.  Every case
  1. asks the library's query for the exact shape and form and asserts the answer (a planner narrowed later fails here),
  2. packs its weights with the project's own packers,
  3. calls the C entry (dense.pointwise_mlp is the bare call; the Python routes only with a policy constant patched),
  4. compares with a torch-CPU f64 reference of the same operation.
Bars: 2e-5 of the output scale for the pointwise and conv kernels, 2e-5 for set abstraction; centre coordinates, the
channel-last / point-major transposes and repeated head results bit for bit.
`test_every_accepted_row_of_the_cpu_tables_has_a_gpu_run` needs no device: a row the CPU tables mark accepted without a GPU
case here (or a named one elsewhere) fails it."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu

OK = 0
F32, F16X2 = 0, 1
BAR = 2e-5


def _err(a, b):
    return (a.detach().cpu() - b).abs().max().item()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _within_bar(got, ref64, what):
    """|got - ref| < 2e-5 of the output scale, the figure printed in front of the assertion."""
    e, bar = _err(got, ref64.float()), BAR * max(1.0, ref64.abs().max().item())
    print(f"{what}: err {e:.3e} bar {bar:.3e}")
    assert e < bar, (what, e, bar)


# ---------------------------------------------------------------- A. pointwise (csrc/pointwise_mlp.hip, plan_pointwise)

# (split, b, cin0, cin, cout, n, hout, form); form: "" | "pm" (point-major y) | "add" (addend, both stride forms)
PW_CASES = [
    # 16-point n-tiles.  K = 512: the 32-point plan, a half last tile (ntv = 1); b = 3 at n = 16: every tile ends its cloud
    (1, 3, 0, 512, 256, 16, 0, ""), (1, 2, 0, 512, 256, 48, 0, ""),
    # K = 640 / 768: the 48-point plan (nt = 3), last tile whole, 16 points, 32 points
    (1, 2, 0, 640, 256, 48, 0, ""), (1, 2, 0, 640, 256, 64, 0, ""), (1, 2, 0, 640, 256, 80, 0, ""),
    (1, 2, 0, 768, 256, 48, 0, ""), (1, 2, 0, 768, 256, 64, 0, ""), (1, 2, 0, 768, 256, 80, 0, ""),
    # K above dense.SPLIT_MAX_K, up to the launch's bound 1152 (planes of 147,456 bytes)
    (1, 2, 0, 896, 256, 32, 0, ""), (1, 1, 0, 896, 256, 64, 0, ""), (1, 2, 0, 896, 1536, 32, 0, ""), (1, 1, 0, 896, 1536, 64, 0, ""),
    (1, 2, 0, 1024, 256, 32, 0, ""), (1, 1, 0, 1024, 256, 64, 0, ""), (1, 2, 0, 1024, 1536, 32, 0, ""), (1, 1, 0, 1024, 1536, 64, 0, ""),
    (1, 2, 0, 1152, 256, 32, 0, ""), (1, 1, 0, 1152, 256, 64, 0, ""), (1, 2, 0, 1152, 1536, 32, 0, ""), (1, 1, 0, 1152, 1536, 64, 0, ""),
    # ... with a head: one row (40 drawn units have their slot behind the planes), 16 rows (no slot fits: dyn_first = units)
    (1, 1, 0, 1152, 1536, 64, 1, ""), (1, 1, 0, 1152, 1536, 64, 16, ""), (1, 2, 0, 768, 1536, 32, 7, ""),
    # narrow inputs, multiples of 8 that are none of 32: K zero-padded to 128 by dense.split_fragments
    (1, 2, 0, 8, 64, 32, 0, ""), (1, 2, 0, 24, 64, 32, 0, ""), (1, 2, 0, 40, 64, 32, 0, ""), (1, 1, 0, 40, 96, 80, 0, ""),
    # units of output rows: one m-tile (fewer units than waves); two from 256 rows up; two where the planes pass half the LDS
    (1, 2, 0, 128, 16, 64, 0, ""), (1, 2, 0, 128, 48, 64, 0, ""), (1, 2, 0, 512, 240, 32, 0, ""), (1, 2, 0, 512, 288, 32, 0, ""),
    (1, 2, 0, 640, 224, 32, 0, ""), (1, 1, 0, 640, 224, 80, 0, ""),
    # a front layer: the policy's widest K (the table rows), then beyond it
    (1, 2, 96, 768, 1536, 32, 0, ""), (1, 2, 96, 768, 1280, 32, 0, ""), (1, 2, 96, 1024, 256, 80, 0, ""),
    (1, 2, 32, 1024, 1280, 80, 0, ""), (1, 1, 96, 1024, 256, 32, 0, ""),
    # the point-major and addend entries: the table rows, and K over the cap at a ragged point count
    (1, 2, 0, 128, 128, 32, 0, "pm"), (1, 2, 0, 128, 128, 32, 0, "add"), (1, 2, 0, 1024, 256, 48, 0, "pm"), (1, 2, 0, 1024, 256, 48, 0, "add"),
    # f32 form: K at its bound, the front tile at its bound, a 16-row head, and the table rows
    (0, 2, 0, 1152, 256, 32, 0, ""), (0, 2, 384, 768, 256, 32, 0, ""), (0, 1, 0, 768, 1536, 32, 16, ""),
    (0, 2, 0, 128, 256, 32, 0, ""), (0, 1, 96, 768, 1536, 32, 7, ""),
]


def _pw_key(case):
    split, _, cin0, cin, cout, n, hout, form = case
    return (split, cin0, cin, cout, n, hout, int(form == "add"), int(form == "pm"))


@gpu
@pytest.mark.parametrize("case", PW_CASES, ids=lambda c: "-".join(str(v) for v in c if v != ""))
def test_pointwise_accepted_shapes(case):
    """gldm_pointwise_mlp[2][_f16x2][_pm | _add] at shapes launch_pointwise plans and dense.py's policy does not route (16-point
    last tiles, K over SPLIT_MAX_K up to 1152, K padded from 8 / 24 / 40 rows, one-m-tile units, a front layer over K = 1024)
    against relu(W1 relu(W0 x + b0) + b1 [+ addend]) and the head Wh y + bh in f64.  The fused front layer is also compared
    with the same two layers as two launches; the head is bitwise repeatable whoever draws which unit of output rows."""
    _need_gpu()
    from graspldm_amd import _lib as L
    from graspldm_amd import dense
    from graspldm_amd.r1d_pack import mfma_a_fragments, mfma_a_fragments_f16x2
    split, b, cin0, cin, cout, n, hout, form = case
    assert L.lib().gldm_pointwise_mlp_supported(*_pw_key(case)) == OK
    g = torch.Generator().manual_seed(11 + cin0 + cin + cout + n + hout)
    frags = mfma_a_fragments_f16x2 if split else mfma_a_fragments
    x = torch.randn(b, cin0 if cin0 else cin, n, generator=g)
    w1, b1 = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    relu = form != "pm"
    front, h_ref = None, x.double()
    if cin0:
        w0, b0 = torch.randn(cin, cin0, generator=g) / cin0 ** 0.5, torch.randn(cin, generator=g)
        h_ref = (torch.einsum("oc,bcn->bon", w0.double(), h_ref) + b0.double().view(1, -1, 1)).relu().float().double()
        front = (frags(w0).cuda(), b0.cuda(), cin) + ((dense.range_gain(w0, b0),) if split else ())
    pre_ref = torch.einsum("oc,bcn->bon", w1.double(), h_ref) + b1.double().view(1, -1, 1)
    act = (lambda t: t.relu()) if relu else (lambda t: t)
    y_ref = act(pre_ref)
    head = None
    if hout:
        wh, bh = torch.randn(hout, cout, generator=g) / cout ** 0.5, torch.randn(hout, generator=g)
        z_ref = torch.einsum("oc,bcn->bon", wh.double(), y_ref) + bh.double().view(1, -1, 1)
        head = (dense.pack_head(wh).cuda(), bh.cuda(), hout)
    w1p = (dense.split_fragments(w1) if split and not cin0 else frags(w1)).cuda()   # (K padded where cin % 128 != 0)
    dx, db1 = x.cuda(), b1.cuda()
    y, z = dense.pointwise_mlp(dx, w1p, db1, cout, relu, head=head, keep_y=True, front=front, split=bool(split))
    _within_bar(y, y_ref, "y")
    if hout:
        _within_bar(z, z_ref, "z")
        for _ in range(3):   # the head sum does not depend on which wave drew which unit of output rows
            _, z2 = dense.pointwise_mlp(dx, w1p, db1, cout, relu, head=head, keep_y=False, front=front, split=bool(split))
            assert torch.equal(z2, z)
    if cin0 and split:
        # the same two layers as two split launches (the second one over the policy's K as well)
        h = dense.pointwise_mlp(dx, dense.split_fragments(w0).cuda(), front[1], cin, True, split=True)[0]
        y2 = dense.pointwise_mlp(h, w1p, db1, cout, True, split=True)[0]
        _within_bar(y2, y_ref, "y, two launches")
        _within_bar(y, y2.double().cpu(), "y, one launch against two")
    st = L.current_stream(dx.device)
    if form == "pm":
        ypm = torch.empty(b, n, cout, device="cuda")
        L.call("gldm_pointwise_mlp_f16x2_pm", L.ptr(dx), L.ptr(w1p), L.ptr(db1), b, cin, cout, n, int(relu), L.ptr(ypm), st)
        assert torch.equal(ypm.transpose(1, 2), y)   # the channel-major result transposed, bit for bit
    if form == "add":
        # a [b, cout, n] tensor (strides cout n, n, 1) and a per-cloud bias [b, cout] (strides cout, 1, 0)
        for add, strides in ((torch.randn(b, cout, n, generator=g), (cout * n, n, 1)), (torch.randn(b, cout, generator=g), (cout, 1, 0))):
            ya, da = torch.empty(b, cout, n, device="cuda"), add.cuda()
            L.call("gldm_pointwise_mlp_f16x2_add", L.ptr(dx), L.ptr(w1p), L.ptr(db1), L.ptr(da), *strides, b, cin, cout, n, int(relu),
                   L.ptr(ya), st)
            _within_bar(ya, act(pre_ref + add.double().reshape(b, cout, -1)), f"y + addend, strides {strides}")


# ---------------------------------------------------------------- B. voxel conv (csrc/conv3d.hip)

# f32 (gldm_conv3d_k3): a guarded last m-tile (three m-tiles at 32^3 with one and with four k-steps per tap); the two-launch
# halves, whole and with a guarded second half; one launch of 8 m-tiles
CONV_F32_CASES = [(48, 40, 24), (1, 40, 24), (16, 17, 16), (32, 120, 8), (5, 33, 32), (5, 48, 32), (3, 40, 32),
                  (32, 256, 8), (128, 256, 8), (64, 128, 16), (32, 64, 32), (32, 250, 8), (16, 120, 16), (8, 60, 32), (64, 128, 8)]
CONV_CL_CASES = [(5, 40, 24), (5, 44, 24), (5, 36, 32)]                     # gldm_conv3d_k3_cl: cout % 4 == 0, no multiple of 16
CONV_SPLIT_CASES = [(16, 256, 8, ""), (16, 128, 4, ""), (16, 32, 32, "gn")]   # "gn": in_coef set, channel-last output


def _groups(c):
    """A group count that divides c (GroupNorm over an odd channel count): the largest one up to 17."""
    return max(g for g in range(1, 18) if c % g == 0)


def _conv_case(cin, cout, r, seed):
    g = torch.Generator().manual_seed(seed + cin * 100 + cout + r)
    b = 2 if r <= 8 else 1
    x = torch.randn(b, cin, r, r, r, generator=g)
    x[:, :, ::3] = 0   # empty voxels, like a real occupancy grid
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias, gamma, beta = (torch.randn(cout, generator=g) * 0.1 for _ in range(3))
    return g, b, x, w, bias, gamma + 1, beta


def _gn_swish64(t, groups, gamma, beta):
    import torch.nn.functional as F
    gn = F.group_norm(t, groups, gamma.double(), beta.double(), 1e-5)
    return gn * torch.sigmoid(gn)


def _check_partials(L, y, part, ref, gamma, beta, b, cout, r):
    """The conv's GroupNorm partials through gldm_groupnorm_swish (in place on y) against F.group_norm + Swish in f64."""
    groups = _groups(cout)
    dg, dbt = gamma.cuda(), beta.cuda()
    L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(part), L.ptr(dg), L.ptr(dbt), b, cout, r, groups, 1e-5, None, L.current_stream())
    _within_bar(y, _gn_swish64(ref, groups, gamma, beta), f"GroupNorm({groups}) + Swish")


@gpu
@pytest.mark.parametrize("cin,cout,r", CONV_F32_CASES)
def test_conv3d_f32_guarded_rows_and_halves(cin, cout, r):
    """gldm_conv3d_k3 where cout is no multiple of 16 (the guarded last m-tile voxel.CONV_ROW_TILE keeps the routes away from;
    partials sized by gldm_conv3d_partial_floats for the odd cout) and as two launches of half the m-tiles (whole, and with a
    guarded second half) against F.conv3d in f64, and its partials through gldm_groupnorm_swish."""
    _need_gpu()
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d
    assert L.lib().gldm_conv3d_k3_supported(F32, cin, cout, r) == OK
    _, b, x, w, bias, gamma, beta = _conv_case(cin, cout, r, 0)
    ref = F.conv3d(x.double(), w.double(), bias.double(), padding=1)
    nf = int(L.lib().gldm_conv3d_partial_floats(b, cout, r))
    assert nf == b * (r // 4) ** 2 * cout * 2
    y, part = torch.empty(b, cout, r, r, r, device="cuda"), torch.full((nf,), float("nan"), device="cuda")
    dx, dw, db = x.cuda(), pack_conv3d(w).cuda(), bias.cuda()
    L.call("gldm_conv3d_k3", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(y), L.ptr(part), L.current_stream())
    _within_bar(y, ref, "conv")
    assert torch.isfinite(part).all()   # every (brick, channel) pair of the odd cout was written
    _check_partials(L, y, part, ref, gamma, beta, b, cout, r)


@gpu
@pytest.mark.parametrize("cin,cout,r", CONV_CL_CASES)
def test_conv3d_channel_last_with_a_guarded_tile(cin, cout, r):
    """gldm_conv3d_k3_cl at cout % 4 == 0 that is no multiple of 16: the channel-last output is the channel-major one
    transposed, bit for bit, and so are the partials (test_channel_last_voxel_stack_tail asserts it for whole tiles)."""
    _need_gpu()
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d
    assert L.lib().gldm_conv3d_k3_supported(F32, cin, cout, r) == OK and cout % 4 == 0 and cout % 16
    _, b, x, w, bias, _, _ = _conv_case(cin, cout, r, 1)
    nf = int(L.lib().gldm_conv3d_partial_floats(b, cout, r))
    y, ycl = torch.empty(b, cout, r ** 3, device="cuda"), torch.empty(b, r ** 3, cout, device="cuda")
    p, pcl = torch.empty(nf, device="cuda"), torch.empty(nf, device="cuda")
    dx, dw, db = x.cuda(), pack_conv3d(w).cuda(), bias.cuda()
    st = L.current_stream()
    L.call("gldm_conv3d_k3", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(y), L.ptr(p), st)
    L.call("gldm_conv3d_k3_cl", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(ycl), L.ptr(pcl), st)
    assert torch.equal(ycl.permute(0, 2, 1), y) and torch.equal(pcl, p)
    _within_bar(y.view(b, cout, r, r, r), F.conv3d(x.double(), w.double(), bias.double(), padding=1), "conv")


@gpu
@pytest.mark.parametrize("cin,cout,r,form", CONV_SPLIT_CASES)
def test_conv3d_split_f16_accepted_shapes(cin, cout, r, form):
    """The accepted (cin, cout, r) test_conv3d_split_f16_kernels leaves out: gldm_conv3d_k3_f16x2, and gldm_conv3d_k3_f16x2_gn
    with in_coef set (swish(a x + s) applied while the bricks are staged) writing channel-last, against F.conv3d in f64."""
    _need_gpu()
    import torch.nn.functional as F
    from graspldm_amd import _lib as L
    from graspldm_amd.voxel import pack_conv3d_f16x2
    assert L.lib().gldm_conv3d_k3_supported(F16X2, cin, cout, r) == OK
    g, b, x, w, bias, gamma, beta = _conv_case(cin, cout, r, 2)
    nf = int(L.lib().gldm_conv3d_partial_floats(b, cout, r))
    y, part = torch.empty(b, cout, r, r, r, device="cuda"), torch.empty(nf, device="cuda")
    dx, dw, db = x.cuda(), pack_conv3d_f16x2(w).cuda(), bias.cuda()
    st = L.current_stream()
    xin = x.double()
    if form == "gn":
        coef = torch.stack([1 + 0.1 * torch.randn(b, cin, generator=g), 0.1 * torch.randn(b, cin, generator=g)], dim=2).contiguous()
        t = coef[:, :, 0].double().view(b, cin, 1, 1, 1) * xin + coef[:, :, 1].double().view(b, cin, 1, 1, 1)
        xin = t * torch.sigmoid(t)
        ycl, dc = torch.empty(b, r ** 3, cout, device="cuda"), coef.cuda()
        L.call("gldm_conv3d_k3_f16x2_gn", L.ptr(dx), L.ptr(dc), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(ycl), L.ptr(part), 1, st)
        y = ycl.permute(0, 2, 1).reshape(b, cout, r, r, r).contiguous()
    else:
        L.call("gldm_conv3d_k3_f16x2", L.ptr(dx), L.ptr(dw), L.ptr(db), b, cin, cout, r, L.ptr(y), L.ptr(part), st)
    ref = F.conv3d(xin, w.double(), bias.double(), padding=1)
    _within_bar(y, ref, "conv")
    _check_partials(L, y, part, ref, gamma, beta, b, cout, r)


# ---------------------------------------------------------------- C. set abstraction (csrc/sa_mlp.hip, plan_sa3, plan_sa_f32)

# (form, b, c, n, m, u, widths[, rows of the f32 table's first layer]); form: the entry called
#   "split"  gldm_sa_mlp_forward_f16x2       "pre"  gldm_sa_mlp_forward_f16x2_pre (first layer per point)
#   "f32"    gldm_sa_mlp_forward
SA_CASES = [
    # the two plans split_plan_ok's PLANNED_PLANES refuses: 13 plane blocks + a 256-row output, 114,752 bytes
    ("split", 2, 256, 200, 20, 16, (128, 256)), ("split", 2, 256, 200, 10, 32, (128, 128, 256)),
    # a last layer that is no multiple of 32 rows
    ("split", 2, 5, 150, 37, 64, (128, 48)), ("split", 2, 5, 150, 37, 32, (64, 112)),
    # 3 + c = 32 gathered rows exactly
    ("split", 2, 29, 128, 9, 64, (64,)), ("split", 2, 29, 128, 9, 32, (64, 128)),
    # K blocks of the gather: 6, 8 (c = 253) and 9 (c = 285)
    ("split", 1, 189, 128, 7, 64, (64,)), ("split", 1, 253, 128, 7, 64, (64,)), ("split", 1, 285, 128, 7, 64, (128,)),
    # one 16-row layer, at both ends of U
    ("split", 2, 5, 128, 9, 64, (16,)), ("split", 2, 5, 128, 9, 16, (16,)),
    # the widest plans: 16 plane blocks + 1008 pooled rows (163,392 of 163,840 bytes), 12 blocks + 1024 rows
    ("split", 1, 253, 128, 5, 64, (256, 1008)), ("split", 1, 125, 128, 5, 64, (256, 1024)),
    # four layers
    ("split", 2, 5, 300, 40, 64, (32, 32, 32, 32)),
    # the hoisted form: wide pooled rows (msg_route's MSG_MAX_POOLED_ROWS), one layer behind the hoisted one
    ("pre", 1, 3, 128, 8, 64, (256, 256, 1008)), ("pre", 1, 3, 128, 8, 64, (256, 512)), ("pre", 1, 3, 128, 8, 64, (256, 128)),
    # four layers behind a hoisted first one (MSG_MAX_LAYERS): single-tile kernel, and the two-tile one (1050 tiles)
    ("pre", 2, 3, 300, 40, 64, (32, 32, 32, 32, 32)), ("pre", 3, 3, 400, 350, 64, (32, 32, 32, 32, 32)),
    # f32, the 64-column kernel: 1 .. 8 neighbours
    ("f32", 2, 3, 128, 37, 1, (32, 64)), ("f32", 2, 3, 128, 37, 2, (32, 64)), ("f32", 2, 3, 128, 37, 4, (32, 64)),
    ("f32", 2, 3, 128, 37, 8, (32, 64)), ("f32", 2, 5, 128, 37, 1, (16,)), ("f32", 2, 5, 128, 37, 8, (16,)),
    # f32: a hidden width of 192 (12 m-tiles), a 16-row last layer (one m-tile), 48 gathered rows, 253 features -> 256 rows
    ("f32", 2, 3, 128, 9, 64, (192, 64)), ("f32", 2, 5, 128, 9, 64, (16,)), ("f32", 2, 40, 128, 9, 64, (64,), 48),
    ("f32", 1, 253, 128, 7, 64, (256,)), ("f32", 2, 29, 128, 9, 64, (64,)), ("f32", 2, 5, 300, 40, 64, (32, 32, 32, 32)),
]


def _pad(c, to):
    return (c + to - 1) // to * to


def _sa_key(case):
    """(form, c, u, cin_pad, cout) as the launch's tables hold them (what sa_pack's packers make of the widths); the GPU test
    asserts that the packed tables say the same, so the coverage test below reads the planner's own arguments."""
    from graspldm_amd import sa_pack
    form, _, c, _, _, u, chans = case[:7]
    if form == "f32":
        couts = [sa_pack._f32_width(w) for w in chans[:-1]] + [chans[-1]]
        k0 = case[7] if len(case) > 7 else _pad(3 + c, 32)
        return (form, c, u, tuple([k0] + [_pad(w, 16) for w in couts[:-1]]), tuple(couts))
    layers = chans[1:] if form == "pre" else chans
    couts = [sa_pack._plane_width(w) for w in layers[:-1]] + [layers[-1]]
    k0 = _pad(chans[0], 32) if form == "pre" else _pad(3 + c, 32)
    return (form, 0 if form == "pre" else c, u, tuple([k0] + couts[:-1]), tuple(couts))


def _f32_table(folded, device, kpad0):
    """sa_pack.pack_f32_table with the first layer's K padded to `kpad0` rows (the packer pads to 32; the launch takes 16)."""
    from graspldm_amd import sa_pack
    from graspldm_amd.r1d_pack import _Buf, mfma_a_fragments
    buf = _Buf()
    cin_pad, cout, w_off, b_off = [], [], [], []
    for i, (w, b) in enumerate(folded):
        kpad = kpad0 if i == 0 else _pad(cout[-1], 16)
        rows = w.shape[0] if i == len(folded) - 1 else sa_pack._f32_width(w.shape[0])
        wp, bp = torch.zeros(rows, kpad), torch.zeros(rows)
        wp[: w.shape[0], : w.shape[1]] = w.cpu()
        bp[: w.shape[0]] = b.cpu()
        cin_pad.append(kpad)
        cout.append(rows)
        w_off.append(buf.add(mfma_a_fragments(wp)))
        b_off.append(buf.add(bp))
    return sa_pack._table(buf, device, cin_pad, cout, w_off, b_off)


class _SaSetup:
    """One set-abstraction module on seeded inputs: the module's weights, the cloud on the device with the library's own
    centres and ball query, and the f64 reference -- oracle.torch_ref.sa_module's steps (farthest points, ball query, grouping
    with the centre subtracted in f32 as the kernels do) with the SharedMLP and the max in f64 on the same weights."""

    def __init__(self, b, c, n, m, u, chans, radius=0.35):
        from graspldm_amd.pvcnn import PointNetSAModule, ball_query, furthest_point_sample
        from graspldm_amd.sa_pack import SaMlpPlan
        from graspldm_amd.synthetic import load_synthetic_weights
        from oracle import torch_ref as R
        mod = PointNetSAModule(num_centers=m, radius=radius, num_neighbors=u, in_channels=c, out_channels=chans).eval()
        load_synthetic_weights(mod, seed=11)
        g = torch.Generator().manual_seed(2 + c + n + m + u + len(chans))
        coords = (torch.rand(b, 3, n, generator=g) * 2 - 1).contiguous()
        feats = torch.randn(b, c, n, generator=g) if c else None
        ectr = R.furthest_point_sample(coords, m)
        grouped = R.ball_group(coords, ectr, feats, radius, u)
        sd = {k: v.detach().double() for k, v in mod.mlps[0].state_dict().items()}
        self.ref = R.shared_mlp(sd, "", grouped.double()).max(dim=-1).values
        self.b, self.c, self.n, self.m, self.u, self.rows = b, c, n, m, u, chans[-1]
        self.points = coords.cuda()
        self.feats = feats.cuda() if c else None
        self.centers = furthest_point_sample(self.points, m).contiguous()
        assert torch.equal(self.centers.cpu(), ectr)
        self.idx = ball_query(self.centers, self.points, radius, u)
        self.plan = SaMlpPlan(mod.mlps[0], self.points.device)

    def out(self):
        return torch.full((self.b, self.rows, self.m), float("nan"), device="cuda")


def _i32(a):
    return ctypes.cast(a, ctypes.c_void_p)


@gpu
@pytest.mark.parametrize("case", SA_CASES, ids=lambda c: "-".join(str(v) for v in c).replace(" ", ""))
def test_sa_mlp_accepted_plans(case):
    """gldm_sa_mlp_forward_f16x2 / _f16x2_pre / gldm_sa_mlp_forward called on the tables sa_pack packs, at the layer plans
    plan_sa3 / plan_sa_f32 accept and sa_pack's policy (PLANNED_PLANES, MSG_MAX_POOLED_ROWS, MSG_MAX_LAYERS) or the packers'
    padding keep the routes away from, against the module in f64 (_SaSetup): 2e-5."""
    _need_gpu()
    from graspldm_amd import _lib as L
    form, b, c, n, m, u, chans = case[:7]
    s = _SaSetup(b, c, n, m, u, chans)
    st = L.current_stream(s.points.device)
    out = s.out()
    if form == "f32":
        table = s.plan.f32 if len(case) == 7 else _f32_table(s.plan._folded, s.points.device, case[7])
    else:
        pre = s.plan._pre_plan() if form == "pre" else None
        table = pre.table if pre else s.plan._split_plan()
    # the planner's answer for the tables this launch gets, and the coverage test's reading of them
    assert (form, 0 if form == "pre" else c, u, tuple(table.cin_pad), tuple(table.cout)) == _sa_key(case)
    nl = len(table.cout)
    if form == "f32":
        assert L.lib().gldm_sa_mlp_supported(c, u, nl, _i32(table.cin_pad), _i32(table.cout)) == OK
        L.call("gldm_sa_mlp_forward", L.ptr(s.points), L.ptr(s.centers), L.ptr(s.feats), L.ptr(s.idx), L.ptr(table.weights),
               b, c, n, m, u, *table.args(), L.ptr(out), st)
    elif form == "split":
        assert L.lib().gldm_sa_mlp_f16x2_lds_bytes(0, c, u, nl, _i32(table.cin_pad), _i32(table.cout), None) > 0
        L.call("gldm_sa_mlp_forward_f16x2", L.ptr(s.points), L.ptr(s.centers), L.ptr(s.feats), L.ptr(s.idx), L.ptr(table.weights),
               b, c, n, m, u, *table.args(), L.ptr(out), st)
    else:
        assert L.lib().gldm_sa_mlp_f16x2_lds_bytes(1, 0, u, nl, _i32(table.cin_pad), _i32(table.cout), None) > 0
        row = s.plan._first_layer_per_point(s.feats, pre)   # [B, N, c1p] = W1b f + b1, point-major
        L.call("gldm_sa_mlp_forward_f16x2_pre", L.ptr(s.points), L.ptr(s.centers), L.ptr(row), 0, L.ptr(s.idx),
               L.ptr(table.weights), pre.wa_off, b, n, m, u, *table.args(), L.ptr(out), st)
    e = _err(out, s.ref.float())
    print(f"sa {form}: err {e:.3e}")
    assert e < BAR, e


def _recorded_calls(monkeypatch):
    """Every entry _lib.call is asked for from here on, in order."""
    from graspldm_amd import _lib as L
    names, real = [], L.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", call)
    return names


@gpu
@pytest.mark.parametrize("b,c,n,m,u,chans", [(2, 256, 200, 20, 16, (128, 256)), (2, 256, 200, 10, 32, (128, 128, 256)),
                                             (3, 256, 3300, 350, 16, (128, 256))])
def test_sa_run_with_the_planning_figure_at_the_launch_s_own(b, c, n, m, u, chans, monkeypatch):
    """SaMlpPlan.run with sa_pack.PLANNED_PLANES at the launch's own two planes: [259] -> [128, 256] at U = 16 and
    [259] -> [128, 128, 256] at U = 32 then take gldm_sa_mlp_forward_f16x2 unhoisted (m u < 2 n) instead of the f32 launch.
    (3, ..., 350): 264 tiles on 256 persistent workgroups, one per CU at this plan's 114,752 bytes."""
    _need_gpu()
    from graspldm_amd import sa_pack
    assert m * u < 2 * n and not sa_pack.split_plan_ok([c + 3] + list(chans[:-1]), list(chans), u)
    monkeypatch.setattr(sa_pack, "PLANNED_PLANES", (1, 1))
    assert sa_pack.split_plan_ok([c + 3] + list(chans[:-1]), list(chans), u)
    s = _SaSetup(b, c, n, m, u, chans)
    names = _recorded_calls(monkeypatch)
    out = s.plan.run(s.points, s.centers, s.feats, s.idx)
    assert names == ["gldm_sa_mlp_forward_f16x2"]
    e = _err(out, s.ref.float())
    print(f"sa run: err {e:.3e}")
    assert e < BAR, e


@gpu
@pytest.mark.parametrize("const,value,chans", [("MSG_MAX_POOLED_ROWS", 1008, (256, 256, 1008)), ("MSG_MAX_POOLED_ROWS", 512, (256, 512)),
                                               ("MSG_MAX_LAYERS", 5, (32, 32, 32, 32, 32))])
def test_sa_run_msg_with_a_policy_constant_at_the_launch_s_bound(const, value, chans, monkeypatch):
    """SaMlpPlan.run_msg with MSG_MAX_POOLED_ROWS / MSG_MAX_LAYERS at what launch_sa3 takes: the branch then runs hoisted
    (gldm_sa_mlp_forward_f16x2_pre: 1008 and 512 pooled rows; four layers behind the hoisted one) and gldm_group_max_concat
    writes its rows behind another branch's in the module's output."""
    _need_gpu()
    from graspldm_amd import sa_pack
    b, c, n, m, u, c0 = 1, 3, 128, 8, 64, 16
    assert sa_pack.msg_route(3 + c, chans, u) is None
    monkeypatch.setattr(sa_pack, const, value)
    assert sa_pack.msg_route(3 + c, chans, u) == "pre"
    s = _SaSetup(b, c, n, m, u, chans)
    names = _recorded_calls(monkeypatch)
    out = torch.full((b, c0 + chans[-1], m), -7.0, device="cuda")
    s.plan.run_msg(s.points, s.centers, s.feats, s.idx, out, c0)
    assert "gldm_sa_mlp_forward_f16x2_pre" in names and names[-1] == "gldm_group_max_concat"
    assert (out[:, :c0] == -7.0).all()
    e = _err(out[:, c0:], s.ref.float())
    print(f"sa run_msg: err {e:.3e}")
    assert e < BAR, e


# ---------------------------------------------------------------- D. the CPU tables' accepted rows all have a GPU run

# Accepted rows of tests/test_envelope_cpu.py that an older GPU test runs at exactly that shape: row -> the test
COVERED_ELSEWHERE = {
    # conv (kind, cin, cout, r)
    (F32, 3, 48, 24): "test_models_gpu.py::test_conv3d_groupnorm_swish_kernels[3-48-24]",
    (F32, 48, 48, 24): "test_models_gpu.py::test_conv3d_groupnorm_swish_kernels[48-48-24]",
    (F16X2, 48, 48, 24): "test_models_gpu.py::test_conv3d_split_f16_kernels[48-48-24]",
    (F16X2, 3, 48, 24): "test_models_gpu.py::test_conv3d_split_f16_kernels[3-48-24]",
    (F16X2, 128, 128, 4): "test_models_gpu.py::test_conv3d_split_f16_kernels[128-128-4]",
}


def test_every_accepted_row_of_the_cpu_tables_has_a_gpu_run():
    """No device needed.  Every row POINTWISE / CONV / SA_SPLIT / SA_F32 of test_envelope_cpu.py mark accepted is the shape of
    a GPU case of this file, or stands in COVERED_ELSEWHERE with the test that runs it: a new accepted row without a GPU run
    fails here.  A set-abstraction row is covered by a case with the same form, U and layer tables and at least its feature
    rows (the row's c only bounds cin_pad[0] from below)."""
    import test_envelope_cpu as T
    import test_models_gpu
    for row, name in COVERED_ELSEWHERE.items():
        fn, _, case_id = name.split("::")[1].partition("[")
        marks = [m for m in getattr(test_models_gpu, fn).pytestmark if m.name == "parametrize"]
        assert name.startswith("test_models_gpu.py::") and case_id == "-".join(str(v) for v in row[1:]) + "]", name
        assert any(row[1:] in m.args[1] for m in marks), name   # the parametrisation still lists the shape
    missing = []
    pw = {_pw_key(c) for c in PW_CASES}
    missing += [("pointwise", shape) for shape, status in T.POINTWISE if status == OK and shape not in pw]
    conv = {(F32, *c) for c in CONV_F32_CASES + CONV_CL_CASES} | {(F16X2, *c[:3]) for c in CONV_SPLIT_CASES}
    missing += [("conv", shape) for shape, status in T.CONV if status == OK and shape not in conv and shape not in COVERED_ELSEWHERE]
    sa = [_sa_key(c) for c in SA_CASES]

    def covered(form, c, u, cin_pad, cout):
        return any(k[0] == form and k[1] >= c and k[2:] == (u, tuple(cin_pad), tuple(cout)) for k in sa)
    for (pre, c, u, cin_pad, cout), answer in T.SA_SPLIT:
        if answer >= 0 and not covered("pre" if pre else "split", c, u, cin_pad, cout):
            missing.append(("sa split", (pre, c, u, cin_pad, cout)))
    for (c, u, cin_pad, cout), status in T.SA_F32:
        if status == OK and not covered("f32", c, u, cin_pad, cout):
            missing.append(("sa f32", (c, u, cin_pad, cout)))
    assert not missing, missing
