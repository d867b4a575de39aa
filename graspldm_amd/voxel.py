"""Voxel branch of PVConv on the HIP path: Conv3d(k3) -> GroupNorm(8) -> Swish -> Conv3d(k3) ->
GroupNorm(8) -> Swish -> SE -> trilinear devoxelize (+ point branch), pvconv.py:47-84, as
gldm_conv3d_k3 / gldm_groupnorm_swish / gldm_se_gate / gldm_devoxelize_fused launches (`run`); with use_attention=True
the PVD Attention block over the voxels stands in place of the second Swish (pvconv.py:68-69; `run_attention`)."""
import torch

from . import _lib as L
from ._abi import CONSTANTS
from .r1d_pack import mfma_a_fragments

# Which (cin, cout, r) a conv kernel is instantiated for is the library's answer (gldm_conv3d_k3_supported reads the list
# the dispatch reads, csrc/conv3d.hip).  What stands next to it in a predicate below is routing policy.
_F32, _F16X2 = CONSTANTS["GLDM_CONV3D_F32"], CONSTANTS["GLDM_CONV3D_F16X2"]   # gldm_conv3d_kind
CONV_ROW_TILE = 16        # policy: whole 16-row m-tiles only (the f32 kernels guard a partial last tile: packed by pack_conv3d, run and compared, not timed: tests/test_envelope_gpu.py::test_conv3d_f32_guarded_rows_and_halves)
FIRST_VOXEL_CONV = (3, 48, 24)   # policy: the shipped encoder's first conv has an f32 form of its own under f32_only() (DESIGN_HISTORY.md, round 6)


def _instantiated(kind, cin, cout, r):
    return L.lib().gldm_conv3d_k3_supported(kind, int(cin), int(cout), int(r)) == 0


def conv_supported(cout, r):
    """Shapes launch_conv / launch_conv_halves have an f32-MFMA instantiation for (csrc/conv3d.hip; gldm_conv3d_k3[_cl]:
    any cin)."""
    return cout % CONV_ROW_TILE == 0 and _instantiated(_F32, 1, cout, r)


def pack_conv3d(weight):
    """[cout, cin, 3, 3, 3] -> MFMA A fragments of [cout, 27 * cin_pad], k = tap * cin_pad + ci."""
    cout, cin = weight.shape[:2]
    cpad = (cin + 15) // 16 * 16
    w = torch.zeros(cout, 27, cpad, dtype=torch.float32)
    w[:, :, :cin] = weight.detach().float().cpu().reshape(cout, cin, 27).permute(0, 2, 1)
    return mfma_a_fragments(w.reshape(cout, 27 * cpad))


def split_conv_supported(cin, cout, r):
    """Shapes conv3d_k3_f16x2_impl dispatches (csrc/conv3d.hip; gldm_conv3d_k3_f16x2[_gn]: the listed (cout, r) with
    cin % 16 == 0, and the shipped encoder's first conv 3 -> 48 @ 24^3 with K = 81 packed into three 32-deep blocks), where
    the split arithmetic is on -- or the shape has no f32 instantiation and so keeps its only MFMA kernel."""
    from .numerics import split_enabled
    if not _instantiated(_F16X2, cin, cout, r):
        return False
    if (cin, cout, r) == FIRST_VOXEL_CONV:
        return split_enabled()   # under f32_only() its f32 form runs (K padded to 27 x 16: slower, exact f32 products)
    return split_enabled() or not conv_supported(cout, r)


def pack_conv3d_fewch_f16x2(weight):
    """[cout, cin <= 4, 3, 3, 3] -> split-f16 A fragments of [cout, roundup(27 cin, 32)], k = tap * cin + ci (tap-major,
    no padding between taps), zero beyond 27 cin."""
    from .r1d_pack import mfma_a_fragments_f16x2
    cout, cin = weight.shape[:2]
    k = 27 * cin
    w = torch.zeros(cout, (k + 31) // 32 * 32, dtype=torch.float32)
    w[:, :k] = weight.detach().float().cpu().reshape(cout, cin, 27).permute(0, 2, 1).reshape(cout, k)
    return mfma_a_fragments_f16x2(w)


def pack_conv3d_f16x2(weight):
    """[cout, cin, 3, 3, 3] (cin % 16 == 0) -> split-f16 A fragments of [cout, cblocks * 14 * 32]: K is walked as
    (16-channel block, pair of taps), k = ((cb * 14 + p) * 32 + 16 (tap - 2 p) + ci; tap 27 (second half of the last
    pair) is zero."""
    from .r1d_pack import mfma_a_fragments_f16x2
    cout, cin = weight.shape[:2]
    cb = cin // 16
    w = torch.zeros(cout, cb, 14, 2, 16, dtype=torch.float32)
    wt = weight.detach().float().cpu().reshape(cout, cb, 16, 27)            # [cout, cb, ci, tap]
    taps = torch.zeros(cout, cb, 16, 28)
    taps[..., :27] = wt
    w[:] = taps.reshape(cout, cb, 16, 14, 2).permute(0, 1, 3, 4, 2)          # [cout, cb, pair, half, ci]
    return mfma_a_fragments_f16x2(w.reshape(cout, cb * 14 * 32))


class VoxelBranchPlan:
    """Packed conv weights of one PVConv on the device (f32 fragments, or split-f16 ones where the conv has that kernel)."""

    def __init__(self, convs, device, r=None):
        from .r1d_pack import SplitRangeError
        self.split = [r is not None and split_conv_supported(c.in_channels, c.out_channels, r) for c in convs]
        # shapes without an MFMA instantiation run the direct kernel on the raw nn.Conv3d weight
        self.generic = [r is not None and not conv_supported(c.out_channels, r) for c in convs]
        self.w = []
        for i, c in enumerate(convs):
            if self.split[i]:
                try:
                    self.w.append((pack_conv3d_fewch_f16x2(c.weight) if c.in_channels < 16 else pack_conv3d_f16x2(c.weight)).to(device))
                    continue
                except SplitRangeError:   # a weight beyond the f16 range: this conv keeps an f32 kernel
                    self.split[i] = False
            self.w.append((c.weight.detach().float().contiguous() if self.generic[i] else pack_conv3d(c.weight)).to(device))


def _launch_conv(plan, i, conv, x, coef, b, r, cl, st):
    """Conv i of a voxel stack on the kernel its shape has -> (raw output, per-brick statistics).  coef: the (a, s) of the
    GroupNorm + Swish this conv applies to x while it stages its bricks, or None; cl: write the output channel-last."""
    cin, cout = conv.in_channels, conv.out_channels
    y = torch.empty((b, cout, r, r, r), dtype=torch.float32, device=x.device)
    nf = L.lib().gldm_conv3d_partial_floats(b, cout, r)
    partial = torch.empty(int(nf), dtype=torch.float32, device=x.device)
    staged = plan.split[i] and cin % 16 == 0
    if staged and (coef is not None or cl):
        L.call("gldm_conv3d_k3_f16x2_gn", L.ptr(x), L.ptr(coef), L.ptr(plan.w[i]), L.ptr(conv.bias), b, cin, cout, r,
               L.ptr(y), L.ptr(partial), 1 if cl else 0, st)
    elif cl:
        assert coef is None
        L.call("gldm_conv3d_k3_cl", L.ptr(x), L.ptr(plan.w[i]), L.ptr(conv.bias), b, cin, cout, r, L.ptr(y), L.ptr(partial), st)
    else:
        assert coef is None
        entry = "gldm_conv3d_k3_generic" if plan.generic[i] else ("gldm_conv3d_k3_f16x2" if plan.split[i] else "gldm_conv3d_k3")
        L.call(entry, L.ptr(x), L.ptr(plan.w[i]), L.ptr(conv.bias), b, cin, cout, r, L.ptr(y), L.ptr(partial), st)
    return y, partial


def _next_conv_stages_norm(plan, convs, i, r):
    """Conv i + 1 applies conv i's GroupNorm + Swish while it stages its planes (a cin % 16 == 0 split kernel on a large grid).
    Measured per 256 clouds: at 24^3 the pass costs 0.26 ms and the staged form 0.1 ms; at 12^3 the pass is 0.06 ms and the
    staged form 0.25 ms -- six channel blocks of exp / rcp in front of short tap loops -- so small grids keep the pass
    between their convs."""
    return plan.split[i + 1] and convs[i + 1].in_channels % 16 == 0 and r >= 16


def _groupnorm_coef(partial, gn, b, c, r, st):
    coef = torch.empty((b, c, 2), dtype=torch.float32, device=partial.device)
    L.call("gldm_groupnorm_coef", L.ptr(partial), L.ptr(gn.weight), L.ptr(gn.bias), b, c, r, gn.num_groups, float(gn.eps),
           L.ptr(coef), st)
    return coef


def run(plan, convs, norms, se, vox, norm_coords, point_feat, r):
    """vox [B, Cin, r, r, r] -> fused features [B, Cout, N] = gate * devox(voxel stack) + point_feat.

    GroupNorm + Swish never run as passes of their own where the consumer can apply them: every conv leaves its raw output
    and its per-brick statistics; gldm_groupnorm_coef folds those with the norm's affine into (a, s) per cloud and channel;
    a following split-f16 conv applies swish(a x + s) while it stages its bricks (gldm_conv3d_k3_f16x2_gn), the SE squeeze
    is a read-only pass (gldm_gn_swish_chan_sum) and the devoxelize pass applies it to the eight corners it reads
    (gldm_devoxelize_gn_fused).  The last conv of the stack, when it is one of the plane-staging kernels, writes its output
    channel-last so that both of those readers take a voxel's channels as one run (gldm_gn_swish_chan_sum_cl,
    gldm_devoxelize_gn_cl_fused: a point's eight corners are eight 16-byte-per-lane runs instead of 8 C scattered dwords).
    A conv without that staging (f32 / generic kernels) still gets gldm_groupnorm_swish in
    front of it."""
    dev = vox.device
    b = vox.shape[0]
    st = L.current_stream(dev)
    x = vox.contiguous()
    coef = None          # (a, s) of the GroupNorm + Swish still to be applied to x, or None
    chan_sum = None
    x_cl = False         # x is channel-last, [B, r^3, C]
    with torch.cuda.device(dev):
        for i, (conv, gn) in enumerate(zip(convs, norms)):
            cin, cout = conv.in_channels, conv.out_channels
            last = i == len(convs) - 1
            staged = plan.split[i] and cin % 16 == 0          # the plane-staging kernels: folded input, channel-last output
            mfma32 = not plan.split[i] and not plan.generic[i]   # the f32-MFMA kernels: channel-last output
            # the last conv's readers (squeeze, devoxelize) take a voxel's channels as one run
            cl = last and (staged or mfma32) and cout % 4 == 0 and cout <= 256 and cout // gn.num_groups <= 64
            y, partial = _launch_conv(plan, i, conv, x, coef, b, r, cl, st)
            x_cl = cl
            # the consumer of this conv's GroupNorm + Swish: the next conv if it stages planes (_next_conv_stages_norm),
            # else the SE pass + devoxelize (last conv), else a pass of its own
            foldable = (last or _next_conv_stages_norm(plan, convs, i, r)) and cout // gn.num_groups <= 64
            if foldable:
                coef = _groupnorm_coef(partial, gn, b, cout, r, st)
            else:
                coef = None
                if last and se is not None:
                    chan_sum = torch.empty((b, cout), dtype=torch.float32, device=dev)
                L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(partial), L.ptr(gn.weight), L.ptr(gn.bias), b, cout, r,
                       gn.num_groups, float(gn.eps), L.ptr(chan_sum) if (last and se is not None) else None, st)
            x = y
        c = x.shape[1]
        gate = None
        if se is not None:
            gate = torch.empty((b, c), dtype=torch.float32, device=dev)
            w1, w2 = se.fc[0].weight, se.fc[2].weight
            if x_cl:
                parts = int(L.lib().gldm_squeeze_parts())
                chan_sum = torch.empty((b, parts, c), dtype=torch.float32, device=dev)
                L.call("gldm_gn_swish_chan_sum_cl", L.ptr(x), L.ptr(coef), b, c, r, L.ptr(chan_sum), st)
                L.call("gldm_se_gate_parts", L.ptr(chan_sum), parts, L.ptr(w1), L.ptr(w2), b, c, w1.shape[0], r,
                       1 if se.use_relu else 0, L.ptr(gate), st)
            else:
                if coef is not None:
                    chan_sum = torch.empty((b, c), dtype=torch.float32, device=dev)
                    L.call("gldm_gn_swish_chan_sum", L.ptr(x), L.ptr(coef), b, c, r, L.ptr(chan_sum), st)
                L.call("gldm_se_gate", L.ptr(chan_sum), L.ptr(w1), L.ptr(w2), b, c, w1.shape[0], r,
                       1 if se.use_relu else 0, L.ptr(gate), st)
        n = norm_coords.shape[2]
        out = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        pf = point_feat.contiguous() if point_feat is not None else None
        if x_cl:
            L.call("gldm_devoxelize_gn_cl_fused", L.ptr(norm_coords), L.ptr(x), L.ptr(coef), L.ptr(gate), L.ptr(pf), b, c, n, r,
                   L.ptr(out), st)
        elif coef is not None:
            L.call("gldm_devoxelize_gn_fused", L.ptr(norm_coords), L.ptr(x), L.ptr(coef), L.ptr(gate), L.ptr(pf), b, c, n, r,
                   L.ptr(out), st)
        else:
            L.call("gldm_devoxelize_fused", L.ptr(norm_coords), L.ptr(x), L.ptr(gate), L.ptr(pf), b, c, n, r, L.ptr(out), st)
    return out


def run_attention(plan, convs, norms, attn, se, vox, norm_coords, point_feat, r):
    """`run` for PVConv(use_attention=True), pvconv.py:57-83 with `Attention` in place of the second Swish (modules.py:34-54):
    Conv3d -> GroupNorm -> Swish -> Conv3d -> GroupNorm -> Attention -> SE -> devoxelize (+ point branch).

    The first conv and its GroupNorm + Swish run as in `run`.  The second conv writes channel-major; its GroupNorm feeds the
    block RAW, so gldm_groupnorm_coef + gldm_groupnorm_affine make x [B, C, r^3] (the residual and, with the block's two
    folds, K and V at once).  Then the folded q' conv, the attention core (attention.attention_core: the fused kernel up to
    128 channels), the folded out conv, and ONE GroupNorm + Swish launch that adds the residual and leaves the SE squeeze
    sums (gldm_groupnorm_swish_points_sum); gldm_se_gate and gldm_devoxelize_fused close the stack."""
    from . import attention as A
    dev = vox.device
    b = vox.shape[0]
    st = L.current_stream(dev)
    x = vox.contiguous()
    coef = None
    with torch.cuda.device(dev):
        for i, (conv, gn) in enumerate(zip(convs, norms)):
            cout, last = conv.out_channels, i == len(convs) - 1
            y, partial = _launch_conv(plan, i, conv, x, coef, b, r, False, st)
            # the first conv's GroupNorm + Swish: staged by the second conv where `run` stages it, else a pass of its own;
            # the last conv's GroupNorm has no Swish: coefficients for the affine launch
            if last or (_next_conv_stages_norm(plan, convs, i, r) and cout // gn.num_groups <= 64):
                coef = _groupnorm_coef(partial, gn, b, cout, r, st)
            else:
                coef = None
                L.call("gldm_groupnorm_swish", L.ptr(y), L.ptr(partial), L.ptr(gn.weight), L.ptr(gn.bias), b, cout, r,
                       gn.num_groups, float(gn.eps), None, st)
            x = y
        c = x.shape[1]
        xa = torch.empty((b, c, r ** 3), dtype=torch.float32, device=dev)
        L.call("gldm_groupnorm_affine", L.ptr(x), L.ptr(coef), b, c, r, L.ptr(xa), st)
        pq, po = attn._packed(dev)
        h = A.run_conv(A.attention_core(A.run_conv(xa, pq), xa, xa), po)
        gate = None
        if se is not None:
            feat, chan_sum = A.groupnorm_swish_sum(h, attn.norm, add=xa)
            gate = torch.empty((b, c), dtype=torch.float32, device=dev)
            w1, w2 = se.fc[0].weight, se.fc[2].weight
            L.call("gldm_se_gate", L.ptr(chan_sum), L.ptr(w1), L.ptr(w2), b, c, w1.shape[0], r, 1 if se.use_relu else 0,
                   L.ptr(gate), st)
        else:
            feat = A.groupnorm_swish(h, attn.norm, add=xa)
        n = norm_coords.shape[2]
        out = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        pf = point_feat.contiguous() if point_feat is not None else None
        L.call("gldm_devoxelize_fused", L.ptr(norm_coords), L.ptr(feat), L.ptr(gate), L.ptr(pf), b, c, n, r, L.ptr(out), st)
    return out
