"""The PVD `Attention` block (grasp_ldm/models/modules/modules.py:10-54): dense softmax attention of every point (D = 1) or
voxel (D = 3) over every other, between k = 1 convs, then residual + GroupNorm + Swish.  Same constructor and state_dict
keys as the reference ({q,k,v,out}.{weight,bias}, norm.{weight,bias}).

Two folds, exact algebra (only rounding changes), done in f64 on the host once per weight version (`fold_attention`):
  * softmax over j ignores terms constant in j, so  S[i, j] ~ q'[:, i] . x[:, j]  with  q' = (Wk^T Wq) x + Wk^T bq:
    the k projection disappears (K = x);
  * rows of P sum to 1, so  Wo (v P^T) + bo = (Wo Wv)(x P^T) + (Wo bv + bo): the v projection disappears (V = x).
The block is then two weight GEMMs (the package's k = 1 launches), the attention core reading ONE tensor as K and V
(gldm_point_attention, csrc/point_attention.hip) and one GroupNorm + Swish launch that adds the residual on its way
(gldm_groupnorm_swish_points, csrc/voxel_norm.hip).  No CPU path.

Voxel attention inside PVConv (pvconv.py:68-69: the block in place of the second Swish, tokens = the r^3 voxels) runs the
same algebra from voxel.run: `check_voxel_supported` is the one gate of its shapes, `attention_core` its dispatch between
the fused kernel (gldm_point_attention_fused: c <= 128, no n x n tensor) and the materialised core above."""
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import dense

MAX_GROUP_CHANNELS = 128   # gldm_groupnorm_swish_points


def supported(c, n=None):
    """Shapes gldm_point_attention is built for: c % 16 == 0 in 16 .. 1024, n % 32 == 0 in 32 .. 4096 (n=None: c alone)."""
    return c % 16 == 0 and 16 <= c <= 1024 and (n is None or (n % 32 == 0 and 32 <= n <= 4096))


def check_supported(c, n=None, num_groups=None):
    if not supported(c, n) or (num_groups is not None and c // num_groups > MAX_GROUP_CHANNELS):
        raise NotImplementedError(f"point attention over (C, N) = ({c}, {n}) has no kernel: C % 16 == 0 in 16..1024, "
                                  f"N % 32 == 0 in 32..4096, C / groups <= {MAX_GROUP_CHANNELS}")


VOXEL_MIN_C, VOXEL_MAX_C = 32, 1024   # voxel attention: channels (C = 16 would pad half of every 32-deep f16 MFMA)
VOXEL_MIN_R, VOXEL_MAX_R = 4, 16       # resolutions, r % 4 == 0: n = r^3 is a multiple of 64 in 64 .. 4096
FUSED_MAX_C = 128                      # gldm_point_attention_fused: 32 <= c <= 128


def voxel_supported(c, r):
    return (c % 16 == 0 and VOXEL_MIN_C <= c <= VOXEL_MAX_C and r % 4 == 0 and VOXEL_MIN_R <= r <= VOXEL_MAX_R)


def check_voxel_supported(c, r):
    """The one gate of PVConv(use_attention=True): out_channels c and voxel resolution r."""
    if not voxel_supported(c, r):
        raise NotImplementedError(f"voxel attention over (C, n) = ({c}, {r ** 3}) at resolution {r} has no kernel: C % 16 == 0 in "
                                  f"{VOXEL_MIN_C}..{VOXEL_MAX_C}, r % 4 == 0 in {VOXEL_MIN_R}..{VOXEL_MAX_R} (n = r^3, a multiple "
                                  f"of 64 in 64..4096)")


def fused_supported(c, n):
    """Shapes gldm_point_attention_fused is built for: c % 16 == 0 in 32 .. 128, n % 32 == 0 in 32 .. 4096."""
    return c % 16 == 0 and 32 <= c <= FUSED_MAX_C and n % 32 == 0 and 32 <= n <= 4096


def fold_attention(wq, bq, wk, wv, bv, wo, bo):
    """(Wq', bq', Wo', bo') in f64 from the four convs' [C, C] matrices and biases (bk drops out of the softmax)."""
    wq, bq, wk, wv, bv, wo, bo = (t.detach().double().cpu() for t in (wq, bq, wk, wv, bv, wo, bo))
    return wk.t() @ wq, wk.t() @ bq, wo @ wv, wo @ bv + bo


class PackedConv(NamedTuple):
    """A k = 1 conv W x + b packed for the launch its shape has (no activation)."""
    w: torch.Tensor
    b: torch.Tensor
    ws: Optional[torch.Tensor]   # split-f16 fragments (gldm_pointwise_mlp_f16x2), or None
    wp: Optional[torch.Tensor]   # f32 fragments (gldm_pointwise_mlp), or None


def pack_conv(w2d, bias, device):
    from .r1d_pack import SplitRangeError, mfma_a_fragments
    w = w2d.detach().float().contiguous()
    cout, cin = w.shape
    ws = wp = None
    if dense.split_mlp_supported(None, cin, cout):
        try:
            ws = dense.split_fragments(w).to(device)
        except SplitRangeError:   # a weight beyond the f16 range keeps the f32-pipe kernels
            ws = None
    if ws is None and dense.fused_mlp_supported(None, cin, cout):
        wp = mfma_a_fragments(w.cpu()).to(device)
    return PackedConv(w.to(device), bias.detach().float().contiguous().to(device), ws, wp)


def run_conv(x, p):
    """W x + b over [B, Cin, N] f32: the split launch, the f32 MFMA launch, or the narrow / any-shape kernel."""
    cout, cin = p.w.shape
    if p.ws is not None and dense.split_mlp_supported(x, cin, cout):
        return dense.pointwise_mlp(x, p.ws, p.b, cout, False, split=True)[0]
    if p.wp is not None and dense.fused_mlp_supported(x, cin, cout):
        return dense.pointwise_mlp(x, p.wp, p.b, cout, False)[0]
    return dense._gemm_bias_act(x, p.w, p.b, False)


def conv1x1(x, conv):
    """A Conv1d(k = 1) module over [B, Cin, N], packed once per weight version (kept on the conv)."""
    from ._cache import cached, params_key
    dev = x.device
    p = cached(conv, "_gldm_k1", params_key([conv.weight, conv.bias], dev),
               lambda: pack_conv(conv.weight.reshape(conv.weight.shape[0], -1), conv.bias, dev), dev)
    return run_conv(x.contiguous().float(), p)


def point_attention(q, k, v):
    """out[b, c, i] = sum_j v[b, c, j] softmax_j(sum_c' q[b, c', i] k[b, c', j]) over [B, C, N] f32 CUDA tensors (k and v may
    be one tensor).  Arithmetic by numerics: split-f16 products by default, exact f32 products under f32_only()."""
    from . import _lib as L
    from .numerics import split_enabled
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError("attention inputs must be CUDA tensors (graspldm_amd has no CPU path)")
    q, k, v = (t if t.is_contiguous() and t.dtype == torch.float32 else t.contiguous().float() for t in (q, k, v))
    b, c, n = q.shape
    check_supported(c, n)
    nbytes = int(L.lib().gldm_point_attention_workspace_bytes(b, c, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)   # stream-ordered: private to the current stream
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        L.call("gldm_point_attention", L.ptr(q), L.ptr(k), L.ptr(v), b, c, n, int(not split_enabled()), L.ptr(ws), nbytes,
               L.ptr(out), L.current_stream(q.device))
    return out


def point_attention_fused(q, k, v):
    """point_attention's contract in one launch without a workspace (gldm_point_attention_fused): c <= 128."""
    from . import _lib as L
    from .numerics import split_enabled
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError("attention inputs must be CUDA tensors (graspldm_amd has no CPU path)")
    q, k, v = (t if t.is_contiguous() and t.dtype == torch.float32 else t.contiguous().float() for t in (q, k, v))
    b, c, n = q.shape
    if not fused_supported(c, n):
        raise NotImplementedError(f"fused point attention over (C, N) = ({c}, {n}) has no kernel: C % 16 == 0 in 32..{FUSED_MAX_C}, "
                                  f"N % 32 == 0 in 32..4096")
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        L.call("gldm_point_attention_fused", L.ptr(q), L.ptr(k), L.ptr(v), b, c, n, int(not split_enabled()), L.ptr(out),
               L.current_stream(q.device))
    return out


def attention_core(q, k, v):
    """The core of the voxel path, by width and under both arithmetics: c <= 128 takes the fused kernel, wider tensors
    the materialised core (measured at three shapes: DESIGN.md 4.6)."""
    return point_attention_fused(q, k, v) if q.shape[1] <= FUSED_MAX_C else point_attention(q, k, v)


def groupnorm_swish_sum(x, norm, add=None):
    """(swish(GroupNorm(x + add)), its per-(cloud, channel) sums over N) over [B, C, N], one launch."""
    from . import _lib as L
    b, c, n = x.shape
    out = torch.empty_like(x)
    chan_sum = torch.empty((b, c), dtype=torch.float32, device=x.device)
    gamma, beta = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
    with torch.cuda.device(x.device):
        L.call("gldm_groupnorm_swish_points_sum", L.ptr(x), L.ptr(add), L.ptr(gamma), L.ptr(beta), b, c, n, int(norm.num_groups),
               float(norm.eps), L.ptr(out), L.ptr(chan_sum), L.current_stream(x.device))
    return out, chan_sum


def groupnorm_swish(x, norm, add=None):
    """swish(GroupNorm(x + add)) over [B, C, N], one launch."""
    from . import _lib as L
    b, c, n = x.shape
    out = torch.empty_like(x)
    gamma, beta = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
    with torch.cuda.device(x.device):
        L.call("gldm_groupnorm_swish_points", L.ptr(x), L.ptr(add), L.ptr(gamma), L.ptr(beta), b, c, n, int(norm.num_groups),
               float(norm.eps), L.ptr(out), L.current_stream(x.device))
    return out


class Attention(nn.Module):
    def __init__(self, in_ch, num_groups, D=3):
        super().__init__()
        assert in_ch % num_groups == 0
        if D not in (1, 3):
            raise ValueError(f"D must be 1 or 3, not {D}")
        check_supported(in_ch, None, num_groups)
        conv = nn.Conv3d if D == 3 else nn.Conv1d
        self.q = conv(in_ch, in_ch, 1)
        self.k = conv(in_ch, in_ch, 1)
        self.v = conv(in_ch, in_ch, 1)
        self.out = conv(in_ch, in_ch, 1)
        self.norm = nn.GroupNorm(num_groups, in_ch)

    def _packed(self, device):
        from ._cache import cached, params_key
        src = [self.q.weight, self.q.bias, self.k.weight, self.v.weight, self.v.bias, self.out.weight, self.out.bias]
        c = self.q.weight.shape[0]

        def build():
            wq, bq, wo, bo = fold_attention(*(t.reshape(c, c) if t.ndim > 1 else t for t in src))
            return pack_conv(wq, bq, device), pack_conv(wo, bo, device)
        return cached(self, "_gldm_attn", params_key(src, device), build, device)

    @torch.no_grad()
    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("input must be a CUDA tensor (graspldm_amd has no CPU path)")
        b, c = x.shape[:2]
        x3 = x.reshape(b, c, -1).contiguous().float()
        check_supported(c, x3.shape[-1], self.norm.num_groups)
        pq, po = self._packed(x.device)
        h = point_attention(run_conv(x3, pq), x3, x3)
        y = groupnorm_swish(run_conv(h, po), self.norm, add=x3)
        return y.reshape(x.shape)
