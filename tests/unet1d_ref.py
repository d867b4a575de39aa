"""Pure-torch restatement of the reference's Unet1D.forward (grasp_ldm/models/modules/resnets.py:622-857), composed
from oracle.torch_ref's ResnetBlock / LinearAttention / LayerNorm / time-embedding helpers plus the five pieces that net
adds: its channel widths and length changes, the middle full-softmax attention, the skip concatenations of the up path,
the tail that re-reads the stem's output, and its conditioning (a second Linear in input_emb_layers, embeddings added
untiled).  Device- and dtype-agnostic; eps fixed at 1e-5 (the reference's f32 branch), so the f64 run is the yardstick.
"""
import math

import torch
import torch.nn.functional as F

from oracle.torch_ref import _chan_layer_norm, _linear_attention, _resnet_block, time_embedding


def sinusoidal_pos_emb(time, dim):
    """SinusoidalPosEmb.forward, resnets.py:34-41."""
    half = dim // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half, device=time.device) * -emb)
    emb = time[:, None] * emb[None, :]
    return torch.cat((emb.sin(), emb.cos()), dim=-1)


def unet_time_embedding(sd, p, time):
    """time_mlp of Unet1D, resnets.py:699-715: the Fourier form is TimeConditionedResNet1D's; the default is SinusoidalPosEmb(dim)."""
    if (p + "time_mlp.0.weights") in sd:
        return time_embedding(sd, p, time)
    dim = sd[p + "init_conv.weight"].shape[0]
    h = F.linear(sinusoidal_pos_emb(time, dim), sd[p + "time_mlp.1.weight"], sd[p + "time_mlp.1.bias"])
    return F.linear(F.gelu(h), sd[p + "time_mlp.3.weight"], sd[p + "time_mlp.3.bias"])


def _mid_attention(sd, p, x, heads=4):
    """Residual(PreNorm(Attention)), resnets.py:238-261; p addresses the Residual ("mid_attn.")."""
    b, c, n = x.shape
    y = _chan_layer_norm(x, sd[p + "fn.norm.g"])
    qkv = F.conv1d(y, sd[p + "fn.fn.to_qkv.weight"])
    q, k, v = (t.reshape(b, heads, -1, n) for t in qkv.chunk(3, dim=1))
    d = q.shape[2]
    q = q * (d ** -0.5)
    sim = torch.einsum("bhdi,bhdj->bhij", q, k)
    attn = sim.softmax(dim=-1)
    out = torch.einsum("bhij,bhdj->bhid", attn, v)
    out = out.permute(0, 1, 3, 2).reshape(b, heads * d, n)
    return F.conv1d(out, sd[p + "fn.fn.to_out.weight"], sd[p + "fn.fn.to_out.bias"]) + x


def unet1d_forward(sd, p, x, z_cond=None, time=None, groups=8, temb=None):
    """Unet1D.forward, resnets.py:779-857, eval mode.  x [B,1,L]; z_cond [B,Dc], [B,R,Dc] (only without time) or None;
    time int64 [B] or None.  temb [B,E]: time-embedding rows to use instead of evaluating time_mlp (the f64 yardstick is fed
    the f32 rows both implementations take from the same host computation)."""
    x = F.conv1d(x, sd[p + "init_conv.weight"], sd[p + "init_conv.bias"], padding=3)
    r = x.clone()
    emb = temb if temb is not None else (unet_time_embedding(sd, p, time) if time is not None else None)
    if z_cond is not None:
        ie = F.silu(F.linear(z_cond, sd[p + "input_emb_layers.0.weight"], sd[p + "input_emb_layers.0.bias"]))
        ie = F.linear(ie, sd[p + "input_emb_layers.2.weight"], sd[p + "input_emb_layers.2.bias"])
        emb = ie if emb is None else emb + ie      # untiled: resnets.py:816-822
    h = []
    n_levels = 0
    while (p + f"downs.{n_levels}.3.weight") in sd:
        n_levels += 1
    for i in range(n_levels):
        q = p + f"downs.{i}."
        x = _resnet_block(sd, q + "0.", x, emb, groups)
        h.append(x)
        x = _resnet_block(sd, q + "1.", x, emb, groups)
        x = _linear_attention(sd, q + "2.", x)
        h.append(x)
        if i < n_levels - 1:
            x = F.conv1d(x, sd[q + "3.weight"], sd[q + "3.bias"], stride=2, padding=1)
        else:
            x = F.conv1d(x, sd[q + "3.weight"], sd[q + "3.bias"], padding=1)
    x = _resnet_block(sd, p + "mid_block1.", x, emb, groups)
    x = _mid_attention(sd, p + "mid_attn.", x)
    x = _resnet_block(sd, p + "mid_block2.", x, emb, groups)
    for j in range(n_levels):
        q = p + f"ups.{j}."
        x = _resnet_block(sd, q + "0.", torch.cat((x, h.pop()), dim=1), emb, groups)
        x = _resnet_block(sd, q + "1.", torch.cat((x, h.pop()), dim=1), emb, groups)
        x = _linear_attention(sd, q + "2.", x)
        if j < n_levels - 1:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            x = F.conv1d(x, sd[q + "3.1.weight"], sd[q + "3.1.bias"], padding=1)
        else:
            x = F.conv1d(x, sd[q + "3.weight"], sd[q + "3.bias"], padding=1)
    x = _resnet_block(sd, p + "final_res_block.", torch.cat((x, r), dim=1), emb, groups)
    return F.conv1d(x, sd[p + "final_conv.weight"], sd[p + "final_conv.bias"])


# The golden configurations (tools/make_golden_unet1d.py, tests/test_unet1d_*.py): constructor arguments of Unet1D,
# sequence length, shape of a z_cond row block (None: no input conditioning) and whether `time` is passed.
CASES = {
    "A": dict(args=dict(dim=16, dim_mults=(1, 2, 4, 8), is_time_conditioned=False, input_conditioning_dims=64,
                        resnet_block_groups=4), L=16, z_shape=(3, 64), seed=21),
    "B": dict(args=dict(dim=16, dim_mults=(1, 2, 4), is_time_conditioned=True, learned_sinusoidal_cond=True,
                        input_conditioning_dims=64, resnet_block_groups=4), L=16, z_shape=(64,), seed=22),
    "C": dict(args=dict(dim=16, dim_mults=(1, 2), is_time_conditioned=True, resnet_block_groups=8), L=4, z_shape=None,
              seed=23),
    "D": dict(args=dict(dim=32, dim_mults=(1, 2, 4), is_time_conditioned=False, resnet_block_groups=8), L=8, z_shape=None,
              seed=24),
    "E": dict(args=dict(dim=16, dim_mults=(1, 2), is_time_conditioned=False, resnet_block_groups=8), L=2, z_shape=None,
              seed=25),
}
GOLDEN_ROWS = 6


def _row(dim, mults, groups, L, rows=0, time=None, seed=0):
    """One ENVELOPE row: `rows` conditioning rows per sample (0: no input conditioning; 1: z_cond [n, 64]; R > 1: [n, R, 64]),
    time None / "fourier" (learned_sinusoidal_cond) / "plain" (SinusoidalPosEmb(dim))."""
    args = dict(dim=dim, dim_mults=mults, is_time_conditioned=time is not None, resnet_block_groups=groups)
    if time == "fourier":
        args["learned_sinusoidal_cond"] = True
    if rows:
        args["input_conditioning_dims"] = 64
    return dict(args=args, L=L, z_shape=None if rows == 0 else ((64,) if rows == 1 else (rows, 64)), seed=seed)


# Corners of the envelope gldm_unet1d_supported accepts that CASES leaves out (tests/test_unet1d_cpu.py holds the list
# of properties CASES and ENVELOPE must cover between them, tests/test_unet1d_envelope_gpu.py runs every row): widths
# that are no power of two or no multiple of 32, in decreasing order, up to 256; deepest levels of 3, 5 and 7 positions;
# tiles of 1 to 16 samples whose columns do not fill their last 16-column block; LDS maps up to the 160 KiB limit.
ENVELOPE = {
    "F": _row(16, (1, 3), 8, 6, seed=31),                        # widths 16 16 48; lengths 6 3; tile 10: 60 columns
    "G": _row(16, (1, 2, 4), 4, 12, 1, "fourier", seed=32),      # lengths 12 6 3; tile 5: 60 columns
    "H": _row(32, (1, 2, 4, 8), 8, 16, 1, "fourier", seed=33),   # tile 3, 151.6 KiB
    "I": _row(32, (1, 2, 4, 8), 4, 8, seed=34),                  # lengths 8 4 2 1; tile 4
    "J": _row(16, (16, 1), 8, 14, 1, seed=35),                   # widths 16 256 16; lengths 14 7; tile 1: 14 columns
    "K": _row(16, (5, 7, 9, 11), 4, 16, 0, "plain", seed=36),    # widths 80 112 144 176; tile 3, 150.5 KiB
    "M": _row(16, (1, 1), 8, 2, seed=37),                        # lengths 2 1; tile 16
    "N": _row(16, (1, 2), 8, 10, seed=38),                       # lengths 10 5; tile 6: 60 columns
    "O": _row(16, (2, 6), 4, 4, 4, seed=39),                     # widths 16 32 96: two-source convs of 96 + 32 and 32 + 16
    "P": _row(32, (1, 3), 8, 2, 2, seed=40),                     # widths 32 32 96; tile 16
    "Q": _row(32, (8, 8), 4, 16, 1, "fourier", seed=41),         # widths 32 256 256; tile 1
    "S": _row(32, (8, 8, 8), 4, 16, seed=42),                    # tile 1, 151.9 KiB
    "U": _row(32, (2, 4, 8, 8), 4, 16, seed=43),                 # tile 2, 158.0 KiB
    "X": _row(16, (1, 2, 4, 8), 8, 8, 1, "fourier", seed=44),    # lengths 8 4 2 1 with conditioning and time
}
# Inside the query's envelope, yet refused by the packer: the LDS map exceeds 160 KiB with one sample per tile.
LDS_REFUSED = {
    "R1": _row(32, (4, 8, 8, 8), 4, 16, seed=51),
    "R2": _row(32, (8, 8, 8, 8), 4, 8, seed=52),
    "R3": _row(16, (16, 16, 16, 16), 4, 8, seed=53),
}


def config(name):
    return CASES[name] if name in CASES else ENVELOPE[name]


def case_inputs(name, n, samples_per_cond=1):
    """(x [n,1,L], z_cond [n / samples_per_cond, ...] or None, time int64 [n] or None) of a configuration of CASES or
    ENVELOPE: drawn from the case's own generator, a different timestep per sample.  The first rows do not depend on n."""
    c = config(name)
    g = torch.Generator().manual_seed(1000 + c["seed"])
    x = torch.randn(4096, 1, c["L"], generator=g)[:n]
    z = None
    if c["z_shape"] is not None:
        z = torch.randn(4096, *c["z_shape"], generator=g)[: (n + samples_per_cond - 1) // samples_per_cond]
    t = torch.randint(0, 1000, (4096,), generator=g)[:n] if c["args"]["is_time_conditioned"] else None
    return x, z, t
