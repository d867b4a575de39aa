"""The shape envelope of the fused ResNet1D engines (csrc/resnet1d.hip: validate, pm_supported, pm16_supported, wide_widths,
ss_table_rows; r1d_tape.h: quad_levels, quad16_levels, gn_fusable) as a table of descriptors, hand-made state dicts for them
and their f64 yardstick.  tests/test_r1d_envelope_cpu.py pins what the library answers for every row,
tests/test_r1d_envelope_gpu.py runs every accepted row.

The Python modules fix emb_dim = 4 dim, dims[0] = dim and seq_len = dim; the C entry takes them apart, so most corners
need a state dict of their own: the key / shape schema of a module of dim = C0 with the embedding shapes overridden, filled
by the synthetic recipe.  The yardstick is oracle.torch_ref on that state dict cast to double, fed the engine's own f32
time-embedding rows (packed["temb"][t]): sin(2 pi t w) at t up to 999 is an f32 evaluation by definition of the module, and
an f64 one differs from it by ~7e-5 -- that would measure torch's sin, not the kernel.
"""
from collections import namedtuple

import torch

UNSUPPORTED = -3      # GLDM_ERR_UNSUPPORTED
PACKER = "packer"     # pack_resnet1d raises ValueError: no descriptor exists
P_NET, P_BOT = "net.", "bottleneck."   # a head row's ResNet1D and bottleneck inside its state dict

Accept = namedtuple("Accept", "cols table park")   # tile columns, scale/shift table and park scratch in the workspace
Row = namedtuple("Row", "name L C0 E widths cond_rows head expected mod seed", defaults=(None, 1))
# head: None (time-conditioned denoiser), "decoder", or ("encoder", Lz).  mod: None, "no_w3" (every split-f16 copy's offset
# zeroed in the descriptor: what a packer without them leaves) or "groups8" (the descriptor says 8 groups).


def _a(cols, table=False, park=False):
    return Accept(cols, table, park)


SHIP4, SHIP16 = (32, 64, 128, 256), (32, 64, 128, 256)
ROWS = [
    # ---- 4 positions, time-conditioned.  r1d_kernel<64, 4>: dims[0] = 4, E = 16, widths 32..256 behind it
    Row("d4_quad_only", 4, 4, 16, (32, 64, 128), 3, None, _a(64)),            # the wave-local chain with nothing behind it
    Row("d4_five_levels", 4, 4, 16, (32, 64, 128, 128, 256), 3, None, _a(64)),
    Row("d4_six_levels", 4, 4, 16, (32, 64, 128, 128, 128, 256), 3, None, _a(64)),   # GLDM_R1D_MAX_LEVELS
    Row("d4_narrower_behind_chain", 4, 4, 16, (32, 64, 128, 64), 3, None, _a(64)),
    Row("d4_256_only", 4, 4, 16, (256,), 3, None, _a(64)),
    Row("d4_128_256", 4, 4, 16, (128, 256), 3, None, _a(64)),
    Row("d4_rows1", 4, 4, 16, SHIP4, 1, None, _a(64)),
    Row("d4_rows2", 4, 4, 16, (32, 64), 2, None, _a(64)),
    Row("d4_rows4", 4, 4, 16, SHIP4, 4, None, _a(64)),          # R S E = 1024 > 1020: the general embedding loop
    Row("d4_rows5", 4, 4, 16, (32, 64, 128), 5, None, _a(64)),  # R > kMaxR: the general loop; pm_supported has no row bound
    # ... <32, 4>: everything else
    Row("d4_width4_behind", 4, 4, 16, (4, 32), 3, None, _a(32)),
    Row("d4_width16_last", 4, 4, 16, (16,), 3, None, _a(32)),
    Row("d4_width16_behind", 4, 4, 16, (32, 16), 3, None, _a(32)),
    Row("d4_emb32", 4, 4, 32, (32, 64), 3, None, _a(32)),       # the largest E of 4 positions (S E <= 320, S = 8)
    Row("d4_first16", 4, 16, 16, (32,), 3, None, _a(32)),
    Row("d4_first16_emb32", 4, 16, 32, (16, 128, 256), 3, None, _a(32)),
    Row("d4_first64", 4, 64, 16, (128,), 3, None, _a(32)),
    Row("d4_no_w3", 4, 4, 16, (32, 64), 3, None, _a(32), "no_w3"),
    Row("d4_seven_levels", 4, 4, 16, (32, 64, 128, 128, 128, 128, 256), 3, None, PACKER),
    Row("d4_emb48", 4, 4, 48, (32,), 3, None, UNSUPPORTED),     # S E = 384
    Row("d4_first8", 4, 8, 32, (32,), 3, None, UNSUPPORTED),    # gn_fusable: 2 channels per group
    Row("d4_no_levels", 4, 4, 16, (), 3, None, UNSUPPORTED),    # n_levels >= 1
    # ---- 16 positions, time-conditioned.  r1d_kernel<64, 16>: dims[0] = 16, E = 64, at most 4 rows, widths 32..256
    Row("d16_quad_only", 16, 16, 64, (32, 64, 128), 3, None, _a(64)),
    Row("d16_park_no_chain", 16, 16, 64, (32, 256), 3, None, _a(64, park=True)),   # one 32-channel block into two m-tiles per wave
    Row("d16_256_only", 16, 16, 64, (256,), 3, None, _a(64, park=True)),           # the same from the padded 16-channel level
    Row("d16_narrower_then_256", 16, 16, 64, (32, 64, 128, 64, 256), 3, None, _a(64, park=True)),
    Row("d16_six_levels", 16, 16, 64, (32, 64, 128, 128, 128, 256), 3, None, _a(64, park=True)),
    Row("d16_rows1", 16, 16, 64, (32, 64), 1, None, _a(64)),
    Row("d16_rows2", 16, 16, 64, SHIP16, 2, None, _a(64, park=True)),
    Row("d16_rows4", 16, 16, 64, SHIP16, 4, None, _a(64, park=True)),   # R S E = 1024 > 1020
    # ... <32, 16>
    Row("d16_rows5", 16, 16, 64, SHIP16, 5, None, _a(32)),      # pm16_supported: cond_rows <= 4
    Row("d16_width16_behind", 16, 16, 64, (16, 32), 3, None, _a(32)),
    Row("d16_width4_last", 16, 16, 64, (4,), 3, None, _a(32)),
    Row("d16_first4", 16, 4, 16, (4, 16), 3, None, _a(32)),     # C = 4 off OP_RES4: OP_CONV with cin = 4, one channel per group
    Row("d16_first4_emb64", 16, 4, 64, (32,), 3, None, _a(32)),
    Row("d16_first32", 16, 32, 128, (64,), 3, None, _a(32)),
    Row("d16_emb160", 16, 16, 160, (32, 128, 256), 3, None, _a(32)),   # S E = 320 > 256 threads: the general loop
    Row("d16_emb144", 16, 16, 144, (16,), 3, None, _a(32)),
    Row("d16_emb48", 16, 16, 48, (32,), 3, None, _a(32)),
    Row("d16_first64", 16, 64, 64, (128, 256), 3, None, _a(32)),
    Row("d16_no_w3", 16, 16, 64, (32, 64), 3, None, _a(32), "no_w3"),
    Row("d16_emb176", 16, 16, 176, (32,), 3, None, UNSUPPORTED),    # S E = 352
    Row("d16_emb72", 16, 16, 72, (32,), 3, None, UNSUPPORTED),      # E % 16
    Row("d16_width512", 16, 16, 64, (512,), 3, None, UNSUPPORTED),
    Row("d16_256_below_last", 16, 16, 64, (256, 128), 3, None, UNSUPPORTED),   # attention levels keep 4 regions in LDS
    Row("d16_width48", 16, 16, 64, (48,), 3, None, UNSUPPORTED),    # no power of two
    Row("d16_groups8", 16, 16, 64, (32,), 3, None, UNSUPPORTED, "groups8"),
    Row("d8_positions", 8, 16, 64, (32,), 3, None, UNSUPPORTED),    # seq_len 4 or 16
    # ---- pose decoder heads (gldm_decode): in_layer, 6 + 1 head rows
    Row("dec4", 4, 4, 16, (32, 64), 3, "decoder", _a(32)),          # latent_dim > 0 keeps it off <64, 4>
    Row("dec16_emb16", 16, 16, 16, (32, 64), 3, "decoder", _a(32)),             # E < 32: no table
    Row("dec16_first4", 16, 4, 64, (32,), 3, "decoder", _a(32)),                # dims[0] < 16: no table
    Row("dec16_emb128", 16, 32, 128, (64, 128), 3, "decoder", _a(32, table=True)),
    Row("dec16_quad_only", 16, 16, 64, (32, 64, 128), 3, "decoder", _a(64, table=True)),
    Row("dec16_park_no_chain", 16, 16, 64, (32, 256), 3, "decoder", _a(64, table=True, park=True)),
    # ---- grasp encoder heads (gldm_encode; 16 positions only): in_layer, 2 Lz folded head rows
    Row("enc_latent1", 16, 16, 64, (32, 64), 3, ("encoder", 1), _a(64, table=True)),
    Row("enc_latent32", 16, 16, 64, (32, 64), 3, ("encoder", 32), _a(64, table=True)),   # GLDM_R1D_MAX_LATENT
    Row("enc_latent32_narrow", 16, 16, 32, (32,), 3, ("encoder", 32), _a(32, table=True)),
    Row("enc_latent33", 16, 16, 64, (32,), 3, ("encoder", 33), PACKER),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
ACCEPTED = [r.name for r in ROWS if isinstance(r.expected, Accept)]


def make_state_dict(C0, E, widths, timed=True, Dc=64, seed=1, prefix=""):
    """Synthetic-recipe (tamed) weights of a TimeConditionedResNet1D (timed) / ResNet1D with first level C0, level widths
    `widths` and embedding width E: the module of dim = C0 gives the keys and shapes, the embedding shapes are overridden
    (every ResnetBlock's mlp.1.weight [2C, E]; input_emb_layers.0 and time_mlp.1 / .3 of width E)."""
    from graspldm_amd.resnets import ResNet1D, TimeConditionedResNet1D
    from graspldm_amd.synthetic import synthetic_state_dict
    kw = dict(dim=C0, channels=1, block_channels=tuple(widths), input_conditioning_dims=Dc, resnet_block_groups=4)
    net = TimeConditionedResNet1D(random_fourier_features=True, **kw) if timed else ResNet1D(**kw)
    schema = {}
    for k, v in net.state_dict().items():
        shape = tuple(v.shape)
        if k.endswith(".mlp.1.weight"):
            shape = (shape[0], E)
        elif k in ("input_emb_layers.0.weight", "time_mlp.1.weight"):
            shape = (E, shape[1])
        elif k in ("input_emb_layers.0.bias", "time_mlp.1.bias", "time_mlp.3.bias"):
            shape = (E,)
        elif k == "time_mlp.3.weight":
            shape = (E, E)
        schema[prefix + k] = (shape, v.dtype)
    return synthetic_state_dict(schema, seed=seed)


def head_state_dict(row):
    """The Linears around a head row's net: a decoder's in_layer [L, 4], tmrp [6, L], class_logits [1, L]; an encoder's
    in_layer [L, 7], out_layer [L, L] and the bottleneck's mu / logvar [Lz, L]."""
    from graspldm_amd.synthetic import synthetic_state_dict
    L, f32 = row.L, torch.float32
    if row.head == "decoder":
        shapes = {"in_layer": (L, 4), "tmrp": (6, L), "class_logits": (1, L)}
    else:
        lz = row.head[1]
        shapes = {"in_layer": (L, 7), "out_layer": (L, L), P_BOT + "mu": (lz, L), P_BOT + "logvar": (lz, L)}
    schema = {}
    for k, (o, i) in shapes.items():
        schema[k + ".weight"], schema[k + ".bias"] = ((o, i), f32), ((o,), f32)
    return synthetic_state_dict(schema, seed=row.seed)


_SD = {}


def state_dict(name, dtype=torch.float32):
    """The row's whole state dict (a head row: the net under "net."), built once per dtype."""
    if (name, dtype) not in _SD:
        if (name, torch.float32) not in _SD:
            row = BY_NAME[name]
            sd = make_state_dict(row.C0, row.E, row.widths, timed=row.head is None, seed=row.seed,
                                 prefix=P_NET if row.head else "")
            if row.head:
                sd.update(head_state_dict(row))
            _SD[name, torch.float32] = sd
        _SD[name, dtype] = {k: v.to(dtype) for k, v in _SD[name, torch.float32].items()}
    return _SD[name, dtype]


def pack(name):
    """pack_resnet1d of the row as the engine wrappers call it (grasp_vae.py for the heads), the row's `mod` applied to the
    descriptor.  Raises what the packer raises."""
    from graspldm_amd.r1d_pack import pack_resnet1d
    row, sd = BY_NAME[name], state_dict(name)
    kw = {}
    if row.head == "decoder":
        kw["decoder"] = dict(in_w=sd["in_layer.weight"], in_b=sd["in_layer.bias"], tmrp_w=sd["tmrp.weight"],
                             tmrp_b=sd["tmrp.bias"], cls_w=sd["class_logits.weight"], cls_b=sd["class_logits.bias"])
    elif row.head:
        kw["encoder"] = dict(in_w=sd["in_layer.weight"], in_b=sd["in_layer.bias"], out_w=sd["out_layer.weight"],
                             out_b=sd["out_layer.bias"], mu_w=sd[P_BOT + "mu.weight"], mu_b=sd[P_BOT + "mu.bias"],
                             logvar_w=sd[P_BOT + "logvar.weight"], logvar_b=sd[P_BOT + "logvar.bias"])
    packed = pack_resnet1d(sd, P_NET if row.head else "", groups=8 if row.mod == "groups8" else 4, seq_len=row.L,
                           cond_rows=row.cond_rows, num_steps=None if row.head else 1000, **kw)
    if row.mod == "no_w3":
        d = packed["desc"]
        for rb in d.rb:
            rb.c1_w3 = rb.c2_w3 = rb.c1_wq = rb.c2_wq = 0
        for lv in d.lv:
            lv.qkvn_w3 = lv.out_w3 = lv.down_w3 = lv.qkvn_wq = lv.out_wq = lv.down_wq = 0
    return packed


def table_rows(row):
    """Floats of one cloud's scale/shift rows: 2 C per ResnetBlock (ss_table_rows of resnet1d.hip)."""
    dims = (row.C0,) + tuple(row.widths)
    return sum(4 * c for c in dims[:-1]) + 2 * dims[-1]


def workspace_bytes(row, n, cus=256):
    """ws_layout of resnet1d.hip restated: 256-byte header + 8 bytes per column of every tile | 256-aligned table of
    n x table_rows floats | 256-aligned park scratch, 64 KiB per workgroup (one per tile, at most one per CU)."""
    a = row.expected
    tiles = -(-n // (a.cols // row.L))
    size = 256 + tiles * a.cols * 8
    if a.table:
        size = -(-size // 256) * 256 + n * table_rows(row) * 4
    if a.park:
        size = -(-size // 256) * 256 + min(tiles, cus) * 65536
    return size


# Two batches per engine geometry: one full tile and a last tile of at most 16 live columns (Ctx::nta == 1), one full tile
# and a wider last tile.  The smallest at which a tile boundary, a short tile and a full tile all occur.
def batches(row):
    s = row.expected.cols // row.L
    return {16: (19, 25), 4: (5, 7), 8: (11, 14), 2: (3, 4)}[s]


def inputs(name, spc=1):
    """(x, z_cond, t) of the row's larger batch, its smaller one being the first rows: x [n, 1, L] latents (a head row: the
    head's input rows [n, 4 | 7]), z_cond [ceil(n / spc), R, 64], t int64 [n] in [0, 1000)."""
    row = BY_NAME[name]
    n = batches(row)[1]
    g = torch.Generator().manual_seed(7000 + 13 * ROWS.index(row) + spc)
    width = {None: row.L, "decoder": 4}.get(row.head, 7)
    x = torch.randn(n, width, generator=g)
    z = torch.randn(-(-n // spc), row.cond_rows, 64, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    return (x.unsqueeze(1) if row.head is None else x), z, t


def per_sample(z, spc, n):
    return z.repeat_interleave(spc, dim=0)[:n]


def forward(name, x, z, t=None, temb=None, dtype=torch.float64):
    """One pass of the row's net in `dtype` (oracle.torch_ref).  Denoiser rows: eps; `temb` [T, E] is the f32 table whose
    rows t are fed instead of time_mlp (None: time_mlp is evaluated, in `dtype`'s own arithmetic after the f32 sin / cos).
    Decoder rows: (tmrp, logit).  Encoder rows: (mu, logvar).  z is one block of rows per sample."""
    from oracle import torch_ref as R
    row, sd = BY_NAME[name], state_dict(name, dtype)
    x, z = x.to(dtype), z.to(dtype)
    if row.head is None:
        return R.resnet1d_forward(sd, "", x, z_cond=z, time=t, temb=None if temb is None else temb[t].to(dtype))
    if row.head == "decoder":
        return R.decoder_forward(sd, "", x, z)
    from test_vae_encode_cpu import oracle_encode
    return oracle_encode(sd, x, z, enc="", bot=P_BOT)


DDIM_STEPS = 6


def ddim_tables():
    """The last 6 of 100 inference steps of the shipped schedule: (timesteps int32 [6], coefficient rows)."""
    from graspldm_amd.diffusion import make_schedule_tables
    ts, coef = make_schedule_tables("ddim", 1000, 5e-5, 1e-3, "linear", "fixed_large", 100)
    return ts[-DDIM_STEPS:].contiguous(), coef[-DDIM_STEPS:].contiguous()


def ddim_run(name, x, z, temb, dtype=torch.float64):
    """The restated loop: the row's net stepped by oracle.schedulers' DDIM (clip_sample on) over ddim_tables()."""
    from oracle import torch_ref as R
    sched = R.make_scheduler("ddim")
    sched.set_timesteps(100)
    xs = x.to(dtype)
    for t in ddim_tables()[0].tolist():
        eps = forward(name, xs, z, torch.full((x.shape[0],), t, dtype=torch.long), temb, dtype)
        xs = sched.step(eps, t, xs).prev_sample
    return xs
