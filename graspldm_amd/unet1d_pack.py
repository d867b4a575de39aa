"""Host-side preparation of a Unet1D (grasp_ldm/models/modules/resnets.py:622-857) for the fused kernel
(csrc/unet1d.hip, C ABI `gldm_unet1d_desc` in include/gldm.h).

Runs once per weight version: weight standardisation of every `Block.proj` (f32, eps 1e-5), every conv / 1x1 as
A fragments of the matrix pipe (split-f16, or f32 under numerics.f32_only()), the K axis of the two-source convs
(an up block's `cat(x, skip)`, the tail's `cat(x, r)`) as [source][tap][channels padded to 32 with zero columns], the
time-embedding table [T, E], and the network itself as the PROGRAM the kernel interprets: a list of ops naming LDS buffers
laid out (and bounds-checked) here for one sequence length and one tile size.  `run_program_cpu` executes the same program
with torch on the CPU: the packer and the LDS map are pinned without a GPU.
"""
import math

import torch
import torch.nn.functional as F

from . import _abi
from .r1d_pack import SplitPrecisionError, _Buf, split_planes, time_embedding_table, weight_standardize

# the descriptor, the limits and the program format of include/gldm.h (csrc/unet1d.hip interprets the same constants)
_C = _abi.CONSTANTS
MAX_LEVELS = _C["GLDM_UNET1D_MAX_LEVELS"]
OP_CONV, OP_GN, OP_ATT, OP_FINAL, OP_STEM = (_C["GLDM_UNET1D_OP_" + n] for n in ("CONV", "GN", "ATT", "FINAL", "STEM"))
OP_INTS = _C["GLDM_UNET1D_OP_INTS"]
EMB_PITCH = _C["GLDM_UNET1D_EMB_PITCH"]
UnetDesc = _abi.STRUCTS["gldm_unet1d_desc"]
LDS_MAX_BYTES = 160 * 1024
LDS_TWO_PER_CU = 80 * 1024
HEADS, DIM_HEAD = 4, 32


def f32_fragments(w2d):
    """[M, K] (M % 16 == 0, K % 32 == 0) -> [M/16][K/32][lane 64][8 f32], lane l = W[16 mt + (l & 15)][32 kb + 8 (l >> 4) + j]:
    the split-f16 fragment's indexing with one f32 per element (same 2 KiB per fragment)."""
    m, k = w2d.shape
    wp = w2d.float().reshape(m // 16, 16, k // 32, 4, 8)          # (mt, i, kb, g, j)
    return wp.permute(0, 2, 3, 1, 4).contiguous().reshape(-1)     # (mt, kb, g, i, j): lane = 16 g + i


def f16x2_fragments(w2d):
    """[M, K] -> [M/16][K/32][plane hi|lo][lane 64][8 f16] as an f32-typed bit container (include/gldm.h)."""
    m, k = w2d.shape
    planes = torch.stack(split_planes(w2d)).reshape(2, m // 16, 16, k // 32, 4, 8)   # (plane, mt, i, kb, g, j)
    frag = planes.permute(1, 3, 0, 4, 2, 5).contiguous()
    return frag.reshape(-1, 8).view(torch.float32).reshape(-1)


def fragments(w2d, exact_f32):
    m, k = w2d.shape
    if m % 16 or k % 32:
        raise ValueError(f"fragments need M % 16 == 0 and K % 32 == 0, not {m} x {k}")
    return f32_fragments(w2d) if exact_f32 else f16x2_fragments(w2d)


def unpack_fragments(flat, m, k, exact_f32):
    """Inverse of `fragments`: the [M, K] matrix the kernel multiplies with (f64: hi + lo is exact there)."""
    n = (m // 16) * (k // 32) * 512
    flat = flat[:n].contiguous()
    if exact_f32:
        return flat.reshape(m // 16, k // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(m, k).double()
    pl = flat.view(torch.float16).reshape(m // 16, k // 32, 2, 4, 16, 8).double().sum(2)   # (mt, kb, g, i, j)
    return pl.permute(0, 3, 1, 2, 4).reshape(m, k)


def pad_sources(w, splits):
    """Conv1d weight [Cout, sum(splits), taps] -> [Cout, K], K = [source][tap][channels padded to whole 32-blocks]
    (zero columns): K = 64 + 32 stays 64 + 32 per tap, 16 + 16 becomes 32 + 32 of which half is zero."""
    cout, _, taps = w.shape
    parts, a = [], 0
    for c in splits:
        cp = (c + 31) // 32 * 32
        blk = torch.zeros(cout, taps, cp, dtype=torch.float32)
        blk[:, :, :c] = w[:, a:a + c, :].permute(0, 2, 1)
        parts.append(blk.reshape(cout, taps * cp))
        a += c
    return torch.cat(parts, dim=1)


def source_columns(splits, taps):
    """For every K column of `pad_sources`: (source, tap, channel) or None for a zero (padding) column."""
    cols = []
    for si, c in enumerate(splits):
        cp = (c + 31) // 32 * 32
        for t in range(taps):
            cols += [(si, t, ch) if ch < c else None for ch in range(cp)]
    return cols


def sinusoidal_time_table(sd, p, num_steps, dim):
    """time_mlp with the plain SinusoidalPosEmb(dim) (resnets.py:29-41,707-715) for t = 0..T-1, in f32 like the module."""
    t = torch.arange(num_steps, dtype=torch.long)
    half = dim // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half) * -emb)
    emb = t[:, None] * emb[None, :]
    emb = torch.cat((emb.sin(), emb.cos()), dim=-1)
    h = F.linear(emb, sd[p + "time_mlp.1.weight"], sd[p + "time_mlp.1.bias"])
    return F.linear(F.gelu(h), sd[p + "time_mlp.3.weight"], sd[p + "time_mlp.3.bias"]).contiguous()


def time_table(sd, p, num_steps, dim):
    if (p + "time_mlp.0.weights") in sd:
        return time_embedding_table(sd, p, num_steps)
    return sinusoidal_time_table(sd, p, num_steps, dim)


def level_lengths(seq_len, n_levels):
    return [seq_len >> min(i, n_levels - 1) for i in range(n_levels)]


def _pitch(s, lc):
    return (s * lc + 15) // 16 * 16 + 2


class _Program:
    """Ops with symbolic buffers; `resolve(S)` lays the buffers out for a tile of S samples."""

    def __init__(self, seq_len, emb_dim):
        self.ops, self.sizes, self.L, self.E = [], {}, seq_len, emb_dim
        self.ss_rows, self.att_len = 0, 0

    def touch(self, name, c, lc):
        self.sizes.setdefault(name, set()).add((c, lc))

    def work(self, *busy):
        return [n for n in ("W0", "W1", "W2") if n not in busy]

    def conv(self, srcs, dst, m, mode, taps, lin, lout, w, b, add=None):
        for n, c in srcs:
            self.touch(n, c, lin)
        self.touch(dst, m, lout)
        self.ops.append(dict(kind=OP_CONV, srcs=srcs, dst=dst, m=m, mode=mode, taps=taps, lin=lin, lout=lout, w=w, b=b, add=add))

    def ss(self, m, w, b):
        self.ss_rows = max(self.ss_rows, m)
        self.ops.append(dict(kind=OP_CONV, ss=True, m=m, w=w, b=b))

    def gn(self, buf, c, lc, gw, gb, use_ss, add, out, groups):
        self.touch(out, c, lc)
        self.ops.append(dict(kind=OP_GN, buf=buf, c=c, l=lc, gw=gw, gb=gb, use_ss=use_ss, add=add, out=out, groups=groups))

    def att(self, x, c, lc, out, lnb, yb, ln_g, qkv_w, out_w, out_b, ln2):
        for n in (out, lnb, yb):
            self.touch(n, c, lc)
        self.att_len = max(self.att_len, lc)
        self.ops.append(dict(kind=OP_ATT, x=x, c=c, l=lc, out=out, lnb=lnb, yb=yb, ln_g=ln_g, qkv_w=qkv_w, out_w=out_w,
                             out_b=out_b, ln2=ln2))

    def lds_floats(self, s):
        return self.resolve(s, dry=True)

    def resolve(self, s, dry=False):
        off, at = {}, 0

        def take(name, n):
            nonlocal at
            off[name] = at
            at += (n + 3) // 4 * 4

        take("LAT", s * self.L)
        take("EPS", s * self.L)
        take("EMB", self.E * EMB_PITCH)
        take("SS", max(self.ss_rows, 1) * s)
        pa = _pitch(s, self.att_len)
        take("QKV", 96 * pa)
        take("O", 32 * pa)
        take("A", s * self.att_len * self.att_len)
        for name in sorted(self.sizes, key=str):
            take(name, max(c * _pitch(s, lc) for c, lc in self.sizes[name]))
        if dry:
            return at
        rows = []
        for o in self.ops:
            r = [0] * OP_INTS
            r[0] = o["kind"]
            if o["kind"] == OP_CONV and o.get("ss"):
                r[1:16] = [off["EMB"], self.E, EMB_PITCH, -1, 0, off["SS"], s, o["m"], 0, 1, 1, 1, o["w"], o["b"], -1]
            elif o["kind"] == OP_CONV:
                (n0, c0), (n1, c1) = o["srcs"][0], (o["srcs"][1] if len(o["srcs"]) > 1 else (None, 0))
                r[1:16] = [off[n0], c0, _pitch(s, o["lin"]), off[n1] if n1 is not None else -1, c1, off[o["dst"]],
                           _pitch(s, o["lout"]), o["m"], o["mode"], o["taps"], o["lin"], o["lout"], o["w"],
                           o["b"] if o["b"] is not None else -1, off[o["add"]] if o["add"] is not None else -1]
            elif o["kind"] == OP_GN:
                r[1:11] = [off[o["buf"]], o["c"], _pitch(s, o["l"]), o["l"], o["gw"], o["gb"], int(o["use_ss"]),
                           off[o["add"]] if o["add"] is not None else -1, off[o["out"]], o["groups"]]
            elif o["kind"] == OP_ATT:
                r[1:13] = [off[o["x"]], o["c"], _pitch(s, o["l"]), o["l"], off[o["out"]], off[o["lnb"]], off[o["yb"]],
                           o["ln_g"], o["qkv_w"], o["out_w"], o["out_b"], o["ln2"] if o["ln2"] is not None else -1]
            elif o["kind"] in (OP_FINAL, OP_STEM):
                r[1:6] = [off[o["buf"]], o["c"], _pitch(s, self.L), o["w"], o["b"]]
            rows.append(r)
        return rows, off, at


def choose_tile_samples(prog):
    """The largest tile (<= 16 samples) whose LDS leaves room for two workgroups per compute unit, if that is at least 4
    samples; otherwise up to 4 samples in whatever one workgroup may take."""
    for s in range(16, 3, -1):
        if prog.lds_floats(s) * 4 <= LDS_TWO_PER_CU:
            return s
    for s in range(4, 0, -1):
        if prog.lds_floats(s) * 4 <= LDS_MAX_BYTES:
            return s
    raise NotImplementedError("this Unet1D does not fit the 160 KiB of LDS of a workgroup even with one sample per tile")


def pack_unet1d(sd, p, groups, seq_len, cond_rows=0, time_cond=False, num_steps=None, tile_samples=None):
    """_pack_unet1d; where a matrix would not be accurate enough in split form (SplitPrecisionError), the whole network in
    the exact_f32 form numerics.f32_only() packs: the kernel has one arithmetic per descriptor."""
    try:
        return _pack_unet1d(sd, p, groups, seq_len, cond_rows, time_cond, num_steps, tile_samples)
    except SplitPrecisionError:
        from .numerics import f32_only
        with f32_only():
            return _pack_unet1d(sd, p, groups, seq_len, cond_rows, time_cond, num_steps, tile_samples)


def _pack_unet1d(sd, p, groups, seq_len, cond_rows=0, time_cond=False, num_steps=None, tile_samples=None):
    """sd: flat state dict (CPU f32), p: prefix of the Unet1D.  cond_rows: 0 without z_cond, 1 for [n, Dc], R for [n, R, Dc].
    -> dict(desc, weights, temb [T, E] | None, cond_w0/b0/w2/b2 | None, ops (the resolved program rows), lds (name -> offset))."""
    from .numerics import split_enabled
    exact = not split_enabled()
    sd = {k: v.detach().float().cpu() for k, v in sd.items() if k.startswith(p)}
    init_w = sd[p + "init_conv.weight"]
    dim = init_w.shape[0]
    n_levels = 0
    while (p + f"downs.{n_levels}.3.weight") in sd:
        n_levels += 1
    dims = [dim] + [sd[p + f"downs.{i}.3.weight"].shape[0] for i in range(n_levels)]
    emb = 4 * dim
    has_emb = bool(time_cond or cond_rows > 0)
    lens = level_lengths(seq_len, n_levels)
    buf = _Buf()
    buf.add(torch.zeros(4))   # offset 0 is never a weight: 0 / -1 mean "absent"
    prog = _Program(seq_len, emb)
    rsum = max(cond_rows, 1)

    def frag(w2d):
        return buf.add(fragments(w2d, exact))

    def resblock(q, srcs, lc, cout, out=None):
        busy = [n for n, _ in srcs]
        wa, wb = prog.work(*busy, out)[:2]
        out = wb if out is None else out
        splits = [c for _, c in srcs]
        if has_emb:
            mw, mb = sd[q + "mlp.1.weight"], sd[q + "mlp.1.bias"]
            comb = rsum * mb
            comb[:cout] = comb[:cout] + rsum      # sum_r (scale_r + 1)
            prog.ss(2 * cout, frag(mw), buf.add(comb))
        w1 = pad_sources(weight_standardize(sd[q + "block1.proj.weight"]), splits)
        prog.conv(srcs, wa, cout, 0, 3, lc, lc, frag(w1), buf.add(sd[q + "block1.proj.bias"]))
        prog.gn(wa, cout, lc, buf.add(sd[q + "block1.norm.weight"]), buf.add(sd[q + "block1.norm.bias"]), has_emb, None, wa,
                groups)
        w2 = pad_sources(weight_standardize(sd[q + "block2.proj.weight"]), [cout])
        prog.conv([(wa, cout)], wb, cout, 0, 3, lc, lc, frag(w2), buf.add(sd[q + "block2.proj.bias"]))
        gw, gb = buf.add(sd[q + "block2.norm.weight"]), buf.add(sd[q + "block2.norm.bias"])
        if (q + "res_conv.weight") in sd:
            prog.gn(wb, cout, lc, gw, gb, False, None, wb, groups)
            wr = pad_sources(sd[q + "res_conv.weight"], splits)
            prog.conv(srcs, out, cout, 0, 1, lc, lc, frag(wr), buf.add(sd[q + "res_conv.bias"]), add=wb)
        else:
            prog.gn(wb, cout, lc, gw, gb, False, srcs[0][0], out, groups)
        return out

    def attention(q, x, c, lc, out=None, mid=False):
        out = x if out is None else out
        lnb, yb = prog.work(x, out)[:2]
        wqkv = sd[q + "fn.fn.to_qkv.weight"][:, :, 0]                      # [384, C]: q | k | v, head h at rows 32 h
        hid = HEADS * DIM_HEAD
        if wqkv.shape[0] != 3 * hid:
            raise NotImplementedError("attention with heads=4, dim_head=32 expected (resnets.py:212,239)")
        rows = torch.cat([wqkv[t * hid + DIM_HEAD * h: t * hid + DIM_HEAD * (h + 1)] for h in range(HEADS) for t in range(3)])
        qkv_w = frag(pad_sources(rows[:, :, None], [c]))
        wo = sd[q + ("fn.fn.to_out.weight" if mid else "fn.fn.to_out.0.weight")][:, :, 0]   # [C, 128]
        out_w = frag(torch.cat([wo[:, DIM_HEAD * h: DIM_HEAD * (h + 1)] for h in range(HEADS)]))   # [4 C, 32]
        out_b = buf.add(sd[q + ("fn.fn.to_out.bias" if mid else "fn.fn.to_out.0.bias")])
        ln2 = None if mid else buf.add(sd[q + "fn.fn.to_out.1.g"])
        prog.att(x, c, lc, out, lnb, yb, buf.add(sd[q + "fn.norm.g"]), qkv_w, out_w, out_b, ln2)
        return out

    prog.touch("r", dim, seq_len)
    prog.ops.append(dict(kind=OP_STEM, buf="r", c=dim, w=buf.add(init_w.reshape(dim, 7)), b=buf.add(sd[p + "init_conv.bias"])))
    x, lc = "r", seq_len
    for i in range(n_levels):
        c, q = dims[i], p + f"downs.{i}."
        assert lc == lens[i]
        x = resblock(q + "0.", [(x, c)], lc, c, out=f"skip{2 * i}")
        x = resblock(q + "1.", [(x, c)], lc, c)
        x = attention(q + "2.", x, c, lc, out=f"skip{2 * i + 1}")
        last = i == n_levels - 1
        w = sd[q + "3.weight"]
        if w.shape[2] != (3 if last else 4):
            raise ValueError("downs.i.3 must be Conv1d(k=4, stride 2) or, on the last level, Conv1d(k=3)")
        dst = prog.work(x)[0]
        lout = lc if last else lc // 2
        prog.conv([(x, c)], dst, dims[i + 1], 0 if last else 1, w.shape[2], lc, lout, frag(pad_sources(w, [c])),
                  buf.add(sd[q + "3.bias"]))
        x, lc = dst, lout
    c = dims[-1]
    x = resblock(p + "mid_block1.", [(x, c)], lc, c)
    x = attention(p + "mid_attn.", x, c, lc, mid=True)
    x = resblock(p + "mid_block2.", [(x, c)], lc, c)
    for j in range(n_levels):
        i = n_levels - 1 - j
        din, dout, q = dims[i], dims[i + 1], p + f"ups.{j}."
        assert lc == lens[i]
        x = resblock(q + "0.", [(x, dout), (f"skip{2 * i + 1}", din)], lc, dout)
        x = resblock(q + "1.", [(x, dout), (f"skip{2 * i}", din)], lc, dout)
        x = attention(q + "2.", x, dout, lc)
        last = j == n_levels - 1
        key = q + ("3." if last else "3.1.")
        dst = prog.work(x)[0]
        lout = lc if last else 2 * lc
        prog.conv([(x, dout)], dst, din, 0 if last else 2, 3, lc, lout, frag(pad_sources(sd[key + "weight"], [dout])),
                  buf.add(sd[key + "bias"]))
        x, lc = dst, lout
    x = resblock(p + "final_res_block.", [(x, dim), ("r", dim)], lc, dim)
    fw = sd[p + "final_conv.weight"]
    if fw.shape[0] != 1:
        raise NotImplementedError("final_conv with one output channel expected (learned_variance, resnets.py:772)")
    prog.ops.append(dict(kind=OP_FINAL, buf=x, c=dim, w=buf.add(fw.reshape(-1)), b=buf.add(sd[p + "final_conv.bias"])))

    s = int(tile_samples) if tile_samples else choose_tile_samples(prog)
    rows, off, lds_floats = prog.resolve(s)
    prog_off = buf.add(torch.tensor(rows, dtype=torch.int32).reshape(-1).view(torch.float32))
    weights = buf.tensor()
    d = UnetDesc()
    d.dim, d.n_levels, d.groups, d.emb_dim = dim, n_levels, groups, emb
    for i, w_ in enumerate(dims):
        d.widths[i] = w_
    d.cond_rows, d.time_cond, d.has_emb, d.exact_f32 = cond_rows, int(bool(time_cond)), int(has_emb), int(exact)
    d.seq_len, d.tile_samples, d.lds_floats, d.prog_off, d.n_ops = seq_len, s, lds_floats, prog_off, len(rows)
    d.o_lat, d.o_eps, d.o_emb, d.o_ss = off["LAT"], off["EPS"], off["EMB"], off["SS"]
    d.o_qkv, d.o_o, d.o_a, d.n_floats = off["QKV"], off["O"], off["A"], weights.numel()
    check_program(d, rows)
    temb = None
    if time_cond:
        if num_steps is None:
            raise ValueError("num_steps needed for the time-embedding table")
        temb = time_table(sd, p, num_steps, dim)
    cond = None
    if cond_rows > 0:
        cond = tuple(sd[p + k].contiguous() for k in ("input_emb_layers.0.weight", "input_emb_layers.0.bias",
                                                       "input_emb_layers.2.weight", "input_emb_layers.2.bias"))
    return dict(desc=d, weights=weights, temb=temb, cond=cond, ops=rows, lds=off)


def check_program(d, rows):
    """Every LDS extent an op reads or writes lies inside the workgroup's allocation and every weight extent inside the
    packed buffer: the kernel trusts the program, so this is where its bounds are checked."""
    s, lds, nw = d.tile_samples, d.lds_floats, d.n_floats

    def in_lds(off, c, pitch, what):
        if off < 0 or off + c * pitch > lds:
            raise AssertionError(f"{what}: LDS extent [{off}, {off + c * pitch}) outside {lds}")

    def in_w(off, n, what):
        if off <= 0 or off + n > nw:
            raise AssertionError(f"{what}: weight extent [{off}, {off + n}) outside {nw}")

    if lds * 4 > LDS_MAX_BYTES:
        raise AssertionError("LDS over 160 KiB")
    for r in rows:
        k = r[0]
        if k == OP_CONV:
            _, s0, c0, pin, s1, c1, dst, pout, m, mode, taps, lin, lout, w, b, add = r
            if m % 16 or s * lout > pout or s * lin > pin:   # only columns < S * L are read or written
                raise AssertionError("conv geometry")
            in_lds(s0, c0, pin, "conv src0")
            if c1 > 0:
                in_lds(s1, c1, pin, "conv src1")
            in_lds(dst, m, pout, "conv dst")
            if add >= 0:
                in_lds(add, m, pout, "conv add")
            kb = taps * ((c0 + 31) // 32 + ((c1 + 31) // 32 if c1 > 0 else 0))
            in_w(w, (m // 16) * kb * 512, "conv w")
            if b >= 0:
                in_w(b, m, "conv bias")
        elif k == OP_GN:
            _, bufo, c, pitch, l, gw, gb, use_ss, add, out, g = r[:11]
            if c % g or s * l > pitch:
                raise AssertionError("gn geometry")
            for o_ in (bufo, out) + ((add,) if add >= 0 else ()):
                in_lds(o_, c, pitch, "gn")
            in_w(gw, c, "gn w"), in_w(gb, c, "gn b")
            if use_ss and d.o_ss + 2 * c * s > lds:
                raise AssertionError("gn scale/shift rows")
        elif k == OP_ATT:
            _, x, c, pitch, l, out, lnb, yb, ln_g, qkv_w, out_w, out_b, ln2 = r[:13]
            for o_ in (x, out, lnb, yb):
                in_lds(o_, c, pitch, "att")
            in_lds(d.o_qkv, 96, pitch, "att qkv"), in_lds(d.o_o, 32, pitch, "att o")
            if d.o_a + s * l * l > lds or l > 16:
                raise AssertionError("att A")
            in_w(qkv_w, 24 * ((c + 31) // 32) * 512, "att qkv_w"), in_w(out_w, 4 * (c // 16) * 512, "att out_w")
            in_w(out_b, c, "att out_b"), in_w(ln_g, c, "att ln_g")
            if ln2 >= 0:
                in_w(ln2, c, "att ln2")
        elif k in (OP_FINAL, OP_STEM):
            _, bufo, c, pitch, w, b = r[:6]
            in_lds(bufo, c, pitch, "stem/final")
            in_w(w, c * (7 if k == OP_STEM else 1), "stem/final w"), in_w(b, 1, "stem/final b")
        else:
            raise AssertionError(f"unknown op {k}")


# ---------------------------------------------------------------------------------------------------------------------
# The program on the CPU (f64, the unpacked fragments): what the kernel computes, op for op.
# ---------------------------------------------------------------------------------------------------------------------

def run_program_cpu(packed, x, temb_rows=None, cemb=None):
    """x [n, L] (n <= tile_samples), temb_rows [n, E] (the time-embedding row of each sample) or None, cemb [n, R, E] or
    None -> the network's output [n, L], by interpreting packed["ops"] over a flat f64 copy of the tile's LDS."""
    d, wts = packed["desc"], packed["weights"]
    s, L, E = d.tile_samples, d.seq_len, d.emb_dim
    n = x.shape[0]
    exact = bool(d.exact_f32)
    lds = torch.zeros(d.lds_floats, dtype=torch.float64)
    w64 = wts.double()

    def view(off, c, pitch, cols):
        return lds[off:off + c * pitch].view(c, pitch)[:, :cols]

    lds[d.o_lat:d.o_lat + n * L] = x.double().reshape(-1)
    if d.has_emb:
        e = torch.zeros(s, max(d.cond_rows, 1), E, dtype=torch.float64)
        if temb_rows is not None:
            e[:n] += temb_rows.double()[:, None, :]
        if cemb is not None:
            e[:n] += cemb.double()
        g = F.silu(e).sum(1)                        # [s, E]
        g[n:] = 0
        view(d.o_emb, E, EMB_PITCH, s).copy_(g.t())

    def conv(r):
        _, s0, c0, pin, s1, c1, dst, pout, m, mode, taps, lin, lout, w, b, add = r
        cols = []
        pos = torch.arange(lout)
        for so, c in ((s0, c0), (s1, c1)):
            if c <= 0:
                continue
            src = view(so, c, pin, s * lin).reshape(c, s, lin)
            cp = (c + 31) // 32 * 32
            for t in range(taps):
                if mode == 0:
                    q, ok = pos + t - taps // 2, torch.ones(lout, dtype=torch.bool)
                elif mode == 1:
                    q, ok = 2 * pos + t - 1, torch.ones(lout, dtype=torch.bool)
                else:
                    u = pos + t - 1
                    ok, q = (u >= 0) & (u < lout), u >> 1
                ok = ok & (q >= 0) & (q < lin)
                blk = torch.zeros(cp, s, lout, dtype=torch.float64)
                blk[:c] = src[:, :, q.clamp(0, lin - 1)] * ok
                cols.append(blk.reshape(cp, s * lout))
        bm = torch.cat(cols)
        wm = unpack_fragments(wts[w:], m, bm.shape[0], exact)
        y = wm @ bm
        if b >= 0:
            y = y + w64[b:b + m, None]
        if add >= 0:
            y = y + view(add, m, pout, s * lout)
        view(dst, m, pout, s * lout).copy_(y)

    def chan_ln(t, g):
        return (t - t.mean(0, keepdim=True)) * (t.var(0, unbiased=False, keepdim=True) + 1e-5).rsqrt() * g[:, None]

    for r in packed["ops"]:
        k = r[0]
        if k == OP_CONV:
            conv(r)
        elif k == OP_GN:
            _, bufo, c, pitch, l, gw, gb, use_ss, add, out, grp = r[:11]
            t = view(bufo, c, pitch, s * l).reshape(c, s, l).permute(1, 0, 2)      # [s, c, l]
            y = F.group_norm(t, grp, w64[gw:gw + c], w64[gb:gb + c], eps=1e-5)
            if use_ss:
                ss = lds[d.o_ss:d.o_ss + 2 * c * s].view(2 * c, s)
                y = y * ss[:c].t()[:, :, None] + ss[c:].t()[:, :, None]
            y = F.silu(y)
            if add >= 0:
                y = y + view(add, c, pitch, s * l).reshape(c, s, l).permute(1, 0, 2)
            view(out, c, pitch, s * l).copy_(y.permute(1, 0, 2).reshape(c, s * l))
        elif k == OP_ATT:
            _, xo, c, pitch, l, out, lnb, yb, ln_g, qkv_w, out_w, out_b, ln2 = r[:13]
            xx = view(xo, c, pitch, s * l).clone()
            cp = (c + 31) // 32 * 32
            y = torch.zeros(cp, s * l, dtype=torch.float64)
            y[:c] = chan_ln(xx, w64[ln_g:ln_g + c])
            wq = unpack_fragments(wts[qkv_w:], 4 * 96, cp, exact)
            wo = unpack_fragments(wts[out_w:], 4 * c, 32, exact)
            acc = w64[out_b:out_b + c, None].expand(c, s * l).clone()
            for h in range(HEADS):
                qkv = (wq[96 * h:96 * h + 96] @ y).reshape(3, 32, s, l)
                q_, k_, v_ = qkv[0], qkv[1], qkv[2]
                if ln2 >= 0:
                    q_ = q_.softmax(0) * DIM_HEAD ** -0.5
                    k_ = k_.softmax(-1)
                    ctx = torch.einsum("dsn,esn->sde", k_, v_)
                    o = torch.einsum("sde,dsn->esn", ctx, q_)
                else:
                    sim = torch.einsum("dsi,dsj->sij", q_ * DIM_HEAD ** -0.5, k_)
                    o = torch.einsum("sij,dsj->dsi", sim.softmax(-1), v_)
                acc = acc + wo[c * h:c * h + c] @ o.reshape(32, s * l)
            if ln2 >= 0:
                acc = chan_ln(acc, w64[ln2:ln2 + c])
            view(out, c, pitch, s * l).copy_(acc + xx)
        elif k == OP_STEM:
            _, dst, c, pitch, w, b = r[:6]
            lat = lds[d.o_lat:d.o_lat + s * L].view(s, 1, L)
            y = F.conv1d(lat, w64[w:w + 7 * c].view(c, 1, 7), w64[b:b + c], padding=3)    # [s, c, L]
            view(dst, c, pitch, s * L).copy_(y.permute(1, 0, 2).reshape(c, s * L))
        elif k == OP_FINAL:
            _, xo, c, pitch, w, b = r[:6]
            y = w64[w:w + c] @ view(xo, c, pitch, s * L) + w64[b]
            lds[d.o_eps:d.o_eps + s * L] = y
    return lds[d.o_eps:d.o_eps + n * L].view(n, L).clone()
