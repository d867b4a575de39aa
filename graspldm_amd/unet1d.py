"""Device-side handle of one Unet1D: owns the packed weight buffers on the GPU (one per sequence length met: the
program's LDS map is laid out for a length) and calls the fused kernel through the C ABI (gldm_unet1d).  Same interface
as r1d.R1dEngine where GaussianDiffusion1D.sample uses it (`cond_embed`, `denoise`), plus `forward`."""
import torch

from . import _lib as L
from .r1d_pack import SCHED_NONE
from .unet1d_pack import UnetDesc, pack_unet1d


def check_supported(desc, seq_len):
    """The library's shape query (gldm_unet1d_supported), asked before any HIP call: NotImplementedError naming the limit.
    Passing it is necessary, not sufficient: the widest shapes inside the envelope do not fit the 160 KiB of LDS even with
    one sample per tile, and the packer refuses those (unet1d_pack.choose_tile_samples: NotImplementedError as well, and
    also before any HIP call)."""
    st = L.lib().gldm_unet1d_supported(L.ref(desc), int(seq_len))
    if st != 0:
        raise NotImplementedError(
            f"Unet1D outside the fused kernel's envelope (dim in {{16, 32}}, 2..4 dim_mults, widths multiples of 16 up to 256, "
            f"groups 4 or 8, 2 <= L <= 16 with L % 2**(levels-1) == 0; inside it the packer still refuses a shape whose LDS map "
            f"exceeds 160 KiB): dim={desc.dim}, widths={list(desc.widths)[:desc.n_levels + 1]}, "
            f"groups={desc.groups}, L={seq_len}")


def header_desc(dim, dims, groups, cond_rows, time_cond):
    d = UnetDesc()
    d.dim, d.n_levels, d.groups, d.emb_dim = dim, len(dims) - 1, groups, 4 * dim
    for i, w in enumerate(dims[:5]):
        d.widths[i] = w
    d.cond_rows, d.time_cond = cond_rows, int(bool(time_cond))
    d.has_emb = int(bool(time_cond or cond_rows > 0))
    return d


class UnetEngine:
    def __init__(self, sd, groups, cond_rows, time_cond, num_steps, device):
        self.device = torch.device(device)
        self._sd, self.groups, self.cond_rows, self.time_cond, self.num_steps = sd, groups, cond_rows, time_cond, num_steps
        self._plans = {}
        self.cond = None
        if cond_rows > 0:
            self.cond = tuple(sd[k].to(self.device).contiguous() for k in
                              ("input_emb_layers.0.weight", "input_emb_layers.0.bias", "input_emb_layers.2.weight",
                               "input_emb_layers.2.bias"))

    def plan(self, seq_len):
        seq_len = int(seq_len)
        hit = self._plans.get(seq_len)
        if hit is None:
            dim = self._sd["init_conv.weight"].shape[0]
            dims, i = [dim], 0
            while f"downs.{i}.3.weight" in self._sd:
                dims.append(self._sd[f"downs.{i}.3.weight"].shape[0])
                i += 1
            check_supported(header_desc(dim, dims, self.groups, self.cond_rows, self.time_cond), seq_len)
            packed = pack_unet1d(self._sd, "", self.groups, seq_len, cond_rows=self.cond_rows, time_cond=self.time_cond,
                                 num_steps=self.num_steps)
            hit = self._plans[seq_len] = dict(desc=packed["desc"], weights=packed["weights"].to(self.device),
                                              temb=packed["temb"].to(self.device) if packed["temb"] is not None else None)
            from ._cache import publish
            publish(self.device)
        return hit

    def check(self):
        """Interface of r1d.R1dEngine: this kernel has no hand-off between workgroups, so nothing can have been lost."""

    def cond_embed(self, z_cond):
        """input_emb_layers = Linear, SiLU, Linear (resnets.py:724-728) on [n, R, Dc] or [n, Dc] -> [n, R, E]; None -> None."""
        if z_cond is None:
            if self.cond_rows:
                raise RuntimeError("this Unet1D is input conditioned: z_cond is required")
            return None
        if self.cond is None:
            raise RuntimeError("this Unet1D was built without input_conditioning_dims: it takes no z_cond")
        w0, b0, w2, b2 = self.cond
        z = z_cond if z_cond.ndim == 3 else z_cond.unsqueeze(1)
        z = z.to(self.device).contiguous().float()
        n, r, dc = z.shape
        e = w0.shape[0]
        if dc != w0.shape[1]:
            raise RuntimeError(f"z_cond has {dc} features per row; this network's conditioning Linear takes {w0.shape[1]}")
        hid = torch.empty((n, r, e), dtype=torch.float32, device=self.device)
        out = torch.empty_like(hid)
        with torch.cuda.device(self.device):
            st = L.current_stream(self.device)
            L.call("gldm_r1d_cond_embed", L.ptr(z), L.ptr(w0), L.ptr(b0), n, r, dc, e, L.ptr(hid), st)
            L.call("gldm_linear_rows", L.ptr(hid), L.ptr(w2), L.ptr(b2), n * r, e, e, L.ptr(out), st)
        return out

    def denoise(self, x_in, cemb, samples_per_cond, timesteps=None, sample_t=None, sched_kind=SCHED_NONE, clip_sample=True,
                coef=None, step_noise=None, sample_emb=None, temb=None):
        """x_in [n, 1, L] -> x after all steps (the module's output when sched_kind == NONE), one launch."""
        if sample_emb is not None or temb is not None:
            raise NotImplementedError("class embeddings and continuous-time tables are not part of the Unet1D kernel")
        n, seq_len = x_in.shape[0], x_in.shape[-1]
        plan = self.plan(seq_len)
        x_in = x_in.to(self.device).contiguous().float()
        out = torch.empty_like(x_in)
        n_steps = 1 if timesteps is None else int(timesteps.numel())
        if cemb is not None:
            cemb = cemb.contiguous()
            if cemb.shape[0] * int(samples_per_cond) < n:
                raise RuntimeError(f"{cemb.shape[0]} conditioning rows x {samples_per_cond} samples do not cover {n} samples")
        if plan["temb"] is not None:
            tmax = int((timesteps if sample_t is None else sample_t).max())
            if tmax >= plan["temb"].shape[0]:
                raise RuntimeError(f"timestep {tmax} beyond the time-embedding table ({plan['temb'].shape[0]} rows)")
        if step_noise is not None:
            step_noise = step_noise.contiguous().float()
        with torch.cuda.device(self.device):
            L.call("gldm_unet1d", L.ref(plan["desc"]), L.ptr(plan["weights"]),
                   L.ptr(plan["temb"]), L.ptr(cemb), int(samples_per_cond), L.ptr(x_in), n, seq_len, L.ptr(timesteps),
                   L.ptr(sample_t), n_steps, int(sched_kind), 1 if clip_sample else 0, L.ptr(coef), L.ptr(step_noise),
                   L.ptr(out), L.current_stream(self.device))
        return out

    def forward(self, x, cemb=None, samples_per_cond=1, sample_t=None):
        return self.denoise(x, cemb, samples_per_cond, sample_t=sample_t, sched_kind=SCHED_NONE)

    def denoise_rng(self, *args, **kwargs):
        raise NotImplementedError("the in-kernel noise stream is not part of the Unet1D kernel: use noise_source='tensor' "
                                  "(DDPM step noise from a [steps, n, 1, L] tensor)")


def _linear_rows(x, w, b):
    """y = x W^T + b over the rows of x [rows, n] (n % 4 == 0) by the hand-written row kernel."""
    rows, n = x.shape
    y = torch.empty((rows, w.shape[0]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.call("gldm_linear_rows", L.ptr(x), L.ptr(w), L.ptr(b), rows, n, w.shape[0], L.ptr(y), L.current_stream(x.device))
    return y


def _pad4(w):
    """Input columns of a Linear weight padded to a multiple of 4 with zeros (the row kernel reads 16-byte pieces)."""
    pad = (-w.shape[1]) % 4
    return torch.cat([w, torch.zeros(w.shape[0], pad)], dim=1) if pad else w


class UnetCoreEngine:
    """A Unet1D as the core of the VAE's pose decoder or grasp encoder (grasp_vae.py:356,440), with R1dEngine's interface
    there (`cond_embed`, `decode`, `encode`).  in_layer runs in front of the fused kernel and the head behind it, each as
    one gldm_linear_rows launch; the head is folded where the algebra allows: [tmrp; class_logits] is one [7, L] matrix, and
    an encoder's out_layer is folded into the bottleneck, [W_mu W_out; W_logvar W_out] (f64 products, rounded once: nothing
    sits between them, grasp_vae.py:113-115,532-536)."""

    def __init__(self, net_engine, in_w, in_b, head_w, head_b, kind):
        self.net, self.device, self.kind = net_engine, net_engine.device, kind
        self.in_w, self.in_b = _pad4(in_w.float()).to(self.device).contiguous(), in_b.float().to(self.device).contiguous()
        self.head_w, self.head_b = head_w.float().to(self.device).contiguous(), head_b.float().to(self.device).contiguous()
        self.in_features = in_w.shape[1]

    @classmethod
    def decoder(cls, net_engine, sd):
        return cls(net_engine, sd["in_layer.weight"], sd["in_layer.bias"],
                   torch.cat([sd["tmrp.weight"], sd["class_logits.weight"]]), torch.cat([sd["tmrp.bias"], sd["class_logits.bias"]]),
                   "decoder")

    @classmethod
    def encoder(cls, net_engine, sd, bottleneck_sd=None):
        ow, ob = sd["out_layer.weight"].double(), sd["out_layer.bias"].double()
        if bottleneck_sd is None:   # out_layer alone: mu = its output
            hw, hb = ow, ob
        else:
            bn = {k: v.double() for k, v in bottleneck_sd.items()}
            hw = torch.cat([bn["mu.weight"] @ ow, bn["logvar.weight"] @ ow])
            hb = torch.cat([bn["mu.weight"] @ ob + bn["mu.bias"], bn["logvar.weight"] @ ob + bn["logvar.bias"]])
        return cls(net_engine, sd["in_layer.weight"], sd["in_layer.bias"], hw, hb, "encoder" if bottleneck_sd is not None else "plain")

    def check(self):
        pass

    def cond_embed(self, z_cond):
        return self.net.cond_embed(z_cond)

    def _core(self, rows, cemb, samples_per_cond):
        rows = rows.reshape(rows.shape[0], -1).to(self.device).contiguous().float()
        if rows.shape[1] != self.in_features:
            raise RuntimeError(f"in_layer takes {self.in_features} features per row, not {rows.shape[1]}")
        if self.in_w.shape[1] != rows.shape[1]:
            rows = torch.nn.functional.pad(rows, (0, self.in_w.shape[1] - rows.shape[1]))
        h = _linear_rows(rows, self.in_w, self.in_b)
        y = self.net.denoise(h.unsqueeze(1), cemb, samples_per_cond, sched_kind=SCHED_NONE)
        return _linear_rows(y.reshape(y.shape[0], -1), self.head_w, self.head_b)

    def decode(self, z_h, cemb, samples_per_cond):
        out = self._core(z_h, cemb, samples_per_cond)
        return out[:, :6].contiguous(), out[:, 6:7].contiguous()

    def encode(self, h, cemb, samples_per_cond, eps=None, mix=(1.0, 1.0), eps_times_std=True, want_z=True):
        """As R1dEngine.encode: (mu, logvar, z) with z = mix[0] mu + mix[1] eps (exp(logvar / 2) if eps_times_std)."""
        out = self._core(h, cemb, samples_per_cond)
        if self.kind == "plain":
            return out, None, None
        lz = out.shape[1] // 2
        mu, logvar = out[:, :lz].contiguous(), out[:, lz:].contiguous()
        z = None
        if want_z:
            z = mix[0] * mu
            if eps is not None:
                e = eps.reshape(mu.shape).to(self.device).float()
                z = z + mix[1] * (e * torch.exp(0.5 * logvar) if eps_times_std else e)
        return mu, logvar, z
