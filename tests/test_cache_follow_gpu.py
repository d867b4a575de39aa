"""GPU: weight updates reach every kernel.  Almost every launch reads weights that were derived once and kept on the module
(graspldm_amd/_cache.py): folded GEMM matrices, split-f16 fragments, set-abstraction tables, voxel-conv packs, the 1-D
engines.  Here every cache owner is built for real, run, and run again after ONE tensor of its state_dict changed
(t <- 1.5 t + 0.125: running_var stays positive, everything stays far inside the f16 range):

  * the output equals, bit for bit, that of a twin built by the same constructor, loaded with the owner's state_dict and
    never run before (same route, same packed bytes);
  * the output differs from the one before the change -- a stale entry would return the old output, so this is what lets
    the test fail.  Tensors that provably cannot move the output stand in NO_EFFECT with their reason, itself asserted in f64;
  * every owner proves the cached route it is here for was taken (`route`), before and after the sweep;
  * after the sweep the last output is compared once with the owner's f64 restatement (oracle/torch_ref.py, tests/*_ref.py,
    assembled in `_ref_*` below) at the bar of the owner's existing test: 2e-5 for a forward, 5e-6 for the ResNet1D engines
    (tests/test_range_gpu.py), each times max(1, max |ref|) as tests/test_models_gpu.py and tests/test_unet1d_gpu.py take it:
    the swept weights are 1.5 times the recipe's, so outputs are no longer O(1).

The 1-D engines hold a hundred tensors and repack on the host per change: they are swept at one tensor per distinct trailing
key name (last two dotted components), first and last occurrence, plus the head tensors outside `net.`.

Once per owner, other ways a weight changes: load_state_dict, an optimiser step, p.data + invalidate_caches(), a device round
trip, numerics.f32_only() entered and left, copy.deepcopy."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

N1D = 11          # samples of the 1-D engine rows
RN = dict(block_channels=(32, 64, 128, 256), input_conditioning_dims=64, resnet_block_groups=4, dropout=0.1)
UN = dict(dim_mults=(1, 2, 4, 8), input_conditioning_dims=64, is_time_conditioned=False, resnet_block_groups=4)

# Tensors that cannot move the output, with the reason; test_no_effect_entries_are_justified asserts each in f64.
NO_EFFECT = {
    # softmax_j(q_i . (W_k x_j + b_k)) = softmax_j(q_i . W_k x_j + q_i . b_k): the added term is the same for every key j
    "attention-1d": {"k.bias"},
    "attention-3d": {"k.bias"},
    "pvconv-attention-32x32-r4": {"voxel_layers.6.k.bias"},
}


def _mode(mode):
    from graspldm_amd import numerics
    return numerics.f32_only() if mode == "f32" else contextlib.nullcontext()


def _split_on():
    from graspldm_amd.numerics import split_enabled
    return split_enabled()


def _tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _perturb(t):
    with torch.no_grad():
        t.mul_(1.5).add_(0.125)


def _floating(module):
    """Every floating tensor of the state_dict, parameters and buffers alike, as the objects the module holds."""
    return {k: t for k, t in module.state_dict(keep_vars=True).items() if t.is_floating_point()}


def _sd(module, dtype=None):
    return {k: (v.detach().cpu().to(dtype) if dtype is not None and v.is_floating_point() else v.detach().cpu())
            for k, v in module.state_dict().items()}


def _value(owner, slot):
    from graspldm_amd._cache import cached_value
    return cached_value(owner, slot) if slot in owner.__dict__ else None


def _one_per_trailing_name(keys, always=()):
    """One tensor per distinct trailing key name (last two dotted components), first and last occurrence, plus `always`."""
    seen = {}
    for k in keys:
        seen.setdefault(".".join(k.split(".")[-2:]), [k, k])[1] = k
    pick = {k for pair in seen.values() for k in pair} | {k for k in keys if k.startswith(tuple(always))}
    return [k for k in keys if k in pick]


class Owner:
    """One row of the table: a constructor, the smallest input that takes the cached route, the call, the proof that the
    route was taken, the f64 restatement and its bar."""

    def __init__(self, ctor, inputs, call, route, ref, bar=2e-5, mode="split", keys=None, seed=3, load=None, f64_outputs=None):
        self.ctor, self.inputs, self.call, self.route, self.ref, self.bar = ctor, inputs, call, route, ref, bar
        self.mode, self.keys, self.seed, self.load = mode, keys or (lambda ks: ks), seed, load
        self.f64_outputs = f64_outputs   # how many of the call's outputs the f64 comparison behind the sweep takes (None: all)

    def fresh(self):
        return self.ctor().cuda().eval()

    def make(self):
        from graspldm_amd.synthetic import load_synthetic_weights
        m = self.ctor()
        if self.load is not None:
            self.load(m)
        else:
            load_synthetic_weights(m, seed=self.seed)
        return m.cuda().eval()

    def twin(self, module):
        """Same constructor, the module's state_dict, never run."""
        t = self.fresh()
        t.load_state_dict(module.state_dict())
        return t


# ---------------------------------------------------------------------------------------------------- dense layers
def _mlp_row(cin, cout, n, want, mode="split"):
    from graspldm_amd.pvcnn import SharedMLP

    def route(m, x):
        from graspldm_amd import dense
        conv, bn = m.layers[0], m.layers[1]
        f = _value(conv, "_gldm_folded")
        assert f is not None and dense.folded_conv_bn(conv, bn, x.device) is f, "no folded layer kept on the conv"
        fused = f.wp is not None and dense.fused_mlp_supported(x, cin, cout)
        if fused:
            got = "split" if f.ws_main is not None and dense.split_supported(cin) else "f32"
        elif f.wp is None and f.ws_main is not None and dense.split_mlp_supported(x, cin, cout):
            got = "split-padded"
        else:
            got = "small" if cin in dense.SMALL_CIN else "any"
        assert got == want, f"{cin} -> {cout} at n = {n} ran the {got} launch, not the {want} one"

    def ref(m, x):
        from oracle import torch_ref as R
        return (R.shared_mlp(_sd(m, torch.float64), "", x.double()),)
    return Owner(lambda: SharedMLP(cin, cout), lambda: (torch.randn(2, cin, n, generator=torch.Generator().manual_seed(cin + n)),),
                 lambda m, x: m(x), route, ref, mode=mode)


def _concat_key_tail(conv):
    from graspldm_amd._cache import cached_key
    return tuple(cached_key(conv, "_gldm_concat")[1:])


def _concat_narrow_row():
    """xa [B, 128, N] wide, xb [B, 3, N] a few rows."""
    from graspldm_amd.pvcnn import SharedMLP

    def call(m, xa, xb):
        from graspldm_amd import dense
        y = dense.concat_conv_bn_relu(xa, xb, m.layers[0], m.layers[1])
        if not _split_on():   # under f32_only() there is no such launch: the caller concatenates (pvcnn._first_layer_of_concat)
            assert y is None
            return m(torch.cat([xa, xb], dim=1))
        assert y is not None, "the narrow-addend form fell back to the concatenation"
        return y

    def route(m, xa, xb):
        assert _value(m.layers[0], "_gldm_concat") is not None and _concat_key_tail(m.layers[0]) == (128, False, False)

    def ref(m, xa, xb):
        from oracle import torch_ref as R
        return (R.shared_mlp(_sd(m, torch.float64), "", torch.cat([xa, xb], dim=1).double()),)

    def inputs():
        g = torch.Generator().manual_seed(31)
        return torch.randn(2, 128, 64, generator=g), torch.randn(2, 3, 64, generator=g)
    return Owner(lambda: SharedMLP(131, 128), inputs, call, route, ref)


def _concat_three_forms_row():
    """One conv 384 -> 256, its ONE `_gldm_concat` slot, two forms in the order A, B, A: A = broadcast (xa [B, 256, 1]),
    B = both wide (xa [B, 256, N]).  Each call evicts the other's entry; the third equals the first bitwise."""
    from graspldm_amd.pvcnn import SharedMLP

    def call(m, xa1, xa, xb):
        from graspldm_amd import dense
        conv, bn = m.layers[0], m.layers[1]
        if not _split_on():   # under f32_only() there is no such launch: the caller concatenates (pvcnn._first_layer_of_concat)
            assert dense.concat_conv_bn_relu(xa1, xb, conv, bn) is None and dense.concat_conv_bn_relu(xa, xb, conv, bn) is None
            return m(torch.cat([xa1.expand(-1, -1, xb.shape[2]), xb], dim=1)), m(torch.cat([xa, xb], dim=1))
        a = dense.concat_conv_bn_relu(xa1, xb, conv, bn)
        assert a is not None and _concat_key_tail(conv) == (256, True, False), "broadcast form not taken"
        b = dense.concat_conv_bn_relu(xa, xb, conv, bn)
        assert b is not None and _concat_key_tail(conv) == (256, False, True), "both-wide form not taken"
        a2 = dense.concat_conv_bn_relu(xa1, xb, conv, bn)
        assert _concat_key_tail(conv) == (256, True, False)
        assert torch.equal(a2, a), "A, B, A on one slot: the third call differs from the first"
        return a, b

    def route(m, xa1, xa, xb):
        assert _value(m.layers[0], "_gldm_concat") is not None and _value(m.layers[0], "_gldm_folded") is not None

    def ref(m, xa1, xa, xb):
        from oracle import torch_ref as R
        sd = _sd(m, torch.float64)
        return (R.shared_mlp(sd, "", torch.cat([xa1.expand(-1, -1, xb.shape[2]), xb], dim=1).double()),
                R.shared_mlp(sd, "", torch.cat([xa, xb], dim=1).double()))

    def inputs():
        g = torch.Generator().manual_seed(32)
        return torch.randn(2, 256, 1, generator=g), torch.randn(2, 256, 64, generator=g), torch.randn(2, 128, 64, generator=g)
    return Owner(lambda: SharedMLP(384, 256), inputs, call, route, ref)


# ---------------------------------------------------------------------------------------------------- attention
def _conv1x1_row():
    def call(m, x):
        from graspldm_amd.attention import conv1x1
        return conv1x1(x, m)

    def route(m, x):
        assert _value(m, "_gldm_k1") is not None, "no packed conv kept on the module"

    def ref(m, x):
        sd = _sd(m, torch.float64)
        return (F.conv1d(x.double(), sd["weight"], sd["bias"]),)
    return Owner(lambda: nn.Conv1d(64, 64, 1), lambda: (torch.randn(2, 64, 192, generator=torch.Generator().manual_seed(41)),),
                 call, route, ref)


def _attention_ref(m, x):
    from test_attention_gpu import block_ref
    return (block_ref(x.double(), _sd(m, torch.float64)),)


def _attention_row(c, d, shape, seed):
    from graspldm_amd.attention import Attention

    def route(m, x):
        assert _value(m, "_gldm_attn") is not None, "no folded attention convs kept on the module"
    return Owner(lambda: Attention(c, 8, D=d), lambda: (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)),),
                 lambda m, x: m(x), route, _attention_ref)


# ---------------------------------------------------------------------------------------------------- classifier head
def _classifier():
    from graspldm_amd.builder import build_model_from_cfg
    from graspldm_amd.pipeline import classifier_model_config
    return build_model_from_cfg(classifier_model_config(64, 12))


def _head_ref(m, x):
    from oracle import torch_ref as R
    sd = _sd(m, torch.float64)
    y = R.shared_mlp(sd, "classifier.0.", x.double())
    z = F.conv1d(y, sd["classifier.2.weight"], sd["classifier.2.bias"])
    logit = F.linear(z, sd["classifier.3.weight"], sd["classifier.3.bias"]).reshape(x.shape[0])
    return logit, torch.sigmoid(logit)


def _head_keys(ks):
    return [k for k in ks if k.startswith("classifier.")]


def _head_row():
    """(c, rows, n) = (backbone width, 128, 76): the smallest classifier of tests/test_classifier_gpu.py, gldm_cls_head."""
    def inputs():
        c = _classifier().base_network.out_channels
        return (torch.randn(3, c, 76, generator=torch.Generator().manual_seed(5)),)

    def route(m, x):
        from graspldm_amd.grasp_classifier import cls_head_supported
        assert cls_head_supported(x.shape[1], 128, x.shape[2]) and _value(m.classifier, "_gldm_head") is not None
    return Owner(_classifier, inputs, lambda m, x: m.head(x), route, _head_ref, keys=_head_keys)


def _head_fallback_row():
    """40 feature channels: cls_head_supported rejects c % 16 != 0, the head runs as its three launches through `_gldm_folded`."""
    def ctor():
        from graspldm_amd.pvcnn import SharedMLP
        m = _classifier()
        m.classifier = nn.Sequential(SharedMLP(40, 128), nn.Dropout(0.5), nn.Conv1d(128, 1, 1), nn.Linear(76, 1))
        return m

    def route(m, x):
        from graspldm_amd.grasp_classifier import cls_head_supported
        assert not cls_head_supported(40, 128, 76) and "_gldm_head" not in m.classifier.__dict__
        assert _value(m.classifier[0].layers[0], "_gldm_folded") is not None
    return Owner(ctor, lambda: (torch.randn(3, 40, 76, generator=torch.Generator().manual_seed(6)),), lambda m, x: m.head(x), route,
                 _head_ref, keys=_head_keys)


# ---------------------------------------------------------------------------------------------------- the encoder's head
def _encoder_row():
    """The shipped PVCNNEncoder on 2 x 1024 points: the two wide layers in front of the head and the folded head, one launch."""
    def ctor():
        from graspldm_amd.pc_encoders import PVCNNEncoder
        return PVCNNEncoder(in_features=3, out_features=64, n_points=1024, scale_channels=0.75, scale_voxel_resolution=0.75,
                            num_blocks=(1, 1, 1, 1), out_channels=3)

    def inputs():
        from graspldm_amd.synthetic import synthetic_batch
        return (synthetic_batch(2, 1024)[0],)

    def wide(m):
        from graspldm_amd.pvcnn import SharedMLP
        idx = [i for i, layer in enumerate(m.pvcnn_modules.point_features) if isinstance(layer, SharedMLP)][-2:]
        assert len(idx) == 2
        return idx

    def keys(ks):
        pre = ("conv_downscale.", "out_layer.0.") + tuple(f"pvcnn_modules.point_features.{i}.layers." for i in wide(ctor()))
        return [k for k in ks if k.startswith(pre)]

    def route(m, pc):
        assert _value(m, "_head_cache") is not None and _value(m, "_head_packed") is not None, "the folded head was not packed"
        for i in wide(m):
            assert _value(m.pvcnn_modules.point_features[i].layers[0], "_gldm_folded") is not None

    def ref(m, pc):
        from oracle import torch_ref as R
        return (R.pvcnn_encoder_forward(_sd(m), "", pc, R.pvcnn_block_spec(0.75, 0.75)),)   # the oracle's C kernels are f32
    return Owner(ctor, inputs, lambda m, pc: m(pc), route, ref, keys=keys, seed=0)


# ---------------------------------------------------------------------------------------------------- set abstraction
def _ref_sa(m, feats, coords, radii, ks):
    """oracle.torch_ref.sa_module with the grouped MLP in f64 (the gather and the centre subtraction are the oracle's, f32)."""
    from oracle import torch_ref as R
    sd = _sd(m, torch.float64)
    centers = R.furthest_point_sample(coords, m.num_centers)
    outs = [R.shared_mlp(sd, f"mlps.{g}.", R.ball_group(coords, centers, feats, rad, k).double()).max(dim=-1).values
            for g, (rad, k) in enumerate(zip(radii, ks))]
    return (torch.cat(outs, dim=1),)


def _sa_plans(m):
    plans = [_value(mlp, "_sa_plan") for mlp in m.mlps]
    assert all(p is not None for p in plans), "a branch ran without its fused plan"
    return plans


def _sa_row(mode):
    """(b, c, n, m, u) = (1, 5, 300, 37, 16), widths (16, 32, 32, 64): tests/test_models_gpu.py, one scale."""
    from graspldm_amd.pvcnn import PointNetSAModule

    def inputs():
        g = torch.Generator().manual_seed(2)
        coords = (torch.rand(1, 3, 300, generator=g) * 2 - 1).contiguous()
        return torch.randn(1, 5, 300, generator=g), coords

    def route(m, feats, coords):
        plan, = _sa_plans(m)
        split = _value(plan, "_split") is not None or _value(plan, "_pre") is not None
        assert split == (mode == "split"), f"split tables packed: {split} under mode {mode}"
    return Owner(lambda: PointNetSAModule(num_centers=37, radius=0.35, num_neighbors=16, in_channels=5, out_channels=(16, 32, 32, 64)),
                 inputs, lambda m, f, c: m((f, c))[0], route, lambda m, f, c: _ref_sa(m, f, c, [0.35], [16]), mode=mode, seed=11)


def _msg_row(which):
    """The multi-scale modules of tests/test_msg_gpu.py: SA1 (two scales) and SA2 (one scale of 128 neighbours, 192 feature
    channels): the hoisted first layer (`_pre`) and, where the per-point layer takes the split launch, its fragments (`_pre_ws`)."""
    import test_msg_gpu as T
    from graspldm_amd.pvcnn import PointNetSAModule
    kw = dict(T.SA1 if which == 1 else T.SA2)

    def inputs():
        n, c = (256, 5) if which == 1 else (64, 192)
        return (torch.randn(2, c, n, generator=torch.Generator().manual_seed(53)), torch.stack([T._cloud(i, n) for i in (0, 1)]))

    def route(m, feats, coords):
        plans = _sa_plans(m)
        assert any(_value(p, "_pre") is not None for p in plans), "no branch hoisted its first layer"
        if which == 2:
            assert _value(plans[0], "_pre_ws") is not None, "the per-point layer did not take the split launch"
    return Owner(lambda: PointNetSAModule(**kw), inputs, lambda m, f, c: m((f, c))[0], route,
                 lambda m, f, c: _ref_sa(m, f, c, kw["radius"], kw["num_neighbors"]), seed=10 + which)


# ---------------------------------------------------------------------------------------------------- PVConv
def _ref_pvconv(m, feats, coords, r, attention, se_relu):
    """oracle.torch_ref.pvconv with the voxel stack in f64 (voxelize / devoxelize are the oracle's f32 C kernels); with
    attention, the block of tests/test_attention_gpu.py in place of the second Swish (pvconv.py:57-83)."""
    from oracle import torch_ref as R
    from oracle.cpu_backend import _backend as B
    sd = _sd(m, torch.float64)
    p = lambda k: sd["voxel_layers." + k]   # noqa: E731
    vox, nc = R.voxelize(feats, coords, r, True)
    h = F.group_norm(F.conv3d(vox.double(), p("0.weight"), p("0.bias"), padding=1), 8, p("1.weight"), p("1.bias"), 1e-5)
    h = h * torch.sigmoid(h)
    h = F.group_norm(F.conv3d(h, p("4.weight"), p("4.bias"), padding=1), 8, p("5.weight"), p("5.bias"), 1e-5)
    if attention:
        from test_attention_gpu import block_ref
        h = block_ref(h, sd, pre="voxel_layers.6.")
    else:
        h = h * torch.sigmoid(h)
    s = F.linear(h.mean(dim=(2, 3, 4)), p("7.fc.0.weight"))
    gate = torch.sigmoid(F.linear(torch.relu(s) if se_relu else s * torch.sigmoid(s), p("7.fc.2.weight")))
    h = (h * gate[:, :, None, None, None]).float().contiguous()
    dv = B.trilinear_devoxelize_forward(r, False, nc.contiguous(), h.view(h.shape[0], h.shape[1], -1))[0]
    return (dv.double() + R.shared_mlp(sd, "point_features.", feats.double()),)


def _pvconv_row(cin, cout, r, want, mode="split"):
    from graspldm_amd.pvcnn import PVConv

    def inputs():
        g = torch.Generator().manual_seed(cin + r)
        return torch.randn(2, cin, 100, generator=g), torch.rand(2, 3, 100, generator=g) * 2 - 1

    def route(m, feats, coords):
        plan = _value(m, "_voxel_plan")
        assert plan is not None, "no voxel plan kept on the module"
        got = ["generic" if g else "split" if s else "f32" for s, g in zip(plan.split, plan.generic)]
        assert got == [want, want], f"the convs ran as {got}, not {want}"
        assert _value(m.point_features.layers[0], "_gldm_folded") is not None
    return Owner(lambda: PVConv(cin, cout, 3, resolution=r, with_se=True), inputs, lambda m, f, c: m((f, c))[0], route,
                 lambda m, f, c: _ref_pvconv(m, f, c, r, False, False), mode=mode)


def _pvconv_attention_row():
    """use_attention=True at r = 4, the smallest resolution of tests/test_voxel_attention_gpu.py, on its inputs."""
    from graspldm_amd.pvcnn import PVConv

    def inputs():
        from test_voxel_attention_gpu import pvconv_inputs
        return pvconv_inputs()

    def route(m, feats, coords):
        assert _value(m, "_voxel_plan") is not None and _value(m.voxel_layers[6], "_gldm_attn") is not None
    return Owner(lambda: PVConv(32, 32, 3, resolution=4, use_attention=True, with_se=True, with_se_relu=True), inputs,
                 lambda m, f, c: m((f, c))[0], route, lambda m, f, c: _ref_pvconv(m, f, c, 4, True, True), seed=0)


# ---------------------------------------------------------------------------------------------------- the 1-D engines
def _engine_route(slots=("_engine",)):
    def route(m, *x):
        for path in slots:
            owner = m
            *mods, slot = path.split(".")
            for name in mods:
                owner = getattr(owner, name)
            assert _value(owner, slot) is not None, f"no engine kept in {path}"
    return route


def _cond(n=N1D, seed=5):
    return torch.randn(n, 3, 64, generator=torch.Generator().manual_seed(seed))


def _resnet1d_row():
    from graspldm_amd.resnets import ResNet1D

    def ref(m, x, z):
        from oracle import torch_ref as R
        return (R.resnet1d_forward(_sd(m, torch.float64), "", x.double(), z_cond=z.double()),)
    return Owner(lambda: ResNet1D(dim=16, **RN), lambda: (torch.randn(N1D, 1, 16, generator=torch.Generator().manual_seed(8)), _cond()),
                 lambda m, x, z: m(x, z_cond=z), _engine_route(), ref, bar=5e-6, keys=_one_per_trailing_name, seed=7)


def _time_resnet_row(dim, shipped):
    """dim 4: the shipped denoiser with the fpc recipe weights; dim 16: the 16-position net of tests/test_range_gpu.py."""
    from graspldm_amd.resnets import TimeConditionedResNet1D

    def load(m):
        from conftest import load_schema
        from graspldm_amd.synthetic import synthetic_state_dict
        p = "diffusion_model.model."
        sd = synthetic_state_dict(load_schema("schema_fpc_ldm.json"), seed=0)
        m.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)}, strict=True)

    def inputs():
        g = torch.Generator().manual_seed(5 + dim)
        return torch.randn(N1D, 1, dim, generator=g), torch.randint(0, 1000, (N1D,), generator=g), _cond()

    def ref(m, x, t, z):
        # the f64 yardstick is fed the f32 time-embedding rows, as tests/test_unet1d_gpu.py feeds its own: the module defines
        # sin / cos of t w 2 pi in f32 (arguments up to 1e4 rad), and with the swept time_mlp weights (rows up to 445) the f64
        # evaluation of that alone sits 4.0e-3 from it at max |ref| = 822 (measured on the CPU), the size of the bar
        from oracle import torch_ref as R
        temb = R.time_embedding(_sd(m), "", t).double()
        return (R.resnet1d_forward(_sd(m, torch.float64), "", x.double(), z_cond=z.double(), temb=temb),)
    return Owner(lambda: TimeConditionedResNet1D(dim=dim, channels=1, is_time_conditioned=True, learned_variance=False,
                                                 learned_sinusoidal_cond=False, random_fourier_features=True, **RN),
                 inputs, lambda m, x, t, z: m(x, time=t, z_cond=z), _engine_route(), ref, bar=5e-6, keys=_one_per_trailing_name,
                 seed=7, load=load if shipped else None)


def _unet_row():
    """Configuration A of tests/unet1d_ref.py (the VAE cores' shape) at L = 16."""
    import unet1d_ref as U
    from graspldm_amd.resnets import Unet1D

    def ref(m, x, z):
        return (U.unet1d_forward(_sd(m, torch.float64), "", x.double(), z.double(), None, groups=4),)
    return Owner(lambda: Unet1D(**U.CASES["A"]["args"]), lambda: U.case_inputs("A", N1D)[:2], lambda m, x, z: m(x, z_cond=z),
                 _engine_route(), ref, bar=2e-5, keys=_one_per_trailing_name, seed=21)


def _core_forward(sd, prefix, core, h, z):
    from oracle import torch_ref as R
    if core == "ResNet1D":
        return R.resnet1d_forward(sd, prefix, h, z_cond=z, groups=4)
    import unet1d_ref as U
    return U.unet1d_forward(sd, prefix, h, z, None, groups=4)


def _decoder_row(core):
    from graspldm_amd.grasp_vae import ConditionalGraspPoseDecoder
    args = RN if core == "ResNet1D" else UN

    def ref(m, zh, z):
        sd = _sd(m, torch.float64)
        h = F.linear(zh.double(), sd["in_layer.weight"], sd["in_layer.bias"]).unsqueeze(-2)
        h = _core_forward(sd, "net.", core, h, z.double()).squeeze(-2)
        return F.linear(h, sd["tmrp.weight"], sd["tmrp.bias"]), F.linear(h, sd["class_logits.weight"], sd["class_logits.bias"])
    return Owner(lambda: ConditionalGraspPoseDecoder(dict(type=core, args=dict(args)), in_features=4, feature_resolution=16),
                 lambda: (torch.randn(N1D, 4, generator=torch.Generator().manual_seed(9)), _cond()),
                 lambda m, zh, z: m(zh, cond=z), _engine_route(), ref, bar=5e-6 if core == "ResNet1D" else 2e-5,
                 keys=lambda ks: _one_per_trailing_name(ks, always=("in_layer.", "tmrp.", "class_logits.")), seed=0)


ENC = "encoder.grasp_encoder."


def _vae_encoder_row(core):
    """GraspCVAE on one 64-point cloud and 11 grasps: grasp_encoder.forward() (the out_layer-only engine) and GraspCVAE.encode
    (the engine fused with the bottleneck) alternate on every run; forward() is asked again behind encode and must repeat."""
    def ctor():
        from graspldm_amd.builder import build_model_from_cfg
        from graspldm_amd.pipeline import fpc_model_config
        return build_model_from_cfg(fpc_model_config(n_points=64, vae_core=core)["vae"])

    def inputs():
        from graspldm_amd.synthetic import synthetic_batch
        g = torch.Generator().manual_seed(12)
        return synthetic_batch(1, 64)[0], torch.randn(N1D, 7, generator=g), torch.randn(N1D, 4, generator=g)

    def call(m, pc, h, eps):
        z_pc = m.encode_pc(pc)
        ge = m.encoder.grasp_encoder
        plain = ge(h.unsqueeze(1), cond=z_pc, samples_per_cond=N1D)
        (mu, logvar, z), _ = m.encode(pc, h, eps=eps)
        assert torch.equal(ge(h.unsqueeze(1), cond=z_pc, samples_per_cond=N1D), plain), "forward() differs behind encode()"
        return plain, mu, logvar, z

    def keys(ks):
        return _one_per_trailing_name([k for k in ks if k.startswith((ENC, "bottleneck."))],
                                      always=(ENC + "in_layer.", ENC + "out_layer.", "bottleneck."))

    def ref(m, pc, h, eps):
        sd = _sd(m, torch.float64)
        with torch.no_grad():
            z_pc = m.encode_pc(pc.cuda()).cpu().double().repeat_interleave(N1D, dim=0)   # the cloud latent is the module's own
        x = F.linear(h.double(), sd[ENC + "in_layer.weight"], sd[ENC + "in_layer.bias"]).unsqueeze(-2)
        x = _core_forward(sd, ENC + "net.", core, x, z_pc).squeeze(-2)
        out = F.linear(x, sd[ENC + "out_layer.weight"], sd[ENC + "out_layer.bias"])
        mu = F.linear(out, sd["bottleneck.mu.weight"], sd["bottleneck.mu.bias"])
        logvar = F.linear(out, sd["bottleneck.logvar.weight"], sd["bottleneck.logvar.bias"])
        return out.unsqueeze(-2), mu, logvar, mu + eps.double() * torch.exp(0.5 * logvar)
    # behind the sweep logvar is in the thousands and z = mu + eps exp(logvar / 2) leaves f32 (inf on both sides): z stays in
    # every bitwise comparison; against f64 it is compared at the recipe's weights (test_encoder_engines_alternate_...)
    return Owner(ctor, inputs, call, _engine_route(("encoder.grasp_encoder._engine", "encoder.grasp_encoder._engine_plain")), ref,
                 bar=5e-6 if core == "ResNet1D" else 2e-5, keys=keys, seed=0, f64_outputs=3)


OWNERS = {
    # SharedMLP / pointwise_conv_bn_relu: one shape per branch of dense.pointwise_conv_bn_relu
    "pointwise-split-128x256-n96": lambda: _mlp_row(128, 256, 96, "split"),
    "pointwise-f32-128x256-n96": lambda: _mlp_row(128, 256, 96, "f32", mode="f32"),
    "pointwise-small-3x48-n96": lambda: _mlp_row(3, 48, 96, "small"),
    "pointwise-small-6x17-n90": lambda: _mlp_row(6, 17, 90, "small"),   # 6 input rows have a lane-per-point instantiation
    "pointwise-any-7x17-n90": lambda: _mlp_row(7, 17, 90, "any"),       # the any-shape kernel: an input width without one
    "concat-narrow-128+3x128": _concat_narrow_row,
    "concat-broadcast-wide-broadcast-384x256": _concat_three_forms_row,
    "conv1x1-64x64-n192": _conv1x1_row,
    "attention-1d": lambda: _attention_row(64, 1, (2, 64, 192), 41),
    "attention-3d": lambda: _attention_row(32, 3, (2, 32, 4, 4, 4), 43),
    "classifier-head": _head_row,
    "classifier-head-fallback": _head_fallback_row,
    "pvcnn-encoder-2x1024": _encoder_row,
    "sa-1x5x300x37x16": lambda: _sa_row("split"),
    "sa-1x5x300x37x16-f32": lambda: _sa_row("f32"),
    "sa-msg-two-scales": lambda: _msg_row(1),
    "sa-msg-192-channels-u128": lambda: _msg_row(2),
    "pvconv-128x128-r4": lambda: _pvconv_row(128, 128, 4, "split"),
    "pvconv-48x96-r12": lambda: _pvconv_row(48, 96, 12, "split"),
    "pvconv-128x128-r4-f32": lambda: _pvconv_row(128, 128, 4, "f32", mode="f32"),
    "pvconv-48x96-r12-f32": lambda: _pvconv_row(48, 96, 12, "f32", mode="f32"),
    "pvconv-16x32-r5-generic": lambda: _pvconv_row(16, 32, 5, "generic"),
    "pvconv-attention-32x32-r4": _pvconv_attention_row,
    "resnet1d": _resnet1d_row,
    "denoiser-4-shipped": lambda: _time_resnet_row(4, True),
    "time-resnet1d-16": lambda: _time_resnet_row(16, False),
    "unet1d-A": _unet_row,
    "decoder-resnet1d": lambda: _decoder_row("ResNet1D"),
    "decoder-unet1d": lambda: _decoder_row("Unet1D"),
    "vae-encoder-resnet1d": lambda: _vae_encoder_row("ResNet1D"),
    "vae-encoder-unet1d": lambda: _vae_encoder_row("Unet1D"),
}


def _runner(o):
    x = tuple(t.cuda() for t in o.inputs())
    return x, (lambda m: _tuple(o.call(m, *x)))


def _check_f64(name, o, module, got, count=None):
    x = o.inputs()
    worst = 0.0
    for i, (y, ref) in enumerate(list(zip(got, o.ref(module, *x)))[:count]):
        assert torch.isfinite(y).all(), f"{name}: output {i} is not finite"
        ref = ref.double()
        err, bar = float((y.cpu().double() - ref).abs().max()), o.bar * max(1.0, float(ref.abs().max()))
        print(f"{name}: output {i} against f64: max err {err:.3e} (bar {bar:.1e}, max |ref| {float(ref.abs().max()):.3f})")
        assert err <= bar, (name, i, err, bar)
        worst = max(worst, err / bar)
    return worst


# the owners with the most tensors and the dearest twins are swept in two halves (even and odd picks), a case each
_HALVES = ("vae-encoder-", "decoder-", "unet1d-")
SWEEPS = [(n, part, 2 if n.startswith(_HALVES) else 1) for n in sorted(OWNERS) for part in range(2 if n.startswith(_HALVES) else 1)]


@pytest.mark.parametrize("name,part,parts", SWEEPS, ids=[n if ps == 1 else f"{n}-{p + 1}of{ps}" for n, p, ps in SWEEPS])
def test_every_tensor_reaches_the_next_forward(name, part, parts):
    o = OWNERS[name]()
    with _mode(o.mode), torch.no_grad():
        m = o.make()
        x, run = _runner(o)
        y0 = run(m)
        o.route(m, *x)
        state = _floating(m)
        keys = o.keys(list(state))[part::parts]
        assert keys, "nothing to sweep"
        prev = y0
        for k in keys:
            _perturb(state[k])
            y1 = run(m)
            assert _same(y1, run(o.twin(m))), f"{name}: after a change of {k} the module and a fresh twin with its weights differ"
            if k in NO_EFFECT.get(name, ()):
                assert _same(y1, prev), f"{name}: {k} is listed as without effect but moved the output"
            else:
                assert not _same(y1, y0) and not _same(y1, prev), f"{name}: a change of {k} did not move the output"
            prev = y1
        o.route(m, *x)
        print(f"{name}: swept {len(keys)} of {len(state)} floating tensors")
        _check_f64(name, o, m, prev, o.f64_outputs)


@pytest.mark.parametrize("name", sorted(NO_EFFECT))
def test_no_effect_entries_are_justified(name):
    """Each NO_EFFECT tensor, changed alone, leaves the owner's f64 restatement where it was (to f64 rounding), while the first
    other tensor of the module moves it: the restatement can see a change."""
    o = OWNERS[name]()
    m = o.ctor()
    from graspldm_amd.synthetic import load_synthetic_weights
    load_synthetic_weights(m, seed=o.seed).eval()
    x = o.inputs()
    base = o.ref(m, *x)
    state = _floating(m)
    for k in sorted(NO_EFFECT[name]):
        _perturb(state[k])
        moved = max(float((a - b).abs().max()) for a, b in zip(o.ref(m, *x), base))
        assert moved <= 1e-12 * max(1.0, max(float(b.abs().max()) for b in base)), (k, moved)
    other = next(k for k in state if k not in NO_EFFECT[name] and k.endswith(".bias"))
    _perturb(state[other])
    assert max(float((a - b).abs().max()) for a, b in zip(o.ref(m, *x), base)) > 1e-6, other


def _first_parameter(o, module):
    state = _floating(module)
    return next(k for k in o.keys(list(state)) if isinstance(state[k], nn.Parameter) and k.endswith("weight"))


@pytest.mark.parametrize("name", sorted(OWNERS))
def test_weights_changed_by_other_means(name):
    """Once per owner: numerics.f32_only() entered and left, copy.deepcopy after the first forward, load_state_dict of a
    second state dict, one SGD step, p.data.mul_(2) + invalidate_caches(), and a device round trip; each against a fresh twin."""
    import graspldm_amd
    from graspldm_amd import numerics
    from graspldm_amd.synthetic import synthetic_state_dict
    o = OWNERS[name]()
    with _mode(o.mode), torch.no_grad():
        m = o.make()
        x, run = _runner(o)
        y0 = run(m)
        o.route(m, *x)
        key = _first_parameter(o, m)
        if o.mode == "split":
            with numerics.f32_only():
                assert _same(run(m), run(o.twin(m))), f"{name}: under f32_only() the module and a twin built there differ"
            assert _same(run(m), y0), f"{name}: the output after leaving f32_only() is not the one before entering"
        c = copy.deepcopy(m)
        _perturb(_floating(c)[key])
        yc = run(c)
        assert _same(yc, run(o.twin(c))) and not _same(yc, y0), f"{name}: the deep copy does not follow its own {key}"
        assert _same(run(m), y0), f"{name}: a change to the deep copy reached the original"
        del c
        m.load_state_dict({k: v.cuda() for k, v in synthetic_state_dict(_sd(m), seed=o.seed + 1).items()})
        y = run(m)
        assert _same(y, run(o.twin(m))) and not _same(y, y0), f"{name}: load_state_dict of a second state dict"
        p = _floating(m)[key]
        p.grad = 0.5 * p.detach()   # p <- 0.75 p (a constant gradient would push a whole layer behind its ReLU)
        torch.optim.SGD([p], lr=0.5).step()
        p.grad = None
        prev, y = y, run(m)
        assert _same(y, run(o.twin(m))) and not _same(y, prev), f"{name}: one SGD step on {key}"
        p.data.mul_(2)
        graspldm_amd.invalidate_caches()
        prev, y = y, run(m)
        assert _same(y, run(o.twin(m))) and not _same(y, prev), f"{name}: p.data.mul_(2) + invalidate_caches() on {key}"
        m.cpu().cuda()
        assert _same(run(m), y) and _same(y, run(o.twin(m))), f"{name}: after .cpu().cuda()"
        o.route(m, *x)


# ---------------------------------------------------------------------------------------------------- engine-only cases
@pytest.mark.parametrize("name", ["resnet1d", "denoiser-4-shipped", "decoder-resnet1d", "decoder-unet1d"])
def test_conditioning_rows_one_three_one(name):
    """z_cond as [n, Dc], then [n, 3, Dc], then [n, Dc]: the engine is packed per row count; the third call equals the first,
    and each equals a twin that only ever saw that form."""
    o = OWNERS[name]()
    with torch.no_grad():
        m = o.make()
        *head, z3 = (t.cuda() for t in o.inputs())
        z1 = z3[:, 0].contiguous()
        a = _tuple(o.call(m, *head, z1))
        b = _tuple(o.call(m, *head, z3))
        a2 = _tuple(o.call(m, *head, z1))
        assert _same(a2, a) and not _same(a, b)
        assert _same(a, _tuple(o.call(o.twin(m), *head, z1))) and _same(b, _tuple(o.call(o.twin(m), *head, z3)))


def test_unet1d_sequence_lengths_a_b_a_with_a_weight_change():
    """One Unet1D at L = 16, then 8, then 16 (UnetEngine keeps one plan per length), with a weight change between the last
    two: both lengths follow the change."""
    import unet1d_ref as U
    o = OWNERS["unet1d-A"]()
    with torch.no_grad():
        m = o.make()
        x16, z = (t.cuda() for t in o.inputs())
        x8 = x16[:, :, :8].contiguous()
        a, b = m(x16, z_cond=z), m(x8, z_cond=z)
        assert len(_value(m, "_engine")._plans) == 2
        _perturb(_floating(m)["mid_block1.block1.proj.weight"])
        a2, b2 = m(x16, z_cond=z), m(x8, z_cond=z)
        t = o.twin(m)
        assert torch.equal(b2, t(x8, z_cond=z)) and torch.equal(a2, t(x16, z_cond=z))
        assert not torch.equal(a2, a) and not torch.equal(b2, b)
        ref = U.unet1d_forward(_sd(m, torch.float64), "", x8.cpu().double(), z.cpu().double(), None, groups=4)
        err, bar = float((b2.cpu().double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
        print(f"Unet1D A at L = 8 after the change: max err {err:.3e} (bar {bar:.1e})")
        assert err <= bar, (err, bar)


def test_encoder_engines_alternate_under_bottleneck_and_out_layer_changes():
    """ConditionalGraspPoseEncoder keeps two engines under two keys.  A bottleneck tensor moves GraspCVAE.encode alone; an
    out_layer tensor moves both; neither call serves the other's entry."""
    for core in ("ResNet1D", "Unet1D"):
        o = OWNERS["vae-encoder-" + core.lower()]()
        with torch.no_grad():
            m = o.make()
            x, run = _runner(o)
            y0 = run(m)
            _check_f64("vae-encoder-" + core.lower() + " (recipe weights)", o, m, y0)
            _perturb(_floating(m)["bottleneck.mu.weight"])
            y1 = run(m)
            assert torch.equal(y1[0], y0[0]) and not torch.equal(y1[1], y0[1]) and torch.equal(y1[2], y0[2]), core
            _perturb(_floating(m)[ENC + "out_layer.bias"])
            y2 = run(m)
            assert all(not torch.equal(a, b) for a, b in zip(y2, y1)), core
            assert _same(y2, run(o.twin(m))), core


def test_ldm_inference_timesteps_three_five_three():
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    pcs = synthetic_batch(1, 64)[0].cuda()
    x_t = torch.randn(4, 1, 4, generator=torch.Generator().manual_seed(7))

    def run(ldm, steps):
        ldm.set_inference_timesteps(steps)
        (tm, lg), _ = ldm.generate_grasps(pcs, num_grasps=4, x_T=x_t)
        ldm.check_engines()
        return tm, lg
    ldm = build_fpc_ldm(n_points=64, device="cuda")
    a, b, a2 = run(ldm, 3), run(ldm, 5), run(ldm, 3)
    assert _same(a2, a) and not _same(a, b)
    assert _same(b, run(build_fpc_ldm(n_points=64, device="cuda"), 5)), "five steps behind three differ from five steps alone"
