"""CPU: the derived-weight caches' key (graspldm_amd/_cache.py) against the one case (data_ptr, _version) cannot tell
apart -- a NEW tensor object on the old address with the old version -- at `cached` itself and at the four 1-D engine sites
(device engines replaced by recorders); and every builder's source list against the builder: perturbing an input changes the
built value exactly when the owner's key lists that tensor.
"""
import gc

import numpy as np
import pytest
import torch
from torch import nn

from graspldm_amd import _cache

CPU = torch.device("cpu")


def _rewrap(arr, fill):
    """A fresh Parameter over `arr` after overwriting it: the address and the version (0) of every earlier wrap of `arr`."""
    arr[...] = fill
    return nn.Parameter(torch.from_numpy(arr))


def test_same_address_same_version_new_tensor_rebuilds():
    """del + assignment, load_state_dict(assign=True) and dtype round trips replace Parameter objects; the allocator may hand
    the new one the freed address.  Made deterministic with a numpy array as the storage of both."""
    arr = np.full((4, 3), 1.0, dtype=np.float32)
    conv = nn.Conv1d(3, 4, 1)
    builds = []

    def entry():
        def build():
            builds.append(float(conv.weight.detach().sum()))
            return conv.weight.detach().clone()
        return _cache.cached(conv, "_slot", _cache.params_key([conv.weight, conv.bias], CPU), build, CPU)

    del conv.weight
    conv.weight = _rewrap(arr, 1.0)
    before = (conv.weight.data_ptr(), conv.weight._version)
    first = entry()
    assert entry() is first and builds == [12.0]                     # unchanged: a hit
    del conv.weight
    gc.collect()
    conv.weight = _rewrap(arr, 2.0)
    assert (conv.weight.data_ptr(), conv.weight._version) == before  # what the old key could not tell apart
    second = entry()
    assert builds == [12.0, 24.0] and torch.equal(second, conv.weight) and second is not first
    assert entry() is second and len(builds) == 2
    # the other tensor of the list, and the contract that stays: p.data writes need invalidate()
    conv.weight.data.mul_(2)
    assert entry() is second
    _cache.invalidate()
    assert entry() is not second and builds[-1] == 48.0


def test_key_equality_rules():
    a, b = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(3))
    k = _cache.params_key([a, b], CPU, 7)
    assert k == _cache.params_key([a, b], CPU, 7) and not (k != _cache.params_key([a, b], CPU, 7))
    assert k != _cache.params_key([a, b], CPU, 8) and k != _cache.params_key([b, a], CPU, 7) and k != _cache.params_key([a], CPU, 7)
    assert (k, 1, True) == (_cache.params_key([a, b], CPU, 7), 1, True) and (k, 1) != (k, 2)      # derived keys (_gldm_concat)
    with torch.no_grad():
        a.add_(1)
    assert k != _cache.params_key([a, b], CPU, 7)
    k = _cache.params_key([a, b], CPU)
    del b
    gc.collect()
    assert k != k, "a key whose source died matches nothing, itself included"


def test_deepcopy_starts_without_entries():
    import copy
    conv = nn.Conv1d(3, 4, 1)
    _cache.cached(conv, "_slot", _cache.params_key([conv.weight], CPU), lambda: object(), CPU)
    twin = copy.deepcopy(conv)
    assert twin.__dict__["_slot"] is None and conv.__dict__["_slot"] is not None
    built = []
    _cache.cached(twin, "_slot", _cache.params_key([twin.weight], CPU), lambda: built.append(1), CPU)
    assert built == [1]


# ------------------------------------------------------------------------------------------ the four engine sites
class _Recorder:
    """Stands where R1dEngine / UnetEngine stand: remembers what it was built from, touches no device."""
    built = []

    def __init__(self, *args):
        self.args, self.device = args, CPU
        _Recorder.built.append(self)


@pytest.fixture()
def recorder(monkeypatch):
    from graspldm_amd import r1d, resnets, unet1d
    _Recorder.built = []
    monkeypatch.setattr(resnets, "R1dEngine", _Recorder)
    monkeypatch.setattr(r1d, "R1dEngine", _Recorder)
    monkeypatch.setattr(unet1d, "UnetEngine", _Recorder)
    return _Recorder


_RN = dict(block_channels=(32, 64, 128, 256), input_conditioning_dims=64, resnet_block_groups=4, dropout=0.1)
_UN = dict(dim_mults=(1, 2), input_conditioning_dims=64, is_time_conditioned=False, resnet_block_groups=4)


def _resnet():
    from graspldm_amd.resnets import ResNet1D
    m = ResNet1D(dim=16, **_RN)
    m.cond_rows = 3
    return m, m, (lambda: m.engine(CPU)), "final_conv"


def _time_resnet():
    from graspldm_amd.resnets import TimeConditionedResNet1D
    m = TimeConditionedResNet1D(dim=4, channels=1, is_time_conditioned=True, random_fourier_features=True, **_RN)
    m.cond_rows = 3
    return m, m, (lambda: m.engine(CPU)), "final_conv"


def _unet():
    from graspldm_amd.resnets import Unet1D
    m = Unet1D(dim=16, **_UN)
    return m, m, (lambda: m.engine(CPU)), "final_conv"


def _decoder(core, args):
    def make():
        from graspldm_amd.grasp_vae import ConditionalGraspPoseDecoder
        m = ConditionalGraspPoseDecoder(dict(type=core, args=args), in_features=4, feature_resolution=16)
        return m, m, (lambda: m._get_engine(CPU, 3 if core == "ResNet1D" else 1)), "tmrp"
    return make


def _encoder(core, args, fused):
    def make():
        from graspldm_amd.grasp_vae import ConditionalGraspPoseEncoder, VAEBottleneck
        m = ConditionalGraspPoseEncoder(dict(type=core, args=dict(in_features=7, **args)), latent_size=4)
        bn = VAEBottleneck(4, 4) if fused else None
        rows = 3 if core == "ResNet1D" else 1
        return m, (bn if fused else m), (lambda: m._get_engine(CPU, rows, bn)), ("mu" if fused else "out_layer")
    return make


SITES = {
    "ResNet1D.engine": _resnet,
    "TimeConditionedResNet1D.engine": _time_resnet,
    "Unet1D.engine": _unet,
    "GraspDecoder[ResNet1D]": _decoder("ResNet1D", _RN),
    "GraspDecoder[Unet1D]": _decoder("Unet1D", _UN),
    "GraspEncoder.plain[ResNet1D]": _encoder("ResNet1D", _RN, False),
    "GraspEncoder.fused[ResNet1D]": _encoder("ResNet1D", _RN, True),
    "GraspEncoder.plain[Unet1D]": _encoder("Unet1D", _UN, False),
    "GraspEncoder.fused[Unet1D]": _encoder("Unet1D", _UN, True),
}


@pytest.mark.parametrize("site", sorted(SITES))
def test_engine_sites_follow_the_same_rule(site, recorder):
    """The address-reuse construction at every engine cache: a hit while nothing changes, a rebuild for a new Parameter
    object on the old address with the old version, for an in-place update and after invalidate()."""
    import graspldm_amd
    _, holder, get, leaf = SITES[site]()
    lin = getattr(holder, leaf)
    arr = lin.weight.detach().numpy().copy()
    del lin.weight
    lin.weight = _rewrap(arr, 0.25)
    first = get()
    assert get() is first
    n = len(recorder.built)
    assert n >= 1
    before = (lin.weight.data_ptr(), lin.weight._version)
    del lin.weight
    gc.collect()
    lin.weight = _rewrap(arr, 0.5)
    assert (lin.weight.data_ptr(), lin.weight._version) == before
    second = get()
    assert second is not first, "a new tensor on the old address was served the old engine"
    assert get() is second
    with torch.no_grad():
        lin.bias.mul_(1.5)
    third = get()
    assert third is not second and get() is third
    lin.bias.data.mul_(2)
    assert get() is third
    graspldm_amd.invalidate_caches()
    assert get() is not third


def test_encoder_keeps_two_engines_apart(recorder):
    """forward() (out_layer only) and GraspCVAE.encode (fused with the bottleneck) alternate without evicting each other, and
    a bottleneck update rebuilds the fused one alone."""
    from graspldm_amd.grasp_vae import ConditionalGraspPoseEncoder, VAEBottleneck
    m = ConditionalGraspPoseEncoder(dict(type="ResNet1D", args=dict(in_features=7, **_RN)), latent_size=4)
    bn = VAEBottleneck(4, 4)
    plain, fused = m._get_engine(CPU, 3), m._get_engine(CPU, 3, bn)
    assert plain is not fused and m._get_engine(CPU, 3) is plain and m._get_engine(CPU, 3, bn) is fused
    with torch.no_grad():
        bn.mu.bias.add_(1)
    assert m._get_engine(CPU, 3) is plain and m._get_engine(CPU, 3, bn) is not fused
    with torch.no_grad():
        m.out_layer.weight.add_(1)
    assert m._get_engine(CPU, 3) is not plain
    assert m._get_engine(CPU, 1) is not m._get_engine(CPU, 3)   # the conditioning rows are part of the key


# ------------------------------------------------------------------------------------------ source lists vs builders
def _flat(value):
    if isinstance(value, torch.Tensor):
        return [value.detach().double().reshape(-1)]
    if isinstance(value, (tuple, list)):
        return [t for v in value for t in _flat(v)]
    if isinstance(value, (int, float)):
        return [torch.tensor([float(value)], dtype=torch.float64)]
    return []


def _sources_of(run, owner, slot):
    """The tensor objects of the key `run()` stores under owner.slot."""
    run()
    key = _cache.cached_key(owner, slot)
    return [r() for r in key.refs]


def _check_source_list(candidates, src, build):
    """Each candidate tensor, perturbed alone, moves build()'s value exactly when it is one of `src`."""
    base = torch.cat(_flat(build()))
    for name, t in candidates.items():
        keep = t.detach().clone()
        with torch.no_grad():
            t.mul_(1.5).add_(0.125)
        moved = not torch.equal(torch.cat(_flat(build())), base)
        with torch.no_grad():
            t.copy_(keep)
        listed = any(t is s for s in src)
        assert moved == listed, f"{name}: the builder {'reads' if moved else 'ignores'} it but the key {'lists' if listed else 'omits'} it"
    assert torch.equal(torch.cat(_flat(build())), base)


def _floating_state(*modules):
    out = {}
    for i, m in enumerate(modules):
        for k, v in m.state_dict(keep_vars=True).items():
            if v.is_floating_point():
                out[f"{i}.{k}"] = v
    return out


@pytest.mark.parametrize("bias", [True, False])
def test_source_list_fold_conv_bn(bias):
    from graspldm_amd import dense
    from graspldm_amd.synthetic import load_synthetic_weights
    conv = load_synthetic_weights(nn.Conv1d(6, 17, 1, bias=bias), seed=1)
    bn = load_synthetic_weights(nn.BatchNorm1d(17), seed=2).eval()
    src = _sources_of(lambda: dense.folded_conv_bn(conv, bn, CPU), conv, "_gldm_folded")
    assert len(src) == (6 if bias else 5)
    _check_source_list(_floating_state(conv, bn), src, lambda: dense.fold_conv_bn(conv, bn))


def test_source_list_fold_attention():
    """k.bias and the GroupNorm are outside the fold (the first by the softmax's shift invariance, the second read at launch)."""
    from graspldm_amd.attention import Attention, fold_attention
    from graspldm_amd.synthetic import load_synthetic_weights
    att = load_synthetic_weights(Attention(16, 8, D=1), seed=3).eval()
    src = _sources_of(lambda: att._packed(CPU), att, "_gldm_attn")
    assert len(src) == 7 and not any(att.k.bias is s for s in src)

    def build():
        w = lambda c: c.weight.reshape(16, 16)   # noqa: E731
        return fold_attention(w(att.q), att.q.bias, w(att.k), w(att.v), att.v.bias, w(att.out), att.out.bias)
    _check_source_list(_floating_state(att), src, build)


def test_source_list_classifier_head():
    from graspldm_amd.grasp_classifier import fold_head
    from graspldm_amd.pipeline import build_classifier
    model = build_classifier(64, 32)
    layers = model._head_layers()
    src = _sources_of(lambda: model._head_pack(CPU), model.classifier, "_gldm_head")
    _check_source_list(_floating_state(model.classifier), src, lambda: fold_head(*layers))
    # the packed form holds nothing the fold does not
    from graspldm_amd.grasp_classifier import _pack_head
    _check_source_list(_floating_state(model.classifier), src, lambda: tuple(_pack_head(*layers, CPU))[:5])


def test_source_list_encoder_folded_head():
    from graspldm_amd.pc_encoders import PVCNNEncoder
    from graspldm_amd.synthetic import load_synthetic_weights
    enc = load_synthetic_weights(PVCNNEncoder(n_points=64, out_features=8, out_channels=3), seed=4).eval()
    src = _sources_of(enc._folded_head, enc, "_head_cache")
    cand = {k: v for k, v in _floating_state(enc).items() if ".conv_downscale." in k or ".out_layer." in k}
    assert len(cand) == 6 and len(src) == 4

    def build():
        enc.__dict__.pop("_head_cache", None)
        return enc._folded_head()
    _check_source_list(cand, src, build)


# ------------------------------------------------------------------------------- the split rule lives under the same keys
def test_folded_layer_crosses_the_split_rule_in_both_directions():
    """r1d_pack.split_fits is decided inside the build the key guards: a running_var grown by 2^24 (folded rows at 2^-12)
    drops the split fragments of that weight version and keeps the f32 ones, the old statistics bring them back bit for
    bit, and nothing is re-decided while the key stands."""
    from graspldm_amd import dense
    from graspldm_amd.synthetic import load_synthetic_weights
    conv = load_synthetic_weights(nn.Conv1d(128, 256, 1), seed=1)
    bn = load_synthetic_weights(nn.BatchNorm1d(256), seed=2).eval()
    first = dense.folded_conv_bn(conv, bn, CPU)
    assert first.ws is not None and first.wp is not None and dense.folded_conv_bn(conv, bn, CPU) is first
    with torch.no_grad():
        bn.running_var.mul_(2.0 ** 24)
    small = dense.folded_conv_bn(conv, bn, CPU)
    assert small is not first and small.ws is None and small.ws_main is None and small.wp is not None
    assert dense.folded_conv_bn(conv, bn, CPU) is small
    with torch.no_grad():
        bn.running_var.mul_(2.0 ** -24)
    back = dense.folded_conv_bn(conv, bn, CPU)
    assert back is not small and torch.equal(back.ws, first.ws) and torch.equal(back.wp, first.wp)


def test_engine_crosses_the_split_rule_in_both_directions(recorder):
    """The same at an engine site: a downsample conv at 2^-12 rebuilds the engine in the exact form (no split copy named),
    the old weight rebuilds it with its split copies, and an untouched network is served from the entry."""
    m, _, get, _ = _time_resnet()
    first = get()
    packed = lambda e: e.args[0]["desc"]   # noqa: E731
    assert packed(first).lv[1].down_w3 != 0 and get() is first
    with torch.no_grad():
        m.blocks[1][3].weight.mul_(2.0 ** -12)
    small = get()
    assert small is not first and get() is small
    assert all(lv.down_w3 == 0 and lv.out_w3 == 0 and lv.qkvn_w3 == 0 for lv in packed(small).lv)
    with torch.no_grad():
        m.blocks[1][3].weight.mul_(2.0 ** 12)
    back = get()
    assert back is not small and packed(back).lv[1].down_w3 == packed(first).lv[1].down_w3
    assert torch.equal(back.args[0]["weights"], first.args[0]["weights"])
