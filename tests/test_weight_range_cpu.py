"""CPU: the small end of the split-f16 weight range (weight side).  Every hot GEMM multiplies an f32 weight
as two f16 pieces; below |w| = 2^-3 the lo piece is an f16 subnormal and the weight carries an ABSOLUTE error of 2^-25.
r1d_pack.split_fits decides per packed matrix, from the exact residual, whether the split form is accurate enough; where
it is not, the layer takes the f32 form it already takes beyond 65504.  Here: the error law of the restated arithmetic
against f64 and where the rule flips on it, the patterns the rule must and must not catch, that no shipped layer changes
route or bits, the 1-D engines' whole-network fallback, and that every family of split packers has a GPU row.
"""
import os
import re

import pytest
import torch
from torch import nn

import weight_range_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
KS = (0, 3, 5, 7, 10, 14, 20)


def _law(K, k, m=64, n=96):
    w = W.kaiming(m, K, seed=K + m) * 2.0 ** -k
    x = torch.randn(K, n, generator=torch.Generator().manual_seed(K + 1))
    ref = w.double() @ x.double()
    err = W.rel(W.restated_gemm(w, x), ref)
    model = (2.0 ** -25 * x.abs().sum(0).max() / ref.abs().max()).item()
    return w, err, model


@pytest.mark.parametrize("K", [128, 1536])
def test_error_law_and_where_the_rule_flips(K):
    """W = randn / sqrt(K) 2^-k against f64.  The model: every weight is off by at most 2^-25, so an output by at most
    2^-25 sum|x|, relative to max|ref|; the errors add like a random walk, so the measured error lies between model / sqrt(K)
    (from k = 5 on, where the weight side dominates) and the model plus the k-independent part (the activations' own split
    and the f32 accumulation: 1e-6).  split_fits says no at the first k whose restated error exceeds half the 2e-5 bar, and
    yes at the last k under a quarter of it.  Measured: K = 128 accepts k <= 4 (3.5e-6 at k = 4, 6.4e-6 at k = 5),
    K = 1536 accepts k <= 2 (2.8e-6 at k = 2, 5.5e-6 at k = 3)."""
    from graspldm_amd.r1d_pack import split_fits
    errs, fits = {}, {}
    for k in KS:
        w, err, model = _law(K, k)
        errs[k], fits[k] = err, split_fits(w)
        print(f"K={K} k={k}: restated err {err:.2e}, model {model:.2e}, split_fits {fits[k]}")
        assert err <= model + 1e-6, (k, err, model)
        if k >= 5:
            assert err >= model / K ** 0.5, (k, err, model)
    over = [k for k in KS if errs[k] > W.BAR / 2]
    under = [k for k in KS if errs[k] < W.BAR / 4]
    assert over and under and max(under) < min(over)
    assert not fits[min(over)] and all(not fits[k] for k in over), (errs, fits)
    assert fits[max(under)] and all(fits[k] for k in under), (errs, fits)
    flip = W.k_inside(lambda k: split_fits(_law(K, k)[0])) + 1
    print(f"K={K}: split_fits flips at k = {flip}")
    assert flip == {128: 5, 1536: 3}[K]    # recorded in DESIGN.md §2; a measurement of the rule, pinned so the record stays true


@pytest.mark.parametrize("K", [128, 1536])
@pytest.mark.parametrize("pattern", [("whole", 12), "rows", "cols"])
def test_patterns_the_rule_catches(K, pattern):
    """(a) the whole tensor at 2^-12, (b) half the rows at 2^-12, per row group against that group's own magnitude, (c) matched
    columns: the restated arithmetic is over the bar on each and split_fits says no."""
    from graspldm_amd.r1d_pack import split_fits
    m, n = 64, 96
    w = W.apply(W.kaiming(m, K, seed=3 * K), pattern)
    x = torch.randn(K, n, generator=torch.Generator().manual_seed(K + 2)) / W.col_scale(K, pattern)[:, None]
    ref, got = w.double() @ x.double(), W.restated_gemm(w, x)
    errs = [W.rel(got[g], ref[g]) for g in W.row_groups(m, pattern)]
    print(f"K={K} {pattern}: restated err per row group {errs}")
    assert errs[-1] > W.BAR, errs
    if pattern == "rows":
        assert errs[0] < W.BAR / 4, errs      # the loud rows are untouched: the tensor's max hides the quiet ones
    assert not split_fits(w)


def test_patterns_the_rule_leaves_alone():
    """Near-zero ENTRIES are no reason to reroute (any trained layer has them), and zero padding is none either."""
    from graspldm_amd.r1d_pack import mfma_a_fragments_f16x2, pad_cin32, split_fits
    g = torch.Generator().manual_seed(9)
    for K in (128, 1536):
        w = W.kaiming(64, K, seed=K)
        holes = torch.rand(64, K, generator=g) < 0.05
        for fill in (1e-9, 0.0):
            v = torch.where(holes, torch.full_like(w, fill), w)
            assert split_fits(v), (K, fill)
            x = torch.randn(K, 96, generator=g)
            assert W.rel(W.restated_gemm(v, x), v.double() @ x.double()) < W.BAR / 4
    w = W.kaiming(40, 3 * 16, seed=1)
    padded = torch.zeros(48, 96)
    padded[:40] = pad_cin32(w, 16, 3)          # M padded to 16, every tap's 16 channels to 32
    assert split_fits(padded) and split_fits(torch.zeros(16, 32))
    mfma_a_fragments_f16x2(pad_cin32(w, 16, 3))
    assert not split_fits(torch.full((16, 32), 7.0e4))   # the other end of the range does not fit either


# ------------------------------------------------------------------------------------------- no shipped layer changes route
class _Recorder:
    def __init__(self, packed, device):
        self.packed, self.device = packed, device


def _tensors(value, out):
    if isinstance(value, torch.Tensor):
        out.append(value)
    elif isinstance(value, dict):
        for v in value.values():
            _tensors(v, out)
    elif isinstance(value, (tuple, list)):
        for v in value:
            _tensors(v, out)
    elif hasattr(value, "_fields_") and not isinstance(value, type):   # a ctypes descriptor
        out.append(torch.frombuffer(bytearray(bytes(value)), dtype=torch.uint8))
    return out


def _concat_splits(cin):
    """The (ca, broadcast, both_wide) dense.concat_conv_bn_relu can be asked for on a first layer of `cin` columns."""
    from graspldm_amd import dense
    out = []
    for ca in range(1, cin):
        cb = cin - ca
        both = cb >= 128 and ca >= 128 and dense.split_supported(ca) and dense.split_supported(cb)
        if dense.split_supported(ca) and (cb in dense.SMALL_CIN or both):
            out.append((ca, False, both))
        if dense.split_supported(cb) and ca % 16 == 0:
            out.append((ca, True, False))
    return out


def _pack_all(model):
    """Every split-capable packer of `model`, driven as the forward passes drive them -> (packed tensors, route flags)."""
    from graspldm_amd import attention, dense, voxel
    from graspldm_amd.grasp_classifier import PointsBasedGraspClassifier
    from graspldm_amd.grasp_vae import ConditionalGraspPoseDecoder, ConditionalGraspPoseEncoder, GraspCVAE
    from graspldm_amd.pvcnn import PVConv, SharedMLP
    from graspldm_amd.resnets import ResNet1D
    from graspldm_amd.sa_pack import SaMlpPlan
    out, routes = [], []
    inside = set()
    for mod in model.modules():
        if isinstance(mod, (ConditionalGraspPoseDecoder, ConditionalGraspPoseEncoder)):
            inside.add(id(mod.net))
    bottleneck = next((m.bottleneck for m in model.modules() if isinstance(m, GraspCVAE)), None)
    for mod in model.modules():
        if isinstance(mod, SharedMLP) and isinstance(mod.layers[0], nn.Conv2d):
            plan = SaMlpPlan(mod, CPU)
            split = plan._split_plan()
            routes.append(split is not None)
            _tensors(split, out)
            if len(plan._folded) >= 2 and plan._folded[0][0].shape[0] <= 256:
                pre = plan._pack_pre()
                _tensors(tuple(pre.table) + (pre.w1b, pre.b1), out)
                if pre.w1b.shape[1] >= dense.SPLIT_PAD_MIN_CIN:
                    out.append(dense.split_fragments(pre.w1b))
        elif isinstance(mod, SharedMLP):
            for i in range(0, len(mod.layers), 3):
                f = dense._pack_folded(mod.layers[i], mod.layers[i + 1], CPU)
                routes.append(f.ws is not None)
                _tensors(tuple(f)[:4], out)
                if i == 0:
                    for ca, broadcast, both in _concat_splits(f.w.shape[1]):
                        _tensors(tuple(dense._pack_concat(f, ca, broadcast, both, CPU)), out)
        elif isinstance(mod, PVConv):
            convs = [m for m in mod.voxel_layers if isinstance(m, nn.Conv3d)]
            plan = voxel.VoxelBranchPlan(convs, CPU, mod.resolution)
            routes += plan.split
            _tensors(plan.w, out)
        elif isinstance(mod, attention.Attention):
            for p in mod._packed(CPU):
                routes.append(p.ws is not None)
                _tensors(tuple(p), out)
        elif isinstance(mod, PointsBasedGraspClassifier):
            pack = mod._head_pack(CPU)
            routes.append(not pack.exact)
            _tensors(tuple(pack)[:4], out)
        elif isinstance(mod, ConditionalGraspPoseDecoder):
            _tensors(mod._pack(CPU, 3).packed, out)
        elif isinstance(mod, ConditionalGraspPoseEncoder):
            _tensors(mod._pack(CPU, 3, bottleneck).packed, out)
        elif isinstance(mod, ResNet1D) and id(mod) not in inside:
            _tensors(mod.engine(CPU).packed, out)
        if getattr(mod, "global_attention", None) is not None:
            cd = mod.conv_downscale
            p = attention.pack_conv(cd.weight.reshape(cd.weight.shape[0], -1), cd.bias, CPU)
            routes.append(p.ws is not None)
            _tensors(tuple(p), out)
    return out, routes


def _ppc():
    from conftest import load_schema
    from graspldm_amd.builder import build_model_from_cfg
    from graspldm_amd.pipeline import fpc_model_config
    from graspldm_amd.synthetic import synthetic_state_dict
    cfg = fpc_model_config(scheduler="ddpm", latent=16, pc_latent=256)
    ldm = build_model_from_cfg(cfg["ddm"])
    ldm.set_vae_model(build_model_from_cfg(cfg["vae"]))
    ldm.load_state_dict(synthetic_state_dict(load_schema("schema_ppc_ldm.json"), seed=0), strict=True)
    return ldm.eval()


def _synthetic(module, seed=0):
    from graspldm_amd.synthetic import load_synthetic_weights
    return load_synthetic_weights(module, seed=seed).eval()


def _attention_modules():
    from graspldm_amd.attention import Attention
    box = nn.Module()
    box.a = _synthetic(Attention(64, 8, D=1))
    box.b = _synthetic(Attention(32, 8, D=3))
    box.c = _synthetic(Attention(128, 8, D=1), seed=3)
    return box


def _msg():
    from graspldm_amd.pvcnn import PointNet2MSG
    return _synthetic(PointNet2MSG(num_shapes=4))


def _pvcnn2():
    from graspldm_amd.pvcnn import PVCNN2
    return _synthetic(PVCNN2())


def _models():
    from graspldm_amd.pipeline import build_classifier, build_fpc_ldm
    return {
        "fpc-1024": lambda: build_fpc_ldm(1024),
        "fpc-64": lambda: build_fpc_ldm(64),
        "fpc-global-attention": lambda: build_fpc_ldm(use_global_attention=True),
        "fpc-pvcnn2-local-attention": lambda: build_fpc_ldm(encoder="PVCNN2Encoder", encoder_scale=(0.5, 0.5), use_local_attention=True),
        "fpc-pvcnn2": lambda: build_fpc_ldm(encoder="PVCNN2Encoder"),
        "ppc": _ppc,
        "pvcnn2": _pvcnn2,
        "msg": _msg,
        "classifier-pvcnn": lambda: build_classifier(1024, 64),
        "classifier-pvcnn-64": lambda: build_classifier(64, 12),
        "classifier-pvcnn2": lambda: build_classifier(1024, 64, "PVCNN2"),
        "attention": _attention_modules,
    }


@pytest.fixture()
def spy(monkeypatch):
    """split_planes (the one place a packer asks the rule) records every matrix it is handed; `parent()` swaps in the
    unchanged split_f16x2, which is what stood there before the rule existed."""
    from graspldm_amd import r1d, r1d_pack, resnets, unet1d_pack
    seen = []
    real = r1d_pack.split_planes

    def recording(w2d):
        seen.append(w2d.detach().clone())
        return real(w2d)

    def use(fn):
        monkeypatch.setattr(r1d_pack, "split_planes", fn)
        monkeypatch.setattr(unet1d_pack, "split_planes", fn)

    use(recording)
    monkeypatch.setattr(resnets, "R1dEngine", _Recorder)
    monkeypatch.setattr(r1d, "R1dEngine", _Recorder)
    seen_box = type("Spy", (), {})()
    seen_box.seen, seen_box.parent, seen_box.current = seen, (lambda: use(r1d_pack.split_f16x2)), (lambda: use(recording))
    return seen_box


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert s.dtype == t.dtype and s.shape == t.shape
        assert torch.equal(s.view(torch.uint8) if s.is_floating_point() else s, t.view(torch.uint8) if t.is_floating_point() else t)


@pytest.mark.parametrize("name", sorted(_models()))
def test_no_shipped_layer_changes_route(name, spy):
    """Every model the GPU suite and bench.py build: each matrix a packer splits passes split_fits, every route flag reads
    "split", and the packed buffers are bit for bit what the packers produce with the unchanged split_f16x2 in the rule's
    place (zero reroutes, zero changed bits)."""
    import graspldm_amd
    from graspldm_amd.r1d_pack import SPLIT_TAU, split_fits
    model = _models()[name]()
    packed, routes = _pack_all(model)
    assert spy.seen, "no packer of this model splits a matrix"
    assert all(split_fits(w, SPLIT_TAU) for w in spy.seen)
    worst = max(_worst_ratio(w) for w in spy.seen)
    print(f"{name}: {len(spy.seen)} split matrices, worst ||r|| / ||w|| over rows and columns {worst:.2e} (tau {SPLIT_TAU:g})")
    graspldm_amd.invalidate_caches()
    spy.parent()
    before, routes_before = _pack_all(model)
    spy.current()
    _same(packed, before)
    assert routes == routes_before


def _worst_ratio(w):
    from graspldm_amd.r1d_pack import split_f16x2
    hi, lo = split_f16x2(w)
    r2, w2 = (w.double() - hi.double() - lo.double()) ** 2, w.double() ** 2
    worst = 0.0
    for d in (0, 1):
        n = w2.sum(d)
        worst = max(worst, float((r2.sum(d)[n > 0] / n[n > 0]).max()) ** 0.5 if (n > 0).any() else 0.0)
    return worst


def _r1d_names():
    import r1d_envelope_cases as C
    return sorted(C.ACCEPTED)


@pytest.mark.parametrize("name", _r1d_names())
def test_r1d_envelope_rows_keep_their_split_copies(name, spy):
    """The accepted rows of tests/r1d_envelope_cases.py pack as before: the engines the GPU envelope tests run are the same."""
    import r1d_envelope_cases as C
    packed = _tensors(C.pack(name), [])
    spy.parent()
    before = _tensors(C.pack(name), [])
    spy.current()
    _same(packed, before)


def _unet_pack(name, sd=None):
    import unet1d_ref as U
    from graspldm_amd.resnets import Unet1D
    from graspldm_amd.unet1d_pack import pack_unet1d
    c = U.config(name)
    if sd is None:
        sd = {k: v.detach() for k, v in _synthetic(Unet1D(**c["args"]), seed=c["seed"]).state_dict().items()}
    rows = 0 if c["z_shape"] is None else (1 if len(c["z_shape"]) == 1 else c["z_shape"][0])
    pk = pack_unet1d(sd, "", c["args"]["resnet_block_groups"], c["L"], cond_rows=rows,
                     time_cond=c["args"]["is_time_conditioned"], num_steps=1000)
    return pk, sd


def _unet_names():
    import unet1d_ref as U
    return sorted(U.CASES) + sorted(U.ENVELOPE)


@pytest.mark.parametrize("name", _unet_names())
def test_unet1d_cases_keep_the_split_form(name, spy):
    pk, sd = _unet_pack(name)
    assert not pk["desc"].exact_f32 and spy.seen
    spy.parent()
    before, _ = _unet_pack(name, sd)
    spy.current()
    _same(_tensors(pk, []), _tensors(before, []))


# ----------------------------------------------------------------------------------------------------------- the engines
def test_resnet1d_engine_falls_back_to_the_exact_form(fpc_state_dict):
    """A downsample conv at 2^-12: pack_resnet1d raises nothing and returns the descriptor without split copies, equal to the
    pack under numerics.f32_only(); the unscaled network keeps its split copies."""
    from graspldm_amd import numerics
    from graspldm_amd.r1d_pack import pack_resnet1d
    p = "diffusion_model.model."
    sd = {k: v.clone() for k, v in fpc_state_dict.items() if k.startswith(p)}
    kw = dict(groups=4, seq_len=4, num_steps=1000)
    assert pack_resnet1d(sd, p, **kw)["desc"].lv[1].down_w3 != 0
    sd[p + "blocks.1.3.weight"] *= 2.0 ** -12
    pk = pack_resnet1d(sd, p, **kw)
    assert all(lv.down_w3 == 0 and lv.out_w3 == 0 and lv.qkvn_w3 == 0 and lv.down_wq == 0 for lv in pk["desc"].lv)
    assert all(rb.c1_w3 == 0 and rb.c1_wq == 0 for rb in pk["desc"].rb)
    with numerics.f32_only():
        exact = pack_resnet1d(sd, p, **kw)
    _same(_tensors(pk, []), _tensors(exact, []))


def test_unet1d_packer_falls_back_to_the_exact_form():
    from graspldm_amd import numerics
    pk, sd = _unet_pack("A")
    assert not pk["desc"].exact_f32
    sd = {k: v.clone() for k, v in sd.items()}
    sd["downs.1.3.weight"] *= 2.0 ** -12
    small, _ = _unet_pack("A", sd)
    assert small["desc"].exact_f32
    with numerics.f32_only():
        exact, _ = _unet_pack("A", sd)
    _same(_tensors(small, []), _tensors(exact, []))


# ------------------------------------------------------------------------------------------------------------- the guard
def test_every_split_packer_has_a_gpu_row():
    """Every package module that packs split-f16 weight fragments (found by name, over the package's Python) has a row in
    weight_range_cases.GPU_TABLE, and every test a row names exists in tests/test_weight_range_gpu.py."""
    pkg = os.path.join(ROOT, "graspldm_amd")
    names = re.compile(r"\b(mfma_a_fragments_f16x2|split_f16x2|split_planes|split_fragments|f16x2_fragments)\b")
    found = {n for n in os.listdir(pkg) if n.endswith(".py") and names.search(open(os.path.join(pkg, n)).read())}
    assert found == set(W.GPU_TABLE), (sorted(found - set(W.GPU_TABLE)), sorted(set(W.GPU_TABLE) - found))
    text = open(os.path.join(ROOT, "tests", "test_weight_range_gpu.py")).read()
    tests = set(re.findall(r"^def (test_\w+)\(", text, flags=re.M))
    for module, rows in W.GPU_TABLE.items():
        assert rows and set(rows) <= tests, (module, sorted(set(rows) - tests))
