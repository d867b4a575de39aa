"""GPU (MI355X): the grasp success classifier -- its two kernels (csrc/grasp_classifier.hip) through the package's launchers
against the same expressions in f64, the model against the reference's own outputs (grasp_classifier.npz) and the
inference harness with a classifier attached.

Head tolerance per case = max(2e-5 max(1, max|logit|), 4 e32): test_attention_gpu.py's rule -- 2e-5 is the project's
single-forward bar, e32 the error of the SAME formula evaluated by torch on the CPU in f32 against f64 on the same inputs
(computed here).  Where x is scaled the biases are zero, so the logit is homogeneous in x, and the first term is
2e-5 max|logit| (the bar moves with max|x|).
End to end: max(5e-5 max(1, max|logit|), 4 d), the encoder bar and the golden's own f32 rounding d (stored with it).

Measured worst error / tolerance ratios on an MI355X are recorded in DESIGN.md §4.5."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROWS = 128
HEAD_SHAPES = [(3, 64, 96), (2, 512, 76), (1, 64, 1088), (2, 1536, 52), (5, 16, 1)]
SCENE_CASES = [  # (Bc, G, Np, Ng), pc_mean given, pc_shift, pc_scale
    ((2, 3, 40, 12), True, 0.0, 0.05),
    ((1, 1, 64, 32), False, 0.0, 1.0),
    ((3, 2, 1024, 64), True, 0.0125, 0.05),
]
GOLDEN_CASES = {"a": ("PVCNN", 1024, 64, 2), "b": ("PVCNN", 64, 12, 2), "c": ("PVCNN2", 1024, 64, 1)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ----------------------------------------------------------------------------------------------------------- scene kernel
def _scene_inputs(bc, g, np_, ng, seed=0):
    from graspldm_amd import gripper
    from graspldm_amd.synthetic import _random_rotation
    gen = torch.Generator().manual_seed(100 + seed + np_)
    raw = 0.1 * torch.randn(bc, np_, 3, generator=gen) + 0.2 * torch.rand(bc, 1, 3, generator=gen)
    H = torch.zeros(bc * g, 4, 4)
    for i in range(bc * g):
        H[i, :3, :3] = _random_rotation(gen).float()
        H[i, :3, 3] = raw[i // g].mean(0) + 0.06 * torch.randn(3, generator=gen)
        H[i, 3, 3] = 1.0
    return raw, H, gripper.control_points(ng)


@pytest.mark.parametrize("shape,with_mean,shift,scale", SCENE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_scene_kernel_against_f64(shape, with_mean, shift, scale):
    from graspldm_amd.grasp_classifier import grasp_scene
    bc, g, np_, ng = shape
    raw, H, gp = _scene_inputs(*shape)
    mean = raw.mean(1) if with_mean else None
    pc = ((raw - mean[:, None] - shift) / scale) if with_mean else raw.clone()
    x = grasp_scene(pc.cuda(), H.cuda(), gp.cuda(), None if mean is None else mean.cuda(), shift, scale)
    x2 = grasp_scene(pc.cuda(), H.cuda(), gp.cuda(), None if mean is None else mean.cuda(), shift, scale)
    assert torch.equal(x, x2)                                                   # bitwise repeatable
    x = x.cpu()
    assert x.shape == (bc * g, 4, np_ + ng)
    rep = pc.repeat_interleave(g, 0).transpose(1, 2)
    assert torch.equal(x[:, :3, :np_], rep)                                     # cloud columns: bit copies
    assert torch.equal(x[:, 3, :np_], torch.zeros(bc * g, np_)) and torch.equal(x[:, 3, np_:], torch.ones(bc * g, ng))
    sh, sc = float(torch.tensor(shift, dtype=torch.float32)), float(torch.tensor(scale, dtype=torch.float32))
    ref = torch.einsum("bij,nj->bin", H[:, :3, :3].double(), gp.double()) + H[:, :3, 3].double()[:, :, None]
    if with_mean:
        ref = ref - mean.double().repeat_interleave(g, 0)[:, :, None]
    ref = (ref - sh) / sc
    err = (x[:, :3, np_:].double() - ref).abs()
    tol = 1e-6 * ref.abs().clamp(min=1.0)
    print(f"grasp_scene {shape}: worst err / tol {float((err / tol).max()):.3f}, max|x| {float(ref.abs().max()):.2f}")
    assert (err <= tol).all(), float((err / tol).max())


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_scene_kernel_reproduces_the_reference_points(case):
    """The gripper columns equal the grasp points the reference pipeline computed from the same poses (H @ [p; 1], minus the
    cloud's mean, over pc_scale: acronym_grasp_points.py:25-28,107,117) BIT FOR BIT: the kernel walks the same order."""
    from graspldm_amd.grasp_classifier import grasp_scene
    from graspldm_amd.synthetic import PC_STD, synthetic_batch
    golden = load_golden("grasp_classifier.npz")
    _, n_cloud, n_grip, g = GOLDEN_CASES[case]
    pcs, metas = synthetic_batch(2, n_cloud)
    x = grasp_scene(pcs.cuda(), golden[f"{case}_H"].cuda(), golden[f"{case}_gripper"].cuda(), metas["pc_mean"].cuda(), 0.0, PC_STD)
    got, want = x[:, :3, n_cloud:].transpose(1, 2).cpu(), golden[f"{case}_grasp_points"]
    assert got.shape == want.shape == (2 * g, n_grip, 3)
    assert torch.equal(got, want), int((got != want).sum())


# ------------------------------------------------------------------------------------------------------------ head kernel
def head_ref(x, w1, b1, w2, l, lb, b2):
    """logit_b = lb + b2 sum_n l_n + sum_n l_n (w2 . relu(W1' x_{b,n} + b1')) in the dtype of the inputs (torch, CPU)."""
    y = torch.relu(torch.einsum("rc,bcn->brn", w1, x) + b1[None, :, None])
    z = torch.einsum("r,brn->bn", w2, y)
    return lb + b2 * l.sum() + (z * l[None]).sum(-1)


def make_head(b, c, n, kind="normal", seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * c + n)
    x = torch.randn(b, c, n, generator=g)
    w1 = torch.randn(ROWS, c, generator=g) / c ** 0.5
    b1 = 0.1 * torch.randn(ROWS, generator=g)
    w2 = torch.randn(ROWS, generator=g) / ROWS ** 0.5
    l = torch.randn(n, generator=g) / n ** 0.5
    lb, b2 = (0.1 * torch.randn(2, generator=g)).tolist()
    if kind == "negative":              # every pre-activation below zero: logit = lb + b2 sum(l) exactly
        b1 = -(w1.abs().sum(1) * x.abs().max() + 1.0)
    elif kind == "last3":               # only the last three points carry weight (the tail of the last tile)
        l[: max(n - 3, 0)] = 0.0
    elif kind.startswith("scale"):      # homogeneous in x: no biases
        b1, lb, b2 = torch.zeros(ROWS), 0.0, 0.0
        x = x * float(kind[5:])
    return x, w1, b1, w2, l, lb, b2


def run_head(x, w1, b1, w2, l, lb, b2, exact):
    from graspldm_amd import numerics
    from graspldm_amd.grasp_classifier import cls_head, pack_head_weights
    c0 = lb + b2 * float(l.double().sum())
    with numerics.f32_only(bool(exact)):
        pack = pack_head_weights(w1, b1, w2, l, c0, "cuda")
    assert pack.exact == bool(exact)
    return cls_head(x.cuda(), pack, w1.shape[0])


def head_case(args, exact, relative=False):
    a64 = [t.double() if torch.is_tensor(t) else t for t in args]
    ref = head_ref(*a64)
    e32 = (head_ref(*args).double() - ref).abs().max().item()
    logit, prob = run_head(*args, exact)
    assert torch.isfinite(logit).all() and torch.isfinite(prob).all()
    scale = ref.abs().max().item()
    tol = max(2e-5 * (scale if relative else max(1.0, scale)), 4 * e32)
    return (logit.cpu().double() - ref).abs().max().item(), tol, ref, logit, prob


@pytest.mark.parametrize("exact", [0, 1], ids=["split", "f32"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_against_f64(shape, exact):
    name = "f32" if exact else "split"
    for kind in ("normal", "negative", "last3", "scale1000", "scale0.001", "scale100000", "scale0.00001"):
        args = make_head(*shape, kind=kind)
        err, tol, ref, logit, prob = head_case(args, exact, relative=kind.startswith("scale"))
        print(f"cls_head {name} {shape} {kind}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (kind, err, tol)
        if kind == "negative":
            c0 = args[5] + args[6] * float(args[4].double().sum())
            assert (logit.cpu().double() - c0).abs().max() <= 1e-6 * max(1.0, abs(c0)), (logit, c0)
        # prob = sigmoid(logit) to one ulp of torch's
        want = torch.sigmoid(logit)
        ulp = (torch.nextafter(want, torch.full_like(want, 2.0)) - want).abs()
        assert ((prob - want).abs() <= ulp).all(), (prob, want)


def test_head_is_repeatable_and_independent_of_the_batch():
    for exact in (0, 1):
        args = make_head(4, 64, 1088, seed=3)
        a, pa = run_head(*args, exact)
        b, pb = run_head(*args, exact)
        assert torch.equal(a, b) and torch.equal(pa, pb)
        one, pone = run_head(args[0][2:3].contiguous(), *args[1:], exact)
        assert torch.equal(one, a[2:3]) and torch.equal(pone, pa[2:3])


def test_head_fallback_layers_agree_outside_the_kernel_limits(monkeypatch):
    """A shape the predicate rejects runs pointwise_conv_bn_relu + pointwise_rows + linear; on a shape both take, the two
    agree within the head bar."""
    from graspldm_amd import grasp_classifier as gc
    from graspldm_amd.pipeline import build_classifier
    model = build_classifier(64, 12).cuda()
    x = torch.randn(3, model.base_network.out_channels, 76, generator=torch.Generator().manual_seed(5)).cuda()
    logit, prob = model.head(x)
    monkeypatch.setattr(gc, "cls_head_supported", lambda c, rows, n: False)
    l2, p2 = model.head(x)
    assert l2.shape == logit.shape == (3,)
    assert (l2 - logit).abs().max() <= 2e-5 * max(1.0, float(logit.abs().max()))
    assert (p2 - prob).abs().max() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ model
@pytest.fixture(scope="module")
def golden():
    return load_golden("grasp_classifier.npz")


@pytest.fixture(scope="module")
def models():
    from graspldm_amd.pipeline import build_classifier
    cache = {}

    def get(backbone, n_cloud, n_grip):
        key = (backbone, n_cloud, n_grip)
        if key not in cache:
            cache[key] = build_classifier(n_cloud, n_grip, backbone, seed=0).cuda()
        return cache[key]
    return get


def _golden_case(case, golden, models):
    from graspldm_amd.synthetic import synthetic_batch
    backbone, n_cloud, n_grip, g = GOLDEN_CASES[case]
    pcs, metas = synthetic_batch(2, n_cloud)
    want, d = golden[f"{case}_logit"].double(), float(golden[f"{case}_d"])
    tol = max(5e-5 * max(1.0, float(want.abs().max())), 4 * d)
    return models(backbone, n_cloud, n_grip), pcs, metas, g, want, d, tol


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_forward_against_the_reference(case, golden, models):
    """forward on the stored grasp points.  Measured on an MI355X: case c (PVCNN2) 1.2e-6 against the bar 5e-5."""
    model, pcs, metas, g, want, d, tol = _golden_case(case, golden, models)
    pc_rep = pcs.repeat_interleave(g, 0).cuda()
    gp = golden[f"{case}_grasp_points"].cuda()
    logit, prob = model.predict(pc_rep, gp)
    none, preds = model(pc_rep, gp, compute_loss=False)
    assert none is None and preds.shape == (2 * g,) and torch.equal(preds, prob)
    assert torch.equal(model.classify_grasps(pc_rep, gp), preds)
    err = float((logit.cpu().double() - want).abs().max())
    print(f"classifier case {case} forward: err {err:.3e}, tol {tol:.3e} (d {d:.2e}), ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)
    assert (prob.cpu().double() - golden[f"{case}_prob"].double()).abs().max() <= tol / 4 + 1e-7   # |sigmoid'| <= 1/4
    one = model(pc_rep[:1], gp[:1], compute_loss=False)[1]
    assert one.ndim == 0 and torch.equal(one, preds[0])          # the reference's .squeeze(): 0-d for B = 1


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_score_poses_against_the_reference(case, golden, models):
    """score_poses on the stored poses: the gripper points come out of gldm_grasp_scene.  The reference's own PVCNN2 logit
    moves by 1.2e-4 when these points are rounded one ulp differently (c_sens in the fixture: farthest-point sampling and
    ball queries select points, evenly spaced gripper points make near-ties), so case c holds only because the kernel
    evaluates the points in the reference's own order (test_scene_kernel_reproduces_the_reference_points)."""
    from graspldm_amd.synthetic import PC_STD
    model, pcs, metas, g, want, d, tol = _golden_case(case, golden, models)
    probs, logit = model.score_poses(pcs.cuda(), golden[f"{case}_H"].cuda(), gripper_points=golden[f"{case}_gripper"].cuda(),
                                     pc_mean=metas["pc_mean"].cuda(), pc_shift=0.0, pc_scale=PC_STD, return_logits=True)
    assert probs.shape == (2, g)
    err = float((logit.reshape(-1).cpu().double() - want).abs().max())
    print(f"classifier case {case} score_poses: err {err:.3e}, tol {tol:.3e} (d {d:.2e}, reference's own sensitivity "
          f"{float(golden[case + '_sens']):.2e}), ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)


def test_score_poses_chunks_bitwise_and_validates(models):
    from graspldm_amd._lib import GldmError
    from graspldm_amd.synthetic import PC_STD, synthetic_batch
    model = models("PVCNN", 64, 12)
    pcs, metas = synthetic_batch(3, 64)
    _, H, _ = _scene_inputs(3, 2, 64, 12, seed=9)
    H[:, :3, 3] = (H[:, :3, 3] - H[:, :3, 3].mean(0)) + metas["pc_mean"].repeat_interleave(2, 0)
    kw = dict(pc_mean=metas["pc_mean"].cuda(), pc_scale=PC_STD)
    pc, Hc = pcs.cuda(), H.view(3, 2, 4, 4).cuda()
    full = model.score_poses(pc, Hc, **kw)
    assert full.shape == (3, 2) and ((full > 0) & (full < 1)).all()
    assert torch.equal(full, model.score_poses(pc, Hc, **kw))                                          # repeatable
    per = model._scene_bytes(76)
    assert torch.equal(full, model.score_poses(pc, Hc, max_bytes=2 * per, **kw))                         # 3 chunks of a cloud
    assert torch.equal(full, model.score_poses(pc, Hc, max_bytes=per, **kw))                             # 6 chunks of a scene
    assert torch.equal(full[1:2], model.score_poses(pc[1:2], Hc[1:2], pc_mean=kw["pc_mean"][1:2], pc_scale=PC_STD))
    bad = pc.clone()
    bad[1, 5, 2] = float("nan")
    with pytest.raises(GldmError, match="non-finite"):
        model.score_poses(bad, Hc, **kw)
    badH = Hc.clone()
    badH[2, 1, 0, 3] = float("inf")
    with pytest.raises(GldmError, match="non-finite"):
        model.score_poses(pc, badH, **kw)
    with pytest.raises(RuntimeError, match="num_pc_points"):
        model.score_poses(pc[:, :60], Hc, gripper_points=torch.zeros(12, 3).cuda(), **kw)


@pytest.mark.parametrize("backbone,n", [("PVCNN", 76), ("PVCNN2", 1100)])
def test_backbones_take_four_channels_at_ragged_point_counts(backbone, n, models):
    """extra_feature_channels = 1 at an N that is no multiple of 32 (1100 = the reference's 1024 + 76)."""
    model = models(backbone, n - 12, 12)
    x = torch.randn(2, 4, n, generator=torch.Generator().manual_seed(2))
    x[:, 3] = (torch.arange(n) >= n - 12).float()
    f = model.base_network(x.cuda())
    assert f.shape == (2, model.base_network.out_channels, n) and torch.isfinite(f).all()
    logit, prob = model._scores(x.cuda())
    assert logit.shape == (2,) and ((prob > 0) & (prob < 1)).all()


# ---------------------------------------------------------------------------------------------------------------- harness
def test_harness_scores_generated_grasps(models):
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    inf = InferenceLDM(model=build_fpc_ldm(n_points=64, scheduler="ddim"), num_inference_steps=5, device="cuda:0")
    pcs, metas = synthetic_batch(2, 64)
    x_T = torch.randn(8, 1, 4, generator=torch.Generator().manual_seed(1))
    plain = inf.generate_grasps(pcs, metas, num_grasps=4, x_T=x_T)
    assert set(plain) == {"grasps", "grasp_tmrp", "confidence", "qualities", "pc", "all_steps_grasps"}
    inf.set_classifier(models("PVCNN", 64, 12))
    res = inf.generate_grasps(pcs, metas, num_grasps=4, x_T=x_T)
    assert set(res) == set(plain) | {"success"}
    assert torch.equal(res["grasps"], plain["grasps"])
    s = res["success"]
    assert s.shape == (2, 4, 1) and ((s > 0) & (s < 1)).all()
    assert torch.equal(s[..., 0], inf.score_grasps(pcs, metas, res["grasps"]))
    inf.set_classifier(None)
    assert set(inf.generate_grasps(pcs, metas, num_grasps=4, x_T=x_T)) == set(plain)
