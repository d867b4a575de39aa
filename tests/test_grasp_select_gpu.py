"""GPU: gldm_grasp_clearance and gldm_select_grasps against their f64 restatements (grasp_select_ref.py), their exactness
properties (cap, chunking, placement, repeatability, ties), and `_InferenceBase.select_grasps` on a synthetic LDM with a
synthetic classifier.

Bars.  clearance: |clearance - f64| <= 2e-6 max(1, M), M = the largest |p - t| coordinate of the pose's cloud: the result is
|w| of a vector reached in about ten f32 roundings of magnitudes <= M, 6e-7 M per component, times sqrt 3, doubled.
contacts: exact, under the precondition (asserted in f64, allowed count zero) that no point's body or sweep distance lies
within that bar of the tube radius.  Diverse selection: index sequences equal the f64 greedy's under the precondition
(asserted in f64) that best and second-best m differ by >= 1e-4 relative at every pick, 100 x the f32 bound of D; gap within
1e-5 relative.  The seeds below are the first ones for which the preconditions hold (margins are properties of the inputs:
they were evaluated in f64 on the CPU).
Measured on an MI355X: worst clearance error / bar 0.004, worst gap error 1.1e-7 relative."""
import math

import pytest
import torch

import grasp_select_ref as ref

pytestmark = pytest.mark.gpu

CAP, R_SWEEP, R_BODY = 0.05, 0.006, 0.006


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(b, g, ns, seed=0):
    """Like test_classifier_gpu._scene_inputs: clouds 0.05 randn + offset, poses at the cloud mean + 0.06 randn with random
    rotations -> (scene [b, ns, 3], H [b, g, 4, 4])."""
    from graspldm_amd.synthetic import _random_rotation
    gen = torch.Generator().manual_seed(1000 + 17 * seed + ns + 3 * g)
    scene = 0.05 * torch.randn(b, ns, 3, generator=gen) + 0.2 * torch.rand(b, 1, 3, generator=gen)
    H = torch.zeros(b, g, 4, 4)
    for c in range(b):
        for i in range(g):
            H[c, i, :3, :3] = _random_rotation(gen).float()
            H[c, i, :3, 3] = scene[c].mean(0) + 0.06 * torch.randn(3, generator=gen)
            H[c, i, 3, 3] = 1.0
    return scene, H


def _segments(sb, ss):
    from graspldm_amd import gripper
    return list(gripper.OPEN_SEGMENTS[:sb]), list(gripper.SWEEP_SEGMENTS[:ss])


def _bar(scene, H):
    m = (scene[:, None, :, :].double() - H[:, :, None, :3, 3].double()).abs().amax(dim=(2, 3))
    return 2e-6 * m.clamp(min=1.0)


def _chunk():
    from graspldm_amd.grasp_select import CHUNK
    return CHUNK


# (b, g, ns or "chunk+37", sb, ss, seed)
CLEARANCE_CASES = [(3, 5, 1000, 4, 2, 0), (2, 3, 63, 4, 2, 0), (1, 1, 1, 4, 2, 0), (2, 4, "chunk+37", 4, 2, 0),
                   (1, 7, 65, 4, 2, 0), (2, 3, 63, 1, 2, 0), (1, 7, 65, 4, 0, 0), (3, 5, 1000, 1, 0, 0)]
WORST = {"clearance": 0.0, "gap": 0.0}


@pytest.mark.parametrize("case", CLEARANCE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_clearance_and_contacts_against_f64(case):
    from graspldm_amd.grasp_select import grasp_clearance
    b, g, ns, sb, ss, seed = case
    ns = _chunk() + 37 if ns == "chunk+37" else ns
    scene, H = _inputs(b, g, ns, seed)
    body, sweep = _segments(sb, ss)
    want, want_contacts, body_d, sweep_d = ref.clearance(scene, H, body, sweep, R_SWEEP, CAP)
    bar = _bar(scene, H)
    # precondition (f64): no point within the bar of a tube's radius -- allowed count: zero
    assert int(((body_d - R_BODY).abs() <= bar[..., None]).sum()) == 0
    if sweep_d is not None:
        assert int(((sweep_d - R_SWEEP).abs() <= bar[..., None]).sum()) == 0
    kw = dict(body_segments=body, sweep_segments=sweep, sweep_radius=R_SWEEP, max_clearance=CAP)
    clear, contacts = grasp_clearance(scene.cuda(), H.cuda(), **kw)
    again = grasp_clearance(scene.cuda(), H.cuda(), **kw)
    assert clear.shape == (b, g) and clear.dtype == torch.float32 and contacts.shape == (b, g) and contacts.dtype == torch.int32
    assert torch.equal(clear, again[0]) and torch.equal(contacts, again[1])                        # repeatable, bit for bit
    ratio = ((clear.cpu().double() - want).abs() / bar).max().item()
    WORST["clearance"] = max(WORST["clearance"], ratio)
    print(f"clearance {case}: worst err / bar {ratio:.3f} (worst so far {WORST['clearance']:.3f}); capped {int((want == CAP).sum())} "
          f"of {b * g}, colliding {int((want <= R_BODY).sum())}, contacts {want_contacts.flatten().tolist()}")
    assert ratio <= 1.0, ratio
    assert torch.equal(contacts.cpu().long(), want_contacts)
    assert ((clear.cpu().double() > R_BODY) == (want > R_BODY)).all()                               # the collision_free decision


def test_far_away_pose_returns_exactly_the_cap():
    from graspldm_amd.grasp_select import grasp_clearance
    scene, H = _inputs(2, 3, 300)
    H[1, 1, :3, 3] += 5.0
    H[0, 2, :3, 3] -= 1.0
    clear, contacts = grasp_clearance(scene.cuda(), H.cuda(), max_clearance=0.0375)
    cap = torch.tensor(0.0375, dtype=torch.float32)
    assert torch.equal(clear[1, 1].cpu(), cap) and torch.equal(clear[0, 2].cpu(), cap)
    assert int(contacts[1, 1]) == 0 and int(contacts[0, 2]) == 0
    assert (clear.cpu() <= cap).all() and (clear.cpu() < cap).any()


def test_chunked_scene_combines_bit_for_bit():
    """min of the clearances and sum of the contacts of two launches over the two halves of a scene = one launch."""
    from graspldm_amd.grasp_select import grasp_clearance
    ns = 2 * _chunk() + 91
    scene, H = _inputs(2, 5, ns)
    one = grasp_clearance(scene.cuda(), H.cuda())
    for cut in (1, _chunk() - 3, ns // 2):
        a = grasp_clearance(scene[:, :cut].contiguous().cuda(), H.cuda())
        b = grasp_clearance(scene[:, cut:].contiguous().cuda(), H.cuda())
        assert torch.equal(torch.minimum(a[0], b[0]), one[0]), cut
        assert torch.equal(a[1] + b[1], one[1]), cut
    assert int(one[1].sum()) > 0 and (one[0] < 0.05).any()                                        # the case is not vacuous


def test_pose_placement_does_not_change_its_bits():
    from graspldm_amd.grasp_select import grasp_clearance
    scene, H = _inputs(1, 5, 700)
    full = grasp_clearance(scene.cuda(), H.cuda())
    alone = grasp_clearance(scene.cuda(), H[:, 3:4].contiguous().cuda())
    assert torch.equal(alone[0][0, 0], full[0][0, 3]) and torch.equal(alone[1][0, 0], full[1][0, 3])
    # a cloud alone against the same cloud in a batch; [G,4,4] / [Ns,3] for one cloud
    scene2, H2 = _inputs(3, 5, 700, seed=1)
    batch = grasp_clearance(scene2.cuda(), H2.cuda())
    single = grasp_clearance(scene2[2].cuda(), H2[2].cuda())
    assert single[0].shape == (1, 5)
    assert torch.equal(single[0][0], batch[0][2]) and torch.equal(single[1][0], batch[1][2])


def test_clearance_validation():
    from graspldm_amd import gripper
    from graspldm_amd._lib import GldmError
    from graspldm_amd.grasp_select import MAX_SEGMENTS, grasp_clearance
    scene, H = _inputs(1, 2, 32)
    bad = scene.clone()
    bad[0, 5, 1] = float("nan")
    with pytest.raises(GldmError, match="non-finite"):
        grasp_clearance(bad.cuda(), H.cuda())
    badH = H.clone()
    badH[0, 1, 2, 3] = float("inf")
    with pytest.raises(GldmError, match="non-finite"):
        grasp_clearance(scene.cuda(), badH.cuda())
    with pytest.raises(NotImplementedError, match=str(MAX_SEGMENTS)):
        grasp_clearance(scene.cuda(), H.cuda(), body_segments=list(gripper.OPEN_SEGMENTS) * 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grasp_clearance(scene, H.cuda())
    with pytest.raises(RuntimeError, match="clouds"):
        grasp_clearance(scene.repeat(2, 1, 1).cuda(), H.cuda())


# ------------------------------------------------------------------------------------------------------------- selection
def _selection_inputs(b, g, seed):
    _, H = _inputs(b, g, 64, seed)
    gen = torch.Generator().manual_seed(77 + seed + g)
    score = torch.rand(b, g, generator=gen)
    keep = torch.rand(b, g, generator=gen) > 1.0 / 3.0
    if g == 1:
        keep[:] = True
    return H, score, keep


# (b, g, k, seed): seeds whose f64 margins are >= 1e-4 at every pick
SELECT_CASES = [(2, 64, 16, 0), (1, 257, 32, 1), (3, 20, 20, 0), (1, 1, 1, 0), (1, 2048, 6, 0)]


@pytest.mark.parametrize("case", SELECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_diverse_selection_equals_the_f64_greedy(case):
    from graspldm_amd import gripper
    from graspldm_amd.grasp_select import select_grasps
    b, g, k, seed = case
    H, score, keep = _selection_inputs(b, g, seed)
    ctrl = gripper.control_points(16)
    for mask in (keep, None):
        index, count, gap = select_grasps(H.cuda(), score.cuda(), keep=None if mask is None else mask.cuda(), k=k, diverse=True)
        assert index.shape == (b, k) and index.dtype == torch.int32 and count.shape == (b,) and gap.shape == (b, k)
        for c in range(b):
            kept = [True] * g if mask is None else mask[c].tolist()
            want, n, gaps, margins = ref.diverse(H[c], score[c], kept, ctrl, k)
            assert min(margins, default=math.inf) >= 1e-4, ("precondition: pick another seed", c, min(margins))
            assert index[c].tolist() == want, (c, index[c].tolist(), want)
            assert int(count[c]) == n == min(k, sum(kept))
            got = gap[c].cpu().double()
            assert got[0] == math.inf and (got[n:] == 0).all()
            if n > 1:
                w = torch.tensor(gaps[1:n], dtype=torch.float64)
                rel = ((got[1:n] - w).abs() / w).max().item()
                WORST["gap"] = max(WORST["gap"], rel)
                assert rel <= 1e-5, rel
    print(f"diverse {case}: worst gap error so far {WORST['gap']:.2e} relative")


@pytest.mark.parametrize("case", SELECT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_topk_equals_a_stable_sort(case):
    from graspldm_amd.grasp_select import select_grasps
    b, g, k, seed = case
    H, score, keep = _selection_inputs(b, g, seed)
    score[:, g // 2] = score[:, 0]                                    # an exact tie: the lower index goes first
    score = (score * 8).round() / 8 if g == 257 else score            # and many ties
    for mask in (keep, None):
        index, count, gap = select_grasps(H.cuda(), score.cuda(), keep=None if mask is None else mask.cuda(), k=k)
        for c in range(b):
            kept = torch.ones(g, dtype=torch.bool) if mask is None else mask[c]
            ids = torch.nonzero(kept).flatten()
            order = ids[torch.sort(score[c][kept], descending=True, stable=True).indices][:k].tolist()
            assert index[c].tolist() == order + [-1] * (k - len(order))
            assert index[c].tolist() == ref.topk(score[c], kept.tolist(), k)[0]
            assert int(count[c]) == len(order)
        assert (gap == 0).all()


def test_exact_duplicates_tie_to_the_lowest_index_and_come_last():
    from graspldm_amd.grasp_select import select_grasps
    H, score, _ = _selection_inputs(1, 6, 3)
    H, score = H[:, :6].clone(), score.clone()
    H[0, 4], H[0, 5], H[0, 1] = H[0, 2], H[0, 2], H[0, 0]          # 2 = 4 = 5 and 0 = 1, bit for bit
    score[0] = torch.tensor([0.5, 0.5, 0.9, 0.1, 0.9, 0.9])
    index, count, gap = select_grasps(H.cuda(), score.cuda(), k=6, diverse=True)
    idx = index[0].tolist()
    assert idx[0] == 2                                               # the lowest index of the tied best scores
    assert sorted(idx[:3]) == [0, 2, 3] and idx[1] in (0, 3)         # the distinct poses first: 0 before its copy 1
    assert idx[3:] == [1, 4, 5]                                      # copies only when nothing else is left, lowest first
    assert int(count[0]) == 6
    g = gap[0].cpu()
    assert g[0] == math.inf and (g[1:3] > 0).all() and (g[3:] == 0).all()
    # with a separation asked for, the copies are never taken
    index, count, _ = select_grasps(H.cuda(), score.cuda(), k=6, diverse=True, min_separation=1e-4)
    assert int(count[0]) == 3 and index[0].tolist()[3:] == [-1, -1, -1]
    # top-k on tied scores: index order
    index, _, _ = select_grasps(H.cuda(), score.cuda(), k=6)
    assert index[0].tolist() == [2, 4, 5, 0, 1, 3]


def test_min_separation_cuts_the_count_where_f64_does():
    from graspldm_amd import gripper
    from graspldm_amd.grasp_select import select_grasps
    H, score, keep = _selection_inputs(2, 64, 0)
    ctrl = gripper.control_points(16)
    free = [ref.diverse(H[c], score[c], keep[c].tolist(), ctrl, 64)[2] for c in range(2)]
    finite = sorted(x for gaps in free for x in gaps if 0 < x < math.inf)
    lo, hi = finite[len(finite) // 2 - 1], finite[len(finite) // 2]
    sep = 0.5 * (lo + hi)                                             # between two gaps that occur: cuts about half
    assert (hi - lo) / hi > 1e-4
    index, count, gap = select_grasps(H.cuda(), score.cuda(), keep=keep.cuda(), k=64, diverse=True, min_separation=sep)
    for c in range(2):
        want, n, _, _ = ref.diverse(H[c], score[c], keep[c].tolist(), ctrl, 64, min_separation=sep)
        assert 1 <= n < int(keep[c].sum()) and int(count[c]) == n and index[c].tolist() == want
        assert (gap[c, 1:n] >= sep).all()


def test_too_few_survivors_pad_with_minus_one():
    from graspldm_amd.grasp_select import select_grasps
    H, score, _ = _selection_inputs(2, 20, 0)
    keep = torch.zeros(2, 20, dtype=torch.bool)
    keep[0, [3, 11, 17]] = True                                       # cloud 1 keeps nothing
    for diverse in (False, True):
        index, count, gap = select_grasps(H.cuda(), score.cuda(), keep=keep.cuda(), k=8, diverse=diverse)
        assert count.tolist() == [3, 0]
        assert sorted(index[0, :3].tolist()) == [3, 11, 17] and index[0, 3:].tolist() == [-1] * 5
        assert index[1].tolist() == [-1] * 8 and (gap[1] == 0).all() and (gap[0, 3:] == 0).all()


def test_selection_validation():
    from graspldm_amd._lib import GldmError
    from graspldm_amd.grasp_select import MAX_CANDIDATES, select_grasps
    H, score, _ = _selection_inputs(1, 20, 0)
    with pytest.raises(NotImplementedError, match=str(MAX_CANDIDATES)):
        select_grasps(H.cuda(), score.cuda(), k=21)
    with pytest.raises(NotImplementedError, match=str(MAX_CANDIDATES)):
        select_grasps(torch.eye(4).repeat(1, MAX_CANDIDATES + 1, 1, 1).cuda(), torch.zeros(1, MAX_CANDIDATES + 1).cuda(), k=4)
    bad = score.clone()
    bad[0, 3] = float("nan")
    with pytest.raises(GldmError, match="non-finite"):
        select_grasps(H.cuda(), bad.cuda(), k=4)
    index, count, _ = select_grasps(H[0].cuda(), score[0].cuda(), k=4)                 # [G,4,4] for one cloud
    assert index.shape == (1, 4) and int(count[0]) == 4


# --------------------------------------------------------------------------------------------------------------- harness
@pytest.fixture(scope="module")
def harness():
    """A synthetic LDM (64-point clouds, 2 clouds x 12 grasps, 10 DDIM steps) with a synthetic classifier, the unselected
    run (scored for all poses) computed once and shared."""
    from graspldm_amd.inference import InferenceLDM
    from graspldm_amd.pipeline import build_classifier, build_fpc_ldm
    from graspldm_amd.synthetic import synthetic_batch
    inf = InferenceLDM(model=build_fpc_ldm(n_points=64, scheduler="ddim"), num_inference_steps=10, device="cuda:0")
    pcs, metas = synthetic_batch(2, 64)
    x_T = torch.randn(24, 1, 4, generator=torch.Generator().manual_seed(5))
    bare = inf.generate_grasps(pcs, metas, num_grasps=12, x_T=x_T)
    inf.set_classifier(build_classifier(64, 12, "PVCNN", seed=0).cuda())
    full = inf.generate_grasps(pcs, metas, num_grasps=12, x_T=x_T)
    return inf, pcs, metas, x_T, bare, full


def _run(harness, selection, **kw):
    inf, pcs, metas, x_T, _, _ = harness
    return inf.generate_grasps(pcs, metas, num_grasps=12, x_T=x_T, selection=selection, **kw)


def _gathered(t, index):
    idx = index.long().clamp(min=0)
    tail = t.shape[2:]
    return t.gather(1, idx.view(*idx.shape, *([1] * len(tail))).expand(-1, -1, *tail))


def test_default_path_is_unchanged(harness):
    inf, pcs, metas, x_T, bare, full = harness
    assert set(bare) == {"grasps", "grasp_tmrp", "confidence", "qualities", "pc", "all_steps_grasps"}
    assert set(full) == set(bare) | {"success"}
    again = inf.generate_grasps(pcs, metas, num_grasps=12, x_T=x_T)               # the selection module is imported by now
    assert set(again) == set(full)
    for k in ("grasps", "grasp_tmrp", "confidence", "pc", "success"):
        assert torch.equal(again[k], full[k]), k
    for k in ("grasps", "grasp_tmrp", "confidence", "pc"):
        assert torch.equal(bare[k], full[k]), k


def test_selected_arrays_are_gathers_of_the_unselected_run(harness):
    from graspldm_amd.grasp_select import GraspSelection
    _, _, _, _, _, full = harness
    before = {k: v.clone() for k, v in full.items() if isinstance(v, torch.Tensor)}
    for sel in (GraspSelection(top_k=5), GraspSelection(top_k=5, diverse=True),
                GraspSelection(collision_free=True, min_contacts=1, top_k=12),
                GraspSelection(min_confidence=float(full["confidence"].median()), top_k=4, diverse=True, min_separation=0.01)):
        res = _run(harness, sel)
        assert set(res) == set(full) | {"selected_index", "selected_count", "selected_gap", "clearance", "contacts"}
        index, count = res["selected_index"], res["selected_count"]
        k = sel.top_k
        assert index.shape == (2, k) and count.shape == (2,) and res["selected_gap"].shape == (2, k)
        valid = torch.arange(k, device=index.device)[None] < count[:, None]
        assert ((index >= 0) == valid).all()
        for key in ("grasps", "grasp_tmrp", "confidence", "success"):
            want = _gathered(full[key], index)
            vm = valid.view(2, k, *([1] * (want.ndim - 2))).expand_as(want)
            assert res[key].shape == want.shape, key
            assert torch.equal(res[key][vm], want[vm]), key                        # bitwise: success too (scored after selection)
            assert torch.isnan(res[key][~vm]).all(), key
        if sel.needs_clearance:
            clear, contacts = res["clearance"], res["contacts"]
            assert clear.shape == (2, 12) and contacts.shape == (2, 12)
            ok = (clear > sel.body_radius) & (contacts >= sel.min_contacts)
            assert count.tolist() == ok.sum(1).tolist()
            for c in range(2):
                assert ok[c][index[c, :int(count[c])].long()].all()
        else:
            assert res["clearance"] is None and res["contacts"] is None
        if not sel.diverse and not sel.needs_clearance:                              # plain top-k by confidence
            order = torch.sort(full["confidence"][..., 0], dim=1, descending=True, stable=True).indices[:, :k]
            assert torch.equal(index.long(), order)
    for k, v in before.items():
        assert torch.equal(full[k], v), k                                            # select_grasps(results=...) leaves results alone
    inf = harness[0]
    res = inf.select_grasps(full, GraspSelection(top_k=3))                          # the method on an existing dict
    assert torch.equal(res["success"], _gathered(full["success"], res["selected_index"]))
    assert full["grasps"].shape == (2, 12, 4, 4)


def test_min_success_scores_the_survivors_only(harness):
    from graspldm_amd.grasp_select import GraspSelection
    inf, pcs, metas, x_T, bare, full = harness
    conf, succ = full["confidence"][..., 0], full["success"][..., 0]
    c_cut, s_cut = float(conf.median()), float(succ.median())
    calls = []
    orig = inf.classifier.score_poses
    inf.classifier.score_poses = lambda pc, H, **kw: (calls.append(tuple(H.shape)), orig(pc, H, **kw))[1]
    try:
        res = _run(harness, GraspSelection(min_confidence=c_cut, min_success=s_cut, score_by="success"))
    finally:
        del inf.classifier.score_poses
    keep = conf >= c_cut
    assert len(calls) == 1 and calls[0][1] == int(keep.sum(1).max()) < 12           # only the survivors were scored
    ok = keep & (succ >= s_cut)
    index, count = res["selected_index"], res["selected_count"]
    assert index.shape == (2, 12) and count.tolist() == ok.sum(1).tolist()
    valid = torch.arange(12, device=index.device)[None] < count[:, None]
    want = _gathered(full["success"], index)[..., 0]
    assert torch.equal(res["success"][..., 0][valid], want[valid])                   # bitwise the all-pose entries
    assert torch.isnan(res["success"][..., 0][~valid]).all()                         # unscored / dropped: NaN
    for c in range(2):                                                               # by falling success
        s = want[c, :int(count[c])]
        assert (s[:-1] >= s[1:]).all()
    clf = inf.classifier
    inf.set_classifier(None)
    try:
        with pytest.raises(RuntimeError, match="classifier"):
            _run(harness, GraspSelection(min_success=0.5))
        res = _run(harness, GraspSelection(top_k=3))
        assert "success" not in res and torch.equal(res["grasps"], _gathered(bare["grasps"], res["selected_index"]))
    finally:
        inf.set_classifier(clf)


def test_scene_cloud_decides_collisions(harness):
    """scene_pc: a slab of points through every gripper makes every pose collide; the object cloud alone does not."""
    from graspldm_amd.grasp_select import GraspSelection
    _, _, _, _, _, full = harness
    H = full["grasps"]
    wall = H[:, :, :3, 3] + 0.03 * H[:, :, :3, 2]                                     # a point on every wrist axis
    scene = torch.cat([full["pc"], wall], dim=1)
    res = _run(harness, GraspSelection(collision_free=True), scene_pc=scene)
    assert res["selected_count"].tolist() == [0, 0] and (res["clearance"] < 1e-6).all()
    assert (res["selected_index"] == -1).all() and torch.isnan(res["grasps"]).all()


# ------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_writes_the_selection_and_leaves_the_plain_run_alone(tmp_path):
    import os
    import sys

    import numpy as np
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import generate_grasps as cli
    common = ["--synthetic", "64", "--mode", "LDM", "--num_samples", "2", "--num_grasps", "8", "--inference_steps", "5", "--seed", "3"]
    plain, picked = str(tmp_path / "plain.npz"), str(tmp_path / "picked.npz")
    cli.main(common + ["--out", plain])
    cli.main(common + ["--collision_free", "--top_k", "3", "--diverse", "--out", picked])
    with np.load(plain) as z:
        assert set(z.files) == {"grasps", "grasp_tmrp", "confidence"}
        all_grasps, all_conf = z["grasps"], z["confidence"]
    with np.load(picked) as z:
        assert set(z.files) == {"grasps", "grasp_tmrp", "confidence", "selected_index", "selected_count", "selected_gap",
                                "clearance", "contacts"}
        index, count, grasps, clear = z["selected_index"], z["selected_count"], z["grasps"], z["clearance"]
        assert z["selected_gap"].shape == (2, 3) and z["contacts"].shape == (2, 8)
    assert all_grasps.shape == (2, 8, 4, 4) and grasps.shape == (2, 3, 4, 4) and index.shape == (2, 3) and clear.shape == (2, 8)
    for c in range(2):
        n = int(count[c])
        assert n == min(3, int((clear[c] > 0.006).sum())) and (index[c, n:] == -1).all()
        assert np.array_equal(grasps[c, :n], all_grasps[c, index[c, :n]]) and np.isnan(grasps[c, n:]).all()
        if n:
            free = np.nonzero(clear[c] > 0.006)[0]
            assert index[c, 0] == free[np.argmax(all_conf[c, free, 0])]             # the first pick: the best survivor
