"""GPU: gldm_knn_radius, gldm_point_normals and gldm_grasp_contact_normals against their restatements (normals_ref.py), and the
friction-cone filter of `_InferenceBase.select_grasps` end to end.

Bars.  The search is a pure function of the inputs in f32 with one rounding per written operation: idx, found and d2 are
BITWISE equal to the restatement, whatever the launch shape and whatever the broad phase skips.  Normals: every component
within 2^-22 of the f64 normal (f32 diffs, f64 scatter matrix, numpy.linalg.eigh) under the precondition, per point and in
f64, that found >= 3 and (lambda_mid - lambda_min) / lambda_max >= 1e-3; at most 1 % of a case's points with found >= 3 may
be left out for it (points with found < 3 are not left out: they must be exactly zero).  The kernel's f64 Jacobi contributes
about 1e-13 at that gap and the output rounding at most 2^-25 per component, so the bar holds an 8x margin.  Contact counts:
exact, under the preconditions (asserted in f64, allowed count zero) that no point lies within the clearance test's bar of
the sweep radius, no |normal . axis| within 1e-6 of cos(friction angle) and no contact's |q.x| within that bar of 0; the
seeds are the first for which they hold (margins are properties of the inputs, evaluated in f64 on the CPU).

"found spans 1 .. k": every cloud of two or more points carries one far-away point (found = 1) next to a cluster, and the
middle radius is the median distance of a cluster point to its min(k, n - 1)-th nearest, so found reaches min(k, n - 1);
the shapes with n <= k cannot reach k, and the assertion is on 1 .. min(k, max(n - 1, 1)).

Measured on an MI355X: search and counts exact; normals worst error / bar 0.125, the output rounding alone."""
import functools
import math

import numpy as np
import pytest
import torch

import normals_ref as ref

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -22
SHAPES = [(1, 1, 3), (1, 2, 3), (2, 11, 12), (1, 12, 12), (1, 13, 12), (3, 63, 12), (1, 64, 16), (2, 65, 8), (1, 255, 12),
          (1, 256, 12), (2, 257, 1), (1, 3 * 256 + 37, 12)]
RADII = ("large", "middle", "small")
WORST = {"normals": 0.0}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _cloud(b, n):
    """[b, n, 3] f32: a cluster 0.05 randn around (0, 0, 0.6); with n >= 2, point 0 of every cloud ten metres away."""
    rng = np.random.default_rng(100 + n)
    pc = 0.05 * rng.standard_normal((b, n, 3)) + np.array([0.0, 0.0, 0.6])
    if n >= 2:
        pc[:, 0, 0] += 10.0
    return pc.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _radius(b, n, k, which):
    if which == "large":
        return 100.0
    if which == "small":
        return 1e-6
    pc = _cloud(b, n).astype(np.float64)
    cluster = pc[:, 1:] if n >= 2 else pc
    m = min(k, cluster.shape[1])
    d = np.sqrt(((cluster[:, :, None, :] - cluster[:, None, :, :]) ** 2).sum(-1))
    return float(np.median(np.sort(d, axis=-1)[:, :, m - 1]))


@functools.lru_cache(maxsize=None)
def _search_ref(b, n, k, which):
    """The restated search for a shape and a radius, computed once and shared by the tests that need it."""
    return ref.knn_radius_batch(_cloud(b, n), k, _radius(b, n, k, which))


def _equal_search(got, want):
    idx, d2, found = (t.cpu().numpy() for t in got)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and found.dtype == np.int32
    assert np.array_equal(found, want[2]), "found"
    assert np.array_equal(idx, want[0]), "idx"
    assert np.array_equal(d2.view(np.uint32), want[1].view(np.uint32)), "d2 bits"


@pytest.mark.parametrize("which", RADII)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_search_is_bitwise_the_restatement(shape, which):
    from graspldm_amd.pointcloud import knn_radius
    b, n, k = shape
    r = _radius(b, n, k, which)
    want = _search_ref(b, n, k, which)
    found = want[2]
    if which == "large":
        assert (found == min(k, n)).all()
    elif which == "small":
        assert (found == 1).all()
    else:
        assert found.min() == 1 and found.max() == min(k, max(n - 1, 1)), (found.min(), found.max())
    pc = torch.from_numpy(_cloud(b, n)).cuda()
    got = knn_radius(pc, k, r)
    again = knn_radius(pc, k, r)
    assert got[0].shape == (b, n, k) and got[1].shape == (b, n, k) and got[2].shape == (b, n)
    _equal_search(got, want)
    for a, c in zip(got, again):
        assert torch.equal(a, c)                                                   # repeatable, bit for bit
    one = knn_radius(pc[b - 1], k, r)                                              # [N,3]: the last cloud alone
    assert one[0].shape == (n, k) and all(torch.equal(o, g[b - 1]) for o, g in zip(one, got))


def test_ties_go_to_the_lower_index():
    from graspldm_amd.pointcloud import knn_radius
    rng = np.random.default_rng(7)
    base = (0.05 * rng.standard_normal((40, 3)) + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    triple = np.tile(base, (3, 1))                                                 # every point present three times
    g = np.arange(6, dtype=np.float32) * np.float32(2.0 ** -6)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(0.5)
    # 8 x 8 x 8 = two 256-point chunks, x = 0..3 and x = 4..7: a point of the face x = 4 ties its neighbours inside its own
    # chunk with lower-indexed ones at x = 3, whose chunk lies at box distance EXACTLY the k-th distance (and, at r = pitch,
    # exactly r): the skip must be strict for them to be seen
    g8 = np.arange(8, dtype=np.float32) * np.float32(2.0 ** -6)
    lattice8 = np.stack(np.meshgrid(g8, g8, g8, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(0.5)
    assert lattice8.shape[0] == 512
    for name, pc, cases in (("triple", triple, ((12, 100.0), (4, 0.03), (16, 0.02))),
                            ("lattice", lattice, ((12, 100.0), (16, 1.5 * 2.0 ** -6), (7, 2.0 ** -6), (12, 1.8 * 2.0 ** -6))),
                            ("lattice8", lattice8, ((12, 100.0), (4, 100.0), (7, 2.0 ** -6), (4, 2.0 ** -6), (16, 1.5 * 2.0 ** -6)))):
        for k, r in cases:
            want = ref.knn_radius(pc, k, r)
            d2 = want[1]
            ties = int(((d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])).sum())
            print(f"{name} k={k} r={r:.4g}: {ties} equal neighbours in the lists")
            assert ties > 0                                                        # the case does test ties
            if name == "lattice8":   # the case does reach across the chunk boundary through a tie
                face = np.arange(256, 256 + 64)
                cross = (want[0][face] < 256) & (want[1][face] == np.float32(2.0 ** -12))
                assert cross.any(axis=1).all()
            got = knn_radius(torch.from_numpy(pc).cuda(), k, r)
            _equal_search(got, want)


def test_broad_phase_changes_no_bit():
    from graspldm_amd.pointcloud import knn_radius
    k = 12
    pc = ref.organised_patch()
    n = pc.shape[0]
    assert n == 3072
    perm = np.random.default_rng(3).permutation(n)
    back = np.append(perm, n)                                                      # shuffled index -> original, n -> n
    dev = torch.from_numpy(pc).cuda()
    shuffled = torch.from_numpy(np.ascontiguousarray(pc[perm])).cuda()
    for r in (0.01, 1.0):
        assert ref.kth_tie_free(pc, k, r) == 0                                     # precondition (f64): no tie at a k-th distance
        longer = ref.knn_radius(pc, k + 1, r)                                      # one restated search: k + 1, cut to k
        assert not ((longer[1][:, k - 1] == longer[1][:, k]) & np.isfinite(longer[1][:, k])).any()   # ... nor in the search's f32
        want = (longer[0][:, :k], longer[1][:, :k], np.minimum(longer[2], k))
        got = knn_radius(dev, k, r)
        _equal_search(got, want)
        idx_s, d2_s, found_s = (t.cpu().numpy() for t in knn_radius(shuffled, k, r))
        assert np.array_equal(found_s, want[2][perm])
        assert np.array_equal(d2_s.view(np.uint32), want[1][perm].view(np.uint32))
        assert np.array_equal(np.sort(back[idx_s], axis=1), np.sort(want[0][perm], axis=1))   # the same neighbour sets
        print(f"patch r={r}: found {want[2].min()} .. {want[2].max()}")


def _check_normals(pc, idx, found, got, view=None, allowed=0.01):
    """One cloud [n,3]: got [n,3] f32 (GPU) against the f64 normals of the restated neighbour lists -> worst error / bar."""
    want, w, dot, live = ref.normals_f64(pc, idx, view)
    assert np.array_equal(live, found)
    ratio = ref.gap_ratio(w)
    plane = live >= 3
    ok = plane & (ratio >= 1e-3)
    left_out = int((plane & ~ok).sum())
    assert left_out <= allowed * pc.shape[0], (left_out, pc.shape[0])
    assert (got[~plane] == 0).all()                                                # found < 3: exactly zero
    g = got.astype(np.float64)
    rel = np.linalg.norm((pc - (np.zeros(3, np.float32) if view is None else np.asarray(view, np.float32))).astype(np.float64), axis=1)
    sure = np.abs(dot) > 1e-6 * rel                                                # the sign is decided
    err = np.where(sure[:, None], np.abs(g - want), np.minimum(np.abs(g - want), np.abs(g + want)))
    worst = float(err[ok].max()) if ok.any() else 0.0
    if ok.any():
        assert np.abs(np.linalg.norm(g[ok], axis=1) - 1.0).max() <= BAR
        assert ((g[ok & sure] * want[ok & sure]).sum(-1) > 0).all()                # the reference's sign
    return worst / BAR, left_out


@pytest.mark.parametrize("shape", SHAPES + [("half-sphere", 1061, 12)], ids=lambda s: "x".join(map(str, s)))
def test_normals_against_f64(shape):
    from graspldm_amd.pointcloud import estimate_normals
    if shape[0] == "half-sphere":
        _, n, k = shape
        pcs, r = ref.half_sphere(n)[None], 0.05
        want = ref.knn_radius_batch(pcs, k, r)
        allowed = 0.0                                                              # this case leaves out none
    else:
        b, n, k = shape
        pcs, r, want, allowed = _cloud(b, n), _radius(b, n, k, "middle"), _search_ref(b, n, k, "middle"), 0.01
    normals, found = estimate_normals(torch.from_numpy(pcs).cuda(), max_radius=r, k=k)
    assert normals.shape == pcs.shape and normals.dtype == torch.float32
    assert np.array_equal(found.cpu().numpy(), want[2])
    got = normals.cpu().numpy()
    worst, out = 0.0, 0
    for c in range(pcs.shape[0]):
        ratio, left = _check_normals(pcs[c], want[0][c], want[2][c], got[c], allowed=allowed)
        worst, out = max(worst, ratio), out + left
    WORST["normals"] = max(WORST["normals"], worst)
    print(f"normals {shape}: worst err / bar {worst:.4f} (worst so far {WORST['normals']:.4f}); left out {out} of {pcs.shape[0] * pcs.shape[1]}; "
          f"found < 3: {int((want[2] < 3).sum())}")
    assert worst <= 1.0, worst


def _wavy_plane(z=0.5, amp=0.0):
    rng = np.random.default_rng(11)
    v, u = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    x = (u - 10) * 0.005 + rng.uniform(-0.001, 0.001, u.shape)
    y = (v - 10) * 0.005 + rng.uniform(-0.001, 0.001, u.shape)
    zz = z + amp * np.sin(40.0 * x) * np.cos(31.0 * y)
    return np.stack([x, y, zz], axis=-1).reshape(-1, 3).astype(np.float32)


def test_plane_gives_the_axis():
    from graspldm_amd.pointcloud import estimate_normals
    pc = _wavy_plane()
    normals, found = estimate_normals(torch.from_numpy(pc).cuda(), max_radius=0.02, k=12)
    assert int(found.min()) >= 3
    err = (normals.cpu().double() - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)).abs().max().item()
    print(f"plane z = 0.5: worst component error {err:.3g}")
    assert err <= BAR


def test_neighbours_form_and_view_point():
    from graspldm_amd.pointcloud import PointCloudHelpers, estimate_normals, knn_radius
    pc = torch.from_numpy(ref.half_sphere(1061)).cuda()
    n, k, r = pc.shape[0], 12, 0.05
    normals, found = estimate_normals(pc, max_radius=r, k=k)
    assert int(found.min()) == k                                                   # every slot live: both forms count k
    idx = knn_radius(pc, k, r)[0].long()
    neighbours = pc[idx]
    by_neighbours = PointCloudHelpers.vectorized_normal_computation(pc, neighbours)
    assert torch.equal(by_neighbours, normals)
    assert torch.equal(PointCloudHelpers.estimate_normals_cam_from_pc(pc, max_radius=r, k=k), normals)
    # a missing slot counts as the point itself: the neighbours form given the point in those slots is the idx form
    small = 0.015
    idx2, _, found2 = knn_radius(pc, k, small)
    assert int(found2.min()) >= 3 and int(found2.min()) < k
    own = torch.arange(n, device=pc.device)[:, None].expand(-1, k)
    filled = pc[torch.where(idx2 == n, own, idx2.long())]
    assert torch.equal(PointCloudHelpers.vectorized_normal_computation(pc, filled), estimate_normals(pc, max_radius=small, k=k)[0])
    # the view point: on the other side of a (wavy) plane every sign flips and nothing else
    wavy = _wavy_plane(amp=0.001)
    idx_w = ref.knn_radius(wavy, k, 0.02)[0]
    other = (0.0, 0.0, 1.0)
    _, _, dot_a, _ = ref.normals_f64(wavy, idx_w)
    _, _, dot_b, _ = ref.normals_f64(wavy, idx_w, other)
    assert (dot_a * dot_b < 0).all() and np.abs(dot_a).min() > 1e-3 and np.abs(dot_b).min() > 1e-3   # precondition (f64)
    w = torch.from_numpy(wavy).cuda()
    a = estimate_normals(w, max_radius=0.02, k=k)[0]
    b = estimate_normals(w, max_radius=0.02, k=k, view_point=other)[0]
    assert torch.equal(a, -b) and (a[:, 2] < 0).all() and bool((a != 0).any(dim=1).all())


# ------------------------------------------------------------------------------------------------ contact normals --
R_SWEEP, FRICTION_DEG = 0.006, 30.0
# (b, g, ns or "chunk+37", seed): the shapes of test_grasp_select_gpu's clearance cases
# at seed 0; these clouds put few points between the fingers, and seed 21 is the first of the first shape at which a pose has
# aligned and unaligned contacts on both sides (test_contact_cases_are_not_vacuous)
CONTACT_CASES = [(3, 5, 1000, 0), (2, 3, 63, 0), (1, 1, 1, 0), (2, 4, "chunk+37", 0), (1, 7, 65, 0), (3, 5, 1000, 21)]


def _contact_inputs(case):
    """Scenes and poses as test_grasp_select_gpu._inputs makes them, random unit normals, every tenth one zero."""
    import test_grasp_select_gpu as base
    from graspldm_amd.grasp_select import CHUNK
    b, g, ns, seed = case
    ns = CHUNK + 37 if ns == "chunk+37" else ns
    scene, H = base._inputs(b, g, ns, seed)
    gen = torch.Generator().manual_seed(500 + seed + ns)
    normals = torch.randn(b, ns, 3, generator=gen)
    normals = normals / normals.norm(dim=-1, keepdim=True)
    normals[:, ::10] = 0.0
    return scene, normals, H, base._bar(scene, H)


def _contact_ref(case):
    from graspldm_amd import gripper
    scene, normals, H, bar = _contact_inputs(case)
    cos_f = math.cos(math.radians(FRICTION_DEG))
    want = ref.contact_normals(scene, normals, H, gripper.SWEEP_SEGMENTS, R_SWEEP, cos_f)
    # preconditions (f64), allowed count: zero
    assert int(((want["sweep_d"] - R_SWEEP).abs() <= bar[..., None]).sum()) == 0
    assert int((((want["axis_dot"] - cos_f).abs() <= 1e-6) & want["nonzero"]).sum()) == 0
    assert int((want["hit"] & (want["qx"].abs() <= bar[..., None])).sum()) == 0
    return scene, normals, H, want


@pytest.mark.parametrize("case", CONTACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_contact_normals_against_f64(case):
    from graspldm_amd.grasp_select import contact_normals, grasp_clearance
    scene, normals, H, want = _contact_ref(case)
    b, g = H.shape[:2]
    side, aligned = contact_normals(scene.cuda(), normals.cuda(), H.cuda(), sweep_radius=R_SWEEP, friction_angle_deg=FRICTION_DEG)
    again = contact_normals(scene.cuda(), normals.cuda(), H.cuda(), sweep_radius=R_SWEEP, friction_angle_deg=FRICTION_DEG)
    assert side.shape == (b, g, 2) and aligned.shape == (b, g, 2) and side.dtype == torch.int32 and aligned.dtype == torch.int32
    assert torch.equal(side, again[0]) and torch.equal(aligned, again[1])
    print(f"contact normals {case}: contacts by side {want['side'].flatten().tolist()}, aligned {want['aligned'].flatten().tolist()}")
    assert torch.equal(side.cpu().long(), want["side"])
    assert torch.equal(aligned.cpu().long(), want["aligned"])
    _, contacts = grasp_clearance(scene.cuda(), H.cuda(), sweep_radius=R_SWEEP)
    assert torch.equal(side.sum(-1, dtype=torch.int32), contacts)                  # bit for bit gldm_grasp_clearance's
    assert bool((aligned <= side).all())


def test_contact_cases_are_not_vacuous():
    """At least one case has aligned and unaligned contacts on both sides (f64 restatement; nothing passes for lack of
    contacts)."""
    both = False
    for case in CONTACT_CASES:
        want = _contact_ref(case)[3]
        s, a = want["side"], want["aligned"]
        both = both or bool(((a > 0) & (a < s)).all(-1).any())
    assert both


def test_zero_normals_are_never_aligned():
    from graspldm_amd.grasp_select import contact_normals
    scene, normals, H, _ = _contact_inputs(CONTACT_CASES[0])
    side, aligned = contact_normals(scene.cuda(), torch.zeros_like(normals).cuda(), H.cuda(), friction_angle_deg=90.0)
    assert int(side.sum()) > 0 and int(aligned.sum()) == 0
    side2, aligned2 = contact_normals(scene.cuda(), normals.cuda(), H.cuda(), sweep_segments=[])
    assert int(side2.sum()) == 0 and int(aligned2.sum()) == 0                      # no sweep family: no contact


# ------------------------------------------------------------------------------------------------------ selection --
def _finger_patches(turn_deg):
    """Two dense planar patches at x = +-0.03 of the gripper frame, between the finger tips (y in +-5 mm, z over both
    sweep segments, 1 mm pitch), each turned turn_deg about the approach axis through its own centre: [n, 3] f64."""
    u, v = np.meshgrid(np.arange(-5, 6) * 0.001, 0.095 + np.arange(17) * 0.001, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    c, s = math.cos(math.radians(turn_deg)), math.sin(math.radians(turn_deg))
    return np.concatenate([np.stack([x0 - u * s, u * c, v], axis=1) for x0 in (0.03, -0.03)])


def test_selection_keeps_the_pose_whose_contacts_face_the_fingers():
    from graspldm_amd.grasp_select import GraspSelection
    from graspldm_amd.inference import _InferenceBase
    from graspldm_amd.synthetic import _random_rotation
    R = _random_rotation(torch.Generator().manual_seed(5)).double().numpy()
    t = np.array([0.1, -0.05, 0.6])
    clouds = np.stack([(_finger_patches(deg) @ R.T + t) for deg in (0.0, 45.0)]).astype(np.float32)
    H = torch.eye(4).repeat(2, 1, 1, 1)
    H[:, 0, :3, :3] = torch.from_numpy(R).float()
    H[:, 0, :3, 3] = torch.from_numpy(t).float()
    results = dict(grasps=H.cuda(), grasp_tmrp=torch.zeros(2, 1, 6).cuda(), confidence=torch.full((2, 1, 1), 0.9).cuda(),
                   qualities=None, pc=torch.from_numpy(clouds).cuda())
    inf = _InferenceBase("cuda")
    plain = inf.select_grasps(results, GraspSelection(min_contacts=4))
    assert plain["selected_count"].tolist() == [1, 1] and (plain["contacts"] >= 4).all()
    assert set(plain) == set(results) | {"selected_index", "selected_count", "selected_gap", "clearance", "contacts"}
    cone = inf.select_grasps(results, GraspSelection(min_contacts=4, min_aligned_contacts=4, both_fingers=True))
    assert cone["selected_count"].tolist() == [1, 0]
    assert cone["aligned_contacts"].shape == (2, 1, 2) and cone["aligned_contacts"].dtype == torch.int32
    assert (cone["aligned_contacts"][0] >= 4).all() and int(cone["aligned_contacts"][1].sum()) == 0
    assert set(cone) == set(plain) | {"aligned_contacts"}
    for key in plain:                                                              # the other keys are what they were
        if isinstance(plain[key], torch.Tensor) and key not in ("grasps", "grasp_tmrp", "confidence", "selected_index",
                                                                "selected_count", "selected_gap"):
            assert torch.equal(plain[key], cone[key]), key
    assert torch.equal(cone["grasps"][0], plain["grasps"][0]) and bool(torch.isnan(cone["grasps"][1]).all())
    # normals handed in replace the estimate; in total instead of per side; a wider cone lets the turned patches through
    from graspldm_amd.pointcloud import estimate_normals
    normals = estimate_normals(results["pc"], max_radius=0.05, k=12)[0]
    given = inf.select_grasps(results, GraspSelection(min_aligned_contacts=4), scene_normals=normals)
    assert torch.equal(given["aligned_contacts"], cone["aligned_contacts"]) and given["selected_count"].tolist() == [1, 0]
    assert given["clearance"] is None and given["contacts"] is None
    wide = inf.select_grasps(results, GraspSelection(min_aligned_contacts=4, both_fingers=True, friction_angle_deg=50.0))
    assert wide["selected_count"].tolist() == [1, 1]


def test_envelope():
    from graspldm_amd import _lib as L
    from graspldm_amd.pointcloud import KNN_MAX_POINTS, estimate_normals, knn_radius
    pc = torch.from_numpy(_cloud(1, 64)).cuda()
    for k in (0, 17):
        with pytest.raises(NotImplementedError, match="16"):
            knn_radius(pc, k, 0.05)
        with pytest.raises(NotImplementedError, match="16"):
            estimate_normals(pc, k=k)
    with pytest.raises(NotImplementedError, match="2\\^20"):
        knn_radius(torch.zeros(KNN_MAX_POINTS + 1, 3, device="cuda"), 3, 0.05)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        knn_radius(pc.cpu(), 3, 0.05)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        estimate_normals(pc.cpu())
    bad = pc.clone()
    bad[0, 5, 1] = float("nan")
    with pytest.raises(L.GldmError, match="non-finite"):
        knn_radius(bad, 3, 0.05)
    bad[0, 5, 1] = float("inf")
    with pytest.raises(L.GldmError, match="non-finite"):
        estimate_normals(bad)
    for r in (-1.0, float("nan"), float("inf"), 1e20):                             # r2 must be finite in f32: +inf is d2's padding
        with pytest.raises(ValueError):
            knn_radius(pc, 3, r)
    # the C entries decide the envelope before they read a pointer or touch the device
    h = L.lib()
    assert h.gldm_knn_radius(None, 1, 10, 17, 0.1, None, 0, None, None, None, None) == -3
    assert h.gldm_knn_radius(None, 1, 10, 0, 0.1, None, 0, None, None, None, None) == -3
    assert h.gldm_knn_radius(None, 1, KNN_MAX_POINTS + 1, 3, 0.1, None, 0, None, None, None, None) == -3
    assert h.gldm_knn_radius(None, 1, 10, 3, float("inf"), None, 0, None, None, None, None) == -1
    assert h.gldm_knn_radius(None, 1, 10, 3, 1e20, None, 0, None, None, None, None) == -1
    assert h.gldm_knn_radius_workspace_bytes(1, KNN_MAX_POINTS + 1) == -3
    assert h.gldm_knn_radius_workspace_bytes(2, 257) == 2 * 2 * 6 * 4
    assert h.gldm_point_normals(None, None, None, 1, 10, 17, None, None, None) == -3
    assert h.gldm_grasp_contact_normals(None, None, None, 1, 1, (1 << 24) + 1, None, 0, 0.006, 0.5, None, None, None) == -3
