"""CPU: the restatements of tests/normals_ref.py against what they restate, and the host logic of the friction-cone filter.

  * the f32 search (lexsort on (d2, index)) finds the neighbour SETS of scipy's cKDTree.query(k, distance_upper_bound,
    workers=-1) -- the reference's call (pointcloud_helpers.py:85-88) with the keyword scipy takes today -- on the three
    half-sphere cases; measured here: 0 points differ in all three;
  * the f64 normals agree with the reference's f32 formula (diffs^T diffs / k^2, numpy.linalg.eig, smallest eigenvalue) to
    2^-20 per component on the first of them; measured here: worst 1.8e-7, every gap ratio >= 0.047;
  * GraspSelection validates its new fields, the CLI parses the new flags, a plain run's arguments are unchanged.
"""
import numpy as np
import pytest

import normals_ref as ref

CASES = [(2000, 0.05), (2000, 0.008), (4000, 0.004)]   # half-sphere: n, radius
K = 12


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_restated_search_finds_scipys_neighbour_sets(case):
    spatial = pytest.importorskip("scipy.spatial")
    n, r = case
    pc = ref.half_sphere(n)
    idx, d2, found = ref.knn_radius(pc, K, r)
    tree = spatial.cKDTree(pc, leafsize=n + 1)
    _, ndx = tree.query(pc, k=K, distance_upper_bound=r, workers=-1)
    differ = sum(set(a.tolist()) != set(b.tolist()) for a, b in zip(idx, ndx))
    print(f"half-sphere n={n} r={r}: {differ} of {n} points differ; found {found.min()} .. {found.max()}")
    assert differ == 0
    assert (idx[:, 0] == np.arange(n)).all() and (d2[:, 0] == 0).all()          # the point itself comes first
    assert ((idx == n) == np.isinf(d2)).all() and ((idx != n).sum(-1) == found).all()
    live = np.where(np.isinf(d2), np.float32(0), d2)
    assert (np.diff(live, axis=1)[idx[:, 1:] != n] >= 0).all()                    # ascending d2 over the live slots


def test_f64_normals_agree_with_the_references_f32_formula():
    n, r = CASES[0]
    pc = ref.half_sphere(n)
    idx, _, found = ref.knn_radius(pc, K, r)
    assert found.min() >= 3
    want, w, _, _ = ref.normals_f64(pc, idx)
    got = ref.normals_reference_f32(pc, idx)
    ratio = ref.gap_ratio(w)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"reference f32 formula against f64: worst component error {err:.3g}, smallest gap ratio {ratio.min():.3g}")
    assert ratio.min() >= 0.037
    assert err <= 2.0 ** -20
    assert np.abs(np.linalg.norm(want, axis=1) - 1.0).max() < 1e-12
    assert ((want * pc.astype(np.float64)).sum(-1) < 0).all()                     # towards the camera


def test_search_restatement_orders_ties_by_index_and_pads():
    pc = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [5, 5, 5]], dtype=np.float32)
    idx, d2, found = ref.knn_radius(pc, 3, 1.5)
    assert idx[0].tolist() == [0, 1, 2] and d2[0].tolist() == [0.0, 1.0, 1.0]   # 1, 2, 3 tie: lowest indices
    assert idx[4].tolist() == [4, 5, 5] and found.tolist() == [3, 3, 3, 3, 1]
    assert np.isinf(d2[4, 1:]).all()
    idx, _, found = ref.knn_radius(pc[:2], 3, 10.0)                               # fewer points than k
    assert idx.tolist() == [[0, 1, 2], [1, 0, 2]] and found.tolist() == [2, 2]


def test_selection_validates_the_new_fields():
    from graspldm_amd.grasp_select import GraspSelection
    s = GraspSelection()
    assert (s.min_aligned_contacts, s.friction_angle_deg, s.both_fingers, s.normals_k, s.normals_radius) == (0, 30.0, False, 12, 0.05)
    assert not s.needs_normals and not s.needs_scene and not s.needs_clearance
    s = GraspSelection(min_aligned_contacts=3, both_fingers=True, friction_angle_deg=90)
    assert s.needs_normals and s.needs_scene and not s.needs_clearance
    assert GraspSelection(min_contacts=1).needs_scene and not GraspSelection(min_contacts=1).needs_normals
    for bad in (dict(min_aligned_contacts=-1), dict(min_aligned_contacts=1.5), dict(min_aligned_contacts=True),
                dict(friction_angle_deg=0.0), dict(friction_angle_deg=90.5), dict(friction_angle_deg=float("nan")),
                dict(both_fingers=1), dict(normals_k=2), dict(normals_k=17), dict(normals_k=12.0),
                dict(normals_radius=0.0), dict(normals_radius=float("inf"))):
        with pytest.raises(ValueError):
            GraspSelection(**bad)


def test_cli_parses_the_friction_cone_flags_and_leaves_a_plain_run_alone():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import generate_grasps as cli
    old = cli.parse_args(["--synthetic", "64", "--mode", "LDM"])
    assert cli.build_selection(old) is None and cli.selection_kwargs(old, None, 0) == {}
    new = cli.parse_args(["--synthetic", "64", "--mode", "LDM", "--min_aligned_contacts", "4", "--friction_angle", "25",
                          "--both_fingers", "--normals_k", "8", "--normals_radius", "0.02"])
    sel = cli.build_selection(new)
    assert (sel.min_aligned_contacts, sel.friction_angle_deg, sel.both_fingers, sel.normals_k, sel.normals_radius) == (4, 25.0, True, 8, 0.02)
    assert sel.needs_normals and not sel.needs_clearance and sel.min_contacts == 0 and not sel.collision_free
    only = cli.build_selection(cli.parse_args(["--synthetic", "64", "--mode", "LDM", "--min_contacts", "2"]))
    assert not only.needs_normals and only.min_aligned_contacts == 0
    for argv in (["--both_fingers"], ["--friction_angle", "20"], ["--normals_k", "8"],
                 ["--min_aligned_contacts", "2", "--friction_angle", "0"], ["--min_aligned_contacts", "2", "--normals_k", "2"]):
        with pytest.raises(SystemExit):
            cli.build_selection(cli.parse_args(["--synthetic", "64", "--mode", "LDM"] + argv))
