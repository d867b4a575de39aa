"""GPU (MI355X): the reference's OWN point-op kernels -- its six .cu files compiled unmodified for gfx950 by
oracle/ref_build.py, reached through oracle/ref_backend.py -- as the authority over both the C oracle and the HIP kernels.

Per case of oracle/ref_cases.CASES, on the same seeded inputs:

  T1  oracle.cpu_backend             == ref_backend.strict      bit for bit, every output
  T2  graspldm_amd.backend._backend  == ref_backend.strict      bit for bit, every output
      (and the fused entries gldm_sa_group / gldm_ball_query_multi against reference ball_query -> grouping - centres)
  T3  ref_backend.default vs ref_backend.strict (contraction sensitivity): every integer difference needs a tie
      witness computed in f64 from the inputs, and at most 2 % of a case's rows may differ; float outputs must be
      finite, their largest ulp distance is printed (a measurement of the reference against itself, not a bar).

One stated exception to bit-exactness: `out` of avg_voxelize, which the reference sums with float atomics in no fixed
order.  Every implementation must keep each voxel within (cnt + 1) * 2^-24 * sum|feat_i| / cnt of the f64 mean: one
rounding of 1/cnt, one per product, one per addition, in any order.

Tie witness (T3).  Both builds evaluate d^2 as a sum of three non-negative terms with at most five roundings, each within
2^-24 of a partial sum <= d^2, so two evaluations of one d^2 differ by less than 8 * 2^-24 * d^2 and a decision can flip only
where the quantities compared are that close in exact arithmetic:
  ball query  a point of that centre with |d^2 - r^2| <= 8 * 2^-24 * r^2
  3-NN        the two centres that swapped at the first differing rank: |d_a^2 - d_b^2| <= 8 * 2^-24 * max
  FPS         the sequences agree up to a first round j*; both picks at j* lie within that relative bound of the maximal
              f64 min-distance to the common prefix; after j* nothing is compared.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_backend, ref_cases

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_backend.available(),
                                 reason="oracle/_ref/libpvcnn_ref*.so not built (build() compiles them where the "
                                        "reference tree is present)")]

EPS = 8.0 * 2.0 ** -24
MAX_FLIP_FRACTION = 0.02
CASES = ref_cases.CASES
IDS = [c["name"] for c in CASES]
INT_OUTPUTS = {"fps": ("indices",), "ball_query": ("indices",), "grouping": (), "three_nn": ("indices",),
               "voxelize": ("ind", "cnt"), "devoxelize": ("inds",)}


@functools.lru_cache(maxsize=None)
def _results(i):
    """Inputs and the outputs of the four implementations for case i, computed once and shared by T1/T2/T3."""
    from graspldm_amd.backend import _backend as hip
    from oracle.cpu_backend import _backend as cpu
    c = CASES[i]
    op, p = c["op"], c["params"]
    x = ref_cases.make_inputs(op, p)
    xd = {k: v.cuda() for k, v in x.items()}
    to_cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    return {"x": x,
            "oracle": ref_cases.run(cpu, op, p, x),
            "strict": to_cpu(ref_cases.run(ref_backend.strict, op, p, xd)),
            "default": to_cpu(ref_cases.run(ref_backend.default, op, p, xd)),
            "hip": to_cpu(ref_cases.run(hip, op, p, xd))}


def _voxel_bound_holds(x, got):
    """avg_voxelize `out` against the f64 mean, per voxel and channel."""
    feat, vc = x["features"].double(), x["coords"].long()
    b, c, n = feat.shape
    r3 = got["cnt"].shape[1]
    r = round(r3 ** (1.0 / 3))
    flat = (vc[:, 0] * r * r + vc[:, 1] * r + vc[:, 2]).unsqueeze(1).expand(b, c, n)
    s = torch.zeros(b, c, r3, dtype=torch.float64).scatter_add_(2, flat, feat)
    sabs = torch.zeros(b, c, r3, dtype=torch.float64).scatter_add_(2, flat, feat.abs())
    cnt = got["cnt"].double().unsqueeze(1)
    mean = s / cnt.clamp(min=1)
    bound = (cnt + 1) * 2.0 ** -24 * sabs / cnt.clamp(min=1)
    err = (got["out"].double() - mean).abs()
    assert bool((err <= bound).all()), f"worst excess {(err - bound).max().item():.3e}"
    assert bool((got["out"][(cnt == 0).expand_as(err)] == 0).all())


def _assert_same(op, x, got, exp, who):
    for k in exp:
        if (op, k) == ("voxelize", "out"):
            _voxel_bound_holds(x, got)
            continue
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (who, k)
        assert torch.equal(got[k], exp[k]), f"{who}: `{k}` differs from the reference kernel at " \
                                            f"{int((got[k] != exp[k]).sum())} of {exp[k].numel()} elements"


def test_case_generators_are_those_of_the_product_tests():
    """ref_cases restates the input recipes of test_point_ops_gpu (so the recorder can live outside tests/)."""
    import test_point_ops_gpu as T
    for kind in ("dup", "sym", "grid"):
        for n in (64, 100, 512, 1000, 1024):
            assert torch.equal(ref_cases.tie_cloud(kind, n), T._tie_cloud(kind, n))
    assert torch.equal(ref_cases.cloud(2, 77, 5, 0.5), T._cloud(2, 77, 5, 0.5))
    assert torch.equal(ref_cases.surface_cloud(1, 1024), T._surface_cloud(1, 1024))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_t1_oracle_equals_reference_kernel(i):
    r = _results(i)
    _assert_same(CASES[i]["op"], r["x"], r["oracle"], r["strict"], "oracle/point_ops.c")
    if CASES[i]["op"] == "voxelize":
        _voxel_bound_holds(r["x"], r["strict"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_t2_hip_kernel_equals_reference_kernel(i):
    r = _results(i)
    _assert_same(CASES[i]["op"], r["x"], r["hip"], r["strict"], "libgldm_hip.so")


# ------------------------------------------------------------------------------------------------- T3: tie witnesses
def _d2(a, b):
    """f64 squared distances between [3, A] and [3, B] -> [A, B]."""
    a, b = a.double().numpy(), b.double().numpy()
    d = a[:, :, None] - b[:, None, :]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def _witness_ball_query(x, p, a, b):
    r2 = float(np.float32(np.float32(p["r"]) * np.float32(p["r"])))
    rows = np.argwhere((a != b).any(-1).numpy())
    for bi, j in rows:
        d2 = _d2(x["centers"][bi][:, j:j + 1], x["points"][bi])[0]
        assert (np.abs(d2 - r2) <= EPS * r2).any(), f"cloud {bi} centre {j}: the builds differ with no point on the sphere"
    return len(rows), a.shape[0] * a.shape[1]


def _witness_three_nn(x, a, b):
    rows = np.argwhere((a != b).any(1).numpy())
    for bi, j in rows:
        d2 = _d2(x["points"][bi][:, j:j + 1], x["centers"][bi])[0]
        rank = int(np.argmax((a[bi, :, j] != b[bi, :, j]).numpy()))
        da, db = d2[int(a[bi, rank, j])], d2[int(b[bi, rank, j])]
        assert abs(da - db) <= EPS * max(da, db), f"cloud {bi} point {j} rank {rank}: {da!r} vs {db!r} is no tie"
    return len(rows), a.shape[0] * a.shape[2]


def _witness_fps(x, a, b):
    flips = 0
    for bi in range(a.shape[0]):
        ne = np.flatnonzero((a[bi] != b[bi]).numpy())
        if not len(ne):
            continue
        flips += 1
        j = int(ne[0])
        prefix = a[bi, :j].long()
        mind = _d2(x["coords"][bi], x["coords"][bi][:, prefix]).min(axis=1)
        top = mind.max()
        for pick in (int(a[bi, j]), int(b[bi, j])):
            assert top - mind[pick] <= EPS * top, f"cloud {bi} round {j}: pick {pick} at {mind[pick]!r}, maximum {top!r}"
    return flips, a.shape[0]


def _ulp_distance(a, b):
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_t3_contraction_sensitivity_of_the_reference(i):
    c = CASES[i]
    op, p = c["op"], c["params"]
    r = _results(i)
    x, d, s = r["x"], r["default"], r["strict"]
    flips = total = 0
    if op == "ball_query":
        flips, total = _witness_ball_query(x, p, d["indices"], s["indices"])
    elif op == "three_nn":
        flips, total = _witness_three_nn(x, d["indices"], s["indices"])
    elif op == "fps":
        flips, total = _witness_fps(x, d["indices"], s["indices"])
    else:
        for k in INT_OUTPUTS[op]:    # no float decides these: grid_stats (vox.cu:18-34), the floor of devoxelize
            assert torch.equal(d[k], s[k]), k
    if op in ("ball_query", "three_nn"):
        assert flips <= MAX_FLIP_FRACTION * total, f"{flips} of {total} rows differ between the two builds"
    if op == "voxelize":
        _voxel_bound_holds(x, d)
    ulps = {}
    for k, v in d.items():
        if v.dtype == torch.float32:
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(s[k]).all()), k
            if flips == 0:
                ulps[k] = _ulp_distance(v, s[k])
    print(f"T3 {c['name']}: integer rows differing {flips}/{total}; max ulp default-vs-strict {ulps}")


def test_lattice_ball_query_is_exact_and_strict():
    """Lattice spacing 0.25, r = 0.5: every d^2 is exact in f32 whatever the contraction, and 6 lattice points of each
    interior centre sit at d^2 == r^2 exactly.  All implementations and both builds agree, and no centre's ball holds
    a point on the sphere (a `<=` would)."""
    i = IDS.index("ball_query-kindlattice-b1-n343-m343-u32-r0.5")
    r = _results(i)
    for who in ("oracle", "default", "hip"):
        assert torch.equal(r[who]["indices"], r["strict"]["indices"]), who
    d2 = _d2(r["x"]["centers"][0], r["x"]["points"][0])
    assert ((d2 == 0.25).sum(1) > 0).all() and (d2 == 0.25).sum(1).max() == 6
    idx = r["strict"]["indices"][0].long().numpy()
    hit = np.take_along_axis(d2, idx, axis=1)
    assert (hit < 0.25).all()
    inside = (d2 < 0.25).sum(1)
    assert inside.max() == 27 and all(len(set(idx[j])) == inside[j] for j in range(idx.shape[0]))


# ------------------------------------------------------------------------------- the fused entries against the reference
@pytest.mark.parametrize("b,c,n,m,u,r", [(2, 128, 512, 128, 64, 0.4), (1, 5, 300, 37, 7, 0.5)])
def test_t2_sa_group_equals_reference_composition(b, c, n, m, u, r):
    """gldm_sa_group == reference ball_query -> reference grouping -> minus centres (modules/ball_query.py:16-34)."""
    from graspldm_amd import _lib as L
    ref = ref_backend.strict
    pts = ref_cases.cloud(b, n, 20).cuda()
    ctr = pts[:, :, :m].contiguous()
    feat = torch.randn(b, c, n, generator=torch.Generator().manual_seed(21)).cuda()
    idx = ref.ball_query(ctr, pts, r, u)
    exp = torch.cat([ref.grouping_forward(pts, idx) - ctr.unsqueeze(-1), ref.grouping_forward(feat, idx)], dim=1)
    out = torch.empty(b, 3 + c, m, u, device="cuda")
    io = torch.empty(b, m, u, dtype=torch.int32, device="cuda")
    L.call("gldm_sa_group", L.ptr(pts), L.ptr(ctr), L.ptr(feat), b, c, n, m, r, u, L.ptr(out), L.ptr(io), L.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(io, idx)
    assert torch.equal(out, exp)


def test_t2_ball_query_multi_equals_reference_per_radius():
    """gldm_ball_query_multi (one scan, three radii) == the reference's ball_query run once per radius."""
    from graspldm_amd.backend import _backend as hip
    pts = ref_cases.cloud(1, 1024, 20).cuda()
    ctr = pts[:, :, :256].contiguous()
    radii, us = [0.1, 0.2, 0.4], [16, 32, 64]
    got = hip.ball_query_multi(ctr, pts, radii, us)
    torch.cuda.synchronize()
    for g, r, u in zip(got, radii, us):
        assert torch.equal(g, ref_backend.strict.ball_query(ctr, pts, r, u)), r


def test_reference_backend_refuses_out_of_range_indices():
    """The reference kernels index unchecked; the front end must raise BEFORE a launch."""
    f = torch.zeros(1, 2, 8, device="cuda")
    with pytest.raises(RuntimeError, match="outside"):
        ref_backend.strict.grouping_forward(f, torch.full((1, 2, 2), 8, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="outside"):
        ref_backend.strict.gather_features_forward(f, torch.full((1, 2), -1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="outside"):
        ref_backend.strict.avg_voxelize_forward(f, torch.full((1, 3, 8), 4, dtype=torch.int32, device="cuda"), 4)
    with pytest.raises(RuntimeError, match="outside"):
        ref_backend.strict.trilinear_devoxelize_forward(2, False, torch.full((1, 3, 4), 1.5, device="cuda"),
                                                        torch.zeros(1, 1, 8, device="cuda"))
