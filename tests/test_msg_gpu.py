"""GPU: multi-scale set abstraction.  gldm_ball_query_multi against one gldm_ball_query per radius and against the scalar
C oracle (bitwise), gldm_group_max_concat against amax (bitwise), the U = 128 fold against the U = 64 route (bitwise), the multi-scale
PointNetSAModule and PointNet2MSG against the reference (tests/golden/sa_msg.npz, pointnet2_msg.npz: written by
tools/make_golden_msg.py, which also checked that no point of these inputs sits within 1e-5 r^2 of a ball's surface, so no
element is left out of a comparison).

The bar against the reference: the project's figure for the kind of module (2e-5 / 5e-5 for the first / second
set-abstraction module, 1e-4 for a backbone) where 4 d is below it, else 4 d -- d = max |f32 - f64| of the reference module
on the same inputs, stored in the fixture (both sides are f32 chains of the same length with different summation orders).
Recorded d: 8.4e-7 / 6.5e-7 (modules), 4.5e-7 (backbone): the project's figures hold."""
import pytest
import torch

from conftest import load_golden, load_schema

pytestmark = pytest.mark.gpu

SCALE = 0.05 / 0.12
SA1 = dict(num_centers=64, radius=[0.2, 0.4], num_neighbors=[32, 128], in_channels=5,
           out_channels=[(32, 32, 64), (64, 96, 128)])
SA2 = dict(num_centers=16, radius=[0.8], num_neighbors=[128], in_channels=192, out_channels=[(128, 196, 256)])


def _err(a, b):
    return (a.detach().cpu().float() - b.detach().cpu().float()).abs().max().item()


def _bar(project, d):
    return max(project, 4.0 * float(d))


def _cloud(index, n_points):
    from graspldm_amd import synthetic
    pc, _ = synthetic.normalize_cloud(synthetic.synthetic_cloud(int(index), n_points))
    return (pc.t() * SCALE).contiguous()


# ---------------------------------------------------------------------------------------------- gldm_ball_query_multi
def _check_multi(centers, points, radii, us):
    from graspldm_amd.backend import _backend
    from oracle.cpu_backend import _backend as _oracle
    got = _backend.ball_query_multi(centers, points, radii, us)
    assert len(got) == len(radii)
    exp = [_backend.ball_query(centers, points, r, u) for r, u in zip(radii, us)]
    for g, e, r, u in zip(got, exp, radii, us):
        assert g.dtype == torch.int32 and g.shape == e.shape and torch.equal(g, e), (r, u)
        # both entries run one scan body (csrc/ball_query.h), so their agreement says nothing about it: the scalar C
        # oracle is the judge
        assert torch.equal(g.cpu(), _oracle.ball_query(centers.cpu(), points.cpu(), r, u)), (r, u)
    return exp


def _points(b, n, seed):
    return torch.rand(b, 3, n, generator=torch.Generator().manual_seed(seed))


def test_ball_query_multi_three_radii_empty_and_full_balls():
    pts = _points(2, 200, 1)                      # 200: not a multiple of the 64 candidates of a step
    ctr = pts[:, :, ::8][:, :, :24].clone()
    ctr[:, :, 5] = 50.0                           # a centre far from every point: empty at every radius
    exp = _check_multi(ctr.cuda(), pts.cuda(), (0.05, 0.3, 5.0), (8, 64, 128))
    assert all(int(e[:, 5].abs().max()) == 0 for e in exp)                     # the empty balls are all zeros
    tiny = exp[0][:, [j for j in range(24) if j != 5]]
    assert (tiny == tiny[:, :, :1]).all(dim=2).any()                           # some tiny balls hold their centre alone
    big = exp[2][0, 0].cpu()
    assert torch.equal(big, torch.arange(128, dtype=torch.int32))              # r = 5 fills from the first 128 points


@pytest.mark.parametrize("radii,us", [((0.25,), (16,)), ((0.1, 0.2, 0.4, 0.8), (32, 64, 128, 1)),
                                      ((0.4, 0.1, 0.8, 0.2), (3, 128, 7, 64))])
def test_ball_query_multi_one_and_four_scales(radii, us):
    pts = _points(2, 333, 2)
    ctr = pts[:, :, 3::9].contiguous()            # 37 centres: more than two blocks of 16, the last one partial
    _check_multi(ctr.cuda(), pts.cuda(), radii, us)


def test_ball_query_multi_above_the_lds_staging_limit():
    pts = _points(1, 5200, 3)                     # 5200 > 5120: read through L2
    ctr = pts[:, :, [0, 1700, 5150, 5199]].contiguous()
    _check_multi(ctr.cuda(), pts.cuda(), (0.05, 0.2, 0.6), (16, 64, 128))


def test_ball_query_multi_duplicated_points():
    base = _points(2, 50, 4)
    pts = torch.cat([base, base, base[:, :, :30]], dim=2).contiguous()         # every point two or three times
    ctr = base[:, :, :20].contiguous()
    exp = _check_multi(ctr.cuda(), pts.cuda(), (1e-3, 0.3), (4, 64))
    first = exp[0].cpu()
    for j in range(20):                           # a centre's own copies, in index order: j, j + 50, j + 100
        assert first[0, j].tolist() == [j, j + 50, j + 100, j]


# ---------------------------------------------------------------------------------------------- gldm_group_max_concat
@pytest.mark.parametrize("h", [1, 2, 4])
@pytest.mark.parametrize("m", [37, 40])
def test_group_max_concat(h, m):
    """C = 20, M = 37 (odd: unaligned rows, the scalar forms and the 4-column tail) and 40 (the 16-byte forms), c0 = 3,
    Ctot = 40; the other rows keep their sentinel."""
    from graspldm_amd.backend import _backend
    b, c, c0, ctot = 2, 20, 3, 40
    part = torch.randn(b, c, m * h, generator=torch.Generator().manual_seed(10 + h)).cuda()
    out = torch.full((b, ctot, m), -7.5, device="cuda")
    assert _backend.group_max_concat(part, h, out, c0) is out
    assert torch.equal(out[:, c0:c0 + c], part.view(b, c, m, h).amax(dim=3))
    assert (out[:, :c0] == -7.5).all() and (out[:, c0 + c:] == -7.5).all()


# ------------------------------------------------------------------------------------------------------ the fold
@pytest.mark.parametrize("reps", [2, 4])
@pytest.mark.parametrize("f32_only", [False, True])
def test_u128_route_equals_u64_route_bitwise(f32_only, reps):
    """One branch, U = 64, and the same branch handed [B, M, 128] (and [B, M, 256]) indices that repeat the first 64: the
    fold adds no arithmetic, so the two agree bit for bit."""
    from graspldm_amd import numerics
    from graspldm_amd.backend import _backend
    from graspldm_amd.pvcnn import SharedMLP
    from graspldm_amd.sa_pack import SaMlpPlan
    from graspldm_amd.synthetic import load_synthetic_weights
    mlp = load_synthetic_weights(SharedMLP(8, [64, 96, 128], dim=2), seed=21).cuda().eval()
    pts = _points(2, 200, 5).cuda()
    feats = torch.randn(2, 5, 200, generator=torch.Generator().manual_seed(6)).cuda()
    ctr = pts[:, :, ::8][:, :, :24].contiguous()
    idx64 = _backend.ball_query(ctr, pts, 0.3, 64)
    idx128 = torch.cat([idx64] * reps, dim=2).contiguous()
    with numerics.f32_only(f32_only), torch.no_grad():
        plan = SaMlpPlan(mlp, pts.device)
        a = plan.run_msg(pts, ctr, feats, idx64, torch.zeros(2, 128, 24, device="cuda"), 0)
        b = plan.run_msg(pts, ctr, feats, idx128, torch.zeros(2, 128, 24, device="cuda"), 0)
    assert a.abs().max() > 0 and torch.equal(a, b)


# ------------------------------------------------------------------------------------- the modules against the reference
@pytest.fixture(scope="module")
def sa_golden():
    return load_golden("sa_msg.npz")


@pytest.fixture(scope="module")
def sa_modules():
    from graspldm_amd.pvcnn import PointNetSAModule
    from graspldm_amd.synthetic import load_synthetic_weights
    sa1 = load_synthetic_weights(PointNetSAModule(**SA1), seed=11).cuda().eval()
    sa2 = load_synthetic_weights(PointNetSAModule(**SA2), seed=12).cuda().eval()
    return sa1, sa2


def _grouped_bytes(batch, kw):
    """The [B, 3 + C, M, U] tensor of the module's widest branch, f32."""
    return batch * (3 + kw["in_channels"]) * kw["num_centers"] * max(kw["num_neighbors"]) * 4


def _peak_delta(fn):
    fn()                                          # warm-up: plans packed, allocator pools grown
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("f32_only", [False, True])
def test_multi_scale_sa_modules_against_the_reference(sa_golden, sa_modules, f32_only):
    from graspldm_amd import numerics
    g = sa_golden
    sa1, sa2 = sa_modules
    feats = torch.randn(2, 5, 256, generator=torch.Generator().manual_seed(53)).cuda()
    coords = torch.stack([_cloud(i, 256) for i in g["clouds"]]).cuda()
    with numerics.f32_only(f32_only), torch.no_grad():
        (f1, c1), peak1 = _peak_delta(lambda: sa1((feats, coords)))
        (f2, c2), peak2 = _peak_delta(lambda: sa2((f1, c1)))
    e1, e2 = _err(f1, g["f1"]), _err(f2, g["f2"])
    print(f"f32_only={f32_only}: err f1 {e1:.3e} (d {float(g['d1']):.3e}), f2 {e2:.3e} (d {float(g['d2']):.3e}); "
          f"peak {peak1} / {peak2} bytes, grouped {_grouped_bytes(2, SA1)} / {_grouped_bytes(2, SA2)}")
    assert f1.shape == (2, 192, 64) and f2.shape == (2, 256, 16)
    assert torch.equal(c1.cpu(), g["c1"]) and torch.equal(c2.cpu(), g["c2"])
    assert e1 < _bar(2e-5, g["d1"]), e1
    assert e2 < _bar(5e-5, g["d2"]), e2
    # no tensor with M * U columns: the whole call stays below the grouped input of its widest branch alone
    assert peak1 < _grouped_bytes(2, SA1), (peak1, _grouped_bytes(2, SA1))
    assert peak2 < _grouped_bytes(2, SA2), (peak2, _grouped_bytes(2, SA2))


def test_pointnet2_msg_against_the_reference():
    from graspldm_amd.pvcnn import PointNet2MSG
    from graspldm_amd.synthetic import synthetic_state_dict
    g = load_golden("pointnet2_msg.npz")
    net = PointNet2MSG(num_shapes=4)
    net.load_state_dict(synthetic_state_dict(load_schema("schema_pointnet2_msg.json"), seed=13), strict=True)
    net = net.cuda().eval()
    extra = torch.randn(2, 3, 1024, generator=torch.Generator().manual_seed(59))
    onehot = torch.zeros(2, 4, 1024)
    for b in range(2):
        onehot[b, b % 4] = 1.0
    x = torch.cat([torch.stack([_cloud(i, 1024) for i in g["clouds"]]), extra, onehot], dim=1).cuda()
    with torch.no_grad():
        out = net(x)
        again = net(x)
    e = _err(out[:, :, ::8], g["out"])
    print(f"PointNet2MSG: err {e:.3e} (d {float(g['d']):.3e})")
    assert out.shape == (2, 128, 1024)
    assert e < _bar(1e-4, g["d"]), e
    assert torch.equal(out, again)
