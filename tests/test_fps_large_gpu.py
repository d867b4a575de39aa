"""GPU: gldm_farthest_points_euclid_large (csrc/fps.hip) against oracle.front_end.farthest_points, the numpy
restatement pinned to the reference by tests/golden/front_end.npz.  Indices must be equal.

The kernel cuts a cloud into slices of gldm_farthest_points_euclid_large_slice(n) rows (1024 up to n = 2^19, then doubling
so that there are at most 512 slices): 8193 rows are 9 slices, 20011 are 20, neither a multiple of 1024; 2^19 + 7 and
2^22 take the 2048- and 8192-row slices (few rounds there: the oracle's cost is n per round)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 3, generator=g) * torch.tensor([0.2, 0.1, 0.05]) + torch.tensor([0.3, -0.1, 0.8])).contiguous()


_ORACLE = {}


def _oracle(n, seed, m):
    """Oracle indices for the first m picks of cloud (n, seed); computed once for the largest m asked (greedy: a prefix)."""
    from oracle import front_end as F
    key = (n, seed)
    if key not in _ORACLE or len(_ORACLE[key]) < m:
        _ORACLE[key] = F.farthest_points(_cloud(n, seed).numpy(), max(m, 300 if n == 20011 else m))
    return torch.from_numpy(_ORACLE[key][:m].astype(np.int32))


@pytest.mark.parametrize("n,m", [(8193, 1), (8193, 64), (20011, 64), (20011, 300), ((1 << 19) + 7, 3), (1 << 22, 2)])
def test_random_clouds_against_the_oracle(n, m):
    from graspldm_amd import _lib as L
    from graspldm_amd.pointcloud import farthest_point_indices
    slice_rows = L.lib().gldm_farthest_points_euclid_large_slice(n)
    if n <= 20011:   # the issue's shapes: no multiple of the slice, at least three slices
        assert n % slice_rows != 0 and -(-n // slice_rows) >= 3
    idx = farthest_point_indices(_cloud(n, 3).cuda(), m)
    assert idx.shape == (1, m) and idx.dtype == torch.int32
    assert torch.equal(idx[0].cpu(), _oracle(n, 3, m))


def test_two_clouds_with_counts_against_each_alone():
    from graspldm_amd.pointcloud import farthest_point_indices, farthest_point_indices_large
    a, b = _cloud(20011, 3), _cloud(9000, 4)
    both = torch.full((2, 20011, 3), float("nan"))
    both[0], both[1, :9000] = a, b
    both[1, 9000:12000] = 1e30
    counts = torch.tensor([20011, 9000], dtype=torch.int32).cuda()
    idx = farthest_point_indices_large(both.cuda(), 64, counts=counts)
    assert torch.equal(idx[0].cpu(), _oracle(20011, 3, 64))
    assert torch.equal(idx[1], farthest_point_indices(b.cuda(), 64)[0])
    assert torch.equal(idx[1].cpu(), _oracle(9000, 4, 64))


def test_count_not_above_m_gives_arange_then_minus_one():
    from graspldm_amd.pointcloud import farthest_point_indices_large
    pc = torch.full((2, 9001, 3), float("nan"))
    pc[:, 1::2] = 1e30   # rows past the counts are poison: never read
    pc[0, :40] = _cloud(40, 5)
    pc[1, :64] = _cloud(64, 6)
    idx = farthest_point_indices_large(pc.cuda(), 64, counts=torch.tensor([40, 64], dtype=torch.int32).cuda()).cpu()
    assert torch.equal(idx[0, :40], torch.arange(40, dtype=torch.int32)) and bool((idx[0, 40:] == -1).all())
    assert torch.equal(idx[1], torch.arange(64, dtype=torch.int32))


def test_exact_ties_go_to_the_lowest_index():
    from oracle import front_end as F
    from graspldm_amd.pointcloud import farthest_point_indices
    ax = torch.arange(0, 22, dtype=torch.float32)
    lattice = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)[:10000].contiguous()
    assert lattice.shape[0] == 10000
    got = farthest_point_indices(lattice.cuda(), 48)[0].cpu()
    assert torch.equal(got, torch.from_numpy(F.farthest_points(lattice.numpy(), 48)))
    half = _cloud(4600, 8)
    dup = torch.cat([half, half]).contiguous()   # 9200 rows, every distance twice
    got = farthest_point_indices(dup.cuda(), 48)[0].cpu()
    assert torch.equal(got, torch.from_numpy(F.farthest_points(dup.numpy(), 48))) and bool((got < 4600).all())


def test_below_the_threshold_the_old_entry_is_the_only_path():
    import ctypes
    from graspldm_amd import _lib as L
    from graspldm_amd.pointcloud import farthest_point_indices
    pc = _cloud(5000, 9).cuda()
    ws = torch.empty(1 << 16, dtype=torch.int64, device="cuda")
    out = torch.full((1, 16), -9, dtype=torch.int32, device="cuda")
    st = L.lib().gldm_farthest_points_euclid_large(L.ptr(pc), None, 1, 5000, 16, L.ptr(ws), ctypes.c_longlong(ws.numel() * 8),
                                                   L.ptr(out), L.current_stream())
    assert st == -3 and bool((out == -9).all())
    old = torch.empty((1, 16), dtype=torch.int32, device="cuda")
    L.call("gldm_farthest_points_euclid", L.ptr(pc.unsqueeze(0).contiguous()), 1, 5000, 16, L.ptr(old), L.current_stream())
    assert torch.equal(farthest_point_indices(pc, 16), old)
    assert torch.equal(old[0].cpu(), _oracle(5000, 9, 16))


def test_two_calls_are_bitwise_equal():
    from graspldm_amd.pointcloud import farthest_point_indices
    pc = _cloud(20011, 3).cuda()
    assert torch.equal(farthest_point_indices(pc, 300), farthest_point_indices(pc, 300))


def test_regularize_pc_point_count_on_a_sensor_sized_cloud():
    from oracle import front_end as F
    from graspldm_amd.pointcloud import PointCloudHelpers as P
    pc = _cloud(20011, 3)
    exp = F.regularize_pc_point_count(pc.numpy(), 1024, use_farthest_point=True)
    got = P.regularize_pc_point_count(pc.cuda(), 1024, use_farthest_point=True)
    assert torch.equal(got.cpu(), torch.from_numpy(exp))
