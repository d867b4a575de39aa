"""CPU: the f64 restatement of the voxel tail (tests/voxel_tail_ref.py) is right before it judges a kernel -- against the
oracle's devoxelize, against the tail of oracle.torch_ref.pvconv, and on a linear field -- and the status codes of the
tail's entry points (csrc/voxel_norm.hip), every one of them returned before anything is launched.

gldm_groupnorm_coef's `c % groups` and `c / groups > 128` are asserted by tests/test_voxel_attention_cpu.py
(test_new_entries_reject_bad_arguments_without_launching) and not again here."""
import pytest
import torch
import torch.nn.functional as F

import voxel_tail_ref as T
from test_voxel_attention_cpu import _host_ptr


@pytest.mark.parametrize("r", [5, 8])
def test_devoxelize_against_the_oracle(r):
    """f64 against the oracle's f32 trilinear_devoxelize_forward, 1e-6 relative to the largest output: random coordinates
    in [0, r - 1) plus points on voxels (a whole cloud position, single axes, the two end corners)."""
    from oracle.cpu_backend import _backend as B
    g = torch.Generator().manual_seed(r)
    b, c, n = 2, 7, 200
    coords = torch.rand(b, 3, n, generator=g) * (r - 1)
    coords[:, :, 0] = 0.0
    coords[:, :, 1] = r - 1
    coords[:, :, 2] = torch.tensor([2.0, 1.0, 3.0]).view(1, 3)
    coords[:, 0, 3], coords[:, 1, 4], coords[:, 2, 5] = r - 1, r - 1, 0.0
    grid = torch.randn(b, c, r, r, r, generator=g)
    want = B.trilinear_devoxelize_forward(r, False, coords.contiguous(), grid.view(b, c, -1).contiguous())[0]
    got = T.devoxelize(coords, grid, None, None, r)
    assert got.dtype == torch.float64 and got.shape == (b, c, n)
    err = (got - want.double()).abs().max().item()
    print(f"devoxelize r={r}: f64 restatement vs f32 oracle {err:.2e}")
    assert err <= 1e-6 * want.abs().max().item(), err
    gate, add = torch.rand(b, c, generator=g), torch.randn(b, c, n, generator=g)
    full = T.devoxelize(coords, grid, gate, add, r)
    assert torch.equal(full, got * gate.double().unsqueeze(-1) + add.double())


@pytest.mark.parametrize("r", [4, 7])
def test_devoxelize_reproduces_a_linear_field_at_integer_coordinates(r):
    """grid = 2 x + 3 y + 5 z at EVERY voxel centre, the corners (0, 0, 0) and (r - 1, r - 1, r - 1) included: exactly
    (small integers in f64: the upper corner of an axis without a fractional part must not be read at lo + 1, which at
    r - 1 is another row of the grid or past its end).  Between the voxels a linear field is reproduced to rounding."""
    ax = torch.arange(r, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    field = 2 * x + 3 * y + 5 * z
    grid = torch.stack([field, -field + 1]).unsqueeze(0)                    # [1, 2, r, r, r]
    coords = torch.stack([x.flatten(), y.flatten(), z.flatten()]).unsqueeze(0)
    assert coords[0, :, 0].tolist() == [0, 0, 0] and coords[0, :, -1].tolist() == [r - 1] * 3
    got = T.devoxelize(coords, grid, None, None, r)
    assert torch.equal(got[0, 0], field.flatten().double()) and torch.equal(got[0, 1], 1 - field.flatten().double())
    g = torch.Generator().manual_seed(r)
    pts = torch.rand(1, 3, 100, generator=g) * (r - 1)
    pd = pts.double()
    want = 2 * pd[:, 0] + 3 * pd[:, 1] + 5 * pd[:, 2]
    assert (T.devoxelize(pts, grid, None, None, r)[:, 0] - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("se_relu", [False, True])
def test_chain_against_the_tail_of_the_oracle_pvconv(se_relu):
    """squeeze -> se_gate -> devoxelize of swish_affine, fed with the raw second conv and its GroupNorm as coefficients,
    against oracle.torch_ref.pvconv (f32) on one small PVConv: sums against means, the weights' orientation, the gate's
    and the addend's place.  1e-5 of the largest output: the oracle's own f32 arithmetic (a GroupNorm over 3 x 125
    values, eight products per point)."""
    from graspldm_amd.pvcnn import PVConv
    from graspldm_amd.synthetic import load_synthetic_weights
    from oracle import torch_ref as R
    cin, c, r, b, n = 4, 32, 5, 2, 60
    net = load_synthetic_weights(PVConv(cin, c, 3, resolution=r, with_se=True, with_se_relu=se_relu), seed=3)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    features = torch.randn(b, cin, n, generator=g)
    coords = torch.randn(b, 3, n, generator=g) * 0.3
    want = R.pvconv(sd, "", features, coords, r, True, se_relu)
    # the front of the block from the oracle's own pieces, up to the RAW second conv
    vox, nc = R.voxelize(features, coords, r, True)
    v = "voxel_layers."
    h = F.conv3d(vox, sd[v + "0.weight"], sd[v + "0.bias"], padding=1)
    h = F.group_norm(h, 8, sd[v + "1.weight"], sd[v + "1.bias"], eps=1e-5)
    y = F.conv3d(h * torch.sigmoid(h), sd[v + "4.weight"], sd[v + "4.bias"], padding=1)
    # its GroupNorm(8) as (a, s) per (cloud, channel)
    yg = y.double().view(b, 8, -1)
    mean, var = yg.mean(-1), yg.var(-1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(c // 8, dim=1)
    mean = mean.repeat_interleave(c // 8, dim=1)
    a = sd[v + "5.weight"].double() * rstd
    coef = torch.stack([a, sd[v + "5.bias"].double() - mean * a], dim=-1).float()
    gate = T.se_gate(T.squeeze(y, coef), sd[v + "7.fc.0.weight"], sd[v + "7.fc.2.weight"], r, se_relu)
    # the synthetic SE weights are small, the gates near 0.5: still hundreds of times the tolerance away from a constant
    assert gate.shape == (b, c) and (gate - gate.mean()).abs().max().item() > 3e-3
    add = R.shared_mlp(sd, "point_features.", features)
    got = T.devoxelize(nc, T.swish_affine(y, coef), gate, add, r)
    err = (got - want.double()).abs().max().item()
    print(f"chain vs oracle pvconv (relu={se_relu}): {err:.2e} of {want.abs().max().item():.2f}")
    assert err <= 1e-5 * max(1.0, want.abs().max().item()), err


def test_tail_entries_reject_bad_arguments_without_launching():
    from graspldm_amd import _lib as L
    h, p = L.lib(), _host_ptr()

    def nulls(fn, args, required):
        """every required pointer in turn NULL: GLDM_ERR_INVALID_ARG"""
        for i in required:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == -1, (fn.__name__, i)

    nulls(h.gldm_gn_swish_chan_sum, (p, p, 3, 8, 5, p, None), (0, 1, 5))
    nulls(h.gldm_gn_swish_chan_sum_cl, (p, p, 3, 8, 5, p, None), (0, 1, 5))
    nulls(h.gldm_se_gate, (p, p, p, 3, 8, 2, 5, 0, p, None), (0, 1, 2, 8))
    nulls(h.gldm_se_gate_parts, (p, 8, p, p, 3, 8, 2, 5, 0, p, None), (0, 2, 3, 9))
    nulls(h.gldm_devoxelize_fused, (p, p, p, p, 3, 8, 10, 5, p, None), (0, 1, 8))               # gate, add: optional
    nulls(h.gldm_devoxelize_gn_fused, (p, p, p, p, p, 3, 8, 10, 5, p, None), (0, 1, 2, 9))
    nulls(h.gldm_devoxelize_gn_cl_fused, (p, p, p, p, p, 3, 8, 10, 5, p, None), (0, 1, 2, 9))
    nulls(h.gldm_groupnorm_coef, (p, p, p, 3, 8, 5, 8, 1e-5, p, None), (0, 1, 2, 8))
    for parts in (0, -1):
        assert h.gldm_se_gate_parts(p, parts, p, p, 3, 8, 2, 5, 0, p, None) == -1
    # the channel-last kernels read channel quads: the squeeze has 256 threads for up to 256 quads, the devoxelize pass
    # 256 x 65 floats of LDS
    for c in (6, 1, 1023):
        assert h.gldm_gn_swish_chan_sum_cl(p, p, 3, c, 5, p, None) == -3, c
    assert h.gldm_gn_swish_chan_sum_cl(p, p, 3, 1028, 5, p, None) == -3
    for c in (6, 1, 255):
        assert h.gldm_devoxelize_gn_cl_fused(p, p, p, p, p, 3, c, 10, 5, p, None) == -3, c
    assert h.gldm_devoxelize_gn_cl_fused(p, p, p, None, None, 3, 260, 10, 5, p, None) == -3
    assert int(h.gldm_squeeze_parts()) >= 1
