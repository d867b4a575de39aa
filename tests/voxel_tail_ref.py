"""TEST INFRASTRUCTURE: what runs behind the voxel convs of PVConv (csrc/voxel_norm.hip: the SE squeeze, the SE gate, the
fused devoxelize entries) restated in torch, f64, from the modules' arithmetic (pvconv.py:76-84, se.py:12-25,
devoxelize.py) -- no kernel code.  Every function takes f32 (or f64) tensors, converts them to f64 and returns f64.
Channel-major throughout: a test that feeds a channel-last kernel permutes its own input.  Pinned to the oracle by
tests/test_voxel_tail_cpu.py before any kernel is judged by it (tests/test_voxel_tail_gpu.py)."""
import itertools

import torch


def swish_affine(y, coef):
    """y [b, c, ...] raw, coef [b, c, 2] = (a, s) per (cloud, channel): t = a y + s, t sigmoid(t)."""
    y, coef = y.double(), coef.double()
    shape = tuple(coef.shape[:2]) + (1,) * (y.ndim - 2)
    t = coef[..., 0].reshape(shape) * y + coef[..., 1].reshape(shape)
    return t * torch.sigmoid(t)


def squeeze(y, coef):
    """The SE squeeze as SUMS over the voxels: [b, c]."""
    return swish_affine(y, coef).flatten(2).sum(-1)


def se_gate(chan_sum, w1, w2, r, use_relu):
    """sigmoid(W2 act(W1 (chan_sum / r^3))), act = ReLU or Swish; chan_sum [b, c] sums over the r^3 voxels, or
    [b, parts, c] partial sums (added here); w1 [hidden, c], w2 [c, hidden]."""
    s = chan_sum.double()
    if s.ndim == 3:
        s = s.sum(1)
    h = (s / float(r) ** 3) @ w1.double().T
    h = torch.relu(h) if use_relu else h * torch.sigmoid(h)
    return torch.sigmoid(h @ w2.double().T)


def devoxelize(coords, grid, gate, add, r):
    """Trilinear interpolation of grid [b, c, r, r, r] (flat voxel index x r^2 + y r + z) at coords [b, 3, n] in
    [0, r - 1], times gate [b, c] (None: 1) plus add [b, c, n] (None: 0): [b, c, n].  Per axis the upper corner is lo + 1
    where the fractional part is positive and lo itself where it is zero (its weight is zero there, and lo + 1 may lie
    outside the grid)."""
    co = coords.double()
    b, _, n = co.shape
    c = grid.shape[1]
    flat = grid.double().reshape(b, c, r ** 3)
    lo = torch.floor(co)
    frac = co - lo
    lo = lo.long()
    hi = lo + (frac > 0).long()
    out = torch.zeros(b, c, n, dtype=torch.float64)
    for up in itertools.product((False, True), repeat=3):
        sel = torch.tensor(up).view(1, 3, 1)
        idx = torch.where(sel, hi, lo)
        w = torch.where(sel, frac, 1.0 - frac).prod(1)                     # [b, n]
        vox = (idx[:, 0] * r + idx[:, 1]) * r + idx[:, 2]                  # [b, n]
        out += w.unsqueeze(1) * flat.gather(2, vox.unsqueeze(1).expand(b, c, n))
    if gate is not None:
        out = out * gate.double().unsqueeze(-1)
    if add is not None:
        out = out + add.double()
    return out
