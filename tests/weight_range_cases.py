"""Shared by tests/test_weight_range_cpu.py and tests/test_weight_range_gpu.py: the split-f16 GEMM restated in torch, the
weight-magnitude patterns, and the table of which GPU test runs which family of split-f16 packers.

Patterns (weight side).  W is a Kaiming-sized [M, K] matrix, x its unit-normal input:
  whole(k)  W 2^-k: every weight k binades further into the range where the lo piece is an f16 subnormal;
  rows      the second half of the ROWS at 2^-12 (what a BatchNorm fold with a large running_var produces): measured per
            row group against that group's own magnitude, since the next normalisation re-amplifies the quiet rows;
  cols      matched COLUMNS: W[:, j] 2^-12 with x[j] 2^12 for the second half of the columns (input channels in other
            units): the product is the one of the unscaled pair, the split weight's absolute error is 4096 times larger.
"""
import torch

BAR = 2e-5          # the single-forward parity bar of every family's existing tests
QUIET = 12          # binades of the rows / cols patterns
PAIRS = [(0, 1), (1, 0), (0, 0)]   # (weight plane, activation plane), small terms first as the kernels issue them


def split2(x):
    hi = x.to(torch.float16).float()      # f16 subnormals kept: the matrix pipe keeps them
    lo = (x - hi).to(torch.float16).float()
    return hi, lo


def restated_gemm(w, x):
    """W [M, K] x [K, N] as the split kernels multiply: hi / lo f16 pieces of both, three products, f32 accumulation."""
    ws, xs = split2(w.float()), split2(x.float())
    return sum(ws[i] @ xs[j] for i, j in PAIRS)


def rel(got, ref):
    """max |got - ref| / max |ref|: the error relative to the output's magnitude (tests/test_range_gpu.py: _rel)."""
    ref = ref.detach().double().cpu()
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def kaiming(m, k, seed):
    return torch.randn(m, k, generator=torch.Generator().manual_seed(seed)) / k ** 0.5


def row_scale(m, pattern):
    """[M] factors on the rows of W (and on its bias) for `pattern` = ("whole", k) | "rows" | "cols"."""
    s = torch.ones(m)
    if isinstance(pattern, tuple):
        s *= 2.0 ** -pattern[1]
    elif pattern == "rows":
        s[m // 2:] = 2.0 ** -QUIET
    return s


def col_scale(k, pattern):
    """[K] factors on the columns of W; the matched input rows take the reciprocal."""
    s = torch.ones(k)
    if pattern == "cols":
        s[k // 2:] = 2.0 ** -QUIET
    return s


def apply(w, pattern):
    return w * row_scale(w.shape[0], pattern)[:, None] * col_scale(w.shape[1], pattern)[None, :]


def row_groups(m, pattern):
    """The row slices an error is measured over, each against its own magnitude."""
    return [slice(0, m // 2), slice(m // 2, m)] if pattern == "rows" else [slice(0, m)]


def k_inside(fits, k_max=24):
    """The largest k in 0 .. k_max with fits(k) and fits(j) for every j below it: the inside edge of the rule for one shape."""
    k = -1
    while k < k_max and fits(k + 1):
        k += 1
    assert 0 <= k < k_max, k
    return k


# Package module that packs split-f16 weight fragments -> the GPU tests (tests/test_weight_range_gpu.py) that run its
# kernels over the patterns.  tests/test_weight_range_cpu.py::test_every_split_packer_has_a_gpu_row greps the package.
GPU_TABLE = {
    "r1d_pack.py": ["test_r1d_engines", "test_pointwise_one_layer"],       # the fragment packer itself; pack_resnet1d
    "dense.py": ["test_pointwise_one_layer", "test_pointwise_two_layers"],
    "sa_pack.py": ["test_sa_module", "test_msg_module"],
    "voxel.py": ["test_conv3d"],
    "grasp_classifier.py": ["test_cls_head"],
    "attention.py": ["test_attention_projections"],
    "unet1d_pack.py": ["test_unet1d"],
}
