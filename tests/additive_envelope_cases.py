"""The shape envelope of the kernel families added behind the encoders and the 1-D engines -- the classifier head, the two
attention cores, the small dense kernels, the point-feature norms and grasp selection -- as tables of accepted corners
(what include/gldm.h documents and the Python predicates pass on, beyond the shapes the shipped models route) and of rows on
both sides of every documented bound.  Shared by tests/test_additive_envelope_cpu.py (no device: the bounds through the
host-only queries and the predicates, the completeness of the tables) and tests/test_additive_envelope_gpu.py (every accepted
row launched through the C ABI against an f64 restatement).

The generators and f64 formulas are those of the families' own tests, imported: make_head / head_ref
(test_classifier_gpu.py), make_qkv / attention_ref (test_attention_gpu.py), make_case (test_voxel_attention_gpu.py),
_inputs / _segments (test_grasp_select_gpu.py)."""
import re
from pathlib import Path

import torch

import test_classifier_gpu as head_tests
from test_attention_gpu import attention_ref, make_qkv
from test_voxel_attention_gpu import KEY_TILE, make_case

CSRC = Path(__file__).resolve().parents[1] / "graspldm_amd" / "csrc"

# ------------------------------------------------------------------------------------------------------ A. gldm_cls_head
# (b, c, rows, n): what each row reaches is in the comment behind it (csrc/grasp_classifier.hip: 128 rows per pass, a wave
# owns two 16-row m-tiles of a pass, 64 points per tile, K in blocks of 32)
HEAD_CASES = [(2, 64, 16, 70),        # one m-tile: waves 1 to 3 fully masked; the last tile has 6 points
              (2, 48, 48, 65),        # c % 32 == 16 at two K blocks; wave 1 one live and one masked m-tile; a 1-point tile
              (1, 64, 144, 64),       # two passes, the second a single m-tile
              (1, 32, 256, 130),      # two full passes, three tiles
              (3, 2032, 496, 33),     # just inside both maxima, a multiple of neither 32 nor 128
              (1, 2048, 512, 64)]     # both maxima: four passes, 64 K blocks
HEAD_KINDS = ("normal", "negative", "last3", "scale1000", "scale0.001", "scale100000", "scale0.00001", "last_rows", "first_rows")
HEAD_BATCH_CASE = (3, 2032, 496, 33)  # a scene's bits against the same scene launched alone
HEAD_MODULE_ROWS = 256                # classifier.0 of the module-level case


def make_head(b, c, rows, n, kind="normal", seed=0):
    """test_classifier_gpu.make_head at `rows` rows (it draws test_classifier_gpu.ROWS of them) plus the two kinds that make
    the pass loop decide the result: w2 zero except on the last / the first 16 rows."""
    base = {"last_rows": "normal", "first_rows": "normal"}.get(kind, kind)
    saved = head_tests.ROWS
    head_tests.ROWS = rows
    try:
        x, w1, b1, w2, l, lb, b2 = head_tests.make_head(b, c, n, kind=base, seed=seed)
    finally:
        head_tests.ROWS = saved
    if kind == "last_rows":
        w2[:rows - 16] = 0.0
    elif kind == "first_rows":
        w2[16:] = 0.0
    return x, w1, b1, w2, l, lb, b2


def first_rows_head(args):
    """The rows = 16 head built from rows 0 to 15 of a `first_rows` case: the same logit, whatever the later passes do."""
    x, w1, b1, w2, l, lb, b2 = args
    return x, w1[:16].contiguous(), b1[:16].contiguous(), w2[:16].contiguous(), l, lb, b2


# ----------------------------------------------------------------------------- B. gldm_point_attention_fused, C. the core
FUSED_CASES = [(2, 80, 32), (1, 96, 160), (2, 112, 96), (1, 128, 4096), (3, 32, 32), (1, 48, 32)]
FUSED_KINDS = ("normal", "last_tile_max", "dominant", "zero_q", "negative", "alias", "ascending", "unit")
FUSED_RANGE_CASE = (1, 112, 96)
RANGE_SCALES = [("v", 1e5), ("v", 1e-6), ("qk", 1e2), ("qk", 1e-3)]
# (shape, arithmetic forms, kinds): exact_f32 = 0 is the default (split-f16) arithmetic
CORE_CASES = [((2, 1024, 32), (0, 1), ("normal", "unit", "dominant", "alias")),
              ((1, 1008, 64), (0, 1), ("normal", "unit", "dominant", "alias")),
              ((1, 1024, 64), (0, 1), ("normal", "unit", "dominant", "alias")),
              ((1, 1024, 4096), (0,), ("normal", "unit"))]
CORE_CHUNK_CASE = (3, 16, 3328)       # one cloud's workspace block is 89,671,936 bytes: 256 MiB hold two -> chunks of 2 and 1


def dominant_keys(b, n):
    """The key that dominates cloud i of a `dominant` case (make_qkv's choice), one per cloud, distinct within a cycle."""
    keys = (n - 3, 17 % n, n // 2)
    assert len(set(keys)) == 3, (n, keys)
    return [keys[i % 3] for i in range(b)]


def make_attention(kind, b, c, n, seed=0):
    """(q, k, v) of a case: make_case's kinds plus `unit`, q and k drawn as randn c^(-1/4) so that logits have unit
    variance (the 2e-5 term of the bar decides, not the f32 slack of 32-sigma logits)."""
    if kind != "unit":
        return make_case(kind, b, c, n, seed)
    q, k, v = make_qkv("normal", b, c, n, seed)
    s = float(c) ** -0.25
    return q * s, k * s, v


_REFS = {}


def attention_reference(kind, shape, seed=0):
    """(q, k, v, f64 reference, e32) of a case, computed once and shared by the tests that need it; the properties the kind
    promises are asserted in f64 on the way (they are properties of the inputs)."""
    key = (kind, shape, seed)
    if key not in _REFS:
        b, c, n = shape
        q, k, v = make_attention(kind, b, c, n, seed)
        ref = attention_ref(q.double(), k.double(), v.double())
        e32 = (attention_ref(q, k, v).double() - ref).abs().max().item()
        if kind in ("last_tile_max", "ascending", "negative", "dominant"):
            logits = q.double().transpose(1, 2) @ k.double()
            if kind == "last_tile_max":
                assert (logits.argmax(dim=-1) >= n - 5).all()
            elif kind == "ascending" and n > KEY_TILE:
                tile_max = logits.reshape(b, n, n // KEY_TILE, KEY_TILE).max(dim=-1).values
                assert (tile_max[..., 1:] > tile_max[..., :-1]).all()
            elif kind == "negative":
                assert logits.max() < -1e3
            elif kind == "dominant":
                top = logits.topk(2, dim=-1)
                assert ((top.values[..., 0] - top.values[..., 1]) > 1e3).all()
                for i, j in enumerate(dominant_keys(b, n)):
                    assert (top.indices[i, :, 0] == j).all()
        _REFS[key] = (q, k, v, ref, e32)
    return _REFS[key]


def attention_tolerance(ref, e32, relative=False):
    """max(2e-5 max(1, max|out|), 4 e32): the rule of tests/test_attention_gpu.py."""
    scale = ref.abs().max().item()
    return max(2e-5 * (scale if relative else max(1.0, scale)), 4 * e32)


# ------------------------------------------------------------------------------------- D. small dense kernels and norms
ROWS_CASES = [(2, 40, h, 36) for h in range(1, 9)] + [(1, 768, 2, 4), (1, 768, 7, 4)]          # (b, cin, hout, n)
SMALL_COUTS, SMALL_NS, SMALL_B = (5, 16, 19), (1, 257), 3


def small_cins():
    """Every cin gldm_pointwise_small dispatches on, read from its source."""
    text = (CSRC / "pointwise_small.hip").read_text()
    return sorted(int(m) for m in re.findall(r"GLDM_PS_CASE\((\d+)\)", text))


SMALL_CINS = [3, 6, 16, 24, 32, 48, 64]
LINEAR_CASES = [(3, 16384, 40), (2, 4, 300), (1, 16380, 257)]                                   # (rows, n, nout)
AFFINE_CASES = [(2, 3, 2), (1, 2, 24), (1, 2, 26), (1, 1, 64)]                                   # (b, c, r): 24 | 26 = gx 1 | 4
SWISH_CASES = [(2, 8, 4, 8), (1, 6, 8, 2), (2, 128, 4, 1), (1, 16, 260, 16)]                     # (b, c, n, groups)

# ------------------------------------------------------------------------------------------------------------ E. selection
CLEARANCE_SHAPE = (2, 3, 300)          # (b, g, ns)
CLEARANCE_SEGMENTS = [(8, 8), (8, 0)]  # (sb, ss)
CLEARANCE_SEED = 0
# (b, g, k, seed): the first seeds whose f64 margins are >= 1e-4 at every pick (300 picks of 300 leave few: 152 is the first)
SELECT_ENVELOPE_CASES = [(1, 300, 300, 152), (2, 2048, 9, 0)]
SELECT_CONTROL_POINTS = 64


def segments(sb, ss):
    """test_grasp_select_gpu._segments extended to eight per family: the gripper's own segments, then copies of them moved
    off the gripper's plane (y is zero on every original) and shortened, each distinct and finite."""
    from graspldm_amd import gripper

    def extend(base, dy, shrink):
        out = [tuple(map(tuple, s)) for s in base]
        i = 0
        while len(out) < 8:
            a, b = base[i % len(base)]
            lap = i // len(base) + 1
            a2 = (a[0] + shrink * lap * (b[0] - a[0]), a[1] + dy * lap, a[2] + shrink * lap * (b[2] - a[2]))
            b2 = (b[0], b[1] - dy * lap, b[2])
            out.append((a2, b2))
            i += 1
        assert len({s for s in out}) == 8
        return out
    return extend(gripper.OPEN_SEGMENTS, 0.012, 0.1)[:sb], extend(gripper.SWEEP_SEGMENTS, 0.009, 0.05)[:ss]


def clearance_inputs(seed=CLEARANCE_SEED):
    """(scene, normals, H): test_grasp_select_gpu._inputs' scene and poses, random unit normals with every tenth zero."""
    import test_grasp_select_gpu as base
    b, g, ns = CLEARANCE_SHAPE
    scene, H = base._inputs(b, g, ns, seed)
    gen = torch.Generator().manual_seed(500 + seed + ns)
    normals = torch.randn(b, ns, 3, generator=gen)
    normals = normals / normals.norm(dim=-1, keepdim=True)
    normals[:, ::10] = 0.0
    return scene, normals, H


# ------------------------------------------------------------------------------------------------------- bounds (host side)
# Rows on both sides of every documented bound: (value, accepted)
ATTN_C_ROWS = [(0, False), (8, False), (16, True), (24, False), (1024, True), (1040, False)]
ATTN_N_ROWS = [(0, False), (16, False), (32, True), (48, False), (4096, True), (4128, False)]
HEAD_ROWS_ROWS = [(0, False), (8, False), (16, True), (24, False), (512, True), (528, False)]
HEAD_C_ROWS = ATTN_C_ROWS[:4] + [(1024, True), (1040, True), (2048, True), (2064, False)]
HEAD_N_ROWS = [(0, False), (1, True), (1 << 20, True), ((1 << 20) + 1, False)]
FUSED_C_ROWS = [(16, False), (32, True), (128, True), (144, False)]
KNN_N_ROWS = [(0, False), (1, True), (1 << 20, True), ((1 << 20) + 1, False)]
