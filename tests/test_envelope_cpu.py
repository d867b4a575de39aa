"""The library owns the shape envelope of the encoders' three MFMA families, Python owns the routing.

Each query below is its launcher's own planner (csrc/pointwise_mlp.hip: plan_pointwise; csrc/conv3d.hip: the instantiation
lists; csrc/sa_mlp.hip: plan_sa3, plan_sa_f32), so the tables pin the planners from both sides of every bound they have.
A shape the query rejects is also handed to the entry itself with non-null dummy HOST pointers, which must answer the same
status before anything is launched.  An entry is called ONLY for a shape the query has just rejected (`_entry_agrees`): this
file also runs where a device is present, and an accepted shape would launch on those pointers."""
import ctypes

import pytest
import torch

from graspldm_amd import _lib as L

OK, INVALID, UNSUPPORTED = 0, -1, -3


def _p():
    buf = (ctypes.c_float * 16)()
    _p.keep = getattr(_p, "keep", []) + [buf]
    return ctypes.cast(buf, ctypes.c_void_p)


def _entry_agrees(status, entry):
    """`entry()` launches nothing only because the query has just said no: never call it for an accepted shape."""
    assert status < 0
    assert entry() == status


def _i32(values):
    return ctypes.cast((ctypes.c_int32 * len(values))(*values), ctypes.c_void_p)


# ---------------------------------------------------------------- pointwise

# (split, cin0, cin, cout, n, hout, addend, point-major) -> status
POINTWISE = [
    # split: n in 16-point n-tiles
    ((1, 0, 512, 256, 16, 0, 0, 0), OK), ((1, 0, 512, 256, 8, 0, 0, 0), UNSUPPORTED),
    # split: the planes of a 32-point tile + 64 bytes in the CU's LDS: K <= 1152
    ((1, 0, 1152, 256, 32, 0, 0, 0), OK), ((1, 0, 1280, 256, 32, 0, 0, 0), UNSUPPORTED),
    # split: one-m-tile units (cout % 16) below 256 rows while the planes fit half the LDS (K <= 512), else cout % 32
    ((1, 0, 512, 240, 32, 0, 0, 0), OK), ((1, 0, 640, 240, 32, 0, 0, 0), UNSUPPORTED), ((1, 0, 640, 224, 32, 0, 0, 0), OK),
    ((1, 0, 512, 264, 32, 0, 0, 0), UNSUPPORTED), ((1, 0, 512, 288, 32, 0, 0, 0), OK),
    # split without a front layer: any multiple of 8 input rows (K padded to 128), with one: whole 256-deep K, cin0 <= 96
    ((1, 0, 8, 64, 32, 0, 0, 0), OK), ((1, 0, 40, 64, 32, 0, 0, 0), OK), ((1, 0, 36, 64, 32, 0, 0, 0), UNSUPPORTED),
    ((1, 96, 768, 1536, 32, 0, 0, 0), OK), ((1, 128, 768, 1536, 32, 0, 0, 0), UNSUPPORTED),
    ((1, 48, 768, 1536, 32, 0, 0, 0), UNSUPPORTED), ((1, 32, 384, 256, 32, 0, 0, 0), UNSUPPORTED),
    ((1, 96, 768, 1280, 32, 0, 0, 0), OK), ((1, 96, 768, 1312, 32, 0, 0, 0), UNSUPPORTED),
    # a head: whole rounds of units, up to 16 rows
    ((1, 0, 768, 1536, 32, 7, 0, 0), OK), ((1, 0, 768, 1568, 32, 7, 0, 0), UNSUPPORTED), ((1, 0, 768, 1536, 32, 17, 0, 0), UNSUPPORTED),
    # the addend and the point-major output are split forms
    ((1, 0, 128, 128, 32, 0, 1, 0), OK), ((1, 0, 128, 128, 32, 0, 0, 1), OK),
    ((0, 0, 128, 256, 32, 0, 1, 0), UNSUPPORTED), ((0, 0, 128, 256, 32, 0, 0, 1), UNSUPPORTED),
    # f32: K in pairs of 16-deep blocks, 4 (32 cin + 4096) bytes in the LDS: cin <= 1152; rounds of 256 rows; 32-point tiles
    ((0, 0, 1152, 256, 32, 0, 0, 0), OK), ((0, 0, 1184, 256, 32, 0, 0, 0), UNSUPPORTED), ((0, 0, 48, 256, 32, 0, 0, 0), UNSUPPORTED),
    ((0, 0, 128, 256, 32, 0, 0, 0), OK), ((0, 0, 128, 128, 32, 0, 0, 0), UNSUPPORTED), ((0, 0, 128, 256, 16, 0, 0, 0), UNSUPPORTED),
    ((0, 96, 768, 1536, 32, 7, 0, 0), OK), ((0, 96, 384, 1536, 32, 0, 0, 0), UNSUPPORTED), ((0, 48, 768, 1536, 32, 0, 0, 0), UNSUPPORTED),
    ((0, 384, 768, 256, 32, 0, 0, 0), OK), ((0, 416, 768, 256, 32, 0, 0, 0), UNSUPPORTED),
    # sizes
    ((1, 0, 0, 256, 32, 0, 0, 0), UNSUPPORTED), ((0, 0, 128, 0, 32, 0, 0, 0), UNSUPPORTED), ((0, -32, 256, 256, 32, 0, 0, 0), UNSUPPORTED),
]


def _pointwise_entry(h, split, cin0, cin, cout, n, hout, add, pm):
    """The entry of one form on dummy pointers, or None where the form has no entry (f32 with addend / point-major)."""
    p = _p()
    head = (p, p, hout) if hout else (None, None, 0)
    z = p if hout else None
    if add or pm:
        if not split:
            return None
        if pm:
            return lambda: h.gldm_pointwise_mlp_f16x2_pm(p, p, p, 1, cin, cout, n, 1, p, None)
        return lambda: h.gldm_pointwise_mlp_f16x2_add(p, p, p, p, 0, 0, 0, 1, cin, cout, n, 1, p, None)
    if cin0:
        if split:
            return lambda: h.gldm_pointwise_mlp2_f16x2(p, p, p, cin0, p, p, 1, cin, cout, n, *head, None, p, z, None)
        return lambda: h.gldm_pointwise_mlp2(p, p, p, cin0, p, p, 1, cin, cout, n, *head, p, z, None)
    name = "gldm_pointwise_mlp_f16x2" if split else "gldm_pointwise_mlp"
    return lambda: getattr(h, name)(p, p, p, 1, cin, cout, n, 1, *head, p, z, None)


@pytest.mark.parametrize("shape,status", POINTWISE)
def test_pointwise_query_and_entries(shape, status):
    h = L.lib()
    assert h.gldm_pointwise_mlp_supported(*shape) == status
    split, cin0, cin, cout, n, hout, add, pm = shape
    entry = _pointwise_entry(h, *shape)
    # the entries call a non-positive size or more than 16 head rows an invalid argument before they plan
    if status != OK and entry is not None and min(cin, cout, n) > 0 and cin0 >= 0 and hout <= 16:
        _entry_agrees(status, entry)


def test_pointwise_policy_refuses_inside_the_envelope():
    """The routing policy of dense.py, one case per term: the library takes the shape, the predicate does not."""
    from graspldm_amd import dense, numerics
    q = L.lib().gldm_pointwise_mlp_supported
    x = lambda cin, n=32: torch.zeros(1, cin, n)
    assert dense.split_mlp_supported(x(512), 512, 128) and q(1, 0, 512, 128, 32, 0, 0, 0) == OK      # nothing refuses
    assert q(1, 0, 512, 128, 16, 0, 0, 0) == OK and not dense.split_mlp_supported(x(512, 16), 512, 128)   # SPLIT_TILE_POINTS
    assert q(1, 0, 24, 128, 32, 0, 0, 0) == OK and not dense.split_mlp_supported(x(24), 24, 128)          # SPLIT_PAD_MIN_CIN
    assert q(1, 0, 128, 48, 32, 0, 0, 0) == OK and not dense.split_mlp_supported(x(128), 128, 48)         # SPLIT_MIN_COUT
    assert q(1, 0, 896, 128, 32, 0, 0, 0) == OK and not dense.split_mlp_supported(x(896), 896, 128)       # SPLIT_MAX_K
    assert q(1, 0, 776, 256, 32, 0, 0, 0) == OK and not dense.split_supported(776) and dense.split_supported(768)
    assert q(1, 96, 1024, 256, 32, 0, 0, 0) == OK and not dense.split_supported(1024, 96) and dense.split_supported(768, 96)
    with numerics.f32_only():                                                                            # split_enabled()
        assert not dense.split_mlp_supported(x(512), 512, 128) and not dense.split_supported(768, 96)
        assert dense.fused_mlp_supported(x(768), 768, 1536) and dense.fused_mlp2_supported(x(96), 96, 768, 1536)
    # ... and never the other way round: what the library refuses, no predicate takes
    assert q(1, 32, 384, 256, 32, 0, 0, 0) == UNSUPPORTED and not dense.split_supported(384, 32)
    assert not dense.split_mlp_supported(x(640), 640, 240) and not dense.fused_mlp_supported(x(1184), 1184, 256)
    assert not dense.fused_mlp2_supported(x(96), 96, 384, 1536)
    assert not dense.fused_mlp2_supported(x(1), 0, 256, 256)   # cin0 = 0 is "no front layer" to the library: not this form
    # a tensor that is not [B, C, N] contiguous is no tile at all
    assert not dense.fused_mlp_supported(torch.zeros(1, 128, 64)[:, :, :32], 128, 256) and dense.fused_mlp_supported(None, 128, 256)


# ---------------------------------------------------------------- conv3d

F32, F16X2 = 0, 1
# (kind, cin, cout, r) -> status
CONV = [
    ((F32, 3, 48, 24), OK), ((F32, 48, 48, 24), OK), ((F32, 48, 40, 24), OK),    # 40 rows: three m-tiles, the last one guarded
    ((F32, 48, 80, 24), UNSUPPORTED), ((F32, 48, 48, 28), UNSUPPORTED), ((F32, 48, 48, 6), UNSUPPORTED),
    ((F32, 32, 64, 32), OK), ((F32, 32, 256, 8), OK), ((F32, 32, 256, 16), UNSUPPORTED),    # two launches of half the rows
    ((F16X2, 48, 48, 24), OK), ((F16X2, 3, 48, 24), OK), ((F16X2, 16, 256, 8), OK), ((F16X2, 128, 128, 4), OK),
    ((F16X2, 3, 32, 32), UNSUPPORTED), ((F16X2, 24, 48, 24), UNSUPPORTED), ((F16X2, 48, 48, 12), UNSUPPORTED),
    ((F16X2, 48, 40, 24), UNSUPPORTED), ((F16X2, 16, 16, 16), UNSUPPORTED),
    ((2, 48, 48, 24), INVALID),
    # (rows are appended: a test's id carries its row's index)  f32 at 32^3: 2, 3 (33 .. 48 rows) and 2 x 2 m-tiles
    ((F32, 5, 33, 32), OK), ((F32, 5, 48, 32), OK), ((F32, 5, 80, 32), UNSUPPORTED),
]


@pytest.mark.parametrize("shape,status", CONV)
def test_conv_query_and_entries(shape, status):
    h = L.lib()
    assert h.gldm_conv3d_k3_supported(*shape) == status
    kind, cin, cout, r = shape
    p = _p()
    if status == UNSUPPORTED and kind == F32:
        _entry_agrees(status, lambda: h.gldm_conv3d_k3(p, p, p, 1, cin, cout, r, p, p, None))
        if cout % 4 == 0:
            _entry_agrees(status, lambda: h.gldm_conv3d_k3_cl(p, p, p, 1, cin, cout, r, p, p, None))
    if status == UNSUPPORTED and kind == F16X2:
        _entry_agrees(status, lambda: h.gldm_conv3d_k3_f16x2(p, p, p, 1, cin, cout, r, p, p, None))
        _entry_agrees(status, lambda: h.gldm_conv3d_k3_f16x2_gn(p, p, p, p, 1, cin, cout, r, p, p, 1, None))


def test_conv_policy_refuses_inside_the_envelope():
    from graspldm_amd import numerics, voxel
    q = L.lib().gldm_conv3d_k3_supported
    assert voxel.conv_supported(48, 24) and voxel.split_conv_supported(48, 48, 24) and voxel.split_conv_supported(3, 48, 24)
    assert q(F32, 1, 40, 24) == OK and not voxel.conv_supported(40, 24)                                   # CONV_ROW_TILE
    with numerics.f32_only():   # split_enabled(): a shape with an f32 instantiation runs it; FIRST_VOXEL_CONV has its own f32 form
        assert q(F16X2, 48, 48, 24) == OK and not voxel.split_conv_supported(48, 48, 24)
        assert q(F16X2, 3, 48, 24) == OK and not voxel.split_conv_supported(3, 48, 24)
    assert not voxel.conv_supported(80, 24) and not voxel.split_conv_supported(24, 48, 24)


# ---------------------------------------------------------------- set abstraction

# (pre, c, u, cin_pad, cout) -> dynamic LDS of the single-tile launch (plane blocks x 8192 + 64 + 32 cout_last), or a status
SA_SPLIT = [
    ((0, 0, 64, [256, 256], [256, 1008]), 16 * 8192 + 64 + 32 * 1008), ((0, 0, 64, [256, 256], [256, 1024]), UNSUPPORTED),
    ((1, 0, 64, [256, 256], [256, 1008]), 16 * 8192 + 64 + 32 * 1008), ((1, 0, 64, [256, 256], [256, 1024]), UNSUPPORTED),
    ((0, 0, 64, [128, 256], [256, 1024]), 12 * 8192 + 64 + 32 * 1024),
    ((0, 0, 64, [288], [128]), 9 * 8192 + 64 + 32 * 128), ((0, 0, 64, [320], [128]), UNSUPPORTED),     # rows of the gather
    ((1, 0, 64, [256], [128]), 8 * 8192 + 64 + 32 * 128), ((1, 0, 64, [288], [128]), UNSUPPORTED),     # rows of `pre`
    ((0, 0, 64, [32], [16]), 8192 + 64 + 32 * 16), ((0, 0, 8, [32], [16]), UNSUPPORTED), ((0, 0, 128, [32], [16]), UNSUPPORTED),
    ((0, 0, 16, [32], [16]), 8192 + 64 + 32 * 16), ((0, 0, 48, [32], [16]), UNSUPPORTED),
    ((0, 0, 64, [256], [64]), 8 * 8192 + 64 + 32 * 64), ((0, 0, 64, [224], [64]), UNSUPPORTED),        # K blocks: <= 6, 8 or 9
    ((0, 0, 64, [192], [64]), 6 * 8192 + 64 + 32 * 64), ((0, 0, 64, [48], [64]), UNSUPPORTED),
    ((0, 0, 64, [32, 128], [128, 24]), UNSUPPORTED), ((0, 0, 64, [32, 128], [128, 48]), 5 * 8192 + 64 + 32 * 48),
    ((0, 0, 64, [32, 96], [96, 64]), UNSUPPORTED), ((0, 0, 64, [32, 512], [512, 64]), UNSUPPORTED),    # hidden: 32 / 64 / 128 / 256
    ((0, 29, 64, [32], [64]), 8192 + 64 + 32 * 64), ((0, 30, 64, [32], [64]), UNSUPPORTED),            # 3 + c rows gathered
    ((0, 0, 64, [32, 32, 32, 32], [32, 32, 32, 32]), 2 * 8192 + 64 + 32 * 32), ((0, 0, 64, [32] * 5, [32] * 5), UNSUPPORTED),
    ((0, 0, 64, [32, 64], [32, 64]), INVALID), ((1, 3, 64, [32], [64]), INVALID), ((0, 0, 0, [32], [64]), INVALID),
    # the two plans split_plan_ok's policy refuses: 13 plane blocks + a 256-row output
    ((0, 0, 16, [288, 128], [128, 256]), 13 * 8192 + 64 + 32 * 256), ((0, 0, 32, [288, 128, 128], [128, 128, 256]), 114752),
]


@pytest.mark.parametrize("plan,answer", SA_SPLIT)
def test_sa_split_query_and_entries(plan, answer):
    h = L.lib()
    pre, c, u, cin_pad, cout = plan
    n = len(cout)
    planes = ctypes.c_longlong(-7)
    got = h.gldm_sa_mlp_f16x2_lds_bytes(pre, c, u, n, _i32(cin_pad), _i32(cout), ctypes.byref(planes))
    assert got == answer
    assert h.gldm_sa_mlp_f16x2_lds_bytes(pre, c, u, n, _i32(cin_pad), _i32(cout), None) == answer
    if answer >= 0:
        assert planes.value == answer - 64 - 32 * cout[-1] and planes.value % 8192 == 0
        return
    assert planes.value == -7   # untouched
    p, off = _p(), _i32([0] * n)
    gain = ctypes.cast((ctypes.c_float * (2 * n))(*[1.0] * (2 * n)), ctypes.c_void_p)
    if u > 0 and not (pre and c):   # the entries call those two an invalid argument themselves; _pre has no c to pass
        if pre:
            _entry_agrees(answer, lambda: h.gldm_sa_mlp_forward_f16x2_pre(p, p, p, 0, p, p, 0, 1, 64, 8, u, n, _i32(cin_pad), _i32(cout),
                                                                         off, off, gain, p, None))
        else:
            _entry_agrees(answer, lambda: h.gldm_sa_mlp_forward_f16x2(p, p, p, p, p, 1, c, 64, 8, u, n, _i32(cin_pad), _i32(cout),
                                                                     off, off, gain, p, None))


# (c, u, cin_pad, cout) -> status of gldm_sa_mlp_forward
SA_F32 = [
    ((0, 64, [32], [16]), OK), ((0, 8, [32], [16]), OK), ((0, 1, [32], [16]), OK), ((0, 48, [32], [16]), UNSUPPORTED),
    ((0, 128, [32], [16]), UNSUPPORTED),
    ((253, 64, [256], [256]), OK), ((253, 64, [288], [256]), UNSUPPORTED), ((253, 64, [256], [272]), UNSUPPORTED),
    ((0, 64, [32, 192], [192, 64]), OK), ((0, 64, [32, 96], [96, 64]), UNSUPPORTED), ((0, 64, [32, 48], [48, 64]), UNSUPPORTED),
    ((0, 64, [32], [120]), UNSUPPORTED), ((0, 64, [40], [64]), UNSUPPORTED), ((0, 64, [48], [64]), OK),
    ((0, 64, [32] * 4, [32] * 4), OK), ((0, 64, [32] * 5, [32] * 5), UNSUPPORTED),
    ((0, 64, [32, 64], [32, 64]), INVALID), ((30, 64, [32], [64]), INVALID), ((29, 64, [32], [64]), OK), ((0, 0, [32], [64]), INVALID),
]


@pytest.mark.parametrize("plan,status", SA_F32)
def test_sa_f32_query_and_entry(plan, status):
    h = L.lib()
    c, u, cin_pad, cout = plan
    n = len(cout)
    assert h.gldm_sa_mlp_supported(c, u, n, _i32(cin_pad), _i32(cout)) == status
    if status != OK:
        p, off = _p(), _i32([0] * n)
        _entry_agrees(status, lambda: h.gldm_sa_mlp_forward(p, p, p, p, p, 1, c, 64, 8, u, n, _i32(cin_pad), _i32(cout), off, off, p, None))


def test_sa_policy_refuses_inside_the_envelope():
    """split_plan_ok keeps the planning figure of the three-plane days (12288 bytes per plane block where launch_sa3 holds
    8192) and msg_route keeps pooled rows to 256: both refuse plans the launcher takes; neither takes one it refuses."""
    from graspldm_amd import numerics, sa_pack
    from graspldm_amd.pvcnn import SharedMLP
    assert sa_pack.sa3_takes(288, [128, 256], 16) and not sa_pack.split_plan_ok([259], [128, 256], 16)           # PLANNED_PLANES
    assert sa_pack.sa3_takes(288, [128, 128, 256], 32) and not sa_pack.split_plan_ok([259], [128, 128, 256], 32)
    assert sa_pack.split_plan_ok([131], [128, 128, 256], 64) and sa_pack.split_plan_ok([19], [16, 32], 32)      # 16 runs as 32
    assert sa_pack.sa3_takes(256, [256, 1008], 64, pre=True) and sa_pack.msg_route(6, (256, 256, 1008), 64) is None   # MSG_MAX_POOLED_ROWS
    assert sa_pack.sa3_takes(32, [32] * 4, 64, pre=True) and sa_pack.msg_route(6, (32,) * 5, 64) is None             # MSG_MAX_LAYERS
    with numerics.f32_only():                                                                                   # split_enabled()
        assert sa_pack.sa3_takes(160, [128, 128, 256], 64) and not sa_pack.split_plan_ok([131], [128, 128, 256], 64)
        assert sa_pack.msg_route(6, (64, 96, 128), 64) == "f32" and sa_pack.msg_route(323, (128, 196, 256), 64) == "f32_pre"
    assert sa_pack.msg_route(6, (64, 96, 128), 64) == "pre" and sa_pack.msg_route(323, (128, 196, 256), 64, hoist=False) == "pre"
    assert not sa_pack.sa3_takes(320, [128], 64) and not sa_pack.split_plan_ok([300], [128], 64)
    assert sa_pack.fusable(SharedMLP(131, [128, 128, 256], dim=2), 64) and not sa_pack.fusable(SharedMLP(131, [128, 96, 256], dim=2), 64)
    assert not sa_pack.fusable(SharedMLP(259, [128, 256], dim=2), 64) and not sa_pack.fusable(SharedMLP(6, [64], dim=2), 48)


def test_queries_are_exported_and_need_no_device():
    """Fails without the feature (the symbol lookup); the planners are pure host functions: this file runs without a GPU."""
    assert L.ABI_VERSION == 15 and L.lib().gldm_abi_version() == 15
    for name in ("gldm_pointwise_mlp_supported", "gldm_conv3d_k3_supported", "gldm_sa_mlp_supported", "gldm_sa_mlp_f16x2_lds_bytes"):
        assert name in L._SIGNATURES
    assert L.lib().gldm_sa_mlp_f16x2_lds_bytes.restype is ctypes.c_longlong
    assert L.lib().gldm_sa_mlp_supported(0, 64, 1, None, _i32([16])) == INVALID
    assert L.lib().gldm_sa_mlp_f16x2_lds_bytes(0, 0, 64, 1, _i32([32]), None, None) == INVALID
