"""CPU: the C-ABI library loads and exports every symbol include/gldm.h declares
(no compute calls without a GPU), and the oracle's C library builds."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "gldm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gldm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    names = _declared()
    assert "gldm_ball_query" in names and "gldm_sa_group" in names and len(names) >= 11


def test_library_exports_every_declared_symbol():
    from graspldm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(h, n)]
    assert not missing, f"declared in gldm.h but not exported: {missing}"
    lib = _lib.lib()
    assert lib.gldm_abi_version() == _lib.ABI_VERSION
    assert lib.gldm_status_string(0) == b"ok"


def test_python_binding_covers_every_declared_symbol():
    """Every name the loose pattern finds in the header is bound on the loaded library, argument and return types both, with
    what graspldm_amd/_abi.py derived from its prototype (nothing is bound by hand, nothing falls back to ctypes' defaults)."""
    from graspldm_amd import _abi, _lib
    h = _lib.lib()
    assert set(_declared()) == set(_abi.PROTOTYPES) == set(_lib._SIGNATURES)
    for name in _declared():
        restype, argtypes = _abi.PROTOTYPES[name]
        fn = getattr(h, name)
        assert fn.restype is restype and restype is not None, name
        assert list(fn.argtypes) == argtypes == _lib._SIGNATURES[name], name


_i, _f, _ll, _ull, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p
# literal signatures of entries that between them use every mapping of the parser
PINNED = {
    "gldm_abi_version": (_i, []),
    "gldm_status_string": (ctypes.c_char_p, [_i]),
    "gldm_denoise_rng": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _ull, _ll, _vp, _vp, _vp, _vp]),
    "gldm_normalize_cloud": (_i, [_vp, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp]),
    "gldm_sa_mlp_f16x2_lds_bytes": (_ll, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "gldm_conv3d_partial_floats": (_ll, [_i, _i, _i]),
    "gldm_r1d_workspace_bytes": (_ll, [_vp, _i]),
    "gldm_unet1d": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gldm_ball_query_multi": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gldm_segment_tile_shape": (_i, [_vp, _vp]),
    "gldm_bias_act": (_i, [_vp, _vp, _i, _i, _ll, _i, _vp]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_signature_matches_the_pinned_literal(name):
    from graspldm_amd import _abi
    assert _abi.PROTOTYPES[name] == PINNED[name]


def _layout_lines(abi):
    """What the C program of the next test prints, from the ctypes classes and the constants dict."""
    lines = []
    for sname, cls in abi.STRUCTS.items():
        lines.append(f"{sname} {ctypes.sizeof(cls)}")
        for fname, _ in cls._fields_:
            f = getattr(cls, fname)
            lines.append(f"{sname}.{fname} {f.offset} {f.size}")
    return lines + [f"{k} {v}" for k, v in abi.CONSTANTS.items()]


def test_struct_layouts_and_constants_match_the_c_compiler(tmp_path):
    """The check that does not go through the parser: a C program including gldm.h prints sizeof of every struct, offsetof
    and size of every field and the value of every constant; the host compiler's answers equal the derived ones line by line."""
    import subprocess
    from graspldm_amd import _abi
    assert list(_abi.STRUCTS) == ["gldm_r1d_resblock", "gldm_r1d_level", "gldm_r1d_desc", "gldm_unet1d_desc"]
    assert [ctypes.sizeof(c) for c in _abi.STRUCTS.values()] == [56, 64, 1208, 104]
    assert len(_abi.CONSTANTS) >= 27 and _abi.CONSTANTS["GLDM_ABI_VERSION"] == 15
    body = []
    for sname, cls in _abi.STRUCTS.items():
        body.append(f'printf("{sname} %zu\\n", sizeof({sname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf("{sname}.{fname} %zu %zu\\n", offsetof({sname}, {fname}), sizeof((({sname} *)0)->{fname}));')
    body += [f'printf("{k} %lld\\n", (long long)({k}));' for k in _abi.CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gldm.h"\nint main(void) {\n  '
                   + "\n  ".join(body) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    want = _layout_lines(_abi)
    assert out == want, [(a, b) for a, b in zip(out, want) if a != b][:10]


GOOD = """
/* int gldm_in_a_comment(float (*f)(int)); */
#define GLDM_N 3
#define GLDM_M (2 * GLDM_N + 1)   /* 7 */
enum gldm_kind { GLDM_A, GLDM_B = GLDM_M - 2, GLDM_C };
typedef void *gldm_stream_t;
typedef struct gldm_in { int32_t a, b[2]; } gldm_in;
typedef struct gldm_out {
  int32_t n;
  gldm_in one, many[GLDM_M];
} gldm_out;
int gldm_f(const gldm_out *d, const float *x /*[n]*/, int32_t *const *rows, int n, float eps, long long big,
           unsigned long long seed, gldm_stream_t stream);
long long gldm_g(void);
const char *gldm_h(int status);
"""


def test_parser_on_synthetic_text():
    from graspldm_amd import _abi
    protos, structs, consts = _abi.parse(GOOD)
    assert consts == {"GLDM_N": 3, "GLDM_M": 7, "GLDM_A": 0, "GLDM_B": 5, "GLDM_C": 6}
    assert protos == {"gldm_f": (_i, [_vp, _vp, _vp, _i, _f, _ll, _ull, _vp]), "gldm_g": (_ll, []),
                      "gldm_h": (ctypes.c_char_p, [_i])}
    assert list(structs) == ["gldm_in", "gldm_out"] and ctypes.sizeof(structs["gldm_in"]) == 12
    out = structs["gldm_out"]
    assert ctypes.sizeof(out) == 4 + 12 + 7 * 12 and out.many.offset == 16 and out.one.size == 12
    d = out()
    d.many[6].b[1] = 9
    assert bytes(d)[-4:] == (9).to_bytes(4, "little")


@pytest.mark.parametrize("bad", [
    "int gldm_x(size_t n);",                                        # unknown type word
    "int gldm_x(const half *p);",                                   # unknown pointee
    "void gldm_x(int n);",                                          # unknown return type
    "int gldm_x(int (*callback)(int), int n);",                     # function-pointer parameter
    "typedef struct gldm_s { int32_t a; float b; } gldm_s;",        # float field
    "typedef struct gldm_s { int32_t *a; } gldm_s;",                # pointer field
    "typedef struct gldm_s { int32_t a[GLDM_UNDEFINED]; } gldm_s;",  # array size that is no known constant
    "typedef struct gldm_s { int32_t a; } gldm_s;\nint gldm_x(gldm_s by_value, int n);",   # struct by value
    "int gldm_x(int n) __attribute__((deprecated));",               # a declared gldm_x( the prototype pattern misses
    "int gldm_ok(int n);\nint gldm_x(int n, ...)\n;int gldm_y(int (*f)(void));",
    "#define GLDM_EPS 1e-5f",                                       # a constant that is no integer
])
def test_parser_raises_on_what_it_does_not_understand(bad):
    from graspldm_amd import _abi
    with pytest.raises(_abi.GldmError):
        _abi.parse("typedef void *gldm_stream_t;\n" + bad + "\n")


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    from graspldm_amd import _abi
    monkeypatch.setattr(_abi, "HEADER", str(tmp_path / "gldm.h"))
    with pytest.raises(_abi.GldmError, match="missing"):
        _abi._load()


def test_invalid_arguments_return_status_not_exit():
    from graspldm_amd import _lib
    h = _lib.lib()
    # null pointers / non-positive sizes are rejected before any HIP call
    assert h.gldm_ball_query(None, None, 1, 1, 1, 0.1, 1, None, None) == -1
    assert h.gldm_grouping_forward(None, None, 0, 0, 0, 0, 0, None, None) == -1
    with pytest.raises(_lib.GldmError):
        _lib.call("gldm_furthest_point_sampling", None, 1, 16, 4, None, None)


def test_backend_has_the_twelve_reference_names():
    from graspldm_amd.backend import _backend
    names = ["gather_features_forward", "gather_features_backward", "furthest_point_sampling", "ball_query",
             "grouping_forward", "grouping_backward", "three_nearest_neighbors_interpolate_forward",
             "three_nearest_neighbors_interpolate_backward", "trilinear_devoxelize_forward",
             "trilinear_devoxelize_backward", "avg_voxelize_forward", "avg_voxelize_backward"]
    for n in names:
        assert callable(getattr(_backend, n)), n
    with pytest.raises(NotImplementedError):
        _backend.grouping_backward(None, None, 0)


def test_backend_rejects_cpu_tensors_like_the_reference():
    import torch
    from graspldm_amd.backend import _backend
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        _backend.ball_query(torch.zeros(1, 3, 4), torch.zeros(1, 3, 8), 0.1, 2)


def test_dpp_hazard_scan_flags_a_close_write(tmp_path):
    """tools/isa/dpp_hazard_scan.py (part of tools/isa/lint.sh): a VALU write one wait state in front of a DPP read of the
    same register is reported, the same pair behind an `s_nop 1` is not."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = tmp_path / "bad.s"
    bad.write_text("0000000000001000 <my_kernel>:\n"
                   "\tv_add_f32_e32 v5, v1, v2                                 // 000000001000: 020A0501\n"
                   "\tv_max_f32_dpp v6, v5, v5 row_ror:4 row_mask:0xf bank_mask:0xf // 000000001004: 160C0AFA\n"
                   "\ts_endpgm\n")
    good = tmp_path / "good.s"
    good.write_text("0000000000001000 <my_kernel>:\n"
                    "\tv_add_f32_e32 v5, v1, v2\n\ts_nop 1\n"
                    "\tv_max_f32_dpp v6, v5, v5 row_ror:4 row_mask:0xf bank_mask:0xf\n"
                    "\tv_mov_b32_e32 v9, v1\n\tv_mov_b32_e32 v10, v1\n\tv_mov_b32_e32 v11, v1\n"
                    "\tv_mov_b32_dpp v7, v9 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_endpgm\n")
    scan = os.path.join(root, "tools", "isa", "dpp_hazard_scan.py")
    r = subprocess.run([sys.executable, scan, str(bad), "my_kernel"], capture_output=True, text=True)
    assert r.returncode == 1 and "1 VALU-write" in r.stdout, r.stdout
    r = subprocess.run([sys.executable, scan, str(good), "my_kernel"], capture_output=True, text=True)
    assert r.returncode == 0 and "2 DPP instructions, 0 VALU-write" in r.stdout, r.stdout


def test_hazard_scan_flags_a_read_of_a_fresh_matrix_result(tmp_path):
    """Second check of tools/isa/dpp_hazard_scan.py (round 6): a VALU instruction that reads a matrix instruction's result
    closer than the compiler ever leaves them -- only an asm statement taking accumulators straight out of the matrix pipe can
    do that (csrc/quad_narrow.h: pos_max8 did, 3 wait states behind a v_mfma_f32_16x16x4_f32) -- is reported; the same read
    behind enough other instructions, or of a register overwritten in between, is not."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scan = os.path.join(root, "tools", "isa", "dpp_hazard_scan.py")
    mfma = "\tv_mfma_f32_16x16x4_f32 v[60:63], v5, v69, 0\n"
    filler = "\tv_mov_b32_e32 v9, v1\n"
    read = "\tv_max_f32_dpp v3, v60, v60 row_ror:4 row_mask:0xf bank_mask:0xf\n"
    head, tail = "0000000000001000 <my_kernel>:\n", "\ts_endpgm\n"
    bad = tmp_path / "bad.s"
    bad.write_text(head + mfma + 3 * filler + read + tail)
    far = tmp_path / "far.s"
    far.write_text(head + mfma + 3 * filler + "\ts_nop 7\n" + read + tail)
    over = tmp_path / "over.s"
    over.write_text(head + mfma + "\tv_mov_b32_e32 v60, v1\n" + 2 * filler + read + tail)
    r = subprocess.run([sys.executable, scan, str(bad), "my_kernel"], capture_output=True, text=True)
    assert r.returncode == 1 and "1 VALU reads of a matrix" in r.stdout, r.stdout
    for f in (far, over):
        r = subprocess.run([sys.executable, scan, str(f), "my_kernel"], capture_output=True, text=True)
        assert r.returncode == 0 and "0 VALU reads of a matrix" in r.stdout, (f, r.stdout)
