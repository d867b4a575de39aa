"""CPU: the recipe that compiles the reference's own point-op kernels for gfx950 (oracle/ref_build.py).  Needs the
reference tree; skipped where it is absent (a clean checkout, the GPU machine)."""
import os

import pytest

from oracle import ref_backend, ref_build
from oracle.ref_import import reference_available

pytestmark = pytest.mark.skipif(not reference_available(), reason="reference tree absent: nothing to compile")


def test_recipe_builds_two_loadable_libraries_and_nothing_else(tmp_path):
    out = tmp_path / "_ref"
    stamp = ref_build.build(str(out))
    assert sorted(os.listdir(out)) == sorted([*ref_backend.LIBS.values(), ref_build.STAMP])
    for name in ref_backend.LIBS.values():
        lib = ref_backend.load_library(str(out / name))        # binds every entry: AttributeError if one is missing
        for entry in ref_build.ENTRIES:
            assert hasattr(lib, entry), (name, entry)
    assert len([e for e in ref_build.ENTRIES if e != "ref_set_stream"]) == 7
    assert "-ffp-contract=off" in stamp["flags"]["libpvcnn_ref_strict.so"]
    assert not any(f.startswith("-ffp-contract") for f in stamp["flags"]["libpvcnn_ref.so"])
    assert set(stamp["sources_sha256"]) >= set(ref_build.KERNEL_SOURCES) and stamp["hipcc_version"]
    assert (out / "libpvcnn_ref.so").read_bytes() != (out / "libpvcnn_ref_strict.so").read_bytes()
