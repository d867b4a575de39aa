"""Build the reference's own point-op kernels for gfx950.  TEST INFRASTRUCTURE.

The six ``.cu`` files of the reference's ``_pvcnn_backend`` extension are
compiled as HIP, unmodified and in place from the reference tree, against the
stub headers of ``oracle/ref_shim/`` and linked with ``ref_shim/entry.hip`` into

  libpvcnn_ref.so         the compiler's default contraction (fused multiply-adds
                          where it likes: the analogue of nvcc's default fmad)
  libpvcnn_ref_strict.so  -ffp-contract=off: every product and sum rounded once,
                          the arithmetic oracle/point_ops.c restates

plus ``stamp.json`` (flags, compiler version, sha256 of every reference source
read).  Nothing else is written to the output directory: no copy of a reference
source, no preprocessed text, no object file.  The products stay out of git.

  python -m oracle.ref_build [out_dir]
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from .ref_import import REFERENCE_ROOT, reference_available

_HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_DIR = os.path.join(_HERE, "ref_shim")
OUT_DIR = os.path.join(_HERE, "_ref")
SRC_REL = "grasp_ldm/models/modules/ext/pvcnn/modules/functional/src"
KERNEL_SOURCES = ("ball_query/ball_query.cu", "grouping/grouping.cu", "interpolate/neighbor_interpolate.cu",
                  "interpolate/trilinear_devox.cu", "sampling/sampling.cu", "voxelization/vox.cu")
HEADERS = ("cuda_utils.cuh", "ball_query/ball_query.cuh", "grouping/grouping.cuh",
           "interpolate/neighbor_interpolate.cuh", "interpolate/trilinear_devox.cuh", "sampling/sampling.cuh",
           "voxelization/vox.cuh")
ARCH = "gfx950"
COMMON_FLAGS = ("-x", "hip", f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17")
VARIANTS = {"libpvcnn_ref.so": (), "libpvcnn_ref_strict.so": ("-ffp-contract=off",)}
STAMP = "stamp.json"
ENTRIES = ("ref_set_stream", "ref_ball_query", "ref_grouping", "ref_gather_features", "ref_furthest_point_sampling",
           "ref_three_nearest_neighbors_interpolate", "ref_trilinear_devoxelize", "ref_avg_voxelize")


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run(cmd):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"reference kernel build failed ({p.returncode}): {' '.join(cmd)}\n{p.stdout}")


def _sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def build(out_dir=OUT_DIR, jobs=None):
    """Compile both libraries and the stamp into `out_dir`; returns the stamp.  Raises when the reference tree is
    absent or a compile fails."""
    if not reference_available():
        raise RuntimeError(f"reference tree not found at {REFERENCE_ROOT}")
    src = os.path.join(REFERENCE_ROOT, SRC_REL)
    hipcc = _hipcc()
    inc = ["-I", SHIM_DIR, "-I", src]
    units = [os.path.join(src, s) for s in KERNEL_SOURCES] + [os.path.join(SHIM_DIR, "entry.hip")]
    os.makedirs(out_dir, exist_ok=True)
    jobs = jobs or min(8, os.cpu_count() or 1)
    # objects live in a scratch directory that is gone when this returns
    with tempfile.TemporaryDirectory(prefix="pvcnn_ref_") as tmp:
        work = []
        for lib, extra in VARIANTS.items():
            for i, u in enumerate(units):
                obj = os.path.join(tmp, f"{lib}.{i}.o")
                work.append((lib, obj, [hipcc, *COMMON_FLAGS, *extra, *inc, "-c", u, "-o", obj]))
        with ThreadPoolExecutor(jobs) as pool:
            list(pool.map(lambda w: _run(w[2]), work))
        for lib in VARIANTS:
            objs = [w[1] for w in work if w[0] == lib]
            linked = os.path.join(tmp, lib)
            _run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", linked, *objs])
            shutil.copyfile(linked, os.path.join(out_dir, lib))
            os.chmod(os.path.join(out_dir, lib), 0o755)
    version = subprocess.run([hipcc, "--version"], stdout=subprocess.PIPE, text=True).stdout.splitlines()
    stamp = {
        "hipcc_version": next((ln for ln in version if "HIP version" in ln), version[0] if version else ""),
        "arch": ARCH,
        "flags": {lib: [*COMMON_FLAGS, *extra] for lib, extra in VARIANTS.items()},
        "sources_sha256": {rel: _sha256(os.path.join(src, rel)) for rel in KERNEL_SOURCES + HEADERS},
        "shim_sha256": {rel: _sha256(os.path.join(SHIM_DIR, rel))
                        for rel in ("entry.hip", "cuda.h", "cuda_runtime.h", "ATen/ATen.h", "ATen/cuda/CUDAContext.h")},
    }
    with open(os.path.join(out_dir, STAMP), "w") as f:
        json.dump(stamp, f, indent=1, sort_keys=True)
        f.write("\n")
    return stamp


if __name__ == "__main__":
    s = build(sys.argv[1] if len(sys.argv) > 1 else OUT_DIR)
    print(json.dumps(s["flags"]))
