"""Record what the reference's own kernels compute, for checkouts without a GPU.  TEST INFRASTRUCTURE; runs on the
MI355X (needs oracle/_ref/libpvcnn_ref_strict.so, built by oracle/ref_build.py):

  python -m oracle.record_ref_point_ops [tests/golden/ref_point_ops.npz]

Executes ref_backend.strict on the `record` subset of oracle/ref_cases.CASES and stores, per case, the kernels' outputs
under "<case name>/<output>", plus a JSON manifest of (op, params) from which ref_cases.make_inputs() regenerates every
input on the CPU.  Integers go in the narrowest dtype that holds them; the float-atomic `out` of avg_voxelize has no
fixed bit pattern and is not stored.  tests/test_oracle_point_ops.py replays the file against oracle/point_ops.c.
"""
import json
import os
import sys

import numpy as np
import torch

from . import ref_backend, ref_cases

_DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                        "ref_point_ops.npz")


def narrow(a):
    """The narrowest signed integer dtype that holds every element of the int array."""
    lo, hi = (int(a.min()), int(a.max())) if a.size else (0, 0)
    for dt in (np.int8, np.int16, np.int32):
        if np.iinfo(dt).min <= lo and hi <= np.iinfo(dt).max:
            return a.astype(dt)
    return a


def record(path=_DEFAULT):
    if not torch.cuda.is_available():
        raise RuntimeError("the reference kernels run on the GPU only")
    if not ref_backend.available():
        raise RuntimeError("oracle/_ref/libpvcnn_ref*.so not built")
    arrays, manifest = {}, []
    for c in ref_cases.CASES:
        if not c["record"]:
            continue
        op, p = c["op"], c["params"]
        x = {k: v.cuda() for k, v in ref_cases.make_inputs(op, p).items()}
        outs = ref_cases.run(ref_backend.strict, op, p, x)
        kept = []
        for k, v in outs.items():
            if (op, k) in ref_cases.UNRECORDED:
                continue
            a = v.cpu().numpy()
            arrays[f"{c['name']}/{k}"] = narrow(a) if a.dtype == np.int32 else a
            kept.append(k)
        manifest.append({"op": op, "name": c["name"], "params": p, "outputs": kept})
    arrays["manifest"] = np.array(json.dumps(manifest))
    np.savez_compressed(path, **arrays)
    return path, len(manifest)


if __name__ == "__main__":
    out, n = record(sys.argv[1] if len(sys.argv) > 1 else _DEFAULT)
    print(f"recorded {n} cases -> {out} ({os.path.getsize(out)} bytes)")
