"""ctypes binding of libgldm_hip.so (C ABI: include/gldm.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If
the shared object is missing or a kernel launch fails, callers get an exception.
"""
import ctypes
import os

from . import _abi
from ._abi import GldmError  # noqa: F401

_PKG = os.path.dirname(os.path.abspath(__file__))
# GLDM_LIB: another build of the same library (diagnostic builds: make -C graspldm_amd/csrc EXTRA=... OUT=...)
LIB_PATH = os.environ.get("GLDM_LIB") or os.path.join(_PKG, "libgldm_hip.so")

ABI_VERSION = _abi.CONSTANTS["GLDM_ABI_VERSION"]   # of the header in the tree; lib() compares the built library with it

_lib = None

# name -> argtypes of every prototype of include/gldm.h (restypes: _abi.PROTOTYPES)
_SIGNATURES = {name: argtypes for name, (_, argtypes) in _abi.PROTOTYPES.items()}


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libgldm_hip.so (hipcc cross-compiles
    without a GPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise GldmError("building libgldm_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """The loaded library; raises GldmError loudly when it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GldmError(
            f"{LIB_PATH} is missing: the gfx950 HIP library is required (no fallback path). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C graspldm_amd/csrc`.")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7, and whichever copy is mapped first
    # serves both.  Loaded in front of torch, this library would bring /opt/rocm's copy in, and launches then fail once torch
    # initialises the device on it (seen as GLDM_ERR_LAUNCH from the first kernel of `python __graft_entry__.py smoke`).
    # The package plumbs torch tensors and streams anyway: import it first.
    import torch  # noqa: F401
    try:
        h = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise GldmError(f"cannot load {LIB_PATH}: {e}") from e
    def bind(name):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _abi.PROTOTYPES[name]
        return fn
    if bind("gldm_abi_version")() != ABI_VERSION:
        raise GldmError(f"libgldm_hip.so was built with ABI {h.gldm_abi_version()}, include/gldm.h has {ABI_VERSION}; rebuild it")
    for name in _abi.PROTOTYPES:
        bind(name)
    _lib = h
    return h


def call(name, *args):
    h = lib()
    status = getattr(h, name)(*args)
    if status != 0:
        raise GldmError(f"{name} failed: {h.gldm_status_string(status).decode()} (status {status})")


def ref(desc):
    """A descriptor struct (gldm_r1d_desc, gldm_unet1d_desc) as the pointer argument of an entry."""
    return ctypes.byref(desc)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def workspace(name, sizes, dtype, device, envelope):
    """The workspace of entry `name` for the shape `sizes` (the arguments of `name`_workspace_bytes): (an uninitialised
    tensor of `dtype` covering the bytes, the bytes); (None, 0) where the entry needs none.  A shape outside the entry's
    envelope raises GldmError with the status string and `envelope`, the caller's words for shape and limits."""
    import torch
    h = lib()
    nbytes = getattr(h, name + "_workspace_bytes")(*sizes)
    if nbytes < 0:
        raise GldmError(f"{name}: {h.gldm_status_string(int(nbytes)).decode()} ({envelope})")
    if nbytes == 0:
        return None, 0
    item = torch.empty((), dtype=dtype).element_size()
    return torch.empty((nbytes + item - 1) // item, dtype=dtype, device=device), nbytes


def current_stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
