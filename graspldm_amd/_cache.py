"""Derived-weight caches (BatchNorm-folded GEMM weights, the folded encoder head, MFMA-packed
set-abstraction / voxel / ResNet1D weight buffers, the 1-D engines) share two rules:

  * key: an entry is rebuilt when any source tensor is another OBJECT than the one it was built from (a Parameter that
    was deleted and re-assigned, `load_state_dict(..., assign=True)`: the sources are remembered weakly, so a new tensor
    that lands on a freed address with the same version is not mistaken for the old one), when any source tensor's
    (data_ptr, _version) changes, when the device changes, when the arithmetic mode changes (numerics.f32_only), or after
    `invalidate()`.  `_version` is bumped by in-place autograd-visible
    writes (`load_state_dict`, `p.copy_()`, optimiser steps) but NOT by writes through `p.data`;
    code that edits weights that way calls `graspldm_amd.invalidate_caches()`.
  * publication: an entry is produced by copies / kernels on whichever HIP stream is current at
    first use, and later consumed by launches on other streams (bench.py rotates three).  `publish()`
    blocks the host once, when the entry is built, until that stream has finished; every launch
    issued afterwards, on any stream, sees completed data.  Entries live on their module
    (no global dict keyed by id()); a `copy.deepcopy` of the module starts without them (they hold device handles and
    belong to the original's tensors) and builds its own at first use.
"""
import weakref

import torch

_EPOCH = [0]


def invalidate():
    """Drop every derived-weight cache (they rebuild on next use)."""
    _EPOCH[0] += 1


class ParamsKey:
    """What an entry was built from: a stamp (epoch, device, arithmetic mode, extras, each source's (data_ptr, _version))
    and the source tensor objects themselves, held weakly.  Two keys are equal when the stamps are and every source is alive
    and the same object on both sides."""
    __slots__ = ("stamp", "refs")
    __hash__ = None

    def __init__(self, stamp, tensors):
        self.stamp, self.refs = stamp, tuple(weakref.ref(t) for t in tensors)

    def __eq__(self, other):
        if not isinstance(other, ParamsKey):
            return NotImplemented
        if self.stamp != other.stamp or len(self.refs) != len(other.refs):
            return False
        for a, b in zip(self.refs, other.refs):
            t = a()
            if t is None or t is not b():
                return False
        return True

    def __repr__(self):
        return f"ParamsKey({self.stamp!r}, {len(self.refs)} sources)"


def params_key(tensors, device, *extra):
    # the arithmetic mode is part of every key: a plan packed under numerics.f32_only() (no split copies, f32 launches) is
    # not the plan of the default mode, and entering / leaving the switch after a module's first forward repacks instead of
    # silently mixing the two arithmetics
    from .numerics import split_enabled
    tensors = list(tensors)
    stamp = (_EPOCH[0], str(device), split_enabled()) + tuple(extra) + tuple((t.data_ptr(), t._version) for t in tensors)
    return ParamsKey(stamp, tensors)


def publish(device):
    device = torch.device(device)
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


class _Entry:
    __slots__ = ("key", "value")

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __deepcopy__(self, memo):
        return None   # a copied owner has no entry: cached() builds it from the copy's own tensors


def cached(owner, slot, key, build, device, required=False):
    """The entry `slot` of `owner` (an nn.Module or a plan object: the entry lives and dies with it), rebuilt by `build()`
    when `key` differs from the key it was stored under and published once per build.  A build that cannot be made in the
    split-f16 range (r1d_pack.SplitRangeError) is an entry like any other: None is stored under the key and returned until
    the key changes, so a weight version that does not fit the split is decided once.  `required`: the entry has no other
    form to fall back to (the 1-D engines), so that error reaches the caller and nothing is stored."""
    hit = owner.__dict__.get(slot)
    if hit is None or hit.key != key:
        from .r1d_pack import SplitRangeError
        try:
            value = build()
        except SplitRangeError:
            if required:
                raise
            value = None
        hit = owner.__dict__[slot] = _Entry(key, value)
        publish(device)
    return hit.value


def cached_key(owner, slot):
    """The key `slot` of `owner` is stored under: the key of an entry derived from that one."""
    return owner.__dict__[slot].key


def cached_value(owner, slot):
    """The value `slot` of `owner` holds now, or None where nothing was built yet (what was built is not checked against
    the weights: for questions about launches that already ran, like an engine's hand-off status)."""
    hit = owner.__dict__.get(slot)
    return None if hit is None else hit.value
