"""Host-side preparation for the fused set-abstraction kernels (csrc/sa_mlp.hip: gldm_sa_mlp_forward*):
fold eval-mode BatchNorm into each 1x1 conv of a SharedMLP (shared_mlp.py:6-35) and lay the
weights out in MFMA A-fragment order: f32 (v_mfma_f32_16x16x4_f32, K padded to a multiple of 16) and split-f16."""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import dense
from ._cache import cached
from .r1d_pack import _Buf, mfma_a_fragments, mfma_a_fragments_f16x2

_OK_MTILES = (1, 2, 4, 8, 12, 16)
# modules without features (first layer = three coordinate products + bias): on the VALU of the gather threads (the hoisted
# form with a broadcast row) instead of a K = 32 block of the matrix pipe -- set by measurement, see DESIGN.md
# SSG-SA1 (3 -> 64 -> 64 -> 128, 512 centres x 64 at 256 clouds): hoisted in the single-tile kernel 1.81 ms, first layer on the
# matrix pipe in the multi-tile kernel 1.47 ms, hoisted in the multi-tile kernel (two tiles per pass) 1.22 ms
PRE_WITHOUT_FEATURES = True
_SA_RUN = 8   # centres per staged run (csrc/sa_mlp.hip: kSaRun)


def fusable(shared_mlp, num_neighbors):
    layers = shared_mlp.layers
    n = len(layers) // 3
    if n < 1 or n > 4 or 64 % int(num_neighbors) != 0:
        return False
    for i in range(n):
        cout = layers[3 * i].weight.shape[0]
        if cout % 16 or cout > 256 or (cout // 16) not in _OK_MTILES:
            return False
    return (layers[0].weight.shape[1] + 31) // 32 * 32 <= 256


def split_plan_ok(cins, couts, num_neighbors):
    """Shapes launch_sa3 takes (csrc/sa_mlp.hip; gldm_sa_mlp_forward_f16x2 and, with the tables of the layers behind a
    hoisted first one, gldm_sa_mlp_forward_f16x2_pre): 64-column tiles on split-f16 planes."""
    from .numerics import split_enabled
    if not split_enabled() or int(num_neighbors) not in (16, 32, 64) or not 1 <= len(couts) <= 4:
        return False
    # hidden widths are packed padded to the 32-row plane blocks (zero weight rows, zero bias: ReLU leaves zeros, and the
    # next layer's weights over those rows are zero): a 16-wide hidden layer (half-width PVCNN2) runs as a 32-wide one
    couts = [(c + 31) // 32 * 32 for c in couts[:-1]] + [couts[-1]]
    kpad = [(cins[0] + 31) // 32 * 32] + list(couts[:-1])
    if any(k % 32 or not (k // 32 <= 6 or k // 32 in (8, 9)) for k in kpad) or any(c % 16 for c in couts):
        return False
    if any(c not in (32, 64, 128, 256) for c in couts[:-1]):
        return False
    blocks_a = max([kpad[0] // 32] + [couts[l] // 32 for l in range(1, len(couts) - 1, 2)])
    blocks_b = max([0] + [couts[l] // 32 for l in range(0, len(couts) - 1, 2)])
    # behind the planes: the eight range words and the staged output rows of a run
    return (blocks_a + blocks_b) * 3072 * 4 + 64 + couts[-1] * _SA_RUN * 4 <= dense.LDS_BYTES


class LayerTable(NamedTuple):
    """The layers of one gldm_sa_mlp_forward* launch: the packed buffer on the device and the host tables into it."""
    weights: torch.Tensor
    cin_pad: ctypes.Array
    cout: ctypes.Array
    w_off: ctypes.Array
    b_off: ctypes.Array
    gain: Optional[ctypes.Array]    # split tables: (gain_r, gain_b) per layer, |layer output| <= gain_r max|input| + gain_b

    def args(self):
        """n_layers and the table pointers, in the order every gldm_sa_mlp_forward* entry takes them."""
        tables = (self.cin_pad, self.cout, self.w_off, self.b_off) + (() if self.gain is None else (self.gain,))
        return (len(self.cout), *(ctypes.cast(t, ctypes.c_void_p) for t in tables))


class HoistedTable(NamedTuple):
    """The split table of layers 2.. with the first layer hoisted out of the (centre, neighbour) pairs:
    W1 [x - c; f] + b1 = W1a (x - c) + (W1b f + b1).  Rows padded to c1p = whole 32-row plane blocks (zero rows)."""
    table: LayerTable
    wa_off: int             # W1a [c1p][4] behind the layer tables in table.weights
    w1b: torch.Tensor       # [c1p, C] on the device
    b1: torch.Tensor        # [c1p]


def _table(buf, device, cin_pad, cout, w_off, b_off, gain=None):
    arr = ctypes.c_int32 * len(cout)
    return LayerTable(buf.tensor().to(device), arr(*cin_pad), arr(*cout), arr(*w_off), arr(*b_off),
                      None if gain is None else (ctypes.c_float * len(gain))(*gain))


def pack_split_table(folded, device, behind=None):
    """Split-f16 fragments [cout x K padded to 32] + biases of the folded (W, b) layers; hidden widths padded to whole
    plane blocks.  `behind`: a tensor stored after the tables.  -> (LayerTable, offset of `behind`)."""
    buf = _Buf()
    cin_pad, cout, w_off, b_off, gain = [], [], [], [], []
    for i, (w, b) in enumerate(folded):
        # |layer output| <= gain_r max|input| + gain_b: the kernel scales the hidden layers' planes from this bound
        gain += [float(w.double().abs().sum(dim=1).max()), float(b.double().abs().max())]
        kpad = (w.shape[1] + 31) // 32 * 32
        rows = w.shape[0] if i == len(folded) - 1 else (w.shape[0] + 31) // 32 * 32
        wp = torch.zeros(rows, kpad)
        wp[: w.shape[0], : w.shape[1]] = w.cpu()
        bp = torch.zeros(rows)
        bp[: w.shape[0]] = b.cpu()
        cin_pad.append(kpad)
        cout.append(rows)
        w_off.append(buf.add(mfma_a_fragments_f16x2(wp)))
        b_off.append(buf.add(bp))
    off = None if behind is None else int(buf.add(behind.reshape(-1)))
    return _table(buf, device, cin_pad, cout, w_off, b_off, gain), off


class SaMlpPlan:
    """Packed weights of one SharedMLP(dim=2) on the device + the layer tables, for one weight version (the owner keys
    the plan; its lazily packed tables are entries of the plan and are decided once).  Where the layer plan fits the
    split-f16 kernel (split_plan_ok: the PointNet++ / PVCNN2 set-abstraction shapes), `run` takes that one; the f32-MFMA
    plan is packed either way (other neighbour counts / widths)."""

    def __init__(self, shared_mlp, device):
        layers = shared_mlp.layers
        self._folded = [dense.fold_conv_bn(layers[i], layers[i + 1]) for i in range(0, len(layers) - 2, 3)]
        self._device = device
        buf = _Buf()
        cin_pad, cout, w_off, b_off = [], [], [], []
        for i, (w, b) in enumerate(self._folded):
            # K in pairs of 16-deep blocks: the kernels' weight-fragment pipeline runs two blocks per trip (an odd count
            # would fall back to load-wait-compute per block); the padding rows are zero in the weights and the tile
            kpad = (w.shape[1] + 31) // 32 * 32 if i == 0 else (w.shape[1] + 15) // 16 * 16  # later layers: cin = cout of the previous one
            wp = torch.zeros(w.shape[0], kpad)
            wp[:, : w.shape[1]] = w.cpu()
            cin_pad.append(kpad)
            cout.append(w.shape[0])
            w_off.append(buf.add(mfma_a_fragments(wp)))
            b_off.append(buf.add(b.cpu()))
        self.f32 = _table(buf, device, cin_pad, cout, w_off, b_off)

    def _split_plan(self):
        """The split LayerTable of every layer, packed on first use; None: a folded weight beyond the f16 range."""
        return cached(self, "_split", None, lambda: pack_split_table(self._folded, self._device)[0], self._device)

    def _pack_pre(self):
        w1, b1 = self._folded[0]
        c1 = w1.shape[0]
        c1p = (c1 + 31) // 32 * 32
        wa = torch.zeros(c1p, 4)
        wa[:c1, :3] = w1[:, :3].cpu()
        table, wa_off = pack_split_table(self._folded[1:], self._device, behind=wa)
        w1b = torch.zeros(c1p, w1.shape[1] - 3)
        w1b[:c1] = w1[:, 3:].cpu()
        b1p = torch.zeros(c1p)
        b1p[:c1] = b1.cpu()
        return HoistedTable(table, wa_off, w1b.to(self._device), b1p.to(self._device))

    def _pre_plan(self):
        """The HoistedTable (gldm_sa_mlp_forward_f16x2_pre), packed on first use; None: beyond the f16 range."""
        return cached(self, "_pre", None, self._pack_pre, self._device)

    def _first_layer_per_point(self, features, pre):
        """[B, N, c1p] (POINT-major) = W1b f + b1: the split-f16 pointwise launch writing that layout where its shape
        set allows, else the any-shape kernel and a transposing copy."""
        x = features.contiguous().float()
        c1p, cin = pre.w1b.shape
        if dense.split_mlp_supported(x, cin, c1p):
            ws = cached(self, "_pre_ws", None, lambda: dense.split_fragments(pre.w1b).to(x.device), x.device)
            if ws is not None:
                b, _, n = x.shape
                y = torch.empty((b, n, c1p), dtype=torch.float32, device=x.device)
                with torch.cuda.device(x.device):
                    L.call("gldm_pointwise_mlp_f16x2_pm", L.ptr(x), L.ptr(ws), L.ptr(pre.b1), b, cin, c1p, n, 0, L.ptr(y),
                           L.current_stream(x.device))
                return y
        return dense._gemm_bias_act(x, pre.w1b, pre.b1, False).transpose(1, 2).contiguous()

    def run(self, points, centers, features, idx):
        b, _, n = points.shape
        m, u = idx.shape[1], idx.shape[2]
        c = 0 if features is None else features.shape[1]
        cins = [w.shape[1] for w, _ in self._folded]
        couts = [w.shape[0] for w, _ in self._folded]
        out = torch.empty((b, couts[-1], m), dtype=torch.float32, device=points.device)
        st = L.current_stream(points.device)
        # first layer per POINT instead of per (centre, neighbour) pair: whenever there are features to hoist and a layer
        # behind it (every point sits in m u / n balls on average: worth it from 2 upwards)
        hoist = (c > 0 and m * u >= 2 * n) or (c == 0 and PRE_WITHOUT_FEATURES)
        pre = None
        if hoist and len(couts) >= 2 and couts[0] <= 256 and split_plan_ok(couts[:-1], couts[1:], u):
            pre = self._pre_plan()
        if pre is not None:
            row = self._first_layer_per_point(features, pre) if c > 0 else pre.b1   # no features: the row b1 for every point
            with torch.cuda.device(points.device):
                L.call("gldm_sa_mlp_forward_f16x2_pre", L.ptr(points), L.ptr(centers), L.ptr(row), 0 if c > 0 else 1, L.ptr(idx),
                       L.ptr(pre.table.weights), pre.wa_off, b, n, m, u, *pre.table.args(), L.ptr(out), st)
            return out
        split = self._split_plan() if split_plan_ok(cins, couts, u) else None
        entry, table = ("gldm_sa_mlp_forward", self.f32) if split is None else ("gldm_sa_mlp_forward_f16x2", split)
        with torch.cuda.device(points.device):
            L.call(entry, L.ptr(points), L.ptr(centers), L.ptr(features), L.ptr(idx), L.ptr(table.weights), b, c, n, m, u,
                   *table.args(), L.ptr(out), st)
        return out
