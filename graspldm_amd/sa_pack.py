"""Host-side preparation for the fused set-abstraction kernels (csrc/sa_mlp.hip: gldm_sa_mlp_forward*):
fold eval-mode BatchNorm into each 1x1 conv of a SharedMLP (shared_mlp.py:6-35) and lay the
weights out in MFMA A-fragment order: f32 (v_mfma_f32_16x16x4_f32, K padded to a multiple of 16) and split-f16."""
import ctypes
from functools import lru_cache
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from . import dense
from ._cache import cached
from .r1d_pack import _Buf, mfma_a_fragments, mfma_a_fragments_f16x2

# modules without features (first layer = three coordinate products + bias): on the VALU of the gather threads (the hoisted
# form with a broadcast row) instead of a K = 32 block of the matrix pipe -- set by measurement, see DESIGN.md
# SSG-SA1 (3 -> 64 -> 64 -> 128, 512 centres x 64 at 256 clouds): hoisted in the single-tile kernel 1.81 ms, first layer on the
# matrix pipe in the multi-tile kernel 1.47 ms, hoisted in the multi-tile kernel (two tiles per pass) 1.22 ms
PRE_WITHOUT_FEATURES = True

# Which layer plans a launch takes is the library's answer (gldm_sa_mlp_supported, gldm_sa_mlp_f16x2_lds_bytes: the planners
# of gldm_sa_mlp_forward and launch_sa3, csrc/sa_mlp.hip), cached per shape.  What stands next to it in a predicate below is
# routing policy, each term a named constant; numerics.split_enabled() stays outside the cache.
PLANNED_PLANES = (3, 2)        # policy: split_plan_ok counts the plane regions as the three bf16 planes of ABI 5-8 (12288 bytes per 32-row block) where launch_sa3 keeps two f16 ones (8192); DESIGN.md, PointNet2MSG -- the two plans it refuses run and compared, not timed (tests/test_envelope_gpu.py::test_sa_run_with_the_planning_figure_at_the_launch_s_own): not lifted untimed
PLANNED_LDS_BYTES = 160 * 1024       # policy: the LDS that figure was planned against
MSG_MAX_POOLED_ROWS = 256            # policy: pooled rows wider than 256 -- 512 / 1008 / 1024 rows run and compared, not timed (tests/test_envelope_gpu.py::test_sa_run_msg_with_a_policy_constant_at_the_launch_s_bound, test_sa_mlp_accepted_plans; DESIGN.md, PointNet2MSG)
MSG_MAX_LAYERS = 4                   # policy: a branch as deep as every route takes it whole (the hoisted form alone would take a fifth layer; no f32 launch stands behind it)
_F32_WIDTHS = (16, 32, 64, 128, 192, 256)   # packing: hidden widths the f32 tables pad to (_f32_width)
_PLANE_WIDTHS = (32, 64, 128, 256)          # packing: hidden widths the split tables pad to (_plane_width)


def _pad32(c):
    return (c + 31) // 32 * 32


@lru_cache(maxsize=None)
def _f32_takes(c, u, cin_pad, cout):
    """gldm_sa_mlp_forward's own answer for a layer plan (tuples as its tables hold them, c feature rows)."""
    arr = ctypes.c_int32 * len(cout)
    return L.lib().gldm_sa_mlp_supported(c, u, len(cout), arr(*cin_pad), arr(*cout)) == 0


@lru_cache(maxsize=None)
def _sa3_bytes(pre, u, cin_pad, cout):
    """launch_sa3's own answer for a layer plan: (dynamic LDS of its single-tile launch, the plane regions' share), or None."""
    arr = ctypes.c_int32 * len(cout)
    planes = ctypes.c_longlong(0)
    total = L.lib().gldm_sa_mlp_f16x2_lds_bytes(int(pre), 0, u, len(cout), arr(*cin_pad), arr(*cout), ctypes.byref(planes))
    return None if total < 0 else (int(total), int(planes.value))


def _tables(kpad0, couts):
    """(cin_pad, cout) as a layer table holds them: every later layer reads the rows of the one in front."""
    couts = tuple(int(c) for c in couts)
    return (int(kpad0),) + couts[:-1], couts


def fusable(shared_mlp, num_neighbors):
    """gldm_sa_mlp_forward takes the module's widths as they are (csrc/sa_mlp.hip; the library's answer)."""
    layers = shared_mlp.layers
    couts = [layers[3 * i].weight.shape[0] for i in range(len(layers) // 3)]
    cin = layers[0].weight.shape[1]
    return bool(couts) and _f32_takes(max(cin - 3, 0), int(num_neighbors), *_tables(_pad32(cin), couts))


def split_plan_ok(cins, couts, num_neighbors):
    """Shapes SaMlpPlan.run sends to launch_sa3 (csrc/sa_mlp.hip; gldm_sa_mlp_forward_f16x2 and, with the tables of the
    layers behind a hoisted first one, gldm_sa_mlp_forward_f16x2_pre): the library's answer, and the routing policy -- the
    launch's LDS with its plane regions counted at PLANNED_PLANES within PLANNED_LDS_BYTES.  The policy refuses plans
    the launcher takes ([259] -> [128, 256] at U = 16: 13 plane blocks + a 256-row output are 114,752 bytes)."""
    from .numerics import split_enabled
    if not split_enabled() or not couts:
        return False
    # hidden widths are packed padded to the 32-row plane blocks (zero weight rows, zero bias: ReLU leaves zeros, and the
    # next layer's weights over those rows are zero): a 16-wide hidden layer (half-width PVCNN2) runs as a 32-wide one
    couts = [_pad32(c) for c in couts[:-1]] + [couts[-1]]
    lds = _sa3_bytes(False, int(num_neighbors), *_tables(_pad32(cins[0]), couts))   # (all of it, its plane regions)
    return lds is not None and lds[0] - lds[1] + lds[1] * PLANNED_PLANES[0] // PLANNED_PLANES[1] <= PLANNED_LDS_BYTES


def _plane_width(c):
    """A hidden width as the split tables pack it: the next width the kernels take (96 -> 128, 196 -> 256; zero weight rows
    and zero bias, ReLU leaves zeros, the next layer's weights over those rows are zero); beyond 256: whole plane blocks."""
    return next((w for w in _PLANE_WIDTHS if w >= c), _pad32(c))


def _f32_width(c):
    """The same for the f32 tables: the next width gldm_sa_mlp_forward has an m-tile count for."""
    return next((w for w in _F32_WIDTHS if w >= c), c)


def sa3_takes(kpad0, couts, num_neighbors, pre=False):
    """What launch_sa3 itself takes (the library's answer): kpad0 = rows of the first layer's input, or of the per-point
    layer's output when `pre`.  split_plan_ok asks the same planner and adds its policy."""
    return bool(couts) and _sa3_bytes(bool(pre), int(num_neighbors), *_tables(kpad0, couts)) is not None


def msg_fold(num_neighbors):
    """(u the fused kernels run with, h): a neighbourhood of U = 64 h runs as h centres of 64 columns and is folded by
    gldm_group_max_concat -- exact: every tile's maximum is final, max is associative."""
    u = int(num_neighbors)
    return (64, u // 64) if u in (128, 256) else (u, 1)


def msg_route(cin, couts, num_neighbors, hoist=True):
    """Which fused launch one branch of a multi-scale set-abstraction module takes (SaMlpPlan.run_msg), or None (the
    grouped tensor + GEMMs).  cin: rows of the grouped input (3 + C); couts: the SharedMLP's widths.
      'pre'      gldm_sa_mlp_forward_f16x2_pre: first layer per point, hidden widths padded to _plane_width
      'split'    gldm_sa_mlp_forward_f16x2
      'f32'      gldm_sa_mlp_forward, hidden widths padded to _f32_width
      'f32_pre'  gldm_sa_mlp_forward with the first layer hoisted (inputs wider than its 256 rows)
    Every route is what its launch takes (sa3_takes, gldm_sa_mlp_supported); policy: pooled rows within MSG_MAX_POOLED_ROWS,
    MSG_MAX_LAYERS layers."""
    from .numerics import split_enabled
    u, _ = msg_fold(num_neighbors)
    couts = [int(c) for c in couts]
    n = len(couts)
    if not 1 <= n <= MSG_MAX_LAYERS or couts[-1] > MSG_MAX_POOLED_ROWS:
        return None
    if split_enabled():
        pc = [_plane_width(c) for c in couts[:-1]] + couts[-1:]
        split_ok = sa3_takes(_pad32(cin), pc, u)
        if n >= 2 and (hoist or not split_ok) and sa3_takes(_pad32(couts[0]), pc[1:], u, pre=True):
            return "pre"
        if split_ok:
            return "split"
    fc = [_f32_width(c) for c in couts[:-1]] + couts[-1:]
    if _f32_takes(max(cin - 3, 0), u, *_tables(_pad32(cin), fc)):
        return "f32"
    if n >= 2 and cin > 3 and _f32_takes(fc[0], u, *_tables(_pad32(3 + fc[0]), fc)):
        return "f32_pre"
    return None


def msg_fusable(shared_mlp, num_neighbors):
    """Next to `fusable` / `split_plan_ok`: the branches of a multi-scale module that run fused (either hoisting choice)."""
    layers = shared_mlp.layers
    couts = [layers[i].weight.shape[0] for i in range(0, len(layers), 3)]
    cin = layers[0].weight.shape[1]
    if msg_route(cin, couts, num_neighbors) is None:
        return False
    # ... and an f32 launch behind it: a folded weight beyond the f16 range sends run_msg there (as SaMlpPlan.run always can)
    from .numerics import f32_only
    with f32_only():
        return msg_route(cin, couts, num_neighbors) is not None


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
    """Split-f16 fragments [cout x K padded to 32] + biases of the folded (W, b) layers; hidden widths padded to the
    next width the kernels take (_plane_width).  `behind`: a tensor stored after the tables.  -> (LayerTable, offset of `behind`)."""
    buf = _Buf()
    cin_pad, cout, w_off, b_off, gain = [], [], [], [], []
    for i, (w, b) in enumerate(folded):
        # |layer output| <= gain_r max|input| + gain_b: the kernel scales the hidden layers' planes from this bound
        gain += [float(w.double().abs().sum(dim=1).max()), float(b.double().abs().max())]
        kpad = (w.shape[1] + 31) // 32 * 32 if i == 0 else cout[-1]   # later layers: the padded rows of the one in front
        rows = w.shape[0] if i == len(folded) - 1 else _plane_width(w.shape[0])
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


def pack_f32_table(folded, device):
    """f32 A fragments + biases of the folded (W, b) layers (gldm_sa_mlp_forward); hidden widths padded to the next width
    the kernel has an m-tile count for (_f32_width: zero rows, zero bias)."""
    buf = _Buf()
    cin_pad, cout, w_off, b_off = [], [], [], []
    for i, (w, b) in enumerate(folded):
        # K in pairs of 16-deep blocks: the kernels' weight-fragment pipeline runs two blocks per trip (an odd count
        # would fall back to load-wait-compute per block); the padding rows are zero in the weights and the tile
        kpad = (w.shape[1] + 31) // 32 * 32 if i == 0 else (cout[-1] + 15) // 16 * 16  # later layers: cin = (padded) cout of the previous one
        rows = w.shape[0] if i == len(folded) - 1 else _f32_width(w.shape[0])
        wp = torch.zeros(rows, kpad)
        wp[: w.shape[0], : w.shape[1]] = w.cpu()
        bp = torch.zeros(rows)
        bp[: w.shape[0]] = b.cpu()
        cin_pad.append(kpad)
        cout.append(rows)
        w_off.append(buf.add(mfma_a_fragments(wp)))
        b_off.append(buf.add(bp))
    return _table(buf, device, cin_pad, cout, w_off, b_off)


class SaMlpPlan:
    """Packed weights of one SharedMLP(dim=2) on the device + the layer tables, for one weight version (the owner keys
    the plan; its lazily packed tables are entries of the plan and are decided once).  Where the layer plan fits the
    split-f16 kernel (split_plan_ok: the PointNet++ / PVCNN2 set-abstraction shapes), `run` takes that one; the f32-MFMA
    plan is packed either way (other neighbour counts / widths)."""

    def __init__(self, shared_mlp, device):
        layers = shared_mlp.layers
        self._folded = [dense.fold_conv_bn(layers[i], layers[i + 1]) for i in range(0, len(layers) - 2, 3)]
        self._device = device
        self.f32 = pack_f32_table(self._folded, device)

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

    def _f32_pre_plan(self):
        """'f32_pre': y = W1b f + b1 per point (rows padded to _f32_width), then the f32 kernel with y as its features and
        [W1a | I] as its first layer: W1 [x - c; f] + b1 = W1a (x - c) + y, in exact f32 products."""
        def pack():
            w1, b1 = self._folded[0]
            c1, c1p = w1.shape[0], _f32_width(w1.shape[0])
            w1b = torch.zeros(c1p, w1.shape[1] - 3)
            w1b[:c1] = w1[:, 3:].cpu()
            b1p = torch.zeros(c1p)
            b1p[:c1] = b1.cpu()
            first = torch.zeros(c1p, 3 + c1p)
            first[:c1, :3] = w1[:, :3].cpu()
            first[:, 3:] = torch.eye(c1p)
            table = pack_f32_table([(first, torch.zeros(c1p))] + list(self._folded[1:]), self._device)
            return table, w1b.to(self._device), b1p.to(self._device)
        return cached(self, "_f32_pre", None, pack, self._device)

    def run_msg(self, points, centers, features, idx, out, c0):
        """One branch of a multi-scale module: the fused MLP on the route msg_route names, its [B, C, M] rows written into
        rows c0.. of the module's output `out` [B, sum C, M] by gldm_group_max_concat (no grouped tensor, no torch.cat).
        U = 64 h: idx [B, M, 64 h] viewed as [B, M h, 64] with every centre repeated h times, folded by the same launch."""
        from .backend import _backend
        b, _, n = points.shape
        m, u_all = idx.shape[1], idx.shape[2]
        u, h = msg_fold(u_all)
        if h > 1:
            idx = idx.view(b, m * h, u)
            centers = centers.repeat_interleave(h, dim=2)
        mh = m * h
        c = 0 if features is None else features.shape[1]
        couts = [w.shape[0] for w, _ in self._folded]
        hoist = (c > 0 and mh * u >= 2 * n) or (c == 0 and PRE_WITHOUT_FEATURES)
        route = msg_route(3 + c, couts, u, hoist)
        pre = split = None
        if route == "pre":
            pre = self._pre_plan()
        elif route == "split":
            split = self._split_plan()
        if pre is None and split is None and route in ("pre", "split"):   # a folded weight beyond the f16 range
            from .numerics import f32_only
            with f32_only():
                route = msg_route(3 + c, couts, u, hoist)
        if route is None:
            raise L.GldmError("run_msg: no fused launch takes this branch (msg_route)")
        # the per-point layer first: its temporaries are gone before the pooled rows are allocated
        row = None if pre is None else (self._first_layer_per_point(features, pre) if c > 0 else pre.b1)
        part = torch.empty((b, couts[-1], mh), dtype=torch.float32, device=points.device)
        st = L.current_stream(points.device)
        with torch.cuda.device(points.device):
            if pre is not None:
                L.call("gldm_sa_mlp_forward_f16x2_pre", L.ptr(points), L.ptr(centers), L.ptr(row), 0 if c > 0 else 1, L.ptr(idx),
                       L.ptr(pre.table.weights), pre.wa_off, b, n, mh, u, *pre.table.args(), L.ptr(part), st)
            elif split is not None:
                L.call("gldm_sa_mlp_forward_f16x2", L.ptr(points), L.ptr(centers), L.ptr(features), L.ptr(idx),
                       L.ptr(split.weights), b, c, n, mh, u, *split.args(), L.ptr(part), st)
            elif route == "f32":
                L.call("gldm_sa_mlp_forward", L.ptr(points), L.ptr(centers), L.ptr(features), L.ptr(idx), L.ptr(self.f32.weights),
                       b, c, n, mh, u, *self.f32.args(), L.ptr(part), st)
            else:
                table, w1b, b1 = self._f32_pre_plan()
                y = dense._gemm_bias_act(features.contiguous().float(), w1b, b1, False)
                L.call("gldm_sa_mlp_forward", L.ptr(points), L.ptr(centers), L.ptr(y), L.ptr(idx), L.ptr(table.weights),
                       b, y.shape[1], n, mh, u, *table.args(), L.ptr(part), st)
        return _backend.group_max_concat(part, h, out, c0)
