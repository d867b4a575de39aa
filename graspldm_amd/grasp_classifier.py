"""PointsBasedGraspClassifier (grasp_ldm/models/grasp_classifier.py:13-143): a cloud and the points of a gripper placed
at a pose -> the probability that the grasp succeeds.  Inference only.

  scene   gldm_grasp_scene: gripper control points at every pose, in the cloud's normalised frame, merged with the cloud
          and the label channel into the backbone's input [scenes, 4, Np + Ng] (one launch; `score_poses`).
  base    PVCNN / PVCNN2 with extra_feature_channels = 1 -> per-point features [scenes, C, N].
  head    gldm_cls_head: the `classifier` Sequential + sigmoid in one launch sequence (MFMA GEMM C -> 128 with ReLU, the
          128 -> 1 conv and the Linear over the point axis applied on the accumulators).  Shapes outside the kernel's
          limits (`cls_head_supported`) run the package's layer launches: pointwise_conv_bn_relu, pointwise_rows, linear.
"""
import ctypes
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import dense
from ._lib import GldmError
from .pvcnn import PVCNN, PVCNN2, SharedMLP

HEAD_MAX_C, HEAD_MAX_ROWS, HEAD_MAX_N = 2048, 512, 1 << 20
DEFAULT_MAX_BYTES = 2 << 30   # score_poses: features + backbone intermediates of one chunk of scenes (see _scene_bytes)


def cls_head_supported(c, rows, n):
    """The shape limits of gldm_cls_head (csrc/grasp_classifier.hip: head_shape_ok; GLDM_ERR_UNSUPPORTED outside them)."""
    return (c % 16 == 0 and 16 <= c <= HEAD_MAX_C and rows % 16 == 0 and 16 <= rows <= HEAD_MAX_ROWS
            and 1 <= n <= HEAD_MAX_N)


def fold_head(conv, bn, conv2, lin):
    """-> (W1' [rows, c], b1' [rows], w2 [rows], l [n], c0): classifier.0 with its BatchNorm folded (dense.fold_conv_bn),
    classifier.2's row, classifier.3's row and the constant lb + b2 sum(l), summed in f64."""
    w1, b1 = dense.fold_conv_bn(conv, bn)
    w2 = conv2.weight.detach().float().reshape(-1).contiguous()
    l = lin.weight.detach().float().reshape(-1).contiguous()
    b2 = float(conv2.bias.detach().double()) if conv2.bias is not None else 0.0
    lb = float(lin.bias.detach().double()) if lin.bias is not None else 0.0
    return w1, b1, w2, l, lb + b2 * float(l.double().sum())


class HeadPack(NamedTuple):
    w1: torch.Tensor      # A fragments of W1': split-f16 (K padded to 32) or f32
    b1: torch.Tensor
    w2: torch.Tensor
    l: torch.Tensor
    c0: float
    exact: bool           # w1 holds f32 fragments (numerics.f32_only(), or a weight beyond the f16 range)


def pack_head_weights(w1, b1, w2, l, c0, device):
    """The folded head (fold_head's tuple) packed for gldm_cls_head on `device`: W1' as split-f16 A fragments (K zero-padded
    to the 32-deep MFMA block), or as f32 fragments under numerics.f32_only() and for weights beyond the f16 range."""
    from .numerics import split_enabled
    from .r1d_pack import SplitRangeError, mfma_a_fragments, mfma_a_fragments_f16x2
    w = w1.detach().float().cpu()
    frag, exact = None, not split_enabled()
    if not exact:
        k = w.shape[1]
        if k % 32:
            w = torch.cat([w, torch.zeros(w.shape[0], 32 - k % 32)], dim=1)
        try:
            frag = mfma_a_fragments_f16x2(w)
        except SplitRangeError:   # |w| >= 65504 (a huge BatchNorm gain): the f32 form
            exact = True
    if exact:
        frag = mfma_a_fragments(w1.detach().float().cpu())
    dev = lambda t: t.detach().float().contiguous().to(device)   # noqa: E731
    return HeadPack(frag.to(device), dev(b1), dev(w2), dev(l), float(c0), exact)


def _pack_head(conv, bn, conv2, lin, device):
    return pack_head_weights(*fold_head(conv, bn, conv2, lin), device)


def cls_head(x, pack, rows):
    """gldm_cls_head on features x [b, c, n] -> (logit [b], prob [b])."""
    from . import _lib as L
    dense._need_cuda(x, "features")
    x = x.contiguous().float()
    b, c, n = x.shape
    h = L.lib()
    need = int(h.gldm_cls_head_workspace_bytes(b, c, rows, n))
    if need < 0:
        raise GldmError(f"gldm_cls_head takes no features of shape c={c}, rows={rows}, n={n}")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    logit = torch.empty(b, dtype=torch.float32, device=x.device)
    prob = torch.empty(b, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.call("gldm_cls_head", L.ptr(x), L.ptr(pack.w1), L.ptr(pack.b1), L.ptr(pack.w2), L.ptr(pack.l), ctypes.c_float(pack.c0),
               b, c, rows, n, int(pack.exact), L.ptr(ws), need, L.ptr(logit), L.ptr(prob), L.current_stream(x.device))
    return logit, prob


def grasp_scene(pc, H, gripper_points, pc_mean=None, pc_shift=0.0, pc_scale=1.0):
    """gldm_grasp_scene: pc [Bc, Np, 3] (normalised), H [Bc*G, 4, 4] (un-normalised cloud frame, row c*G + g of cloud c),
    gripper_points [Ng, 3], pc_mean [Bc, 3] or None -> x [Bc*G, 4, Np + Ng]."""
    from . import _lib as L
    for t, name in ((pc, "pc"), (H, "H"), (gripper_points, "gripper_points")):
        dense._need_cuda(t, name)
    if pc.ndim != 3 or pc.shape[-1] != 3 or H.ndim != 3 or H.shape[-2:] != (4, 4) or H.shape[0] % pc.shape[0]:
        raise RuntimeError(f"pc must be [Bc,Np,3] and H [Bc*G,4,4], not {tuple(pc.shape)} and {tuple(H.shape)}")
    if gripper_points.ndim != 2 or gripper_points.shape[-1] != 3:
        raise RuntimeError(f"gripper_points must be [Ng,3], not {tuple(gripper_points.shape)}")
    if not float(pc_scale) != 0.0:
        raise ValueError("pc_scale must not be zero")
    pc, H, gp = pc.contiguous().float(), H.contiguous().float(), gripper_points.to(pc.device).contiguous().float()
    mean = None
    if pc_mean is not None:
        mean = pc_mean.to(pc.device).float().reshape(-1, 3).contiguous()
        if mean.shape[0] != pc.shape[0]:
            raise RuntimeError(f"pc_mean must be [Bc,3], not {tuple(pc_mean.shape)}")
    bc, np_ = pc.shape[:2]
    g, ng = H.shape[0] // bc, gp.shape[0]
    x = torch.empty((bc * g, 4, np_ + ng), dtype=torch.float32, device=pc.device)
    with torch.cuda.device(pc.device):
        L.call("gldm_grasp_scene", L.ptr(pc), L.ptr(H), L.ptr(gp), L.ptr(mean), ctypes.c_float(pc_shift), ctypes.c_float(pc_scale),
               bc, g, np_, ng, L.ptr(x), L.current_stream(pc.device))
    return x


class PointsBasedGraspClassifier(nn.Module):
    SUPPORTED_BASE_NETWORKS = {"PVCNN": PVCNN, "PVCNN2": PVCNN2}

    def __init__(self, num_pc_points, points_backbone_config, loss_config: Optional[dict] = None):
        """grasp_classifier.py:18-52.  num_pc_points: points of the MERGED scene (cloud + gripper), the width of the final
        Linear.  loss_config is accepted and ignored (training is out of scope)."""
        super().__init__()
        t = points_backbone_config["type"]
        if t not in self.SUPPORTED_BASE_NETWORKS:
            raise NotImplementedError(f"Base network arch of type=`{t}` is not implemented. "
                                      f"Available base network types are: {list(self.SUPPORTED_BASE_NETWORKS)}")
        self.num_pc_points = num_pc_points
        self.base_network = self.SUPPORTED_BASE_NETWORKS[t](**dict(points_backbone_config["args"]))
        # create_mlp_components(out_channels=[128, 0.5, 1], classifier=True, dim=2) + Linear: ext/pvcnn/utils.py:30-62
        self.classifier = nn.Sequential(SharedMLP(self.base_network.out_channels, 128), nn.Dropout(0.5),
                                        nn.Conv1d(128, 1, 1), nn.Linear(num_pc_points, 1))
        self.sigmoid = nn.Sigmoid()

    # ------------------------------------------------------------------ head
    def _head_layers(self):
        mlp = self.classifier[0].layers
        return mlp[0], mlp[1], self.classifier[2], self.classifier[3]

    def _head_pack(self, device):
        from ._cache import cached, params_key
        conv, bn, conv2, lin = self._head_layers()
        src = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv2.weight, lin.weight]
        src += [t for t in (conv.bias, conv2.bias, lin.bias) if t is not None]
        return cached(self.classifier, "_gldm_head", params_key(src, device), lambda: _pack_head(conv, bn, conv2, lin, device),
                      device)

    def head(self, feats):
        """features [B, C, N] -> (logit [B], prob [B])."""
        dense._need_cuda(feats, "features")
        conv, bn, conv2, lin = self._head_layers()
        b, c, n = feats.shape
        rows = conv.weight.shape[0]
        if cls_head_supported(c, rows, n):
            return cls_head(feats, self._head_pack(feats.device), rows)
        y = dense.pointwise_conv_bn_relu(feats.contiguous().float(), conv, bn)
        logit = dense.linear(dense.pointwise_rows(y, conv2), lin).reshape(b)
        return logit, torch.sigmoid(logit)

    def _scores(self, x):
        """Backbone input x [B, 4, N] -> (logit [B], prob [B])."""
        if self.training:
            raise NotImplementedError("the classifier runs in eval mode only (training is out of scope)")
        if x.shape[-1] != self.num_pc_points:
            raise RuntimeError(f"the scene has {x.shape[-1]} points (cloud + gripper) but the classifier was built for "
                               f"num_pc_points={self.num_pc_points}")
        return self.head(self.base_network(x))

    # ------------------------------------------------------------- interface
    @torch.no_grad()
    def forward(self, pc, grasp_points, *, cls_target=None, compute_loss=True):
        """grasp_classifier.py:54-104.  pc [B, Np, 3], grasp_points [B, Ng, 3] -> (None, preds [B]; 0-d for B = 1)."""
        if compute_loss:
            raise NotImplementedError("the classification loss is training-only (out of scope): call forward(pc, "
                                      "grasp_points, compute_loss=False) for the predictions")
        return None, self.predict(pc, grasp_points)[1].squeeze()

    @torch.no_grad()
    def predict(self, pc, grasp_points):
        """forward's computation with the logits kept: (logit [B], prob [B])."""
        if not (pc.is_cuda and grasp_points.is_cuda):
            raise RuntimeError("pc and grasp_points must be CUDA tensors (graspldm_amd has no CPU path)")
        _check_finite(pc, "the input point cloud")
        _check_finite(grasp_points, "the grasp points")
        xyz = torch.cat((pc.float(), grasp_points.float()), dim=-2)
        label = torch.cat((torch.zeros_like(pc[..., :1], dtype=torch.float32),
                           torch.ones_like(grasp_points[..., :1], dtype=torch.float32)), dim=-2)
        return self._scores(torch.cat((xyz, label), dim=-1).transpose(1, 2).contiguous())

    def classify_grasps(self, pc, grasp_pose):
        return self.forward(pc, grasp_pose, compute_loss=False)[1]

    def _scene_bytes(self, n):
        """Bytes one scene holds while it runs: the features [C, N], three live point tensors of the widest layer and three
        voxel grids of the largest (channels x resolution^3) stage -- an estimate from above of what the backbone's launches
        keep alive at once, f32."""
        width = max([m.out_channels for m in self.base_network.modules() if isinstance(m, (nn.Conv1d, nn.Conv2d))] + [4])
        grid = max([m.out_channels * m.resolution ** 3 for m in self.base_network.modules()
                    if hasattr(m, "voxel_layers")] + [0])
        return 4 * (self.base_network.out_channels * n + 3 * width * n + 3 * grid)

    @torch.no_grad()
    def score_poses(self, pc, H, gripper_points=None, pc_mean=None, pc_shift=0.0, pc_scale=1.0, max_bytes=DEFAULT_MAX_BYTES,
                    return_logits=False):
        """Success probability of every pose: pc [Bc, Np, 3] normalised clouds, H [Bc, G, 4, 4] (or [Bc*G, 4, 4], row
        c*G + g of cloud c) in the un-normalised cloud frame -> [Bc, G].  gripper_points [Ng, 3] (default:
        gripper.control_points(num_pc_points - Np)); pc_mean [Bc, 3], pc_shift, pc_scale: the cloud's normalisation
        (x_norm = (x - pc_mean - pc_shift) / pc_scale; None / 0 / 1: the poses are in the clouds' frame already).
        Scenes run in chunks whose features and backbone intermediates (_scene_bytes) stay under max_bytes (default 2 GiB:
        ~190 scenes of 1088 points at C = 512); a scene's score does not depend on the chunking."""
        if not (pc.is_cuda and H.is_cuda):
            raise RuntimeError("pc and H must be CUDA tensors (graspldm_amd has no CPU path)")
        if pc.ndim != 3:
            raise RuntimeError(f"pc must be [Bc,Np,3], not {tuple(pc.shape)}")
        bc, np_ = pc.shape[:2]
        H = H.reshape(-1, 4, 4)
        if H.shape[0] % bc:
            raise RuntimeError(f"{H.shape[0]} poses do not divide over {bc} clouds")
        g = H.shape[0] // bc
        _check_finite(pc, "the input point cloud")
        _check_finite(H, "the grasp poses")
        if gripper_points is None:
            from .gripper import control_points
            if self.num_pc_points <= np_:
                raise RuntimeError(f"a cloud of {np_} points leaves no room for gripper points in num_pc_points={self.num_pc_points}")
            gripper_points = control_points(self.num_pc_points - np_, device=pc.device)
        gripper_points = gripper_points.to(pc.device)
        n = np_ + gripper_points.shape[0]
        if n != self.num_pc_points:
            raise RuntimeError(f"the scene has {n} points (cloud {np_} + gripper {gripper_points.shape[0]}) but the classifier "
                               f"was built for num_pc_points={self.num_pc_points}")
        mean = None if pc_mean is None else pc_mean.to(pc.device).float().reshape(bc, 3)
        # whole clouds per chunk while a cloud's poses fit, else a cloud's poses in pieces
        per_chunk = max(1, int(max_bytes) // self._scene_bytes(n))
        out = torch.empty(bc * g, dtype=torch.float32, device=pc.device)
        logits = torch.empty_like(out)
        H = H.contiguous().float()

        def run(c0, c1, g0, g1):   # clouds [c0, c1), poses [g0, g1) of each
            hh = H.view(bc, g, 4, 4)[c0:c1, g0:g1].reshape(-1, 4, 4)
            x = grasp_scene(pc[c0:c1], hh, gripper_points, None if mean is None else mean[c0:c1], pc_shift, pc_scale)
            lo, pr = self._scores(x)
            out.view(bc, g)[c0:c1, g0:g1] = pr.view(c1 - c0, g1 - g0)
            logits.view(bc, g)[c0:c1, g0:g1] = lo.view(c1 - c0, g1 - g0)

        if per_chunk >= g:
            step = per_chunk // g
            for c0 in range(0, bc, step):
                run(c0, min(bc, c0 + step), 0, g)
        else:
            for c0 in range(bc):
                for g0 in range(0, g, per_chunk):
                    run(c0, c0 + 1, g0, min(g, g0 + per_chunk))
        return (out.view(bc, g), logits.view(bc, g)) if return_logits else out.view(bc, g)


def _check_finite(t, what):
    if not bool(torch.isfinite(t).all()):
        raise GldmError(f"{what} holds non-finite values")
