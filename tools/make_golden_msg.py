"""Capture the golden vectors of multi-scale set abstraction from the reference's own Python.  CONTAINER-ONLY (needs the
reference checkout, like tools/make_golden_voxel_attention.py whose shims and weight recipe it shares); run from the repo
root after `python __graft_entry__.py` (the oracle's C library serves the reference's point operators):

    python tools/make_golden_msg.py

  schema_pointnet2_msg.json  state-dict key -> (shape, dtype) of the reference's PointNet2(sa_blocks=PointNet2MSG.sa_blocks,
                             fp_blocks=PointNet2MSG.fp_blocks, with_one_hot_shape_id=True, num_shapes=4) (PointNet2MSG
                             itself cannot be constructed there: pointnet2.py:142-159)
  sa_msg.npz                 sa1 = PointNetSAModule(64, [0.2, 0.4], [32, 128], in_channels=5, out_channels=[(32, 32, 64),
                             (64, 96, 128)]) (recipe weights, seed 11) on 2 clouds x 256 points and sa2 =
                             PointNetSAModule(16, [0.8], [128], 192, [(128, 196, 256)]) (seed 12) fed by its output:
                             f1, c1, f2, c2 (features and centres), d1, d2, clouds
  pointnet2_msg.npz          the PointNet2 of the schema (recipe weights, seed 13) on 2 clouds x 1024 points, 3 extra
                             feature channels and one-hot rows: out = every 8th point of the [2, 128, 1024] output, d,
                             clouds

Inputs are not stored: `clouds` holds the indices of the synthetic clouds (scaled by 0.05 / 0.12 to about unit size so that
the radii bite), the feature channels come from torch.Generator seed 53 (sa_msg) / 59 (pointnet2_msg), and cloud b carries
shape id b % 4.  tests/test_msg_gpu.py draws the same.

d = max |f32 - f64|: the reference module against a .double() copy of it on the same inputs, with the index decisions (FPS,
ball query, 3-NN) of the f32 coordinates -- two f32 chains of this length with different summation orders may differ by a
few d.

Boundary flips: a comparison that leaves no element out needs inputs on which the ball queries of two f32
implementations cannot disagree.  For every (centre, point, radius) of every stage of both fixtures the script asserts
|d^2 - r^2| > 1e-5 r^2 (f64, from the f32 coordinates); starting from clouds 0 and 1 it takes the next indices until two
clouds pass, and stores them.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graspldm_amd import synthetic  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle.cpu_backend import _backend as cpu  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCALE = 0.05 / 0.12
MARGIN = 1e-5
SA_POINTS, SA_FEATURE_SEED, SA_CHANNELS = 256, 53, 5
NET_POINTS, NET_FEATURE_SEED, NUM_SHAPES = 1024, 59, 4
SA1 = dict(num_centers=64, radius=[0.2, 0.4], num_neighbors=[32, 128], in_channels=SA_CHANNELS,
           out_channels=[(32, 32, 64), (64, 96, 128)])
SA2 = dict(num_centers=16, radius=[0.8], num_neighbors=[128], in_channels=192, out_channels=[(128, 196, 256)])


def _save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrays.items()})
    print(f"  {name:32s} {os.path.getsize(path) / 1024:8.1f} KiB")


def cloud(index, n_points):
    """[3, n] f32: synthetic cloud `index`, normalised and scaled to about unit size."""
    pc, _ = synthetic.normalize_cloud(synthetic.synthetic_cloud(index, n_points))
    return (pc.t() * SCALE).contiguous()


def sa_inputs(clouds):
    """(features [2, 5, 256], coords [2, 3, 256]) of sa_msg.npz."""
    feats = torch.randn(len(clouds), SA_CHANNELS, SA_POINTS, generator=torch.Generator().manual_seed(SA_FEATURE_SEED))
    return feats, torch.stack([cloud(i, SA_POINTS) for i in clouds])


def net_inputs(clouds):
    """[2, 3 + 3 + 4, 1024] of pointnet2_msg.npz: coordinates, 3 feature channels, one-hot shape id b % 4."""
    extra = torch.randn(len(clouds), 3, NET_POINTS, generator=torch.Generator().manual_seed(NET_FEATURE_SEED))
    onehot = torch.zeros(len(clouds), NUM_SHAPES, NET_POINTS)
    for b in range(len(clouds)):
        onehot[b, b % NUM_SHAPES] = 1.0
    return torch.cat([torch.stack([cloud(i, NET_POINTS) for i in clouds]), extra, onehot], dim=1)


# ------------------------------------------------------------------------------------------------ boundary margins
def stage_margin(points, stages):
    """min over the stages [(num_centers, radii)] of |d^2 - r^2| / r^2, every stage's centres sampled (FPS) from the
    previous stage's; points [1, 3, n] f32, distances in f64."""
    worst = float("inf")
    for num_centers, radii in stages:
        idx = cpu.furthest_point_sampling(points.contiguous(), num_centers)
        centers = cpu.gather_features_forward(points.contiguous(), idx)
        d2 = ((centers.double()[:, :, :, None] - points.double()[:, :, None, :]) ** 2).sum(dim=1)
        for r in radii:
            r2 = float(r) ** 2
            worst = min(worst, float(((d2 - r2).abs() / r2).min()))
        points = centers
    return worst


def settle(n_points, stages, count=2, limit=20000):
    """The first `count` synthetic cloud indices (from 0 upwards) on which no (centre, point, radius) sits in the margin."""
    found = []
    for index in range(limit):
        if stage_margin(cloud(index, n_points)[None], stages) > MARGIN:
            found.append(index)
            if len(found) == count:
                return found
    raise RuntimeError("no clouds outside the boundary margin")


def assert_margin(coords, stages):
    for b in range(coords.shape[0]):
        m = stage_margin(coords[b:b + 1], stages)
        assert m > MARGIN, f"cloud {b}: a point sits {m:.2e} r^2 from a ball's surface"


# ------------------------------------------------------------------------------------- the .double() copy's operators
class _AnyPrecisionBackend:
    """The oracle's point operators for f32 tensors; for the f64 copy of a module the same INDEX decisions (taken on the
    f32 coordinates, which the f64 copy holds exactly) with the values gathered / interpolated in f64."""

    @staticmethod
    def furthest_point_sampling(coords, num_samples):
        return cpu.furthest_point_sampling(coords.float().contiguous(), num_samples)

    @staticmethod
    def ball_query(centers_coords, points_coords, radius, num_neighbors):
        return cpu.ball_query(centers_coords.float().contiguous(), points_coords.float().contiguous(), radius, num_neighbors)

    @staticmethod
    def gather_features_forward(features, indices):
        if features.dtype == torch.float32:
            return cpu.gather_features_forward(features, indices)
        return torch.gather(features, 2, indices.long()[:, None, :].expand(-1, features.shape[1], -1))

    @staticmethod
    def grouping_forward(features, indices):
        if features.dtype == torch.float32:
            return cpu.grouping_forward(features, indices)
        b, m, u = indices.shape
        flat = indices.long().reshape(b, 1, m * u).expand(-1, features.shape[1], -1)
        return torch.gather(features, 2, flat).reshape(b, features.shape[1], m, u)

    @staticmethod
    def three_nearest_neighbors_interpolate_forward(points_coords, centers_coords, centers_features):
        if centers_features.dtype == torch.float32:
            return cpu.three_nearest_neighbors_interpolate_forward(points_coords, centers_coords, centers_features)
        _, idx, wgt = cpu.three_nearest_neighbors_interpolate_forward(
            points_coords.float().contiguous(), centers_coords.float().contiguous(), centers_features.float().contiguous())
        b, c, _ = centers_features.shape
        n = idx.shape[2]
        out = torch.zeros(b, c, n, dtype=torch.float64)
        for k in range(3):
            out += torch.gather(centers_features, 2, idx[:, k].long()[:, None, :].expand(-1, c, -1)) * wgt[:, k].double()[:, None, :]
        return [out, idx, wgt]


def install_any_precision_backend():
    import grasp_ldm.models.modules.ext.pvcnn.modules.functional as F
    for name in ("ball_query", "grouping", "sampling", "interpolatation"):
        sys.modules[F.__name__ + "." + name]._backend = _AnyPrecisionBackend


def _schema(name, module):
    with open(os.path.join(OUT, name), "w") as f:
        json.dump({k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()}, f, indent=0)


# ---------------------------------------------------------------------------------------------------------- fixtures
@torch.no_grad()
def sa_golden():
    from grasp_ldm.models.modules.ext.pvcnn.modules.pointnet import PointNetSAModule
    stages = [(SA1["num_centers"], SA1["radius"]), (SA2["num_centers"], SA2["radius"])]
    clouds = settle(SA_POINTS, stages)
    feats, coords = sa_inputs(clouds)
    assert_margin(coords, stages)
    sa1 = synthetic.load_synthetic_weights(PointNetSAModule(**SA1), seed=11).eval()
    sa2 = synthetic.load_synthetic_weights(PointNetSAModule(**SA2), seed=12).eval()
    f1, c1 = sa1((feats, coords))
    f2, c2 = sa2((f1, c1))
    g1, h1 = copy.deepcopy(sa1).double()((feats.double(), coords.double()))
    g2, h2 = copy.deepcopy(sa2).double()((f1.double(), c1.double()))      # the stage alone: fed the f32 stage-1 output
    assert torch.equal(h1.float(), c1) and torch.equal(h2.float(), c2)
    d1, d2 = float((f1.double() - g1).abs().max()), float((f2.double() - g2).abs().max())
    print(f"  SA modules on clouds {clouds}: d1 = {d1:.3e} (max |f1| {float(f1.abs().max()):.2f}), "
          f"d2 = {d2:.3e} (max |f2| {float(f2.abs().max()):.2f})")
    _save("sa_msg.npz", f1=f1, c1=c1, f2=f2, c2=c2, d1=d1, d2=d2, clouds=np.asarray(clouds, dtype=np.int64))


@torch.no_grad()
def net_golden():
    from grasp_ldm.models.modules.ext.pvcnn.pointnet2 import PointNet2, PointNet2MSG
    net = PointNet2(sa_blocks=PointNet2MSG.sa_blocks, fp_blocks=PointNet2MSG.fp_blocks, with_one_hot_shape_id=True,
                    num_shapes=NUM_SHAPES)
    synthetic.load_synthetic_weights(net, seed=13)
    net.eval()
    _schema("schema_pointnet2_msg.json", net)
    stages = [(c, r) for _, (c, r, _, _) in PointNet2MSG.sa_blocks if c is not None]
    clouds = settle(NET_POINTS, stages)
    x = net_inputs(clouds)
    assert_margin(x[:, :3].contiguous(), stages)
    out = net(x)
    d = float((out.double() - copy.deepcopy(net).double()(x.double())).abs().max())
    print(f"  PointNet2 (MSG tables) on clouds {clouds}: out {tuple(out.shape)}, max |out| {float(out.abs().max()):.2f}, d = {d:.3e}")
    _save("pointnet2_msg.npz", out=out[:, :, ::8], d=d, clouds=np.asarray(clouds, dtype=np.int64))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref_import.install_shims()
    import grasp_ldm.models.modules.ext.pvcnn.modules.pointnet  # noqa: E402,F401  (binds the functional modules)
    install_any_precision_backend()
    sa_golden()
    net_golden()
