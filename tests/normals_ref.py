"""Restatements of the definitions of csrc/normals.hip and of gldm_grasp_contact_normals (include/gldm.h, "surface normals",
"grasp selection"), point by point and without any of the kernels' shortcuts (no chunks, no boxes, no sorted registers, no
Jacobi).  A helper for test_normals_cpu.py / test_normals_gpu.py, like grasp_select_ref.py.

  knn_radius            the search in f32 numpy, in the header's operation order, ordered by lexsort on (d2, index)
  normals_f64           f32 diffs, f64 scatter matrix, numpy.linalg.eigh, orientation; also the eigenvalues and the dots the
                        preconditions of the tests are taken on
  normals_reference_f32 the reference's own formula (pointcloud_helpers.py:99-122) in its f32: diffs^T diffs / k^2,
                        numpy.linalg.eig, the column of the smallest eigenvalue, flipped where dot(normal, point) >= 0
  contact_normals       grasp_select_ref.clearance's contact set in f64, split by finger and judged by the friction cone,
                        with the margins
  half_sphere / patch   the clouds the issue names
"""
import numpy as np
import torch

import grasp_select_ref as gsref


def knn_radius(pc, k, max_radius, rows=512):
    """pc [n,3] -> (idx int32 [n,k], d2 f32 [n,k], found int32 [n]): gldm_knn_radius's definition for one cloud."""
    pc = np.ascontiguousarray(np.asarray(pc, dtype=np.float32))
    n = pc.shape[0]
    r2 = np.float32(max_radius) * np.float32(max_radius)
    idx = np.full((n, k), n, dtype=np.int32)
    d2o = np.full((n, k), np.inf, dtype=np.float32)
    found = np.zeros(n, dtype=np.int32)
    col = np.arange(n)
    for r0 in range(0, n, rows):
        q = pc[r0:r0 + rows]
        d = pc[None, :, :] - q[:, None, :]                                   # f32, differences first
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]   # one f32 rounding per operation
        assert d2.dtype == np.float32
        inside = d2 <= r2
        key = np.where(inside, d2, np.float32(np.inf))
        order = np.lexsort((np.broadcast_to(col, key.shape), key), axis=-1)[:, :k]     # (d2, index) ascending
        cnt = np.minimum(inside.sum(-1), k)
        live = np.arange(order.shape[1])[None, :] < cnt[:, None]
        kk = order.shape[1]
        idx[r0:r0 + rows, :kk] = np.where(live, order, n)
        d2o[r0:r0 + rows, :kk] = np.where(live, np.take_along_axis(d2, order, axis=-1), np.float32(np.inf))
        found[r0:r0 + rows] = cnt
    return idx, d2o, found


def knn_radius_batch(pc, k, max_radius):
    out = [knn_radius(c, k, max_radius) for c in np.asarray(pc, dtype=np.float32)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _diffs(pc, idx):
    pc = np.asarray(pc, dtype=np.float32)
    n = pc.shape[0]
    own = np.arange(n)[:, None]
    src = np.where((idx >= 0) & (idx < n), idx, own)         # a missing slot counts as the point itself
    return pc[src] - pc[:, None, :]                           # f32


def normals_f64(pc, idx, view=None):
    """-> (normals f64 [n,3], eigenvalues f64 [n,3] ascending, dot f64 [n], live int [n]).  dot = normal . (p - view)
    BEFORE the flip, of the eigh eigenvector; normals are flipped where dot >= 0; live < 3 gives the zero vector."""
    pc = np.asarray(pc, dtype=np.float32)
    n = pc.shape[0]
    diffs = _diffs(pc, idx).astype(np.float64)
    cov = np.einsum("nki,nkj->nij", diffs, diffs)
    w, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0].copy()
    view = np.zeros(3, dtype=np.float32) if view is None else np.asarray(view, dtype=np.float32)
    rel = (pc - view[None, :]).astype(np.float64)             # f32 difference, as the kernel forms it
    dot = (nrm * rel).sum(-1)
    nrm[dot >= 0] *= -1.0
    live = ((idx >= 0) & (idx < n)).sum(-1)
    nrm[live < 3] = 0.0
    return nrm, w, dot, live


def normals_reference_f32(pc, idx):
    """The reference's formula in its own precision (f32 throughout, numpy.linalg.eig)."""
    pc = np.asarray(pc, dtype=np.float32)
    e = _diffs(pc, idx)                                                   # [n, k, 3] f32
    k = np.float32(e.shape[1])
    scatter = np.einsum("nsi,nsj->nij", e, e) / (k * k)                   # sum_s e_s e_s^T / k^2, f32
    assert scatter.dtype == np.float32
    lam, vec = np.linalg.eig(scatter)
    lam, vec = lam.real, vec.real
    smallest = np.argmin(lam, axis=1)
    normal = np.take_along_axis(vec, smallest[:, None, None], axis=2)[:, :, 0]
    facing_away = np.einsum("ni,ni->n", normal, pc) >= 0
    return np.where(facing_away[:, None], -normal, normal)


def gap_ratio(w):
    """(lambda_mid - lambda_min) / lambda_max of ascending eigenvalues [n,3]; 0 where lambda_max is 0."""
    top = np.where(w[:, 2] > 0, w[:, 2], 1.0)
    return np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / top, 0.0)


def contact_normals(scene, normals, H, sweep, r_sweep, cos_friction):
    """scene, normals [B,Ns,3], H [B,G,4,4] -> dict: side, aligned int64 [B,G,2]; hit bool [B,G,Ns]; sweep_d (distance to
    the nearest sweep segment), axis_dot (|normal . closing axis|), qx: f64 [B,G,Ns] -- what the margins are taken on."""
    q = gsref.gripper_frame(scene, H)
    sweep = torch.as_tensor(sweep, dtype=torch.float64).reshape(-1, 2, 3)
    sweep_d2 = gsref.segment_distance2(q, sweep).min(-1).values
    hit = sweep_d2 <= float(r_sweep) ** 2
    left = q[..., 0] > 0
    axis = H.double()[:, :, :3, 0]
    axis_dot = torch.einsum("bgc,bnc->bgn", axis, normals.double()).abs()
    nonzero = (normals != 0).any(-1)[:, None, :]
    cone = (axis_dot >= float(cos_friction)) & nonzero
    side = torch.stack([(hit & left).sum(-1), (hit & ~left).sum(-1)], dim=-1)
    aligned = torch.stack([(hit & left & cone).sum(-1), (hit & ~left & cone).sum(-1)], dim=-1)
    return dict(side=side, aligned=aligned, hit=hit, sweep_d=sweep_d2.sqrt(), axis_dot=axis_dot, qx=q[..., 0],
                nonzero=nonzero.expand_as(hit))


def half_sphere(n, seed=0, radius=0.08, distance=0.6, bump=0.002):
    """A bumpy half-sphere facing the origin: n points, f32 [n,3]."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    ct = u                                                    # uniform on the half with z towards the camera
    st = np.sqrt(1.0 - ct * ct)
    r = radius + bump * np.sin(9.0 * phi) * np.sin(7.0 * np.arccos(ct))
    p = np.stack([r * st * np.cos(phi), r * st * np.sin(phi), distance - r * ct], axis=1)
    return p.astype(np.float32)


def organised_patch(h=48, w=64, pitch=0.001, z=0.6, bump_radius=0.02, seed=0):
    """A plane at z with a spherical bump in pixel order (row-major), pitch metres between pixels, a little jitter so that
    no two distances tie: f32 [h*w, 3]."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x = (u - w / 2) * pitch + rng.uniform(-0.1, 0.1, u.shape) * pitch
    y = (v - h / 2) * pitch + rng.uniform(-0.1, 0.1, u.shape) * pitch
    rr = x * x + y * y
    zz = z - np.sqrt(np.maximum(bump_radius ** 2 - rr, 0.0)) + rng.uniform(-0.02, 0.02, u.shape) * pitch
    return np.stack([x, y, zz], axis=-1).reshape(-1, 3).astype(np.float32)


def kth_tie_free(pc, k, max_radius):
    """f64 precondition of the broad-phase test: for every point, the k-th and (k+1)-th smallest distances among those
    within the radius differ (no tie at any k-th distance) -> the number of points where they do not."""
    pc = np.asarray(pc, dtype=np.float32).astype(np.float64)
    d = pc[None] - pc[:, None]
    d2 = (d * d).sum(-1)
    d2 = np.where(d2 <= float(max_radius) ** 2 * (1 + 1e-6), d2, np.inf)
    s = np.sort(d2, axis=-1)
    if s.shape[1] <= k:
        return 0
    a, b = s[:, k - 1], s[:, k]
    return int((np.isfinite(b) & (a == b)).sum())
