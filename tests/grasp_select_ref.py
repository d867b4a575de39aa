"""f64 restatements of the two definitions of csrc/grasp_select.hip (include/gldm.h, "grasp selection"), point by point and
without any of the kernel's shortcuts (no broad phase, no closed form, no reduction tree).  A helper for
test_grasp_select_cpu.py / test_grasp_select_gpu.py, like unet1d_ref.py."""
import torch


def segment_distance2(q, seg):
    """q [..., 3] f64, seg [S, 2, 3] f64 -> squared distance of every q to every segment [..., S]."""
    a, b = seg[:, 0], seg[:, 1]
    ab = b - a
    len2 = (ab * ab).sum(-1)
    qa = q.unsqueeze(-2) - a
    u = ((qa * ab).sum(-1) / torch.where(len2 > 0, len2, torch.ones_like(len2))).clamp(0.0, 1.0)
    u = torch.where(len2 > 0, u, torch.zeros_like(u))
    w = qa - u.unsqueeze(-1) * ab
    return (w * w).sum(-1)


def gripper_frame(scene, H):
    """scene [B, Ns, 3], H [B, G, 4, 4] -> q [B, G, Ns, 3] = R^T (p - t) in f64."""
    scene, H = scene.double(), H.double()
    v = scene[:, None, :, :] - H[:, :, None, :3, 3]
    return torch.einsum("bgji,bgnj->bgni", H[:, :, :3, :3], v)


def clearance(scene, H, body, sweep, r_sweep, cap):
    """-> (clearance [B, G] f64, contacts [B, G] int64, body_d [B, G, Ns] f64, sweep_d [B, G, Ns] f64 or None): the
    last two are every point's distance to the nearest body / sweep segment (what the margins of a test are taken on)."""
    q = gripper_frame(scene, H)
    body_d = segment_distance2(q, torch.as_tensor(body, dtype=torch.float64)).min(-1).values.sqrt()
    clear = body_d.min(-1).values.clamp(max=float(cap))
    sweep = torch.as_tensor(sweep, dtype=torch.float64).reshape(-1, 2, 3)
    if sweep.shape[0] == 0:
        return clear, torch.zeros(clear.shape, dtype=torch.int64), body_d, None
    sweep_d2 = segment_distance2(q, sweep).min(-1).values
    contacts = (sweep_d2 <= float(r_sweep) ** 2).sum(-1)
    return clear, contacts, body_d, sweep_d2.sqrt()


def pose_distance(H, ctrl):
    """H [G, 4, 4], ctrl [Np, 3] -> D [G, G] f64: mean squared distance of the control points placed at two poses
    (grasp_ldm/losses/loss.py:77-127), point by point."""
    pts = placed_points(H, ctrl)
    d = pts[:, None] - pts[None, :]
    return (d * d).sum(-1).mean(-1)


def placed_points(H, ctrl):
    """H [G, 4, 4], ctrl [Np, 3] -> the control points placed at every pose [G, Np, 3] f64."""
    H, ctrl = H.double(), torch.as_tensor(ctrl).double()
    return torch.einsum("gij,nj->gni", H[:, :3, :3], ctrl) + H[:, None, :3, 3]


def pose_distance_row(pts, i):
    """Row i of pose_distance from placed_points' output [G] f64: the same definition, point by point, without the G x G x
    Np x 3 tensor (6 GB at 2048 poses and 64 control points)."""
    d = pts[i][None] - pts
    return (d * d).sum(-1).mean(-1)


def topk(score, keep, k):
    """One cloud: -> (index list padded with -1 to k, count): kept candidates by (score falling, index rising)."""
    order = sorted((j for j in range(len(score)) if keep[j]), key=lambda j: (-float(score[j]), j))[:k]
    return order + [-1] * (k - len(order)), len(order)


def diverse(H, score, keep, ctrl, k, min_separation=0.0):
    """One cloud, the greedy of gldm_select_grasps mode 1 in f64 -> (index padded with -1, count, gap list padded with 0,
    margins): margins[r] = (best - second best) / best of the m values at pick r >= 1 (inf when there is no second)."""
    pts = placed_points(H, ctrl)
    g = H.shape[0]
    alive = [bool(keep[j]) for j in range(g)]
    picks, gaps, margins = [], [], []
    if any(alive):
        first = max((j for j in range(g) if alive[j]), key=lambda j: (float(score[j]), -j))
        picks.append(first)
        gaps.append(float("inf"))
        alive[first] = False
        m = pose_distance_row(pts, first)
        while len(picks) < k and any(alive):
            cand = [j for j in range(g) if alive[j]]
            best = max(cand, key=lambda j: (float(m[j]), -j))
            if float(m[best]) < float(min_separation) ** 2:
                break
            rest = [float(m[j]) for j in cand if j != best]
            margins.append((float(m[best]) - max(rest)) / float(m[best]) if rest and float(m[best]) > 0 else float("inf"))
            picks.append(best)
            gaps.append(float(m[best]) ** 0.5)
            alive[best] = False
            m = torch.minimum(m, pose_distance_row(pts, best))
    n = len(picks)
    return picks + [-1] * (k - n), n, gaps + [0.0] * (k - n), margins
