"""The Panda parallel-jaw gripper as data: the key points of grasp_ldm/utils/gripper.py:18-31 (SimplePandaGripper, origin at
the top of the wrist, fingers along +z) and control points spread over the four segments of the open gripper.  The
reference trains its classifier on a file of 76 such points that is not part of its tree (`gripper_points_76.npy`), so
every entry point that takes gripper points accepts any [Ng, 3] tensor; `control_points` is the default."""
import torch

TOP = (0.0, 0.0, 0.0)
CENTER = (0.0, 0.0, 0.0659999996)
CENTER_RIGHT = (-4.1e-02, 0.0, 6.59999996e-02)
CENTER_LEFT = (4.1e-02, 0.0, 6.59999996e-02)
BOTTOM_RIGHT = (-4.1e-02, 0.0, 1.12169998e-01)
BOTTOM_LEFT = (4.1e-02, 0.0, 1.12169998e-01)
BOTTOM_CENTER = (0.0, 0.0, 1.12169998e-01)

# left finger, right finger, wrist, palm
OPEN_SEGMENTS = ((CENTER_LEFT, BOTTOM_LEFT), (CENTER_RIGHT, BOTTOM_RIGHT), (TOP, CENTER), (CENTER_RIGHT, CENTER_LEFT))

# the "finger sweep" segments between the finger tips (gripper.py:33-47, COLLISION_SEGMENTS): what lies within
# SWEEP_RADIUS of them is between the fingers (create_grasp_collision_marker, :80-103: tubes of radius 0.006 m "for checking
# collisions in the grasp area"; create_grasp_body_marker :105-128 wraps OPEN_SEGMENTS in the same tubes)
SWEEP_SEGMENTS = (((4.1e-02, -7.27595772e-12, 1.08169998e-01), (-4.1e-02, -7.27595772e-12, 1.08169998e-01)),
                  ((4.1e-02, -7.27595772e-12, 0.98169998e-01), (-4.1e-02, -7.27595772e-12, 0.98169998e-01)))
SWEEP_RADIUS = 0.006
BODY_RADIUS = 0.006

DEFAULT_POINTS = 64   # 1024 cloud points + 64 = 1088 = 34 x 32: the merged scene stays on the 32-point-tile launches


def segment_counts(n):
    """Points per segment: in proportion to the segment lengths (largest remainders first, ties by segment order), at
    least one each when n >= 4."""
    seg = torch.tensor(OPEN_SEGMENTS, dtype=torch.float64)
    length = (seg[:, 1] - seg[:, 0]).norm(dim=1)
    base = [1] * 4 if n >= 4 else [0] * 4
    rest = n - sum(base)
    share = length / length.sum() * rest
    counts = [b + int(s) for b, s in zip(base, share.tolist())]
    order = sorted(range(4), key=lambda i: (-(share[i].item() - int(share[i].item())), i))
    for i in order[: n - sum(counts)]:
        counts[i] += 1
    return counts


def control_points(n=DEFAULT_POINTS, dtype=torch.float32, device=None):
    """[n, 3] points on the open gripper: every segment carries its share of n at the midpoints of equal sub-intervals
    (no point is shared by two segments), segment after segment in OPEN_SEGMENTS order."""
    if n < 1:
        raise ValueError("control_points needs n >= 1")
    seg = torch.tensor(OPEN_SEGMENTS, dtype=torch.float64)
    pts = []
    for (a, b), k in zip(seg, segment_counts(n)):
        if k:
            t = ((torch.arange(k, dtype=torch.float64) + 0.5) / k).unsqueeze(1)
            pts.append(a + t * (b - a))
    return torch.cat(pts).to(dtype=dtype, device=device)
