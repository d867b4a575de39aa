"""TEST INFRASTRUCTURE: a labelled depth frame restated with tests/depth_ref.py, nothing more than
`deproject(mask=(labels == k) & mask)` for k = 1 .. K, concatenated in ascending label, plus starts and counts -- the
contract of gldm_depth_to_objects (include/gldm.h)."""
import torch

from depth_ref import deproject


def deproject_objects(depth, K, labels, num_labels, mask=None, **kw):
    """depth, labels [H, W] -> (points [n, 3] f32, pixel [n] int32, start [num_labels], count [num_labels])."""
    labels = torch.as_tensor(labels)
    pts, pix, start, count = [], [], [], []
    total = 0
    for k in range(1, num_labels + 1):
        m = labels == k
        if mask is not None:
            m = m & (torch.as_tensor(mask) != 0)
        p, i = deproject(depth, K, mask=m, **kw)
        pts.append(p)
        pix.append(i)
        start.append(total)
        count.append(p.shape[0])
        total += p.shape[0]
    return torch.cat(pts).contiguous(), torch.cat(pix), start, count
