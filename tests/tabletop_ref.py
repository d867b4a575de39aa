"""TEST INFRASTRUCTURE: the three tabletop contracts of include/gldm.h (gldm_plane_ransac, gldm_plane_moments,
gldm_segment_tabletop) restated in numpy, f32, one elementwise op per step in the written order.  Points come from
depth_ref.deproject; components from a plain union-find over the link list; ranking by (-count, root)."""
import numpy as np

from depth_ref import deproject

F = np.float32


def inliers(points, plane, tol):
    """bool [n]: fabsf(((nx*x + ny*y) + nz*z) + d) <= tol in f32."""
    p = np.asarray(points, dtype=F)
    a, b, c, d = [F(v) for v in plane]
    with np.errstate(all="ignore"):
        return np.abs(((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d) <= F(tol)


def ransac(points, triples, tol, min_cross2):
    """-> (planes [t, 4] f32, counts [t] int32); degenerate hypotheses: plane 0, count -1."""
    p = np.asarray(points, dtype=F)
    tri = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    n, t = p.shape[0], tri.shape[0]
    planes = np.zeros((t, 4), dtype=F)
    counts = np.full(t, -1, dtype=np.int32)
    i, j, k = tri[:, 0], tri[:, 1], tri[:, 2]
    ok = (tri >= 0).all(1) & (tri < n).all(1) & (i != j) & (i != k) & (j != k)
    with np.errstate(all="ignore"):
        for h in np.nonzero(ok)[0]:
            p0, p1, p2 = p[i[h]], p[j[h]], p[k[h]]
            e1, e2 = p1 - p0, p2 - p0
            cx = e1[1] * e2[2] - e1[2] * e2[1]
            cy = e1[2] * e2[0] - e1[0] * e2[2]
            cz = e1[0] * e2[1] - e1[1] * e2[0]
            l2 = (cx * cx + cy * cy) + cz * cz
            if not l2 >= F(min_cross2):
                continue
            ln = np.sqrt(l2)
            nx, ny, nz = cx / ln, cy / ln, cz / ln
            d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
            planes[h] = (nx, ny, nz, d)
            counts[h] = int(inliers(p, planes[h], tol).sum())
    return planes, counts


def moment_terms(points, plane, tol):
    """The ten f64 term columns [m, 10] of the inliers: 1, x, y, z, xx, xy, xz, yy, yz, zz."""
    q = np.asarray(points, dtype=F)[inliers(points, plane, tol)].astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([np.ones_like(x), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)


def moments(points, plane, tol):
    """-> (sums f64 [10], sum of |term| f64 [10])."""
    t = moment_terms(points, plane, tol)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def plane_from_moments(m):
    m = np.asarray(m, dtype=np.float64)
    mean = m[1:4] / m[0]
    sec = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]], dtype=np.float64) / m[0]
    _, vec = np.linalg.eigh(sec - np.outer(mean, mean))
    n = vec[:, 0]
    return n.astype(F), F(-np.dot(n, mean))


def orient(normal, offset, centre=(0.0, 0.0, 0.0)):
    n, o = np.asarray(normal, dtype=F), F(offset)
    hgt = float(np.dot(n.astype(np.float64), np.asarray(centre, dtype=np.float64)) + np.float64(o))
    if hgt == 0.0:
        nz = n[n != 0]
        flip = nz.size > 0 and nz[0] < 0
    else:
        flip = hgt < 0.0
    return (-n, -o) if flip else (n, o)


def fit_plane(points, triples, tol, min_cross2, refit=True, centre=(0.0, 0.0, 0.0)):
    """-> (normal f32 [3], offset f32, inliers, hypothesis): highest count, ties to the lowest index."""
    planes, counts = ransac(points, triples, tol, min_cross2)
    best = int(np.argmax(counts))
    assert counts[best] >= 0
    normal, offset = planes[best, :3], planes[best, 3]
    if refit:
        normal, offset = plane_from_moments(moments(points, planes[best], tol)[0])
    normal, offset = orient(normal, offset, centre)
    return normal, offset, int(counts[best]), best


def foreground(depth, K, plane, h_min, h_max, **opts):
    """-> (fg bool [h, w], xyz f32 [h, w, 3]; rows of background pixels are 0)."""
    h, w = np.asarray(depth).shape
    pts, pix = deproject(depth, K, **opts)
    pts, pix = pts.numpy().astype(F), pix.numpy().astype(np.int64)
    a, b, c, d = [F(v) for v in plane]
    with np.errstate(all="ignore"):
        hgt = ((a * pts[:, 0] + b * pts[:, 1]) + c * pts[:, 2]) + d
        keep = (hgt > F(h_min)) & (hgt <= F(h_max))
    fg = np.zeros(h * w, dtype=bool)
    xyz = np.zeros((h * w, 3), dtype=F)
    fg[pix[keep]] = True
    xyz[pix[keep]] = pts[keep]
    return fg.reshape(h, w), xyz.reshape(h, w, 3)


def _links(fg, xyz, link_dist, axis):
    a = xyz[:, :-1] if axis == 1 else xyz[:-1]
    b = xyz[:, 1:] if axis == 1 else xyz[1:]
    fa = fg[:, :-1] if axis == 1 else fg[:-1]
    fb = fg[:, 1:] if axis == 1 else fg[1:]
    link2 = F(link_dist) * F(link_dist)
    with np.errstate(all="ignore"):
        dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        return fa & fb & (((dx * dx + dy * dy) + dz * dz) <= link2)


def components(fg, right, down):
    """root [h, w] int64: the lowest pixel index of each pixel's component, -1 for background."""
    h, w = fg.shape
    par = list(range(h * w))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    vs, us = np.nonzero(right)
    edges = [(v * w + u, v * w + u + 1) for v, u in zip(vs.tolist(), us.tolist())]
    vs, us = np.nonzero(down)
    edges += [(v * w + u, (v + 1) * w + u) for v, u in zip(vs.tolist(), us.tolist())]
    for p, q in edges:
        a, b = find(p), find(q)
        if a != b:
            par[max(a, b)] = min(a, b)
    root = np.full(h * w, -1, dtype=np.int64)
    for p in np.nonzero(fg.reshape(-1))[0].tolist():
        root[p] = find(p)
    return root.reshape(h, w)


def label_components(root, min_pixels, max_labels):
    """-> (labels int32 [h, w], num, label_pixels int32 [max_labels], label_root int32 [max_labels])."""
    flat = root.reshape(-1)
    roots, cnt = np.unique(flat[flat >= 0], return_counts=True)
    order = sorted((int(-c), int(r)) for r, c in zip(roots, cnt) if c >= min_pixels)[:max_labels]
    labels = np.zeros(flat.shape, dtype=np.int32)
    pixels = np.zeros(max_labels, dtype=np.int32)
    lroot = np.full(max_labels, -1, dtype=np.int32)
    for k, (negc, r) in enumerate(order):
        labels[flat == r] = k + 1
        pixels[k], lroot[k] = -negc, r
    return labels.reshape(root.shape), len(order), pixels, lroot


def segment(depth, K, plane, h_min=0.01, h_max=0.5, link_dist=0.01, min_pixels=32, max_labels=64, **opts):
    fg, xyz = foreground(depth, K, plane, h_min, h_max, **opts)
    root = components(fg, _links(fg, xyz, link_dist, 1), _links(fg, xyz, link_dist, 0))
    return label_components(root, min_pixels, max_labels)
