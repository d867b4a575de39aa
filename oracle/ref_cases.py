"""The point-op cases on which the reference's own kernels (oracle/ref_backend.py)
are compared with the C oracle and the HIP kernels.  TEST INFRASTRUCTURE.

One list for tests/test_ref_kernels_gpu.py (all of it), for
oracle/record_ref_point_ops.py (the `record` subset, run on the GPU) and for the
CPU replay in tests/test_oracle_point_ops.py.  A case is (op, params): `params`
holds only shapes, seeds and cloud kinds, and make_inputs() regenerates every
input from it on the CPU with torch's seeded CPU generator, so a recorded output
needs no recorded input beside it.
"""
import torch

OPS = ("fps", "ball_query", "grouping", "three_nn", "voxelize", "devoxelize")


def cloud(b, n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(b, 3, n, generator=g) * 2 - 1) * scale).contiguous()


def surface_cloud(b, n):
    from graspldm_amd.synthetic import synthetic_batch
    pcs, _ = synthetic_batch(b, n)
    return pcs.transpose(1, 2).contiguous()


def tie_cloud(kind, n):
    """The clouds of tests/test_point_ops_gpu._tie_cloud: FPS rounds that end in exact maximal-distance ties."""
    if kind == "dup":
        base = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [.5, .5, 1]])
    elif kind == "sym":
        cube = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)])
        octa = torch.tensor([[2., 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]])
        base = torch.cat([cube, octa])
    elif kind == "grid":
        base = torch.tensor([[x, y, z] for x in range(5) for y in range(5) for z in range(5)], dtype=torch.float32)
    else:
        raise ValueError(kind)
    rep = -(-n // base.shape[0])
    return base.repeat(rep, 1)[:n].T.unsqueeze(0).contiguous()   # [1, 3, n]


def lattice_cloud(side=7, spacing=0.25):
    """side^3 lattice points, spacing 0.25, centred on the origin: every coordinate, difference, square and sum of
    squares is a small multiple of 2^-4, exact in f32 with or without fused multiply-adds.  With r = 0.5 each interior
    point has 27 lattice points with d^2 < r^2 and 6 more with d^2 == r^2 exactly."""
    ax = (torch.arange(side, dtype=torch.float32) - (side - 1) / 2) * spacing
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)]).unsqueeze(0).contiguous()


def _case(op, record, **params):
    name = op + "-" + "-".join(f"{k}{v}" for k, v in params.items())
    return {"op": op, "name": name, "record": record, "params": params}


def _build_cases():
    cs = []
    # ---- FPS.  3072 / 3073 / 4096: either side of the reference's 3072-point LDS buffer (sampling.cu:100-133)
    for (b, n, m), rec in (((2, 64, 16), True), ((1, 100, 100), True), ((2, 777, 300), True), ((1, 3072, 24), True),
                           ((1, 3073, 24), True), ((1, 4096, 64), False), ((1, 8192, 32), False)):
        cs.append(_case("fps", rec, kind="rand", b=b, n=n, m=m))
    cs.append(_case("fps", True, kind="surface", b=1, n=1024, m=512))
    for kind in ("dup", "sym", "grid"):
        for n in (64, 100, 512, 1000, 1024):
            cs.append(_case("fps", True, kind=kind, b=1, n=n, m=min(n, 12)))
            cs.append(_case("fps", True, kind=kind, b=2, n=n, m=min(n, 12)))   # [cloud, cloud reversed]
    # ---- ball query: the shapes of test_ball_query_exact, the empty ball, the lattice (strict '<' against r^2)
    for (b, n, m, u, r), rec in (((2, 1024, 512, 64, 0.2), False), ((2, 512, 128, 64, 0.4), True),
                                 ((1, 1024, 1024, 32, 0.1), False), ((3, 100, 10, 8, 0.5), True),
                                 ((1, 257, 33, 16, 0.3), True), ((1, 6000, 40, 32, 0.15), True),
                                 ((2, 64, 64, 4, 0.05), True), ((1, 1024, 16, 128, 2.0), True)):
        cs.append(_case("ball_query", rec, kind="rand", b=b, n=n, m=m, u=u, r=r))
    cs.append(_case("ball_query", True, kind="empty", b=2, n=1024, m=64, u=32, r=0.1))
    cs.append(_case("ball_query", True, kind="lattice", b=1, n=343, m=343, u=32, r=0.5))
    # ---- grouping + gather: the shapes of test_grouping_exact
    for (b, c, n, m, u), rec in (((2, 128, 512, 128, 64), False), ((1, 3, 1024, 512, 64), False),
                                 ((2, 7, 100, 13, 5), True), ((1, 35, 1024, 1024, 32), False)):
        cs.append(_case("grouping", rec, b=b, c=c, n=n, m=m, u=u))
    # ---- 3-NN: the shapes of test_three_nn_interpolate_exact; m = 1, 2: `best` stays 1e40 and clamps to 1e10;
    # 'coincide': the centres are the first m points, d = 0 clamps to 1e-10
    for (b, c, m, n), rec in (((2, 256, 128, 512), False), ((1, 1024, 1, 128), False), ((2, 6, 17, 90), True),
                              ((1, 128, 512, 1024), False), ((1, 3, 1, 40), True), ((2, 4, 2, 50), True)):
        cs.append(_case("three_nn", rec, kind="rand", b=b, c=c, m=m, n=n))
    cs.append(_case("three_nn", True, kind="coincide", b=2, c=5, m=20, n=60))
    # ---- voxelise (r = 2: every point in one voxel) and devoxelise
    for b, c, n, r in ((2, 3, 1024, 24), (1, 5, 200, 4), (2, 4, 64, 2), (1, 3, 100, 5)):
        cs.append(_case("voxelize", True, b=b, c=c, n=n, r=r))
    for (b, c, n, r, train), rec in (((2, 48, 1024, 24, False), False), ((2, 96, 1024, 12, False), False),
                                     ((1, 3, 77, 6, True), True)):
        cs.append(_case("devoxelize", rec, b=b, c=c, n=n, r=r, train=train))
    return cs


CASES = _build_cases()


def make_inputs(op, p):
    """CPU input tensors of one case, from its params alone."""
    if op == "fps":
        if p["kind"] == "rand":
            pts = cloud(p["b"], p["n"], p["n"])
        elif p["kind"] == "surface":
            pts = surface_cloud(p["b"], p["n"])
        else:
            pts = tie_cloud(p["kind"], p["n"])
            if p["b"] == 2:
                pts = torch.cat([pts, pts.flip(2)]).contiguous()
        return {"coords": pts}
    if op == "ball_query":
        b, n, m = p["b"], p["n"], p["m"]
        if p["kind"] == "rand":
            pts = cloud(b, n, 10 + n)
            ctr = pts[:, :, torch.randperm(n, generator=torch.Generator().manual_seed(1))[:m]].contiguous()
        elif p["kind"] == "empty":
            pts = surface_cloud(b, n)
            ctr = torch.cat([pts[:, :, :m - 4], torch.full((b, 3, 4), 50.0)], dim=2).contiguous()
        else:
            pts = lattice_cloud()
            ctr = pts.clone()
        return {"centers": ctr, "points": pts}
    if op == "grouping":
        g = torch.Generator().manual_seed(3)
        f = torch.randn(p["b"], p["c"], p["n"], generator=g)
        idx = torch.randint(0, p["n"], (p["b"], p["m"], p["u"]), generator=g, dtype=torch.int32)
        return {"features": f, "indices": idx}
    if op == "three_nn":
        b, c, m, n = p["b"], p["c"], p["m"], p["n"]
        pts = cloud(b, n, 4)
        ctr = cloud(b, m, 5) if p["kind"] == "rand" else pts[:, :, :m].contiguous()
        feat = torch.randn(b, c, m, generator=torch.Generator().manual_seed(6))
        return {"points": pts, "centers": ctr, "features": feat}
    if op == "voxelize":
        g = torch.Generator().manual_seed(8)
        feat = torch.randn(p["b"], p["c"], p["n"], generator=g)
        vc = torch.randint(0, p["r"], (p["b"], 3, p["n"]), generator=g, dtype=torch.int32)
        if p["r"] == 2:
            vc[:] = 1
        return {"features": feat, "coords": vc}
    if op == "devoxelize":
        g = torch.Generator().manual_seed(9)
        r = p["r"]
        grid = torch.randn(p["b"], p["c"], r ** 3, generator=g)
        coords = torch.rand(p["b"], 3, p["n"], generator=g) * (r - 1)
        coords[:, :, 0] = r - 1
        coords[:, :, 1] = 0
        return {"coords": coords.contiguous(), "grid": grid}
    raise ValueError(op)


def run(backend, op, p, x):
    """Run one case on `backend` (any object with the reference pybind module's forward names) on the tensors `x`
    (already on the backend's device).  Returns {output name: tensor}."""
    if op == "fps":
        return {"indices": backend.furthest_point_sampling(x["coords"], p["m"])}
    if op == "ball_query":
        return {"indices": backend.ball_query(x["centers"], x["points"], p["r"], p["u"])}
    if op == "grouping":
        first = x["indices"][:, :, 0].contiguous()
        return {"grouped": backend.grouping_forward(x["features"], x["indices"]),
                "gathered": backend.gather_features_forward(x["features"], first)}
    if op == "three_nn":
        o, i, w = backend.three_nearest_neighbors_interpolate_forward(x["points"], x["centers"], x["features"])
        return {"out": o, "indices": i, "weights": w}
    if op == "voxelize":
        o, i, k = backend.avg_voxelize_forward(x["features"], x["coords"], p["r"])
        return {"out": o, "ind": i, "cnt": k}
    if op == "devoxelize":
        o, i, w = backend.trilinear_devoxelize_forward(p["r"], p["train"], x["coords"], x["grid"])
        return {"out": o, "inds": i, "wgts": w}
    raise ValueError(op)


# outputs a fixture does not keep: the float-atomic sum has no fixed order in the reference (vox.cu:48-72)
UNRECORDED = {("voxelize", "out")}
