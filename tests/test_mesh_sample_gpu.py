"""GPU: gldm_mesh_sample_surface against the numpy restatement (tests/mesh_ref.py): exact equality of every output.  Every
call goes through the C ABI TWICE, each time with the outputs poisoned and the workspace filled with other garbage, and the two
results are compared bitwise.  No tolerance: the weights are integers, the scan is an integer scan, and every f32 / f64
operation of the rule rounds once."""
import numpy as np
import pytest
import torch

import mesh_ref as ref
from graspldm_amd import mesh as M
from test_mesh_cpu import batch_args, sliver_mesh

pytestmark = pytest.mark.gpu

POISON = -7
KEYS = ("points", "face", "normals")
SIZES = (1, 63, 64, 65, 1000)


def _garbage(nbytes, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, ((nbytes + 7) // 8 + 2,), generator=g, dtype=torch.int64).cuda()


def _twice(run):
    a, b = run(1), run(2)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), f"two calls differ in {key}"
    return a


def _sample(vertices, faces, vs, vc, fs, fc, n, rand=None, seed=0, f_max=None):
    from graspldm_amd import _lib as L
    lib = L.lib()
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).cuda()
    rg = torch.tensor(np.stack([vs, vc, fs, fc]).astype(np.int32)).cuda()
    b = rg.shape[1]
    f_max = max(max(int(c) for c in fc), 0) if f_max is None else f_max
    sizes = (b, f_max, v.shape[0], f.shape[0], n)
    nbytes = lib.gldm_mesh_sample_surface_workspace_bytes(*sizes)
    assert nbytes == 16 * f.shape[0] + 16 * b
    r = None if rand is None else torch.from_numpy(np.ascontiguousarray(rand, np.float32)).cuda()

    def run(k):
        ws = _garbage(nbytes, k)
        points = torch.full((b, n, 3), float("nan"), dtype=torch.float32).cuda()
        normals = torch.full((b, n, 3), float("nan"), dtype=torch.float32).cuda()
        face = torch.full((b, n), POISON, dtype=torch.int32).cuda()
        L.call("gldm_mesh_sample_surface", L.ptr(v) if v.shape[0] else None, L.ptr(f) if f.shape[0] else None, L.ptr(rg[0]),
               L.ptr(rg[1]), L.ptr(rg[2]), L.ptr(rg[3]), *sizes, L.ptr(r), seed, L.ptr(ws), nbytes, L.ptr(points), L.ptr(face),
               L.ptr(normals), L.current_stream())
        torch.cuda.synchronize()
        return dict(points=points.cpu().numpy(), face=face.cpu().numpy(), normals=normals.cpu().numpy())

    return _twice(run)


def _uniform24(shape, seed):
    return (np.random.default_rng(seed).integers(0, 1 << 24, shape).astype(np.float32) * np.float32(2.0 ** -24))


def _check(arrays, n, rand=None, seed=0, f_max=None):
    got = _sample(*arrays, n, rand=rand, seed=seed, f_max=f_max)
    kw = {} if f_max is None else dict(f_max=f_max)
    exp = ref.sample_surface(*arrays, n, rand=rand, seed=seed, **kw)
    for key in KEYS:
        assert got[key].dtype == exp[key].dtype and got[key].shape == exp[key].shape, key
        assert got[key].tobytes() == exp[key].tobytes(), (key, n)
    return got


def _check_normals(arrays, got):
    """Unit, and orthogonal to the face's edges.  The normal is the f64 cross product divided by its f64 length, each
    component rounded once to f32 (relative error 2^-24): the length is off by at most 2^-24 (1 + o(1)) and n . e by at most
    sqrt(3) 2^-24 |e|, beside an f64 term of the order 2^-50 (|e1| |e2| / 2A) that only slivers far thinner than these
    would make visible.  4 * 2^-24 covers both."""
    vertices, faces, vs = np.asarray(arrays[0], np.float64).reshape(-1, 3), np.asarray(arrays[1]).reshape(-1, 3), arrays[2]
    eps = 4 * 2.0 ** -24
    for j in range(got["face"].shape[0]):
        hit = got["face"][j] >= 0
        if not hit.any():
            assert not got["normals"][j].any()
            continue
        assert hit.all()
        tri = vertices[int(vs[j]) + faces[got["face"][j]]]
        nrm = got["normals"][j].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1) <= eps)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            e = tri[:, b] - tri[:, a]
            assert np.all(np.abs(np.einsum("ij,ij->i", nrm, e)) <= eps * np.linalg.norm(e, axis=1))


def ragged_batch():
    """Three meshes packed with gaps: a sphere, one without faces, and a box one of whose faces has an index outside its
    mesh and one a negative index -- a MeshBatch refuses such a batch, the C entry has to live with it."""
    sphere, cube = M.icosphere(1, 0.2), M.box((0.3, 0.2, 0.1), center=(1, 2, 3))
    vertices = np.full((60, 3), np.nan, np.float32)
    vertices[2:44] = sphere.vertices
    vertices[47:55] = cube.vertices
    faces = np.full((110, 3), 1 << 30, np.int32)
    faces[5:85] = sphere.faces
    faces[90:102] = cube.faces
    faces[93] = (0, 1, 8)      # 8 = vert_count: the first row of the gap behind the box
    faces[97] = (-1, 2, 3)
    return vertices, faces, [2, 44, 47], [42, 3, 8], [5, 85, 90], [80, 0, 12]


MESHES = {
    "triangle": lambda: batch_args(M.MeshBatch([M.Mesh([[0.1, 0.2, 0.3], [1.5, 0.1, 0.4], [0.3, 2.0, -1.0]], [[0, 1, 2]])])),
    "box": lambda: batch_args(M.MeshBatch([M.box((0.07, 0.2, 0.13), center=(0.5, -0.2, 0.9))])),
    "slivers": lambda: batch_args(M.MeshBatch([sliver_mesh()])),
    "ragged": ragged_batch,
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_bitwise_against_the_restatement_with_both_sources_of_uniforms(name):
    arrays = MESHES[name]()
    b = len(arrays[2])
    for n in SIZES:
        got = _check(arrays, n, rand=_uniform24((b, n, 3), seed=n))
        _check_normals(arrays, got)
        got = _check(arrays, n, seed=0x1234_5678_9ABC_DEF0 + n)
        _check_normals(arrays, got)
        if name == "ragged":
            assert np.all(got["face"][1] == -1) and not got["points"][1].any()      # no faces: no area
            assert not np.isin(got["face"][2], (93, 97)).any() and np.all(got["face"][2] >= 90)
            assert np.all((got["face"][0] >= 5) & (got["face"][0] < 85))
            assert np.isfinite(got["points"]).all()                                  # no row of a gap was read
        if name == "slivers" and n == 1000:
            assert not np.isin(got["face"][0], (5, 6)).any() and len(np.unique(got["face"][0])) >= 3


def test_in_kernel_uniforms_are_the_host_philox_stream():
    """The kernel's own draw equals a tensor call fed with Philox4x32-10 from the host (oracle/philox.py, itself held to the
    Random123 known-answer vectors by test_philox_cpu.py): key = seed, counter = (sample, mesh, 0, 0), 24 high bits a word."""
    arrays = ragged_batch()
    n, seed = 257, (0xDEADBEEF << 32) | 0x12345
    own = _sample(*arrays, n, seed=seed)
    rand = np.zeros((3, n, 3), np.float32)
    for j in range(3):
        k0, u1, u2 = ref.uniforms(seed, j, n)
        rand[j] = np.stack([k0.astype(np.float32) * np.float32(2.0 ** -24), u1, u2], axis=1)
    fed = _sample(*arrays, n, rand=rand)
    for key in KEYS:
        assert own[key].tobytes() == fed[key].tobytes(), key
    assert rand.min() >= 0 and rand.max() < 1 and 0.4 < rand.mean() < 0.6


def test_uniforms_outside_the_unit_interval_and_ranges_that_leave_the_arrays():
    arrays = list(MESHES["box"]())
    rand = _uniform24((1, 64, 3), seed=5)
    rand[0, :8] = [[np.nan, 0.5, 0.25], [2.0, 0.1, 0.1], [-1.0, 0.9, 0.9], [1.0, 1.0, 1.0], [0.5, np.inf, 0.0],
                   [0.999999999, 0.3, -np.inf], [0.5, 0.5, 0.5], [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 0.0]]
    got = _check(arrays, 64, rand=rand)
    assert np.isfinite(got["points"]).all() and np.all(got["face"] >= 0)
    # f_max below the face count clamps it; a face range or a vertex range that leaves its array makes the mesh empty
    _check(arrays, 65, seed=3, f_max=5)
    for at, value in ((4, 1), (4, -1), (2, 1), (2, -3), (5, -4)):   # face_start, vert_start, face_count of the one mesh
        bad = [np.array(a).copy() for a in arrays]
        bad[at][0] = value
        got = _check(bad, 64, seed=4)
        assert np.all(got["face"] == -1) and not got["points"].any() and not got["normals"].any()


def test_public_entry_matches_the_c_entry():
    from graspldm_amd.pointcloud import sample_mesh_surface
    mb = M.MeshBatch([M.icosphere(2, 0.1), M.cylinder(0.05, 0.2, 24)])
    exp = ref.sample_surface(*batch_args(mb), 1024, seed=77)
    pts, face, nrm = sample_mesh_surface(mb, 1024, seed=77, return_faces=True, return_normals=True)
    assert pts.is_cuda and pts.cpu().numpy().tobytes() == exp["points"].tobytes()
    assert face.cpu().numpy().tobytes() == exp["face"].tobytes() and nrm.cpu().numpy().tobytes() == exp["normals"].tobytes()
    rand = torch.rand((2, 300, 3), device="cuda")
    pts = sample_mesh_surface(mb, 300, rand=rand)
    assert pts.cpu().numpy().tobytes() == ref.sample_surface(*batch_args(mb), 300, rand=rand.cpu().numpy())["points"].tobytes()
    torch.manual_seed(5)
    a = sample_mesh_surface(mb, 64)
    torch.manual_seed(5)
    assert torch.equal(a, sample_mesh_surface(mb, 64)) and not torch.equal(a, sample_mesh_surface(mb, 64))
    assert sample_mesh_surface(mb, 0, seed=1).shape == (2, 0, 3)
    # area-weighted: the share of the samples on the sphere's faces is the sphere's share of the area, within 5 sigma
    area = [0.5 * np.linalg.norm(np.cross(*(m.vertices[m.faces][:, k].astype(np.float64) - m.vertices[m.faces][:, 0]
                                            for k in (1, 2))), axis=1) for m in (mb.mesh(0), mb.mesh(1))]
    _, face = sample_mesh_surface(M.MeshBatch([M.Mesh(np.concatenate([mb.mesh(0).vertices, mb.mesh(1).vertices]),
                                                      np.concatenate([mb.mesh(0).faces, mb.mesh(1).faces + 162]))]),
                                  20000, seed=9, return_faces=True)
    p = area[0].sum() / (area[0].sum() + area[1].sum())
    share = float((face < 320).float().mean())
    assert abs(share - p) < 5 * np.sqrt(p * (1 - p) / 20000), (share, p)
