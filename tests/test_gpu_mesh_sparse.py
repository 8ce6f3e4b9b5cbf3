"""Brick-sparse marching cubes on the device (csrc/mesh_sparse.hip, vdn_hip/mesh.py: marching_cubes_sparse, the `sparse` keyword of
extract_geometry / validate_mesh) against the dense path of the same process: marching_cubes on
extract_fields_device's lattice. The claim is equality, element for element - torch.equal on the device arrays, array_equal on the
numpy ones, the bytes of the PLY - never a tolerance."""
import numpy as np
import pytest
import torch

from test_mesh_sparse_cpu import HI, LO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


# ---- the fields of test_mesh_sparse_cpu.py as query_funcs: [P,3] device points -> [P] values, each row on its own -------------------
def _norm(p, c=(0.0, 0.0, 0.0)):
    x, y, z = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return torch.sqrt(x * x + y * y + z * z)


def sphere(r, c=(0.0, 0.0, 0.0)):
    return lambda p: _norm(p, c) - r


def torus(p):
    q = torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) - 0.6
    return torch.sqrt(q * q + p[:, 2] * p[:, 2]) - 0.23


def two_spheres(p):
    return torch.minimum(sphere(0.31, (-0.45, 0.1, 0.0))(p), sphere(0.27, (0.4, -0.2, 0.15))(p))


def steep(p):
    return 4.0 * (_norm(p) - 0.537)


def slab(R):
    x16 = float(torch.linspace(LO, HI, R)[16])
    return lambda p: p[:, 0] - x16


def noise(R):
    """white noise on the nodes, looked up by the nearest node (the coarse pass asks between nodes: any value will do there)"""
    u = torch.from_numpy(np.random.default_rng(11).standard_normal((R, R, R)).astype(np.float32)).to(DEV)

    def f(p):
        i = torch.round((p - LO) / (HI - LO) * (R - 1)).long().clamp(0, R - 1)
        return u[i[:, 0], i[:, 1], i[:, 2]]
    return f


def axes(R, lo=(LO,) * 3, hi=(HI,) * 3):
    return [torch.linspace(a, b, R).to(DEV) for a, b in zip(lo, hi)]


def dense(f, R, level=0.0, lo=(LO,) * 3, hi=(HI,) * 3):
    from dpt_models.renderer import extract_fields_device
    from vdn_hip import mesh
    u = extract_fields_device(torch.tensor(lo), torch.tensor(hi), R, f, device=torch.device(DEV))
    return mesh.marching_cubes(u, level)


class Counting:
    def __init__(self, f):
        self.f, self.points, self.largest = f, 0, 0

    def __call__(self, p):
        assert p.is_cuda and p.dim() == 2 and p.shape[1] == 3 and p.dtype == torch.float32
        self.points += p.shape[0]
        self.largest = max(self.largest, p.shape[0])
        return self.f(p)


CASES = {
    "sphere-R37-b8": (sphere(0.537), 37, 0.0, 8, 1.0),
    "torus-R41-b4": (torus, 41, 0.0, 4, 1.0),
    "torus-R41-b8": (torus, 41, 0.0, 8, 1.0),
    "torus-R41-level0.05": (torus, 41, 0.05, 8, 1.0),
    "big_sphere-R37": (sphere(1.3), 37, 0.0, 8, 1.0),
    "slab-R33": (slab(33), 33, 0.0, 8, 1.0),
    "two_spheres-R41": (two_spheres, 41, 0.0, 8, 1.0),
    "sphere-R3": (sphere(0.537), 3, 0.0, 8, 1.0),
    "sphere-R9": (sphere(0.537), 9, 0.0, 8, 1.0),
    "noise-R19-b4-inf": (None, 19, 0.0, 4, float("inf")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sparse_equals_dense_on_analytic_fields(case):
    from vdn_hip import mesh
    f, R, level, brick, L = CASES[case]
    f = f or noise(R)
    V0, F0 = dense(f, R, level)
    q = Counting(f)
    V1, F1, stats = mesh.marching_cubes_sparse(q, *axes(R), threshold=level, brick=brick, lipschitz=L)
    assert F0.shape[0] > 0
    assert V1.dtype == torch.float64 and F1.dtype == torch.int64 and V1.device == V0.device
    assert stats["missed_edges"] == 0 and stats["points_evaluated"] == q.points
    B = min(brick, R - 1)
    nb = -(-(R - 1) // B)
    assert stats["bricks"] == nb ** 3 and q.points == nb ** 3 + stats["active_bricks"] * (B + 1) ** 3
    assert torch.equal(F1, F0)
    assert torch.equal(V1, V0)
    if case == "noise-R19-b4-inf":
        assert stats["active_bricks"] == stats["bricks"]
        cases = set()                                        # all 256 cases went through the sparse indexing
        u = f(torch.stack(torch.meshgrid(*axes(R), indexing="ij"), dim=-1).reshape(-1, 3)).reshape(R, R, R) <= 0.0
        n = R - 1
        code = sum(u[a:a + n, b:b + n, c:c + n].long() << m for m, (a, b, c) in
                   enumerate([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]))
        cases.update(code.unique().tolist())
        assert len(cases) == 256
    elif nb > 2 and case != "big_sphere-R37":
        assert 0 < stats["active_bricks"] < stats["bricks"]


def test_small_chunks_give_the_same_arrays():
    """chunk_points below one brick's block and no divisor of anything: the coarse and the fine pass both go in many pieces"""
    from vdn_hip import mesh
    V0, F0 = dense(torus, 41)
    q = Counting(torus)
    V1, F1, stats = mesh.marching_cubes_sparse(q, *axes(41), brick=8, lipschitz=1.0, chunk_points=613)
    assert q.largest == 613 and q.points == stats["points_evaluated"]
    assert torch.equal(F1, F0) and torch.equal(V1, V0)


def test_anisotropic_box_through_extract_geometry():
    """different extents per axis: the radius is the brick's own diagonal; the world-coordinate arrays are equal too"""
    from dpt_models.renderer import extract_geometry
    from vdn_hip import mesh
    lo, hi, R = (-1.0, -0.7, -0.5), (1.2, 0.8, 0.45), 35
    f = sphere(0.41, (0.1, 0.05, -0.02))
    V0, F0 = dense(f, R, 0.0, lo, hi)
    V1, F1, stats = mesh.marching_cubes_sparse(f, *axes(R, lo, hi), brick=8, lipschitz=1.0)
    assert F0.shape[0] > 0 and 0 < stats["active_bricks"] < stats["bricks"] and stats["missed_edges"] == 0
    assert torch.equal(F1, F0) and torch.equal(V1, V0)
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    v0, t0 = extract_geometry(lo_t, hi_t, R, 0.0, f)
    v1, t1 = extract_geometry(lo_t, hi_t, R, 0.0, f, sparse={"brick": 8, "lipschitz": 1.0})
    v2, t2 = extract_geometry(lo_t, hi_t, R, 0.0, f, sparse=True)
    assert np.array_equal(v0, v1) and np.array_equal(t0, t1) and np.array_equal(v0, v2) and np.array_equal(t0, t2)
    assert v1.dtype == np.float64 and v1.shape[0] == V0.shape[0]


def test_evaluation_count_follows_the_surface():
    """sphere at R = 65, brick 8, lipschitz 1: the numpy model gives 128 active bricks of 512, 0.34 of R^3 with the shared faces
    evaluated per brick; the cap of one half leaves room for bricks that flip on the last ulp. A cap, not a measurement."""
    from vdn_hip import mesh
    q = Counting(sphere(0.537))
    V1, F1, stats = mesh.marching_cubes_sparse(q, *axes(65), brick=8, lipschitz=1.0)
    assert q.points == stats["points_evaluated"]
    print("points evaluated %d = %.4f of R^3, active bricks %d of %d" % (q.points, q.points / 65.0 ** 3, stats["active_bricks"], stats["bricks"]))
    assert stats["points_evaluated"] < 0.5 * 65 ** 3
    V0, F0 = dense(sphere(0.537), 65)
    assert torch.equal(F1, F0) and torch.equal(V1, V0)


def test_a_violated_bound_raises_and_nothing_faulted():
    from vdn_hip import mesh
    with pytest.raises(mesh.SparseExtractionError) as e:
        mesh.marching_cubes_sparse(steep, *axes(37), brick=8, lipschitz=1.0)
    assert "lipschitz" in str(e.value) and "dense" in str(e.value)
    V0, F0 = dense(steep, 37)                                 # the process is intact
    assert F0.shape[0] > 0
    V1, F1, stats = mesh.marching_cubes_sparse(steep, *axes(37), brick=8, lipschitz=4.0)
    assert stats["missed_edges"] == 0 and stats["active_bricks"] < stats["bricks"]
    assert torch.equal(F1, F0) and torch.equal(V1, V0)


def test_empty_level_set():
    from vdn_hip import mesh
    q = Counting(lambda p: torch.ones_like(p[:, 0]))
    V, F, stats = mesh.marching_cubes_sparse(q, *axes(37), brick=8, lipschitz=1.0)
    assert V.shape == (0, 3) and F.shape == (0, 3) and V.dtype == torch.float64 and F.dtype == torch.int64
    assert stats == {"bricks": 125, "active_bricks": 0, "points_evaluated": 125, "missed_edges": 0} and q.points == 125
    # active bricks whose cells are all on one side: the sizes come back zero after the count pass
    V, F, stats = mesh.marching_cubes_sparse(lambda p: torch.full_like(p[:, 0], 0.01), *axes(37), brick=8, lipschitz=1.0)
    assert V.shape == (0, 3) and F.shape == (0, 3) and stats["active_bricks"] == 125


def test_cpu_tensors_and_bad_query_funcs_are_refused():
    from vdn_hip import mesh
    X, Y, Z = axes(17)
    f = sphere(0.537)
    for args in ((X.cpu(), Y, Z), (X, Y.cpu(), Z), (X, Y, Z.cpu()), (X.double(), Y, Z), (X[:-1], Y, Z), (X[None], Y, Z), (X[:1], Y[:1], Z[:1]),
                 (X.cpu().numpy(), Y, Z)):
        with pytest.raises(ValueError):
            mesh.marching_cubes_sparse(f, *args)
    with pytest.raises(ValueError):
        mesh.marching_cubes_sparse(lambda p: p, X, Y, Z)       # three values per point
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4, 4))             # (the dense entry's own rule, for comparison)


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def _network(precision):
    """-> (renderer, lo, hi, L, dense (v, t)): L = 2 x the largest |gradient| over the dense lattice's nodes"""
    if precision not in _CACHE:
        from vdn_train import factory, synth
        R = 64
        rend = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(5), precision=precision)
        lo, hi = torch.tensor([LO] * 3), torch.tensor([HI] * 3)
        pts = torch.stack(torch.meshgrid(*axes(R), indexing="ij"), dim=-1).reshape(-1, 3)
        with torch.no_grad():
            g = torch.cat([rend.sdf_network.gradient(p).reshape(-1, 3).float().norm(dim=-1) for p in pts.split(1 << 16)])
        L = 2.0 * float(g.max())
        _CACHE[precision] = (rend, lo, hi, L, rend.extract_geometry(lo, hi, R, threshold=0.0))
    return _CACHE[precision]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_network_extraction_is_equal(precision, monkeypatch):
    monkeypatch.delenv("VDN_MESH_SPARSE", raising=False)
    rend, lo, hi, L, (v0, t0) = _network(precision)
    assert t0.shape[0] > 100 and np.isfinite(L) and L > 0
    v1, t1 = rend.extract_geometry(lo, hi, 64, threshold=0.0, sparse={"brick": 8, "lipschitz": L})
    assert v1.dtype == v0.dtype and t1.dtype == t0.dtype
    assert np.array_equal(t1, t0) and np.array_equal(v1, v0)
    # the switch of an unchanged runner
    monkeypatch.setenv("VDN_MESH_SPARSE", "8:%r" % L)
    v2, t2 = rend.extract_geometry(lo, hi, 64, threshold=0.0)
    assert np.array_equal(t2, t0) and np.array_equal(v2, v0)
    # it does skip work on the network
    from vdn_hip import mesh
    q = Counting(lambda p: -rend.sdf_network.sdf(p))
    _, _, stats = mesh.marching_cubes_sparse(q, *axes(64), brick=8, lipschitz=L)
    print("%s: L = %.4f, active bricks %d of %d, points %d = %.3f of R^3" % (precision, L, stats["active_bricks"], stats["bricks"], q.points,
                                                                           q.points / 64.0 ** 3))
    assert stats["active_bricks"] < stats["bricks"] and q.points == stats["points_evaluated"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_validate_mesh_writes_the_same_file(precision, tmp_path, monkeypatch):
    from vdn_train import validate
    monkeypatch.delenv("VDN_MESH_SPARSE", raising=False)
    rend, lo, hi, L, (v0, t0) = _network(precision)
    p0, nv0, nf0 = validate.validate_mesh(rend, lo, hi, str(tmp_path / "dense.ply"), resolution=64)
    p1, nv1, nf1 = validate.validate_mesh(rend, lo, hi, str(tmp_path / "sparse.ply"), resolution=64, sparse={"brick": 8, "lipschitz": L})
    assert (nv0, nf0) == (nv1, nf1) == (v0.shape[0], t0.shape[0])
    assert open(p0, "rb").read() == open(p1, "rb").read()
    monkeypatch.setenv("VDN_MESH_SPARSE", "8:%r" % L)
    p2, _, _ = validate.validate_mesh(rend, lo, hi, str(tmp_path / "env.ply"), resolution=64, vertex_colors=False, vertex_normals=False)
    monkeypatch.delenv("VDN_MESH_SPARSE")
    p3, _, _ = validate.validate_mesh(rend, lo, hi, str(tmp_path / "bare.ply"), resolution=64, vertex_colors=False, vertex_normals=False)
    assert open(p2, "rb").read() == open(p3, "rb").read()
