"""Brick-sparse marching cubes, the parts that need no device: a numpy model of the brick cut, the coarse test, the
compact cell order and the missed-edge check, fed through oracle.marching_cubes (nodes that are never evaluated are +-inf there), on
the fields the GPU tests use; the argument errors of the Python entry points; the C layouts of the new argument blocks."""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import marching_cubes as omc

LO, HI = -1.01, 1.01
SLACK = 1e-5             # vdn_hip.mesh.SPARSE_RADIUS_SLACK, restated
_DENSE = {}


# ---- the fields (numpy fp32 in, fp32 out; the GPU tests restate them in torch) ---------------------------------------------------------
def _norm(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def sphere(r, c=(0.0, 0.0, 0.0)):
    return lambda x, y, z: _norm(x - np.float32(c[0]), y - np.float32(c[1]), z - np.float32(c[2])) - np.float32(r)


def torus(x, y, z):
    q = np.sqrt(x * x + y * y) - np.float32(0.6)
    return np.sqrt(q * q + z * z) - np.float32(0.23)


def two_spheres(x, y, z):
    return np.minimum(sphere(0.31, (-0.45, 0.1, 0.0))(x, y, z), sphere(0.27, (0.4, -0.2, 0.15))(x, y, z))


def steep(x, y, z):
    return np.float32(4.0) * (_norm(x, y, z) - np.float32(0.537))


def slab(R):
    x16 = axis(R)[16]
    return lambda x, y, z: (x - x16) + np.float32(0.0) * (y + z)


def axis(R, lo=LO, hi=HI):
    return torch.linspace(lo, hi, R).numpy()


def lattice(f, R):
    X = axis(R)
    return f(X[:, None, None], X[None, :, None], X[None, None, :]).astype(np.float32)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def np_sparse_model(f, R, level, brick, lipschitz):
    """-> dict: the dense lattice u, the lattice with the never-evaluated nodes at +-inf, the active-brick mask, the active-cell mask,
    the missed-edge count (the triples vdn_mesh_sparse_count adds up) and the points the model evaluates."""
    X = axis(R)
    u = lattice(f, R)
    n = R - 1
    B = min(brick, n)
    nb = -(-n // B)
    level = float(np.float32(level))
    lo = np.arange(nb) * B
    hi = np.minimum(lo + B, n)
    mid = ((X[lo].astype(np.float64) + X[hi].astype(np.float64)) * 0.5).astype(np.float32)
    ext = X[hi].astype(np.float64) - X[lo].astype(np.float64)
    fc = f(mid[:, None, None], mid[None, :, None], mid[None, None, :]).astype(np.float32)
    r = 0.5 * np.sqrt(ext[:, None, None] ** 2 + ext[None, :, None] ** 2 + ext[None, None, :] ** 2)
    ulp = float(np.abs(X).max()) * 2.0 ** -23
    active = ~(np.abs(fc.astype(np.float64) - level) > lipschitz * (r * (1.0 + SLACK) + ulp))
    evaluated = np.zeros((R, R, R), bool)
    fill = np.zeros((R, R, R), np.float32)
    cell_active = np.zeros((n, n, n), bool)
    for bi in range(nb):
        for bj in range(nb):
            for bk in range(nb):
                box = (slice(lo[bi], hi[bi] + 1), slice(lo[bj], hi[bj] + 1), slice(lo[bk], hi[bk] + 1))
                if active[bi, bj, bk]:
                    evaluated[box] = True
                    cell_active[lo[bi]:hi[bi], lo[bj]:hi[bj], lo[bk]:hi[bk]] = True
                else:
                    fill[box] = np.inf if fc[bi, bj, bk] > level else -np.inf
    us = np.where(evaluated, u, fill)
    # missed edges: per cut lattice edge, (active cells round it) x (existing cells round it in dropped bricks)
    inside = u.astype(np.float64) <= level
    missed = 0
    for ax in range(3):
        cut = np.take(inside, range(0, n), axis=ax) != np.take(inside, range(1, R), axis=ax)      # [.., n along ax, ..] over nodes
        n_act = np.zeros(cut.shape, np.int64)
        n_drop = np.zeros(cut.shape, np.int64)
        o1, o2 = [a for a in range(3) if a != ax]
        for d1 in (0, 1):
            for d2 in (0, 1):
                # the cell at node index l - d along the two other axes, where it exists
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                dst[o1], src[o1] = (slice(1, R), slice(0, n)) if d1 else (slice(0, n), slice(0, n))
                dst[o2], src[o2] = (slice(1, R), slice(0, n)) if d2 else (slice(0, n), slice(0, n))
                n_act[tuple(dst)] += cell_active[tuple(src)]
                n_drop[tuple(dst)] += ~cell_active[tuple(src)]
        missed += int((cut * n_act * n_drop).sum())
    n_active = int(active.sum())
    return {"u": u, "u_sparse": us, "active": active, "cell_active": cell_active, "missed": missed, "B": B, "nb": nb,
            "points": nb ** 3 + n_active * (B + 1) ** 3}


def np_rank_tables(active, R, B):
    """the brick tables of include/vdn_render.h's rank formula, as vdn_hip.mesh.marching_cubes_sparse builds them"""
    n = R - 1
    nb = active.shape[0]
    lo = np.arange(nb) * B
    width = np.minimum(lo + B, n) - lo
    zc = active.astype(np.int64) * width[None, None, :]
    col = zc.sum(axis=2)
    colw = col * width[None, :]
    row = colw.sum(axis=1)
    roww = row * width
    base = (np.cumsum(roww) - roww)[:, None, None] + (np.cumsum(colw, axis=1) - colw)[:, :, None] + (np.cumsum(zc, axis=2) - zc)
    return base, col, row


def dense_oracle(name, f, R, level):
    key = (name, R, level)
    if key not in _DENSE:
        _DENSE[key] = omc.marching_cubes(lattice(f, R), level)
    return _DENSE[key]


CASES = [("sphere", sphere(0.537), 37, 0.0, 8), ("torus", torus, 41, 0.0, 4), ("torus", torus, 41, 0.0, 8), ("torus", torus, 41, 0.05, 8),
         ("big_sphere", sphere(1.3), 37, 0.0, 8), ("slab", slab(33), 33, 0.0, 8), ("two_spheres", two_spheres, 41, 0.0, 8),
         ("sphere", sphere(0.537), 3, 0.0, 8), ("sphere", sphere(0.537), 9, 0.0, 8)]


@pytest.mark.parametrize("name,f,R,level,brick", CASES, ids=["%s-R%d-l%g-b%d" % (c[0], c[2], c[3], c[4]) for c in CASES])
def test_sparse_model_equals_the_dense_oracle_bit_for_bit(name, f, R, level, brick):
    m = np_sparse_model(f, R, level, brick, 1.0)
    v0, t0 = dense_oracle(name, f, R, level)
    v1, t1 = omc.marching_cubes(m["u_sparse"], level)
    assert t0.shape[0] > 0
    assert m["missed"] == 0
    assert v0.tobytes() == v1.tobytes() and np.array_equal(t0, t1)
    # every cut cell of the dense lattice lies in an active brick
    ins = m["u"].astype(np.float64) <= float(np.float32(level))
    n = R - 1
    corners = np.stack([ins[a:a + n, b:b + n, c:c + n] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    cut = corners.any(axis=0) & ~corners.all(axis=0)
    assert not (cut & ~m["cell_active"]).any()


def test_the_cases_do_skip_bricks_and_the_slab_ties():
    """the model is not vacuous: bricks are dropped where there are enough of them, and the slab has f == level on the nodes of a
    brick face"""
    for name, f, R, level, brick in CASES:
        m = np_sparse_model(f, R, level, brick, 1.0)
        if m["nb"] > 2 and name != "big_sphere":
            assert 0 < m["active"].sum() < m["active"].size, name
    u = lattice(slab(33), 33)
    assert (u[16] == 0.0).all() and 16 % 8 == 0
    # the sphere at R = 65, brick 8: the figure the GPU test's cap of one half of R^3 is set against
    m = np_sparse_model(sphere(0.537), 65, 0.0, 8, 1.0)
    assert m["active"].size == 512 and int(m["active"].sum()) == 128
    assert abs(m["points"] / 65.0 ** 3 - 0.34) < 0.005


@pytest.mark.parametrize("R,brick", [(37, 8), (41, 4), (9, 8), (3, 8), (20, 3)])
def test_compact_order_is_the_sorted_global_cell_numbers(R, brick):
    """rank(i, j, k) from the brick tables == the position of the cell among the active cells sorted by (i (R-1) + j) (R-1) + k"""
    m = np_sparse_model(torus, R, 0.0, brick, 1.0)
    if R == 20:
        rng = np.random.default_rng(5)
        m["active"] = rng.random(m["active"].shape) < 0.4                   # bricks interleaving in every column
    B, nb, n = m["B"], m["nb"], R - 1
    base, col, row = np_rank_tables(m["active"], R, B)
    cells = []
    for b in np.argwhere(m["active"]):
        i, j, k = np.meshgrid(*[np.arange(b[a] * B, min((b[a] + 1) * B, n)) for a in range(3)], indexing="ij")
        rank = base[b[0], b[1], b[2]] + (i - b[0] * B) * row[b[0]] + (j - b[1] * B) * col[b[0], b[1]] + (k - b[2] * B)
        cells.append(np.stack([((i * n + j) * n + k).ravel(), rank.ravel()], axis=1))
    cells = np.concatenate(cells)
    order = np.argsort(cells[:, 0], kind="stable")
    assert np.array_equal(cells[order, 1], np.arange(cells.shape[0]))


def test_a_violated_bound_is_seen_and_a_true_one_is_not():
    m = np_sparse_model(steep, 37, 0.0, 8, 1.0)
    assert m["missed"] > 0
    v0, t0 = dense_oracle("steep", steep, 37, 0.0)
    m4 = np_sparse_model(steep, 37, 0.0, 8, 4.0)
    v1, t1 = omc.marching_cubes(m4["u_sparse"], 0.0)
    assert m4["missed"] == 0 and v0.tobytes() == v1.tobytes() and np.array_equal(t0, t1)
    assert m4["active"].sum() < m4["active"].size


# ---- argument errors that need no device ------------------------------------------------------------------------------------------------
def test_marching_cubes_sparse_refuses_bad_options_before_any_device():
    from vdn_hip import mesh
    assert issubclass(mesh.SparseExtractionError, RuntimeError)
    assert mesh.SPARSE_RADIUS_SLACK == SLACK and mesh.SPARSE_LIPSCHITZ == 2.0
    X = torch.linspace(LO, HI, 9)
    f = lambda p: p[:, 0]
    for kw in ({"brick": 0}, {"brick": -3}, {"brick": 2.5}, {"lipschitz": 0.0}, {"lipschitz": -1.0}, {"lipschitz": float("nan")},
               {"chunk_points": 0}):
        with pytest.raises(ValueError):
            mesh.marching_cubes_sparse(f, X, X, X, **kw)
    with pytest.raises(ValueError):                       # CPU tensors
        mesh.marching_cubes_sparse(f, X, X, X)
    assert mesh.check_sparse_options(4, float("inf"), 10) == (4, float("inf"), 10)


def test_extract_geometry_refuses_bad_sparse_arguments_before_any_device(monkeypatch):
    from dpt_models import renderer as R
    monkeypatch.delenv("VDN_MESH_SPARSE", raising=False)
    monkeypatch.delenv("VDN_MESH_METHOD", raising=False)
    lo, hi = torch.tensor([LO] * 3), torch.tensor([HI] * 3)

    def never(pts):
        raise AssertionError("query_func must not run")
    for sparse in ({"bricks": 8}, {"brick": 8, "slack": 1.0}, {"brick": 0}, {"lipschitz": 0.0}, {"lipschitz": float("nan")}, "yes", 8):
        with pytest.raises(ValueError):
            R.extract_geometry(lo, hi, 9, 0.0, never, sparse=sparse)
    for sparse in (True, {"brick": 4}):
        with pytest.raises(ValueError):
            R.extract_geometry(lo, hi, 9, 0.0, never, method="tets", sparse=sparse)
    monkeypatch.setenv("VDN_MESH_METHOD", "tets")
    with pytest.raises(ValueError):
        R.extract_geometry(lo, hi, 9, 0.0, never, sparse=True)
    monkeypatch.delenv("VDN_MESH_METHOD")
    for env in ("8", "8:", "a:b", "8:2:1", "0:2", "8:0", "8:nan", "yes"):
        monkeypatch.setenv("VDN_MESH_SPARSE", env)
        with pytest.raises(ValueError):
            R.extract_geometry(lo, hi, 9, 0.0, never)
    # what the switch parses to
    monkeypatch.setenv("VDN_MESH_SPARSE", "4:2.5")
    assert R.parse_sparse(None) == {"brick": 4, "lipschitz": 2.5, "chunk_points": 1 << 22}
    assert R.parse_sparse({"brick": 16}) == {"brick": 16, "lipschitz": 2.0, "chunk_points": 1 << 22}      # the argument wins
    monkeypatch.setenv("VDN_MESH_SPARSE", "1")
    assert R.parse_sparse(False) == {"brick": 8, "lipschitz": 2.0, "chunk_points": 1 << 22}
    for env in ("", "0"):
        monkeypatch.setenv("VDN_MESH_SPARSE", env)
        assert R.parse_sparse(None) is None
    monkeypatch.delenv("VDN_MESH_SPARSE")
    assert R.parse_sparse(None) is None and R.parse_sparse(True)["brick"] == 8
    with pytest.raises(ValueError):
        R.parse_sparse(True, method="tets")


def test_the_keyword_reaches_every_layer():
    import inspect
    from dpt_models import renderer as R
    from vdn_train import validate
    for fn in (R.extract_geometry, R.NeuSRenderer.extract_geometry, R.NeuSRenderer.extract_colored_geometry, validate.validate_mesh):
        assert inspect.signature(fn).parameters["sparse"].default is None


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("vdn_mesh_sparse_nodes", "vdn_mesh_sparse_count", "vdn_mesh_sparse_emit")


def test_sparse_argument_blocks_are_c_layouts_and_declared():
    from vdn_hip import lib
    _, funcs = lib.parse_header()
    for fn in ENTRY_POINTS:
        assert funcs[fn] == [ctypes.c_void_p, ctypes.c_void_p]
    N = lib.VdnMeshSparseNodesArgs                         # {5 pointers, 2 int64, 4 int32}
    assert ctypes.sizeof(N) == 5 * 8 + 2 * 8 + 4 * 4 == 72
    assert (N.X.offset, N.active.offset, N.points.offset, N.first.offset, N.n_points.offset, N.R.offset, N.A.offset) == (0, 24, 32, 40, 48, 56, 68)
    S = lib.VdnMeshSparseArgs                              # {pointer, double, 4 int32, 5 pointers, int64, 4 pointers, 2 pointers, 2 int64, 2 pointers}
    assert ctypes.sizeof(S) == 8 + 8 + 16 + 5 * 8 + 8 + 4 * 8 + 2 * 8 + 2 * 8 + 2 * 8 == 160
    assert (S.values.offset, S.isovalue.offset, S.R.offset, S.A.offset, S.active.offset, S.row_cells.offset, S.n_cells.offset, S.cube_case.offset,
            S.missed.offset, S.vert_offsets.offset, S.V.offset, S.F.offset, S.vertices.offset, S.triangles.offset) == (
                0, 8, 16, 28, 32, 64, 72, 80, 104, 112, 128, 136, 144, 152)
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28     # additive: no bump
    so = lib.load()
    for fn in ENTRY_POINTS:
        assert getattr(so, fn) is not None


def _blocks(lib, R=17, brick=8, nb=2, A=1):
    na = lib.VdnMeshSparseNodesArgs()
    na.X = na.Y = na.Z = na.active = na.points = 16
    na.R, na.brick, na.nb, na.A, na.first, na.n_points = R, brick, nb, A, 0, 1
    a = lib.VdnMeshSparseArgs()
    for f in ("values", "active", "brick_map", "cell_base", "col_cells", "row_cells", "cube_case", "n_verts", "n_tris", "missed", "vert_offsets",
              "tri_offsets", "vertices", "triangles"):
        setattr(a, f, 16)
    a.R, a.brick, a.nb, a.A, a.n_cells, a.V, a.F = R, brick, nb, A, 1, 1, 1
    return na, a


def test_sparse_entry_points_refuse_bad_blocks_on_the_host():
    """checked before anything is launched: the pointers are never dereferenced"""
    from vdn_hip import lib
    for name, args in (("vdn_mesh_sparse_nodes", lib.VdnMeshSparseNodesArgs()), ("vdn_mesh_sparse_count", lib.VdnMeshSparseArgs()),
                       ("vdn_mesh_sparse_emit", lib.VdnMeshSparseArgs())):
        with pytest.raises(lib.VdnError):
            lib.call(name, args, None)
        with pytest.raises(lib.VdnError):
            lib.call(name, None, None)
    # sizes beyond 32-bit indexing: status -10, nothing launched
    for R, brick, nb, A in ((1 << 14, 8, 1 << 11, 1), ((1 << 23) + 1, 8, 1 << 20, 1), (8 * 1000 + 1, 8, 1000, 3_000_000), (2049, 2048, 1, 1)):
        na, a = _blocks(lib, R, brick, nb, A)
        a.n_cells = 1
        assert lib.try_call("vdn_mesh_sparse_nodes", na, None) is False, (R, brick, nb, A)
        assert lib.try_call("vdn_mesh_sparse_count", a, None) is False and lib.try_call("vdn_mesh_sparse_emit", a, None) is False, (R, brick, nb, A)
    # inconsistent blocks: status -1
    for field, bad in (("R", 1), ("brick", 0), ("nb", 3), ("nb", 1), ("A", -1), ("A", 9)):
        na, a = _blocks(lib)
        setattr(na, field, bad)
        setattr(a, field, bad)
        with pytest.raises(lib.VdnError):
            lib.call("vdn_mesh_sparse_nodes", na, None)
        with pytest.raises(lib.VdnError):
            lib.call("vdn_mesh_sparse_count", a, None)
    na, a = _blocks(lib)
    for first, n_points in ((-1, 1), (0, 0), (0, 730), (729, 1)):
        na.first, na.n_points = first, n_points
        with pytest.raises(lib.VdnError):
            lib.call("vdn_mesh_sparse_nodes", na, None)
    for field, bad in (("n_cells", 0), ("n_cells", 513), ("A", 0), ("V", 0), ("F", 0)):
        na, a = _blocks(lib)
        setattr(a, field, bad)
        with pytest.raises(lib.VdnError):
            lib.call("vdn_mesh_sparse_emit", a, None)
