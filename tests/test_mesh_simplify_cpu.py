"""Numpy restatements of the mesh simplification (csrc/mesh_simplify.hip, vdn_hip/mesh.py: cluster_quadrics / simplify_mesh; DESIGN.md
3p) and their own checks; tests/test_gpu_mesh_simplify.py holds the kernels to them. np_quadrics and np_means follow the device's
summation order literally (lane l of 64 adds the entries j = l, l + 64, .. in increasing j from +0.0, then a tree over the lanes), so
their sums can be compared to the bit; np_place solves with np.linalg.solve; np_simplify applies the first-occurrence duplicate rule
by a walk over the triangles in input order."""
import os

import numpy as np
import pytest

R = 24                                   # the fixtures' lattice, on [-1, 1]^3
ORIGIN = (-0.37, -0.21, -0.13)
CELL_SIZES = (2.5, 4.0)
_CACHE = {}


# ---- fixtures: marching-cubes surfaces in lattice-index coordinates -----------------------------------------------------------------
def _rot(p):
    """rotate by 0.3 rad about z, then by 0.2 rad about x (rows of p are points)"""
    cz, sz, cx, sx = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return p @ (Rx @ Rz).T


def sdf(name, p):
    """the fixture fields at world points p [N,3] in [-1, 1]^3"""
    p = np.asarray(p, np.float64)
    if name == "sphere":
        return np.linalg.norm(p, axis=1) - 0.71
    if name == "torus":
        return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.55) ** 2 + p[:, 2] ** 2) - 0.27
    if name == "box":                    # a max-norm box of half-width 0.52, rotated: the field at p is the box's at the point rotated back
        return np.abs(p @ _rot(np.eye(3))).max(axis=1) - 0.52
    raise KeyError(name)


def to_world(x):
    return np.asarray(x, np.float64) / (R - 1.0) * 2.0 - 1.0


def surface(name):
    """-> (vertices [V,3] fp32 in lattice-index coordinates, triangles [F,3] int64) of oracle.marching_cubes on the 24^3 lattice"""
    if name not in _CACHE:
        from oracle import marching_cubes
        g = np.linspace(-1.0, 1.0, R)
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        v, t = marching_cubes.marching_cubes(sdf(name, pts).reshape(R, R, R).astype(np.float32), 0.0)
        _CACHE[name] = (v.astype(np.float32), t.astype(np.int64))
    return _CACHE[name]


def hand_made():
    """-> (vertices fp32 [8,3], triangles [8,3], cell_size, origin): cells A (0,0,0), B (1,0,0), C (0,1,0), D (1,1,0)"""
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [1.5, 1.5, 0.5], [np.nan, 0.0, 0.0],
                  [5.5, 5.5, 5.5],       # used by no triangle
                  [1.4, 0.6, 0.5]], np.float32)
    t = np.array([[0, 1, 2],             # A B C: emitted
                  [0, 1, 2],             # repeated: goes
                  [1, 2, 0],             # rotated: goes
                  [0, 2, 1],             # reversed: stays
                  [0, 3, 1],             # two corners in A: collapsed
                  [1, 4, 5],             # a corner that is not finite
                  [7, 4, 2],             # B D C: emitted
                  [3, 7, 2]], np.int64)  # A B C through other vertices: goes
    return v, t, 1.0, (0.0, 0.0, 0.0)


HAND_TRIANGLES = np.array([[0, 1, 2], [0, 2, 1], [1, 3, 2]])
HAND_VERTEX_CLUSTER = np.array([0, 1, 2, 0, 3, -1, -1, 1])
HAND_REPORT = {"vertices_in": 8, "faces_in": 8, "clusters": 4, "vertices_out": 4, "faces_out": 3, "faces_collapsed": 1, "faces_duplicate": 3,
               "faces_non_finite": 1}


def two_sheets():
    """two 17 x 17 sheets at spacing 0.5, z = 0.9 and z = 1.3 plus a small ripple, the upper one wound the other way"""
    i, j = np.meshgrid(np.arange(17), np.arange(17), indexing="ij")
    x, y = 0.5 * i.reshape(-1), 0.5 * j.reshape(-1)
    ripple = 0.02 * np.sin(1.7 * x) * np.cos(1.3 * y)
    q = (i[:-1, :-1] * 17 + j[:-1, :-1]).reshape(-1)
    lower = np.concatenate([np.stack([q, q + 17, q + 18], 1), np.stack([q, q + 18, q + 1], 1)])
    v = np.concatenate([np.stack([x, y, 0.9 + ripple], 1), np.stack([x, y, 1.3 + ripple], 1)]).astype(np.float32)
    t = np.concatenate([lower, lower[:, ::-1] + 17 * 17]).astype(np.int64)
    return v, t


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def np_keys(v32, t, h, origin=None):
    """-> dict: live [F] bool, used [V] bool, origin (3 floats), index [V,3] int64 (floor((double(v) - origin) / h), rows of vertices
    that are not finite hold 0), lo [3], dims [3], key [V] int64 (-1: not finite or outside the grid of the used vertices)"""
    v = np.asarray(v32, np.float32).astype(np.float64)
    fin = np.isfinite(v).all(axis=1)
    live = fin[t].all(axis=1) if len(t) else np.zeros(0, bool)
    used = np.zeros(len(v), bool)
    used[t[live].reshape(-1)] = True
    if not used.any():
        return {"live": live, "used": used, "origin": origin, "key": np.full(len(v), -1, np.int64)}
    origin = np.asarray(v[used].min(axis=0) if origin is None else origin, np.float64)
    with np.errstate(invalid="ignore"):
        index = np.floor((v - origin[None]) / h)
    index = np.where(fin[:, None], index, 0.0).astype(np.int64)
    lo, hi = index[used].min(axis=0), index[used].max(axis=0)
    dims = hi - lo + 1
    rel = index - lo[None]
    inside = fin & ((rel >= 0) & (rel < dims[None])).all(axis=1)
    key = np.where(inside, rel[:, 0] + dims[0] * (rel[:, 1] + dims[1] * rel[:, 2]), -1)
    return {"live": live, "used": used, "origin": origin, "index": index, "lo": lo, "dims": dims, "key": key}


def np_clusters(v32, t, h, origin=None):
    """np_keys plus: C, vertex_cluster [V] (-1: in no cluster), cell [C,3], centre [C,3] = origin + (cell + 0.5) h"""
    k = np_keys(v32, t, h, origin)
    vc = np.full(len(v32), -1, np.int64)
    if k["used"].any():
        uniq, inv = np.unique(k["key"][k["used"]], return_inverse=True)           # ascending key order
        vc[k["used"]] = inv
        d = k["dims"]
        cell = np.stack([uniq % d[0], (uniq // d[0]) % d[1], uniq // (d[0] * d[1])], axis=1) + k["lo"][None]
        k.update(C=len(uniq), cell=cell, centre=k["origin"][None] + (cell.astype(np.float64) + 0.5) * h)
    else:
        k.update(C=0, cell=np.zeros((0, 3), np.int64), centre=np.zeros((0, 3)))
    k["vertex_cluster"] = vc
    return k


def lane_sum(values):
    """values [n,K] float64 -> [K]: lane l of 64 adds the rows j = l, l + 64, .. in increasing j from +0.0 (a missing row is a +0.0,
    which changes no bit of a sum that started at +0.0), then partial[l] += partial[l + s] for s = 32, 16, 8, 4, 2, 1, l < s"""
    values = np.asarray(values, np.float64)
    n, K = values.shape
    rows = max(1, -(-n // 64))
    padded = np.zeros((rows * 64, K))
    padded[:n] = values
    partial = np.zeros((64, K))
    for r in range(rows):
        partial = partial + padded[r * 64:(r + 1) * 64]
    for s in (32, 16, 8, 4, 2, 1):
        partial[:s] = partial[:s] + partial[s:2 * s]
    return partial[0].copy()


def np_means(rows32, vertex_cluster, C):
    """the segmented mean of fp32 rows [V,K] -> float64 [C,K]: lane_sum over a cluster's members in ascending vertex index / count"""
    rows = np.asarray(rows32, np.float32).astype(np.float64).reshape(len(rows32), -1)
    out = np.empty((C, rows.shape[1]))
    order = np.argsort(np.where(vertex_cluster < 0, C, vertex_cluster), kind="stable")
    start = np.searchsorted(np.where(vertex_cluster < 0, C, vertex_cluster)[order], np.arange(C + 1))
    for c in range(C):
        m = order[start[c]:start[c + 1]]
        out[c] = lane_sum(rows[m]) / float(len(m))
    return out


def plane_terms(pa, pb, pc):
    """the ten values a triangle adds, from its corners relative to a centre (rows)"""
    u, w = pb - pa, pc - pa
    n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    d = -((n0 * pa[:, 0] + n1 * pa[:, 1]) + n2 * pa[:, 2])
    return np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2, n0 * d, n1 * d, n2 * d, d * d], axis=1)


def np_quadrics(v32, t, k):
    """cluster quadrics [C,10] of np_clusters' dict k: a cluster's corner records in (triangle, corner) order, each recomputed from
    its triangle relative to that cluster's centre, summed by lane_sum"""
    v = np.asarray(v32, np.float32).astype(np.float64)
    C, vc = k["C"], k["vertex_cluster"]
    corner = np.where(k["live"][:, None], vc[np.where(k["live"][:, None], t, 0)], C).reshape(-1)
    order = np.argsort(corner, kind="stable")
    start = np.searchsorted(corner[order], np.arange(C + 1))
    out = np.empty((C, 10))
    for c in range(C):
        f = order[start[c]:start[c + 1]] // 3
        ctr = k["centre"][c][None]
        out[c] = lane_sum(plane_terms(v[t[f, 0]] - ctr, v[t[f, 1]] - ctr, v[t[f, 2]] - ctr))
    return out


def np_place(quadric, mean, h, eps=1e-3):
    """-> (x [C,3] relative to the centre, status [C] uint8)"""
    x, status = np.array(mean, np.float64), np.zeros(len(mean), np.uint8)
    for c, (q, m) in enumerate(zip(quadric, mean)):
        A = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
        tr = q[0] + q[3] + q[5]
        if not (tr > 0.0 and np.isfinite(tr)):
            status[c] = 1
            continue
        y = m + np.linalg.solve(A + eps * tr * np.eye(3), -q[6:9] - A @ m)
        if not np.isfinite(y).all() or (np.abs(y) > 0.5 * h).any():
            status[c] = 2
            continue
        x[c] = y
    return x, status


def np_emit(t, k):
    """-> (emit [F] bool, corner clusters [F,3], counts): the first-occurrence rule by a walk in input order"""
    C, vc = k["C"], k["vertex_cluster"]
    emit, seen = np.zeros(len(t), bool), set()
    cc = np.full((len(t), 3), -1, np.int64)
    collapsed = duplicate = 0
    for f in range(len(t)):
        if not k["live"][f]:
            continue
        c = [int(vc[i]) for i in t[f]]
        cc[f] = c
        if len(set(c)) < 3:
            collapsed += 1
            continue
        s = c.index(min(c))
        triple = (c[s], c[(s + 1) % 3], c[(s + 2) % 3])
        if triple in seen:
            duplicate += 1
            continue
        seen.add(triple)
        emit[f] = True
    return emit, cc, {"faces_collapsed": collapsed, "faces_duplicate": duplicate, "faces_non_finite": int((~k["live"]).sum())}


def np_simplify(v32, t, h, origin=None, placement="quadric", eps=1e-3, attributes=()):
    """-> dict(vertices [V',3] float64, triangles [F',3], vertex_cluster [V] (the new vertex, -1: none), status [V'], attributes
    (float64 means), report, and the cluster-level arrays: clusters (np_clusters' dict), quadric, mean, x, kept)"""
    t = np.asarray(t, np.int64)
    k = np_clusters(v32, t, h, origin)
    C = k["C"]
    emit, cc, counts = np_emit(t, k)
    mean_abs = np_means(v32, k["vertex_cluster"], C) if C else np.zeros((0, 3))
    mean = mean_abs - k["centre"]
    quadric = np_quadrics(v32, t, k) if C else np.zeros((0, 10))
    if placement == "mean":
        position, status, x = mean_abs, np.zeros(C, np.uint8), mean
    else:
        x, status = np_place(quadric, mean, h, eps)
        position = k["centre"] + x
    kept = np.unique(cc[emit].reshape(-1))
    new = np.full(C + 1, -1, np.int64)
    new[kept] = np.arange(len(kept))
    report = dict(counts, vertices_in=len(v32), faces_in=len(t), clusters=C, vertices_out=len(kept), faces_out=int(emit.sum()))
    return {"vertices": position[kept], "triangles": new[cc[emit]], "vertex_cluster": new[k["vertex_cluster"]], "status": status[kept],
            "attributes": [np_means(a, k["vertex_cluster"], C)[kept] for a in attributes], "report": report,
            "clusters": k, "quadric": quadric, "mean": mean, "x": x, "kept": kept}


def quadric_error(q, p):
    """p^T A p + 2 b.p + c at points p [N,3] relative to the centre"""
    A = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
    return np.einsum("ni,ij,nj->n", p, A, p) + 2.0 * p @ q[6:9] + q[9]


# ---- checks on the restatements ---------------------------------------------------------------------------------------------------
def test_lane_sum_is_the_sum_and_follows_the_strided_order():
    rng = np.random.default_rng(0)
    for n in (0, 1, 63, 64, 65, 1000):
        x = rng.standard_normal((n, 3))
        assert np.allclose(lane_sum(x), x.sum(axis=0), rtol=0, atol=1e-12 * max(n, 1))
    # the order is visible: 1e16 in lane 0 swallows lane 0's later 1.0s, while the 1.0s of the other lanes meet it in the tree
    x = np.zeros((128, 1))
    x[0], x[64], x[1], x[65] = 1e16, 1.0, 1.0, 1.0
    assert lane_sum(x)[0] == 1e16 + 2.0


def test_keys_follow_the_division_and_the_grid():
    v, t, h, origin = hand_made()
    k = np_clusters(v, t, h, origin)
    assert k["dims"].tolist() == [2, 2, 1] and k["lo"].tolist() == [0, 0, 0]
    assert k["key"].tolist() == [0, 1, 2, 0, 3, -1, -1, 1]                 # the NaN vertex and the one outside the grid
    assert k["cell"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    assert np.array_equal(k["centre"], np.array(k["cell"]) + 0.5)
    # a vertex below a given origin has a negative cell index; the keys stay non-negative
    k2 = np_clusters(v, t, h, (1.0, 0.0, 0.0))
    assert k2["lo"].tolist() == [-1, 0, 0] and k2["cell"][0].tolist() == [-1, 0, 0] and k2["key"].max() == 3


def test_a_planes_cluster_quadric_vanishes_on_the_plane():
    rng = np.random.default_rng(1)
    n = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    e1 = np.cross(n, [1.0, 0, 0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    uv = rng.uniform(-0.4, 0.4, (30, 2))
    base = np.array([5.0, 5.0, 5.0]) + 0.1 * n
    v = (base[None] + uv[:, :1] * e1[None] + uv[:, 1:] * e2[None]).astype(np.float32)
    t = rng.integers(0, 30, (40, 3))
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    res = np_simplify(v, t, 10.0, origin=(0.0, 0.0, 0.0))                  # one cell holds everything
    assert res["clusters"]["C"] == 1 and res["report"]["faces_out"] == 0
    q = res["quadric"][0]
    on_plane = v.astype(np.float64) - res["clusters"]["centre"][0][None]
    off_plane = on_plane + 0.05 * n[None]
    scale = q[0] + q[3] + q[5]                                             # sum |n|^2: the error of a point at distance 1
    assert (np.abs(quadric_error(q, on_plane)) <= 1e-10 * scale).all()    # (the fp32 vertices are off the plane by ~1e-7)
    assert np.allclose(quadric_error(q, off_plane), 0.05 ** 2 * scale, rtol=1e-3)


def test_three_orthogonal_planes_are_placed_at_their_corner():
    # the corner of a rotated cube at `corner`, three faces fanned into triangles; the members' mean is far from it
    corner = np.array([2.0, 2.1, 1.9])
    axes = _rot(np.eye(3))
    v, t = [corner], []
    for a in range(3):
        e1, e2 = axes[(a + 1) % 3], axes[(a + 2) % 3]
        b = len(v)
        v += [corner + 0.9 * e1, corner + 0.9 * e1 + 0.9 * e2, corner + 0.9 * e2]
        t += [[0, b, b + 1], [0, b + 1, b + 2]]
    v = np.array(v, np.float32)
    res = np_simplify(v, np.array(t), 4.0, origin=(0.0, 0.0, 0.0), eps=1e-6)
    k = res["clusters"]
    assert k["C"] == 1
    x, status = np_place(res["quadric"], res["mean"], 4.0, eps=1e-6)
    assert status[0] == 0 and np.abs(k["centre"][0] + x[0] - corner).max() < 1e-4
    assert np.linalg.norm(res["mean"][0] + k["centre"][0] - corner) > 0.5
    # the regulariser pulls towards the mean, continuously: at eps = 1e-3 the corner is still found to about a thousandth of the way
    x3, _ = np_place(res["quadric"], res["mean"], 4.0, eps=1e-3)
    assert np.abs(k["centre"][0] + x3[0] - corner).max() < 5e-3


def test_flat_and_empty_quadrics_fall_back_to_the_mean():
    m = np.array([[0.1, -0.2, 0.3]])
    x, status = np_place(np.zeros((1, 10)), m, 1.0)
    assert status[0] == 1 and np.array_equal(x, m)
    # a plane far from the mean: the minimiser leaves the cell
    q = np.zeros((1, 10))
    q[0, 0], q[0, 6], q[0, 9] = 1.0, -3.0, 9.0                              # (x - 3)^2
    x, status = np_place(q, m, 1.0)
    assert status[0] == 2 and np.array_equal(x, m)


def test_hand_made_list_gives_the_expected_output():
    v, t, h, origin = hand_made()
    for placement in ("mean", "quadric"):
        res = np_simplify(v, t, h, origin, placement=placement)
        assert np.array_equal(res["triangles"], HAND_TRIANGLES)
        assert np.array_equal(res["vertex_cluster"], HAND_VERTEX_CLUSTER)
        assert {k: res["report"][k] for k in HAND_REPORT} == HAND_REPORT
    res = np_simplify(v, t, h, origin, placement="mean")
    v64 = v.astype(np.float64)
    want = np.stack([(v64[0] + v64[3]) / 2, (v64[1] + v64[7]) / 2, v64[2], v64[4]])
    assert np.array_equal(res["vertices"], want)


def test_two_sheets_closer_than_a_cell_stay_as_opposite_pairs():
    v, t = two_sheets()
    res = np_simplify(v, t, 2.0)
    tri = res["triangles"]
    assert len(res["vertices"]) == 25 and len(tri) == 64
    as_set = {tuple(x) for x in tri.tolist()}
    canon = lambda a: tuple(np.roll(a, -int(np.argmin(a))))
    assert len({canon(x) for x in tri}) == 64
    assert all(canon(x[::-1]) in {canon(y) for y in tri} for x in tri) and len(as_set) == 64


@pytest.mark.parametrize("name,h,want", [("sphere", 2.5, (170, 336)), ("sphere", 4.0, (72, 140)), ("torus", 2.5, (140, 280)), ("torus", 4.0, (62, 124))])
def test_fixture_counts_and_euler_characteristic(name, h, want):
    v, t = surface(name)
    res = np_simplify(v, t, h, ORIGIN)
    assert (len(res["vertices"]), len(res["triangles"])) == want
    assert len(res["vertices"]) - len(res["triangles"]) // 2 == (2 if name == "sphere" else 0)


def test_quadric_placement_beats_the_mean_on_the_fixtures():
    for name in ("sphere", "torus", "box"):
        v, t = surface(name)
        for h in CELL_SIZES:
            q, m = np_simplify(v, t, h, ORIGIN), np_simplify(v, t, h, ORIGIN, placement="mean")
            eq, em = np.abs(sdf(name, to_world(q["vertices"]))).mean(), np.abs(sdf(name, to_world(m["vertices"]))).mean()
            assert eq < em * (0.5 if (name, h) == ("box", 4.0) else 1.0), (name, h, eq / em)
            # the fixture condition of the GPU test: no coordinate near the fallback's threshold
            assert (np.abs(np.abs(q["x"]) - 0.5 * h) > 1e-6 * h).all()


# ---- the interface, as far as it shows without a device ---------------------------------------------------------------------------
def test_library_declares_and_exports_the_simplification_entry_points():
    from vdn_hip import build, lib
    names = ("vdn_simplify_mark", "vdn_simplify_keys", "vdn_simplify_records", "vdn_segment_mean", "vdn_cluster_quadrics", "vdn_cluster_place")
    for n in names:
        assert len(lib.FUNCTIONS[n]) == 2
    if os.path.exists(lib.LIB_PATH):
        for n in names:
            assert hasattr(lib.load(), n)
    assert build.PER_FILE_FLAGS["mesh_simplify.hip"] == ["-ffp-contract=off"]              # the sums are specified to the bit
    for s in ("VdnSimplifyArgs", "VdnSegmentMeanArgs", "VdnClusterQuadricArgs"):
        assert s in lib.STRUCTS


def test_validate_mesh_defaults_to_no_simplification():
    import inspect
    from vdn_train import mesh_simplify, validate
    for fn in (validate.validate_mesh, validate.validate_scene_mesh):
        assert inspect.signature(fn).parameters["simplify"].default is None
    p = inspect.signature(mesh_simplify.simplify_mesh).parameters
    assert p["cell_size"].default is None and p["target_faces"].default is None and p["placement"].default == "quadric"
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int64))             # neither size nor budget
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int64), cell_size=1.0, target_faces=5)


def test_command_line_tool_parses():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "simplify_mesh.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--cell-size", "--target-faces", "--placement", "--eps"):
        assert opt in r.stdout
    for args in (["a.ply", "b.ply"], ["a.ply", "b.ply", "--cell-size", "1", "--target-faces", "5"]):     # exactly one of the two
        assert subprocess.run([sys.executable, tool] + args, capture_output=True, text=True).returncode == 2
