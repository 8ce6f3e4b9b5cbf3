"""Numpy restatement of the adaptive simplification (include/vdn_render.h: vdn_octree_*; vdn_hip/mesh.py: cluster_octree, select_octree,
simplify_mesh(tolerance=..)) and its own checks; tests/test_gpu_mesh_octree.py holds the kernels to it. np_octree moves
and adds the children's records in the header's order (slot by slot, every product and sum on its own), so quadric, mean, count and
trace can be compared to the bit; the placement is np_place of test_mesh_simplify_cpu (np.linalg.solve), so position and error
agree to rounding only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_mesh_simplify_cpu as M

ORIGIN = M.ORIGIN
ORIGIN_INSIDE = (11.37, 9.21, 12.13)         # among the fixtures' vertices: negative cell indices on every axis
SHAPES = ("sphere", "torus", "box", "bump")
H0, L = 1.5, 2                               # the 24^3 fixtures' finest cell and levels
TOL = 0.1                                    # the tolerance of the GPU file's fixtures
_CACHE = {}


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def sdf(name, p):
    """M.sdf plus the bump: a slab |z| <= 0.25, max(|x|, |y|) <= 0.8 with a ball of radius 0.3 about (0.2, -0.1, 0.25) on it"""
    if name != "bump":
        return M.sdf(name, p)
    p = np.asarray(p, np.float64)
    slab = np.maximum(np.abs(p[:, 2]) - 0.25, np.maximum(np.abs(p[:, 0]), np.abs(p[:, 1])) - 0.8)
    return np.minimum(slab, np.linalg.norm(p - np.array([0.2, -0.1, 0.25])[None], axis=1) - 0.3)


def surface(name, R=24):
    """-> (vertices fp32 in lattice-index coordinates, triangles int64) of oracle.marching_cubes on the R^3 lattice over [-1, 1]^3"""
    if (name, R) not in _CACHE:
        if R == M.R and name != "bump":
            _CACHE[(name, R)] = M.surface(name)
        else:
            from oracle import marching_cubes
            g = np.linspace(-1.0, 1.0, R)
            pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
            v, t = marching_cubes.marching_cubes(sdf(name, pts).reshape(R, R, R).astype(np.float32), 0.0)
            _CACHE[(name, R)] = (v.astype(np.float32), t.astype(np.int64))
    return _CACHE[(name, R)]


def surface_error(name, R, vertices, triangles, n=40000, seed=0):
    """(mean, rms) of |field| in lattice spacings at n area-weighted samples of a mesh in lattice-index coordinates"""
    rng = np.random.default_rng(seed)
    p = np.asarray(vertices, np.float64)[triangles]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    f = rng.choice(len(triangles), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    x = (1 - r1)[:, None] * p[f, 0] + (r1 * (1 - r2))[:, None] * p[f, 1] + (r1 * r2)[:, None] * p[f, 2]
    d = np.abs(sdf(name, x / (R - 1.0) * 2.0 - 1.0)) * (R - 1.0) / 2.0
    return d.mean(), np.sqrt((d ** 2).mean())


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def np_measure(q, x):
    """-> (error, trace) of quadrics [C,10] at x [C,3], in the header's order; a NaN error becomes 0"""
    Ax = [(q[:, i] * x[:, 0] + q[:, j] * x[:, 1]) + q[:, k] * x[:, 2] for i, j, k in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
    with np.errstate(invalid="ignore"):
        e = (((x[:, 0] * Ax[0] + x[:, 1] * Ax[1]) + x[:, 2] * Ax[2]) + 2.0 * ((q[:, 6] * x[:, 0] + q[:, 7] * x[:, 1]) + q[:, 8] * x[:, 2])) + q[:, 9]
        return np.where(e > 0.0, e, 0.0), (q[:, 0] + q[:, 3]) + q[:, 5]


def _level(cell, quadric, mean, count, h, origin, eps):
    centre = np.asarray(origin, np.float64)[None] + (cell.astype(np.float64) + 0.5) * h
    x, status = M.np_place(quadric, mean, h, eps)
    error, trace = np_measure(quadric, x)
    return {"cell": cell, "centre": centre, "quadric": quadric, "mean": mean, "count": count, "x": x, "position": centre + x, "status": status,
            "error": error, "trace": trace, "h": h}


def np_octree(v32, t, h0, levels, origin=None, eps=1e-3):
    """-> dict(vertex_cluster [V] (level 0), origin, levels: a list of levels + 1 dicts with cell, centre, quadric, mean, count, x,
    position, status, error, trace, h, parent (below the top), children [C,8] (above level 0)), clusters: np_clusters' dict"""
    t = np.asarray(t, np.int64)
    k = M.np_clusters(v32, t, h0, origin)
    C, vc = k["C"], k["vertex_cluster"]
    tree = {"vertex_cluster": vc, "origin": k["origin"], "clusters": k, "levels": []}
    if C == 0:
        return tree
    lv = _level(k["cell"], M.np_quadrics(v32, t, k), M.np_means(v32, vc, C) - k["centre"], np.bincount(vc[vc >= 0], minlength=C), h0,
                k["origin"], eps)
    tree["levels"].append(lv)
    for l in range(1, levels + 1):
        prev, h = lv, h0 * 2.0 ** l
        up = prev["cell"] >> 1                                               # (numpy's shift of a signed integer is the floor)
        lo = up.min(axis=0)
        d = up.max(axis=0) - lo + 1
        key, parent = np.unique((up[:, 0] - lo[0]) + d[0] * ((up[:, 1] - lo[1]) + d[1] * (up[:, 2] - lo[2])), return_inverse=True)
        cell = np.stack([key % d[0], (key // d[0]) % d[1], key // (d[0] * d[1])], axis=1) + lo[None]
        P = len(key)
        prev["parent"] = parent
        slot = (prev["cell"][:, 0] & 1) + 2 * (prev["cell"][:, 1] & 1) + 4 * (prev["cell"][:, 2] & 1)
        children = np.full((P, 8), -1, np.int64)
        children[parent, slot] = np.arange(len(parent))
        quadric, S, count = np.zeros((P, 10)), np.zeros((P, 3)), np.zeros(P, np.int64)
        for s in range(8):
            p = np.nonzero(children[:, s] >= 0)[0]
            c = children[p, s]
            q, m, n = prev["quadric"][c], prev["mean"][c], prev["count"][c]
            dd = np.array([0.25 * h if (s >> a) & 1 else -(0.25 * h) for a in range(3)])
            Ad = [(q[:, i] * dd[0] + q[:, j] * dd[1]) + q[:, kk] * dd[2] for i, j, kk in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
            moved = np.empty_like(q)
            moved[:, :6] = q[:, :6]
            for a in range(3):
                moved[:, 6 + a] = q[:, 6 + a] - Ad[a]
            moved[:, 9] = (q[:, 9] - 2.0 * ((q[:, 6] * dd[0] + q[:, 7] * dd[1]) + q[:, 8] * dd[2])) + ((dd[0] * Ad[0] + dd[1] * Ad[1]) + dd[2] * Ad[2])
            quadric[p] = quadric[p] + moved
            count[p] = count[p] + n
            S[p] = S[p] + n.astype(np.float64)[:, None] * (m + dd[None])
        lv = _level(cell, quadric, S / count.astype(np.float64)[:, None], count, h, k["origin"], eps)
        lv["children"] = children
        tree["levels"].append(lv)
    return tree


def np_select(levels, tolerance):
    """levels: dicts with error, trace, children (above level 0) and parent (below the top) -> (level [C0] uint8, node [C0] int64,
    solid: one bool array per level, accept: likewise)"""
    tol2 = float(tolerance) * float(tolerance)
    solid, accept = [np.ones(len(levels[0]["error"]), bool)], [np.ones(len(levels[0]["error"]), bool)]
    for l in range(1, len(levels)):
        tr, ch = levels[l]["trace"], levels[l]["children"]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = (tr > 0.0) & (tr < np.inf) & (levels[l]["error"] < tol2 * tr)
        kids = np.where(ch >= 0, solid[l - 1][np.maximum(ch, 0)], True).all(axis=1)
        accept.append(acc)
        solid.append(acc & kids)
    C0 = len(solid[0])
    level, node = np.zeros(C0, np.uint8), np.arange(C0, dtype=np.int64)
    for c in range(C0):
        n, l = c, 0
        while l + 1 < len(levels) and solid[l + 1][levels[l]["parent"][n]]:
            n, l = int(levels[l]["parent"][n]), l + 1
        level[c], node[c] = l, n
    return level, node, solid, accept


def np_octree_simplify(v32, t, h0, levels, tolerance, origin=None, eps=1e-3, attributes=(), tree=None):
    """-> np_simplify's dict for the adaptive mode, plus level [V'], nodes_per_level, tree, select = (level, node) per level-0 cluster"""
    t = np.asarray(t, np.int64)
    tree = tree or np_octree(v32, t, h0, levels, origin, eps)
    lv, vc0 = tree["levels"], tree["vertex_cluster"]
    level, node, _, _ = np_select(lv, tolerance)
    start = np.concatenate([[0], np.cumsum([len(x["cell"]) for x in lv])])
    used, inv = np.unique(start[level.astype(np.int64)] + node, return_inverse=True)          # level-major numbering
    C = len(used)
    vmap = np.where(vc0 >= 0, inv[np.maximum(vc0, 0)], -1)
    k = {"C": C, "vertex_cluster": vmap, "live": tree["clusters"]["live"]}
    emit, cc, counts = M.np_emit(t, k)
    position, status = np.concatenate([x["position"] for x in lv])[used], np.concatenate([x["status"] for x in lv])[used]
    node_level = (np.searchsorted(start, used, side="right") - 1).astype(np.uint8)
    kept = np.unique(cc[emit].reshape(-1))
    new = np.full(C + 1, -1, np.int64)
    new[kept] = np.arange(len(kept))
    report = dict(counts, vertices_in=len(v32), faces_in=len(t), clusters=C, vertices_out=len(kept), faces_out=int(emit.sum()))
    return {"vertices": position[kept], "triangles": new[cc[emit]], "vertex_cluster": new[vmap], "status": status[kept], "level": node_level[kept],
            "attributes": [M.np_means(a, vmap, C)[kept] for a in attributes], "report": report, "tree": tree, "select": (level, node),
            "nodes_per_level": np.bincount(node_level, minlength=len(lv)).tolist(), "node_h": (h0 * 2.0 ** node_level[kept])}


def tree_of(name, R=24, h0=H0, levels=L, origin=ORIGIN):
    key = ("tree", name, R, h0, levels, origin)
    if key not in _CACHE:
        v, t = surface(name, R)
        _CACHE[key] = np_octree(v, t, h0, levels, origin)
    return _CACHE[key]


def threshold_ratios(tree, tolerance):
    """error / (tolerance^2 trace) of every node above level 0 with a positive trace"""
    out = [lv["error"][lv["trace"] > 0] / (tolerance ** 2 * lv["trace"][lv["trace"] > 0]) for lv in tree["levels"][1:]]
    return np.concatenate(out)


# ---- cells and propagation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [ORIGIN, ORIGIN_INSIDE])
@pytest.mark.parametrize("name", SHAPES)
def test_level_cells_are_the_uniform_cells_of_the_doubled_size(name, origin):
    v, t = surface(name)
    tree = tree_of(name, origin=origin)
    # (the fixtures live in [0, 23]^3: ORIGIN lies below them, ORIGIN_INSIDE among them, where the floor of the shift matters)
    assert (tree["levels"][0]["cell"].min() < 0) == (origin is ORIGIN_INSIDE)
    member = tree["vertex_cluster"]
    for l in range(L + 1):
        k = M.np_clusters(v, t, H0 * 2.0 ** l, origin)
        assert np.array_equal(tree["levels"][l]["cell"], k["cell"]) and np.array_equal(tree["levels"][l]["centre"], k["centre"])
        assert np.array_equal(member, k["vertex_cluster"])
        assert np.array_equal(tree["levels"][l]["count"], np.bincount(member[member >= 0], minlength=k["C"]))
        if l < L:
            member = np.where(member >= 0, tree["levels"][l]["parent"][np.maximum(member, 0)], -1)


@pytest.mark.parametrize("origin", [ORIGIN, ORIGIN_INSIDE])
@pytest.mark.parametrize("name", SHAPES)
def test_propagated_quadrics_and_means_equal_the_recomputed_ones(name, origin):
    v, t = surface(name)
    tree = tree_of(name, origin=origin)
    for l in (1, 2):
        h = H0 * 2.0 ** l
        k = M.np_clusters(v, t, h, origin)
        q, m = M.np_quadrics(v, t, k), M.np_means(v, k["vertex_cluster"], k["C"]) - k["centre"]
        got = tree["levels"][l]
        eq = (np.abs(got["quadric"] - q) / np.abs(q).max(axis=1, keepdims=True)).max()
        em = np.abs(got["mean"] - m).max() / h
        print("%s level %d: quadric %.2e of the largest entry, mean %.2e cell sizes" % (name, l, eq, em))
        assert eq <= 1e-12 and em <= 1e-12


# ---- end points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_tolerance_zero_is_the_uniform_pass_at_the_finest_size(name):
    v, t = surface(name)
    got, want = np_octree_simplify(v, t, H0, L, 0.0, ORIGIN, tree=tree_of(name)), M.np_simplify(v, t, H0, ORIGIN)
    for key in ("vertices", "triangles", "vertex_cluster", "status"):
        assert np.array_equal(got[key], want[key]), key
    assert got["report"] == want["report"] and (got["level"] == 0).all()


@pytest.mark.parametrize("name", SHAPES)
def test_a_huge_tolerance_is_the_uniform_pass_at_the_coarsest_size(name):
    v, t = surface(name)
    tree = tree_of(name)
    assert all((lv["trace"] > 0).all() for lv in tree["levels"])
    hL = H0 * 2.0 ** L
    got, want = np_octree_simplify(v, t, H0, L, 1e30, ORIGIN, tree=tree), M.np_simplify(v, t, hL, ORIGIN)
    assert np.array_equal(got["triangles"], want["triangles"]) and np.array_equal(got["vertex_cluster"], want["vertex_cluster"])
    err = np.abs(got["vertices"] - want["vertices"]).max() / hL
    print("%s: positions differ by %.2e of the coarsest cell" % (name, err))
    assert err <= 1e-9 and (got["level"] == L).all() and got["report"] == want["report"]


# ---- partition and heredity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_the_selected_nodes_partition_the_referenced_vertices(name):
    v, t = surface(name)
    tree = tree_of(name)
    res = np_octree_simplify(v, t, H0, L, TOL, ORIGIN, tree=tree)
    level, node, solid, _ = np_select(tree["levels"], TOL)
    assert len(set(level.tolist())) > 1                                       # the fixture mixes levels
    vc0 = tree["vertex_cluster"]
    used = tree["clusters"]["used"]
    assert np.array_equal(vc0 >= 0, used)                                    # every referenced vertex has one node, no other has
    lv_of, node_of = level[vc0[used]].astype(np.int64), node[vc0[used]]
    p = v[used].astype(np.float64)
    for l in range(L + 1):
        at = lv_of == l
        h = H0 * 2.0 ** l
        assert np.array_equal(np.floor((p[at] - np.array(ORIGIN)[None]) / h).astype(np.int64), tree["levels"][l]["cell"][node_of[at]])
    for l in range(1, L + 1):                                                 # a solid node's children are solid
        ch = tree["levels"][l]["children"][solid[l]]
        assert solid[l - 1][ch[ch >= 0]].all()
    # a cluster's node is solid, and its parent is not
    for c in range(len(level)):
        l, n = int(level[c]), int(node[c])
        assert solid[l][n] and (l == L or not solid[l + 1][tree["levels"][l]["parent"][n]])
    assert sum(res["nodes_per_level"]) == res["report"]["clusters"]


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------------
HAND_LEVELS = [
    {"error": np.zeros(5), "trace": np.ones(5), "parent": np.array([0, 0, 1, 1, 2])},
    # P0 flat, P1 creased (rms 0.2 > 0.1), P2 flat
    {"error": np.array([1e-4, 0.04, 0.0]), "trace": np.array([1.0, 1.0, 2.0]), "parent": np.array([0, 0, 1]),
     "children": np.array([[0, 1, -1, -1, -1, -1, -1, -1], [-1, -1, 2, -1, -1, 3, -1, -1], [-1, -1, -1, 4, -1, -1, -1, -1]])},
    # Q0 would be accepted (rms 0.05) but its child P1 is not solid; Q1 merges
    {"error": np.array([0.0025, 0.0]), "trace": np.array([1.0, 3.0]),
     "children": np.array([[0, -1, -1, 1, -1, -1, -1, -1], [2, -1, -1, -1, -1, -1, -1, -1]])},
]


def test_hand_made_records_select_as_written():
    level, node, solid, accept = np_select(HAND_LEVELS, 0.1)
    assert accept[1].tolist() == [True, False, True] and accept[2].tolist() == [True, True]
    assert solid[1].tolist() == [True, False, True] and solid[2].tolist() == [False, True]
    assert level.tolist() == [1, 1, 0, 0, 2] and node.tolist() == [0, 0, 2, 3, 1]
    # the inequality is strict: error = tolerance^2 trace is refused
    lv = [dict(x) for x in HAND_LEVELS]
    lv[1] = dict(lv[1], error=np.array([0.25 * 0.25, 0.04, 0.0]))
    assert np_select(lv, 0.25)[3][1].tolist() == [False, True, True]
    # a trace that is not positive and finite is never accepted
    lv[1] = dict(lv[1], trace=np.array([0.0, np.inf, np.nan]), error=np.zeros(3))
    assert np_select(lv, 1e30)[3][1].tolist() == [False, False, False]


def hand_sheets():
    """h0 = 1, two levels, origin 0. Sheet A: the plane z = 0.1 + 0.9 x over [0, 4)^2 (inside the level-2 cell (0, 0, 0)).
    Sheet B over x in [8, 12), y in [0, 2) at z = 0.5 with a ridge of height 0.3 along y between x = 8.25 and 9.75: the level-1
    cell (4, 0, 0) holds the ridge, (5, 0, 0) is flat; both lie in the level-2 cell (2, 0, 0). Vertices at spacing 0.5 from 0.25:
    none on a cell face."""
    def sheet(x0, nx, ny, z):
        i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        x, y = x0 + 0.25 + 0.5 * i.reshape(-1), 0.25 + 0.5 * j.reshape(-1)
        q = (i[:-1, :-1] * ny + j[:-1, :-1]).reshape(-1)
        return np.stack([x, y, z(x)], 1), np.concatenate([np.stack([q, q + ny, q + ny + 1], 1), np.stack([q, q + ny + 1, q + 1], 1)])
    va, ta = sheet(0.0, 8, 8, lambda x: 0.1 + 0.9 * x)
    vb, tb = sheet(8.0, 8, 4, lambda x: 0.5 + 0.6 * np.maximum(0.0, 0.75 - np.abs(x - 9.0)).clip(max=0.5))
    return np.concatenate([va, vb]).astype(np.float32), np.concatenate([ta, tb + len(va)]).astype(np.int64)


def test_hand_made_sheets_merge_where_they_are_flat():
    v, t = hand_sheets()
    tree = np_octree(v, t, 1.0, 2, (0.0, 0.0, 0.0))
    level, node, solid, accept = np_select(tree["levels"], 0.05)
    cell0, cell1, cell2 = (tree["levels"][l]["cell"] for l in range(3))
    in_a = cell0[:, 0] < 4
    assert (level[in_a] == 2).all() and len(set(node[in_a].tolist())) == 1            # the plane: one node at the top
    assert cell2[node[in_a][0]].tolist() == [0, 0, 0]
    ridge = (cell0[:, 0] >= 8) & (cell0[:, 0] < 10)
    flat = cell0[:, 0] >= 10
    assert (level[ridge] == 0).all()                                                  # the creased block stays at the finest cells
    assert (level[flat] == 1).all() and {tuple(cell1[n]) for n in node[flat]} == {(5, 0, 0)}
    p1 = {tuple(c): i for i, c in enumerate(cell1.tolist())}
    r = p1[(4, 0, 0)]
    rms = np.sqrt(tree["levels"][1]["error"][r] / tree["levels"][1]["trace"][r])
    assert rms > 0.05 and not accept[1][r] and solid[1][p1[(5, 0, 0)]]
    top = {tuple(c): i for i, c in enumerate(cell2.tolist())}[(2, 0, 0)]
    assert not solid[2][top] and tree["levels"][2]["children"][top][tree["levels"][2]["children"][top] >= 0].tolist() == [r, p1[(5, 0, 0)]]
    # the plane's error vanishes to rounding at every level
    for l in (1, 2):
        a = tree["levels"][l]["cell"][:, 0] < (4 >> l)
        assert a.any() and (tree["levels"][l]["error"][a] <= 1e-10 * tree["levels"][l]["trace"][a]).all()    # (fp32 vertices: ~1e-7 off the plane)


# ---- quality ----------------------------------------------------------------------------------------------------------------------------
def quality(name, tol, R=48, h0=2.0, levels=2):
    """-> ((faces, rms) of the adaptive mesh, (faces, rms) of the uniform one at h = 4) on the R^3 lattice"""
    key = ("quality", name, tol)
    if key not in _CACHE:
        v, t = surface(name, R)
        a = np_octree_simplify(v, t, h0, levels, tol, ORIGIN)
        u = M.np_simplify(v, t, 4.0, ORIGIN)
        _CACHE[key] = ((len(a["triangles"]), surface_error(name, R, a["vertices"], a["triangles"])[1]),
                       (len(u["triangles"]), surface_error(name, R, u["vertices"], u["triangles"])[1]))
    return _CACHE[key]


@pytest.mark.parametrize("name,tol", [("box", 0.2), ("bump", 0.1)])
def test_adaptive_needs_fewer_faces_for_less_error_on_shapes_with_flat_parts(name, tol):
    (fa, ra), (fu, ru) = quality(name, tol)
    print("%s tol=%g: faces %d / %d = %.2f, rms %.4f / %.4f = %.2f" % (name, tol, fa, fu, fa / fu, ra, ru, ra / ru))
    assert fa < fu and ra <= 0.75 * ru


def test_adaptive_degrades_gracefully_on_the_sphere():
    (fa, ra), (fu, ru) = quality("sphere", 0.1)
    print("sphere tol=0.1: faces %d / %d = %.2f, rms %.4f / %.4f = %.2f" % (fa, fu, fa / fu, ra, ru, ra / ru))
    assert fa <= 1.05 * fu and ra <= 1.05 * ru


# ---- the GPU file's precondition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_no_node_of_the_gpu_fixtures_sits_on_the_threshold(name):
    r = threshold_ratios(tree_of(name), TOL)
    print("%s: nearest error / (tol^2 trace) to 1: %.2e away" % (name, np.abs(r - 1.0).min()))
    assert (np.abs(r - 1.0) > 1e-6).all()


# ---- the interface, as far as it shows without a device -----------------------------------------------------------------------------------
def test_library_declares_and_exports_the_octree_entry_points():
    from vdn_hip import build, lib
    names = ("vdn_octree_merge", "vdn_octree_select", "vdn_octree_assign")
    for n in names:
        assert len(lib.FUNCTIONS[n]) == 2
    if os.path.exists(lib.LIB_PATH):
        for n in names:
            assert hasattr(lib.load(), n)
    for s in ("VdnOctreeMergeArgs", "VdnOctreeSelectArgs", "VdnOctreeAssignArgs"):
        assert s in lib.STRUCTS
    import re
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28       # additive only
    assert build.PER_FILE_FLAGS["mesh_simplify.hip"] == ["-ffp-contract=off"]


def test_front_doors_take_the_new_arguments_and_keep_their_defaults():
    import inspect
    from vdn_hip import mesh
    from vdn_train import mesh_simplify, validate
    for fn in (mesh.simplify_mesh, mesh_simplify.simplify_mesh):
        p = inspect.signature(fn).parameters
        for k in ("tolerance", "levels"):
            assert p[k].default is None and p[k].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (validate.validate_mesh, validate.validate_scene_mesh):
        assert inspect.signature(fn).parameters["simplify"].default is None
    v, t = np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int64)
    for kw in ({"tolerance": 0.1}, {"levels": 2}, {"tolerance": 0.1, "levels": 2},                      # adaptive mode needs the finest cell
               {"cell_size": 1.0, "tolerance": 0.1, "target_faces": 5},                                # a tolerance or a budget, not both
               {"cell_size": 1.0, "tolerance": 0.1, "placement": "mean"}, {"cell_size": 1.0, "tolerance": -1.0},
               {"cell_size": 1.0, "tolerance": 0.1, "levels": 0}, {"cell_size": 1.0, "tolerance": 0.1, "levels": 9},
               {"cell_size": 1.0, "levels": 2}):                                                       # levels alone: no tolerance, no budget
        with pytest.raises(ValueError):
            mesh_simplify.simplify_mesh(v, t, **kw)


def test_command_line_tool_parses_the_new_flags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "simplify_mesh.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--tolerance" in r.stdout and "--levels" in r.stdout
    for args in (["a.ply", "b.ply", "--tolerance", "0.1"], ["a.ply", "b.ply", "--levels", "2"]):        # no finest cell size
        assert subprocess.run([sys.executable, tool] + args, capture_output=True, text=True).returncode == 2
