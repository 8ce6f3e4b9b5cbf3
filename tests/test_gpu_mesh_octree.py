"""Adaptive simplification on the device (csrc/mesh_simplify.hip: vdn_octree_*; vdn_hip/mesh.py: cluster_octree, select_octree,
count_octree_faces, simplify_mesh(tolerance=..); vdn_train/mesh_simplify.py, validate_mesh(simplify=...), tools/simplify_mesh.py)
against the numpy restatement of test_mesh_octree_cpu.py: cells, links and counts exactly; quadric, mean and trace bit for bit (the
model moves and adds the children's records in the kernel's order); positions within 1e-9 of the node's cell size of
np.linalg.solve, as for the uniform pass (test_gpu_mesh_simplify.py); the error within 1e-9 trace h^2, the size of the terms it is
the sum of (x.Ax, 2 b.x and c are each up to ~trace h^2 and cancel)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_mesh_octree_cpu as O
import test_mesh_simplify_cpu as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ("box", "bump", "sphere", "torus")
H0, L, TOL = O.H0, O.L, O.TOL
_CACHE = {}


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def model(name, tol=TOL):
    key = (name, tol)
    if key not in _CACHE:
        v, t = O.surface(name)
        _CACHE[key] = O.np_octree_simplify(v, t, H0, L, tol, O.ORIGIN, tree=O.tree_of(name))
    return _CACHE[key]


def device_tree(name, index_dtype=torch.int64):
    from vdn_hip import mesh
    key = ("tree", name, index_dtype)
    if key not in _CACHE:
        v, t = O.surface(name)
        _CACHE[key] = mesh.cluster_octree(dev(v), dev(t, index_dtype), H0, L, origin=O.ORIGIN)
    return _CACHE[key]


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", SHAPES)
def test_tree_equals_the_model(name, index_dtype):
    want, got = O.tree_of(name), device_tree(name, index_dtype)
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), want["vertex_cluster"]) and list(got["origin"]) == list(O.ORIGIN)
    assert len(got["levels"]) == L + 1
    for l, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        h = H0 * 2.0 ** l
        assert np.array_equal(g["cell"].cpu().numpy(), w["cell"]) and np.array_equal(g["count"].cpu().numpy(), w["count"])
        assert g["count"].dtype == torch.int64 and g["status"].dtype == torch.uint8
        for key in ("quadric", "mean", "trace"):
            assert g[key].dtype == torch.float64 and np.array_equal(bits(g[key]), bits(w[key])), (l, key)
        if l < L:
            assert np.array_equal(g["parent"].cpu().numpy(), w["parent"])
        else:
            assert "parent" not in g
        if l > 0:
            assert np.array_equal(g["children"].cpu().numpy(), w["children"])
        ep = np.abs(g["position"].cpu().numpy() - w["position"]).max() / h
        ee = (np.abs(g["error"].cpu().numpy() - w["error"]) / (w["trace"] * h * h)).max()
        print("%s level %d: position %.2e cell sizes, error %.2e trace h^2" % (name, l, ep, ee))
        assert ep <= 1e-9 and ee <= 1e-9
        # the fallback is a threshold: the fixture keeps every coordinate clear of it (a condition on the fixture, as in 3p)
        assert (np.abs(np.abs(w["x"]) - 0.5 * h) > 1e-6 * h).all()
        assert np.array_equal(g["status"].cpu().numpy(), w["status"])


def test_level_zero_is_the_uniform_stage_bit_for_bit():
    from vdn_hip import mesh
    v, t = O.surface("box")
    tree, cq = device_tree("box"), mesh.cluster_quadrics(dev(v), dev(t), H0, origin=O.ORIGIN)
    uni = mesh.simplify_mesh(dev(v, torch.float64), dev(t), H0, origin=O.ORIGIN)
    assert torch.equal(tree["levels"][0]["quadric"], cq["quadric"]) and torch.equal(tree["levels"][0]["mean"], cq["mean"])
    assert torch.equal(tree["levels"][0]["cell"], cq["cell"])
    new, old = uni["vertex_cluster"], tree["vertex_cluster"]                  # the same placement, vertex by vertex
    assert int((new >= 0).sum()) > 1000
    assert np.array_equal(bits(tree["levels"][0]["position"][old[new >= 0]]), bits(uni["vertices"][new[new >= 0]]))


def test_negative_cell_indices_merge_by_the_floor():
    from vdn_hip import mesh
    v, t = O.surface("torus")
    want = O.tree_of("torus", origin=O.ORIGIN_INSIDE)
    got = mesh.cluster_octree(dev(v), dev(t), H0, L, origin=O.ORIGIN_INSIDE)
    assert want["levels"][0]["cell"].min() < 0
    for g, w in zip(got["levels"], want["levels"]):
        assert np.array_equal(g["cell"].cpu().numpy(), w["cell"])
        assert np.array_equal(bits(g["quadric"]), bits(w["quadric"])) and np.array_equal(bits(g["mean"]), bits(w["mean"]))


# ---- selection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_selection_equals_the_model(name):
    from vdn_hip import mesh
    assert (np.abs(O.threshold_ratios(O.tree_of(name), TOL) - 1.0) > 1e-6).all()      # the precondition: no node on the threshold
    level, node = mesh.select_octree(device_tree(name), TOL)
    want_level, want_node = model(name)["select"]
    assert level.dtype == torch.uint8 and node.dtype == torch.int64
    assert np.array_equal(level.cpu().numpy(), want_level) and np.array_equal(node.cpu().numpy(), want_node)
    assert len(set(want_level.tolist())) > 1
    assert mesh.count_octree_faces(device_tree(name), TOL) == len(model(name)["triangles"])


# ---- the simplified mesh ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", SHAPES)
def test_adaptive_mesh_equals_the_model(name, index_dtype):
    from vdn_hip import mesh
    v, t = O.surface(name)
    want = model(name)
    got = mesh.simplify_mesh(dev(v, torch.float64), dev(t, index_dtype), H0, origin=O.ORIGIN, tolerance=TOL, levels=L)
    assert got["vertices"].dtype == torch.float64 and got["triangles"].dtype == index_dtype and got["level"].dtype == torch.uint8
    for key in ("triangles", "vertex_cluster", "status", "level"):
        assert np.array_equal(got[key].cpu().numpy(), want[key]), key
    err = (np.abs(got["vertices"].cpu().numpy() - want["vertices"]).max(axis=1) / want["node_h"]).max()
    print("%s: max |position - model| = %.3e of the node's cell" % (name, err))
    assert err <= 1e-9
    rep = got["report"]
    assert {k: rep[k] for k in want["report"]} == want["report"]
    assert (rep["tolerance"], rep["levels"], rep["cell_size"], rep["nodes_per_level"]) == (TOL, L, H0, want["nodes_per_level"])
    assert rep["status"] == {str(k): int((want["status"] == k).sum()) for k in range(3)}
    again = mesh.simplify_mesh(dev(v, torch.float64), dev(t, index_dtype), H0, origin=O.ORIGIN, tolerance=TOL, levels=L)
    for key in ("vertices", "triangles", "vertex_cluster", "status", "level"):                        # two calls: the same bits
        assert torch.equal(got[key], again[key])
    # without a tolerance nothing is new
    uni = mesh.simplify_mesh(dev(v), dev(t, index_dtype), H0, origin=O.ORIGIN)
    assert "level" not in uni and not {"tolerance", "levels", "nodes_per_level"} & set(uni["report"])


@pytest.mark.parametrize("name", SHAPES)
def test_end_points_are_the_uniform_passes_of_the_library(name):
    from vdn_hip import mesh
    v, t = O.surface(name)
    dv, dt = dev(v, torch.float64), dev(t)
    fine, zero = mesh.simplify_mesh(dv, dt, H0, origin=O.ORIGIN), mesh.simplify_mesh(dv, dt, H0, origin=O.ORIGIN, tolerance=0.0, levels=L)
    for key in ("triangles", "vertex_cluster", "status"):
        assert torch.equal(fine[key], zero[key])
    assert np.array_equal(bits(fine["vertices"]), bits(zero["vertices"])) and int(zero["level"].max()) == 0
    assert {k: zero["report"][k] for k in fine["report"]} == fine["report"]
    hL = H0 * 2.0 ** L
    coarse, huge = mesh.simplify_mesh(dv, dt, hL, origin=O.ORIGIN), mesh.simplify_mesh(dv, dt, H0, origin=O.ORIGIN, tolerance=1e30, levels=L)
    for key in ("triangles", "vertex_cluster", "status"):
        assert torch.equal(coarse[key], huge[key])
    err = float((coarse["vertices"] - huge["vertices"]).abs().max()) / hL
    print("%s: coarsest end point within %.2e cell sizes" % (name, err))
    assert err <= 1e-9 and int(huge["level"].min()) == L


def test_attributes_are_the_segmented_mean_over_the_final_map():
    from vdn_hip import mesh
    v, t = O.surface("bump")
    rng = np.random.default_rng(3)
    fa = rng.standard_normal((len(v), 3)).astype(np.float32)
    ua = rng.integers(0, 256, (len(v), 2)).astype(np.uint8)
    want = O.np_octree_simplify(v, t, H0, L, TOL, O.ORIGIN, attributes=[fa, ua], tree=O.tree_of("bump"))
    got = mesh.simplify_mesh(dev(v), dev(t), H0, origin=O.ORIGIN, tolerance=TOL, levels=L, attributes=[dev(fa, torch.float64), dev(ua)])
    a64, a8 = got["attributes"]
    assert a64.dtype == torch.float64 and np.array_equal(bits(a64), bits(want["attributes"][0]))
    assert a8.dtype == torch.uint8 and np.array_equal(a8.cpu().numpy(), np.rint(want["attributes"][1]).astype(np.uint8))


# ---- quality, with the kernels in the loop ------------------------------------------------------------------------------------------------
def _device_quality(name, tol, R=48):
    """-> ((faces, rms) adaptive at h0 = 2, two levels; (faces, rms) uniform at h = 4): device marching cubes, device simplification,
    device surface samples (about 40 000), the analytic field at them in lattice spacings"""
    from vdn_hip import mesh
    g = np.linspace(-1.0, 1.0, R)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    v, t = mesh.marching_cubes(dev(O.sdf(name, pts).reshape(R, R, R).astype(np.float32)), 0.0)
    out = []
    for kw in ({"cell_size": 2.0, "tolerance": tol, "levels": 2}, {"cell_size": 4.0}):
        res = mesh.simplify_mesh(v, t, kw.pop("cell_size"), origin=O.ORIGIN, **kw)
        area = float(mesh.triangle_areas(res["vertices"], res["triangles"]).sum())
        p = mesh.sample_surface(res["vertices"], res["triangles"], (area / 40000.0) ** 0.5)[0].cpu().numpy().astype(np.float64)
        d = np.abs(O.sdf(name, p / (R - 1.0) * 2.0 - 1.0)) * (R - 1.0) / 2.0
        out.append((int(res["triangles"].shape[0]), float(np.sqrt((d ** 2).mean()))))
    return out


@pytest.mark.parametrize("name,tol", [("box", 0.2), ("bump", 0.1), ("sphere", 0.1)])
def test_quality_holds_with_the_kernels_in_the_loop(name, tol):
    (fa, ra), (fu, ru) = _device_quality(name, tol)
    print("%s tol=%g: faces %d / %d = %.2f, rms %.4f / %.4f = %.2f" % (name, tol, fa, fu, fa / fu, ra, ru, ra / ru))
    if name == "sphere":
        assert fa <= 1.05 * fu and ra <= 1.05 * ru
    else:
        assert fa < fu and ra <= 0.75 * ru


# ---- the front doors ----------------------------------------------------------------------------------------------------------------------
def test_target_faces_finds_the_smallest_tolerance_that_fits():
    from vdn_hip import mesh
    from vdn_train import mesh_simplify
    v, t = O.surface("box")
    res = mesh_simplify.simplify_mesh(v, t, cell_size=H0, levels=L, target_faces=300, origin=O.ORIGIN)
    rep = res["report"]
    assert isinstance(res["vertices"], np.ndarray) and isinstance(res["level"], np.ndarray) and res["level"].dtype == np.uint8
    assert len(res["triangles"]) == rep["faces_out"] <= 300 and 2 <= len(rep["tried"]) <= mesh_simplify.TARGET_PASSES
    tried = sorted(rep["tried"])
    at = [x for x, _ in tried].index(rep["tolerance"])
    assert tried[at][1] == rep["faces_out"] and at > 0 and tried[at - 1][1] > 300
    assert all(n > 300 for x, n in tried if x < rep["tolerance"])
    same = mesh_simplify.simplify_mesh(v, t, cell_size=H0, levels=L, tolerance=rep["tolerance"], origin=O.ORIGIN)
    assert np.array_equal(same["vertices"], res["vertices"]) and np.array_equal(same["triangles"], res["triangles"])
    # a budget the finest cells already meet stops after one count; one the coarsest cells miss is an error that says what to do
    assert len(mesh_simplify.simplify_mesh(v, t, cell_size=H0, levels=L, target_faces=10 ** 9)["report"]["tried"]) == 1
    coarsest = mesh.count_simplified_faces(dev(v), dev(t), H0 * 2.0 ** L, origin=O.ORIGIN)
    with pytest.raises(ValueError, match="levels or cell_size"):
        mesh_simplify.simplify_mesh(v, t, cell_size=H0, levels=L, target_faces=coarsest - 1, origin=O.ORIGIN)


def test_argument_errors_and_the_empty_mesh():
    from vdn_hip import mesh
    from vdn_train import mesh_simplify
    v, t = O.surface("sphere")
    dv, dt = dev(v), dev(t)
    for kw in ({"tolerance": -0.1}, {"tolerance": float("nan")}, {"tolerance": "x"}, {"tolerance": 0.1, "levels": 0},
               {"tolerance": 0.1, "levels": 9}, {"tolerance": 0.1, "levels": 1.5}, {"levels": 2}, {"tolerance": 0.1, "placement": "mean"}):
        with pytest.raises(ValueError):
            mesh.simplify_mesh(dv, dt, H0, **kw)
    for bad_levels in (0, 9, 2.5, None):
        with pytest.raises(ValueError):
            mesh.cluster_octree(dv, dt, H0, bad_levels)
    with pytest.raises(ValueError):
        mesh.cluster_octree(torch.from_numpy(v), torch.from_numpy(t), H0, L)       # CPU tensors
    with pytest.raises(ValueError):
        mesh.cluster_octree(dv, dt, 1e308, 8)                                      # the coarsest edge overflows
    with pytest.raises(ValueError):
        mesh.select_octree(device_tree("sphere"), -1.0)
    with pytest.raises(ValueError):
        mesh.simplify_mesh(dv, dt, H0, tolerance=0.1, levels=3, tree=device_tree("sphere"))            # a tree of two levels
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, t, tolerance=0.1)
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, t, cell_size=H0, tolerance=0.1, target_faces=100)
    # nothing was corrupted on the way
    assert np.array_equal(mesh.simplify_mesh(dv, dt, H0, origin=O.ORIGIN, tolerance=TOL, levels=L)["triangles"].cpu().numpy(),
                          model("sphere")["triangles"])
    nan = torch.full_like(dv, float("nan"))
    for vv, tt in ((dv, dt[:0]), (dv[:0], dt[:0]), (nan, dt), (dv, dt[:0].int())):
        res = mesh.simplify_mesh(vv, tt, H0, tolerance=TOL, attributes=[vv])
        assert res["vertices"].shape == (0, 3) and res["triangles"].shape == (0, 3) and res["triangles"].dtype == tt.dtype
        assert res["level"].shape == (0,) and res["level"].dtype == torch.uint8 and (res["vertex_cluster"] == -1).all()
        assert res["report"]["nodes_per_level"] == [0] * 4 and res["report"]["levels"] == 3 and res["report"]["faces_out"] == 0
        tree = mesh.cluster_octree(vv, tt, H0, L)
        assert len(tree["levels"]) == L + 1 and all(x["quadric"].shape == (0, 10) for x in tree["levels"])
        assert mesh.select_octree(tree, TOL)[0].shape == (0,) and mesh.count_octree_faces(tree, TOL) == 0
    e = mesh_simplify.simplify_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), cell_size=1.0, levels=2, target_faces=10)
    assert e["vertices"].shape == (0, 3) and e["level"].shape == (0,)


def test_validate_mesh_and_the_command_line_tool(tmp_path):
    from vdn_train import factory, mesh_simplify, meshio, synth, validate
    rend = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(0, variance=0.4), precision="bf16")
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    cell = 2.0 / 23                                                          # one lattice spacing, in object space
    kw = {"cell_size": cell, "tolerance": 0.1 * cell, "levels": 2}
    path, Vs, Fs = validate.validate_mesh(rend, lo, hi, str(tmp_path / "adaptive.ply"), resolution=24, vertex_colors=False,
                                          vertex_normals=False, simplify=kw)
    got = meshio.read_ply(path)
    v, t = rend.extract_geometry(lo, hi, resolution=24, threshold=0.0)
    res = mesh_simplify.simplify_mesh(v, t, **kw)
    assert 0 < Fs == len(res["triangles"]) < len(t) and Vs == len(res["vertices"]) and int(res["level"].max()) > 0
    assert np.array_equal(got["triangles"], res["triangles"]) and np.array_equal(got["vertices"], res["vertices"].astype(np.float32))
    # the tool, on the file of a fixture
    v, t = O.surface("bump")
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    meshio.write_ply(src, v, t)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "simplify_mesh.py"), src, out, "--cell-size", str(H0), "--tolerance", str(TOL),
                        "--levels", str(L)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    want = O.np_octree_simplify(v, t, H0, L, TOL)                            # (the default origin: the box's minimum corner)
    assert (np.abs(O.threshold_ratios(want["tree"], TOL) - 1.0) > 1e-6).all()
    assert np.array_equal(meshio.read_ply(out)["triangles"], want["triangles"])
    assert (rep["faces_out"], rep["levels"], rep["tolerance"], rep["nodes_per_level"]) == (len(want["triangles"]), L, TOL, want["nodes_per_level"])
