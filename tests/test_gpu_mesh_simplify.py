"""Mesh simplification on the device (csrc/mesh_simplify.hip, vdn_hip/mesh.py: cluster_quadrics / simplify_mesh,
vdn_train/mesh_simplify.py, validate_mesh(simplify=...), tools/simplify_mesh.py) against the numpy restatements of
test_mesh_simplify_cpu.py: keys, clusters and triangles exactly, the two segmented sums bit for bit (the model follows the device's
summation order), the placed positions within 1e-9 cell sizes of np.linalg.solve (the system's condition number is at most
1 + 1/eps ~ 1e3 and its right-hand side is formed in cell-local coordinates, so fp64 leaves ~1e-12 cell sizes of error; the bound
keeps three orders of margin and is far below an fp32 ulp of the output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_mesh_simplify_cpu as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS, _CACHE = {}, {}
SHAPES = ("sphere", "torus", "box")


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def model(name, h, placement="quadric"):
    key = (name, h, placement)
    if key not in _MODELS:
        v, t = M.surface(name)
        _MODELS[key] = M.np_simplify(v, t, h, M.ORIGIN, placement=placement)
    return _MODELS[key]


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---- keys, clusters, cells ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("h", M.CELL_SIZES)
@pytest.mark.parametrize("name", SHAPES)
def test_clusters_equal_the_model(name, h, index_dtype):
    from vdn_hip import mesh
    v, t = M.surface(name)
    want = model(name, h)["clusters"]
    got = mesh.cluster_quadrics(dev(v), dev(t, index_dtype), h, origin=M.ORIGIN)
    assert got["vertex_cluster"].dtype == torch.int64 and got["cell"].dtype == torch.int64
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), want["vertex_cluster"])
    assert np.array_equal(got["cell"].cpu().numpy(), want["cell"])
    assert list(got["origin"]) == list(M.ORIGIN)
    # the cell of every clustered vertex is the floor of the division, and the clusters ascend in key order
    vc = want["vertex_cluster"]
    assert np.array_equal(got["cell"].cpu().numpy()[vc[vc >= 0]], want["index"][vc >= 0])
    d, lo = want["dims"], want["lo"]
    rel = got["cell"].cpu().numpy() - lo[None]
    key = rel[:, 0] + d[0] * (rel[:, 1] + d[1] * rel[:, 2])
    assert (np.diff(key) > 0).all()


def test_default_origin_is_the_minimum_corner_of_the_referenced_vertices():
    from vdn_hip import mesh
    v, t = M.surface("torus")
    v = np.concatenate([v, np.array([[-50.0, 3.0, 3.0], [np.inf, 0.0, 0.0]], np.float32)])      # two vertices no triangle uses
    want = M.np_clusters(v, t, 3.0)
    got = mesh.cluster_quadrics(dev(v), dev(t), 3.0)
    assert list(got["origin"]) == v[:-2].astype(np.float64).min(axis=0).tolist()
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), want["vertex_cluster"]) and (want["vertex_cluster"][-2:] == -1).all()
    assert np.array_equal(got["cell"].cpu().numpy(), want["cell"]) and want["cell"].min() == 0


# ---- the two segmented sums: bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", M.CELL_SIZES)
@pytest.mark.parametrize("name", SHAPES)
def test_quadrics_and_means_equal_the_model_bit_for_bit(name, h):
    from vdn_hip import mesh
    v, t = M.surface(name)
    want = model(name, h)
    got = mesh.cluster_quadrics(dev(v), dev(t), h, origin=M.ORIGIN)
    again = mesh.cluster_quadrics(dev(v), dev(t), h, origin=M.ORIGIN)
    assert got["quadric"].dtype == torch.float64 and got["mean"].dtype == torch.float64
    assert np.array_equal(bits(got["quadric"]), bits(want["quadric"]))
    assert np.array_equal(bits(got["mean"]), bits(want["mean"]))
    assert np.array_equal(bits(got["quadric"]), bits(again["quadric"])) and np.array_equal(bits(got["mean"]), bits(again["mean"]))


def test_one_cell_with_the_whole_sphere_goes_through_the_strided_part():
    from vdn_hip import mesh
    v, t = M.surface("sphere")
    want = M.np_simplify(v, t, 64.0, M.ORIGIN)
    assert want["clusters"]["C"] == 1 and len(v) > 1000 and 3 * len(t) > 5000
    got = mesh.cluster_quadrics(dev(v), dev(t), 64.0, origin=M.ORIGIN)
    assert np.array_equal(bits(got["quadric"]), bits(want["quadric"])) and np.array_equal(bits(got["mean"]), bits(want["mean"]))
    res = mesh.simplify_mesh(dev(v), dev(t), 64.0, origin=M.ORIGIN)
    assert res["vertices"].shape == (0, 3) and res["triangles"].shape == (0, 3) and res["report"]["faces_collapsed"] == len(t)
    assert (res["vertex_cluster"] == -1).all()


# ---- positions, status, triangles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("h", M.CELL_SIZES)
@pytest.mark.parametrize("name", SHAPES)
def test_simplified_mesh_equals_the_model(name, h, index_dtype):
    from vdn_hip import mesh
    v, t = M.surface(name)
    want = model(name, h)
    # the fallback is a threshold: the fixture must keep every coordinate clear of it (a condition on the fixture, not on the code)
    assert (np.abs(np.abs(want["x"]) - 0.5 * h) > 1e-6 * h).all()
    got = mesh.simplify_mesh(dev(v, torch.float64), dev(t, index_dtype), h, origin=M.ORIGIN)       # fp64 in, fp64 out
    assert got["vertices"].dtype == torch.float64 and got["triangles"].dtype == index_dtype and got["status"].dtype == torch.uint8
    err = np.abs(got["vertices"].cpu().numpy() - want["vertices"]).max()
    print("%s h=%g: max |position - model| = %.3e cell sizes" % (name, h, err / h))
    assert got["vertices"].shape == want["vertices"].shape and err <= 1e-9 * h
    assert np.array_equal(got["status"].cpu().numpy(), want["status"])
    assert np.array_equal(got["triangles"].cpu().numpy(), want["triangles"])
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), want["vertex_cluster"])
    rep = got["report"]
    assert {k: rep[k] for k in want["report"]} == want["report"] and rep["cell_size"] == h
    assert rep["status"] == {str(k): int((want["status"] == k).sum()) for k in range(3)}
    if h == 2.5:
        assert rep["status"]["2"] >= 2 and rep["status"]["0"] > 0                 # both branches ran
    # fp32 in, fp32 out: the same mesh, rounded
    got32 = mesh.simplify_mesh(dev(v), dev(t, index_dtype), h, origin=M.ORIGIN)
    assert got32["vertices"].dtype == torch.float32
    assert np.array_equal(got32["vertices"].cpu().numpy(), got["vertices"].cpu().numpy().astype(np.float32))
    assert torch.equal(got32["triangles"], got["triangles"])


@pytest.mark.parametrize("name,h,want", [("sphere", 2.5, (170, 336)), ("sphere", 4.0, (72, 140)), ("torus", 2.5, (140, 280)), ("torus", 4.0, (62, 124))])
def test_euler_characteristic_survives(name, h, want):
    from vdn_hip import mesh
    v, t = M.surface(name)
    got = mesh.simplify_mesh(dev(v), dev(t), h, origin=M.ORIGIN)
    V, F = got["vertices"].shape[0], got["triangles"].shape[0]
    assert (V, F) == want and V - F // 2 == (2 if name == "sphere" else 0)


def test_hand_made_triangle_list():
    from vdn_hip import mesh
    v, t, h, origin = M.hand_made()
    for placement in ("quadric", "mean"):
        got = mesh.simplify_mesh(dev(v), dev(t), h, origin=origin, placement=placement)
        assert np.array_equal(got["triangles"].cpu().numpy(), M.HAND_TRIANGLES)        # the reversed one stays, the repeats go
        assert np.array_equal(got["vertex_cluster"].cpu().numpy(), M.HAND_VERTEX_CLUSTER)
        assert {k: got["report"][k] for k in M.HAND_REPORT} == M.HAND_REPORT
    v64 = v.astype(np.float64)
    want = np.stack([(v64[0] + v64[3]) / 2, (v64[1] + v64[7]) / 2, v64[2], v64[4]]).astype(np.float32)
    assert np.array_equal(got["vertices"].cpu().numpy(), want) and got["report"]["status"] == {"0": 4, "1": 0, "2": 0}


def test_two_sheets_closer_than_a_cell_stay_as_opposite_pairs():
    from vdn_hip import mesh
    v, t = M.two_sheets()
    want = M.np_simplify(v, t, 2.0)
    got = mesh.simplify_mesh(dev(v), dev(t), 2.0)
    tri = got["triangles"].cpu().numpy()
    assert got["vertices"].shape[0] == 25 and len(tri) == 64 and np.array_equal(tri, want["triangles"])
    canon = lambda a: tuple(np.roll(a, -int(np.argmin(a))))
    all_of = {canon(x) for x in tri}
    assert len(all_of) == 64 and all(canon(x[::-1]) in all_of for x in tri)        # 32 pairs of opposite orientation


@pytest.mark.parametrize("name", SHAPES)
def test_mean_placement_equals_the_models_means_bit_for_bit(name):
    from vdn_hip import mesh
    v, t = M.surface(name)
    want = model(name, 4.0, "mean")
    got = mesh.simplify_mesh(dev(v, torch.float64), dev(t), 4.0, origin=M.ORIGIN, placement="mean")
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"]))
    assert np.array_equal(got["triangles"].cpu().numpy(), want["triangles"]) and int(got["status"].sum()) == 0


def test_quadric_placement_lies_closer_to_the_surface_than_the_mean():
    from vdn_hip import mesh
    for name in SHAPES:
        v, t = M.surface(name)
        q = mesh.simplify_mesh(dev(v), dev(t), 4.0, origin=M.ORIGIN)["vertices"].cpu().numpy()
        m = mesh.simplify_mesh(dev(v), dev(t), 4.0, origin=M.ORIGIN, placement="mean")["vertices"].cpu().numpy()
        eq, em = np.abs(M.sdf(name, M.to_world(q))).mean(), np.abs(M.sdf(name, M.to_world(m))).mean()
        print("%s: mean |sdf| quadric / mean = %.3f" % (name, eq / em))
        assert eq <= (0.5 if name == "box" else 1.0) * em and (name == "box" or eq < em)


def test_attributes_are_averaged_by_the_same_mean():
    from vdn_hip import mesh
    v, t = M.surface("torus")
    rng = np.random.default_rng(3)
    fa = rng.standard_normal((len(v), 3)).astype(np.float32)
    ua = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    want = M.np_simplify(v, t, 2.5, M.ORIGIN, attributes=[fa, ua])
    got = mesh.simplify_mesh(dev(v), dev(t), 2.5, origin=M.ORIGIN, attributes=[dev(fa, torch.float64), dev(fa), dev(ua)])
    a64, a32, a8 = got["attributes"]
    assert a64.dtype == torch.float64 and np.array_equal(bits(a64), bits(want["attributes"][0]))       # before the cast
    assert a32.dtype == torch.float32 and np.array_equal(a32.cpu().numpy(), want["attributes"][0].astype(np.float32))
    assert a8.dtype == torch.uint8 and np.array_equal(a8.cpu().numpy(), np.rint(want["attributes"][1]).astype(np.uint8))
    # halves go to even: two members 1 and 2 -> 1.5 -> 2, 2 and 3 -> 2.5 -> 2
    vh, th, h, origin = M.hand_made()
    u = np.zeros((8, 2), np.uint8)
    u[0], u[3] = (1, 2), (2, 3)
    out = mesh.simplify_mesh(dev(vh), dev(th), h, origin=origin, attributes=[dev(u)])["attributes"][0]
    assert out[0].tolist() == [2, 2]


# ---- the front door -----------------------------------------------------------------------------------------------------------------
def test_target_faces_finds_the_smallest_size_that_fits():
    from vdn_train import mesh_simplify
    v, t = M.surface("sphere")
    res = mesh_simplify.simplify_mesh(v, t, target_faces=200)
    rep = res["report"]
    assert isinstance(res["vertices"], np.ndarray) and res["vertices"].dtype == np.float32 and res["triangles"].dtype == np.int64
    assert len(res["triangles"]) == rep["faces_out"] <= 200 and 2 <= len(rep["tried"]) <= mesh_simplify.TARGET_PASSES
    tried = sorted(rep["tried"])
    sizes = [h for h, _ in tried]
    at = sizes.index(rep["cell_size"])
    assert tried[at][1] == rep["faces_out"] and at > 0 and tried[at - 1][1] > 200
    assert all(n > 200 for h, n in tried if h < rep["cell_size"])
    same = mesh_simplify.simplify_mesh(v, t, cell_size=rep["cell_size"])
    assert np.array_equal(same["vertices"], res["vertices"]) and np.array_equal(same["triangles"], res["triangles"])
    # a budget the mesh already meets changes nothing but the merges of the finest size
    big = mesh_simplify.simplify_mesh(v, t, target_faces=10 ** 9)
    assert len(big["report"]["tried"]) == 1


def test_numpy_and_tensor_inputs_give_the_same_mesh():
    from vdn_train import mesh_simplify
    v, t = M.surface("box")
    a = mesh_simplify.simplify_mesh(v, t.astype(np.int32), cell_size=4.0, origin=M.ORIGIN, attributes=[v])
    b = mesh_simplify.simplify_mesh(dev(v), dev(t), cell_size=4.0, origin=M.ORIGIN, attributes=[dev(v)])
    assert a["triangles"].dtype == np.int32 and torch.is_tensor(b["vertices"]) and b["triangles"].dtype == torch.int64
    assert np.array_equal(a["vertices"], b["vertices"].cpu().numpy()) and np.array_equal(a["triangles"], b["triangles"].cpu().numpy())
    assert np.array_equal(a["attributes"][0], b["attributes"][0].cpu().numpy())
    # the mean of the positions, carried as an attribute, is the mean placement
    m = mesh_simplify.simplify_mesh(v, t, cell_size=4.0, origin=M.ORIGIN, placement="mean")
    assert np.array_equal(m["vertices"], a["attributes"][0])


def test_argument_errors_and_the_empty_mesh():
    from vdn_hip import mesh
    from vdn_train import mesh_simplify
    v, t = M.surface("sphere")
    dv, dt = dev(v), dev(t)
    for fn in (mesh.simplify_mesh, mesh.cluster_quadrics):
        with pytest.raises(ValueError):
            fn(torch.from_numpy(v), torch.from_numpy(t), 2.5)              # CPU tensors
        with pytest.raises(ValueError):
            fn(dv[:, :2], dt, 2.5)
        with pytest.raises(ValueError):
            fn(dv, dt[:, :2], 2.5)
        with pytest.raises(ValueError):
            fn(dv, dt.float(), 2.5)
        for h in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                fn(dv, dt, h)
        bad = dt.clone()
        bad[7, 1] = len(v)
        with pytest.raises(ValueError):
            fn(dv, bad, 2.5)
        bad[7, 1] = -1
        with pytest.raises(ValueError):
            fn(dv, bad, 2.5)
        with pytest.raises(ValueError):
            fn(dv, dt, 1e-18)                                               # nx ny nz beyond 62 bits
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            mesh.simplify_mesh(dv, dt, 2.5, eps=eps)
    with pytest.raises(ValueError):
        mesh.simplify_mesh(dv, dt, 2.5, placement="median")
    with pytest.raises(ValueError):
        mesh.simplify_mesh(dv, dt, 2.5, attributes=[dv[:-1]])
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, t)
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, t, cell_size=2.5, target_faces=100)
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, t, target_faces=-1)
    # nothing was corrupted on the way
    assert np.array_equal(mesh.simplify_mesh(dv, dt, 4.0, origin=M.ORIGIN)["triangles"].cpu().numpy(), model("sphere", 4.0)["triangles"])
    # empty meshes: no triangles, no vertices, and triangles without a finite corner
    nan = torch.full_like(dv, float("nan"))
    for vv, tt in ((dv, dt[:0]), (dv[:0], dt[:0]), (nan, dt), (dv, dt[:0].int())):
        res = mesh.simplify_mesh(vv, tt, 2.5, attributes=[vv])
        assert res["vertices"].shape == (0, 3) and res["triangles"].shape == (0, 3) and res["triangles"].dtype == tt.dtype
        assert res["attributes"][0].shape == (0, 3) and res["status"].shape == (0,) and (res["vertex_cluster"] == -1).all()
        assert res["report"]["faces_out"] == 0 and res["report"]["faces_non_finite"] == tt.shape[0]
        cq = mesh.cluster_quadrics(vv, tt, 2.5)
        assert cq["quadric"].shape == (0, 10) and cq["cell"].shape == (0, 3) and cq["vertex_cluster"].shape == (vv.shape[0],)
    e = mesh_simplify.simplify_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), target_faces=10)
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3)


# ---- validate_mesh and the command line ------------------------------------------------------------------------------------------------
def _renderer():
    from vdn_train import factory, synth
    if "renderer" not in _CACHE:
        _CACHE["renderer"] = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(0, variance=0.4), precision="bf16")
    return _CACHE["renderer"]


def test_validate_mesh_with_simplification(tmp_path, monkeypatch):
    from vdn_hip import mesh
    from vdn_train import meshio, validate
    rend = _renderer()
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    scale_mat = np.array([[2.5, 0, 0, 0.5], [0, 2.5, 0, -1.0], [0, 0, 2.5, 3.0], [0, 0, 0, 1.0]])
    kw = dict(resolution=24, world_space=True, scale_mat=scale_mat)
    raw_path, V, F = validate.validate_mesh(rend, lo, hi, str(tmp_path / "raw.ply"), **kw)
    none_path, _, _ = validate.validate_mesh(rend, lo, hi, str(tmp_path / "none.ply"), simplify=None, **kw)
    assert open(raw_path, "rb").read() == open(none_path, "rb").read()
    calls, real = [], mesh.shade_points

    def counted(renderer, points, *a, **k):
        calls.append(int(points.shape[0]))
        return real(renderer, points, *a, **k)
    monkeypatch.setattr(mesh, "shade_points", counted)
    cell = 3 * 2.0 / 23                                                      # three lattice spacings, in object space
    path, Vs, Fs = validate.validate_mesh(rend, lo, hi, str(tmp_path / "light.ply"), simplify={"cell_size": cell}, **kw)
    monkeypatch.undo()
    got = meshio.read_ply(path)
    assert (Vs, Fs) == (len(got["vertices"]), len(got["triangles"])) and 0 < Fs < F and 0 < Vs < V
    assert calls == [Vs]                                                     # one shading pass, over the vertices of the file
    assert np.abs(np.linalg.norm(got["normals"].astype(np.float64), axis=1) - 1.0).max() < 1e-5
    # the file's colours and normals are shade_points' at its own (object-space) vertices
    v, t = rend.extract_geometry(lo, hi, resolution=24, threshold=0.0)
    from vdn_train import mesh_simplify
    res = mesh_simplify.simplify_mesh(v, t, cell_size=cell)
    assert np.array_equal(got["triangles"], res["triangles"])
    assert np.array_equal(got["vertices"], (res["vertices"] * scale_mat[0, 0] + scale_mat[:3, 3][None]).astype(np.float32))
    _, g, c = mesh.shade_points(rend, dev(res["vertices"], torch.float32))
    assert np.array_equal(got["colors"], mesh.quantize_colors_bgr(c.cpu().numpy()))
    assert np.array_equal(got["normals"], (g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)).cpu().numpy())
    # bare geometry simplifies too, and a face budget is met
    bare, Vb, Fb = validate.validate_mesh(rend, lo, hi, str(tmp_path / "bare.ply"), vertex_colors=False, vertex_normals=False,
                                          simplify={"target_faces": 300}, **kw)
    b = meshio.read_ply(bare)
    assert b["normals"] is None and b["colors"] is None and 0 < Fb == len(b["triangles"]) <= 300


def test_command_line_tool(tmp_path):
    from vdn_train import meshio
    v, t = M.surface("torus")
    rng = np.random.default_rng(5)
    n = rng.standard_normal((len(v), 3)).astype(np.float32)
    c = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    meshio.write_ply(src, v, t, normals=n, colors=c)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "simplify_mesh.py"), src, out, "--cell-size", "2.5"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    got = meshio.read_ply(out)
    assert (rep["vertices_out"], rep["faces_out"]) == (len(got["vertices"]), len(got["triangles"])) and rep["faces_in"] == len(t)
    assert rep["faces_out"] + rep["faces_collapsed"] + rep["faces_duplicate"] + rep["faces_non_finite"] == len(t)
    want = M.np_simplify(v, t, 2.5, attributes=[n, c])
    assert np.array_equal(got["triangles"], want["triangles"]) and len(got["vertices"]) == len(want["vertices"])
    m = want["attributes"][0].astype(np.float32)
    assert np.allclose(got["normals"], m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), 1e-12), rtol=0, atol=1e-6)
    assert np.array_equal(got["colors"], np.rint(want["attributes"][1]).astype(np.uint8))
