"""Textured meshes on the device (csrc/mesh_texture.hip, vdn_hip/mesh.py: texel_points / project_step / gather_atlas / sample_texture /
bake_texture / render_textured_view, vdn_train/mesh_texture.py, validate_mesh(texture=...), tools/texture_mesh.py) against the integer
and fp64 models of test_mesh_texture_cpu.py: texel points bit for bit, atlases byte for byte, lookups within one fp32 rounding of a
value in [0, 1] (2^-23), Newton steps within 8 fp32 ulps of the points' magnitude."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_mesh_texture_cpu as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def bits32(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).view(np.int32)


def square_atlas(F, n, spare=0):
    """the smallest atlas size that holds F faces in cells of n texels, plus `spare` texels of remainder strip"""
    k = 1
    while k * k < (F + 1) // 2:
        k += 1
    return k * n + spare


def meshes(name):
    v, t = M.icosphere(2 if name == "ico320" else 1)
    if name == "odd":
        t = t[:-1]
    if name == "one":
        t = t[7:8]
    return v, t


# ---- texel points: bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("n", [4, 5, 8])
@pytest.mark.parametrize("name", ["ico80", "ico320", "odd", "one"])
def test_texel_points_equal_the_model_bit_for_bit(name, n, index_dtype):
    from vdn_hip import mesh
    v, t = meshes(name)
    lay = mesh.texture_layout(len(t), square_atlas(len(t), n, spare=3), n)
    want_p, want_f = M.np_texel_points(v, t, n)
    got_p, got_f = mesh.texel_points(dev(v), dev(t, index_dtype), lay)
    assert got_p.dtype == torch.float32 and got_f.dtype == torch.int32 and tuple(got_p.shape) == (lay["points"], 3)
    assert np.array_equal(bits32(got_p), bits32(want_p))
    assert np.array_equal(got_f.cpu().numpy(), want_f)


def test_texel_points_refuse_a_bad_corner_index():
    from vdn_hip import mesh
    v, t = meshes("ico80")
    lay = mesh.texture_layout(len(t), 64, 4)
    for bad_value in (len(v), -1):
        bad = t.copy()
        bad[41, 2] = bad_value
        with pytest.raises(ValueError):
            mesh.texel_points(dev(v), dev(bad), lay)
    got, _ = mesh.texel_points(dev(v), dev(t), lay)                           # nothing was corrupted on the way
    assert np.array_equal(bits32(got), bits32(M.np_texel_points(v, t, 4)[0]))


# ---- the atlas: byte for byte ----------------------------------------------------------------------------------------------------------
def awkward_colors(rows, seed):
    """random rows with values below 0, above 1 and at the rounding thresholds (k +- 0.5) / 255, as fp32"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.2, 1.2, (rows, 3))
    k = rng.integers(0, 256, (rows, 3))
    edge = (k + rng.choice([-0.5, 0.5], (rows, 3))) / 255.0
    edge = edge.astype(np.float32)
    pick = rng.random((rows, 3))
    c = np.where(pick < 0.4, edge, c.astype(np.float32))
    c = np.where((pick >= 0.4) & (pick < 0.45), np.nextafter(edge, np.float32(2.0)), c)          # and one fp32 step to either side
    c = np.where((pick >= 0.45) & (pick < 0.5), np.nextafter(edge, np.float32(-2.0)), c)
    assert c.dtype == np.float32
    return c


@pytest.mark.parametrize("F,S,n", [(5, 13, 4), (80, 38, 5), (320, 104, 8), (79, 7 * 4 + 1, 4), (1, 4, 4), (2, 9, 9)])
def test_gather_atlas_equals_the_model_byte_for_byte(F, S, n):
    from vdn_hip import mesh
    lay = mesh.texture_layout(F, S, n)
    col = awkward_colors(lay["points"], F)
    want = M.np_atlas(col, lay)
    got = mesh.gather_atlas(dev(col), lay)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (S, S, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    # the cases hold what they are there for: a remainder strip, empty cells, a half-filled last cell
    if (F, S, n) == (5, 13, 4):
        assert S % n and lay["C"] ** 2 > (F + 1) // 2 and F % 2 == 1 and not want[12].any() and not want[:, 12].any()
    assert np.array_equal(mesh.gather_atlas(dev(col, torch.float64), lay).cpu().numpy(), want)       # taken as fp32


def test_gather_atlas_of_an_empty_mesh_is_zero():
    from vdn_hip import mesh
    lay = mesh.texture_layout(0, 16)
    got = mesh.gather_atlas(torch.empty(0, 3, device=DEV), lay)
    assert tuple(got.shape) == (16, 16, 3) and not got.any()


# ---- no bleed ----------------------------------------------------------------------------------------------------------------------------
def neighbour_steps(C):
    """id differences of faces whose patches touch: the cell mate, and the cells left, right, above and below"""
    return (1, 2, 3, 2 * C - 1, 2 * C, 2 * C + 1)


def face_colors(F, C):
    """BGR bytes per face id, drawn until every id is at least 8 levels away, in every channel, from the ids next to it in the atlas"""
    rng = np.random.default_rng(F + C)
    out = np.zeros((F, 3), np.int64)
    for f in range(F):
        near = [out[f - s] for s in neighbour_steps(C) if f - s >= 0]
        while True:
            out[f] = rng.integers(0, 256, 3)
            if all((np.abs(out[f] - x) >= 8).all() for x in near):
                break
    return out


@pytest.mark.parametrize("n", [4, 5, 8])
def test_no_face_reads_its_neighbours_texels(n):
    from vdn_hip import mesh
    v, t = meshes("ico80")
    F = len(t)
    S = square_atlas(F, n, spare=1)
    byte = face_colors(F, S // n)
    for step in neighbour_steps(S // n):
        assert (np.abs(byte[step:] - byte[:-step]) >= 8).all()
    table = dev(byte.astype(np.float32) / np.float32(255.0))
    baked = mesh.bake_texture(None, v, t, texture_size=S, patch=n, project=0, shade=lambda p, f: table[f.long()])
    rng = np.random.default_rng(n)
    inner = rng.dirichlet([1.0, 1.0, 1.0], 16)
    bary = np.concatenate([np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]], [[1 / 3, 1 / 3, 1 / 3]], inner])
    face = np.repeat(np.arange(F), len(bary))
    pts = (np.tile(bary, (F, 1))[:, :, None] * v[t[face]]).sum(axis=1)
    got = mesh.sample_texture(baked["texture"], baked["layout"], dev(v), dev(t), dev(face), dev(pts)).cpu().numpy()
    want = (byte[face][:, ::-1] / 255.0).astype(np.float32)
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all()


# ---- lookups against the fp64 model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S,n", [("ico320", 104, 8), ("odd", 7 * 5 + 2, 5), ("one", 4, 4)])
def test_sample_texture_against_the_fp64_model(name, S, n):
    from vdn_hip import mesh
    v, t = meshes(name)
    lay = mesh.texture_layout(len(t), S, n)
    rng = np.random.default_rng(S)
    tex = rng.integers(0, 256, (S, S, 3)).astype(np.uint8)
    face, pts, _ = M.surface_samples(v, t, 3000, 5)
    # in the plane but outside the triangle (clamped), off the plane, far away, misses, ids past the end, a NaN point
    outside = rng.uniform(-0.4, 1.4, (1000, 3))
    outside[:, 0] = 1.0 - outside[:, 1] - outside[:, 2]
    pts[:1000] = (outside[:, :, None] * v[t[face[:1000]]]).sum(axis=1)
    pts[1000:2000] += 0.05 * rng.standard_normal((1000, 3))
    pts[2000:2010] *= 1e6
    face[2010:2100] = -1
    face[2100:2110] = len(t) + rng.integers(0, 5, 10)
    pts[2110] = np.nan
    bg = (0.25, 0.5, 1.0)
    want = M.np_sample(tex, lay, v, t, face, pts, background=bg)
    for index_dtype in (torch.int64, torch.int32):
        got = mesh.sample_texture(dev(tex), lay, dev(v), dev(t, index_dtype), dev(face), dev(pts), background=bg)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3000, 3)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print("%s: max |lookup - model| = %.3e" % (name, err.max()))
        assert err.max() <= 2.0 ** -23
    assert np.array_equal(got.cpu().numpy()[2010:2110], np.tile(np.asarray(bg, np.float32), (100, 1)))
    assert got.min() >= 0.0 and got.max() <= 1.0


# ---- the networks ------------------------------------------------------------------------------------------------------------------------
def _renderer(precision="bf16"):
    from vdn_train import factory, synth
    if precision not in _CACHE:
        _CACHE[precision] = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(0, variance=0.4), precision=precision)
    return _CACHE[precision]


BOX = (torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]))
CELL = 1.5 * 2.0 / 23                                                            # one and a half lattice spacings of a 24^3 lattice over the box


def _light_mesh():
    """the synthetic surface on a 24^3 lattice, simplified to a few hundred faces -> (vertices float64, triangles int64), numpy"""
    if "light" not in _CACHE:
        from vdn_train import mesh_simplify
        v, t = _renderer().extract_geometry(BOX[0], BOX[1], resolution=24, threshold=0.0)
        res = mesh_simplify.simplify_mesh(v, t, cell_size=CELL)
        _CACHE["light"] = (res["vertices"], res["triangles"].astype(np.int64))
        assert 100 <= len(res["triangles"]) <= 1000, len(res["triangles"])
    return _CACHE["light"]


def test_project_step_against_the_fp64_model():
    from vdn_hip import mesh
    rend = _renderer()
    v, t = _light_mesh()
    x0_np, _ = M.np_texel_points(v, t, 4)
    x0 = dev(x0_np)
    sdf, g, _ = mesh.shade_points(rend, x0)
    r = float((sdf.abs() / g.norm(dim=1).clamp_min(1e-6)).median())               # about half of the first steps leave the ball
    x, clamped = x0, []
    for k in range(2):
        sdf, g, _ = mesh.shade_points(rend, x)
        got = mesh.project_step(x, x0, sdf, g, r)
        want = M.np_project_step(x.cpu().numpy(), x0_np, sdf.cpu().numpy(), g.cpu().numpy(), r)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        bound = 8.0 * float(np.spacing(np.float32(np.abs(x.cpu().numpy()).max() + r)))
        dist = np.linalg.norm(got.cpu().numpy().astype(np.float64) - x0_np.astype(np.float64), axis=1)
        clamped.append(float((dist > r * (1.0 - 2.0 ** -10)).mean()))              # (an fp32 ulp of |x| is about 1e-4 r: well inside 2^-10)
        print("step %d: max |x' - model| = %.3e (bound %.3e), max |x' - x0| / r = 1 + %.3e, on the ball %.2f, median |sdf| %.3e"
              % (k, err, bound, dist.max() / r - 1.0, clamped[-1], float(sdf.abs().median())))
        assert got.dtype == torch.float32 and err <= bound
        assert (dist <= r * (1.0 + 2.0 ** -20)).all()
        x = got
    assert 0.05 < clamped[0] < 0.95                                              # both branches ran
    assert torch.equal(mesh.project_points(rend, x0, rounds=2, max_offset=r), x)       # the loop of the library is this loop
    assert torch.equal(mesh.project_points(rend, x0, rounds=0, max_offset=r), x0)
    assert torch.equal(mesh.project_step(x0, x0, sdf, g, 0.0), x0)                # a ball of radius 0 holds the point in place
    # rows with a non-finite sdf, gradient or position stay where they were
    s2, g2, x2 = sdf.clone(), g.clone(), x0.clone()
    s2[0], s2[1], g2[2, 1], g2[3, 0], x2[4, 2] = float("nan"), float("inf"), float("nan"), float("-inf"), float("nan")
    out = mesh.project_step(x2, x0, s2, g2, r)
    assert np.array_equal(bits32(out[:5]), bits32(x2[:5]))
    assert torch.equal(out[5:], mesh.project_step(x0, x0, sdf, g, r)[5:])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_bake_texture_is_shade_points_gathered_by_the_layout(precision):
    from vdn_hip import mesh
    rend = _renderer(precision)
    v, t = _light_mesh()
    F = len(t)
    S = square_atlas(F, 4, spare=2)
    for batch in (1 << 20, 1000):
        baked = mesh.bake_texture(rend, v, t, texture_size=S, patch=4, project=0, batch=batch)
        lay = baked["layout"]
        assert lay == M.np_layout(F, S, 4) and np.array_equal(baked["uv"], M.np_uv(lay))
        pts, _ = M.np_texel_points(v, t, 4)
        assert np.array_equal(bits32(baked["points"]), bits32(pts))
        _, _, c = mesh.shade_points(rend, dev(pts), batch=batch)
        want = M.np_atlas(None, lay, rgb=mesh.quantize_colors_bgr(c.cpu().numpy()))
        assert baked["texture"].dtype == torch.uint8 and np.array_equal(baked["texture"].cpu().numpy(), want)
    # (the head ends in a sigmoid: every owned texel has a colour in (0, 1), and only what nobody owns is black)
    cells = (F + 1) // 2
    assert int(want.any(axis=2).sum()) == cells * 16 - (F % 2) * 6
    # the default patch is the largest that fits, and tensors give what arrays give
    auto = mesh.bake_texture(rend, dev(v), dev(t, torch.int32), texture_size=S + 40, project=0)
    assert auto["layout"] == M.np_layout(F, S + 40) and auto["layout"]["n"] > 4


def test_bake_texture_projects_by_default():
    from vdn_hip import mesh
    from vdn_train import mesh_texture
    rend = _renderer()
    v, t = _light_mesh()
    S = square_atlas(len(t), 4)
    baked = mesh_texture.bake_texture(rend, v, t, texture_size=S, patch=4)
    assert isinstance(baked["texture"], np.ndarray) and isinstance(baked["points"], np.ndarray) and baked["points"].dtype == np.float32
    x0, _ = M.np_texel_points(v, t, 4)
    r = mesh.mean_edge_length(dev(v), dev(t))
    tri = v[t]
    edges = np.linalg.norm(tri - np.roll(tri, -1, axis=1), axis=2)
    assert abs(r - edges.mean()) <= 1e-12 * edges.mean()
    want = mesh.project_points(rend, dev(x0), rounds=2, max_offset=r)
    assert np.array_equal(bits32(baked["points"]), bits32(want))
    assert np.array_equal(baked["texture"], mesh.bake_texture(rend, v, t, texture_size=S, patch=4, project=2, max_offset=r)["texture"].cpu().numpy())
    before, after = (float(mesh.shade_points(rend, dev(p))[0].abs().median()) for p in (x0, baked["points"]))
    print("median |sdf| at the texel points: %.3e on the triangles, %.3e after two steps" % (before, after))


# ---- accuracy and the preview -----------------------------------------------------------------------------------------------------------
def device_field(p, face):
    phase = torch.tensor(M.PHASE, device=p.device)
    return (0.5 + 0.5 * torch.sin(12.0 * p.double()[:, :1] + phase[None])).float()


def _baked_sphere():
    if "sphere" not in _CACHE:
        from vdn_hip import mesh
        v, t, lay, face, pts, bary = M.accuracy_case()
        _CACHE["sphere"] = mesh.bake_texture(None, v, t, texture_size=lay["S"], patch=lay["n"], project=0, shade=device_field)
        assert _CACHE["sphere"]["layout"] == lay
    return _CACHE["sphere"]


def test_texture_lookup_beats_interpolated_vertex_colours_on_the_device():
    from vdn_hip import mesh
    v, t, lay, face, pts, bary = M.accuracy_case()
    baked = _baked_sphere()
    got = mesh.sample_texture(baked["texture"], lay, dev(v), dev(t), dev(face), dev(pts)).cpu().numpy().astype(np.float64)
    tex_err = np.abs(got - M.color_field(pts)[:, ::-1])
    vtx_err = M.vertex_color_error(v, t, face, pts, bary)
    print("texture: mean %.4f max %.3f; vertex colours: mean %.4f max %.3f; ratio %.3f" %
          (tex_err.mean(), tex_err.max(), vtx_err.mean(), vtx_err.max(), tex_err.mean() / vtx_err.mean()))
    assert tex_err.mean() <= 0.25 * vtx_err.mean()


def test_render_textured_view_is_cast_then_sample():
    from vdn_hip import mesh
    from vdn_train import mesh_texture
    v, t, lay, _, _, _ = M.accuracy_case()
    baked = _baked_sphere()
    grid = mesh.MeshGrid(dev(v, torch.float32), dev(t))
    px = (np.arange(24) + 0.5) / 12.0 - 1.0                                       # a pinhole at (0.3, -0.2, 3) looking down -z, 24 x 24 pixels
    xx, yy = np.meshgrid(px, px)
    d = np.stack([0.5 * xx.ravel(), 0.5 * yy.ravel(), -np.ones(576)], axis=1)
    o = np.tile(np.array([[0.3, -0.2, 3.0]]), (576, 1))
    bg = (0.125, 0.25, 0.5)
    got = mesh.render_textured_view(grid, baked, o, d, background=bg)
    tt, face = grid.cast(dev(o), dev(d))
    tt, face = tt.cpu().numpy(), face.cpu().numpy()
    hit = face >= 0
    assert 100 < hit.sum() < 500 and got.dtype == torch.float32 and tuple(got.shape) == (576, 3)
    x = o + np.where(hit, tt, 0.0)[:, None] * d
    want = mesh.sample_texture(baked["texture"], lay, grid.vertices, grid.triangles, dev(face), dev(x), background=bg)
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy()[~hit], np.tile(np.asarray(bg, np.float32), (int((~hit).sum()), 1)))
    model = M.np_sample(baked["texture"].cpu().numpy(), lay, grid.vertices.cpu().numpy(), t, face, x, background=bg)
    assert np.abs(got.cpu().numpy() - model).max() <= 2.0 ** -23
    # what is seen is the field at the hit points, up to the texture's resolution
    seen = np.abs(got.cpu().numpy()[hit] - M.color_field(x[hit])[:, ::-1])
    assert seen.mean() < 0.03
    # and the numpy front door gives the same picture
    again = mesh_texture.render_textured_view(v.astype(np.float32), t, dict(baked, texture=baked["texture"].cpu().numpy()), o, d, background=bg)
    assert isinstance(again, np.ndarray) and np.array_equal(again, got.cpu().numpy())


# ---- validate_mesh and the command line -------------------------------------------------------------------------------------------------
def test_validate_mesh_with_a_texture(tmp_path):
    from PIL import Image
    from vdn_hip import mesh
    from vdn_train import meshio, validate
    rend = _renderer()
    v, t = _light_mesh()
    scale_mat = np.array([[2.5, 0, 0, 0.5], [0, 2.5, 0, -1.0], [0, 0, 2.5, 3.0], [0, 0, 0, 1.0]])
    kw = dict(resolution=24, world_space=True, scale_mat=scale_mat, simplify={"cell_size": CELL})
    plain, V, F = validate.validate_mesh(rend, BOX[0], BOX[1], str(tmp_path / "plain.ply"), **kw)
    assert sorted(os.listdir(tmp_path)) == ["plain.ply"]
    S = square_atlas(F, 4, spare=1)
    tex_kw = dict(texture_size=S, patch=4)
    path, V2, F2 = validate.validate_mesh(rend, BOX[0], BOX[1], str(tmp_path / "tex.ply"), texture=tex_kw, **kw)
    assert (V2, F2) == (V, F) == (len(v), len(t)) and open(path, "rb").read() == open(plain, "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["plain.ply", "tex.mtl", "tex.obj", "tex.ply", "tex.png"]
    ply, obj = meshio.read_ply(path), meshio.read_obj(str(tmp_path / "tex.obj"))
    assert np.array_equal(obj["vertices"], ply["vertices"]) and np.array_equal(obj["triangles"], ply["triangles"])
    assert np.array_equal(obj["normals"], ply["normals"]) and obj["texture_path"] == str(tmp_path / "tex.png")
    baked = mesh.bake_texture(rend, v, t, **tex_kw)                              # object space, the default two projection rounds
    assert np.array_equal(np.asarray(Image.open(obj["texture_path"]).convert("RGB")), baked["texture"].cpu().numpy())
    assert np.array_equal(obj["uv"], baked["uv"].reshape(-1, 2))
    with pytest.raises(ValueError):
        validate.validate_mesh(rend, BOX[0], BOX[1], str(tmp_path / "bad.ply"), texture=True, **kw)


def test_command_line_tool(tmp_path):
    from PIL import Image
    from vdn_train import meshio
    v, t = _light_mesh()
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.obj")
    meshio.write_ply(src, v, t)
    S = square_atlas(len(t), 5, spare=3)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "texture_mesh.py"), src, out, "--synthetic", "0", "--texture-size", str(S),
                        "--patch", "5", "--project", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    obj = meshio.read_obj(out)
    png = np.asarray(Image.open(obj["texture_path"]).convert("RGB"))
    assert rep["faces"] == len(t) == len(obj["triangles"]) and rep["patch"] == 5 and rep["texels_shaded"] == len(t) * 10
    assert rep["texture_size"] == S and png.shape == (S, S, 3) and rep["project"] == 1
    assert set(rep["seconds"]) == {"points", "project", "shade", "gather", "write"} and all(x >= 0 for x in rep["seconds"].values())
    assert np.array_equal(obj["vertices"], v.astype(np.float32)) and np.array_equal(obj["triangles"], t)
    lay = M.np_layout(len(t), S, 5)
    assert np.array_equal(obj["uv"], M.np_uv(lay).reshape(-1, 2))
    used = png.any(axis=2)
    assert used[:lay["C"] * 5, :lay["C"] * 5].mean() > 0.5 and not used[lay["C"] * 5:].any() and not used[:, lay["C"] * 5:].any()


# ---- argument errors and the empty mesh ----------------------------------------------------------------------------------------------
def test_argument_errors_and_the_empty_mesh():
    from vdn_hip import mesh
    from vdn_train import mesh_texture
    v, t = meshes("ico80")
    dv, dt = dev(v), dev(t)
    lay = mesh.texture_layout(len(t), 64, 4)
    table = dev(np.full((len(t), 3), 0.5, np.float32))
    shade = lambda p, f: table[f.long()]
    with pytest.raises(ValueError):
        mesh.texel_points(torch.from_numpy(v), torch.from_numpy(t), lay)        # CPU tensors
    with pytest.raises(ValueError):
        mesh.texel_points(dv[:, :2], dt, lay)
    with pytest.raises(ValueError):
        mesh.texel_points(dv, dt.float(), lay)
    with pytest.raises(ValueError):
        mesh.texel_points(dv, dt[:-1], lay)                                      # a layout of another face count
    with pytest.raises(ValueError):
        mesh.texel_points(dv, dt, dict(lay, C=lay["C"] + 1))                     # a record texture_layout does not give
    with pytest.raises(ValueError):
        mesh.gather_atlas(torch.zeros(lay["points"] - 1, 3, device=DEV), lay)
    with pytest.raises(ValueError):
        mesh.gather_atlas(torch.zeros(lay["points"], 3), lay)
    tex = torch.zeros(64, 64, 3, dtype=torch.uint8, device=DEV)
    f0, p0 = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, 3, dtype=torch.float64, device=DEV)
    for bad in (dict(texture=tex[:63]), dict(texture=tex.float()), dict(face=f0.double()), dict(points=p0[:1]), dict(background=(1, 1))):
        kw = dict(texture=tex, layout=lay, vertices=dv, triangles=dt, face=f0, points=p0)
        kw.update(bad)
        with pytest.raises(ValueError):
            mesh.sample_texture(**kw)
    x = torch.zeros(4, 3, device=DEV)
    for bad in (dict(x0=x[:3]), dict(sdf=x), dict(gradient=x[:, :2]), dict(max_offset=-1.0), dict(max_offset=float("nan")), dict(x=x.cpu())):
        kw = dict(x=x, x0=x, sdf=x[:, 0], gradient=x, max_offset=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            mesh.project_step(**kw)
    for bad in (dict(texture_size=16), dict(patch=3), dict(project=-1), dict(project=1), dict(batch=0), dict(shade=3), dict(max_offset=-1.0)):
        kw = dict(texture_size=64, patch=4, project=0, shade=shade)
        kw.update(bad)
        with pytest.raises(ValueError):
            mesh.bake_texture(None, v, t, **kw)                                  # (project = 1 without a renderer is one of them)
    with pytest.raises(ValueError):
        mesh.bake_texture(None, v, t, texture_size=64, project=0)               # neither networks nor a stand-in
    with pytest.raises(ValueError):
        mesh.bake_texture(None, v, t, texture_size=64, project=0, shade=lambda p, f: table[f.long()][:, :2])
    with pytest.raises(ValueError):
        mesh.render_textured_view(None, {}, np.zeros((1, 3)), np.ones((1, 3)))
    # nothing was corrupted on the way
    ok = mesh.bake_texture(None, v, t, texture_size=64, patch=4, project=0, shade=shade)
    assert np.array_equal(ok["texture"].cpu().numpy(), M.np_atlas(np.full((lay["points"], 3), 0.5, np.float32), lay))
    # the empty mesh: an all-zero atlas, and every lookup a miss
    for vv, tt in ((v, t[:0]), (v[:0], t[:0]), (dv, dt[:0].int())):
        e = mesh.bake_texture(None, vv, tt, texture_size=16, project=0, shade=shade)
        assert tuple(e["texture"].shape) == (16, 16, 3) and not e["texture"].any() and e["uv"].shape == (0, 3, 2) and tuple(e["points"].shape) == (0, 3)
        rgb = mesh.sample_texture(e["texture"], e["layout"], dv, dt[:0], f0 - 1, p0, background=(0.5, 0.25, 0.0))
        assert rgb.tolist() == [[0.5, 0.25, 0.0]] * 2
    e = mesh_texture.bake_texture(None, np.zeros((0, 3)), np.zeros((0, 3), np.int64), texture_size=8, project=0, shade=shade)
    assert isinstance(e["texture"], np.ndarray) and not e["texture"].any()
