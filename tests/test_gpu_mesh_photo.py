"""Texel colours from the photographs on the device (csrc/mesh_photo.hip, vdn_hip/mesh.py: photo_colors, bake_texture(photos=),
vdn_train/mesh_texture.py: bake_photo_texture, tools/texture_mesh.py --photos) against np_photo_colors, the fp64 model of
test_mesh_photo_cpu.py, no texel excluded: n_views and best_view exactly, colours within one fp32 rounding of a value in [0, 1]
(2^-23 absolute), weights within 2^-23 relative; atlases byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_mesh_photo_cpu as C
import test_mesh_texture_cpu as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def dev(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def run(case, grid, blend, anchors="case", **kw):
    from vdn_hip import mesh
    scalars = dict(C.FIXTURE_SCALARS, **kw)
    return mesh.photo_colors(grid, dev(case["points"]), dev(case["face"]), case["P"], dev(case["images"]), normals=dev(case["normals"]),
                             anchors=dev(case["anchors"]) if anchors == "case" else anchors, blend=blend, **scalars)


def check(got, want, what=""):
    assert got["colors"].dtype == torch.float32 and got["weight"].dtype == torch.float32
    assert got["n_views"].dtype == torch.int32 and got["best_view"].dtype == torch.int32
    assert np.array_equal(got["n_views"].cpu().numpy(), want["n_views"])
    assert np.array_equal(got["best_view"].cpu().numpy(), want["best_view"])
    col, wgt = got["colors"].cpu().numpy().astype(np.float64), got["weight"].cpu().numpy().astype(np.float64)
    e_col = np.abs(col - want["colors"]).max()
    e_wgt = (np.abs(wgt - want["weight"]) / np.maximum(want["weight"], 1e-300)).max()
    print("%s max |colour - model| = %.3e, max relative |weight - model| = %.3e" % (what, e_col, e_wgt))
    assert e_col <= 2.0 ** -23 and e_wgt <= 2.0 ** -23
    unseen = want["n_views"] == 0
    assert not col[unseen].any() and not wgt[unseen].any()


# ---- the launch against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_anchors", [False, True])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("blend", ["mean", "best"])
def test_photo_colors_equal_the_model(blend, n, with_normals, index_dtype, with_anchors):
    from vdn_hip import mesh
    case = C.fixture_case(n, with_normals, with_anchors)
    assert len(case["points"]) in (80 * 6 + 12, 80 * 10 + 20)
    grid = mesh.MeshGrid(dev(case["v"], torch.float32), dev(case["t"], index_dtype))
    want = C.fixture_model(n, with_normals, with_anchors, blend)
    check(run(case, grid, blend), want, "with the anchors:" if with_anchors else "")
    if with_anchors:
        # the own-face rule is what keeps these texels: the same points without the anchors lose cameras, in the model and on the device
        lost = C.fixture_model(n, with_normals, True, blend, use_anchors=False)
        assert ((lost["n_views"] == 0) & (want["n_views"] > 0)).any() and (lost["n_views"] < want["n_views"]).sum() > 20
        check(run(case, grid, blend, anchors=None), lost, "without them:")


def test_two_calls_and_two_grids_give_the_same_bits():
    from vdn_hip import mesh
    case = C.fixture_case(5, True, True)
    v, t = dev(case["v"], torch.float32), dev(case["t"])
    first = run(case, mesh.MeshGrid(v, t), "mean")
    grids = [mesh.MeshGrid(v, t), mesh.MeshGrid(v, t, cell_size=0.11), mesh.MeshGrid(v, t, cell_size=0.7)]
    assert len({tuple(g.dims) for g in grids}) == 3
    for g in grids:
        again = run(case, g, "mean")
        for k in ("colors", "weight", "n_views", "best_view"):
            assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), (k, g.h)


def test_refusals_and_empties():
    from vdn_hip import mesh
    case = C.fixture_case(4, True, False)
    v, t = dev(case["v"], torch.float32), dev(case["t"])
    grid = mesh.MeshGrid(v, t)
    pts, face, img, nrm = dev(case["points"]), dev(case["face"]), dev(case["images"]), dev(case["normals"])
    P = case["P"]
    good = dict(grid=grid, points=pts, face=face, P=P, images=img, normals=nrm, blend="mean", **C.FIXTURE_SCALARS)
    for bad_value in (len(case["t"]), -1):
        bad = face.clone()
        bad[77] = bad_value
        with pytest.raises(ValueError):
            mesh.photo_colors(**dict(good, face=bad))
    singular = P.copy()
    singular[2, 2, :3] = singular[2, 1, :3]
    for bad in (dict(points=pts.cpu()), dict(face=face.cpu()), dict(face=face.long()), dict(points=pts[:, :2]), dict(face=face[:-1]),
                dict(images=img.cpu()), dict(images=img.double()), dict(images=img[..., :2]), dict(images=img.permute(0, 2, 1, 3)),
                dict(images=img[:4]), dict(normals=nrm[:-1]), dict(normals=nrm.cpu()), dict(anchors=pts[:5]), dict(P=singular), dict(P=P[:, :2]),
                dict(blend="median"), dict(cos_min=1.0), dict(cos_min=-0.1), dict(feather=-1.0), dict(feather=float("nan")), dict(eps=1.0),
                dict(eps=-1e-4), dict(grid=None)):
        with pytest.raises(ValueError):
            mesh.photo_colors(**dict(good, **bad))
    check(mesh.photo_colors(**good), C.fixture_model(4, True, False, "mean"), "after the refusals:")      # nothing was corrupted on the way

    def unseen(out, rows):
        assert tuple(out["colors"].shape) == (rows, 3) and not out["colors"].any() and not out["weight"].any() and not out["n_views"].any()
        assert (out["best_view"] == -1).all() and out["best_view"].dtype == torch.int32 and tuple(out["best_view"].shape) == (rows,)
    unseen(mesh.photo_colors(**dict(good, points=pts[:0], face=face[:0], normals=None)), 0)
    unseen(mesh.photo_colors(**dict(good, P=P[:0], images=img[:0])), len(case["points"]))
    unseen(mesh.photo_colors(**dict(good, grid=mesh.MeshGrid(v, t[:0]))), len(case["points"]))


# ---- bake_texture(photos=...) ------------------------------------------------------------------------------------------------------------
def _renderer():
    from vdn_train import factory, synth
    if "rend" not in _CACHE:
        _CACHE["rend"] = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(0, variance=0.4), precision="bf16")
    return _CACHE["rend"]


def _expected_atlas(lay, model, fallback):
    colors = np.where((model["n_views"] > 0)[:, None], model["colors"].astype(np.float32), np.asarray(fallback, np.float32))
    return M.np_atlas(colors, lay)


def test_bake_texture_from_the_photographs():
    from vdn_hip import mesh
    rend = _renderer()
    v, t = M.icosphere(1)
    P, images = C.fixture_cameras(), C.fixture_images()
    S, n = 7 * 5 + 2, 5
    pts, face = M.np_texel_points(v, t, n)
    _, grad, net = mesh.shade_points(rend, dev(pts))
    corners = v.astype(np.float32)[t]
    photos = {"P": P, "images": images}
    # with the networks: the SDF gradient is the normal (one-sided), the network's colour fills what no camera sees
    model = C.np_photo_colors(corners, pts, face, P, images, normals=grad.cpu().numpy())
    seen = model["n_views"] > 0
    assert 0 < seen.sum() < len(seen)
    plain = mesh.bake_texture(rend, v, t, texture_size=S, patch=n, project=0)
    assert set(plain) == {"texture", "uv", "layout", "points"}
    want_plain = M.np_atlas(None, plain["layout"], rgb=mesh.quantize_colors_bgr(net.cpu().numpy()))
    assert np.array_equal(plain["texture"].cpu().numpy(), want_plain)            # the path without photos is what it was
    baked = mesh.bake_texture(rend, v, t, texture_size=S, patch=n, project=0, photos=photos)
    lay = baked["layout"]
    assert lay == plain["layout"] and np.array_equal(baked["uv"], plain["uv"]) and torch.equal(baked["points"], plain["points"])
    assert np.array_equal(baked["n_views"].cpu().numpy(), model["n_views"]) and baked["coverage"] == seen.sum() / len(seen)
    atlas = baked["texture"].cpu().numpy()
    assert np.array_equal(atlas, _expected_atlas(lay, model, net.cpu().numpy()))
    from_photos, from_network = M.np_atlas(np.repeat(seen[:, None], 3, 1).astype(np.float32), lay) > 0, M.np_atlas(np.repeat(~seen[:, None], 3, 1).astype(np.float32), lay) > 0
    assert from_network.any() and np.array_equal(atlas[from_network], want_plain[from_network])
    assert (atlas[from_photos] != want_plain[from_photos]).mean() > 0.5
    # without them: the faces' own normals, two-sided, and the fill colour
    model2 = C.np_photo_colors(corners, pts, face, P, images, blend="best", feather=4.0)
    for fill in ((0.5, 0.5, 0.5), (0.25, 0.5, 1.0)):
        ph = dict(photos, blend="best", feather=4.0)
        if fill != (0.5, 0.5, 0.5):
            ph["fill"] = fill
        got = mesh.bake_texture(None, dev(v), dev(t, torch.int32), texture_size=S, patch=n, project=0, photos=ph)
        assert np.array_equal(got["texture"].cpu().numpy(), _expected_atlas(lay, model2, fill))
        assert got["coverage"] == (model2["n_views"] > 0).mean() and 0 < got["coverage"] < 1
    # projection: the anchors stay on the triangles, the lookups move, the last round's gradient is the normal
    x0 = dev(pts)
    r = mesh.mean_edge_length(dev(v), dev(t))
    sdf, g, _ = mesh.shade_points(rend, x0)
    x1 = mesh.project_step(x0, x0, sdf, g, r)
    model3 = C.np_photo_colors(corners, x1.cpu().numpy(), face, P, images, normals=g.cpu().numpy(), anchors=pts)
    got = mesh.bake_texture(rend, v, t, texture_size=S, patch=n, project=1, photos=photos)
    assert torch.equal(got["points"], x1) and np.array_equal(got["n_views"].cpu().numpy(), model3["n_views"])
    rows = np.nonzero(model3["n_views"] == 0)[0]
    fallback = np.zeros((len(pts), 3), np.float32)
    fallback[rows] = mesh.shade_points(rend, x1[dev(rows)])[2].cpu().numpy()
    assert np.array_equal(got["texture"].cpu().numpy(), _expected_atlas(lay, model3, fallback))
    # refusals
    with pytest.raises(ValueError):
        mesh.bake_texture(rend, v, t, texture_size=S, patch=n, project=0, photos=photos, shade=lambda p, f: p)
    with pytest.raises(ValueError):
        mesh.bake_texture(None, v, t, texture_size=S, patch=n, project=1, photos=photos)
    with pytest.raises(ValueError):
        mesh.bake_texture(None, v, t, texture_size=S, patch=n, project=0, photos=dict(photos, images=(images * 255).astype(np.uint8)))
    empty = mesh.bake_texture(None, v, t[:0], texture_size=16, project=0, photos=photos)
    assert not empty["texture"].any() and empty["coverage"] == 0.0 and tuple(empty["n_views"].shape) == (0,)


# ---- the numpy front door and the command line -------------------------------------------------------------------------------------------
def _write_scene(root, P, images_bgr_bytes):
    """a scene directory of vdn_train.dataset.SceneData: image/*.png, image/mask/*.png (all white), cameras_sphere.npz"""
    from PIL import Image
    from vdn_train import dataset
    os.makedirs(os.path.join(root, "image", "mask"))
    names = ["%03d" % k for k in range(len(P))]
    for name, img in zip(names, images_bgr_bytes):
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(os.path.join(root, "image", name + ".png"))
        Image.fromarray(np.full(img.shape, 255, np.uint8)).save(os.path.join(root, "image", "mask", name + ".png"))
    world = [np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]]) for p in P]
    dataset.write_cameras_npz(os.path.join(root, "cameras_sphere.npz"), names, world, [np.eye(4)] * len(P))


def test_validate_scene_mesh_fills_in_the_scenes_photographs(tmp_path):
    from PIL import Image
    from vdn_hip import mesh
    from vdn_train import dataset, mesh_simplify, validate
    rend = _renderer()
    scene_dir = str(tmp_path / "scene")
    _write_scene(scene_dir, C.fixture_cameras(), np.random.default_rng(6).integers(0, 256, (5, C.H, C.W, 3)).astype(np.uint8))
    scene = dataset.SceneData(scene_dir)
    cell = 1.5 * 2.02 / 23
    kw = dict(resolution=24, simplify={"cell_size": cell})
    tex = dict(texture_size=128, patch=4, project=0)
    path, V, F = validate.validate_scene_mesh(rend, scene, str(tmp_path / "out"), iter_step=7, texture=dict(tex, photos={"blend": "best"}), **kw)
    stem = os.path.splitext(path)[0]
    assert sorted(os.listdir(os.path.dirname(path))) == ["00000007.mtl", "00000007.obj", "00000007.ply", "00000007.png"]
    v, t = rend.extract_geometry(torch.tensor(scene.object_bbox_min, dtype=torch.float32), torch.tensor(scene.object_bbox_max, dtype=torch.float32),
                                 resolution=24, threshold=0.0)
    res = mesh_simplify.simplify_mesh(v, t, cell_size=cell)
    v, t = res["vertices"], res["triangles"]
    assert (V, F) == (len(v), len(t))
    photos = {"P": scene.projection_matrices(world_space=False), "images": scene.images, "blend": "best"}
    want = mesh.bake_texture(rend, v, t, photos=photos, **tex)
    assert want["coverage"] > 0
    png = np.asarray(Image.open(stem + ".png").convert("RGB"))
    assert np.array_equal(png, want["texture"].cpu().numpy())
    assert not np.array_equal(png, mesh.bake_texture(rend, v, t, **tex)["texture"].cpu().numpy())
    # validate_mesh takes the cameras and images as given; "photos": True is the scene's, with the defaults
    again, _, _ = validate.validate_mesh(rend, torch.tensor(scene.object_bbox_min, dtype=torch.float32), torch.tensor(scene.object_bbox_max, dtype=torch.float32),
                                         str(tmp_path / "again.ply"), texture=dict(tex, photos=photos), **kw)
    assert np.array_equal(np.asarray(Image.open(os.path.splitext(again)[0] + ".png").convert("RGB")), png)
    validate.validate_scene_mesh(rend, scene, str(tmp_path / "out"), iter_step=8, texture=dict(tex, photos=True), **kw)
    mean = mesh.bake_texture(rend, v, t, photos=dict(photos, blend="mean"), **tex)["texture"].cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(os.path.join(os.path.dirname(path), "00000008.png")).convert("RGB")), mean)
    with pytest.raises(ValueError):
        validate.validate_scene_mesh(rend, scene, str(tmp_path / "out"), iter_step=9, texture=dict(tex, photos=3), **kw)


def test_bake_photo_texture_and_the_command_line(tmp_path):
    from PIL import Image
    from vdn_hip import mesh
    from vdn_train import dataset, mesh_texture, meshio
    v, t = C.fixture_mesh()
    v = v.astype(np.float32)
    P = C.fixture_cameras()
    bytes_bgr = np.random.default_rng(5).integers(0, 256, (5, C.H, C.W, 3)).astype(np.uint8)
    scene_dir = str(tmp_path / "scene")
    _write_scene(scene_dir, P, bytes_bgr)
    scene = dataset.SceneData(scene_dir)
    images = (bytes_bgr.astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(scene.images, images)
    P32 = scene.projection_matrices(world_space=False)
    S, n = 7 * 5 + 3, 5
    views = [4, 0, 2, 1]
    pts, face = M.np_texel_points(v, t, n)
    model = C.np_photo_colors(v[t], pts, face, P32[views], images[views])
    seen = model["n_views"] > 0
    assert 0 < seen.sum() < len(seen)
    # numpy in, numpy out - from the scene, from an explicit pair, from the scene with its resident images; tensors in, tensors out
    kw = dict(texture_size=S, patch=n, project=0)
    want = _expected_atlas(M.np_layout(len(t), S, n), model, (0.5, 0.5, 0.5))
    a = mesh_texture.bake_photo_texture(None, scene, v, t, views=views, **kw)
    assert all(isinstance(a[k], np.ndarray) for k in ("texture", "points", "n_views", "uv")) and np.array_equal(a["texture"], want)
    assert a["coverage"] == seen.mean() and np.array_equal(a["n_views"], model["n_views"])
    b = mesh_texture.bake_photo_texture(None, (P32[views], images[views]), v, t, **kw)
    c = mesh_texture.bake_photo_texture(None, (scene, scene.rays_generator(DEV)), dev(v), dev(t), views=views, **kw)
    assert np.array_equal(b["texture"], want) and torch.is_tensor(c["texture"]) and np.array_equal(c["texture"].cpu().numpy(), want)
    tensor_path = mesh.bake_texture(None, dev(v), dev(t), photos={"P": P32[views], "images": dev(images[views])}, **kw)
    assert np.array_equal(tensor_path["texture"].cpu().numpy(), a["texture"]) and tensor_path["coverage"] == a["coverage"]
    d = mesh_texture.bake_photo_texture(None, scene, v, t, blend="best", fill=(0.0, 0.0, 1.0), **kw)
    model_best = C.np_photo_colors(v[t], pts, face, P32, images, blend="best")
    assert np.array_equal(d["texture"], _expected_atlas(M.np_layout(len(t), S, n), model_best, (0.0, 0.0, 1.0)))
    with pytest.raises(ValueError):
        mesh_texture.bake_photo_texture(None, scene, v, t, views=[0, 5], **kw)
    # the command line: no weights are needed when nothing is projected
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.obj")
    meshio.write_ply(src, v, t)
    tool = os.path.join(ROOT, "tools", "texture_mesh.py")
    r = subprocess.run([sys.executable, tool, src, out, "--photos", scene_dir, "--views", "4,0,2,1", "--texture-size", str(S), "--patch", str(n),
                        "--project", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path)) == ["in.ply", "out.mtl", "out.obj", "out.png", "scene"]
    obj = meshio.read_obj(out)
    assert rep["coverage"] == seen.mean() and rep["faces"] == len(t) == len(obj["triangles"]) and rep["views"] == 4 and rep["blend"] == "mean"
    assert set(rep["seconds"]) == {"photo", "write"} and rep["seconds"]["photo"] >= 0
    assert np.array_equal(np.asarray(Image.open(obj["texture_path"]).convert("RGB")), want)
    bad = subprocess.run([sys.executable, tool, src, out, "--photos", scene_dir, "--project", "1"], capture_output=True, text=True)
    assert bad.returncode == 2                                                   # projection needs the networks
