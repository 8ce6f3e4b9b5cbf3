"""Ray casting against the mesh and visibility culling on the device (csrc/mesh_ray.hip, vdn_hip/mesh.py: MeshGrid,
visibility_votes; vdn_train/mesh_clean.py) against the numpy models of test_mesh_visibility_cpu.py: brute-force Moller-Trumbore in
the documented order, on a case the model itself finds free of ambiguous decisions - so every face must be equal, t within 1e-9
relative (about 10^7 fp64 epsilons on well-conditioned pairs), and both bit-identical across cell sizes and calls."""
import json

import numpy as np
import pytest
import torch

from test_mesh_visibility_cpu import H, W, WINDOWS, np_cast, np_visibility, referenced_faces, valid_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CELL_SIZES = (None, 0.05, 0.5, 1e3)          # the default, a fine grid, a coarse one, one cell
_CACHE = {}


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def grids():
    """one MeshGrid of the case mesh per cell size"""
    if "grids" not in _CACHE:
        from vdn_hip import mesh
        c = valid_case()
        _CACHE["grids"] = {h: mesh.MeshGrid(dev(c["v32"]), dev(c["tri"]), cell_size=h) for h in CELL_SIZES}
    return _CACHE["grids"]


def plane_rays():
    """Rays whose origins lie exactly on grid planes lo + k h of the default and of the fine grid (on one, two or all three axes),
    random directions; re-drawn until the model finds no ambiguous decision among them, as the case's own jitter is.
    -> (origins, directions, {window: (t, face)})"""
    if "plane" not in _CACHE:
        c = valid_case()
        for seed in range(20):
            rng = np.random.default_rng(100 + seed)
            o = []
            for h in (None, 0.05):
                g = grids()[h]
                lo, n = np.array(g.lo), np.array(g.dims)
                k = np.stack([rng.integers(0, n[a] + 1, 150) for a in range(3)], axis=1)
                on = lo[None] + k * g.h                                    # (the planes as the kernel forms them: lo + k h in double)
                free = rng.uniform(lo - 0.3, lo + n * g.h + 0.3, (150, 3))
                which = rng.integers(1, 8, 150)                            # a bit per axis: which coordinates sit on a plane
                o.append(np.where((which[:, None] >> np.arange(3)) & 1, on, free))
            o = np.concatenate(o)
            d = rng.normal(size=o.shape)
            d[::7] *= (rng.random((len(d[::7]), 3)) > 0.4)                 # some with zero components, moving inside the plane
            d[(d == 0).all(axis=1)] = (0.0, 0.0, -1.0)
            cast, ambiguous = {}, 0
            for w in WINDOWS:
                t, face, amb = np_cast(c["v32"], c["tri"], o, d, w[0], w[1], return_ambiguous=True)
                cast[w], ambiguous = (t, face), ambiguous + amb
            if ambiguous == 0:
                break
        assert ambiguous == 0
        _CACHE["plane"] = (o, d, cast)
    return _CACHE["plane"]


def all_rays():
    c, (po, pd, pcast) = valid_case(), plane_rays()
    o, d = np.concatenate([c["origins"], po]), np.concatenate([c["directions"], pd])
    return o, d, {w: (np.concatenate([c["cast"][w][0], pcast[w][0]]), np.concatenate([c["cast"][w][1], pcast[w][1]])) for w in WINDOWS}


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
def test_grid_tables_reference_every_triangle_its_box_overlaps():
    c = valid_case()
    assert c["ambiguous"] == 0
    ref = referenced_faces(c["v32"], c["tri"])
    p = c["v32"].astype(np.float64)[c["tri"][ref]]
    for h, g in grids().items():
        start, refs = g.cell_start.cpu().numpy(), g.refs.cpu().numpy()[:g.n_refs]
        assert start.dtype == np.int32 and start[0] == 0 and start[-1] == g.n_refs == len(refs) and (np.diff(start) >= 0).all()
        assert len(start) == g.n_cells + 1 == int(np.prod(g.dims)) + 1 and g.nbytes > 0
        assert set(np.unique(refs)) == set(np.nonzero(ref)[0])             # the degenerate faces are in no cell, the others in some
        # the reference rule, restated: the cells a triangle's grown box overlaps, per axis
        lo, n = np.array(g.lo), np.array(g.dims)
        c0 = np.clip(np.floor((p.min(axis=1) - g.margin - lo) / g.h), 0, n - 1).astype(int)
        c1 = np.clip(np.floor((p.max(axis=1) + g.margin - lo) / g.h), 0, n - 1).astype(int)
        assert g.n_refs == int((c1 - c0 + 1).prod(axis=1).sum())
        cell_of_ref = np.repeat(np.arange(g.n_cells), np.diff(start))
        cz, cy, cx = cell_of_ref // (n[0] * n[1]), cell_of_ref // n[0] % n[1], cell_of_ref % n[0]
        face_row = np.cumsum(ref)[refs] - 1
        inside = (np.stack([cx, cy, cz], axis=1) >= c0[face_row]) & (np.stack([cx, cy, cz], axis=1) <= c1[face_row])
        assert inside.all() and len(np.unique(np.stack([cell_of_ref, refs]), axis=1).T) == g.n_refs        # in range, and each pair once
        if h == 1e3:
            assert g.dims == [1, 1, 1] and g.n_refs == int(ref.sum())
    g = grids()[0.05]
    quad = np.nonzero((c["part"][c["tri"]] == 3).all(axis=1))[0]
    per_face = np.bincount(g.refs.cpu().numpy()[:g.n_refs], minlength=len(c["tri"]))
    assert g.n_cells > 20000 and (per_face[quad] > 2000).all()            # the large triangles sit in thousands of cells
    assert grids()[None].n_cells > 8                                       # the default is a real grid on this mesh


# ---- closest hit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", range(len(WINDOWS)))
def test_closest_hit_equals_the_model_on_every_grid(window):
    w = WINDOWS[window]
    o, d, cast = all_rays()
    want_t, want_f = cast[w]
    assert 4000 <= len(o) <= 5000 and (want_f >= 0).sum() > 400 and (want_f < 0).sum() > 400
    od, dd = dev(o), dev(d)
    first = None
    for h, g in grids().items():
        t, face = g.cast(od, dd, t_min=w[0], t_max=w[1])
        assert t.dtype == torch.float64 and face.dtype == torch.int64 and t.shape == face.shape == (len(o),) and t.is_cuda
        tn, fn = t.cpu().numpy(), face.cpu().numpy()
        wrong = np.nonzero(fn != want_f)[0]
        assert len(wrong) == 0, (h, wrong[:10], fn[wrong[:10]], want_f[wrong[:10]])
        hit = want_f >= 0
        assert np.isposinf(tn[~hit]).all()
        rel = np.abs(tn[hit] - want_t[hit]) / np.abs(want_t[hit])
        print("cell size", h, "window", w, "max relative error of t", rel.max(), "bit-equal", int((tn[hit] == want_t[hit]).sum()), "of", int(hit.sum()))
        assert rel.max() <= 1e-9, h
        t2, face2 = g.cast(od, dd, t_min=w[0], t_max=w[1])
        assert torch.equal(t2, t) and torch.equal(face2, face)              # two calls: the same bits
        if first is None:
            first = (t, face)
        assert torch.equal(t, first[0]) and torch.equal(face, first[1]), h  # and the same bits at every cell size


def test_any_hit_finds_a_hit_exactly_where_there_is_one():
    o, d, cast = all_rays()
    od, dd = dev(o), dev(d)
    for w in WINDOWS:
        for h, g in grids().items():
            t, face = g.cast(od, dd, t_min=w[0], t_max=w[1], any_hit=True)
            fn, tn = face.cpu().numpy(), t.cpu().numpy()
            assert np.array_equal(fn >= 0, cast[w][1] >= 0), (w, h)
            assert (fn[fn < 0] == -1).all() and np.isposinf(tn[fn < 0]).all()
            assert ((tn > w[0]) & (tn < w[1]))[fn >= 0].all() and referenced_faces(valid_case()["v32"], valid_case()["tri"])[fn[fn >= 0]].all()


def test_skip_vertex_equals_the_model_without_the_incident_faces():
    c = valid_case()
    o, d = c["origins"][::2], c["directions"][::2]
    base = c["cast"][WINDOWS[0]][1][::2]
    rng = np.random.default_rng(5)
    # half of the rays that hit skip a corner of the face they hit, the rest a random vertex (or one that does not exist)
    skip = rng.integers(-3, len(c["v32"]) + 3, len(o))
    hit = np.nonzero(base >= 0)[0][::2]
    skip[hit] = c["tri"][base[hit], rng.integers(0, 3, len(hit))]
    want_t, want_f, ambiguous = np_cast(c["v32"], c["tri"], o, d, skip_vertex=skip, return_ambiguous=True)
    assert ambiguous == 0 and (want_f[hit] != base[hit]).all() and (want_f[hit] >= 0).sum() > 100
    first = None
    for h, g in grids().items():
        for sk in (dev(skip), dev(skip, torch.int32), skip):
            t, face = g.cast(dev(o), dev(d), skip_vertex=sk)
            assert np.array_equal(face.cpu().numpy(), want_f), h
            got = t.cpu().numpy()
            assert np.isposinf(got[want_f < 0]).all() and (np.abs(got - want_t)[want_f >= 0] <= 1e-9 * np.abs(want_t[want_f >= 0])).all()
            first = first if first is not None else t
            assert torch.equal(t, first)


def test_tests_per_ray_fall_with_the_grid():
    c = valid_case()
    o, d, cast = all_rays()
    n_ref = int(referenced_faces(c["v32"], c["tri"]).sum())
    one = grids()[1e3]
    t, face, tests = one.cast(dev(o), dev(d), return_tests=True)
    assert tests.dtype == torch.int32 and tests.shape == (len(o),)
    tn = tests.cpu().numpy()
    assert set(np.unique(tn)) <= {0, n_ref}                                # one cell: all of its faces or, past the box, none
    # a ray crosses the box for certain where it has a hit; it stays clear of it for certain when it never comes within the margin
    assert (tn[cast[WINDOWS[0]][1] >= 0] == n_ref).all()
    lo, hi = np.array(one.lo) - 1e-6, np.array(one.lo) + one.h + 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
        near = np.where(d != 0, np.minimum(ta, tb), np.where((o >= lo) & (o <= hi), -np.inf, np.inf)).max(axis=1)
        far = np.where(d != 0, np.maximum(ta, tb), np.where((o >= lo) & (o <= hi), np.inf, -np.inf)).min(axis=1)
    crosses = np.maximum(near, 0.0) < far
    assert (tn[~crosses] == 0).all() and 0 < (~crosses).sum()
    t2, face2, tests2 = grids()[None].cast(dev(o), dev(d), return_tests=True)
    assert torch.equal(t2, t) and torch.equal(face2, face)
    total_one, total_default = int(tn.sum()), int(tests2.sum().item())
    print("ray-triangle tests per ray: one cell %.1f, default grid (h = %.4f, %s cells) %.2f: ratio %.4f; fine grid %.2f"
          % (total_one / len(o), grids()[None].h, grids()[None].dims, total_default / len(o), total_default / total_one,
             grids()[0.05].cast(dev(o), dev(d), return_tests=True)[2].sum().item() / len(o)))
    assert 0 < total_default < total_one


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
def test_rays_that_cannot_hit_miss_and_return():
    g = grids()[None]
    nan, inf = np.nan, np.inf
    o = np.array([[nan, 0, 2], [0, inf, 2], [0, 0, 2], [0, 0, 2], [0, 0, 2], [0, 0, 2], [0, 0, 2.0], [0, 0, 2.0]])
    d = np.array([[0, 0, -1], [0, 0, -1], [0, nan, -1], [-inf, 0, -1], [0, 0, 0], [0, 0, -1e-320], [0, 0, -1.0], [0, 0, -1e-300]])
    for h, gr in grids().items():
        t, face, tests = gr.cast(o, d, return_tests=True)
        assert face.tolist()[:6] == [-1] * 6 and torch.isposinf(t[:6]).all() and tests.tolist()[:6] == [0] * 6, h
        assert face[6].item() >= 0 and face[7].item() == face[6].item() and abs(t[6].item() - 1.4) < 0.01       # the top of the outer sphere
    for kw in (dict(t_min=2.0, t_max=1.0), dict(t_min=1.0, t_max=1.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=-inf)):
        t, face, tests = g.cast(o[6:7], d[6:7], return_tests=True, **kw)
        assert face.item() == -1 and t.item() == inf and tests.item() == 0, kw
    e = g.cast(np.zeros((0, 3)), np.zeros((0, 3)), return_tests=True, skip_vertex=np.zeros(0, np.int64))
    assert e[0].shape == e[1].shape == e[2].shape == (0,) and e[0].dtype == torch.float64 and e[1].dtype == torch.int64


def test_a_mesh_without_faces_is_all_misses():
    from vdn_hip import mesh
    c = valid_case()
    o, d = dev(c["origins"][:300]), dev(c["directions"][:300])
    bad = c["tri"][~referenced_faces(c["v32"], c["tri"])]
    for tri in (c["tri"][:0], bad):                                       # no faces at all; only faces that are never referenced
        for h in (None, 0.05):
            g = mesh.MeshGrid(dev(c["v32"]), dev(tri), cell_size=h)
            assert g.n_refs == 0
            t, face, tests = g.cast(o, d, return_tests=True)
            assert (face == -1).all() and torch.isposinf(t).all() and (tests == 0).all()
            assert (g.cast(o, d, any_hit=True)[1] == -1).all()
    n_img, n_vis = mesh.visibility_votes(dev(c["v32"]), dev(c["tri"][:0]), c["P"], (H, W))
    assert np.array_equal(n_img.cpu().numpy(), c["votes"][0]) and torch.equal(n_vis, n_img)      # nothing hides anything


def test_out_of_range_corner_is_an_error_and_corrupts_nothing():
    from vdn_hip import lib, mesh
    c = valid_case()
    V, F = len(c["v32"]), len(c["tri"])
    good = grids()[0.5]
    for index_dtype in (torch.int64, torch.int32):
        for bad in (-1, V, V + 1000, (1 << 40) if index_dtype == torch.int64 else (1 << 31) - 1):
            t = c["tri"].copy()
            t[17, 2] = bad
            with pytest.raises(ValueError):
                mesh.MeshGrid(dev(c["v32"]), dev(t, index_dtype), cell_size=0.5)
            with pytest.raises(ValueError):
                mesh.visibility_votes(dev(c["v32"]), dev(t, index_dtype), c["P"], (H, W))
            # the count pass on buffers of the test's own, canaries on both sides of each output
            G = 1024
            count = torch.full((good.n_cells + 2 * G,), -77, dtype=torch.int32, device=DEV)
            count[G:G + good.n_cells] = 0
            records = torch.full(((F + 2 * G) * 12,), 7.25, dtype=torch.float32, device=DEV)
            err = torch.tensor([0, -77, -77, -77], dtype=torch.int32, device=DEV)
            v, td = dev(c["v32"]), dev(t, index_dtype)
            a = good._geometry(lib.VdnRayGridArgs())
            a.vertices, a.triangles, a.V, a.F, a.index_bytes = v.data_ptr(), td.data_ptr(), V, F, td.element_size()
            a.cell_count, a.records, a.error = count[G:].data_ptr(), records[G * 12:].data_ptr(), err.data_ptr()
            lib.call("vdn_ray_bin_count", a, torch.cuda.current_stream().cuda_stream)
            assert err.tolist() == [1, -77, -77, -77]
            assert (count[:G] == -77).all() and (count[G + good.n_cells:] == -77).all()
            assert (records[:G * 12] == 7.25).all() and (records[(G + F) * 12:] == 7.25).all()
            assert (records[(G + 17) * 12:(G + 18) * 12] == 0).all()       # the bad triangle's record is empty, and it is in no cell:
            without = mesh.MeshGrid(v, dev(np.delete(c["tri"], 17, axis=0)), cell_size=0.5)
            assert (without.lo, without.h, without.dims) == (good.lo, good.h, good.dims)
            assert torch.equal(torch.cumsum(count[G:G + good.n_cells], 0).to(torch.int32), without.cell_start[1:])
    # and the next well-formed grid is whole
    g = mesh.MeshGrid(dev(c["v32"]), dev(c["tri"]), cell_size=0.5)
    assert g.n_refs == good.n_refs and torch.equal(g.cell_start, good.cell_start)


def test_argument_errors():
    from vdn_hip import mesh
    c = valid_case()
    v, t = dev(c["v32"]), dev(c["tri"])
    with pytest.raises(ValueError):
        mesh.MeshGrid(v, t, cell_size=0.01, max_refs=1000)                # more references than allowed: refused after the count pass
    quad = c["tri"][(c["part"][c["tri"]] == 3).all(axis=1)]
    with pytest.raises(ValueError):
        mesh.MeshGrid(v, dev(np.concatenate([quad, c["tri"][:50]])), cell_size=0.02, max_refs=1 << 14)      # one huge triangle over a fine grid
    assert mesh.MeshGrid(v, dev(quad), cell_size=0.02, max_cells=1 << 12).n_cells <= 1 << 12                # max_cells raises h instead
    for bad in (lambda: mesh.MeshGrid(v, t.float()), lambda: mesh.MeshGrid(v, t[:, :2]), lambda: mesh.MeshGrid(v[:, :2], t),
                lambda: mesh.MeshGrid(v.long(), t), lambda: mesh.MeshGrid(v, t.to(torch.int16)), lambda: mesh.MeshGrid(v, t, cell_size=0.0),
                lambda: mesh.MeshGrid(v, t, cell_size=float("nan")), lambda: mesh.MeshGrid(v, t, max_cells=0), lambda: mesh.MeshGrid(v[:0], t)):
        with pytest.raises(ValueError):
            bad()
    g = grids()[None]
    o, d = c["origins"][:10], c["directions"][:10]
    for bad in (lambda: g.cast(o, d[:9]), lambda: g.cast(o[:, :2], d[:, :2]), lambda: g.cast(o.astype(np.int64), d), lambda: g.cast(o[0], d[0]),
                lambda: g.cast(o, d, skip_vertex=np.zeros(9, np.int64)), lambda: g.cast(o, d, skip_vertex=np.zeros(10)),
                lambda: g.cast(o, d, skip_vertex=np.zeros(10, bool))):
        with pytest.raises(ValueError):
            bad()
    assert g.cast(o.astype(np.float32), dev(d).float())[1].shape == (10,)                                   # float32 rays are widened
    for bad in (lambda: mesh.visibility_votes(v, t, c["P"][:, :, :3], (H, W)), lambda: mesh.visibility_votes(v, t, c["P"], (H,)),
                lambda: mesh.visibility_votes(v, t, c["P"], (0, W)), lambda: mesh.visibility_votes(v, t, c["P"], (H, W), eps=1.0),
                lambda: mesh.visibility_votes(v, t, c["P"] * 0.0, (H, W)), lambda: mesh.visibility_votes(v, t, c["P"], (H, W), grid=3),
                lambda: mesh.visibility_votes(v, t[:100], c["P"], (H, W), grid=g)):
        with pytest.raises(ValueError):
            bad()


# ---- votes ------------------------------------------------------------------------------------------------------------------------
def test_visibility_votes_equal_the_model():
    from vdn_hip import mesh
    c = valid_case()
    v, t = dev(c["v32"]), dev(c["tri"])
    want_img, want_vis = c["votes"]
    for h, g in grids().items():
        n_img, n_vis = mesh.visibility_votes(v, t, c["P"], (H, W), grid=g)
        assert n_img.dtype == n_vis.dtype == torch.int32 and n_img.shape == n_vis.shape == (len(c["v32"]),)
        assert np.array_equal(n_img.cpu().numpy(), want_img), h
        wrong = np.nonzero(n_vis.cpu().numpy() != want_vis)[0]
        assert len(wrong) == 0, (h, wrong, n_vis.cpu().numpy()[wrong], want_vis[wrong])
    own = mesh.visibility_votes(v.double(), dev(c["tri"], torch.int32), dev(c["P"]), (H, W))              # a grid of its own, P on the device
    assert np.array_equal(own[1].cpu().numpy(), want_vis)
    masks = torch.ones(len(c["P"]), H, W, dtype=torch.uint8, device=DEV)
    assert torch.equal(mesh.mask_votes(v, c["P"], masks)[0], own[0])                                        # one "in image" rule
    assert (want_vis[c["part"] == 1] == 0).all() and (own[1].cpu().numpy()[c["part"] == 1] == 0).all()      # the inner sphere: unseen
    # eps: with the segment's end left open by a wide margin, the faces just behind a vertex stop counting, never the reverse
    loose = mesh.visibility_votes(v, t, c["P"], (H, W), eps=0.5)[1]
    assert (loose >= own[1]).all() and (loose > own[1]).any()
    m_img, m_vis, amb = np_visibility(c["v32"], c["tri"], c["P"], H, W, eps=0.5, return_ambiguous=True)
    assert amb == 0 and np.array_equal(loose.cpu().numpy(), m_vis)
    e = mesh.visibility_votes(v[:0], t[:0], c["P"], (H, W))
    assert e[0].shape == e[1].shape == (0,)


# ---- cleaning ---------------------------------------------------------------------------------------------------------------------
def np_filter(v, t, kv):
    alive = kv[t].all(axis=1)
    used = np.zeros(len(v), bool)
    used[t[alive].reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[t[alive]].astype(t.dtype), np.nonzero(used)[0]


def clean_case():
    c = valid_case()
    return c, c["v32"], c["tri"]


def test_clean_mesh_drops_what_no_camera_sees():
    from vdn_train import mesh_clean
    c, v32, tri = clean_case()
    want_vis = c["votes"][1]
    keep = want_vis >= 1
    want = np_filter(v32, tri, keep)
    nrm = np.random.default_rng(3).normal(size=(len(v32), 3)).astype(np.float32)
    col = np.random.default_rng(4).integers(0, 256, (len(v32), 3)).astype(np.uint8)
    res = mesh_clean.clean_mesh(v32, tri, keep="all", cameras=c["P"], image_size=(H, W), visibility={"min_visible": 1}, attributes=[nrm, col])
    assert isinstance(res["vertices"], np.ndarray) and res["vertices"].dtype == v32.dtype and res["triangles"].dtype == tri.dtype
    assert np.array_equal(res["vertex_index"], want[2]) and np.array_equal(res["triangles"], want[1]) and np.array_equal(res["vertices"], want[0])
    assert np.array_equal(res["attributes"][0], nrm[want[2]]) and np.array_equal(res["attributes"][1], col[want[2]])
    part, z = c["part"][res["vertex_index"]], res["vertices"][:, 2]
    assert not (part == 1).any()                                           # the inner sphere is gone,
    assert not ((part == 0) & (z < -0.5)).any()                            # and the underside nobody sees;
    up = (c["part"] == 0) & (v32[:, 2] > 0.15)
    assert np.isin(np.nonzero(up)[0], res["vertex_index"]).all()           # the upper outer sphere stays
    rep = res["report"]
    assert json.loads(json.dumps(rep)) == rep and "mask_culling" not in rep
    vc = rep["visibility_culling"]
    assert set(vc) == {"cameras", "min_visible", "eps", "vertices_removed", "faces_removed", "components_after"}
    assert (vc["cameras"], vc["min_visible"], vc["eps"]) == (6, 1, 1e-4)
    # (keep="all" without thresholds drops no face before the stage, but the vertices no face uses: the degenerate corners stay
    # referenced, so stage 2 hands over every vertex)
    assert vc["vertices_removed"] == len(v32) - len(want[0]) and vc["faces_removed"] == len(tri) - len(want[1])
    assert vc["components_after"] >= 1 and rep["vertices_out"] == len(want[0]) and rep["faces_out"] == len(want[1])
    # device tensors, int32 faces, a stricter vote and a chosen cell size
    rd = mesh_clean.clean_mesh(dev(v32), dev(tri, torch.int32), keep="all", cameras=c["P"], image_size=(H, W),
                               visibility={"min_visible": 2, "cell_size": 0.3, "eps": 1e-4})
    w2 = np_filter(v32, tri, want_vis >= 2)
    assert rd["vertices"].is_cuda and rd["triangles"].dtype == torch.int32 and np.array_equal(rd["triangles"].cpu().numpy(), w2[1])
    assert np.array_equal(rd["vertex_index"].cpu().numpy(), w2[2]) and rd["report"]["visibility_culling"]["min_visible"] == 2
    # min_visible = 0 keeps everything the earlier stages kept
    r0 = mesh_clean.clean_mesh(v32, tri, keep="all", cameras=c["P"], image_size=(H, W), visibility={"min_visible": 0})
    assert np.array_equal(r0["triangles"], tri) and r0["report"]["visibility_culling"]["vertices_removed"] == 0


def test_dropped_pieces_cast_no_shadow_and_masks_supply_the_image_size():
    from vdn_train import mesh_clean
    c, v32, tri = clean_case()
    masks = np.ones((len(c["P"]), H, W), np.uint8)
    # keep="largest": only the outer sphere's component reaches stage 3 - the inner sphere, the floater and the ground are gone
    res = mesh_clean.clean_mesh(v32, tri, keep="largest", cameras=c["P"], masks=masks, visibility={})
    kept = c["part"][res["vertex_index"]]
    assert (kept == 0).all() and res["report"]["mask_culling"]["vertices_removed"] >= 1 and res["report"]["components"]["after"] == 1
    outer = np.nonzero((c["part"][tri] == 0).all(axis=1))[0]
    alone_v, alone_t, alone_i = np_filter(v32, tri[outer], np.ones(len(v32), bool))
    img, vis, amb = np_visibility(alone_v, alone_t, c["P"], H, W, return_ambiguous=True)
    assert amb == 0
    want = np_filter(alone_v, alone_t, vis >= 1)
    assert np.array_equal(res["vertex_index"], alone_i[want[2]]) and np.array_equal(res["triangles"], want[1])
    full = c["votes"][1][alone_i]                                          # with fewer occluders no vertex is seen by fewer cameras
    assert (vis >= full).all()
    with pytest.raises(ValueError):
        mesh_clean.clean_mesh(v32, tri, cameras=c["P"], masks=masks, image_size=(H + 1, W), visibility={})


def test_visibility_none_is_todays_output():
    from vdn_train import mesh_clean
    c, v32, tri = clean_case()
    masks = (np.random.default_rng(9).random((len(c["P"]), H, W)) > 0.02).astype(np.uint8)
    a = mesh_clean.clean_mesh(v32, tri, keep="all", cameras=c["P"], masks=masks, max_outside=1, visibility=None)
    b = mesh_clean.clean_mesh(v32, tri, keep="all", cameras=c["P"], masks=masks, max_outside=1)
    # today's pipeline, stage by stage, from its own parts
    from vdn_hip import mesh
    n_img, n_msk = mesh.mask_votes(dev(v32), c["P"], dev(masks))
    v1, t1, i1 = mesh.filter_mesh(dev(v32), dev(tri), keep_vertices=mesh_clean.vote_keep(n_img, n_msk, 1, 1))
    for r in (a, b):
        assert "visibility_culling" not in r["report"] and r["report"] == a["report"]
        assert np.array_equal(r["vertices"], v1.cpu().numpy()) and np.array_equal(r["triangles"], t1.cpu().numpy())
        assert np.array_equal(r["vertex_index"], i1.cpu().numpy())
    assert 0 < len(a["vertices"]) < len(v32)


def test_validate_mesh_with_visibility_culling(tmp_path):
    from test_gpu_mesh_clean import _renderer, look_at
    from vdn_train import mesh_clean, meshio, validate
    rend = _renderer()
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    kw = dict(resolution=24, world_space=True, scale_mat=np.array([[2.5, 0, 0, 0.5], [0, 2.5, 0, -1.0], [0, 0, 2.5, 3.0], [0, 0, 0, 1.0]]))
    raw_path, V, F = validate.validate_mesh(rend, lo, hi, str(tmp_path / "raw.ply"), **kw)
    # one camera on the z axis: what faces away from it goes
    Hc, Wc = 32, 48
    P = look_at((0, 0, 3.0), 12.0, Hc, Wc)[None]
    clean = dict(keep="all", visibility={"min_visible": 1}, cameras=P, image_size=(Hc, Wc))
    path, Vc, Fc = validate.validate_mesh(rend, lo, hi, str(tmp_path / "seen.ply"), clean=clean, **kw)
    raw, got = meshio.read_ply(raw_path), meshio.read_ply(path)
    assert (Vc, Fc) == (len(got["vertices"]), len(got["triangles"])) and 0 < Fc < F and 0 < Vc < V
    v, t = rend.extract_geometry(lo, hi, resolution=24, threshold=0.0)
    res = mesh_clean.clean_mesh(v, t, **clean)
    idx = res["vertex_index"]
    assert len(idx) == Vc and np.array_equal(got["triangles"], res["triangles"])
    assert np.array_equal(got["vertices"], raw["vertices"][idx])
    assert np.array_equal(got["normals"], raw["normals"][idx]) and np.array_equal(got["colors"], raw["colors"][idx])      # they followed their vertices
    assert res["report"]["visibility_culling"]["vertices_removed"] == V - Vc > 0
