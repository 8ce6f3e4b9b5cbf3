"""Mesh cleaning on the device (csrc/mesh_clean.hip, vdn_hip/mesh.py, vdn_train/mesh_clean.py) against the numpy restatements of
test_mesh_clean_cpu.py: canonical labels of a plain union-find (exact), face areas in float64, the brute-force window maximum
(exact), a float64 projection (exact votes, on vertices kept clear of every rounding boundary), numpy fancy indexing for the
compaction, and the way through clean_mesh and validate_mesh."""
import os

import numpy as np
import pytest
import torch

from test_mesh_clean_cpu import np_dilate, np_labels, np_project, np_votes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


def dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


# ---- labels -----------------------------------------------------------------------------------------------------------------------
def strip(n, number):
    """n triangles (i, i+1, i+2) over n + 2 vertices, vertex k renamed number[k]"""
    i = np.arange(n)
    return np.asarray(number)[np.stack([i, i + 1, i + 2], axis=1)], n + 2


def label_cases():
    if "labels" in _CACHE:
        return _CACHE["labels"]
    rng = np.random.default_rng(2024)
    cases = {}
    for F in (0, 1, 63, 64, 65, 257):
        cases["random_%d" % F] = (rng.integers(0, 300, (F, 3)), 300)
    cases["disjoint_2000"] = (rng.permutation(6000).reshape(2000, 3), 6000)
    cases["strip_permuted"] = strip(5000, rng.permutation(5002))
    cases["strip_descending"] = strip(5000, np.arange(5002)[::-1])
    # two fans (centres 0 and 21) whose rims meet at vertex 20: one component
    fan1 = [(0, k, k + 1) for k in range(1, 20)]
    fan2 = [(21, k, k + 1) for k in range(22, 40)] + [(21, 40, 20)]
    cases["two_fans"] = (np.array(fan1 + fan2), 41)
    # every third vertex is in no triangle
    used = np.array([k for k in range(150) if k % 3 != 0])
    cases["isolated_50"] = (used[rng.integers(0, len(used), (40, 3))], 150)
    deg = [(5, 5, 9), (9, 9, 9), (2, 3, 3), (7, 8, 7), (10, 11, 12), (10, 11, 12), (12, 11, 10), (5, 5, 9)]
    cases["degenerate_and_repeated"] = (np.array(deg), 14)
    _CACHE["labels"] = {k: (np.asarray(t, np.int64).reshape(-1, 3), V, np_labels(t, V)) for k, (t, V) in cases.items()}
    return _CACHE["labels"]


CASE_NAMES = ["random_0", "random_1", "random_63", "random_64", "random_65", "random_257", "disjoint_2000", "strip_permuted",
              "strip_descending", "two_fans", "isolated_50", "degenerate_and_repeated"]


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_labels_equal_the_canonical_union_find_labels(name, index_dtype):
    from vdn_hip import mesh
    tri, V, want = label_cases()[name]
    t = dev(tri, index_dtype)
    got = mesh.connected_components(t, V)
    assert got.dtype == torch.int32 and got.shape == (V,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(mesh.connected_components(t, V), got)                       # two calls: the same bits
    perm = np.random.default_rng(5).permutation(len(tri))
    assert torch.equal(mesh.connected_components(dev(tri[perm], index_dtype), V), got)       # any order of the triangles
    # the contract itself: each label is the smallest index that carries it
    lab = got.cpu().numpy()
    assert np.array_equal(lab[lab], lab) and (lab <= np.arange(V)).all()


def test_label_case_properties():
    c = label_cases()
    assert len(np.unique(c["disjoint_2000"][2])) == 2000 and len(np.unique(c["two_fans"][2])) == 1
    assert len(np.unique(c["strip_permuted"][2])) == 1 and (c["strip_descending"][2] == 0).all()
    iso = c["isolated_50"][2]
    assert all(iso[k] == k for k in range(0, 150, 3))
    assert set(CASE_NAMES) == set(c)


def test_out_of_range_corner_is_an_error_and_corrupts_nothing():
    from vdn_hip import mesh
    tri, V, want = label_cases()["random_257"]
    for bad in (-1, V, 1 << 40):
        t = tri.copy()
        t[100, 1] = bad
        with pytest.raises(ValueError):
            mesh.connected_components(dev(t), V)
        with pytest.raises(ValueError):
            mesh.filter_mesh(torch.zeros(V, 3, device=DEV), dev(t))
        with pytest.raises(ValueError):
            mesh.triangle_areas(torch.zeros(V, 3, device=DEV), dev(t))
    t32 = tri.astype(np.int32)
    t32[0, 0] = V
    with pytest.raises(ValueError):
        mesh.connected_components(dev(t32), V)
    assert np.array_equal(mesh.connected_components(dev(tri), V).cpu().numpy(), want)
    with pytest.raises(ValueError):
        mesh.connected_components(dev(tri), -1)
    with pytest.raises(ValueError):
        mesh.connected_components(dev(tri).float(), V)
    with pytest.raises(ValueError):
        mesh.connected_components(dev(tri)[:, :2], V)
    assert mesh.connected_components(dev(tri[:0]), 0).shape == (0,)
    assert mesh.connected_components(dev(tri[:0]), 7).tolist() == list(range(7))


# ---- the lattice mesh: two separated spheres and a small blob -----------------------------------------------------------------------
R = 48
BIG, SMALL, BLOB = ((-0.45, 0.0, 0.0), 0.35), ((0.5, 0.1, 0.0), 0.25), ((0.0, 0.7, 0.5), 0.1)


def lattice_mesh():
    """-> (vertices [V,3] float64 in [-1, 1]^3, triangles [F,3] int64, owner [V]: 0 big sphere, 1 small sphere, 2 blob), numpy"""
    if "lattice" not in _CACHE:
        from vdn_hip import mesh
        g = np.linspace(-1.0, 1.0, R)
        x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1)
        d = np.stack([np.linalg.norm(x - np.array(c), axis=-1) - r for c, r in (BIG, SMALL, BLOB)], axis=-1)
        v, t = mesh.marching_cubes(dev(d.min(axis=-1), torch.float32), 0.0)
        v = v.cpu().numpy() / (R - 1.0) * 2.0 - 1.0
        owner = np.stack([np.abs(np.linalg.norm(v - np.array(c), axis=1) - r) for c, r in (BIG, SMALL, BLOB)], axis=1).argmin(axis=1)
        _CACHE["lattice"] = (v, t.cpu().numpy(), owner)
    return _CACHE["lattice"]


def test_lattice_mesh_has_exactly_three_components():
    from vdn_hip import mesh
    v, t, owner = lattice_mesh()
    V = len(v)
    assert len(t) > 3000 and (np.bincount(owner, minlength=3) > 0).all()
    got = mesh.connected_components(dev(t), V).cpu().numpy()
    assert np.array_equal(got, np_labels(t, V))
    assert len(np.unique(got)) == 3
    for k in range(3):                                              # one label per surface
        assert len(np.unique(got[owner == k])) == 1
    assert torch.equal(mesh.connected_components(dev(t[np.random.default_rng(1).permutation(len(t))]), V).cpu(), torch.from_numpy(got))


# ---- table ------------------------------------------------------------------------------------------------------------------------
def np_areas(v32, t):
    p = np.asarray(v32, np.float32).astype(np.float64)[t]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def table_meshes():
    v, t, _ = lattice_mesh()
    rng = np.random.default_rng(8)
    yield "lattice", v.astype(np.float32), t
    yield "random", (rng.normal(size=(300, 3)) * 3.0).astype(np.float32), label_cases()["random_257"][0]
    yield "isolated", rng.normal(size=(150, 3)).astype(np.float32), label_cases()["isolated_50"][0]


def test_component_table_counts_exact_and_areas_in_double():
    from vdn_hip import mesh
    for name, v32, t in table_meshes():
        V, F = len(v32), len(t)
        vd, td = dev(v32), dev(t)
        labels = mesh.connected_components(td, V)
        tab = {k: x.cpu().numpy() for k, x in mesh.component_table(vd, td, labels).items()}
        lab = np_labels(t, V)
        root, vc = np.unique(lab, return_inverse=True)
        C = len(root)
        assert tab["root"].dtype == np.int64 and np.array_equal(tab["root"], root), name
        assert np.array_equal(tab["vertex_component"], vc) and np.array_equal(tab["face_component"], vc[t[:, 0]]), name
        assert np.array_equal(tab["n_vertices"], np.bincount(vc, minlength=C)) and tab["n_vertices"].dtype == np.int64, name
        assert np.array_equal(tab["n_faces"], np.bincount(vc[t[:, 0]], minlength=C)) and tab["n_faces"].dtype == np.int64, name
        assert tab["n_vertices"].sum() == V and tab["n_faces"].sum() == F
        # a handful of fp64 roundings on differences bounded by the bounding-box diagonal
        diag2 = float(((v32.astype(np.float64).max(axis=0) - v32.astype(np.float64).min(axis=0)) ** 2).sum())
        ref = np_areas(v32, t)
        assert tab["face_area"].dtype == np.float64 and tab["face_area"].shape == (F,)
        err = np.abs(tab["face_area"] - ref).max()
        print(name, "max face area error", err, "bound", 1e-14 * diag2)
        assert err <= 1e-14 * diag2, name
        want = np.bincount(vc[t[:, 0]], weights=ref, minlength=C)
        err_c = np.abs(tab["area"] - want)
        bound = tab["n_faces"] * 1e-14 * diag2 + 1e-12 * want
        print(name, "max component area error / bound", (err_c / np.maximum(bound, 1e-300)).max())
        assert tab["area"].dtype == np.float64 and (err_c <= bound).all(), name
        assert torch.equal(mesh.triangle_areas(vd, dev(t, torch.int32)).cpu(), torch.from_numpy(tab["face_area"])), name


def test_non_finite_vertices_give_zero_area():
    from vdn_hip import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e38, 3e38, 0]], np.float32)
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 0, 1], [0, 1, 5]])
    got = mesh.triangle_areas(dev(v), dev(t)).cpu().numpy()
    assert got[0] == 0.5 and got[1] == 0.0 and got[2] == 0.0 and got[3] == 0.0 and np.isfinite(got[4]) and got[4] > 1e38


# ---- dilation ---------------------------------------------------------------------------------------------------------------------
def blob_masks():
    """3 x 37 x 53, random blobs, some on each of the four borders (and the four corner pixels set in plane 0)"""
    if "masks" not in _CACHE:
        rng = np.random.default_rng(77)
        N, H, W = 3, 37, 53
        m = np.zeros((N, H, W), np.uint8)
        yy, xx = np.mgrid[:H, :W]
        centres = [(0, 7), (H - 1, 40), (20, 0), (11, W - 1)] + [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(5)]
        for n in range(N):
            for cy, cx in centres:
                cy, cx = (cy + 3 * n) % H if cy not in (0, H - 1) else cy, (cx + 5 * n) % W if cx not in (0, W - 1) else cx
                m[n][(yy - cy) ** 2 + (xx - cx) ** 2 <= int(rng.integers(1, 9))] = 255 if n < 2 else 1
        m[0, [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 7
        _CACHE["masks"] = m
    return _CACHE["masks"]


@pytest.mark.parametrize("r", [0, 1, 3, 40])
def test_dilation_equals_the_window_maximum(r):
    from vdn_hip import mesh
    m = blob_masks()
    for n in range(3):
        assert m[n, 0].any() and m[n, -1].any() and m[n, :, 0].any() and m[n, :, -1].any() and not m[n].all()
    src = dev(m)
    got = mesh.dilate_masks(src, r)
    assert got.dtype == torch.uint8 and got.shape == src.shape and torch.equal(src.cpu(), torch.from_numpy(m))      # the input is untouched
    want = np_dilate(m, r)
    assert np.array_equal(got.cpu().numpy(), want)
    if r == 0:
        assert np.array_equal(want, m) and got.data_ptr() != src.data_ptr()
    if r == 40:                                                       # larger than the image height: all-set columns
        assert (want.min(axis=1) > 0).any()
    one = mesh.dilate_masks(src[1:2, :5, :1].contiguous(), r)         # a single column
    assert np.array_equal(one.cpu().numpy(), np_dilate(m[1:2, :5, :1], r))


def test_dilation_argument_errors():
    from vdn_hip import mesh
    src = dev(blob_masks())
    for bad in (lambda: mesh.dilate_masks(src, -1), lambda: mesh.dilate_masks(src, 1.5), lambda: mesh.dilate_masks(src.float(), 1),
                lambda: mesh.dilate_masks(src[0], 1), lambda: mesh.dilate_masks(src[:0], 1)):
        with pytest.raises(ValueError):
            bad()


# ---- votes ------------------------------------------------------------------------------------------------------------------------
def look_at(c, f, H, W):
    """3 x 4 projection of a pinhole at c looking at the origin, focal f px, principal point at the image centre"""
    c = np.asarray(c, np.float64)
    fwd = -c / np.linalg.norm(c)
    right = np.cross(fwd, [0.0, 0.0, 1.0] if abs(fwd[2]) < 0.9 else [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    rot = np.stack([right, np.cross(fwd, right), fwd])               # world -> camera, z forward
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return K @ np.concatenate([rot, -(rot @ c)[:, None]], axis=1)


def clear_of_boundaries(v32, P):
    """every projection with w > 0 is >= 0.05 px from a rounding boundary, and |w| > 1e-3 everywhere"""
    u, v, w = np_project(v32, P)
    fu, fv = u + 0.5 - np.floor(u + 0.5), v + 0.5 - np.floor(v + 0.5)
    with np.errstate(invalid="ignore"):
        ok = (w <= 0) | ((fu >= 0.05) & (fu <= 0.95) & (fv >= 0.05) & (fv <= 0.95))
    return (ok & (np.abs(w) > 1e-3)).all(axis=0)


def vote_case():
    if "votes" in _CACHE:
        return _CACHE["votes"]
    rng = np.random.default_rng(31)
    N, H, W, V = 6, 40, 56, 4000
    # all cameras on the z > 0 side, looking at the origin: a point far up the z axis is behind every one of them
    cams = [(3 * np.cos(a) * 0.8, 3 * np.sin(a) * 0.8, 1.8 + 0.2 * k) for k, a in enumerate(np.linspace(0, 2 * np.pi, N, endpoint=False))]
    P = np.stack([look_at(c, 45.0, H, W) for c in cams])

    def draw(kind, n):
        if kind == 0:                                                # through a pixel of one camera, at a random depth
            out = np.empty((n, 3))
            for i in range(n):
                Pn = P[rng.integers(0, N)]
                uv = np.array([rng.integers(0, W), rng.integers(0, H)]) + rng.uniform(-0.4, 0.4, 2)
                depth = rng.uniform(1.0, 5.0)
                out[i] = np.linalg.solve(Pn[:, :3], depth * np.array([uv[0], uv[1], 1.0]) - Pn[:, 3])
            return out
        if kind == 1:                                                # behind every camera
            return np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(8, 20, n)], axis=1)
        a, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(40, 80, n)   # far outside every frustum: above the horizon of cameras that look down
        return np.stack([rad * np.cos(a), rad * np.sin(a), rng.uniform(5, 8, n)], axis=1)
    kinds = np.concatenate([np.zeros(V - 200, int), np.ones(100, int), np.full(100, 2)])
    v32 = np.concatenate([draw(k, int((kinds == k).sum())) for k in (0, 1, 2)]).astype(np.float32)
    for _ in range(60):                                              # input construction: re-draw what sits near a boundary
        bad = np.nonzero(~clear_of_boundaries(v32, P))[0]
        if len(bad) == 0:
            break
        for k in (0, 1, 2):
            sel = bad[kinds[bad] == k]
            v32[sel] = draw(k, len(sel)).astype(np.float32)
    masks = (rng.random((N, H, W)) > 0.5).astype(np.uint8) * np.array([1, 255, 3, 1, 128, 1], np.uint8)[:, None, None]
    _CACHE["votes"] = (v32, P, masks, kinds)
    return _CACHE["votes"]


def test_votes_equal_the_float64_projection():
    from vdn_hip import mesh
    v32, P, masks, kinds = vote_case()
    assert v32.shape == (4000, 3) and P.shape == (6, 3, 4)
    assert clear_of_boundaries(v32, P).all()                         # none left after the re-draws, or the case is not valid
    n_img, n_msk = np_votes(v32, P, masks)
    _, _, w = np_project(v32, P)
    assert (w[:, kinds == 1] < 0).all() and (n_img[kinds == 1] == 0).all() and (n_img[kinds == 2] == 0).all()
    assert (n_img[kinds == 0] >= 1).all() and n_img.max() >= 3 and 0 < n_msk.sum() < n_img.sum()
    got_img, got_msk = mesh.mask_votes(dev(v32), P, dev(masks))
    assert got_img.dtype == got_msk.dtype == torch.int32
    assert np.array_equal(got_img.cpu().numpy(), n_img) and np.array_equal(got_msk.cpu().numpy(), n_msk)
    # P as a device tensor, float64 vertices (cast to fp32 on the way in), a zero-vertex call
    got2 = mesh.mask_votes(dev(v32.astype(np.float64)), dev(P), dev(masks))
    assert torch.equal(got2[0], got_img) and torch.equal(got2[1], got_msk)
    e = mesh.mask_votes(dev(v32[:0]), P, dev(masks))
    assert e[0].shape == (0,) and e[1].shape == (0,)
    # non-finite vertices are in no image
    odd = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, 0]], np.float32)
    o_img, o_msk = mesh.mask_votes(dev(odd), P, dev(masks))
    assert o_img.tolist()[:3] == [0, 0, 0] and o_msk.tolist()[:3] == [0, 0, 0] and o_img[3].item() == 6      # the origin: the centre of every image
    for bad in (lambda: mesh.mask_votes(dev(v32), P[:5], dev(masks)), lambda: mesh.mask_votes(dev(v32), P, dev(masks).float()),
                lambda: mesh.mask_votes(dev(v32)[:, :2], P, dev(masks))):
        with pytest.raises(ValueError):
            bad()


# ---- compaction -------------------------------------------------------------------------------------------------------------------
def np_filter(v, t, kv=None, kf=None, drop=True):
    alive = np.ones(len(t), bool) if kf is None else kf.copy()
    if kv is not None:
        alive &= kv[t].all(axis=1)
    used = np.zeros(len(v), bool)
    used[t[alive].reshape(-1)] = True
    keep = used if drop else (np.ones(len(v), bool) if kv is None else kv)
    index = np.nonzero(keep)[0]
    new = np.cumsum(keep) - 1
    return v[index], new[t[alive]].astype(t.dtype), index


@pytest.mark.parametrize("index_dtype", [np.int64, np.int32])
@pytest.mark.parametrize("F", [1, 64, 65, 1000])
def test_filter_mesh_equals_numpy_fancy_indexing(F, index_dtype):
    from vdn_hip import mesh
    rng = np.random.default_rng(F)
    V = F + 10
    v = rng.normal(size=(V, 3))
    t = rng.integers(0, V, (F, 3)).astype(index_dtype)
    kv, kf = rng.random(V) > 0.15, rng.random(F) > 0.3
    if F == 1:
        kv[t[0]], kf[0] = True, True
    for vd in (v.astype(np.float32), v):                             # the vertices' own dtype comes back
        for kwv, kwf, drop in ((kv, kf, True), (kv, None, True), (None, kf, True), (kv, kf, False), (None, kf, False), (None, None, True),
                               (None, None, False)):
            want = np_filter(vd, t, kwv, kwf, drop)
            got = mesh.filter_mesh(dev(vd), dev(t), None if kwv is None else dev(kwv), None if kwf is None else dev(kwf), drop_unreferenced=drop)
            assert got[0].dtype == dev(vd).dtype and got[1].dtype == dev(t).dtype and got[2].dtype == torch.int64
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g.cpu().numpy(), w)
            assert torch.equal(dev(vd)[got[2]], got[0])              # vertices[vertex_index] round-trips
    # all dropped: [0,3] arrays
    for kw in (dict(keep_faces=dev(np.zeros(F, bool))), dict(keep_vertices=dev(np.zeros(V, bool)))):
        e = mesh.filter_mesh(dev(v), dev(t), **kw)
        assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,) and e[1].dtype == dev(t).dtype
    # all kept on a mesh without an unreferenced vertex: the identity
    ts, Vs = strip(F, np.arange(F + 2))
    ts = ts.astype(index_dtype)
    vs = rng.normal(size=(Vs, 3)).astype(np.float32)
    for kw in ({}, dict(keep_vertices=dev(np.ones(Vs, bool)), keep_faces=dev(np.ones(F, bool)))):
        i = mesh.filter_mesh(dev(vs), dev(ts), **kw)
        assert np.array_equal(i[0].cpu().numpy(), vs) and np.array_equal(i[1].cpu().numpy(), ts) and i[2].tolist() == list(range(Vs))
    # uint8 keeps count as bool; a wrong length is refused
    u = mesh.filter_mesh(dev(v), dev(t), keep_faces=dev(kf.astype(np.uint8) * 3))
    assert np.array_equal(u[1].cpu().numpy(), np_filter(v, t, None, kf)[1])
    with pytest.raises(ValueError):
        mesh.filter_mesh(dev(v), dev(t), keep_faces=dev(np.ones(F + 1, bool)))
    with pytest.raises(ValueError):
        mesh.filter_mesh(dev(v), dev(t), keep_vertices=dev(np.ones(V, np.int64)))


def test_filter_mesh_without_faces():
    from vdn_hip import mesh
    v = dev(np.arange(12.0).reshape(4, 3))
    t = torch.zeros(0, 3, dtype=torch.int64, device=DEV)
    a = mesh.filter_mesh(v, t)
    assert a[0].shape == (0, 3) and a[1].shape == (0, 3) and a[2].shape == (0,)
    b = mesh.filter_mesh(v, t, keep_vertices=dev(np.array([True, False, True, True])), drop_unreferenced=False)
    assert b[2].tolist() == [0, 2, 3] and torch.equal(b[0], v[[0, 2, 3]])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def silhouette_masks(cams, f, H, W, centre, radius):
    """mask[n, y, x] = the ray of camera n through pixel (x, y) passes within `radius` of `centre`"""
    m = np.zeros((len(cams), H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    pix = np.stack([xx, yy, np.ones_like(xx)], axis=-1).reshape(-1, 3).astype(np.float64)
    for n, c in enumerate(cams):
        P = look_at(c, f, H, W)
        d = np.linalg.solve(P[:, :3], pix.T).T                      # ray directions in the world
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        s = np.asarray(centre) - np.asarray(c, np.float64)
        off = np.linalg.norm(s[None] - (d @ s)[:, None] * d, axis=1)
        m[n] = ((off <= radius) & (d @ s > 0)).reshape(H, W)
    return m


def test_clean_mesh_keeps_the_big_sphere():
    from vdn_train import mesh_clean
    v, t, owner = lattice_mesh()
    want = np_filter(v, t, None, owner[t[:, 0]] == 0)
    nrm = np.random.default_rng(3).normal(size=(len(v), 3)).astype(np.float32)
    col = np.random.default_rng(4).integers(0, 256, (len(v), 3)).astype(np.uint8)
    res = mesh_clean.clean_mesh(v, t, keep="largest", attributes=[nrm, col])
    assert isinstance(res["vertices"], np.ndarray) and res["vertices"].dtype == v.dtype and res["triangles"].dtype == t.dtype
    assert np.array_equal(res["vertices"], want[0]) and np.array_equal(res["triangles"], want[1]) and np.array_equal(res["vertex_index"], want[2])
    assert np.array_equal(res["attributes"][0], nrm[want[2]]) and np.array_equal(res["attributes"][1], col[want[2]])
    rep = res["report"]
    import json
    assert json.loads(json.dumps(rep)) == rep
    assert rep["components_in"] == 3 and rep["components"]["before"] == 3 and rep["components"]["after"] == 1 and "mask_culling" not in rep
    assert rep["components"]["faces_removed"] == int((owner[t[:, 0]] != 0).sum()) and rep["components"]["vertices_removed"] == int((owner != 0).sum())
    assert (rep["vertices_in"], rep["faces_in"], rep["vertices_out"], rep["faces_out"]) == (len(v), len(t), len(want[0]), len(want[1]))
    areas = np.bincount(owner[t[:, 0]], weights=np_areas(v, t), minlength=3)
    assert abs(rep["components"]["kept_area_fraction"] - areas[0] / areas.sum()) < 1e-9
    # device tensors in, device tensors out; by area the same piece; thresholds keep two of the three
    rd = mesh_clean.clean_mesh(dev(v), dev(t, torch.int32), by="area", attributes=[dev(col)])
    assert rd["vertices"].is_cuda and rd["triangles"].dtype == torch.int32 and rd["vertex_index"].is_cuda
    assert np.array_equal(rd["triangles"].cpu().numpy(), want[1]) and np.array_equal(rd["attributes"][0].cpu().numpy(), col[want[2]])
    n_blob = int((owner[t[:, 0]] == 2).sum())
    two = mesh_clean.clean_mesh(v, t, keep="all", min_faces=n_blob + 1)
    w2 = np_filter(v, t, None, owner[t[:, 0]] != 2)
    assert np.array_equal(two["triangles"], w2[1]) and np.array_equal(two["vertex_index"], w2[2]) and two["report"]["components"]["after"] == 2
    everything = mesh_clean.clean_mesh(v, t, keep="all")
    assert np.array_equal(everything["triangles"], t) and np.array_equal(everything["vertices"], v)


def test_clean_mesh_culls_by_the_masks_first():
    from vdn_train import mesh_clean
    v, t, owner = lattice_mesh()
    H = W = 96
    cams = [(0, 0, 3.0), (0, 0, -3.0), (0, 3.0, 0), (0, -3.0, 0.3), (0, 2.1, 2.1), (0, -2.1, 2.1)]       # none along the spheres' axis
    P = np.stack([look_at(c, 100.0, H, W) for c in cams])
    # the big sphere's silhouette, grown by 0.04: the mesh lies inside the sphere and half a pixel is 0.015 at this distance
    masks = silhouette_masks(cams, 100.0, H, W, BIG[0], BIG[1] + 0.04)
    n_img, n_msk = np_votes(v.astype(np.float32), P, masks)
    assert (n_img == 6).all() and (n_msk[owner == 0] == 6).all() and (n_msk[owner != 0] < 6).all()          # the case is what it claims to be
    want = np_filter(v, t, owner == 0)
    for mk in (masks, masks.astype(bool), masks[..., None].astype(np.float32), np.repeat(masks[..., None], 3, 3).astype(np.float32) * 0.9):
        res = mesh_clean.clean_mesh(v, t, cameras=P, masks=mk)
        assert np.array_equal(res["triangles"], want[1]) and np.array_equal(res["vertices"], want[0]) and np.array_equal(res["vertex_index"], want[2])
        rep = res["report"]
        assert rep["components_in"] == 3 and rep["mask_culling"]["faces_removed"] == int((owner[t[:, 0]] != 0).sum())
        assert rep["mask_culling"]["vertices_removed"] == int((owner != 0).sum()) and rep["mask_culling"]["cameras"] == 6
        assert rep["components"]["before"] == 1 and rep["components"]["after"] == 1 and rep["components"]["faces_removed"] == 0
        assert rep["components"]["kept_area_fraction"] == 1.0
    # a tight silhouette loses the rim of the sphere; dilating it by 3 px brings the whole sphere back
    tight = silhouette_masks(cams, 100.0, H, W, BIG[0], BIG[1] - 0.05)
    t_img, t_msk = np_votes(v.astype(np.float32), P, tight)
    w_lost = np_filter(v, t, mesh_clean.vote_keep(t_img, t_msk, 1, 2))
    lost = mesh_clean.clean_mesh(v, t, cameras=P, masks=tight, keep="all", max_outside=2)
    assert np.array_equal(lost["triangles"], w_lost[1]) and 0 < lost["report"]["faces_out"] < len(want[1])
    none = mesh_clean.clean_mesh(v, t, cameras=P, masks=tight)      # every vertex is on some camera's rim: an empty mesh, not an error
    assert none["vertices"].shape == (0, 3) and none["triangles"].shape == (0, 3) and none["report"]["components"]["kept_area_fraction"] is None
    back = mesh_clean.clean_mesh(v, t, cameras=P, masks=tight, dilate=3)
    assert np.array_equal(back["triangles"], want[1])
    # votes relaxed until nothing is culled: the components stage then does the work, and the report says so
    lax = mesh_clean.clean_mesh(v, t, cameras=P, masks=masks, min_inside=0, max_outside=6)
    assert lax["report"]["mask_culling"]["faces_removed"] == 0 and lax["report"]["components"]["before"] == 3
    assert np.array_equal(lax["triangles"], want[1])


def _renderer():
    from vdn_train import factory, synth
    if "renderer" not in _CACHE:
        _CACHE["renderer"] = factory.build_renderer(device=torch.device(DEV), states=synth.make_all_states(0, variance=0.4), precision="bf16")
    return _CACHE["renderer"]


def test_validate_mesh_with_cleaning(tmp_path):
    from vdn_train import mesh_clean, meshio, validate
    rend = _renderer()
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    kw = dict(resolution=24, world_space=True, scale_mat=np.array([[2.5, 0, 0, 0.5], [0, 2.5, 0, -1.0], [0, 0, 2.5, 3.0], [0, 0, 0, 1.0]]))
    raw_path, V, F = validate.validate_mesh(rend, lo, hi, str(tmp_path / "raw.ply"), **kw)
    none_path, _, _ = validate.validate_mesh(rend, lo, hi, str(tmp_path / "none.ply"), clean=None, **kw)
    assert open(raw_path, "rb").read() == open(none_path, "rb").read()
    # one camera on the z axis whose mask is the left half of the image: about half of the surface goes
    H, W = 32, 48
    P = look_at((0, 0, 3.0), 12.0, H, W)[None]
    masks = np.zeros((1, H, W), np.float32)
    masks[:, :, :W // 2] = 1.0
    clean = dict(keep="largest", cameras=P, masks=masks)
    path, Vc, Fc = validate.validate_mesh(rend, lo, hi, str(tmp_path / "meshes" / "clean.ply"), clean=clean, **kw)
    raw, got = meshio.read_ply(raw_path), meshio.read_ply(path)
    assert (Vc, Fc) == (len(got["vertices"]), len(got["triangles"])) and 0 < Fc < F and 0 < Vc < V
    v, t = rend.extract_geometry(lo, hi, resolution=24, threshold=0.0)
    res = mesh_clean.clean_mesh(v, t, **clean)
    idx = res["vertex_index"]
    assert len(idx) == Vc and np.array_equal(got["triangles"], res["triangles"])
    assert np.array_equal(got["vertices"], raw["vertices"][idx])                 # cleaned in object space, then the same world map
    assert np.array_equal(got["normals"], raw["normals"][idx]) and np.array_equal(got["colors"], raw["colors"][idx])
    assert res["report"]["mask_culling"]["vertices_removed"] > 0 and res["report"]["components"]["after"] == 1
    # bare geometry cleans too
    bare, Vb, Fb = validate.validate_mesh(rend, lo, hi, str(tmp_path / "bare.ply"), vertex_colors=False, vertex_normals=False, clean=clean, **kw)
    b = meshio.read_ply(bare)
    assert (Vb, Fb) == (Vc, Fc) and b["normals"] is None and np.array_equal(b["vertices"], got["vertices"])
