"""Ray-cast visibility culling, the parts that need no device: the numpy models the GPU tests compare against (np_cast: brute-force
Moller-Trumbore over all triangles in the order include/vdn_render.h documents, with its tie rule; np_visibility on top of it), the
case mesh and rays they share, the model held against a second evaluation in np.longdouble, the policy function, the argument
errors of clean_mesh, the C layouts of the new argument blocks and the command line's new flags."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from test_mesh_clean_cpu import np_project

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vdn_ray_bin_count", "vdn_ray_bin_fill", "vdn_ray_cast", "vdn_visibility_votes")
H, W = 40, 56
CLEAR = 1e-7            # the validity margin of a (ray, triangle) decision
_CACHE = {}


# ---- the models -------------------------------------------------------------------------------------------------------------------
def referenced_faces(v32, tri):
    """bool [F]: the triangles a MeshGrid references - finite corners, three different corner indices, an area (vdn_tri_area's
    expression) above 0. The corner indices are taken to be in range."""
    tri = np.asarray(tri)
    p = np.asarray(v32, np.float32).astype(np.float64)[tri]
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cx, cy, cz = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
        distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
        return np.isfinite(p).all(axis=(1, 2)) & distinct & (area > 0) & np.isfinite(area)


def _dot(a0, b0, a1, b1, a2, b2, reverse):
    return a2 * b2 + a1 * b1 + a0 * b0 if reverse else a0 * b0 + a1 * b1 + a2 * b2


def np_pairs(v32, tri, origins, directions, dtype=np.float64, reverse=False):
    """det, u, v, t [R,F] of every (ray, triangle) pair, each product and sum rounded on its own in `dtype`, sums left to right:
    the expression order of vdn_ray_cast. reverse: the three-term sums right to left - a second opinion, not the kernel's order."""
    p = np.asarray(v32, np.float32).astype(dtype)[np.asarray(tri)]
    o, d = np.asarray(origins, np.float64).astype(dtype)[:, None, :], np.asarray(directions, np.float64).astype(dtype)[:, None, :]
    a = p[None, :, 0]
    e1, e2 = (p[:, 1] - p[:, 0])[None], (p[:, 2] - p[:, 0])[None]
    with np.errstate(all="ignore"):
        px, py, pz = d[..., 1] * e2[..., 2] - d[..., 2] * e2[..., 1], d[..., 2] * e2[..., 0] - d[..., 0] * e2[..., 2], d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]
        det = _dot(e1[..., 0], px, e1[..., 1], py, e1[..., 2], pz, reverse)
        inv = dtype(1.0) / det
        s = o - a
        u = _dot(s[..., 0], px, s[..., 1], py, s[..., 2], pz, reverse) * inv
        qx, qy, qz = s[..., 1] * e1[..., 2] - s[..., 2] * e1[..., 1], s[..., 2] * e1[..., 0] - s[..., 0] * e1[..., 2], s[..., 0] * e1[..., 1] - s[..., 1] * e1[..., 0]
        v = _dot(d[..., 0], qx, d[..., 1], qy, d[..., 2], qz, reverse) * inv
        t = _dot(e2[..., 0], qx, e2[..., 1], qy, e2[..., 2], qz, reverse) * inv
    return det, u, v, t


def np_cast(v32, tri, origins, directions, t_min=0.0, t_max=np.inf, skip_vertex=None, dtype=np.float64, return_ambiguous=False, reverse=False):
    """Brute force over all referenced triangles -> (t [R] float64, +inf on a miss; face [R] int64, -1 on a miss): a hit iff
    det != 0 and finite, u >= 0, v >= 0, u + v <= 1, t_min < t < t_max; the smallest t wins, the lower face index on equal t.
    return_ambiguous adds the number of (ray, referenced triangle) pairs whose decision is not clear by CLEAR: neither some
    quantity among u, v, 1 - u - v, t - t_min, t_max - t below -CLEAR, nor all of them above CLEAR with det != 0. (A triangle
    that is not referenced is never tested: there is no decision to be unsure of.)"""
    tri = np.asarray(tri).reshape(-1, 3)
    if len(tri) == 0:
        miss = np.full(len(origins), np.inf), np.full(len(origins), -1, np.int64)
        return miss + (0,) if return_ambiguous else miss
    det, u, v, t = np_pairs(v32, tri, origins, directions, dtype, reverse)
    ok = referenced_faces(v32, tri)[None, :]
    if skip_vertex is not None:
        ok = ok & ~(tri[None, :, :] == np.asarray(skip_vertex)[:, None, None]).any(axis=2)
    lo, hi = dtype(t_min), dtype(t_max)
    with np.errstate(all="ignore"):
        hit = ok & (det != 0) & np.isfinite(det) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > lo) & (t < hi)
        th = np.where(hit, t, np.inf)
        face = np.where(hit.any(axis=1), th.argmin(axis=1), -1).astype(np.int64)        # (argmin: the first, so the lowest, index)
        best = th.min(axis=1).astype(np.float64)
        if not return_ambiguous:
            return best, face
        q = np.stack([u, v, 1 - u - v, t - lo, hi - t])
        clear = (q < -CLEAR).any(axis=0) | ((q > CLEAR).all(axis=0) & (det != 0))
    return best, face, int((ok & ~clear).sum())


def np_centres(P):
    P = np.asarray(P, np.float64)
    return np.stack([-np.linalg.solve(Pn[:, :3], Pn[:, 3]) for Pn in P])


def np_in_image(v32, P, H, W):
    """bool [N,V]: mask_votes' "in image" rule (test_mesh_clean_cpu.np_votes states the same)"""
    u, v, w = np_project(v32, P)
    with np.errstate(invalid="ignore"):
        px, py = np.floor(u + 0.5), np.floor(v + 0.5)
        return (w > 0) & np.isfinite(u) & np.isfinite(v) & (px >= 0) & (px < W) & (py >= 0) & (py < H)


def np_visibility(v32, tri, P, H, W, eps=1e-4, dtype=np.float64, return_ambiguous=False, reverse=False):
    """-> (n_in_image [V] int32, n_visible [V] int32): vertex x in image of camera n is visible iff no triangle without x as a
    corner is hit by c_n + t (x - c_n), 0 < t < 1 - eps. return_ambiguous adds np_cast's count over the segments cast."""
    x = np.asarray(v32, np.float32).astype(np.float64)
    inside = np_in_image(v32, P, H, W)
    seen, ambiguous = np.zeros_like(inside), 0
    for n, c in enumerate(np_centres(P)):
        sel = np.nonzero(inside[n])[0]
        if len(sel) == 0:
            continue
        res = np_cast(v32, tri, np.broadcast_to(c, (len(sel), 3)), x[sel] - c[None], 0.0, 1.0 - eps, sel, dtype, True, reverse)
        seen[n, sel] = res[1] < 0
        ambiguous += res[2]
    out = inside.sum(axis=0).astype(np.int32), seen.sum(axis=0).astype(np.int32)
    return out + (ambiguous,) if return_ambiguous else out


# ---- the case ---------------------------------------------------------------------------------------------------------------------
def uv_sphere(radius, n_lon, n_lat, centre=(0.0, 0.0, 0.0)):
    """-> (vertices [n_lon (n_lat - 1) + 2, 3], triangles): the two poles first, then the rings from +z down"""
    v = [(0.0, 0.0, radius), (0.0, 0.0, -radius)]
    for j in range(1, n_lat):
        th = np.pi * j / n_lat
        for i in range(n_lon):
            ph = 2 * np.pi * i / n_lon
            v.append((radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)))
    ring = lambda j, i: 2 + (j - 1) * n_lon + i % n_lon
    t = []
    for i in range(n_lon):
        t.append((0, ring(1, i), ring(1, i + 1)))
        t.append((1, ring(n_lat - 1, i + 1), ring(n_lat - 1, i)))
        for j in range(1, n_lat - 1):
            t.append((ring(j, i), ring(j + 1, i), ring(j + 1, i + 1)))
            t.append((ring(j, i), ring(j + 1, i + 1), ring(j, i + 1)))
    return np.array(v) + np.array(centre), np.array(t)


def cameras():
    """the six look_at cameras of test_gpu_mesh_clean.vote_case, all on the z > 0 side"""
    from test_gpu_mesh_clean import look_at
    cams = [(3 * np.cos(a) * 0.8, 3 * np.sin(a) * 0.8, 1.8 + 0.2 * k) for k, a in enumerate(np.linspace(0, 2 * np.pi, 6, endpoint=False))]
    return np.stack([look_at(c, 45.0, H, W) for c in cams])


def case_mesh(seed):
    """-> (v32 [248,3] fp32, tri [F,3] int64, part [V]: 0 outer sphere, 1 inner sphere, 2 floater, 3 ground quad, 4 the corners of
    the degenerate faces). An outer sphere of radius 0.6, a concentric one of 0.3, a floater, jittered by N(0, 1e-3); two large
    triangles under all of it that span the box; and faces that must never be referenced: zero area, a repeated index, a NaN corner."""
    rng = np.random.default_rng(seed)
    parts, vs, ts, base = [], [], [], 0
    for k, (r, n_lon, n_lat, c) in enumerate(((0.6, 16, 10, (0, 0, 0)), (0.3, 10, 6, (0, 0, 0)), (0.08, 8, 6, (0.9, 0.1, 0.3)))):
        v, t = uv_sphere(r, n_lon, n_lat, c)
        vs.append(v), ts.append(t + base), parts.append(np.full(len(v), k))
        base += len(v)
    vs.append(np.array([(-1.2, -1.2, -0.75), (1.2, -1.2, -0.75), (1.2, 1.2, -0.75), (-1.2, 1.2, -0.75)]))
    ts.append(np.array([(0, 1, 2), (0, 2, 3)]) + base), parts.append(np.full(4, 3))
    base += 4
    v = np.concatenate(vs)
    v32 = (v + rng.normal(0.0, 1e-3, v.shape)).astype(np.float32)
    # three collinear points (exact in fp32: the cross product is exactly 0) and a NaN vertex
    extra = np.array([(0.125, 0.125, 0.125), (0.25, 0.125, 0.125), (0.375, 0.125, 0.125), (np.nan, 0.0, 0.0)], np.float32)
    e = base
    degenerate = np.array([(e, e + 1, e + 2), (e + 2, e, e + 1), (5, 5, 9), (7, 30, 7), (3, 4, e + 3), (e + 3, e + 3, e + 3)])
    v32 = np.concatenate([v32, extra])
    tri = np.concatenate(ts + [degenerate]).astype(np.int64)
    # the degenerate faces go in the middle of the list, so that a hit's face index has them on both sides
    order = np.concatenate([np.arange(0, 200), np.arange(len(tri) - len(degenerate), len(tri)), np.arange(200, len(tri) - len(degenerate))])
    return v32, tri[order], np.concatenate(parts + [np.full(4, 4)])


WINDOWS = ((0.0, np.inf), (0.9, 2.6), (-np.inf, 1.4))


def case_rays(seed):
    """-> (origins [R,3], directions [R,3]) float64, about 4 000: random origins inside and outside the box with random directions,
    rays aimed at the box from outside, directions with one and with two zero components (both signs on every axis), rays that
    miss the box and rays that point away from it."""
    rng = np.random.default_rng(seed)
    o, d = [rng.uniform(-2.0, 2.0, (2400, 3))], [rng.normal(size=(2400, 3))]
    a = rng.normal(size=(700, 3))
    a = 2.5 * a / np.linalg.norm(a, axis=1, keepdims=True)
    o.append(a), d.append(rng.uniform((-1.1, -1.1, -0.7), (1.1, 1.1, 0.55), (700, 3)) - a)
    for k in range(3):                                              # two zero components: along +-e_k
        for sgn in (1.0, -1.0):
            n = 40
            start = rng.uniform((-1.0, -1.0, -0.7), (1.0, 1.0, 0.55), (n, 3))
            start[:, k] = -sgn * rng.uniform(0.0, 2.0, n)
            dirs = np.zeros((n, 3))
            dirs[:, k] = sgn * rng.uniform(0.5, 2.0, n)
            o.append(start), d.append(dirs)
    for k in range(3):                                              # one zero component, the other two with every pair of signs
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                n = 30
                dirs = rng.uniform(0.2, 1.5, (n, 3)) * np.roll([0.0, s1, s2], k)
                o.append(rng.uniform(-1.5, 1.5, (n, 3))), d.append(dirs)
    # past the box: above it, parallel to its top; and behind a plane, pointing away
    miss = rng.uniform(-2.0, 2.0, (150, 3))
    miss[:, 2] = rng.uniform(0.8, 3.0, 150)
    md = rng.normal(size=(150, 3))
    md[:, 2] = np.abs(md[:, 2]) * 0.2
    o.append(miss), d.append(md)
    away = rng.uniform(-1.0, 1.0, (150, 3))
    away[:, 0] = rng.uniform(1.5, 3.0, 150)
    ad = rng.normal(size=(150, 3))
    ad[:, 0] = np.abs(ad[:, 0]) + 0.1
    o.append(away), d.append(ad)
    return np.concatenate(o), np.concatenate(d)


def valid_case():
    """The first jitter seed at which the model has no ambiguous decision, for the rays under every window and for the
    camera-vertex segments -> dict(v32, tri, part, P, origins, directions, cast: {window: (t, face)}, votes: (n_img, n_vis),
    seed, ambiguous). The models run once; every test reads this."""
    if "case" in _CACHE:
        return _CACHE["case"]
    P = cameras()
    o, d = case_rays(11)
    for seed in range(20):
        v32, tri, part = case_mesh(seed)
        cast, ambiguous = {}, 0
        for w in WINDOWS:
            t, face, amb = np_cast(v32, tri, o, d, w[0], w[1], return_ambiguous=True)
            cast[w], ambiguous = (t, face), ambiguous + amb
        n_img, n_vis, amb = np_visibility(v32, tri, P, H, W, return_ambiguous=True)
        ambiguous += amb
        if ambiguous == 0:
            break
    _CACHE["case"] = dict(v32=v32, tri=tri, part=part, P=P, origins=o, directions=d, cast=cast, votes=(n_img, n_vis), seed=seed, ambiguous=ambiguous)
    return _CACHE["case"]


# ---- the model checks itself ------------------------------------------------------------------------------------------------------
def test_the_case_is_valid_and_what_it_claims_to_be():
    c = valid_case()
    v32, tri, part = c["v32"], c["tri"], c["part"]
    assert c["ambiguous"] == 0                                       # or the case decides nothing
    assert v32.shape == (248, 3) and v32.dtype == np.float32 and 450 < len(tri) < 520
    ref = referenced_faces(v32, tri)
    assert (~ref).sum() == 6 and not ref[200:206].any()
    assert 3500 <= len(c["origins"]) <= 4500
    t, face = c["cast"][WINDOWS[0]]
    assert 0.2 < (face >= 0).mean() < 0.8 and ref[face[face >= 0]].all()
    quad = np.nonzero((part[tri] == 3).all(axis=1))[0]
    assert len(quad) == 2 and np.isin(face, quad).sum() > 100        # the large triangles are hit, too
    for w in WINDOWS[1:]:                                            # the windows cut off first hits
        tw, fw = c["cast"][w]
        assert ((fw != face) & (face >= 0)).sum() > 100 and ((fw >= 0) & (fw != face)).sum() > 20
        assert ((tw > w[0]) & (tw < w[1]))[fw >= 0].all()
    n_img, n_vis = c["votes"]
    assert (n_vis <= n_img).all() and n_img.max() == 6
    assert (n_vis[part == 1] == 0).all() and (n_img[part == 1] == 6).all()      # the inner sphere: in every image, seen by no camera
    z = v32[:, 2]
    assert (n_vis[(part == 0) & (z > 0.15)] >= 1).all()              # the upper outer sphere is seen,
    assert (n_vis[(part == 0) & (z < -0.5)] == 0).all()              # its underside by nobody: every camera is above
    assert 60 < (n_vis == 0).sum() < 160


def test_the_model_agrees_with_a_second_evaluation():
    """Two second opinions: the same expressions in np.longdouble (where the platform gives it a wider significand than float64)
    and in float64 with every three-term sum taken right to left. Every face must agree and t to 1e-11 relative - two decades
    under the 1e-9 the GPU tests hold the kernel to, so that tolerance measures the kernel and not the model."""
    c = valid_case()
    sel = np.arange(0, len(c["origins"]), 3)                        # a third of the rays: long double is slow
    o, d = c["origins"][sel], c["directions"][sel]
    opinions = [dict(reverse=True)]
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        opinions.append(dict(dtype=np.longdouble))
    for kw in opinions:
        worst = 0.0
        for w in WINDOWS:
            t, face = c["cast"][w][0][sel], c["cast"][w][1][sel]
            t2, f2 = np_cast(c["v32"], c["tri"], o, d, w[0], w[1], **kw)
            assert np.array_equal(face, f2), kw
            hit = face >= 0
            assert hit.any() and np.isinf(t[~hit]).all() and np.isinf(t2[~hit]).all()
            worst = max(worst, float((np.abs(t[hit] - t2[hit]) / np.abs(t2[hit])).max()))
        print("model vs", kw, ": max relative difference of t", worst)
        assert worst <= 1e-11 < 1e-9, kw
        img, vis = np_visibility(c["v32"], c["tri"], c["P"], H, W, **kw)
        assert np.array_equal(img, c["votes"][0]) and np.array_equal(vis, c["votes"][1]), kw


def test_model_on_hand_made_rays():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    tri = np.array([[3, 4, 5], [0, 1, 2], [0, 2, 1], [0, 0, 1]])
    o = np.array([[0.25, 0.25, 2.0], [0.25, 0.25, 2.0], [0.25, 0.25, 0.5], [2.0, 2.0, 2.0], [0.25, 0.25, -1.0]])
    d = np.array([[0, 0, -1.0], [0, 0, 1.0], [0, 0, -2.0], [0, 0, -1.0], [0, 0, 0.0]])
    t, f = np_cast(v, tri, o, d)
    assert f.tolist() == [0, -1, 1, -1, -1] and t[0] == 1.0 and t[2] == 0.25 and np.isinf(t[[1, 3, 4]]).all()      # faces 1, 2: equal t, the lower index
    t, f = np_cast(v, tri, o[:1], d[:1], 1.0, 2.5)                   # the window is open: t = 1 is cut off, t = 2 is not
    assert f.tolist() == [1] and t[0] == 2.0
    t, f = np_cast(v, tri, o[:1], d[:1], skip_vertex=np.array([4]))
    assert f.tolist() == [1]
    t, f = np_cast(v, tri, o[:1], d[:1], skip_vertex=np.array([0]), t_max=1.5)
    assert f.tolist() == [0]
    t, f = np_cast(v, tri[:0], o, d)
    assert (f == -1).all() and np.isinf(t).all()


# ---- policy and arguments ---------------------------------------------------------------------------------------------------------
def test_visible_keep_on_hand_written_counts():
    from vdn_train.mesh_clean import visible_keep
    n = np.array([0, 1, 2, 5])
    assert visible_keep(n).tolist() == [False, True, True, True] and visible_keep(n, 2).tolist() == [False, False, True, True]
    assert visible_keep(n, 0).all() and not visible_keep(n, 6).any()
    out = visible_keep(torch.as_tensor(n), 2)
    assert torch.is_tensor(out) and out.dtype == torch.bool and out.tolist() == [False, False, True, True]
    with pytest.raises(ValueError):
        visible_keep(n, -1)


def test_visibility_is_off_by_default():
    from vdn_train import mesh_clean
    sig = inspect.signature(mesh_clean.clean_mesh).parameters
    assert sig["visibility"].default is None and sig["image_size"].default is None
    assert sig["visibility"].kind == sig["image_size"].kind == inspect.Parameter.KEYWORD_ONLY


def test_clean_mesh_argument_errors_that_need_no_device():
    from vdn_train import mesh_clean
    v, t = np.zeros((4, 3)), np.zeros((2, 3), np.int64)
    P, m = np.zeros((2, 3, 4)), np.zeros((2, 4, 4), np.uint8)
    vis = {"min_visible": 1}
    for kw in (dict(visibility=vis),                                                     # no cameras
               dict(visibility=vis, masks=m),
               dict(visibility=vis, cameras=P),                                          # neither masks nor image_size
               dict(visibility=vis, cameras=P, image_size=(4,)), dict(visibility=vis, cameras=P, image_size=(0, 4)),
               dict(visibility=vis, cameras=P, image_size="big"),
               dict(visibility=True, cameras=P, image_size=(4, 4)), dict(visibility=3, cameras=P, image_size=(4, 4)),
               dict(visibility={"min_visibel": 1}, cameras=P, image_size=(4, 4)),
               dict(visibility={"min_visible": -1}, cameras=P, image_size=(4, 4)), dict(visibility={"min_visible": 1.5}, cameras=P, image_size=(4, 4)),
               dict(visibility={"eps": 1.0}, cameras=P, image_size=(4, 4)), dict(visibility={"eps": -1e-3}, cameras=P, image_size=(4, 4)),
               dict(visibility={"cell_size": 0.0}, cameras=P, image_size=(4, 4)), dict(visibility={"cell_size": np.inf}, cameras=P, image_size=(4, 4)),
               dict(cameras=P, image_size=(4, 4)),                                       # without visibility the old rule stands
               dict(cameras=P), dict(masks=m)):
        with pytest.raises(ValueError):
            mesh_clean.clean_mesh(v, t, **kw)


def test_camera_centres_on_the_host():
    from vdn_hip import mesh
    P = cameras()
    c = mesh.camera_centres(P)
    assert c.dtype == np.float64 and c.shape == (6, 3) and np.array_equal(c, np_centres(P))
    want = np.array([(3 * np.cos(a) * 0.8, 3 * np.sin(a) * 0.8, 1.8 + 0.2 * k) for k, a in enumerate(np.linspace(0, 2 * np.pi, 6, endpoint=False))])
    assert np.abs(c - want).max() < 1e-12
    assert np.array_equal(mesh.camera_centres(torch.from_numpy(P)), c)
    flat = P.copy()
    flat[2, 2, :3] = flat[2, 0, :3] * 0.5                           # rank 2
    for bad in (flat, np.zeros((1, 3, 4)), P[:, :, :3], P[0]):
        with pytest.raises(ValueError):
            mesh.camera_centres(bad)
    nan = P.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        mesh.camera_centres(nan)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_ray_argument_blocks_are_c_layouts_and_declared():
    from vdn_hip import lib
    structs, funcs = lib.parse_header()
    for fn in ENTRY_POINTS:
        assert funcs[fn] == [ctypes.c_void_p, ctypes.c_void_p]
    # VdnRayGridArgs {7 pointers, 3 int64, 5 double, 4 int32}
    G = lib.VdnRayGridArgs
    assert ctypes.sizeof(G) == 7 * 8 + 3 * 8 + 5 * 8 + 4 * 4 == 136
    assert (G.vertices.offset, G.cell_count.offset, G.cursor.offset, G.refs.offset, G.records.offset, G.error.offset, G.V.offset, G.n_refs.offset,
            G.lo_x.offset, G.margin.offset, G.nx.offset, G.index_bytes.offset) == (0, 16, 24, 32, 40, 48, 56, 72, 80, 112, 120, 132)
    # VdnRayCastArgs {9 pointers, 3 int64, 7 double, 4 int32}
    C = lib.VdnRayCastArgs
    assert ctypes.sizeof(C) == 9 * 8 + 3 * 8 + 7 * 8 + 4 * 4 == 168
    assert (C.origins.offset, C.skip_vertex.offset, C.records.offset, C.t.offset, C.tests.offset, C.R.offset, C.lo_x.offset, C.t_min.offset,
            C.t_max.offset, C.nx.offset, C.any_hit.offset) == (0, 16, 24, 48, 64, 72, 96, 136, 144, 152, 164)
    # VdnVisibilityArgs {8 pointers, 4 int64, 6 double, 6 int32}
    S = lib.VdnVisibilityArgs
    assert ctypes.sizeof(S) == 8 * 8 + 4 * 8 + 6 * 8 + 6 * 4 == 168
    assert (S.centres.offset, S.n_in_image.offset, S.n_visible.offset, S.V.offset, S.n_refs.offset, S.eps.offset, S.nx.offset, S.H.offset,
            S.W.offset) == (16, 48, 56, 64, 88, 136, 144, 156, 160)
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28     # additive: no bump
    so = lib.load()
    for fn in ENTRY_POINTS:
        assert getattr(so, fn) is not None
    assert lib.call_value("vdn_abi_version") == 28


def _grid_block(a):
    a.lo_x = a.lo_y = a.lo_z = 0.0
    a.h, a.margin, a.nx, a.ny, a.nz = 1.0, 1e-9, 2, 2, 2
    return a


def test_ray_entry_points_refuse_bad_blocks_on_the_host():
    """checked before anything is launched: the pointers are never dereferenced"""
    from vdn_hip import lib
    for name, args in (("vdn_ray_bin_count", lib.VdnRayGridArgs()), ("vdn_ray_bin_fill", lib.VdnRayGridArgs()), ("vdn_ray_cast", lib.VdnRayCastArgs()),
                       ("vdn_visibility_votes", lib.VdnVisibilityArgs())):
        with pytest.raises(lib.VdnError):
            lib.call(name, args, None)
        with pytest.raises(lib.VdnError):
            lib.call(name, None, None)
    big = 1 << 31
    g = _grid_block(lib.VdnRayGridArgs())
    g.vertices = g.triangles = g.cell_count = g.cursor = g.refs = g.records = g.error = 16
    g.index_bytes, g.n_refs = 8, 1
    for V, F, dims in ((big, 1, (2, 2, 2)), (3, big, (2, 2, 2)), (3, 1, (1 << 11, 1 << 10, 1 << 10)), (3, 1, (1 << 16, 1 << 16, 1))):
        g.V, g.F, (g.nx, g.ny, g.nz) = V, F, dims
        assert lib.try_call("vdn_ray_bin_count", g, None) is False and lib.try_call("vdn_ray_bin_fill", g, None) is False, (V, F, dims)
    g.V, g.F, (g.nx, g.ny, g.nz), g.n_refs = 3, 1, (2, 2, 2), big
    assert lib.try_call("vdn_ray_bin_fill", g, None) is False
    for field, bad in (("h", 0.0), ("h", float("nan")), ("margin", -1.0), ("lo_x", float("inf")), ("nx", 0), ("index_bytes", 2)):
        g2 = _grid_block(lib.VdnRayGridArgs())
        g2.vertices = g2.triangles = g2.cell_count = g2.cursor = g2.refs = g2.records = g2.error = 16
        g2.index_bytes, g2.n_refs, g2.V, g2.F = 8, 1, 3, 1
        setattr(g2, field, bad)
        with pytest.raises(lib.VdnError):
            lib.call("vdn_ray_bin_count", g2, None)
    c = _grid_block(lib.VdnRayCastArgs())
    c.origins = c.directions = c.records = c.cell_start = c.refs = c.t = c.face = 16
    for R, F, n_refs in ((big, 1, 1), (1, big, 1), (1, 1, big)):
        c.R, c.F, c.n_refs = R, F, n_refs
        assert lib.try_call("vdn_ray_cast", c, None) is False
    s = _grid_block(lib.VdnVisibilityArgs())
    s.vertices = s.P = s.centres = s.records = s.cell_start = s.refs = s.n_in_image = s.n_visible = 16
    s.H, s.W, s.eps = 4, 4, 1e-4
    for V, N in ((big, 1), (1, big)):
        s.V, s.N, s.F, s.n_refs = V, N, 1, 1
        assert lib.try_call("vdn_visibility_votes", s, None) is False
    s.V, s.N, s.eps = 1, 1, 1.0
    with pytest.raises(lib.VdnError):
        lib.call("vdn_visibility_votes", s, None)


def test_python_layer_refuses_cpu_tensors():
    from vdn_hip import mesh
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for call in (lambda: mesh.MeshGrid(v, t), lambda: mesh.visibility_votes(v, t, cameras(), (H, W))):
        with pytest.raises(ValueError):
            call()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_command_line_has_the_new_flags_and_parses_the_old_vectors_as_before():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import clean_mesh as tool
    finally:
        sys.path.pop(0)
    p = tool.parser()
    a = p.parse_args(["in.ply", "out.ply", "--keep", "all", "--by", "area", "--min-faces", "5", "--scene", "d", "--dilate", "3", "--world-space"])
    assert (a.mesh, a.out, a.keep, a.by, a.min_faces, a.scene, a.dilate, a.world_space, a.min_inside, a.max_outside) == ("in.ply", "out.ply", "all", "area", 5, "d", 3, True, 1, 0)
    assert a.visible_from is None and a.visibility_eps is None       # absent = off
    a = p.parse_args(["in.ply", "out.ply"])
    assert (a.keep, a.by, a.min_faces, a.min_area_fraction, a.scene, a.dilate, a.world_space, a.device, a.visible_from) == ("largest", "faces", 0, 0.0, None, 0, False, "cuda:0", None)
    a = p.parse_args(["in.ply", "out.ply", "--scene", "d", "--visible-from", "2", "--visibility-eps", "1e-3"])
    assert a.visible_from == 2 and a.visibility_eps == 1e-3 and a.scene == "d"
    help_text = p.format_help()
    assert "--visible-from" in help_text and "--visibility-eps" in help_text


def test_command_line_new_flags_need_a_scene(monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import clean_mesh as tool
    finally:
        sys.path.pop(0)
    for argv in (["in.ply", "out.ply", "--visible-from", "1"], ["in.ply", "out.ply", "--scene", "d", "--visibility-eps", "1e-3"]):
        monkeypatch.setattr(sys, "argv", ["clean_mesh.py"] + argv)
        with pytest.raises(SystemExit) as e:
            tool.main()                                              # refused by the parser, before any file is read
        assert e.value.code == 2
    assert "--visible-from needs --scene" in capsys.readouterr().err
