"""Textured meshes without a device: the integer layout of the per-face atlas and the fp64 models of the four kernels of
csrc/mesh_texture.hip (include/vdn_render.h has the rules; tests/test_gpu_mesh_texture.py holds the kernels to these models), the
proof by enumeration that a bilinear lookup inside a face touches that face's texels only, the OBJ writer and reader, and the
accuracy the scheme buys over interpolated vertex colours - all in numpy and exact rationals."""
import os
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the layout, restated ------------------------------------------------------------------------------------------------------------
def np_layout(F, S, patch=None):
    """the record of vdn_hip.mesh.texture_layout, patch=None by trying every n from the largest down"""
    cells = (F + 1) // 2
    if patch is None:
        fits = [n for n in range(4, S + 1) if cells <= (S // n) ** 2]
        if not fits:
            raise ValueError("nothing fits")
        n = max(fits)
    else:
        n = patch
        if n < 4 or n > S or cells > (S // n) ** 2:
            raise ValueError("patch does not fit")
    return {"F": F, "S": S, "n": n, "C": S // n, "T": n * (n - 1) // 2, "m": n - 3, "points": F * (n * (n - 1) // 2)}


def enumerate_half(n):
    """[(i, j)] of a half's own frame in the order of r: j = 0 .. n - 2 outside, i = 0 .. n - 2 - j inside"""
    return [(i, j) for j in range(n - 1) for i in range(n - 1 - j)]


def rank(n, i, j):
    return j * (2 * n - 1 - j) // 2 + i


def owner(n, i, j):
    """local texel (i, j) of a cell -> (half, i', j') in the half's own frame, "diagonal", or None outside the cell"""
    if not (0 <= i < n and 0 <= j < n):
        return None
    if i + j <= n - 2:
        return 0, i, j
    if i + j >= n:
        return 1, n - 1 - i, n - 1 - j
    return "diagonal"


def diagonal_source(i, j):
    return (i, j - 1) if j > 0 else (i - 1, 0)


def barycentrics(n, i, j):
    """(b0, b1, b2) of texel (i, j) of a half's own frame, in double"""
    m = n - 3
    if i + j <= m:
        b1, b2 = np.float64(i) / np.float64(m), np.float64(j) / np.float64(m)
        return (np.float64(1.0) - b1) - b2, b1, b2
    b1 = np.float64(min(max((np.float64(i) - 0.5) / np.float64(m), 0.0), 1.0))
    return np.float64(0.0), b1, np.float64(1.0) - b1


def corner_positions(n, h):
    """continuous cell-local positions of the corners 0, 1, 2 of half h"""
    m = n - 3
    if h == 0:
        return [(0.5, 0.5), (m + 0.5, 0.5), (0.5, m + 0.5)]
    return [(n - 0.5, n - 0.5), (n - 0.5 - m, n - 0.5), (n - 0.5, n - 0.5 - m)]


def np_uv(lay):
    F, S, n, C = lay["F"], lay["S"], lay["n"], lay["C"]
    uv = np.zeros((F, 3, 2))
    for f in range(F):
        c = f >> 1
        ox, oy = (c % C) * n, (c // C) * n
        for k, (x, y) in enumerate(corner_positions(n, f & 1)):
            uv[f, k] = ((ox + x) / S, 1.0 - (oy + y) / S)
    return uv


# ---- fp64 models of the kernels --------------------------------------------------------------------------------------------------------
def np_texel_points(v, t, n):
    """-> (points fp32 [F T,3], face int32 [F T]): (b0 v0 + b1 v1) + b2 v2 in double, rounded once"""
    v = np.asarray(v, np.float64)
    t = np.asarray(t, np.int64)
    F, half = len(t), enumerate_half(n)
    out = np.zeros((F, len(half), 3))
    for r, (i, j) in enumerate(half):
        b0, b1, b2 = barycentrics(n, i, j)
        out[:, r] = (b0 * v[t[:, 0]] + b1 * v[t[:, 1]]) + b2 * v[t[:, 2]]
    return out.reshape(-1, 3).astype(np.float32), np.repeat(np.arange(F, dtype=np.int32), len(half))


def np_quantize_bgr(c):
    c = np.asarray(c, np.float32)
    return np.rint(np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)[:, ::-1]


def np_atlas(colors, lay, rgb=None):
    """the atlas in scatter form: every face writes its texels, then every used cell's diagonal is filled. colors: float BGR rows
    of the texel points - or rgb: their bytes, already quantised and in RGB order"""
    F, S, n, C, T = lay["F"], lay["S"], lay["n"], lay["C"], lay["T"]
    rgb = (np_quantize_bgr(colors) if rgb is None else np.asarray(rgb, np.uint8)).reshape(F, T, 3)
    atlas = np.zeros((S, S, 3), np.uint8)
    f = np.arange(F)
    ox, oy = ((f >> 1) % C) * n, ((f >> 1) // C) * n
    up = (f & 1) == 1
    for r, (i, j) in enumerate(enumerate_half(n)):
        x, y = ox + np.where(up, n - 1 - i, i), oy + np.where(up, n - 1 - j, j)
        atlas[y, x] = rgb[:, r]
    for c in range((F + 1) // 2):
        cx, cy = (c % C) * n, (c // C) * n
        for i in range(n):
            j = n - 1 - i
            si, sj = diagonal_source(i, j)
            atlas[cy + j, cx + i] = atlas[cy + sj, cx + si]
    return atlas


def np_sample(texture, lay, v, t, face, pts, background=(1.0, 1.0, 1.0)):
    """-> float64 [R,3], not rounded: the lookup of vdn_tex_sample, operation by operation"""
    S, n, C, m = lay["S"], lay["n"], lay["C"], float(lay["m"])
    v, t, face, pts = np.asarray(v, np.float64), np.asarray(t, np.int64), np.asarray(face, np.int64), np.asarray(pts, np.float64)
    tex = np.asarray(texture).astype(np.float64)
    hit = (face >= 0) & (face < len(t))
    f = np.where(hit, face, 0)
    v0 = v[t[f, 0]]
    e1, e2, w = v[t[f, 1]] - v0, v[t[f, 2]] - v0, pts - v0
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    a11, a12, a22, r1, r2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(w, e1), dot(w, e2)
    det = a11 * a22 - a12 * a12
    with np.errstate(all="ignore"):
        ok = (det > 0.0) & (det < np.inf)
        b1 = np.where(ok, (a22 * r1 - a12 * r2) / det, 0.0)
        b2 = np.where(ok, (a11 * r2 - a12 * r1) / det, 0.0)
        b1, b2 = np.where(b1 > 0.0, b1, 0.0), np.where(b2 > 0.0, b2, 0.0)
        s = b1 + b2
        b1, b2 = np.where(s > 1.0, b1 / s, b1), np.where(s > 1.0, b2 / s, b2)
        b1, b2 = np.where(b1 <= 1.0, b1, 0.0), np.where(b2 <= 1.0, b2, 0.0)
    cell = f >> 1
    ox, oy = ((cell % C) * n).astype(np.float64), ((cell // C) * n).astype(np.float64)
    low = (f & 1) == 0
    x = np.where(low, (ox + 0.5) + m * b1, (ox + (n - 0.5)) - m * b1)
    y = np.where(low, (oy + 0.5) + m * b2, (oy + (n - 0.5)) - m * b2)
    tx, ty = x - 0.5, y - 0.5
    fx0, fy0 = np.floor(tx), np.floor(ty)
    fx, fy = tx - fx0, ty - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    cl = lambda k: np.clip(k, 0, S - 1)
    x0, x1, y0, y1 = cl(x0), cl(x0 + 1), cl(y0), cl(y0 + 1)
    w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    out = ((w00[:, None] * tex[y0, x0] + w10[:, None] * tex[y0, x1]) + (w01[:, None] * tex[y1, x0] + w11[:, None] * tex[y1, x1])) / 255.0
    return np.where(hit[:, None], out, np.asarray(background, np.float64)[None])


def np_project_step(x, x0, sdf, g, max_offset):
    """-> float64 [P,3], not rounded: one Newton step inside the ball around x0; rows with a non-finite sdf, g or result stay"""
    x, x0, sdf, g = (np.asarray(a, np.float64) for a in (x, x0, sdf, g))
    with np.errstate(all="ignore"):
        den = np.maximum((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2], 1e-12)
        y = x + (-sdf[:, None] * g) / den[:, None]
        e = y - x0
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        y = np.where((r > max_offset)[:, None], x0 + e * (max_offset / r)[:, None], y)
    ok = np.isfinite(sdf) & np.isfinite(g).all(axis=1) & np.isfinite(y).all(axis=1)
    return np.where(ok[:, None], y, x)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
_ICO = {}


def icosphere(level):
    """the unit icosphere after `level` midpoint subdivisions -> (vertices float64 [V,3], triangles int64 [20 * 4^level,3])"""
    if level in _ICO:
        return _ICO[level]
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nt = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    _ICO[level] = (np.stack(v), np.asarray(t, np.int64))
    return _ICO[level]


PHASE = np.array([0.0, 2.0, 4.0])


def color_field(p):
    """BGR colour of a point: 0.5 + 0.5 sin(12 x + phase), one phase per channel"""
    p = np.asarray(p, np.float64)
    return 0.5 + 0.5 * np.sin(12.0 * p[:, :1] + PHASE[None])


def surface_samples(v, t, count, seed):
    """`count` uniform points of uniformly drawn faces -> (face int64 [count], points float64 [count,3], barycentrics [count,3])"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, len(t), count)
    u = rng.random((count, 2))
    flip = u.sum(axis=1) > 1.0
    u[flip] = 1.0 - u[flip]
    b = np.stack([1.0 - u[:, 0] - u[:, 1], u[:, 0], u[:, 1]], axis=1)
    p = (b[:, :, None] * v[t[f]]).sum(axis=1)
    return f, p, b


def accuracy_case():
    """the 320-face icosphere, 8 x 8 patches on the smallest atlas that holds them, 20 000 surface points"""
    v, t = icosphere(2)
    lay = np_layout(len(t), 13 * 8, 8)
    face, pts, bary = surface_samples(v, t, 20000, 11)
    return v, t, lay, face, pts, bary


def vertex_color_error(v, t, face, pts, bary):
    """|interpolated quantised vertex colours - the field| at the points, RGB order"""
    vc = np_quantize_bgr(color_field(v)).astype(np.float64) / 255.0
    return np.abs((bary[:, :, None] * vc[t[face]]).sum(axis=1) - color_field(pts)[:, ::-1])


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 9, 16])
def test_halves_are_disjoint_and_the_enumeration_round_trips(n):
    half = enumerate_half(n)
    assert len(half) == n * (n - 1) // 2 and len(set(half)) == len(half)
    assert [rank(n, i, j) for i, j in half] == list(range(len(half)))
    owned = {0: set(), 1: set()}
    diagonal, free = set(), set()
    for j in range(n):
        for i in range(n):
            o = owner(n, i, j)
            if o == "diagonal":
                diagonal.add((i, j))
            else:
                owned[o[0]].add((i, j))
                assert (o[1], o[2]) in half
    assert len(owned[0]) == len(owned[1]) == n * (n - 1) // 2 and not owned[0] & owned[1]
    assert {(n - 1 - i, n - 1 - j) for i, j in owned[0]} == owned[1]           # a half turn
    assert len(diagonal) == n and len(owned[0]) + len(owned[1]) + n == n * n
    for i, j in diagonal:                                                       # the fill comes from the lower half's gutter
        si, sj = diagonal_source(i, j)
        assert (si, sj) in owned[0] and si + sj == n - 2
    # corners sit on texel centres of their own half, m = n - 3 apart
    for h in (0, 1):
        for x, y in corner_positions(n, h):
            assert owner(n, int(x - 0.5), int(y - 0.5))[0] == h and x - 0.5 == int(x - 0.5)


def test_texture_layout_picks_the_largest_patch_that_fits():
    from vdn_hip import mesh
    for S in (4, 7, 16, 33, 104, 256):
        for F in (0, 1, 2, 3, 5, 8, 9, 31, 32, 33, 80, 319, 320):
            try:
                want = np_layout(F, S)
            except ValueError:
                with pytest.raises(ValueError):
                    mesh.texture_layout(F, S)
                continue
            assert mesh.texture_layout(F, S) == want
            assert (F + 1) // 2 <= want["C"] ** 2 and (want["n"] == S or (F + 1) // 2 > (S // (want["n"] + 1)) ** 2)
            assert mesh.texture_layout(F, S, want["n"]) == want
    assert mesh.texture_layout(320, 2048)["n"] == 2048 // 13
    assert mesh.texture_layout(9, 16, 4) == np_layout(9, 16, 4)
    for F, S, patch in ((33, 16, None), (1, 3, None), (9, 16, 8), (2, 16, 3), (2, 16, 17), (-1, 16, None), (2, 16, 4.5), (2.5, 16, None)):
        with pytest.raises(ValueError):
            mesh.texture_layout(F, S, patch)


def test_texture_coordinates_follow_the_corner_positions():
    from vdn_hip import mesh
    for F, S, n in ((1, 8, 8), (5, 13, 4), (80, 70, 5), (0, 16, None)):
        lay = mesh.texture_layout(F, S, n)
        uv = mesh.texture_uv(lay)
        assert uv.dtype == np.float64 and uv.shape == (F, 3, 2) and np.array_equal(uv, np_uv(lay))
        assert ((uv > 0.0) & (uv < 1.0)).all()


# ---- ownership: no lookup inside a face reads another face's texel ----------------------------------------------------------------------
def bilinear_taps(n, h, b1, b2):
    """[(i, j, weight)] of the lookup at the barycentrics (b1, b2) of half h, cell-local, in exact rationals"""
    m, half = n - 3, Fraction(1, 2)
    x, y = (half + m * b1, half + m * b2) if h == 0 else (n - half - m * b1, n - half - m * b2)
    tx, ty = x - half, y - half
    x0, y0 = tx.numerator // tx.denominator, ty.numerator // ty.denominator
    fx, fy = tx - x0, ty - y0
    return [(x0, y0, (1 - fx) * (1 - fy)), (x0 + 1, y0, fx * (1 - fy)), (x0, y0 + 1, (1 - fx) * fy), (x0 + 1, y0 + 1, fx * fy)]


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 9])
def test_every_tap_with_weight_is_an_owned_texel(n):
    D = 6 * (n - 3)                                   # texel centres, texel edges and thirds between them; edges and corners included
    seen = set()
    for h in (0, 1):
        for a in range(D + 1):
            for b in range(D + 1 - a):
                taps = bilinear_taps(n, h, Fraction(a, D), Fraction(b, D))
                assert sum(w for _, _, w in taps) == 1
                for i, j, w in taps:
                    if w != 0:
                        o = owner(n, i, j)
                        assert o is not None and o != "diagonal" and o[0] == h, (n, h, a, b, i, j, w)
                        seen.add((h, i, j))
    # and every owned texel is read somewhere, the gutter included, but for its two end texels (n - 2, 0) and (0, n - 2): padding only
    ends = {(0, n - 2, 0), (0, 0, n - 2), (1, 1, n - 1), (1, n - 1, 1)}
    assert seen == {(o[0], i, j) for i in range(n) for j in range(n) for o in [owner(n, i, j)] if o != "diagonal"} - ends


# ---- the models against each other -----------------------------------------------------------------------------------------------------
def test_texel_points_of_the_model_lie_on_their_faces():
    v, t = icosphere(1)
    for n in (4, 5, 8):
        pts, face = np_texel_points(v, t, n)
        T = n * (n - 1) // 2
        assert pts.dtype == np.float32 and pts.shape == (len(t) * T, 3) and np.array_equal(face, np.repeat(np.arange(len(t)), T))
        p = pts.reshape(len(t), T, 3).astype(np.float64)
        tri = v[t]
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        assert np.abs(((p - tri[:, None, 0]) * nrm[:, None]).sum(axis=2)).max() < 1e-6
        for k, (x, y) in enumerate(corner_positions(n, 0)):        # the corner texels are the corners
            assert np.array_equal(p[:, rank(n, int(x - 0.5), int(y - 0.5))], tri[:, k].astype(np.float32).astype(np.float64))


def test_atlas_model_fills_diagonals_and_leaves_the_rest_zero():
    rng = np.random.default_rng(0)
    for F, S, n in ((5, 13, 4), (7, 10, 5), (1, 4, 4)):
        lay = np_layout(F, S, n)
        col = rng.uniform(0.2, 1.0, (lay["points"], 3)).astype(np.float32)      # no zero byte among the owned texels
        atlas = np_atlas(col, lay)
        used = atlas.any(axis=2)
        C = lay["C"]
        for y in range(S):
            for x in range(S):
                cx, cy = x // n, y // n
                o = owner(n, x - cx * n, y - cy * n) if cx < C and cy < C else None
                f = None if o is None else 2 * (cy * C + cx) + (0 if o == "diagonal" else o[0])
                assert used[y, x] == (f is not None and f < F), (F, S, n, x, y)
        # a lookup at a texel centre returns that texel
        assert np.array_equal(atlas[0, 0], np_quantize_bgr(col[:1])[0])


def test_sample_model_returns_corner_texels_and_background():
    v, t = icosphere(0)
    lay = np_layout(len(t), 20, 5)
    rng = np.random.default_rng(1)
    tex = rng.integers(0, 256, (20, 20, 3)).astype(np.uint8)
    f = np.arange(len(t))
    for k in range(3):
        got = np_sample(tex, lay, v, t, f, v[t[:, k]])
        uv = np_uv(lay)[:, k]
        x, y = (uv[:, 0] * 20 - 0.5).round().astype(int), ((1.0 - uv[:, 1]) * 20 - 0.5).round().astype(int)
        assert np.abs(got - tex[y, x] / 255.0).max() < 1e-12
    miss = np_sample(tex, lay, v, t, np.array([-1, 99]), np.zeros((2, 3)), background=(0.25, 0.5, 0.75))
    assert np.array_equal(miss, [[0.25, 0.5, 0.75]] * 2)


def test_project_model_steps_onto_a_plane_and_stays_in_the_ball():
    x0 = np.array([[0.0, 0.0, 0.3], [0.0, 0.0, 0.3], [1.0, 1.0, 1.0], [0.0, 0.0, 0.3]])
    g = np.array([[0.0, 0.0, 2.0]] * 3 + [[0.0, np.nan, 2.0]])
    sdf = np.array([0.6, 0.6, np.inf, 0.6])                            # the field 2 z: zero at z = 0
    y = np_project_step(x0, x0, sdf, g, 1.0)
    assert np.allclose(y[0], [0, 0, 0]) and np.array_equal(y[2], x0[2]) and np.array_equal(y[3], x0[3])
    y = np_project_step(x0, x0, sdf, g, 0.1)
    assert np.allclose(y[1], [0, 0, 0.2]) and abs(np.linalg.norm(y[1] - x0[1]) - 0.1) < 1e-15


# ---- what the texture buys -------------------------------------------------------------------------------------------------------------
def test_texture_lookup_beats_interpolated_vertex_colours_in_the_model():
    v, t, lay, face, pts, bary = accuracy_case()
    assert len(t) == 320 and lay["n"] == 8
    tp, _ = np_texel_points(v, t, lay["n"])
    atlas = np_atlas(color_field(tp), lay)
    want = color_field(pts)[:, ::-1]
    tex_err = np.abs(np_sample(atlas, lay, v, t, face, pts) - want)
    vtx_err = vertex_color_error(v, t, face, pts, bary)
    print("texture: mean %.4f max %.3f; vertex colours: mean %.4f max %.3f; ratio %.3f" %
          (tex_err.mean(), tex_err.max(), vtx_err.mean(), vtx_err.max(), tex_err.mean() / vtx_err.mean()))
    assert tex_err.mean() <= 0.25 * vtx_err.mean()


# ---- files -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals", [False, True])
def test_write_obj_read_obj_round_trip(tmp_path, with_normals):
    from PIL import Image
    from vdn_hip import mesh
    from vdn_train import meshio
    v, t = icosphere(0)
    v, t = v.astype(np.float32) * 3.25 + 0.1, t[:19]                           # 19 faces: the last cell is half empty
    lay = mesh.texture_layout(len(t), 23, 5)
    uv = mesh.texture_uv(lay)
    rng = np.random.default_rng(2)
    tex = rng.integers(0, 256, (23, 23, 3)).astype(np.uint8)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32) if with_normals else None
    path = meshio.write_obj(str(tmp_path / "m.obj"), v, t, uv, tex, normals=nrm)
    assert path == str(tmp_path / "m.obj") and sorted(os.listdir(tmp_path)) == ["m.mtl", "m.obj", "m.png"]
    assert "map_Kd m.png" in open(tmp_path / "m.mtl").read().splitlines()
    assert "mtllib m.mtl" in open(path).read().splitlines()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.png").convert("RGB")), tex)
    got = meshio.read_obj(path)
    assert got["vertices"].dtype == np.float32 and np.array_equal(got["vertices"], v) and np.array_equal(got["triangles"], t)
    assert np.array_equal(got["uv"], uv.reshape(-1, 2)) and np.array_equal(got["uv_index"], np.arange(3 * len(t)).reshape(-1, 3))
    assert got["texture_path"] == str(tmp_path / "m.png") and got["mtllib"] == "m.mtl"
    if with_normals:
        assert np.array_equal(got["normals"], nrm) and np.array_equal(got["normal_index"], t)
    else:
        assert got["normals"] is None and got["normal_index"] is None
    # an empty mesh writes and reads
    e = meshio.read_obj(meshio.write_obj(str(tmp_path / "e.obj"), np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros((0, 3, 2)), tex[:4, :4]))
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3) and e["uv"].shape == (0, 2)
    for bad in (dict(uv=uv[:-1]), dict(texture=tex.astype(np.float32)), dict(triangles=t + 100), dict(normals=np.zeros((3, 3))), dict(path=str(tmp_path / "m.ply"))):
        kw = dict(path=path, vertices=v, triangles=t, uv=uv, texture=tex)
        kw.update(bad)
        with pytest.raises(ValueError):
            meshio.write_obj(**kw)
    with open(tmp_path / "quad.obj", "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError):
        meshio.read_obj(str(tmp_path / "quad.obj"))


# ---- the interface, as far as it shows without a device --------------------------------------------------------------------------------
def test_library_declares_and_exports_the_texture_entry_points():
    import re
    from vdn_hip import build, lib
    names = ("vdn_tex_points", "vdn_tex_project", "vdn_tex_gather", "vdn_tex_sample")
    for n in names:
        assert len(lib.FUNCTIONS[n]) == 2
    if os.path.exists(lib.LIB_PATH):
        for n in names:
            assert hasattr(lib.load(), n)
        assert lib.call_value("vdn_abi_version") == 28
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28
    assert build.PER_FILE_FLAGS["mesh_texture.hip"] == ["-ffp-contract=off"]               # the positions are specified to the bit
    assert "VdnTexArgs" in lib.STRUCTS and "VdnTexProjectArgs" in lib.STRUCTS


def test_validate_mesh_defaults_to_no_texture_and_the_tool_parses():
    import inspect
    import subprocess
    import sys
    from vdn_hip import mesh
    from vdn_train import validate
    for fn in (validate.validate_mesh, validate.validate_scene_mesh):
        assert inspect.signature(fn).parameters["texture"].default is None
    p = inspect.signature(mesh.bake_texture).parameters
    assert (p["texture_size"].default, p["patch"].default, p["project"].default, p["max_offset"].default, p["shade"].default, p["batch"].default) == \
        (2048, None, 2, None, None, 1 << 20)
    tool = os.path.join(ROOT, "tools", "texture_mesh.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--checkpoint", "--synthetic", "--texture-size", "--patch", "--project"):
        assert opt in r.stdout
    for args in (["a.ply", "b.obj"], ["a.ply", "b.obj", "--checkpoint", "c.pth", "--synthetic", "0"]):      # exactly one source of weights
        assert subprocess.run([sys.executable, tool] + args, capture_output=True, text=True).returncode == 2
