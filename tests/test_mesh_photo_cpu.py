"""Texel colours from the photographs without a device: np_photo_colors, the fp64 model of vdn_tex_photo (csrc/mesh_photo.hip) in the
expression order include/vdn_render.h states, with brute-force occlusion over all triangles (the Moller-Trumbore expressions of
cast_ray on the grid's fp32 corner values); the fixture tests/test_gpu_mesh_photo.py holds the kernel to, with the proof that it takes
every branch; the model against an analytically painted sphere; and what shows of the interface without a device."""
import os
import re

import numpy as np
import pytest

import test_mesh_texture_cpu as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}

CONTRIBUTES, BEHIND, OUT_OF_FRAME, NOT_FACING, OCCLUDED, NO_NORMAL = 0, 1, 2, 3, 4, 5


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def np_centres(P):
    P = np.asarray(P, np.float64)
    return np.stack([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P]) if len(P) else np.zeros((0, 3))


def np_occluded(corners, o, d, own, t_max, chunk=256):
    """any-hit of the segments o + t d[r], 0 < t < t_max, against every triangle but own[r] -> bool [R]; corners float64 [F,3,3]"""
    a, e1, e2 = corners[:, 0], corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    F = len(corners)
    out = np.zeros(len(d), bool)
    s = (o - a)[None]                                                            # [1,F,3]
    q = np.stack([s[..., 1] * e1[:, 2] - s[..., 2] * e1[:, 1], s[..., 2] * e1[:, 0] - s[..., 0] * e1[:, 2], s[..., 0] * e1[:, 1] - s[..., 1] * e1[:, 0]], -1)
    with np.errstate(all="ignore"):
        for b in range(0, len(d), chunk):
            dd = d[b:b + chunk, None, :]                                         # [R,1,3]
            px = dd[..., 1] * e2[:, 2] - dd[..., 2] * e2[:, 1]
            py = dd[..., 2] * e2[:, 0] - dd[..., 0] * e2[:, 2]
            pz = dd[..., 0] * e2[:, 1] - dd[..., 1] * e2[:, 0]
            det = e1[:, 0] * px + e1[:, 1] * py + e1[:, 2] * pz
            ok = (det != 0.0) & np.isfinite(det)
            idet = 1.0 / det
            u = (s[..., 0] * px + s[..., 1] * py + s[..., 2] * pz) * idet
            v = (dd[..., 0] * q[..., 0] + dd[..., 1] * q[..., 1] + dd[..., 2] * q[..., 2]) * idet
            t = (e2[:, 0] * q[..., 0] + e2[:, 1] * q[..., 1] + e2[:, 2] * q[..., 2]) * idet
            hit = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > 0.0) & (t < t_max)
            hit &= np.arange(F)[None] != own[b:b + chunk, None]
            finite = np.isfinite(d[b:b + chunk]).all(axis=1) & np.isfinite(o).all() & (d[b:b + chunk] != 0.0).any(axis=1)
            out[b:b + chunk] = hit.any(axis=1) & finite
    return out


def np_photo_colors(corners, points, face, P, images, normals=None, anchors=None, cos_min=0.2, feather=16.0, eps=1e-4, blend="mean"):
    """-> dict(colors float64 [P,3], weight float64 [P], n_views, best_view int32 [P], reason int8 [P,N], w float64 [P,N], tie bool [P]),
    colours and weights not rounded. corners: the grid's records, fp32 [F,3,3]; points, anchors, normals fp32; P float64 [N,3,4];
    images fp32 [N,H,W,3]. reason[p,k] says which test camera k failed for texel p (CONTRIBUTES = none); tie[p]: the best weight
    was reached by more than one camera."""
    corners = np.asarray(corners, np.float32).astype(np.float64)
    x = np.asarray(points, np.float32).astype(np.float64)
    y = x if anchors is None else np.asarray(anchors, np.float32).astype(np.float64)
    face = np.asarray(face, np.int64)
    Pm, img = np.asarray(P, np.float64), np.asarray(images, np.float32)
    N, H, W = img.shape[0], img.shape[1], img.shape[2]
    n_pts, F = len(x), len(corners)
    assert ((face >= 0) & (face < F)).all()
    centres = np_centres(Pm)
    if normals is not None:
        g = np.asarray(normals, np.float32).astype(np.float64)
    else:
        c = corners[face]
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    sum_w, sum_c = np.zeros(n_pts), np.zeros((n_pts, 3))
    best_w, best_c, best = np.zeros(n_pts), np.zeros((n_pts, 3)), np.full(n_pts, -1, np.int32)
    n_views, tie = np.zeros(n_pts, np.int32), np.zeros(n_pts, bool)
    reason, w_all = np.full((n_pts, N), NO_NORMAL, np.int8), np.zeros((n_pts, N))
    with np.errstate(all="ignore"):
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        live = (length > 0.0) & (length < np.inf)
        n = g / length[:, None]
        for k in range(N):
            m = Pm[k]
            row = lambda r: ((m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1]) + m[r, 2] * x[:, 2]) + m[r, 3]
            uw, vw, w = row(0), row(1), row(2)
            front = w > 0.0
            u, v = uw / w, vw / w
            ur, vr = np.float64(W - 1) - u, np.float64(H - 1) - v
            frame = (u >= 0.0) & (ur >= 0.0) & (v >= 0.0) & (vr >= 0.0)
            mm = np.minimum(np.minimum(u, ur), np.minimum(v, vr))
            border = np.minimum(1.0, mm / feather) if feather > 0.0 else np.ones(n_pts)
            r = centres[k][None] - x
            cs = ((n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]) / np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
            if normals is None:
                cs = np.maximum(cs, -cs)
            wk = (cs * cs) * border
            facing = (cs > cos_min) & (wk > 0.0)
            cand = live & front & frame & facing
            rows = np.nonzero(cand)[0]
            occ = np.zeros(n_pts, bool)
            occ[rows] = np_occluded(corners, centres[k], y[rows] - centres[k][None], face[rows], 1.0 - eps)
            ok = cand & ~occ
            reason[:, k] = np.where(~live, NO_NORMAL, np.where(~front, BEHIND, np.where(~frame, OUT_OF_FRAME, np.where(~facing, NOT_FACING,
                                    np.where(occ, OCCLUDED, CONTRIBUTES))))).astype(np.int8)
            i = np.nonzero(ok)[0]
            fx0, fy0 = np.floor(u[i]), np.floor(v[i])
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            tx, ty = (u[i] - fx0)[:, None], (v[i] - fy0)[:, None]
            w00, w10, w01, w11 = (1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty
            tap = lambda yy, xx: img[k, yy, xx].astype(np.float64)
            col = (w00 * tap(y0, x0) + w10 * tap(y0, x1)) + (w01 * tap(y1, x0) + w11 * tap(y1, x1))
            wi = wk[i]
            w_all[i, k] = wi
            sum_c[i] = sum_c[i] + wi[:, None] * col
            sum_w[i] = sum_w[i] + wi
            better = wi > best_w[i]
            tie[i] = np.where(better, False, tie[i] | (wi == best_w[i]))
            best_c[i] = np.where(better[:, None], col, best_c[i])
            best[i] = np.where(better, k, best[i])
            best_w[i] = np.where(better, wi, best_w[i])
            n_views[i] += 1
        seen = n_views > 0
        if blend == "mean":
            colors, weight = np.where(seen[:, None], sum_c / sum_w[:, None], 0.0), np.where(seen, sum_w, 0.0)
        else:
            assert blend == "best"
            colors, weight = np.where(seen[:, None], best_c, 0.0), np.where(seen, best_w, 0.0)
    return {"colors": colors, "weight": weight, "n_views": n_views, "best_view": best, "reason": reason, "w": w_all, "tie": tie}


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
H, W, FOCAL = 48, 64, 60.0
FIXTURE_SCALARS = dict(cos_min=0.2, feather=6.0, eps=1e-4)


def look_at(centre, target, focal=FOCAL, height=H, width=W, up=(0.0, 0.0, 1.0)):
    """P = K [R | -R c] of a pinhole at `centre` looking at `target`: x to the right, y down, pixel centres at integers"""
    c, t = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    upv = np.asarray(up, np.float64)
    if abs(z @ upv) > 0.99:
        upv = np.array([0.0, 1.0, 0.0])
    xx = np.cross(z, upv)
    xx /= np.linalg.norm(xx)
    yy = np.cross(z, xx)
    R = np.stack([xx, yy, z])
    K = np.array([[focal, 0.0, (width - 1) / 2.0], [0.0, focal, (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    return K @ np.concatenate([R, -(R @ c)[:, None]], axis=1)


def fixture_mesh():
    """icosphere(1) plus a two-triangle plate at x = 2, between camera 0 and the sphere -> (vertices float64 [46,3], triangles int64 [82,3])"""
    v, t = M.icosphere(1)
    plate = np.array([[2.0, -0.3, -0.3], [2.0, 0.3, -0.3], [2.0, 0.3, 0.4], [2.0, -0.3, 0.4]])
    pt = np.array([[0, 1, 2], [0, 2, 3]], np.int64) + len(v)
    return np.concatenate([v, plate]), np.concatenate([t, pt])


def fixture_cameras():
    """five pinholes: 0 on the +x axis (the plate hides part of the sphere from it), 1 and 2 mirror images about the plane y = 0 -
    a symmetry plane of the mesh - on the same ring, 3 at +z looking away (everything is behind it), 4 close under the sphere (most
    of what faces it projects outside its frame or into the feather band) -> P float64 [5,3,4]"""
    a = np.deg2rad(140.0)
    ring = [(4.0, 0.0, 0.0), (4.0 * np.cos(a), 4.0 * np.sin(a), 0.0), (4.0 * np.cos(a), -4.0 * np.sin(a), 0.0)]
    P = [look_at(c, (0.0, 0.0, 0.0)) for c in ring]
    P.append(look_at((0.0, 0.0, 4.0), (0.0, 0.0, 8.0)))
    P.append(look_at((0.0, 0.0, -1.6), (0.0, 0.0, 0.0), focal=80.0))
    return np.stack(P)


def fixture_images():
    """seeded uniform noise, so that a wrong tap or a swapped axis shows -> fp32 [5,48,64,3]"""
    return np.random.default_rng(20).random((5, H, W, 3), dtype=np.float32)


def fixture_case(n, with_normals, with_anchors):
    """the arguments of one configuration -> dict(v, t, corners, points, anchors, face, normals, P, images); `anchors` are the texel
    points on their triangles, and with_anchors moves the lookup points 0.02 inwards along the outward normal. The outward normals
    (the sphere's radius vector, +x on the plate) have y = 0 exactly on the plane y = 0, where cameras 1 and 2 tie."""
    key = ("case", n, with_normals, with_anchors)
    if key not in _CACHE:
        v, t = fixture_mesh()
        on_face, face = M.np_texel_points(v, t, n)
        outward = np.where((face >= 80)[:, None], np.array([[1.0, 0.0, 0.0]], np.float32), on_face).astype(np.float32)
        unit = (outward.astype(np.float64) / np.linalg.norm(outward.astype(np.float64), axis=1, keepdims=True))
        points = (on_face.astype(np.float64) - 0.02 * unit).astype(np.float32) if with_anchors else on_face
        _CACHE[key] = dict(v=v, t=t, corners=v.astype(np.float32)[t], points=points, anchors=on_face if with_anchors else None, face=face,
                           normals=outward if with_normals else None, P=fixture_cameras(), images=fixture_images())
    return _CACHE[key]


def fixture_model(n, with_normals, with_anchors, blend, use_anchors=True):
    key = ("model", n, with_normals, with_anchors, blend, use_anchors)
    if key not in _CACHE:
        c = fixture_case(n, with_normals, with_anchors)
        _CACHE[key] = np_photo_colors(c["corners"], c["points"], c["face"], c["P"], c["images"], normals=c["normals"],
                                      anchors=c["anchors"] if use_anchors else None, blend=blend, **FIXTURE_SCALARS)
    return _CACHE[key]


@pytest.mark.parametrize("n", [4, 5])
def test_the_fixture_takes_every_branch(n):
    c = fixture_case(n, True, False)
    assert len(c["t"]) == 82 and len(c["points"]) == {4: 80 * 6 + 12, 5: 80 * 10 + 20}[n] and len(c["points"]) % 64 != 0 and len(c["points"]) > 256
    # cameras 1 and 2 are mirror images about y = 0, and the mesh is its own mirror image there
    c1, c2 = np_centres(c["P"])[1:3]
    assert np.allclose(c1 * [1, -1, 1], c2, atol=1e-12)
    mirrored = c["v"] * [1, -1, 1]
    assert all(np.abs(c["v"] - m).sum(axis=1).min() < 1e-12 for m in mirrored)
    got = fixture_model(n, True, False, "mean")
    r = got["reason"]
    assert (r[:, 3] == BEHIND).all()                                             # the camera that looks away
    assert (r[:, :3] != BEHIND).all()
    for code in (CONTRIBUTES, OUT_OF_FRAME, NOT_FACING):
        assert (r[:, 4] == code).any(), code                                     # the close camera
    assert (r[:, 0] == OCCLUDED).any() and not (r[:, 1:] == OCCLUDED).any()      # the plate hides from camera 0 only (given, one-sided normals)
    sphere = c["face"] < 80
    assert (r[sphere, 0] == OCCLUDED).any() and (r[sphere, 0] == CONTRIBUTES).any()
    # the feather band: a weight scaled down by the border factor, and weights that are not
    cs2 = got["w"][:, 4][r[:, 4] == CONTRIBUTES]
    assert len(cs2) > 0
    band = fixture_model(n, True, False, "mean")["w"][:, 4] != np_photo_colors(
        c["corners"], c["points"], c["face"], c["P"], c["images"], normals=c["normals"], cos_min=0.2, feather=0.0, eps=1e-4)["w"][:, 4]
    assert band.any()
    # the tie: cameras 1 and 2 reach the same, best weight at texels of the plane y = 0, and the lower index wins
    tie = got["tie"] & (got["w"][:, 1] == got["w"][:, 2]) & (got["w"][:, 1] > 0) & (got["w"][:, 1] >= got["w"].max(axis=1))
    assert tie.any() and (got["best_view"][tie] == 1).all() and (c["points"][tie][:, 1] == 0).all()
    assert (got["n_views"] == 0).any() and (got["n_views"] >= 2).any()
    assert (got["best_view"][got["n_views"] == 0] == -1).all() and not got["colors"][got["n_views"] == 0].any()
    # two-sided face normals let the far side pass the facing test: the walk is what rejects it
    two = fixture_model(n, False, False, "mean")
    assert (two["reason"][sphere][:, :3] == OCCLUDED).sum() > (r[sphere][:, :3] == OCCLUDED).sum()
    # best picks one camera's colour, mean mixes: they differ where two cameras see a texel, and agree where one does
    best = fixture_model(n, True, False, "best")
    assert np.array_equal(best["n_views"], got["n_views"]) and np.array_equal(best["best_view"], got["best_view"])
    one = got["n_views"] == 1
    assert one.any() and np.abs(best["colors"][one] - got["colors"][one]).max() < 1e-15
    assert np.abs(best["colors"][got["n_views"] >= 2] - got["colors"][got["n_views"] >= 2]).max() > 0.01


@pytest.mark.parametrize("n", [4, 5])
def test_the_own_face_rule_needs_the_anchors(n):
    """lookup points 0.02 under their triangles: with the anchors the segments end on the triangle and the own face is ignored; without
    them the segments end under the surface, behind the neighbours, and texels lose their cameras"""
    flat = fixture_model(n, True, False, "mean")
    with_anchors = fixture_model(n, True, True, "mean")
    without = fixture_model(n, True, True, "mean", use_anchors=False)
    assert (without["n_views"] < with_anchors["n_views"]).sum() > 20
    assert ((without["n_views"] == 0) & (with_anchors["n_views"] > 0)).any()
    # and with them, exactly the cameras that see the point on its triangle are left, up to the frame and the angle moving a little
    assert (with_anchors["n_views"] != flat["n_views"]).mean() < 0.1


def test_model_on_a_hand_made_case():
    """one triangle facing a camera on its axis: the colour is the bilinear value at the projected position, the weight cos^2"""
    corners = np.array([[[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]]], np.float32)
    P = look_at((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), focal=50.0, height=9, width=11)[None]
    img = np.zeros((1, 9, 11, 3), np.float32)
    img[0, :, :, 0] = np.arange(11)[None] / 10.0
    img[0, :, :, 1] = np.arange(9)[:, None] / 8.0
    pts = np.array([[0.0, 0.0, 0.0], [0.25, -0.125, 0.0], [0.0, 0.0, 0.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], np.float32)
    got = np_photo_colors(corners, pts, [0, 0, 0], P, img, normals=nrm, feather=0.0)
    assert got["n_views"].tolist() == [1, 1, 0] and got["best_view"].tolist() == [0, 0, -1] and got["reason"][2, 0] == NOT_FACING
    assert abs(got["weight"][0] - 1.0) < 1e-15
    uv = (P[0] @ np.append(pts[1].astype(np.float64), 1.0))
    u, v = uv[0] / uv[2], uv[1] / uv[2]
    assert np.abs(got["colors"][1] - [u / 10.0, v / 8.0, 0.0]).max() < 1e-7
    assert np.abs(got["colors"][0] - [0.5, 0.5, 0.0]).max() < 1e-7
    # a second triangle in front of the first hides it, unless it is the texel's own
    both = np.concatenate([corners, corners + np.float32([0, 0, 1])])
    assert np_photo_colors(both, pts[:1], [0], P, img, normals=nrm[:1])["reason"][0, 0] == OCCLUDED
    assert np_photo_colors(both, pts[:1] + np.float32([0, 0, 1]), [1], P, img, normals=nrm[:1])["n_views"][0] == 1
    # without normals the face's own counts, from either side
    assert np_photo_colors(corners[:, ::-1], pts[:1], [0], P, img)["n_views"][0] == 1


# ---- the model against a painted sphere --------------------------------------------------------------------------------------------------
PAINT_H, PAINT_W, PAINT_FOCAL, PAINT_COS_MIN = 96, 128, 120.0, 0.5
# max |model - paint| measured here (icosphere(3), n = 4, six 96 x 128 views from distance 3, seed-free): the bilinear sampling error
PAINT_MEASURED = 1.74e-3


def paint(p):
    """a smooth colour of a point of the unit sphere, three channels in [0, 1]"""
    p = np.asarray(p, np.float64)
    return 0.5 + 0.5 * np.sin(4.0 * p @ np.array([[1.0, 0.3, -0.5], [-0.4, 1.0, 0.2], [0.3, -0.6, 1.0]]) + M.PHASE[None])


def painted_views():
    """six cameras on the axes at distance 3; every pixel's ray is intersected with the unit sphere analytically -> (P, images)"""
    centres = [np.array(c, np.float64) * 3.0 for c in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    P = np.stack([look_at(c, (0, 0, 0), focal=PAINT_FOCAL, height=PAINT_H, width=PAINT_W) for c in centres])
    px, py = np.meshgrid(np.arange(PAINT_W, dtype=np.float64), np.arange(PAINT_H, dtype=np.float64))
    images = np.zeros((6, PAINT_H, PAINT_W, 3), np.float32)
    for k, c in enumerate(centres):
        d = np.linalg.solve(P[k][:, :3], np.stack([px.ravel(), py.ravel(), np.ones(px.size)]))      # M d = (u, v, 1)
        d = (d / np.linalg.norm(d, axis=0)).T
        b = d @ c
        disc = b * b - (c @ c - 1.0)
        hit = disc > 0.0
        tt = -b - np.sqrt(np.where(hit, disc, 0.0))
        col = np.where(hit[:, None], paint(c[None] + tt[:, None] * d), 0.0)
        images[k] = col.reshape(PAINT_H, PAINT_W, 3).astype(np.float32)
    return P, images


def test_model_against_a_painted_sphere():
    v, t = M.icosphere(3)
    on_face, face = M.np_texel_points(v, t, 4)
    on_sphere = (on_face.astype(np.float64) / np.linalg.norm(on_face.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    P, images = painted_views()
    got = np_photo_colors(v.astype(np.float32)[t], on_sphere, face, P, images, normals=on_sphere, anchors=on_face, cos_min=PAINT_COS_MIN, feather=0.0)
    seen = got["n_views"] > 0
    err = np.abs(got["colors"][seen] - paint(on_sphere[seen].astype(np.float64)))
    print("painted sphere: coverage %.3f, max |model - paint| = %.3e, mean %.3e" % (seen.mean(), err.max(), err.mean()))
    assert seen.mean() > 0.7
    assert err.max() <= 2.0 * PAINT_MEASURED
    # mixing the images up is far outside that bound: the check has teeth
    wrong = np_photo_colors(v.astype(np.float32)[t], on_sphere, face, P, images[::-1], normals=on_sphere, anchors=on_face, cos_min=PAINT_COS_MIN, feather=0.0)
    assert np.abs(wrong["colors"][seen] - paint(on_sphere[seen].astype(np.float64))).max() > 0.1


# ---- the interface, as far as it shows without a device --------------------------------------------------------------------------------
def test_library_declares_the_entry_point_and_keeps_the_abi():
    import ctypes
    from vdn_hip import build, lib
    text = open(lib.HEADER).read()
    assert re.search(r"int\s+vdn_tex_photo\s*\(\s*const\s+VdnTexPhotoArgs\s*\*", text)
    assert len(lib.FUNCTIONS["vdn_tex_photo"]) == 2
    # 15 pointers, 4 int64, 8 doubles, 6 int32
    assert ctypes.sizeof(lib.VdnTexPhotoArgs) == 15 * 8 + 4 * 8 + 8 * 8 + 6 * 4
    names = [f[0] for f in lib.VdnTexPhotoArgs._fields_]
    assert names[:7] == ["points", "anchors", "face", "normals", "P_mat", "centres", "images"] and names[-1] == "blend"
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", text).group(1)) == 28
    if os.path.exists(lib.LIB_PATH):
        assert hasattr(lib.load(), "vdn_tex_photo") and lib.call_value("vdn_abi_version") == 28
    assert build.PER_FILE_FLAGS["mesh_photo.hip"] == ["-ffp-contract=off"]
    assert "mesh_photo.hip" in build._sources()
    # the walk is shared, not copied
    ray = open(os.path.join(lib.PKG, "csrc", "mesh_ray.hip")).read()
    photo = open(os.path.join(lib.PKG, "csrc", "mesh_photo.hip")).read()
    for src in (ray, photo):
        assert '#include "k_ray_grid.h"' in src and "RayHit cast_ray" not in src


def test_entry_point_refuses_bad_blocks_on_the_host():
    from vdn_hip import lib
    if not os.path.exists(lib.LIB_PATH):                                         # (as test_mesh_texture_cpu.py: the declaration tests stand alone)
        return
    so = lib.load()
    import ctypes

    def block(**kw):
        a = lib.VdnTexPhotoArgs()
        for name, ctype in a._fields_:
            if ctype is ctypes.c_void_p:
                setattr(a, name, 64)                                             # (never dereferenced: every call below is refused)
        a.P, a.N, a.F, a.n_refs, a.h, a.nx, a.ny, a.nz, a.H, a.W = 10, 2, 4, 8, 1.0, 2, 2, 2, 8, 8
        a.cos_min, a.feather, a.eps = 0.2, 16.0, 1e-4
        for k, x in kw.items():
            setattr(a, k, x)
        return a
    assert so.vdn_tex_photo(None, None) == -1
    for bad in (dict(points=None), dict(images=None), dict(error=None), dict(P=0), dict(N=0), dict(F=0), dict(H=0), dict(blend=2), dict(cos_min=1.0),
                dict(cos_min=float("nan")), dict(feather=-1.0), dict(feather=float("inf")), dict(eps=1.0), dict(h=0.0), dict(nx=0)):
        assert so.vdn_tex_photo(ctypes.byref(block(**bad)), None) == -1, bad
    for big in (dict(P=1 << 31), dict(N=1 << 31), dict(F=1 << 31), dict(n_refs=1 << 31), dict(nx=1 << 11, ny=1 << 10, nz=1 << 10)):
        assert so.vdn_tex_photo(ctypes.byref(block(**big)), None) == -10, big


def test_front_doors_take_the_new_arguments():
    import inspect
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import texture_mesh
    finally:
        sys.path.pop(0)
    from vdn_hip import mesh
    from vdn_train import mesh_texture
    p = inspect.signature(mesh.photo_colors).parameters
    assert (p["normals"].default, p["anchors"].default, p["cos_min"].default, p["feather"].default, p["eps"].default, p["blend"].default) == \
        (None, None, 0.2, 16.0, 1e-4, "mean")
    assert inspect.signature(mesh.bake_texture).parameters["photos"].default is None
    assert callable(mesh_texture.bake_photo_texture)
    ap = texture_mesh.parser()
    a = ap.parse_args(["a.ply", "b.obj", "--photos", "scene", "--blend", "best", "--cos-min", "0.3", "--feather", "8", "--views", "0,2,5", "--project", "0"])
    assert (a.photos, a.blend, a.cos_min, a.feather, a.views, a.checkpoint, a.synthetic) == ("scene", "best", 0.3, 8.0, "0,2,5", None, None)
    a = ap.parse_args(["a.ply", "b.obj", "--synthetic", "0"])
    assert (a.photos, a.blend, a.cos_min, a.feather, a.views) == (None, "mean", 0.2, 16.0, None)
    with pytest.raises(SystemExit):
        ap.parse_args(["a.ply", "b.obj", "--blend", "median", "--synthetic", "0"])
    # argument checks that need no device
    with pytest.raises(ValueError):
        mesh.bake_texture(None, np.zeros((3, 3)), np.zeros((1, 3), np.int64), project=0, shade=lambda p, f: p, photos={"P": np.zeros((0, 3, 4)), "images": None})
    for bad in ({"P": 1}, {"P": 1, "images": 2, "colour": 3}, {"P": 1, "images": 2, "blend": "median"}, {"P": 1, "images": 2, "cos_min": 1.0},
                {"P": 1, "images": 2, "feather": -1}, {"P": 1, "images": 2, "eps": 1.0}, {"P": 1, "images": 2, "fill": (1, 2)}, [1, 2]):
        with pytest.raises(ValueError):
            mesh.bake_texture(None, np.zeros((3, 3)), np.zeros((1, 3), np.int64), project=0, photos=bad)
