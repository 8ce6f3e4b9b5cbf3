"""Constructed inputs for the hierarchical sampler (tests/test_sampler_model_cpu.py, tests/test_gpu_sampler.py).

Every case is a dict of float32 numpy arrays plus a few Python scalars, deterministic from its name, and BUILT to land in a class
- homogeneous in conditioning, so that one bound holds for every entry of it:

  tight   every ray crosses a surface inside the unit sphere (or is a given-weights row): float32 and float64 agree on every new
          depth to <= 1e-5 and no u comes within 10 x the CDF's float32 error of a CDF knot or of the denom < 1e-5 threshold.
          Held entry by entry to the float64 depths.
  ill     rays that miss or graze, rays wholly outside the unit sphere, a constant SDF: the weights are all ~1e-5 + round-off, the
          CDF is flat and the inverse is ill-conditioned in depth. Held by the CDF residual instead.

The SDF rows are numbers the kernel is handed, not a network's output: where a profile along the ray says more than a sphere
(saturation, a first sample inside the surface, ties) it is written down directly. Every |p| - 1 is at least 1e-4 from zero
(checked in float64 on the float32 values at the end of the builder), so the `inside` flag cannot flip with the precision.
The seeds in the table were chosen so that the class conditions hold; tests/test_sampler_model_cpu.py asserts that they do.
"""
import zlib

import numpy as np
import torch

MARGIN = 1e-4
LD_FIXED = 160

# name -> (builder, cls, B, M, n_imp, ld ("M" | "M+n" | 160), inv_s, seed)
UPSAMPLE_CASES = {
    "clean-B77-M64-n16": ("sphere", "tight", 77, 64, 16, "M", 64.0, 0),
    "clean-B4-M128-n16": ("sphere", "tight", 4, 128, 16, 160, 2048.0, 0),
    "clean-B1-M2-n1": ("sphere", "tight", 1, 2, 1, "M+n", 64.0, 0),
    "clean-B3-M3-n17": ("sphere", "tight", 3, 3, 17, 160, 512.0, 0),
    "noisy-B5-M112-n16": ("noisy", "tight", 5, 112, 16, 160, 512.0, 0),
    "noisy-B77-M65-n17": ("noisy", "tight", 77, 65, 17, "M+n", 64.0, 0),
    "noisy-B3-M255-n64": ("noisy", "tight", 3, 255, 64, "M", 64.0, 0),
    "two_surfaces-B5-M63-n16": ("two_surfaces", "tight", 5, 63, 16, "M+n", 64.0, 0),
    "first_inside-B5-M64-n16": ("first_inside", "tight", 5, 64, 16, 160, 64.0, 0),
    "first_deep-B4-M65-n17": ("first_deep", "tight", 4, 65, 17, "M", 2048.0, 0),
    "ties-B5-M112-n16": ("ties", "tight", 5, 112, 16, "M+n", 2048.0, 0),
    "saturated-B3-M256-n64": ("saturated", "tight", 3, 256, 64, "M", 2048.0, 0),
    "leave-B77-M128-n16": ("leave", "tight", 77, 128, 16, 160, 512.0, 0),
    "miss-B5-M63-n16": ("miss", "ill", 5, 63, 16, "M", 64.0, 0),
    "graze-B77-M112-n16": ("graze", "ill", 77, 112, 16, 160, 512.0, 0),
    "outside-B4-M65-n17": ("outside", "ill", 4, 65, 17, "M+n", 512.0, 0),
    "constant-B3-M128-n64": ("constant", "ill", 3, 128, 64, 160, 2048.0, 0),
    # the given-weights form (sample_pdf alone): w_ld M - 1 and M + 2
    "zero_runs-B5-M64-n16": ("zero_runs", "tight", 5, 64, 16, "M", 64.0, 0),
    "flat_u-B3-M65-n17": ("flat_u", "tight", 3, 65, 17, 160, 64.0, 0),
    "exact_knots-B5-M5-n3": ("exact_knots", "tight", 5, 5, 3, "M+n", 64.0, 0),
    "given-B4-M256-n64": ("given", "tight", 4, 256, 64, "M", 64.0, 0),
}
GIVEN_WEIGHTS = ("zero_runs", "flat_u", "exact_knots", "given")


def upsample_case_names(cls=None):
    return [n for n, c in UPSAMPLE_CASES.items() if cls is None or c[1] == cls]


def _rng(name, seed=0):
    return np.random.RandomState(zlib.crc32(("%s/%d" % (name, seed)).encode()))


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays(rs, B, b_max, dist=2.5):
    """Origins at `dist` from the centre, aimed at a point within b_max of it. -> float32 o, d and float64 mid = -o.d (|d| = 1)."""
    o = _unit(rs.randn(B, 3)) * dist
    d = _unit(_unit(rs.randn(B, 3)) * b_max * rs.rand(B, 1) - o)
    o, d = _f32(o), _f32(d)
    mid = -(o.astype(np.float64) * d).sum(-1) / (d.astype(np.float64) ** 2).sum(-1)
    return o, d, mid


def _rows(rs, lo, hi, M):
    """Jittered, strictly ascending depths in [lo, hi] per ray: spacing between 0.4 and 1.6 of (hi - lo) / M."""
    t = (np.arange(M)[None, :] + 0.5 + 0.6 * (rs.rand(lo.shape[0], M) - 0.5)) / M
    return _f32(lo[:, None] + (hi - lo)[:, None] * t)


def _pts(o, d, z):
    return o.astype(np.float64)[:, None, :] + d.astype(np.float64)[:, None, :] * z.astype(np.float64)[..., None]


def _keep_off_the_unit_sphere(o, d, z):
    """Move a depth whose |p| comes within 2 MARGIN of 1 by 6 MARGIN (the rows' spacing is >= 3e-3: the order is kept)."""
    pn = np.linalg.norm(_pts(o, d, z), axis=-1)
    z = np.where(np.abs(pn - 1.0) < 2 * MARGIN, z + np.float32(6 * MARGIN), z)
    return _f32(z)


def _sphere_sdf(o, d, z, centre, radius):
    return np.linalg.norm(_pts(o, d, z) - centre[:, None, :], axis=-1) - radius[:, None]


def _sphere_beside(rs, o, d, mid, gap):
    """(centre, radius) of a sphere whose surface the ray passes at the distance `gap` [B] (closest at depth mid)."""
    n = _unit(np.cross(d.astype(np.float64), rs.randn(o.shape[0], 3)))
    return _pts(o, d, mid[:, None])[:, 0] + n * 0.5, 0.5 - gap


def _profile(z, knots_z, knots_s):
    """Piecewise-linear SDF profile along each ray through (knots_z[b], knots_s[b])."""
    return np.stack([np.interp(z[b].astype(np.float64), knots_z[b], knots_s[b]) for b in range(z.shape[0])])


def upsample_case(name):
    """-> dict: rays_o, rays_d [B,3], z, sdf [B,M] (sdf None for the given-weights form), weights [B,M-1] or None, u [n_imp], and
    B, M, n_imp, ld, w_ld, inv_s, cls, kind, exact_knots."""
    kind, cls, B, M, n_imp, ld, inv_s, seed = UPSAMPLE_CASES[name]
    rs = _rng(name, seed)
    ld = M if ld == "M" else M + n_imp if ld == "M+n" else ld
    u = torch.linspace(0.5 / n_imp, 1.0 - 0.5 / n_imp, n_imp).numpy()      # the renderer's own u
    c = {"name": name, "kind": kind, "cls": cls, "B": B, "M": M, "n_imp": n_imp, "ld": ld, "inv_s": inv_s, "weights": None,
         "w_ld": 0, "exact_knots": False}
    if kind in ("outside",):
        # the ray passes the unit sphere at a distance of 1.3: no sample is inside it
        o = _unit(rs.randn(B, 3)) * 2.5
        perp = _unit(np.cross(o, rs.randn(B, 3)))
        d = _unit(perp * 1.3 - o)
        o, d = _f32(o), _f32(d)
        mid = -(o.astype(np.float64) * d).sum(-1)
    else:
        o, d, mid = _rays(rs, B, 0.25)
    if kind == "leave":
        z = _rows(rs, mid - 0.6, mid + 1.5, M)                 # |p| passes 1 on the way out
    else:
        z = _rows(rs, mid - 0.9, mid + 0.9, M)                 # |p|^2 <= 0.25^2 + 0.81 < 1 (outside: >= 1.3^2)
    z = _keep_off_the_unit_sphere(o, d, z)
    centre = _unit(rs.randn(B, 3)) * 0.08
    radius = 0.4 + 0.2 * rs.rand(B)
    sdf = _sphere_sdf(o, d, z, centre, radius)
    zc = mid + 0.5 * (rs.rand(B) - 0.5)                        # where the written-down profiles cross zero
    z0, z1 = z[:, 0].astype(np.float64), z[:, -1].astype(np.float64)
    if kind == "noisy":
        sdf = sdf + 0.01 * rs.randn(B, M)
    elif kind == "leave":
        # every other ray meets its surface where it leaves the unit sphere (a fall of 1 per unit depth through |p| = 1): the
        # section that carries the weight has one end inside and one outside
        oo = o.astype(np.float64)
        z_exit = mid + np.sqrt(1.0 - ((oo ** 2).sum(-1) - mid ** 2))
        sdf[1::2] = np.clip(z_exit[:, None] - z.astype(np.float64), -0.3, 0.5)[1::2]
    elif kind == "two_surfaces":
        # the first sphere is passed at sdf = +0.02 (it absorbs a part of the ray at inv_s = 64), the second is crossed
        p1 = _pts(o, d, (mid - 0.45)[:, None].astype(np.float32))[:, 0]
        n = _unit(np.cross(d.astype(np.float64), rs.randn(B, 3)))
        s1 = _sphere_sdf(o, d, z, p1 + n * 0.22, np.full(B, 0.2))
        p2 = _pts(o, d, (mid + 0.4)[:, None].astype(np.float32))[:, 0]
        s2 = _sphere_sdf(o, d, z, p2 + n * 0.05, np.full(B, 0.25))
        sdf = np.minimum(s1, s2)
    elif kind == "first_inside":
        # sample 0 is already behind the surface and the row goes deeper (slope -0.5), comes out, and ends on a steep fall
        # (slope -3): prev_cos of sample 0 is zero, not the slope of the row's other end
        kz = np.stack([z0, z0 + 0.25, z0 + 0.7, z1 - 0.12, z1], -1)
        ks = np.stack([-0.003 + 0 * z0, -0.128 + 0 * z0, 0.3 + 0 * z0, 0.3 + 0 * z0, -0.06 + 0 * z0], -1)
        sdf = _profile(z, kz, ks)
    elif kind == "first_deep":
        # sample 0 at sdf = -0.01 with inv_s = 2048: prev_cdf ~ 1e-9, the 1e-5 of alpha's quotient is all of it
        kz = np.stack([z0, z0 + 0.5, z1], -1)
        ks = np.stack([-0.01 + 0 * z0, -0.2 + 0 * z0, -0.3 + 0 * z0], -1)
        sdf = _profile(z, kz, ks)
    elif kind == "saturated":
        # a fall of 30 per unit depth across the surface: one section takes |sdf| * inv_s from > 90 to < -90
        sdf = np.clip(-30.0 * (z.astype(np.float64) - zc[:, None]), -0.2, 0.2)
    elif kind == "ties":
        # the clean sphere at inv_s = 2048, with per ray (k = the last sample in front of the surface):
        #   a near-tie z[k+1] = z[k] + 1e-6 across the surface (sdf +-0.015): raw cos = -0.03 / 1.1e-5 < -1e3, the lower clip;
        #   an exact tie with equal sdf in front of the surface (what a merge of a duplicate depth makes): raw cos = 0;
        #   an exact tie and a near-tie with a fall of 0.03 behind the surface: raw cos ~ -3e3, the lower clip again
        z = z.astype(np.float64)
        for b in range(B):
            k = int(np.argmax(sdf[b] < 0.0)) - 1
            assert 8 <= k < M - 12, (name, b, k)
            delta = 2e-4 * (rs.rand() - 0.5)
            z[b, k + 1] = np.float32(z[b, k]) + np.float32(1e-6)
            sdf[b, k], sdf[b, k + 1] = 0.015 + delta, -0.015 + delta
            z[b, 4], sdf[b, 4] = z[b, 3], sdf[b, 3]
            z[b, k + 8], sdf[b, k + 8] = z[b, k + 7], sdf[b, k + 7] - 0.03
            z[b, k + 11], sdf[b, k + 11] = np.float32(z[b, k + 10]) + np.float32(1e-6), sdf[b, k + 10] - 0.03
        z = _f32(z)
    elif kind == "miss":
        # the sphere is passed at a distance: sdf >= 0.15 everywhere, every weight ~2e-5
        sdf = _sphere_sdf(o, d, z, *_sphere_beside(rs, o, d, mid, 0.15 + 0.2 * rs.rand(B)))
    elif kind == "graze":
        # ... at 0.004 to 0.008: sdf * inv_s comes down to 2 .. 4, a part of the ray is absorbed
        sdf = _sphere_sdf(o, d, z, *_sphere_beside(rs, o, d, mid, 0.004 * (1.0 + rs.rand(B))))
    elif kind == "constant":
        sdf = np.full((B, M), 0.05) * (1.0 + np.arange(B))[:, None]
    if kind in GIVEN_WEIGHTS:
        w = rs.rand(B, M - 1) ** 3
        w = w / w.sum(-1, keepdims=True)
        c["w_ld"] = M + 2 if kind in ("flat_u", "given") else M - 1
        if kind == "zero_runs":
            w[:, 5:12] = 0.0
            w[:, 30:31] = 0.0
            w[:, M - 9:] = 0.0
            w[1::2, :3] = 0.0
        elif kind == "flat_u":
            # one weight row for every ray (u is shared by the rays), sum(w + 1e-5) = 4/3: a zero weight is a bin of 7.5e-6, flat
            # (< 1e-5) with 2.5e-6 to spare, and three of the u sit 5e-6 behind such a bin's left knot, 2.5e-6 in front of the next
            w = np.repeat(w[:1], B, 0)
            w[:, 20:31] = 0.0
            w = w / w.sum(-1, keepdims=True) * (4.0 / 3.0 - (M - 1) * 1e-5)
            w = _f32(w).astype(np.float64)
            cdf = np.concatenate([[0.0], np.cumsum((w[0] + 1e-5) / (w[0] + 1e-5).sum())])
            u = np.sort(np.concatenate([u[:-3].astype(np.float64), cdf[[22, 25, 28]] + 5e-6])).astype(np.float32)
        elif kind == "exact_knots":
            # equal weights, M - 1 = 4: pdf = 0.25 and the knots 0.25, 0.5, 0.75 exactly, in float32 and in float64; u ON them
            # (t == 0 there and the new depth IS z[below]; the depths run from -3 to 3 with |z| falling by a factor of ~10 per bin on the way, so that the neighbouring
            # bin's z[k-1] + 1 * (z[k] - z[k-1]) rounds and a search with right=False shows; a camera inside the unit sphere has
            # negative depths too)
            w = np.full((B, M - 1), 0.3)
            u = np.asarray([0.25, 0.5, 0.75], np.float32)
            z = _f32(np.sort(np.asarray([-3.1, -0.37, 0.011, 0.23, 2.9])[None, :] * (1.0 + 0.3 * rs.rand(B, M)), -1))
            c["exact_knots"] = True
        elif kind == "given":
            # no bin thinner than 1 / 2000 of the mass; the first and the last bin are drawn from: below == 0, above == M - 1
            w = 0.2 + rs.rand(B, M - 1)
            w[:, 0] = w[:, -1] = 40.0
            w = w / w.sum(-1, keepdims=True)
        c["weights"] = _f32(w)
        sdf = None
    c.update({"rays_o": o, "rays_d": d, "z": z, "sdf": None if sdf is None else _f32(sdf), "u": u})
    pn = np.linalg.norm(_pts(o, d, z), axis=-1)
    assert (np.abs(pn - 1.0) >= MARGIN).all(), name
    assert (np.diff(z, axis=-1) >= 0).all(), name
    return c


# ---- merge ------------------------------------------------------------------------------------------------------------------
# name -> (B, M, K, ld, ld_out, in_place, with_sdf, old row sorted)
MERGE_CASES = {
    "merge-B1-M1-K1": (1, 1, 1, 1, 2, False, True, True),
    "merge-B3-M64-K16-inplace": (3, 64, 16, 128, 128, True, True, True),
    "merge-B5-M112-K16-inplace-nosdf": (5, 112, 16, 128, 128, True, False, True),
    "merge-B3-M64-K16-nosdf": (3, 64, 16, 64, 80, False, False, True),
    "merge-B5-M112-K16": (5, 112, 16, 112, 131, False, True, True),
    "merge-B2-M192-K64": (2, 192, 64, 200, 256, False, True, True),
    "merge-B77-M240-K16-inplace": (77, 240, 16, 256, 256, True, True, True),
    "merge-B4-M80-K16-unsorted": (4, 80, 16, 96, 160, False, True, False),
    "merge-B9-M96-K32-unsorted-inplace-nosdf": (9, 96, 32, 160, 160, True, False, False),
}


def merge_case(name):
    """-> dict: z, sdf [B,M], new_z, new_sdf [B,K] (sdf None without), shapes. Depths on a grid of 1/40, so that ties between old
    and new, among the old and among the new ones are everywhere; an unsorted old row takes the counting path."""
    B, M, K, ld, ld_out, in_place, with_sdf, old_sorted = MERGE_CASES[name]
    rs = _rng(name)
    z = np.round(rs.rand(B, M) * 40) / 40 + 1.0
    nz = np.sort(np.round(rs.rand(B, K) * 40) / 40 + 1.0, -1)
    if old_sorted:
        z = np.sort(z, -1)
    else:
        z[0] = np.sort(z[0])                                   # one sorted row among the unsorted ones
    c = {"name": name, "B": B, "M": M, "K": K, "ld": ld, "ld_out": ld_out, "in_place": in_place, "z": _f32(z), "new_z": _f32(nz),
         "sdf": _f32(rs.randn(B, M)) if with_sdf else None, "new_sdf": _f32(rs.randn(B, K)) if with_sdf else None}
    return c


# ---- merge + up-sample (vdn_merge_upsample) and the training step's last merge (vdn_train_prep) ------------------------------

MERGE_UPSAMPLE_SHAPES = [(1, 1, 1, 1), (2, 64, 16, 16), (3, 112, 16, 16), (77, 64, 16, 16), (3, 240, 16, 64), (2, 64, 64, 64), (77, 112, 1, 16),
                         (1, 240, 16, 1), (3, 1, 64, 16)]          # (B, M, K, n_imp), in place with ld = ld_out = 160


def merge_upsample_case(B, M, K, n_imp):
    """A noisy-sphere row of M + K ascending depths split at random into M old and K new ones (each part in ascending order),
    with their SDF values; inv_s = 512. -> dict with z, sdf [B,M], new_z, new_sdf [B,K], rays, u."""
    name = "mu-B%d-M%d-K%d-n%d" % (B, M, K, n_imp)
    rs = _rng(name)
    o, d, mid = _rays(rs, B, 0.25)
    zz = _keep_off_the_unit_sphere(o, d, _rows(rs, mid - 0.9, mid + 0.9, M + K))
    sd = _f32(_sphere_sdf(o, d, zz, _unit(rs.randn(B, 3)) * 0.08, 0.4 + 0.2 * rs.rand(B)) + 0.01 * rs.randn(B, M + K))
    old = np.stack([np.sort(rs.permutation(M + K)[:M]) for _ in range(B)])
    new = np.stack([np.setdiff1d(np.arange(M + K), old[b]) for b in range(B)])
    take = lambda a, i: np.ascontiguousarray(np.take_along_axis(a, i, 1))
    return {"name": name, "B": B, "M": M, "K": K, "n_imp": n_imp, "inv_s": 512.0, "rays_o": o, "rays_d": d, "cls": "tight",
            "z": take(zz, old), "sdf": take(sd, old), "new_z": take(zz, new), "new_sdf": take(sd, new),
            "u": torch.linspace(0.5 / n_imp, 1.0 - 0.5 / n_imp, n_imp).numpy()}


TRAIN_PREP_SHAPES = [(1, 128, 112, 128), (5, 128, 127, 160), (37, 128, 64, 160), (4, 128, 112, 160)]      # (B, N, M_old, z_ld), n_outside = 32


def train_prep_case(B, N, M_old, z_ld, O=32):
    """Sorted old row [B,M_old], the last round's samples [B,N-M_old] and outside depths [B,O] on a grid of 1/64 over the same
    range, so that the old row, the new samples and the outside depths tie with each other."""
    name = "tp-B%d-N%d-M%d-ld%d" % (B, N, M_old, z_ld)
    rs = _rng(name)
    o, d, mid = _rays(rs, B, 0.25)
    grid = lambda n: _f32(np.sort(mid[:, None] - 1.0 + np.round(rs.rand(B, n) * 128) / 64, -1))
    return {"name": name, "B": B, "N": N, "M_old": M_old, "z_ld": z_ld, "O": O, "rays_o": o, "rays_d": d, "z": grid(M_old),
            "new_z": grid(N - M_old), "z_out": grid(O)}


def network_rays(B, tag="net"):
    """Rays for the launches that evaluate a network's SDF themselves: aimed within 0.25 of the centre (they cross the sphere of
    radius 0.5 a geometric initialisation makes), near / far = mid -+ 0.95, so that every sample lies inside the unit sphere
    (|p|^2 <= 0.25^2 + 0.95^2 < 0.97) and the `inside` flag cannot depend on the precision. -> float32 o, d [B,3], near, far [B]."""
    o, d, mid = _rays(_rng("%s-B%d" % (tag, B)), B, 0.25)
    return o, d, _f32(mid - 0.95), _f32(mid + 0.95)
