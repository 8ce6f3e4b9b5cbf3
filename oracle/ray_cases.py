"""Constructed inputs for the per-ray kernels (tests/test_ray_ops_model_cpu.py, tests/test_gpu_ray_ops.py).

Every case is a dict of float32 numpy arrays (plus a few Python scalars), deterministic from its name, and BUILT to land in a
regime - not drawn and hoped for. Every discontinuity of the operators is kept at a distance of 1e-4 (checked in float64 on the
float32 values, by nudging the offending input at generation time and asserting at the end), or sits exactly on the stated
boundary value where float32 and float64 agree by construction:
  | |p| - 1 |, | |p| - 1.2 |      sample position against the unit / relaxed sphere (exact rows: |p| == 1.0, == float32(1.2))
  |true_cos|, |true_cos - 1|      the two ReLUs of iter_cos (exact: the zero normal, true_cos == 0)
  |raw alpha|                     the clip at 0, wherever it can be reached at all: prev_cdf < next_cdf, i.e. a negative section
                                  length. With dists >= 0 the sigmoid's monotonicity gives p >= 0 and raw >= 1e-5 / (1 + 1e-5) in
                                  any precision, so no margin is needed (or possible: raw IS ~1e-5 wherever iter_cos == 0).
  |color - true_rgb|, |d_feats - gt_feats|      sign() of the L1 terms (exact rows in the loss cases: color == true_rgb)
  |weight_sum - 1e-3|, |weight_sum - (1 - 1e-3)|    the BCE clip gate
"""
import zlib

import numpy as np
import torch

from . import ray_ops

MARGIN = 1e-4
SHAPES = [(1, 1, 1), (3, 5, 6), (5, 64, 64), (7, 63, 95), (4, 128, 160), (130, 128, 160), (9, 130, 162), (2, 192, 256), (3, 256, 256)]
FEAT_CH = [0, 1, 64, 65, 96, 128]
WELL_CONDITIONED = ("smooth", "clip_hi", "clip_lo", "gates", "alpha_clip", "spheres", "background", "eikonal")
ILL_CONDITIONED = ("sharp", "saturated", "deep")

# regime -> (variance, the shapes it runs on)
REGIMES = {
    "smooth": (0.3, SHAPES),
    "sharp": (0.65, [(3, 5, 6), (4, 128, 160), (3, 256, 256)]),
    "clip_hi": (1.5, [(5, 64, 64), (7, 63, 95), (2, 192, 256)]),
    "clip_lo": (-1.5, [(1, 1, 1), (9, 130, 162), (4, 128, 160)]),
    "saturated": (0.3, [(3, 5, 6), (130, 128, 160), (2, 192, 256)]),
    "deep": (0.3, [(5, 64, 64), (7, 63, 95), (4, 128, 160)]),
    "gates": (0.3, [(7, 63, 95), (4, 128, 160), (9, 130, 162), (3, 256, 256), (5, 64, 64), (130, 128, 160)]),
    "alpha_clip": (0.3, [(3, 5, 6), (9, 130, 162), (2, 192, 256)]),
    "spheres": (0.3, [(3, 5, 6), (7, 63, 95), (4, 128, 160), (3, 256, 256)]),
    "background": (0.3, [(3, 5, 6), (5, 64, 64), (4, 128, 160), (2, 192, 256), (3, 256, 256)]),
    "eikonal": (0.3, [(3, 5, 6), (7, 63, 95), (130, 128, 160)]),
}
_GATE_CAR = [(0.0, False), (0.5, True), (1.0, False), (0.0, True), (0.5, False), (1.0, True)]     # (cos_anneal, through the device scalar)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def composite_case_names():
    names, k = [], 0
    for regime, (_, shapes) in REGIMES.items():
        for j, (B, N, T) in enumerate(shapes):
            names.append("%s-B%dN%dT%d-C%d-%d" % (regime, B, N, T, FEAT_CH[k % len(FEAT_CH)], j))
            k += 1
    return names


def _parse(name):
    regime, shape, c, j = name.split("-")
    B, rest = shape[1:].split("N")
    N, T = rest.split("T")
    return regime, int(B), int(N), int(T), int(c[1:]), int(j)


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def composite_case(name):
    """-> dict: the inputs of VdnCompositeArgs / VdnCompositeBwdArgs (float32), upstream gradients, targets of the fused loss."""
    regime, B, N, T, C, j = _parse(name)
    rs = _rng(name)
    variance = REGIMES[regime][0]
    k_all = composite_case_names().index(name)
    car, use_dev = [(0.5, False), (0.0, True), (1.0, False)][k_all % 3]
    if regime == "gates":
        car, use_dev = _GATE_CAR[j]
    # the background pass: always with outside samples; with T == N only where the regime asks for the blend alone
    has_bg = T > N or (regime == "background" and (B, N, T) == (3, 256, 256))
    inv_s = float(np.clip(np.exp(np.float64(np.float32(variance)) * 10.0), 1e-6, 1e6))
    unit = np.exp(3.0) / inv_s                     # lengths are laid out for inv_s = e^3 (variance 0.3) and scaled to the case's

    # ---- rays: |o + d t|^2 = |b|^2 + (t - c)^2 with b the foot of the perpendicular: all three sphere zones on every ray
    d = _unit(rs.standard_normal((B, 3)))
    perp = _unit(np.cross(d, rs.standard_normal((B, 3))))
    c = rs.uniform(1.5, 2.5, (B, 1))
    o = perp * rs.uniform(0.0, 0.6, (B, 1)) - d * c
    mid = np.sort(rs.uniform(c - 1.7, c + 1.7, (B, N)), -1)
    exact_pn = np.zeros((B, N), bool)
    if regime == "spheres":                        # ray 0: o = 0, d = e_x, |p| = mid_z: exactly 1.0 and exactly float32(1.2)
        o[0], d[0] = 0.0, (1.0, 0.0, 0.0)
        mid[0] = np.sort(rs.uniform(0.05, 1.6, N))
        mid[0, N // 3], mid[0, (2 * N) // 3] = 1.0, np.float32(1.2)
        exact_pn[0, N // 3] = exact_pn[0, (2 * N) // 3] = True
    o, d, mid = _f32(o), _f32(d), _f32(mid)
    for _ in range(100):
        pn = np.linalg.norm(o[:, None, :].astype(np.float64) + d[:, None, :].astype(np.float64) * mid[..., None].astype(np.float64), axis=-1)
        bad = ((np.abs(pn - 1.0) < 2 * MARGIN) | (np.abs(pn - 1.2) < 2 * MARGIN)) & ~exact_pn
        if not bad.any():
            break
        mid = np.where(bad, mid + np.float32(1e-3), mid).astype(np.float32)

    # ---- section lengths
    dists = rs.uniform(0.5, 1.5, (B, N)) * 0.1 * unit
    if regime == "sharp":                          # real section lengths at inv_s = 665: dist * inv_s / 2 ~ 9 at N = 128
        dists = rs.uniform(0.5, 1.5, (B, N)) * min(3.4 / N, 0.03)
    neg = np.zeros((B, N), bool)
    if regime == "alpha_clip":                     # (not reachable from sorted depths: the operator's contract, renderer.py:282)
        neg = rs.uniform(size=(B, N)) < 0.12
        neg[:, N // 2] = True
        dists = np.where(neg, -dists, dists)

    # ---- normals: true_cos = d . n placed in (-inf, 0), (0, 1) or (1, inf)
    cls = rs.choice(3, size=(B, N), p=[0.5, 0.3, 0.2])
    tc = np.where(cls == 0, -rs.uniform(0.05, 1.3, (B, N)), np.where(cls == 1, rs.uniform(0.05, 0.95, (B, N)), rs.uniform(1.05, 1.8, (B, N))))
    if regime == "alpha_clip":
        tc = np.where(neg, -rs.uniform(0.5, 1.0, (B, N)), tc)      # a clipped alpha needs iter_cos well away from zero
    dd = d.astype(np.float64)[:, None, :]
    side = _unit(np.cross(np.broadcast_to(dd, (B, N, 3)), rs.standard_normal((B, N, 3))))
    lat = np.where(np.abs(tc) < 1.0, np.sqrt(np.maximum(1.0 - tc ** 2, 0.0)) * rs.uniform(0.8, 1.2, (B, N)), rs.uniform(0.0, 0.5, (B, N)))
    normals = tc[..., None] * dd + lat[..., None] * side
    special = np.zeros((B, N), bool)
    if regime == "eikonal":
        normals[0, 0], special[0, 0] = 0.0, True   # the gn > 0 guard; true_cos == 0 exactly
        for r in range(B):
            for i in range(1, min(N, 4)):          # length exactly 1
                normals[r, i] = np.eye(3)[(r + i) % 3] * (1.0 if (r + i) % 2 else -1.0)
    sat = np.zeros((B, N), bool)
    half = np.zeros((B, N))
    if regime == "saturated":                      # 1, 2, 3 samples per ray with prev_cdf ~ 1 and next_cdf ~ 0
        for r in range(B):
            ns = min(1 + r % 3, N)
            for q in range(ns):
                i = (N * (q + 1)) // (ns + 1)
                sat[r, i], half[r, i] = True, (100.0, 14.0, 9.0)[q]
                normals[r, i] = -dd[r, 0]          # iter_cos = -1 for every cos_anneal
    normals = _f32(normals)
    for _ in range(100):
        tcv = (dd * normals.astype(np.float64)).sum(-1)
        bad = ((np.abs(tcv) < 2 * MARGIN) | (np.abs(tcv - 1.0) < 2 * MARGIN)) & ~special
        if not bad.any():
            break
        normals = np.where(bad[..., None], normals + (np.float32(1e-3) * d)[:, None, :], normals).astype(np.float32)

    # ---- sdf
    frac = (np.arange(N) / max(N - 1, 1))[None, :] if N > 1 else np.full((1, 1), 0.5)
    sdf = (0.25 - 0.45 * frac + 0.02 * rs.standard_normal((B, N))) * unit
    if regime == "sharp":                          # a surface crossed inside the ray at real scale: |sdf| * inv_s up to ~1000
        t0 = mid.astype(np.float64)[:, N // 2:N // 2 + 1] + rs.uniform(-0.005, 0.005, (B, 1))     # (a sample within reach of it)
        sdf = rs.uniform(0.5, 1.0, (B, 1)) * (t0 - mid.astype(np.float64))
    if regime == "deep":                           # sdf * inv_s in [-30, -12] on a quarter of the samples: p, c ~ 1e-6 .. 1e-13
        deep = rs.uniform(size=(B, N)) < 0.25
        sdf = np.where(deep, -rs.uniform(12.0, 30.0, (B, N)) / inv_s, sdf)
    if regime == "saturated":
        sdf = np.where(sat, 0.0, sdf)
        dists = np.where(sat, 2.0 * half / inv_s, dists)
    sdf, dists = _f32(sdf), _f32(dists)

    case = {"name": name, "regime": regime, "B": B, "N": N, "T": T, "C": C, "variance": np.float32(variance),
            "cos_anneal": car, "cos_anneal_by_value": 0.77 if use_dev else car, "use_dev": use_dev,
            "rays_o": o, "rays_d": d, "sdf": sdf, "normals": normals.reshape(B * N, 3), "dists": dists, "mid_z": mid,
            "color": _f32(rs.uniform(0.0, 1.0, (B, N, 3))), "feat": _f32(rs.standard_normal((B, N, C))) if C else None,
            "background_rgb": _f32(rs.uniform(0.5, 1.0, 3)) if k_all % 3 != 2 else None,
            "bg_density": None, "bg_rgb": None, "bg_feat": None, "bg_dists": None,
            "neg_dists": neg, "saturated": sat, "exact_pn": exact_pn}
    if has_bg:                                     # raw densities in the three softplus regimes: < -30, ~0, > 20
        kind = rs.choice(3, size=(B, T), p=[0.3, 0.5, 0.2])
        rho = np.where(kind == 0, rs.uniform(-40.0, -31.0, (B, T)), np.where(kind == 1, rs.uniform(-1.5, 1.5, (B, T)), rs.uniform(20.5, 30.0, (B, T))))
        case.update({"bg_density": _f32(rho), "bg_rgb": _f32(rs.uniform(0.0, 1.0, (B, T, 3))),
                     "bg_feat": _f32(rs.standard_normal((B, T, C))) if C else None,
                     "bg_dists": _f32(rs.uniform(0.5, 1.5, (B, T)) * 0.05)})
    # upstream gradients of the adjoint
    case.update({"g_color": _f32(rs.standard_normal((B, 3))), "g_feat": _f32(rs.standard_normal((B, C)) / np.sqrt(C)) if C else None,
                 "g_weights": _f32(rs.standard_normal((B, T))), "g_cdf": _f32(0.1 * rs.standard_normal((B, N))),
                 "g_eik": _f32([0.1])})
    # targets of the fused loss launches, kept away from the model's own colour / features (sign() of the L1 terms)
    with torch.no_grad():
        out = ray_ops.CompositeModel(case).out
    true_rgb, col = rs.uniform(0.0, 1.0, (B, 3)), out["color"].numpy()
    true_rgb = _f32(np.where(np.abs(_f32(true_rgb) - col) < 2 * MARGIN, true_rgb + 1e-3, true_rgb))
    case["true_rgb"] = true_rgb
    if C:
        gt, ft = rs.standard_normal((B, C)), out["d_feats"].numpy()
        case["gt_feats"] = _f32(np.where(np.abs(_f32(gt) - ft) < 2 * MARGIN, gt + 1e-3, gt))
    else:
        case["gt_feats"] = None
    return case


# ---- vdn_loss_fwd_bwd -------------------------------------------------------------------------------------------------------
#            B     T    C     mask     mask_weight grad_scale
LOSS_CASES = {"loss-B1": (1, 6, None, None, 0.0, 1.0),
              "loss-B1023": (1023, 6, 1, "binary", 0.3, 1.0),
              "loss-B1024": (1024, 160, 96, "fractional", 0.3, 0.5),
              "loss-B1025": (1025, 6, None, None, 0.3, 1.0),
              "loss-B5000a": (5000, 6, 96, "binary", 0.0, 0.5),
              "loss-B5000b": (5000, 32, 1, "fractional", 0.3, 1.0)}


def loss_case(name):
    B, T, C, mask_kind, mask_weight, grad_scale = LOSS_CASES[name]
    rs = _rng(name)
    true_rgb = _f32(rs.uniform(0.0, 1.0, (B, 3)))
    diff = rs.uniform(2 * MARGIN, 0.3, (B, 3)) * rs.choice([-1.0, 1.0], size=(B, 3))
    same = rs.uniform(size=(B, 1)) < 0.1                          # rays with color == true_rgb exactly: sign(0)
    same[0] = B > 1
    color = np.where(same, true_rgb, _f32(true_rgb.astype(np.float64) + diff)).astype(np.float32)
    # weight_sum below 1e-3, inside the clip, above 1 - 1e-3 (a third of the rays each), 1e-4 away from both gates
    zone = np.arange(B) % 3 if B > 1 else np.array([1])
    rs.shuffle(zone)
    # (inside the clip: mostly mid-range, and some within 1e-3 of either gate, so that a gate moved by as little as that shows)
    near = rs.uniform(size=B)
    mid_ws = np.where(near < 0.7, rs.uniform(0.01, 0.99, B), np.where(near < 0.85, rs.uniform(0.9981, 0.99885, B), rs.uniform(1.15e-3, 2e-3, B)))
    ws = np.where(zone == 0, rs.uniform(1e-5, 8e-4, B), np.where(zone == 1, mid_ws, rs.uniform(0.9993, 1.0005, B)))
    share = rs.uniform(0.1, 1.0, (B, T))
    weights = _f32(share / share.sum(-1, keepdims=True) * ws[:, None])
    wsum = weights.astype(np.float64).sum(-1)
    assert (np.abs(wsum - 1e-3) > MARGIN).all() and (np.abs(wsum - (1.0 - 1e-3)) > MARGIN).all()
    mask = None
    if mask_kind == "binary":
        mask = _f32(rs.uniform(size=B) < 0.6)
    elif mask_kind == "fractional":
        mask = _f32(rs.uniform(0.05, 0.95, B))
    case = {"name": name, "B": B, "T": T, "C": C or 0, "color": color, "true_rgb": true_rgb, "mask": mask, "weights": weights,
            "eik": _f32([0.0371, 12.5, 337.0]), "igr_weight": 0.1, "mask_weight": mask_weight, "depth_weight": 0.7,
            "grad_scale": grad_scale, "feats": None, "gt_feats": None, "same_rows": same[:, 0], "zone": zone}
    if C:
        gt = _f32(rs.standard_normal((B, C)))
        d = rs.uniform(2 * MARGIN, 1.0, (B, C)) * rs.choice([-1.0, 1.0], size=(B, C))
        case["gt_feats"], case["feats"] = gt, _f32(gt.astype(np.float64) + d)
    return case


# ---- vdn_ray_adjoint ----------------------------------------------------------------------------------------------------------
RAY_ADJOINT_CASES = {"rayadj-B1N1T1": (1, 1, 1), "rayadj-B3N5T6": (3, 5, 6), "rayadj-B5N64T64": (5, 64, 64), "rayadj-B7N63T95": (7, 63, 95),
                     "rayadj-B130N128T160": (130, 128, 160), "rayadj-B9N130T162": (9, 130, 162), "rayadj-B2N192T256": (2, 192, 256),
                     "rayadj-B3N256T256": (3, 256, 256)}


def ray_adjoint_case(name):
    B, N, T = RAY_ADJOINT_CASES[name]
    rs = _rng(name)
    z = _f32(np.sort(rs.uniform(0.5, 3.5, (B, N)), -1))
    z_out = _f32(np.sort(rs.uniform(3.6, 60.0, (B, T - N)), -1)) if T > N else None
    n = lambda *s: _f32(rs.standard_normal(s))
    case = {"name": name, "B": B, "N": N, "T": T, "sample_dist": float(np.float32(2.0 / 64)), "rays_o": n(B, 3), "rays_d": _f32(_unit(rs.standard_normal((B, 3)))),
            "z": z, "z_out": z_out, "d_pts": n(B, N, 3), "d_dirs": n(B, N, 3), "d_dists": n(B, N), "d_dir_cos": n(B, 3),
            "d_bg_pts": n(B, T, 3) if T > N else None, "d_bg_dirs": n(B, T, 3) if T > N else None, "d_bg_dists": n(B, T) if T > N else None}
    return case


# ---- vdn_sections / vdn_coarse_z ----------------------------------------------------------------------------------------------
def sections_case(name, B, n, ld):
    rs = _rng(name)
    z = np.full((B, ld), np.nan, np.float32)
    z[:, :n] = _f32(np.sort(rs.uniform(0.3, 6.0, (B, n)), -1))
    return {"name": name, "B": B, "n": n, "ld": ld, "z": z, "sample_dist": float(np.float32(2.0 / 64))}


def coarse_case(name, B, n_samples, n_outside, jitter_in, jitter_out):
    rs = _rng(name)
    near = _f32(rs.uniform(0.2, 2.0, (B, 1)))
    far = _f32(near + rs.uniform(1.5, 2.5, (B, 1)))
    lin = torch.linspace(0.0, 1.0, n_samples).numpy()
    case = {"name": name, "B": B, "n_samples": n_samples, "n_outside": n_outside, "near": near, "far": far, "lin_samples": lin,
            "lin_outside": None, "out_lower": None, "out_upper": None,
            "t_rand": _f32(rs.uniform(size=(B, 1))) if jitter_in else None, "t_rand_out": None}
    if n_outside > 0:
        zo = torch.linspace(1e-3, 1.0 - 1.0 / (n_outside + 1.0), n_outside)
        mids = 0.5 * (zo[1:] + zo[:-1])
        case.update({"lin_outside": zo.numpy(), "out_upper": torch.cat([mids, zo[-1:]], -1).numpy(),
                     "out_lower": torch.cat([zo[:1], mids], -1).numpy(),
                     "t_rand_out": _f32(rs.uniform(size=(B, n_outside))) if jitter_out else None})
    return case
