"""The hierarchical sampler as functions of plain tensors (torch, CPU, any float dtype), stage by stage.

`upsample_stages` is one up-sampling round (VdnUpsampleArgs: renderer.py:147-191 with sample_pdf, 44-74, det=True) and returns every
intermediate the kernel's branches depend on; `merge` is cat_z_vals' sort (VdnMergeArgs: renderer.py:197-205). The round is the
line-cited neus_oracle.up_sample / sample_pdf_det operation for operation (tests/test_sampler_model_cpu.py asserts element-for-
element equality in float32 and float64), with `u` a parameter, as it is for the kernel, so that a case can put it exactly on a
CDF knot.

What the tests judge a kernel by lives here too, computed from the float64 model alone: `classify` (which entries sit so close to
a discontinuity - a CDF knot, the denom < 1e-5 threshold - that either side is a legitimate rounding, and the values either side
gives), `cdf_residual` (|CDF64(z) - u|, the quantity that stays well-conditioned where depths do not) and `judge`, the comparator
shared by the CPU test (which feeds it the float32 model with seeded defects) and tests/test_gpu_sampler.py (which feeds it the
kernels' output).
"""
import numpy as np
import torch

from .ray_ops import excl_cumprod_weights

FLAT = 1e-5            # renderer.py:70: denom < 1e-5 -> 1
DEFECTS = ("search_left", "no_trans_eps", "prev_cos_wraps", "inside_and", "no_lower_clip", "no_flat_threshold", "no_weight_eps",
           "no_alpha_eps", "last_interval", "inv_s_next_round", "inv_s_prev_round")
MERGE_DEFECTS = ("new_before_equal_old",)


def _interp(z, cdf, u, inds, flat=None):
    """renderer.py:64-73 from the search result `inds` on. flat: None = the reference's rule, True / False = that branch forced."""
    M = cdf.shape[-1]
    below = (inds - 1).clamp(min=0, max=M - 1)
    above = inds.clamp(min=0, max=M - 1)
    cdf_b, cdf_a = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bin_b, bin_a = torch.gather(z, 1, below), torch.gather(z, 1, above)
    denom = cdf_a - cdf_b
    is_flat = denom < FLAT if flat is None else torch.full_like(denom, bool(flat), dtype=torch.bool)
    den = torch.where(is_flat, torch.ones_like(denom), denom)
    t = (u - cdf_b) / den
    return {"below": below, "above": above, "denom": denom, "flat": is_flat, "t": t, "new_z": bin_b + t * (bin_a - bin_b)}


def upsample_stages(rays_o, rays_d, z, sdf, u, inv_s, weights=None, defect=None):
    """One round on z [B,M] (sorted), sdf [B,M], u [n_imp] -> dict of stages; weights [B,M-1] given = sample_pdf alone (rays_o,
    rays_d, sdf may then be None). `defect` (one of DEFECTS) seeds one deviation a wrong kernel could have: the yardstick test's
    stand-in for such a kernel, never used otherwise."""
    assert defect is None or defect in DEFECTS
    B, M = z.shape
    dt = z.dtype
    st = {}
    if defect == "last_interval":      # i < M for i < M - 1: the kernel would read one element past the row, which the tests keep NaN
        nan = torch.full((B, 1), float("nan"), dtype=dt)
        z = torch.cat([z, nan], -1)
        sdf = None if sdf is None else torch.cat([sdf, nan], -1)
        weights = None if weights is None else torch.cat([weights, nan], -1)
    if weights is None:
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., :, None]
        radius = torch.linalg.norm(pts, ord=2, dim=-1)
        r0, r1 = radius[:, :-1] < 1.0, radius[:, 1:] < 1.0
        inside = (r0 & r1) if defect == "inside_and" else (r0 | r1)                  # renderer.py:153-154
        prev_sdf, next_sdf = sdf[:, :-1], sdf[:, 1:]
        prev_z, next_z = z[:, :-1], z[:, 1:]
        mid_sdf = (prev_sdf + next_sdf) * 0.5
        raw_cos = (next_sdf - prev_sdf) / (next_z - prev_z + 1e-5)                    # renderer.py:159
        first = raw_cos[:, -1:] if defect == "prev_cos_wraps" else torch.zeros(B, 1, dtype=dt)
        prev_cos = torch.cat([first, raw_cos[:, :-1]], -1)
        min_cos = torch.minimum(prev_cos, raw_cos)                                    # renderer.py:176-178
        clipped = min_cos.clip(max=0.0) if defect == "no_lower_clip" else min_cos.clip(-1e3, 0.0)
        cos_val = clipped * inside                                                    # renderer.py:179
        dist = next_z - prev_z
        s = inv_s * 2.0 if defect == "inv_s_next_round" else inv_s * 0.5 if defect == "inv_s_prev_round" else inv_s
        prev_cdf = torch.sigmoid((mid_sdf - cos_val * dist * 0.5) * s)
        next_cdf = torch.sigmoid((mid_sdf + cos_val * dist * 0.5) * s)
        if defect == "no_alpha_eps":
            alpha = (prev_cdf - next_cdf) / prev_cdf
        else:
            alpha = (prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)                  # renderer.py:186
        if defect == "no_trans_eps":
            one = torch.ones(B, 1, dtype=dt)
            trans = torch.cumprod(torch.cat([one, 1.0 - alpha], -1), -1)[:, :-1]
            w = alpha * trans
        else:
            w = excl_cumprod_weights(alpha)                                           # renderer.py:187-188
            trans = torch.cumprod(torch.cat([torch.ones(B, 1, dtype=dt), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
        st.update({"radius": radius, "inside": inside, "raw_cos": raw_cos, "prev_cos": prev_cos, "min_cos": min_cos, "cos": cos_val,
                   "prev_cdf": prev_cdf, "next_cdf": next_cdf, "alpha": alpha, "trans": trans})
    else:
        w = weights
    st["weights"] = w
    wp = w if defect == "no_weight_eps" else w + 1e-5                                 # renderer.py:46
    pdf = wp / wp.sum(-1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    uu = u.to(dt).expand(B, u.shape[0]).contiguous()
    inds = torch.searchsorted(cdf, uu, right=(defect != "search_left"))               # renderer.py:61
    st.update({"pdf": pdf, "cdf": cdf, "u": uu, "inds": inds, "z": z})
    st.update(_interp(z, cdf, uu, inds, False if defect == "no_flat_threshold" else None))
    return st


def merge(z, sdf, new_z, new_sdf, defect=None):
    """cat + stable sort + gather (renderer.py:197-205): old elements come before equal new ones. -> (z [B,M+K], sdf or None)."""
    assert defect is None or defect in MERGE_DEFECTS
    M = z.shape[1]
    if defect == "new_before_equal_old":
        zc, idx = torch.sort(torch.cat([new_z, z], -1), dim=-1, stable=True)
        sc = None if sdf is None else torch.gather(torch.cat([new_sdf, sdf], -1), 1, idx)
        return zc, sc
    zc, idx = torch.sort(torch.cat([z, new_z], -1), dim=-1, stable=True)
    sc = None if sdf is None else torch.gather(torch.cat([sdf, new_sdf], -1), 1, idx)
    return zc, sc


def merge_takes_counting_path(z):
    """The rows of z [B,M] that are not sorted: the kernel ranks those by counting instead of by index / binary search."""
    return (z[:, 1:] < z[:, :-1]).any(-1)


def classify(st64, tau, exact_knots=False):
    """-> (sensitive [B,n] bool, candidates [B,n,6]). An entry is branch-sensitive if its u lies within tau of a CDF knot or
    |denom - 1e-5| <= 2 tau: a legitimate float32 rounding may then search into the neighbouring bin, or take the other side of the
    flat threshold. The candidates are the same formula in the bins inds-1, inds, inds+1, each with the threshold's rule and with
    the other side forced (NaN where that would divide by zero). exact_knots: a u EXACTLY on a knot is not sensitive (the case
    promises knots that are exact in every precision: searchsorted(right=True) then decides, and t == 0)."""
    cdf, u, inds, z = st64["cdf"], st64["u"], st64["inds"], st64["z"]
    M = cdf.shape[-1]
    dist = (u[:, :, None] - cdf[:, None, :]).abs()
    if exact_knots:
        dist = torch.where(dist == 0.0, torch.full_like(dist, float("inf")), dist)
    near_knot = dist.min(-1)[0] <= tau
    near_flat = (st64["denom"] - FLAT).abs() <= 2.0 * tau
    cands = []
    for shift in (-1, 0, 1):
        ii = (inds + shift).clamp(0, M)
        rule = _interp(z, cdf, u, ii, None)
        other_flat = _interp(z, cdf, u, ii, True)["new_z"]
        other_lin = _interp(z, cdf, u, ii, False)["new_z"]
        cands.append(rule["new_z"])
        cands.append(torch.where(rule["flat"], other_lin, other_flat))
    cand = torch.stack(cands, -1)
    cand = torch.where(torch.isfinite(cand), cand, torch.full_like(cand, float("nan")))
    return near_knot | near_flat, cand


def cdf_residual(st64, z_got):
    """|CDF64(z_got) - u| on the piecewise-linear float64 CDF through (z[k], cdf[k]); where z_got equals one or more (tied) knots
    the CDF there is the whole interval of their values and the residual is the distance to it. inf outside [z[0], z[M-1]]."""
    z, cdf, u = st64["z"], st64["cdf"], st64["u"]
    B, M = z.shape
    zg = z_got.to(z.dtype).contiguous()
    lo = torch.searchsorted(z.contiguous(), zg, right=False)       # first idx with z[idx] >= zg
    hi = torch.searchsorted(z.contiguous(), zg, right=True)        # first idx with z[idx] >  zg
    g = lambda t, i: torch.gather(t, 1, i.clamp(0, M - 1))
    z0, z1, c0, c1 = g(z, lo - 1), g(z, lo), g(cdf, lo - 1), g(cdf, lo)
    between = c0 + (c1 - c0) * (zg - z0) / torch.where(z1 > z0, z1 - z0, torch.ones_like(z0))
    on_knot = hi > lo
    c_lo = torch.where(on_knot, g(cdf, lo), between)
    c_hi = torch.where(on_knot, g(cdf, hi - 1), between)
    res = torch.maximum(torch.maximum(c_lo - u, u - c_hi), torch.zeros_like(u))
    outside = (~on_knot & ((lo == 0) | (lo >= M))) | ~torch.isfinite(zg)
    return torch.where(outside, torch.full_like(res, float("inf")), res)


def floors(st64, st32):
    """F_z = max|z32 - z64|, F_cdf = max|cdf32 - cdf64|: what plain float32 arithmetic of the same formulas costs (the reference
    against itself; never measured from a kernel)."""
    return (float((st32["new_z"].double() - st64["new_z"]).abs().max()), float((st32["cdf"].double() - st64["cdf"]).abs().max()))


def judge(case, st64, st32, z_got):
    """The comparator. case: dict with "cls" ("tight" / "ill") and optionally "exact_knots"; z_got [B,n] (any float dtype).
    -> dict(ok, worst = the worst error in units of its bound, n_sensitive, n_by_candidate, F_z, F_cdf, why).

    tight: every entry |z - z64| <= max(U, 3 F_z), U = 1e-6 max(1, max|z|); an entry whose u is exactly on an exact knot
    (exact_knots) has t == 0 and must equal z[below] bit for bit. ill: every entry cdf_residual <= 3 F_cdf (+ 1e-5 where the model
    took the flat branch); the new depths ascend within each ray and lie within [z[0], z[M-1]]. A branch-sensitive entry (tau =
    10 F_cdf tight, 3 F_cdf ill) may instead match one of its candidates to max(U, 3 F_z). Nothing is excluded: NaN fails."""
    F_z, F_cdf = floors(st64, st32)
    got = z_got.double()
    z64 = st64["new_z"]
    zin = st64["z"]
    U = 1e-6 * max(1.0, float(zin.abs().max()))
    bz = max(U, 3.0 * F_z)
    tight = case["cls"] == "tight"
    sens, cand = classify(st64, (10.0 if tight else 3.0) * F_cdf, bool(case.get("exact_knots")))
    by_cand = sens & (((got[:, :, None] - cand).abs() <= bz).any(-1))
    why = []
    if tight:
        units = (got - z64).abs() / bz
        if case.get("exact_knots"):
            on = (st64["t"] == 0.0) & ~sens
            exact_ok = got == torch.gather(zin, 1, st64["below"])
            units = torch.where(on, torch.where(exact_ok, torch.zeros_like(units), torch.full_like(units, float("inf"))), units)
    else:
        bc = 3.0 * F_cdf + torch.where(st64["flat"], torch.full_like(z64, FLAT), torch.zeros_like(z64))
        units = cdf_residual(st64, got) / bc
        M = zin.shape[1]
        if not bool((got[:, 1:] >= got[:, :-1]).all()):
            why.append("new depths do not ascend")
        if not bool(((got >= zin[:, :1]) & (got <= zin[:, M - 1:M])).all()):
            why.append("new depths leave [z[0], z[M-1]]")
    units = torch.where(torch.isfinite(got), units, torch.full_like(units, float("inf")))
    fails = ~((units <= 1.0) | by_cand)
    if bool(fails.any()):
        b, j = [int(x) for x in torch.nonzero(fails)[0]]
        why.append("%d entries beyond the bound, first [%d,%d]: got %r, model %r, %.3g units" %
                   (int(fails.sum()), b, j, float(got[b, j]), float(z64[b, j]), float(units[b, j])))
    judged = torch.where(by_cand & ~(units <= 1.0), torch.zeros_like(units), units)
    return {"ok": not why, "worst": float(judged.max()), "n_sensitive": int(sens.sum()), "n_by_candidate": int((by_cand & ~(units <= 1.0)).sum()),
            "F_z": F_z, "F_cdf": F_cdf, "bound_z": bz, "why": "; ".join(why)}


def stages_of(case, dtype, defect=None, z=None, sdf=None):
    """upsample_stages of a case dict (oracle/sampler_cases.py: float32 numpy arrays) in `dtype`; z / sdf override the case's rows
    (the GPU test feeds the kernel's own merged rows and SDF values)."""
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    M = case["M"]
    zz = t(case["z"] if z is None else z)[:, :M]
    sd = case.get("sdf") if sdf is None else sdf
    w = case.get("weights")
    return upsample_stages(t(case.get("rays_o")), t(case.get("rays_d")), zz, None if sd is None else t(sd)[:, :M], t(case["u"]),
                           float(case["inv_s"]), None if w is None else t(w)[:, :M - 1], defect=defect)
