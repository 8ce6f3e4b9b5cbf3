"""The float64 model of the per-ray kernels (oracle/ray_ops.py) and its constructed inputs (oracle/ray_cases.py), without a GPU:
the proof that tests/test_gpu_ray_ops.py tests what it claims.

* coverage: every regime reaches the branches it is named for (counted over the regime's cases, from the float64 model alone),
  and every discontinuity is either exactly on its boundary value or further than 1e-4 from it;
* conditioning: the same model in float32 against float64, per output tensor, in units of conftest.relelem's bound (the tensor's
  "fp32 floor"). Outside the sharp / saturated / deep-inside regimes every floor is <= 1: plain float32 meets the project's 1e-4
  criterion there, so the GPU test's bound max(1, 3 x floor) is at most 3 units;
* the refactor of neus_oracle.render_core onto ray_ops.composite: bit-identical to the previous body, which is kept here as
  `_render_core_before` (two golden fixtures, float32 and float64).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.neus_oracle as orc
from oracle import ray_cases, ray_ops
from vdn_train import synth
from conftest import relelem

NAMES = ray_cases.composite_case_names()
M = ray_cases.MARGIN


@pytest.fixture(scope="module")
def models():
    out = {}
    for name in NAMES:
        case = ray_cases.composite_case(name)
        out[name] = (case, ray_ops.CompositeModel(case, torch.float64), ray_ops.CompositeModel(case, torch.float32))
    return out


def test_case_matrix_covers_the_shapes_and_channel_counts():
    shapes = {ray_cases._parse(n)[1:4] for n in NAMES}
    assert shapes == set(ray_cases.SHAPES)
    assert {ray_cases._parse(n)[4] for n in NAMES} == set(ray_cases.FEAT_CH)
    assert {ray_cases._parse(n)[0] for n in NAMES} == set(ray_cases.WELL_CONDITIONED + ray_cases.ILL_CONDITIONED)
    a, b = ray_cases.composite_case(NAMES[3]), ray_cases.composite_case(NAMES[3])
    assert all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))          # deterministic from the name


def test_margins_hold_in_every_case(models):
    for name, (case, m64, _) in models.items():
        o = m64.out
        pn, tc, raw, p = (o[k].detach().numpy() for k in ("pts_norm", "true_cos", "raw_alpha", "p"))
        for edge in (1.0, 1.2):
            off = np.abs(pn - edge)
            on_it = ((pn == 1.0) | (pn == float(np.float32(1.2)))) & case["exact_pn"]     # exactly 1.0 / float32(1.2), the kernel's constant
            assert ((off > M) | on_it).all(), (name, "sphere", edge)
        zero_n = (case["normals"].reshape(pn.shape + (3,)) == 0.0).all(-1)
        assert ((np.abs(tc) > M) | (zero_n & (tc == 0.0))).all(), (name, "true_cos 0")
        assert (np.abs(tc - 1.0) > M).all(), (name, "true_cos 1")
        # the clip of alpha at 0 is reachable only where prev_cdf < next_cdf (ray_cases docstring); at 1 only with next_cdf == 0,
        # where raw == 1.0 exactly in both precisions and both sides pass the gradient
        assert (np.abs(raw[p < 0.0]) > M).all(), (name, "raw alpha")
        assert ((p >= 0.0) | case["neg_dists"]).all() and (raw <= 1.0).all(), name
        assert (np.abs(o["color"].detach().numpy() - case["true_rgb"]) > M).all(), (name, "color - true_rgb")
        if case["C"]:
            assert (np.abs(o["d_feats"].detach().numpy() - case["gt_feats"]) > M).all(), (name, "d_feats - gt_feats")


def _count(models, regime, fn):
    return sum(int(fn(c, m.out)) for n, (c, m, _) in models.items() if c["regime"] == regime)


def test_every_regime_reaches_its_branches(models):
    n = lambda t: t.detach().numpy()
    cnt = lambda regime, fn: _count(models, regime, fn)
    # smooth: alpha strictly inside (0, 1) on every inside sample
    assert cnt("smooth", lambda c, o: ((n(o["raw_alpha"]) > 0) & (n(o["raw_alpha"]) < 1)).all() and n(o["raw_alpha"]).size) >= 8
    # sharp: |est| * inv_s beyond the sigmoid's float32 saturation on both sides of a crossing inside the ray
    assert cnt("sharp", lambda c, o: (n(o["cdf"]) > 1 - 1e-7).sum()) >= 8 and cnt("sharp", lambda c, o: (n(o["cdf"]) < 1e-7).sum()) >= 8
    assert cnt("sharp", lambda c, o: ((n(o["cdf"]) > 0.01) & (n(o["cdf"]) < 0.99)).sum()) >= 8
    # the clipped inv_s, both ends; d_variance must then be exactly zero in the model too
    for regime, val in (("clip_hi", 1e6), ("clip_lo", 1e-6)):
        assert cnt(regime, lambda c, o: float(n(o["inv_s"]).max()) == val == float(n(o["inv_s"]).min())) >= 3
        for name, (case, m64, _) in models.items():
            if case["regime"] == regime:
                ad = m64.adjoints(**ray_ops.upstream_of(case))
                assert float(ad["d_var_partial"].abs().max()) == 0.0 and float(ad["d_var_abs"].abs().max()) == 0.0
                assert float(ad["d_sdf"].abs().max()) > 0.0
    # saturated: alpha == 1 exactly (f = 1e-7) and alpha within 1e-4 of 1; transmittance down to 1e-7 .. 1e-21 behind them
    assert cnt("saturated", lambda c, o: (n(o["alpha"])[:, :c["N"]][c["saturated"]] == 1.0).sum()) >= 8
    assert cnt("saturated", lambda c, o: ((n(o["alpha"])[:, :c["N"]][c["saturated"]] < 1.0) & (n(o["alpha"])[:, :c["N"]][c["saturated"]] > 1 - 1e-4)).sum()) >= 8
    tr = lambda o: n(o["weights"]) / np.maximum(n(o["alpha"]), 1e-300)
    assert cnt("saturated", lambda c, o: ((tr(o) < 1e-6) & (tr(o) > 1e-22) & (n(o["alpha"]) > 0)).sum()) >= 8
    # deep inside: p and c both below 1e-5, so raw -> 1e-5 / 1e-5 and the 1 / (c + 1e-5)^2 factor is ~1e10
    assert cnt("deep", lambda c, o: ((n(o["cdf"]) < 1e-6) & (np.abs(n(o["p"])) < 1e-6)).sum()) >= 8
    # cosine gates: each interval of true_cos with each cos_anneal, by value and through the device scalar
    for car in (0.0, 0.5, 1.0):
        for dev in (False, True):
            sel = [(c, m.out) for _, (c, m, _) in models.items() if c["regime"] == "gates" and c["cos_anneal"] == car and c["use_dev"] == dev]
            assert len(sel) == 1 and (not dev or sel[0][0]["cos_anneal_by_value"] != car)
            tc = n(sel[0][1]["true_cos"])
            assert (tc < 0).sum() >= 8 and ((tc > 0) & (tc < 1)).sum() >= 8 and (tc > 1).sum() >= 8
    # alpha clip: raw < 0 (clipped to 0, zero adjoint through it)
    assert cnt("alpha_clip", lambda c, o: (n(o["raw_alpha"]) < 0).sum()) >= 8
    # spheres: the three zones on one and the same ray, and the two exact boundaries (strict <: outside both)
    def zones(c, o):
        pn = n(o["pts_norm"])
        return (((pn < 1).sum(-1) >= 8) & (((pn >= 1) & (pn < 1.2)).sum(-1) >= 8) & ((pn >= 1.2).sum(-1) >= 8)).sum()
    assert cnt("spheres", zones) >= 8
    for edge, key in ((1.0, "inside_sphere"), (float(np.float32(1.2)), "relax_sphere")):
        assert cnt("spheres", lambda c, o: ((n(o["pts_norm"]) == edge) & (n(o[key]) == 0.0) & c["exact_pn"]).sum()) >= 1
    # background: the three softplus regimes, T - N in {0, 1, 32, 64}, no background at all with T == N
    for lo, hi in ((-1e9, -30.0), (-2.0, 2.0), (20.0, 1e9)):
        assert cnt("background", lambda c, o: 0 if c["bg_density"] is None else ((c["bg_density"] > lo) & (c["bg_density"] < hi)).sum()) >= 8
    bgc = [c for _, (c, _, _) in models.items() if c["regime"] == "background"]
    assert {c["T"] - c["N"] for c in bgc if c["bg_density"] is not None} == {0, 1, 32, 64}
    assert any(c["bg_density"] is None and c["T"] == c["N"] for c in bgc)
    # eikonal: a zero normal, normals of length exactly 1
    assert cnt("eikonal", lambda c, o: (np.abs(c["normals"]).sum(-1) == 0).sum()) >= 1
    assert cnt("eikonal", lambda c, o: (np.linalg.norm(c["normals"].astype(np.float64), axis=-1) == 1.0).sum()) >= 8


def test_autograd_of_the_norm_is_zero_at_the_zero_normal(models):
    """The kernel guards the eikonal term's adjoint with gn > 0; autograd of linalg.norm gives 0 at 0 as well - asserted, not assumed."""
    case, m64, m32 = models[[n for n in NAMES if n.startswith("eikonal")][0]]
    for m in (m64, m32):
        g = m.adjoints(g_eik=1.0)["d_normals"].reshape(case["B"], case["N"], 3)
        assert (case["normals"].reshape(case["B"], case["N"], 3)[0, 0] == 0).all()
        assert torch.isfinite(g).all() and (g[0, 0] == 0).all() and float(g.abs().max()) > 0


def fp32_floors(case, m64, m32):
    """-> {tensor: units of relelem's bound by which the float32 model misses the float64 one}, forward and full adjoint."""
    rows = {}
    f64, f32 = ray_ops.forward_arrays(m64), ray_ops.forward_arrays(m32)
    for k in f64:
        rows[k] = relelem(f32[k], f64[k])
    up = ray_ops.upstream_of(case)
    a64, a32 = ray_ops.adjoint_arrays(m64, **up), ray_ops.adjoint_arrays(m32, **up)
    for k in a64:
        if k == "d_var_abs":
            continue
        if k == "d_var_partial":
            rows[k] = ray_ops.var_units(a32[k], a64[k], a64["d_var_abs"])
        elif k == "d_variance":
            rows[k] = ray_ops.var_units(a32[k], a64[k], a64["d_var_abs"].sum())
        else:
            rows[k] = relelem(a32[k], a64[k])
    return rows


def test_fp32_floor_of_the_well_conditioned_regimes(models):
    worst, lines = 0.0, []
    for name, (case, m64, m32) in models.items():
        assert np.array_equal(m64.out["inside_sphere"].numpy(), m32.out["inside_sphere"].double().numpy()), name
        assert np.array_equal(m64.out["relax_sphere"].numpy(), m32.out["relax_sphere"].double().numpy()), name
        rows = fp32_floors(case, m64, m32)
        k = max(rows, key=rows.get)
        lines.append("%-34s worst fp32 floor %.3f (%s)" % (name, rows[k], k))
        if case["regime"] in ray_cases.WELL_CONDITIONED:
            worst = max(worst, rows[k])
            assert rows[k] <= 1.0, (name, k, rows[k])
        else:       # the comparison must not be empty: the float32 model within 10 % of each tensor's largest entry
            assert rows[k] < 0.1 / 1e-6, (name, k, rows[k])
    print("\n".join(lines))
    print("worst floor over the well-conditioned regimes: %.3f units" % worst)


# ---- loss / geometry / coarse cases ----------------------------------------------------------------------------------------

def test_loss_cases_reach_their_branches():
    seen_B, seen_C = set(), set()
    for name in ray_cases.LOSS_CASES:
        c = ray_cases.loss_case(name)
        seen_B.add(c["B"]); seen_C.add(c["C"])
        ws = c["weights"].astype(np.float64).sum(-1)
        d = c["color"].astype(np.float64) - c["true_rgb"]
        assert ((np.abs(d) > M) | ((d == 0) & c["same_rows"][:, None])).all(), name
        if c["B"] > 1:
            assert c["same_rows"].sum() >= 1 and (d[c["same_rows"]] == 0).all()
            assert (ws < 1e-3).sum() >= 8 and ((ws > 1e-3) & (ws < 1 - 1e-3)).sum() >= 8 and (ws > 1 - 1e-3).sum() >= 8
            # ... and inside the clip but within 1e-3 of either gate (a gate that is off by a factor of two must show)
            assert ((ws > 1e-3) & (ws < 2e-3)).sum() >= 8 and ((ws > 1 - 2e-3) & (ws < 1 - 1e-3)).sum() >= 8
        assert (np.abs(ws - 1e-3) > M).all() and (np.abs(ws - (1 - 1e-3)) > M).all()
        r64, r32 = ray_ops.loss_adjoints(c, torch.float64), ray_ops.loss_adjoints(c, torch.float32)
        for k in r64:
            a, b = r32[k].double().numpy(), r64[k].numpy()
            assert relelem(a, b) <= 1.0 if np.abs(b).max() > 0 else (a == 0).all(), (name, k)
        if c["mask_weight"] != 0:        # the BCE gate: zero outside the clip, non-zero inside
            gw = r64["g_weights"].numpy()
            inside = (ws > 1e-3) & (ws < 1 - 1e-3)
            assert (gw[~inside] == 0).all()
            if c["mask"] is None or c["name"] != "loss-B1":
                assert (gw[inside] != 0).any()
    assert seen_B == {1, 1023, 1024, 1025, 5000} and {1, 96} <= seen_C
    assert {ray_cases.LOSS_CASES[n][3] for n in ray_cases.LOSS_CASES} == {None, "binary", "fractional"}
    assert {ray_cases.LOSS_CASES[n][4] for n in ray_cases.LOSS_CASES} == {0.0, 0.3}
    assert {ray_cases.LOSS_CASES[n][5] for n in ray_cases.LOSS_CASES} == {1.0, 0.5}


def test_ray_geometry_and_coarse_z_models():
    for name in ray_cases.RAY_ADJOINT_CASES:
        c = ray_cases.ray_adjoint_case(name)
        r64, r32 = ray_ops.ray_geometry_adjoints(c, torch.float64), ray_ops.ray_geometry_adjoints(c, torch.float32)
        for k in ("d_rays_o", "d_rays_d", "d_z", "d_z_out"):
            if k in r64:
                assert relelem(r32[k].double().numpy(), r64[k].numpy()) <= 1.0, (name, k)
    # coarse_z restates neus_oracle.coarse_and_outside_z on vectors passed in: equal in float64 up to the float32 rounding of
    # the linspace vectors the kernel is given
    c = ray_cases.coarse_case("coarse-cpu", 5, 64, 32, True, True)
    t = lambda k: None if c[k] is None else torch.tensor(c[k]).double()
    z, zo = ray_ops.coarse_z(t("near"), t("far"), t("lin_samples"), t("lin_outside"), t("out_lower"), t("out_upper"), t("t_rand"), t("t_rand_out"))
    z2, zo2 = orc.coarse_and_outside_z(t("near"), t("far"), orc.RendererConf(), 1.0, t("t_rand"), t("t_rand_out"))
    assert float((z - z2).abs().max()) < 1e-6 and float(((zo - zo2).abs() / zo2.abs()).max()) < 1e-6


# ---- render_core before / after ---------------------------------------------------------------------------------------------

def _render_core_before(nets, rays_o, rays_d, z_vals, sample_dist, bg=None, background_rgb=None, cos_anneal_ratio=0.0):
    """neus_oracle.render_core as it stood before its compositor moved to ray_ops.composite (kept verbatim as the 'before')."""
    B, N = z_vals.shape
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dists = torch.cat([dists, torch.full_like(dists[..., :1], sample_dist)], -1)
    mid_z = z_vals + dists * 0.5
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * mid_z[..., :, None]).reshape(-1, 3)
    dirs = rays_d[:, None, :].expand(B, N, 3).reshape(-1, 3)
    out, gradients = orc.sdf_forward(nets.sdf, pts, nets.sdf_conf, with_gradient=True)
    sdf, feature = out[:, :1], out[:, 1:]
    sampled_feat = None
    if nets.vdn is not None:
        sampled_feat = orc.rendering_forward(nets.vdn, pts, gradients, dirs, feature, nets.vdn_conf).reshape(B, N, -1)
    sampled_color = orc.rendering_forward(nets.color, pts, gradients, dirs, feature, nets.color_conf).reshape(B, N, -1)
    inv_s = torch.exp(nets.variance * 10.0).clip(1e-6, 1e6)
    true_cos = (dirs * gradients).sum(-1, keepdim=True)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + F.relu(-true_cos) * cos_anneal_ratio)
    d = dists.reshape(-1, 1)
    est_next = sdf + iter_cos * d * 0.5
    est_prev = sdf - iter_cos * d * 0.5
    prev_cdf = torch.sigmoid(est_prev * inv_s)
    next_cdf = torch.sigmoid(est_next * inv_s)
    p, c = prev_cdf - next_cdf, prev_cdf
    alpha = ((p + 1e-5) / (c + 1e-5)).reshape(B, N).clip(0.0, 1.0)
    pts_norm = torch.linalg.norm(pts, ord=2, dim=-1, keepdim=True).reshape(B, N)
    inside = (pts_norm < 1.0).to(z_vals.dtype).detach()
    relax = (pts_norm < 1.2).to(z_vals.dtype).detach()
    if bg is not None:
        alpha = alpha * inside + bg["alpha"][:, :N] * (1.0 - inside)
        alpha = torch.cat([alpha, bg["alpha"][:, N:]], -1)
        sampled_color = sampled_color * inside[:, :, None] + bg["sampled_color"][:, :N] * (1.0 - inside)[:, :, None]
        sampled_color = torch.cat([sampled_color, bg["sampled_color"][:, N:]], 1)
        if sampled_feat is not None:
            sampled_feat = sampled_feat * inside[:, :, None] + bg["sampled_feat"][:, :N] * (1.0 - inside)[:, :, None]
            sampled_feat = torch.cat([sampled_feat, bg["sampled_feat"][:, N:]], 1)
    one = torch.ones(B, 1, dtype=alpha.dtype)
    weights = alpha * torch.cumprod(torch.cat([one, 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    weights_sum = weights.sum(-1, keepdim=True)
    color = (sampled_color * weights[:, :, None]).sum(1)
    d_feats = None if sampled_feat is None else (sampled_feat * weights[:, :, None]).sum(1)
    if background_rgb is not None:
        color = color + background_rgb * (1.0 - weights_sum)
    gerr = (torch.linalg.norm(gradients.reshape(B, N, 3), ord=2, dim=-1) - 1.0) ** 2
    eik_num, eik_den = (relax * gerr).sum(), relax.sum()
    return {"d_feats": d_feats, "color": color, "weights": weights, "cdf": c.reshape(B, N), "alpha": alpha,
            "gradient_error": eik_num / (eik_den + 1e-5), "inside_sphere": inside, "eik_num": eik_num, "eik_den": eik_den,
            "s_val": (1.0 / inv_s).expand(B * N, 1), "sampled_color": sampled_color}


@pytest.mark.parametrize("name,dtype", [("wdepth_v065_c1", torch.float32), ("white_v03_c0", torch.float64), ("black_v03", torch.float32)])
def test_render_core_is_bit_identical_to_its_previous_body(golden, name, dtype):
    fx = golden(name)
    st = synth.make_all_states(int(fx["seed"]), wdepth=bool(fx["wdepth"]), variance=float(fx["variance"]))
    nets = orc.nets_from_numpy(st, dtype=dtype)
    tt = lambda x: torch.tensor(x, dtype=dtype)
    o, d, z = tt(fx["rays_o"]), tt(fx["rays_d"]), tt(fx["z_vals_inside"])
    conf = orc.RendererConf()
    _, z_out = orc.coarse_and_outside_z(tt(fx["near"]), tt(fx["far"]), conf, 1.0, tt(fx["t_rand"]), tt(fx["t_rand_out"]))
    sd = 2.0 / conf.n_samples
    bgrgb = torch.ones(1, 3, dtype=dtype) if fx["white"] else None
    with torch.no_grad():
        bg = orc.render_core_outside(nets, o, d, torch.sort(torch.cat([z, z_out], -1), dim=-1)[0], sd)
        for b in (bg, None):
            new = orc.render_core(nets, o, d, z, sd, bg=b, background_rgb=bgrgb, cos_anneal_ratio=float(fx["cos_anneal"]))
            old = _render_core_before(nets, o, d, z, sd, bg=b, background_rgb=bgrgb, cos_anneal_ratio=float(fx["cos_anneal"]))
            for k, v in old.items():
                if v is None:
                    assert new[k] is None
                else:
                    assert torch.equal(new[k], v), (name, k)
