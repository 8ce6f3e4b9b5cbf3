"""The per-ray operators of the renderer as functions of plain tensors (torch, CPU, any float dtype).

One function per kernel family of include/vdn_render.h: `composite` (VdnCompositeArgs: renderer.py:262-315 with the background
alpha of renderer.py:124), `loss_terms` (VdnLossArgs: dpt_runner.py:208-243), `sections` (VdnSectionArgs), `ray_geometry`
(VdnRayAdjointArgs' forward) and `coarse_z` (VdnCoarseArgs). They state the mathematics only: no derivative is written here,
every adjoint a test needs is `torch.autograd.grad` on float64 leaves (`CompositeModel.adjoints`, `loss_adjoints`,
`ray_geometry_adjoints` merely assemble the scalar `sum(g_x * x)` and call it). `neus_oracle.render_core` runs its compositor
through `composite`, so the function is pinned to the reference's golden vectors.
"""
import numpy as np
import torch
import torch.nn.functional as F


def inv_s_from_variance(variance):
    """fields.py:363-364 + renderer.py:262: exp(10 v).clip(1e-6, 1e6)."""
    return torch.exp(variance * 10.0).clip(1e-6, 1e6)


def excl_cumprod_weights(alpha):
    """alpha * exclusive-cumprod(1 - alpha + 1e-7)  (renderer.py:126,187-188,301)."""
    B = alpha.shape[0]
    one = torch.ones(B, 1, dtype=alpha.dtype, device=alpha.device)
    return alpha * torch.cumprod(torch.cat([one, 1.0 - alpha + 1e-7], -1), -1)[:, :-1]


def background_alpha(bg_density, bg_dists):
    """renderer.py:124 on the raw NeRF density [B,T]."""
    return 1.0 - torch.exp(-F.softplus(bg_density) * bg_dists)


def composite(rays_o, rays_d, sdf, normals, dists, mid_z, color, feat, variance,
              bg_density, bg_rgb, bg_feat, bg_dists, background_rgb, cos_anneal_ratio, s_scale=None):
    """renderer.py:262-315. rays_o / rays_d [B,3]; sdf [B*N,1] (or [B,N]); normals [B*N,3]; dists, mid_z [B,N]; color [B,N,3];
    feat [B,N,C] or None; variance: the SingleVarianceNetwork scalar (or [B]: one per ray, which is how a test reads the per-ray
    share of d loss / d variance off autograd); bg_density [B,T] RAW (or None = no background pass), bg_rgb [B,T,3], bg_feat
    [B,T,C] or None, bg_dists [B,T]; background_rgb [1,3] / [3] or None. s_scale [B,N] or None: a factor on inv_s per sample
    (ones), whose gradient is that sample's term of d loss / d log inv_s - the size a cancelling d_variance is judged by.
    """
    B, N = mid_z.shape
    dt = mid_z.dtype
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * mid_z[..., :, None]).reshape(-1, 3)
    dirs = rays_d[:, None, :].expand(B, N, 3).reshape(-1, 3)
    gradients = normals.reshape(-1, 3)
    sdf = sdf.reshape(-1, 1)

    inv_s = inv_s_from_variance(variance)                                          # renderer.py:262-263
    s_val = 1.0 / inv_s
    if inv_s.numel() > 1:
        inv_s = inv_s.reshape(B, 1).expand(B, N).reshape(-1, 1)
    if s_scale is not None:
        inv_s = inv_s * s_scale.reshape(-1, 1)
    true_cos = (dirs * gradients).sum(-1, keepdim=True)                            # renderer.py:265
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) +
                 F.relu(-true_cos) * cos_anneal_ratio)                             # renderer.py:269-270
    d = dists.reshape(-1, 1)
    est_next = sdf + iter_cos * d * 0.5
    est_prev = sdf - iter_cos * d * 0.5
    prev_cdf = torch.sigmoid(est_prev * inv_s)
    next_cdf = torch.sigmoid(est_next * inv_s)
    p, c = prev_cdf - next_cdf, prev_cdf
    raw = ((p + 1e-5) / (c + 1e-5)).reshape(B, N)
    alpha = raw.clip(0.0, 1.0)                                                     # renderer.py:282

    pts_norm = torch.linalg.norm(pts, ord=2, dim=-1, keepdim=True).reshape(B, N)
    inside = (pts_norm < 1.0).to(dt).detach()
    relax = (pts_norm < 1.2).to(dt).detach()

    sampled_color, sampled_feat, bg_alpha = color, feat, None
    if bg_density is not None:                                                     # renderer.py:289-299
        bg_alpha = background_alpha(bg_density, bg_dists)
        alpha = alpha * inside + bg_alpha[:, :N] * (1.0 - inside)
        alpha = torch.cat([alpha, bg_alpha[:, N:]], -1)
        sampled_color = sampled_color * inside[:, :, None] + bg_rgb[:, :N] * (1.0 - inside)[:, :, None]
        sampled_color = torch.cat([sampled_color, bg_rgb[:, N:]], 1)
        if sampled_feat is not None:
            sampled_feat = sampled_feat * inside[:, :, None] + bg_feat[:, :N] * (1.0 - inside)[:, :, None]
            sampled_feat = torch.cat([sampled_feat, bg_feat[:, N:]], 1)

    weights = excl_cumprod_weights(alpha)                                          # renderer.py:301
    weights_sum = weights.sum(-1, keepdim=True)
    color_out = (sampled_color * weights[:, :, None]).sum(1)
    d_feats = None if sampled_feat is None else (sampled_feat * weights[:, :, None]).sum(1)
    if background_rgb is not None:
        color_out = color_out + background_rgb * (1.0 - weights_sum)               # renderer.py:309-310

    g3 = gradients.reshape(B, N, 3)
    gerr = (torch.linalg.norm(g3, ord=2, dim=-1) - 1.0) ** 2
    eik_num = (relax * gerr).sum()
    eik_den = relax.sum()
    gradient_error = eik_num / (eik_den + 1e-5)                                    # renderer.py:313-315
    return {"alpha": alpha, "weights": weights, "cdf": c.reshape(B, N), "inside_sphere": inside, "relax_sphere": relax,
            "color": color_out, "d_feats": d_feats, "weight_sum": weights_sum, "weight_max": weights.max(-1, keepdim=True)[0],
            "s_val": s_val, "eik_num_ray": (relax * gerr).sum(-1), "eik_den_ray": relax.sum(-1),
            "eik_num": eik_num, "eik_den": eik_den, "gradient_error": gradient_error,
            "sampled_color": sampled_color, "sampled_feat": sampled_feat, "bg_alpha": bg_alpha,
            # what the branches see (for the coverage / margin tests; not outputs of the operator)
            "true_cos": true_cos.reshape(B, N), "raw_alpha": raw, "p": p.reshape(B, N), "pts_norm": pts_norm, "inv_s": inv_s}


# the tensors vdn_alpha_composite_bwd differentiates with respect to, by the names of its outputs
COMPOSITE_LEAVES = {"d_sdf": "sdf", "d_normals": "normals", "d_color": "color", "d_feat": "feat", "d_bg_density": "bg_density",
                    "d_bg_rgb": "bg_rgb", "d_bg_feat": "bg_feat", "d_dists": "dists", "d_bg_dists": "bg_dists"}


class CompositeModel:
    """composite() of one case (oracle/ray_cases.py) in `dtype`, its graph kept, so that several sets of upstream gradients can
    be pulled back through it. The inputs are the case's float32 arrays cast to `dtype`."""

    def __init__(self, case, dtype=torch.float64):
        t = lambda k: None if case.get(k) is None else torch.tensor(case[k]).to(dtype)
        B, N, T = case["B"], case["N"], case["T"]
        self.B, self.N, self.T, self.dtype = B, N, T, dtype
        self.x = {k: t(k) for k in ("rays_o", "rays_d", "sdf", "normals", "dists", "mid_z", "color", "feat", "bg_density", "bg_rgb",
                                    "bg_feat", "bg_dists", "background_rgb")}
        x = self.x
        for k in ("sdf", "normals", "dists", "color", "feat", "bg_density", "bg_rgb", "bg_feat", "bg_dists"):
            if x[k] is not None:
                x[k].requires_grad_(True)
        # one variance per ray and one inv_s factor per sample: d_var_partial and the size of its terms come out of autograd
        self.var_rays = torch.full((B,), float(case["variance"]), dtype=torch.float32).to(dtype).requires_grad_(True)
        self.s_scale = torch.ones(B, N, dtype=dtype, requires_grad=True)
        # VdnCompositeBwdArgs.d_dir_cos is the adjoint of the direction inside true_cos alone. The only other use composite()
        # makes of rays_d is the sample position behind the (detached) inside / relax tests, so a leaf passed as rays_d gets
        # exactly that adjoint.
        self.dir_cos = x["rays_d"].clone().requires_grad_(True)
        self.out = composite(x["rays_o"], self.dir_cos, x["sdf"], x["normals"], x["dists"], x["mid_z"], x["color"], x["feat"],
                             self.var_rays, x["bg_density"], x["bg_rgb"], x["bg_feat"], x["bg_dists"], x["background_rgb"],
                             float(case["cos_anneal"]), s_scale=self.s_scale)

    def adjoints(self, g_color=None, g_feat=None, g_weights=None, g_cdf=None, g_eik=None):
        """autograd.grad(sum(g_x * x), leaves) -> dict by the kernel's output names, plus d_var_partial [B], d_variance and
        d_var_abs [B] = sum_i |sample i's term of d_var_partial|. An upstream gradient that is None counts as zero."""
        o, dt = self.out, self.dtype
        tt = lambda g: torch.tensor(g).to(dt)
        L = o["color"].sum() * 0.0
        if g_color is not None:
            L = L + (tt(g_color) * o["color"]).sum()
        if g_feat is not None and o["d_feats"] is not None:
            L = L + (tt(g_feat) * o["d_feats"]).sum()
        if g_weights is not None:
            L = L + (tt(g_weights) * o["weights"]).sum()
        if g_cdf is not None:
            L = L + (tt(g_cdf) * o["cdf"]).sum()
        if g_eik is not None:
            L = L + float(g_eik) * o["gradient_error"]
        names = [k for k, v in COMPOSITE_LEAVES.items() if self.x[v] is not None]
        leaves = [self.x[COMPOSITE_LEAVES[k]] for k in names] + [self.var_rays, self.s_scale, self.dir_cos]
        grads = torch.autograd.grad(L, leaves, retain_graph=True, allow_unused=True)
        grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
        res = {k: g.detach() for k, g in zip(names, grads)}
        dvar, dscale, ddir = grads[-3].detach(), grads[-2].detach(), grads[-1].detach()
        res["d_var_partial"] = dvar
        res["d_variance"] = dvar.sum()
        # d L / d s_scale_i = inv_s dL / d inv_s_i, and d inv_s / d variance = 10 inv_s where the clip is inactive, 0 where active
        active = 1.0 if 1e-6 <= float(torch.exp(self.var_rays[0].detach().double() * 10.0)) <= 1e6 else 0.0
        res["d_var_abs"] = 10.0 * active * dscale.abs().sum(-1)
        res["d_dir_cos"] = ddir
        return res


def loss_terms(color, true_rgb, mask, feats, gt_feats, weights, gradient_error, igr_weight, mask_weight, depth_weight):
    """dpt_runner.py:208-243 on raw tensors: color, true_rgb [B,3]; mask [B,1] or None (= ones); feats, gt_feats [B,C] or None;
    weights [B,T] (weight_sum = their sum per ray); gradient_error: scalar tensor. Returns the six scalars of
    VdnLossArgs.out_scalars by name (mask_loss is 0 when mask_weight == 0: the term is not formed then, as in the runner)."""
    if mask is None:
        mask = torch.ones_like(true_rgb[:, :1])
    mask_sum = mask.sum() + 1e-5
    err = (color - true_rgb) * mask
    color_loss = err.abs().sum() / mask_sum
    psnr = 20.0 * torch.log10(1.0 / (((color - true_rgb) ** 2 * mask).sum() / (mask_sum * 3.0)).sqrt())
    loss = color_loss + gradient_error * igr_weight
    mask_loss = torch.zeros((), dtype=color.dtype)
    if mask_weight != 0.0:
        weight_sum = weights.sum(-1, keepdim=True)
        mask_loss = F.binary_cross_entropy(weight_sum.clip(1e-3, 1.0 - 1e-3), mask)
        loss = loss + mask_loss * mask_weight
    depth_loss = torch.zeros((), dtype=color.dtype)
    if feats is not None:
        depth_loss = ((feats - gt_feats) * mask).abs().sum() / mask_sum
        loss = loss + depth_loss * depth_weight
    return {"loss": loss, "color_loss": color_loss, "psnr": psnr, "eikonal": gradient_error + 0.0, "depth_loss": depth_loss,
            "mask_loss": mask_loss}


LOSS_SCALARS = ("loss", "color_loss", "psnr", "eikonal", "depth_loss", "mask_loss")


def loss_adjoints(case, dtype=torch.float64):
    """loss_terms of a loss case and grad_scale * d loss / d (color, feats, weights), d loss / d gradient_error by autograd."""
    t = lambda k: None if case.get(k) is None else torch.tensor(case[k]).to(dtype)
    color, feats, weights = t("color"), t("feats"), t("weights")
    eik = torch.tensor(float(case["eik"][0]), dtype=torch.float32).to(dtype)
    leaves = {"g_color": color, "g_weights": weights, "g_eik": eik}
    if feats is not None:
        leaves["g_feats"] = feats
    for v in leaves.values():
        v.requires_grad_(True)
    mask = t("mask")
    out = loss_terms(color, t("true_rgb"), None if mask is None else mask[:, None], feats, t("gt_feats"), weights, eik,
                     float(case["igr_weight"]), float(case["mask_weight"]), float(case["depth_weight"]))
    grads = torch.autograd.grad(out["loss"], list(leaves.values()), allow_unused=True)
    res = {k: out[k].detach() for k in LOSS_SCALARS}
    gs = float(case["grad_scale"])
    for (k, l), g in zip(leaves.items(), grads):
        g = torch.zeros_like(l) if g is None else g
        res[k] = (g if k == "g_eik" else g * gs).detach()       # (grad_scale multiplies the per-ray gradients only: header)
    res["weight_sum"] = weights.detach().sum(-1)
    return res


def sections(z, sample_dist):
    """renderer.py:228-230 / 107-109: dists = diff(z) with last = sample_dist; mid_z = z + dists / 2."""
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, torch.full_like(z[..., :1], sample_dist)], -1)
    return dists, z + dists * 0.5


def ray_geometry(rays_o, rays_d, z, z_out, sample_dist):
    """The ray geometry of render_core and render_core_outside (renderer.py:107-115, 228-237): points, directions, section lengths
    and mid-points of the inside pass over z [B,N] and, with z_out [B,T-N], of the background pass over [z | z_out]."""
    B, N = z.shape
    dists, mid = sections(z, sample_dist)
    out = {"pts": rays_o[:, None, :] + rays_d[:, None, :] * mid[..., :, None], "dirs": rays_d[:, None, :].expand(B, N, 3),
           "dists": dists, "mid": mid}
    if z_out is not None:
        zf = torch.cat([z, z_out], -1)
        bd, bm = sections(zf, sample_dist)
        out.update({"bg_pts": rays_o[:, None, :] + rays_d[:, None, :] * bm[..., :, None],
                    "bg_dirs": rays_d[:, None, :].expand(B, zf.shape[1], 3), "bg_dists": bd, "bg_mid": bm})
    return out


def ray_geometry_adjoints(case, dtype=torch.float64):
    """autograd of sum(upstream * output) over ray_geometry's outputs (+ d_dir_cos . rays_d: the compositor's share of d rays_d)."""
    t = lambda k: None if case.get(k) is None else torch.tensor(case[k]).to(dtype)
    o, d, z, zo = t("rays_o").requires_grad_(True), t("rays_d").requires_grad_(True), t("z").requires_grad_(True), t("z_out")
    if zo is not None:
        zo.requires_grad_(True)
    g = ray_geometry(o, d, z, zo, float(case["sample_dist"]))
    L = (t("d_pts") * g["pts"]).sum() + (t("d_dirs") * g["dirs"]).sum() + (t("d_dists") * g["dists"]).sum() + (t("d_dir_cos") * d).sum()
    if zo is not None:
        L = L + (t("d_bg_pts") * g["bg_pts"]).sum() + (t("d_bg_dirs") * g["bg_dirs"]).sum() + (t("d_bg_dists") * g["bg_dists"]).sum()
    leaves = [o, d, z] + ([zo] if zo is not None else [])
    grads = torch.autograd.grad(L, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if gg is None else gg for gg, l in zip(grads, leaves)]
    res = dict(zip(("d_rays_o", "d_rays_d", "d_z", "d_z_out"), grads))
    res["mid"], res["bg_mid"] = g["mid"].detach(), (g["bg_mid"].detach() if zo is not None else None)
    return res


def coarse_z(near, far, lin_samples, lin_outside, out_lower, out_upper, t_rand, t_rand_out):
    """renderer.py:334-359 on the vectors VdnCoarseArgs passes in: near, far [B,1]; lin_samples [n]; lin_outside, out_lower,
    out_upper [n_out] or None; t_rand [B,1] / t_rand_out [B,n_out] or None. -> z [B,n], z_out [B,n_out] or None."""
    n = lin_samples.shape[0]
    z = near + (far - near) * lin_samples[None, :]
    if t_rand is not None:
        z = z + (t_rand - 0.5) * 2.0 / n
    z_out = None
    if lin_outside is not None and lin_outside.shape[0] > 0:
        zo = lin_outside[None, :].expand(near.shape[0], -1)
        if t_rand_out is not None:
            zo = out_lower[None, :] + (out_upper - out_lower)[None, :] * t_rand_out
        z_out = far / torch.flip(zo, dims=[-1]) + 1.0 / n
    return z, z_out


# ---- what the tests compare: the kernels' output buffers by name, from a CompositeModel ------------------------------------

UPSTREAM = ("g_color", "g_feat", "g_weights", "g_cdf", "g_eik")


def forward_arrays(model):
    """The outputs of vdn_alpha_composite_fwd (VdnCompositeArgs' names) as float64 numpy arrays."""
    o = model.out
    n = lambda t: t.detach().double().numpy()
    res = {"weights": n(o["weights"]), "alpha_out": n(o["alpha"]), "cdf": n(o["cdf"]), "inside_sphere": n(o["inside_sphere"]),
           "color_out": n(o["color"]), "weight_sum": n(o["weight_sum"])[:, 0], "weight_max": n(o["weight_max"])[:, 0],
           "s_val": n(o["s_val"]).reshape(-1), "eik_partial": n(torch.stack([o["eik_num_ray"], o["eik_den_ray"]], -1)),
           "eik_out": n(torch.stack([o["gradient_error"], o["eik_num"], o["eik_den"]]))}
    if o["d_feats"] is not None:
        res["feat_out"] = n(o["d_feats"])
    return res


def upstream_of(case, drop=None):
    """The adjoint's upstream gradients of a case, `drop` (one of UPSTREAM) left out = NULL = zero."""
    kw = {k: case[k] for k in UPSTREAM if k != drop and case.get(k) is not None}
    if "g_eik" in kw:
        kw["g_eik"] = float(kw["g_eik"][0])
    return kw


def adjoint_arrays(model, **upstream):
    return {k: v.double().numpy() for k, v in model.adjoints(**upstream).items()}


def var_units(got, ref, abs_sum, rtol=1e-4, floor=1e-6):
    """d_var_partial / d_variance are signed sums that cancel: judged against the sum of the absolute per-sample terms (per ray;
    for d_variance over the batch), |got - ref| <= rtol * that sum, floored at `floor` of the largest such sum."""
    got, ref, abs_sum = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(abs_sum, np.float64)
    if abs_sum.max() == 0.0:
        return 0.0 if (got == 0.0).all() else float("inf")          # the clipped inv_s: exactly zero
    return float((np.abs(got - ref) / (rtol * abs_sum + floor * abs_sum.max())).max())
