"""The exactness claim behind the heads' prefix of the foreground work list (DESIGN.md "Work lists", third consequence), held to
the oracle: in oracle/ray_ops.composite (renderer.py:284-299) the colour and the VDN feature of an inside sample with
inside_sphere = 0 are multiplied by an exact 0.0 in the blend with the background pass. So whatever those slots hold (finite),
no output moves by one bit, and autograd's gradient with respect to them is exactly zero - which is why the colour and the VDN
head need not run on the listed samples with 1 <= |p| < 1.2, forward or backward."""
import numpy as np
import torch

from oracle import ray_ops


def _case(seed, B=6, N=24, O=8, C=5):
    rng = np.random.default_rng(seed)
    T = N + O
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    o = rng.standard_normal((B, 3)) * 0.3
    d = rng.standard_normal((B, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mid = np.sort(rng.uniform(0.0, 2.2, (B, N)), axis=1)          # samples on both sides of |p| = 1 and of |p| = 1.2
    x = dict(rays_o=t(o), rays_d=t(d), sdf=t(rng.standard_normal((B * N, 1)) * 0.2), normals=t(rng.standard_normal((B * N, 3))),
             dists=t(rng.uniform(0.01, 0.05, (B, N))), mid_z=t(mid), color=t(rng.uniform(0, 1, (B, N, 3))), feat=t(rng.uniform(0, 1, (B, N, C))),
             variance=t(0.3), bg_density=t(rng.standard_normal((B, T))), bg_rgb=t(rng.uniform(0, 1, (B, T, 3))),
             bg_feat=t(rng.uniform(0, 1, (B, T, C))), bg_dists=t(rng.uniform(0.01, 0.05, (B, T))), background_rgb=t(np.ones((1, 3))))
    return x


def _run(x):
    return ray_ops.composite(x["rays_o"], x["rays_d"], x["sdf"], x["normals"], x["dists"], x["mid_z"], x["color"], x["feat"], x["variance"],
                             x["bg_density"], x["bg_rgb"], x["bg_feat"], x["bg_dists"], x["background_rgb"], 0.4)


OUTPUTS = ("alpha", "weights", "cdf", "color", "d_feats", "weight_sum", "weight_max", "gradient_error", "sampled_color", "sampled_feat")


def test_heads_outputs_outside_the_unit_sphere_reach_no_output_and_get_zero_gradient():
    for seed in (1, 2, 3):
        x = _case(seed)
        ref = _run(x)
        inside = ref["inside_sphere"]
        relax = ref["relax_sphere"]
        shell = (inside == 0) & (relax == 1)
        assert shell.any() and (inside == 1).any() and (relax == 0).any()        # all three kinds of inside sample occur
        # any finite value in the slots the blend multiplies by zero: no output moves
        y = dict(x)
        rng = np.random.default_rng(100 + seed)
        off = (inside == 0)[:, :, None]
        y["color"] = torch.where(off, torch.tensor(rng.uniform(0, 1e3, tuple(x["color"].shape))), x["color"])
        y["feat"] = torch.where(off, torch.tensor(rng.uniform(0, 1e3, tuple(x["feat"].shape))), x["feat"])
        assert not torch.equal(y["color"], x["color"])
        got = _run(y)
        for k in OUTPUTS:
            assert torch.equal(got[k], ref[k]), k
        # autograd: the gradient with respect to those slots is exactly zero, for any upstream gradient
        z = dict(x)
        z["color"] = x["color"].clone().requires_grad_(True)
        z["feat"] = x["feat"].clone().requires_grad_(True)
        out = _run(z)
        gc, gf = torch.tensor(rng.standard_normal(tuple(out["color"].shape))), torch.tensor(rng.standard_normal(tuple(out["d_feats"].shape)))
        loss = (out["color"] * gc).sum() + (out["d_feats"] * gf).sum() + out["gradient_error"] + out["weight_sum"].sum()
        d_color, d_feat = torch.autograd.grad(loss, [z["color"], z["feat"]])
        assert (d_color[inside == 0] == 0).all() and (d_feat[inside == 0] == 0).all()
        assert (d_color[inside == 1] != 0).any() and (d_feat[inside == 1] != 0).any()
