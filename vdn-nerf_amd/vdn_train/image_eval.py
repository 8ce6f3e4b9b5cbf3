"""Image figures of a trained model against its ground-truth views: L1, PSNR and SSIM, over the object mask and over every pixel -
the image row of a NeuS / VDN-NeRF results table, and the reference's whole-set check Runner.val_all_imgs (dpt_runner.py:493-518)
with the `both_mask` pair of val_img (482-489). All of it on the device: render() writes the colours there, the ground truth and
the masks live there (RaysGenerator.images, .masks), and vdn_hip.image.image_stats (csrc/image_eval.hip) turns two
images into the sums in double, bit-reproducibly. Only result vectors of ten numbers per image travel to the host, once.

L1 and PSNR are the reference's (477-480): l1 = sum |e| m / mask_sum over the three channels, not divided by 3, psnr =
20 log10(1 / sqrt(sum e^2 m / (3 mask_sum))), mask_sum = count + 1e-5, a pixel in the mask when mask > 0.1. SSIM is Wang et al.
2004 with the 11-tap Gaussian window (sigma 1.5), C1 = 0.01^2, C2 = 0.03^2, data range 1, over the windows that lie inside the
image. `ssim_masked`, the mean over the windows whose centre pixel is in the mask, is this project's definition: the reference
has no SSIM at all."""
import json
import math

import numpy as np
import torch

from vdn_hip import image as vimage
from vdn_train import validate

FIGURES = ("l1", "psnr", "l1_masked", "psnr_masked", "ssim", "ssim_masked", "gradient_error")


def evaluate_image(pred, gt, mask=None, ssim_map=False, device=None):
    """pred, gt [H,W,3] in [0,1], mask [H,W,1|3] or None; float32 numpy arrays or tensors, moved to the device where needed (the
    device of the first tensor that is on one, else `device`, else cuda:0) -> vdn_hip.image.finish's dict (and, with ssim_map, the
    [H-10,W-10] map of the channel-mean SSIM as a numpy array under "ssim_map")."""
    given = [(name, x if torch.is_tensor(x) else np.asarray(x)) for name, x in (("pred", pred), ("gt", gt), ("mask", mask)) if x is not None]
    vimage.check_images(*[x for _, x in given])
    for name, x in given:
        if x.dtype not in (torch.float32, np.float32):
            raise ValueError("%s must be float32, got %s (shape %r)" % (name, x.dtype, tuple(x.shape)))
    dev = next((x.device for _, x in given if torch.is_tensor(x) and x.device.type == "cuda"), None)
    if dev is None:
        dev = torch.device(device if device is not None else "cuda:0")
    t = [x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for _, x in given]
    out = vimage.image_stats(t[0], t[1], t[2] if mask is not None else None, ssim_map=ssim_map)
    if ssim_map:
        res = vimage.finish(out[0].cpu())
        res["ssim_map"] = out[1].cpu().numpy()
        return res
    return vimage.finish(out.cpu())


@torch.no_grad()
def _view_on_device(renderer, rays_gen, idx, resolution_level, batch_size, cos_anneal_ratio, white_bkgd, depth_before_color, jitter, ssim_map):
    """One view -> (result vector [10] float64, mean gradient_error [] float64, map or None), all on the
    device, nothing read back."""
    rays_o, rays_d = rays_gen.gen_rays_at(idx, resolution_level=resolution_level)
    H, W, _ = rays_o.shape
    rays_o, rays_d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    dev = rays_o.device
    bg = torch.ones(1, 3, device=dev) if white_bkgd else None
    rgb = torch.empty(H * W, 3, device=dev)
    eik = []
    for s, n, out in validate._render_batches(renderer, rays_gen, rays_o, rays_d, batch_size, jitter=jitter, cos_anneal_ratio=cos_anneal_ratio,
                                              background_rgb=bg, depth_before_color=depth_before_color):
        rgb[s:s + n] = out["color_fine"]
        eik.append(out["gradient_error"].clone())
        del out
    rgb = rgb.reshape(H, W, 3)
    gt = rays_gen.image_at_device(idx, resolution_level=resolution_level)
    mask = rays_gen.mask_at_device(idx, resolution_level=resolution_level) if rays_gen.masks is not None else None
    out = vimage.image_stats(rgb, gt, mask, ssim_map=ssim_map)
    vec, smap = out if ssim_map else (out, None)
    return vec, torch.stack(eik).double().mean(), smap


def evaluate_view(renderer, rays_gen, idx, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0, white_bkgd=True,
                  depth_before_color=False, jitter=None, ssim_map=False):
    """Render view `idx` at 1/resolution_level size (validate._render_batches, `jitter` as there) and compare it with the
    generator's image and mask at that level, on the device -> vdn_hip.image.finish's dict plus "gradient_error" (the mean of the
    batches' eikonal terms, as val_img's), "idx", and with ssim_map the numpy map under "ssim_map". Without masks in the generator
    the masked figures equal the unmasked ones. The colour image never goes to the host: one read of eleven numbers ends the call."""
    vec, eik, smap = _view_on_device(renderer, rays_gen, int(idx), resolution_level, batch_size, cos_anneal_ratio, white_bkgd,
                                        depth_before_color, jitter, ssim_map)
    host = torch.cat([vec, eik[None]]).cpu()
    res = vimage.finish(host[:vimage.RESULT_LEN])
    res["gradient_error"], res["idx"] = float(host[-1]), int(idx)
    if ssim_map:
        res["ssim_map"] = smap.cpu().numpy()
    return res


def evaluate_images(renderer, rays_gen, indices=None, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0, white_bkgd=True,
                    depth_before_color=False, jitter=None):
    """Runner.val_all_imgs (dpt_runner.py:493-518) with both_mask: every view of `indices` (default: all of the generator's) as
    evaluate_view sees it -> {"images": [per-view dict], "mean": {figure: mean over the views}, "n_images", "resolution_level"}.
    The means are means of the per-view figures - PSNR the mean of the views' PSNRs - as the reference prints them (514-518); a
    view whose figure is nan (ssim_masked over an empty mask) is left out of that figure's mean. The views' result vectors stay on
    the device and are read back once, after the last view. jitter: None, or one list per view of _render_batches' jitter.
    Follows VDN_RENDER_GRAPH the way _render_batches does."""
    indices = list(range(rays_gen.n_images)) if indices is None else [int(i) for i in indices]
    for i in indices:
        if not 0 <= i < rays_gen.n_images:
            raise ValueError("view %d is outside the generator's %d images" % (i, rays_gen.n_images))
    if not indices:
        raise ValueError("no views to evaluate")
    if jitter is not None and len(jitter) != len(indices):
        raise ValueError("jitter must hold one list per view: %d views, %d lists" % (len(indices), len(jitter)))
    rows = []
    for k, i in enumerate(indices):
        vec, eik, _ = _view_on_device(renderer, rays_gen, i, resolution_level, batch_size, cos_anneal_ratio, white_bkgd,
                                         depth_before_color, None if jitter is None else jitter[k], False)
        rows.append(torch.cat([vec, eik[None]]))
    host = torch.stack(rows).cpu().numpy()                                # the one read
    fig = vimage.finish(host[:, :vimage.RESULT_LEN])
    fig["gradient_error"] = host[:, -1]
    images = []
    for k, i in enumerate(indices):
        d = {key: (int(v[k]) if key.startswith("n_") else float(v[k])) for key, v in fig.items()}
        d["idx"] = i
        images.append(d)
    mean = {}
    for key in FIGURES:
        v = np.asarray([d[key] for d in images], dtype=np.float64)
        v = v[~np.isnan(v)]
        mean[key] = float(v.mean()) if v.size else float("nan")
    return {"images": images, "mean": mean, "n_images": len(images), "resolution_level": int(resolution_level)}


def to_json(result):
    """One JSON line of an evaluate_image / evaluate_view / evaluate_images result: nan and inf as null, maps left out."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items() if k != "ssim_map"}
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return float(v) if math.isfinite(v) else None
        if isinstance(v, np.integer):
            return int(v)
        return v
    return json.dumps(clean(result))
