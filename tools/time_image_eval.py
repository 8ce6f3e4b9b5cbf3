"""Image evaluation on the device (vdn_hip.image.image_stats) against the host path it replaces:

    python tools/time_image_eval.py --out profiles/image_eval.json

Three legs, one process:
  image_stats   for each --sizes image (default 400x300, 800x600, 1600x1200; random pred / gt, a disc mask): the device time of one
                image_stats call between events (both launches), with and without the SSIM map, the median of --repeats calls
                after a warm-up call.
  baseline      the same images through what there was before: the device -> host copy of the rendered image plus
                validate.image_metrics on the host (host clock, twice: unmasked and masked, as the both_mask pair needs), and SSIM
                as torch float64 conv2d calls on the device (between events) with its difference from image_stats' figure.
  whole loop    one evaluate_view call against one validate.val_img call (host clock, device synchronised) on a synthetic view of
                --view WxH pixels, bf16 networks, and image_stats' device time at that size: its share of the view's time.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=size, nargs="*", default=[(400, 300), (800, 600), (1600, 1200)], metavar="WxH")
    ap.add_argument("--view", type=size, default=(200, 150), metavar="WxH", help="the whole-loop leg's image")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from vdn_hip import image
    from vdn_train import factory, image_eval, synth, validate
    from vdn_train.rays import RaysGenerator
    if not torch.cuda.is_available():
        raise SystemExit("time_image_eval.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")

    def device_ms(fn):
        fn()                                                 # warm-up: code objects, the allocator's blocks for this size
        runs = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1))
        return {"device_ms_median": statistics.median(runs), "device_ms_all": runs}

    def wall_ms(fn):
        fn()
        runs = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            s = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            runs.append(1e3 * (time.perf_counter() - s))
        return {"wall_ms_median": statistics.median(runs), "wall_ms_all": runs}

    k = torch.arange(-5, 6, dtype=torch.float64, device=dev)
    g = torch.exp(-(k * k) / 4.5)
    g = g / g.sum()
    kh, kv = g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), g.view(1, 1, 11, 1).repeat(3, 1, 1, 1)

    def torch_ssim(pred, gt):
        """the definition as torch float64 ops: ten depthwise conv2d calls and a dozen element-wise ones -> mean S, on the device"""
        F = torch.nn.functional
        x, y = pred.double().permute(2, 0, 1)[None], gt.double().permute(2, 0, 1)[None]
        f = lambda t: F.conv2d(F.conv2d(t, kh, groups=3), kv, groups=3)
        mx, my = f(x), f(y)
        vx, vy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        S = ((2.0 * mx * my + 1e-4) * (2.0 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
        return S.mean()

    rows = []
    for W, H in a.sizes:
        gen = torch.Generator(device=dev).manual_seed(H * 10007 + W)
        gt = torch.rand(H, W, 3, device=dev, generator=gen)
        pred = (gt + 0.05 * torch.randn(H, W, 3, device=dev, generator=gen)).clamp(0.0, 1.0)
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        mask = (((yy - 0.5 * H) ** 2 + (xx - 0.5 * W) ** 2) <= (0.4 * min(H, W)) ** 2).float()[..., None].contiguous()
        gt_host, mask_host = gt.cpu().numpy(), mask.cpu().numpy()
        fig = image.finish(image.image_stats(pred, gt, mask).cpu())
        row = {"width": W, "height": H, "tiles": int(image.lib.call_value("vdn_image_stats_tiles", H, W)),
               "figures": {key: fig[key] for key in ("l1", "psnr", "l1_masked", "psnr_masked", "ssim", "ssim_masked")},
               "image_stats": device_ms(lambda: image.image_stats(pred, gt, mask)),
               "image_stats_with_map": device_ms(lambda: image.image_stats(pred, gt, mask, ssim_map=True)),
               "image_stats_call_wall": wall_ms(lambda: image.image_stats(pred, gt, mask))}

        def host_metrics():
            img = pred.cpu().numpy()
            return validate.image_metrics(img, gt_host, None), validate.image_metrics(img, gt_host, mask_host)
        row["host_copy_and_image_metrics"] = wall_ms(host_metrics)
        (l1, psnr), (l1m, psnrm) = host_metrics()
        row["host_figures"] = {"l1": l1, "psnr": psnr, "l1_masked": l1m, "psnr_masked": psnrm}
        try:
            row["torch_float64_conv2d_ssim"] = device_ms(lambda: torch_ssim(pred, gt))
            row["torch_float64_conv2d_ssim"]["ssim"] = float(torch_ssim(pred, gt))
            row["torch_float64_conv2d_ssim"]["difference_from_image_stats"] = row["torch_float64_conv2d_ssim"]["ssim"] - fig["ssim"]
        except RuntimeError as e:                             # (a build of torch without a double convolution)
            row["torch_float64_conv2d_ssim"] = {"error": str(e).splitlines()[0]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del gt, pred, mask

    W, H = a.view
    K = np.eye(4)
    K[0, 0] = K[1, 1] = synth.FOCAL * W / synth.W_IMG
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    cams = synth.make_cameras(0)[:1]
    blank = RaysGenerator(np.ones((1, H, W, 3), np.float32), None, cams, K, device=dev)          # (for the view's rays)
    o, d = blank.gen_rays_at(0)
    images = synth.target_colors(o.reshape(-1, 3).cpu().numpy(), d.reshape(-1, 3).cpu().numpy()).reshape(1, H, W, 3)
    masks = (images.min(axis=-1, keepdims=True) < 1.0).astype(np.float32)
    gen = RaysGenerator(images, masks, cams, K, device=dev)
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0), precision="bf16")
    view_img = torch.rand(H, W, 3, device=dev)
    loop = {"width": W, "height": H, "rays": H * W, "batch_size": 512, "precision": "bf16",
            "evaluate_view": wall_ms(lambda: image_eval.evaluate_view(rend, gen, 0)),
            "val_img_use_mask": wall_ms(lambda: validate.val_img(rend, None, gen, 0, use_mask=True)),
            "image_stats_at_this_size": device_ms(lambda: image.image_stats(view_img, gen.images[0], gen.masks[0]))}
    loop["image_stats_share_of_evaluate_view"] = loop["image_stats_at_this_size"]["device_ms_median"] / loop["evaluate_view"]["wall_ms_median"]
    loop["rays_per_second_evaluate_view"] = H * W / (1e-3 * loop["evaluate_view"]["wall_ms_median"])
    print(json.dumps(loop), file=sys.stderr, flush=True)

    out = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "torch": torch.__version__,
           "timer": "device_ms: device events around the call on the current stream, synchronised before and after; wall_ms: host clock "
                    "around the call, device synchronised; each the median of %d calls after one warm-up call" % a.repeats,
           "rows": rows, "whole_loop": loop}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
