"""L1, PSNR and SSIM of rendered images against their ground truth, over a mask and over every pixel, on the device
(vdn_train/image_eval.py; INTEGRATION.md "Image evaluation"). Two modes, one JSON line each:

    python tools/eval_images.py --pred renders/ --gt images/ [--mask images/mask/]

PNG folders, paired by sorted file name (the folders must hold the same number of files of one size per pair); no networks needed.

    python tools/eval_images.py --scene data/scan24 --checkpoint ckpt_300000.pth [--conf wdepth] [--resolution-level 4]
                                [--indices 0 8 16] [--precision bf16] [--out images.json]

A scene directory (vdn_train.dataset.SceneData) and the runner's checkpoint file: every view (or --indices) is rendered and
compared on the device, the reference's Runner.val_all_imgs with both_mask. --conf names the shipped configuration the checkpoint
was trained with: `white` (womsk_white) or `wdepth` (womsk_white_wdepth: the VDN head and the depth features)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", default=None, metavar="DIR", help="folder of rendered PNGs")
    ap.add_argument("--gt", default=None, metavar="DIR", help="folder of ground-truth PNGs")
    ap.add_argument("--mask", default=None, metavar="DIR", help="folder of mask PNGs (in the mask where > 0.1 of full scale)")
    ap.add_argument("--scene", default=None, metavar="DIR", help="scene directory (cameras_sphere.npz, image/, image/mask/)")
    ap.add_argument("--checkpoint", default=None, metavar="CKPT", help="trained weights, the runner's checkpoint file")
    ap.add_argument("--conf", choices=("white", "wdepth"), default="white")
    ap.add_argument("--resolution-level", type=int, default=1)
    ap.add_argument("--indices", type=int, nargs="*", default=None, help="views to evaluate (default: all)")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, metavar="FILE", help="also write the JSON line there")
    return ap


def list_pngs(folder):
    files = sorted(f for f in os.listdir(folder) if f.lower().endswith(".png"))
    if not files:
        raise SystemExit("no *.png under %s" % folder)
    return [os.path.join(folder, f) for f in files]


def read_png(path, mask=False):
    """-> float32 [H,W,3] in [0,1] (RGB; the figures do not depend on the channel order), or [H,W,1] for a mask."""
    import numpy as np
    from PIL import Image
    im = Image.open(path).convert("L" if mask else "RGB")
    a = np.asarray(im, dtype=np.float32) / np.float32(255.0)
    return np.ascontiguousarray(a[:, :, None] if mask else a)


def evaluate_folders(pred_dir, gt_dir, mask_dir=None, device="cuda:0"):
    """-> {"images": [per-pair dict with "pred", "gt" file names], "mean": {...}, "n_images"}: evaluate_image per pair, paired by
    sorted file name; the means are means of the per-image figures (nan left out), as evaluate_images'."""
    import numpy as np
    from vdn_train import image_eval
    pred, gt = list_pngs(pred_dir), list_pngs(gt_dir)
    mask = list_pngs(mask_dir) if mask_dir is not None else [None] * len(pred)
    if not (len(pred) == len(gt) == len(mask)):
        raise SystemExit("the folders do not pair up: %d predictions, %d ground-truth images%s" % (
            len(pred), len(gt), "" if mask_dir is None else ", %d masks" % len(mask)))
    images = []
    for p, g, m in zip(pred, gt, mask):
        res = image_eval.evaluate_image(read_png(p), read_png(g), None if m is None else read_png(m, mask=True), device=device)
        images.append(dict(res, pred=os.path.basename(p), gt=os.path.basename(g)))
    mean = {}
    for key in image_eval.FIGURES:
        v = np.asarray([d[key] for d in images if key in d], dtype=np.float64)
        v = v[~np.isnan(v)]
        if v.size:
            mean[key] = float(v.mean())
    return {"images": images, "mean": mean, "n_images": len(images)}


def evaluate_scene(a):
    import torch
    from vdn_train import factory, image_eval
    from vdn_train.dataset import SceneData
    dev = torch.device(a.device)
    wdepth = a.conf == "wdepth"
    ckpt = torch.load(a.checkpoint, map_location="cpu")
    keys = ("nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine") + (("depth_network_fine",) if wdepth else ())
    states = {k: {n: (x.numpy() if torch.is_tensor(x) else x) for n, x in ckpt[k].items()} for k in keys}
    rend = factory.build_renderer(wdepth=wdepth, device=dev, states=states, precision=a.precision)
    scene = SceneData(a.scene, with_depth=False)
    with torch.cuda.device(dev):
        res = image_eval.evaluate_images(rend, scene.rays_generator(device=dev), indices=a.indices, resolution_level=a.resolution_level,
                                         batch_size=a.batch_size)
    for d in res["images"]:
        d["name"] = scene.names[d["idx"]]
    return res


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    folders, scene = a.pred is not None or a.gt is not None, a.scene is not None or a.checkpoint is not None
    if folders == scene or (folders and (a.pred is None or a.gt is None)) or (scene and (a.scene is None or a.checkpoint is None)):
        ap.error("give either --pred DIR --gt DIR [--mask DIR] or --scene DIR --checkpoint FILE")
    from vdn_train import image_eval
    res = evaluate_folders(a.pred, a.gt, a.mask, device=a.device) if folders else evaluate_scene(a)
    line = image_eval.to_json(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
