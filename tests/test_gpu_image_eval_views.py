"""vdn_train.image_eval.evaluate_view / evaluate_images end to end on the synthetic rig: three 24 x 32 views with disc masks, the
shipped networks with synthetic weights, fp32 and bf16. Level 1 is 768 rays (one full 512-ray batch and a ragged one), level 2 is
12 x 16 (the resize path, still one whole SSIM window per side).

With the same injected jitter the render is bit-reproducible between calls (test_gpu_parity.py holds val_img's image to direct
render() calls bit for bit), so evaluate_view's figures are held to validate.val_img's (float32 sums on the host: rtol 1e-5) and to
the float64 model applied to the very image val_img returns (tests/test_gpu_image_eval.py's tolerances)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_model as im  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N, BS, CAR, SEED = 24, 32, 3, 512, 0.8, 11


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def rig(request):
    from vdn_train import synth, factory
    from vdn_train.rays import RaysGenerator
    dev = torch.device("cuda:0")
    K = np.eye(4)
    K[:3, :3] = [[30.0, 0, (W - 1) / 2.0], [0, 30.0, (H - 1) / 2.0], [0, 0, 1]]
    images = synth.uniform(SEED, "views/images", (N, H, W, 3)).astype(np.float32)
    masks = np.stack([im.make_mask("disc", H, W) for _ in range(N)])
    gen = RaysGenerator(images, masks, synth.make_cameras(SEED)[:N], K, device=dev)
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(SEED), precision=request.param)

    def jitter(idx, level):
        n = (H // level) * (W // level)
        out = []
        for b, s in enumerate(range(0, n, BS)):
            t1, t2 = synth.jitter(SEED, 100 * idx + 10 * level + b, min(BS, n - s))
            out.append((torch.from_numpy(t1).to(dev), torch.from_numpy(t2).to(dev)))
        return out
    return rend, gen, jitter


@pytest.mark.parametrize("level", [1, 2])
def test_view_matches_val_img_and_the_model(rig, level):
    from vdn_train import image_eval, validate
    rend, gen, jitter = rig
    idx = 1
    jit = jitter(idx, level)
    assert len(jit) == (2 if level == 1 else 1)
    ev = image_eval.evaluate_view(rend, gen, idx, resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR, jitter=jit, ssim_map=True)
    l1, psnr, eik, img = validate.val_img(rend, None, gen, idx, resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR, jitter=jit)
    l1m, psnrm, _, img_m = validate.val_img(rend, None, gen, idx, resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR,
                                            use_mask=True, jitter=jit)
    assert np.array_equal(img, img_m) and img.shape == (H // level, W // level, 3) and img.dtype == np.float32
    print("level", level, "evaluate_view", {k: v for k, v in ev.items() if k != "ssim_map"}, "val_img", (l1, psnr, l1m, psnrm))
    # validate.val_img: the same figures from float32 sums on the host
    assert math.isclose(ev["l1"], l1, rel_tol=1e-5) and math.isclose(ev["psnr"], psnr, rel_tol=1e-5)
    assert math.isclose(ev["l1_masked"], l1m, rel_tol=1e-5) and math.isclose(ev["psnr_masked"], psnrm, rel_tol=1e-5)
    assert math.isclose(ev["gradient_error"], float(eik.astype(np.float64).mean()), rel_tol=1e-6) and eik.shape == (len(jit),)
    # the device-side ground truth is image_at's / mask_at's, bit for bit
    gt = gen.image_at_device(idx, resolution_level=level)
    mask = gen.mask_at_device(idx, resolution_level=level)
    assert gt.is_cuda and gt.is_contiguous() and mask.is_cuda and mask.is_contiguous()
    gt, mask = gt.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal((gt * 255).clip(0, 255), gen.image_at(idx, resolution_level=level))
    assert np.array_equal(mask, gen.mask_at(idx, resolution_level=level)) and mask.shape == (H // level, W // level, 1)
    assert np.abs(mask - 0.1).min() > 0.05
    # the float64 model on the image val_img returned
    want, wmap = im.image_stats(img, gt, mask)
    wf = im.figures(want)
    w32 = wmap.astype(np.float32)
    err = np.abs(ev["ssim_map"].astype(np.float64) - w32.astype(np.float64))
    print("map: max err %.3g" % err.max())
    assert ev["ssim_map"].shape == wmap.shape and np.all(err <= 1e-9 + np.spacing(np.abs(w32)).astype(np.float64))
    for k in ("l1", "l1_masked", "ssim", "ssim_masked"):
        assert abs(ev[k] - wf[k]) <= 1e-9 * abs(wf[k]), (k, ev[k], wf[k])
    for k in ("psnr", "psnr_masked"):
        assert abs(ev[k] - wf[k]) <= 1e-7, (k, ev[k], wf[k])
    for k in ("n_pixels", "n_mask", "n_valid", "n_valid_masked"):
        assert ev[k] == wf[k], k
    # (at level 2 all 2 x 6 window centres lie inside the disc)
    assert 0 < ev["n_mask"] < ev["n_pixels"] and 0 < ev["n_valid_masked"] <= ev["n_valid"] and ev["idx"] == idx
    assert level == 2 or ev["n_valid_masked"] < ev["n_valid"]


def same(a, b):
    assert a.keys() == b.keys()
    for key, v in a.items():
        assert math.isclose(v, b[key], rel_tol=1e-14), key


def test_all_views_means_and_selection(rig):
    from vdn_train import image_eval
    rend, gen, jitter = rig
    level = 2
    jits = [jitter(i, level) for i in range(N)]
    res = image_eval.evaluate_images(rend, gen, resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR, jitter=jits)
    assert res["n_images"] == N and [d["idx"] for d in res["images"]] == [0, 1, 2] and res["resolution_level"] == level
    for key in image_eval.FIGURES:
        vals = [d[key] for d in res["images"]]
        assert all(math.isfinite(v) for v in vals), key
        assert math.isclose(res["mean"][key], float(np.mean(vals)), rel_tol=1e-14), key
    # each entry is evaluate_view's (the same result vector; finish on a stack may round its last bit differently than on one vector)
    for i in range(N):
        one = image_eval.evaluate_view(rend, gen, i, resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR, jitter=jits[i])
        same(one, res["images"][i])
    sel = image_eval.evaluate_images(rend, gen, indices=[2, 0], resolution_level=level, batch_size=BS, cos_anneal_ratio=CAR,
                                     jitter=[jits[2], jits[0]])
    assert sel["n_images"] == 2
    same(sel["images"][0], res["images"][2])
    same(sel["images"][1], res["images"][0])
    assert math.isclose(sel["mean"]["psnr"], (res["images"][2]["psnr"] + res["images"][0]["psnr"]) / 2, rel_tol=1e-14)
    for bad in ([3], [-1], []):
        with pytest.raises(ValueError):
            image_eval.evaluate_images(rend, gen, indices=bad, resolution_level=level)
    # without injected jitter (render()'s own draws): the default path, all views
    torch.manual_seed(3)
    free = image_eval.evaluate_images(rend, gen, resolution_level=level, cos_anneal_ratio=CAR)
    assert free["n_images"] == N and all(math.isfinite(free["mean"][k]) for k in image_eval.FIGURES)
    line = image_eval.to_json(free)
    assert "\n" not in line and '"mean"' in line


def test_cli_scene_mode_equals_the_api(tmp_path, capsys):
    """tools/eval_images.py --scene --checkpoint: scene files and a checkpoint file on disk -> the JSON line of evaluate_images over the
    same scene, weights and device random state (render() draws its jitter from the device generator; nothing else in either path does)."""
    import importlib.util
    import json
    from PIL import Image
    from vdn_train import dataset, factory, image_eval, synth
    spec = importlib.util.spec_from_file_location("eval_images_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                   "tools", "eval_images.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    dev = torch.device("cuda:0")
    n, root = 2, str(tmp_path / "scene")
    os.makedirs(os.path.join(root, "image", "mask"))
    cams = synth.make_cameras(SEED)[:n]
    K4 = np.eye(4)
    K4[:3, :3] = [[30.0, 0, (W - 1) / 2.0], [0, 30.0, (H - 1) / 2.0], [0, 0, 1]]
    names = ["%03d" % i for i in range(n)]
    dataset.write_cameras_npz(os.path.join(root, "cameras_sphere.npz"), names, [K4 @ np.linalg.inv(c) for c in cams], [np.eye(4)] * n)
    g = im.rng_of("views/cli")
    disc = (im.make_mask("disc", H, W)[..., 0] * 255).astype(np.uint8)
    for nm in names:
        Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB").save(os.path.join(root, "image", nm + ".png"))
        Image.fromarray(np.repeat(disc[:, :, None], 3, axis=2), "RGB").save(os.path.join(root, "image", "mask", nm + ".png"))
    states = synth.make_all_states(SEED)
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({k: {name: torch.from_numpy(np.ascontiguousarray(v)) for name, v in d.items()} for k, d in states.items() if d is not None}, ckpt)
    out = str(tmp_path / "out" / "images.json")
    torch.manual_seed(5)
    res = tool.main(["--scene", root, "--checkpoint", ckpt, "--resolution-level", "2", "--indices", "1", "--precision", "fp32", "--out", out])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == json.loads(open(out).read()) and json.loads(line)["images"][0]["name"] == "001"
    assert res["n_images"] == 1 and res["images"][0]["idx"] == 1 and res["images"][0]["name"] == "001"
    gen = dataset.SceneData(root).rays_generator(dev)
    rend = factory.build_renderer(device=dev, states=states, precision="fp32")
    torch.manual_seed(5)
    want = image_eval.evaluate_images(rend, gen, indices=[1], resolution_level=2)
    got = dict(res["images"][0])
    got.pop("name")
    same(got, want["images"][0])
    assert 0 < got["n_mask"] < got["n_pixels"] == (H // 2) * (W // 2) and math.isfinite(got["ssim"])
