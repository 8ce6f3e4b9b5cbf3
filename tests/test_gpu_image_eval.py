"""vdn_image_stats (csrc/image_eval.hip) against the float64 model of tests/image_model.py: every pixel of the SSIM map and every
entry of the result vector, nothing excluded.

Tolerances (derived, not measured): both sides work in double on the same float32 inputs and every product of two inputs is exact,
so they differ only by the rounding of the 11-term and 121-term sums, at most about 50 * 2^-53 = 6e-15 per moment; S divides that
by factors no smaller than C1 = 1e-4: about 6e-11 on S. Map: 1e-9 absolute against the model rounded to float32, plus one float32
ulp (the kernel rounds its own double once); sums: rtol 1e-9; PSNR: 1e-7 dB; counts: exact.
Shapes: 11 x 11 (one window), 11 x 70 (one valid row, two tiles across), 45 x 12 (two valid columns, three tiles down), 37 x 53
(ragged both ways, 2 x 2 tiles), 75 x 83 (5 x 3 tiles of 16 x 32 centres, ragged last tiles), 256 x 256 (128 tiles: the second
launch's lanes take two tiles each)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_model as im  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS, SUMS = (0, 6, 8, 9), (1, 2, 3, 4, 5, 7)
SHAPES = [(11, 11), (11, 70), (45, 12), (37, 53), (75, 83), (256, 256)]
CONTENTS = ["noise", "smooth", "bright_flat", "zeros", "identical"]
MASKS = ["none", "disc", "empty", "full", "margin"]


def dev_of(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


def run(pred, gt, mask):
    """-> (result vector, map) as numpy, having checked that the call without a map gives the same vector bit for bit."""
    from vdn_hip import image
    p, g, m = dev_of(pred), dev_of(gt), dev_of(mask)
    r, smap = image.image_stats(p, g, m, ssim_map=True)
    r2 = image.image_stats(p, g, m)
    assert r.dtype == torch.float64 and r.shape == (10,) and r.device.type == "cuda"
    assert smap.dtype == torch.float32 and smap.shape == (pred.shape[0] - 10, pred.shape[1] - 10)
    assert torch.equal(r.view(torch.int64), r2.view(torch.int64))
    return r.cpu().numpy(), smap.cpu().numpy()


def check(pred, gt, mask, tag):
    from vdn_hip import image
    if mask is not None:
        assert np.abs(mask - 0.1).min() > 0.05                       # no value near the threshold
    r, smap = run(pred, gt, mask)
    want, wmap = im.image_stats(pred, gt, mask)
    w32 = wmap.astype(np.float32)
    err = np.abs(smap.astype(np.float64) - w32.astype(np.float64))
    print(tag, "map: max err %.3g (vs the float64 model %.3g)" % (err.max(), np.abs(smap - wmap).max()),
          "sums: worst rel %.3g" % max(abs(r[i] - want[i]) / abs(want[i]) if want[i] != 0 else abs(r[i]) for i in SUMS))
    assert np.all(err <= 1e-9 + np.spacing(np.abs(w32)).astype(np.float64)), tag
    for i in COUNTS:
        assert r[i] == want[i], (tag, i, r[i], want[i])
    for i in SUMS:
        assert abs(r[i] - want[i]) <= 1e-9 * abs(want[i]), (tag, i, r[i], want[i])
    f, wf = image.finish(r), im.figures(want)
    for k in ("psnr", "psnr_masked"):
        assert f[k] == wf[k] or abs(f[k] - wf[k]) <= 1e-7, (tag, k, f[k], wf[k])
    for k in ("l1", "l1_masked", "ssim", "ssim_masked"):
        assert (math.isnan(f[k]) and math.isnan(wf[k])) or abs(f[k] - wf[k]) <= 1e-9 * abs(wf[k]), (tag, k, f[k], wf[k])
    for k in ("n_pixels", "n_mask", "n_valid", "n_valid_masked"):
        assert f[k] == wf[k], (tag, k)
    return r, smap, f


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape(shape):
    H, W = shape
    name = "gpu/shape/%dx%d" % shape
    pred, gt = im.make_pair("noise", H, W, name)
    check(pred, gt, None, name + "/none")
    check(pred, gt, im.make_mask("disc", H, W), name + "/disc")


@pytest.mark.parametrize("shape", [(37, 53), (75, 83)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", CONTENTS)
def test_every_content(kind, shape):
    H, W = shape
    name = "gpu/content/%dx%d" % shape
    pred, gt = im.make_pair(kind, H, W, name)
    for mk in ("none", "disc"):
        r, smap, f = check(pred, gt, im.make_mask(mk, H, W), "%s/%s/%s" % (name, kind, mk))
        if kind in ("identical", "zeros"):
            # exact: x == y makes numerator and denominator the same bits
            assert np.all(smap == 1.0) and f["ssim"] == 1.0 and f["ssim_masked"] == 1.0
            assert f["l1"] == 0.0 and f["psnr"] == math.inf and f["l1_masked"] == 0.0 and f["psnr_masked"] == math.inf


@pytest.mark.parametrize("shape", [(37, 53), (75, 83)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mask_kind", MASKS)
def test_every_mask(mask_kind, shape):
    H, W = shape
    name = "gpu/mask/%dx%d" % shape
    pred, gt = im.make_pair("noise", H, W, name)
    r, _, f = check(pred, gt, im.make_mask(mask_kind, H, W), name + "/" + mask_kind)
    if mask_kind != "none":
        r3, _, _ = check(pred, gt, im.make_mask(mask_kind, H, W, channels=3), name + "/" + mask_kind + "/3ch")
        assert np.array_equal(r3.view(np.int64), r.view(np.int64))           # only the first channel is read
    if mask_kind == "empty":
        assert f["n_mask"] == 0 and f["l1_masked"] == 0.0 and math.isnan(f["ssim_masked"]) and f["n_valid_masked"] == 0
        assert r[1] == 0.0 and r[2] == 0.0 and r[7] == 0.0
    if mask_kind in ("none", "full"):
        # the masked and the unmasked figures are the same sums in the same order: equal bit for bit
        assert r[0] == r[9] and r[8] == r[6]
        assert r[1:3].tobytes() == r[3:5].tobytes() and r[7:8].tobytes() == r[5:6].tobytes()
        assert f["l1"] == f["l1_masked"] and f["psnr"] == f["psnr_masked"] and f["ssim"] == f["ssim_masked"]
    if mask_kind == "margin":
        assert f["n_mask"] == H * W - (H - 10) * (W - 11) and f["n_valid_masked"] == H - 10


def test_two_calls_give_the_same_bits():
    from vdn_hip import image
    for H, W in ((75, 83), (256, 256)):
        name = "gpu/repro/%dx%d" % (H, W)
        pred, gt = im.make_pair("noise", H, W, name)
        p, g, m = dev_of(pred), dev_of(gt), dev_of(im.make_mask("disc", H, W))
        r0, s0 = image.image_stats(p, g, m, ssim_map=True)
        for _ in range(3):
            r1, s1 = image.image_stats(p, g, m, ssim_map=True)
            assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


def test_non_contiguous_inputs_and_the_front_door():
    """image_stats takes strided views (it makes them contiguous); evaluate_image takes numpy arrays and gives finish's dict."""
    from vdn_hip import image
    from vdn_train import image_eval
    H, W = 37, 53
    pred, gt = im.make_pair("smooth", H, W, "gpu/door")
    mask = im.make_mask("disc", H, W)
    want = image.finish(image.image_stats(dev_of(pred), dev_of(gt), dev_of(mask)).cpu())
    wide = torch.zeros(H, W, 6, device=DEV)
    wide[..., ::2] = dev_of(pred)
    got = image.finish(image.image_stats(wide[..., ::2], dev_of(gt), dev_of(mask)).cpu())
    assert got == want
    res = image_eval.evaluate_image(pred, gt, mask, ssim_map=True)
    smap = res.pop("ssim_map")
    assert res == want and smap.shape == (H - 10, W - 10)
    assert image_eval.evaluate_image(torch.from_numpy(pred), dev_of(gt), mask) == want
