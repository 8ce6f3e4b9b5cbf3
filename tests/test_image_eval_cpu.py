"""Image evaluation without a device: the float64 model (tests/image_model.py) against an independent scipy formulation and against
validate.image_metrics, the header / ABI of vdn_image_stats, the argument errors of every layer, vdn_hip.image.finish on hand-made
result vectors, and the folder mode of tools/eval_images.py with the device call replaced by the model."""
import ctypes
import importlib.util
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_model as im  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("eval_images_tool", os.path.join(ROOT, "tools", "eval_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "smooth", "bright_flat"])
def test_model_matches_a_scipy_formulation(kind):
    """gaussian_filter(sigma=1.5, truncate=3.5) has radius int(3.5 * 1.5 + 0.5) = 5: the same 11 normalised taps; away from the border
    (crop 5) the reflect mode does not show. Tolerance 1e-10 absolute on the map (observed: 4e-15 noise, 2e-13 smooth, 1.1e-12 bright flat)."""
    from scipy.ndimage import gaussian_filter
    x, y = im.make_pair(kind, 37, 53, "cpu/scipy")
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: np.stack([gaussian_filter(a[..., c], sigma=1.5, truncate=3.5, mode="reflect") for c in range(3)], axis=-1)[5:-5, 5:-5]
    mx, my = f(xd), f(yd)
    vx, vy, vxy = f(xd * xd) - mx * mx, f(yd * yd) - my * my, f(xd * yd) - mx * my
    S = (2 * mx * my + im.C1) * (2 * vxy + im.C2) / ((mx * mx + my * my + im.C1) * (vx + vy + im.C2))
    got = im.ssim_channels(x, y)
    assert got.shape == (27, 43, 3)
    err = float(np.abs(got - S).max())
    print(kind, "model vs scipy: max |dS| =", err)
    assert err <= 1e-10
    r, smap = im.image_stats(x, y)
    assert abs(smap - S.mean(axis=2)).max() <= 1e-10
    assert r[6] == 27 * 43 and r[9] == 37 * 53 and r[0] == r[9] and r[8] == r[6]
    assert math.isclose(im.figures(r)["ssim"], S.mean(), rel_tol=0, abs_tol=1e-10)


def test_model_taps_and_exact_identity():
    g = im.taps()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])
    assert math.isclose(g[5] / g[4], math.exp(1.0 / 4.5), rel_tol=1e-14)
    x, _ = im.make_pair("identical", 23, 31, "cpu/identity")
    r, smap = im.image_stats(x, x)
    assert np.all(smap == 1.0) and r[5] == 3.0 * r[6]
    f = im.figures(r)
    assert f["ssim"] == 1.0 and f["l1"] == 0.0 and f["psnr"] == math.inf


@pytest.mark.parametrize("mask_kind", ["none", "disc"])
def test_model_l1_psnr_match_image_metrics(mask_kind):
    """validate.image_metrics sums in float32: rtol 1e-5."""
    from vdn_train import validate
    x, y = im.make_pair("noise", 37, 53, "cpu/metrics")
    mask = im.make_mask(mask_kind, 37, 53)
    l1, psnr = validate.image_metrics(x, y, mask)
    f = im.figures(im.image_stats(x, y, mask)[0])
    assert math.isclose(f["l1_masked"], l1, rel_tol=1e-5) and math.isclose(f["psnr_masked"], psnr, rel_tol=1e-5)
    l1a, psnra = validate.image_metrics(x, y, None)
    assert math.isclose(f["l1"], l1a, rel_tol=1e-5) and math.isclose(f["psnr"], psnra, rel_tol=1e-5)
    if mask_kind == "none":
        assert f["l1"] == f["l1_masked"] and f["psnr"] == f["psnr_masked"] and f["ssim"] == f["ssim_masked"]
    else:
        assert 0 < f["n_mask"] < f["n_pixels"] and 0 < f["n_valid_masked"] < f["n_valid"]


def test_masks_are_far_from_the_threshold():
    for kind in ("disc", "empty", "full", "margin"):
        for ch in (1, 3):
            m = im.make_mask(kind, 37, 53, ch)
            assert m.dtype == np.float32 and m.shape == (37, 53, ch) and set(np.unique(m)) <= {0.0, 1.0}
    m = im.make_mask("margin", 37, 53)[..., 0] > 0.1
    assert m[:5].all() and m[-5:].all() and m[:, :5].all() and m[:, -5:].all()          # the whole 5-pixel margin
    assert not m[5:-5, 5:-6].any() and m[5:-5, -6].all()                                # and one column of window centres


# ---- header and ABI -----------------------------------------------------------------------------------------------------------
def test_library_declares_and_exports_the_image_entry_point():
    from vdn_hip import build, lib
    assert len(lib.FUNCTIONS["vdn_image_stats"]) == 2 and len(lib.FUNCTIONS["vdn_image_stats_tiles"]) == 2
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28
    assert build.PER_FILE_FLAGS["image_eval.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(build.CSRC, "image_eval.hip"))
    a = lib.STRUCTS["VdnImageStatsArgs"]
    # C's layout: six pointers, one int64, four int32
    assert ctypes.sizeof(a) == 6 * 8 + 8 + 4 * 4
    assert a.result.offset == 32 and a.partials_rows.offset == 48 and a.H.offset == 56 and a.mask_ch.offset == 64
    l = lib.load()                                       # (raises where the library is not built: there is no other path)
    assert hasattr(l, "vdn_image_stats") and hasattr(l, "vdn_image_stats_tiles")
    assert lib.call_value("vdn_abi_version") == 28
    # tiles of 16 x 32 window centres
    assert lib.call_value("vdn_image_stats_tiles", 11, 11) == 1
    assert lib.call_value("vdn_image_stats_tiles", 75, 83) == 5 * 3
    assert lib.call_value("vdn_image_stats_tiles", 10, 83) == 0 and lib.call_value("vdn_image_stats_tiles", 83, 10) == 0


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_entry_point_rejects_an_empty_block():
    from vdn_hip import lib
    with pytest.raises(lib.VdnError):
        lib.call("vdn_image_stats", lib.VdnImageStatsArgs(), None)
    a = lib.VdnImageStatsArgs()
    a.pred = a.gt = a.result = a.partials = 8            # never dereferenced: the shape is refused first
    a.partials_rows = 1
    for H, W in ((10, 11), (11, 10)):
        a.H, a.W = H, W
        with pytest.raises(lib.VdnError):
            lib.call("vdn_image_stats", a, None)


def test_python_layers_reject_bad_arguments():
    from vdn_hip import image
    from vdn_train import image_eval
    z = lambda *s: torch.zeros(*s)
    bad = [(z(10, 20, 3), z(10, 20, 3), None), (z(20, 10, 3), z(20, 10, 3), None), (z(12, 12, 3), z(12, 13, 3), None),
           (z(12, 12, 3), z(12, 12, 3), z(12, 13, 1)), (z(12, 12, 3), z(12, 12, 3), z(12, 12, 2)), (z(12, 12, 4), z(12, 12, 4), None),
           (z(12, 12, 3).double(), z(12, 12, 3).double(), None), (z(12, 12, 3), z(12, 12, 3).half(), None)]
    for p, g, m in bad:
        for fn in (image.image_stats, image_eval.evaluate_image):
            with pytest.raises(ValueError):
                fn(p, g, m)
        with pytest.raises(ValueError):
            image_eval.evaluate_image(p.numpy(), g.numpy(), None if m is None else m.numpy())
    with pytest.raises(ValueError, match=r"\(10, 20, 3\)"):                  # the offending shape is named
        image.image_stats(z(10, 20, 3), z(10, 20, 3))
    with pytest.raises(ValueError, match="on the device"):
        image.image_stats(z(12, 12, 3), z(12, 12, 3))
    with pytest.raises(ValueError):
        image.image_stats(z(12, 12, 3).numpy(), z(12, 12, 3).numpy())


# ---- result vectors ---------------------------------------------------------------------------------------------------------------
def test_finish_on_hand_made_result_vectors():
    from vdn_hip import image
    #            n_mask  |e|m  e2m   |e|   e2    S     nv    Sm    nvm   HW
    v = np.array([50.0, 5.0, 0.75, 12.0, 3.0, 540.0, 200.0, 81.0, 30.0, 400.0])
    f = image.finish(v)
    assert f == image.finish(torch.from_numpy(v)) and f.keys() == im.figures(v).keys()
    assert (f["n_pixels"], f["n_mask"], f["n_valid"], f["n_valid_masked"]) == (400, 50, 200, 30) and isinstance(f["n_mask"], int)
    assert f["l1"] == 12.0 / (400.0 + 1e-5) and f["l1_masked"] == 5.0 / (50.0 + 1e-5)
    assert math.isclose(f["psnr"], -10.0 * math.log10(3.0 / (3.0 * (400.0 + 1e-5))), rel_tol=1e-14)
    assert math.isclose(f["psnr_masked"], -10.0 * math.log10(0.75 / (3.0 * (50.0 + 1e-5))), rel_tol=1e-14)
    assert f["ssim"] == 540.0 / 600.0 and f["ssim_masked"] == 81.0 / 90.0
    for k, x in im.figures(v).items():
        assert f[k] == x, k
    empty = np.array([0.0, 0.0, 0.0, 12.0, 3.0, 540.0, 200.0, 0.0, 0.0, 400.0])
    f = image.finish(empty)
    assert f["n_mask"] == 0 and f["l1_masked"] == 0.0 and math.isnan(f["ssim_masked"]) and f["n_valid_masked"] == 0 and f["ssim"] == 0.9
    same = np.array([50.0, 0.0, 0.0, 0.0, 0.0, 600.0, 200.0, 90.0, 30.0, 400.0])
    f = image.finish(same)
    assert f["l1"] == 0.0 and f["psnr"] == math.inf and f["psnr_masked"] == math.inf and f["ssim"] == 1.0 and f["ssim_masked"] == 1.0
    st = image.finish(np.stack([v, empty, same]))
    assert st["psnr"].shape == (3,) and st["n_mask"].dtype == np.int64 and st["n_mask"].tolist() == [50, 0, 50]
    for k, row in enumerate((v, empty, same)):
        one = image.finish(row)
        for key, x in one.items():
            assert st[key][k] == x or (math.isnan(x) and math.isnan(st[key][k])), (key, k)
    assert image.finish(np.stack([v, same]).reshape(1, 2, 10))["ssim"].shape == (1, 2)
    with pytest.raises(ValueError):
        image.finish(np.zeros(9))
    from vdn_train import image_eval
    line = json.loads(image_eval.to_json({"images": [dict(image.finish(empty), idx=0, ssim_map=np.zeros((2, 2)))], "mean": image.finish(same)}))
    assert line["images"][0]["ssim_masked"] is None and "ssim_map" not in line["images"][0] and line["mean"]["psnr"] is None


# ---- the command-line tool, folder mode ---------------------------------------------------------------------------------------------
def test_cli_folder_mode_pairs_by_sorted_name(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from vdn_train import image_eval
    tool = _tool()
    g = im.rng_of("cpu/cli")
    names = ["b_002.png", "a_010.png", "c_001.png"]
    arrays = {}
    for d in ("pred", "gt", "mask"):
        os.makedirs(tmp_path / d)
    for n in names:
        gt = g.integers(0, 256, (13, 17, 3), dtype=np.uint8)
        pred = np.clip(gt.astype(np.int64) + g.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
        mask = (g.random((13, 17)) > 0.4).astype(np.uint8) * 255
        Image.fromarray(pred).save(tmp_path / "pred" / n)
        Image.fromarray(gt).save(tmp_path / "gt" / n)
        Image.fromarray(mask).save(tmp_path / "mask" / n)
        arrays[n] = (pred, gt, mask)
    (tmp_path / "pred" / "notes.txt").write_text("not an image")
    calls = []

    def model_evaluate(pred, gt, mask=None, ssim_map=False, device=None):
        calls.append((pred, gt, mask))
        return im.figures(im.image_stats(pred, gt, mask)[0])
    monkeypatch.setattr(image_eval, "evaluate_image", model_evaluate)
    out_file = tmp_path / "out" / "res.json"
    res = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--mask", str(tmp_path / "mask"), "--out", str(out_file)])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == json.loads(out_file.read_text())
    assert [d["pred"] for d in res["images"]] == sorted(names) and [d["gt"] for d in res["images"]] == sorted(names)
    assert res["n_images"] == 3 and len(calls) == 3
    for (pred, gt, mask), n in zip(calls, sorted(names)):
        p8, g8, m8 = arrays[n]
        assert pred.dtype == np.float32 and pred.shape == (13, 17, 3) and mask.shape == (13, 17, 1)
        assert np.array_equal(pred, p8.astype(np.float32) / np.float32(255)) and np.array_equal(gt, g8.astype(np.float32) / np.float32(255))
        assert np.array_equal(mask[..., 0] > 0.1, m8 > 0)
    for key in ("l1", "psnr", "l1_masked", "psnr_masked", "ssim", "ssim_masked"):
        assert math.isclose(res["mean"][key], np.mean([d[key] for d in res["images"]]), rel_tol=1e-15)
    # without masks; and the two modes exclude each other
    res2 = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt")])
    assert all(c[2] is None for c in calls[3:]) and res2["images"][0]["l1"] == res["images"][0]["l1"]
    os.remove(tmp_path / "gt" / names[0])
    with pytest.raises(SystemExit):
        tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt")])
    for argv in (["--pred", "x"], ["--pred", "x", "--gt", "y", "--scene", "z"], ["--scene", "z"], []):
        with pytest.raises(SystemExit):
            tool.main(argv)
