"""The float64 numpy model of the image evaluation (include/vdn_render.h: vdn_image_stats; INTEGRATION.md "Image evaluation"):
the valid separable Gaussian convolution, the per-channel SSIM map S, and every entry of the result vector - what
csrc/image_eval.hip is held to. A plain module (no tests, no fixtures), shared by test_image_eval_cpu.py, test_gpu_image_eval.py and
test_gpu_image_eval_views.py. Inputs are widened from float32 first: every product of two inputs is then exact, only sums round."""
import numpy as np

R = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps():
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def valid_filter(img):
    """[H,W,...] float64 -> [H-10,W-10,...]: the 11-tap window along x, then along y, each an in-order sum; no padding."""
    g = taps()
    H, W = img.shape[:2]
    h = np.zeros((H, W - 2 * R) + img.shape[2:], dtype=np.float64)
    for k in range(2 * R + 1):
        h += g[k] * img[:, k:k + W - 2 * R]
    v = np.zeros((H - 2 * R, W - 2 * R) + img.shape[2:], dtype=np.float64)
    for k in range(2 * R + 1):
        v += g[k] * h[k:k + H - 2 * R]
    return v


def s_from_moments(mx, my, xx, yy, xy):
    """S of the five filtered moments, in the kernel's expression: x == y gives exactly 1."""
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx, vy, vxy = xx - mxx, yy - myy, xy - mxy
    return ((2.0 * mxy + C1) * (2.0 * vxy + C2)) / (((mxx + myy) + C1) * ((vx + vy) + C2))


def ssim_channels(pred, gt):
    """-> S [H-10,W-10,3] float64."""
    x, y = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    return s_from_moments(valid_filter(x), valid_filter(y), valid_filter(x * x), valid_filter(y * y), valid_filter(x * y))


def in_mask(mask, shape):
    """[H,W] bool: mask > 0.1 on the first channel; every pixel without a mask."""
    if mask is None:
        return np.ones(shape[:2], dtype=bool)
    return np.asarray(mask, dtype=np.float64)[..., 0] > 0.1


def image_stats(pred, gt, mask=None):
    """-> (result vector [10] float64 in the kernel's layout, map [H-10,W-10] float64 of the channel-mean S)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == gt.shape and pred.shape[2] == 3
    H, W = pred.shape[:2]
    m = in_mask(mask, pred.shape)
    e = pred.astype(np.float64) - gt.astype(np.float64)
    a, s = np.abs(e).sum(axis=2), (e * e).sum(axis=2)
    S = ssim_channels(pred, gt)
    s3 = (S[..., 0] + S[..., 1]) + S[..., 2]
    mc = m[R:H - R, R:W - R]
    r = np.array([m.sum(), a[m].sum(), s[m].sum(), a.sum(), s.sum(), s3.sum(), s3.size, s3[mc].sum(), mc.sum(), H * W], dtype=np.float64)
    return r, s3 / 3.0


def figures(r):
    """The figures of one result vector, straight from the definitions (an independent restatement of vdn_hip.image.finish)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"n_mask": int(r[0]), "n_pixels": int(r[9]), "n_valid": int(r[6]), "n_valid_masked": int(r[8])}
        for tag, n, sa, sq in (("", r[9], r[3], r[4]), ("_masked", r[0], r[1], r[2])):
            ms = n + 1e-5
            out["l1" + tag] = float(sa / ms)
            out["psnr" + tag] = float(20.0 * np.log10(1.0 / np.sqrt(sq / (3.0 * ms))))
        out["ssim"] = float(np.float64(r[5]) / (3.0 * r[6]))
        out["ssim_masked"] = float(np.float64(r[7]) / (3.0 * np.float64(r[8])))
    return out


# ---- seeded inputs, named by the case ---------------------------------------------------------------------------------------------
def rng_of(name):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_pair(kind, H, W, name):
    """-> (pred, gt) float32 [H,W,3] in [0,1] of one of the contents the issue names."""
    g = rng_of(name + "/" + kind)
    if kind == "noise":
        x = g.random((H, W, 3))
        y = np.clip(x + 0.1 * g.standard_normal((H, W, 3)), 0.0, 1.0)
    elif kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        x = np.stack([0.5 + 0.4 * np.sin(0.13 * xx + 0.07 * yy + c) * np.cos(0.05 * yy - 0.3 * c) for c in range(3)], axis=-1)
        y = 0.97 * x + 0.01
    elif kind == "bright_flat":
        x = np.ones((H, W, 3))
        y = 1.0 - 0.002 * g.random((H, W, 3))
    elif kind == "zeros":
        x = np.zeros((H, W, 3))
        y = np.zeros((H, W, 3))
    elif kind == "identical":
        x = g.random((H, W, 3))
        y = x
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


def make_mask(kind, H, W, channels=1):
    """-> float32 [H,W,channels] of {0, 1}, or None."""
    if kind == "none":
        return None
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "disc":
        m = (yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2 <= (0.35 * min(H, W)) ** 2
    elif kind == "empty":
        m = np.zeros((H, W), dtype=bool)
    elif kind == "full":
        m = np.ones((H, W), dtype=bool)
    elif kind == "margin":
        # a frame whose inner edge is the last pixel row / column of the 5-pixel margin: it touches the valid region from outside on
        # three sides and reaches one pixel into it on the fourth
        m = np.ones((H, W), dtype=bool)
        m[R:H - R, R:W - R - 1] = False
    else:
        raise ValueError(kind)
    out = np.zeros((H, W, channels), dtype=np.float32)
    out[..., 0] = m
    if channels > 1:
        out[..., 1:] = 1.0 - out[..., :1]               # the other channels must not matter
    return out
