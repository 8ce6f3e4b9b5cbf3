"""Image evaluation on the device (csrc/image_eval.hip): the sums behind L1, PSNR and SSIM of a rendered image
against its ground truth, over a mask and over every pixel, from one launch pair on torch's current stream. image_stats leaves
its result vector on the device; finish turns result vectors that have reached the host into the figures."""
import numpy as np
import torch

from . import lib

RESULT_LEN = 10             # include/vdn_render.h: VdnImageStatsArgs.result
WINDOW = 11                 # taps of the SSIM window; an image must hold one whole window
# result vector entries
N_MASK, ABS_MASKED, SQ_MASKED, ABS_ALL, SQ_ALL, SSIM_SUM, N_VALID, SSIM_SUM_MASKED, N_VALID_MASKED, N_PIXELS = range(RESULT_LEN)


def check_images(pred, gt, mask=None):
    """ValueError, naming the offending shape, unless pred and gt are [H,W,3] with H, W >= 11 and mask (if any) [H,W,1|3]."""
    ps, gs = tuple(pred.shape), tuple(gt.shape)
    if len(ps) != 3 or ps[2] != 3:
        raise ValueError("pred must be [H,W,3], got %r" % (ps,))
    if gs != ps:
        raise ValueError("gt must have pred's shape %r, got %r" % (ps, gs))
    if ps[0] < WINDOW or ps[1] < WINDOW:
        raise ValueError("an image must hold one %d x %d SSIM window, got %r" % (WINDOW, WINDOW, ps))
    if mask is not None:
        ms = tuple(mask.shape)
        if len(ms) != 3 or ms[:2] != ps[:2] or ms[2] not in (1, 3):
            raise ValueError("mask must be [%d,%d,1] or [%d,%d,3], got %r" % (ps[0], ps[1], ps[0], ps[1], ms))


def image_stats(pred, gt, mask=None, ssim_map=False):
    """pred, gt [H,W,3], mask [H,W,1|3] or None: float32 tensors on one device -> the float64 [10] result vector of
    vdn_image_stats on that device, or (result vector, float32 [H-10,W-10] map of the channel-mean SSIM) with ssim_map.
    Nothing is read back to the host."""
    tensors = [("pred", pred), ("gt", gt)] + ([("mask", mask)] if mask is not None else [])
    for name, t in tensors:
        if not torch.is_tensor(t):
            raise ValueError("%s must be a torch tensor, got %s" % (name, type(t).__name__))
    check_images(pred, gt, mask)
    for name, t in tensors:
        if t.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s (shape %r)" % (name, t.dtype, tuple(t.shape)))
        if t.device.type != "cuda":
            raise ValueError("%s must be on the device, got %s (shape %r)" % (name, t.device, tuple(t.shape)))
        if t.device != pred.device:
            raise ValueError("%s is on %s, pred on %s" % (name, t.device, pred.device))
    H, W = int(pred.shape[0]), int(pred.shape[1])
    tiles = lib.call_value("vdn_image_stats_tiles", H, W)
    if tiles < 1:
        raise ValueError("image shape %r is beyond 32-bit indexing" % (tuple(pred.shape),))
    dev = pred.device
    pred, gt = pred.detach().contiguous(), gt.detach().contiguous()
    mask = None if mask is None else mask.detach().contiguous()
    with torch.cuda.device(dev):
        partials = torch.empty(tiles, 9, dtype=torch.float64, device=dev)
        result = torch.empty(RESULT_LEN, dtype=torch.float64, device=dev)
        smap = torch.empty(H - WINDOW + 1, W - WINDOW + 1, dtype=torch.float32, device=dev) if ssim_map else None
        a = lib.VdnImageStatsArgs()
        a.pred, a.gt, a.partials, a.result = pred.data_ptr(), gt.data_ptr(), partials.data_ptr(), result.data_ptr()
        if mask is not None:
            a.mask, a.mask_ch = mask.data_ptr(), int(mask.shape[2])
        if smap is not None:
            a.ssim_map = smap.data_ptr()
        a.partials_rows, a.H, a.W = tiles, H, W
        # (the workspace and any contiguous copy were allocated on this stream: the allocator hands them on in stream order)
        lib.call("vdn_image_stats", a, lib.stream_handle())
    return (result, smap) if ssim_map else result


def finish(result_vector):
    """One result vector [10], or a stack [..., 10], on the host (array or CPU tensor) -> dict of l1, psnr, l1_masked, psnr_masked,
    ssim, ssim_masked, n_pixels, n_mask, n_valid, n_valid_masked: Python numbers for one vector, arrays of the stack's shape
    otherwise. l1 is summed over the three channels and not divided by 3, mask_sum = count + 1e-5, as the reference has them;
    identical images give psnr = inf, an empty mask ssim_masked = nan."""
    if torch.is_tensor(result_vector):
        if result_vector.device.type != "cpu":
            raise ValueError("finish takes result vectors that are on the host: copy the stack back once, then call it")
        result_vector = result_vector.numpy()
    r = np.asarray(result_vector, dtype=np.float64)
    if r.ndim < 1 or r.shape[-1] != RESULT_LEN:
        raise ValueError("a result vector has %d entries, got shape %r" % (RESULT_LEN, r.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        def pair(n, s_abs, s_sq):
            mask_sum = n + 1e-5
            return s_abs / mask_sum, 20.0 * np.log10(1.0 / np.sqrt(s_sq / (3.0 * mask_sum)))
        l1, psnr = pair(r[..., N_PIXELS], r[..., ABS_ALL], r[..., SQ_ALL])
        l1_m, psnr_m = pair(r[..., N_MASK], r[..., ABS_MASKED], r[..., SQ_MASKED])
        ssim = r[..., SSIM_SUM] / (3.0 * r[..., N_VALID])
        ssim_m = r[..., SSIM_SUM_MASKED] / (3.0 * r[..., N_VALID_MASKED])
    out = {"l1": l1, "psnr": psnr, "l1_masked": l1_m, "psnr_masked": psnr_m, "ssim": ssim, "ssim_masked": ssim_m}
    counts = {"n_pixels": r[..., N_PIXELS], "n_mask": r[..., N_MASK], "n_valid": r[..., N_VALID], "n_valid_masked": r[..., N_VALID_MASKED]}
    if r.ndim == 1:
        out = {k: float(v) for k, v in out.items()}
        out.update((k, int(v)) for k, v in counts.items())
    else:
        out.update((k, v.astype(np.int64)) for k, v in counts.items())
    return out
