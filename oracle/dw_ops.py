"""Plain models of the parameter-update tail of the training step (include/vdn_render.h: vdn_dw_gemm_f32 / _bf16, vdn_dw_finalize,
vdn_weightnorm_materialize, vdn_weightnorm_bwd, vdn_adam_step / _ranges), parametrised by dtype: float64 is the reference of
tests/test_gpu_dw_tail.py, float32 its rounding floor. Nothing here is restated from a kernel: the weight-norm backward is autograd
of the forward, Adam is torch.optim.Adam's documented update (tests/test_dw_ops_model_cpu.py holds it to torch in float64).
"""
import numpy as np
import torch

F32_STAGE, BF16_STAGE = 32, 128        # rows a K split is rounded up to (csrc/train_dw_f32.hip, csrc/train_dw_bf16.hip)
ULP = 2.0 ** -24                       # half the spacing of float32 around 1: the unit every tolerance is expressed in


# ---- weight-gradient GEMM ---------------------------------------------------------------------------------------------------

def dw_gemm(segments, rows, dtype=np.float64):
    """segments: [(A [P,M], B [P,N] or None)] -> (sum_seg A[:rows].T @ B[:rows] as [M,N] or None, column sums of segment 1's A)."""
    prod = None
    for a, b in segments:
        if b is None:
            continue
        t = np.asarray(a[:rows], dtype).T @ np.asarray(b[:rows], dtype)
        prod = t if prod is None else prod + t
    return prod, np.asarray(segments[0][0][:rows], dtype).sum(0)


def dw_gemm_units(segments, rows):
    """The unit of one output element: 2^-24 sum_p |a_p b_p| (2^-24 sum_p |a_p| for the column sums)."""
    prod, cs = dw_gemm([(np.abs(a), None if b is None else np.abs(b)) for a, b in segments], rows)
    return (None if prod is None else ULP * prod), ULP * cs


def fma_chain_f32(a, b):
    """The float32 floor of a contraction: acc = float32(float64(acc) + float64(a_p) * float64(b_p)), row after row (the product
    of two float32 is exact in float64: one rounding per row, as a k-ordered fmaf chain). a [P,M], b [P,N] or None (column
    sums of a: b_p = 1) -> float32 [M,N] or [M]."""
    a = np.asarray(a, np.float64)
    if b is None:
        acc = np.zeros(a.shape[1], np.float32)
        for p in range(a.shape[0]):
            acc = (acc.astype(np.float64) + a[p]).astype(np.float32)
        return acc
    b = np.asarray(b, np.float64)
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for p in range(a.shape[0]):
        acc = (acc.astype(np.float64) + a[p][:, None] * b[p][None, :]).astype(np.float32)
    return acc


def dw_gemm_chain_f32(segments, rows):
    """dw_gemm as one float32 chain over the rows of segment 1, then segment 2."""
    seg = [(a[:rows], None if b is None else b[:rows]) for a, b in segments]
    prod = None
    if seg[0][1] is not None:
        prod = fma_chain_f32(np.concatenate([a for a, _ in seg]), np.concatenate([b for _, b in seg]))
    return prod, fma_chain_f32(seg[0][0], None)


def split_ranges(P, splits, two_segments, stage):
    """-> [(segment, k_begin, k_end)] per split, k_end <= k_begin for a split that gets no rows. With two segments the first half
    of the splits contracts segment 1 (include/vdn_render.h: VdnDwDesc); a segment's rows are dealt in equal shares rounded up
    to `stage` rows (F32_STAGE / BF16_STAGE)."""
    seg_splits = splits // 2 if two_segments else splits
    per = (P + seg_splits - 1) // seg_splits
    per = (per + stage - 1) // stage * stage
    out = []
    for s in range(splits):
        seg = 1 if two_segments and s >= seg_splits else 0
        k0 = (s - seg * seg_splits) * per
        out.append((seg, k0, min(k0 + per, P)))
    return out


# ---- finalize -----------------------------------------------------------------------------------------------------------------

def _seq_sum(x, dtype):
    """Sum over axis 0 in `dtype`, one term after the other."""
    x = np.asarray(x, dtype)
    acc = np.zeros(x.shape[1:], dtype)
    for s in range(x.shape[0]):
        acc = acc + x[s]
    return acc


def finalize(desc, slab, colsum, xsum, target0, btarget0, dtype=np.float64):
    """target[rmap[i] * t_stride + cmap[j]] (+)= scale * sum_s slab[s,i,j]  (+ xscale * sum_s xsum[s, cmap[j]] on target row xrow);
    btarget[rmap[i]] (+)= bscale * sum_s colsum[s,i]; negative map entries are skipped (include/vdn_render.h: VdnDwFinalizeDesc).
    desc: dict(rmap, cmap, t_stride, splits, M, N, accumulate, scale, bscale[, xrow, xscale]); slab [splits,M,N], colsum
    [splits,M], xsum [xsplits,xM] (or None each); target0 / btarget0: flat arrays (or None) -> new (target, btarget)."""
    M, N, acc = desc["M"], desc["N"], desc["accumulate"]
    rmap = np.asarray(desc["rmap"])
    tgt = None if target0 is None else np.array(target0, dtype)
    bt = None if btarget0 is None else np.array(btarget0, dtype)
    if tgt is not None and N:
        cmap = np.asarray(desc["cmap"])
        val = dtype(desc["scale"]) * _seq_sum(slab, dtype)                             # [M, N]
        xs = None if xsum is None else dtype(desc["xscale"]) * _seq_sum(xsum, dtype)      # [xM]
        for i in range(M):
            r = int(rmap[i])
            if r < 0:
                continue
            j = np.nonzero(cmap >= 0)[0]
            cc = cmap[j]
            v = val[i, j]
            if xs is not None and r == desc["xrow"]:
                v = v + xs[cc]
            idx = r * desc["t_stride"] + cc
            tgt[idx] = tgt[idx] + v if acc else v
    if bt is not None:
        bval = dtype(desc["bscale"]) * _seq_sum(colsum, dtype)
        i = np.nonzero(rmap[:M] >= 0)[0]
        bt[rmap[i]] = bt[rmap[i]] + bval[i] if acc else bval[i]
    return tgt, bt


def finalize_units(desc, slab, colsum, xsum, target0, btarget0):
    """2^-24 (|scale| sum_s |slab| + |xscale| sum_s |xsum| + |old target| if accumulating), laid out like the targets (0 where
    nothing is written); the bias target alike."""
    d = dict(desc, scale=abs(desc["scale"]), bscale=abs(desc["bscale"]), xscale=abs(desc.get("xscale", 0.0)), accumulate=1)
    ab = lambda x: None if x is None else np.abs(np.asarray(x, np.float64))
    old = lambda x: None if x is None else (np.nan_to_num(np.abs(np.asarray(x, np.float64)), nan=0.0) if desc["accumulate"] else np.zeros(len(x)))
    t, b = finalize(d, ab(slab), ab(colsum), ab(xsum), old(target0), old(btarget0))
    return (None if t is None else ULP * t), (None if b is None else ULP * b)


# ---- weight norm --------------------------------------------------------------------------------------------------------------

def weightnorm(g, v):
    """torch tensors g [rows], v [rows, cols] (any float dtype) -> (w = g v / |v| per row, inv_norm = 1 / |v|)."""
    norm = (v * v).sum(1, keepdim=True).sqrt()
    return g[:, None] * v / norm, (1.0 / norm)[:, 0]


def weightnorm_bwd(g, v, dw, dtype=torch.float64):
    """(dg, dv) for the upstream gradient dw: autograd of weightnorm in `dtype`."""
    g = torch.as_tensor(g).to(dtype).clone().requires_grad_(True)
    v = torch.as_tensor(v).to(dtype).clone().requires_grad_(True)
    w, _ = weightnorm(g, v)
    w.backward(torch.as_tensor(dw).to(dtype))
    return g.grad, v.grad


def weightnorm_units(g, v, dw):
    """float64 numpy units of (w, dg, dv): 2^-24 |w|; 2^-24 sum_c |dw v| / |v|; 2^-24 |k1| (|dw| + |k2 v|) with k1 = g / |v| and
    k2 = <dw, v> / |v|^2 - the two terms of dv cancel (entirely when cols == 1), as the variance sums of ray_ops.var_units do."""
    g, v, dw = (np.asarray(x, np.float64) for x in (g, v, dw))
    norm = np.sqrt((v * v).sum(1))
    k1, k2 = g / norm, (dw * v).sum(1) / norm ** 2
    return (ULP * np.abs(k1[:, None] * v), ULP * np.abs(dw * v).sum(1) / norm,
            ULP * np.abs(k1)[:, None] * (np.abs(dw) + np.abs(k2[:, None] * v)))


# ---- Adam ---------------------------------------------------------------------------------------------------------------------

def adam(p, g, m, v, ranges, lr, betas, eps, step):
    """torch.optim.Adam (no weight decay, no amsgrad) at step count `step` over the element ranges [(begin, end), ...] of the flat
    float64 arrays only -> new (p, m, v). dp = p_new - p is what the units of the parameter are built from."""
    p, g, m, v = (np.array(x, np.float64) for x in (p, g, m, v))
    b1, b2 = betas
    for lo, hi in ranges:
        s = slice(lo, hi)
        m[s] = b1 * m[s] + (1.0 - b1) * g[s]
        v[s] = b2 * v[s] + (1.0 - b2) * g[s] * g[s]
        denom = np.sqrt(v[s]) / np.sqrt(1.0 - b2 ** step) + eps
        p[s] = p[s] - lr / (1.0 - b1 ** step) * m[s] / denom
    return p, m, v


def adam_torch(p, g, m, v, ranges, lr, betas, eps, step, dtype):
    """The same through torch.optim.Adam itself (foreach=False) in `dtype` on the CPU: one parameter per range, its state set to
    (step - 1, m, v). float32: the rounding floor of the update; float64: the proof of `adam`."""
    out = [np.array(x, np.float64) for x in (p, m, v)]
    for lo, hi in ranges:
        if hi <= lo:
            continue
        par = torch.nn.Parameter(torch.as_tensor(np.asarray(p[lo:hi])).to(dtype).clone())
        par.grad = torch.as_tensor(np.asarray(g[lo:hi])).to(dtype).clone()
        opt = torch.optim.Adam([par], lr=lr, betas=tuple(betas), eps=eps, foreach=False)
        opt.state[par] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.as_tensor(np.asarray(m[lo:hi])).to(dtype).clone(),
                              exp_avg_sq=torch.as_tensor(np.asarray(v[lo:hi])).to(dtype).clone())
        opt.step()
        st = opt.state[par]
        assert int(st["step"]) == step
        for o, t in zip(out, (par.detach(), st["exp_avg"], st["exp_avg_sq"])):
            o[lo:hi] = t.double().numpy()
    return tuple(out)


def adam_units(p0, g, m0, v0, p1):
    """m: 2^-24 (|m0| + |g|); v: 2^-24 (v0 + g^2); p: 2^-24 (|p0| + |dp|), dp from the float64 model's p1."""
    p0, g, m0, v0, p1 = (np.asarray(x, np.float64) for x in (p0, g, m0, v0, p1))
    return ULP * (np.abs(p0) + np.abs(p1 - p0)), ULP * (np.abs(m0) + np.abs(g)), ULP * (v0 + g * g)


def units_err(got, ref, unit):
    """Worst |got - ref| in units (0 where both the error and the unit are 0)."""
    got, ref, unit = (np.asarray(x, np.float64) for x in (got, ref, unit))
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / (unit + 1e-300)).max())
