"""The per-ray kernels as operators, through the C ABI (include/vdn_render.h), one launch per case, against the float64 model of
oracle/ray_ops.py differentiated by autograd, on the constructed inputs of oracle/ray_cases.py (whose coverage, margins and
conditioning tests/test_ray_ops_model_cpu.py proves without a GPU).

Every output buffer is pre-filled with NaN and sits between two NaN guard bands: after the launch every element the header says
is written is finite and compared, every other element is still NaN. No element of any output is excluded and no case skipped.

Tolerance against the float64 model: conftest.relelem at its defaults (1e-4 of the element, floored at 1e-6 of the tensor's
largest entry; <= 1 passes), with the margin tests/test_gpu_grads.py::_compare grants: per (case, tensor) the kernel stays
within max(1, 3 x fp32 floor) units, the floor being relelem(float32 model on the CPU, float64 model) - measured at run time
from the reference, never from the kernel. Three times, because the kernel's operation order differs from torch's and one extra
rounding per step may land the other way; not more, because the kernels accumulate in double where torch does not. In the
ill-conditioned regimes (sharp / saturated / deep inside) the quantities that stay well-conditioned - weights, color_out, d_color,
d_bg_rgb - are held to the plain 1-unit bound. Every (case, tensor) whose bound exceeded 1 unit is printed (pytest -rA).
d_var_partial / d_variance, signed sums that cancel, are judged against the sum of the absolute per-sample terms
(ray_ops.var_units). The alpha-clip regime feeds negative section lengths: not a production input (sorted depths cannot make one)
but the operator's contract (renderer.py:282: the clip, and a zero adjoint through it).

The fused launches (vdn_feat_composite, vdn_eikonal_terms, vdn_eikonal_reduce, vdn_composite_train, vdn_composite_fwd_train /
_bwd_train) promise bit-identity with the separate calls: asserted exactly, over the whole case matrix they accept, together
with -10 and nothing written for what they decline.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ray_cases, ray_ops
from conftest import relelem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 96                       # NaN elements in front of and behind every output buffer
STRICT_WHEN_ILL = ("weights", "color_out", "d_color", "d_bg_rgb")
NAMES = ray_cases.composite_case_names()


class Bufs:
    """Device buffers of one launch: inputs, and NaN-filled outputs between NaN guard bands."""

    def __init__(self):
        self.keep, self.outs = [], {}

    def inp(self, a, dtype=torch.float32):
        if a is None:
            return None
        t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def out(self, name, *shape):
        n = int(np.prod(shape))
        base = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
        self.outs[name] = (base, base[GUARD:GUARD + n].view(*shape))
        return base[GUARD:].data_ptr()

    def __getitem__(self, name):
        return self.outs[name][1]

    def check(self, written=None, unwritten=()):
        """Guard bands untouched; every output finite (or, for `unwritten`, still all NaN)."""
        torch.cuda.synchronize()
        for name, (base, view) in self.outs.items():
            assert torch.isnan(base[:GUARD]).all() and torch.isnan(base[-GUARD:]).all(), "guard band of %s was written" % name
            if name in unwritten:
                assert torch.isnan(view).all(), "%s was written" % name
            elif written is None or name in written:
                assert torch.isfinite(view).all(), "%s has unwritten or non-finite elements" % name

    def np(self, name):
        return self[name].detach().cpu().double().numpy()


def _status(fn, *args):
    from vdn_hip import lib
    cargs = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args]
    return int(getattr(lib.load(), fn)(*cargs))


def _call(fn, *args):
    rc = _status(fn, *args)
    assert rc == 0, "%s returned %d" % (fn, rc)


def _stream():
    return torch.cuda.current_stream().cuda_stream


_MODELS = {}


def _models(name):
    if name not in _MODELS:
        case = ray_cases.composite_case(name)
        _MODELS.clear()                              # (one case's graphs at a time)
        _MODELS[name] = (case, ray_ops.CompositeModel(case, torch.float64), ray_ops.CompositeModel(case, torch.float32))
    return _MODELS[name]


def _judge(case, tensor, got, ref64, ref32, rows, units=relelem, **kw):
    """Assert `got` within max(1, 3 x fp32 floor) units of ref64 (1 unit for the well-conditioned tensors of the ill regimes)."""
    floor = units(ref32, ref64, **kw)
    err = units(got, ref64, **kw)
    strict = case.get("regime") in ray_cases.ILL_CONDITIONED and tensor.split("/")[-1] in STRICT_WHEN_ILL
    bound = 1.0 if strict else max(1.0, 3.0 * floor)
    if bound > 1.0:
        rows.append("%-34s %-22s bound %.2f units (fp32 floor %.3f)  kernel error %.3f" % (case["name"], tensor, bound, floor, err))
    assert err <= bound, "%s %s: kernel error %.3f units > bound %.2f (fp32 floor %.3f)" % (case["name"], tensor, err, bound, floor)
    return err


def _report(rows):
    if rows:
        print("(case, tensor) pairs whose bound exceeded 1 unit:\n" + "\n".join(rows))


# ---- the forward ------------------------------------------------------------------------------------------------------------

def _composite_inputs(a, b, case, with_feat=True):
    """Fill the input half shared by VdnCompositeArgs and VdnCompositeBwdArgs."""
    for k in ("rays_o", "rays_d", "sdf", "normals", "dists", "mid_z", "color", "bg_density", "bg_rgb", "bg_dists", "background_rgb"):
        setattr(a, k, b.inp(case[k]))
    a.variance = b.inp(np.asarray([case["variance"]], np.float32))
    if with_feat and case["C"]:
        a.feat, a.bg_feat = b.inp(case["feat"]), b.inp(case["bg_feat"])
    a.cos_anneal_ratio = float(case["cos_anneal_by_value"])
    if case["use_dev"]:                              # the by-value field holds a different number: the device scalar must win
        a.cos_anneal_dev = b.inp(np.asarray([case["cos_anneal"]], np.float32))
    a.B, a.N, a.T, a.feat_ch = case["B"], case["N"], case["T"], case["C"] if with_feat else 0


def _forward_args(case, b, with_feat=True):
    from vdn_hip import lib
    B, N, T, C = case["B"], case["N"], case["T"], case["C"]
    a = lib.VdnCompositeArgs()
    _composite_inputs(a, b, case, with_feat)
    a.weights, a.alpha_out = b.out("weights", B, T), b.out("alpha_out", B, T)
    a.cdf, a.inside_sphere = b.out("cdf", B, N), b.out("inside_sphere", B, N)
    a.color_out, a.weight_sum, a.weight_max, a.s_val = b.out("color_out", B, 3), b.out("weight_sum", B), b.out("weight_max", B), b.out("s_val", B)
    a.eik_partial = b.out("eik_partial", B, 2)
    a.eik_out = b.out("eik_out", 3)
    if with_feat and C:
        a.feat_out = b.out("feat_out", B, C)
    return a


def _forward(case, with_feat=True):
    b = Bufs()
    a = _forward_args(case, b, with_feat)
    _call("vdn_alpha_composite_fwd", a, _stream())
    b.check()
    return a, b


@pytest.mark.parametrize("name", NAMES)
def test_composite_forward_vs_float64_model(name):
    case, m64, m32 = _models(name)
    _, b = _forward(case)
    r64, r32 = ray_ops.forward_arrays(m64), ray_ops.forward_arrays(m32)
    rows = []
    assert set(b.outs) == set(r64)
    assert np.array_equal(b.np("inside_sphere"), r64["inside_sphere"])
    assert np.array_equal(b.np("eik_partial")[:, 1], r64["eik_partial"][:, 1]) and b.np("eik_out")[2] == r64["eik_out"][2]
    for k in r64:
        if k == "eik_partial":                       # (numerator per ray; the denominator, a count, is exact above)
            _judge(case, k, b.np(k)[:, 0], r64[k][:, 0], r32[k][:, 0], rows)
        elif k == "eik_out":                         # three scalars of different sizes: each on its own
            for i in range(3):
                _judge(case, "eik_out[%d]" % i, b.np(k)[i:i + 1], r64[k][i:i + 1], r32[k][i:i + 1], rows)
        elif k != "inside_sphere":
            _judge(case, k, b.np(k), r64[k], r32[k], rows)
    if (case["neg_dists"]).any():                    # the clip: alpha exactly 0 where raw < 0 (inside the sphere, or without a background)
        raw, ins = m64.out["raw_alpha"].detach().numpy(), r64["inside_sphere"]
        sel = (raw < 0) & ((ins == 1) | (case["bg_density"] is None))
        assert sel.any() and (b.np("alpha_out")[:, :case["N"]][sel] == 0.0).all()
    _report(rows)


@pytest.mark.parametrize("name", NAMES)
def test_forward_side_launches_are_bit_identical_to_the_compositor(name):
    """vdn_feat_composite, vdn_eikonal_terms, vdn_eikonal_reduce and vdn_composite_fwd_train against vdn_alpha_composite_fwd."""
    from vdn_hip import lib
    case, m64, _ = _models(name)
    B, N, T, C = case["B"], case["N"], case["T"], case["C"]
    a, b = _forward(case)
    # the eikonal sums alone, and the reduction alone
    e = Bufs()
    ea = lib.VdnEikonalArgs()
    ea.rays_o, ea.rays_d, ea.mid_z, ea.normals = (e.inp(case[k]) for k in ("rays_o", "rays_d", "mid_z", "normals"))
    ea.B, ea.N = B, N
    ea.eik_partial, ea.eik_out = e.out("eik_partial", B, 2), e.out("eik_out", 3)
    _call("vdn_eikonal_terms", ea, _stream())
    e.check()
    assert torch.equal(e["eik_partial"], b["eik_partial"]) and torch.equal(e["eik_out"], b["eik_out"])
    red = Bufs()
    _call("vdn_eikonal_reduce", ctypes.c_void_p(b["eik_partial"].data_ptr()), B, ctypes.c_void_p(red.out("eik_out", 3)), _stream())
    red.check()
    assert torch.equal(red["eik_out"], b["eik_out"])
    if not C:
        # without feature channels the feature launches are argument errors - the feature-channel check itself (-2 / -5 in
        # rays.hip; every other pointer is valid) - and nothing is launched or written
        f = Bufs()
        fa = _forward_args(case, f)
        g_feats = f.out("g_feats", B, 1)
        assert _status("vdn_feat_composite", fa, _stream()) == -2
        assert _status("vdn_composite_fwd_train", fa, ctypes.c_void_p(f.inp(np.zeros((B, 1)))), ctypes.c_void_p(g_feats), 0.7, 1.0, _stream()) == -5
        f.check(unwritten=tuple(f.outs))
        return
    # the feature sums alone, from the weights / inside flags the compositor left
    f = Bufs()
    fa = lib.VdnCompositeArgs()
    _composite_inputs(fa, f, case)
    fa.weights, fa.inside_sphere = b["weights"].data_ptr(), b["inside_sphere"].data_ptr()
    fa.feat_out = f.out("feat_out", B, C)
    _call("vdn_feat_composite", fa, _stream())
    f.check()
    assert torch.equal(f["feat_out"], b["feat_out"])
    # the training forward: compositor + feature sums + d loss / d render_feats; eik_out is not written
    t = Bufs()
    ta = _forward_args(case, t)
    g_feats = t.out("g_feats", B, C)
    gs, dw = 0.5, 0.7
    _call("vdn_composite_fwd_train", ta, ctypes.c_void_p(t.inp(case["gt_feats"])), ctypes.c_void_p(g_feats), dw, gs, _stream())
    t.check(unwritten=("eik_out",))
    for k in b.outs:
        if k != "eik_out":
            assert torch.equal(t[k], b[k]), k
    # ... whose g_feats is vdn_loss_fwd_bwd's on those features, bit for bit
    l = Bufs()
    la = _loss_args(l, dict(B=B, T=T, C=C, color=b.np("color_out"), true_rgb=case["true_rgb"], mask=None, feats=None, gt_feats=case["gt_feats"],
                            weights=None, eik=b.np("eik_out"), igr_weight=0.1, mask_weight=0.0, depth_weight=dw, grad_scale=gs),
                    feats_ptr=b["feat_out"].data_ptr())
    _call("vdn_loss_fwd_bwd", la, _stream())
    l.check(written=("g_color", "g_feats", "g_eik", "out_scalars"))
    assert torch.equal(l["g_feats"], t["g_feats"])


# ---- the adjoint ------------------------------------------------------------------------------------------------------------

def _backward_args(case, b, fwd, upstream, trio, scratch, with_feat=True, eik=True):
    """VdnCompositeBwdArgs on the forward's saved alpha / weights / eik. upstream: dict of the g_* given (others NULL)."""
    from vdn_hip import lib
    B, N, T, C = case["B"], case["N"], case["T"], case["C"] if with_feat else 0
    a = lib.VdnCompositeBwdArgs()
    _composite_inputs(a, b, case, with_feat)
    a.alpha, a.weights = fwd["alpha_out"].data_ptr(), fwd["weights"].data_ptr()
    if eik:
        a.eik = fwd["eik_out"].data_ptr()
    for k in ("g_color", "g_feat", "g_weights", "g_cdf"):
        if k in upstream and (k != "g_feat" or C):
            setattr(a, k, b.inp(case[k]))
    if "g_eik" in upstream:
        a.g_eik = b.inp(case["g_eik"])
    has_bg = case["bg_density"] is not None
    a.d_sdf, a.d_normals, a.d_color = b.out("d_sdf", B, N), b.out("d_normals", B * N, 3), b.out("d_color", B, N, 3)
    a.d_var_partial, a.d_variance = b.out("d_var_partial", B), b.out("d_variance", 1)
    if has_bg:
        a.d_bg_density, a.d_bg_rgb = b.out("d_bg_density", B, T), b.out("d_bg_rgb", B, T, 3)
    if C and "g_feat" in upstream:                   # (the feature adjoints are written only with an upstream g_feat)
        a.d_feat = b.out("d_feat", B, N, C)
        if has_bg:
            a.d_bg_feat = b.out("d_bg_feat", B, T, C)
        if scratch:
            a.feat_scratch = b.out("feat_scratch", B * (2 * T + N))
    if trio:
        a.d_dists, a.d_dir_cos = b.out("d_dists", B, N), b.out("d_dir_cos", B, 3)
        if has_bg:
            a.d_bg_dists = b.out("d_bg_dists", B, T)
    return a


def _judge_adjoint(case, tag, b, a64, a32, rows):
    for k in b.outs:
        if k == "feat_scratch":
            continue
        label = "%s/%s" % (tag, k)
        if k == "d_var_partial":
            _judge(case, label, b.np(k), a64[k], a32[k], rows, units=ray_ops.var_units, abs_sum=a64["d_var_abs"])
        elif k == "d_variance":
            _judge(case, label, b.np(k)[0], a64[k], a32[k], rows, units=ray_ops.var_units, abs_sum=a64["d_var_abs"].sum())
        elif np.abs(a64[k]).max() == 0.0:
            assert (b.np(k) == 0.0).all(), label
        else:
            _judge(case, label, b.np(k).reshape(a64[k].shape), a64[k], a32[k], rows)
    if float(np.exp(np.float64(case["variance"]) * 10.0)) > 1e6 or float(np.exp(np.float64(case["variance"]) * 10.0)) < 1e-6:
        assert (b.np("d_var_partial") == 0.0).all() and (b.np("d_variance") == 0.0).all()       # the active clip: exactly zero


@pytest.mark.parametrize("name", NAMES)
def test_composite_backward_vs_autograd_of_the_model(name):
    """Random upstream gradients, all given and each in turn NULL; the ray-adjoint trio on and off; with feature channels once
    through feat_scratch (three launches) and once in the per-ray kernel. Prints whether those two paths are bit-equal."""
    case, m64, m32 = _models(name)
    _, fwd = _forward(case)
    rows, C = [], case["C"]
    variants = [("all+trio+scratch", None, True, True), ("all", None, False, False)]
    variants += [("no_%s" % g, g, i % 2 == 0, i % 2 == 1) for i, g in enumerate(ray_ops.UPSTREAM)]
    feat_paths = {}
    for tag, drop, trio, scratch in variants:
        if drop == "g_feat" and not C:
            continue
        up = ray_ops.upstream_of(case, drop)
        b = Bufs()
        a = _backward_args(case, b, fwd, up, trio, scratch)
        _call("vdn_alpha_composite_bwd", a, _stream())
        b.check(written=set(b.outs) - {"feat_scratch"})
        a64, a32 = ray_ops.adjoint_arrays(m64, **up), ray_ops.adjoint_arrays(m32, **up)
        _judge_adjoint(case, tag, b, a64, a32, rows)
        if drop is None and C:
            feat_paths[scratch] = {k: b[k].clone() for k in b.outs if k != "feat_scratch"}
    if C:
        same = all(torch.equal(feat_paths[True][k], feat_paths[False][k]) for k in feat_paths[False])
        print("%s: feat_scratch path and in-kernel feature path bit-equal: %s" % (name, same))
    _report(rows)


# ---- forward + loss gradient + adjoint in one launch ------------------------------------------------------------------------

def _loss_args(b, c, feats_ptr=None, weights_ptr=None):
    from vdn_hip import lib
    a = lib.VdnLossArgs()
    a.color, a.true_rgb, a.mask = b.inp(c["color"]), b.inp(c["true_rgb"]), b.inp(c["mask"])
    a.feats = feats_ptr if feats_ptr is not None else b.inp(c["feats"])
    a.gt_feats = b.inp(c["gt_feats"]) if a.feats else None
    a.weights = weights_ptr if weights_ptr is not None else b.inp(c["weights"])
    a.eik = b.inp(c["eik"])
    a.igr_weight, a.mask_weight, a.depth_weight, a.grad_scale = c["igr_weight"], c["mask_weight"], c["depth_weight"], c["grad_scale"]
    a.B, a.T, a.C = c["B"], c["T"], c["C"]
    a.g_color, a.g_eik, a.out_scalars = b.out("g_color", c["B"], 3), b.out("g_eik", 1), b.out("out_scalars", 6)
    if a.feats:
        a.g_feats = b.out("g_feats", c["B"], c["C"])
    if a.weights:
        a.g_weights = b.out("g_weights", c["B"], c["T"])
    return a


@pytest.mark.parametrize("name", NAMES)
def test_fused_training_launches_are_bit_identical_to_the_separate_calls(name):
    """vdn_composite_train (no feature channels) and vdn_composite_fwd_train + vdn_composite_bwd_train (with them) against
    vdn_alpha_composite_fwd + vdn_loss_fwd_bwd + vdn_alpha_composite_bwd; fg_count = the model's relaxed-sphere count."""
    case, m64, _ = _models(name)
    B, N, T, C = case["B"], case["N"], case["T"], case["C"]
    igr, gs, dw = 0.1, 0.5, 0.7
    fg = int(m64.out["eik_den"])
    # the separate calls, without and with the feature channels
    for with_feat in ((False, True) if C else (False,)):
        _, fwd = _forward(case, with_feat)
        assert float(fwd["eik_out"][2]) == fg
        l = Bufs()
        la = _loss_args(l, dict(B=B, T=T, C=C if with_feat else 0, color=None, true_rgb=case["true_rgb"], mask=None, feats=None,
                                gt_feats=case["gt_feats"] if with_feat else None, weights=None, eik=fwd.np("eik_out"), igr_weight=igr,
                                mask_weight=0.0, depth_weight=dw, grad_scale=gs),
                        feats_ptr=fwd["feat_out"].data_ptr() if with_feat else None)
        la.color = fwd["color_out"].data_ptr()
        _call("vdn_loss_fwd_bwd", la, _stream())
        l.check()
        sep = Bufs()
        sa = _backward_args(case, sep, fwd, {}, False, True, with_feat)
        sa.g_color, sa.g_eik = l["g_color"].data_ptr(), l["g_eik"].data_ptr()
        if with_feat:
            sa.g_feat = l["g_feats"].data_ptr()
            sa.d_feat = sep.out("d_feat", B, N, C)
            sa.feat_scratch = sep.out("feat_scratch", B * (2 * T + N))
            if case["bg_density"] is not None:
                sa.d_bg_feat = sep.out("d_bg_feat", B, T, C)
        _call("vdn_alpha_composite_bwd", sa, _stream())
        sep.check(written=set(sep.outs) - {"feat_scratch"})
        count = torch.tensor([fg], dtype=torch.int32, device=DEV)
        if not with_feat:
            f, fb = Bufs(), Bufs()
            fa = _forward_args(case, f, False)
            ba = _backward_args(case, fb, f, {}, False, False, False, eik=False)
            g_color = fb.out("g_color", B, 3)
            args = (fa, ba, ctypes.c_void_p(fb.inp(case["true_rgb"])), ctypes.c_void_p(g_color), ctypes.c_void_p(count.data_ptr()), igr, gs, _stream())
            _call("vdn_composite_train", *args)
            f.check(unwritten=("eik_out",))
            fb.check()
            for k in f.outs:
                if k != "eik_out":
                    assert torch.equal(f[k], fwd[k]), k
            assert torch.equal(fb["g_color"], l["g_color"])
            for k in sep.outs:
                assert torch.equal(fb[k], sep[k]), k
            # what it declines: -10, nothing launched
            for field in ("g_weights", "g_cdf"):
                d, db = Bufs(), Bufs()
                da = _forward_args(case, d, False)
                dba = _backward_args(case, db, d, {field: True}, False, False, False, eik=False)
                assert _status("vdn_composite_train", da, dba, *args[2:]) == -10, field
                d.check(unwritten=tuple(d.outs))
                db.check(unwritten=tuple(db.outs))
            d, db = Bufs(), Bufs()
            da = _forward_args(case, d, False)
            dba = _backward_args(case, db, d, {}, True, False, False, eik=False)
            assert _status("vdn_composite_train", da, dba, *args[2:]) == -10
            d.check(unwritten=tuple(d.outs))
            db.check(unwritten=tuple(db.outs))
            if C:                                    # ... and the feature channels: fwd.feat_out, bwd.g_feat, bwd.d_feat, each alone
                for field in ("feat_out", "g_feat", "d_feat"):
                    d, db = Bufs(), Bufs()
                    da = _forward_args(case, d, field == "feat_out")
                    dba = _backward_args(case, db, d, {"g_feat": True} if field == "g_feat" else {}, False, False, True, eik=False)
                    if field == "g_feat":
                        dba.d_feat = dba.d_bg_feat = None
                    elif field == "d_feat":
                        dba.d_feat = db.out("d_feat", B, N, C)
                    assert _status("vdn_composite_train", da, dba, *args[2:]) == -10, field
                    d.check(unwritten=tuple(d.outs))
                    db.check(unwritten=tuple(db.outs))
        else:
            fb = Bufs()
            ba = _backward_args(case, fb, fwd, {}, False, True, True, eik=False)
            ba.g_feat = l["g_feats"].data_ptr()
            ba.d_feat = fb.out("d_feat", B, N, C)
            ba.feat_scratch = fb.out("feat_scratch", B * (2 * T + N))
            if case["bg_density"] is not None:
                ba.d_bg_feat = fb.out("d_bg_feat", B, T, C)
            g_color = fb.out("g_color", B, 3)
            args = (ctypes.c_void_p(fwd["color_out"].data_ptr()), ctypes.c_void_p(fb.inp(case["true_rgb"])), ctypes.c_void_p(g_color),
                    ctypes.c_void_p(count.data_ptr()), igr, gs, _stream())
            _call("vdn_composite_bwd_train", ba, *args)
            fb.check(written=set(fb.outs) - {"feat_scratch"})
            assert torch.equal(fb["g_color"], l["g_color"])
            for k in sep.outs:
                if k != "feat_scratch":
                    assert torch.equal(fb[k], sep[k]), k
            for up, trio in (({"g_weights": True}, False), ({"g_cdf": True}, False), ({}, True)):
                db = Bufs()
                dba = _backward_args(case, db, fwd, up, trio, False, True, eik=False)
                assert _status("vdn_composite_bwd_train", dba, *args) == -10, (up, trio)
                db.check(unwritten=tuple(db.outs))


# ---- the loss ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ray_cases.LOSS_CASES))
def test_loss_vs_autograd_of_the_model(name):
    c = ray_cases.loss_case(name)
    b = Bufs()
    a = _loss_args(b, c)
    _call("vdn_loss_fwd_bwd", a, _stream())
    unwritten = ("g_weights",) if c["mask_weight"] == 0.0 else ()          # (header: only needed when mask_weight != 0)
    b.check(unwritten=unwritten)
    r64, r32 = ray_ops.loss_adjoints(c, torch.float64), ray_ops.loss_adjoints(c, torch.float32)
    rows = []
    got = b.np("out_scalars")
    for i, k in enumerate(ray_ops.LOSS_SCALARS):
        ref, ref32 = float(r64[k]), float(r32[k])
        if ref == 0.0:
            assert got[i] == 0.0, k
        else:
            _judge(c, k, got[i:i + 1], np.asarray([ref]), np.asarray([ref32]), rows)
    assert float(b.np("g_eik")[0]) == float(np.float32(c["igr_weight"]))
    for k in ("g_color", "g_feats", "g_weights"):
        if k in b.outs and k not in unwritten:
            ref = r64[k].numpy()
            _judge(c, k, b.np(k), ref, r32[k].double().numpy(), rows)
            assert np.array_equal(b.np(k) == 0.0, ref == 0.0), k          # sign(0) rows and the BCE gate: exactly zero, nowhere else
    _report(rows)


# ---- the ray adjoint --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,background", [(n, bg) for n, (_, N, T) in ray_cases.RAY_ADJOINT_CASES.items()
                                             for bg in ((True, False) if T > N else (False,))])
def test_ray_adjoint_vs_autograd_of_the_geometry(name, background):
    from vdn_hip import lib
    c = dict(ray_cases.ray_adjoint_case(name))
    B, N, T = c["B"], c["N"], c["T"]
    with_bg = background
    if not with_bg:
        c["z_out"] = None
    r64, r32 = ray_ops.ray_geometry_adjoints(c, torch.float64), ray_ops.ray_geometry_adjoints(c, torch.float32)
    # mid-points as vdn_sections makes them (float32)
    z32 = torch.tensor(c["z"])
    _, mid = ray_ops.sections(z32, c["sample_dist"])
    b = Bufs()
    a = lib.VdnRayAdjointArgs()
    a.rays_d, a.mid_z = b.inp(c["rays_d"]), b.inp(mid.numpy())
    for k in ("d_pts", "d_dirs", "d_dists", "d_dir_cos"):
        setattr(a, k, b.inp(c[k]))
    a.B, a.N, a.T = B, N, T if with_bg else N
    a.d_rays_o, a.d_rays_d, a.d_z = b.out("d_rays_o", B, 3), b.out("d_rays_d", B, 3), b.out("d_z", B, N)
    if with_bg:
        _, bmid = ray_ops.sections(torch.cat([z32, torch.tensor(c["z_out"])], -1), c["sample_dist"])
        a.bg_mid = b.inp(bmid.numpy())
        a.d_bg_pts, a.d_bg_dirs, a.d_bg_dists = b.inp(c["d_bg_pts"]), b.inp(c["d_bg_dirs"]), b.inp(c["d_bg_dists"])
        a.d_z_out = b.out("d_z_out", B, T - N)
    _call("vdn_ray_adjoint", a, _stream())
    b.check()
    rows = []
    for k in b.outs:
        _judge(c, k, b.np(k), r64[k].numpy(), r32[k].double().numpy(), rows)
    _report(rows)


# ---- sections, coarse depths -------------------------------------------------------------------------------------------------
# A handful of float32 roundings of add / mul / div each: the bound is (roundings) x 2^-24 x (largest intermediate) per element,
# derived below - NOT the 1e-4 criterion, which would hide a wrong 1/n term.
U = 2.0 ** -24


@pytest.mark.parametrize("B,n,ld", [(1, 1, 1), (3, 5, 6), (7, 63, 95), (130, 128, 160), (1000, 160, 256), (5, 256, 256)])
def test_sections_vs_float64_model(B, n, ld):
    from vdn_hip import lib
    c = ray_cases.sections_case("sections-%d-%d-%d" % (B, n, ld), B, n, ld)
    b = Bufs()
    a = lib.VdnSectionArgs()
    a.z, a.sample_dist, a.B, a.n, a.ld = b.inp(c["z"]), c["sample_dist"], B, n, ld
    a.dists, a.mid_z = b.out("dists", B, n), b.out("mid_z", B, n)
    _call("vdn_sections", a, _stream())
    b.check()
    z = torch.tensor(c["z"][:, :n]).double()
    dists, mid = ray_ops.sections(z, float(np.float32(c["sample_dist"])))
    # dists_i = z_{i+1} - z_i: one rounding of a result of size |dists_i| (the last one is the argument itself: exact)
    assert (np.abs(b.np("dists") - dists.numpy()) <= U * np.abs(dists.numpy())).all()
    # mid_i = z_i + dists_i * 0.5: the halving is exact, so two roundings (dists_i, the sum); largest intermediate max(|z_i|, |mid_i|)
    assert (np.abs(b.np("mid_z") - mid.numpy()) <= 2 * U * np.maximum(np.abs(z.numpy()), np.abs(mid.numpy()))).all()


@pytest.mark.parametrize("B,n_samples,n_outside,z_ld,jitter_in,jitter_out",
                         [(1, 64, 0, 64, False, False), (5, 64, 32, 128, True, True), (130, 64, 32, 128, False, True),
                          (7, 64, 32, 64, True, False), (9, 63, 0, 130, True, False), (1000, 64, 32, 128, False, False)])
def test_coarse_z_vs_float64_model(B, n_samples, n_outside, z_ld, jitter_in, jitter_out):
    from vdn_hip import lib
    c = ray_cases.coarse_case("coarse-%d-%d-%d-%d%d" % (B, n_samples, n_outside, jitter_in, jitter_out), B, n_samples, n_outside, jitter_in, jitter_out)
    b = Bufs()
    a = lib.VdnCoarseArgs()
    for k in ("near", "far", "lin_samples", "lin_outside", "out_lower", "out_upper", "t_rand", "t_rand_out"):
        setattr(a, k, b.inp(c[k]))
    a.B, a.n_samples, a.n_outside, a.z_ld = B, n_samples, n_outside, z_ld
    a.z = b.out("z", B, z_ld)
    if n_outside:
        a.z_out = b.out("z_out", B, n_outside)
    _call("vdn_coarse_z", a, _stream())
    b.check(written=("z_out",))
    zg = b.np("z")
    assert np.isfinite(zg[:, :n_samples]).all() and np.isnan(zg[:, n_samples:]).all()      # z_ld > n_samples: the row's tail is not written
    t = lambda k: None if c[k] is None else torch.tensor(c[k]).double()
    z, z_out = ray_ops.coarse_z(t("near"), t("far"), t("lin_samples"), t("lin_outside"), t("out_lower"), t("out_upper"), t("t_rand"), t("t_rand_out"))
    near, far = c["near"].astype(np.float64), c["far"].astype(np.float64)
    # z = near + (far - near) * lin [+ (t - 0.5) * 2 / n]: roundings of far - near, the product and the sum (3), plus t - 0.5, the
    # division by n and the last sum with the jitter (6; the doubling is exact); largest intermediate max(|near|, |far|, |z|, 1)
    big = np.maximum(np.maximum(np.abs(near), np.abs(far)), np.maximum(np.abs(z.numpy()), 1.0))
    assert (np.abs(zg[:, :n_samples] - z.numpy()) <= (6 if jitter_in else 3) * U * big).all()
    if n_outside:
        # z_out = far / zo + 1/n. Without jitter zo is an input: roundings of the quotient, of 1/n and of the sum (3), largest
        # intermediate q = |far / zo| (>= z_out - 1/n). With jitter zo = lower + (upper - lower) * t carries 3 roundings of size
        # <= upper, i.e. a relative error 3 U upper / zo, which the quotient inherits: 3 U q upper / zo on top.
        zo = torch.flip(t("lin_outside")[None, :].expand(B, -1) if not jitter_out else
                        t("out_lower")[None, :] + (t("out_upper") - t("out_lower"))[None, :] * t("t_rand_out"), dims=[-1]).numpy()
        q = np.abs(far / zo)
        bound = 3 * U * np.maximum(q, np.abs(z_out.numpy()))
        if jitter_out:
            bound = bound + 3 * U * q * np.flip(c["out_upper"].astype(np.float64))[None, :] / zo
        assert (np.abs(b.np("z_out") - z_out.numpy()) <= bound).all()
