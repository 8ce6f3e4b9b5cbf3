"""Point-mode backward of the standalone networks (dpt_models/fields.py under autograd).

SDFNetwork.forward / .sdf / .gradient, RenderingNetwork.forward and NeRF.forward on explicit points, with the saves the
hand-derived backward needs, and that backward: the same kernels as the ray engine (vdn_hip/train.py) - the saving forwards,
rbar / fbar (or the one-launch split kernel), the heads' and the background network's delta chains - then the weight-gradient
GEMM + finalize + weight-norm backward over the per-network entries of train.py.

Per call, saves and deltas come from torch's caching allocator (bf16 planes padded with layout.rows) and live as long as the
autograd node. Everything runs on the caller's current stream: no side streams.

The weight-gradient plan is cached per (network, row count P, precision), at most _CAP entries per network. The key holds the
exact P, not the padded plane rows: the GEMM descriptors carry P (rows beyond it are masked) and the K splits follow from it, so
two calls whose P round to the same padded rows still get plans of their own. What the cache keeps for sure is the host-side
layout (splits, workgroup offsets) and the device copy of the row / column maps. The device descriptor tables hold the
addresses of that call's planes, slab, column sums and gradient buffers, which are all fresh allocations: the cached tables
are reused only when every address (and the SDF scale) matches the previous call's - which torch's caching allocator usually
arranges for a loop at a fixed P - and are rebuilt and uploaded (one train.DwGroup: three small host-to-device copies) otherwise.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import layout, lib
from . import train as _train

_CAP = 4
_stream = lib.stream_handle


def _store_dtype(precision):
    return torch.float32 if precision == "fp32" else torch.bfloat16


def _net_grads(module, dev):
    """One zeroed flat gradient buffer over the module's parameters -> (_Net, [grad view per parameter])."""
    params = lib.module_params(module)
    flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    views, out, off = {}, [], 0
    for p in params:
        v = flat[off:off + p.numel()].view(p.shape)
        views[id(p)] = v
        out.append(v)
        off += p.numel()
    return _train._Net(module, dev, views), out


def _weight_grads(module, ent, net, precision, sdf_scale=1.0):
    """Weight-gradient GEMM + finalize + weight-norm backward of `ent` (entries of one network over one row count) into net's
    gradient views, on the current stream."""
    P = ent[0]["Pn"]
    assert all(e["Pn"] == P for e in ent)
    key = (ent[0]["net"], P, precision)
    dev, st = net.dweff.device, _stream()
    cache = module.__dict__.setdefault("_pt_plans", OrderedDict())
    c = cache.get(key)
    if c is None:
        lay, maps, slab_elems, cs_elems, wgs = _train.dw_layout(ent, precision)
        c = cache[key] = dict(lay=lay, maps=torch.from_numpy(np.concatenate(maps)).to(dev), slab_elems=slab_elems,
                              cs_elems=cs_elems, wgs=wgs, ptrs=None, group=None)
        while len(cache) > _CAP:
            cache.popitem(last=False)
    else:
        cache.move_to_end(key)
    slab = torch.empty(max(c["slab_elems"], 1), dtype=torch.float32, device=dev)
    colsum = torch.empty(max(c["cs_elems"], 1), dtype=torch.float32, device=dev)
    nets = {ent[0]["net"]: net}
    wn, _ = _train.weightnorm_table(nets)
    ptrs = (tuple(s[0].data_ptr() for e in ent for s in (e["A"], e["B"], e.get("A2"), e.get("B2")) if s is not None)
            + (slab.data_ptr(), colsum.data_ptr(), net.dweff.data_ptr(), next(iter(net.grads.values())).data_ptr(),
               wn.view(np.uint8).tobytes(), sdf_scale))
    if c["ptrs"] != ptrs:
        dw, fin = _train.dw_tables(ent, c["lay"], nets, precision, slab, colsum, c["maps"], [0] * len(ent), sdf_scale)
        c["group"] = _train.dw_group(dw, fin, wn, 0, len(ent), c["wgs"], dev, wn_idx=range(len(wn)))
        c["ptrs"] = ptrs
    c["group"].launch("_f32" if precision == "fp32" else "_bf16", st)
    # (slab / colsum go back to the caching allocator in stream order: the launches above are their last readers)


# ---- SDF network ---------------------------------------------------------------------------------------------------------
def sdf_saves(module, P, dev, want_x):
    prec = module.precision
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    sv = dict(H=torch.empty(8, Pr, 256, dtype=sdt, device=dev), V=torch.empty(8, Pr, 256, dtype=sdt, device=dev),
              PE=torch.empty(Pr, 64, dtype=sdt, device=dev))
    if want_x:
        sv["U_pe"] = torch.empty(P, 39, dtype=torch.float32, device=dev)
    return sv


def sdf_backward(module, x, sv, g_sdf, g_feat, g_normals, want_x):
    """Adjoints of (sdf [P], feat [P,256] fp32 row-major, normals [P,3]) of a saving mode-1 forward on x [P,3]
    -> (d x or None, [d parameter ...] in module.parameters() order)."""
    prec, P, dev = module.precision, x.shape[0], x.device
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    net, grads = _net_grads(module, dev)
    img = net.img
    g_sdf, g_normals = g_sdf.contiguous(), g_normals.contiguous()
    gf = g_feat.contiguous() if prec == "fp32" else layout.to_pt32(g_feat)
    UB, EX, AB = torch.empty(Pr * 2144, dtype=sdt, device=dev), torch.empty(8, Pr, 256, dtype=sdt, device=dev), torch.empty(Pr * 2336, dtype=sdt, device=dev)
    # bf16: no softplus' planes; the chains re-derive it from H (in units of 1/(100 log2 e): s_from_h = 2)
    s_from_h = 2 if prec == "bf16" else 0
    S = sv["H"] if s_from_h else sv["S"]
    rb = lib.VdnSdfRbarArgs()
    rb.blob, rb.pts, rb.n_per_ray, rb.z_ld = img.blobs["full"].data_ptr(), x.data_ptr(), 1, 1
    rb.P, rb.scale = P, float(module.scale)
    rb.g_normals, rb.S, rb.V, rb.UB, rb.EX = g_normals.data_ptr(), S.data_ptr(), sv["V"].data_ptr(), UB.data_ptr(), EX.data_ptr()
    rb.s_from_h = s_from_h
    fb = lib.VdnSdfFbarArgs()
    fb.blob = img.blobs["fbar"].data_ptr()
    fb.g_sdf, fb.g_feat, fb.S, fb.EX, fb.AB = g_sdf.data_ptr(), gf.data_ptr(), S.data_ptr(), EX.data_ptr(), AB.data_ptr()
    fb.P, fb.scale, fb.s_from_h = P, float(module.scale), s_from_h
    dx = None
    if want_x:
        dx = torch.empty(P, 3, dtype=torch.float32, device=dev)
        fb.pts, fb.n_per_ray, fb.z_ld = x.data_ptr(), 1, 1
        fb.g_normals, fb.U_pe, fb.acc_pts, fb.d_pts = g_normals.data_ptr(), sv["U_pe"].data_ptr(), 0, dx.data_ptr()
    st = _stream()
    # as the ray engine: both chains in one launch (bf16, no input adjoint) unless the split kernel declines the size (-10)
    if not (prec == "bf16" and not want_x and lib.try_call("vdn_sdf_bwd_split_bf16", rb, fb, st)):
        lib.call("vdn_sdf_bwd_rbar" + module._sfx(), rb, st)
        lib.call("vdn_sdf_bwd_fbar" + module._sfx(), fb, st)
    ent = _train.sdf_dw_entries(sv["H"], sv["V"], sv["PE"], UB, AB, P, Pr, prec)
    _weight_grads(module, ent, net, prec, float(module.scale))
    return dx, grads


# ---- RenderingNetwork ----------------------------------------------------------------------------------------------------
def rendering_saves(module, P, dev):
    prec = module.precision
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    sv = dict(h=torch.empty(4, Pr, 256, dtype=sdt, device=dev), small=torch.empty(Pr, 64, dtype=sdt, device=dev))
    if module.conf["d_feature"] == 352:
        sv["extra"] = torch.empty(Pr, 96, dtype=sdt, device=dev)
    return sv


def rendering_backward(module, inputs, fv, out, sv, g_out, want_inputs):
    """inputs = (points, normals, view_dirs) [P,3] contiguous; fv = the feature plane the forward read ([P,256] fp32 or the bf16
    PT32 buffer); out [P,d_out] the forward's output -> (d points, d normals, d view_dirs, d feature_vectors [P,d_feature],
    [d parameter ...])."""
    prec = module.precision
    pts, normals, dirs = inputs
    P, dev = pts.shape[0], pts.device
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    d_out = module.conf["d_out"]
    ldo = 96 if d_out == 96 else 32
    net, grads = _net_grads(module, dev)
    dout, dh = torch.empty(Pr, ldo, dtype=sdt, device=dev), torch.empty(4, Pr, 256, dtype=sdt, device=dev)
    d_feat = torch.empty(Pr, 256, dtype=sdt, device=dev)
    d_normals = torch.empty(P, 3, dtype=torch.float32, device=dev)
    g_out = g_out.contiguous()
    b = lib.VdnRenderNetBwdArgs()
    b.blob = net.img.blobs["bwd"].data_ptr()
    b.g_out, b.out, b.save_h = g_out.data_ptr(), out.data_ptr(), sv["h"].data_ptr()
    b.delta_out, b.delta_h = dout.data_ptr(), dh.data_ptr()
    b.d_feat, b.d_normals, b.acc_feat, b.acc_normals = d_feat.data_ptr(), d_normals.data_ptr(), 0, 0
    b.P, b.d_out, b.squeeze_out = P, d_out, int(module.squeeze_out)
    d_pts = d_dirs = d_extra = None
    if want_inputs:
        d_pts, d_dirs = torch.empty(P, 3, dtype=torch.float32, device=dev), torch.empty(P, 3, dtype=torch.float32, device=dev)
        b.dirs, b.n_per_ray, b.acc_pts, b.d_pts, b.d_dirs = dirs.data_ptr(), 1, 0, d_pts.data_ptr(), d_dirs.data_ptr()
    if "extra" in sv:
        d_extra = torch.zeros(P, 96, dtype=torch.float32, device=dev)          # (the kernel adds into it)
        b.d_extra = d_extra.data_ptr()
    lib.call("vdn_rendernet_bwd" + module._sfx(), b, _stream())
    feat_plane = fv.view(Pr, 256)
    ent = _train.rendering_dw_entries("net", net.img.streams["fwd"][0].kmap, dh, dout, sv["h"], sv["small"], feat_plane,
                                      sv.get("extra"), P, d_out)
    _weight_grads(module, ent, net, prec)
    d_fv = d_feat if prec == "fp32" else layout.from_pt32(d_feat, P, 256)
    if d_extra is not None:
        d_fv = torch.cat([d_fv, d_extra], dim=1)
    return d_pts, d_normals, d_dirs, d_fv, grads


# ---- background NeRF -----------------------------------------------------------------------------------------------------
def nerf_saves(module, P, dev):
    prec = module.precision
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    e = lambda *shape: torch.empty(*shape, dtype=sdt, device=dev)
    return dict(h=e(8, Pr, 256), pe=e(Pr, 96), feature=e(Pr, 256), vpe=e(Pr, 32), hv=e(Pr, 128))


def nerf_backward(module, pts4, dirs, sv, g_density, g_rgb, g_feat, want_inputs):
    """Adjoints of (density [P], rgb [P,3], feat [P,96] or None) of a saving forward on pts4 [P,4] / dirs [P,3]
    -> (d pts4, d dirs, [d parameter ...])."""
    prec = module.precision
    P, dev = pts4.shape[0], pts4.device
    Pr, sdt = layout.rows(P, prec), _store_dtype(prec)
    dpt = bool(module.gen_depth_feats)
    net, grads = _net_grads(module, dev)
    e = lambda *shape: torch.empty(*shape, dtype=sdt, device=dev)
    do, dv, dhead, dh = e(Pr, 128 if dpt else 32), e(Pr, 128), e(Pr, 288), e(8, Pr, 256)
    g_density, g_rgb = g_density.contiguous(), g_rgb.contiguous()
    if dpt and g_feat is None:
        g_feat = torch.zeros(P, 96, dtype=torch.float32, device=dev)
    nb = lib.VdnNerfBwdArgs()
    nb.blob = net.img.blobs["bwd"].data_ptr()
    nb.g_density, nb.g_rgb = g_density.data_ptr(), g_rgb.data_ptr()
    if dpt:
        g_feat = g_feat.contiguous()
        nb.g_feat = g_feat.data_ptr()
    nb.save_h, nb.save_hv = sv["h"].data_ptr(), sv["hv"].data_ptr()
    nb.delta_o, nb.delta_v, nb.delta_head, nb.delta_h = do.data_ptr(), dv.data_ptr(), dhead.data_ptr(), dh.data_ptr()
    nb.P, nb.n_per_ray = P, 1
    d_pts4 = d_dirs = None
    if want_inputs:
        d_pts4, d_dirs = torch.empty(P, 4, dtype=torch.float32, device=dev), torch.empty(P, 3, dtype=torch.float32, device=dev)
        ig = lib.VdnNerfInputGradArgs()
        ig.pts4, ig.dirs, ig.d_pts4, ig.d_dirs, ig.accumulate = pts4.data_ptr(), dirs.data_ptr(), d_pts4.data_ptr(), d_dirs.data_ptr(), 0
        lib.call("vdn_nerf_mlp_bwd_input" + module._sfx(), nb, ig, _stream())
    else:
        lib.call("vdn_nerf_mlp_bwd" + module._sfx(), nb, _stream())
    ent = _train.nerf_dw_entries(net.img.streams, dh, sv["h"], sv["pe"], dhead, dv, sv["feature"], sv["vpe"], do, sv["hv"], P, dpt)
    _weight_grads(module, ent, net, prec)
    return d_pts4, d_dirs, grads
