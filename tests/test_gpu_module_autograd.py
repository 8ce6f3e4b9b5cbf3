"""Autograd through the standalone SDFNetwork, RenderingNetwork and NeRF (dpt_models/fields.py -> vdn_hip/points.py): gradients
to every parameter and to the inputs against the fp64 oracle's autograd (oracle/neus_oracle.py), the bf16 path by cosine, and
the module contract (switch, bit-identical outputs, determinism, once_differentiable)."""
import numpy as np
import pytest
import torch

from test_gpu_grads import _compare

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _states(dbc=False):
    from vdn_train import synth
    return synth.make_all_states(3, wdepth=True, variance=0.3, depth_before_color=dbc)


def _rend(dev, precision="fp32", dbc=False):
    from vdn_train import factory
    return factory.build_renderer(wdepth=True, device=dev, states=_states(dbc), precision=precision, depth_before_color=dbc)


def _oracle(dtype, dbc=False):
    import oracle.neus_oracle as orc
    return orc, orc.nets_from_numpy(_states(dbc), dtype=dtype, requires_grad=True)


def _rand(tag, shape, lo=-1.0, hi=1.0):
    from vdn_train import synth
    return torch.tensor((synth.uniform(17, "mod_ag/" + tag, shape) * (hi - lo) + lo).astype(np.float32))


def _clear(*mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


def _named(prefix, mod):
    return [(prefix + "." + n, p) for n, p in mod.named_parameters()]


def _oracle_grads(dtype, loss_fn, params_key, inputs, dbc=False):
    """loss_fn(orc, nets, *inputs as dtype leaf tensors) -> scalar; -> ({name: grad}, [input grads])."""
    orc, nets = _oracle(dtype, dbc)
    xs = [t.to(dtype).requires_grad_(True) for t in inputs]
    loss = loss_fn(orc, nets, *xs)
    named = [(k + "." + n, p) for k in params_key for n, p in getattr(nets, k).items()]
    gs = torch.autograd.grad(loss, [p for _, p in named] + xs, allow_unused=True)
    ref = {n: (torch.zeros_like(p) if g is None else g).detach() for (n, p), g in zip(named, gs)}
    return ref, [g.detach() if g is not None else None for g in gs[len(named):]]


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _cos(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-300))


def _check_inputs(got, ref, ref32, names):
    """Input gradients: rel-to-max error 1e-4 vs fp64 (or 3x the fp32 oracle's own). Through ReLU networks a point whose
    pre-activation lies within fp32 round-off of zero takes the other branch on the device (see _compare); such a point's
    input gradient is not diluted by a sum over points (and through the background network's 10-octave encoding of pts4 a
    flipped unit reaches d pts4 amplified by up to 2^9), so a tensor is also accepted when at most 1 % of its rows miss the
    bound, none by more than 5e-2, and the whole tensor is within 1e-3 relative L2."""
    for n, a, b, b32 in zip(names, got, ref, ref32):
        floor = _relmax(b32, b)
        err = _relmax(a, b)
        tol = max(1e-4, 3 * floor)
        if err < tol:
            continue
        a, b = a.detach().double().cpu(), b.double()
        row_err = ((a - b).abs() / b.abs().max()).reshape(a.shape[0], -1).max(1).values
        rel_l2 = float((a - b).norm() / b.norm())
        assert err < 5e-2 and float((row_err > tol).double().mean()) <= 0.01 and rel_l2 < 1e-3, (n, err, floor, rel_l2)


# ---- losses (the same on the device and in the oracle) ------------------------------------------------------------------
def _sdf_loss(which, R1, R2):
    def dev_loss(net, x):
        r1, r2 = R1.to(x.device), R2.to(x.device)
        loss = 0.0
        if which in ("both", "forward"):
            loss = loss + (net(x) * r1).sum()
        if which == "sdf":
            loss = loss + (net.sdf(x) * r1[:, :1]).sum()
        if which in ("both", "gradient"):
            loss = loss + (net.gradient(x)[:, 0] * r2).sum()
        return loss

    def ref_loss(orc, nets, x):
        out, grad = orc.sdf_forward(nets.sdf, x, nets.sdf_conf, with_gradient=True)
        loss = 0.0
        if which in ("both", "forward"):
            loss = loss + (out * R1.to(x.dtype)).sum()
        if which == "sdf":
            loss = loss + (out[:, :1] * R1[:, :1].to(x.dtype)).sum()
        if which in ("both", "gradient"):
            loss = loss + (grad * R2.to(x.dtype)).sum()
        return loss
    return dev_loss, ref_loss


# ---- 1. SDF, fp32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,which", [(1, "both"), (31, "both"), (1000, "both"), (65536, "both"), (1000, "sdf"), (1000, "gradient")])
def test_sdf_fp32_vs_oracle(dev, P, which):
    rend = _rend(dev)
    net = rend.sdf_network
    x = _rand("x%d" % P, (P, 3), -1.1, 1.1)
    R1, R2 = _rand("r1%d" % P, (P, 257)), _rand("r2%d" % P, (P, 3))
    dev_loss, ref_loss = _sdf_loss(which, R1, R2)
    xg = x.to(dev).requires_grad_(True)
    dev_loss(net, xg).backward()
    ref, (gx,) = _oracle_grads(F64, ref_loss, ["sdf"], [x])
    ref32, (gx32,) = _oracle_grads(F32, ref_loss, ["sdf"], [x])
    _compare(_named("sdf", net), ref, 1e-4, ref32)
    _check_inputs([xg.grad], [gx], [gx32], ["x"])


# ---- 2. RenderingNetwork, fp32 -------------------------------------------------------------------------------------------
def _rn_inputs(P, dfeat):
    pts, nrm, dirs = _rand("rp", (P, 3)), _rand("rn", (P, 3)), _rand("rd", (P, 3))
    return pts, nrm, dirs, _rand("rf%d" % dfeat, (P, dfeat))


@pytest.mark.parametrize("head", ["color", "vdn", "color352"])
def test_rendering_fp32_vs_oracle(dev, head):
    P = 1000
    dbc = head == "color352"
    rend = _rend(dev, dbc=dbc)
    net = rend.depth_network if head == "vdn" else rend.color_network
    key = "vdn" if head == "vdn" else "color"
    ins = _rn_inputs(P, 352 if dbc else 256)
    R = _rand("ro" + head, (P, net.conf["d_out"]))
    gins = [t.to(dev).requires_grad_(True) for t in ins]
    (net(*gins) * R.to(dev)).sum().backward()

    def ref_loss(orc, nets, *xs):
        return (orc.rendering_forward(getattr(nets, key), *xs, getattr(nets, key + "_conf")) * R.to(xs[0].dtype)).sum()
    ref, gref = _oracle_grads(F64, ref_loss, [key], ins, dbc)
    ref32, gref32 = _oracle_grads(F32, ref_loss, [key], ins, dbc)
    _compare(_named(key, net), ref, 1e-4, ref32)
    _check_inputs([t.grad for t in gins], gref, gref32, ["points", "normals", "view_dirs", "feature_vectors"])


# ---- 3. NeRF, fp32 ------------------------------------------------------------------------------------------------------
def _nerf_inputs(P):
    p = _rand("np", (P, 3), -4.0, 4.0)
    r = p.norm(dim=1, keepdim=True).clamp(1.0, 1e10)
    return torch.cat([p / r, 1.0 / r], 1), _rand("nd", (P, 3))


def _nerf_net(rend, dpt):
    """The renderer's background network, or (dpt=False) the same weights without the 96-channel head."""
    from dpt_models.fields import NeRF
    if dpt:
        return rend.nerf
    net = NeRF(**dict(rend.nerf.conf, skips=list(rend.nerf.conf["skips"]), gen_depth_feats=False, use_viewdirs=True))
    net.load_state_dict({k: v for k, v in rend.nerf.state_dict().items() if not k.startswith("dpt_linear")})
    net.precision = rend.nerf.precision
    return net.to(rend.nerf.alpha_linear.weight.device)


def _nerf_case(net, dpt, P, dev):
    """device backward of a random linear loss on the background network's outputs + the oracle's loss of the same form"""
    import oracle.neus_oracle as orc
    p4, d = _nerf_inputs(P)
    Rd, Rr, Rf = _rand("nrd", (P, 1)), _rand("nrr", (P, 3)), _rand("nrf", (P, 96))
    gp, gd = p4.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    a, rgb, feat = net(gp, gd)
    loss = (a * Rd.to(dev)).sum() + (rgb * Rr.to(dev)).sum()
    if dpt:
        loss = loss + (feat * Rf.to(dev)).sum()
    loss.backward()

    def ref_loss(o, nets, x, v):
        a_, r_, f_ = o.nerf_forward(nets.nerf, x, v, orc.NeRFConf(gen_depth_feats=dpt))
        l_ = (a_ * Rd.to(x.dtype)).sum() + (r_ * Rr.to(x.dtype)).sum()
        return l_ + (f_ * Rf.to(x.dtype)).sum() if dpt else l_
    return (gp, gd), (p4, d), ref_loss


@pytest.mark.parametrize("dpt", [False, True])
def test_nerf_fp32_vs_oracle(dev, dpt):
    P = 16384         # (ReLU branch flips, see _compare: diluted over more points)
    net = _nerf_net(_rend(dev), dpt)
    (gp, gd), ins, ref_loss = _nerf_case(net, dpt, P, dev)
    ref, gref = _oracle_grads(F64, ref_loss, ["nerf"], ins)
    ref32, gref32 = _oracle_grads(F32, ref_loss, ["nerf"], ins)
    _compare(_named("nerf", net), ref, 1e-4, ref32)
    _check_inputs([gp.grad, gd.grad], gref, gref32, ["input_pts", "input_views"])


# ---- 4. chained, and joined with render() --------------------------------------------------------------------------------
def _chain_dev(rend, x, dirs, R):
    sdf, col = rend.sdf_network, rend.color_network
    out = sdf(x)
    n = sdf.gradient(x)[:, 0]
    return (col(x, n, dirs, out[:, 1:]) * R).sum() + out[:, 0].sum()


def test_chained_vs_oracle_and_joined_with_render(dev):
    P = 2000
    rend = _rend(dev)
    rend.sdf_network.differentiable = rend.color_network.differentiable = True
    x, dirs, R = _rand("cx", (P, 3), -1.1, 1.1), _rand("cd", (P, 3)), _rand("cr", (P, 3))
    _chain_dev(rend, x.to(dev), dirs.to(dev), R.to(dev)).backward()
    mods = (("sdf", rend.sdf_network), ("color", rend.color_network))

    def ref_loss(orc, nets, xx, dd):
        out, grad = orc.sdf_forward(nets.sdf, xx, nets.sdf_conf, with_gradient=True)
        c = orc.rendering_forward(nets.color, xx, grad, dd, out[:, 1:], nets.color_conf)
        return (c * R.to(xx.dtype)).sum() + out[:, 0].sum()
    ref, _ = _oracle_grads(F64, ref_loss, ["sdf", "color"], [x, dirs])
    ref32, _ = _oracle_grads(F32, ref_loss, ["sdf", "color"], [x, dirs])
    named = [(k + "." + n, p) for k, m in mods for n, p in m.named_parameters()]
    _compare(named, ref, 1e-4, ref32)

    # one backward of render() loss + module loss == the two computed separately
    from vdn_train import synth
    cams = synth.make_cameras(0)
    B = 32
    px = np.floor(synth.uniform(0, "mod_ag/px", (B,)) * 400) + 200
    py = np.floor(synth.uniform(0, "mod_ag/py", (B,)) * 400) + 200
    o, d = synth.pixel_rays(cams[0], px, py)
    near, far = synth.near_far_from_sphere(o, d)
    t1, t2 = synth.jitter(0, 0, B)
    gg = lambda a: torch.tensor(a).to(dev)

    def render_loss():
        out = rend.render(gg(o), gg(d), gg(near), gg(far), background_rgb=torch.ones(1, 3, device=dev), cos_anneal_ratio=0.5,
                          t_rand=gg(t1), t_rand_out=gg(t2))
        return out["color_fine"].sum() + out["gradient_error"]
    params = rend._all_parameters()

    def grads(fn):
        for p in params:
            p.grad = None
        fn().backward()
        return [None if p.grad is None else p.grad.clone() for p in params]
    xd, dd, Rd = x.to(dev), dirs.to(dev), R.to(dev)
    ga = grads(render_loss)
    gb = grads(lambda: _chain_dev(rend, xd, dd, Rd))
    gc = grads(lambda: render_loss() + _chain_dev(rend, xd, dd, Rd))
    for a, b, c in zip(ga, gb, gc):
        want = (0 if a is None else a) + (0 if b is None else b)
        if c is None:
            assert a is None and b is None
            continue
        assert _relmax(c, want) <= 1e-6


# ---- 5. bf16 ------------------------------------------------------------------------------------------------------------
def _net_cos(named, ref):
    a = torch.cat([p.grad.detach().double().cpu().reshape(-1) for n, p in named])
    b = torch.cat([ref[n].double().reshape(-1) for n, p in named])
    return _cos(a, b)


@pytest.mark.parametrize("P", [1000, 4096])
def test_bf16_vs_oracle(dev, P):
    """Per network, cosine similarity to the fp64 gradients > 0.99 (the bar of test_gpu_bf16.py)."""
    rend = _rend(dev, "bf16")
    sdf = rend.sdf_network
    # SDF with x requiring grad (rbar + fbar), then the same loss on plain points with the switch on (the one-launch split kernel)
    x = _rand("bx%d" % P, (P, 3), -1.1, 1.1)
    R1, R2 = _rand("br1%d" % P, (P, 257)), _rand("br2%d" % P, (P, 3))
    dev_loss, ref_loss = _sdf_loss("both", R1, R2)
    ref, (gx,) = _oracle_grads(F64, ref_loss, ["sdf"], [x])
    xg = x.to(dev).requires_grad_(True)
    dev_loss(sdf, xg).backward()
    assert _net_cos(_named("sdf", sdf), ref) > 0.99
    assert _cos(xg.grad, gx) > 0.99
    _clear(sdf)
    sdf.differentiable = True
    dev_loss(sdf, x.to(dev)).backward()
    assert _net_cos(_named("sdf", sdf), ref) > 0.99
    # heads: colour, VDN, and a d_feature = 352 colour head
    rend352 = _rend(dev, "bf16", dbc=True)
    for key, net, dbc in (("color", rend.color_network, False), ("vdn", rend.depth_network, False),
                          ("color", rend352.color_network, True)):
        ins = _rn_inputs(P, 352 if dbc else 256)
        R = _rand("bro" + key, (P, net.conf["d_out"]))
        gins = [t.to(dev).requires_grad_(True) for t in ins]
        (net(*gins) * R.to(dev)).sum().backward()
        ref, gref = _oracle_grads(F64, lambda orc, nets, *xs: (orc.rendering_forward(getattr(nets, key), *xs, getattr(nets, key + "_conf"))
                                                               * R.to(xs[0].dtype)).sum(), [key], ins, dbc)
        assert _net_cos(_named(key, net), ref) > 0.99, (key, dbc)
        for t, r in zip(gins, gref):
            assert _cos(t.grad, r) > 0.99, (key, dbc)
    # background network, with and without the dpt head
    for dpt in (True, False):
        net = _nerf_net(rend, dpt)
        (gp, gd), ins, nerf_loss = _nerf_case(net, dpt, P, dev)
        ref, gref = _oracle_grads(F64, nerf_loss, ["nerf"], ins)
        assert _net_cos(_named("nerf", net), ref) > 0.99, dpt
        assert _cos(gp.grad, gref[0]) > 0.99 and _cos(gd.grad, gref[1]) > 0.99, dpt


def test_bf16_weight_grad_plan_follows_the_row_count(dev):
    """The weight-gradient step of the point path on the SAME planes, slab sizes and gradient buffers (so the same device
    addresses) for P = 1000 and P = 999, which share the padded plane rows: each count contracts over exactly its own rows -
    equal, bit for bit, to a plan built from scratch for that count - however the calls alternate."""
    from vdn_hip import points
    from vdn_hip import train as T
    sdf = _rend(dev, "bf16").sdf_network
    Pr = 1024
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: (torch.randn(*shape, device=dev, generator=gen) * 0.1).to(torch.bfloat16)
    H, V, PE, UB, AB = rnd(8, Pr, 256), rnd(8, Pr, 256), rnd(Pr, 64), rnd(Pr * 2144), rnd(Pr * 2336)
    net, grads = points._net_grads(sdf, dev)

    def run(P, out, scratch=False):
        if scratch:
            sdf.__dict__.pop("_pt_plans", None)
        points._weight_grads(sdf, T.sdf_dw_entries(H, V, PE, UB, AB, P, Pr, "bf16"), net, "bf16", float(sdf.scale))
        for o, g in zip(out, grads):
            o.copy_(g)
    seq = (1000, 999, 1000, 999, 999, 1000)
    want = {P: [torch.empty_like(g) for g in grads] for P in (1000, 999)}
    got = [[torch.empty_like(g) for g in grads] for _ in seq]
    for P in (1000, 999):
        run(P, want[P], scratch=True)
    # (no device allocation between the calls below but their own: the slab and column sums of one call land where the
    # previous call's were, so a plan reused across row counts would go unnoticed by an address check)
    for P, out in zip(seq, got):
        run(P, out)
    assert not all(torch.equal(a, b) for a, b in zip(want[1000], want[999]))       # (row 999 enters the P = 1000 sums)
    for P, out in zip(seq, got):
        assert all(torch.equal(a, b) for a, b in zip(out, want[P])), P


@pytest.mark.parametrize("order", [(1000, 999), (999, 1000)])
def test_bf16_row_counts_within_one_padded_block(dev, order):
    """bf16 planes are padded to 32 rows, so P = 999 and P = 1000 share plane sizes (and, through torch's caching allocator,
    usually addresses). Each call's weight gradients must still contract over exactly its own P rows: on a module that just
    ran the other count they equal, bit for bit, those of a fresh module that never did."""
    def run(nets, P):
        x, R = _rand("rc%d" % P, (P, 3), -1.1, 1.1).to(dev), _rand("rcr%d" % P, (P, 257)).to(dev)
        ins = [t.to(dev) for t in _rn_inputs(P, 256)]
        p4, d = (t.to(dev) for t in _nerf_inputs(P))
        sdf, col, nerf = nets
        (sdf(x) * R).sum().backward()                       # plain points: the one-launch split kernel
        (col(*ins) * R[:, :3]).sum().backward()
        sum((t * R[:, :t.shape[1]]).sum() for t in nerf(p4, d)).backward()
        return [p.grad.clone() for m in nets for p in m.parameters()]

    def fresh():
        r = _rend(dev, "bf16")
        nets = (r.sdf_network, r.color_network, r.nerf)
        for m in nets:
            m.differentiable = True
        return nets
    a = fresh()
    run(a, order[0])
    _clear(*a)
    got = run(a, order[1])
    want = run(fresh(), order[1])
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert all(torch.isfinite(g).all() for g in got)


def test_bf16_split_fallback_matches_fp32(dev):
    """P = 950 000 > 919 296: the one-launch split kernel declines, rbar + fbar run (bf16); against the fp32 kernels."""
    P = 950_000
    x = _rand("big", (P, 3), -1.1, 1.1).to(dev)
    R1, R2 = _rand("bigr1", (P, 257)).to(dev), _rand("bigr2", (P, 3)).to(dev)
    dev_loss, _ = _sdf_loss("both", R1, R2)
    grads = {}
    for prec in ("bf16", "fp32"):
        net = _rend(dev, prec).sdf_network
        net.differentiable = True
        dev_loss(net, x).backward()
        grads[prec] = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
        del net
        torch.cuda.empty_cache()
    assert _cos(grads["bf16"], grads["fp32"]) > 0.999


# ---- 6. contract --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_contract(dev, precision):
    rend = _rend(dev, precision)
    P = 777
    x = _rand("kx", (P, 3), -1.1, 1.1).to(dev)
    sdf, col, nerf = rend.sdf_network, rend.color_network, rend.nerf
    ins = [t.to(dev) for t in _rn_inputs(P, 256)]
    p4, d = (t.to(dev) for t in _nerf_inputs(P))
    calls = {"forward": lambda: sdf(x), "sdf": lambda: sdf.sdf(x), "gradient": lambda: sdf.gradient(x),
             "color": lambda: col(*ins), "nerf": lambda: torch.cat([t for t in nerf(p4, d) if t is not None], 1)}
    plain = {}
    for k, f in calls.items():
        y = f()
        assert not y.requires_grad and y.grad_fn is None, k        # flag off, plain inputs: today's graph-less call
        plain[k] = y
    for m in (sdf, col, nerf):
        m.differentiable = True
    with torch.no_grad():
        for k, f in calls.items():
            assert f().grad_fn is None, k
    for k, f in calls.items():
        y = f()
        assert y.grad_fn is not None, k
        assert torch.equal(y.detach(), plain[k]), k                  # graph-building == graph-less, bit for bit
    # determinism: two identical backward calls
    R = torch.randn(P, 3, device=dev)
    xs = x.clone().requires_grad_(True)
    runs = []
    for _ in range(2):
        _clear(sdf, col)
        xs.grad = None
        out = sdf(xs)
        (col(xs, sdf.gradient(xs)[:, 0], ins[2], out[:, 1:]) * R).sum().backward()
        runs.append([xs.grad.clone()] + [p.grad.clone() for m in (sdf, col) for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # second order through the node raises
    xs.grad = None
    # (grad_outputs that require grad: only then does the first differentiation build a graph that a second one could follow)
    go = torch.ones(P, 1, device=dev, requires_grad=True)
    gx, = torch.autograd.grad(sdf.sdf(xs), xs, grad_outputs=go, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gx.sum().backward()
    # an in-place parameter update between forward and backward is reported
    y = sdf.sdf(xs).sum()
    with torch.no_grad():
        next(sdf.parameters()).add_(0.0)
    with pytest.raises(RuntimeError):
        y.backward()
    # mesh extraction stays graph-less
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    sdf.differentiable = False
    V0, F0 = rend.extract_geometry(lo, hi, resolution=48, threshold=0.0)
    sdf.differentiable = True
    V1, F1 = rend.extract_geometry(lo, hi, resolution=48, threshold=0.0)
    assert np.array_equal(np.asarray(V0), np.asarray(V1)) and np.array_equal(np.asarray(F0), np.asarray(F1))


# ---- 7. a short fit -----------------------------------------------------------------------------------------------------
def test_short_sdf_fit_bf16(dev):
    from dpt_models.fields import SDFNetwork
    from vdn_train.factory import CONF
    torch.manual_seed(0)
    net = SDFNetwork(**CONF["sdf_network"]).to(dev)
    net.precision = "bf16"
    net.differentiable = True
    x = _rand("fit", (65536, 3), -1.0, 1.0).to(dev)
    target = x.norm(dim=1, keepdim=True) - 0.35
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        n = net.gradient(x)[:, 0]
        loss = (net.sdf(x) - target).abs().mean() + 0.1 * ((n.norm(dim=1) - 1.0) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] / 10, (losses[0], losses[-1])
