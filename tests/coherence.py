"""Weight-coherence harness (tests/test_gpu_weight_coherence.py holds the assertions).

Between torch's Parameters and every kernel sits a layer of caches: the weight images (vdn_hip/images.py: NetImages, rebuilt when a
version counter, an address or an object changes), trust() / refresh_together() and their table caches, the Trainer's raw-pointer Adam,
its _stream_join hooks, the renderer's engines, the captured graphs (_TrainPlan, RenderPlan: raw pointers to the blobs, to row 0 of W8 and
to the variance itself) and the NeRF scratch buffer. If one of them goes stale every kernel is still bit-exact - on the wrong weights.

The method: a renderer whose caches all exist, a ROUTE that changes its weights, then every CONSUMER on it against the same consumer
on its `twin` - a renderer freshly built from the changed state_dict, which has never seen another weight - with torch.equal.

A renderer under test always has a Trainer attached from the start (as a training process has), with learning rate 0: its step is a
consumer (the scalars it returns) that leaves the weights as they are; the `trainer_step` route switches the rate on for its steps.

Routes that move storage return the old tensors, and the caller keeps them until the test ends: whatever a stale pointer reads is
then old, never freed, memory. Nothing here empties the allocator's cache."""
import contextlib
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vdn-nerf_amd")
for _p in (PKG, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

DEV = torch.device("cuda:0")
SEED = 3
B_RAGGED, B_PLAN = 77, 64        # 77: a ragged last workgroup; 64: the graph plans' and the Trainer's batch
N_POINTS = 300                   # not a multiple of 128
RESOLUTION = 16
NETS = ("nerf", "sdf_network", "color_network", "depth_network")
CK_KEYS = {"nerf": "nerf", "sdf_network": "sdf_network_fine", "deviation_network": "variance_network_fine",
           "color_network": "color_network_fine", "depth_network": "depth_network_fine"}
# (anneal_end = 0: the compositor's annealing ratio is 1 at every step - a Trainer's scalars then depend on the weights alone,
# not on how many steps it has taken)
TRAIN_CONF = dict(learning_rate=0.0, warm_up_end=0, end_iter=1000, anneal_end=0, depth_start_iter=-1)
STEP_LR = 5e-4

_STATE = {}              # shared, read-only inputs
_ATTACHED = {}           # id(renderer) -> dict(rend=, trainer=, plan=): the harness's own per-renderer objects (never inside the renderer)


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def forget():
    """Drop every Trainer / plan the harness attached (end of a test)."""
    _ATTACHED.clear()


def _slot(rend):
    return _ATTACHED.setdefault(id(rend), dict(rend=rend, trainer=None, plan=None, retired=[]))


def networks(rend):
    return [(n, getattr(rend, n)) for n in NETS if getattr(rend, n) is not None]


def all_modules(rend):
    return networks(rend) + [("deviation_network", rend.deviation_network)]


def named_params(rend):
    return [(n + "." + k, p) for n, m in all_modules(rend) for k, p in m.named_parameters()]


# ---------------------------------------------------------------------------------------------------------------------------
# fixed inputs (made once, shared, never written)
# ---------------------------------------------------------------------------------------------------------------------------
def rays(B):
    key = ("rays", B)
    if key not in _STATE:
        from vdn_train import synth
        cams = synth.make_cameras(SEED)
        o, d = synth.random_pixel_batch(SEED, 1, 1, B, rank=0, cams=cams, crop=500)
        near, far = synth.near_far_from_sphere(o, d)
        t1, t2 = synth.jitter(SEED, 1, B)
        rgb = synth.target_colors(o, d, albedo=0.8)
        _STATE[key] = tuple(torch.tensor(x).to(DEV) for x in (o, d, near, far, t1, t2, rgb))
    return _STATE[key]


def points():
    if "points" not in _STATE:
        g = torch.Generator().manual_seed(SEED)
        r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
        pts, nrm, dirs = r(N_POINTS, 3) * 1.1, r(N_POINTS, 3), torch.nn.functional.normalize(r(N_POINTS, 3), dim=1)
        feat = r(N_POINTS, 256) * 0.5
        p4 = torch.cat([torch.nn.functional.normalize(r(N_POINTS, 3), dim=1), torch.rand(N_POINTS, 1, generator=g)], dim=1)
        _STATE["points"] = tuple(t.to(DEV) for t in (pts, nrm, dirs, feat, p4))
    return _STATE["points"]


def loss_weights(name, shape):
    """Fixed coefficients of the linear loss on output `name`."""
    key = ("w", name, tuple(shape))
    if key not in _STATE:
        g = torch.Generator().manual_seed(SEED + sum(map(ord, name)))
        _STATE[key] = (torch.rand(tuple(shape), generator=g) + 0.5).to(DEV)
    return _STATE[key]


def base_states(wdepth=True):
    key = ("states", wdepth)
    if key not in _STATE:
        from vdn_train import synth
        _STATE[key] = synth.make_all_states(SEED, wdepth=wdepth)
    return _STATE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# renderers
# ---------------------------------------------------------------------------------------------------------------------------
def attach_trainer(rend):
    """A new Trainer on `rend` (it re-points every parameter into its own flat buffer), kept beside it."""
    from vdn_train.trainer import Trainer
    tr = Trainer(rend, B_PLAN, DEV, conf=dict(TRAIN_CONF))
    slot = _slot(rend)
    if slot["trainer"] is not None:
        slot["retired"].append(slot["trainer"])        # (its flat buffer is the storage the parameters just left: it stays alive)
    slot["trainer"] = tr
    return tr


def trainer_of(rend):
    """The renderer's Trainer; a new one when the old one no longer fits - its parameters moved or were replaced, or the precision
    changed: such a Trainer raises at its next step, and the user has to build another."""
    tr = _slot(rend)["trainer"]
    if tr is not None:
        eng = tr.engine
        same = (eng._ptr_key() == eng._param_ptrs and eng.precision == rend.precision
                and all(a is b for a, b in zip(tr._params, rend._all_parameters()))
                and all(p.data_ptr() == tr._param_flat.data_ptr() + 4 * off for p, off in zip(tr._params, _offsets(tr._params))))
        if not same:
            tr = None
    return tr if tr is not None else attach_trainer(rend)


def _offsets(params):
    off, out = 0, []
    for p in params:
        out.append(off)
        off += p.numel()
    return out


def make(precision, wdepth=True):
    """A renderer of the shipped family with synthetic weights and its Trainer."""
    from vdn_train import factory
    rend = factory.build_renderer(wdepth=wdepth, device=DEV, states=base_states(wdepth), precision=precision)
    attach_trainer(rend)
    return rend


def twin(rend, trainer=True):
    """A renderer freshly built by factory.build_renderer(states=...) from the current state_dict() of `rend`'s five networks: same
    precision, wdepth and renderer overrides. It has never seen another weight: its images are built once, from the final values."""
    from vdn_train import factory
    states = {}
    for n, m in all_modules(rend):
        join = getattr(m, "_join_trainer", None)
        if join is not None:
            join()                         # (the reference must read complete values: a Trainer's side-stream half may be in flight)
        states[CK_KEYS[n]] = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    states.setdefault("depth_network_fine", None)
    over = {k: getattr(rend, k) for k in ("n_samples", "n_importance", "n_outside", "up_sample_steps", "perturb")}
    assert rend.precision in ("fp32", "bf16")
    tw = factory.build_renderer(wdepth=rend.depth_network is not None, device=DEV, states=states, precision=rend.precision, **over)
    if trainer:
        attach_trainer(tw)
    return tw


# ---------------------------------------------------------------------------------------------------------------------------
# consumers: (renderer) -> {name: tensor}
# ---------------------------------------------------------------------------------------------------------------------------
RENDER_KW = dict(perturb_overwrite=0, cos_anneal_ratio=0.7)
LOSS_KEYS = ("color_fine", "weights", "render_feats", "weight_sum", "gradient_error", "s_val")


def _bg():
    if "bg" not in _STATE:
        _STATE["bg"] = torch.ones(1, 3, device=DEV)
    return _STATE["bg"]


def _clone(out):
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


def c_render_nograd(rend):
    o, d, near, far = rays(B_RAGGED)[:4]
    with torch.no_grad():
        return _clone(rend.render(o, d, near, far, background_rgb=_bg(), **RENDER_KW))


def _render_grad(rend, B):
    o, d, near, far = rays(B)[:4]
    out = rend.render(o, d, near, far, background_rgb=_bg(), **RENDER_KW)
    loss = sum((out[k] * loss_weights(k, out[k].shape)).sum() for k in LOSS_KEYS if out.get(k) is not None)
    names, params = zip(*named_params(rend))
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    res = _clone(out)
    for n, g in zip(names, grads):
        assert g is not None, n
        res["grad/" + n] = g.detach().clone()
    return res


def c_render_grad_eager(rend):
    """render() under grad as the first call of a configuration runs it: every launch issued eagerly."""
    with environ(VDN_RENDER_GRAPHS="0"):
        return _render_grad(rend, B_RAGGED)


def c_render_grad_replay(rend):
    """... and called until its _TrainPlan exists and replays (forward and backward graphs)."""
    with environ(VDN_RENDER_GRAPHS="1"):
        for _ in range(3):
            res = _render_grad(rend, B_PLAN)
    plans = [pl for k, eng in rend.__dict__["_engines"].items() if k[0] == B_PLAN for pl in eng.__dict__.get("_plans", {}).values()]
    assert plans and all(pl.bwd and all(pl.bwd.values()) for pl in plans), "render() under grad did not reach its graph plans"
    return res


def c_render_plan(rend):
    """A RenderPlan built at the first call - before the route - and called after it."""
    slot = _slot(rend)
    o, d, near, far = rays(B_PLAN)[:4]
    with torch.no_grad():
        if slot["plan"] is None:
            slot["plan"] = rend.plan(B_PLAN, background_rgb=_bg(), **RENDER_KW)
        return _clone(slot["plan"](o, d, near, far))


def _lin(name, t):
    return (t * loss_weights(name, t.shape)).sum()


def c_modules(rend):
    pts, nrm, dirs, feat, p4 = points()
    sn, cn, dn, nf = rend.sdf_network, rend.color_network, rend.depth_network, rend.nerf
    res = {}
    with torch.no_grad():
        res["sdf"], res["gradient"], res["forward"] = sn.sdf(pts), sn.gradient(pts), sn(pts)
        res["color"] = cn(pts, nrm, dirs, feat)
        if dn is not None:
            res["vdn"] = dn(pts, nrm, dirs, feat)
        dens, rgb, nfeat = nf(p4, dirs)
        res["nerf/density"], res["nerf/rgb"] = dens, rgb
        if nfeat is not None:
            res["nerf/feat"] = nfeat

    def with_grad(tag, module, fn, inputs):
        """The vdn_hip/points.py path: inputs that require grad; gradients of a fixed linear loss to them and to every parameter."""
        xs = [t.clone().requires_grad_(True) for t in inputs]
        outs = fn(*xs)
        outs = [t for t in (outs if isinstance(outs, tuple) else (outs,)) if t is not None]
        loss = sum(_lin("%s/%d" % (tag, i), t) for i, t in enumerate(outs))
        names, params = zip(*module.named_parameters())
        grads = torch.autograd.grad(loss, list(xs) + list(params), allow_unused=True)
        for i, t in enumerate(outs):
            res["%s/out%d" % (tag, i)] = t
        for n, g in zip(["in%d" % i for i in range(len(xs))] + list(names), grads):
            assert g is not None, (tag, n)
            res["%s/grad/%s" % (tag, n)] = g
    with_grad("g_forward", sn, lambda x: sn(x), [pts])
    with_grad("g_sdf", sn, lambda x: sn.sdf(x), [pts])
    with_grad("g_gradient", sn, lambda x: sn.gradient(x), [pts])
    with_grad("g_color", cn, lambda a, b, c, f: cn(a, b, c, f), [pts, nrm, dirs, feat])
    if dn is not None:
        with_grad("g_vdn", dn, lambda a, b, c, f: dn(a, b, c, f), [pts, nrm, dirs, feat])
    with_grad("g_nerf", nf, lambda a, b: nf(a, b), [p4, dirs])
    return _clone(res)


def c_shade_points(rend):
    from vdn_hip import mesh
    sdf, grad, col = mesh.shade_points(rend, points()[0])
    return _clone(dict(sdf=sdf, gradient=grad, color=col))


def c_lattice(rend):
    u = rend.extract_fields([-1.01, -1.01, -1.01], [1.01, 1.01, 1.01], RESOLUTION)
    return dict(u=torch.from_numpy(np.ascontiguousarray(u)))


def _train_step(tr):
    o, d, near, far, t1, t2, rgb = rays(B_PLAN)
    return tr.train_step(o, d, near, far, rgb, t_rand=t1, t_rand_out=t2)


def c_trainer_scalars(rend):
    """The scalars Trainer.train_step returns on its next step (learning rate 0: the step leaves the weights as they are, bit for
    bit - p - 0 * x - and still runs the whole schedule, refresh_together() included)."""
    tr = trainer_of(rend)
    assert tr.conf["learning_rate"] == 0.0
    sc = _train_step(tr).clone()
    return dict(scalars=sc)


# (order matters in one place: the Trainer's step rebuilds every weight image, so it runs last - in front of the others it would
# repair what they are there to catch)
CONSUMERS = {"render_nograd": c_render_nograd, "render_grad_eager": c_render_grad_eager, "render_grad_replay": c_render_grad_replay,
             "render_plan": c_render_plan, "modules": c_modules, "shade_points": c_shade_points, "lattice": c_lattice,
             "trainer_scalars": c_trainer_scalars}
# the networks each consumer's outputs depend on ("var": the variance)
DEPENDS = {"render_nograd": {"nerf", "sdf", "color", "vdn", "var"}, "render_grad_eager": {"nerf", "sdf", "color", "vdn", "var"},
           "render_grad_replay": {"nerf", "sdf", "color", "vdn", "var"}, "render_plan": {"nerf", "sdf", "color", "vdn", "var"},
           "modules": {"nerf", "sdf", "color", "vdn"}, "shade_points": {"sdf", "color"}, "lattice": {"sdf"},
           "trainer_scalars": {"nerf", "sdf", "color", "var"}}


def consume(rend, only=None):
    """Every consumer on `rend`, in order -> {consumer: {name: tensor}}."""
    return {name: fn(rend) for name, fn in CONSUMERS.items() if only is None or name in only}


def differing(a, b):
    """[(consumer, tensor name)] where two consume() results are not bit-identical (a missing tensor differs)."""
    out = []
    for c in a:
        for k in sorted(set(a[c]) | set(b[c])):
            if k not in a[c] or k not in b[c] or a[c][k].shape != b[c][k].shape or not torch.equal(a[c][k], b[c][k]):
                out.append((c, k))
    return out


def max_abs_diff(a, b, consumer):
    return max(float((a[consumer][k].double() - b[consumer][k].double()).abs().max()) for k in a[consumer])


# ---------------------------------------------------------------------------------------------------------------------------
# routes: (renderer) -> (networks touched, [old tensors to keep alive])
# ---------------------------------------------------------------------------------------------------------------------------
ALL = {"nerf", "sdf", "color", "vdn", "var"}
_SHORT = {"nerf": "nerf", "sdf_network": "sdf", "color_network": "color", "depth_network": "vdn", "deviation_network": "var"}


def _change_(p):
    """The change every route makes, in place on tensor `p`: x 1.01, or + 0.003 (biases start at zero: scaling moves nothing)."""
    if p.dim() <= 1:
        p.add_(0.003)
    else:
        p.mul_(1.01)


def _changed(t):
    return t + 0.003 if t.dim() <= 1 else t * 1.01


def r_inplace(rend):
    with torch.no_grad():
        for _, p in named_params(rend):
            _change_(p)
    return ALL, []


def _only(suffix):
    def route(rend):
        hit = set()
        with torch.no_grad():
            for n, p in named_params(rend):
                if n.endswith(suffix):
                    p.mul_(1.01) if suffix == "weight_g" else p.add_(0.003)
                    hit.add(_SHORT[n.split(".")[0]])
        return hit, []
    return route


def _adam(**kw):
    def route(rend):
        import pytest
        params = [p for _, p in named_params(rend)]
        try:
            opt = torch.optim.Adam(params, lr=1e-3, **kw)
        except (RuntimeError, ValueError) as e:
            pytest.skip("torch.optim.Adam(%s) is refused here: %s" % (kw, e))
        o, d, near, far = rays(B_PLAN)[:4]
        out = rend.render(o, d, near, far, background_rgb=_bg(), **RENDER_KW)
        sum((out[k] * loss_weights(k, out[k].shape)).sum() for k in LOSS_KEYS if out.get(k) is not None).backward()
        assert all(p.grad is not None for p in params)
        try:
            opt.step()
        except RuntimeError as e:
            if not kw.get("fused"):
                raise
            pytest.skip("torch.optim.Adam(fused=True) is refused on this device: %s" % e)
        for p in params:
            p.grad = None
        return ALL, []
    return route


def r_load_state_dict(rend):
    for _, m in all_modules(rend):
        m.load_state_dict({k: _changed(v) for k, v in m.state_dict().items()})
    return ALL, []


def r_load_state_dict_assign(rend):
    keep = [p for _, p in named_params(rend)]
    for _, m in all_modules(rend):
        m.load_state_dict({k: _changed(v.detach()).clone() for k, v in m.state_dict().items()}, assign=True)
    assert all(a is not b for a, (_, b) in zip(keep, named_params(rend)))
    return ALL, keep


def r_setattr_parameter(rend):
    """One layer's Parameter object replaced, in every network (and the variance)."""
    keep = []

    def swap(holder, name):
        old = getattr(holder, name)
        keep.append(old)
        setattr(holder, name, nn.Parameter(_changed(old.detach()).clone()))
    swap(rend.sdf_network.lin3, "weight_v")
    swap(rend.color_network.lin1, "weight_g")
    swap(rend.nerf.pts_linears[5], "weight")
    if rend.depth_network is not None:
        swap(rend.depth_network.lin4, "bias")
    swap(rend.deviation_network, "variance")
    return ALL, keep


def r_data_rebind(rend):
    keep = []
    for _, p in named_params(rend):
        keep.append(p.data)
        p.data = _changed(p.data)
    return ALL, keep


def r_cpu_and_back(rend):
    keep = [p.data for _, p in named_params(rend)]
    for _, m in all_modules(rend):
        m.to("cpu")
    with torch.no_grad():
        for _, p in named_params(rend):
            _change_(p)
    for _, m in all_modules(rend):
        m.to(DEV)
    return ALL, keep


def r_data_inplace(rend):
    """Writes through .data - invisible to torch's version counters - followed by the call that says so."""
    for _, p in named_params(rend):
        _change_(p.data)
    rend.weights_changed()
    return ALL, []


def r_trainer_construct(rend):
    """A Trainer built after every consumer has run: every parameter moves into its flat buffer."""
    keep = [None, [p.data for _, p in named_params(rend)]]
    attach_trainer(rend)
    assert all(a.data_ptr() != p.data_ptr() for a, (_, p) in zip(keep[1], named_params(rend)))
    r_inplace(rend)
    return ALL, keep


def r_trainer_step(rend):
    """Two steps of the fused training loop (raw-pointer Adam on two streams); no join() behind them."""
    tr = trainer_of(rend)
    tr.conf["learning_rate"] = STEP_LR
    try:
        for _ in range(2):
            _train_step(tr)
    finally:
        tr.conf["learning_rate"] = 0.0
    return {"nerf", "sdf", "color", "var"}, []          # (the depth loss is off: the VDN head has no gradient)


def r_trainer_load_checkpoint(rend):
    tr = trainer_of(rend)
    ck = tr.state_dict()
    for key in CK_KEYS.values():
        if ck.get(key) is not None:
            ck[key] = {k: _changed(v) for k, v in ck[key].items()}
    tr.load_checkpoint(ck)
    return ALL, []


ROUTES = {
    "inplace": r_inplace, "g_only": _only("weight_g"), "bias_only": _only("bias"), "variance_only": _only("variance"),
    "adam_single": _adam(foreach=False), "adam_foreach": _adam(foreach=True), "adam_fused": _adam(fused=True),
    "load_state_dict": r_load_state_dict, "load_state_dict_assign": r_load_state_dict_assign,
    "setattr_parameter": r_setattr_parameter, "data_rebind": r_data_rebind, "cpu_and_back": r_cpu_and_back,
    "data_inplace": r_data_inplace, "trainer_construct": r_trainer_construct, "trainer_step": r_trainer_step,
    "trainer_load_checkpoint": r_trainer_load_checkpoint,
    # the two routes with a flow of their own (run_cell below)
    "precision_round_trip": None, "deepcopy_then_change_copy": None,
}


# ---------------------------------------------------------------------------------------------------------------------------
# one cell of the matrix
# ---------------------------------------------------------------------------------------------------------------------------
def check_against_twin(rend, got, what, tol=None):
    """`got` = consume(rend) must equal consume(twin(rend)) bit for bit (tol: {consumer: max |a - b|} for a consumer whose control
    is not bit-identical)."""
    want = consume(twin(rend))
    bad = differing(got, want)
    if tol:
        bad = [(c, k) for c, k in bad if c not in tol or float((got[c][k].double() - want[c][k].double()).abs().max()) > tol[c]]
    assert not bad, "%s: %d tensors differ from its twin, e.g. %s" % (what, len(bad), bad[:8])
    return want


def check_moved(before, after, touched, what):
    """A route that did not move the outputs proves nothing: every consumer that depends on a touched network must have moved."""
    moved = {c for c, _ in differing(before, after)}
    still = [c for c in after if (DEPENDS[c] & touched) and c not in moved]
    assert not still, "%s: vacuous - the route did not move the output of %s" % (what, still)


def run_cell(route, precision, tol=None, keep=None):
    """Consumers, route, consumers again, twin. `keep`: a list that receives everything that must stay alive until the test ends."""
    keep = [] if keep is None else keep
    rend = make(precision)
    keep.append(rend)
    before = consume(rend)
    what = "%s/%s" % (route, precision)
    if route == "precision_round_trip":
        other = "fp32" if precision == "bf16" else "bf16"
        rend.precision = other
        touched, old = r_inplace(rend)
        mid = consume(rend)
        check_against_twin(rend, mid, what + " at " + other, tol)
        rend.precision = precision
        after = consume(rend)
        check_against_twin(rend, after, what + " back at " + precision, tol)
        check_moved(before, after, touched, what)
        return
    if route == "deepcopy_then_change_copy":
        cp = copy.deepcopy(rend)
        keep.append(cp)
        touched, old = r_inplace(cp)
        again = consume(rend)
        bad = differing(before, again)
        assert not bad, "%s: changing the copy changed the original: %s" % (what, bad[:8])
        after = consume(cp)
        check_against_twin(cp, after, what + " (the copy)", tol)
        check_moved(before, after, touched, what)
        return
    touched, old = ROUTES[route](rend)
    keep.append(old)
    after = consume(rend)
    check_against_twin(rend, after, what, tol)
    check_moved(before, after, touched, what)
