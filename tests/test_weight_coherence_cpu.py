"""Host side of weight coherence (tests/test_gpu_weight_coherence.py holds the device side).

No kernel reads a Parameter: they read vdn_hip.images.NetImages, rebuilt when its staleness predicate fires. The predicate can only
see what torch lets it see - a parameter's `_version`, its `data_ptr()` and its identity - so this file (1) pins, for the installed
torch, which way of changing a weight moves which of the three (a torch upgrade that changes a row fails here, not silently on the
device), and (2) drives the predicate itself on CPU-resident NetImages, where no launch is needed: after every detectable route
`stale()` is true and the descriptor tables hold the new addresses and objects; after a write through `.data` it is NOT - the
documented limit of automatic detection - until weights_changed() is called."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from vdn_hip import images, lib
from vdn_train import factory, synth


# ---------------------------------------------------------------------------------------------------------------------------
# 1. what torch shows of each route: (bumps _version, moves data_ptr(), replaces the Parameter object)
# ---------------------------------------------------------------------------------------------------------------------------
def _adam(**kw):
    def route(m):
        m(torch.ones(2, 3)).sum().backward()
        torch.optim.Adam(m.parameters(), lr=1e-3, **kw).step()
    return route


def _no_grad_add(m):
    with torch.no_grad():
        m.weight.add_(0.003)


def _load_state_dict(assign):
    def route(m):
        m.load_state_dict({k: v * 1.01 for k, v in m.state_dict().items()}, assign=assign)
    return route


def _rebind(m):
    m.weight.data = m.weight.data * 1.01


TORCH_TABLE = {
    # route: (callable on an nn.Linear(3, 4), bumps _version, moves data_ptr(), replaces the object)
    "data_add_": (lambda m: m.weight.data.add_(0.003), False, False, False),
    "data_copy_": (lambda m: m.weight.data.copy_(m.weight.data * 1.01), False, False, False),
    "data_rebind": (_rebind, False, True, False),
    "no_grad_add_": (_no_grad_add, True, False, False),
    "detach_mul_": (lambda m: m.weight.detach().mul_(1.01), True, False, False),
    "load_state_dict": (_load_state_dict(False), True, False, False),
    "nn_init": (lambda m: nn.init.normal_(m.weight), True, False, False),
    "adam_single": (_adam(foreach=False), True, False, False),
    "adam_foreach": (_adam(foreach=True), True, False, False),
    # the fused multi-tensor kernel bumps nothing: vdn_hip.images._fused_step_hook stands in for the version counter
    "adam_fused": (_adam(fused=True), False, False, False),
    "load_state_dict_assign": (_load_state_dict(True), None, True, True),
}


@pytest.mark.parametrize("route", sorted(TORCH_TABLE))
def test_what_torch_shows_of_each_route(route):
    fn, bumps, moves, replaces = TORCH_TABLE[route]
    torch.manual_seed(0)
    m = nn.Linear(3, 4)
    p, before = m.weight, m.weight.detach().clone()
    version, ptr = p._version, p.data_ptr()
    fn(m)
    assert not torch.equal(m.weight.detach(), before), "the route changed nothing"
    assert (m.weight is not p) == replaces
    assert (m.weight.data_ptr() != ptr) == moves
    if bumps is not None:                      # (a replaced object has a counter of its own: nothing to compare)
        assert (m.weight._version != version) == bumps


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the staleness predicate on CPU-resident images
# ---------------------------------------------------------------------------------------------------------------------------
def _nets(precision="bf16"):
    rend = factory.build_renderer(wdepth=True, device="cpu", states=synth.make_all_states(2, wdepth=True), precision=precision)
    return rend, {"sdf": rend.sdf_network, "color": rend.color_network, "vdn": rend.depth_network, "nerf": rend.nerf}


def _fresh_images(net):
    """NetImages of `net` on the CPU device (as tests/test_boundary_cpu.py builds the descriptor tables), following the module's
    current parameters as _HipNet._image_state makes it, and marked fresh the way refresh() / refresh_together() do."""
    fmt = images.FMT_F32 if net.precision == "fp32" else images.FMT_BF16
    im = images.NetImages(net._matrices(), net._streams(), torch.device("cpu"), fmt, source=net)
    assert im.stale()                          # never built
    im.mark_fresh()
    assert not im.stale()
    return im


def _a_layer(net):
    """One weight-carrying layer holder of the network (its triple has a bias and a v / weight)."""
    return net.lin3 if hasattr(net, "lin3") else net.pts_linears[5]


def _v(layer):
    return layer.weight_v if hasattr(layer, "weight_v") else layer.weight


def _set_v(layer, p):
    if hasattr(layer, "weight_v"):
        layer.weight_v = p
    else:
        layer.weight = p


def _r_no_grad(net):
    with torch.no_grad():
        _v(_a_layer(net)).mul_(1.01)


def _r_bias(net):
    with torch.no_grad():
        _a_layer(net).bias.add_(0.003)


def _r_g(net):
    with torch.no_grad():
        t = _a_layer(net).triple()[0]
        (t if t is not None else _a_layer(net).bias).mul_(1.01)


def _r_detach(net):
    _v(_a_layer(net)).detach().mul_(1.01)


def _r_init(net):
    nn.init.normal_(_v(_a_layer(net)), std=0.05)


def _r_load(net):
    net.load_state_dict({k: v * 1.01 for k, v in net.state_dict().items()})


def _r_adam(**kw):
    def route(net):
        ps = list(net.parameters())
        for p in ps:
            p.grad = torch.ones_like(p)
        torch.optim.Adam(ps, lr=1e-3, **kw).step()
        for p in ps:
            p.grad = None
    return route


def _r_rebind(net):
    p = _v(_a_layer(net))
    keep = p.data
    p.data = keep * 1.01
    return keep


def _r_assign(net):
    keep = list(net.parameters())
    net.load_state_dict({k: v * 1.01 for k, v in net.state_dict().items()}, assign=True)
    return keep


def _r_setattr(net):
    layer = _a_layer(net)
    keep = _v(layer)
    _set_v(layer, nn.Parameter(keep.detach() * 1.01))
    return keep


def _r_setattr_same_storage(net):
    """A new Parameter object on the OLD storage: no address moves and the orphan's version counter is the one that stays put."""
    layer = _a_layer(net)
    keep = _v(layer)
    _set_v(layer, nn.Parameter(keep.data))
    with torch.no_grad():
        _v(layer).mul_(1.01)
    return keep


DETECTED = {"no_grad_mul_": _r_no_grad, "bias_only": _r_bias, "g_only": _r_g, "detach_mul_": _r_detach, "nn_init": _r_init,
            "load_state_dict": _r_load, "adam_single": _r_adam(foreach=False), "adam_foreach": _r_adam(foreach=True),
            "adam_fused": _r_adam(fused=True), "data_rebind": _r_rebind,
            "load_state_dict_assign": _r_assign, "setattr_parameter": _r_setattr, "setattr_same_storage": _r_setattr_same_storage}


def _table_pointers(im):
    wn = np.frombuffer(im.wn_table.numpy().tobytes(), dtype=lib.struct_dtype("VdnWeightNormDesc"))
    ch = np.frombuffer(im.chunk_table.numpy().tobytes(), dtype=lib.struct_dtype("VdnChunkDesc"))
    return {int(x) for d in wn for x in (d["g"], d["v"])} | {int(d["bias"]) for d in ch}


@pytest.mark.parametrize("route", sorted(DETECTED))
@pytest.mark.parametrize("which", ["sdf", "color", "vdn", "nerf"])
def test_every_detectable_route_makes_the_images_stale(route, which):
    rend, nets = _nets()
    net = nets[which]
    im = _fresh_images(net)
    others = {k: _fresh_images(n) for k, n in nets.items() if k != which}
    keep = DETECTED[route](net)                # (old tensors stay referenced: no address can be recycled under the comparison)
    assert im.stale(), "the route went unnoticed"
    # stale() has brought the tables up to date: they name the module's CURRENT parameters, objects and addresses
    cur = lib.module_params(net)
    assert len(im._params()) == len(cur) and {id(t) for t in im._params()} == {id(p) for p in cur}
    assert {id(t) for n in im.matrices for t in im.matrices[n] if t is not None} == {id(p) for p in cur}
    assert {p.data_ptr() for p in cur} <= _table_pointers(im) | {0}
    assert all(t.data_ptr() in _table_pointers(im) for t in im._params())
    # ... a build later the images are fresh again, and nobody else was disturbed
    builds = im.builds
    im.mark_fresh()
    assert not im.stale() and im.builds == builds + 1
    assert not any(o.stale() for o in others.values())
    del keep


@pytest.mark.parametrize("which", ["sdf", "color", "vdn", "nerf"])
def test_data_inplace_needs_weights_changed(which):
    """`p.data.mul_()` moves no version counter and no address: stale() cannot see it (the documented limit). weights_changed() on
    the network - or on the renderer - says it."""
    rend, nets = _nets()
    net = nets[which]
    net.__dict__["_img"] = im = _fresh_images(net)         # (where _HipNet keeps it: weights_changed() finds it there)
    builds = im.builds
    before = _v(_a_layer(net)).detach().clone()
    _v(_a_layer(net)).data.mul_(1.01)
    assert not torch.equal(_v(_a_layer(net)).detach(), before)
    assert not im.stale()
    net.weights_changed()
    assert im.stale() and im.builds == builds + 1          # (`builds` moves too: the NeRF scratch buffer is keyed on it)
    im.mark_fresh()
    _a_layer(net).bias.data.add_(0.003)
    assert not im.stale()
    rend.weights_changed()
    assert im.stale()


def test_weights_changed_before_first_use_is_harmless():
    rend, nets = _nets()
    rend.weights_changed()
    assert all("_img" not in n.__dict__ for n in nets.values())


def test_replaced_parameter_of_another_shape_is_refused():
    rend, nets = _nets()
    net = nets["sdf"]
    im = _fresh_images(net)
    net.lin3.weight_v = nn.Parameter(torch.zeros(100, 256))
    with pytest.raises(RuntimeError, match="shapes"):
        im.stale()


def test_rebuilt_tables_never_share_a_cache_key():
    """refresh_together() caches the concatenated tables under NetImages.tables_gen: every build of any image set in the process
    gets a number of its own (an address, which the allocator recycles, is not one)."""
    rend, nets = _nets()
    seen = set()
    for net in nets.values():
        im = _fresh_images(net)
        for _ in range(3):
            assert im.tables_gen not in seen and im.tables_gen > 0
            seen.add(im.tables_gen)
            keep = _r_rebind(net)
            assert im.stale()
            del keep


def test_deepcopy_and_pickle_carry_no_device_state():
    import copy
    import pickle
    rend, nets = _nets()
    for n in nets.values():
        n.__dict__["_img"] = _fresh_images(n)
    rend.__dict__["_engines"] = {"k": object()}
    rend.__dict__["_img_tables"] = {"key": 1}
    for cp in (copy.deepcopy(rend), pickle.loads(pickle.dumps(rend))):
        assert "_engines" not in cp.__dict__ and "_img_tables" not in cp.__dict__ and cp._const_cache == {}
        for name in ("sdf_network", "color_network", "depth_network", "nerf"):
            a, b = getattr(rend, name), getattr(cp, name)
            assert "_img" not in b.__dict__ and "_img" in a.__dict__
            assert all(torch.equal(x, y) and x.data_ptr() != y.data_ptr() for x, y in zip(a.parameters(), b.parameters()))
        assert cp.precision == rend.precision and cp.n_samples == rend.n_samples
