"""CPU-side checks of the standalone networks' autograd support: the explicit-input NeRF adjoint is declared and exported,
malformed argument blocks are refused before anything is launched, the ABI stays additive, and the module switch exists."""
import re

import pytest
import torch

from vdn_hip import lib

NEW = ("vdn_nerf_mlp_bwd_input_f32", "vdn_nerf_mlp_bwd_input_bf16")


def test_new_symbols_declared_and_exported():
    text = open(lib.HEADER).read()
    declared = set(re.findall(r"\bint\s+(vdn_\w+)\s*\(", text))
    l = lib.load()
    for name in NEW:
        assert name in declared and name in lib.FUNCTIONS, name
        assert hasattr(l, name), name
    assert "VdnNerfInputGradArgs" in lib.STRUCTS
    assert [f for f, _ in lib.VdnNerfInputGradArgs._fields_] == ["pts4", "dirs", "d_pts4", "d_dirs", "accumulate"]


def test_abi_version_unchanged():
    assert lib.load().vdn_abi_version() == 28


@pytest.mark.parametrize("name", NEW)
def test_malformed_argument_blocks_are_refused(name):
    b, ig = lib.VdnNerfBwdArgs(), lib.VdnNerfInputGradArgs()
    with pytest.raises(lib.VdnError):
        lib.call(name, b, ig, None)                    # empty blocks
    with pytest.raises(lib.VdnError):
        lib.call(name, None, None, None)               # null blocks
    # a complete backward block (fake, never dereferenced) with an empty input block: refused, nothing launched
    for f in ("blob", "g_density", "g_rgb", "save_h", "save_hv", "delta_o", "delta_v", "delta_head", "delta_h"):
        setattr(b, f, 16)
    b.P = 32
    with pytest.raises(lib.VdnError):
        lib.call(name, b, ig, None)
    with pytest.raises(lib.VdnError):
        lib.call(name, b, None, None)
    # the ray-regenerated adjoint and the explicit one are exclusive
    ig.pts4 = ig.dirs = ig.d_pts4 = ig.d_dirs = 16
    b.d_pts = 16
    with pytest.raises(lib.VdnError):
        lib.call(name, b, ig, None)


def test_differentiable_switch_defaults_off():
    from dpt_models import fields
    from vdn_train import factory
    rend = factory.build_renderer(wdepth=True, device="cpu")
    for m in (rend.sdf_network, rend.color_network, rend.depth_network, rend.nerf):
        assert m.differentiable is False
        assert not m._graph_wanted(torch.zeros(2, 3))
        assert m._graph_wanted(torch.zeros(2, 3, requires_grad=True))
        m.differentiable = True
        assert m._graph_wanted(torch.zeros(2, 3))
        with torch.no_grad():
            assert not m._graph_wanted(torch.zeros(2, 3, requires_grad=True))
    assert fields._HipNet.differentiable is False


def test_module_graph_path_has_no_cpu_fallback():
    from vdn_train import factory
    rend = factory.build_renderer(device="cpu")
    rend.sdf_network.differentiable = True
    with pytest.raises(RuntimeError):
        rend.sdf_network(torch.zeros(4, 3, requires_grad=True))
