"""Coloured mesh export: vdn_shade_points_bf16 (csrc/k_sdf_fwd2.h MODE 4) - SDF network + gradient sweep + colour head on
free-standing points, each seen straight down its own normal - against the separate launches of the same bf16 path, the
exact-fp32 arm of vdn_hip.mesh.shade_points against the fp64 oracle, and the way from the lattice to a PLY file
(NeuSRenderer.extract_colored_geometry, vdn_train.validate.validate_mesh).

Points: uniform in the shell 0.3 <= |x| <= 1.0, where the geometric initialisation is sphere-like; every point has
|gradient| >= 0.5 in the fp64 oracle (asserted below), so -g/|g| is well conditioned and the tolerances measure the kernels."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import relelem

pytestmark = pytest.mark.gpu

P_MAX = 1000
SIZES = [1, 31, 128, 129, 1000]        # one lane, a partial wave, exactly one workgroup, one more point, several workgroups + a partial tail


POINT_SEED = 25     # chosen on the CPU for the condition below alone: point seeds 0 .. 24 each leave 3 - 7 of 1000 points under 0.5


def shell_points(n, seed=POINT_SEED):
    """n points uniform in direction and in radius over 0.3 <= |x| <= 1.0 (float32; float64 generator of vdn_train.synth)."""
    from vdn_train import synth
    d = synth.normal(seed, "shade_points/dir", (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 0.3 + 0.7 * synth.uniform(seed, "shade_points/radius", (n, 1))
    return (d * r).astype(np.float32)


_CACHE = {}


def _states():
    from vdn_train import synth
    if "st" not in _CACHE:
        _CACHE["st"] = synth.make_all_states(0, variance=0.4)
    return _CACHE["st"]


def _renderer(precision):
    from vdn_train import factory
    if precision not in _CACHE:
        _CACHE[precision] = factory.build_renderer(device=torch.device("cuda:0"), states=_states(), precision=precision)
    return _CACHE[precision]


def _oracle():
    """fp64 oracle on the P_MAX test points, computed once: sdf [P], gradient [P,3], colour [P,3] (the oracle's own -g/|g|)."""
    if "oracle" not in _CACHE:
        import oracle.neus_oracle as orc
        nets = orc.nets_from_numpy(_states(), dtype=torch.float64)
        x = torch.tensor(shell_points(P_MAX), dtype=torch.float64)
        out, g = orc.sdf_forward(nets.sdf, x, nets.sdf_conf, with_gradient=True)
        view = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        col = orc.rendering_forward(nets.color, x, g, view, out[:, 1:], nets.color_conf)
        _CACHE["oracle"] = tuple(t.numpy() for t in (out[:, 0], g, col))
    return _CACHE["oracle"]


def _points(dev, n=P_MAX):
    return torch.from_numpy(shell_points(P_MAX)[:n]).to(dev)


def _shade(rend, x, fused, **kw):
    from vdn_hip import mesh
    os.environ["VDN_SHADE_POINTS_FUSED"] = "1" if fused else "0"
    try:
        return mesh.shade_points(rend, x, **kw)
    finally:
        del os.environ["VDN_SHADE_POINTS_FUSED"]


def test_the_test_points_are_well_conditioned():
    """The condition on the inputs: |gradient| >= 0.5 at every test point in the fp64 oracle, and the points lie in the shell."""
    r = np.linalg.norm(shell_points(P_MAX).astype(np.float64), axis=1)
    assert r.min() >= 0.3 - 1e-6 and r.max() <= 1.0 + 1e-6
    _, g, _ = _oracle()
    assert np.linalg.norm(g, axis=1).min() >= 0.5


@pytest.mark.parametrize("P", SIZES)
def test_fused_point_shading_equals_the_separate_launches(P):
    """sdf and gradient: the bits of vdn_sdf_mlp_fwd_bf16 mode 1 (the same arithmetic). Colour: against color_network(x, g,
    -normalize(g), feat) on the bf16 kernels, < 2e-3 max abs - the bound tests/test_gpu_shade_fused.py holds MODE 2 to for the same
    difference (the normal's z component enters the first colour layer as an f32 term here, as a bf16 operand there); this arm adds
    the rounding of the normalisation (the in-kernel 1/sqrt against torch's). Measured on MI355X: 1.4e-5 (P = 1), 2.2e-5 (31), 2.6e-5 (128, 129),
    3.4e-5 (1000) - the size of one bf16 rounding of one input, as in MODE 2; 1 048 576 points: 7.0e-5."""
    from vdn_hip import layout, mesh
    dev = torch.device("cuda:0")
    rend = _renderer("bf16")
    assert mesh.fused_point_shading(rend)
    x = _points(dev, P)
    sdf, grad, col = _shade(rend, x, True)
    assert sdf.shape == (P,) and grad.shape == (P, 3) and col.shape == (P, 3)
    assert sdf.dtype == grad.dtype == col.dtype == torch.float32 and sdf.device == x.device
    sn, cn = rend.sdf_network, rend.color_network
    with torch.no_grad():
        sdf1, feat1, nrm1 = sn._run(1, pts=x)                                   # vdn_sdf_mlp_fwd_bf16 mode 1 on the same points
        ref = cn(x, nrm1, -torch.nn.functional.normalize(nrm1, dim=-1), layout.from_pt32(feat1, P, 256))
    assert torch.equal(sdf, sdf1) and torch.equal(grad, nrm1)
    err = float((col - ref).abs().max())
    print("P = %d: fused colour vs separate launches, max abs %.3e" % (P, err))
    assert err < 2e-3
    # the A/B switch (VDN_SHADE_POINTS_FUSED=0, set by _shade) runs exactly those launches
    sdf0, grad0, col0 = _shade(rend, x, False)
    assert torch.equal(sdf0, sdf1) and torch.equal(grad0, nrm1) and torch.equal(col0, ref)
    # a second call gives the same bits; small batches give the same bits as one launch
    again = _shade(rend, x, True)
    split = _shade(rend, x, True, batch=100)
    for a, b, c in zip((sdf, grad, col), again, split):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.isfinite(a).all()


def test_fp32_arm_against_the_fp64_oracle():
    """The exact-fp32 arm (the module calls, view direction formed in torch) at the project's fp32 bound: 1e-4 of each element."""
    dev = torch.device("cuda:0")
    rend = _renderer("fp32")
    sdf, grad, col = _shade(rend, _points(dev), True)         # (fp32 networks take the module calls whatever the switch says)
    o_sdf, o_grad, o_col = _oracle()
    for name, a, b in (("sdf", sdf, o_sdf), ("gradient", grad, o_grad), ("colour", col, o_col)):
        e = relelem(a.cpu().numpy(), b, rtol=1e-4)
        print("fp32 arm vs fp64 oracle, %s: %.3f of the bound" % (name, e))
        assert e <= 1.0, (name, e)


def test_bf16_fused_against_the_fp32_arm():
    """The throughput path against the parity path on the same 1000 points: finite, and the colour within 2e-2 max abs - the bound
    tests/test_gpu_bf16.py::test_bf16_stages_vs_oracle holds the bf16 colour head's per-point output to. Measured on MI355X:
    colour mean abs 1.1e-5, max abs 5.2e-5 (the synthetic colour head is nearly flat: 0.49 .. 0.51 over the shell); sdf max abs
    2.7e-3, gradient max abs 1.3e-2."""
    dev = torch.device("cuda:0")
    x = _points(dev)
    b_sdf, b_grad, b_col = _shade(_renderer("bf16"), x, True)
    f_sdf, f_grad, f_col = _shade(_renderer("fp32"), x, True)
    for t in (b_sdf, b_grad, b_col, f_sdf, f_grad, f_col):
        assert torch.isfinite(t).all()
    d = (b_col - f_col).abs()
    print("bf16 fused vs fp32 arm, colour: mean abs %.3e, max abs %.3e; sdf max abs %.3e; gradient max abs %.3e"
          % (float(d.mean()), float(d.max()), float((b_sdf - f_sdf).abs().max()), float((b_grad - f_grad).abs().max())))
    assert float(d.max()) < 2e-2


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_zero_gradient_gives_a_zero_view_direction_not_nan(precision):
    """No point of a real network has a zero gradient, so the guard max(|g|, 1e-12) is tested on a copy of the renderer whose SDF
    network computes nothing: every weight_g and bias zeroed (the effective weights v * g / |v| are then exact zeros; zeroing v
    as well would make the weight norm itself 0 / 0)."""
    dev = torch.device("cuda:0")
    rend = copy.copy(_renderer(precision))                   # the shared renderer keeps its own SDF network
    rend.sdf_network = copy.deepcopy(rend.sdf_network)
    with torch.no_grad():
        for name, q in rend.sdf_network.named_parameters():
            if name.endswith("weight_g") or name.endswith("bias"):
                q.zero_()
    sdf, grad, col = _shade(rend, _points(dev, 129), True)
    assert torch.equal(grad, torch.zeros_like(grad)) and torch.equal(sdf, torch.zeros_like(sdf))
    assert torch.isfinite(col).all()
    assert float(col.min()) >= 0.0 and float(col.max()) <= 1.0


def test_uncovered_colour_networks_take_the_module_calls():
    """d_feature = 352 (the depth_before_color head, fed cat([feature, VDN output])) and a non-'idr' head have no "c2" stream: on
    bf16 too they run sdf_network(x), .gradient(x), (depth_network,) color_network(x, g, -normalize(g), feat), and give exactly that."""
    from vdn_hip import mesh
    from vdn_train import synth, factory
    dev = torch.device("cuda:0")
    x = _points(dev, 129)
    r352 = factory.build_renderer(wdepth=True, device=dev, states=synth.make_all_states(0, wdepth=True, depth_before_color=True),
                                  precision="bf16", depth_before_color=True)
    rnn = factory.build_renderer(device=dev, states=_states(), precision="bf16", color_mode="no_normal")
    for rend in (r352, rnn):
        assert not mesh.fused_point_shading(rend)
        sdf, grad, col = mesh.shade_points(rend, x)
        with torch.no_grad():
            out = rend.sdf_network(x)
            g = rend.sdf_network.gradient(x)[:, 0]
            view = -torch.nn.functional.normalize(g, dim=-1)
            feat = out[:, 1:]
            if rend is r352:
                feat = torch.cat([feat, rend.depth_network(x, g, view, feat)], dim=-1)
            ref = rend.color_network(x, g, view, feat)
        assert torch.equal(sdf, out[:, 0]) and torch.equal(grad, g) and torch.equal(col, ref)
        assert col.shape == (129, 3) and torch.isfinite(col).all()


def test_entry_point_declines_what_it_does_not_cover():
    """Training saves, a work list, the tail split: -10 with nothing launched - the preset output buffers stay as they were."""
    from vdn_hip import lib
    dev = torch.device("cuda:0")
    rend = _renderer("bf16")
    P = 129
    x = _points(dev, P)
    c2 = rend.color_network._images().blobs["c2"]
    st = torch.cuda.current_stream().cuda_stream
    plane = torch.zeros(8, 160, 256, dtype=torch.bfloat16, device=dev)
    idx = torch.arange(P, dtype=torch.int32, device=dev)
    n_act = torch.tensor([P], dtype=torch.int32, device=dev)

    def block():
        sdf, nrm, col = (torch.full(s, 7.0, device=dev) for s in ((P,), (P, 3), (P, 3)))
        a = lib.VdnSdfArgs()
        a.blob = rend.sdf_network._images().blobs["full"].data_ptr()
        a.pts, a.n_per_ray, a.sdf_ld, a.P, a.scale = x.data_ptr(), 1, 1, P, float(rend.sdf_network.scale)
        a.sdf, a.normals = sdf.data_ptr(), nrm.data_ptr()
        return a, (sdf, nrm, col)

    def with_saves(a):
        a.H, a.V = plane.data_ptr(), plane.data_ptr()

    def with_u_pe(a):
        a.U_pe = plane.data_ptr()

    def with_feat(a):
        a.feat = plane.data_ptr()

    def with_list(a):
        a.active_idx, a.n_active = idx.data_ptr(), n_act.data_ptr()

    def with_tail(a):
        a.tail_row0, a.tail_max_rows = 128, 128

    for change in (with_saves, with_u_pe, with_feat, with_list, with_tail):
        a, outs = block()
        change(a)
        assert not lib.try_call("vdn_shade_points_bf16", a, lib.ptr(c2), 1, lib.ptr(outs[2]), st), change.__name__
        torch.cuda.synchronize()
        for t in outs:
            assert torch.equal(t, torch.full_like(t, 7.0)), change.__name__
    # the same block without any of them is taken
    a, outs = block()
    assert lib.try_call("vdn_shade_points_bf16", a, lib.ptr(c2), 1, lib.ptr(outs[2]), st)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() and not torch.equal(t, torch.full_like(t, 7.0)) for t in outs)
    # ray form (no points) is an argument error, not a shape to decline
    a, outs = block()
    a.pts = None
    with pytest.raises(lib.VdnError):
        lib.call("vdn_shade_points_bf16", a, lib.ptr(c2), 1, lib.ptr(outs[2]), st)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_coloured_mesh_end_to_end(tmp_path, precision):
    """Lattice -> marching cubes -> vertex shading -> PLY, resolution 24 on the unit box: geometry untouched, unit outward normals
    on the sphere-like initial surface, colours = the quantised shade_points colour, and the file holds what was computed."""
    from vdn_hip import mesh
    from vdn_train import meshio, validate
    dev = torch.device("cuda:0")
    rend = _renderer(precision)
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    v0, t0 = rend.extract_geometry(lo, hi, resolution=24, threshold=0.0)
    v, t, nrm, colors = rend.extract_colored_geometry(lo, hi, resolution=24, threshold=0.0)
    V = v.shape[0]
    assert V > 0 and t.shape[0] > 0
    assert v.dtype == v0.dtype and np.array_equal(v, v0) and t.dtype == t0.dtype and np.array_equal(t, t0)
    assert nrm.shape == (V, 3) and nrm.dtype == np.float32 and colors.shape == (V, 3) and colors.dtype == np.uint8
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    assert ((nrm * (v / np.linalg.norm(v, axis=1, keepdims=True))).sum(axis=1) > 0).all()
    _, g, c = mesh.shade_points(rend, torch.from_numpy(v.astype(np.float32)).to(dev))
    assert np.array_equal(colors, mesh.quantize_colors_bgr(c.cpu().numpy()))
    assert np.array_equal(colors[:, ::-1], np.rint(np.clip(c.cpu().numpy(), 0, 1) * 255).astype(np.uint8))      # RGB = BGR reversed
    assert np.array_equal(nrm, (g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)).cpu().numpy())
    # the file, in world space: a uniform scale and a translation
    s, tr = 2.5, np.array([0.5, -1.0, 3.0])
    scale_mat = np.diag([s, s, s, 1.0])
    scale_mat[:3, 3] = tr
    path, nv, nf = validate.validate_mesh(rend, lo, hi, str(tmp_path / "meshes" / "00000000.ply"), resolution=24, world_space=True,
                                          scale_mat=scale_mat)
    assert (nv, nf) == (V, t.shape[0]) and os.path.exists(path)
    got = meshio.read_ply(path)
    assert np.array_equal(got["vertices"], (v * s + tr[None]).astype(np.float32))
    assert np.array_equal(got["triangles"], t) and np.array_equal(got["normals"], nrm) and np.array_equal(got["colors"], colors)
    # both attribute flags off: the reference's bare mesh
    path2, nv2, nf2 = validate.validate_mesh(rend, lo, hi, str(tmp_path / "bare.ply"), resolution=24, vertex_colors=False,
                                             vertex_normals=False)
    bare = meshio.read_ply(path2)
    assert bare["normals"] is None and bare["colors"] is None and (nv2, nf2) == (V, t.shape[0])
    assert np.array_equal(bare["vertices"], v.astype(np.float32)) and np.array_equal(bare["triangles"], t)
    assert os.path.getsize(path2) == len(meshio.ply_header(V, t.shape[0])) + V * 12 + t.shape[0] * 13
