"""The colour head INSIDE the fused SDF launches (csrc/k_sdf_fwd2.h MODE 3 / 2 / 4), through the C ABI (include/vdn_render.h), held
to the float64 one-layer models of oracle/mlp_ops.py (fused_head_plane_models) on the cases of oracle/mlp_cases.py (FUSED_CASES,
SHADE_CASES, POINT_CASES); what models, cases and comparator are worth is proven without a GPU by tests/test_mlp_ops_model_cpu.py
(each planted defect - a wrong tail column, swapped small columns, the neighbouring ray's direction, a scaled point, an unrounded
feature operand, nz in bf16, permuted output rows, an unwritten col_small column - is rejected there). This head is not the code
of vdn_rendernet_fwd_bf16, which tests/test_gpu_mlp_planes.py holds: its own "c2" weight stream (9 k-tiles, the 33rd input as an
f32 rank-1 term with a weight column read from the chunks' tails), the feature vector from registers, point and direction formed
per row in the launch, its own plane stores. test_gpu_mlp_planes.py::test_blob_holds_the_operand_weights decodes the "c2" blob,
tail included, for both weight states used here.

MODE 3, vdn_sdf_color_train_bf16 (every case: 1, 33, 129 and 300 rows in ray form with ray boundaries inside a wave, scale 1.5, a
work list that is not ascending, the "hot" SDF state): the SDF side - sdf, normals, feat, PE, every H[l] and V[l] - is bit for bit
vdn_sdf_mlp_fwd_bf16 mode 1 with the same arguments (which test_gpu_mlp_planes.py holds to float64); col_small, col_h[0..3] and
col_out are judged by mlp_ops.judge against the models evaluated on the planes the launch itself saved. Bound per (case, plane):
max(1, 3 x float32 floor) units + the plane's documented extra term (the table in oracle/mlp_ops.py), then a bf16 rounding
(col_out, f32: none); the floor is the float32 model against the float64 model, measured at run time. Outputs are pre-filled with
NaN between guard bands; compact rows follow the list, col_out of unlisted points stays NaN; a launch on the OTHER state's c2 blob
is rejected; U_pe and tail_max_rows are declined (-10), `pts` is an argument error (-2), nothing written.

MODE 2, vdn_shade_fused_bf16 (1 and 3 rays of 128 samples, T = 128 and T = 160 with background inputs, with and without the
feature plane = both instantiations): sdf and normals are MODE 3's bits on the same rays; every compositor output is bit for bit
vdn_alpha_composite_fwd + vdn_eikonal_reduce fed MODE 3's sdf / normals / col_out (both go through composite_row; the head's
epilogue is explicit fmaf behind the same MFMA sequence in every instantiation); the feature plane is MODE 3's bits; a second call
gives the same bits (the ticket is left at zero).

MODE 4, vdn_shade_points_bf16 (P = 1, 33, 129, 300; once on the state whose sdf is constant): sdf and normals bit for bit mode 1;
no plane is saved, so col_out is judged end to end against simulate_fused_head_forward in float64 on the mode-1 launch's feature
plane, MODE 4's own f32 normals and view = -g / max(|g|, 1e-12) formed in float64: conftest.relelem at its defaults, bound
max(1, 3 x floor), the floor being the float32 chain against the float64 chain on the same inputs (an intermediate plane can round
to the neighbouring bf16 value in either chain); three times for the reason tests/test_gpu_ray_ops.py gives. On the constant-sdf
state the normals are exactly 0, the colour is finite and within the same bound of the model at view = 0.

Every (case, plane) is printed with bound, floor and kernel error (pytest -rA). "kernel error" is what the kernel needs, in units,
beyond a bf16 rounding of the reference and beyond the extra term; "of its allowance" the largest share of an element's whole
allowance it needs. Measured on the MI355X (worst over the cases; no bf16 plane has an element off the two bf16 values next to its
model, and the MODE 2 comparisons are bit for bit in both instantiations):

train fwd  small       6 cases  bound <=  2.86  floor <= 0.952  kernel error <= 0.000 units, <= 0.00 of its allowance
train fwd  h0          6 cases  bound <=  1.00  floor <= 0.287  kernel error <= 0.000 units, <= 0.00 of its allowance
train fwd  h1          6 cases  bound <=  3.64  floor <= 1.214  kernel error <= 0.000 units, <= 0.00 of its allowance
train fwd  h2          6 cases  bound <=  3.03  floor <= 1.011  kernel error <= 0.000 units, <= 0.00 of its allowance
train fwd  h3          6 cases  bound <=  2.85  floor <= 0.948  kernel error <= 0.000 units, <= 0.00 of its allowance
train fwd  out         6 cases  bound <=  1.00  floor <= 0.170  kernel error <= 0.170 units, <= 0.36 of its allowance
points     col_out     5 cases  bound <=  1.00  floor <= 0.288  kernel error <= 0.132 units (conftest.relelem)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import relelem
from oracle import mlp_cases, mlp_ops
from test_gpu_mlp_planes import PlaneBufs, _hold
from test_gpu_ray_ops import Bufs, _call, _status, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD_PLANES = ("small", "h0", "h1", "h2", "h3", "out")


def _p(ptr):
    return ctypes.c_void_p(ptr)


@functools.lru_cache(maxsize=None)
def _images(state):
    """The refreshed images of one weight state: the SDF network's, the colour network's, and layers 0..4 of its "c2" stream as
    operands (from the effective weights the device materialised)."""
    from vdn_train import factory
    r = factory.build_renderer(wdepth=True, device=torch.device(DEV), states=mlp_cases.fused_states(state), precision="bf16")
    sdf, col = r.sdf_network._images(), r.color_network._images()
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(col)
    return {"renderer": r, "sdf": sdf, "color": col, "c2": [mlp_ops.operand_weights(host, "c2", l) for l in range(5)]}


def _sdf_block(c, b, saves, feat=True):
    """VdnSdfArgs of a case (ray form, or explicit points where the case has them) with NaN-filled outputs in `b`."""
    from vdn_hip import lib
    img = _images(c["state"])["sdf"]
    P = c["P"]
    a = lib.VdnSdfArgs()
    a.blob = img.blobs["full"].data_ptr()
    if "pts" in c:
        a.pts, a.n_per_ray, a.sdf_ld = b.inp(c["pts"]), 1, 1
    else:
        a.rays_o, a.rays_d, a.z = b.inp(c["rays_o"]), b.inp(c["rays_d"]), b.inp(c["z"])
        a.n_per_ray = a.z_ld = a.sdf_ld = c["n_per_ray"]
    a.P, a.scale = P, c["scale"]
    a.sdf, a.normals = b.out("sdf", P), b.out("normals", P, 3)
    if feat:
        a.feat = b.plane("feat", 1, P, 256)
    if saves:
        a.H, a.V, a.PE = b.plane("H", 8, P, 256), b.plane("V", 8, P, 256), b.plane("PE", 1, P, 64)
    if c["active_idx"] is not None:
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([c["n_active"]]), torch.int32)
    return a


def _sdf_planes(c, b):
    """What the SDF side left: compact rows of the planes (layer 3: its 217 outputs), sdf / normals of the listed points in list
    order; the outputs of unlisted points are still NaN."""
    P = c["P"]
    rows = mlp_cases.fused_rows_of(c) if "pts" not in c else np.arange(P)
    n = len(rows)
    planes = {"feat": b.rows("feat", 0, P, 256, n)}
    if "H" in b.outs:
        planes["PE"] = b.rows("PE", 0, P, 64, n)[:, :39]
        for l in range(8):
            w = 217 if l == 3 else 256
            planes["H%d" % l], planes["V%d" % l] = b.rows("H", l, P, 256, n)[:, :w], b.rows("V", l, P, 256, n)[:, :w]
    listed = np.zeros(P, bool)
    listed[rows] = True
    for k in ("sdf", "normals"):
        assert np.isnan(b.np(k)[~listed]).all(), "%s of an unlisted point was written" % k
        planes[k] = b.np(k)[rows]
    return planes


def _train_forward(c, c2_state=None):
    """vdn_sdf_color_train_bf16 with every save -> (PlaneBufs, SDF-side planes, head planes {small, h0..h3, out} in compact rows)."""
    c2 = _images(c2_state or c["state"])["color"].blobs["c2"]
    P = c["P"]
    b = PlaneBufs()
    a = _sdf_block(c, b, saves=True)
    col_h, col_small, col_out = b.plane("col_h", 4, P, 256), b.plane("col_small", 1, P, 64), b.out("col_out", P, 3)
    _call("vdn_sdf_color_train_bf16", a, _p(c2.data_ptr()), int(c["squeeze"]), _p(col_h), _p(col_small), _p(col_out), _stream())
    b.check_guards()
    rows = mlp_cases.fused_rows_of(c)
    n = len(rows)
    head = {"small": b.rows("col_small", 0, P, 64, n)[:, :33]}
    for l in range(4):
        head["h%d" % l] = b.rows("col_h", l, P, 256, n)
    listed = np.zeros(P, bool)
    listed[rows] = True
    assert np.isnan(b.np("col_out")[~listed]).all(), "col_out of an unlisted point was written"
    head["out"] = b.np("col_out")[rows]
    return b, _sdf_planes(c, b), head


def _head_models(c, sdf_side, head):
    return mlp_ops.fused_head_plane_models(_images(c["state"])["c2"], c["rays_o"], c["rays_d"], c["z"], mlp_cases.fused_rows_of(c),
                                           sdf_side["normals"], sdf_side["feat"], head, c["squeeze"], c["scale"])


# ---- MODE 3: the training forward -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mlp_cases.FUSED_CASES))
def test_training_forward_head_planes_vs_float64_layer_models(name):
    """vdn_sdf_color_train_bf16: the SDF side bit for bit vdn_sdf_mlp_fwd_bf16 mode 1 with the same arguments; col_small from the
    rays and the launch's own f32 normals, col_h[0] from the feature plane, the saved col_small and the f32 normal's z with the tail
    column, col_h[1..3] and col_out from the plane before - in the compact rows of the list, col_out at the dense point ids."""
    c = mlp_cases.fused_case(name)
    _, sdf_side, head = _train_forward(c)
    b1 = PlaneBufs()
    _call("vdn_sdf_mlp_fwd_bf16", 1, _sdf_block(c, b1, saves=True), _stream())
    b1.check_guards()
    ref = _sdf_planes(c, b1)
    assert set(ref) == set(sdf_side)
    for k in ref:
        assert np.isfinite(ref[k]).all() and np.array_equal(ref[k], sdf_side[k]), "%s: %s differs from vdn_sdf_mlp_fwd_bf16 mode 1" % (name, k)
    models = _head_models(c, sdf_side, head)
    assert set(models) == set(head) == set(HEAD_PLANES)
    for k in head:
        got = head[k][:, :models[k]["y64"].shape[1]]
        assert got.shape == models[k]["y64"].shape and np.isfinite(got).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, head), rows)
    print("\n".join(rows))
    for l in (0, 2):                                        # the silenced unit: a pre-activation that is exactly zero
        assert (head["h%d" % l][:, mlp_cases.SILENT_UNIT] == 0).all()


def test_the_training_forward_on_the_other_colour_weights_is_rejected():
    """The wiring from the launch to the comparator: the same launch on the OTHER state's c2 blob (seed 4, the same units silenced),
    judged against this state's models, is rejected at every plane behind a weight matrix (col_small has none)."""
    c = mlp_cases.fused_case("rays-3x11-s1")
    _, sdf_side, head = _train_forward(c, c2_state="heads-other")
    res = mlp_ops.judge_planes(_head_models(c, sdf_side, head), head)
    assert res["small"]["ok"]
    for k, j in res.items():
        if k != "small":
            assert not j["ok"] and j["err"] > 1e3, (k, j)


def test_the_training_forward_declines_what_it_does_not_cover():
    """U_pe and the tail split: -10; explicit points: -2 (an argument error); nothing is launched and nothing written."""
    c = mlp_cases.fused_case("rays-3x11-s1")
    c2 = _images(c["state"])["color"].blobs["c2"]
    P = c["P"]

    def with_u_pe(a, b):
        a.U_pe = b.out("U_pe", P, 39)

    def with_tail(a, b):
        a.tail_row0, a.tail_max_rows = 0, 128

    def with_pts(a, b):
        a.pts = b.inp(mlp_cases.fused_points_of(c))

    for change, want in ((with_u_pe, -10), (with_tail, -10), (with_pts, -2)):
        b = PlaneBufs()
        a = _sdf_block(c, b, saves=True)
        ptrs = [b.plane("col_h", 4, P, 256), b.plane("col_small", 1, P, 64), b.out("col_out", P, 3)]
        change(a, b)
        assert _status("vdn_sdf_color_train_bf16", a, _p(c2.data_ptr()), 1, *[_p(x) for x in ptrs], _stream()) == want, change.__name__
        torch.cuda.synchronize()
        for k, (base, _) in b.outs.items():
            assert torch.isnan(base).all(), "%s: %s was written" % (change.__name__, k)


# ---- MODE 2: the inference launch -------------------------------------------------------------------------------------------

COMPOSITE_OUTS = (("weights", "T"), ("alpha_out", "T"), ("cdf", "N"), ("inside_sphere", "N"), ("color_out", 3), ("weight_sum", 1),
                  ("weight_max", 1), ("s_val", 1), ("eik_partial", 2))


def _composite_block(c, b):
    from vdn_hip import lib
    a = lib.VdnCompositeArgs()
    a.rays_o, a.rays_d, a.dists, a.mid_z = b.inp(c["rays_o"]), b.inp(c["rays_d"]), b.inp(c["dists"]), b.inp(c["z"])
    a.variance = b.inp(np.asarray([c["variance"]], np.float32))
    a.bg_density, a.bg_rgb, a.bg_dists, a.background_rgb = (b.inp(c[k]) for k in ("bg_density", "bg_rgb", "bg_dists", "background_rgb"))
    a.cos_anneal_ratio = float(c["cos_anneal"])
    a.B, a.N, a.T = c["B"], c["N"], c["T"]
    for k, w in COMPOSITE_OUTS:
        setattr(a, k, b.out(k, c["B"], c[w] if isinstance(w, str) else w))
    a.eik_out = b.out("eik_out", 3)
    return a


def _shade_fused(c, save):
    b = PlaneBufs()
    sa = _sdf_block(c, b, saves=False, feat=save)
    cm = _composite_block(c, b)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    c2 = _images(c["state"])["color"].blobs["c2"]
    _call("vdn_shade_fused_bf16", sa, _p(c2.data_ptr()), int(c["squeeze"]), cm, _p(ticket.data_ptr()), _stream())
    b.check_guards()
    assert int(ticket.item()) == 0, "the arrival counter was not left at zero"
    return b


@pytest.mark.parametrize("save", [False, True], ids=["no-feature-plane", "feature-plane"])
@pytest.mark.parametrize("name", list(mlp_cases.SHADE_CASES))
def test_shade_fused_is_the_training_forward_plus_the_compositor_bit_for_bit(name, save):
    """vdn_shade_fused_bf16 against vdn_sdf_color_train_bf16 on the same rays, then vdn_alpha_composite_fwd + vdn_eikonal_reduce on
    what that launch left: sdf, normals, the feature plane (when given) and every compositor output, bit for bit, twice in a row."""
    c = mlp_cases.shade_case(name)
    b3, _, _ = _train_forward(c)
    cb = Bufs()
    ca = _composite_block(c, cb)
    ca.sdf, ca.normals, ca.color = (b3[k].data_ptr() for k in ("sdf", "normals", "col_out"))
    _call("vdn_alpha_composite_fwd", ca, _stream())
    cb.check()
    red = Bufs()
    _call("vdn_eikonal_reduce", _p(cb["eik_partial"].data_ptr()), c["B"], _p(red.out("eik_out", 3)), _stream())
    red.check()
    assert torch.equal(red["eik_out"], cb["eik_out"])
    first = _shade_fused(c, save)
    again = _shade_fused(c, save)
    for k in [k for k, _ in COMPOSITE_OUTS] + ["eik_out"]:
        assert torch.isfinite(first[k]).all(), "%s has unwritten or non-finite elements" % k
        assert torch.equal(first[k], cb[k]), "%s differs from the compositor on the training forward's outputs" % k
        assert torch.equal(first[k], again[k]), "%s: the second call differs" % k
    for k in ("sdf", "normals") + (("feat",) if save else ()):
        assert torch.isfinite(first[k].float()).all() and torch.equal(first[k], b3[k]), "%s differs from the training forward's" % k
        assert torch.equal(first[k], again[k]), "%s: the second call differs" % k
    assert ("feat" in first.outs) == save


# ---- MODE 4: free-standing points -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mlp_cases.POINT_CASES))
def test_shade_points_colour_vs_float64_chain(name):
    """vdn_shade_points_bf16: sdf and normals bit for bit vdn_sdf_mlp_fwd_bf16 mode 1 on the same points; col_out end to end against
    the float64 chain on that launch's feature plane, the f32 normals and the view direction formed from them in float64."""
    c = mlp_cases.point_case(name)
    P = c["P"]
    b1 = PlaneBufs()
    _call("vdn_sdf_mlp_fwd_bf16", 1, _sdf_block(c, b1, saves=False), _stream())
    b1.check_guards()
    b4 = PlaneBufs()
    a = _sdf_block(c, b4, saves=False, feat=False)
    c2 = _images(c["state"])["color"].blobs["c2"]
    _call("vdn_shade_points_bf16", a, _p(c2.data_ptr()), int(c["squeeze"]), _p(b4.out("col_out", P, 3)), _stream())
    b4.check_guards()
    for k in ("sdf", "normals"):
        assert torch.isfinite(b4[k]).all() and torch.equal(b4[k], b1[k]), "%s differs from vdn_sdf_mlp_fwd_bf16 mode 1" % k
    feat, normals, got = b1.rows("feat", 0, P, 256, P), b4.np("normals").astype(np.float32), b4.np("col_out")
    assert np.isfinite(feat).all() and np.isfinite(got).all(), "unwritten or non-finite elements"
    view = mlp_ops.view_down_the_normal(normals)
    if c["state"] == "heads-flat":                           # a zero gradient gives a zero direction, never NaN
        assert (normals == 0).all() and (view == 0).all()
    else:
        assert np.abs(np.linalg.norm(view, axis=1) - 1).max() < 1e-12
    ops = _images(c["state"])["c2"]
    ref64, ref32 = (mlp_ops.simulate_fused_head_forward(ops, c["pts"], view, normals, feat, c["squeeze"], dtype=dt)["out"]
                    for dt in (torch.float64, torch.float32))
    floor, err = relelem(ref32, ref64), relelem(got, ref64)
    bound = max(1.0, 3.0 * floor)
    print("%-14s col_out bound %.2f units (fp32 floor %.3f)  kernel error %.3f units" % (name, bound, floor, err))
    assert err <= bound, "%s col_out: kernel error %.3f units > bound %.2f (fp32 floor %.3f)" % (name, err, bound, floor)
