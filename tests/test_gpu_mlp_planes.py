"""The planes of the bf16 forward launches, through the C ABI (include/vdn_render.h), each held to the float64 one-layer model of
oracle/mlp_ops.py evaluated on the plane BEFORE it as the launch itself saved it ("teacher forcing") and on the bf16 weights the
blob holds - which test_blob_holds_the_operand_weights decodes and holds to oracle/mlp_ops.py operand_weights exactly, for every
stream of every network. Cases: oracle/mlp_cases.py; what the models, the cases and the comparator are worth is proven without a
GPU by tests/test_mlp_ops_model_cpu.py.

vdn_sdf_mlp_fwd_bf16 mode 1 with training saves and U_pe: PE, H[0..7], feat, sdf, V[7..0], U_pe, normals; vdn_sdf_fwd_tail_bf16 with
tail_row0 = 0 gives the same planes bit for bit. vdn_rendernet_fwd_bf16 (colour head, VDN head, the d_feature = 352 colour head):
save_small, save_extra, save_h[0..3], out, save_mask = (save_h > 0) exactly. vdn_nerf_mlp_fwd_bf16 (with and without the dpt head;
once with a work list): save_pe, save_vpe, save_h[0..7], save_feature, save_hv, density, rgb, feat, both masks exactly. One launch
per network on the OTHER weight state, judged against this state's models, must be rejected (the wiring checks). Every output is pre-filled with NaN (masks: a byte pattern) between
guard bands; afterwards every promised element is finite and judged - no element excluded, no case skipped -, the guard bands and
(with a work list) the outputs of every unlisted point are untouched. Pad rows of the PT32 planes may hold duplicates of a row
("out-of-range lanes work on a clamped row and store duplicates of it") and columns 217..255 of H[3] and V[3] are
not outputs of layer 3: neither is read.

Bound per (case, plane): max(1, 3 x float32 floor) units + the plane's documented extra term (the table in oracle/mlp_ops.py),
then a bf16 rounding in either direction; f32 outputs without the rounding. "kernel error" is what the kernel needs of that, in
units, beyond a bf16 rounding of the reference and beyond the extra term; "of its allowance" the largest share of an element's whole
allowance (units and extra terms) it needs. Every (case, plane) is printed with bound, floor and kernel error (pytest -rA).

Measured on the MI355X (worst over the cases of a launch; "sdf (hot)" = the weight state that reaches t >= 25 and t >= 128 in every
layer; "sdf bwd" = rbar + fbar over all cases and upstream gradients, "d_pts+acc" = fbar's acc_pts = 1 over a finite pre-fill; "head acc" = the acc_* = 1 forms). The hidden planes need one unit where t is just below -24 (1 + 2^t rounds to 1: the float32 evaluation of the documented
formula itself); the V planes need almost the whole code step their contract grants (the 8-bit softplus' is a truncated code):

sdf        PE          6 cases  bound <=  2.09  floor <= 0.695  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf        H0          6 cases  bound <=  3.00  floor <= 1.000  kernel error <= 1.000 units, <= 0.33 of its allowance
sdf        H1          6 cases  bound <=  6.01  floor <= 2.005  kernel error <= 1.000 units, <= 0.33 of its allowance
sdf        H2          6 cases  bound <=  6.08  floor <= 2.027  kernel error <= 0.998 units, <= 0.33 of its allowance
sdf        H3          6 cases  bound <=  4.96  floor <= 1.654  kernel error <= 1.000 units, <= 0.33 of its allowance
sdf        H4          6 cases  bound <=  3.00  floor <= 0.999  kernel error <= 0.999 units, <= 0.33 of its allowance
sdf        H5          6 cases  bound <=  4.55  floor <= 1.516  kernel error <= 1.000 units, <= 0.32 of its allowance
sdf        H6          6 cases  bound <=  6.32  floor <= 2.107  kernel error <= 1.000 units, <= 0.33 of its allowance
sdf        H7          6 cases  bound <=  5.26  floor <= 1.753  kernel error <= 1.000 units, <= 0.30 of its allowance
sdf        feat        6 cases  bound <= 14.47  floor <= 4.823  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf        sdf         6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.24 of its allowance
sdf        V7          6 cases  bound <=  1.35  floor <= 0.451  kernel error <= 0.000 units, <= 0.99 of its allowance
sdf        V6          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf        V5          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf        V4          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf        V3          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf        V2          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf        V1          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf        V0          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf        U_pe        6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.23 of its allowance
sdf        normals     6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.40 of its allowance
sdf (hot)  PE          2 cases  bound <=  2.08  floor <= 0.693  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf (hot)  H0          2 cases  bound <=  3.00  floor <= 0.999  kernel error <= 0.999 units, <= 0.33 of its allowance
sdf (hot)  H1          2 cases  bound <=  4.19  floor <= 1.397  kernel error <= 0.999 units, <= 0.25 of its allowance
sdf (hot)  H2          2 cases  bound <=  4.01  floor <= 1.337  kernel error <= 0.999 units, <= 0.29 of its allowance
sdf (hot)  H3          2 cases  bound <=  4.45  floor <= 1.483  kernel error <= 1.000 units, <= 0.27 of its allowance
sdf (hot)  H4          2 cases  bound <=  3.00  floor <= 1.000  kernel error <= 0.998 units, <= 0.33 of its allowance
sdf (hot)  H5          2 cases  bound <=  3.43  floor <= 1.143  kernel error <= 0.999 units, <= 0.33 of its allowance
sdf (hot)  H6          2 cases  bound <=  4.40  floor <= 1.466  kernel error <= 0.999 units, <= 0.25 of its allowance
sdf (hot)  H7          2 cases  bound <=  3.64  floor <= 1.213  kernel error <= 0.998 units, <= 0.32 of its allowance
sdf (hot)  feat        2 cases  bound <= 14.00  floor <= 4.667  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf (hot)  sdf         2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.22 of its allowance
sdf (hot)  V7          2 cases  bound <=  1.35  floor <= 0.451  kernel error <= 0.000 units, <= 0.99 of its allowance
sdf (hot)  V6          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.96 of its allowance
sdf (hot)  V5          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.96 of its allowance
sdf (hot)  V4          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (hot)  V3          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf (hot)  V2          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (hot)  V1          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (hot)  V0          2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (hot)  U_pe        2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.30 of its allowance
sdf (hot)  normals     2 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.27 of its allowance
sdf bwd    ub0        12 cases  bound <=  1.00  floor <= 0.250  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf bwd    ub1        12 cases  bound <=  5.58  floor <= 1.859  kernel error <= 0.047 units, <= 0.01 of its allowance
sdf bwd    EX0        12 cases  bound <=  3.78  floor <= 1.260  kernel error <= 0.500 units, <= 0.33 of its allowance
sdf bwd    ub2        12 cases  bound <=  5.87  floor <= 1.956  kernel error <= 0.042 units, <= 0.01 of its allowance
sdf bwd    EX1        12 cases  bound <=  4.48  floor <= 1.492  kernel error <= 0.500 units, <= 0.33 of its allowance
sdf bwd    ub3        12 cases  bound <=  5.00  floor <= 1.668  kernel error <= 0.025 units, <= 0.01 of its allowance
sdf bwd    EX2        12 cases  bound <=  5.05  floor <= 1.684  kernel error <= 0.500 units, <= 0.31 of its allowance
sdf bwd    ub4        12 cases  bound <=  4.14  floor <= 1.381  kernel error <= 0.012 units, <= 0.00 of its allowance
sdf bwd    EX3        12 cases  bound <=  4.81  floor <= 1.603  kernel error <= 0.500 units, <= 0.30 of its allowance
sdf bwd    ub5        12 cases  bound <=  5.33  floor <= 1.778  kernel error <= 0.022 units, <= 0.00 of its allowance
sdf bwd    EX4        12 cases  bound <=  3.51  floor <= 1.169  kernel error <= 0.500 units, <= 0.27 of its allowance
sdf bwd    ub6        12 cases  bound <=  5.41  floor <= 1.804  kernel error <= 0.025 units, <= 0.01 of its allowance
sdf bwd    EX5        12 cases  bound <=  3.73  floor <= 1.242  kernel error <= 0.500 units, <= 0.30 of its allowance
sdf bwd    ub7        12 cases  bound <=  6.50  floor <= 2.167  kernel error <= 0.051 units, <= 0.01 of its allowance
sdf bwd    EX6        12 cases  bound <=  5.40  floor <= 1.799  kernel error <= 0.500 units, <= 0.31 of its allowance
sdf bwd    ub8        12 cases  bound <=  5.91  floor <= 1.971  kernel error <= 0.105 units, <= 0.02 of its allowance
sdf bwd    EX7        12 cases  bound <=  4.96  floor <= 1.652  kernel error <= 0.500 units, <= 0.28 of its allowance
sdf bwd    ub4pe      12 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf bwd    ab8        12 cases  bound <=  2.00  floor <= 0.666  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf bwd    ab7        12 cases  bound <=  1.82  floor <= 0.606  kernel error <= 0.011 units, <= 0.01 of its allowance
sdf bwd    ab6        12 cases  bound <=  5.00  floor <= 1.665  kernel error <= 0.131 units, <= 0.03 of its allowance
sdf bwd    ab5        12 cases  bound <=  3.96  floor <= 1.319  kernel error <= 0.011 units, <= 0.00 of its allowance
sdf bwd    ab4        12 cases  bound <=  6.95  floor <= 2.316  kernel error <= 0.111 units, <= 0.03 of its allowance
sdf bwd    ab3        12 cases  bound <=  5.53  floor <= 1.844  kernel error <= 0.291 units, <= 0.10 of its allowance
sdf bwd    ab2        12 cases  bound <=  4.36  floor <= 1.453  kernel error <= 0.171 units, <= 0.04 of its allowance
sdf bwd    ab1        12 cases  bound <=  5.01  floor <= 1.668  kernel error <= 0.035 units, <= 0.01 of its allowance
sdf bwd    ab0        12 cases  bound <=  4.92  floor <= 1.642  kernel error <= 0.081 units, <= 0.02 of its allowance
sdf bwd    d_pts      12 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.16 of its allowance
sdf bwd    d_pts+acc  12 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.16 of its allowance
head       small       5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.00 of its allowance
head       h0          5 cases  bound <=  2.80  floor <= 0.932  kernel error <= 0.000 units, <= 0.00 of its allowance
head       h1          5 cases  bound <=  2.97  floor <= 0.991  kernel error <= 0.000 units, <= 0.00 of its allowance
head       h2          5 cases  bound <=  3.27  floor <= 1.091  kernel error <= 0.000 units, <= 0.00 of its allowance
head       h3          5 cases  bound <=  2.48  floor <= 0.826  kernel error <= 0.000 units, <= 0.00 of its allowance
head       out         5 cases  bound <=  1.00  floor <= 0.237  kernel error <= 0.239 units, <= 0.39 of its allowance
head       extra       1 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   delta_out   5 cases  bound <=  2.14  floor <= 0.714  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   delta_h3    5 cases  bound <=  3.75  floor <= 1.249  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   delta_h2    5 cases  bound <=  2.66  floor <= 0.887  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   delta_h1    5 cases  bound <=  3.75  floor <= 1.250  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   delta_h0    5 cases  bound <=  3.39  floor <= 1.129  kernel error <= 0.033 units, <= 0.02 of its allowance
head bwd   d_feat      5 cases  bound <=  3.10  floor <= 1.032  kernel error <= 0.000 units, <= 0.00 of its allowance
head bwd   d_normals   5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.07 of its allowance
head bwd   d_pts       5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.07 of its allowance
head bwd   d_dirs      5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.02 of its allowance
head bwd   d_extra     1 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.980 units, <= 0.98 of its allowance
head acc   d_feat      5 cases  bound <=  1.45  floor <= 0.483  kernel error <= 0.000 units, <= 0.00 of its allowance
head acc   d_normals   5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.933 units, <= 0.93 of its allowance
head acc   d_pts       5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.935 units, <= 0.94 of its allowance
head acc   d_dirs      5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.188 units, <= 0.47 of its allowance
nerf       pe          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.49 of its allowance
nerf       vpe         6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h0          6 cases  bound <=  3.63  floor <= 1.209  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h1          6 cases  bound <=  3.25  floor <= 1.082  kernel error <= 0.232 units, <= 0.08 of its allowance
nerf       h2          6 cases  bound <=  3.20  floor <= 1.067  kernel error <= 0.012 units, <= 0.00 of its allowance
nerf       h3          6 cases  bound <=  3.02  floor <= 1.005  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h4          6 cases  bound <=  2.56  floor <= 0.852  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h5          6 cases  bound <=  9.47  floor <= 3.158  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h6          6 cases  bound <=  3.76  floor <= 1.253  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       h7          6 cases  bound <=  3.18  floor <= 1.058  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf       hv          6 cases  bound <=  3.47  floor <= 1.158  kernel error <= 0.064 units, <= 0.02 of its allowance
nerf       feature     6 cases  bound <=  3.73  floor <= 1.244  kernel error <= 0.043 units, <= 0.02 of its allowance
nerf       density     6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.13 of its allowance
nerf       rgb         6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.11 of its allowance
nerf       feat        5 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.18 of its allowance
nerf bwd   d_pts4      6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.29 of its allowance
nerf bwd   d_dirs      6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.03 of its allowance
nerf bwd   delta_o     6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_v     6 cases  bound <=  5.12  floor <= 1.706  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_head  6 cases  bound <=  4.68  floor <= 1.561  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h7    6 cases  bound <=  3.61  floor <= 1.204  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h6    6 cases  bound <=  2.88  floor <= 0.959  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h5    6 cases  bound <=  3.31  floor <= 1.104  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h4    6 cases  bound <=  3.03  floor <= 1.012  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h3    6 cases  bound <=  4.10  floor <= 1.366  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h2    6 cases  bound <=  2.95  floor <= 0.984  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h1    6 cases  bound <=  3.10  floor <= 1.034  kernel error <= 0.000 units, <= 0.00 of its allowance
nerf bwd   delta_h0    6 cases  bound <=  4.17  floor <= 1.391  kernel error <= 0.000 units, <= 0.00 of its allowance

vdn_rendernet_bwd_bf16 (the three heads) on the forward's own planes: delta_out, delta_h[3..0], d_feat, d_normals, d_pts,
d_dirs, d_extra; `mask` against mask = NULL bit for bit; the acc_* = 1 forms.

vdn_nerf_mlp_bwd_bf16 on the forward's own planes: delta_o, delta_v, delta_head, delta_h[7..0]; with the masks and without.

vdn_nerf_mlp_bwd_input_bf16: the same delta planes bit for bit, d_pts4 and d_dirs. vdn_sdf_bwd_rbar_bf16 then vdn_sdf_bwd_fbar_bf16
on the forward's own planes, for random upstream gradients and for each chain alone (g_feat = g_sdf = 0; g_normals = 0): every UB
block, EX[l], every AB block, d_pts (acc_pts = 0, and acc_pts = 1 into a pre-filled d_pts); vdn_sdf_bwd_split_bf16 gives UB and AB bit
for bit and leaves EX alone.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mlp_cases, mlp_ops
from test_gpu_ray_ops import GUARD as F32_GUARD
from test_gpu_ray_ops import Bufs, _call, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                      # NaN bf16 elements in front of and behind every plane
NAMES = list(mlp_cases.SDF_CASES)


class PlaneBufs(Bufs):
    """Bufs with NaN-filled bf16 planes (PT32, rows padded to 32) between NaN guard bands."""

    def plane(self, name, count, P, ld):
        from vdn_hip import layout
        n = count * layout.pad32(P) * ld
        base = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.bfloat16, device=DEV)
        self.outs[name] = (base, base[GUARD:GUARD + n].view(count, -1))
        return base[GUARD:].data_ptr()

    def check_guards(self):
        torch.cuda.synchronize()
        for name, (base, _) in self.outs.items():
            g = GUARD if base.dtype == torch.bfloat16 else F32_GUARD
            assert torch.isnan(base[:g]).all() and torch.isnan(base[-g:]).all(), "guard band of %s was written" % name

    def rows(self, name, i, P, ld, n_rows):
        """Plane i of `name` as [n_rows, ld] float64 (its first n_rows rows)."""
        from vdn_hip import layout
        return layout.from_pt32(self[name][i], P, ld)[:n_rows].double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _renderer(state):
    from vdn_train import factory
    st = mlp_cases.head_states(state) if state in ("heads", "heads-other", "heads352", "nodpt") else mlp_cases.states(state)
    return factory.build_renderer(wdepth=state != "nodpt", device=torch.device(DEV), states=st, precision="bf16",
                                  depth_before_color=state == "heads352")


@functools.lru_cache(maxsize=None)
def _sdf_images(state):
    """(refreshed NetImages of the SDF network, its operand weights layer by layer, those of the sweep's W_l^T by l)."""
    img = _renderer(state).sdf_network._images()
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(img)
    return img, mlp_ops.sdf_ops(host), mlp_ops.sdf_sweep_ops(host)


def _sdf_forward(c, state=None, entry="vdn_sdf_mlp_fwd_bf16"):
    """-> (PlaneBufs after the launch, planes {name: float64 rows} in the order of the saves, n_rows)."""
    from vdn_hip import lib
    img = _sdf_images(state or c["state"])[0]
    P = c["P"]
    b = PlaneBufs()
    a = lib.VdnSdfArgs()
    a.blob = img.blobs["full"].data_ptr()
    a.pts, a.n_per_ray, a.sdf_ld, a.P, a.scale = b.inp(c["pts"]), 1, 1, P, c["scale"]
    a.w8row = img.weff_view("lin8").data_ptr()
    a.sdf, a.normals = b.out("sdf", P), b.out("normals", P, 3)
    a.feat = b.plane("feat", 1, P, 256)
    a.H, a.V, a.PE = b.plane("H", 8, P, 256), b.plane("V", 8, P, 256), b.plane("PE", 1, P, 64)
    n = P
    if c["active_idx"] is not None:
        n = c["n_active"]
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([n]), torch.int32)
    if entry == "vdn_sdf_mlp_fwd_bf16":
        a.U_pe = b.out("U_pe", P, 39)
        _call(entry, 1, a, _stream())
    else:
        a.tail_row0, a.tail_max_rows = 0, 1 << 20
        _call(entry, a, _stream())
    b.check_guards()                                     # (what is finite is asserted plane by plane by the callers)
    planes = {"PE": b.rows("PE", 0, P, 64, n)[:, :39], "feat": b.rows("feat", 0, P, 256, n)}
    for l in range(8):
        planes["H%d" % l] = b.rows("H", l, P, 256, n)
        planes["V%d" % l] = b.rows("V", l, P, 256, n)
    if "U_pe" in b.outs:                                 # rows follow the saves
        assert torch.isnan(b["U_pe"][n:]).all(), "U_pe was written behind the last listed row"
        planes["U_pe"] = b.np("U_pe")[:n]
    sdf = b.np("sdf")
    if c["active_idx"] is not None:
        listed = np.zeros(P, bool)
        listed[c["active_idx"][:n]] = True
        assert np.isnan(sdf[~listed]).all() and np.isnan(b.np("normals")[~listed]).all(), "an unlisted point's outputs were written"
        planes["sdf"] = sdf[c["active_idx"][:n]]
        planes["normals"] = b.np("normals")[c["active_idx"][:n]]
    else:
        planes["sdf"], planes["normals"] = sdf, b.np("normals")
    return b, planes, n


def _hold(c, res, rows):
    for k, j in res.items():
        line = "%-22s %-7s bound %.2f units (fp32 floor %.3f)  kernel error %.3f units, %.2f of its allowance" % (
            c["name"], k, j["bound"], j["floor"], j["err"], j["used"])
        rows.append(line)
        assert j["ok"], "%s: %d of %d elements outside, first at %s" % (line, j["n_bad"], j["n"], j["worst"])


# ---- what the blob holds ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,state", [("sdf_network", "init"), ("sdf_network", "hot"), ("color_network", "init"),
                                       ("depth_network", "init"), ("nerf", "init"), ("color_network", "heads"), ("nerf", "heads"),
                                       ("color_network", "heads352"), ("nerf", "nodpt"), ("color_network", "heads-other")])
def test_blob_holds_the_operand_weights(net, state):
    """vdn_build_images, fmt 1: every chunk of every stream decoded by the documented layout (vdn_hip/layout.py
    decode_chunk_bf16) equals operand_weights - bf16_rne(float32(scale) W_eff[nmap, kmap]), zeros at -1 map entries, the float32
    bias block, the tail constants - exactly; the rest of the bias block's KiB is zero. The colour network's states "heads" and
    "heads-other" are those of tests/test_gpu_fused_head_planes.py: their "c2" stream (the fused SDF launches' colour head) carries
    source column 32 of lin0 in every chunk's tail, which has to be among the decoded streams."""
    from vdn_hip import images, layout
    img = getattr(_renderer(state), net)._images()
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(img)
    assert img.fmt == images.FMT_BF16 and img.blobs
    n_chunks = 0
    for sname, blob in img.blobs.items():
        layers = img.streams[sname]
        stride = images.chunk_stride(max(max(L.kt for L in layers), images.STREAM_KT_MAX.get(sname, 0)), images.FMT_BF16)
        raw = blob.cpu()
        assert raw.numel() == stride * sum(len(L.chunks) for L in layers)
        off = 0
        for li in range(len(layers)):
            want = mlp_ops.operand_weights(host, sname, li)
            kt = want["kt"]
            for ci in range(want["n_chunks"]):
                chunk = raw[off:off + stride]
                W, bias = layout.decode_chunk_bf16(chunk, kt)
                where = "%s %s layer %d chunk %d" % (net, sname, li, ci)
                assert np.array_equal(W.double().numpy(), want["W"][32 * ci:32 * ci + 32]), where
                assert np.array_equal(bias.double().numpy(), want["b"][32 * ci:32 * ci + 32]), where
                assert not chunk[kt * 2048 + 128:kt * 2048 + 1024].any(), where + ": the bias block's padding"
                if want["tail"] is not None:
                    t0 = layers[li].tail[1]
                    got = chunk[t0:t0 + 4 * len(want["tail"])].clone().view(torch.float32).double().numpy()
                    assert np.array_equal(got, want["tail"]), where + ": tail"
                off += stride
                n_chunks += 1
    assert n_chunks > 20
    if net == "color_network" and state != "heads352":
        assert "c2" in img.blobs and all(L.tail is not None and L.tail[2] == 256 for L in img.streams["c2"])


# ---- the SDF forward --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_sdf_forward_planes_vs_float64_layer_models(name):
    c = mlp_cases.sdf_case(name)
    _, ops, ops_sweep = _sdf_images(c["state"])
    _, planes, n = _sdf_forward(c)
    models = mlp_ops.sdf_plane_models(ops, mlp_cases.rows_of(c), c["scale"], planes, ops_sweep)
    assert set(models) == set(planes)
    for k, m in models.items():
        got = planes[k][:, :m["y64"].shape[1]] if planes[k].ndim == 2 else planes[k]
        assert got.shape == m["y64"].shape and np.isfinite(got).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))


@pytest.mark.parametrize("name", NAMES)
def test_sdf_tail_entry_point_gives_the_same_planes_bit_for_bit(name):
    """vdn_sdf_fwd_tail_bf16 with tail_row0 = 0 (32-row workgroups) against the 128-row kernel: every row of every plane."""
    c = mlp_cases.sdf_case(name)
    _, big, n = _sdf_forward(c)
    _, tail, _ = _sdf_forward(c, entry="vdn_sdf_fwd_tail_bf16")
    assert set(big) == set(tail) | {"U_pe"}
    for k in tail:
        cols = 217 if k in ("H3", "V3") else big[k].shape[-1]
        x, y = (p[k][:, :cols] if p[k].ndim == 2 else p[k] for p in (big, tail))
        assert np.isfinite(x).all() and np.array_equal(x, y), (name, k)


def test_the_launch_on_the_other_weights_is_rejected():
    """The wiring from the launch to the comparator: the same launch on the OTHER state's blob, judged against this state's
    models, is rejected at every plane that depends on a weight matrix (the sdf row of W_8, which also makes V[7], is the
    geometric init's constant in both states; the encoding and its Jacobian have no weights)."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    _, ops, ops_sweep = _sdf_images(c["state"])
    _, planes, _ = _sdf_forward(c, state="other")
    res = mlp_ops.judge_planes(mlp_ops.sdf_plane_models(ops, c["pts"], c["scale"], planes, ops_sweep), planes)
    assert res["PE"]["ok"] and res["normals"]["ok"]
    for k, j in res.items():
        if k not in ("PE", "normals", "sdf", "V7"):
            assert not j["ok"] and j["err"] > 1e3, (k, j)


# ---- the heads' forward -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _head_images(net, state):
    img = getattr(_renderer(state), net)._images()
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(img)
    return img, [mlp_ops.operand_weights(host, "fwd", l) for l in range(5)]


MASK_FILL = 0xA5


def _head_forward(c, state=None):
    """The launch with every save -> (planes {name: float64 rows}, the four mask planes as bool [P,256])."""
    from vdn_hip import layout, lib
    img, _ = _head_images(c["net"], state or c["state"])
    P, d_out = c["P"], c["d_out"]
    b = PlaneBufs()
    a = lib.VdnRenderNetArgs()
    feat_in = layout.to_pt32(torch.as_tensor(c["feat"]).to(DEV))
    a.blob, a.feat = img.blobs["fwd"].data_ptr(), feat_in.data_ptr()
    a.pts, a.dirs, a.normals, a.n_per_ray = b.inp(c["pts"]), b.inp(c["dirs"]), b.inp(c["normals"]), 1
    a.P, a.d_out, a.squeeze_out = P, d_out, int(c["squeeze"])
    a.out = b.out("out", P, d_out)
    a.save_h, a.save_small = b.plane("h", 4, P, 256), b.plane("small", 1, P, 64)
    if c["extra"] is not None:
        a.extra, a.save_extra = b.inp(c["extra"]), b.plane("extra", 1, P, 96)
    n_mask = layout.pad32(P) * 32
    mask = torch.full((4 * n_mask + 2 * GUARD,), MASK_FILL, dtype=torch.uint8, device=DEV)
    a.save_mask = mask[GUARD:].data_ptr()
    _call("vdn_rendernet_fwd_bf16", a, _stream())
    b.check_guards()
    assert (mask[:GUARD] == MASK_FILL).all() and (mask[-GUARD:] == MASK_FILL).all(), "guard band of save_mask was written"
    planes = {"small": b.rows("small", 0, P, 64, P)[:, :33], "out": b.np("out")}
    if c["extra"] is not None:
        planes["extra"] = b.rows("extra", 0, P, 96, P)
    for l in range(4):
        planes["h%d" % l] = b.rows("h", l, P, 256, P)
    bits = [layout.mask_from_plane(mask[GUARD + l * n_mask:GUARD + (l + 1) * n_mask], P, 256).cpu().numpy() for l in range(4)]
    c["_fwd"] = (b, mask)                                # (the device buffers, for the backward launch)
    return planes, bits


def _head_models(c, planes):
    _, ops = _head_images(c["net"], c["state"])
    return mlp_ops.head_plane_models(ops, c["pts"], c["dirs"], c["normals"], mlp_ops.bf16_rne(c["feat"]), planes, c["squeeze"],
                                     c["d_out"], extra=c["extra"])


@pytest.mark.parametrize("name", list(mlp_cases.HEAD_CASES))
def test_head_forward_planes_vs_float64_layer_models(name):
    """vdn_rendernet_fwd_bf16 (colour head: 3 sigmoid outputs; VDN head: 96; the d_feature = 352 colour head with `extra` and
    save_extra) on explicit points and directions, with every save: save_small (and save_extra) from the inputs, save_h[0] from the
    feature plane it was given and its own save_small (and save_extra), save_h[1..3] and out from the plane before; save_mask =
    (save_h > 0) exactly; a unit whose pre-activation is exactly zero stores 0 and mask bit 0."""
    c = mlp_cases.head_case(name)
    planes, bits = _head_forward(c)
    models = _head_models(c, planes)
    assert set(models) == set(planes)
    for k in planes:
        assert np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))
    for l in range(4):
        assert np.array_equal(bits[l], planes["h%d" % l] > 0), "save_mask of layer %d" % l
    for l in (0, 2):
        assert (planes["h%d" % l][:, mlp_cases.SILENT_UNIT] == 0).all()


def test_the_head_launch_on_the_other_weights_is_rejected():
    """The wiring check of the heads: the colour head's launch on the OTHER state's blob (seed 4, the same units silenced), judged
    against this state's models, is rejected at every plane behind a weight matrix (save_small has none)."""
    c = mlp_cases.head_case("color-P33")
    planes, _ = _head_forward(c, state="heads-other")
    res = mlp_ops.judge_planes(_head_models(c, planes), planes)
    assert res["small"]["ok"]
    for k, j in res.items():
        if k != "small":
            assert not j["ok"] and j["err"] > 1e3, (k, j)


# ---- the heads' backward ------------------------------------------------------------------------------------------------------

def _head_backward(c, fwd, with_mask, acc=None):
    """vdn_rendernet_bwd_bf16 on the forward's own buffers. acc: {target: prefill} -> the acc_* = 1 forms on pre-filled targets."""
    from vdn_hip import layout, lib
    fb, mask = fwd
    img, _ = _head_images(c["net"], c["state"])
    P, d_out = c["P"], c["d_out"]
    ldo = 96 if d_out == 96 else 32
    b = PlaneBufs()
    a = lib.VdnRenderNetBwdArgs()
    a.blob, a.g_out, a.out, a.save_h = img.blobs["bwd"].data_ptr(), b.inp(mlp_cases.head_upstream(c)), fb["out"].data_ptr(), fb["h"].data_ptr()
    a.delta_out, a.delta_h, a.d_feat = b.plane("delta_out", 1, P, ldo), b.plane("delta_h", 4, P, 256), b.plane("d_feat", 1, P, 256)
    a.d_normals, a.d_pts, a.d_dirs = b.out("d_normals", P, 3), b.out("d_pts", P, 3), b.out("d_dirs", P, 3)
    a.dirs, a.n_per_ray, a.P, a.d_out, a.squeeze_out = b.inp(c["dirs"]), 1, P, d_out, int(c["squeeze"])
    if c["extra"] is not None:                           # (the kernel ADDS d loss / d extra into d_extra)
        a.d_extra = b.out("d_extra", P, 96)
        b["d_extra"].copy_(torch.as_tensor(_d_extra_before(c)).to(DEV))
    if acc is not None:
        a.acc_feat = a.acc_normals = a.acc_pts = 1
        b["d_feat"][0].copy_(layout.to_pt32(torch.as_tensor(acc["d_feat"]).float().to(DEV)))
        for k in ("d_normals", "d_pts", "d_dirs"):
            b[k].copy_(torch.as_tensor(acc[k]).float().to(DEV))
    if with_mask:
        a.mask = mask[GUARD:].data_ptr()
    _call("vdn_rendernet_bwd_bf16", a, _stream())
    b.check_guards()
    planes = {"delta_out": b.rows("delta_out", 0, P, ldo, P)[:, :d_out], "d_feat": b.rows("d_feat", 0, P, 256, P)}
    for l in range(4):
        planes["delta_h%d" % l] = b.rows("delta_h", l, P, 256, P)
    for k in ("d_normals", "d_pts", "d_dirs") + (("d_extra",) if c["extra"] is not None else ()):
        planes[k] = b.np(k)
    return planes


def _d_extra_before(c):
    return np.random.RandomState(11).standard_normal((c["P"], 96)).astype(np.float32)


@pytest.mark.parametrize("name", list(mlp_cases.HEAD_CASES))
def test_head_backward_planes_vs_float64_layer_models(name):
    """vdn_rendernet_bwd_bf16 on the forward's own planes: delta_out from g_out and out, every delta_h from the delta plane after
    it, d_feat / d_normals / d_pts from the saved delta_h[0], d_dirs through the encoding's Jacobian, d_extra (d_feature = 352) added
    into what it held; with `mask` the same bits as with mask = NULL; the acc_* = 1 forms add into pre-filled targets."""
    c = mlp_cases.head_case(name)
    fplanes, _ = _head_forward(c)
    fwd = c["_fwd"]
    planes = _head_backward(c, fwd, with_mask=False)
    for k in planes:
        assert np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    ops_bwd = [mlp_ops.operand_weights(mlp_ops.HostImages.of(_head_images(c["net"], c["state"])[0]), "bwd", l) for l in range(5)]
    hs = [fplanes["h%d" % l] for l in range(4)]
    g_out = mlp_cases.head_upstream(c)
    models = mlp_ops.head_bwd_plane_models(ops_bwd, g_out, fplanes["out"], hs, planes, c["squeeze"], c["d_out"],
                                           d_extra_before=None if c["extra"] is None else _d_extra_before(c).astype(np.float64))
    models["d_dirs"] = mlp_ops.head_d_dirs_model(ops_bwd, planes["delta_h0"], c["dirs"])
    assert set(models) == set(planes)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))
    masked = _head_backward(c, fwd, with_mask=True)
    for k in planes:
        assert np.array_equal(planes[k], masked[k]), "%s: with mask and with mask = NULL differ" % k
    # acc_* = 1: the same launch adds into what the targets held (bf16 plane: a rounding of the sum; f32: one more rounding)
    rs = np.random.RandomState(5)
    pre = {"d_feat": mlp_ops.bf16_rne(rs.standard_normal((c["P"], 256))), "d_normals": rs.standard_normal((c["P"], 3)).astype(np.float32),
           "d_pts": rs.standard_normal((c["P"], 3)).astype(np.float32), "d_dirs": rs.standard_normal((c["P"], 3)).astype(np.float32)}
    added = _head_backward(c, fwd, with_mask=True, acc=pre)
    for k in ("delta_out", "delta_h0", "delta_h1", "delta_h2", "delta_h3"):
        assert np.array_equal(planes[k], added[k]), k
    acc_models = {}
    for k in pre:
        m = models[k]
        y64 = m["y64"] + pre[k]
        acc_models[k] = dict(y64=y64, y32=m["y32"] + pre[k], unit=m["unit"] + mlp_ops.U24 * np.abs(y64), extra=m["extra"], stored=m["stored"])
    rows = []
    _hold(dict(c, name=name + "+acc"), mlp_ops.judge_planes(acc_models, added), rows)
    print("\n".join(rows))


# ---- the background network's forward ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nerf_images(state):
    img = _renderer(state).nerf._images()
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(img)
    return img, [mlp_ops.operand_weights(host, "fwd", l) for l in range(11)]


def _nerf_forward(c, state=None):
    """The launch with every save and both masks -> (planes, mask bits of pts_linears.0..7, mask bits of views_linears.0, rows)."""
    from vdn_hip import layout, lib
    img, _ = _nerf_images(state or c["state"])
    dpt = c["state"] != "nodpt"
    P = c["P"]
    b = PlaneBufs()
    a = lib.VdnNerfArgs()
    a.blob, a.pts4, a.dirs, a.n_per_ray, a.P = img.blobs["fwd"].data_ptr(), b.inp(c["pts4"]), b.inp(c["dirs"]), 1, P
    a.density, a.rgb = b.out("density", P), b.out("rgb", P, 3)
    if dpt:
        a.feat = b.out("feat", P, 96)
    a.save_h, a.save_pe, a.save_feature = b.plane("h", 8, P, 256), b.plane("pe", 1, P, 96), b.plane("feature", 1, P, 256)
    a.save_vpe, a.save_hv = b.plane("vpe", 1, P, 32), b.plane("hv", 1, P, 128)
    n_mask = layout.pad32(P) * 32
    mask = torch.full((8 * n_mask + n_mask // 2 + 3 * GUARD,), MASK_FILL, dtype=torch.uint8, device=DEV)
    mask_v = mask[GUARD + 8 * n_mask + GUARD:]
    a.save_mask, a.save_mask_v = mask[GUARD:].data_ptr(), mask_v.data_ptr()
    n = P
    if c["active_idx"] is not None:
        n = c["n_active"]
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([n]), torch.int32)
    _call("vdn_nerf_mlp_fwd_bf16", a, _stream())
    b.check_guards()
    for lo in (0, GUARD + 8 * n_mask, 2 * GUARD + 8 * n_mask + n_mask // 2):
        assert (mask[lo:lo + GUARD] == MASK_FILL).all(), "guard band of the masks was written"
    planes = {"pe": b.rows("pe", 0, P, 96, n)[:, :84], "vpe": b.rows("vpe", 0, P, 32, n)[:, :27],
              "feature": b.rows("feature", 0, P, 256, n), "hv": b.rows("hv", 0, P, 128, n)}
    for l in range(8):
        planes["h%d" % l] = b.rows("h", l, P, 256, n)
    sel = np.arange(P) if c["active_idx"] is None else c["active_idx"][:n]
    listed = np.zeros(P, bool)
    listed[sel] = True
    for k in ("density", "rgb") + (("feat",) if dpt else ()):
        assert np.isnan(b.np(k)[~listed]).all(), "%s of an unlisted point was written" % k
        planes[k] = b.np(k)[sel]
    bits = [layout.mask_from_plane(mask[GUARD + l * n_mask:GUARD + (l + 1) * n_mask], P, 256)[:n].cpu().numpy() for l in range(8)]
    c["_fwd"] = (b, mask, mask_v)                        # (the device buffers, for the backward launch)
    return planes, bits, layout.mask_from_plane(mask_v[:n_mask // 2], P, 128)[:n].cpu().numpy()


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_forward_planes_vs_float64_layer_models(name):
    """vdn_nerf_mlp_fwd_bf16 on explicit points and directions with every save and both masks (with the dpt head; once with a
    work list: saves in compact rows, outputs at the dense positions, every other output untouched; once without the dpt head:
    feat = NULL): save_pe / save_vpe from the inputs, every other plane and output from the planes before it; the masks =
    (plane > 0) exactly; the unit whose pre-activation is exactly zero."""
    c = mlp_cases.nerf_case(name)
    planes, bits, bits_v = _nerf_forward(c)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    models = mlp_ops.nerf_plane_models(_nerf_images(c["state"])[1], pts4, dirs, planes)
    assert set(models) == set(planes) and ("feat" in planes) == (c["state"] != "nodpt")
    for k in planes:
        assert np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))
    for l in range(8):
        assert np.array_equal(bits[l], planes["h%d" % l] > 0), "save_mask of layer %d" % l
    assert np.array_equal(bits_v, planes["hv"] > 0), "save_mask_v"
    assert (planes["h2"][:, mlp_cases.SILENT_UNIT] == 0).all()


def test_the_background_launch_on_the_other_weights_is_rejected():
    """The wiring check of the background network: the launch on the OTHER state's blob, judged against this state's models, is
    rejected at every plane behind a weight matrix (the two encodings have none)."""
    c = mlp_cases.nerf_case("nerf-P33")
    planes, _, _ = _nerf_forward(c, state="heads-other")
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    res = mlp_ops.judge_planes(mlp_ops.nerf_plane_models(_nerf_images(c["state"])[1], pts4, dirs, planes), planes)
    assert res["pe"]["ok"] and res["vpe"]["ok"]
    for k, j in res.items():
        if k not in ("pe", "vpe"):
            assert not j["ok"] and j["err"] > 1e3, (k, j)


# ---- the background network's backward --------------------------------------------------------------------------------------

def _nerf_backward(c, with_mask, input_adjoint=False):
    from vdn_hip import lib
    fb, mask, mask_v = c["_fwd"]
    img, _ = _nerf_images(c["state"])
    P = c["P"]
    g_density, g_rgb, g_feat = mlp_cases.nerf_upstream(c)
    b = PlaneBufs()
    a = lib.VdnNerfBwdArgs()
    a.blob, a.g_density, a.g_rgb, a.g_feat = img.blobs["bwd"].data_ptr(), b.inp(g_density), b.inp(g_rgb), b.inp(g_feat)
    a.save_h, a.save_hv, a.P, a.n_per_ray = fb["h"].data_ptr(), fb["hv"].data_ptr(), P, 1
    ldo = 128 if g_feat is not None else 32
    a.delta_o, a.delta_v = b.plane("delta_o", 1, P, ldo), b.plane("delta_v", 1, P, 128)
    a.delta_head, a.delta_h = b.plane("delta_head", 1, P, 288), b.plane("delta_h", 8, P, 256)
    n = P
    if c["active_idx"] is not None:
        n = c["n_active"]
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([n]), torch.int32)
    if with_mask:
        a.mask, a.mask_v = mask[GUARD:].data_ptr(), mask_v.data_ptr()
    if input_adjoint:                                    # (explicit inputs: rows by the dense point id)
        ig = lib.VdnNerfInputGradArgs()
        ig.pts4, ig.dirs, ig.accumulate = b.inp(c["pts4"]), b.inp(c["dirs"]), 0
        ig.d_pts4, ig.d_dirs = b.out("d_pts4", P, 4), b.out("d_dirs", P, 3)
        _call("vdn_nerf_mlp_bwd_input_bf16", a, ig, _stream())
    else:
        _call("vdn_nerf_mlp_bwd_bf16", a, _stream())
    b.check_guards()
    planes = {"delta_o": b.rows("delta_o", 0, P, ldo, n), "delta_v": b.rows("delta_v", 0, P, 128, n),
              "delta_head": b.rows("delta_head", 0, P, 288, n)[:, :257]}
    for l in range(8):
        planes["delta_h%d" % l] = b.rows("delta_h", l, P, 256, n)
    if input_adjoint:
        sel = np.arange(P) if c["active_idx"] is None else c["active_idx"][:n]
        listed = np.zeros(P, bool)
        listed[sel] = True
        for k in ("d_pts4", "d_dirs"):
            assert np.isnan(b.np(k)[~listed]).all(), "%s of an unlisted point was written" % k
            planes[k] = b.np(k)[sel]
    return planes


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_input_adjoint_vs_float64_models(name):
    """vdn_nerf_mlp_bwd_input_bf16: the delta planes of vdn_nerf_mlp_bwd_bf16 bit for bit, and d_pts4 / d_dirs = the encodings'
    Jacobians on the adjoints of the encoded inputs, modelled from the saved delta_h0, delta_h5 and delta_v."""
    c = mlp_cases.nerf_case(name)
    _nerf_forward(c)
    plain = _nerf_backward(c, with_mask=False)
    planes = _nerf_backward(c, with_mask=False, input_adjoint=True)
    for k in plain:
        assert np.array_equal(plain[k], planes[k]), "%s differs from vdn_nerf_mlp_bwd_bf16" % k
    ob = [mlp_ops.operand_weights(mlp_ops.HostImages.of(_nerf_images(c["state"])[0]), "bwd", l) for l in range(11)]
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    models = mlp_ops.nerf_input_adjoint_models(ob, pts4, dirs, planes)
    got = {k: planes[k] for k in models}
    for k in got:
        assert np.isfinite(got[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, got), rows)
    print("\n".join(rows))


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_backward_planes_vs_float64_layer_models(name):
    """vdn_nerf_mlp_bwd_bf16 on the forward's own planes (with and without the dpt head, with a work list: g_* at the dense
    positions, deltas in compact rows): delta_o from the upstream gradients, delta_v, delta_head and delta_h[7..0] each from the
    delta plane after it; with mask / mask_v the same bits as without."""
    c = mlp_cases.nerf_case(name)
    fplanes, _, _ = _nerf_forward(c)
    planes = _nerf_backward(c, with_mask=False)
    sel = slice(None) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    g = [None if x is None else x[sel] for x in mlp_cases.nerf_upstream(c)]
    ob = [mlp_ops.operand_weights(mlp_ops.HostImages.of(_nerf_images(c["state"])[0]), "bwd", l) for l in range(10)]
    # delta_o = [g_rgb (3) | padding | g_feat (96)]: the padding behind rgb is read by the GEMM of delta_v against zero rows of
    # W_out^T, so it has to be there and zero - the model holds it to exactly that
    models = mlp_ops.nerf_bwd_plane_models(ob, *g, [fplanes["h%d" % l] for l in range(8)], fplanes["hv"], planes)
    assert set(models) == set(planes)
    for k in planes:
        assert np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))
    masked = _nerf_backward(c, with_mask=True)
    for k in planes:
        assert np.array_equal(planes[k], masked[k]), "%s: with the masks and without differ" % k


# ---- the SDF backward -------------------------------------------------------------------------------------------------------

def _blocks(flat, P, cols, n):
    """The PT32 blocks of a flat workspace (UB / AB: P-row blocks of the given widths, one behind the other) as float64 rows."""
    from vdn_hip import layout
    Pp, out, off = layout.pad32(P), [], 0
    for w in cols:
        out.append(layout.from_pt32(flat[off:off + Pp * w], P, w)[:n].double().cpu().numpy())
        off += Pp * w
    return out


AB_COLS = (288,) + (256,) * 8


def _sdf_backward(c, fb, kind, entry, before=None):
    """rbar + fbar ("two") or vdn_sdf_bwd_split_bf16 ("split") on the forward's own planes -> (ub blocks, EX planes or None, ab
    blocks by layer). before [P,3]: fbar with acc_pts = 1 on a d_pts that holds it."""
    from vdn_hip import layout, lib
    img = _sdf_images(c["state"])[0]
    P = c["P"]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    n = P if c["active_idx"] is None else c["n_active"]
    rows = np.arange(P) if c["active_idx"] is None else c["active_idx"][:n]
    gf = np.zeros((P, 256), np.float32)
    gf[:n] = g_feat[rows]                                # (a plane: compact rows, like every save and delta)
    gf_plane = layout.to_pt32(torch.as_tensor(gf).to(DEV))
    b = PlaneBufs()
    rb, fa = lib.VdnSdfRbarArgs(), lib.VdnSdfFbarArgs()
    rb.blob, rb.pts, rb.n_per_ray, rb.z_ld, rb.P, rb.scale = img.blobs["full"].data_ptr(), b.inp(c["pts"]), 1, 1, P, c["scale"]
    rb.g_normals, rb.S, rb.V, rb.s_from_h = b.inp(g_n), fb["H"].data_ptr(), fb["V"].data_ptr(), 2
    rb.UB, rb.EX = b.plane("UB", 1, P, 2144), b.plane("EX", 8, P, 256)
    fa.blob, fa.g_sdf, fa.g_feat = img.blobs["fbar"].data_ptr(), b.inp(g_sdf), gf_plane.data_ptr()
    fa.S, fa.EX, fa.AB, fa.P, fa.scale, fa.s_from_h = fb["H"].data_ptr(), b["EX"].data_ptr(), b.plane("AB", 1, P, 2336), P, c["scale"], 2
    if c["active_idx"] is not None:
        rb.active_idx = fa.active_idx = b.inp(c["active_idx"], torch.int32)
        rb.n_active = fa.n_active = b.inp(np.asarray([n]), torch.int32)
    if entry == "two":                                   # (with the ray adjoint, which the one-launch form declines)
        fa.pts, fa.n_per_ray, fa.z_ld, fa.g_normals, fa.U_pe = rb.pts, 1, 1, rb.g_normals, fb["U_pe"].data_ptr()
        fa.acc_pts, fa.d_pts = int(before is not None), b.out("d_pts", P, 3)
        if before is not None:
            b["d_pts"].copy_(torch.as_tensor(before).to(DEV))
        _call("vdn_sdf_bwd_rbar_bf16", rb, _stream())
        _call("vdn_sdf_bwd_fbar_bf16", fa, _stream())
    else:
        _call("vdn_sdf_bwd_split_bf16", rb, fa, _stream())
    b.check_guards()
    ub = _blocks(b["UB"][0], P, mlp_ops.UB_COLS, n)
    ab = _blocks(b["AB"][0], P, AB_COLS, n)[::-1]        # (stored ab8, ab7, .. ab0: index by layer)
    if entry == "split":
        assert torch.isnan(b["EX"]).all(), "the split launch wrote EX"
        return ub, None, ab
    d_pts = b.np("d_pts")
    listed = np.zeros(P, bool)
    listed[rows] = True
    if before is None:
        assert np.isnan(d_pts[~listed]).all(), "d_pts of an unlisted point was written"
    else:
        assert np.array_equal(d_pts[~listed], np.asarray(before, np.float64)[~listed]), "d_pts of an unlisted point was written"
    c["_d_pts"] = d_pts[rows]
    return ub, [b.rows("EX", l, P, 256, n) for l in range(8)], ab


SDF_BWD = [(name, "random") for name in NAMES] + [("uniform-P129-s1", k) for k in mlp_cases.SDF_UPSTREAM[1:]] + \
          [("hot-P300-s1.5", k) for k in mlp_cases.SDF_UPSTREAM[1:]]


@pytest.mark.parametrize("name,kind", SDF_BWD)
def test_sdf_backward_blocks_vs_float64_layer_models(name, kind):
    """vdn_sdf_bwd_rbar_bf16 then vdn_sdf_bwd_fbar_bf16 on the forward's own planes: ub_0 from g_normals, every further UB block
    and EX[l] from the UB block before it (and H[l], V[l]), ab_8 from g_feat / g_sdf, every further AB block from the AB block
    after it (and H, EX), d_pts from ab_0, ab_4 and the forward's U_pe. vdn_sdf_bwd_split_bf16 gives UB and AB bit for bit and leaves
    EX alone. With g_normals = 0, UB and EX are
    exactly zero. fbar's acc_pts = 1 adds the ray adjoint into a pre-filled d_pts."""
    c = mlp_cases.sdf_case(name)
    fb, fplanes, n = _sdf_forward(c)
    ub, EX, ab = _sdf_backward(c, fb, kind, "two")
    img, ops, _ = _sdf_images(c["state"])
    ofb = mlp_ops.sdf_fbar_ops(mlp_ops.HostImages.of(img))
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:n]
    H, V = [fplanes["H%d" % l] for l in range(8)], [fplanes["V%d" % l] for l in range(8)]
    models = mlp_ops.sdf_bwd_models(ops, ofb, mlp_cases.rows_of(c), c["scale"], g_sdf[sel], mlp_ops.bf16_rne(g_feat[sel]), g_n[sel],
                                    H, V, ub, EX, ab)
    planes = {"ub0": ub[0][:, :39], "ub4pe": ub[4][:, 224:263], "ab8": ab[8][:, :257], "d_pts": c["_d_pts"]}
    for l in range(8):
        w = 217 if l == 3 else 256
        planes["ub%d" % (l + 1)], planes["EX%d" % l], planes["ab%d" % l] = ub[l + 1][:, :w], EX[l][:, :w], ab[l][:, :w]
    models["d_pts"] = mlp_ops.sdf_d_pts_model(ofb, mlp_cases.rows_of(c), c["scale"], g_n[sel], fplanes["U_pe"], ab[0], ab[4])
    assert set(models) == set(planes)
    for k in planes:
        assert np.isfinite(planes[k]).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(dict(c, name="%s/%s" % (name, kind)), mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))
    if kind == "g_normals=0":
        assert all((planes[k] == 0).all() for k in planes if k.startswith(("ub", "EX")))
    # acc_pts = 1: the same launches add the adjoint into what d_pts held (one more rounding), the blocks bit for bit
    before = mlp_cases.sdf_d_pts_prefill(c)
    ub3, EX3, ab3 = _sdf_backward(c, fb, kind, "two", before=before)
    assert all(np.array_equal(x, y, equal_nan=True) for a3, a in ((ub3, ub), (EX3, EX), (ab3, ab)) for x, y in zip(a3, a))
    acc = mlp_ops.sdf_d_pts_model(ofb, mlp_cases.rows_of(c), c["scale"], g_n[sel], fplanes["U_pe"], ab[0], ab[4], before=before[sel])
    rows = []
    _hold(dict(c, name="%s/%s+acc" % (name, kind)), mlp_ops.judge_planes({"d_pts": acc}, {"d_pts": c["_d_pts"]}), rows)
    print("\n".join(rows))
    ub2, _, ab2 = _sdf_backward(c, fb, kind, "split")
    for l in range(9):
        for tag, x, y in (("ub", ub[l], ub2[l]), ("ab", ab[l], ab2[l])):
            w = {("ub", 0): 39, ("ub", 4): None, ("ab", 8): 257, ("ab", 3): 217}.get((tag, l), 256)
            if w is None:
                assert np.array_equal(x[:, :217], y[:, :217]) and np.array_equal(x[:, 224:263], y[:, 224:263]), "ub4: split differs"
            else:
                assert np.array_equal(x[:, :w], y[:, :w]), "%s%d: the split launch differs" % (tag, l)
