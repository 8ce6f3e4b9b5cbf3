"""The bf16 SDF launches that save no planes, and the hand-off of a work list's tail, through the C ABI (include/vdn_render.h): each
held, BIT FOR BIT, to the one launch tests/test_gpu_mlp_planes.py holds to float64 plane by plane - vdn_sdf_mlp_fwd_bf16 mode 1 with
the training saves (csrc/k_sdf_fwd2.h, sdf2::launch<1, true, 4, 3>), "the training launch" below - on the same points and weights.

Why bits and not a bound. Read from the code, the hidden layers and the sdf row of mode 0 are operation for operation those of
mode 1. csrc/k_sdf_fwd2.h instantiates ONE kernel body for Prog<0> and Prog<1>: the same encoding and residue slots, the same chunk
step (bias into the accumulator, k-steps in order), the same softplus_sigma and bf16 packing, and the sdf row as the f32 fma chain of
layer 7's epilogue over the UNROUNDED activations (tile by tile, pair by pair, W_8's row 0 from the chunks' tails), the two lane
halves added once, then fmaf(dot, 1 / (100 log2 e), b_8[0]) * (1 / scale) - Prog<0> only stops after one chunk of layer 8 and
takes b_8[0] from that chunk's bias block instead of the ninth's. csrc/k_sdf_fwd0_split.h (up to 8192 points) writes the same
expressions in the same order with the features split over the waves. Ring depth (4 or 5 slots), barrier cadence, occupancy and the
cold-start prologue move no arithmetic. The premise - layers 0..7 of the "sdf" stream ARE those of "full", its layer 8 is row 256 of
"full"'s with the same bias and tail - is checked once on the device's blobs (and on the host by tests/test_mlp_ops_model_cpu.py).
So the promise is equality of bits, include/vdn_render.h states it at VdnSdfArgs, and a difference is a finding, not a tolerance.

Cases: oracle/mlp_cases.py SDF_VALUE_CASES - SDF_CASES as they are (explicit points; a work list; both hot states); the ray form with z
and sdf as column slices of wider rows (z_ld > n_per_ray, sdf_ld != z_ld, non-zero first columns; 1 row, ray boundaries inside a
wave, the split kernel's two rays per workgroup, 2 x 64, 129 rows at scale 1.5, a work list); P = 8193 and a work list in P = 8200,
which the entry point routes to the 128-point kernel, their points the 300-row case tiled. tests/test_mlp_ops_model_cpu.py proves
that another ray, column, stride or weight state, or a missing 1 / scale, moves the sdf of every row.

  * the anchor of the ray cases: the ray-form training launch itself, every plane against the float64 one-layer models at the
    float64 points o + d z, with the point's own float32 rounding (mlp_ops.ray_points) added to the encoding's extra term;
  * mode 0, split kernel: sdf = the training launch's sdf; guard bands, unlisted points, and in ray form every element outside
    the column slice still NaN;
  * mode 0, 128-point kernel (P > 8192): every row = the split kernel's value of the same point of the 300-row case, so every
    repetition carries the same bits;
  * the inference launch (mode 1, H = V = PE = NULL; 5-slot ring): sdf, normals and the listed rows of feat = the training
    launch's; nothing behind the last listed row of feat; the large cases' training launch = the 300-row one, tiled;
  * cold_start = 1: the bits of cold_start = 0;
  * the tail hand-off (VdnSdfArgs.tail_row0 / tail_max_rows; csrc/k_sdf_fwd2.h MODE 1 against csrc/k_sdf_fwd1_split.h, SAVE = true
    and false), on a dense launch and on a work list whose count is read on the device: after the main launch alone the handed-off
    rows and their points' outputs are untouched and the rows below final; the tail launch alone writes nothing below tail_row0 or
    behind the list; both together = the single launch with tail_max_rows = 0, every plane, bit for bit; the tail idle, one row,
    172 rows, the second workgroup boundary, a list that ends beyond the window;
  * what the tail entry point refuses (-4, -4, -10) writes nothing;
  * the launches on the OTHER state's blobs differ from this state's training launch in every row.

Every output is pre-filled with NaN between guard bands. Columns 217..255 of H[3] and V[3] are not outputs of layer 3 and are not
compared (they are still required to be untouched where a whole row is).

Measured on the MI355X: every comparison above is exact. The anchor (ray-form training launch, 6 cases; bound = max(1, 3 x float32
floor) units + the plane's extra term, as in tests/test_gpu_mlp_planes.py):

sdf (rays) PE          6 cases  bound <=  1.00  floor <= 0.319  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf (rays) H0          6 cases  bound <=  3.00  floor <= 0.998  kernel error <= 0.998 units, <= 0.33 of its allowance
sdf (rays) H1          6 cases  bound <=  4.67  floor <= 1.555  kernel error <= 0.999 units, <= 0.27 of its allowance
sdf (rays) H2          6 cases  bound <=  5.28  floor <= 1.761  kernel error <= 1.000 units, <= 0.27 of its allowance
sdf (rays) H3          6 cases  bound <=  5.25  floor <= 1.752  kernel error <= 0.999 units, <= 0.33 of its allowance
sdf (rays) H4          6 cases  bound <=  3.00  floor <= 1.000  kernel error <= 1.000 units, <= 0.33 of its allowance
sdf (rays) H5          6 cases  bound <=  5.56  floor <= 1.854  kernel error <= 1.000 units, <= 0.29 of its allowance
sdf (rays) H6          6 cases  bound <=  6.23  floor <= 2.076  kernel error <= 0.997 units, <= 0.23 of its allowance
sdf (rays) H7          6 cases  bound <=  5.08  floor <= 1.693  kernel error <= 0.999 units, <= 0.30 of its allowance
sdf (rays) feat        6 cases  bound <= 14.24  floor <= 4.747  kernel error <= 0.000 units, <= 0.00 of its allowance
sdf (rays) sdf         6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.18 of its allowance
sdf (rays) V7          6 cases  bound <=  1.01  floor <= 0.336  kernel error <= 0.000 units, <= 0.99 of its allowance
sdf (rays) V6          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (rays) V5          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf (rays) V4          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (rays) V3          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf (rays) V2          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (rays) V1          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.98 of its allowance
sdf (rays) V0          6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.97 of its allowance
sdf (rays) U_pe        6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.24 of its allowance
sdf (rays) normals     6 cases  bound <=  1.00  floor <= 0.000  kernel error <= 0.000 units, <= 0.23 of its allowance

74 tests, 4 s. No defect found.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mlp_cases, mlp_ops
from test_gpu_mlp_planes import PlaneBufs, _hold, _sdf_images
from test_gpu_ray_ops import _call, _status, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINT_NAMES = list(mlp_cases.SDF_CASES)
RAY_NAMES = list(mlp_cases.SDF_VALUE_RAY_CASES)
LARGE_NAMES = list(mlp_cases.SDF_VALUE_LARGE_CASES)
PLANES = ("PE", "H", "V", "feat")
LD = {"PE": 64, "H": 256, "V": 256, "feat": 256}
COUNT = {"PE": 1, "H": 8, "V": 8, "feat": 1}


@functools.lru_cache(maxsize=None)
def _case(name):
    return mlp_cases.sdf_value_case(name)


def _block(c, b, kind, state=None, cold=0, tail=(0, 0), u_pe=False):
    """VdnSdfArgs of a case with NaN-filled outputs in `b`. kind: "mode0" (the "sdf" stream; sdf only), "infer" (mode 1 without
    saves), "train" (mode 1 with H, V, PE; U_pe on request). Ray form: z and sdf point INTO their wider rows."""
    from vdn_hip import lib
    img = _sdf_images(state or c["state"])[0]
    P = c["P"]
    a = lib.VdnSdfArgs()
    a.blob = img.blobs["sdf" if kind == "mode0" else "full"].data_ptr()
    a.P, a.scale, a.cold_start = P, c["scale"], cold
    a.tail_row0, a.tail_max_rows = tail
    if c["form"] == "pts":
        a.pts, a.n_per_ray, a.sdf_ld = b.inp(c["pts"]), 1, 1
        a.sdf = b.out("sdf", P)
    else:
        z = torch.as_tensor(c["z_wide"]).to(DEV)
        b.keep.append(z)
        a.rays_o, a.rays_d, a.z = b.inp(c["rays_o"]), b.inp(c["rays_d"]), z[:, c["z_col0"]:].data_ptr()
        a.n_per_ray, a.z_ld, a.sdf_ld = c["n_per_ray"], c["z_ld"], c["sdf_ld"]
        b.out("sdf", c["B"], c["sdf_ld"])
        a.sdf = b["sdf"][:, c["sdf_col0"]:].data_ptr()
    if kind != "mode0":
        a.w8row = img.weff_view("lin8").data_ptr()
        a.normals, a.feat = b.out("normals", P, 3), b.plane("feat", 1, P, 256)
    if kind == "train":
        a.H, a.V, a.PE = b.plane("H", 8, P, 256), b.plane("V", 8, P, 256), b.plane("PE", 1, P, 64)
        if u_pe:
            a.U_pe = b.out("U_pe", P, 39)
    if c["active_idx"] is not None:
        a.active_idx, a.n_active = b.inp(c["active_idx"], torch.int32), b.inp(np.asarray([c["n_active"]]), torch.int32)
    return a


def _n_rows(c):
    return c["P"] if c["active_idx"] is None else c["n_active"]


def _ids(c, lo=0, hi=None):
    """The dense point ids behind rows [lo, hi) of the list, on the device."""
    return torch.as_tensor(mlp_cases.value_rows_of(c)[lo:hi]).long().to(DEV)


def _sdf_by_point(c, b):
    """sdf [P] by dense point id; in ray form everything outside the column slice must still be NaN."""
    s = b["sdf"]
    if c["form"] == "pts":
        return s
    inside = torch.zeros_like(s, dtype=torch.bool)
    inside[:, c["sdf_col0"]:c["sdf_col0"] + c["n_per_ray"]] = True
    assert torch.isnan(s[~inside]).all(), "sdf was written outside its column slice"
    return s[:, c["sdf_col0"]:c["sdf_col0"] + c["n_per_ray"]].reshape(-1)


def _outputs(c, b):
    """{sdf, normals} by dense point id."""
    out = {"sdf": _sdf_by_point(c, b)}
    if "normals" in b.outs:
        out["normals"] = b["normals"]
    return out


def _written(c, b, lo=0, hi=None):
    """The guard bands are intact, the per-point outputs of rows [lo, hi) of the list are finite and every other one is NaN."""
    b.check_guards()
    ids = _ids(c, lo, hi)
    for k, t in _outputs(c, b).items():
        listed = torch.zeros(c["P"], dtype=torch.bool, device=DEV)
        listed[ids] = True
        assert torch.isfinite(t[listed]).all(), "%s has unwritten or non-finite elements" % k
        assert torch.isnan(t[~listed]).all(), "%s of a point outside rows [%s, %s) was written" % (k, lo, hi)


def _rows(b, name, i, P):
    """Plane i of `name`, every row up to pad32(P), float32 (a bf16 value converts exactly)."""
    from vdn_hip import layout
    return layout.from_pt32(b[name][i], layout.pad32(P), LD[name])


def _cols(name, i):
    return 217 if name in ("H", "V") and i == 3 else (39 if name == "PE" else LD[name])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(x, y):
    return x.shape == y.shape and bool(torch.isfinite(x).all()) and torch.equal(_bits(x), _bits(y))


def _launch(c, kind, **kw):
    b = PlaneBufs()
    a = _block(c, b, kind, **kw)
    _call("vdn_sdf_mlp_fwd_bf16", 0 if kind == "mode0" else 1, a, _stream())
    _written(c, b)
    return b


@functools.lru_cache(maxsize=None)
def _train(name, state=None):
    """The training launch of a case: the reference of everything below (computed once, never modified)."""
    return _launch(_case(name), "train", state=state, u_pe=True)


@functools.lru_cache(maxsize=None)
def _split_tile():
    """The split kernel's sdf of the 300-row case the large cases tile."""
    return _launch(_case(mlp_cases.SDF_VALUE_TILE), "mode0")["sdf"]


def _equal_outputs(c, b, ref, what):
    for k, t in _outputs(c, b).items():
        full, want = b[k], ref[k]                             # (the whole buffers: the NaN of every untouched element included)
        assert full.shape == want.shape and torch.equal(_bits(full), _bits(want)), "%s: %s differs from %s" % (c["name"], k, what)


def _equal_feat(c, b, ref, what):
    n, P = _n_rows(c), c["P"]
    got, want = _rows(b, "feat", 0, P), _rows(ref, "feat", 0, P)
    assert _same(got[:n], want[:n]), "%s: feat differs from %s" % (c["name"], what)
    assert torch.isnan(got[n:]).all(), "%s: feat was written behind the last listed row" % c["name"]


# ---- the premise ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["init", "hot"])
def test_the_sdf_stream_holds_the_first_nine_layers_of_the_full_stream(state):
    """On the blobs the launches read: the 63 chunks of layers 0..7 are the same bytes in "sdf" and "full" (weights, bias blocks,
    tails, padding); the one chunk of "sdf"'s layer 8 decodes to the sdf row - row 0 of the ninth chunk of "full"'s layer 8 - with
    the same bias and the same f32 tail, every other row zero; and both streams' layers equal operand_weights of each other."""
    from vdn_hip import images, layout
    img = _sdf_images(state)[0]
    torch.cuda.synchronize()
    host = mlp_ops.HostImages.of(img)
    stride = images.chunk_stride(9, images.FMT_BF16)
    sdf, full = img.blobs["sdf"].cpu(), img.blobs["full"].cpu()
    n_hidden = sum(len(L.chunks) for L in img.streams["sdf"][:8])
    assert n_hidden == 63 and sdf.numel() == 64 * stride and len(img.streams["full"][8].chunks) == 9
    assert full.numel() == stride * sum(len(L.chunks) for L in img.streams["full"])
    assert [len(L.chunks) for L in img.streams["full"][:8]] == [len(L.chunks) for L in img.streams["sdf"][:8]]
    assert torch.equal(sdf[:63 * stride], full[:63 * stride])
    for l in range(8):
        a, b = mlp_ops.operand_weights(host, "sdf", l), mlp_ops.operand_weights(host, "full", l)
        assert a["kt"] == b["kt"] and all(np.array_equal(a[k], b[k]) for k in ("W", "b", "tail"))
    last = sdf[63 * stride:64 * stride]
    W, bias = layout.decode_chunk_bf16(last, 8)
    W9, bias9 = layout.decode_chunk_bf16(full[(63 + 8) * stride:(63 + 9) * stride], 8)
    assert torch.equal(W[0], W9[0]) and torch.equal(bias[:1], bias9[:1]) and W[0].any() and bias[0] != 0
    assert not W[1:].any() and not bias[1:].any()
    t0 = images.SDF_TAIL_OFF
    assert torch.equal(last[t0:t0 + 1024], full[t0:t0 + 1024]) and torch.equal(last[t0:t0 + 1024], full[71 * stride + t0:71 * stride + t0 + 1024])
    want = mlp_ops.operand_weights(host, "sdf", 8)
    assert np.array_equal(W.double().numpy(), want["W"]) and np.array_equal(last[t0:t0 + 1024].clone().view(torch.float32).double().numpy(), want["tail"])


# ---- the anchor of the ray cases ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RAY_NAMES)
def test_ray_form_training_launch_planes_vs_float64_layer_models(name):
    """vdn_sdf_mlp_fwd_bf16 mode 1 with saves in RAY form (test_gpu_mlp_planes.py holds it on explicit points): every plane against
    the float64 one-layer models at the float64 points o + d z of the listed rows, the launch's own float32 point within
    mlp_ops.ray_points' bound of them; sdf read at r sdf_ld + s of the wide buffer, nothing else of which is written."""
    c = _case(name)
    b = _train(name)
    n, P = _n_rows(c), c["P"]
    ids = _ids(c)
    f64 = lambda t: t.double().cpu().numpy()
    planes = {"PE": f64(_rows(b, "PE", 0, P)[:n, :39]), "feat": f64(_rows(b, "feat", 0, P)[:n]), "U_pe": f64(b["U_pe"][:n]),
              "sdf": f64(_sdf_by_point(c, b)[ids]), "normals": f64(b["normals"][ids])}
    assert torch.isnan(b["U_pe"][n:]).all(), "U_pe was written behind the last listed row"
    for l in range(8):
        planes["H%d" % l], planes["V%d" % l] = f64(_rows(b, "H", l, P)[:n]), f64(_rows(b, "V", l, P)[:n])
    _, ops, ops_sweep = _sdf_images(c["state"])
    p64, err = mlp_ops.ray_points(c["rays_o"], c["rays_d"], c["z"], mlp_cases.value_rows_of(c))
    models = mlp_ops.sdf_plane_models(ops, p64, c["scale"], planes, ops_sweep, pts_err=err)
    assert set(models) == set(planes)
    for k, m in models.items():
        got = planes[k][:, :m["y64"].shape[1]] if planes[k].ndim == 2 else planes[k]
        assert got.shape == m["y64"].shape and np.isfinite(got).all(), "%s %s: unwritten or non-finite elements" % (name, k)
    rows = []
    _hold(c, mlp_ops.judge_planes(models, planes), rows)
    print("\n".join(rows))


# ---- mode 0 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", POINT_NAMES + RAY_NAMES)
def test_mode0_split_kernel_gives_the_training_launch_sdf_bit_for_bit(name):
    """vdn_sdf_mlp_fwd_bf16 mode 0 up to 8192 points (csrc/k_sdf_fwd0_split.h) on the "sdf" stream: the training launch's sdf of
    every listed point; unlisted points, the columns outside the slice and the guard bands untouched."""
    c = _case(name)
    b = _launch(c, "mode0")
    assert set(b.outs) == {"sdf"}
    _equal_outputs(c, b, _train(name), "the training launch")


@pytest.mark.parametrize("name", LARGE_NAMES)
def test_mode0_large_kernel_gives_the_split_kernel_sdf_of_every_repetition(name):
    """P > 8192 (csrc/k_sdf_fwd2.h MODE 0): row i carries the split kernel's bits of point i % 300 - which the test above holds to
    the training launch -, so every repetition is identical; unlisted points and guard bands untouched."""
    c = _case(name)
    assert c["P"] > 8192 and c["tile"] == 300
    b = _launch(c, "mode0")
    ids = _ids(c)
    tile = _split_tile()
    assert torch.isfinite(tile).all() and torch.equal(_bits(b["sdf"][ids]), _bits(tile[ids % c["tile"]])), name


# ---- the inference launch -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", POINT_NAMES + RAY_NAMES + LARGE_NAMES)
def test_inference_launch_gives_the_training_launch_bit_for_bit(name):
    """vdn_sdf_mlp_fwd_bf16 mode 1 with H = V = PE = NULL (sdf2::launch<1, false, 5, 3>: the 5-slot ring, one barrier per two chunk
    steps): sdf, normals and the listed rows of feat are the training launch's bits; nothing behind the last listed row of feat.
    The large cases' training launch is, row by row, the 300-row case's."""
    c = _case(name)
    ref = _train(name)
    b = _launch(c, "infer")
    assert set(b.outs) == {"sdf", "normals", "feat"}
    _equal_outputs(c, b, ref, "the training launch")
    _equal_feat(c, b, ref, "the training launch")
    if c["tile"]:
        t = _train(mlp_cases.SDF_VALUE_TILE)
        ids = _ids(c)
        for k in ("sdf", "normals"):
            assert torch.equal(_bits(ref[k][ids]), _bits(t[k][ids % c["tile"]])), "%s: %s of a repetition differs" % (name, k)
        assert _same(_rows(ref, "feat", 0, c["P"])[:len(ids)], _rows(t, "feat", 0, c["tile"])[ids % c["tile"]])


# ---- the cold-start prologue ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", [("mode0", "uniform-P300-s1.5"), ("mode0", "value-rays-3x43-s1.5"), ("infer", "uniform-P300-s1.5"),
                                       ("infer", "value-rays-3x43-s1.5"), ("mode0", "cold-tiled-P4097-s1.5"), ("mode0", "cold-rays-65x64-s1"),
                                       ("mode0", "cold-tiled-P16385-s1.5"), ("mode0", "cold-rays-257x64-s1"),
                                       ("infer", "cold-tiled-P16385-s1.5"), ("infer", "cold-rays-257x64-s1")])
def test_cold_start_changes_no_bit(kind, name):
    """cold_start = 1 (the first round of workgroups reads the weight stream and the kernel's code ahead: warm_l2, warm_code)
    against cold_start = 0 of the same launch: on small cases, where the prologue only adds its barrier, and on the smallest
    launches whose first round is wide enough (128 workgroups) for it to read ahead - the split kernel, the 128-point MODE 0 and
    the inference launch, explicit points and ray form; the tiled ones also against the 300-row case they tile."""
    c = _case(name)
    warm, cold = _launch(c, kind), _launch(c, kind, cold=1)
    _equal_outputs(c, cold, warm, "cold_start = 0")
    if kind == "infer":
        _equal_feat(c, cold, warm, "cold_start = 0")
    if c["tile"]:
        ids = _ids(c)
        if kind == "mode0":
            assert torch.equal(_bits(cold["sdf"]), _bits(_split_tile()[ids % c["tile"]]))
        else:
            t = _train(mlp_cases.SDF_VALUE_TILE)
            for k in ("sdf", "normals"):
                assert torch.equal(_bits(cold[k]), _bits(t[k][ids % c["tile"]])), k
            assert _same(_rows(cold, "feat", 0, c["P"])[:c["P"]], _rows(t, "feat", 0, c["tile"])[ids % c["tile"]])


# ---- the tail hand-off ------------------------------------------------------------------------------------------------------------

def _plane_names(b):
    return [k for k in PLANES if k in b.outs]


@pytest.mark.parametrize("split", mlp_cases.SDF_TAIL_SPLITS, ids=lambda s: "row0=%d-max=%d-n=%d" % s)
@pytest.mark.parametrize("save", [True, False], ids=["saves", "no-saves"])
@pytest.mark.parametrize("form", ["dense", "list"])
def test_tail_hand_off_writes_every_row_exactly_once(form, save, split):
    """vdn_sdf_mlp_fwd_bf16 mode 1 and vdn_sdf_fwd_tail_bf16 on the SAME struct, each deciding on the device-side row count.
    (a) The main launch alone leaves the handed-off rows of every plane, and the outputs of their points, untouched; the rows
    below are the single launch's. (b) The tail launch alone writes nothing below tail_row0 and nothing behind the list. (c) Both
    give the single launch (tail_max_rows = 0) bit for bit: PE, H[0..7], V[0..7] (217 columns of H[3] / V[3]), feat, sdf, normals."""
    row0, max_rows, n = split
    c = mlp_cases.sdf_tail_case(form, n)
    P, kind = c["P"], "train" if save else "infer"
    assert _n_rows(c) == n
    off = mlp_cases.handed_off(*split)
    lo = row0 if off else n                                  # rows [0, lo) are the main launch's, [lo, n) the tail's
    single = _launch(c, kind)

    def compare(b, r0, r1, what):
        for k, t in _outputs(c, b).items():
            ids = _ids(c, r0, r1)
            assert torch.equal(_bits(t[ids]), _bits(_outputs(c, single)[k][ids])), "%s: %s differs from the single launch" % (what, k)
        for k in _plane_names(single):
            for i in range(COUNT[k]):
                got, want = _rows(b, k, i, P)[r0:r1, :_cols(k, i)], _rows(single, k, i, P)[r0:r1, :_cols(k, i)]
                assert _same(got, want), "%s: %s[%d] differs from the single launch" % (what, k, i)

    def untouched(b, r0, r1, what):
        for k in _plane_names(b):
            for i in range(COUNT[k]):
                rows = _rows(b, k, i, P)
                assert torch.isnan(rows[r0:r1]).all(), "%s: %s[%d] was written in rows [%d, %s)" % (what, k, i, r0, r1)

    # (a) the main launch alone, (c) then the tail launch on the same struct
    b = PlaneBufs()
    a = _block(c, b, kind, tail=(row0, max_rows))
    _call("vdn_sdf_mlp_fwd_bf16", 1, a, _stream())
    _written(c, b, 0, lo)
    assert set(_plane_names(b)) == (set(PLANES) if save else {"feat"})
    compare(b, 0, lo, "the main launch alone")
    untouched(b, lo, None, "the main launch alone")
    _call("vdn_sdf_fwd_tail_bf16", a, _stream())
    _written(c, b, 0, n)
    compare(b, 0, n, "main + tail")
    untouched(b, n, None, "main + tail")
    # (b) the tail launch alone
    bt = PlaneBufs()
    _call("vdn_sdf_fwd_tail_bf16", _block(c, bt, kind, tail=(row0, max_rows)), _stream())
    _written(c, bt, lo, n)
    untouched(bt, 0, lo, "the tail launch alone")
    untouched(bt, n, None, "the tail launch alone")
    compare(bt, lo, n, "the tail launch alone")


@pytest.mark.parametrize("save", [True, False], ids=["saves", "no-saves"])
def test_what_the_tail_entry_point_refuses_writes_nothing(save):
    c = mlp_cases.sdf_tail_case("dense", 300)
    kind = "train" if save else "infer"
    for tail, u_pe, entry, want in (((64, 256), False, "vdn_sdf_fwd_tail_bf16", -4), ((128, 0), False, "vdn_sdf_fwd_tail_bf16", -4),
                                    ((128, 256), True, "vdn_sdf_fwd_tail_bf16", -10)):
        if u_pe and not save:
            continue
        b = PlaneBufs()
        a = _block(c, b, kind, tail=tail, u_pe=u_pe)
        assert _status(entry, a, _stream()) == want, (tail, u_pe)
        b.check_guards()
        for k in b.outs:
            assert torch.isnan(b[k]).all(), "%s was written by a refused call" % k


# ---- the wiring -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform-P33-s1.5", "value-rays-3x11-s1"])
def test_the_launches_on_the_other_weights_differ_in_every_row(name):
    """The mode-0 and inference launches on the OTHER state's blobs against this state's training launch: every row of sdf, feat and
    normals differs (tests/test_mlp_ops_model_cpu.py: the other state moves the sdf of every row of these cases)."""
    c = _case(name)
    ref = _outputs(c, _train(name))
    m0 = _outputs(c, _launch(c, "mode0", state="other"))
    assert (m0["sdf"] != ref["sdf"]).all()
    bi = _launch(c, "infer", state="other")
    inf = _outputs(c, bi)
    assert (inf["sdf"] != ref["sdf"]).all() and (inf["normals"] != ref["normals"]).any(1).all()
    assert (_rows(bi, "feat", 0, c["P"])[:c["P"]] != _rows(_train(name), "feat", 0, c["P"])[:c["P"]]).any(1).all()
    assert torch.equal(_bits(m0["sdf"]), _bits(inf["sdf"]))   # (and the two plane-less launches agree with each other there too)
