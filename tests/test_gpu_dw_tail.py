"""The parameter-update tail of the training step as operators, through the C ABI (include/vdn_render.h), one launch per case:
vdn_dw_gemm_f32 / _bf16, vdn_dw_finalize, vdn_weightnorm_materialize, vdn_weightnorm_bwd, vdn_adam_step / _ranges, against the
float64 models of oracle/dw_ops.py on the constructed inputs of oracle/dw_cases.py (whose models, exactness and branch coverage
tests/test_dw_ops_model_cpu.py proves without a GPU).

Every output buffer is pre-filled (NaN, or the values a '+=' or an optimizer step starts from) and sits between two NaN guard
bands: after the launch every element the header says is written is finite and compared, every other element is bit-identical to
its pre-fill, the guard bands are untouched. The bands are wider than a target row and the Adam buffers longer than the ranges
need, so a kernel that follows a -1 map entry or forgets to rebase the second range shows as a changed element, not as an
out-of-bounds write. No element is excluded and no case skipped.

exact cases (small integers, power-of-two scales): bit-identical to the float64 model cast to float32. Splits without rows, and
the column sums of second-segment splits, are exactly 0.
random cases: the kernel's error in units (dw_ops.*_units: 2^-24 times the sum of the absolute terms of the element) is held to
max(1, 3 x floor), the floor being the float32 model's error against the float64 model in the same units - measured at run time
from the reference, never from the kernel (tests/test_gpu_grads.py::_compare, tests/test_gpu_ray_ops.py::_judge). The float32
models: the k-ordered chain dw_ops.fma_chain_f32 for the GEMMs (bf16 operands: the same chain on the bf16 values), a sequential
float32 sum for finalize, the same model in float32 for weight norm, torch.optim.Adam in float32 on the CPU for Adam. The
hyper-parameters of Adam are C floats: both models get the float32 values (beta2 = float32(0.999), ...), as the kernel does.
Adam's second moment is judged in two groups: g = 1e-20, whose g^2 (1 - beta2) is a subnormal with seven significant bits (floor:
85 units of 2^-24 g^2), and everything else (floor below 1 unit).

Every (case, tensor) whose bound exceeded 1 unit is printed (pytest -rA). On the MI355X:

gemm_f32/mat300/random         slab0       bound  10.97 units (fp32 floor  3.657)  kernel error  3.657
gemm_f32/mat300/random         colsum0     bound   5.74 units (fp32 floor  1.914)  kernel error  1.003
gemm_f32/mat300/random         slab1       bound   9.19 units (fp32 floor  3.062)  kernel error  1.619
gemm_f32/mat300/random         colsum1     bound   5.73 units (fp32 floor  1.910)  kernel error  0.648
gemm_bf16/mat300/random        slab0       bound   5.67 units (fp32 floor  1.889)  kernel error  1.440
gemm_bf16/mat300/random        slab1       bound   5.16 units (fp32 floor  1.719)  kernel error  0.630
gemm_f32/rows5000/random       slab0       bound  10.88 units (fp32 floor  3.626)  kernel error  2.284
gemm_f32/rows5000/random       colsum0     bound   3.99 units (fp32 floor  1.330)  kernel error  0.806
gemm_f32/rows5000/random       slab1       bound  13.17 units (fp32 floor  4.390)  kernel error  1.556
gemm_f32/rows5000/random       colsum1     bound   3.26 units (fp32 floor  1.085)  kernel error  0.422
gemm_f32/rows5000/random       slab2       bound  13.20 units (fp32 floor  4.401)  kernel error  1.432
gemm_f32/rows5000/random       colsum2     bound   2.47 units (fp32 floor  0.822)  kernel error  0.378
gemm_bf16/rows5000/random      slab0       bound   9.08 units (fp32 floor  3.026)  kernel error  0.857
gemm_bf16/rows5000/random      slab1       bound   7.73 units (fp32 floor  2.578)  kernel error  0.508
gemm_bf16/rows5000/random      slab2       bound  10.27 units (fp32 floor  3.422)  kernel error  0.613
gemm_f32/p1/random             slab0       bound   2.97 units (fp32 floor  0.991)  kernel error  0.991
gemm_f32/p1/random             slab1       bound   4.68 units (fp32 floor  1.559)  kernel error  0.942
gemm_bf16/p1/random            slab1       bound   2.56 units (fp32 floor  0.852)  kernel error  0.000
gemm_f32/p40/random            slab0       bound   9.74 units (fp32 floor  3.246)  kernel error  2.565
gemm_f32/p40/random            colsum0     bound   5.43 units (fp32 floor  1.809)  kernel error  0.743
gemm_f32/p40/random            slab1       bound   8.36 units (fp32 floor  2.787)  kernel error  1.308
gemm_f32/p40/random            colsum2     bound   1.60 units (fp32 floor  0.535)  kernel error  0.467
gemm_bf16/p40/random           slab0       bound   3.58 units (fp32 floor  1.194)  kernel error  1.041
gemm_bf16/p40/random           slab1       bound   3.66 units (fp32 floor  1.219)  kernel error  0.552
gemm_f32/rounds/random         slab0       bound   8.49 units (fp32 floor  2.831)  kernel error  0.579
gemm_f32/rounds/random         colsum0     bound   2.85 units (fp32 floor  0.949)  kernel error  0.211
gemm_f32/rounds/random         slab1       bound   8.27 units (fp32 floor  2.758)  kernel error  0.527
gemm_f32/rounds/random         colsum1     bound   4.08 units (fp32 floor  1.359)  kernel error  0.190
gemm_f32/rounds/random         slab2       bound  13.00 units (fp32 floor  4.332)  kernel error  0.423
gemm_f32/rounds/random         colsum2     bound   4.70 units (fp32 floor  1.568)  kernel error  0.242
gemm_f32/rounds/random         colsum3     bound   2.69 units (fp32 floor  0.895)  kernel error  0.159
gemm_bf16/rounds/random        slab0       bound   5.21 units (fp32 floor  1.736)  kernel error  0.310
gemm_bf16/rounds/random        slab1       bound   4.25 units (fp32 floor  1.415)  kernel error  0.154
gemm_bf16/rounds/random        slab2       bound   4.75 units (fp32 floor  1.582)  kernel error  0.171
gemm_f32/wide/random           slab0       bound  12.03 units (fp32 floor  4.009)  kernel error  1.933
gemm_f32/wide/random           colsum0     bound   5.11 units (fp32 floor  1.703)  kernel error  0.533
gemm_bf16/wide/random          slab0       bound   7.59 units (fp32 floor  2.531)  kernel error  0.721
gemm_f32/slice/random          slab0       bound  13.21 units (fp32 floor  4.402)  kernel error  2.098
gemm_f32/slice/random          colsum0     bound   3.43 units (fp32 floor  1.142)  kernel error  0.454
gemm_f32/slice/random          slab1       bound  10.30 units (fp32 floor  3.432)  kernel error  3.432
gemm_f32/slice/random          colsum1     bound   2.35 units (fp32 floor  0.782)  kernel error  0.677
finalize/shapes/random         t0          bound   2.76 units (fp32 floor  0.920)  kernel error  0.920
finalize/shapes/random         b0          bound   1.87 units (fp32 floor  0.623)  kernel error  0.623
finalize/shapes/random         t1          bound   9.13 units (fp32 floor  3.042)  kernel error  2.633
finalize/shapes/random         b1          bound   5.88 units (fp32 floor  1.960)  kernel error  1.311
finalize/shapes/random         t2          bound   9.33 units (fp32 floor  3.111)  kernel error  2.098
finalize/shapes/random         b2          bound   4.61 units (fp32 floor  1.537)  kernel error  1.060
finalize/shapes/random         t3          bound  10.41 units (fp32 floor  3.471)  kernel error  2.572
finalize/shapes/random         b3          bound   5.46 units (fp32 floor  1.821)  kernel error  1.821
finalize/shapes/random         b4          bound   5.45 units (fp32 floor  1.817)  kernel error  1.091
finalize/shapes/random         var         bound   3.18 units (fp32 floor  1.060)  kernel error  0.004
finalize/shapes/random         t5          bound   7.15 units (fp32 floor  2.384)  kernel error  1.535
finalize/pair_xsum/random      w4          bound   8.98 units (fp32 floor  2.994)  kernel error  2.551
finalize/pair_xsum/random      b4          bound   4.53 units (fp32 floor  1.510)  kernel error  1.395
finalize/pair_xsum/random      w8          bound   9.57 units (fp32 floor  3.189)  kernel error  2.510
finalize/pair_xsum/random      b8          bound   5.67 units (fp32 floor  1.891)  kernel error  1.716
finalize/pair_xsum/random      w9          bound   3.32 units (fp32 floor  1.108)  kernel error  0.983
finalize/phases/random         s0          bound   6.14 units (fp32 floor  2.046)  kernel error  2.061
finalize/phases/random         c0          bound   4.50 units (fp32 floor  1.501)  kernel error  1.044
finalize/phases/random         s1          bound   9.15 units (fp32 floor  3.048)  kernel error  2.353
finalize/phases/random         a0          bound   4.65 units (fp32 floor  1.551)  kernel error  1.242
finalize/phases/random         d0          bound   1.40 units (fp32 floor  0.465)  kernel error  0.465
finalize/phases/random         a1          bound   4.17 units (fp32 floor  1.392)  kernel error  1.506
weightnorm/tall_last/3x3       w           bound   2.71 units (fp32 floor  0.902)  kernel error  1.799
weightnorm/tall_last/3x3       inv_norm    bound   3.15 units (fp32 floor  1.050)  kernel error  1.050
weightnorm/tall_last/4x39      w           bound   6.75 units (fp32 floor  2.250)  kernel error  1.420
weightnorm/tall_last/4x39      inv_norm    bound   3.45 units (fp32 floor  1.151)  kernel error  1.067
weightnorm/tall_last/5x64      w           bound   7.36 units (fp32 floor  2.454)  kernel error  1.974
weightnorm/tall_last/5x64      inv_norm    bound   4.85 units (fp32 floor  1.615)  kernel error  1.116
weightnorm/tall_last/257x65    w           bound   8.74 units (fp32 floor  2.912)  kernel error  3.102
weightnorm/tall_last/257x65    inv_norm    bound   6.33 units (fp32 floor  2.110)  kernel error  1.692
weightnorm/tall_last/3x256     w           bound   8.04 units (fp32 floor  2.682)  kernel error  1.562
weightnorm/tall_last/3x256     inv_norm    bound   2.94 units (fp32 floor  0.978)  kernel error  0.978
weightnorm/tall_last/5x352     w           bound   6.99 units (fp32 floor  2.329)  kernel error  2.012
weightnorm/tall_first/257x1    w           bound   5.42 units (fp32 floor  1.805)  kernel error  1.950
weightnorm/tall_first/257x1    inv_norm    bound   2.69 units (fp32 floor  0.897)  kernel error  0.897
weightnorm/tall_first/5x3      w           bound   4.67 units (fp32 floor  1.556)  kernel error  2.808
weightnorm/tall_first/5x3      inv_norm    bound   2.15 units (fp32 floor  0.718)  kernel error  1.807
weightnorm/tall_first/1x39     w           bound   5.78 units (fp32 floor  1.926)  kernel error  1.525
weightnorm/tall_first/1x39     inv_norm    bound   2.55 units (fp32 floor  0.851)  kernel error  1.112
weightnorm/tall_first/4x64     w           bound   5.47 units (fp32 floor  1.823)  kernel error  1.672
weightnorm/tall_first/4x64     inv_norm    bound   1.52 units (fp32 floor  0.506)  kernel error  0.739
weightnorm/tall_first/3x65     w           bound   5.83 units (fp32 floor  1.944)  kernel error  2.149
weightnorm/tall_first/3x65     inv_norm    bound   3.98 units (fp32 floor  1.325)  kernel error  1.325
weightnorm/tall_first/257x256  w           bound  10.23 units (fp32 floor  3.410)  kernel error  3.273
weightnorm/tall_first/257x256  inv_norm    bound   5.58 units (fp32 floor  1.859)  kernel error  1.934
weightnorm/tall_first/4x352    w           bound   7.21 units (fp32 floor  2.405)  kernel error  1.744
weightnorm_bwd/tall_last/1x1   dg          bound   3.50 units (fp32 floor  1.166)  kernel error  0.000
weightnorm_bwd/tall_last/3x3   dg          bound   2.21 units (fp32 floor  0.736)  kernel error  0.327
weightnorm_bwd/tall_last/3x3   dv          bound   8.05 units (fp32 floor  2.682)  kernel error  1.398
weightnorm_bwd/tall_last/4x39  dg          bound   2.13 units (fp32 floor  0.711)  kernel error  0.315
weightnorm_bwd/tall_last/4x39  dv          bound   9.20 units (fp32 floor  3.066)  kernel error  2.424
weightnorm_bwd/tall_last/5x64  dg          bound   1.06 units (fp32 floor  0.354)  kernel error  0.350
weightnorm_bwd/tall_last/5x64  dv          bound  18.09 units (fp32 floor  6.029)  kernel error  9.418
weightnorm_bwd/tall_last/257x65 dg          bound   2.99 units (fp32 floor  0.996)  kernel error  0.887
weightnorm_bwd/tall_last/257x65 dv          bound 117.82 units (fp32 floor 39.272)  kernel error 18.478
weightnorm_bwd/tall_last/3x256 dg          bound   1.39 units (fp32 floor  0.465)  kernel error  0.172
weightnorm_bwd/tall_last/3x256 dv          bound  15.93 units (fp32 floor  5.311)  kernel error  2.881
weightnorm_bwd/tall_last/5x352 dv          bound  27.34 units (fp32 floor  9.112)  kernel error  6.060
weightnorm_bwd/tall_first/257x1 dg          bound   5.59 units (fp32 floor  1.863)  kernel error  1.979
weightnorm_bwd/tall_first/257x1 dv          bound   5.73 units (fp32 floor  1.909)  kernel error  1.622
weightnorm_bwd/tall_first/5x3  dg          bound   3.69 units (fp32 floor  1.231)  kernel error  1.009
weightnorm_bwd/tall_first/5x3  dv          bound   4.56 units (fp32 floor  1.520)  kernel error  1.673
weightnorm_bwd/tall_first/1x39 dv          bound   7.25 units (fp32 floor  2.416)  kernel error  1.772
weightnorm_bwd/tall_first/4x64 dv          bound   9.38 units (fp32 floor  3.127)  kernel error  2.366
weightnorm_bwd/tall_first/3x65 dg          bound   1.73 units (fp32 floor  0.577)  kernel error  0.158
weightnorm_bwd/tall_first/3x65 dv          bound  50.07 units (fp32 floor 16.690)  kernel error  1.946
weightnorm_bwd/tall_first/257x256 dg          bound   1.64 units (fp32 floor  0.546)  kernel error  0.582
weightnorm_bwd/tall_first/257x256 dv          bound  91.90 units (fp32 floor 30.634)  kernel error 33.396
weightnorm_bwd/tall_first/4x352 dv          bound  12.91 units (fp32 floor  4.304)  kernel error  6.191
adam/n255_begin7               p           bound   2.62 units (fp32 floor  0.872)  kernel error  0.872
adam/n255_begin7               m           bound   2.02 units (fp32 floor  0.674)  kernel error  0.908
adam/n255_begin7               v           bound   4.13 units (fp32 floor  1.377)  kernel error  1.377
adam/n255_begin7               v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
adam/n256_gap                  p           bound   2.76 units (fp32 floor  0.919)  kernel error  0.919
adam/n256_gap                  m           bound   2.59 units (fp32 floor  0.862)  kernel error  0.862
adam/n256_gap                  v           bound   5.34 units (fp32 floor  1.781)  kernel error  1.781
adam/n256_gap                  v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
adam/n257_empty2nd             p           bound   4.25 units (fp32 floor  1.416)  kernel error  1.285
adam/n257_empty2nd             v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
adam/n257_step2                p           bound   2.85 units (fp32 floor  0.951)  kernel error  0.951
adam/n257_step2                m           bound   2.19 units (fp32 floor  0.731)  kernel error  0.766
adam/n257_step2                v           bound   4.12 units (fp32 floor  1.372)  kernel error  1.372
adam/n257_step2                v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
adam/wrap_gap                  p           bound   9.83 units (fp32 floor  3.276)  kernel error  4.481
adam/wrap_gap                  m           bound   2.82 units (fp32 floor  0.942)  kernel error  1.021
adam/wrap_gap                  v           bound   5.73 units (fp32 floor  1.909)  kernel error  1.909
adam/wrap_gap                  v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
adam/wrap_single               p           bound  26.47 units (fp32 floor  8.823)  kernel error  3.906
adam/wrap_single               m           bound   2.81 units (fp32 floor  0.937)  kernel error  1.014
adam/wrap_single               v           bound   5.76 units (fp32 floor  1.919)  kernel error  1.919
adam/wrap_single               v(g=1e-20)  bound 254.94 units (fp32 floor 84.979)  kernel error 84.979
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dw_cases, dw_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024                     # NaN elements in front of and behind every output buffer: more than the longest target row


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


class Bufs:
    """Device buffers of one launch: inputs, and pre-filled outputs between NaN guard bands."""

    def __init__(self):
        self.keep, self.outs = [], {}

    def inp(self, a, dtype=torch.float32):
        t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def dev(self, t):
        t = t.to(DEV).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def out(self, name, n, prefill=None):
        base = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
        pre = np.full(n, np.nan, np.float32) if prefill is None else np.ascontiguousarray(prefill, np.float32)
        assert pre.shape == (n,)
        base[GUARD:GUARD + n] = torch.from_numpy(pre).to(DEV)
        self.outs[name] = (base, n, _bits(pre).copy())
        return base[GUARD:].data_ptr()

    def get(self, name):
        """-> (float32 numpy copy, pre-fill bits), after checking the guard bands."""
        torch.cuda.synchronize()
        base, n, pre = self.outs[name]
        host = base.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + n:]).all(), "guard band of %s was written" % name
        return host[GUARD:GUARD + n], pre

    def check(self, name, want64, exact, judge=None):
        """want64: float64, NaN where the launch must not write. Written elements finite and compared (bit for bit when `exact`,
        else judge(got, mask)); the others bit-identical to the pre-fill. -> the float32 result."""
        got, pre = self.get(name)
        w = ~np.isnan(want64)
        assert np.array_equal(_bits(got)[~w], pre[~w]), "%s: an element outside the written set changed" % name
        assert np.isfinite(got[w]).all(), "%s has unwritten or non-finite elements" % name
        if exact:
            want = torch.from_numpy(want64[w]).to(torch.float32)
            assert torch.equal(torch.from_numpy(got[w].copy()), want), "%s differs from the float64 model" % name
        elif judge is not None:
            judge(got, w)
        return got

    def unchanged(self, name, bits=None):
        got, pre = self.get(name)
        assert np.array_equal(_bits(got), pre if bits is None else bits), "%s was written" % name


def _status(fn, *args):
    from vdn_hip import lib
    return int(getattr(lib.load(), fn)(*args))


def _call(fn, *args):
    rc = _status(fn, *args)
    assert rc == 0, "%s returned %d" % (fn, rc)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _table(b, arr):
    return ctypes.c_void_p(b.dev(torch.from_numpy(arr.view(np.uint8).copy())))


def _judge(case, tensor, got, ref64, ref32, unit, rows):
    """Assert `got` within max(1, 3 x float32 floor) units of ref64."""
    floor = dw_ops.units_err(ref32, ref64, unit)
    err = dw_ops.units_err(got, ref64, unit)
    bound = max(1.0, 3.0 * floor)
    if bound > 1.0:
        rows.append("%-28s %-12s bound %6.2f units (fp32 floor %6.3f)  kernel error %6.3f" % (case, tensor, bound, floor, err))
    assert err <= bound, "%s %s: kernel error %.3f units > bound %.2f (fp32 floor %.3f)" % (case, tensor, err, bound, floor)


def _report(rows):
    if rows:
        print("(case, tensor) pairs whose bound exceeded 1 unit:\n" + "\n".join(rows))


# ---- weight-gradient GEMMs ----------------------------------------------------------------------------------------------------

def _plane(b, case, x, sliced):
    """Device plane of operand x [P, cols] -> (pointer, ld). Rows the kernel must not contract over hold NaN: [rows, P), and a
    few more behind P; the bf16 layout's padding up to a multiple of 32 rows holds 3.0e38."""
    from vdn_hip import layout
    P, rows = case["P"], case["rows"]
    if case["precision"] == "bf16":
        full = torch.full((layout.pad32(P), x.shape[1]), 3.0e38)
        full[:P] = torch.from_numpy(x)
        full[rows:P] = float("nan")
        return b.dev(layout.to_pt32(full)), x.shape[1]
    ld, c0 = (288, 256) if sliced else (x.shape[1], 0)
    full = torch.full((P + 5, ld), float("nan"))          # (a slice: every other column of the wider plane is NaN too)
    full[:rows, c0:c0 + x.shape[1]] = torch.from_numpy(x[:rows])
    return b.dev(full) + 4 * c0, ld


@pytest.mark.parametrize("name,kind,precision", dw_cases.gemm_case_ids())
def test_dw_gemm_vs_float64_model(name, kind, precision):
    from vdn_hip import lib
    case, ref = dw_cases.gemm_reference(name, kind, precision)
    sfx = "_f32" if precision == "fp32" else "_bf16"
    label = "gemm%s/%s/%s" % (sfx, name, kind)
    b = Bufs()
    pdev = None if case["P_dev"] is None else b.inp(np.asarray([case["P_dev"]], np.int32), torch.int32)
    dw = np.zeros(len(case["entries"]), dtype=lib.struct_dtype("VdnDwDesc"))
    wg = 0
    for i, e in enumerate(case["entries"]):
        d = dw[i]
        for s, (a, bm) in enumerate(e["segs"]):
            d["A%d" % (s + 1)], d["lda%d" % (s + 1)] = _plane(b, case, a, e["slice"])
            if bm is not None:
                d["B%d" % (s + 1)], d["ldb%d" % (s + 1)] = _plane(b, case, bm, False)
        d["P"], d["m_tiles"], d["n_tiles"], d["splits"], d["wg_begin"] = case["P"], e["M"] // 32, e["N"] // 32, e["splits"], wg
        d["slab"] = b.out("slab%d" % i, e["splits"] * e["M"] * e["N"])
        d["colsum"] = b.out("colsum%d" % i, e["splits"] * e["M"]) if e["colsum"] else 0
        if pdev is not None:
            d["P_dev"] = pdev
        wg += lib.call_value("vdn_dw_entry_wgs" + sfx, e["M"] // 32, e["N"] // 32, e["splits"])
    _call("vdn_dw_gemm" + sfx, _table(b, dw), len(dw), wg, _stream())
    rows = []
    for i, (e, r) in enumerate(zip(case["entries"], ref)):
        M, N, splits = e["M"], e["N"], e["splits"]
        empty = np.array([k1 <= k0 for _, k0, k1 in r["ranges"]])
        seg2 = np.array([s == 1 for s, _, _ in r["ranges"]])
        slab, _ = b.get("slab%d" % i)
        assert np.isfinite(slab).all(), "entry %d: slab has unwritten or non-finite elements" % i
        slab = slab.reshape(splits, M, N).astype(np.float64)
        assert not slab[empty].any(), "entry %d: a split without rows is not exactly 0" % i
        if N:
            total = slab.sum(0)
            if kind == "exact":
                assert torch.equal(torch.from_numpy(total).float(), torch.from_numpy(r["prod"]).float()), "entry %d: slab" % i
                # which slab is which segment: the first half of the splits holds segment 1 alone
                first, _ = dw_ops.dw_gemm(e["segs"][:1], case["rows"])
                assert np.array_equal(slab[~seg2].sum(0), first), "entry %d: segment 1 is not in the first half of the splits" % i
            else:
                _judge(label, "slab%d" % i, total, r["prod"], r["chain_prod"], r["u_prod"], rows)
        if e["colsum"]:
            cs, _ = b.get("colsum%d" % i)
            assert np.isfinite(cs).all(), "entry %d: colsum has unwritten or non-finite elements" % i
            cs = cs.reshape(splits, M).astype(np.float64)
            assert not cs[empty | seg2].any(), "entry %d: colsum of a split without rows of segment 1 is not exactly 0" % i
            if kind == "exact":
                assert torch.equal(torch.from_numpy(cs.sum(0)).float(), torch.from_numpy(r["cs"]).float()), "entry %d: colsum" % i
            else:
                _judge(label, "colsum%d" % i, cs.sum(0), r["cs"], r["chain_cs"], r["u_cs"], rows)
    _report(rows)


# ---- finalize -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", dw_cases.finalize_case_ids())
def test_dw_finalize_vs_float64_model(name, kind):
    from vdn_hip import lib
    case = dw_cases.finalize_case(name, kind)
    a0, a1, units = dw_cases.finalize_reference(case)
    f0, f1, _ = dw_cases.finalize_reference(case, np.float32)
    b = Bufs()
    tptr = {k: b.out(k, len(v), v) for k, v in case["targets"].items()}
    fin = np.zeros(len(case["descs"]), dtype=lib.struct_dtype("VdnDwFinalizeDesc"))
    for f, d in zip(fin, case["descs"]):
        f["slab"], f["colsum"] = b.inp(d["slab"]), b.inp(d["colsum"])
        f["rmap"] = b.inp(d["rmap"], torch.int32)
        f["cmap"] = 0 if d["cmap"] is None else b.inp(d["cmap"], torch.int32)
        f["target"] = 0 if d["tgt"] is None else tptr[d["tgt"]]
        f["btarget"] = 0 if d["bt"] is None else tptr[d["bt"]]
        f["t_stride"], f["splits"], f["M"], f["N"], f["accumulate"] = d["t_stride"], d["splits"], d["M"], d["N"], d["accumulate"]
        f["scale"], f["bscale"] = d["scale"], d["bscale"]
        if d["xsum"] is not None:
            f["xsum"], f["xscale"] = b.inp(d["xsum"]), d["xscale"]
            f["xsplits"], f["xM"], f["xrow"] = d["xsum"].shape[0], d["xsum"].shape[1], d["xrow"]
    table = _table(b, fin)
    accumulating = {k for d in case["descs"] if d["accumulate"] for k in (d["tgt"], d["bt"]) if k is not None}
    rows, after0 = [], {}
    for phase, want, f32 in ((0, a0, f0), (1, a1, f1)):
        if phase and not accumulating:
            break
        _call("vdn_dw_finalize", table, len(fin), case["max_M"], phase, _stream())
        for k in case["targets"]:
            if (k in accumulating) != bool(phase):
                # phase 0 leaves the '+=' targets at their pre-fill, phase 1 the '=' targets at what phase 0 wrote: bit for bit
                b.unchanged(k, after0.get(k))
                continue
            judge = lambda got, w, k=k: _judge("finalize/%s/%s" % (name, kind), k, got[w], want[k][w], f32[k][w], units[k][w], rows)
            after0[k] = _bits(b.check(k, want[k], kind == "exact", judge)).copy()
    _report(rows)


# ---- weight norm --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(dw_cases.WEIGHTNORM))
def test_weightnorm_materialize_vs_float64_model(name):
    from vdn_hip import lib
    descs = dw_cases.weightnorm_case(name)
    b = Bufs()
    tab = np.zeros(len(descs), dtype=lib.struct_dtype("VdnWeightNormDesc"))
    last_normed = max(i for i, d in enumerate(descs) if d["normed"])
    for i, (t, d) in enumerate(zip(tab, descs)):
        t["g"] = b.inp(d["g"]) if d["normed"] else 0
        t["v"], t["rows"], t["cols"] = b.inp(d["v"]), d["rows"], d["cols"]
        t["w_eff"] = b.out("w%d" % i, d["rows"] * d["cols"])
        t["inv_norm"] = 0 if i == last_normed else b.out("inv%d" % i, d["rows"])          # (NULL is allowed)
    _call("vdn_weightnorm_materialize", _table(b, tab), len(tab), max(d["rows"] for d in descs), _stream())
    rows = []
    for i, d in enumerate(descs):
        label = "weightnorm/%s/%dx%d" % (name, d["rows"], d["cols"])
        if not d["normed"]:                          # the copy path: w = v bit for bit, inv_norm is not written
            b.check("w%d" % i, d["v"].ravel().astype(np.float64), True)
            b.unchanged("inv%d" % i)
            continue
        g, v = torch.from_numpy(d["g"]), torch.from_numpy(d["v"])
        w64, inv64 = (x.numpy() for x in dw_ops.weightnorm(g.double(), v.double()))
        w32, inv32 = (x.numpy() for x in dw_ops.weightnorm(g, v))
        uw = dw_ops.weightnorm_units(d["g"], d["v"], d["dw"])[0]
        b.check("w%d" % i, w64.ravel(), False, lambda got, w: _judge(label, "w", got, w64.ravel(), w32.ravel(), uw.ravel(), rows))
        if i != last_normed:
            b.check("inv%d" % i, inv64, False, lambda got, w: _judge(label, "inv_norm", got, inv64, inv32, dw_ops.ULP * inv64, rows))
    _report(rows)


@pytest.mark.parametrize("name", list(dw_cases.WEIGHTNORM))
def test_weightnorm_bwd_vs_float64_autograd(name):
    from vdn_hip import lib
    descs = [d for d in dw_cases.weightnorm_case(name) if d["normed"]]
    b = Bufs()
    tab = np.zeros(len(descs), dtype=lib.struct_dtype("VdnWeightNormBwdDesc"))
    for i, (t, d) in enumerate(zip(tab, descs)):
        inv64 = dw_ops.weightnorm(torch.from_numpy(d["g"]).double(), torch.from_numpy(d["v"]).double())[1].numpy()
        t["g"], t["v"], t["inv_norm"], t["dw_eff"] = b.inp(d["g"]), b.inp(d["v"]), b.inp(inv64), b.inp(d["dw"])
        t["dg"], t["dv"] = b.out("dg%d" % i, d["rows"]), b.out("dv%d" % i, d["rows"] * d["cols"])
        t["rows"], t["cols"] = d["rows"], d["cols"]
    _call("vdn_weightnorm_bwd", _table(b, tab), len(tab), max(d["rows"] for d in descs), _stream())
    rows = []
    for i, d in enumerate(descs):
        label = "weightnorm_bwd/%s/%dx%d" % (name, d["rows"], d["cols"])
        dg64, dv64 = (x.numpy() for x in dw_ops.weightnorm_bwd(d["g"], d["v"], d["dw"]))
        dg32, dv32 = (x.numpy() for x in dw_ops.weightnorm_bwd(d["g"], d["v"], d["dw"], torch.float32))
        _, udg, udv = dw_ops.weightnorm_units(d["g"], d["v"], d["dw"])
        b.check("dg%d" % i, dg64, False, lambda got, w: _judge(label, "dg", got, dg64, dg32, udg, rows))
        b.check("dv%d" % i, dv64.ravel(), False, lambda got, w: _judge(label, "dv", got, dv64.ravel(), dv32.ravel(), udv.ravel(), rows))
    _report(rows)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------

def _adam_launch(b, c, ranges, step, single, tag=""):
    h = dw_cases.adam_hyper()
    ptr = lambda k: ctypes.c_void_p(b.out(k + tag, c["size"], c[k]))
    p, m, v = ptr("p"), ptr("m"), ptr("v")
    g = ctypes.c_void_p(b.inp(c["g"]))
    tail = (h["lr"], h["betas"][0], h["betas"][1], h["eps"], step, _stream())
    if single:
        assert ranges[0][0] == 0 and ranges[1] == (0, 0)
        return _status("vdn_adam_step", p, g, m, v, ranges[0][1], *tail)
    return _status("vdn_adam_step_ranges", p, g, m, v, ranges[0][0], ranges[0][1], ranges[1][0], ranges[1][1], *tail)


@pytest.mark.parametrize("name", list(dw_cases.ADAM))
def test_adam_vs_float64_model(name):
    c, ref, f32, units = dw_cases.adam_reference(name)
    b = Bufs()
    assert _adam_launch(b, c, c["ranges"], c["step"], c["single"]) == 0
    sel = c["sel"]
    tiny = c["g"][sel] == np.float32(1e-20)
    rows = []
    for k, r64, r32, u in zip("pmv", ref, f32, units):
        want = np.full(c["size"], np.nan)
        want[sel] = r64
        # everything outside the two ranges - the gap between them included - is bit-identical to its pre-fill
        got = b.check(k, want, False)[sel]
        groups = [("v", ~tiny), ("v(g=1e-20)", tiny)] if k == "v" else [(k, np.ones(len(sel), bool))]
        for tensor, mask in groups:
            if mask.any():
                _judge("adam/" + name, tensor, got[mask], r64[mask], r32[mask], u[mask], rows)
    zero = (c["g"][sel] == 0) & (c["m"][sel] == 0) & (c["v"][sel] == 0)          # nothing to move: the parameter stays bit for bit
    assert np.array_equal(_bits(b.get("p")[0][sel][zero]), _bits(c["p"][sel][zero]))
    _report(rows)


@pytest.mark.parametrize("name", list(dw_cases.ADAM_ERRORS))
def test_adam_argument_errors_write_nothing(name):
    b0, e0, b1, e1, step = dw_cases.ADAM_ERRORS[name]
    rs = np.random.RandomState(3)
    c = dict(size=64, **{k: rs.standard_normal(64).astype(np.float32) for k in "pgmv"})
    c["v"] = np.abs(c["v"])
    b = Bufs()
    assert _adam_launch(b, c, [(b0, e0), (b1, e1)], step, False) == -1
    if name == "step0":
        assert _adam_launch(b, c, [(0, 64), (0, 0)], step, True, "/single") == -1
    for k in b.outs:
        b.unchanged(k)
