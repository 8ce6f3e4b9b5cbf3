"""Constructed inputs for the parameter-update tail (tests/test_dw_ops_model_cpu.py, tests/test_gpu_dw_tail.py): weight-gradient
GEMMs, finalize, weight norm and Adam. Every case is deterministic from its name (crc32 seeding, as oracle/ray_cases.py).

Two kinds of value:
  exact   small integers (|x| <= 8: exact in bf16) and power-of-two scales. Every product and every partial sum, in any order,
          is an integer below 64 x 8269 x 2 < 2^24 times a power of two: exact in float32. A kernel must equal the float64 model
          bit for bit whatever its accumulation order or the matrix core's internal width; one wrong, missing or doubled row
          shows at zero tolerance.
  random  normal values, judged in the units of oracle/dw_ops.py against the float32 floor.
"""
import functools
import zlib

import numpy as np
import torch

from . import dw_ops

KINDS = ("exact", "random")


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _values(rs, kind, shape, bf16=False):
    if kind == "exact":
        return rs.randint(-8, 9, size=shape).astype(np.float32)
    x = rs.standard_normal(shape).astype(np.float32)
    if bf16:                                   # the bf16 kernel's operands: the case holds the values the plane will hold
        x = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    return x


# ---- weight-gradient GEMM ---------------------------------------------------------------------------------------------------
# name -> (P, P_dev, [(m_cols, n_cols, two_segments, splits[, options])], kinds, precisions)
# options: "nocs" = colsum NULL; "slice" = A is columns [256, 288) of a [P, 288] plane (fp32 only: alpha_linear of nerf_dw_entries)
_BOTH = ("fp32", "bf16")
GEMM = {
    # the matrix of tests/test_gpu_dw_gemm.py
    "mat4096": (4096, None, [(256, 256, False, 1)], ("exact",), _BOTH),
    "mat5000": (5000, None, [(256, 256, True, 4), (256, 64, False, 2), (32, 256, False, 2), (288, 256, False, 2)], ("exact",), _BOTH),
    "mat8269": (8269, 6013, [(256, 256, True, 6), (128, 288, False, 3), (256, 0, False, 3), (96, 128, False, 3)], ("exact",), _BOTH),
    "mat300": (300, 31, [(256, 256, False, 2), (64, 96, True, 2)], KINDS, _BOTH),
    # random values at the largest row count the chained floor model affords
    "rows5000": (5000, None, [(256, 64, False, 2), (32, 256, True, 4), (96, 128, False, 3)], ("random",), _BOTH),
    # an empty work list, a single row, splits without rows (P = 40 is two fp32 stages, one bf16 stage: 4 resp. 5 of 6 empty)
    "pdev0": (300, 0, [(64, 96, True, 2), (32, 0, False, 3), (96, 64, False, 9)], ("exact",), _BOTH),
    "p1": (1, None, [(64, 64, False, 1), (32, 96, True, 2)], KINDS, _BOTH),
    "p40": (40, None, [(96, 64, False, 6), (64, 32, True, 6, "nocs"), (32, 0, False, 6)], KINDS, _BOTH),
    # split counts across the 8-slot rounds of the fp32 id space
    "rounds": (1500, 1403, [(32, 64, False, 9), (64, 32, False, 17), (64, 64, True, 18), (32, 0, False, 17)], KINDS, _BOTH),
    # the widest output: 9 x 11 tiles, partial last tile groups (3 x 3 of 128 in fp32, 2 x 2 of 256 in bf16)
    "wide": (700, None, [(288, 352, False, 3)], KINDS, _BOTH),
    "slice": (1000, 997, [(32, 256, False, 2, "slice"), (32, 32, False, 1)], KINDS, ("fp32",)),
}


def gemm_case_ids():
    """[(name, kind, precision)]"""
    return [(n, k, p) for n, (_, _, _, kinds, precs) in GEMM.items() for k in kinds for p in precs]


def gemm_case(name, kind, precision):
    """-> dict(P, P_dev, rows, stage, entries): entries = [dict(M, N, two, splits, colsum, slice, segs=[(A [P,M], B [P,N] | None)])],
    float32 arrays holding the values the planes hold (bf16-representable for the bf16 kernel); rows = min(P, P_dev)."""
    P, P_dev, ents, kinds, precs = GEMM[name]
    assert kind in kinds and precision in precs
    # (exact values are bf16-representable as they are: both precisions share them)
    rs = _rng("gemm/%s/%s" % (name, kind) if kind == "exact" else "gemm/%s/%s/%s" % (name, kind, precision))
    entries = []
    for e in ents:
        M, N, two, splits = e[:4]
        opts = e[4:]
        segs = [(_values(rs, kind, (P, M), precision == "bf16"), _values(rs, kind, (P, N), precision == "bf16") if N else None)
                for _ in range(2 if two else 1)]
        entries.append(dict(M=M, N=N, two=two, splits=splits, colsum="nocs" not in opts, slice="slice" in opts, segs=segs))
    rows = P if P_dev is None else min(P, P_dev)
    return dict(name=name, kind=kind, precision=precision, P=P, P_dev=P_dev, rows=rows, entries=entries,
                stage=dw_ops.F32_STAGE if precision == "fp32" else dw_ops.BF16_STAGE)


@functools.lru_cache(maxsize=4)
def gemm_reference(name, kind, precision):
    """-> (case, [per entry dict(prod, cs: float64 model; u_prod, u_cs: units; ranges: split_ranges; random cases only: chain_prod,
    chain_cs: the float32 chain model, floor_prod, floor_cs: its error in units)]). Computed once and shared; nobody writes into it."""
    case = gemm_case(name, kind, precision)
    out = []
    for e in case["entries"]:
        prod, cs = dw_ops.dw_gemm(e["segs"], case["rows"])
        u_prod, u_cs = dw_ops.dw_gemm_units(e["segs"], case["rows"])
        r = dict(prod=prod, cs=cs, u_prod=u_prod, u_cs=u_cs, ranges=dw_ops.split_ranges(case["rows"], e["splits"], e["two"], case["stage"]))
        if kind == "random":
            c_prod, c_cs = dw_ops.dw_gemm_chain_f32(e["segs"], case["rows"])
            r["chain_prod"], r["chain_cs"] = c_prod, c_cs
            r["floor_prod"] = 0.0 if prod is None else dw_ops.units_err(c_prod, prod, u_prod)
            r["floor_cs"] = dw_ops.units_err(c_cs, cs, u_cs)
        out.append(r)
    return case, out


# ---- finalize -----------------------------------------------------------------------------------------------------------------
# A case is one descriptor table launched as phase 0, then phase 1. A descriptor spec:
#   dict(splits, M, N, rmap, cmap, acc, tgt (name of the target buffer or None), t_stride, t_rows, bt (name or None), bt_rows,
#        x = (xsplits, xM, xrow) or None)
# Targets are named buffers: two descriptors may write disjoint column ranges of one.

def _maps():
    from vdn_hip import images
    m = {n: (np.asarray(km, np.int32), np.asarray(nm, np.int32)) for n, km, nm, _ in images.sdf_layer_maps()}
    rs = _rng("finalize/maps")
    holes = np.full(352, -1, np.int32)                   # 323 of 352 image columns in a scrambled order, the rest -1
    holes[np.sort(rs.permutation(352)[:323])] = rs.permutation(323)
    perm224 = rs.permutation(224).astype(np.int32)
    perm256 = rs.permutation(256).astype(np.int32)
    return dict(id3_32=images.ident_map(3, 32), id32=images.ident_map(32), id84_96=images.ident_map(84, 96), id96=images.ident_map(96),
                id256=images.ident_map(256), id1=np.zeros(1, np.int32), lin8_rows=m["lin8"][1], lin4_rows=m["lin4"][1],
                lin4_lo=m["lin4"][0][:224], lin4_hi=m["lin4"][0][224:], lin3_rows=np.concatenate([m["lin3"][1], np.full(32, -1, np.int32)]),
                holes352=holes, perm224=perm224, perm256=perm256, id288_257=images.ident_map(257, 288)), 1.0 / images.SDF_UNIT


def _d(splits, M, N, rmap, cmap, acc=0, tgt=None, t_stride=0, t_rows=0, bt=None, bt_rows=0, x=None):
    return dict(splits=splits, M=M, N=N, rmap=rmap, cmap=cmap, acc=acc, tgt=tgt, t_stride=t_stride, t_rows=t_rows, bt=bt,
                bt_rows=bt_rows, x=x)


FINALIZE = {
    # (descriptors, max_M beyond the tallest descriptor)
    "shapes": ([
        _d(1, 32, 32, "id3_32", "id32", tgt="t0", t_stride=32, t_rows=3, bt="b0", bt_rows=3),
        _d(7, 96, 224, "id84_96", "perm224", tgt="t1", t_stride=224, t_rows=84, bt="b1", bt_rows=84),
        _d(8, 256, 288, "lin3_rows", "lin4_lo+64", tgt="t2", t_stride=300, t_rows=217, bt="b2", bt_rows=217),
        _d(9, 288, 352, "lin8_rows", "holes352", tgt="t3", t_stride=323, t_rows=257, bt="b3", bt_rows=257),
        _d(19, 256, 0, "id256", None, tgt="t4", t_stride=8, t_rows=256, bt="b4", bt_rows=256),       # N = 0: the bias alone
        _d(512, 1, 0, "id1", None, bt="var", bt_rows=1),                                             # the variance descriptor
        _d(19, 96, 32, "id96", "id32", tgt="t5", t_stride=40, t_rows=96),                            # btarget NULL
    ], 5),
    "pair_xsum": ([
        # the lin4 pair: 224 + 64 image columns into disjoint columns of one [256, 256] target
        _d(8, 256, 224, "lin4_rows", "lin4_lo", tgt="w4", t_stride=256, t_rows=256, bt="b4", bt_rows=256),
        _d(9, 256, 64, "lin4_rows", "lin4_hi", tgt="w4", t_stride=256, t_rows=256),
        # the extra row: xsplits != splits, a scrambled cmap (the sums are indexed by the TARGET column), image row 256 -> row 0
        _d(7, 288, 256, "lin8_rows", "perm256", tgt="w8", t_stride=256, t_rows=257, bt="b8", bt_rows=257, x=(19, 256, 0)),
        _d(1, 288, 32, "id288_257", "id32", tgt="w9", t_stride=33, t_rows=257, x=(3, 32, 256)),
    ], 0),
    "phases": ([
        _d(9, 96, 32, "id84_96", "id32", acc=0, tgt="s0", t_stride=32, t_rows=84, bt="c0", bt_rows=84),
        _d(19, 32, 224, "id3_32", "perm224", acc=1, tgt="a0", t_stride=224, t_rows=3, bt="d0", bt_rows=3),
        _d(8, 256, 32, "lin4_rows", "id32", acc=1, tgt="a1", t_stride=48, t_rows=256, x=(7, 32, 5)),
        _d(7, 32, 288, "id32", "lin4_lo+64", acc=0, tgt="s1", t_stride=288, t_rows=32),
        _d(512, 1, 0, "id1", None, acc=1, bt="var", bt_rows=1),
    ], 3),
}


def finalize_case_ids():
    return [(n, k) for n in FINALIZE for k in KINDS]


@functools.lru_cache(maxsize=8)
def finalize_case(name, kind):
    """-> dict(descs, max_M, targets): descs carry the arrays (rmap, cmap int32; slab [splits,M,N], colsum [splits,M], xsum
    [xsplits,xM] float32) and the float32 scales; targets = {name: flat float32 pre-fill}: NaN, and finite values exactly where an
    accumulating descriptor adds."""
    specs, extra = FINALIZE[name]
    maps, inv_unit = _maps()
    rs = _rng("finalize/%s/%s" % (name, kind))

    def get_map(key):
        if key is None:
            return None
        if key == "lin4_lo+64":            # 288 image columns: the 224 of lin4's first entry, then 64 more target columns
            return np.concatenate([maps["lin4_lo"], 217 + np.arange(64, dtype=np.int32)])
        return maps[key]

    descs, targets = [], {}
    for k, sp in enumerate(specs):
        d = dict(sp)
        d["rmap"], d["cmap"] = get_map(sp["rmap"]), get_map(sp["cmap"])
        assert len(d["rmap"]) == d["M"] and (d["cmap"] is None or len(d["cmap"]) == d["N"])
        d["accumulate"] = sp["acc"]
        pw = lambda: np.float32(2.0 ** rs.randint(-3, 3))
        if kind == "exact":
            d["scale"], d["bscale"], d["xscale"] = pw(), pw(), pw()
        else:
            d["scale"], d["bscale"], d["xscale"] = np.float32(inv_unit), np.float32(-0.7 * inv_unit), np.float32(inv_unit)
        d["slab"] = _values(rs, kind, (d["splits"], d["M"], d["N"]))
        d["colsum"] = _values(rs, kind, (d["splits"], d["M"]))
        d["xsum"] = None
        d["xrow"] = 0
        if sp["x"] is not None:
            xsplits, xM, d["xrow"] = sp["x"]
            d["xsum"] = _values(rs, kind, (xsplits, xM))
            assert d["cmap"].max() < xM
        for key, n in ((sp["tgt"], sp["t_rows"] * sp["t_stride"]), (sp["bt"], sp["bt_rows"])):
            if key is not None and key not in targets:
                targets[key] = np.full(n, np.nan, np.float32)
        if sp["acc"]:                      # '+=' needs something finite to add to - there and only there
            r = d["rmap"][d["rmap"] >= 0]
            if sp["tgt"] is not None and d["N"]:
                c = d["cmap"][d["cmap"] >= 0]
                idx = (r[:, None] * sp["t_stride"] + c[None, :]).ravel()
                targets[sp["tgt"]][idx] = _values(rs, kind, idx.shape)
            if sp["bt"] is not None:
                targets[sp["bt"]][r] = _values(rs, kind, r.shape)
        descs.append(d)
    return dict(name=name, kind=kind, descs=descs, max_M=max(d["M"] for d in descs) + extra, targets=targets)


def finalize_reference(case, dtype=np.float64):
    """Apply phase 0 then phase 1 of the table with dw_ops.finalize -> ({target: after phase 0}, {target: after phase 1},
    {target: units (0 where nothing is written)})."""
    state = {k: np.array(v, dtype) for k, v in case["targets"].items()}
    units = {k: np.zeros(len(v)) for k, v in case["targets"].items()}
    after = []
    for phase in (0, 1):
        for d in case["descs"]:
            if d["accumulate"] != phase:
                continue
            t0 = None if d["tgt"] is None else state[d["tgt"]]
            b0 = None if d["bt"] is None else state[d["bt"]]
            ut, ub = dw_ops.finalize_units(d, d["slab"], d["colsum"], d["xsum"], t0, b0)
            t, b = dw_ops.finalize(d, d["slab"], d["colsum"], d["xsum"], t0, b0, dtype)
            for key, new, u in ((d["tgt"], t, ut), (d["bt"], b, ub)):
                if key is not None:
                    state[key] = new
                    units[key] = np.maximum(units[key], u)
        after.append({k: v.copy() for k, v in state.items()})
    return after[0], after[1], units


# ---- weight norm --------------------------------------------------------------------------------------------------------------
# name -> [(rows, cols, weight-normed)]: descriptors of different height in one launch; max_rows = the tallest
WEIGHTNORM = {
    "tall_last": [(1, 1, True), (3, 3, True), (4, 39, True), (5, 64, True), (257, 65, True), (3, 256, True), (5, 352, True), (3, 65, False)],
    "tall_first": [(257, 1, True), (5, 3, True), (1, 39, True), (4, 64, True), (3, 65, True), (257, 256, True), (4, 352, True), (5, 39, False)],
}


def weightnorm_case(name):
    """-> [dict(rows, cols, normed, g [rows], v [rows,cols], dw [rows,cols])] float32."""
    rs = _rng("weightnorm/" + name)
    out = []
    for rows, cols, normed in WEIGHTNORM[name]:
        out.append(dict(rows=rows, cols=cols, normed=normed, g=(rs.standard_normal(rows) * 2.0).astype(np.float32),
                        v=(rs.standard_normal((rows, cols)) * 0.3).astype(np.float32), dw=rs.standard_normal((rows, cols)).astype(np.float32)))
    return out


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
WRAP = 2048 * 256                          # elements one pass of the grid covers (csrc/train_opt.hip)
# name -> (begin0, end0, begin1, end1, step, single): single = through vdn_adam_step (begin0 = 0, no second range)
ADAM = {
    "n1": (0, 1, 0, 0, 1, True),
    "n255_begin7": (7, 262, 0, 0, 2, False),
    "n256_gap": (3, 131, 200, 328, 1000, False),
    "n257_empty2nd": (0, 257, 300, 300, 1, False),
    "n257_step2": (0, 257, 0, 0, 2, True),
    "wrap_gap": (5, 400005, 400100, 400100 + WRAP + 3 - 400000, 2, False),
    "wrap_single": (0, WRAP + 3, 0, 0, 1000, True),
}
ADAM_ERRORS = {"step0": (0, 64, 0, 0, 0), "end_before_begin": (10, 9, 0, 0, 1), "end1_before_begin1": (0, 8, 20, 19, 1),
               "empty": (5, 5, 9, 9, 1), "negative_begin": (-1, 8, 0, 0, 1)}
ADAM_HYPER = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8)


def adam_hyper():
    """The hyper-parameters as the entry point receives them: C floats. Both models get these float32 values (as Python floats)."""
    f = lambda x: float(np.float32(x))
    return dict(lr=f(ADAM_HYPER["lr"]), betas=tuple(f(b) for b in ADAM_HYPER["betas"]), eps=f(ADAM_HYPER["eps"]))


def adam_case(name):
    """-> dict(size, ranges, step, single, p, g, m, v float32 [size]). Outside the ranges everything is NaN (a kernel that reads or
    writes there shows); the buffers are long enough that second-range indices taken without rebasing stay inside them. Every
    seventh selected element has g = 0 on zero moments, g = 1e-20 (g^2 subnormal) or g = 1e4 in turn."""
    b0, e0, b1, e1, step, single = ADAM[name]
    n = (e0 - b0) + (e1 - b1)
    size = max(e0, e1, b1 + n) + 64
    rs = _rng("adam/" + name)
    p, g, m, v = (np.full(size, np.nan, np.float32) for _ in range(4))
    sel = np.concatenate([np.arange(b0, e0), np.arange(b1, e1)])
    p[sel] = rs.standard_normal(n) * 0.3
    g[sel] = rs.standard_normal(n) * 10.0 ** rs.uniform(-4, 0, n)
    if step == 1:
        m[sel], v[sel] = 0.0, 0.0
    else:
        m[sel] = rs.standard_normal(n) * 0.01
        v[sel] = (rs.standard_normal(n) * 0.01) ** 2
    if n == 1:
        g[sel] = 1e4
    else:
        k = sel[::7]
        g[k[0::3]], m[k[0::3]], v[k[0::3]] = 0.0, 0.0, 0.0
        g[k[1::3]] = 1e-20
        m[k[1::6]], v[k[1::6]] = 0.0, 0.0              # half of them on zero moments: v = g^2 (1 - beta2) stays subnormal
        g[k[2::3]] = 1e4
    return dict(name=name, size=size, ranges=[(b0, e0), (b1, e1)], step=step, single=single, p=p, g=g, m=m, v=v, sel=sel)


@functools.lru_cache(maxsize=2)
def adam_reference(name):
    """-> (case, (p, m, v) float64 model, (p, m, v) torch.optim.Adam in float32, (up, um, uv) units), over the selected elements."""
    c = adam_case(name)
    h = adam_hyper()
    sel = c["sel"]
    z = lambda x: np.nan_to_num(x.astype(np.float64), nan=0.0)
    ref = dw_ops.adam(z(c["p"]), z(c["g"]), z(c["m"]), z(c["v"]), c["ranges"], step=c["step"], **h)
    f32 = dw_ops.adam_torch(z(c["p"]), z(c["g"]), z(c["m"]), z(c["v"]), c["ranges"], step=c["step"], dtype=torch.float32, **h)
    units = dw_ops.adam_units(z(c["p"])[sel], z(c["g"])[sel], z(c["m"])[sel], z(c["v"])[sel], ref[0][sel])
    return c, tuple(x[sel] for x in ref), tuple(x[sel] for x in f32), units
