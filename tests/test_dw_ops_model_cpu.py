"""The float64 models of the parameter-update tail (oracle/dw_ops.py) and their constructed cases (oracle/dw_cases.py), proven
without a GPU: the models against torch itself in float64 (torch.optim.Adam, torch.nn.utils.weight_norm under autograd) and against
a dense np.add.at scatter, the exact cases exact in any float32 order, every branch the GPU test is after hit by a named case,
and the float32 floors of the random cases (printed: pytest -rA)."""
import numpy as np
import pytest
import torch

from oracle import dw_cases, dw_ops


# ---- the models -------------------------------------------------------------------------------------------------------------

def test_adam_model_equals_torch_optim_adam_float64():
    """Two parameter groups at different step counts, 3 steps each, with torch's own state carried from step to step."""
    rs = np.random.RandomState(7)
    n = 300
    ranges = [(5, 120), (160, 290)]
    start = (0, 41)                                   # steps already taken per group
    p, m, v = rs.standard_normal(n), np.zeros(n), np.zeros(n)
    m[160:290], v[160:290] = rs.standard_normal(130) * 0.01, (rs.standard_normal(130) * 0.01) ** 2
    hyper = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6)]
    pars, opts = [], []
    for (lo, hi), s0, h in zip(ranges, start, hyper):
        par = torch.nn.Parameter(torch.tensor(p[lo:hi]))
        opt = torch.optim.Adam([par], foreach=False, **h)
        if s0:
            opt.state[par] = dict(step=torch.tensor(float(s0)), exp_avg=torch.tensor(m[lo:hi]), exp_avg_sq=torch.tensor(v[lo:hi]))
        pars.append(par)
        opts.append(opt)
    p0 = p.copy()
    for k in range(3):
        g = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 1, n)
        for (lo, hi), s0, h, par, opt in zip(ranges, start, hyper, pars, opts):
            p, m, v = dw_ops.adam(p, g, m, v, [(lo, hi)], step=s0 + k + 1, **h)
            par.grad = torch.tensor(g[lo:hi])
            opt.step()
            st = opt.state[par]
            for mine, theirs in ((p, par.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                np.testing.assert_allclose(mine[lo:hi], theirs.numpy(), rtol=1e-13, atol=1e-300)
            # and the one-step wrapper the float32 floor comes from
            one = dw_ops.adam_torch(p, g, m, v, [], step=1, dtype=torch.float64, **h)
            assert all(np.array_equal(a, b) for a, b in zip(one, (p, m, v)))
    out = np.ones(n, bool)
    for lo, hi in ranges:
        out[lo:hi] = False
    assert np.array_equal(p[out], p0[out]) and not m[out].any() and not v[out].any()          # nothing outside the ranges


def test_adam_torch_wrapper_restores_the_step_count():
    """adam_torch(step = s) on (m, v) equals torch.optim.Adam's s-th step: against the model, float64, steps 1, 2 and 1000."""
    rs = np.random.RandomState(8)
    n = 64
    p, g = rs.standard_normal(n), rs.standard_normal(n)
    m, v = rs.standard_normal(n) * 0.1, rs.standard_normal(n) ** 2
    h = dw_cases.adam_hyper()
    for step in (1, 2, 1000):
        a = dw_ops.adam(p, g, m, v, [(3, 20), (30, 64)], step=step, **h)
        b = dw_ops.adam_torch(p, g, m, v, [(3, 20), (30, 64)], step=step, dtype=torch.float64, **h)
        for x, y in zip(a, b):
            np.testing.assert_allclose(x, y, rtol=1e-13)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 39), (5, 64), (4, 65), (257, 352)])
def test_weightnorm_model_equals_torch_weight_norm_float64(rows, cols):
    rs = np.random.RandomState(rows * 1000 + cols)
    g, v, dw = rs.standard_normal(rows), rs.standard_normal((rows, cols)), rs.standard_normal((rows, cols))
    lin = torch.nn.utils.weight_norm(torch.nn.Linear(cols, rows, bias=False).double(), dim=0)
    with torch.no_grad():
        lin.weight_g.copy_(torch.tensor(g)[:, None])
        lin.weight_v.copy_(torch.tensor(v))
    # (weight_norm recomputes .weight in a forward pre-hook: run one forward, then backpropagate dw into the weight)
    lin(torch.zeros(1, cols, dtype=torch.float64))
    lin.weight.backward(torch.tensor(dw))
    w, inv = dw_ops.weightnorm(torch.tensor(g), torch.tensor(v))
    np.testing.assert_allclose(w.numpy(), lin.weight.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(inv.numpy(), 1.0 / np.sqrt((v * v).sum(1)), rtol=1e-13)
    dg, dv = dw_ops.weightnorm_bwd(g, v, dw)
    np.testing.assert_allclose(dg.numpy(), lin.weight_g.grad[:, 0].numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(dv.numpy(), lin.weight_v.grad.numpy(), rtol=1e-11, atol=1e-14)
    uw, udg, udv = dw_ops.weightnorm_units(g, v, dw)
    assert uw.shape == w.shape and udg.shape == (rows,) and udv.shape == dv.shape and (udv > 0).all()
    if cols == 1:                                     # dv cancels entirely: its unit must not
        assert np.abs(dv.numpy()).max() <= 1e-12 * np.abs(dw).max() and (udv >= dw_ops.ULP * np.abs(g[:, None] * dw / v) * 0.99).all()


@pytest.mark.parametrize("name,kind", dw_cases.finalize_case_ids())
def test_finalize_model_equals_a_dense_scatter(name, kind):
    case = dw_cases.finalize_case(name, kind)
    a0, a1, units = dw_cases.finalize_reference(case)
    state = {k: v.astype(np.float64) for k, v in case["targets"].items()}
    for phase in (0, 1):
        for d in case["descs"]:
            if d["accumulate"] != phase:
                continue
            rmap = d["rmap"]
            i = np.nonzero(rmap >= 0)[0]
            if d["tgt"] is not None and d["N"]:
                j = np.nonzero(d["cmap"] >= 0)[0]
                dense = float(d["scale"]) * d["slab"].astype(np.float64).sum(0)
                if d["xsum"] is not None:
                    row = np.nonzero(rmap == d["xrow"])[0]
                    dense[row[:, None], j[None, :]] += float(d["xscale"]) * d["xsum"].astype(np.float64).sum(0)[d["cmap"][j]][None, :]
                idx = rmap[i][:, None] * d["t_stride"] + d["cmap"][j][None, :]
                t = state[d["tgt"]]
                if not phase:
                    t[idx.ravel()] = 0.0
                np.add.at(t, idx.ravel(), dense[i[:, None], j[None, :]].ravel())
            if d["bt"] is not None:
                b = state[d["bt"]]
                if not phase:
                    b[rmap[i]] = 0.0
                np.add.at(b, rmap[i], float(d["bscale"]) * d["colsum"].astype(np.float64).sum(0)[i])
        want = a0 if phase == 0 else a1
        for k in state:
            assert np.array_equal(np.isnan(state[k]), np.isnan(want[k])), (k, phase)
            np.testing.assert_allclose(np.nan_to_num(want[k]), np.nan_to_num(state[k]), rtol=1e-13, atol=1e-13, err_msg="%s phase %d" % (k, phase))
    for k, u in units.items():                       # a unit wherever something is written, none elsewhere
        written = ~np.isnan(a1[k])
        assert not u[~written].any()
        if kind == "random":
            assert (u[written] > 0).all(), k


def test_split_ranges_partition_the_rows():
    for P in (0, 1, 31, 40, 300, 1403, 6013):
        for splits, two in ((1, False), (6, False), (9, False), (17, False), (2, True), (6, True), (18, True)):
            for stage in (dw_ops.F32_STAGE, dw_ops.BF16_STAGE):
                rg = dw_ops.split_ranges(P, splits, two, stage)
                assert len(rg) == splits
                for seg in ((0, 1) if two else (0,)):
                    cover = np.zeros(P, int)
                    for s, k0, k1 in rg:
                        if s == seg and k1 > k0:
                            assert k0 % stage == 0
                            cover[k0:k1] += 1
                    assert (cover == 1).all()
                assert [s for s, _, _ in rg] == sorted(s for s, _, _ in rg)             # first half = segment 1


# ---- the cases --------------------------------------------------------------------------------------------------------------

def test_cases_are_deterministic_from_their_names():
    a, b = dw_cases.gemm_case("p40", "random", "bf16"), dw_cases.gemm_case("p40", "random", "bf16")
    assert all(np.array_equal(x["segs"][0][0], y["segs"][0][0]) for x, y in zip(a["entries"], b["entries"]))
    assert np.array_equal(dw_cases.adam_case("n256_gap")["g"], dw_cases.adam_case("n256_gap")["g"], equal_nan=True)
    a, b = dw_cases.weightnorm_case("tall_last"), dw_cases.weightnorm_case("tall_last")
    assert all(np.array_equal(x["v"], y["v"]) for x, y in zip(a, b))


@pytest.mark.parametrize("name", [n for n, spec in dw_cases.GEMM.items() if "exact" in spec[3]])
def test_exact_gemm_cases_are_exact_in_float32(name):
    """The float32 chain equals the float64 model bit for bit, and so does any other order: sum |a b| stays below 2^24."""
    case, ref = dw_cases.gemm_reference(name, "exact", dw_cases.GEMM[name][4][0])
    for e, r in zip(case["entries"], ref):
        for a, b in e["segs"]:
            for x in (a, b):
                if x is not None:
                    assert np.abs(x).max() <= 8 and np.array_equal(x, np.round(x))
                    assert np.array_equal(x, torch.from_numpy(x).to(torch.bfloat16).float().numpy())
        chain, chain_cs = dw_ops.dw_gemm_chain_f32(e["segs"], case["rows"])
        if e["N"]:
            assert r["u_prod"].max() / dw_ops.ULP < 2 ** 24
            assert chain.dtype == np.float32 and np.array_equal(chain.astype(np.float64), r["prod"])
        assert np.array_equal(chain_cs.astype(np.float64), r["cs"])


@pytest.mark.parametrize("name", list(dw_cases.FINALIZE))
def test_exact_finalize_cases_are_exact_in_float32(name):
    case = dw_cases.finalize_case(name, "exact")
    for d in case["descs"]:
        for s in (d["scale"], d["bscale"], d["xscale"]):
            assert np.log2(float(s)) == np.round(np.log2(float(s)))
    a0, a1, _ = dw_cases.finalize_reference(case)
    b0, b1, _ = dw_cases.finalize_reference(case, np.float32)
    for k in a1:
        assert b1[k].dtype == np.float32
        assert np.array_equal(b0[k].astype(np.float64), a0[k], equal_nan=True) and np.array_equal(b1[k].astype(np.float64), a1[k], equal_nan=True)


def test_every_branch_is_hit_by_a_named_case():
    ids = dw_cases.gemm_case_ids()
    for prec in ("fp32", "bf16"):
        ents = [(n, k, P, P_dev, e) for n, (P, P_dev, es, kinds, precs) in dw_cases.GEMM.items() if prec in precs for k in kinds for e in es]
        stage = dw_ops.F32_STAGE if prec == "fp32" else dw_ops.BF16_STAGE
        # split counts across the 8-slot rounds: one-segment 9 and 17, two-segment 18
        assert {(e[3], e[2]) for *_, e in ents} >= {(9, False), (17, False), (18, True)}
        # splits that receive no rows although the entry has some; an empty work list; a single row
        empties = lambda P, P_dev, e: sum(k1 <= k0 for _, k0, k1 in dw_ops.split_ranges(P if P_dev is None else min(P, P_dev), e[3], e[2], stage))
        assert any(P == 40 and e[3] == 6 and 0 < empties(P, P_dev, e) < 6 for _, _, P, P_dev, e in ents)
        assert any(P_dev == 0 for _, _, _, P_dev, _ in ents) and any(P == 1 for _, _, P, _, _ in ents)
        assert any(P_dev is not None and 0 < P_dev < P and P_dev % stage for _, _, P, P_dev, _ in ents)
        # the widest output, n_tiles = 0, colsum NULL, and the matrix of tests/test_gpu_dw_gemm.py on exact values
        assert any(e[:2] == (288, 352) for *_, e in ents) and any(e[1] == 0 for *_, e in ents) and any("nocs" in e for *_, e in ents)
        for n in ("mat4096", "mat5000", "mat8269", "mat300"):
            assert (n, "exact", prec) in ids
        # both kinds of value on every new shape that has rows
        for n in ("p1", "p40", "rounds", "wide"):
            assert (n, "exact", prec) in ids and (n, "random", prec) in ids
        assert all(P <= 5000 for _, k, P, _, _ in ents if k == "random")
    assert ("slice", "exact", "fp32") in ids and any("slice" in e for e in dw_cases.GEMM["slice"][2])
    # finalize
    descs = [d for specs, _ in dw_cases.FINALIZE.values() for d in specs]
    assert {d["splits"] for d in descs} >= {1, 7, 8, 9, 19, 512}          # below 8, the main loop alone, main loop + ragged tail
    assert {d["N"] for d in descs} >= {0, 32, 224, 288, 352} and {d["M"] for d in descs} >= {1, 32, 96, 256, 288}
    assert any(d["M"] == 1 and d["N"] == 0 and d["splits"] == 512 and d["tgt"] is None for d in descs)
    built = [d for n in dw_cases.FINALIZE for d in dw_cases.finalize_case(n, "exact")["descs"]]
    assert any((d["rmap"] < 0).any() for d in built) and any(d["cmap"] is not None and (d["cmap"] < 0).any() for d in built)
    assert any(d["rmap"].tolist() == list(range(3)) + [-1] * 29 for d in built)
    assert any(d["cmap"] is not None and d["cmap"].tolist() == list(range(84)) + [-1] * 12 for d in built) or \
        any(d["rmap"].tolist() == list(range(84)) + [-1] * 12 for d in built)
    perm = lambda m: (m >= 0).any() and not np.array_equal(m[m >= 0], np.arange((m >= 0).sum()))
    assert any(perm(d["rmap"]) for d in built)
    assert any(d["xsum"] is not None and d["x"][0] != d["splits"] and perm(d["cmap"]) for d in built)
    assert any(d["bt"] is None for d in built) and any(d["tgt"] is not None and d["t_stride"] > d["N"] > 0 for d in built)
    pair = [d for d in built if d["tgt"] == "w4"]
    assert [d["N"] for d in pair] == [224, 64] and not set(pair[0]["cmap"][pair[0]["cmap"] >= 0]) & set(pair[1]["cmap"][pair[1]["cmap"] >= 0])
    for n, (specs, extra) in dw_cases.FINALIZE.items():
        assert extra > 0 or len({d["M"] for d in specs}) > 1               # max_M above some descriptor's M
    assert any({d["acc"] for d in specs} == {0, 1} for specs, _ in dw_cases.FINALIZE.values())
    # weight norm
    shapes = [s for v in dw_cases.WEIGHTNORM.values() for s in v]
    assert {r for r, _, _ in shapes} >= {1, 3, 4, 5, 257} and {c for _, c, _ in shapes} >= {1, 3, 39, 64, 65, 256, 352}
    assert any(c % 64 and c > 64 for _, c, _ in shapes) and any(not normed for _, _, normed in shapes)
    assert all(len({r for r, _, _ in v}) > 1 for v in dw_cases.WEIGHTNORM.values())
    # Adam
    A = dw_cases.ADAM
    assert {(e0 - b0) + (e1 - b1) for b0, e0, b1, e1, _, _ in A.values()} >= {1, 255, 256, 257, dw_cases.WRAP + 3}
    assert {s for *_, s, _ in A.values()} >= {1, 2, 1000}
    assert any(b0 > 0 for b0, *_ in A.values()) and any(e1 > b1 > e0 for _, e0, b1, e1, _, _ in A.values())
    assert any(e1 == b1 and b1 > 0 for _, _, b1, e1, _, _ in A.values())
    assert any(e1 > b1 and (e0 - b0) + (e1 - b1) > dw_cases.WRAP for b0, e0, b1, e1, _, _ in A.values())
    c = dw_cases.adam_case("n255_begin7")
    g, m, v = (c[k][c["sel"]] for k in "gmv")
    assert ((g == 0) & (m == 0) & (v == 0)).any() and (g == np.float32(1e4)).any()
    tiny = g == np.float32(1e-20)
    assert (tiny & (v == 0)).any() and (tiny & (v > 0)).any() and 0 < float(np.float32(1e-20)) ** 2 < np.finfo(np.float32).tiny
    for k in "pgmv":                                 # NaN everywhere outside the ranges
        out = np.ones(c["size"], bool)
        out[c["sel"]] = False
        assert np.isnan(c[k][out]).all() and np.isfinite(c[k][c["sel"]]).all()
    for b0, e0, b1, e1, step in dw_cases.ADAM_ERRORS.values():
        assert step < 1 or e0 < b0 or e1 < b1 or (e0 - b0) + (e1 - b1) == 0 or b0 < 0


def test_print_the_float32_floors_of_the_random_cases():
    """Not an assertion on a kernel: the floors max(1, 3 x floor) is built from, on this machine's torch / numpy (pytest -rA)."""
    rows = []
    for n, k, p in dw_cases.gemm_case_ids():
        if k == "random":
            case, ref = dw_cases.gemm_reference(n, k, p)
            for i, r in enumerate(ref):
                rows.append("gemm %-5s %-9s entry %d  slab %.3f  colsum %.3f" % (p, n, i, r["floor_prod"], r["floor_cs"]))
                assert np.isfinite([r["floor_prod"], r["floor_cs"]]).all()
    for n in dw_cases.FINALIZE:
        case = dw_cases.finalize_case(n, "random")
        _, a1, units = dw_cases.finalize_reference(case)
        _, b1, _ = dw_cases.finalize_reference(case, np.float32)
        for key in a1:
            w = ~np.isnan(a1[key])
            rows.append("finalize %-10s %-4s %.3f" % (n, key, dw_ops.units_err(b1[key][w], a1[key][w], units[key][w])))
    for n in dw_cases.WEIGHTNORM:
        for i, d in enumerate(dw_cases.weightnorm_case(n)):
            if d["normed"]:
                rows.append("weightnorm %-10s desc %d  w %.3f  dg %.3f  dv %.3f" % ((n, i) + weightnorm_floors(d)))
    for n in dw_cases.ADAM:
        _, ref, f32, units = dw_cases.adam_reference(n)
        rows.append("adam %-14s p %.3f  m %.3f  v %.3f" % ((n,) + tuple(dw_ops.units_err(f32[i], ref[i], units[i]) for i in range(3))))
    print("float32 floors in units:\n" + "\n".join(rows))


def weightnorm_floors(d):
    g, v, dw = (torch.from_numpy(d[k]) for k in ("g", "v", "dw"))
    uw, udg, udv = dw_ops.weightnorm_units(d["g"], d["v"], d["dw"])
    w64, _ = dw_ops.weightnorm(g.double(), v.double())
    w32, _ = dw_ops.weightnorm(g, v)
    dg64, dv64 = dw_ops.weightnorm_bwd(g, v, dw)
    dg32, dv32 = dw_ops.weightnorm_bwd(g, v, dw, torch.float32)
    return (dw_ops.units_err(w32.numpy(), w64.numpy(), uw), dw_ops.units_err(dg32.numpy(), dg64.numpy(), udg),
            dw_ops.units_err(dv32.numpy(), dv64.numpy(), udv))
