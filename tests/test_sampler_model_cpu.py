"""The float64 model of the hierarchical sampler (oracle/sampler_ops.py) and its constructed inputs (oracle/sampler_cases.py),
without a GPU: the proof that tests/test_gpu_sampler.py tests what it claims.

* fidelity: upsample_stages' new_z is element for element neus_oracle.up_sample / sample_pdf_det, in float32 and in float64;
  merge is neus_oracle.cat_z_vals' sort;
* floors per case: F_z = max|z32 - z64| and F_cdf = max|cdf32 - cdf64|, the float32 CPU model against the float64 one;
* conditions per class: tight - no entry branch-sensitive at tau = 10 F_cdf and F_z <= 1e-5; ill-conditioned - at most 2 % of the
  entries branch-sensitive at tau = 3 F_cdf. The float32 model itself passes the comparator in every case;
* coverage: every branch of the round and of the merge is taken by at least 8 entries somewhere;
* the yardstick bites: the float32 model with one seeded defect at a time, judged by the comparator the GPU test uses
  (sampler_ops.judge), is rejected by at least one case, for every defect;
* the floors committed in profiles/sampler_floors_cpu.json (tools/sampler_floors.py) describe these cases.
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle.neus_oracle as orc
from oracle import sampler_cases as sc
from oracle import sampler_ops as so

NAMES = sc.upsample_case_names()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a defect of the SDF-derived weights cannot show in a case that is handed its weights
NEEDS_SDF = ("no_trans_eps", "prev_cos_wraps", "inside_and", "no_lower_clip", "no_alpha_eps", "inv_s_next_round", "inv_s_prev_round")


@pytest.fixture(scope="module")
def models():
    out = {}
    for name in NAMES:
        case = sc.upsample_case(name)
        out[name] = (case, so.stages_of(case, torch.float64), so.stages_of(case, torch.float32))
    return out


def test_case_matrix_covers_the_shapes():
    cs = [sc.upsample_case(n) for n in NAMES]
    assert {c["B"] for c in cs} >= {1, 3, 4, 5, 77}
    assert {c["M"] for c in cs} >= {2, 3, 63, 64, 65, 112, 128, 255, 256}
    assert {c["n_imp"] for c in cs} >= {1, 16, 17, 64}
    assert {c["inv_s"] for c in cs} == {64.0, 512.0, 2048.0}
    assert {"M" if c["ld"] == c["M"] else "M+n" if c["ld"] == c["M"] + c["n_imp"] else c["ld"] for c in cs} == {"M", "M+n", 160}
    given = [c for c in cs if c["weights"] is not None]
    assert {c["w_ld"] - c["M"] for c in given} == {-1, 2}
    assert max(c["B"] for c in cs) <= 257 and all(c["ld"] >= c["M"] for c in cs)
    a, b = sc.upsample_case(NAMES[4]), sc.upsample_case(NAMES[4])
    assert all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))          # deterministic from the name
    assert {(c[0], c[1], c[2]) for c in sc.MERGE_CASES.values()} >= {(1, 1, 1), (3, 64, 16), (5, 112, 16), (2, 192, 64), (77, 240, 16)}
    assert any(c[4] > c[1] + c[2] for c in sc.MERGE_CASES.values())
    assert {(c[5], c[6]) for c in sc.MERGE_CASES.values()} == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_model_equals_the_line_cited_oracle(models, dtype):
    for name, (case, _, _) in models.items():
        if case["exact_knots"] or case["kind"] == "flat_u":
            continue                                    # (their u is not the linspace the oracle draws for itself)
        t = lambda k: torch.as_tensor(case[k]).to(dtype)
        n = case["n_imp"]
        u = torch.linspace(0.5 / n, 1.0 - 0.5 / n, n, dtype=dtype)
        if case["weights"] is None:
            st = so.upsample_stages(t("rays_o"), t("rays_d"), t("z"), t("sdf"), u, case["inv_s"])
            ref = orc.up_sample(t("rays_o"), t("rays_d"), t("z"), t("sdf"), n, case["inv_s"])
        else:
            st = so.upsample_stages(None, None, t("z"), None, u, case["inv_s"], weights=t("weights"))
            ref = orc.sample_pdf_det(t("z"), t("weights"), n)
        assert st["new_z"].dtype == dtype and torch.equal(st["new_z"], ref), name
    for name in sc.MERGE_CASES:
        c = sc.merge_case(name)
        t = lambda k: None if c[k] is None else torch.as_tensor(c[k]).to(dtype)
        zs, sd = so.merge(t("z"), t("sdf"), t("new_z"), t("new_sdf"))
        fn = lambda pts: t("new_sdf").reshape(-1, 1)
        o = torch.zeros(c["B"], 3, dtype=dtype)
        rz, rs = orc.cat_z_vals(fn, o, o, t("z"), t("new_z"), t("sdf"), last=c["sdf"] is None)
        assert torch.equal(zs, rz), name
        # (torch.sort without stable=True, as the reference calls it, promises no order among ties: only the depths are compared
        # there; with distinct depths the sdf rows agree too)
        if c["sdf"] is not None:
            distinct = (zs[:, 1:] != zs[:, :-1]).all(-1)
            assert torch.equal(sd[distinct], rs[distinct]), name


def _record(models):
    rec = {}
    for name, (case, s64, s32) in models.items():
        F_z, F_cdf = so.floors(s64, s32)
        tau = (10.0 if case["cls"] == "tight" else 3.0) * F_cdf
        sens, _ = so.classify(s64, tau, case["exact_knots"])
        rec[name] = {"cls": case["cls"], "B": case["B"], "M": case["M"], "n_imp": case["n_imp"], "inv_s": case["inv_s"], "F_z": F_z,
                     "F_cdf": F_cdf, "tau": tau, "sensitive": int(sens.sum()), "entries": int(sens.numel())}
    return rec


def test_floors_and_conditions_per_class(models):
    rec = _record(models)
    for name, (case, s64, s32) in models.items():
        r = rec[name]
        print("%-28s %-5s F_z %.2e  F_cdf %.2e  sensitive %d / %d" % (name, r["cls"], r["F_z"], r["F_cdf"], r["sensitive"], r["entries"]))
        if case["cls"] == "tight":
            assert r["sensitive"] == 0 and r["F_z"] <= 1e-5, (name, r)
        else:
            assert r["sensitive"] <= 0.02 * r["entries"], (name, r)
        # the yardstick is passable: plain float32 arithmetic of the same formulas meets it, within a third of the bound in depth
        j = so.judge(case, s64, s32, s32["new_z"])
        assert j["ok"] and j["n_by_candidate"] == 0, (name, j)
        assert torch.isfinite(s64["new_z"]).all() and torch.isfinite(s32["new_z"]).all(), name
    assert sum(r["cls"] == "ill" and r["F_z"] > 1e-5 for r in rec.values()) >= 1          # the ill class IS ill-conditioned in depth


def test_recorded_floors_describe_these_cases(models):
    with open(os.path.join(ROOT, "profiles", "sampler_floors_cpu.json")) as f:
        doc = json.load(f)
    rec = _record(models)
    assert set(doc["cases"]) == set(rec)
    for name, r in rec.items():
        d = doc["cases"][name]
        assert all(d[k] == r[k] for k in ("cls", "B", "M", "n_imp", "inv_s", "entries")), name
        # (float32 libm / vector width may move a floor's last digits from one build of torch to the next: same size, not same bits)
        assert d["F_z"] <= 1e-5 if r["cls"] == "tight" else d["sensitive"] <= 0.02 * d["entries"], name
        for k in ("F_z", "F_cdf"):
            assert d[k] == r[k] or 0.25 * d[k] <= r[k] <= 4.0 * d[k], (name, k, d[k], r[k])


def test_margins_hold_in_every_case(models):
    for name, (case, s64, _) in models.items():
        if case["weights"] is None:
            assert ((s64["radius"] - 1.0).abs() >= sc.MARGIN).all(), name
        assert (s64["z"][:, 1:] >= s64["z"][:, :-1]).all(), name
        assert case["z"].shape == (case["B"], case["M"]) and case["u"].shape == (case["n_imp"],)
    for name in sc.upsample_case_names("tight"):
        case, s64, _ = models[name]
        if case["weights"] is None and case["M"] >= 8 and case["kind"] not in ("first_inside", "first_deep", "saturated"):
            crosses = ((s64["z"].new_tensor(case["sdf"]) < 0).any(-1))
            assert crosses.all() or case["kind"] == "two_surfaces", name          # every ray of the tight class meets its surface


def test_every_branch_is_taken(models):
    tot = lambda fn, pred=lambda c: True: sum(int(fn(c, s)) for c, s, _ in models.values() if pred(c))
    sdf = lambda c: c["weights"] is None
    cnt = {
        # the two arms of min(prev_cos, cos), where the section is inside and the result survives the clip at 0
        "min: prev_cos": tot(lambda c, s: ((s["prev_cos"] < s["raw_cos"]) & (s["prev_cos"] < 0) & s["inside"]).sum(), sdf),
        "min: cos": tot(lambda c, s: ((s["raw_cos"] < s["prev_cos"]) & (s["raw_cos"] < 0) & s["inside"]).sum(), sdf),
        "clip at 0": tot(lambda c, s: ((s["min_cos"] > 0) & s["inside"]).sum(), sdf),
        "clip at -1e3": tot(lambda c, s: ((s["min_cos"] < -1e3) & s["inside"]).sum(), sdf),
        "inside 0 and 1 in one ray": tot(lambda c, s: (s["inside"].any(-1) & (~s["inside"]).any(-1)).sum(), sdf),
        "inside by one end only": tot(lambda c, s: ((s["radius"][:, :-1] < 1) != (s["radius"][:, 1:] < 1)).sum(), sdf),
        "inside 0 everywhere": tot(lambda c, s: (~s["inside"]).all(-1).sum() * (c["M"] - 1), sdf),   # (sections of such rays)
        "prev_cos 0 at i = 0 decides": tot(lambda c, s: (s["raw_cos"][:, 0] < 0).sum(), sdf),
        "exact tie z[i] == z[i+1]": tot(lambda c, s: (s["z"][:, 1:] == s["z"][:, :-1]).sum(), sdf),
        "near-tie at 1e-6": tot(lambda c, s: (((s["z"][:, 1:] - s["z"][:, :-1]) > 0) & ((s["z"][:, 1:] - s["z"][:, :-1]) < 2e-6)).sum(), sdf),
        "saturation |sdf| inv_s > 90": tot(lambda c, s: ((s["z"].new_tensor(c["sdf"]).abs() * c["inv_s"]) > 90).sum(), sdf),
        "alpha == 1 (factor 1e-7)": tot(lambda c, s: (s["alpha"] >= 1.0).sum(), lambda c: c["kind"] == "saturated"),
        "flat branch": tot(lambda c, s: s["flat"].sum()),
        "u exactly on a knot": tot(lambda c, s: (s["u"][:, :, None] == s["cdf"][:, None, :]).any(-1).sum()),
        "below == 0": tot(lambda c, s: (s["below"] == 0).sum()),
        "above == M - 1": tot(lambda c, s: (s["above"] == c["M"] - 1).sum()),
        "zero weights": tot(lambda c, s: (s["weights"] == 0).sum(), lambda c: not sdf(c)),
        "merge: counting path": sum(int(so.merge_takes_counting_path(torch.as_tensor(sc.merge_case(n)["z"])).sum()) for n in sc.MERGE_CASES),
        "merge: tie old / new": 0, "merge: tie old / old": 0, "merge: tie new / new": 0,
    }
    for n in sc.MERGE_CASES:
        c = sc.merge_case(n)
        z, nz = torch.as_tensor(c["z"]), torch.as_tensor(c["new_z"])
        cnt["merge: tie old / new"] += int((z[:, :, None] == nz[:, None, :]).any(-1).sum())
        cnt["merge: tie old / old"] += int((torch.sort(z, -1)[0][:, 1:] == torch.sort(z, -1)[0][:, :-1]).sum())
        cnt["merge: tie new / new"] += int((nz[:, 1:] == nz[:, :-1]).sum())
    for tp in sc.TRAIN_PREP_SHAPES:
        c = sc.train_prep_case(*tp)
        z, nz, zo = (torch.as_tensor(c[k]) for k in ("z", "new_z", "z_out"))
        cnt.setdefault("train_prep: tie old / new", 0)
        cnt.setdefault("train_prep: tie inside / outside", 0)
        cnt["train_prep: tie old / new"] += int((z[:, :, None] == nz[:, None, :]).any(-1).sum())
        cnt["train_prep: tie inside / outside"] += int((torch.cat([z, nz], -1)[:, :, None] == zo[:, None, :]).any(-1).sum())
    print("\n".join("%-34s %d" % kv for kv in cnt.items()))
    assert all(v >= 8 for v in cnt.values()), {k: v for k, v in cnt.items() if v < 8}


def test_every_seeded_defect_is_rejected(models):
    """The float32 model with one defect stands in for a wrong kernel; the comparator is the GPU test's."""
    caught = {d: [] for d in so.DEFECTS}
    for name, (case, s64, s32) in models.items():
        for d in so.DEFECTS:
            if case["weights"] is not None and d in NEEDS_SDF:
                continue
            j = so.judge(case, s64, s32, so.stages_of(case, torch.float32, defect=d)["new_z"])
            if not j["ok"]:
                caught[d].append(name)
    print("\n".join("%-20s rejected by %2d cases: %s" % (d, len(v), ", ".join(v[:4])) for d, v in caught.items()))
    assert all(caught.values()), [d for d, v in caught.items() if not v]
    # each special case is there for a defect only it can show
    for d, name in (("search_left", "exact_knots-B5-M5-n3"), ("prev_cos_wraps", "first_inside-B5-M64-n16"), ("inside_and", "leave-B77-M128-n16"),
                    ("no_lower_clip", "ties-B5-M112-n16"), ("no_flat_threshold", "flat_u-B3-M65-n17"), ("no_alpha_eps", "first_deep-B4-M65-n17")):
        assert name in caught[d], (d, name)
    # the merge: new before equal old is a different row wherever an old and a new depth tie (the sdf travels with the depth)
    for n in sc.MERGE_CASES:
        c = sc.merge_case(n)
        t = lambda k: None if c[k] is None else torch.as_tensor(c[k])
        good, bad = so.merge(t("z"), t("sdf"), t("new_z"), t("new_sdf")), so.merge(t("z"), t("sdf"), t("new_z"), t("new_sdf"), defect="new_before_equal_old")
        assert torch.equal(good[0], bad[0])
        if c["sdf"] is not None and c["M"] > 1:
            assert not torch.equal(good[1], bad[1]), n


def test_cdf_residual_and_classify_on_known_rows():
    z = torch.tensor([[0.0, 1.0, 1.0, 2.0, 4.0]], dtype=torch.float64)
    w = torch.tensor([[0.5, 0.25, 0.125, 0.125]], dtype=torch.float64) - 1e-5
    u = torch.tensor([0.25, 0.6, 0.8125], dtype=torch.float64)
    st = so.upsample_stages(None, None, z, None, u, 64.0, weights=w)
    assert torch.allclose(st["cdf"], torch.tensor([[0.0, 0.5, 0.75, 0.875, 1.0]], dtype=torch.float64), atol=1e-15)
    assert torch.allclose(st["new_z"], torch.tensor([[0.5, 1.0, 1.5]], dtype=torch.float64), atol=1e-12)
    assert float(so.cdf_residual(st, st["new_z"]).max()) < 1e-12
    # z = 1 is a tied knot pair: the CDF there is the interval [0.5, 0.75]
    res = so.cdf_residual(st, torch.tensor([[1.0, 1.0, 1.0]], dtype=torch.float64))
    assert torch.allclose(res, torch.tensor([[0.25, 0.0, 0.0625]], dtype=torch.float64), atol=1e-12)
    assert torch.isinf(so.cdf_residual(st, torch.tensor([[-0.1, 4.5, float("nan")]], dtype=torch.float64))).all()
    sens, cand = so.classify(st, 1e-3)
    assert sens.tolist() == [[False, False, False]]
    sens, cand = so.classify(st, 0.07)                  # 0.8125 is within 0.07 of the knot 0.875 (and of 0.75)
    assert sens.tolist() == [[False, False, True]] and cand.shape == (1, 3, 6)
    assert float((cand[0, 2] - 1.5).abs().min()) < 1e-12
