"""Mesh alignment on the device: vdn_icp_round as an operator (vdn_hip.nn.IcpRound), the loop (vdn_hip.nn.icp) and the public layer
(vdn_train.mesh_align.align_mesh, evaluate_mesh(align=...)) against the float64 numpy model of tests/align_model.py on the same
fp32 inputs. The model's own properties on these cases are asserted in tests/test_mesh_align_cpu.py and again where a check here
leans on them.

Tolerances.
- dist / idx: bit-equal to PointGrid.query(y, max_dist) with y formed on the host by the documented expression (the kernel shares
  vdn_nn_query's search); the hit set equal to the brute-force one, every case asserting on CPU values that no brute-force distance
  lies within 1e-5 relative of max_dist; the fp64 distance to ref[idx] equal to the brute-force minimum within rtol 1e-6 (the
  bound of test_gpu_mesh_eval.py: ties are legal, so idx itself is not compared with the argmin).
- the 19 sums: within 1e-13 x sum |terms| of the exact sum (math.fsum) of the model's terms over the device's pairs. Every term is
  exact in double (products of widened fp32 values; the three-term sums round twice, identically in the model), so only the
  additions of the reduction round: at most N <= 1 650 of them on any path, each 2^-53 relative to a partial sum that is at most
  sum |terms|: 1.8e-13 at the very worst, and the tree's depth (6 butterfly steps, 3 wave adds, the blocks) makes it about 1e-15.
  The pair count is exact. Two calls give identical bits.
- the loop: R, t within 1e-5 absolute and s within 1e-5 relative of the truth: the fp32 rounding of y and of the stored source is
  2^-24 = 6e-8 of a coordinate <= 1, two orders of magnitude below the bound, and any defect is far above it.
- trim: the thresholds are fp32 distances on the device and fp64 ones in the model: rtol 1e-6."""
import math

import numpy as np
import pytest
import torch

import align_model as am

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CELLS = (None, 1.0 / 60, 5.0)              # default; small: most cells empty, several shells; one cell


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_round(src, ref, M, max_dist, grid, order="cell", expect_all_miss=False):
    """One vdn_icp_round on src against `grid` of ref at M, checked against the model -> (dist, idx, sums) of the device."""
    from vdn_hip import nn
    r = am.round_model(src, ref, M, max_dist)
    assert am.clear_of(r["dist"], max_dist)
    tsrc, y = dev(src), dev(r["y"])
    op = nn.IcpRound(tsrc, grid, order=nn.query_order(grid, y) if order == "cell" else None, with_dist=True, with_idx=True)
    sums = op(M, max_dist).clone()
    dist, idx = op.dist.clone(), op.idx.clone()
    op.dist.fill_(-7.0)
    op.idx.fill_(-7)
    op.partials.fill_(float("nan"))                         # (the workspace need not be initialised)
    again = op(M, max_dist)
    assert torch.equal(again, sums) and torch.equal(op.dist, dist) and torch.equal(op.idx, idx)          # bit-identical
    qd, qi = grid.query(y, max_dist)
    assert torch.equal(dist, qd) and torch.equal(idx, qi)
    d, i, x = dist.cpu().numpy(), idx.cpu().numpy(), sums.cpu().numpy()
    hit = r["hit"]
    assert np.array_equal(np.isfinite(d), hit) and np.array_equal(i >= 0, hit) and np.array_equal(i == -1, ~hit) and np.isinf(d[~hit]).all()
    assert x[am.S_N] == hit.sum()
    if expect_all_miss:
        assert not hit.any() and (x == 0.0).all() and not np.signbit(x).any()
        return dist, idx, x
    assert hit.any() and ((i[hit] >= 0) & (i[hit] < ref.shape[0])).all()
    bf = r["dist"][hit]
    assert (np.abs(d[hit].astype(np.float64) - bf) <= 1e-6 * bf).all()
    own = np.sqrt(((r["y"][hit].astype(np.float64) - ref[i[hit]].astype(np.float64)) ** 2).sum(1))
    assert (np.abs(own - bf) <= 1e-6 * bf).all()
    T = am.pair_terms(src[hit], ref[i[hit]], r["y"][hit])
    want = np.array([math.fsum(T[:, j]) for j in range(am.N_SUMS)])
    mag = np.array([math.fsum(np.abs(T[:, j])) for j in range(am.N_SUMS)])
    err = np.abs(x - want)
    print("worst sum error / sum|terms| %.3g over %d pairs" % (float((err / np.maximum(mag, 1e-300)).max()), int(hit.sum())))
    assert (err <= 1e-13 * mag).all(), (err / np.maximum(mag, 1e-300)).max()
    return dist, idx, x


# ---- 1. one round as an operator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", ["initial", "converged"])
def test_one_round_matches_the_model_at_every_cell_size(at):
    from vdn_hip import nn
    c = am.case("rigid")
    if at == "initial":
        M = am.matrix(1.0, np.eye(3), np.zeros(3))
    else:
        m = am.case_model("rigid", 1e-10)
        assert m["converged"]
        M = am.matrix(m["s"], m["R"], m["t"])
    tref = dev(c["ref"])
    results, cells = [], []
    for h in CELLS:
        grid = nn.PointGrid(tref, cell_size=h)
        cells.append(grid.n_cells)
        results.append(check_round(c["src"], c["ref"], M, c["max_dist"], grid))
    assert cells[2] == 1 and cells[1] > 4 * c["ref"].shape[0]
    for dist, idx, x in results[1:]:
        assert torch.equal(dist, results[0][0]) and torch.equal(idx, results[0][1])
        # the sums: the same pairs, visited in another order - equal within the bound, the count exactly
        assert x[am.S_N] == results[0][2][am.S_N] == 1500
    if at == "converged":
        assert results[0][2][am.S_RES] / 1500 <= 1e-12               # rms <= 1e-6: the source sits on its matches


# ---- 2. block and wave edges ------------------------------------------------------------------------------------------------------
def _shuffled(name="rigid"):
    c = am.case(name)
    perm = np.random.default_rng(5).permutation(c["src"].shape[0])       # inliers and outliers mixed
    return c, c["src"][perm]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_source_counts_at_the_wave_and_block_edges(n):
    from vdn_hip import nn
    c, src = _shuffled()
    src = src[:n] if n > 1 else c["src"][:1]                             # (the single point is an inlier: a hit)
    grid = nn.PointGrid(dev(c["ref"]))
    M = am.matrix(1.0, np.eye(3), np.zeros(3))
    a = check_round(src, c["ref"], M, c["max_dist"], grid)
    if n in (65, 257):                                                   # the caller's own order
        b = check_round(src, c["ref"], M, c["max_dist"], grid, order=None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2][am.S_N] == b[2][am.S_N]


def test_a_round_that_matches_nothing_gives_zeros_and_icp_raises():
    from vdn_hip import nn
    c, src = _shuffled()
    src = src[:300]
    d = am.brute(src, c["ref"])[0]
    tiny = 1e-6
    assert d.min() > tiny * (1.0 + 1e-5)
    tref = dev(c["ref"])
    check_round(src, c["ref"], am.matrix(1.0, np.eye(3), np.zeros(3)), tiny, nn.PointGrid(tref), expect_all_miss=True)
    with pytest.raises(ValueError, match="max_dist"):
        nn.icp(dev(src), tref, max_dist=tiny)
    for bad in (lambda: nn.icp(dev(src), tref, max_dist=-1.0), lambda: nn.icp(dev(src), tref, max_dist=0.1, trim=0.0),
                lambda: nn.icp(dev(src), tref, max_dist=0.1, trim=1.5), lambda: nn.icp(dev(src)[:0], tref, max_dist=0.1),
                lambda: nn.icp(dev(src), tref, max_dist=0.1, max_rounds=0),
                lambda: nn.IcpRound(dev(src), nn.PointGrid(tref), order=torch.zeros(300, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            bad()


# ---- 3. the loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(am.CASES))
def test_icp_recovers_the_transform(name):
    from vdn_hip import nn
    c = am.case(name)
    m = am.case_model(name, 1e-7)
    assert m["converged"] and all(n == 1500 for n in m["n_pairs"]) and max(am.pose_error(m, c["truth"])) <= 1e-6
    assert all(am.clear_of(d, c["max_dist"]) for d in m["dists"])
    res = nn.icp(dev(c["src"]), dev(c["ref"]), max_dist=c["max_dist"], scale=c["scale"], max_rounds=60, tol=1e-7)
    eR, et, es = am.pose_error(res, c["truth"])
    print(name, "rounds", res["rounds"], "(model %d)" % m["rounds"], "errors", eR, et, es, "rms", res["rms"][-1])
    assert res["converged"] and res["rounds"] <= 60
    assert res["n_pairs"][-1] == 1500 and res["n_pairs"] == m["n_pairs"]
    assert eR <= 1e-5 and et <= 1e-5 and es <= 1e-5
    assert c["scale"] or res["s"] == 1.0
    assert res["threshold"] == [c["max_dist"]] * res["rounds"] and len(res["rms"]) == res["rounds"]
    assert np.allclose(res["rms"], m["rms"], rtol=1e-4, atol=1e-7)
    assert res["matrix"].shape == (4, 4) and np.array_equal(res["matrix"][:3, :3], res["s"] * res["R"]) and np.array_equal(res["matrix"][:3, 3], res["t"])
    assert abs(np.linalg.det(res["R"]) - 1.0) <= 1e-12
    # from the truth: one round to see that nothing moves
    again = nn.icp(dev(c["src"]), nn.PointGrid(dev(c["ref"])), init=c["truth"], max_dist=c["max_dist"], scale=c["scale"], tol=1e-6)
    assert again["converged"] and again["rounds"] == 1 and again["n_pairs"] == [1500]


# ---- 4. trimming ------------------------------------------------------------------------------------------------------------------
def _inlier_error(c, res):
    """RMS distance of the 1 500 inliers from where the truth puts them"""
    p, q = c["src"][:1500].astype(np.float64), c["ref"][c["pick"]].astype(np.float64)
    return float(np.sqrt((((res["s"] * p @ res["R"].T + res["t"]) - q) ** 2).sum(1).mean()))


def test_trimmed_icp_rejects_near_outliers():
    from vdn_hip import nn
    c = am.case("rigid", near_outliers=True)
    plain_m = am.case_model("rigid", 1e-7, 100, True, None)
    trim_m = am.case_model("rigid", 1e-7, 100, True, 0.9)
    assert plain_m["n_pairs"][0] > 1500                                          # some outliers ARE within max_dist
    assert _inlier_error(c, trim_m) < _inlier_error(c, plain_m)                  # the model shows the effect first
    assert all(am.clear_of(d, t) for d, t in zip(trim_m["dists"][:3], trim_m["threshold"][:3]))
    tsrc, tref = dev(c["src"]), dev(c["ref"])
    plain = nn.icp(tsrc, tref, max_dist=c["max_dist"], max_rounds=100, tol=1e-7)
    trim = nn.icp(tsrc, tref, max_dist=c["max_dist"], max_rounds=100, tol=1e-7, trim=0.9)
    print("thresholds", trim["threshold"][:3], "model", trim_m["threshold"][:3], "errors", _inlier_error(c, trim), _inlier_error(c, plain))
    assert trim["threshold"][0] == c["max_dist"] and trim["rounds"] >= 3
    assert np.allclose(trim["threshold"][:3], trim_m["threshold"][:3], rtol=1e-6, atol=0.0)
    assert trim["n_pairs"][:3] == trim_m["n_pairs"][:3]
    assert all(t <= c["max_dist"] for t in trim["threshold"])
    assert _inlier_error(c, trim) < _inlier_error(c, plain)
    assert trim["converged"] and plain["converged"]


# ---- 5. the public layer ----------------------------------------------------------------------------------------------------------
def test_align_mesh_and_evaluate_mesh_with_align():
    from vdn_hip import mesh
    from vdn_train import mesh_align, mesh_eval
    v, f = am.lobed_icosphere(3)
    R, t = am.rotation((1.0, 2.0, 3.0), 5.0), np.array([0.03, -0.015, 0.02])
    moved = (v.astype(np.float64) @ R.T + t).astype(np.float32)                  # the mesh, displaced
    back = (1.0, R.T, -R.T @ t)                                                  # what alignment should find
    spacing, max_dist = 0.02, 0.15
    tv, tm, tf = dev(v), dev(moved), dev(f)
    gt = mesh.sample_surface(tv, tf, spacing)[0]
    res = mesh_align.align_mesh(tm, tf, gt, spacing, max_dist, max_rounds=80)
    eR, et, es = am.pose_error(res, back)
    print("align_mesh rounds", res["rounds"], "errors", eR, et, "rms", res["rms"][0], res["rms"][-1], "samples", res["n_samples"])
    assert res["converged"] and eR <= 1e-5 and et <= 1e-5 and res["s"] == 1.0
    assert res["vertices"].dtype == torch.float32 and res["vertices"].shape == tm.shape
    assert float((res["vertices"] - tv).abs().max()) <= 1e-5
    plain = mesh_eval.evaluate_mesh(tm, tf, gt, spacing, max_dist)
    assert "align" not in plain and set(plain) == {"n_mesh_samples", "n_gt", "accuracy", "n_accuracy_used", "completeness",
                                                   "n_completeness_used", "chamfer", "precision", "recall", "fscore"}
    icp_ed = mesh_eval.evaluate_mesh(tm, tf, gt, spacing, max_dist, align={"max_rounds": 80})
    given = mesh_eval.evaluate_mesh(tm, tf, gt, spacing, max_dist, align=back)
    print("chamfer", plain["chamfer"], "aligned by icp", icp_ed["chamfer"], "by the known motion", given["chamfer"])
    for out in (icp_ed, given):
        assert set(out) == set(plain) | {"align"} and out["chamfer"] < 0.1 * plain["chamfer"]
        assert np.abs(np.array(out["align"]["R"]) - R.T).max() <= 1e-5 and np.abs(np.array(out["align"]["t"]) + R.T @ t).max() <= 1e-5
        mesh_eval.to_json(out)
    assert icp_ed["align"]["converged"] and icp_ed["align"]["n_pairs"] == res["n_pairs"][-1] and "rounds" not in given["align"]
    # a PointGrid built before, a start from the known motion, thinning on the way
    from vdn_hip import nn
    res2 = mesh_align.align_mesh(tm, tf, nn.PointGrid(gt), spacing, max_dist, init=back, thin=spacing)
    assert res2["converged"] and res2["rounds"] <= 3 and res2["n_samples"] < res["n_samples"]
    for bad in (lambda: mesh_align.align_mesh(tm, tf, gt, 0.0, max_dist), lambda: mesh_align.align_mesh(tm, tf, gt, spacing, max_dist, colour=1)):
        with pytest.raises((ValueError, TypeError)):
            bad()
