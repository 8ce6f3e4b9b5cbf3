"""The DTU steps of mesh evaluation on the device: vdn_hip.nn.thin_points (vdn_thin_round) against the sequential numpy loop of its
definition, and evaluate_mesh with thin / obs_mask / plane against a float64 numpy restatement.

Thinning: the masks must be EQUAL. That is fair because every case first asserts, in float64 on the CPU, that no pair of points
lies within 1e-5 relative of `radius` (fp32 rounds a squared distance by some 2e-7 relative): then every `<=` has one answer, and the
definition has one result. Every case runs at three cell sizes (default; the minimum radius + margin; one cell for everything) whose
masks must be bit-identical, and is checked independently of the reference too: kept points are pairwise more than `radius` apart,
every removed point has a kept lower-index neighbour within `radius`.
The number of rounds is never compared between two calls: it may differ from run to run, the mask may not.
Pipeline: counts exact, means rtol 1e-5 (the metrics' tolerance of test_gpu_mesh_eval.py: both sides use the same fp32 points, the
device's distances are off by a few 2^-24)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CACHE = {}


# ---- numpy references ---------------------------------------------------------------------------------------------------------
def greedy(p, radius):
    """the definition, as a loop: fp32 difference form, inclusive"""
    p = np.asarray(p, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    keep = np.ones(len(p), bool)
    for i in range(len(p)):
        if keep[i]:
            d = p - p[i]
            near = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2
            near[i] = False
            keep[near] = False
    return keep


def pair_d2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d2 = np.zeros((len(a), len(b)))
    for k in range(3):
        d2 += (a[:, k:k + 1] - b[None, :, k]) ** 2
    return d2


def pairs_near_radius(p, radius):
    """(pairs i < j with distance within 1e-5 relative of radius, pairs within radius), float64, in row blocks"""
    near = within = 0
    for s in range(0, len(p), 512):
        d = np.sqrt(pair_d2(p[s:s + 512], p))
        upper = np.arange(len(p))[None, :] > np.arange(s, min(s + 512, len(p)))[:, None]
        near += int((upper & (np.abs(d - radius) <= 1e-5 * radius)).sum())
        within += int((upper & (d <= radius)).sum())
    return near, within


def sphere_points(rng, n, radius):
    d = rng.normal(size=(n, 3))
    return (radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def with_duplicates(rng, p, n):
    q = np.concatenate([p, p[rng.integers(0, len(p), size=n)]])
    return q[rng.permutation(len(q))]


def thin_case(name):
    """-> (points [N,3] fp32, radius)"""
    rng = np.random.default_rng(0)
    if name == "sphere":
        return sphere_points(rng, 3000, 0.5), 0.03
    if name == "cube":
        return rng.uniform(size=(3000, 3)).astype(np.float32), 0.05
    if name in ("sphere_duplicates", "cube_duplicates"):
        p, r = thin_case(name.split("_")[0])
        return with_duplicates(np.random.default_rng(1), p, 700), r
    if name == "line":                                   # in index order: point i waits for point i - 1, about N / 2 rounds
        p = np.zeros((200, 3), np.float32)
        p[:, 0] = np.arange(200) * 0.6
        return p, 1.0
    if name == "coplanar":                               # one cell thick
        p = np.random.default_rng(3).uniform(size=(2000, 3)).astype(np.float32)         # (seed 2 has a pair within 1e-5 of the radius)
        p[:, 2] = 0.25
        return p, 0.03
    if name == "radius_beyond_the_box":
        return rng.uniform(size=(500, 3)).astype(np.float32), 2.0
    if name == "radius_below_every_gap":
        p = rng.uniform(size=(500, 3)).astype(np.float32)
        d2 = pair_d2(p, p) + np.eye(500) * 10.0
        return p, 0.5 * float(np.sqrt(d2.min()))
    if name.startswith("count_"):
        return rng.uniform(size=(485, 3)).astype(np.float32)[:int(name[6:])], 0.15
    raise KeyError(name)


THIN_CASES = ["sphere", "cube", "sphere_duplicates", "cube_duplicates", "line", "coplanar", "radius_beyond_the_box", "radius_below_every_gap",
              "count_1", "count_63", "count_64", "count_65", "count_485"]


def thin_reference(name):
    if name not in _CACHE:
        p, radius = thin_case(name)
        _CACHE[name] = (p, radius, greedy(p, radius), pairs_near_radius(p, radius))
    return _CACHE[name]


def check_independent(p, radius, keep):
    k = np.flatnonzero(keep)
    d = np.sqrt(pair_d2(p[k], p[k])) + np.eye(len(k)) * 1e30
    assert (d > radius).all()                                     # kept points are pairwise more than radius apart
    gone = np.flatnonzero(~keep)
    if len(gone):
        d = np.sqrt(pair_d2(p[gone], p[k]))
        lower = k[None, :] < gone[:, None]
        assert ((d <= radius) & lower).any(1).all()               # every removed point has a kept lower-index neighbour within it


@pytest.mark.parametrize("name", THIN_CASES)
def test_thin_points_equals_the_sequential_loop_at_every_cell_size(name):
    from vdn_hip import nn
    p, radius, want, (near, within) = thin_reference(name)
    print("%s: %d points, %d pairs within the radius, %d near it, the loop keeps %d" % (name, len(p), within, near, int(want.sum())))
    assert near == 0                                              # what makes exact equality fair
    tp = torch.from_numpy(p).to(DEV)
    extent = float((p.max(0) - p.min(0)).max())
    masks, rounds = [], []
    for cell_size in (None, 0.5 * radius, 10.0 * (extent + radius)):
        keep, n = nn.thin_points(tp, radius, cell_size=cell_size, return_rounds=True)
        assert keep.dtype == torch.bool and keep.shape == (len(p),) and keep.device == tp.device and isinstance(n, int) and n >= 1
        masks.append(keep.cpu().numpy())
        rounds.append(n)
    print("rounds", rounds)
    assert np.array_equal(masks[0], want), (int(masks[0].sum()), int(want.sum()))
    assert np.array_equal(masks[1], masks[0]) and np.array_equal(masks[2], masks[0])
    assert torch.equal(nn.thin_points(tp, radius), torch.from_numpy(masks[0]).to(DEV))        # without return_rounds: the mask alone
    check_independent(p, radius, masks[0])
    if name in ("sphere", "cube"):
        assert 0.3 * len(p) < want.sum() < 0.7 * len(p)           # both outcomes are exercised
    if name.endswith("duplicates"):
        first = {}
        for i, key in enumerate(map(bytes, p)):
            first.setdefault(key, i)
        assert not any(masks[0][i] for i, key in enumerate(map(bytes, p)) if first[key] != i)      # of equal points the later one goes
    if name == "line":
        assert np.array_equal(masks[0], np.arange(200) % 2 == 0) and min(rounds) >= 50
    if name == "radius_beyond_the_box":
        assert masks[0].tolist() == [True] + [False] * 499
    if name == "radius_below_every_gap":
        assert masks[0].all() and rounds == [1, 1, 1]


def test_thin_points_order_empty_cloud_and_argument_errors():
    from vdn_hip import nn
    p, radius, want, _ = thin_reference("cube")
    tp = torch.from_numpy(p).to(DEV)
    # another visiting order is the caller's permutation: the loop on the permuted cloud
    perm = np.random.default_rng(3).permutation(len(p))
    got = nn.thin_points(tp[torch.from_numpy(perm).to(DEV)], radius).cpu().numpy()
    assert np.array_equal(got, greedy(p[perm], radius)) and not np.array_equal(got, want[perm])
    # float64 points are taken as their fp32 roundings
    assert np.array_equal(nn.thin_points(tp.double(), radius).cpu().numpy(), want)
    keep, rounds = nn.thin_points(torch.zeros(0, 3, device=DEV), 0.1, return_rounds=True)
    assert keep.shape == (0,) and keep.dtype == torch.bool and rounds == 0
    bad = tp.clone()
    bad[7, 1] = float("nan")
    inf = tp.clone()
    inf[0, 0] = float("inf")
    for call in (lambda: nn.thin_points(torch.from_numpy(p), radius), lambda: nn.thin_points(tp[:, :2], radius), lambda: nn.thin_points(tp.reshape(-1), radius),
                 lambda: nn.thin_points(bad, radius), lambda: nn.thin_points(inf, radius), lambda: nn.thin_points(tp, 0.0),
                 lambda: nn.thin_points(tp, -1.0), lambda: nn.thin_points(tp, float("nan")), lambda: nn.thin_points(tp, float("inf")), lambda: nn.thin_points(tp, 1e39),
                 lambda: nn.thin_points(tp, radius, cell_size=0.0), lambda: nn.thin_points(tp, radius, max_cells=0)):
        with pytest.raises(ValueError):
            call()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


def nearest_d(q, ref):
    """float64 distance of every query to its nearest reference point, in row blocks"""
    return np.concatenate([np.sqrt(pair_d2(q[s:s + 512], ref).min(1)) for s in range(0, len(q), 512)]) if len(q) else np.zeros(0)


def clear_of(d, *levels):
    return all((np.abs(d - t) > 1e-5 * t).all() for t in levels)


SPACING, THIN, MAX_DIST, THRESHOLDS, PATCH = 0.02, 0.03, 0.1, (0.025, 0.04), 0.05
BB = np.float32([[-0.45, -0.6, -0.6], [0.3, 0.6, 0.6]])
RES = 0.0375
PLANE = (0.1, 0.0, 1.0, 0.2)


def obs_mask_array():
    m = np.zeros((32, 32, 32), bool)
    m[10:] = True                                              # the half-space x >= bb[0].x + 9.5 res = -0.09375 was observed
    return m


def pipeline_inputs():
    if "pipeline" not in _CACHE:
        v, f = icosphere(2, 0.5)
        gt = sphere_points(np.random.default_rng(7), 3000, 0.52)
        _CACHE["pipeline"] = (v, f, gt)
    return _CACHE["pipeline"]


def np_pipeline(samples, gt):
    """evaluate_mesh's documented pipeline on the device's own sample points: thinning by the loop, the two filters by their formulas (fp32 where
    the contract says fp32), distances and means in float64"""
    near, _ = pairs_near_radius(samples, THIN)
    assert near == 0
    keep = greedy(samples, THIN)
    s = samples[keep]
    t = (s.astype(np.float64) - BB[0].astype(np.float64)) / RES
    assert np.abs(t - np.floor(t) - 0.5).min() > 1e-4          # no voxel index hinges on rounding
    lo, hi = BB[0] - np.float32(PATCH), BB[1] + np.float32(2.0) * np.float32(PATCH)
    assert np.abs(s - lo).min() > 1e-6 and np.abs(s - hi).min() > 1e-6
    inbound = (s >= lo).all(1) & (s < hi).all(1)
    g = np.rint((s - BB[0]) / np.float32(RES))
    mask = obs_mask_array()
    inside = ((g >= 0) & (g < 32)).all(1)
    gi = np.where(inside[:, None], g, 0).astype(np.int64)
    observed = inbound & inside & mask[gi[:, 0], gi[:, 1], gi[:, 2]]
    pv = PLANE[0] * gt[:, 0].astype(np.float64) + PLANE[1] * gt[:, 1].astype(np.float64) + PLANE[2] * gt[:, 2].astype(np.float64) + PLANE[3]
    assert np.abs(pv).min() > 1e-9
    above = pv > 0
    d_acc, d_comp = nearest_d(s[observed], gt), nearest_d(gt[above], s[inbound])
    assert clear_of(d_acc, MAX_DIST, *THRESHOLDS) and clear_of(d_comp, MAX_DIST, *THRESHOLDS)
    out = {"n_mesh_samples": int(keep.sum()), "n_gt": len(gt), "n_thinned": int((~keep).sum()), "n_inbound": int(inbound.sum()),
           "n_observed": int(observed.sum()), "n_gt_above_plane": int(above.sum()), "precision": {}, "recall": {}, "fscore": {}}
    for key, d in (("accuracy", d_acc), ("completeness", d_comp)):
        used = d <= MAX_DIST
        out["n_%s_used" % key] = int(used.sum())
        out[key] = float(d[used].mean())
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for t in THRESHOLDS:
        p, r = float((d_acc <= t).sum()) / len(d_acc), float((d_comp <= t).sum()) / len(d_comp)
        out["precision"][t], out["recall"][t], out["fscore"][t] = p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


OLD_KEYS = {"n_mesh_samples", "n_gt", "accuracy", "n_accuracy_used", "completeness", "n_completeness_used", "chamfer", "precision", "recall",
            "fscore"}
NEW_KEYS = {"n_thinned", "thin_rounds", "n_inbound", "n_observed", "n_gt_above_plane"}


def without_rounds(result):
    """thin_rounds may differ between two calls on the same input (what a lane sees of another wave's stores inside a round is a
    matter of timing); every other entry may not"""
    return {k: v for k, v in result.items() if k != "thin_rounds"}


def check_pipeline(got, want):
    assert set(got) == OLD_KEYS | NEW_KEYS
    for k in ("n_mesh_samples", "n_gt", "n_thinned", "n_inbound", "n_observed", "n_gt_above_plane", "n_accuracy_used", "n_completeness_used"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("accuracy", "completeness", "chamfer"):
        print(k, got[k], want[k], abs(got[k] - want[k]) / abs(want[k]))
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    for t in THRESHOLDS:
        assert got["precision"][t] == want["precision"][t] and got["recall"][t] == want["recall"][t]
        assert abs(got["fscore"][t] - want["fscore"][t]) <= 1e-12


def test_evaluate_mesh_with_the_dtu_steps_matches_the_numpy_restatement():
    from vdn_hip import mesh
    from vdn_train import mesh_eval
    v, f, gt = pipeline_inputs()
    tv, tf, tg = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV)
    samples = mesh.sample_surface(tv, tf, SPACING)[0].cpu().numpy()
    want = np_pipeline(samples, gt)
    print(want)
    # every step bites, and the two sample sets differ
    assert 0 < want["n_observed"] < want["n_inbound"] < want["n_mesh_samples"] < len(samples) and 0 < want["n_gt_above_plane"] < want["n_gt"]
    assert want["n_accuracy_used"] == want["n_observed"] and 0 < want["n_completeness_used"] < want["n_gt_above_plane"]
    got = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, thin=THIN, obs_mask=(obs_mask_array(), BB, RES), patch=PATCH,
                                  plane=PLANE)
    print(got)
    check_pipeline(got, want)
    assert got["thin_rounds"] >= 2
    # tensors on the device in place of arrays
    dev = lambda x: torch.from_numpy(np.asarray(x)).to(DEV)
    again = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, thin=THIN, obs_mask=(dev(obs_mask_array().astype(np.uint8)), dev(BB), RES),
                                    patch=PATCH, plane=dev(np.float64(PLANE)))
    assert without_rounds(again) == without_rounds(got) and again["thin_rounds"] >= 1
    # without the new arguments: today's keys, and each argument alone adds the five new ones
    plain = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS)
    assert set(plain) == OLD_KEYS and plain["n_mesh_samples"] == len(samples)
    assert plain == mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, patch=1.0)      # patch alone is no step
    only_plane = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, plane=PLANE)
    assert set(only_plane) == OLD_KEYS | NEW_KEYS and only_plane["accuracy"] == plain["accuracy"] and only_plane["thin_rounds"] == 0
    assert only_plane["n_thinned"] == 0 and only_plane["n_inbound"] == only_plane["n_observed"] == len(samples)
    assert only_plane["n_gt_above_plane"] == want["n_gt_above_plane"]
    only_thin = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, thin=THIN)
    assert only_thin["n_mesh_samples"] == only_thin["n_inbound"] == only_thin["n_observed"] == want["n_mesh_samples"]
    assert only_thin["n_gt_above_plane"] == len(gt)
    # a filter that leaves a side empty
    for kw in (dict(plane=(0.0, 0.0, 1.0, -5.0)), dict(obs_mask=(np.zeros((32, 32, 32), bool), BB, RES)),
               dict(obs_mask=(obs_mask_array(), BB + np.float32(50.0), RES), patch=PATCH)):
        with pytest.raises(ValueError):
            mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, **kw)
    with pytest.raises(ValueError):
        mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, obs_mask=obs_mask_array())


def edge_bound(level, radius):
    """an upper bound on every edge (chord) of icosphere(level, radius). The icosahedron's edges span the angle atan(2). One
    subdivision: a new edge is half an old arc, or joins two arc midpoints - in the plane that segment is half the third edge, and
    pushing its ends out to the sphere from a distance of at least radius cos(theta / 2) stretches it by at most 1 / cos(theta / 2);
    that bound covers the half arcs too (2 r sin(theta / 4) = (e / 2) / cos(theta / 4))."""
    e = 2.0 * radius * math.sin(0.5 * math.atan(2.0))
    for _ in range(level):
        theta = 2.0 * math.asin(e / (2.0 * radius))
        e = 0.5 * e / math.cos(0.5 * theta)
    return e


def test_evaluate_mesh_dtu_analytic_anchor():
    """Concentric spheres: an icosphere of level 4 and radius r = 0.5 as the mesh, the vertices of one of level 5 and radius R = 0.55
    as the cloud, all filters open. A point of a flat facet with corners on the sphere and edges <= e is
    sum w_i v_i with |.|^2 = r^2 - sum_{i<j} w_i w_j |v_i - v_j|^2 >= r^2 - e^2 / 3: the facet sags by at most r - sqrt(r^2 - e^2 / 3),
    and it is within (1 - max w) e <= 2 e / 3 of its corner of largest weight. So every distance is at least R - r; a mesh sample s
    finds, along its own direction, the cloud's facet point q within R - |s| and a cloud vertex within 2 e_R / 3 of q; a cloud point
    finds along its direction the mesh's facet point within R - r + sag, a sample of that facet (each has at least one) within e_r,
    and a kept sample within `thin` of that."""
    from vdn_train import mesh_eval
    r, R, spacing, thin = 0.5, 0.55, 0.02, 0.02
    v, f = icosphere(4, r)
    gt = icosphere(5, R)[0]
    e_r, e_R = edge_bound(4, r), edge_bound(5, R)
    edges = np.linalg.norm(v[f].astype(np.float64) - v[np.roll(f, 1, axis=1)].astype(np.float64), axis=2)
    assert 0.8 * e_r < edges.max() <= e_r * (1 + 1e-6)         # the bound holds on this mesh, and is not slack
    sag = r - math.sqrt(r * r - e_r * e_r / 3.0)
    mask, bb = np.ones((4, 4, 4), bool), np.float32([[-1, -1, -1], [1, 1, 1]])
    out = mesh_eval.evaluate_mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV), spacing, 0.2, (0.1,),
                                  thin=thin, obs_mask=(mask, bb, 0.5), patch=1.0, plane=(0.0, 0.0, 1.0, 5.0))
    print(out, "sag", sag, "e_r", e_r, "e_R", e_R)
    lo = (R - r) * (1 - 1e-5)
    assert lo <= out["accuracy"] <= R - r + sag + 2.0 * e_R / 3.0
    assert lo <= out["completeness"] <= R - r + sag + e_r + thin
    assert out["n_thinned"] > 0 and out["n_inbound"] == out["n_observed"] == out["n_accuracy_used"] == out["n_mesh_samples"]
    assert out["n_gt_above_plane"] == out["n_completeness_used"] == out["n_gt"] == len(gt)
    assert out["precision"][0.1] == out["recall"][0.1] == out["fscore"][0.1] == 1.0


def test_evaluate_ply_round_trip_through_read_dtu_aux(tmp_path):
    from vdn_train import mesh_eval, meshio
    v, f, gt = pipeline_inputs()
    mesh_path = meshio.write_ply(str(tmp_path / "mesh.ply"), v, f)
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(gt)] + ["property float %s" % n for n in "xyz"] + ["end_header"]
    gt_path = str(tmp_path / "scan.ply")
    with open(gt_path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(gt.astype("<f4").tobytes())
    np.savez(tmp_path / "obs.npz", ObsMask=obs_mask_array(), BB=BB, Res=RES)
    np.savez(tmp_path / "plane.npz", P=np.float64(PLANE))
    from_files = mesh_eval.evaluate_ply(mesh_path, gt_path, SPACING, MAX_DIST, THRESHOLDS, device=DEV, thin=THIN, obs_mask=str(tmp_path / "obs.npz"),
                                        patch=PATCH, plane=str(tmp_path / "plane.npz"))
    tv, tf, tg = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV)
    in_memory = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS, thin=THIN, obs_mask=(obs_mask_array(), BB, RES), patch=PATCH,
                                        plane=PLANE)
    assert without_rounds(from_files) == without_rounds(in_memory) and set(from_files) == OLD_KEYS | NEW_KEYS and from_files["thin_rounds"] >= 1
    assert set(mesh_eval.evaluate_ply(mesh_path, gt_path, SPACING, MAX_DIST, THRESHOLDS, device=DEV)) == OLD_KEYS
    with pytest.raises(ValueError):                            # a file without the names that step needs
        mesh_eval.evaluate_ply(mesh_path, gt_path, SPACING, MAX_DIST, THRESHOLDS, device=DEV, obs_mask=str(tmp_path / "plane.npz"))
    with pytest.raises(ValueError):
        mesh_eval.evaluate_ply(mesh_path, gt_path, SPACING, MAX_DIST, THRESHOLDS, device=DEV, plane=str(tmp_path / "obs.npz"))
