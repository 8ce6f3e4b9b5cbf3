"""Mesh evaluation on the device: vdn_hip.mesh.sample_surface (vdn_surf_count / vdn_surf_emit), vdn_hip.nn.PointGrid
(vdn_nn_bin / vdn_nn_query) and vdn_train.mesh_eval against numpy restatements in float64 on the same fp32 inputs.

Tolerances. Nearest neighbour: both sides see the same fp32 inputs and the kernel uses the difference form sqrt(sum (q - r)^2), so a
distance is off by a few units of 2^-24: rtol 1e-6, NO absolute term (an exact hit is exactly 0). `idx` is not compared with the
brute-force argmin (ties are legal): it must be in range and the fp64 distance to ref[idx] must equal the brute-force minimum
within the same rtol. The +inf / -1 set must equal the brute-force one exactly; every case asserts on the CPU values that no
brute-force distance lies within 1e-5 relative of max_dist. Every case runs at three cell sizes (default; small: most cells empty,
several rings; one cell) whose results must agree bit for bit.
Sampling: counts within [ceil(r (1 - 1e-9)), ceil(r (1 + 1e-9))] of the fp64 ratio r = area / spacing^2, points within 1e-6 of the
bounding-box diagonal of the restatement, barycentrics >= -1e-6. Metrics: means rtol 1e-5, counts exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-6
A1, A2 = 0.7548776662466927, 0.5698402909980532


# ---- numpy references ---------------------------------------------------------------------------------------------------------
def brute(q, ref):
    """fp64 distance of every fp32 query to its nearest fp32 reference point, difference form -> (dist [Q], argmin [Q])."""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    d2 = np.zeros((q.shape[0], ref.shape[0]))
    for a in range(3):
        d2 += (q[:, a:a + 1] - ref[None, :, a]) ** 2
    i = d2.argmin(1) if q.shape[0] else np.zeros(0, np.int64)
    return np.sqrt(d2[np.arange(q.shape[0]), i]), i


def clear_of(d, *levels):
    """no distance within 1e-5 relative of a level (so a <= decision cannot hinge on fp32 rounding)"""
    return all((np.abs(d - t) > 1e-5 * t).all() for t in levels)


def rng_of(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(name):
    h = 1469598103934665603
    for c in name.encode():
        h = ((h ^ c) * 1099511628211) % (1 << 63)
    return h


def sphere_points(rng, n, radius):
    d = rng.normal(size=(n, 3))
    return (radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def nn_case(name):
    """-> (q [Q,3] fp32, ref [R,3] fp32, max_dist or None, cell sizes, max_cells)"""
    rng = rng_of(name)
    u = lambda *s: rng.uniform(size=s)
    if name == "cube":
        return u(3000, 3).astype(np.float32), u(2500, 3).astype(np.float32), None, (None, 1.0 / 40, 4.0), 1 << 24
    if name == "cube_max_dist":
        return u(3000, 3).astype(np.float32), u(2500, 3).astype(np.float32), 0.052, (None, 1.0 / 40, 4.0), 1 << 24
    if name == "sphere":
        return sphere_points(rng, 3000, 0.5), sphere_points(rng, 2500, 0.52), 0.03, (None, 1.0 / 60, 5.0), 1 << 24
    if name == "coplanar":
        ref = u(2500, 3).astype(np.float32)
        ref[:, 2] = 0.25
        return (u(1500, 3) * [1, 1, 0.5]).astype(np.float32), ref, 0.2, (None, 1.0 / 200, 4.0), 1 << 24
    if name == "identical":
        ref = np.tile(np.float32([0.3, -1.7, 2.9]), (200, 1))
        return (ref[:100] + rng.normal(size=(100, 3)) * 0.5).astype(np.float32), ref, None, (None, 1e-3, 10.0), 1 << 24
    if name == "single":
        ref = np.float32([[0.3, -1.7, 2.9]])
        q = np.concatenate([ref, (ref + rng.normal(size=(130, 3))).astype(np.float32)])
        return q, ref, 1.0, (None, 1e-3, 10.0), 1 << 24
    if name == "duplicates_and_hits":
        base = u(1200, 3).astype(np.float32)
        ref = np.concatenate([base, base[:700], base[:100]])[rng.permutation(2000)]
        return np.concatenate([ref[::3], u(500, 3).astype(np.float32)]), ref, None, (None, 1.0 / 40, 4.0), 1 << 24
    if name == "outside":
        ref = u(2500, 3).astype(np.float32)
        inside = u(400, 3)
        q = [inside]
        for axis in range(3):
            for side, far in ((-1, 0.07), (1, 0.07), (-1, 0.9), (1, 0.9), (-1, 30.0), (1, 30.0)):
                p = u(60, 3)
                p[:, axis] = (1.0 + far * u(60)) if side > 0 else (-far * u(60))
                q.append(p)
        q.append(u(200, 3) * 3 - 1)                  # off the corners and edges too
        return np.concatenate(q).astype(np.float32), ref, 0.5, (None, 1.0 / 40, 4.0), 1 << 24
    if name == "outside_unbounded":
        q, ref = nn_case("outside")[:2]
        return q[::5], ref, None, (None, 1.0 / 25, 4.0), 1 << 24
    if name == "elongated":
        ref = (u(2000, 3) * [1000.0, 1.0, 1.0]).astype(np.float32)
        q = (u(1500, 3) * [1100.0, 2.0, 2.0] - [50.0, 0.5, 0.5]).astype(np.float32)
        return q, ref, 3.0, (None, 1.0, 5000.0), 64
    raise KeyError(name)


NN_CASES = ["cube", "cube_max_dist", "sphere", "coplanar", "identical", "single", "duplicates_and_hits", "outside", "outside_unbounded",
            "elongated"]
_CACHE = {}


def nn_reference(name):
    if name not in _CACHE:
        q, ref, max_dist, sizes, max_cells = nn_case(name)
        _CACHE[name] = (q, ref, max_dist, sizes, max_cells) + brute(q, ref)
    return _CACHE[name]


def check_nn(q, ref, bf, dist, idx, max_dist):
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (q.shape[0],)
    far = bf > max_dist if max_dist is not None else np.zeros(len(bf), bool)
    assert np.array_equal(np.isinf(dist), far) and np.array_equal(idx == -1, far)
    near = ~far
    err = np.abs(dist[near].astype(np.float64) - bf[near])
    worst = float((err / np.maximum(bf[near], 1e-300)).max()) if near.any() else 0.0
    print("worst relative distance error %.3g over %d queries" % (worst, int(near.sum())))
    assert (err <= RTOL * bf[near]).all(), worst
    assert (dist[near][bf[near] == 0] == 0).all()
    i = idx[near]
    assert ((i >= 0) & (i < ref.shape[0])).all()
    d_own = np.sqrt(((q[near].astype(np.float64) - ref[i].astype(np.float64)) ** 2).sum(1))
    assert (np.abs(d_own - bf[near]) <= RTOL * bf[near]).all()


@pytest.mark.parametrize("name", NN_CASES)
def test_nearest_neighbour_matches_brute_force_at_every_cell_size(name):
    from vdn_hip import nn
    q, ref, max_dist, sizes, max_cells, bf, _ = nn_reference(name)
    if max_dist is not None:
        assert clear_of(bf, max_dist)
        assert (bf > max_dist).any() and (bf <= max_dist).any()
    tq, tr = torch.from_numpy(q).to(DEV), torch.from_numpy(ref).to(DEV)
    results, cells = [], []
    for h in sizes:
        grid = nn.PointGrid(tr, cell_size=h, max_cells=max_cells)
        assert grid.n_cells <= max_cells
        cells.append(grid.n_cells)
        dist, idx = grid.query(tq, max_dist)
        check_nn(q, ref, bf, dist, idx, max_dist)
        results.append((dist, idx))
    assert cells[2] == 1                                       # the large size is the one-cell grid
    if name not in ("identical", "single"):
        assert cells[1] > 4 * ref.shape[0] or name == "elongated"      # the small size leaves most cells empty
    if name == "elongated":
        assert nn.PointGrid(tr, cell_size=1.0, max_cells=max_cells).h > 1.0       # the clamp ran
    for dist, idx in results[1:]:
        assert torch.equal(dist, results[0][0]) and torch.equal(idx, results[0][1])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 7 + 37])
def test_nearest_neighbour_query_counts(n):
    from vdn_hip import nn
    q, ref, _, sizes, _, bf, _ = nn_reference("cube")
    tq, tr = torch.from_numpy(q[:n]).to(DEV), torch.from_numpy(ref).to(DEV)
    out = [nn.nearest(tq, tr, cell_size=h) for h in sizes]
    check_nn(q[:n], ref, bf[:n], out[0][0], out[0][1], None)
    for dist, idx in out[1:]:
        assert torch.equal(dist, out[0][0]) and torch.equal(idx, out[0][1])


def test_nearest_neighbour_empty_query_rings_and_argument_errors():
    from vdn_hip import nn
    q, ref, _, _, _, bf, _ = nn_reference("cube")
    tq, tr = torch.from_numpy(q).to(DEV), torch.from_numpy(ref).to(DEV)
    grid = nn.PointGrid(tr)
    dist, idx = grid.query(torch.zeros(0, 3, device=DEV))
    assert dist.shape == (0,) and idx.shape == (0,) and dist.dtype == torch.float32 and idx.dtype == torch.int64
    dist, idx, rings = grid.query(tq[:500], return_rings=True)
    check_nn(q[:500], ref, bf[:500], dist, idx, None)
    assert rings.dtype == torch.int32 and int(rings.min()) >= 1 and int(rings.max()) <= max(grid.dims)
    # max_dist = 0 keeps exact hits only
    dist, idx = grid.query(torch.cat([tr[:3], tq[:3]]), max_dist=0.0)
    assert dist.tolist() == [0.0, 0.0, 0.0] + [float("inf")] * 3 and idx[3:].tolist() == [-1, -1, -1]
    assert (tr[idx[:3]] == tr[:3]).all()
    for bad in (lambda: nn.PointGrid(torch.zeros(0, 3, device=DEV)), lambda: nn.PointGrid(torch.from_numpy(ref)),
                lambda: nn.PointGrid(tr[:, :2]), lambda: nn.PointGrid(tr.reshape(-1)), lambda: nn.PointGrid(tr, cell_size=0.0),
                lambda: grid.query(torch.from_numpy(q)), lambda: grid.query(tq[:, :2]), lambda: grid.query(tq, max_dist=-1.0),
                lambda: grid.query(tq, max_dist=float("nan")), lambda: nn.nearest(tq, torch.zeros(0, 3, device=DEV)),
                lambda: nn.PointGrid(torch.full((4, 3), float("nan"), device=DEV))):
        with pytest.raises(ValueError):
            bad()


# ---- surface sampling -----------------------------------------------------------------------------------------------------------
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


def sample_mesh(name):
    """-> (vertices [V,3] fp32, triangles [F,3] int64, spacing)"""
    if name == "square":
        return np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), np.int64([[0, 1, 2], [0, 2, 3]]), 0.07
    if name == "icosphere":
        v, f = icosphere(2)
        return v, f, 0.05
    if name == "lattice_sphere":
        from oracle import marching_cubes as mc
        g = np.arange(24, dtype=np.float64) - 11.5
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        v, f = mc.marching_cubes((8.3 - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 0.0)
        return v.astype(np.float32), f.astype(np.int64), 0.6
    if name == "degenerate_and_huge":
        v, f = icosphere(1, 0.5)                               # 80 triangles of area ~0.038
        n = len(v)
        extra = np.float32([[0, 0, 2], [1, 1, 2], [2, 2, 2],                 # collinear: zero area
                            [-14, -14, -3], [14, -14, -3], [0, 14, -3]])     # area 392: ~10^4 times the others
        v = np.concatenate([v, extra])
        f = np.concatenate([[[n, n + 1, n + 2]], f[:40], [[n + 3, n + 4, n + 5]], [[n, n, n]], f[40:], [[n + 2, n + 1, n]]])
        return v, f.astype(np.int64), 0.12
    raise KeyError(name)


def np_ratio(v, f, spacing):
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1) / (spacing * spacing)


def np_samples(v, f, counts):
    """the issue's formulas on the device's own counts -> (points [S,3] fp64, face [S])"""
    face = np.repeat(np.arange(len(f)), counts)
    off = np.cumsum(counts) - counts
    j1 = (np.arange(len(face)) - off[face] + 1).astype(np.float64)
    uu, vv = 0.5 + j1 * A1, 0.5 + j1 * A2
    uu, vv = uu - np.floor(uu), vv - np.floor(vv)
    fold = uu + vv > 1.0
    uu, vv = np.where(fold, 1.0 - uu, uu), np.where(fold, 1.0 - vv, vv)
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    return a + uu[:, None] * (b - a) + vv[:, None] * (c - a), face


def barycentrics(p, a, b, c):
    e1, e2, d = b - a, c - a, p - a
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    u, v = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    return np.stack([1.0 - u - v, u, v], 1)


@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", ["square", "icosphere", "lattice_sphere", "degenerate_and_huge"])
def test_sample_surface_matches_the_formulas(name, index_dtype):
    from vdn_hip import mesh
    v, f, spacing = sample_mesh(name)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV).to(index_dtype)
    points, face, counts = mesh.sample_surface(tv, tf, spacing)
    again = mesh.sample_surface(tv, tf, spacing)
    assert all(torch.equal(x, y) for x, y in zip((points, face, counts), again))              # no random state
    assert points.dtype == torch.float32 and face.dtype == torch.int32 and counts.dtype == torch.int32
    counts, points, face = counts.cpu().numpy().astype(np.int64), points.cpu().numpy(), face.cpu().numpy()
    r = np_ratio(v, f, spacing)
    assert np.isfinite(r).all()
    assert (counts >= np.ceil(r * (1 - 1e-9))).all() and (counts <= np.ceil(r * (1 + 1e-9))).all()
    if name == "square":
        assert counts.tolist() == [103, 103]                   # r = 102.04 per triangle
    if name == "degenerate_and_huge":
        assert counts[0] == 0 and counts[42] == 0 and counts[-1] == 0 and counts[41] > 5000 * np.median(counts)
    want, want_face = np_samples(v, f, counts)
    assert points.shape == want.shape and np.array_equal(face, want_face)
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    assert np.abs(points - want).max() <= 1e-6 * diag
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    assert barycentrics(points.astype(np.float64), a, b, c).min() >= -1e-6


def test_sample_surface_edges_and_argument_errors():
    from vdn_hip import mesh
    v, f, spacing = sample_mesh("icosphere")
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    points, face, counts = mesh.sample_surface(tv, tf[:0], spacing)
    assert points.shape == (0, 3) and face.shape == (0,) and counts.shape == (0,)
    total = int(mesh.sample_surface(tv, tf, spacing)[2].sum())
    assert mesh.sample_surface(tv, tf, spacing, max_samples=total)[0].shape[0] == total
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError):
        mesh.sample_surface(tv, tf, spacing, max_samples=total - 1)
    with pytest.raises(ValueError):                           # ~1e9 samples (12 GB of points): refused on the counts, before allocation
        mesh.sample_surface(tv, tf, 1e-4)
    with pytest.raises(ValueError):                           # int32 counts saturate instead of wrapping ...
        mesh.sample_surface(tv, tf, 1e-9)
    with pytest.raises(ValueError):                           # ... and a total beyond 32-bit indexing is refused whatever max_samples says
        mesh.sample_surface(tv, tf, 1e-9, max_samples=1 << 40)
    assert torch.cuda.mem_get_info()[0] >= free - (64 << 20)
    for bad_index in (len(v), -1, 1 << 40):
        bad = tf.clone()
        bad[17, 1] = bad_index
        with pytest.raises(ValueError):
            mesh.sample_surface(tv, bad, spacing)
    bad = tf.to(torch.int32).clone()
    bad[5, 2] = len(v)
    with pytest.raises(ValueError):
        mesh.sample_surface(tv, bad, spacing)
    for args in ((torch.from_numpy(v), tf, spacing), (tv, torch.from_numpy(f), spacing), (tv[:, :2], tf, spacing), (tv, tf[:, :2], spacing),
                 (tv, tf.float(), spacing), (tv, tf, 0.0), (tv, tf, -0.1), (tv, tf, float("nan"))):
        with pytest.raises(ValueError):
            mesh.sample_surface(*args)


# ---- the metrics ----------------------------------------------------------------------------------------------------------------
MAX_DIST, THRESHOLDS, SPACING = 0.1, (0.031, 0.04), 0.03


def metric_inputs():
    if "metric" not in _CACHE:
        v, f = icosphere(2, 0.5)
        rng = rng_of("metric")
        gt = sphere_points(rng, 3600, 0.52)
        gt = gt[gt[:, 2] < 0.52 * 0.7][:3000]                                    # one cap removed: completeness != accuracy
        assert gt.shape[0] == 3000
        gt = np.concatenate([gt, sphere_points(rng, 50, 2.0)])                   # 50 outliers beyond max_dist
        _CACHE["metric"] = (v, f, gt)
    return _CACHE["metric"]


def np_metrics(samples, gt, max_dist, thresholds):
    d_acc, d_comp = brute(samples, gt)[0], brute(gt, samples)[0]
    assert clear_of(d_acc, max_dist, *thresholds) and clear_of(d_comp, max_dist, *thresholds)
    out = {"n_mesh_samples": len(samples), "n_gt": len(gt), "precision": {}, "recall": {}, "fscore": {}}
    for key, d in (("accuracy", d_acc), ("completeness", d_comp)):
        used = d <= max_dist
        out["n_%s_used" % key] = int(used.sum())
        out[key] = float(d[used].mean()) if used.any() else float("nan")
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for t in thresholds:
        p, r = float((d_acc <= t).sum()) / len(samples), float((d_comp <= t).sum()) / len(gt)
        out["precision"][t], out["recall"][t], out["fscore"][t] = p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def check_metrics(got, want):
    assert set(got) == set(want) == {"n_mesh_samples", "n_gt", "accuracy", "n_accuracy_used", "completeness", "n_completeness_used",
                                     "chamfer", "precision", "recall", "fscore"}
    for k in ("n_mesh_samples", "n_gt", "n_accuracy_used", "n_completeness_used"):
        assert got[k] == want[k], k
    for k in ("accuracy", "completeness", "chamfer"):
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    for t in want["precision"]:
        # numerators exact: the shares are integer counts over the same totals
        assert round(got["precision"][t] * got["n_mesh_samples"]) == round(want["precision"][t] * want["n_mesh_samples"])
        assert round(got["recall"][t] * got["n_gt"]) == round(want["recall"][t] * want["n_gt"])
        assert got["precision"][t] == want["precision"][t] and got["recall"][t] == want["recall"][t]
        assert abs(got["fscore"][t] - want["fscore"][t]) <= 1e-12


def test_evaluate_mesh_matches_the_numpy_restatement():
    from vdn_hip import mesh
    from vdn_train import mesh_eval
    v, f, gt = metric_inputs()
    tv, tf, tg = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV)
    samples = mesh.sample_surface(tv, tf, SPACING)[0].cpu().numpy()             # the device's own sample points
    want = np_metrics(samples, gt, MAX_DIST, THRESHOLDS)
    got = mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, THRESHOLDS)
    print(got)
    check_metrics(got, want)
    assert got["n_accuracy_used"] < got["n_mesh_samples"] and got["n_completeness_used"] == 3000        # the cap; the outliers
    assert abs(got["accuracy"] - got["completeness"]) > 1e-4
    # a bare cloud in place of the mesh: the same figures from the same points
    check_metrics(mesh_eval.evaluate_mesh(torch.from_numpy(samples).to(DEV), None, tg, SPACING, MAX_DIST, THRESHOLDS), want)
    # nothing within max_dist on either side: means over nothing
    far = mesh_eval.evaluate_mesh(tv, tf, tg[-50:], SPACING, MAX_DIST, THRESHOLDS)
    assert np.isnan(far["accuracy"]) and np.isnan(far["completeness"]) and np.isnan(far["chamfer"])
    assert far["n_accuracy_used"] == far["n_completeness_used"] == 0 and far["fscore"] == {t: 0.0 for t in THRESHOLDS}
    with pytest.raises(ValueError):
        mesh_eval.evaluate_mesh(tv, tf, tg, SPACING, MAX_DIST, (0.04, 0.11))


def test_evaluate_mesh_analytic_anchor():
    """the unit square against a dense grid of pitch g on the plane z = 0.01: every nearest distance is at least the plane gap, and
    on average at most one pitch off sideways"""
    from vdn_train import mesh_eval
    v, f, _ = sample_mesh("square")
    g = 0.02
    x, y = np.meshgrid(np.arange(51) * g, np.arange(51) * g, indexing="ij")
    gt = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.01)], 1).astype(np.float32)
    out = mesh_eval.evaluate_mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV), g, 0.1, (0.05,))
    print(out)
    lo, hi = float(np.float32(0.01)), float(np.sqrt(0.01 ** 2 + g ** 2))          # (the plane sits at fp32(0.01) = 0.01 (1 - 2.2e-8))
    assert lo <= out["accuracy"] <= hi and lo <= out["completeness"] <= hi
    assert out["n_accuracy_used"] == out["n_mesh_samples"] and out["n_completeness_used"] == out["n_gt"] == 2601
    assert out["precision"][0.05] == out["recall"][0.05] == out["fscore"][0.05] == 1.0


def test_evaluate_ply_round_trip(tmp_path):
    from vdn_train import mesh_eval, meshio
    v, f, gt = metric_inputs()
    rng = rng_of("ply")
    mesh_path = meshio.write_ply(str(tmp_path / "mesh.ply"), v, f)
    rec = np.empty(len(gt), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                   ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for d, n in enumerate("xyz"):
        rec[n], rec["n" + n] = gt[:, d], rng.normal(size=len(gt))
    for n in ("red", "green", "blue"):
        rec[n] = rng.integers(0, 256, size=len(gt))
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(gt)] + ["property float %s" % n for n in "xyz"]
    head += ["property float n%s" % n for n in "xyz"] + ["property uchar %s" % n for n in ("red", "green", "blue")] + ["end_header"]
    gt_path = str(tmp_path / "scan.ply")
    with open(gt_path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
    from_files = mesh_eval.evaluate_ply(mesh_path, gt_path, SPACING, MAX_DIST, THRESHOLDS, device=DEV)
    in_memory = mesh_eval.evaluate_mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(gt).to(DEV),
                                        SPACING, MAX_DIST, THRESHOLDS)
    assert from_files == in_memory
