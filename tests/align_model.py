"""A float64 numpy model of mesh alignment (vdn_hip.nn: vdn_icp_round, solve_sim3, icp), for tests/test_mesh_align_cpu.py and
tests/test_gpu_mesh_align.py: the documented expression of y, brute-force matches, the 19 sums, the closed-form solve, the loop
with its convergence and trim rules, and the cases both test files share. Nothing here touches the device or the library."""
import math

import numpy as np

N_SUMS = 19
S_N, S_P, S_Q, S_PP, S_QQ, S_QP, S_RES = 0, 1, 4, 7, 8, 9, 18


# ---- the round ------------------------------------------------------------------------------------------------------------------
def matrix(s, R, t):
    M = np.empty((3, 4))
    M[:, :3], M[:, 3] = float(s) * np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    return M


def transform_y(M, p):
    """y = fp32(((m0 x + m1 y) + m2 z) + m3) per row, products and sums in double: bit for bit the kernel's y. p [N,3] fp32."""
    p = np.asarray(p, np.float32).astype(np.float64)
    y = np.empty_like(p)
    for r in range(3):
        y[:, r] = ((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]
    return y.astype(np.float32)


def brute(q, ref):
    """fp64 distance of every fp32 query to its nearest fp32 reference point, difference form -> (dist [Q], argmin [Q])."""
    q, ref = np.asarray(q, np.float32).astype(np.float64), np.asarray(ref, np.float32).astype(np.float64)
    d2 = np.zeros((q.shape[0], ref.shape[0]))
    for a in range(3):
        d2 += (q[:, a:a + 1] - ref[None, :, a]) ** 2
    i = d2.argmin(1)
    return np.sqrt(d2[np.arange(q.shape[0]), i]), i


def clear_of(d, *levels):
    """no distance within 1e-5 relative of a level (so a <= decision cannot hinge on fp32 rounding)"""
    return all((np.abs(d - t) > 1e-5 * t).all() for t in levels)


def pair_terms(p, q, y):
    """[n,19] float64: the terms of the pairs (p [n,3] fp32 source, q [n,3] fp32 match, y [n,3] fp32 transformed source)."""
    p, q, y = (np.asarray(x, np.float32).astype(np.float64) for x in (p, q, y))
    T = np.zeros((p.shape[0], N_SUMS))
    T[:, S_N] = 1.0
    T[:, S_P:S_P + 3], T[:, S_Q:S_Q + 3] = p, q
    T[:, S_PP] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    T[:, S_QQ] = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    for r in range(3):
        for c in range(3):
            T[:, S_QP + 3 * r + c] = q[:, r] * p[:, c]
    e = y - q
    T[:, S_RES] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return T


def round_model(src, ref, M, max_dist):
    """-> dict: y, dist (fp64 brute force, all points), idx, hit, sums [19] (math.fsum: the exact sum, rounded once), mag [19] = sum |terms|."""
    y = transform_y(M, src)
    dist, idx = brute(y, ref)
    hit = dist <= max_dist
    T = pair_terms(np.asarray(src)[hit], np.asarray(ref)[idx[hit]], y[hit])
    sums = np.array([math.fsum(T[:, j]) for j in range(N_SUMS)])
    mag = np.array([math.fsum(np.abs(T[:, j])) for j in range(N_SUMS)])
    return {"y": y, "dist": dist, "idx": idx, "hit": hit, "sums": sums, "mag": mag}


# ---- the solve ------------------------------------------------------------------------------------------------------------------
def solve_sim3(x, scale=True):
    x = np.asarray(x, np.float64)
    n = x[S_N]
    if not n >= 3:
        raise ValueError("fewer than 3 pairs")
    mp, mq = x[S_P:S_P + 3] / n, x[S_Q:S_Q + 3] / n
    C = x[S_QP:S_QP + 9].reshape(3, 3) / n - np.outer(mq, mp)
    vp = x[S_PP] / n - mp @ mp
    U, D, Vt = np.linalg.svd(C)
    if not (D[0] > 0 and D[1] > 1e-12 * D[0] and vp > 0):
        raise ValueError("degenerate pairs")
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / vp) if scale else 1.0
    return s, R, mq - s * (R @ mp)


def sums_of_pairs(p, q, y=None):
    """the 19 sums of given pairs in float64 (for solve tests: p, q any float64 arrays)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    x = np.zeros(N_SUMS)
    x[S_N] = len(p)
    x[S_P:S_P + 3], x[S_Q:S_Q + 3] = p.sum(0), q.sum(0)
    x[S_PP], x[S_QQ] = (p * p).sum(), (q * q).sum()
    x[S_QP:S_QP + 9] = (q.T @ p).reshape(-1)
    if y is not None:
        x[S_RES] = ((np.asarray(y, np.float64) - q) ** 2).sum()
    return x


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def box_corners(src):
    src = np.asarray(src, np.float32).astype(np.float64)
    lo, hi = src.min(0), src.max(0)
    corners = np.array([[(lo, hi)[(c >> d) & 1][d] for d in range(3)] for c in range(8)])
    return corners, float(np.linalg.norm(hi - lo))


def corner_motion(corners, A, B):
    ya = A[0] * corners @ A[1].T + A[2]
    yb = B[0] * corners @ B[1].T + B[2]
    return float(np.sqrt(((ya - yb) ** 2).sum(1)).max())


def icp_model(src, ref, init=None, max_dist=np.inf, scale=False, max_rounds=50, tol=1e-7, trim=None):
    """The loop of vdn_hip.nn.icp on brute-force matches -> the same dict, plus `dists` (every round's fp64 distances)."""
    T = (1.0, np.eye(3), np.zeros(3)) if init is None else (float(init[0]), np.asarray(init[1], np.float64), np.asarray(init[2], np.float64))
    corners, diag = box_corners(src)
    out = {"n_pairs": [], "rms": [], "threshold": [], "dists": [], "converged": False}
    thr = float(max_dist)
    for k in range(max_rounds):
        r = round_model(src, ref, matrix(*T), thr)
        n = int(r["hit"].sum())
        out["n_pairs"].append(n)
        out["rms"].append(math.sqrt(r["sums"][S_RES] / n) if n else float("nan"))
        out["threshold"].append(thr)
        out["dists"].append(r["dist"])
        if n < 3:
            raise ValueError("round %d matched %d points within max_dist" % (k, n))
        T_new = solve_sim3(r["sums"], scale)
        moved = corner_motion(corners, T, T_new)
        T = T_new
        if trim is not None:
            kth = max(int(math.ceil(trim * n)), 1)
            thr = min(float(max_dist), float(np.sort(r["dist"][r["hit"]])[kth - 1]))
        if moved <= tol * diag:
            out["converged"] = True
            break
    out["rounds"] = len(out["n_pairs"])
    out["s"], out["R"], out["t"] = T
    out["matrix"] = np.vstack([matrix(*T), [0, 0, 0, 1.0]])
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
MAX_DIST = 0.15
CASES = {  # name: (degrees about (1, 2, 3), translation, scale, the `scale` argument)
    "rigid": (8.0, (0.04, -0.02, 0.0133), 1.0, False),
    "similarity": (6.0, (0.03, -0.015, 0.01), 1.04, True),
    "large": (15.0, (0.06, -0.03, 0.02), 1.0, False),
}


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def lobed(d):
    """unit directions d [n,3] -> fp32 points on the lobed ellipsoid r(d) = 0.5 (1 + 0.3 sin(3 dx + 1) + 0.25 cos(4 dy dz + 0.5) + 0.2 dz),
    scaled by (1, 0.8, 0.6) per axis"""
    r = 0.5 * (1.0 + 0.3 * np.sin(3.0 * d[:, 0] + 1.0) + 0.25 * np.cos(4.0 * d[:, 1] * d[:, 2] + 0.5) + 0.2 * d[:, 2])
    return (d * r[:, None] * np.array([1.0, 0.8, 0.6])).astype(np.float32)


def lobed_ellipsoid(rng, n):
    d = rng.normal(size=(n, 3))
    return lobed(d / np.linalg.norm(d, axis=1, keepdims=True))


def lobed_icosphere(subdivisions):
    """-> (vertices [V,3] fp32 on the lobed ellipsoid, triangles [F,3] int64): a subdivided icosahedron pushed onto the surface"""
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
    return lobed(np.array(v)), np.array(f, np.int64)


_CASES = {}


def case(name, near_outliers=False):
    """-> dict: src [1650,3] fp32 (1500 inliers first, then 150 outliers), ref [4000,3] fp32, truth (s, R, t), scale, max_dist.
    near_outliers: the outliers are uniform in the target's box (some within max_dist) instead of on the sphere of radius 3."""
    key = (name, near_outliers)
    if key not in _CASES:
        deg, t, s, scale = CASES[name]
        rng = np.random.default_rng(20240 + sorted(CASES).index(name))
        ref = lobed_ellipsoid(rng, 4000)
        R, t = rotation((1.0, 2.0, 3.0), deg), np.array(t, np.float64)
        pick = rng.permutation(4000)[:1500]
        inl = ((ref[pick].astype(np.float64) - t) @ R) / s                  # R^T (q - t) / s, row-wise
        if near_outliers:
            lo, hi = ref.min(0).astype(np.float64), ref.max(0).astype(np.float64)
            outl = ((lo + rng.uniform(size=(150, 3)) * (hi - lo) - t) @ R) / s
        else:
            d = rng.normal(size=(150, 3))
            outl = 3.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
        src = np.concatenate([inl, outl]).astype(np.float32)
        _CASES[key] = {"src": src, "ref": ref, "truth": (s, R, t), "scale": scale, "max_dist": MAX_DIST, "pick": pick}
    return _CASES[key]


_MODEL = {}


def case_model(name, tol, max_rounds=60, near_outliers=False, trim=None):
    """icp_model on a case, computed once per argument set and shared (nobody modifies it)."""
    key = (name, tol, max_rounds, near_outliers, trim)
    if key not in _MODEL:
        c = case(name, near_outliers)
        _MODEL[key] = icp_model(c["src"], c["ref"], None, c["max_dist"], c["scale"], max_rounds, tol, trim)
    return _MODEL[key]


def pose_error(result, truth):
    """(max |R - R*|, max |t - t*|, |s / s* - 1|)"""
    return (float(np.abs(result["R"] - truth[1]).max()), float(np.abs(result["t"] - truth[2]).max()), abs(result["s"] / truth[0] - 1.0))
