"""Exact nearest neighbours of 3-D points on the device: a uniform grid over the reference cloud's bounding box
(vdn_nn_bin / vdn_nn_query, include/vdn_render.h; csrc/mesh_eval.hip). The distance half of an accuracy / completeness / Chamfer
figure (vdn_train/mesh_eval.py), usable on its own:

    grid = PointGrid(ref)                 # ref [R,3] fp32 CUDA
    dist, idx = grid.query(q, max_dist)   # dist [Q] fp32, idx [Q] int64 into ref; +inf / -1 beyond max_dist

and, on the same grid construction, greedy radius thinning of a cloud to a fixed density (vdn_thin_round):

    keep = thin_points(points, radius)    # keep [N] bool: kept points are pairwise more than `radius` apart

and registration against the grid's cloud (vdn_icp_round, csrc/mesh_align.hip): one launch pair per ICP round

    res = icp(src, grid, max_dist=d)      # res["s"], res["R"], res["t"]: src -> the cloud; solve_sim3, IcpRound on their own

The kernels bin and search; the stable sorts and the cell-start table between them are torch ops on the device (the convention of
vdn_hip/mesh.py). The cell size changes the speed only, never a result (the stopping rule and its margin)."""
import math

import numpy as np
import torch

from . import lib
from .mesh import _call_sized

# h = DEFAULT_CELL_FACTOR * L_max * sqrt(1 / R): ~8 points per occupied cell where the cloud is a surface filling its box's face
DEFAULT_CELL_FACTOR = math.sqrt(8.0)
# the stop bound's slack, in units of (largest box extent + h): 16 ulps of fp32. The binning floor((p - lo) / h) is off by at most
# 2 roundings (2^-23 of the extent) per point and per query, the squared distances compared against the bound by 2^-22 of themselves
MARGIN_ULPS = 16.0


def _check_points(x, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.shape[1] == 3 and x.is_floating_point()):
        raise ValueError("%s must be a float [N,3] CUDA tensor" % what)
    return x.detach().float().contiguous()


def _fp32_at_most(x):
    """The largest fp32 value <= x: an fp32 distance d has d <= x exactly when d <= this."""
    f = np.float32(min(x, float(np.finfo(np.float32).max)))
    if float(f) > x:
        f = np.nextafter(f, np.float32(-np.inf))
    return float(f)


class PointGrid:
    """The reference cloud `ref` [R,3] sorted into a dense uniform grid over its bounding box.
    cell_size: the cells' edge (default: DEFAULT_CELL_FACTOR * largest extent / sqrt(R)), or a function (largest extent, R) -> edge for
    a caller whose edge depends on the box (thin_points); raised until the grid has at most max_cells cells. Each axis has floor(extent / h) + 1 cells, so a flat or single-point cloud has one cell across."""

    def __init__(self, ref, cell_size=None, max_cells=1 << 24):
        ref = _check_points(ref, "ref")
        R = ref.shape[0]
        if R == 0:
            raise ValueError("the reference cloud is empty")
        if max_cells < 1:
            raise ValueError("max_cells must be at least 1")
        if cell_size is not None and not callable(cell_size) and not (float(cell_size) > 0.0 and float(cell_size) < float("inf")):
            raise ValueError("cell_size must be positive and finite, got %r" % (cell_size,))
        box = torch.stack([ref.amin(0), ref.amax(0)]).tolist()                # one host read
        lo, hi = box
        if not all(math.isfinite(x) for x in lo + hi):
            raise ValueError("the reference cloud has non-finite coordinates")
        ext = [float(np.float32(h_) - np.float32(l_)) for l_, h_ in zip(lo, hi)]
        L = max(ext)
        if callable(cell_size):
            h = float(cell_size(L, R))
        else:
            h = float(cell_size) if cell_size is not None else DEFAULT_CELL_FACTOR * L / math.sqrt(R)
        h = float(np.float32(h))
        if not (h > 0.0 and math.isfinite(h)):
            h = 1.0                                                           # (all points equal: any size gives the one cell)
        dims = lambda s: [int(math.floor(e / s)) + 1 for e in ext]
        while np.prod(dims(h), dtype=object) > max_cells:
            h = float(np.float32(h * 1.25))
        self.ref, self.R, self.device = ref, R, ref.device
        self.lo, self.h, self.dims = [float(x) for x in lo], h, dims(h)
        self.n_cells = int(np.prod(self.dims, dtype=object))
        self.margin = float(np.float32(MARGIN_ULPS * 2.0 ** -24 * (L + h)))
        with torch.cuda.device(self.device):
            cell = self._bin(ref)
            cell, order = torch.sort(cell, stable=True)
            self.records = torch.empty(R, 4, dtype=torch.float32, device=self.device)
            self.records[:, :3] = ref[order]
            self.records.view(torch.int32)[:, 3] = order.to(torch.int32)      # the original index, as bits
            count = torch.bincount(cell, minlength=self.n_cells)
            self.cell_start = torch.zeros(self.n_cells + 1, dtype=torch.int32, device=self.device)
            self.cell_start[1:] = torch.cumsum(count, 0).to(torch.int32)
            self.cell_count = count

    def _args(self, pts):
        a = lib.VdnNnArgs()
        a.pts, a.N = pts.data_ptr(), pts.shape[0]
        a.lo_x, a.lo_y, a.lo_z, a.h, a.margin = self.lo[0], self.lo[1], self.lo[2], self.h, self.margin
        a.nx, a.ny, a.nz = self.dims
        return a

    def _bin(self, pts):
        """cell id [N] int32 of pts [N,3] fp32 (vdn_nn_bin)."""
        cell = torch.empty(pts.shape[0], dtype=torch.int32, device=self.device)
        a = self._args(pts)
        a.cell = cell.data_ptr()
        _call_sized("vdn_nn_bin", a, lib.stream_handle())
        return cell

    def query(self, q, max_dist=None, return_rings=False):
        """q [Q,3] -> (dist [Q] fp32, idx [Q] int64 into the caller's ref): the nearest reference point of every query, the lower
        index on equal distances. With max_dist, a query with no reference point within it (inclusive) gets +inf and -1.
        return_rings adds the number of grid shells each query visited (int32 [Q])."""
        q = _check_points(q, "q")
        if q.device != self.device:
            raise ValueError("q must be on the reference's device")
        if max_dist is not None and not (float(max_dist) >= 0.0):
            raise ValueError("max_dist must be >= 0, got %r" % (max_dist,))
        Q = q.shape[0]
        dist = torch.empty(Q, dtype=torch.float32, device=self.device)
        idx = torch.empty(Q, dtype=torch.int64, device=self.device)
        rings = torch.empty(Q, dtype=torch.int32, device=self.device) if return_rings else None
        if Q > 0:
            with torch.cuda.device(self.device):
                # queries in their own cell order: the 64 lanes of a wave walk the same few cells
                order = torch.sort(self._bin(q), stable=True)[1].to(torch.int32)
                a = self._args(q)
                a.ref, a.cell_start, a.order, a.R = self.records.data_ptr(), self.cell_start.data_ptr(), order.data_ptr(), self.R
                a.dist, a.idx = dist.data_ptr(), idx.data_ptr()
                a.rings = rings.data_ptr() if return_rings else None
                a.max_dist = float("inf") if max_dist is None else _fp32_at_most(float(max_dist))
                _call_sized("vdn_nn_query", a, lib.stream_handle())
        return (dist, idx, rings) if return_rings else (dist, idx)


def nearest(q, ref, max_dist=None, cell_size=None):
    """dist [Q] fp32, idx [Q] int64: PointGrid(ref, cell_size).query(q, max_dist)."""
    return PointGrid(ref, cell_size=cell_size).query(q, max_dist)


def _thin_min_cell(radius, extent):
    """The smallest fp32 cell edge h with h >= radius + PointGrid's margin at that h (margin = m (extent + h), m = 16 * 2^-24):
    then two points within `radius` of each other are at most one cell apart on every axis, the fp32 binning included."""
    m = MARGIN_ULPS * 2.0 ** -24
    h = np.float32((radius + m * extent) / (1.0 - m))
    while not (float(h) >= radius + float(np.float32(m * (extent + float(h))))):
        h = np.nextafter(h, np.float32(np.inf))
    return float(np.nextafter(h, np.float32(np.inf)))            # (one more: the margin itself is rounded to fp32)


def _rounds_to_fixpoint(one_round, N):
    """Calls one_round() -> the number of points still undecided, until it says 0 -> the number of calls. Every round of a correct
    kernel decides at least the lowest undecided index (the first one: point 0), so the number strictly decreases from N and the
    loop ends within N rounds; anything else is a defect and raises RuntimeError instead of looping."""
    rounds, before = 0, N
    while True:
        now = one_round()
        rounds += 1
        if now == 0:
            return rounds
        if not (0 < now < before):
            raise RuntimeError("thin_points: round %d left %d points undecided after %d: no progress" % (rounds, now, before))
        before = now


def thin_points(points, radius, cell_size=None, max_cells=1 << 24, return_rounds=False):
    """points [N,3] float CUDA -> keep [N] bool (with return_rounds: (keep, rounds)): greedy radius thinning, exactly this loop over
    the caller's index order, on the device (vdn_thin_round, include/vdn_render.h):

        keep = ones(N)
        for i in 0..N-1:
            if keep[i]: keep[j] = False for every j != i with |p_i - p_j| <= radius

    - the lexicographically first maximal set of points that are pairwise more than `radius` apart. `<=` is inclusive, the distance
    is (dx*dx + dy*dy + dz*dz) <= radius*radius in fp32 (PointGrid.query's difference form), of two equal points the later one goes.
    Another visiting order: permute the points first.

    The parallel form runs in rounds: a point is removed once a lower-index neighbour is kept, kept once all its lower-index
    neighbours are removed, and waits for the next round otherwise; the fixpoint is the loop's result whatever the scheduling.
    Every round costs one host read of the number of points still waiting. How many rounds depends on the index order, not only on
    the cloud: surface samples at radius = sample spacing took 5 to 10 rounds in sample_surface's own order and in a random order
    (10^6 and 10^7 samples, measured), 19 and 32 in a strip-like order (sorted into bands; 2 * 10^4 and 2 * 10^5 points, counted on
    the CPU by tools/count_thin_rounds.py), while points on a line in index order need about N / 2 - legal and slow; permute such a
    cloud.

    The number of rounds is NOT a function of the cloud alone: inside a round a lane may or may not see what another wave has just
    stored, so `rounds` can differ by a few between two calls on the same points (197 to 200 on the 200-point line of the tests).
    `keep` never differs.

    cell_size: the grid's cell edge; raised to the minimum radius + margin (the 27 cells around a point then hold all its
    neighbours) and further until the grid has at most max_cells cells. Default: the larger of that minimum and extent / sqrt(N),
    which suits a surface cloud; a cloud that fills its box gets fuller cells than it needs where radius is far below the point
    spacing - pass cell_size there. It changes the speed only.

    ValueError for a radius that is not positive and finite (in fp32 too), a non-CUDA or non-[N,3] tensor or non-finite
    coordinates; RuntimeError if a round decides nothing (a defect: the loop never spins). N = 0 launches nothing."""
    if not (float(radius) > 0.0 and math.isfinite(float(radius))):
        raise ValueError("radius must be positive and finite, got %r" % (radius,))
    with np.errstate(over="ignore"):
        r32 = float(np.float32(float(radius)))
    if not (r32 > 0.0 and math.isfinite(r32)):
        raise ValueError("radius %r is not a positive finite fp32 number" % (radius,))
    radius = r32
    if cell_size is not None and not (float(cell_size) > 0.0 and float(cell_size) < float("inf")):
        raise ValueError("cell_size must be positive and finite, got %r" % (cell_size,))
    points = _check_points(points, "points")
    N, dev = points.shape[0], points.device
    if N == 0:
        keep = torch.zeros(0, dtype=torch.bool, device=dev)
        return (keep, 0) if return_rounds else keep
    # the edge needs the box's extent: PointGrid reads and checks the box once and asks back
    edge = lambda extent, n: max(_thin_min_cell(radius, extent), float(cell_size) if cell_size is not None else extent / math.sqrt(n))
    try:
        grid = PointGrid(points, cell_size=edge, max_cells=max_cells)
    except ValueError as e:
        raise ValueError(str(e).replace("the reference cloud", "the cloud"))
    if not (grid.h >= radius + grid.margin):
        raise RuntimeError("thin_points: cell edge %r does not cover radius %r + margin %r" % (grid.h, radius, grid.margin))
    with torch.cuda.device(dev):
        state = torch.zeros(N, dtype=torch.int32, device=dev)
        left = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnThinArgs()
        a.rec, a.cell_start, a.state, a.undecided, a.N = grid.records.data_ptr(), grid.cell_start.data_ptr(), state.data_ptr(), left.data_ptr(), N
        a.lo_x, a.lo_y, a.lo_z, a.h, a.radius = grid.lo[0], grid.lo[1], grid.lo[2], grid.h, radius
        a.nx, a.ny, a.nz = grid.dims

        def one_round():
            left.zero_()
            _call_sized("vdn_thin_round", a, lib.stream_handle())
            return int(left.item())

        rounds = _rounds_to_fixpoint(one_round, N)
        keep = torch.empty(N, dtype=torch.bool, device=dev)
        keep[grid.records.view(torch.int32)[:, 3].long()] = state == 1
    return (keep, rounds) if return_rounds else keep


# ---- registration: one ICP round on the device, the closed-form solve, the loop ---------------------------------
ICP_SUMS = 19
# the slots of vdn_icp_round's result (include/vdn_render.h: VDN_ICP_*)
ICP_N, ICP_P, ICP_Q, ICP_PP, ICP_QQ, ICP_QP, ICP_RES = 0, 1, 4, 7, 8, 9, 18


def sim3_matrix(s, R, t):
    """(s, R, t) -> the 3 x 4 float64 matrix [sR | t] vdn_icp_round takes."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    if R.shape != (3, 3):
        raise ValueError("R must be 3 x 3")
    M = np.empty((3, 4))
    M[:, :3], M[:, 3] = float(s) * R, t
    if not np.isfinite(M).all():
        raise ValueError("the transform is not finite")
    return M


def query_order(grid, y):
    """The visiting order PointGrid.query uses for the queries y [N,3] fp32: their stable sort by cell, int32 [N]."""
    with torch.cuda.device(grid.device):
        return torch.sort(grid._bin(y), stable=True)[1].to(torch.int32)


class IcpRound:
    """One registration round as an operator (vdn_icp_round): src [N,3] float CUDA against the PointGrid `grid` of the target.

        sums = IcpRound(src, grid)(M, max_dist)          # [19] float64 on the device: see ICP_* and include/vdn_render.h

    order: an int32 [N] visiting order (query_order) or None; with_dist / with_idx keep vdn_nn_query's per-point outputs of the
    last call in .dist [N] fp32 / .idx [N] int64. The workspace is allocated once; every call is two launches and no host read."""

    def __init__(self, src, grid, order=None, with_dist=False, with_idx=False):
        if not isinstance(grid, PointGrid):
            raise ValueError("grid must be a PointGrid")
        src = _check_points(src, "src")
        if src.device != grid.device:
            raise ValueError("src must be on the target's device")
        N = src.shape[0]
        if N == 0:
            raise ValueError("the source cloud is empty")
        if order is not None and not (torch.is_tensor(order) and order.dtype == torch.int32 and order.shape == (N,) and
                                      order.device == src.device and order.is_contiguous()):
            raise ValueError("order must be a contiguous int32 [N] tensor on the source's device")
        self.src, self.grid, self.order, self.N = src, grid, order, N
        dev = src.device
        blocks = lib.call_value("vdn_icp_round_blocks", N)
        if blocks < 1:
            raise ValueError("vdn_icp_round: the sizes do not fit 32-bit indexing")
        self.partials = torch.empty(blocks, ICP_SUMS, dtype=torch.float64, device=dev)
        self.result = torch.empty(ICP_SUMS, dtype=torch.float64, device=dev)
        self.dist = torch.empty(N, dtype=torch.float32, device=dev) if with_dist else None
        self.idx = torch.empty(N, dtype=torch.int64, device=dev) if with_idx else None
        a = self.args = lib.VdnIcpArgs()
        a.src, a.ref, a.cell_start = src.data_ptr(), grid.records.data_ptr(), grid.cell_start.data_ptr()
        a.order = order.data_ptr() if order is not None else None
        a.dist = self.dist.data_ptr() if with_dist else None
        a.idx = self.idx.data_ptr() if with_idx else None
        a.partials, a.result, a.partials_rows = self.partials.data_ptr(), self.result.data_ptr(), blocks
        a.N, a.R = N, grid.R
        a.lo_x, a.lo_y, a.lo_z, a.h, a.margin = grid.lo[0], grid.lo[1], grid.lo[2], grid.h, grid.margin
        a.nx, a.ny, a.nz = grid.dims

    def __call__(self, M, max_dist):
        M = np.asarray(M, np.float64)
        if M.shape != (3, 4) or not np.isfinite(M).all():
            raise ValueError("M must be a finite 3 x 4 matrix")
        if not (float(max_dist) >= 0.0):
            raise ValueError("max_dist must be >= 0, got %r" % (max_dist,))
        a = self.args
        (a.m00, a.m01, a.m02, a.m03, a.m10, a.m11, a.m12, a.m13, a.m20, a.m21, a.m22, a.m23) = [float(x) for x in M.reshape(-1)]
        a.max_dist = _fp32_at_most(float(max_dist))
        with torch.cuda.device(self.src.device):
            _call_sized("vdn_icp_round", a, lib.stream_handle())
        return self.result


def solve_sim3(sums, scale=True):
    """The 19 sums of a round (ICP_*: n, sum p, sum q, sum p.p, sum q.q, sum q p^T, the residual) -> (s, R, t), float64 numpy: the
    similarity q ~ s R p + t that minimises sum |s R p + t - q|^2 over the pairs, by Umeyama's closed form:
        mp, mq = sum p / n, sum q / n;   C = sum q p^T / n - mq mp^T;   vp = sum p.p / n - |mp|^2;   C = U D V^T
        S = diag(1, 1, sign(det U det V))  (the reflection guard: det R = +1 always);   R = U S V^T
        s = trace(D S) / vp (1 when scale=False);   t = mq - s R mp
    ValueError when fewer than 3 pairs matched, or when the pairs' covariance C has rank < 2 (its second singular value <= 1e-12 of
    the first: source or matches on a line or in a point - the rotation about that line is not determined)."""
    x = np.asarray(sums.detach().cpu() if torch.is_tensor(sums) else sums, dtype=np.float64).reshape(-1)
    if x.shape[0] != ICP_SUMS:
        raise ValueError("sums must hold %d numbers" % ICP_SUMS)
    n = x[ICP_N]
    if not (n >= 3):
        raise ValueError("fewer than 3 pairs matched (%d)" % int(n))
    mp, mq = x[ICP_P:ICP_P + 3] / n, x[ICP_Q:ICP_Q + 3] / n
    C = x[ICP_QP:ICP_QP + 9].reshape(3, 3) / n - np.outer(mq, mp)
    vp = x[ICP_PP] / n - float(mp @ mp)
    U, D, Vt = np.linalg.svd(C)
    if not (D[0] > 0.0 and D[1] > 1e-12 * D[0] and vp > 0.0):
        raise ValueError("the matched pairs are degenerate (covariance of rank < 2): no rotation is determined")
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
    R = (U * S) @ Vt
    s = float((D * S).sum() / vp) if scale else 1.0
    return s, R, mq - s * (R @ mp)


def _corner_motion(corners, A, B):
    """the largest displacement of the corners [8,3] between the transforms A and B ((s, R, t) each)"""
    ya = A[0] * corners @ A[1].T + A[2]
    yb = B[0] * corners @ B[1].T + B[2]
    return float(np.sqrt(((ya - yb) ** 2).sum(1)).max())


def icp(src, target, init=None, max_dist=float("inf"), scale=False, max_rounds=50, tol=1e-7, trim=None):
    """Point-to-point ICP from src [N,3] (float CUDA) to `target` (a PointGrid, or a [R,3] CUDA tensor a grid is built of), one way.
    init: (s, R, t) or None for the identity. Every round is one vdn_icp_round at the current transform T (transform, nearest
    target point within the round's threshold, the pairs' 19 moments), one host read of the 19 doubles and one solve_sim3 on them,
    which gives the next T whole (the moments are of the untransformed source: no chain of increments).
      threshold  round 0: max_dist. With trim = f (0 < f <= 1), round k >= 1: min(max_dist, the ceil(f n)-th smallest of the n
                 finite distances of round k - 1) (torch.kthvalue on the device; one more host read per round)
      converged  when the 8 corners of the source's bounding box move by <= tol x the box's diagonal between consecutive transforms
    -> dict: s, R [3,3], t [3], matrix [4,4] (float64 numpy), rounds, converged, and per round the lists n_pairs, rms
    (sqrt(residual sum / n_pairs), at the round's T) and threshold.
    ValueError for a round that matches fewer than 3 points (it names max_dist) or degenerate pairs. The samples are visited in
    the cell order of the initial transform (it changes the speed only)."""
    grid = target if isinstance(target, PointGrid) else PointGrid(_check_points(target, "target"))
    src = _check_points(src, "src")
    if src.shape[0] == 0:
        raise ValueError("the source cloud is empty")
    if not (float(max_dist) >= 0.0):
        raise ValueError("max_dist must be >= 0, got %r" % (max_dist,))
    if trim is not None and not (0.0 < float(trim) <= 1.0):
        raise ValueError("trim must be in (0, 1], got %r" % (trim,))
    if int(max_rounds) < 1 or not (float(tol) >= 0.0):
        raise ValueError("max_rounds must be >= 1 and tol >= 0")
    T = (1.0, np.eye(3), np.zeros(3)) if init is None else (float(init[0]), np.asarray(init[1], np.float64), np.asarray(init[2], np.float64).reshape(3))
    M = sim3_matrix(*T)
    box = torch.stack([src.amin(0), src.amax(0)]).double().cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError("the source cloud has non-finite coordinates")
    corners = np.array([[box[(c >> d) & 1, d] for d in range(3)] for c in range(8)])
    diag = float(np.linalg.norm(box[1] - box[0]))
    with torch.cuda.device(src.device):
        y0 = (src.double() @ torch.from_numpy(M[:, :3].T.copy()).to(src.device) + torch.from_numpy(M[:, 3].copy()).to(src.device)).float()
        op = IcpRound(src, grid, order=query_order(grid, y0), with_dist=trim is not None)
        del y0
    out = {"n_pairs": [], "rms": [], "threshold": [], "converged": False}
    thr = float(max_dist)
    for k in range(int(max_rounds)):
        x = op(M, thr).cpu().numpy()
        n = int(x[ICP_N])
        out["n_pairs"].append(n)
        out["rms"].append(math.sqrt(x[ICP_RES] / n) if n > 0 else float("nan"))
        out["threshold"].append(thr)
        if n < 3:
            raise ValueError("round %d matched %d points within max_dist = %r (threshold %r): fewer than 3" % (k, n, max_dist, thr))
        T_new = solve_sim3(x, scale=scale)
        moved = _corner_motion(corners, T, T_new)
        T, M = T_new, sim3_matrix(*T_new)
        if trim is not None:
            kth = int(math.ceil(float(trim) * n))
            thr = min(float(max_dist), float(torch.kthvalue(op.dist, max(kth, 1)).values.item()))
        if moved <= float(tol) * diag:
            out["converged"] = True
            break
    out["rounds"] = len(out["n_pairs"])
    out["s"], out["R"], out["t"] = T
    out["matrix"] = np.vstack([M, [0.0, 0.0, 0.0, 1.0]])
    return out
