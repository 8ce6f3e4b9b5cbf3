"""Exact nearest neighbours of 3-D points on the device: a uniform grid over the reference cloud's bounding box
(vdn_nn_bin / vdn_nn_query, include/vdn_render.h; csrc/mesh_eval.hip). The distance half of an accuracy / completeness / Chamfer
figure (vdn_train/mesh_eval.py), usable on its own:

    grid = PointGrid(ref)                 # ref [R,3] fp32 CUDA
    dist, idx = grid.query(q, max_dist)   # dist [Q] fp32, idx [Q] int64 into ref; +inf / -1 beyond max_dist

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
    cell_size: the cells' edge (default: DEFAULT_CELL_FACTOR * largest extent / sqrt(R)); raised until the grid has at most
    max_cells cells. Each axis has floor(extent / h) + 1 cells, so a flat or single-point cloud has one cell across."""

    def __init__(self, ref, cell_size=None, max_cells=1 << 24):
        ref = _check_points(ref, "ref")
        R = ref.shape[0]
        if R == 0:
            raise ValueError("the reference cloud is empty")
        if max_cells < 1:
            raise ValueError("max_cells must be at least 1")
        if cell_size is not None and not (float(cell_size) > 0.0 and float(cell_size) < float("inf")):
            raise ValueError("cell_size must be positive and finite, got %r" % (cell_size,))
        box = torch.stack([ref.amin(0), ref.amax(0)]).tolist()                # one host read
        lo, hi = box
        if not all(math.isfinite(x) for x in lo + hi):
            raise ValueError("the reference cloud has non-finite coordinates")
        ext = [float(np.float32(h_) - np.float32(l_)) for l_, h_ in zip(lo, hi)]
        L = max(ext)
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
