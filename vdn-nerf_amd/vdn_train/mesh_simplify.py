"""Mesh simplification: bring an extracted surface down to a chosen density before it is viewed, shipped or compared - vertex
clustering with quadric error placement on the device (vdn_hip/mesh.py: simplify_mesh, csrc/mesh_simplify.hip; DESIGN.md 3p,
INTEGRATION.md "Mesh simplification"). simplify_mesh here is the front door for arrays of either kind: it takes a cell size, or a
face budget that it turns into a cell size by bisection on a count-only pass; with a tolerance (or a budget and levels) the cells
grow adaptively, by octree merging under an error bound."""
import math

import numpy as np
import torch

from vdn_train.mesh_clean import _device_of

TARGET_PASSES = 16          # count passes of the search for a face budget, at most


def _search_bounds(v, t):
    """-> (mean triangle extent, box diagonal) over the triangles with finite corners, as floats (one host read); (0, 0) without one"""
    V = v.shape[0]
    if t.shape[0] == 0:
        return 0.0, 0.0
    tl = t.long()
    ok = ((tl >= 0) & (tl < V)).all(dim=1)
    if V == 0 or not bool(ok.all()):
        raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
    p = v.float()[tl]
    ok = torch.isfinite(p).all(dim=2).all(dim=1)
    if not bool(ok.any()):
        return 0.0, 0.0
    p = p[ok].double()
    lo, hi = p.amin(dim=1), p.amax(dim=1)
    ext = (hi - lo).amax(dim=1).mean()
    diag = (hi.amax(dim=0) - lo.amin(dim=0)).norm()
    return tuple(torch.stack([ext, diag]).tolist())


def find_cell_size(vertices, triangles, target_faces, origin=None):
    """The smallest cell size tried whose simplified mesh has at most target_faces triangles -> (cell_size, tried), tried = the
    (cell_size, faces) pairs in the order they were counted. A bisection of log(cell_size) between the mean triangle extent (where
    hardly anything merges) and the box diagonal (where everything falls into a few cells), at most TARGET_PASSES count-only passes
    (vdn_hip.mesh.count_simplified_faces: keys, corner records and the duplicate rule, no quadrics). The face count is not
    monotone in the cell size cell by cell, only in the large; the answer is the smallest size SEEN to fit, and the bracket's lower
    end was seen not to fit (unless the mesh fits as it is)."""
    from vdn_hip import mesh
    if int(target_faces) != target_faces or target_faces < 0:
        raise ValueError("target_faces must be a non-negative integer, got %r" % (target_faces,))
    lo, hi = _search_bounds(vertices, triangles)
    tried = []

    def count(h):
        n = mesh.count_simplified_faces(vertices, triangles, h, origin=origin)
        tried.append((h, n))
        return n
    if not (lo > 0.0 and hi > 0.0 and math.isfinite(hi)):
        return 1.0, tried                                    # (no triangle with an extent: any cell size gives the same)
    if count(lo) <= target_faces:
        return lo, tried
    hi *= 1.0 + 1e-6                                         # (one cell then holds the whole box: no triangle survives)
    if count(hi) > target_faces:                             # (cannot happen with a default origin: kept for a given one)
        raise ValueError("no cell size up to the box diagonal brings the mesh under %d faces" % target_faces)
    best = hi
    while len(tried) < TARGET_PASSES:
        mid = math.sqrt(lo * hi)
        if count(mid) <= target_faces:
            best = hi = mid
        else:
            lo = mid
    return best, tried


def find_tolerance(tree, target_faces):
    """The smallest tolerance tried whose adaptive mesh (vdn_hip.mesh.simplify_mesh(tolerance=..) on the built cluster_octree `tree`)
    has at most target_faces triangles -> (tolerance, tried), tried = the (tolerance, faces) pairs in the order they were counted.
    A bisection of log(tolerance) between 1e-6 finest cells (nothing merges) and sqrt(3) (1 + 1e-6) coarsest cells - above that
    every cell with a positive trace is accepted, because each recorded triangle's plane passes through a corner inside the cell,
    no further from the placed vertex than the cell's diagonal - with at most TARGET_PASSES count passes
    (vdn_hip.mesh.count_octree_faces: select, assign, records and the duplicate rule on the one tree; no quadrics). The count is
    monotone only in the large; the answer is the smallest tolerance SEEN to fit. ValueError when the upper end does not fit: the
    coarsest cells are too fine for the budget."""
    from vdn_hip import mesh
    if int(target_faces) != target_faces or target_faces < 0:
        raise ValueError("target_faces must be a non-negative integer, got %r" % (target_faces,))
    h0, levels = tree["cell_size"], len(tree["levels"]) - 1
    lo, hi = 1e-6 * h0, math.sqrt(3.0) * h0 * 2.0 ** levels * (1.0 + 1e-6)
    tried = []

    def count(tol):
        n = mesh.count_octree_faces(tree, tol)
        tried.append((tol, n))
        return n
    if count(lo) <= target_faces:
        return lo, tried
    if count(hi) > target_faces:
        raise ValueError("even with every cell merged up to %g (cell_size %g, %d levels) the mesh keeps %d faces, more than %d: raise "
                         "levels or cell_size" % (h0 * 2.0 ** levels, h0, levels, tried[-1][1], target_faces))
    best = hi
    while len(tried) < TARGET_PASSES:
        mid = math.sqrt(lo * hi)
        if count(mid) <= target_faces:
            best = hi = mid
        else:
            lo = mid
    return best, tried


def simplify_mesh(vertices, triangles, *, cell_size=None, target_faces=None, origin=None, placement="quadric", eps=None, attributes=(),
                  tolerance=None, levels=None):
    """vertices [V,3] float, triangles [F,3] integer (numpy arrays or CUDA tensors) -> dict(vertices, triangles, attributes,
    vertex_cluster, status, report), arrays of the inputs' kind and dtypes: vdn_hip.mesh.simplify_mesh. Exactly one of cell_size
    (the clustering cells' edge, in the mesh's units) and target_faces (a face budget: find_cell_size picks the cell size, and the
    report lists every (size, faces) pair it tried under "tried") is given. `attributes` (a sequence of [V,...] float or uint8 arrays:
    normals, colours) are averaged per new vertex; an averaged normal is no unit vector any more - renormalise it, or shade the new
    vertices afresh (validate_mesh(simplify=...) does that).

    The adaptive mode is on when `tolerance` or `levels` is given, and then cell_size is required: it is the finest cell, and cells
    grow by octree merging, up to cell_size 2^levels (levels defaults to vdn_hip.mesh.OCTREE_LEVELS), wherever the merged cell's
    vertex stays within `tolerance` (an rms distance, in the mesh's units) of the planes it replaces; the result gains `level`.
    With target_faces in place of the tolerance the tree is built once and find_tolerance picks the tolerance; the report lists
    the (tolerance, faces) pairs under "tried"."""
    from vdn_hip import mesh
    adaptive = tolerance is not None or levels is not None
    if adaptive:
        if cell_size is None:
            raise ValueError("the adaptive mode (tolerance, levels) needs cell_size, its finest cell")
        if (tolerance is None) == (target_faces is None):
            raise ValueError("the adaptive mode needs exactly one of tolerance and target_faces")
        if placement != "quadric":
            raise ValueError("the adaptive mode needs placement='quadric': the error it bounds is the quadric's")
        levels = mesh._check_levels(mesh.OCTREE_LEVELS if levels is None else levels)
        if tolerance is not None:
            tolerance = mesh._check_tolerance(tolerance)
    elif (cell_size is None) == (target_faces is None):
        raise ValueError("exactly one of cell_size and target_faces must be given")
    as_numpy = not torch.is_tensor(vertices)
    v_in = vertices if torch.is_tensor(vertices) else np.asarray(vertices)
    t_in = triangles if torch.is_tensor(triangles) else np.asarray(triangles)
    if v_in.ndim != 2 or v_in.shape[1] != 3 or t_in.ndim != 2 or t_in.shape[1] != 3:
        raise ValueError("simplify_mesh needs vertices [V,3] and triangles [F,3], got %s and %s" % (tuple(v_in.shape), tuple(t_in.shape)))
    attributes = list(attributes)
    for x in attributes:
        if x.shape[0] != v_in.shape[0]:
            raise ValueError("an attribute has %d rows for %d vertices" % (x.shape[0], v_in.shape[0]))
    dev = _device_of(v_in, t_in)
    to_dev = lambda x: x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    v, t = to_dev(v_in), to_dev(t_in)
    if not v.is_floating_point() or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("simplify_mesh needs float vertices and integer triangles, got %s and %s" % (v.dtype, t.dtype))
    t_dtype = t.dtype
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    kw = {} if eps is None else {"eps": eps}
    tried = None
    with torch.cuda.device(dev):
        if adaptive:
            tree = mesh.cluster_octree(v, t, cell_size, levels, origin=origin, **kw)
            if target_faces is not None:
                tolerance, tried = find_tolerance(tree, target_faces)
            res = mesh.simplify_mesh(v, t, cell_size, origin=origin, attributes=[to_dev(x) for x in attributes], tolerance=tolerance,
                                     levels=levels, tree=tree, **kw)
        else:
            if target_faces is not None:
                cell_size, tried = find_cell_size(v, t, target_faces, origin=origin)
            res = mesh.simplify_mesh(v, t, cell_size, origin=origin, placement=placement, attributes=[to_dev(x) for x in attributes], **kw)
    if tried is not None:
        res["report"].update(target_faces=int(target_faces), tried=[[float(h), int(n)] for h, n in tried])
    res["triangles"] = res["triangles"].to(t_dtype)
    if as_numpy:
        for k in ("vertices", "triangles", "vertex_cluster", "status") + (("level",) if adaptive else ()):
            res[k] = res[k].cpu().numpy()
    res["attributes"] = [x if torch.is_tensor(a) else x.cpu().numpy() for a, x in zip(attributes, res["attributes"])]
    return res
