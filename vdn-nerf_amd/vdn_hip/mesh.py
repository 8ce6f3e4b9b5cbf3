"""Iso-surface of a device lattice (reference renderer.py:36 calls mcubes.marching_cubes there), two forms:
  marching_cubes  - vdn_mesh_mc_count / vdn_mesh_mc_emit: the classic 256-case marching cubes with PyMCubes' own vertex and
                    triangle numbering (include/vdn_render.h; the default of extract_geometry since round 6);
  marching_tets   - vdn_mesh_count / vdn_mesh_emit: marching tetrahedra on the Kuhn decomposition (rounds 3-5), kept as an option.
  marching_cubes_sparse - vdn_mesh_sparse_*: marching_cubes' arrays from the bricks near the surface only; the field is given as a
                    function and evaluated at those bricks' nodes, never on the full lattice (csrc/mesh_sparse.hip).
The prefix sums (and the tetrahedra form's vertex welding) are torch ops on the device; nothing runs on the host.

shade_points evaluates the networks at free-standing surface points - the vertex attributes of a mesh that goes to disk
(NeuSRenderer.extract_colored_geometry, vdn_train.validate.validate_mesh).

Mesh cleaning (csrc/mesh_clean.hip; the policy on top is vdn_train/mesh_clean.py): connected_components / component_table label
the pieces of a mesh, dilate_masks / mask_votes count in how many object masks a vertex falls, filter_mesh drops faces and
vertices and renumbers the rest.

Ray casting (csrc/mesh_ray.hip): MeshGrid references the triangles from a uniform grid and casts rays against them (closest hit
or any hit, two-sided Moller-Trumbore in double); visibility_votes counts the cameras that see each vertex unoccluded.

Simplification (csrc/mesh_simplify.hip; the front door is vdn_train/mesh_simplify.py): cluster_quadrics groups the vertices by the
cells of a uniform grid and sums each cluster's quadric in a fixed order, simplify_mesh places one vertex per cluster and emits the
triangles that survive, count_simplified_faces is the count-only pass a face budget is searched with.

Textured meshes (csrc/mesh_texture.hip; the front door is vdn_train/mesh_texture.py): texture_layout gives every face a triangular
patch of a per-face atlas, texel_points / project_points place a surface point under every texel, gather_atlas writes the shaded
colours into the atlas, bake_texture is the three in a row; sample_texture looks an atlas up at points of the mesh and
render_textured_view does that where rays hit. photo_colors (csrc/mesh_photo.hip) colours the texel points from the photographs
that see them instead of the colour network - bake_texture(photos=...)."""
import math

import numpy as np
import torch

from . import lib, switches


def marching_tets(u, threshold=0.0):
    """u [R,R,R] fp32 CUDA tensor -> (vertices [V,3] fp32 in lattice index coordinates, triangles [F,3] int64)."""
    if not (torch.is_tensor(u) and u.is_cuda and u.dim() == 3 and u.shape[0] == u.shape[1] == u.shape[2]):
        raise ValueError("marching_tets needs a cubic [R,R,R] CUDA tensor")
    u = u.contiguous().float()
    R = u.shape[0]
    if R < 2:
        raise ValueError("lattice resolution must be at least 2")
    st = torch.cuda.current_stream().cuda_stream
    n = (R - 1) ** 3
    counts = torch.empty(n, dtype=torch.int32, device=u.device)
    a = lib.VdnMeshArgs()
    a.u, a.threshold, a.R, a.counts = u.data_ptr(), float(threshold), R, counts.data_ptr()
    lib.call("vdn_mesh_count", a, st)
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    n_tri = int(incl[-1].item())
    if n_tri == 0:
        return torch.zeros(0, 3, device=u.device), torch.zeros(0, 3, dtype=torch.int64, device=u.device)
    offsets = (incl - counts).contiguous()
    pos = torch.empty(n_tri, 3, 3, dtype=torch.float32, device=u.device)
    key = torch.empty(n_tri, 3, dtype=torch.int64, device=u.device)
    a.offsets, a.tri_pos, a.tri_key = offsets.data_ptr(), pos.data_ptr(), key.data_ptr()
    lib.call("vdn_mesh_emit", a, st)
    # weld: one vertex per cut lattice edge
    uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)
    first = torch.full((uniq.numel(),), n_tri * 3, dtype=torch.int64, device=u.device)
    first.scatter_reduce_(0, inv, torch.arange(n_tri * 3, device=u.device), reduce="amin")
    vertices = pos.reshape(-1, 3)[first]
    return vertices, inv.reshape(n_tri, 3)


def marching_cubes(u, threshold=0.0):
    """u [R,R,R] fp32 CUDA tensor -> (vertices [V,3] float64 in lattice index coordinates, triangles [F,3] int64): the two arrays
    `mcubes.marching_cubes(u, threshold)` returns (PyMCubes 0.1.2, as restated in oracle/marching_cubes.py), element for element."""
    if not (torch.is_tensor(u) and u.is_cuda and u.dim() == 3 and u.shape[0] == u.shape[1] == u.shape[2]):
        raise ValueError("marching_cubes needs a cubic [R,R,R] CUDA tensor")
    u = u.contiguous().float()
    R = u.shape[0]
    if R < 2:
        raise ValueError("lattice resolution must be at least 2")
    st = torch.cuda.current_stream().cuda_stream
    n, dev = (R - 1) ** 3, u.device
    case = torch.empty(n, dtype=torch.uint8, device=dev)
    nv, nt = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    a = lib.VdnMeshMcArgs()
    # (the library's array entry point takes the level as a C float - `_mcubes.pyx`: `float isovalue` - before its C++ code widens it)
    a.u, a.isovalue, a.R = u.data_ptr(), float(torch.tensor(float(threshold), dtype=torch.float32).item()), R
    a.cube_case, a.n_verts, a.n_tris = case.data_ptr(), nv.data_ptr(), nt.data_ptr()
    lib.call("vdn_mesh_mc_count", a, st)
    iv, it = torch.cumsum(nv, 0, dtype=torch.int64), torch.cumsum(nt, 0, dtype=torch.int64)
    totals = torch.stack([iv[-1], it[-1]]).tolist()          # one host read: the sizes of the two outputs
    V, F = int(totals[0]), int(totals[1])
    vertices = torch.empty(V, 3, dtype=torch.float64, device=dev)
    triangles = torch.empty(F, 3, dtype=torch.int64, device=dev)
    if F == 0:
        return vertices, triangles
    vo, to = (iv - nv).contiguous(), (it - nt).contiguous()
    a.vert_offsets, a.tri_offsets, a.vertices, a.triangles = vo.data_ptr(), to.data_ptr(), vertices.data_ptr(), triangles.data_ptr()
    lib.call("vdn_mesh_mc_emit", a, st)
    return vertices, triangles


class SparseExtractionError(RuntimeError):
    """marching_cubes_sparse found the surface leaving the bricks it evaluated: the Lipschitz bound does not hold for this field."""


# The default bound on |grad f| that decides which bricks marching_cubes_sparse evaluates. A POLICY, not a measurement: the eikonal
# term trains |grad f| of the SDF network towards 1, and 2 is a factor of two over that. A field steeper than the bound is caught
# only where the surface leaves an evaluated brick (the missed-edge check); tools/time_mesh_extract.py records the largest
# |grad f| it sees on the lattice nodes so that a reader can judge the margin.
SPARSE_LIPSCHITZ = 2.0
# A brick's radius is inflated by this relative slack, plus one fp32 ulp of the largest |coordinate| of the lattice, before the
# test: the brick's midpoint is rounded to fp32 (at most half an ulp per axis) and the radius is computed from rounded nodes.
SPARSE_RADIUS_SLACK = 1e-5
SPARSE_KEYS = ("brick", "lipschitz", "chunk_points")


def check_sparse_options(brick=8, lipschitz=SPARSE_LIPSCHITZ, chunk_points=1 << 22):
    """-> (brick, lipschitz, chunk_points) as int, float, int; ValueError on brick < 1, lipschitz <= 0 or NaN (inf is legal: every
    brick is evaluated), chunk_points < 1. Touches no device."""
    try:
        b, L, c = int(brick), float(lipschitz), int(chunk_points)
    except (TypeError, ValueError):
        raise ValueError("brick, lipschitz and chunk_points must be numbers, got %r, %r, %r" % (brick, lipschitz, chunk_points))
    if b != brick or b < 1:
        raise ValueError("brick must be an integer >= 1, got %r" % (brick,))
    if not L > 0.0:                                          # (NaN fails every comparison)
        raise ValueError("lipschitz must be positive (inf allowed), got %r" % (lipschitz,))
    if c != chunk_points or c < 1:
        raise ValueError("chunk_points must be an integer >= 1, got %r" % (chunk_points,))
    return b, L, c


def _query(query_func, pts, counter):
    counter[0] += pts.shape[0]
    val = query_func(pts)
    if not (torch.is_tensor(val) and val.numel() == pts.shape[0]):
        raise ValueError("query_func must return one value per point")
    return val.reshape(-1).float()


def marching_cubes_sparse(query_func, X, Y, Z, threshold=0.0, brick=8, lipschitz=SPARSE_LIPSCHITZ, chunk_points=1 << 22):
    """marching_cubes(u, threshold) of the lattice u[i,j,k] = query_func((X[i], Y[j], Z[k])) without ever filling u ->
    (vertices [V,3] float64 in lattice index coordinates, triangles [F,3] int64, stats). X, Y, Z: the lattice's coordinate
    vectors, fp32 [R] CUDA tensors of one length (torch.linspace(lo, hi, R) per axis reproduces extract_fields_device's floats);
    query_func maps [P,3] device points to P values, each row on its own (the same point must give the same bits in any batch).

    The (R-1)^3 cells are cut into bricks of brick^3 cells (the last per axis may be partial; R - 1 < brick gives one brick).
    Coarse pass: one evaluation per brick at the midpoint c of its closed node box; the brick is ACTIVE when
    |f(c) - level| <= lipschitz * r, r = half the world-space diagonal of that box, in double, inflated by SPARSE_RADIUS_SLACK
    (relative) plus one fp32 ulp of the largest |coordinate|. If |grad f| <= lipschitz inside a dropped brick, f keeps one sign on it
    and none of its cells is cut. lipschitz = inf keeps every brick. Fine pass: the nodes of the active bricks, (brick+1)^3 per
    brick (shared faces are evaluated once per brick), at most chunk_points per query_func call. The active cells are then
    triangulated in ascending global cell number (csrc/mesh_sparse.hip), which makes the two arrays equal to marching_cubes' on
    the dense lattice, element for element, whenever no dropped brick holds a cut cell.

    stats = {"bricks", "active_bricks", "points_evaluated" (every point handed to query_func, coarse pass included),
    "missed_edges"}. The check behind missed_edges: for every cut lattice edge of an active cell, every existing cell that contains
    the edge must lie in an active brick. A violation means the surface leaves the evaluated region - the bound is too small for
    this field - and raises SparseExtractionError. What it cannot see: a component of the surface that lies WHOLLY inside dropped
    bricks (no active cell touches it); only a true bound excludes that.

    Two host reads: the number of active bricks, then (V, F, missed). ValueError on CPU tensors, wrong shapes, bad options, or
    sizes beyond 32-bit indexing (status -10 of the entry points)."""
    brick, lipschitz, chunk_points = check_sparse_options(brick, lipschitz, chunk_points)
    for name, t in (("X", X), ("Y", Y), ("Z", Z)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 1 and t.dtype == torch.float32):
            raise ValueError("marching_cubes_sparse needs %s as an fp32 [R] CUDA tensor" % name)
    if not (X.shape == Y.shape == Z.shape and X.device == Y.device == Z.device):
        raise ValueError("X, Y and Z must have one length and one device")
    R, dev = X.shape[0], X.device
    if R < 2:
        raise ValueError("lattice resolution must be at least 2")
    X, Y, Z = X.contiguous(), Y.contiguous(), Z.contiguous()
    n = R - 1
    B = min(brick, n)                                        # (one brick when R - 1 < brick: its block is the lattice)
    nb, E = -(-n // B), B + 1
    if nb ** 3 >= 1 << 31:
        raise ValueError("marching_cubes_sparse: the sizes do not fit 32-bit indexing")
    level = float(torch.tensor(float(threshold), dtype=torch.float32).item())      # a C float, as marching_cubes takes it
    counter = [0]
    with torch.cuda.device(dev), torch.no_grad():
        st = lib.stream_handle()
        # ---- coarse pass: one value per brick against lipschitz * radius
        lo_i = torch.arange(nb, device=dev) * B
        hi_i = (lo_i + B).clamp_max(n)
        ends = [(A[lo_i].double(), A[hi_i].double()) for A in (X, Y, Z)]
        mid = [((a + b) * 0.5).float() for a, b in ends]
        ext = [b - a for a, b in ends]
        ulp = torch.stack([X.abs().max(), Y.abs().max(), Z.abs().max()]).max().double() * 2.0 ** -23
        width = (hi_i - lo_i).to(torch.int64)                # cells per brick along one axis
        active = torch.empty(nb ** 3, dtype=torch.bool, device=dev)
        for s in range(0, nb ** 3, chunk_points):
            b = torch.arange(s, min(s + chunk_points, nb ** 3), device=dev)
            bi, bj, bk = b // (nb * nb), (b // nb) % nb, b % nb
            f = _query(query_func, torch.stack([mid[0][bi], mid[1][bj], mid[2][bk]], dim=-1), counter)
            r = 0.5 * torch.sqrt(ext[0][bi] ** 2 + ext[1][bj] ** 2 + ext[2][bk] ** 2)
            # closed test, written so that a NaN value keeps its brick
            active[s:s + b.numel()] = ~((f.double() - level).abs() > lipschitz * (r * (1.0 + SPARSE_RADIUS_SLACK) + ulp))
        act = torch.nonzero(active).reshape(-1)              # host read 1: the number of active bricks
        A = int(act.shape[0])
        stats = {"bricks": nb ** 3, "active_bricks": A, "points_evaluated": counter[0], "missed_edges": 0}
        vertices = torch.empty(0, 3, dtype=torch.float64, device=dev)
        triangles = torch.empty(0, 3, dtype=torch.int64, device=dev)
        if A == 0:
            return vertices, triangles, stats
        if A * E ** 3 >= 1 << 31:
            raise ValueError("marching_cubes_sparse: %d active bricks of %d^3 nodes do not fit 32-bit indexing" % (A, E))
        act32 = act.to(torch.int32)
        # ---- fine pass: the nodes of the active bricks, in chunks
        values = torch.empty(A * E ** 3, dtype=torch.float32, device=dev)
        na = lib.VdnMeshSparseNodesArgs()
        na.X, na.Y, na.Z, na.active = X.data_ptr(), Y.data_ptr(), Z.data_ptr(), act32.data_ptr()
        na.R, na.brick, na.nb, na.A = R, B, nb, A
        pts = torch.empty(min(chunk_points, A * E ** 3), 3, dtype=torch.float32, device=dev)
        for s in range(0, A * E ** 3, chunk_points):
            m = min(chunk_points, A * E ** 3 - s)
            na.points, na.first, na.n_points = pts.data_ptr(), s, m
            _call_sized("vdn_mesh_sparse_nodes", na, st)
            values[s:s + m] = _query(query_func, pts[:m], counter)
        del pts
        stats["points_evaluated"] = counter[0]
        # ---- the brick tables of the compact cell order (include/vdn_render.h: the rank formula)
        act3 = active.reshape(nb, nb, nb).to(torch.int64)
        zcells = act3 * width[None, None, :]                 # active cells of one (i, j) column inside each brick
        col = zcells.sum(dim=2)                              # [nb, nb]  col_cells
        colw = col * width[None, :]
        row = colw.sum(dim=1)                                # [nb]      row_cells
        roww = row * width
        base = ((torch.cumsum(roww, 0) - roww)[:, None, None] + (torch.cumsum(colw, 1) - colw)[:, :, None] + (torch.cumsum(zcells, 2) - zcells))
        # the compact arrays' length: exact when no brick is partial, else an upper bound whose unused tail stays zero (the true
        # count is a device value; zeros add nothing to the prefix sums)
        n_cells = A * B ** 3
        brick_map = torch.full((nb ** 3,), -1, dtype=torch.int32, device=dev)
        brick_map[act] = torch.arange(A, dtype=torch.int32, device=dev)
        base32, col32, row32 = base.reshape(-1).to(torch.int32), col.reshape(-1).to(torch.int32), row.to(torch.int32)
        case = torch.zeros(n_cells, dtype=torch.uint8, device=dev)
        nv, nt = torch.zeros(n_cells, dtype=torch.int32, device=dev), torch.zeros(n_cells, dtype=torch.int32, device=dev)
        missed = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnMeshSparseArgs()
        a.values, a.isovalue, a.R, a.brick, a.nb, a.A = values.data_ptr(), level, R, B, nb, A
        a.active, a.brick_map, a.cell_base = act32.data_ptr(), brick_map.data_ptr(), base32.data_ptr()
        a.col_cells, a.row_cells, a.n_cells = col32.data_ptr(), row32.data_ptr(), n_cells
        a.cube_case, a.n_verts, a.n_tris, a.missed = case.data_ptr(), nv.data_ptr(), nt.data_ptr(), missed.data_ptr()
        _call_sized("vdn_mesh_sparse_count", a, st)
        iv, it = torch.cumsum(nv, 0, dtype=torch.int64), torch.cumsum(nt, 0, dtype=torch.int64)
        V, F, bad = torch.stack([iv[-1], it[-1], missed[0].long()]).tolist()       # host read 2: the output sizes and the check
        stats["missed_edges"] = int(bad)
        if bad:
            raise SparseExtractionError(
                "sparse extraction missed the surface at %d lattice edges: a cut edge of an evaluated cell borders a brick that "
                "lipschitz = %g dropped. Raise `lipschitz` (the field is steeper than the bound) or extract densely (sparse=None)."
                % (bad, lipschitz))
        vertices = torch.empty(int(V), 3, dtype=torch.float64, device=dev)
        triangles = torch.empty(int(F), 3, dtype=torch.int64, device=dev)
        if F == 0:
            return vertices, triangles, stats
        vo, to = (iv - nv).contiguous(), (it - nt).contiguous()
        a.vert_offsets, a.tri_offsets, a.V, a.F = vo.data_ptr(), to.data_ptr(), int(V), int(F)
        a.vertices, a.triangles = vertices.data_ptr(), triangles.data_ptr()
        _call_sized("vdn_mesh_sparse_emit", a, st)
    return vertices, triangles, stats


def sample_surface(vertices, triangles, spacing, max_samples=1 << 26):
    """Area-weighted, deterministic samples of a triangle mesh (vdn_surf_count / vdn_surf_emit, include/vdn_render.h):
    vertices [V,3] CUDA float, triangles [F,3] CUDA int64 or int32 -> (points [S,3] fp32, face [S] int32, counts [F] int32).
    Triangle f gets counts[f] = ceil(area_f / spacing^2) samples (0 for a zero or non-finite area), sample j at the R2
    low-discrepancy point j + 1 folded into the triangle; no random state, two calls give the same bits. ValueError on CPU
    tensors, wrong shapes, spacing <= 0, a corner index outside [0, V), or more than max_samples samples (checked on the
    counts, before the outputs are allocated)."""
    if not (torch.is_tensor(vertices) and vertices.is_cuda and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.is_floating_point()):
        raise ValueError("sample_surface needs vertices as a float [V,3] CUDA tensor")
    if not (torch.is_tensor(triangles) and triangles.is_cuda and triangles.dim() == 2 and triangles.shape[1] == 3 and
            triangles.dtype in (torch.int64, torch.int32)):
        raise ValueError("sample_surface needs triangles as an int64 or int32 [F,3] CUDA tensor")
    if triangles.device != vertices.device:
        raise ValueError("vertices and triangles must be on the same device")
    if not (float(spacing) > 0.0 and float(spacing) < float("inf")):
        raise ValueError("spacing must be positive and finite, got %r" % (spacing,))
    dev = vertices.device
    v, t = vertices.detach().float().contiguous(), triangles.contiguous()
    V, F = v.shape[0], t.shape[0]
    if F == 0:
        return (torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        st = lib.stream_handle()
        counts = torch.empty(F, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnSurfArgs()
        a.vertices, a.triangles, a.spacing, a.V, a.F = v.data_ptr(), t.data_ptr(), float(spacing), V, F
        a.index_bytes, a.counts, a.error = t.element_size(), counts.data_ptr(), err.data_ptr()
        _call_sized("vdn_surf_count", a, st)
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        S, bad = torch.stack([incl[-1], err[0].long()]).tolist()         # one host read: the output size and the error flag
        if bad:
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
        if S > max_samples or S >= 1 << 31:
            raise ValueError("spacing %g gives %d samples, more than max_samples = %d (or than 32-bit indexing holds)" % (spacing, S, max_samples))
        points = torch.empty(S, 3, dtype=torch.float32, device=dev)
        face = torch.empty(S, dtype=torch.int32, device=dev)
        if S > 0:
            offsets = (incl - counts).contiguous()
            a.S, a.offsets, a.points, a.face = S, offsets.data_ptr(), points.data_ptr(), face.data_ptr()
            _call_sized("vdn_surf_emit", a, st)
    return points, face, counts


def _call_sized(name, *args):
    """lib.call for the entry points that decline sizes beyond 32-bit indexing with status -10: that is the caller's ValueError."""
    if not lib.try_call(name, *args):
        raise ValueError("%s: the sizes do not fit 32-bit indexing" % name)


# ---- mesh cleaning ----------------------------------------------------------------------------------------------------------------
def _check_triangles(name, triangles):
    if not (torch.is_tensor(triangles) and triangles.is_cuda and triangles.dim() == 2 and triangles.shape[1] == 3 and
            triangles.dtype in (torch.int64, torch.int32)):
        raise ValueError("%s needs triangles as an int64 or int32 [F,3] CUDA tensor" % name)


def _check_vertices(name, vertices, triangles=None):
    if not (torch.is_tensor(vertices) and vertices.is_cuda and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.is_floating_point()):
        raise ValueError("%s needs vertices as a float [V,3] CUDA tensor" % name)
    if triangles is not None and triangles.device != vertices.device:
        raise ValueError("vertices and triangles must be on the same device")


def connected_components(triangles, n_vertices):
    """Connected components of a triangle mesh (vdn_cc_union / vdn_cc_flatten, include/vdn_render.h): triangles [F,3] CUDA int64 or
    int32 over n_vertices vertices -> labels [V] int32, labels[v] = the smallest vertex index of v's component. Two triangles are
    connected when they share a vertex index; a vertex in no triangle is its own component. The labels do not depend on the thread
    order or on the order of the triangles. ValueError on CPU tensors, wrong shapes, n_vertices < 0 or a corner outside [0, V)."""
    _check_triangles("connected_components", triangles)
    V = int(n_vertices)
    if V < 0:
        raise ValueError("n_vertices must not be negative, got %r" % (n_vertices,))
    dev, t = triangles.device, triangles.contiguous()
    F = t.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError("connected_components: the sizes do not fit 32-bit indexing")
    if V == 0:
        if F > 0:
            raise ValueError("a triangle refers to a vertex outside [0, 0)")
        return torch.empty(0, dtype=torch.int32, device=dev)
    parent = torch.arange(V, dtype=torch.int32, device=dev)
    if F == 0:
        return parent
    with torch.cuda.device(dev):
        st = lib.stream_handle()
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnCcArgs()
        a.triangles, a.parent, a.label, a.error = t.data_ptr(), parent.data_ptr(), labels.data_ptr(), err.data_ptr()
        a.V, a.F, a.index_bytes = V, F, t.element_size()
        _call_sized("vdn_cc_union", a, st)
        _call_sized("vdn_cc_flatten", a, st)
        if int(err.item()):                                   # one host read: the error flag
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
    return labels


def triangle_areas(vertices, triangles):
    """area [F] float64 of each triangle, 0.5 |(b - a) x (c - a)| in double from the fp32 vertices (vdn_tri_area: the expression
    sample_surface counts with), 0 where it is not finite."""
    _check_triangles("triangle_areas", triangles)
    _check_vertices("triangle_areas", vertices, triangles)
    dev = vertices.device
    v, t = vertices.detach().float().contiguous(), triangles.contiguous()
    V, F = v.shape[0], t.shape[0]
    area = torch.empty(F, dtype=torch.float64, device=dev)
    if F == 0:
        return area
    if V == 0:
        raise ValueError("a triangle refers to a vertex outside [0, 0)")
    with torch.cuda.device(dev):
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnTriAreaArgs()
        a.vertices, a.triangles, a.area, a.error = v.data_ptr(), t.data_ptr(), area.data_ptr(), err.data_ptr()
        a.V, a.F, a.index_bytes = V, F, t.element_size()
        _call_sized("vdn_tri_area", a, lib.stream_handle())
        if int(err.item()):
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
    return area


def component_table(vertices, triangles, labels):
    """The components of connected_components' labels, ordered by label (ascending root index) -> dict of device tensors:
    root [C] int64, n_vertices [C] and n_faces [C] int64 (exact), area [C] float64 (the sum of face_area), face_component [F] and
    vertex_component [V] int64 (dense ids into the table), face_area [F] float64 (triangle_areas)."""
    _check_triangles("component_table", triangles)
    _check_vertices("component_table", vertices, triangles)
    V = vertices.shape[0]
    if not (torch.is_tensor(labels) and labels.device == vertices.device and labels.shape == (V,) and labels.dtype in (torch.int32, torch.int64)):
        raise ValueError("component_table needs labels as an int32 [V] tensor on the vertices' device")
    face_area = triangle_areas(vertices, triangles)          # (checks the corner indices)
    root, vertex_component = torch.unique(labels.long(), sorted=True, return_inverse=True)
    C = root.shape[0]
    face_component = vertex_component[triangles[:, 0].long()]
    area = torch.zeros(C, dtype=torch.float64, device=vertices.device).index_add_(0, face_component, face_area)
    return {"root": root, "n_vertices": torch.bincount(vertex_component, minlength=C), "n_faces": torch.bincount(face_component, minlength=C),
            "area": area, "face_component": face_component, "vertex_component": vertex_component, "face_area": face_area}


def _check_masks(name, masks):
    if not (torch.is_tensor(masks) and masks.is_cuda and masks.dim() == 3 and masks.dtype == torch.uint8 and masks.numel() > 0):
        raise ValueError("%s needs masks as a non-empty uint8 [N,H,W] CUDA tensor (nonzero = set)" % name)


def dilate_masks(masks, radius):
    """masks uint8 [N,H,W] CUDA (nonzero = set) -> uint8 [N,H,W]: the maximum over the (2 radius + 1)^2 square around each pixel,
    pixels outside the image counting as unset (vdn_mask_dilate: cv.dilate with a kernel of ones). radius = 0 copies."""
    _check_masks("dilate_masks", masks)
    if int(radius) != radius or radius < 0:
        raise ValueError("radius must be a non-negative integer, got %r" % (radius,))
    m = masks.contiguous()
    out, scratch = torch.empty_like(m), torch.empty_like(m)
    a = lib.VdnMaskDilateArgs()
    a.src, a.scratch, a.dst = m.data_ptr(), scratch.data_ptr(), out.data_ptr()
    a.N, a.H, a.W, a.radius = m.shape[0], m.shape[1], m.shape[2], min(int(radius), max(m.shape[1], m.shape[2]))
    with torch.cuda.device(m.device):
        _call_sized("vdn_mask_dilate", a, lib.stream_handle())
    return out


def mask_votes(vertices, P, masks):
    """vertices [V,3] CUDA float, P [N,3,4] float64 (the mesh's own frame -> (u w, v w, w)), masks uint8 [N,H,W] CUDA ->
    (n_in_image [V] int32, n_in_mask [V] int32): the cameras a vertex projects into (w > 0, pixel floor(u + 0.5), floor(v + 0.5)
    inside the image) and those of them whose mask is set there (vdn_mask_votes)."""
    _check_vertices("mask_votes", vertices)
    _check_masks("mask_votes", masks)
    if masks.device != vertices.device:
        raise ValueError("vertices and masks must be on the same device")
    P = torch.as_tensor(P)
    if P.shape != (masks.shape[0], 3, 4) or not P.is_floating_point():
        raise ValueError("P must be a float [N,3,4] = %s array, got %s" % ((masks.shape[0], 3, 4), tuple(P.shape)))
    dev = vertices.device
    v, m = vertices.detach().float().contiguous(), masks.contiguous()
    Pd = P.detach().to(device=dev, dtype=torch.float64).contiguous()
    V = v.shape[0]
    n_img, n_msk = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    if V == 0:
        return n_img, n_msk
    a = lib.VdnMaskVotesArgs()
    a.vertices, a.P, a.masks, a.n_in_image, a.n_in_mask = v.data_ptr(), Pd.data_ptr(), m.data_ptr(), n_img.data_ptr(), n_msk.data_ptr()
    a.V, a.N, a.H, a.W = V, m.shape[0], m.shape[1], m.shape[2]
    with torch.cuda.device(dev):
        _call_sized("vdn_mask_votes", a, lib.stream_handle())
    return n_img, n_msk


def _keep_bytes(name, keep, n, dev):
    if keep is None:
        return None
    if not (torch.is_tensor(keep) and keep.device == dev and keep.shape == (n,) and keep.dtype in (torch.bool, torch.uint8)):
        raise ValueError("%s must be a bool [%d] tensor on the mesh's device" % (name, n))
    return (keep != 0).contiguous().view(torch.uint8)


def filter_mesh(vertices, triangles, keep_vertices=None, keep_faces=None, drop_unreferenced=True):
    """Drop faces and vertices and renumber the rest (vdn_mesh_filter_mark / vdn_mesh_filter_remap) ->
    (vertices' [V',3], triangles' [F',3], vertex_index [V'] int64). A face survives iff keep_faces[f] (bool [F], optional) and
    keep_vertices (bool [V], optional) of its three corners; a vertex survives iff keep_vertices[v] and, with drop_unreferenced,
    a surviving face uses it. Order and dtypes are the inputs'; vertex_index holds the old index of each new vertex, so
    per-vertex attributes follow by one gather. ValueError on CPU tensors, wrong shapes or a corner outside [0, V)."""
    _check_triangles("filter_mesh", triangles)
    _check_vertices("filter_mesh", vertices, triangles)
    dev = vertices.device
    t = triangles.contiguous()
    V, F = vertices.shape[0], t.shape[0]
    kv, kf = _keep_bytes("keep_vertices", keep_vertices, V, dev), _keep_bytes("keep_faces", keep_faces, F, dev)
    used = torch.zeros(V, dtype=torch.uint8, device=dev)
    alive = torch.zeros(F, dtype=torch.uint8, device=dev)
    if F > 0 and V == 0:
        raise ValueError("a triangle refers to a vertex outside [0, 0)")
    with torch.cuda.device(dev):
        st = lib.stream_handle()
        a = lib.VdnMeshFilterArgs()
        n_alive = 0
        if F > 0:
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            a.triangles, a.face_alive, a.vertex_used, a.error = t.data_ptr(), alive.data_ptr(), used.data_ptr(), err.data_ptr()
            a.keep_face, a.keep_vertex = (None if kf is None else kf.data_ptr()), (None if kv is None else kv.data_ptr())
            a.V, a.F, a.index_bytes = V, F, t.element_size()
            _call_sized("vdn_mesh_filter_mark", a, st)
            f_incl = torch.cumsum(alive, 0, dtype=torch.int64)
            n_alive, bad = torch.stack([f_incl[-1], err[0].long()]).tolist()      # one host read: the output size and the error flag
            if bad:
                raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
        keep_v = used if drop_unreferenced else (kv if kv is not None else torch.ones(V, dtype=torch.uint8, device=dev))
        v_incl = torch.cumsum(keep_v, 0, dtype=torch.int64)
        vertex_index = torch.nonzero(keep_v).reshape(-1)
        out_t = torch.empty(n_alive, 3, dtype=t.dtype, device=dev)
        if n_alive > 0:
            f_off, v_new = (f_incl - alive).contiguous(), (v_incl - keep_v).contiguous()
            a.face_offsets, a.vertex_new, a.out_triangles, a.F_out = f_off.data_ptr(), v_new.data_ptr(), out_t.data_ptr(), n_alive
            _call_sized("vdn_mesh_filter_remap", a, st)
    return vertices[vertex_index], out_t, vertex_index


# ---- ray casting against the mesh (csrc/mesh_ray.hip) ---------------------------------------------------------------------------------
# default cell edge, in units of the mean triangle extent (the longest side of a triangle's own box): a marching-cubes triangle
# then overlaps about (1 + 1/2)^3 = 3.4 cells and a ray takes half as many steps as at one extent per cell. An expectation, not a
# measurement.
RAY_CELL_FACTOR = 2.0
# the grown boxes' margin, in units of (largest |coordinate| of the box + largest extent + h): 2^-32, i.e. 2^21 ulps of fp64 -
# DESIGN.md 3m has the argument
RAY_MARGIN = 2.0 ** -32


class MeshGrid:
    """The triangles of a mesh referenced from a dense uniform grid over the bounding box of its referenced, finite vertices
    (vdn_ray_bin_count / vdn_ray_bin_fill, include/vdn_render.h), for `cast`. vertices [V,3] CUDA float (taken as fp32), triangles
    [F,3] CUDA int64 or int32. A triangle with a non-finite corner, a repeated corner index or zero area is never referenced; F = 0
    is legal (every ray misses). cell_size: the cells' edge - default RAY_CELL_FACTOR * the mean triangle extent - raised by steps
    of 1.25 until the grid has at most max_cells cells; it changes the speed only, never a result. ValueError on CPU tensors, wrong
    shapes or dtypes, a corner index outside [0, V) (found on the device), or more than max_refs references (checked after the
    count pass, before the list is allocated: one huge triangle over a fine grid)."""

    def __init__(self, vertices, triangles, cell_size=None, max_cells=1 << 22, max_refs=1 << 27):
        _check_triangles("MeshGrid", triangles)
        _check_vertices("MeshGrid", vertices, triangles)
        if max_cells < 1 or max_refs < 1:
            raise ValueError("max_cells and max_refs must be at least 1")
        if cell_size is not None and not (float(cell_size) > 0.0 and float(cell_size) < float("inf")):
            raise ValueError("cell_size must be positive and finite, got %r" % (cell_size,))
        dev = vertices.device
        v, t = vertices.detach().float().contiguous(), triangles.contiguous()
        V, F = v.shape[0], t.shape[0]
        if V >= 1 << 31 or F >= 1 << 31:
            raise ValueError("MeshGrid: the sizes do not fit 32-bit indexing")
        if F > 0 and V == 0:
            raise ValueError("a triangle refers to a vertex outside [0, 0)")
        self.device, self.V, self.F = dev, V, F
        self.vertices, self.triangles = v, t                  # (the arrays the grid was built from: render_textured_view samples on them)
        lo, hi, mean_extent = [0.0] * 3, [0.0] * 3, 0.0
        with torch.cuda.device(dev):
            if F > 0:
                # the box and the mean extent over the triangles whose corners are in range and finite (gathered at safe indices)
                tl = t.long()
                ok = ((tl >= 0) & (tl < V)).all(dim=1)
                p = v[torch.where(ok[:, None], tl, torch.zeros_like(tl))]
                ok &= torch.isfinite(p).all(dim=2).all(dim=1)
                inf = torch.full((1, 3), float("inf"), device=dev)
                bmin, bmax = torch.where(ok[:, None], p.amin(dim=1), inf), torch.where(ok[:, None], p.amax(dim=1), -inf)
                n_ok = ok.sum()
                ext = torch.where(ok, (bmax - bmin).amax(dim=1), torch.zeros((), device=dev)).double().sum() / n_ok.clamp_min(1)
                stats = torch.cat([bmin.amin(dim=0).double(), bmax.amax(dim=0).double(), ext[None], n_ok[None].double()]).tolist()   # one host read
                if stats[7] > 0:
                    lo, hi, mean_extent = stats[0:3], stats[3:6], stats[6]
            extent = [b - a for a, b in zip(lo, hi)]
            L = max(extent)
            h = float(cell_size) if cell_size is not None else RAY_CELL_FACTOR * mean_extent
            if not (h > 0.0 and math.isfinite(h)):
                h = L if L > 0.0 else 1.0                          # (no triangle with an extent: one cell)
            dims = lambda s: [int(math.floor(e / s)) + 1 for e in extent]
            while np.prod(dims(h), dtype=object) > max_cells:
                h *= 1.25
            self.lo, self.h, self.dims = [float(x) for x in lo], h, dims(h)
            self.n_cells = int(np.prod(self.dims, dtype=object))
            self.margin = RAY_MARGIN * (max(abs(x) for x in lo + hi) + L + h)
            self.records = torch.empty(max(F, 1), 12, dtype=torch.float32, device=dev)
            count = torch.zeros(self.n_cells, dtype=torch.int32, device=dev)
            self.cell_start = torch.zeros(self.n_cells + 1, dtype=torch.int32, device=dev)
            self.n_refs = 0
            if F > 0:
                st = lib.stream_handle()
                err = torch.zeros(1, dtype=torch.int32, device=dev)
                a = self._geometry(lib.VdnRayGridArgs())
                a.vertices, a.triangles, a.V, a.F, a.index_bytes = v.data_ptr(), t.data_ptr(), V, F, t.element_size()
                a.cell_count, a.records, a.error = count.data_ptr(), self.records.data_ptr(), err.data_ptr()
                _call_sized("vdn_ray_bin_count", a, st)
                incl = torch.cumsum(count, 0, dtype=torch.int64)
                n_refs, bad = torch.stack([incl[-1], err[0].long()]).tolist()         # one host read: the list's size and the error flag
                if bad:
                    raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
                if n_refs > max_refs or n_refs >= 1 << 31:
                    raise ValueError("a cell size of %g gives %d triangle references, more than max_refs = %d (or than 32-bit indexing holds)"
                                     % (h, n_refs, max_refs))
                self.n_refs = int(n_refs)
                self.cell_start[1:] = incl.to(torch.int32)
            self.refs = torch.empty(max(self.n_refs, 1), dtype=torch.int32, device=dev)
            if self.n_refs > 0:
                cursor = self.cell_start[:-1].clone()
                a.cursor, a.refs, a.n_refs = cursor.data_ptr(), self.refs.data_ptr(), self.n_refs
                _call_sized("vdn_ray_bin_fill", a, st)
        self.nbytes = sum(x.numel() * x.element_size() for x in (self.records, self.cell_start, self.refs))

    def _geometry(self, a):
        """the grid's tables and geometry into an argument block (the fields every block of csrc/mesh_ray.hip names alike)"""
        a.lo_x, a.lo_y, a.lo_z, a.h, a.margin = self.lo[0], self.lo[1], self.lo[2], self.h, self.margin
        a.nx, a.ny, a.nz = self.dims
        if hasattr(a, "cell_start"):
            a.records, a.cell_start, a.refs = self.records.data_ptr(), self.cell_start.data_ptr(), self.refs.data_ptr()
            a.F, a.n_refs = self.F, self.n_refs
        return a

    def _rays(self, x, what):
        x = torch.as_tensor(x)
        if x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
            raise ValueError("%s must be a float [R,3] array, got %s %s" % (what, x.dtype, tuple(x.shape)))
        return x.detach().to(device=self.device, dtype=torch.float64).contiguous()

    def cast(self, origins, directions, t_min=0.0, t_max=float("inf"), any_hit=False, skip_vertex=None, return_tests=False):
        """Rays origins[r] + t directions[r] ([R,3], taken as float64) against the mesh -> (t [R] float64, face [R] int64): the
        closest hit with t_min < t < t_max, the lower face index on equal t; +inf and -1 on a miss (vdn_ray_cast: two-sided
        Moller-Trumbore in double, bit-identical between calls and across cell sizes). any_hit: stop at the first hit found -
        only face >= 0 means anything then. skip_vertex [R] integers (optional): the triangles with that vertex as a corner are
        ignored for that ray. return_tests adds tests [R] int32, the ray-triangle tests made per ray. Rays that are not finite,
        have no direction or an empty window miss. Pass the rays in a coherent order: a wave is as slow as its longest walk."""
        o, d = self._rays(origins, "origins"), self._rays(directions, "directions")
        if o.shape != d.shape:
            raise ValueError("origins and directions must have one shape, got %s and %s" % (tuple(o.shape), tuple(d.shape)))
        R, dev = o.shape[0], self.device
        skip = None
        if skip_vertex is not None:
            skip = torch.as_tensor(skip_vertex)
            if skip.shape != (R,) or skip.is_floating_point() or skip.dtype == torch.bool:
                raise ValueError("skip_vertex must be an integer [%d] array" % R)
            skip = skip.to(device=dev, dtype=torch.int64).contiguous()
        t = torch.full((R,), float("inf"), dtype=torch.float64, device=dev)
        face = torch.full((R,), -1, dtype=torch.int64, device=dev)
        tests = torch.zeros(R, dtype=torch.int32, device=dev) if return_tests else None
        if R > 0:
            a = self._geometry(lib.VdnRayCastArgs())
            a.origins, a.directions, a.skip_vertex = o.data_ptr(), d.data_ptr(), (None if skip is None else skip.data_ptr())
            a.t, a.face, a.tests, a.R = t.data_ptr(), face.data_ptr(), (tests.data_ptr() if return_tests else None), R
            a.t_min, a.t_max, a.any_hit = float(t_min), float(t_max), 1 if any_hit else 0
            with torch.cuda.device(dev):
                _call_sized("vdn_ray_cast", a, lib.stream_handle())
        return (t, face, tests) if return_tests else (t, face)


def camera_centres(P):
    """P float [N,3,4] = [M | p4] -> centres float64 [N,3] numpy, c = -M^-1 p4 (the point every ray of the camera passes through),
    on the host. ValueError when an M is singular."""
    P = np.asarray(P.detach().cpu() if torch.is_tensor(P) else P, dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] != (3, 4):
        raise ValueError("P must be a float [N,3,4] array, got %s" % (P.shape,))
    c = np.empty((P.shape[0], 3))
    for n in range(P.shape[0]):
        M = P[n, :, :3]
        # (rank by the singular values: a determinant's size says nothing about a matrix in pixels x metres)
        if not np.isfinite(P[n]).all() or np.linalg.matrix_rank(M) < 3:
            raise ValueError("camera %d has a singular 3 x 3 block: it has no centre" % n)
        c[n] = -np.linalg.solve(M, P[n, :, 3])
    return c


def visibility_votes(vertices, triangles, P, image_size, eps=1e-4, grid=None):
    """vertices [V,3] CUDA float, triangles [F,3] CUDA int64 or int32, P [N,3,4] float64 (as mask_votes takes it), image_size
    (H, W) -> (n_in_image [V] int32, n_visible [V] int32) (vdn_visibility_votes): the cameras a vertex projects into - mask_votes'
    rule - and those of them that see it: no triangle without the vertex as a corner is hit by the segment from the camera's
    centre c to the vertex x, c + t (x - c) with 0 < t < 1 - eps. eps keeps a position-duplicated, unwelded vertex of a foreign
    PLY (and the triangles around it) from hiding its twin; 1e-4 is an interface default, not a measurement. fp64 Moller-Trumbore
    has no watertight edge rule: a segment can in principle pass between two triangles along their shared edge, which adds one
    vote. grid: a MeshGrid of the same mesh (built here when None)."""
    _check_triangles("visibility_votes", triangles)
    _check_vertices("visibility_votes", vertices, triangles)
    try:
        H, W = (int(x) for x in image_size)
    except (TypeError, ValueError):
        raise ValueError("image_size must be (H, W), got %r" % (image_size,))
    if H < 1 or W < 1:
        raise ValueError("image_size must be positive, got %r" % (image_size,))
    if not (0.0 <= float(eps) < 1.0):
        raise ValueError("eps must be in [0, 1), got %r" % (eps,))
    centres = camera_centres(P)
    dev = vertices.device
    if grid is None:
        grid = MeshGrid(vertices, triangles)
    if not isinstance(grid, MeshGrid) or grid.device != dev or (grid.V, grid.F) != (vertices.shape[0], triangles.shape[0]):
        raise ValueError("grid must be a MeshGrid of this mesh")
    v = vertices.detach().float().contiguous()
    Pd = torch.as_tensor(P).detach().to(device=dev, dtype=torch.float64).contiguous()
    cd = torch.from_numpy(centres).to(dev)
    V, N = v.shape[0], Pd.shape[0]
    n_img, n_vis = torch.zeros(V, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.int32, device=dev)
    if V == 0 or N == 0:
        return n_img, n_vis
    a = grid._geometry(lib.VdnVisibilityArgs())
    a.vertices, a.P, a.centres, a.n_in_image, a.n_visible = v.data_ptr(), Pd.data_ptr(), cd.data_ptr(), n_img.data_ptr(), n_vis.data_ptr()
    a.V, a.N, a.H, a.W, a.eps = V, N, H, W, float(eps)
    with torch.cuda.device(dev):
        _call_sized("vdn_visibility_votes", a, lib.stream_handle())
    return n_img, n_vis


def fused_point_shading(renderer):
    """True where vdn_shade_points_bf16 (csrc/k_sdf_fwd2.h MODE 4) covers the configuration: both networks on the bf16 kernels and
    the colour head the "c2" stream exists for ('idr', d_feature 256, d_out 3). VDN_SHADE_POINTS_FUSED=0 forces the separate launches."""
    sn, cn = renderer.sdf_network, renderer.color_network
    return (switches.flag("VDN_SHADE_POINTS_FUSED") and sn.precision == "bf16" and cn.precision == "bf16"
            and cn.conf.get("mode") == "idr" and cn.conf.get("d_feature") == 256 and cn.conf.get("d_out") == 3)


def view_from_gradient(g):
    """The view direction a surface point is shaded with: straight down its normal, -g / max(|g|, 1e-12) - the convention of
    torch.nn.functional.normalize, so a zero gradient gives a zero direction, never NaN."""
    return -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def quantize_colors_bgr(c):
    """The colour network's output [V,3] (float, BGR order: vdn_train/dataset.py trains in cv.imread's order) -> uint8 RGB:
    rint(clip(c, 0, 1) * 255) in the array's own precision, channels reversed. rint rounds to nearest, halves to even
    (0.5 -> 127.5 -> 128)."""
    c = np.asarray(c)
    if c.ndim != 2 or c.shape[1] != 3 or not np.issubdtype(c.dtype, np.floating):
        raise ValueError("colours must be a float [V,3] array, got %s %s" % (c.dtype, c.shape))
    q = np.rint(np.clip(c, 0.0, 1.0) * 255).astype(np.uint8)
    return np.ascontiguousarray(q[:, ::-1])


def shade_points(renderer, points, batch=1 << 20):
    """points [P,3] (object space) -> (sdf [P], gradient [P,3], colour [P,3]) as fp32 device tensors:
        sdf, feat = sdf_network(x);  g = sdf_network.gradient(x)  (raw, as render_core feeds it to the colour head);
        view = -g / max(|g|, 1e-12);  colour = color_network(x, g, view, feat)  (the network's own channel order: BGR).
    At most `batch` points per launch, so the workspace is bounded at any mesh size. bf16 networks with the covered colour head:
    ONE launch per batch (vdn_shade_points_bf16); otherwise - fp32, d_feature = 352, non-'idr' heads, VDN_SHADE_POINTS_FUSED=0 -
    the module calls, which on fp32 are the exact-fp32 reference of the fused launch."""
    if not (torch.is_tensor(points) and points.is_cuda and points.dim() == 2 and points.shape[1] == 3):
        raise ValueError("shade_points needs a [P,3] CUDA tensor")
    if batch < 1:
        raise ValueError("batch must be at least 1")
    sn, cn = renderer.sdf_network, renderer.color_network
    x_all = points.detach().float().contiguous()
    P, dev = x_all.shape[0], x_all.device
    sdf = torch.empty(P, dtype=torch.float32, device=dev)
    grad = torch.empty(P, 3, dtype=torch.float32, device=dev)
    col = torch.empty(P, int(cn.conf.get("d_out", 3)), dtype=torch.float32, device=dev)
    fused = fused_point_shading(renderer)
    with torch.no_grad():
        for s in range(0, P, batch):
            x = x_all[s:s + batch]
            n = x.shape[0]
            if fused:
                a = lib.VdnSdfArgs()
                a.blob = sn._images().blobs["full"].data_ptr()
                a.pts, a.n_per_ray, a.sdf_ld, a.P, a.scale = x.data_ptr(), 1, 1, n, float(sn.scale)
                a.sdf, a.normals = sdf[s:s + n].data_ptr(), grad[s:s + n].data_ptr()
                lib.call("vdn_shade_points_bf16", a, lib.ptr(cn._images().blobs["c2"]), int(cn.squeeze_out), lib.ptr(col[s:s + n]),
                         lib.stream_handle())
                continue
            out = sn(x)
            g = sn.gradient(x)[:, 0]
            feat = out[:, 1:]
            if cn.conf.get("d_feature") == 352:         # render(depth_before_color=True): cat([feature_vector, VDN output]), renderer.py:247-248
                if renderer.depth_network is None:
                    raise ValueError("a d_feature = 352 colour network needs the renderer's depth_network")
                feat = torch.cat([feat, renderer.depth_network(x, g, view_from_gradient(g), feat)], dim=-1)
            sdf[s:s + n], grad[s:s + n] = out[:, 0], g
            col[s:s + n] = cn(x, g, view_from_gradient(g), feat)
    return sdf, grad, col


# ---- simplification: quadric vertex clustering (csrc/mesh_simplify.hip) -----------------------------------------------
SIMPLIFY_EPS = 1e-3          # the regulariser of the placement solve, relative to the quadric's trace: an interface default


def _positive_finite(name, x):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, x))
    if not (x > 0.0 and x < float("inf")):
        raise ValueError("%s must be positive and finite, got %r" % (name, x))
    return x


def _first_of_each(codes, n):
    """codes [n] int64 -> bool [n]: True at the first position of each distinct value"""
    uniq, inv = torch.unique(codes, return_inverse=True)
    first = torch.full((uniq.numel(),), n, dtype=torch.int64, device=codes.device)
    first.scatter_reduce_(0, inv, torch.arange(n, device=codes.device), reduce="amin")
    out = torch.zeros(n, dtype=torch.bool, device=codes.device)
    out[first] = True
    return out


def _segments(ids, n_segments):
    """ids [N] int64 in [0, n_segments] (n_segments = the sentinel of entries in no segment) -> (members [N] int64: a stable sort by
    id, so ascending position inside a segment; start [n_segments + 1] int64)"""
    members = torch.sort(ids, stable=True)[1].contiguous()
    count = torch.bincount(ids, minlength=n_segments + 1)[:n_segments]
    start = torch.zeros(n_segments + 1, dtype=torch.int64, device=ids.device)
    start[1:] = torch.cumsum(count, 0)
    return members, start


def _records_stage(a, st, vertex_cluster, C, F, dev):
    """Corner records of a vertex map (vdn_simplify_records; `a` holds the mesh and its live bytes) and the duplicate rule
    -> (corner [3 F], survive [F] uint8, emit [F] bool)"""
    corner = torch.empty(3 * F, dtype=torch.int64, device=dev)
    canonical = torch.empty(F, 3, dtype=torch.int64, device=dev)
    survive = torch.empty(F, dtype=torch.uint8, device=dev)
    a.vertex_cluster, a.corner_cluster, a.canonical, a.survive, a.C = (vertex_cluster.data_ptr(), corner.data_ptr(), canonical.data_ptr(),
                                                                         survive.data_ptr(), C)
    _call_sized("vdn_simplify_records", a, st)
    # the duplicate rule: among the survivors with one canonical triple the first in input order is emitted
    idx = torch.nonzero(survive).reshape(-1)
    emit = torch.zeros(F, dtype=torch.bool, device=dev)
    if idx.numel() > 0:
        tri = canonical[idx]
        if C <= 1 << 21:
            codes = (tri[:, 0] * C + tri[:, 1]) * C + tri[:, 2]
        else:                                            # (three 31-bit ids do not fit one word: pair the first two, then the third)
            pair = torch.unique(tri[:, 0] * C + tri[:, 1], return_inverse=True)[1]
            codes = pair * C + tri[:, 2]
        emit[idx[_first_of_each(codes, idx.numel())]] = True
    return corner, survive, emit


def _cluster_stage(name, vertices, triangles, cell_size, origin):
    """The part simplify_mesh, cluster_quadrics and count_simplified_faces share: mark, keys, clusters, corner records and the
    duplicate rule -> dict (None-valued arrays for an empty mesh). Two host reads."""
    _check_triangles(name, triangles)
    _check_vertices(name, vertices, triangles)
    h = _positive_finite("cell_size", cell_size)
    if origin is not None:
        try:
            origin = [float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin)]
        except (TypeError, ValueError):
            raise ValueError("origin must be three numbers, got %r" % (origin,))
        if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
            raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    dev = vertices.device
    v, t = vertices.detach().float().contiguous(), triangles.contiguous()
    V, F = v.shape[0], t.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError("%s: the sizes do not fit 32-bit indexing" % name)
    if F > 0 and V == 0:
        raise ValueError("a triangle refers to a vertex outside [0, 0)")
    s = {"v": v, "t": t, "V": V, "F": F, "h": h, "origin": origin, "C": 0, "n_live": 0,
         "vertex_cluster": torch.full((V,), -1, dtype=torch.int64, device=dev)}
    if F == 0:
        return s
    with torch.cuda.device(dev):
        st = lib.stream_handle()
        live = torch.empty(F, dtype=torch.uint8, device=dev)
        used = torch.zeros(V, dtype=torch.uint8, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = lib.VdnSimplifyArgs()
        a.vertices, a.triangles, a.live, a.vertex_used, a.error = v.data_ptr(), t.data_ptr(), live.data_ptr(), used.data_ptr(), err.data_ptr()
        a.V, a.F, a.index_bytes, a.h = V, F, t.element_size(), h
        _call_sized("vdn_simplify_mark", a, st)
        ub = used.bool()
        inf = torch.full((1, 3), float("inf"), device=dev)
        lo = torch.where(ub[:, None], v, inf).amin(dim=0).double()
        hi = torch.where(ub[:, None], v, -inf).amax(dim=0).double()
        stats = torch.cat([lo, hi, torch.stack([err[0].long(), live.sum(), used.sum()]).double()]).tolist()    # host read 1: box, flag, counts
        if stats[6]:
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % V)
        n_live, n_used = int(stats[7]), int(stats[8])
        s["n_live"] = n_live
        if n_live == 0:
            return s
        if origin is None:
            origin = stats[0:3]
        # the grid covers the cells of the referenced finite vertices; floor is monotone, so the box's corners give the range
        i_lo = [math.floor((stats[k] - origin[k]) / h) for k in range(3)]
        i_hi = [math.floor((stats[3 + k] - origin[k]) / h) for k in range(3)]
        dims = [b - c + 1 for b, c in zip(i_hi, i_lo)]
        if max(abs(x) for x in i_lo + i_hi) >= 1 << 52 or dims[0] * dims[1] * dims[2] >= 1 << 62:
            raise ValueError("%s: a cell size of %g gives a grid of %s cells, more than 62 bits hold" % (name, h, "x".join(str(d) for d in dims)))
        key = torch.empty(V, dtype=torch.int64, device=dev)
        a.key, a.origin_x, a.origin_y, a.origin_z = key.data_ptr(), origin[0], origin[1], origin[2]
        a.lo_x, a.lo_y, a.lo_z, a.nx, a.ny, a.nz = i_lo[0], i_lo[1], i_lo[2], dims[0], dims[1], dims[2]
        _call_sized("vdn_simplify_keys", a, st)
        # clusters = the distinct keys of the referenced vertices, ascending; an unreferenced vertex sorts first as -1
        uniq, inv = torch.unique(torch.where(ub, key, torch.full_like(key, -1)), sorted=True, return_inverse=True)
        if n_used < V:
            uniq, inv = uniq[1:], inv - 1
        C = int(uniq.shape[0])
        vertex_cluster = inv.contiguous()
        cell = torch.stack([uniq % dims[0] + i_lo[0], (uniq // dims[0]) % dims[1] + i_lo[1], uniq // (dims[0] * dims[1]) + i_lo[2]], dim=1)
        corner, survive, emit = _records_stage(a, st, vertex_cluster, C, F, dev)
        s.update(origin=origin, C=C, vertex_cluster=vertex_cluster, cell=cell, corner=corner, survive=survive, emit=emit, live=live,
                 grid_lo=i_lo, grid_hi=i_hi, key=uniq.contiguous(), args=a,
                 centre=(torch.tensor(origin, dtype=torch.float64, device=dev)[None] + (cell.double() + 0.5) * h).contiguous())
    return s


def _segment_mean(rows, members, start, C):
    """rows fp32 [N,K] -> fp64 [C,K] by vdn_segment_mean"""
    rows = rows.contiguous()
    out = torch.empty(C, rows.shape[1], dtype=torch.float64, device=rows.device)
    a = lib.VdnSegmentMeanArgs()
    a.rows, a.members, a.start, a.out = rows.data_ptr(), members.data_ptr(), start.data_ptr(), out.data_ptr()
    a.N, a.M, a.C, a.K = rows.shape[0], members.shape[0], C, rows.shape[1]
    _call_sized("vdn_segment_mean", a, lib.stream_handle())
    return out


def _vertex_members(s):
    vc = s["vertex_cluster"]
    return _segments(torch.where(vc < 0, torch.full_like(vc, s["C"]), vc), s["C"])


def _quadric_stage(s):
    """-> (quadric [C,10], mean [C,3] relative to the centre, vertex members, start) of a non-empty cluster stage"""
    v, t, C = s["v"], s["t"], s["C"]
    with torch.cuda.device(v.device):
        vm, vstart = _vertex_members(s)
        mean = _segment_mean(v, vm, vstart, C) - s["centre"]
        rm, rstart = _segments(s["corner"], C)
        quadric = torch.empty(C, 10, dtype=torch.float64, device=v.device)
        a = lib.VdnClusterQuadricArgs()
        a.vertices, a.triangles, a.members, a.start = v.data_ptr(), t.data_ptr(), rm.data_ptr(), rstart.data_ptr()
        a.centre, a.quadric = s["centre"].data_ptr(), quadric.data_ptr()
        a.V, a.F, a.M, a.C, a.index_bytes = s["V"], s["F"], rm.shape[0], C, t.element_size()
        _call_sized("vdn_cluster_quadrics", a, lib.stream_handle())
    return quadric, mean.contiguous(), vm, vstart


def cluster_quadrics(vertices, triangles, cell_size, origin=None):
    """The clusters of vertex clustering on a grid of cubic cells of edge cell_size from `origin` (default: the minimum corner of the
    box of the referenced finite vertices), and Lindstrom's quadric of each (vdn_simplify_*, vdn_segment_mean, vdn_cluster_quadrics:
    include/vdn_render.h) -> dict of device tensors: vertex_cluster [V] int64 (-1 for a vertex in no cluster: not finite, or used
    by no live triangle), cell [C,3] int64 (floor((v - origin) / cell_size) per axis), quadric [C,10] float64 (Axx, Axy, Axz, Ayy,
    Ayz, Azz, bx, by, bz, c of sum (n.x + d)^2 over the cluster's corner records, n the unnormalised normal, coordinates relative to
    the cell centre origin + (cell + 0.5) cell_size), mean [C,3] float64 (the members' mean position, relative to the cell centre)
    and origin (3 floats). A triangle is live when its three corners are finite; clusters are numbered in ascending key order.
    Both sums have a fixed order: two calls give the same bits. ValueError as simplify_mesh."""
    s = _cluster_stage("cluster_quadrics", vertices, triangles, cell_size, origin)
    dev = vertices.device
    if s["C"] == 0:
        return {"vertex_cluster": s["vertex_cluster"], "cell": torch.empty(0, 3, dtype=torch.int64, device=dev),
                "quadric": torch.empty(0, 10, dtype=torch.float64, device=dev), "mean": torch.empty(0, 3, dtype=torch.float64, device=dev),
                "origin": s["origin"]}
    quadric, mean, _, _ = _quadric_stage(s)
    return {"vertex_cluster": s["vertex_cluster"], "cell": s["cell"], "quadric": quadric, "mean": mean, "origin": s["origin"]}


def count_simplified_faces(vertices, triangles, cell_size, origin=None):
    """The number of triangles simplify_mesh(vertices, triangles, cell_size, origin=origin) emits, without the quadrics, the means or
    the output: keys, corner records and the duplicate rule only (what a search for a cell size needs)."""
    s = _cluster_stage("count_simplified_faces", vertices, triangles, cell_size, origin)
    return int(s["emit"].sum()) if s["C"] > 0 else 0


# ---- adaptive simplification: octree vertex clustering under an error bound (csrc/mesh_simplify.hip: vdn_octree_*) ----
OCTREE_LEVELS = 3            # the levels above the finest cells when a tolerance is given without them: an interface default
OCTREE_MAX_LEVELS = 8


def _check_levels(levels):
    try:
        ok = not isinstance(levels, bool) and int(levels) == levels and 1 <= levels <= OCTREE_MAX_LEVELS
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("levels must be an integer in [1, %d], got %r" % (OCTREE_MAX_LEVELS, levels))
    return int(levels)


def _check_tolerance(tolerance):
    try:
        tolerance = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError("tolerance must be a number, got %r" % (tolerance,))
    if not tolerance >= 0.0:
        raise ValueError("tolerance must not be negative, got %r" % (tolerance,))
    return tolerance


def _octree_node(lv, h, eps, prev=None, grid=None):
    """vdn_octree_merge on one level: fills position, status, error, trace of the level dict lv (and quadric, mean, count, children
    from the level below, `prev` on the grid `grid` = (lo, dims), in merge mode)"""
    C, dev = lv["cell"].shape[0], lv["cell"].device
    a = lib.VdnOctreeMergeArgs()
    if prev is not None:
        lv["quadric"], lv["mean"] = torch.empty(C, 10, dtype=torch.float64, device=dev), torch.empty(C, 3, dtype=torch.float64, device=dev)
        lv["count"], lv["children"] = torch.empty(C, dtype=torch.int64, device=dev), torch.empty(C, 8, dtype=torch.int64, device=dev)
        a.cell, a.child_key, a.child_quadric, a.child_mean, a.child_count = (lv["cell"].data_ptr(), prev["key"].data_ptr(),
                                                                             prev["quadric"].data_ptr(), prev["mean"].data_ptr(), prev["count"].data_ptr())
        a.children, a.count, a.Cc = lv["children"].data_ptr(), lv["count"].data_ptr(), prev["cell"].shape[0]
        (a.lo_x, a.lo_y, a.lo_z), (a.nx, a.ny, a.nz) = grid
    lv["position"], lv["status"] = torch.empty(C, 3, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.uint8, device=dev)
    lv["error"], lv["trace"] = torch.empty(C, dtype=torch.float64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)
    a.centre, a.quadric, a.mean = lv["centre"].data_ptr(), lv["quadric"].data_ptr(), lv["mean"].data_ptr()
    a.position, a.status, a.error, a.trace = lv["position"].data_ptr(), lv["status"].data_ptr(), lv["error"].data_ptr(), lv["trace"].data_ptr()
    a.C, a.h, a.eps = C, h, eps
    _call_sized("vdn_octree_merge", a, lib.stream_handle())


def _build_octree(name, vertices, triangles, cell_size, levels, origin, eps):
    levels, eps = _check_levels(levels), _positive_finite("eps", eps)
    s = _cluster_stage(name, vertices, triangles, cell_size, origin)
    dev, h0 = vertices.device, s["h"]
    if not math.isfinite(h0 * 2.0 ** levels):
        raise ValueError("%s: a cell size of %g is too large for %d levels" % (name, h0, levels))
    tree = {"vertex_cluster": s["vertex_cluster"], "origin": s["origin"], "cell_size": h0, "eps": eps, "levels": [], "_stage": s}
    if s["C"] == 0:
        e = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)
        for l in range(levels + 1):
            lv = {"cell": e(0, 3, dtype=torch.int64), "quadric": e(0, 10), "mean": e(0, 3), "count": e(0, dtype=torch.int64), "position": e(0, 3),
                  "status": e(0, dtype=torch.uint8), "error": e(0), "trace": e(0)}
            if l < levels:
                lv["parent"] = e(0, dtype=torch.int64)
            tree["levels"].append(lv)
        return tree
    with torch.cuda.device(dev):
        quadric, mean, vm, vstart = _quadric_stage(s)
        origin_t = torch.tensor(s["origin"], dtype=torch.float64, device=dev)[None]
        lv = {"cell": s["cell"].contiguous(), "key": s["key"], "centre": s["centre"], "quadric": quadric, "mean": mean,
              "count": (vstart[1:] - vstart[:-1]).contiguous()}
        _octree_node(lv, h0, eps)
        tree["levels"].append(lv)
        lo, hi = list(s["grid_lo"]), list(s["grid_hi"])
        for l in range(1, levels + 1):
            prev, grid = lv, (lo, [b - c + 1 for b, c in zip(hi, lo)])
            lo, hi = [x >> 1 for x in lo], [x >> 1 for x in hi]                # (Python's shift is the floor, as the tensors' is)
            dims = [b - c + 1 for b, c in zip(hi, lo)]
            up = prev["cell"] >> 1
            uniq, inv = torch.unique((up[:, 0] - lo[0]) + dims[0] * ((up[:, 1] - lo[1]) + dims[1] * (up[:, 2] - lo[2])), sorted=True,
                                     return_inverse=True)                      # (the host learns C_l here: one read per level)
            prev["parent"] = inv.contiguous()
            cell = torch.stack([uniq % dims[0] + lo[0], (uniq // dims[0]) % dims[1] + lo[1], uniq // (dims[0] * dims[1]) + lo[2]], dim=1).contiguous()
            h = h0 * 2.0 ** l
            lv = {"cell": cell, "key": uniq.contiguous(), "centre": (origin_t + (cell.double() + 0.5) * h).contiguous()}
            _octree_node(lv, h, eps, prev, grid)
            tree["levels"].append(lv)
        sizes = [x["cell"].shape[0] for x in tree["levels"]]
        start = [0]
        for n in sizes:
            start.append(start[-1] + n)
        # the level-major concatenation vdn_octree_assign walks, and what the final nodes are gathered from
        tree["_start"] = start
        tree["_start_t"] = torch.tensor(start, dtype=torch.int64, device=dev)
        tree["_parent"] = torch.cat([x["parent"] + start[l + 1] for l, x in enumerate(tree["levels"][:-1])] +
                                    [torch.full((sizes[-1],), -1, dtype=torch.int64, device=dev)]).contiguous()
        tree["_level_of"] = torch.cat([torch.full((n,), l, dtype=torch.uint8, device=dev) for l, n in enumerate(sizes)])
    return tree


def cluster_octree(vertices, triangles, cell_size, levels, origin=None, eps=SIMPLIFY_EPS):
    """The octree of clusters above cluster_quadrics' cells (vdn_octree_merge, include/vdn_render.h): level l has cubic cells of
    edge cell_size 2^l from `origin`, the cell of a level-0 cell being its index >> l per axis, 1 <= levels <= 8 -> dict:
    vertex_cluster [V] int64 (the level-0 cluster, -1: none), origin, cell_size, eps and `levels`, a list of levels + 1 dicts of
    device tensors: cell [C_l,3] int64 (ascending key order), quadric [C_l,10] and mean [C_l,3] float64 relative to the cell centre
    (level 0: cluster_quadrics'; above: the children's, moved to the parent's centre and added in slot order), count [C_l] int64
    (referenced vertices), position [C_l,3] float64 (absolute: simplify_mesh's placement, with that level's edge), status [C_l]
    uint8, error [C_l] (the quadric at the placed vertex, clamped at 0), trace [C_l], parent [C_l] int64 (the index in the next
    level; absent at the top) and, above level 0, children [C_l,8] int64 (-1: absent). The tree does not depend on a tolerance.
    Host reads: the two of the level-0 stage and one per level above it (C_l). ValueError as simplify_mesh."""
    return _build_octree("cluster_octree", vertices, triangles, cell_size, levels, origin, eps)


def select_octree(tree, tolerance):
    """The node of every level-0 cluster of a cluster_octree tree under a tolerance (vdn_octree_select, vdn_octree_assign): a node
    is ACCEPTED when its trace is positive and finite and error < tolerance^2 trace (error / trace is the area-squared-weighted
    mean squared distance of the placed vertex to the planes of the node's triangles: the tolerance is an rms distance in the
    mesh's units), SOLID when it is accepted and all its children are solid (level 0 is solid); a cluster's node is its highest
    solid ancestor -> (level [C_0] uint8, node [C_0] int64: the index inside that level). No host read."""
    tol = _check_tolerance(tolerance)
    lv = tree["levels"]
    C0, dev = lv[0]["cell"].shape[0], lv[0]["cell"].device
    if C0 == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        start, st = tree["_start"], lib.stream_handle()
        solid = torch.ones(start[-1], dtype=torch.uint8, device=dev)
        for l in range(1, len(lv)):
            a = lib.VdnOctreeSelectArgs()
            a.error, a.trace, a.children = lv[l]["error"].data_ptr(), lv[l]["trace"].data_ptr(), lv[l]["children"].data_ptr()
            a.child_solid, a.solid = solid[start[l - 1]:].data_ptr(), solid[start[l]:].data_ptr()
            a.C, a.Cc, a.tolerance2 = start[l + 1] - start[l], start[l] - start[l - 1], tol * tol
            _call_sized("vdn_octree_select", a, st)
        level, node = torch.empty(C0, dtype=torch.uint8, device=dev), torch.empty(C0, dtype=torch.int64, device=dev)
        a = lib.VdnOctreeAssignArgs()
        a.parent, a.solid, a.level_start, a.level, a.node = (tree["_parent"].data_ptr(), solid.data_ptr(), tree["_start_t"].data_ptr(),
                                                             level.data_ptr(), node.data_ptr())
        a.C0, a.N, a.levels = C0, start[-1], len(lv) - 1
        _call_sized("vdn_octree_assign", a, st)
    return level, node


def _octree_map(tree, tolerance):
    """-> (vertex map [V] int64 onto the nodes in use, numbered level-major; their global numbers [C'] ascending). One host read."""
    level, node = select_octree(tree, tolerance)
    used, inv = torch.unique(tree["_start_t"][level.long()] + node, sorted=True, return_inverse=True)
    vc = tree["vertex_cluster"]
    return torch.where(vc >= 0, inv[vc.clamp_min(0)], torch.full_like(vc, -1)).contiguous(), used


def count_octree_faces(tree, tolerance):
    """The number of triangles simplify_mesh emits for a tolerance, from a built cluster_octree tree: select, assign, corner records
    and the duplicate rule; no quadrics (what a search for a tolerance needs)."""
    s = tree["_stage"]
    if s["C"] == 0:
        return 0
    with torch.cuda.device(s["v"].device):
        vmap, used = _octree_map(tree, tolerance)
        emit = _records_stage(s["args"], lib.stream_handle(), vmap, int(used.shape[0]), s["F"], s["v"].device)[2]
        return int(emit.sum())


def simplify_mesh(vertices, triangles, cell_size, *, origin=None, placement="quadric", eps=SIMPLIFY_EPS, attributes=(), tolerance=None,
                  levels=None, tree=None):
    """Vertex clustering with quadric error placement: vertices [V,3] CUDA float (taken as fp32), triangles [F,3] CUDA int64 or int32
    -> dict(vertices [V',3] (the input's float dtype), triangles [F',3] (the input's integer dtype), attributes, vertex_cluster [V]
    int64 (the NEW vertex of each old one, -1 where it has none), status [V'] uint8, report).

    Every cluster of cluster_quadrics becomes one vertex. placement="mean": the members' mean position (status 0).
    placement="quadric": x = m + delta with (A + eps tr(A) I) delta = -b - A m, m the mean relative to the cell centre - the
    minimiser of the cluster's quadric, its free directions pulled to the mean (status 0); x = m where tr(A) is not positive and
    finite (status 1) or where x is not finite or leaves the cell, |x_k| > cell_size / 2 (status 2).
    A triangle SURVIVES when it is live (three finite corners) and its corners fall into three different clusters. A triangle is
    emitted iff it survives and is the first in input order among the survivors with its canonical triple (the three cluster ids
    rotated so that the smallest comes first). Emitted triangles keep the input's order and their corner order. A triangle and its
    mirror image have different canonical triples: coincident triangles of opposite orientation - a thin sheet collapsed onto
    itself - both stay. Clusters no emitted triangle uses are dropped (filter_mesh). `attributes`: a sequence of [V] or [V,...]
    CUDA tensors, averaged per cluster by the same segmented mean as the positions (fp64 mean of the fp32 values): float attributes
    come back in their dtype, uint8 ones as the float mean rounded to nearest, halves to even.
    report: vertices_in, faces_in, clusters, vertices_out, faces_out, faces_collapsed, faces_duplicate, faces_non_finite,
    cell_size, origin, placement, eps, status (the count of each status value).

    tolerance (keyword, with levels, default OCTREE_LEVELS): the adaptive mode. cell_size is the finest cell; the clusters are the
    nodes select_octree picks in a cluster_octree of `levels` levels, numbered level-major (ascending level, then index): cells
    grow, up to cell_size 2^levels, wherever the placed vertex stays within `tolerance` (rms) of the planes it replaces. tolerance
    = 0 gives the uniform result at cell_size, a tolerance beyond sqrt(3) cell_size 2^levels the uniform result at the coarsest
    size. Everything after the vertex map - records, survive and duplicate rule, attributes - is as above. The result gains level
    [V'] uint8 (the level of each new vertex's node; status and the fallback refer to that node's cell), the report tolerance,
    levels and nodes_per_level (the nodes in use per level; clusters is their sum). `tree`: a cluster_octree tree of the same
    mesh, cell size, origin, levels and eps, to spare building it again. Needs placement="quadric".

    ValueError on CPU tensors, wrong shapes, a corner index outside [0, V), a cell_size or eps that is not positive and finite, a
    negative tolerance, levels outside [1, 8] or without a tolerance, or a grid whose nx ny nz does not fit 62 bits. An empty mesh
    (or one without a live triangle) returns an empty mesh."""
    if placement not in ("quadric", "mean"):
        raise ValueError("placement must be 'quadric' or 'mean', got %r" % (placement,))
    eps = _positive_finite("eps", eps)
    adaptive = tolerance is not None
    if adaptive:
        tolerance, levels = _check_tolerance(tolerance), _check_levels(OCTREE_LEVELS if levels is None else levels)
        if placement != "quadric":
            raise ValueError("a tolerance needs placement='quadric': the error it bounds is the quadric's")
    elif levels is not None or tree is not None:
        raise ValueError("levels and tree belong to the adaptive mode: give a tolerance")
    attributes = list(attributes)
    V = vertices.shape[0] if torch.is_tensor(vertices) and vertices.dim() > 0 else 0
    for x in attributes:
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() >= 1 and x.shape[0] == V and (x.is_floating_point() or x.dtype == torch.uint8)):
            raise ValueError("an attribute must be a float or uint8 CUDA tensor with one row per vertex")
    if adaptive:
        if tree is None:
            tree = _build_octree("simplify_mesh", vertices, triangles, cell_size, levels, origin, eps)
        elif (len(tree["levels"]) != levels + 1 or tree["cell_size"] != float(cell_size) or tree["eps"] != eps or tree["_stage"]["V"] != V or
              tree["_stage"]["F"] != triangles.shape[0] or (origin is not None and tree["origin"] is not None and
                                                            [float(x) for x in origin] != list(tree["origin"]))):
            raise ValueError("the tree was built with other arguments")
        s = tree["_stage"]
    else:
        s = _cluster_stage("simplify_mesh", vertices, triangles, cell_size, origin)
    dev, C, F = vertices.device, s["C"], s["F"]
    report = {"vertices_in": s["V"], "faces_in": F, "clusters": C, "cell_size": s["h"], "origin": s["origin"], "placement": placement,
              "eps": eps, "faces_non_finite": F - s["n_live"]}
    if adaptive:
        report.update(tolerance=tolerance, levels=levels, nodes_per_level=[0] * (levels + 1))
    if C == 0:
        report.update(vertices_out=0, faces_out=0, faces_collapsed=0, faces_duplicate=0, status={"0": 0, "1": 0, "2": 0})
        res = {"vertices": torch.empty(0, 3, dtype=vertices.dtype, device=dev), "triangles": torch.empty(0, 3, dtype=triangles.dtype, device=dev),
               "attributes": [torch.empty((0,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev) for x in attributes],
               "vertex_cluster": s["vertex_cluster"], "status": torch.empty(0, dtype=torch.uint8, device=dev), "report": report}
        if adaptive:
            res["level"] = torch.empty(0, dtype=torch.uint8, device=dev)
        return res
    with torch.cuda.device(dev):
        vertex_cluster, corner, survive, emit, level = s["vertex_cluster"], s["corner"], s["survive"], s["emit"], None
        if adaptive:
            vertex_cluster, used = _octree_map(tree, tolerance)
            C = int(used.shape[0])
            corner, survive, emit = _records_stage(s["args"], lib.stream_handle(), vertex_cluster, C, F, dev)
            vm, vstart = _segments(torch.where(vertex_cluster < 0, torch.full_like(vertex_cluster, C), vertex_cluster), C)
            position = torch.cat([x["position"] for x in tree["levels"]])[used]
            status, level = torch.cat([x["status"] for x in tree["levels"]])[used], tree["_level_of"][used]
        elif placement == "mean":
            status = torch.zeros(C, dtype=torch.uint8, device=dev)
            vm, vstart = _vertex_members(s)
            position = _segment_mean(s["v"], vm, vstart, C)          # (= centre + the mean relative to it, without the round trip)
        else:
            status = torch.zeros(C, dtype=torch.uint8, device=dev)
            quadric, mean, vm, vstart = _quadric_stage(s)
            position = torch.empty(C, 3, dtype=torch.float64, device=dev)
            a = lib.VdnClusterQuadricArgs()
            a.centre, a.quadric, a.mean, a.position, a.status = (s["centre"].data_ptr(), quadric.data_ptr(), mean.data_ptr(), position.data_ptr(),
                                                                 status.data_ptr())
            a.V, a.F, a.C, a.h, a.eps = s["V"], F, C, s["h"], eps
            _call_sized("vdn_cluster_place", a, lib.stream_handle())
        # (the records of a triangle that is not emitted may hold the sentinel C: not an index filter_mesh accepts)
        corner = torch.where(emit[:, None], corner.reshape(F, 3), torch.zeros((), dtype=torch.int64, device=dev)).to(triangles.dtype)
        new_v, new_t, kept = filter_mesh(position, corner, keep_faces=emit)
        out_attrs = []
        for x in attributes:
            m = _segment_mean(x.reshape(V, -1).float(), vm, vstart, C)[kept].reshape((kept.shape[0],) + tuple(x.shape[1:]))
            out_attrs.append(torch.round(m).clamp_(0, 255).to(torch.uint8) if x.dtype == torch.uint8 else m.to(x.dtype))
        new_of_cluster = torch.full((C + 1,), -1, dtype=torch.int64, device=dev)
        new_of_cluster[kept] = torch.arange(kept.shape[0], device=dev)
        status = status[kept]
        n_surv, n_stat = int(survive.sum()), torch.bincount(status.long(), minlength=3).tolist()       # host read 3
        if adaptive:
            report.update(clusters=C, nodes_per_level=torch.bincount(level.long(), minlength=levels + 1).tolist())
    report.update(vertices_out=int(new_v.shape[0]), faces_out=int(new_t.shape[0]), faces_collapsed=s["n_live"] - n_surv,
                  faces_duplicate=n_surv - int(new_t.shape[0]), status={str(k): int(n) for k, n in enumerate(n_stat)})
    res = {"vertices": new_v.to(vertices.dtype), "triangles": new_t, "attributes": out_attrs,
           "vertex_cluster": new_of_cluster[vertex_cluster], "status": status, "report": report}
    if adaptive:
        res["level"] = level[kept]
    return res


# ---- textured meshes: a per-face atlas (csrc/mesh_texture.hip) ----------------------------------------------------------
TEXTURE_MIN_PATCH = 4        # m = n - 3 >= 1: a patch needs its three corner texels apart, a gutter and the diagonal
TEXTURE_PROJECT_ROUNDS = 2   # Newton steps of the texel points towards the level set: an interface default, not a measurement


def texture_layout(F, texture_size, patch=None):
    """The atlas layout of F faces on a texture_size^2 atlas (include/vdn_render.h has the rules) -> dict(F, S, n, C, T, m, points):
    n the cell edge in texels, C = S // n cells per row, T = n (n - 1) / 2 texels per face, m = n - 3, points = F T. patch=None picks
    the largest n with ceil(F / 2) <= (S // n)^2. ValueError when even n = 4 does not fit, or a given patch does not. Host integers."""
    try:
        F_, S = int(F), int(texture_size)
    except (TypeError, ValueError):
        raise ValueError("F and texture_size must be integers, got %r and %r" % (F, texture_size))
    if F_ != F or F_ < 0 or S != texture_size or S < TEXTURE_MIN_PATCH:
        raise ValueError("texture_layout needs F >= 0 and texture_size >= %d as integers, got %r and %r" % (TEXTURE_MIN_PATCH, F, texture_size))
    if S * S >= 1 << 31:
        raise ValueError("texture_size %d: the atlas does not fit 32-bit indexing" % S)
    cells = (F_ + 1) // 2
    if patch is None:
        k = max(1, math.isqrt(cells))                                              # ceil(sqrt(cells)), at least one cell per row
        if k * k < cells:
            k += 1
        n = S // k                                                                 # the largest n with S // n >= k
        if n < TEXTURE_MIN_PATCH:
            raise ValueError("%d faces need %d x %d cells: a %d^2 atlas leaves them fewer than %d texels per edge" % (F_, k, k, S, TEXTURE_MIN_PATCH))
    else:
        try:
            n = int(patch)
        except (TypeError, ValueError):
            raise ValueError("patch must be an integer, got %r" % (patch,))
        if n != patch or n < TEXTURE_MIN_PATCH or n > S:
            raise ValueError("patch must be an integer in [%d, texture_size], got %r" % (TEXTURE_MIN_PATCH, patch))
        if cells > (S // n) ** 2:
            raise ValueError("%d faces do not fit a %d^2 atlas in cells of %d texels (%d cells)" % (F_, S, n, (S // n) ** 2))
    T = n * (n - 1) // 2
    if F_ * T >= 1 << 31:
        raise ValueError("%d faces of %d texels do not fit 32-bit indexing" % (F_, T))
    return {"F": F_, "S": S, "n": n, "C": S // n, "T": T, "m": n - 3, "points": F_ * T}


def texture_uv(layout):
    """OBJ texture coordinates of every face corner -> float64 [F,3,2] numpy: vt = (x / S, 1 - y / S) of the corner's continuous
    atlas position (x, y) (row 0 of the atlas is its top, v = 0 of an OBJ its bottom)."""
    F, S, n, C, m = (layout[k] for k in ("F", "S", "n", "C", "m"))
    f = np.arange(F, dtype=np.int64)
    c, h = f >> 1, f & 1
    ox, oy = ((c % C) * n).astype(np.float64), ((c // C) * n).astype(np.float64)
    lower = np.array([[0.5, 0.5], [m + 0.5, 0.5], [0.5, m + 0.5]])
    upper = np.array([[n - 0.5, n - 0.5], [n - 0.5 - m, n - 0.5], [n - 0.5, n - 0.5 - m]])
    local = np.where((h == 0)[:, None, None], lower[None], upper[None])
    x, y = ox[:, None] + local[:, :, 0], oy[:, None] + local[:, :, 1]
    return np.stack([x / S, 1.0 - y / S], axis=-1)


def _texture_mesh(name, vertices, triangles):
    """-> (vertices float64 [V,3], triangles int32 / int64 [F,3]) contiguous on the device"""
    _check_triangles(name, triangles)
    _check_vertices(name, vertices, triangles)
    if vertices.shape[0] >= 1 << 31 or triangles.shape[0] >= 1 << 31:
        raise ValueError("%s: the sizes do not fit 32-bit indexing" % name)
    if triangles.shape[0] > 0 and vertices.shape[0] == 0:
        raise ValueError("a triangle refers to a vertex outside [0, 0)")
    return vertices.detach().double().contiguous(), triangles.contiguous()


def _check_layout(layout, F):
    if not (isinstance(layout, dict) and all(k in layout for k in ("F", "S", "n", "C", "T", "m", "points"))):
        raise ValueError("layout must be a record of texture_layout")
    if layout["F"] != F:
        raise ValueError("the layout is one of %d faces, the mesh has %d" % (layout["F"], F))
    if layout != texture_layout(F, layout["S"], layout["n"]):
        raise ValueError("the layout record is not one texture_layout gives")


def _tex_args(layout, v=None, t=None):
    a = lib.VdnTexArgs()
    a.S, a.n, a.F = layout["S"], layout["n"], layout["F"]
    if v is not None:
        a.vertices, a.triangles, a.V, a.index_bytes = v.data_ptr(), t.data_ptr(), v.shape[0], t.element_size()
    return a


def texel_points(vertices, triangles, layout):
    """The surface point every owned texel of the atlas shows (vdn_tex_points) -> (points [F T,3] fp32, face [F T] int32), face-major:
    row f T + r is texel r of face f. vertices [V,3] CUDA float (taken as float64), triangles [F,3] CUDA int64 or int32. The points
    are (b0 v0 + b1 v1) + b2 v2 in double, rounded once. ValueError on CPU tensors, wrong shapes or a corner index outside [0, V)."""
    v, t = _texture_mesh("texel_points", vertices, triangles)
    _check_layout(layout, t.shape[0])
    dev, P = v.device, layout["points"]
    points = torch.empty(P, 3, dtype=torch.float32, device=dev)
    face = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return points, face
    with torch.cuda.device(dev):
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = _tex_args(layout, v, t)
        a.points, a.face, a.error = points.data_ptr(), face.data_ptr(), err.data_ptr()
        _call_sized("vdn_tex_points", a, lib.stream_handle())
        if int(err.item()):                                   # one host read: the error flag
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % v.shape[0])
    return points, face


def _rows(name, x, n=None, cols=3):
    """x as a contiguous fp32 tensor: [P,cols], or [P] with cols = 0; n: the row count it must have"""
    ok = torch.is_tensor(x) and x.is_cuda and x.is_floating_point() and ((x.dim() == 2 and x.shape[1] == cols) if cols else x.dim() == 1)
    if not (ok and (n is None or x.shape[0] == n)):
        raise ValueError("%s must be a float CUDA tensor %s%s" % (name, "[P,%d]" % cols if cols else "[P]", "" if n is None else " with P = %d" % n))
    return x.detach().float().contiguous()


def project_step(x, x0, sdf, gradient, max_offset):
    """One Newton step of the points x towards the zero level of a field with the values `sdf` [P] and gradients `gradient` [P,3] at
    x, kept within max_offset of x0 (vdn_tex_project; all four fp32 CUDA tensors) -> x' [P,3] fp32:
    x' = x - sdf g / max(|g|^2, 1e-12), pulled back onto the ball |x' - x0| <= max_offset; a row whose sdf, g or result is not finite
    stays where it was."""
    if not (torch.is_tensor(x) and torch.is_tensor(x0) and torch.is_tensor(sdf) and torch.is_tensor(gradient)):
        raise ValueError("project_step needs CUDA tensors")
    x = _rows("x", x)
    P = x.shape[0]
    x0, g, s = _rows("x0", x0, P), _rows("gradient", gradient, P), _rows("sdf", sdf.reshape(-1) if sdf.dim() == 2 and sdf.shape[1] == 1 else sdf, P, cols=0)
    if not (x0.device == g.device == s.device == x.device):
        raise ValueError("x, x0, sdf and gradient must be on one device")
    try:
        r = float(max_offset)
    except (TypeError, ValueError):
        raise ValueError("max_offset must be a number, got %r" % (max_offset,))
    if not (r >= 0.0 and r < float("inf")):
        raise ValueError("max_offset must be finite and not negative, got %r" % (max_offset,))
    out = torch.empty_like(x)
    if P > 0:
        a = lib.VdnTexProjectArgs()
        a.x, a.x0, a.sdf, a.g, a.out, a.N, a.max_offset = x.data_ptr(), x0.data_ptr(), s.data_ptr(), g.data_ptr(), out.data_ptr(), P, r
        with torch.cuda.device(x.device):
            _call_sized("vdn_tex_project", a, lib.stream_handle())
    return out


def project_points(renderer, points, rounds=TEXTURE_PROJECT_ROUNDS, max_offset=0.0, batch=1 << 20):
    """`rounds` Newton steps of points [P,3] (CUDA, object space) towards the SDF network's zero level set, each row kept within
    max_offset of where it started -> [P,3] fp32. Between the steps the value and the raw gradient come from shade_points (the
    existing launch; its colour is not used), at most `batch` points at a time; then project_step. rounds = 0 returns the points."""
    if int(rounds) != rounds or rounds < 0:
        raise ValueError("rounds must be a non-negative integer, got %r" % (rounds,))
    x0 = _rows("points", points)
    x = x0
    for _ in range(int(rounds)):
        if renderer is None:
            raise ValueError("projection needs the renderer: its SDF network is the level set")
        sdf, g, _c = shade_points(renderer, x, batch=batch)
        x = project_step(x, x0, sdf, g, max_offset)
    return x


def gather_atlas(colors, layout):
    """The atlas of a layout from the colours of its texel points (vdn_tex_gather): colors [F T,3] float CUDA tensor in the
    networks' BGR order -> uint8 [S,S,3] RGB, row 0 at the top; each byte is quantize_colors_bgr's rint(clip(c, 0, 1) * 255) in
    fp32. The diagonal of every cell repeats its neighbour in the lower half; whatever no face owns is 0."""
    if not (isinstance(layout, dict) and "points" in layout):
        raise ValueError("layout must be a record of texture_layout")
    _check_layout(layout, layout["F"])
    if not torch.is_tensor(colors):
        raise ValueError("gather_atlas needs colours as a float [F T,3] CUDA tensor")
    c = _rows("colors", colors, layout["points"])
    S = layout["S"]
    atlas = torch.empty(S, S, 3, dtype=torch.uint8, device=c.device)
    a = _tex_args(layout)
    a.colors, a.n_colors, a.atlas = (c.data_ptr() if c.shape[0] > 0 else None), c.shape[0], atlas.data_ptr()
    with torch.cuda.device(c.device):
        _call_sized("vdn_tex_gather", a, lib.stream_handle())
    return atlas


def sample_texture(texture, layout, vertices, triangles, face, points, background=(1.0, 1.0, 1.0)):
    """Bilinear lookups of an atlas at points of the mesh (vdn_tex_sample): texture uint8 [S,S,3] CUDA, layout its record, face [R]
    integers (-1 = miss) and points [R,3] (taken as float64) -> fp32 [R,3] RGB in [0, 1]. A point is projected onto its face's plane
    and clamped into the triangle; a miss gives `background`. vertices are taken as float64."""
    v, t = _texture_mesh("sample_texture", vertices, triangles)
    _check_layout(layout, t.shape[0])
    dev, S = v.device, layout["S"]
    if not (torch.is_tensor(texture) and texture.device == dev and texture.dtype == torch.uint8 and tuple(texture.shape) == (S, S, 3)):
        raise ValueError("texture must be a uint8 [%d,%d,3] tensor on the mesh's device" % (S, S))
    face, points = torch.as_tensor(face), torch.as_tensor(points)
    if face.dim() != 1 or face.is_floating_point() or face.dtype == torch.bool:
        raise ValueError("face must be an integer [R] array")
    R = face.shape[0]
    if points.dim() != 2 or tuple(points.shape) != (R, 3) or not points.is_floating_point():
        raise ValueError("points must be a float [%d,3] array, got %s" % (R, tuple(points.shape)))
    try:
        bg = [float(x) for x in background]
        assert len(bg) == 3
    except (TypeError, ValueError, AssertionError):
        raise ValueError("background must be three numbers, got %r" % (background,))
    face = face.detach().to(device=dev, dtype=torch.int64).contiguous()
    points = points.detach().to(device=dev, dtype=torch.float64).contiguous()
    rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    if R == 0:
        return rgb
    if t.shape[0] == 0:                                       # no face to hit: every query is a miss
        rgb[:] = torch.tensor(bg, dtype=torch.float64, device=dev).float()
        return rgb
    with torch.cuda.device(dev):
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = _tex_args(layout, v, t)
        a.atlas, a.hit_face, a.hit_points, a.rgb, a.R, a.error = texture.contiguous().data_ptr(), face.data_ptr(), points.data_ptr(), rgb.data_ptr(), R, err.data_ptr()
        a.bg_r, a.bg_g, a.bg_b = bg
        _call_sized("vdn_tex_sample", a, lib.stream_handle())
        if int(err.item()):
            raise ValueError("a triangle refers to a vertex outside [0, %d)" % v.shape[0])
    return rgb


def mean_edge_length(vertices, triangles):
    """The mean length of the 3 F triangle sides, in double (one host read); 0.0 for an empty mesh."""
    if triangles.shape[0] == 0:
        return 0.0
    p = vertices.double()[triangles.long()]
    return float((p - p.roll(-1, dims=1)).norm(dim=2).mean())


# ---- texel colours from the photographs (csrc/mesh_photo.hip) ---------------------------------------------------------
# interface defaults, not measurements: the steepest viewing angle that still counts (cos 78 degrees), the width in pixels of the
# band along an image's border over which its weight falls to zero, and visibility_votes' eps
PHOTO_COS_MIN = 0.2
PHOTO_FEATHER = 16.0
PHOTO_EPS = 1e-4
PHOTO_BLENDS = {"mean": 0, "best": 1}
PHOTO_KEYS = ("P", "images", "cos_min", "feather", "eps", "blend", "fill")


def _photo_scalars(cos_min, feather, eps, blend):
    try:
        c, fe, e = float(cos_min), float(feather), float(eps)
    except (TypeError, ValueError):
        raise ValueError("cos_min, feather and eps must be numbers, got %r, %r and %r" % (cos_min, feather, eps))
    if not (0.0 <= c < 1.0):
        raise ValueError("cos_min must be in [0, 1), got %r" % (cos_min,))
    if not (fe >= 0.0 and fe < float("inf")):
        raise ValueError("feather must be finite and not negative, got %r" % (feather,))
    if not (0.0 <= e < 1.0):
        raise ValueError("eps must be in [0, 1), got %r" % (eps,))
    if blend not in PHOTO_BLENDS:
        raise ValueError("blend must be one of %s, got %r" % (sorted(PHOTO_BLENDS), blend))
    return c, fe, e, PHOTO_BLENDS[blend]


def photo_colors(grid, points, face, P, images, normals=None, anchors=None, cos_min=PHOTO_COS_MIN, feather=PHOTO_FEATHER, eps=PHOTO_EPS,
                 blend="mean"):
    """The colour every texel point takes from the photographs that see it (vdn_tex_photo, include/vdn_render.h has the rules) ->
    {"colors" fp32 [P,3], "weight" fp32 [P], "n_views" int32 [P], "best_view" int32 [P]} on the grid's device. grid: the MeshGrid of the
    mesh; points [P,3] float CUDA: where the colour is looked up; face [P] int32 CUDA: the face of each point; P [N,3,4] (taken as
    float64, as visibility_votes takes it); images [N,H,W,3] float32 contiguous on the grid's device, in [0, 1], in whatever channel
    order the caller holds - the colours come back in it. Camera k colours a point iff the point is in front of it, inside its frame,
    faces it (cos > cos_min against `normals` [P,3], one-sided - or against the face's own normal, two-sided, when None) and no face
    but its own lies on the segment from the camera's centre to anchors[p] (default: the point), 0 < t < 1 - eps. The weight is
    cos^2, scaled down linearly over the `feather` pixels next to the image's border. blend "mean": the weighted mean, weight = the
    sum; "best": the camera with the largest weight (the lower index on a tie). A point no camera passes has colour 0, weight 0,
    n_views 0, best_view -1. ValueError on CPU tensors, wrong shapes or dtypes, a singular camera, scalars out of range or a face
    outside [0, F) (found on the device; one host read). Pass the points face-major, as texel_points gives them."""
    if not isinstance(grid, MeshGrid):
        raise ValueError("grid must be a MeshGrid of the mesh")
    dev = grid.device
    if not torch.is_tensor(points) or not torch.is_tensor(face):
        raise ValueError("photo_colors needs points and face as CUDA tensors")
    x = _rows("points", points)
    n = x.shape[0]
    if not (face.is_cuda and face.dtype == torch.int32 and tuple(face.shape) == (n,)):
        raise ValueError("face must be an int32 [%d] CUDA tensor" % n)
    nrm = anc = None
    if normals is not None:
        if not torch.is_tensor(normals):
            raise ValueError("normals must be a float CUDA tensor [P,3]")
        nrm = _rows("normals", normals, n)
    if anchors is not None:
        if not torch.is_tensor(anchors):
            raise ValueError("anchors must be a float CUDA tensor [P,3]")
        anc = _rows("anchors", anchors, n)
    if any(q is not None and q.device != dev for q in (x, face, nrm, anc)):
        raise ValueError("points, face, normals and anchors must be on the grid's device")
    if not (torch.is_tensor(images) and images.device == dev and images.dtype == torch.float32 and images.dim() == 4 and images.shape[3] == 3
            and images.is_contiguous()):
        raise ValueError("images must be a contiguous float32 [N,H,W,3] tensor on the grid's device")
    c_min, fe, e, mode = _photo_scalars(cos_min, feather, eps, blend)
    centres = camera_centres(P)
    N, H, W = images.shape[0], images.shape[1], images.shape[2]
    if centres.shape[0] != N:
        raise ValueError("%d cameras for %d images" % (centres.shape[0], N))
    out = {"colors": torch.zeros(n, 3, dtype=torch.float32, device=dev), "weight": torch.zeros(n, dtype=torch.float32, device=dev),
           "n_views": torch.zeros(n, dtype=torch.int32, device=dev), "best_view": torch.full((n,), -1, dtype=torch.int32, device=dev)}
    if n == 0 or N == 0 or grid.F == 0:
        return out
    if H < 1 or W < 1:
        raise ValueError("images must have at least one pixel, got %d x %d" % (H, W))
    Pd = torch.as_tensor(P).detach().to(device=dev, dtype=torch.float64).contiguous()
    cd = torch.from_numpy(centres).to(dev)
    fc = face.contiguous()
    with torch.cuda.device(dev):
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        a = grid._geometry(lib.VdnTexPhotoArgs())
        a.points, a.anchors, a.face, a.normals = x.data_ptr(), (None if anc is None else anc.data_ptr()), fc.data_ptr(), (None if nrm is None else nrm.data_ptr())
        a.P_mat, a.centres, a.images = Pd.data_ptr(), cd.data_ptr(), images.data_ptr()
        a.colors, a.weight, a.n_views, a.best_view = (out[k].data_ptr() for k in ("colors", "weight", "n_views", "best_view"))
        a.error = err.data_ptr()
        a.P, a.N, a.H, a.W, a.cos_min, a.feather, a.eps, a.blend = n, N, H, W, c_min, fe, e, mode
        _call_sized("vdn_tex_photo", a, lib.stream_handle())
        if int(err.item()):                                   # one host read: the error flag
            raise ValueError("a face index is outside [0, %d)" % grid.F)
    return out


def _check_photos(photos):
    if not (isinstance(photos, dict) and "P" in photos and "images" in photos):
        raise ValueError('photos must be a dict with "P" [N,3,4] and "images" [N,H,W,3]')
    unknown = sorted(set(photos) - set(PHOTO_KEYS))
    if unknown:
        raise ValueError("photos has the unknown keys %s (known: %s)" % (unknown, ", ".join(PHOTO_KEYS)))
    _photo_scalars(photos.get("cos_min", PHOTO_COS_MIN), photos.get("feather", PHOTO_FEATHER), photos.get("eps", PHOTO_EPS), photos.get("blend", "mean"))
    try:
        fill = [float(x) for x in photos.get("fill", (0.5, 0.5, 0.5))]
        assert len(fill) == 3
    except (TypeError, ValueError, AssertionError):
        raise ValueError("photos['fill'] must be three numbers, got %r" % (photos.get("fill"),))


def _bake_photos(renderer, v, t, layout, anchors, face, photos, project, max_offset, batch):
    """bake_texture's photo path: the texel points on their triangles are the anchors; the projected points look the colours up; the
    SDF gradient of the last shade_points call is the normal (none without a renderer: the faces' own, two-sided); texels no camera
    sees take the network's colour, or photos["fill"] without a renderer."""
    dev = v.device
    images = photos["images"]
    images = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
    if images.dtype != torch.float32:
        raise ValueError("photos['images'] must be float32 [N,H,W,3] in [0, 1], got %s" % images.dtype)
    images = images.to(dev).contiguous()
    points, normals, net = anchors, None, None
    if renderer is not None:
        for _ in range(project):
            sdf, normals, _c = shade_points(renderer, points, batch=batch)
            points = project_step(points, anchors, sdf, normals, max_offset)
        if project == 0:
            _s, normals, net = shade_points(renderer, points, batch=batch)      # (the one extra call: its colours are the network bake)
    grid = MeshGrid(v, t)
    kw = {k: photos[k] for k in ("cos_min", "feather", "eps", "blend") if k in photos}
    got = photo_colors(grid, points, face, photos["P"], images, normals=normals, anchors=anchors, **kw)
    colors, unseen = got["colors"], got["n_views"] == 0
    if renderer is None:
        fill = torch.tensor([float(x) for x in photos.get("fill", (0.5, 0.5, 0.5))], dtype=torch.float64, device=dev).float()
        colors = torch.where(unseen[:, None], fill[None], colors)
    else:
        rows = torch.nonzero(unseen)[:, 0]
        if net is None:
            net = shade_points(renderer, points[rows], batch=batch)[2]           # only the rows no camera sees
        else:
            net = net[rows]
        if net.shape[1] != 3:
            raise ValueError("a texture needs a colour network with three outputs, got %d" % net.shape[1])
        colors[rows] = net
    coverage = (colors.shape[0] - int(unseen.sum())) / colors.shape[0]          # one host read
    return {"texture": gather_atlas(colors, layout), "uv": texture_uv(layout), "layout": layout, "points": points,
            "coverage": coverage, "n_views": got["n_views"]}


def bake_texture(renderer, vertices, triangles, texture_size=2048, patch=None, project=TEXTURE_PROJECT_ROUNDS, max_offset=None,
                 shade=None, batch=1 << 20, photos=None):
    """Bake the appearance of a mesh into a per-face atlas -> {"texture": uint8 [S,S,3] RGB, "uv": float64 [F,3,2] (numpy: OBJ vt per
    face corner), "layout": texture_layout's record, "points": fp32 [F T,3] the shaded points}; texture and points are device tensors.
    vertices [V,3] float, triangles [F,3] integers, object space, numpy arrays or tensors (moved to the renderer's device, or cuda).
    The texel points of the layout (texel_points) take `project` Newton steps towards the SDF network's level set, each within
    max_offset (default: the mesh's mean edge length) of its place on the triangle (project_points; 0 switches it off), are shaded -
    shade_points(renderer, points, batch): view = -normal, exactly as the vertices of a PLY are shaded - and gathered (gather_atlas).
    `shade`: a callable (points [P,3] cuda fp32, face [P] int32) -> colour [P,3] float BGR that stands in for the colour network,
    called with at most `batch` points; renderer may then be None when project is 0. patch / texture_size: texture_layout's; every
    face gets the same patch, which suits meshes whose faces are of one size. An empty mesh gives an all-zero atlas. Filtering is
    safe at the base level only: mip levels mix neighbouring patches.
    `photos`: {"P": [N,3,4] object-space projection matrices, "images": float32 [N,H,W,3] in [0, 1], BGR as the scene loader holds
    them} plus, optionally, photo_colors' cos_min, feather, eps and blend, and "fill": the texels take their colour from the
    photographs (photo_colors; layout, texel points and projection are the same). The points on the triangles are the occlusion
    anchors, the projected points look the colours up; with a renderer the SDF gradient of the last shade_points call is the normal
    (the last projection round's, or one extra call when project is 0) and a texel no camera sees takes the network's colour; without
    one (project 0 only) the faces' own normals count, two-sided, and such a texel takes `fill` (default mid grey). The result gains
    "coverage", the fraction of texels some camera sees, and "n_views" int32 [F T]. photos and shade together are a ValueError."""
    if int(project) != project or project < 0:
        raise ValueError("project must be a non-negative integer, got %r" % (project,))
    if int(batch) != batch or batch < 1:
        raise ValueError("batch must be at least 1")
    if shade is not None and not callable(shade):
        raise ValueError("shade must be callable")
    if shade is not None and photos is not None:
        raise ValueError("shade and photos both say where the colours come from: give one")
    if photos is not None:
        _check_photos(photos)
    if renderer is None and ((shade is None and photos is None) or project > 0):
        raise ValueError("bake_texture needs the renderer unless `shade` or `photos` is given and project is 0")
    if renderer is not None:
        dev = lib.first_param(renderer.sdf_network).device
    else:
        dev = next((x.device for x in (vertices, triangles) if torch.is_tensor(x) and x.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    to_dev = lambda x: x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    v, t = to_dev(vertices), to_dev(triangles)
    if v.dim() != 2 or v.shape[1] != 3 or t.dim() != 2 or t.shape[1] != 3 or not v.is_floating_point() or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("bake_texture needs float vertices [V,3] and integer triangles [F,3]")
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    F = t.shape[0]
    layout = texture_layout(F, texture_size, patch)
    if max_offset is not None and not (float(max_offset) >= 0.0 and float(max_offset) < float("inf")):
        raise ValueError("max_offset must be finite and not negative, got %r" % (max_offset,))
    with torch.cuda.device(dev), torch.no_grad():
        if F == 0:
            res = {"texture": torch.zeros(layout["S"], layout["S"], 3, dtype=torch.uint8, device=dev), "uv": texture_uv(layout),
                   "layout": layout, "points": torch.empty(0, 3, dtype=torch.float32, device=dev)}
            if photos is not None:
                res["coverage"], res["n_views"] = 0.0, torch.zeros(0, dtype=torch.int32, device=dev)
            return res
        points, face = texel_points(v, t, layout)
        if photos is not None:
            r = mean_edge_length(v, t) if max_offset is None and project > 0 else float(max_offset or 0.0)
            return _bake_photos(renderer, v, t, layout, points, face, photos, int(project), r, batch)
        if project > 0:
            r = mean_edge_length(v, t) if max_offset is None else float(max_offset)
            points = project_points(renderer, points, rounds=project, max_offset=r, batch=batch)
        if shade is None:
            colors = shade_points(renderer, points, batch=batch)[2]
            if colors.shape[1] != 3:
                raise ValueError("a texture needs a colour network with three outputs, got %d" % colors.shape[1])
        else:
            colors = torch.empty(points.shape[0], 3, dtype=torch.float32, device=dev)
            for s in range(0, points.shape[0], batch):
                c = shade(points[s:s + batch], face[s:s + batch])
                if not (torch.is_tensor(c) and tuple(c.shape) == (min(batch, points.shape[0] - s), 3)):
                    raise ValueError("shade must return one BGR colour per point")
                colors[s:s + batch] = c
        texture = gather_atlas(colors, layout)
    return {"texture": texture, "uv": texture_uv(layout), "layout": layout, "points": points}


def render_textured_view(grid, texture, origins, directions, background=(1.0, 1.0, 1.0)):
    """What a textured mesh looks like along rays: MeshGrid.cast (the closest hit) followed by sample_texture at o + t d -> fp32 [R,3]
    RGB in [0, 1], `background` where a ray misses. grid: the MeshGrid of the baked mesh; texture: bake_texture's result (its
    "texture" and "layout"). The preview of a bake, and its end-to-end check."""
    if not isinstance(grid, MeshGrid):
        raise ValueError("grid must be a MeshGrid of the baked mesh")
    if not (isinstance(texture, dict) and "texture" in texture and "layout" in texture):
        raise ValueError("texture must be the result of bake_texture")
    o, d = grid._rays(origins, "origins"), grid._rays(directions, "directions")
    t, face = grid.cast(o, d)
    hit = face >= 0
    x = o + torch.where(hit, t, torch.zeros_like(t))[:, None] * d
    return sample_texture(texture["texture"], texture["layout"], grid.vertices, grid.triangles, face, x, background=background)
