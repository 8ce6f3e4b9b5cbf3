"""Iso-surface of a device lattice (reference renderer.py:36 calls mcubes.marching_cubes there), two forms:
  marching_cubes  - vdn_mesh_mc_count / vdn_mesh_mc_emit: the classic 256-case marching cubes with PyMCubes' own vertex and
                    triangle numbering (include/vdn_render.h; the default of extract_geometry since round 6);
  marching_tets   - vdn_mesh_count / vdn_mesh_emit: marching tetrahedra on the Kuhn decomposition (rounds 3-5), kept as an option.
The prefix sums (and the tetrahedra form's vertex welding) are torch ops on the device; nothing runs on the host.

shade_points evaluates the networks at free-standing surface points - the vertex attributes of a mesh that goes to disk
(NeuSRenderer.extract_colored_geometry, vdn_train.validate.validate_mesh).

Mesh cleaning (csrc/mesh_clean.hip; the policy on top is vdn_train/mesh_clean.py): connected_components / component_table label
the pieces of a mesh, dilate_masks / mask_votes count in how many object masks a vertex falls, filter_mesh drops faces and
vertices and renumbers the rest."""
import os

import numpy as np
import torch

from . import lib


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


def fused_point_shading(renderer):
    """True where vdn_shade_points_bf16 (csrc/k_sdf_fwd2.h MODE 4) covers the configuration: both networks on the bf16 kernels and
    the colour head the "c2" stream exists for ('idr', d_feature 256, d_out 3). VDN_SHADE_POINTS_FUSED=0 forces the separate launches."""
    sn, cn = renderer.sdf_network, renderer.color_network
    return (os.environ.get("VDN_SHADE_POINTS_FUSED", "1") != "0" and sn.precision == "bf16" and cn.precision == "bf16"
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
