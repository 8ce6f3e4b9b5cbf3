"""Iso-surface of a device lattice (reference renderer.py:36 calls mcubes.marching_cubes there), two forms:
  marching_cubes  - vdn_mesh_mc_count / vdn_mesh_mc_emit: the classic 256-case marching cubes with PyMCubes' own vertex and
                    triangle numbering (include/vdn_render.h; the default of extract_geometry since round 6);
  marching_tets   - vdn_mesh_count / vdn_mesh_emit: marching tetrahedra on the Kuhn decomposition (rounds 3-5), kept as an option.
The prefix sums (and the tetrahedra form's vertex welding) are torch ops on the device; nothing runs on the host.

shade_points evaluates the networks at free-standing surface points - the vertex attributes of a mesh that goes to disk
(NeuSRenderer.extract_colored_geometry, vdn_train.validate.validate_mesh)."""
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
