"""Mesh cleaning: what the NeuS family does to an extracted surface before it is compared with a scan - drop the vertices that
project outside the (dilated) object masks, then keep the largest connected piece (their `clean_mesh` scripts do it with trimesh
and cv.dilate on the host; here the labelling, the dilation, the votes and the compaction are kernels: vdn_hip/mesh.py,
csrc/mesh_clean.hip; INTEGRATION.md "Mesh cleaning").

A third, optional stage drops what no camera sees: an SDF network closes its surface where nothing looked (the underside of an
object on a table, the inside of a cavity), that geometry is attached to the real surface and projects inside the masks, and a scan
cannot contain it. The occlusion queries are rays against the mesh itself (vdn_hip.mesh.visibility_votes, csrc/mesh_ray.hip).

select_components is the policy on a component table, plain arithmetic that runs anywhere; vote_keep is the rule on the mask
votes, visible_keep the rule on the visibility votes; clean_mesh strings the stages together and reports what each removed."""
import numpy as np
import torch


def _table_column(table, key, dtype):
    x = table[key]
    return (x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(dtype)


def select_components(table, keep="largest", by="faces", min_faces=0, min_area_fraction=0.0):
    """Which components of a vdn_hip.mesh.component_table (or of a dict of numpy arrays with its `n_faces` and `area` columns,
    ordered by ascending root) stay -> bool [C], a tensor on the table's device (numpy for a numpy table).
    keep="largest": the one component with the most faces (by="faces", exact) or the largest area (by="area"), ties to the lower
    root - and only if it passes the two thresholds; keep="all": every component with n_faces >= min_faces and
    area >= min_area_fraction * (total area)."""
    if keep not in ("largest", "all"):
        raise ValueError("keep must be 'largest' or 'all', got %r" % (keep,))
    if by not in ("faces", "area"):
        raise ValueError("by must be 'faces' or 'area', got %r" % (by,))
    if min_faces < 0 or not (0.0 <= float(min_area_fraction) <= 1.0):
        raise ValueError("min_faces must be >= 0 and min_area_fraction in [0, 1], got %r, %r" % (min_faces, min_area_fraction))
    as_numpy = not torch.is_tensor(table["n_faces"])
    n_faces, area = _table_column(table, "n_faces", torch.int64), _table_column(table, "area", torch.float64)
    if n_faces.dim() != 1 or area.shape != n_faces.shape:
        raise ValueError("n_faces and area must be [C] columns of one table")
    ok = (n_faces >= int(min_faces)) & (area >= float(min_area_fraction) * area.sum())
    if keep == "largest" and n_faces.numel() > 0:
        key = n_faces if by == "faces" else area
        first = torch.nonzero(key == key.max()).reshape(-1)[:1]          # (the table is ordered by root: the first is the lowest)
        one = torch.zeros_like(ok)
        one[first] = True
        ok = ok & one
    return ok.numpy() if as_numpy else ok


def vote_keep(n_in_image, n_in_mask, min_inside=1, max_outside=0):
    """The vote rule on vdn_hip.mesh.mask_votes' counts (tensors or numpy): a vertex stays iff at least `min_inside` cameras see it
    inside their mask and at most `max_outside` cameras see it in the image but outside the mask. A camera that does not see the
    vertex at all (behind it, outside the frame) does not vote."""
    if min_inside < 0 or max_outside < 0:
        raise ValueError("min_inside and max_outside must be >= 0, got %r, %r" % (min_inside, max_outside))
    return (n_in_mask >= int(min_inside)) & ((n_in_image - n_in_mask) <= int(max_outside))


def visible_keep(n_visible, min_visible=1):
    """The rule on vdn_hip.mesh.visibility_votes' count (a tensor or numpy): a vertex stays iff at least `min_visible` cameras see
    it unoccluded."""
    if min_visible < 0:
        raise ValueError("min_visible must be >= 0, got %r" % (min_visible,))
    return n_visible >= int(min_visible)


VISIBILITY_DEFAULTS = {"min_visible": 1, "eps": 1e-4, "cell_size": None}


def _visibility_options(visibility):
    """clean_mesh's `visibility` dict with its defaults filled in; ValueError on anything else"""
    if not isinstance(visibility, dict):
        raise ValueError("visibility must be None or a dict with the keys %s, got %r" % (sorted(VISIBILITY_DEFAULTS), visibility))
    unknown = sorted(set(visibility) - set(VISIBILITY_DEFAULTS))
    if unknown:
        raise ValueError("visibility has unknown keys %s (known: %s)" % (unknown, sorted(VISIBILITY_DEFAULTS)))
    opt = dict(VISIBILITY_DEFAULTS, **visibility)
    if int(opt["min_visible"]) != opt["min_visible"]:
        raise ValueError("min_visible must be an integer, got %r" % (opt["min_visible"],))
    visible_keep(0, opt["min_visible"])
    if not (0.0 <= float(opt["eps"]) < 1.0):
        raise ValueError("visibility eps must be in [0, 1), got %r" % (opt["eps"],))
    if opt["cell_size"] is not None and not (0.0 < float(opt["cell_size"]) < float("inf")):
        raise ValueError("visibility cell_size must be positive and finite, got %r" % (opt["cell_size"],))
    return opt


def _image_size(image_size):
    try:
        H, W = (int(x) for x in image_size)
    except (TypeError, ValueError):
        raise ValueError("image_size must be (H, W), got %r" % (image_size,))
    if H < 1 or W < 1:
        raise ValueError("image_size must be positive, got %r" % (image_size,))
    return H, W


def masks_to_uint8(masks, device=None):
    """Object masks in any of the shapes a scene holds them -> uint8 [N,H,W] tensor, 1 = set: bool, integers (nonzero = set) or
    floats (> 0.5), [N,H,W] or [N,H,W,1|3] (channel 0 of a 3-channel mask: vdn_train.dataset.SceneData.masks)."""
    m = masks if torch.is_tensor(masks) else torch.as_tensor(np.asarray(masks))
    if m.dim() == 4 and m.shape[-1] in (1, 3):
        m = m[..., 0]
    if m.dim() != 3:
        raise ValueError("masks must be [N,H,W] or [N,H,W,1|3], got %s" % (tuple(m.shape),))
    if device is not None:
        m = m.to(device)
    return ((m > 0.5) if m.is_floating_point() else (m != 0)).to(torch.uint8).contiguous()


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def clean_mesh(vertices, triangles, *, keep="largest", by="faces", min_faces=0, min_area_fraction=0.0, cameras=None, masks=None,
               dilate=0, min_inside=1, max_outside=0, attributes=(), visibility=None, image_size=None):
    """vertices [V,3] float, triangles [F,3] integer (numpy arrays or CUDA tensors) -> dict(vertices, triangles, attributes,
    vertex_index, report), arrays of the inputs' kind and dtypes.
      1. with `cameras` (float64 [N,3,4], the mesh's frame -> (u w, v w, w): SceneData.projection_matrices) and `masks`
         ([N,H,W] or [N,H,W,1|3]; bool, integer nonzero = set, float > 0.5): masks dilated by the (2 dilate + 1)^2 square, votes
         per vertex, vote_keep(min_inside, max_outside); a face goes when one of its corners does;
      2. connected components of what is left, select_components(keep, by, min_faces, min_area_fraction); the faces of the
         dropped components go;
      3. with `visibility` (None: the stage is off; or a dict with the keys min_visible (1), eps (1e-4) and cell_size (None: the
         grid's default)): the visibility votes of `cameras` on the mesh that survived 1 and 2 - what was dropped casts no
         shadow - and visible_keep(min_visible): a vertex no camera sees unoccluded goes, and a face with it. The stage needs
         `cameras` but not `masks`; without masks, image_size = (H, W) says where the images end.
    Vertices no surviving face uses are dropped, the rest keep their order; vertex_index [V'] int64 holds their old indices and
    `attributes` (a sequence of [V,...] arrays: normals, colours) come back gathered by it. `report` is plain JSON data."""
    from vdn_hip import mesh
    if visibility is None:
        if (cameras is None) != (masks is None):
            raise ValueError("cameras and masks go together: got only one of them")
    else:
        visibility = _visibility_options(visibility)
        if cameras is None:
            raise ValueError("visibility culling needs `cameras`")
        if masks is None and image_size is None:
            raise ValueError("visibility culling without masks needs image_size = (H, W)")
    if image_size is not None:
        image_size = _image_size(image_size)
    select_components({"n_faces": np.zeros(0, np.int64), "area": np.zeros(0)}, keep, by, min_faces, min_area_fraction)   # argument errors first
    vote_keep(0, 0, min_inside, max_outside)
    if int(dilate) != dilate or dilate < 0:
        raise ValueError("dilate must be a non-negative integer, got %r" % (dilate,))
    as_numpy = not torch.is_tensor(vertices)
    v_in = vertices if torch.is_tensor(vertices) else np.asarray(vertices)
    t_in = triangles if torch.is_tensor(triangles) else np.asarray(triangles)
    if v_in.ndim != 2 or v_in.shape[1] != 3 or t_in.ndim != 2 or t_in.shape[1] != 3:
        raise ValueError("clean_mesh needs vertices [V,3] and triangles [F,3], got %s and %s" % (tuple(v_in.shape), tuple(t_in.shape)))
    attributes = list(attributes)
    for x in attributes:
        if x.shape[0] != v_in.shape[0]:
            raise ValueError("an attribute has %d rows for %d vertices" % (x.shape[0], v_in.shape[0]))
    dev = _device_of(v_in, t_in)
    v = v_in.to(dev) if torch.is_tensor(v_in) else torch.from_numpy(np.ascontiguousarray(v_in)).to(dev)
    t = t_in.to(dev) if torch.is_tensor(t_in) else torch.from_numpy(np.ascontiguousarray(t_in)).to(dev)
    if not v.is_floating_point() or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("clean_mesh needs float vertices and integer triangles, got %s and %s" % (v.dtype, t.dtype))
    t_dtype = t.dtype
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    V0, F0 = v.shape[0], t.shape[0]
    report = {"vertices_in": V0, "faces_in": F0, "components_in": int(torch.unique(mesh.connected_components(t, V0)).numel())}
    index = torch.arange(V0, device=dev)

    if masks is not None:
        m = masks_to_uint8(masks, dev)
        if dilate:
            m = mesh.dilate_masks(m, int(dilate))
        if image_size is not None and tuple(m.shape[1:]) != image_size:
            raise ValueError("image_size %s does not match the masks' %s" % (image_size, tuple(m.shape[1:])))
        image_size = tuple(int(x) for x in m.shape[1:])
        n_img, n_msk = mesh.mask_votes(v, cameras, m)
        v, t, idx = mesh.filter_mesh(v, t, keep_vertices=vote_keep(n_img, n_msk, min_inside, max_outside))
        index = index[idx]
        report["mask_culling"] = {"cameras": int(m.shape[0]), "dilate": int(dilate), "min_inside": int(min_inside), "max_outside": int(max_outside),
                                  "vertices_removed": V0 - v.shape[0], "faces_removed": F0 - t.shape[0]}
    V1, F1 = v.shape[0], t.shape[0]

    table = mesh.component_table(v, t, mesh.connected_components(t, V1))
    chosen = select_components(table, keep, by, min_faces, min_area_fraction)
    v, t, idx = mesh.filter_mesh(v, t, keep_faces=chosen[table["face_component"]])
    index = index[idx]
    total, kept = float(table["area"].sum()), float(table["area"][chosen].sum())
    report["components"] = {"keep": keep, "by": by, "min_faces": int(min_faces), "min_area_fraction": float(min_area_fraction),
                            "before": int(chosen.numel()), "after": int(chosen.sum()), "vertices_removed": V1 - v.shape[0],
                            "faces_removed": F1 - t.shape[0], "kept_area_fraction": kept / total if total > 0 else None}

    if visibility is not None:
        V2, F2 = v.shape[0], t.shape[0]
        grid = mesh.MeshGrid(v, t, cell_size=visibility["cell_size"])
        _, n_vis = mesh.visibility_votes(v, t, cameras, image_size, eps=visibility["eps"], grid=grid)
        v, t, idx = mesh.filter_mesh(v, t, keep_vertices=visible_keep(n_vis, visibility["min_visible"]))
        index = index[idx]
        report["visibility_culling"] = {"cameras": int(len(cameras)), "min_visible": int(visibility["min_visible"]), "eps": float(visibility["eps"]),
                                        "vertices_removed": V2 - v.shape[0], "faces_removed": F2 - t.shape[0],
                                        "components_after": int(torch.unique(mesh.connected_components(t, v.shape[0])).numel())}
    report.update(vertices_out=int(v.shape[0]), faces_out=int(t.shape[0]))

    t = t.to(t_dtype)
    host = index.cpu()
    gathered = [x[index.to(x.device)] if torch.is_tensor(x) else np.asarray(x)[host.numpy()] for x in attributes]
    if as_numpy:
        v, t, index = v.cpu().numpy(), t.cpu().numpy(), host.numpy()
    return {"vertices": v, "triangles": t, "attributes": gathered, "vertex_index": index, "report": report}
