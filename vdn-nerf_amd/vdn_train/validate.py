"""Whole-image rendering through the HIP renderer: Runner.validate_image (dpt_runner.py:520-587: colour + normal image),
Runner.render_novel_image (589-616: interpolated view) and the arithmetic of Runner.val_img (dpt_runner.py:417-491) - rays of
one camera in batches, colour image, L1 / PSNR against the ground truth, and the weight-argmax depth written back as
`depth_from_sdf/sdf_<name>.npy` for the wavelet fine-tuning loop (dpt_runner.py:449-453). Everything stays on the device
until the final image copy (the reference copies every batch to the host). validate_mesh (dpt_runner.py:699-713) writes the
extracted surface as a PLY file, with vertex normals and colours."""
import os

import numpy as np
import torch

from vdn_hip import switches


def _render_batches(renderer, rays_gen, rays_o, rays_d, batch_size, jitter=None, **kw):
    """render() over the rays of one image in batches -> yields (first ray, n rays, outputs). With VDN_RENDER_GRAPH=1 the
    full batches replay one captured plan (dpt_models.renderer.RenderPlan: a fifth of the host time per batch, ~3% more device
    time) and only the ragged last batch is a plain call. The outputs of a replay are overwritten by the next one: consume
    them before advancing. jitter: optional list of (t_rand [n,1], t_rand_out [n,O]) per batch, injected in place of the two
    torch.rand draws of render() (renderer.py:348,355) - how the parity tests reproduce the reference's runs."""
    n = rays_o.shape[0]
    plan = None
    if switches.flag("VDN_RENDER_GRAPH") and n >= 2 * batch_size and jitter is None:
        plan = renderer.plan(batch_size, **kw)
    for b, s in enumerate(range(0, n, batch_size)):
        o, d = rays_o[s:s + batch_size], rays_d[s:s + batch_size]
        near, far = rays_gen.near_far_from_sphere(o, d)
        if plan is not None and o.shape[0] == batch_size:
            yield s, batch_size, plan(o, d, near, far)
        elif jitter is not None:
            yield s, o.shape[0], renderer.render(o, d, near, far, t_rand=jitter[b][0], t_rand_out=jitter[b][1], **kw)
        else:
            yield s, o.shape[0], renderer.render(o, d, near, far, **kw)


@torch.no_grad()
def render_image(renderer, rays_gen, idx, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0, white_bkgd=True,
                 gen_depth_for_finetune=False, jitter=None):
    """-> dict(img_fine [H,W,3] float32 in [0,1], gradient_error [n_batches], weight_depth [H,W,1] | None)."""
    rays_o, rays_d = rays_gen.gen_rays_at(idx, resolution_level=resolution_level)
    H, W, _ = rays_o.shape
    rays_o, rays_d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    dev = rays_o.device
    bg = torch.ones(1, 3, device=dev) if white_bkgd else None
    rgb = torch.empty(H * W, 3, device=dev)
    depth = torch.empty(H * W, 1, device=dev) if gen_depth_for_finetune else None
    eik = []
    for s, n, out in _render_batches(renderer, rays_gen, rays_o, rays_d, batch_size, jitter=jitter, cos_anneal_ratio=cos_anneal_ratio, background_rgb=bg):
        rgb[s:s + n] = out["color_fine"]
        eik.append(out["gradient_error"].clone())
        if gen_depth_for_finetune:                                   # dpt_runner.py:449-455
            inside = out["inside_sphere"]
            w = out["weights"][:, :inside.shape[1]] * inside
            depth[s:s + n] = out["z_vals"].gather(1, torch.argmax(w, dim=-1, keepdim=True))
        del out
    return {"img_fine": rgb.reshape(H, W, 3).cpu().numpy(), "gradient_error": torch.stack(eik).cpu().numpy(),
            "weight_depth": depth.reshape(H, W, 1).cpu().numpy() if gen_depth_for_finetune else None}


@torch.no_grad()
def validate_image(renderer, rays_gen, idx, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0, white_bkgd=True,
                   depth_before_color=False, out_dir=None, iter_step=0, jitter=None):
    """Runner.validate_image (dpt_runner.py:520-587): the colour image and the normal image of one camera.
    -> (img_fine [H,W,3] in 0..255, normal_img [H,W,3] in 0..255): normals = sum_i gradients_i * weights_i * inside_sphere_i
    per ray (553-557), rotated into the camera frame by inv(pose[:3,:3]) and mapped by * 128 + 128 (570-573). With `out_dir`
    the two PNGs are written as the runner writes them (575-587): validations_fine/ holds the render stacked over the
    ground-truth image (`image_at`), normals/ the normal image. The pipeline's channel order is cv.imread's BGR
    (dataset._read_png) and cv.imwrite takes its array as BGR, so the files show true colours: PIL gets the array reversed."""
    rays_o, rays_d = rays_gen.gen_rays_at(idx, resolution_level=resolution_level)
    H, W, _ = rays_o.shape
    rays_o, rays_d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    dev = rays_o.device
    bg = torch.ones(1, 3, device=dev) if white_bkgd else None
    rgb = torch.empty(H * W, 3, device=dev)
    nrm = torch.empty(H * W, 3, device=dev)
    n_in = renderer.n_samples + renderer.n_importance
    for s, n, out in _render_batches(renderer, rays_gen, rays_o, rays_d, batch_size, jitter=jitter, cos_anneal_ratio=cos_anneal_ratio,
                                     background_rgb=bg, depth_before_color=depth_before_color):
        rgb[s:s + n] = out["color_fine"]
        nrm[s:s + n] = (out["gradients"] * out["weights"][:, :n_in, None] * out["inside_sphere"][..., None]).sum(dim=1)
        del out
    img_fine = (rgb.reshape(H, W, 3).cpu().numpy() * 255).clip(0, 255)
    rot = np.linalg.inv(rays_gen.pose_all[idx, :3, :3].detach().cpu().numpy())
    normal_img = (np.matmul(rot[None, :, :], nrm.cpu().numpy()[:, :, None]).reshape(H, W, 3) * 128 + 128).clip(0, 255)
    if out_dir is not None:
        from PIL import Image
        val_im = np.concatenate([img_fine, rays_gen.image_at(idx, resolution_level=resolution_level)])      # dpt_runner.py:577-578
        for sub, arr in (("validations_fine", val_im), ("normals", normal_img)):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
            # cv.imwrite(path, float array) = the array read as BGR, converted with saturate_cast<uchar> (round to nearest):
            # hand PIL the RGB view of that
            Image.fromarray(np.ascontiguousarray(np.rint(arr).clip(0, 255).astype(np.uint8)[..., ::-1])).save(
                os.path.join(out_dir, sub, "{:0>8d}_{}_{}.png".format(iter_step, 0, idx)))
    return img_fine, normal_img


@torch.no_grad()
def render_novel_image(renderer, rays_gen, idx_0, idx_1, ratio, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0,
                       white_bkgd=True, depth_before_color=False):
    """Runner.render_novel_image (dpt_runner.py:589-616): the view interpolated between two cameras -> uint8 [H,W,3]
    (the runner's `* 256` clip). Argument order as RaysGenerator.gen_rays_between defines it (ratio first, poses.py:214);
    the runner itself calls it with (idx_0, idx_1, ratio), SURVEY.md Appendix A."""
    rays_o, rays_d = rays_gen.gen_rays_between(ratio, idx_0, idx_1, resolution_level=resolution_level)
    H, W, _ = rays_o.shape
    rays_o, rays_d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    dev = rays_o.device
    bg = torch.ones(1, 3, device=dev) if white_bkgd else None
    rgb = torch.empty(H * W, 3, device=dev)
    for s, n, out in _render_batches(renderer, rays_gen, rays_o, rays_d, batch_size, cos_anneal_ratio=cos_anneal_ratio,
                                     background_rgb=bg, depth_before_color=depth_before_color):
        rgb[s:s + n] = out["color_fine"]
    return (rgb.reshape(H, W, 3).cpu().numpy() * 256).clip(0, 255).astype(np.uint8)


def image_metrics(img_fine, gt, mask=None):
    """color L1 and PSNR of dpt_runner.py:470-474 (mask = ones when masks are not used)."""
    mask = np.ones_like(gt[..., :1]) if mask is None else (mask > 0.1).astype(np.float32)
    mask_sum = mask.sum() + 1e-5
    l1 = np.abs((img_fine - gt) * mask).sum() / mask_sum
    psnr = 20.0 * np.log10(1.0 / np.sqrt(((img_fine - gt) ** 2 * mask).sum() / (mask_sum * 3.0)))
    return float(l1), float(psnr)


def weight_max_image(weight_depth):
    """The runner's picture of the weight-argmax depths (dpt_runner.py:463-468): stretched between their 50th and 95th percentile."""
    lb, ub = np.percentile(weight_depth, [50, 95])
    return ((weight_depth - lb) / (ub - lb) * 255).clip(0, 255)


def val_img(renderer, scene, rays_gen, idx, resolution_level=1, batch_size=512, cos_anneal_ratio=1.0, white_bkgd=True,
            use_mask=False, gen_depth_for_finetune=False, jitter=None, out_dir=None, iter_step=0):
    """Runner.val_img (dpt_runner.py:417-491) for a vdn_train.dataset.SceneData (or None: nothing is written into a scene
    directory then): -> (color_loss, psnr, gradient_error, img_fine). The ground truth is the generator's `image_at` / `mask_at`
    (poses.py:254-262: cv.resize of the loaded image) as in the reference; with gen_depth_for_finetune the weight-argmax depths
    go to depth_from_sdf/sdf_<name>.npy under the scene directory (449-453) and, with `out_dir`, their picture to
    weight_max/weight_max_<iter>_<idx>.png (463-468)."""
    res = render_image(renderer, rays_gen, idx, resolution_level, batch_size, cos_anneal_ratio, white_bkgd, gen_depth_for_finetune, jitter=jitter)
    gt = rays_gen.image_at(idx, resolution_level=resolution_level) / 255.0
    mask = rays_gen.mask_at(idx, resolution_level=resolution_level) if use_mask else None
    l1, psnr = image_metrics(res["img_fine"], gt, mask)
    if gen_depth_for_finetune:
        if scene is not None:
            path = scene.depth_from_sdf_path(idx)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, res["weight_depth"])
        if out_dir is not None:
            from PIL import Image
            os.makedirs(os.path.join(out_dir, "weight_max"), exist_ok=True)
            Image.fromarray(np.rint(weight_max_image(res["weight_depth"])[..., 0]).astype(np.uint8)).save(
                os.path.join(out_dir, "weight_max", "weight_max_{}_{}.png".format(iter_step, idx)))
    return l1, psnr, res["gradient_error"], res["img_fine"]


def validate_mesh(renderer, bound_min, bound_max, out_path, resolution=256, threshold=0.0, world_space=False, scale_mat=None,
                  vertex_colors=True, vertex_normals=True, clean=None, sparse=None, simplify=None, texture=None):
    """Runner.validate_mesh (dpt_runner.py:699-713) without trimesh: the iso-surface of the SDF network inside the box, written
    to `out_path` as a binary PLY (vdn_train/meshio.py) -> (out_path, V, F). `world_space` maps the vertices by
    v * scale_mat[0,0] + scale_mat[:3,3] (708; a uniform scale and a translation: unit normals are unchanged). Beyond the
    reference's bare mesh, each vertex carries its unit normal and its colour seen straight down that normal
    (NeuSRenderer.extract_colored_geometry); with both flags off the file is the reference's and no network runs past the lattice.
    `clean` (a dict of vdn_train.mesh_clean.clean_mesh's keyword arguments, or None: the raw surface) cleans the mesh in object
    space, before the world_space map; normals and colours follow their vertices, and V, F are the cleaned mesh's. `sparse` is
    extract_geometry's: None (dense, or what VDN_MESH_SPARSE says), True or a dict - the same file from the bricks near the surface.
    `simplify` (a dict of vdn_train.mesh_simplify.simplify_mesh's keyword arguments - cell_size or target_faces, or cell_size with
    tolerance / levels for the adaptive mode, in object-space units - or None: the file as it always was) thins the mesh after
    `clean` and before the world_space map. The vertices are then
    shaded AFTER the simplification, at their new positions (renderer.shade_vertices): normals and colours come from the networks,
    not from averages, and the fine surface is never shaded at all - one shading pass, over the vertices that reach the file.
    `texture` (a dict of vdn_hip.mesh.bake_texture's keyword arguments - texture_size, patch, project, ... - or None: nothing beyond
    the PLY) bakes a per-face atlas of the mesh that reaches the file, after `clean` and `simplify`, in object space, and writes
    <stem>.obj, <stem>.mtl and <stem>.png beside the PLY (vdn_train.meshio.write_obj), the vertices mapped as the PLY's are. The PLY
    and the return value are what they are without it. A "photos" entry ({"P": object-space cameras, "images": ...}, bake_texture's)
    colours the atlas from the photographs instead of the colour network."""
    from vdn_train import meshio
    if texture is not None and not isinstance(texture, dict):
        raise ValueError("texture must be a dict of bake_texture's keyword arguments, got %r" % (texture,))
    normals = colors = None
    if simplify is not None:
        from vdn_train import mesh_simplify
        if "attributes" in simplify:
            raise ValueError("validate_mesh shades the simplified vertices itself: `simplify` takes no attributes")
        vertices, triangles = renderer.extract_geometry(bound_min, bound_max, resolution=resolution, threshold=threshold, sparse=sparse)
        if clean is not None:
            from vdn_train import mesh_clean
            res = mesh_clean.clean_mesh(vertices, triangles, **clean)
            vertices, triangles = res["vertices"], res["triangles"]
        res = mesh_simplify.simplify_mesh(vertices, triangles, **simplify)
        vertices, triangles = res["vertices"], res["triangles"]
        if vertex_colors or vertex_normals:
            normals, colors = renderer.shade_vertices(vertices)
            normals = normals if vertex_normals else None
            colors = colors if vertex_colors else None
        clean = None
    elif vertex_colors or vertex_normals:
        vertices, triangles, normals, colors = renderer.extract_colored_geometry(bound_min, bound_max, resolution=resolution, threshold=threshold,
                                                                                   sparse=sparse)
        normals = normals if vertex_normals else None
        colors = colors if vertex_colors else None
    else:
        vertices, triangles = renderer.extract_geometry(bound_min, bound_max, resolution=resolution, threshold=threshold, sparse=sparse)
    if clean is not None:
        from vdn_train import mesh_clean
        attrs = [x for x in (normals, colors) if x is not None]
        res = mesh_clean.clean_mesh(vertices, triangles, attributes=attrs, **clean)
        vertices, triangles, attrs = res["vertices"], res["triangles"], list(res["attributes"])
        normals = attrs.pop(0) if normals is not None else None
        colors = attrs.pop(0) if colors is not None else None
    baked = None
    if texture is not None:
        from vdn_train import mesh_texture
        baked = mesh_texture.bake_texture(renderer, np.asarray(vertices), np.asarray(triangles), **texture)
    if world_space:
        if scale_mat is None:
            raise ValueError("world_space=True needs the scene's scale_mat (SceneData.scale_mats_np[0])")
        scale_mat = np.asarray(scale_mat)
        vertices = vertices * scale_mat[0, 0] + scale_mat[:3, 3][None]
    out_dir = os.path.dirname(out_path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    meshio.write_ply(out_path, vertices, triangles, normals=normals, colors=colors)
    if baked is not None:
        meshio.write_obj(os.path.splitext(out_path)[0] + ".obj", vertices, triangles, baked["uv"], baked["texture"], normals=normals)
    return out_path, int(vertices.shape[0]), int(triangles.shape[0])


def validate_scene_mesh(renderer, scene, out_dir, iter_step=0, clean=None, simplify=None, texture=None, **kw):
    """validate_mesh for a vdn_train.dataset.SceneData: its object bounding box and scale_mats_np[0], the runner's file name
    meshes/<iter_step, 8 digits>.ply under `out_dir` (dpt_runner.py:700-711). A `clean` dict with a true "use_masks" entry gets
    the scene's object-space cameras and its masks (cleaning happens in object space); a true "use_cameras" entry gets the cameras
    and the image size without the masks - what a "visibility" entry needs (either of the two satisfies it). `simplify` is
    validate_mesh's, in object-space units, and so is `texture`: meshes/<iter_step>.obj, .mtl and .png beside the PLY. A `texture`
    dict with "photos": True (or a dict of photo_colors' options - cos_min, feather, eps, blend, fill) colours the atlas from the
    scene's own photographs: its object-space cameras and its decoded images are filled in (vdn_hip.mesh.bake_texture(photos=))."""
    if clean is not None:
        clean = dict(clean)
        use_masks, use_cameras = clean.pop("use_masks", False), clean.pop("use_cameras", False)
        if use_masks:
            clean.update(cameras=scene.projection_matrices(world_space=False), masks=scene.masks)
        elif use_cameras:
            clean.update(cameras=scene.projection_matrices(world_space=False), image_size=(int(scene.H), int(scene.W)))
    if isinstance(texture, dict) and texture.get("photos") is not None and texture["photos"] is not False:
        photos = {} if texture["photos"] is True else texture["photos"]
        if not isinstance(photos, dict):
            raise ValueError("texture['photos'] must be True or a dict of bake_texture's photo options, got %r" % (photos,))
        photos = dict(photos)
        photos.setdefault("P", scene.projection_matrices(world_space=False))
        photos.setdefault("images", scene.images)
        texture = dict(texture, photos=photos)
    bound_min = torch.tensor(scene.object_bbox_min, dtype=torch.float32)
    bound_max = torch.tensor(scene.object_bbox_max, dtype=torch.float32)
    return validate_mesh(renderer, bound_min, bound_max, os.path.join(out_dir, "meshes", "{:0>8d}.ply".format(iter_step)),
                         scale_mat=scene.scale_mats_np[0], clean=clean, simplify=simplify, texture=texture, **kw)
