"""Textured meshes: bake the colour network's view of a (simplified) surface into a per-face atlas and look it up again - the
numpy-in / numpy-out front door of vdn_hip/mesh.py's bake_texture, sample_texture and render_textured_view (csrc/mesh_texture.hip;
DESIGN.md 3q, INTEGRATION.md "Textured meshes"). vdn_train.meshio.write_obj puts the result on disk; validate_mesh(texture=...) and
tools/texture_mesh.py do both. bake_photo_texture colours the atlas from a scene's photographs instead (csrc/mesh_photo.hip,
DESIGN.md 3t)."""
import numpy as np
import torch

from vdn_train.mesh_clean import _device_of


def _to_dev(x, dev):
    return x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def bake_texture(renderer, vertices, triangles, **kw):
    """vdn_hip.mesh.bake_texture for arrays of either kind -> {"texture", "uv", "layout", "points"}: texture (uint8 [S,S,3] RGB) and
    points (fp32 [F T,3]) are numpy arrays when the vertices are, device tensors otherwise; uv is always float64 [F,3,2] numpy."""
    from vdn_hip import mesh
    res = mesh.bake_texture(renderer, vertices, triangles, **kw)
    if not torch.is_tensor(vertices):
        res["texture"], res["points"] = res["texture"].cpu().numpy(), res["points"].cpu().numpy()
    return res


def scene_photos(source, views=None):
    """The cameras and photographs of a scene as bake_texture's `photos` takes them -> (P float64 [N,3,4] numpy, images [N,H,W,3]
    float32, numpy or device tensor). source: a vdn_train.dataset.SceneData (its object-space cameras, projection_matrices(
    world_space=False), and its decoded images), a pair (SceneData, RaysGenerator) (the images already resident on the device), a
    lone RaysGenerator (cameras rebuilt in float64 from its fixed poses and intrinsics) or an explicit pair (P, images). views: the
    indices of the cameras to use, in the order they are to be visited (default: all)."""
    from vdn_train.rays import RaysGenerator
    if isinstance(source, RaysGenerator):
        K = torch.inverse(source.intrin_inv.double().cpu())
        w2c = torch.inverse(source.pose_all.double().cpu())[:, :3, :4]
        P, images = (K @ w2c).numpy(), source.images
    elif isinstance(source, (tuple, list)) and len(source) == 2:
        first, second = source
        if hasattr(first, "projection_matrices"):
            P, images = first.projection_matrices(world_space=False), (second.images if isinstance(second, RaysGenerator) else second)
        else:
            P, images = first, second
    elif hasattr(source, "projection_matrices") and hasattr(source, "images"):
        P, images = source.projection_matrices(world_space=False), source.images
    else:
        raise ValueError("the photographs come from a SceneData, a RaysGenerator, (SceneData, RaysGenerator) or (P, images), got %r" % (type(source),))
    P = np.asarray(P.detach().cpu() if torch.is_tensor(P) else P, dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] != (3, 4) or len(images) != len(P):
        raise ValueError("P must be [N,3,4] with one image per camera, got %s and %d images" % (P.shape, len(images)))
    if views is not None:
        idx = np.asarray(views)
        if idx.ndim != 1 or idx.dtype.kind not in "iu" or (len(idx) and (idx.min() < 0 or idx.max() >= len(P))):
            raise ValueError("views must be camera indices in [0, %d), got %r" % (len(P), views))
        P = P[idx]
        images = images[torch.as_tensor(idx, device=images.device).long()] if torch.is_tensor(images) else np.asarray(images)[idx]
    return P, images


def bake_photo_texture(renderer, scene, vertices, triangles, views=None, cos_min=None, feather=None, eps=None, blend=None, fill=None, **kw):
    """bake_texture with the atlas coloured from the photographs (vdn_hip.mesh.bake_texture(photos=), csrc/mesh_photo.hip): every
    texel takes the weighted mean - or, blend="best", the best view - of the cameras that see it, and the colour network's answer
    (or `fill`, without a renderer) where none does -> bake_texture's dict plus "coverage" and "n_views"; numpy in, numpy out.
    renderer may be None when project=0. scene: whatever scene_photos takes; views selects cameras. The cameras are the scene's
    fixed ones: learned poses are the caller's business - whoever trained with refined poses passes (P, images) with the P built
    from them. The mesh is in object space, like P. The remaining keywords are bake_texture's (texture_size, patch, project, ...)."""
    from vdn_hip import mesh
    P, images = scene_photos(scene, views)
    photos = {"P": P, "images": images}
    photos.update({k: x for k, x in (("cos_min", cos_min), ("feather", feather), ("eps", eps), ("blend", blend), ("fill", fill)) if x is not None})
    res = mesh.bake_texture(renderer, vertices, triangles, photos=photos, **kw)
    if not torch.is_tensor(vertices):
        res["texture"], res["points"], res["n_views"] = res["texture"].cpu().numpy(), res["points"].cpu().numpy(), res["n_views"].cpu().numpy()
    return res


def sample_texture(texture, layout, vertices, triangles, face, points, background=(1.0, 1.0, 1.0)):
    """vdn_hip.mesh.sample_texture for arrays of either kind -> fp32 [R,3] RGB, numpy when the texture is."""
    from vdn_hip import mesh
    dev = _device_of(texture, vertices, triangles)
    t = _to_dev(triangles, dev)
    if t.dtype not in (torch.int32, torch.int64) and not t.is_floating_point() and t.dtype != torch.bool:
        t = t.long()
    with torch.cuda.device(dev):
        rgb = mesh.sample_texture(_to_dev(texture, dev), layout, _to_dev(vertices, dev), t, _to_dev(face, dev), _to_dev(points, dev),
                                  background=background)
    return rgb if torch.is_tensor(texture) else rgb.cpu().numpy()


def render_textured_view(vertices, triangles, baked, origins, directions, background=(1.0, 1.0, 1.0)):
    """The baked mesh seen along rays (vdn_hip.mesh.render_textured_view over a MeshGrid built here) -> fp32 [R,3] RGB, numpy when
    the vertices are. baked: bake_texture's result for this mesh."""
    from vdn_hip import mesh
    dev = _device_of(vertices, triangles, baked["texture"])
    t = _to_dev(triangles, dev)
    if t.dtype not in (torch.int32, torch.int64):
        t = t.long()
    with torch.cuda.device(dev):
        grid = mesh.MeshGrid(_to_dev(vertices, dev), t)
        rgb = mesh.render_textured_view(grid, dict(baked, texture=_to_dev(baked["texture"], dev)), _to_dev(origins, dev), _to_dev(directions, dev),
                                        background=background)
    return rgb if torch.is_tensor(vertices) else rgb.cpu().numpy()
