"""Textured meshes: bake the colour network's view of a (simplified) surface into a per-face atlas and look it up again - the
numpy-in / numpy-out front door of vdn_hip/mesh.py's bake_texture, sample_texture and render_textured_view (csrc/mesh_texture.hip;
DESIGN.md 3q, INTEGRATION.md "Textured meshes"). vdn_train.meshio.write_obj puts the result on disk; validate_mesh(texture=...) and
tools/texture_mesh.py do both."""
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
