"""Texture a mesh file with the colour network or from the photographs (vdn_train/mesh_texture.py; INTEGRATION.md "Textured meshes"): every face gets a
patch of a per-face atlas, baked on the device, and the mesh goes out as an OBJ with its material library and its PNG:

    python tools/texture_mesh.py meshes/light.ply light.obj --checkpoint ckpt_300000.pth --texture-size 4096
    python tools/texture_mesh.py light.ply light.obj --synthetic 0 --patch 8 --project 0
    python tools/texture_mesh.py light.ply light.obj --checkpoint ckpt.pth --photos data/scene --blend best
    python tools/texture_mesh.py light.ply light.obj --photos data/scene --project 0

MESH.ply is a PLY of vdn_train.meshio in the networks' object space (validate_mesh without world_space writes one; simplify it
first - tools/simplify_mesh.py - so that a face has more than a handful of texels). --checkpoint: a file with the runner's keys
(nerf, sdf_network_fine, variance_network_fine, color_network_fine); --synthetic SEED: vdn_train.synth.make_all_states(SEED).
--photos SCENE_DIR colours the atlas from the scene's photographs (its cameras_sphere.npz and image/*.png; the mesh must be in the
scene's object space): every texel takes the weighted mean (--blend best: the best view) of the cameras that see it, the colour
network's answer where none does - or mid grey when no weights are given, which --project 0 allows.
The file's vertex normals go into the OBJ; its vertex colours are not used. The last line printed is one JSON record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("out")
    src = ap.add_mutually_exclusive_group()                # (one of the two, unless --photos is given with --project 0: main checks)
    src.add_argument("--checkpoint", default=None, metavar="CKPT", help="trained weights, the runner's checkpoint file")
    src.add_argument("--synthetic", type=int, default=None, metavar="SEED", help="the synthetic weights of that seed")
    ap.add_argument("--texture-size", type=int, default=2048, metavar="S", help="the atlas is S x S texels")
    ap.add_argument("--patch", type=int, default=None, metavar="N", help="texels per cell edge (default: the largest that fits)")
    ap.add_argument("--project", type=int, default=2, metavar="K", help="Newton steps of the texel points towards the level set")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--photos", default=None, metavar="SCENE_DIR", help="colour the texels from this scene's photographs")
    ap.add_argument("--blend", choices=("mean", "best"), default="mean", help="the weighted mean of the cameras that see a texel, or the best one")
    ap.add_argument("--cos-min", type=float, default=0.2, metavar="C", help="a camera counts where the cosine of its viewing angle exceeds C")
    ap.add_argument("--feather", type=float, default=16.0, metavar="PX", help="the band along an image's border over which its weight falls to 0")
    ap.add_argument("--views", default=None, metavar="I,J,...", help="the cameras to use, by index (default: all)")
    return ap


def check_sources(ap, a):
    """exactly one source of weights - or none, when the photographs colour the atlas and nothing is projected"""
    if a.checkpoint is None and a.synthetic is None and not (a.photos is not None and a.project == 0):
        ap.error("one of the arguments --checkpoint --synthetic is required (unless --photos is given with --project 0)")
    if a.views is not None:
        try:
            a.views = [int(x) for x in a.views.split(",")]
        except ValueError:
            ap.error("--views takes camera indices separated by commas, got %r" % (a.views,))
    if a.photos is None and (a.views is not None or a.blend != "mean"):
        ap.error("--views and --blend need --photos")


def main():
    ap = parser()
    a = ap.parse_args()
    check_sources(ap, a)
    import torch
    from vdn_hip import mesh
    from vdn_train import factory, meshio, synth
    dev = torch.device(a.device)
    rend = None
    if a.synthetic is not None:
        states = synth.make_all_states(a.synthetic)
    elif a.checkpoint is not None:
        ckpt = torch.load(a.checkpoint, map_location="cpu")
        states = {k: {n: (x.numpy() if torch.is_tensor(x) else x) for n, x in ckpt[k].items()}
                  for k in ("nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine")}
    if a.synthetic is not None or a.checkpoint is not None:
        rend = factory.build_renderer(device=dev, states=states, precision=a.precision)
    m = meshio.read_ply(a.mesh)
    seconds = {}

    def stage(name, fn):
        torch.cuda.synchronize(dev)
        s = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        seconds[name] = time.perf_counter() - s
        return out
    record = {}
    with torch.cuda.device(dev), torch.no_grad():
        v = torch.from_numpy(m["vertices"]).to(dev)
        t = torch.from_numpy(m["triangles"]).to(dev)
        layout = mesh.texture_layout(t.shape[0], a.texture_size, a.patch)
        if a.photos is not None:
            from vdn_train import dataset, mesh_texture
            P, images = mesh_texture.scene_photos(dataset.SceneData(a.photos), a.views)
            photos = {"P": P, "images": torch.from_numpy(images).to(dev), "blend": a.blend, "cos_min": a.cos_min, "feather": a.feather}
            # (one stage: the projection, the photo launch and the network's answer for the texels no camera sees)
            baked = stage("photo", lambda: mesh.bake_texture(rend, v, t, texture_size=a.texture_size, patch=a.patch, project=a.project, photos=photos))
            texture, record = baked["texture"], {"coverage": baked["coverage"], "views": int(len(P)), "blend": a.blend}
        else:
            points, _ = stage("points", lambda: mesh.texel_points(v, t, layout))
            if a.project > 0 and t.shape[0] > 0:
                r = mesh.mean_edge_length(v, t)
                points = stage("project", lambda: mesh.project_points(rend, points, rounds=a.project, max_offset=r))
            if t.shape[0] > 0:
                colors = stage("shade", lambda: mesh.shade_points(rend, points)[2])
            else:
                colors = torch.empty(0, 3, device=dev)
            texture = stage("gather", lambda: mesh.gather_atlas(colors, layout))
    stage("write", lambda: meshio.write_obj(a.out, m["vertices"], m["triangles"], mesh.texture_uv(layout), texture.cpu().numpy(), normals=m["normals"]))
    print(json.dumps(dict({"mesh": a.mesh, "out": a.out, "vertices": int(v.shape[0]), "faces": int(t.shape[0]), "patch": layout["n"],
                           "texels_shaded": layout["points"], "texture_size": layout["S"], "project": a.project, "seconds": seconds}, **record)))


if __name__ == "__main__":
    main()
