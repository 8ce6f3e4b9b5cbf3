"""Texture a mesh file with the colour network (vdn_train/mesh_texture.py; INTEGRATION.md "Textured meshes"): every face gets a
patch of a per-face atlas, baked on the device, and the mesh goes out as an OBJ with its material library and its PNG:

    python tools/texture_mesh.py meshes/light.ply light.obj --checkpoint ckpt_300000.pth --texture-size 4096
    python tools/texture_mesh.py light.ply light.obj --synthetic 0 --patch 8 --project 0

MESH.ply is a PLY of vdn_train.meshio in the networks' object space (validate_mesh without world_space writes one; simplify it
first - tools/simplify_mesh.py - so that a face has more than a handful of texels). --checkpoint: a file with the runner's keys
(nerf, sdf_network_fine, variance_network_fine, color_network_fine); --synthetic SEED: vdn_train.synth.make_all_states(SEED).
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
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint", default=None, metavar="CKPT", help="trained weights, the runner's checkpoint file")
    src.add_argument("--synthetic", type=int, default=None, metavar="SEED", help="the synthetic weights of that seed")
    ap.add_argument("--texture-size", type=int, default=2048, metavar="S", help="the atlas is S x S texels")
    ap.add_argument("--patch", type=int, default=None, metavar="N", help="texels per cell edge (default: the largest that fits)")
    ap.add_argument("--project", type=int, default=2, metavar="K", help="Newton steps of the texel points towards the level set")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main():
    a = parser().parse_args()
    import torch
    from vdn_hip import mesh
    from vdn_train import factory, meshio, synth
    dev = torch.device(a.device)
    if a.synthetic is not None:
        states = synth.make_all_states(a.synthetic)
    else:
        ckpt = torch.load(a.checkpoint, map_location="cpu")
        states = {k: {n: (x.numpy() if torch.is_tensor(x) else x) for n, x in ckpt[k].items()}
                  for k in ("nerf", "sdf_network_fine", "variance_network_fine", "color_network_fine")}
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
    with torch.cuda.device(dev), torch.no_grad():
        v = torch.from_numpy(m["vertices"]).to(dev)
        t = torch.from_numpy(m["triangles"]).to(dev)
        layout = mesh.texture_layout(t.shape[0], a.texture_size, a.patch)
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
    print(json.dumps({"mesh": a.mesh, "out": a.out, "vertices": int(v.shape[0]), "faces": int(t.shape[0]), "patch": layout["n"],
                      "texels_shaded": layout["points"], "texture_size": layout["S"], "project": a.project, "seconds": seconds}))


if __name__ == "__main__":
    main()
