"""Clean a mesh file on the device (vdn_train/mesh_clean.py; INTEGRATION.md "Mesh cleaning"): drop what projects outside the
scene's object masks, then keep the largest connected piece (or every piece above a size), then - on request - drop what none of
the scene's cameras sees:

    python tools/clean_mesh.py meshes/00300000.ply clean.ply --scene data/scan24 --dilate 50 --world-space
    python tools/clean_mesh.py raw.ply clean.ply --keep all --min-faces 100
    python tools/clean_mesh.py meshes/00300000.ply clean.ply --scene data/scan24 --dilate 50 --world-space --visible-from 1

Both files are PLYs of vdn_train.meshio (validate_mesh writes one); normals and colours follow their vertices. With --scene the
masks and cameras of that scene directory vote (--world-space: the mesh was written by validate_mesh(world_space=True); otherwise
it is in object space). Prints the report as one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("out")
    ap.add_argument("--keep", choices=("largest", "all"), default="largest")
    ap.add_argument("--by", choices=("faces", "area"), default="faces", help="what 'largest' means")
    ap.add_argument("--min-faces", type=int, default=0, help="components with fewer faces go")
    ap.add_argument("--min-area-fraction", type=float, default=0.0, help="components under this share of the total area go")
    ap.add_argument("--scene", default=None, help="scene directory: its masks and cameras cull the vertices first")
    ap.add_argument("--dilate", type=int, default=0, help="dilate the masks by the (2 R + 1)^2 square")
    ap.add_argument("--min-inside", type=int, default=1, help="a vertex needs this many views inside the mask")
    ap.add_argument("--max-outside", type=int, default=0, help="and at most this many views in the image but outside the mask")
    ap.add_argument("--world-space", action="store_true", help="the mesh is in world space (scale_mat applied)")
    ap.add_argument("--visible-from", type=int, default=None, metavar="K",
                    help="ray-cast visibility culling: a vertex needs K of the scene's cameras to see it unoccluded (needs --scene; absent = off)")
    ap.add_argument("--visibility-eps", type=float, default=None,
                    help="the visibility segments end at 1 - EPS of the way to the vertex (needs --visible-from; default: clean_mesh's)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main():
    ap = parser()
    a = ap.parse_args()
    if a.visible_from is not None and a.scene is None:
        ap.error("--visible-from needs --scene (the cameras are the scene's)")
    if a.visibility_eps is not None and a.visible_from is None:
        ap.error("--visibility-eps needs --visible-from")
    import torch
    from vdn_train import mesh_clean, meshio
    m = meshio.read_ply(a.mesh)
    kw = dict(keep=a.keep, by=a.by, min_faces=a.min_faces, min_area_fraction=a.min_area_fraction)
    if a.scene is not None:
        from vdn_train.dataset import SceneData
        scene = SceneData(a.scene)
        kw.update(cameras=scene.projection_matrices(world_space=a.world_space), masks=scene.masks, dilate=a.dilate,
                  min_inside=a.min_inside, max_outside=a.max_outside)
        if a.visible_from is not None:
            kw["visibility"] = dict(min_visible=a.visible_from, **({} if a.visibility_eps is None else {"eps": a.visibility_eps}))
    names = [n for n in ("normals", "colors") if m[n] is not None]
    with torch.cuda.device(torch.device(a.device)):
        res = mesh_clean.clean_mesh(m["vertices"], m["triangles"], attributes=[m[n] for n in names], **kw)
    meshio.write_ply(a.out, res["vertices"], res["triangles"], **dict(zip(names, res["attributes"])))
    print(json.dumps(dict(res["report"], mesh=a.mesh, out=a.out)))


if __name__ == "__main__":
    main()
