"""Simplify a mesh file on the device (vdn_train/mesh_simplify.py; INTEGRATION.md "Mesh simplification"): vertex clustering on a
grid of cubic cells, each cluster's vertex placed by its quadric (or at its members' mean):

    python tools/simplify_mesh.py meshes/00300000.ply light.ply --target-faces 200000
    python tools/simplify_mesh.py raw.ply light.ply --cell-size 0.01 --placement mean
    python tools/simplify_mesh.py raw.ply light.ply --cell-size 0.005 --tolerance 0.001 --levels 3

Both files are PLYs of vdn_train.meshio (validate_mesh writes one). --cell-size is in the file's own units; --target-faces searches
for the smallest cell size that brings the mesh under that many faces. --tolerance (with --levels) is the adaptive mode: cells grow
from --cell-size by octree merging wherever the surface stays within the tolerance; with --target-faces in its place the tolerance
is searched for. The file's normals and colours are averaged per new vertex;
averaged normals are renormalised, n / max(|n|, 1e-12). Prints the report as one JSON line."""
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
    ap.add_argument("--cell-size", type=float, default=None, metavar="H", help="edge of the (finest) clustering cells, in the file's units")
    ap.add_argument("--target-faces", type=int, default=None, metavar="N",
                    help="face budget: the smallest cell size found that meets it (adaptive mode: the smallest tolerance)")
    ap.add_argument("--tolerance", type=float, default=None, metavar="T",
                    help="adaptive mode: merge cells while the merged vertex stays within T (rms, the file's units) of the planes it replaces")
    ap.add_argument("--levels", type=int, default=None, metavar="L", help="adaptive mode: octree levels above --cell-size, 1..8 (default 3)")
    ap.add_argument("--placement", choices=("quadric", "mean"), default="quadric", help="where a cluster's vertex goes")
    ap.add_argument("--eps", type=float, default=None, metavar="E", help="regulariser of the quadric solve, relative to the trace (default: simplify_mesh's)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def main():
    ap = parser()
    a = ap.parse_args()
    if a.tolerance is not None or a.levels is not None:
        if a.cell_size is None or (a.tolerance is None) == (a.target_faces is None):
            ap.error("--tolerance / --levels need --cell-size, and exactly one of --tolerance and --target-faces")
    elif (a.cell_size is None) == (a.target_faces is None):
        ap.error("exactly one of --cell-size and --target-faces is required")
    import numpy as np
    import torch
    from vdn_train import mesh_simplify, meshio
    m = meshio.read_ply(a.mesh)
    names = [n for n in ("normals", "colors") if m[n] is not None]
    with torch.cuda.device(torch.device(a.device)):
        res = mesh_simplify.simplify_mesh(m["vertices"], m["triangles"], cell_size=a.cell_size, target_faces=a.target_faces,
                                          placement=a.placement, eps=a.eps, attributes=[m[n] for n in names], tolerance=a.tolerance,
                                          levels=a.levels)
    attrs = dict(zip(names, res["attributes"]))
    if "normals" in attrs:
        n = attrs["normals"]
        attrs["normals"] = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)).astype(n.dtype)
    meshio.write_ply(a.out, res["vertices"], res["triangles"], **attrs)
    print(json.dumps(dict(res["report"], mesh=a.mesh, out=a.out)))


if __name__ == "__main__":
    main()
