"""Accuracy / completeness / Chamfer distance / F-scores of a mesh file against a ground-truth point cloud, on the device
(vdn_train/mesh_eval.py; INTEGRATION.md "Mesh evaluation"):

    python tools/eval_mesh.py meshes/00300000.ply scan.ply --spacing 0.2 --max-dist 20 --thresholds 1 2

The mesh is a PLY of vdn_train.meshio.write_ply (validate_mesh(world_space=True) writes one in the scan's frame); the cloud is any
binary little-endian PLY whose first element is `vertex` with x, y, z. The DTU protocol's steps are optional:

    ... --thin 0.2 --obs-mask ObsMask24_10.mat --plane Plane24.mat [--patch 60]

--thin R thins the mesh samples to pairwise more than R apart, --obs-mask FILE (.npz or .mat with ObsMask, BB, Res) leaves unobserved
samples out of the accuracy, --plane FILE (.npz or .mat with P) leaves the scan's table out of the completeness.

    ... --align [--scale] [--trim F] [--cameras-est pose.npy|pnf.pth --cameras-ref cameras_sphere.npz]

--align registers the mesh to the scan first (tools/align_mesh.py's options; INTEGRATION.md "Mesh alignment") and evaluates the
aligned mesh; the result gains the key `align` (the transform, the rounds, and with cameras the pose errors). Prints one JSON line."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("ground_truth")
    ap.add_argument("--spacing", type=float, required=True, help="one mesh sample per spacing^2 of area")
    ap.add_argument("--max-dist", type=float, required=True, help="distances beyond it are outliers: left out of the means")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="F-score thresholds (each <= --max-dist)")
    ap.add_argument("--thin", type=float, default=None, metavar="R", help="thin the mesh samples: no two kept samples within R")
    ap.add_argument("--obs-mask", default=None, metavar="FILE", help=".npz / .mat with ObsMask, BB, Res (the DTU observation mask)")
    ap.add_argument("--plane", default=None, metavar="FILE", help=".npz / .mat with P (the DTU ground plane)")
    ap.add_argument("--patch", type=float, default=60.0, metavar="X", help="the band around the observation mask's box")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--align", action="store_true", help="register the mesh to the scan by ICP before evaluating it")
    ap.add_argument("--align-max-dist", type=float, default=None, metavar="D", help="the registration's match distance (default: --max-dist)")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import align_mesh as align_tool
    align_tool.add_align_arguments(ap)
    a = ap.parse_args()
    from vdn_train import mesh_eval
    align, cams = None, None
    if a.align:
        init, cams = align_tool.camera_start(a)
        align = {"init": init, "scale": a.scale, "trim": a.trim, "max_rounds": a.max_rounds, "tol": a.tol, "thin": a.thin}
        if a.align_max_dist is not None:
            align["max_dist"] = a.align_max_dist
    res = mesh_eval.evaluate_ply(a.mesh, a.ground_truth, a.spacing, a.max_dist, a.thresholds, device=a.device,
                                 thin=a.thin, obs_mask=a.obs_mask, patch=a.patch, plane=a.plane, align=align)
    if cams is not None:
        import numpy as np
        al = res["align"]
        res["align"] = dict(al, pose_errors=align_tool.pose_report(cams, (al["s"], np.array(al["R"]), np.array(al["t"]))))
    print(mesh_eval.to_json(dict(res, mesh=a.mesh, ground_truth=a.ground_truth, spacing=a.spacing, max_dist=a.max_dist)))


if __name__ == "__main__":
    main()
