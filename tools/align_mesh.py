"""Register a mesh file to a scanned point cloud on the device (vdn_train/mesh_align.py; INTEGRATION.md "Mesh alignment"):

    python tools/align_mesh.py meshes/00300000.ply scan.ply --spacing 0.2 --max-dist 5 --trim 0.9 \\
        --cameras-est cam_poses/pose_300000.npy --cameras-ref cameras_sphere.npz --out aligned.ply

The mesh is a PLY of vdn_train.meshio.write_ply, the cloud any binary little-endian PLY whose first element is `vertex` with x, y,
z. With both camera files the start is the similarity that maps the estimated camera centres onto the reference's (Umeyama;
--scale: with its scale, otherwise rigid) and the pose errors after that alignment are reported; without them ICP starts from the
identity. --cameras-est is a pose_*.npy of store_current_pose or a pose checkpoint (pnf_*.pth); its cameras live in the normalised
object frame and are brought to the world frame by the reference file's scale_mat (--est-frame world: they already are there, as
a mesh of validate_mesh(world_space=True) is). --cameras-ref is a cameras_sphere.npz (world_mat_<i>, scale_mat_<i>).
ICP runs one way, mesh samples -> scan, point to point: keep --max-dist (and --trim) tight enough to leave out what the scan lacks.
Prints one JSON line: the transform, the rounds, and the pose errors when cameras are given."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def add_align_arguments(ap):
    """the options tools/eval_mesh.py --align shares"""
    ap.add_argument("--scale", action="store_true", help="estimate a similarity (with scale) instead of a rigid motion")
    ap.add_argument("--trim", type=float, default=None, metavar="F", help="keep the closest share F of each round's matches")
    ap.add_argument("--max-rounds", type=int, default=50)
    ap.add_argument("--tol", type=float, default=1e-7, help="stop when the source's box moves by less than this share of its diagonal")
    ap.add_argument("--cameras-est", default=None, metavar="FILE", help="pose_*.npy or pnf_*.pth: the estimated cameras")
    ap.add_argument("--cameras-ref", default=None, metavar="FILE", help="cameras_sphere.npz: the reference cameras")
    ap.add_argument("--est-frame", choices=("object", "world"), default="object", help="the frame of the estimated cameras")


def camera_start(a):
    """-> (init or None, pose errors or None) from --cameras-est / --cameras-ref"""
    from vdn_train import mesh_align
    if (a.cameras_est is None) != (a.cameras_ref is None):
        raise SystemExit("--cameras-est and --cameras-ref go together")
    if a.cameras_est is None:
        return None, None
    est = mesh_align.load_estimated_poses(a.cameras_est)
    ref, scale_mat = mesh_align.load_reference_poses(a.cameras_ref)
    if a.est_frame == "object":
        est = mesh_align.poses_to_world(est, scale_mat)
    init = mesh_align.align_cameras(est, ref, scale=a.scale)
    return init, (est, ref)


def pose_report(cams, sim3):
    from vdn_train import mesh_align
    e = mesh_align.pose_errors(cams[0], cams[1], sim3)
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in e.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("scan")
    ap.add_argument("--spacing", type=float, required=True, help="one mesh sample per spacing^2 of area")
    ap.add_argument("--max-dist", type=float, required=True, help="matches beyond it are left out")
    ap.add_argument("--thin", type=float, default=None, metavar="R", help="thin the mesh samples: no two kept samples within R")
    add_align_arguments(ap)
    ap.add_argument("--out", default=None, metavar="PLY", help="write the aligned mesh here")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    import numpy as np
    import torch
    from vdn_train import mesh_align, meshio
    init, cams = camera_start(a)
    m = meshio.read_ply(a.mesh)
    dev = torch.device(a.device)
    tv = torch.from_numpy(np.ascontiguousarray(m["vertices"])).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(m["triangles"])).to(dev)
    gt = torch.from_numpy(np.ascontiguousarray(meshio.read_points_ply(a.scan), dtype=np.float32)).to(dev)
    res = mesh_align.align_mesh(tv, tf, gt, a.spacing, a.max_dist, init=init, scale=a.scale, thin=a.thin, max_rounds=a.max_rounds,
                                tol=a.tol, trim=a.trim)
    out = dict(mesh_align.summary(res), mesh=a.mesh, scan=a.scan, spacing=a.spacing, max_dist=a.max_dist, n_samples=res["n_samples"],
               n_pairs_per_round=res["n_pairs"], rms_per_round=res["rms"], threshold_per_round=res["threshold"])
    if cams is not None:
        out["cameras"] = {"start": {"s": init[0], "R": init[1].tolist(), "t": init[2].tolist()},
                          "errors_at_start": pose_report(cams, init), "errors_after_icp": pose_report(cams, (res["s"], res["R"], res["t"]))}
    if a.out:
        meshio.write_ply(a.out, res["vertices"].cpu().numpy(), m["triangles"], normals=None, colors=m.get("colors"))
        out["out"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
