"""Mesh alignment: bring a reconstruction into the frame of a scanned cloud before it is evaluated against it (INTEGRATION.md
"Mesh alignment"). A run that learns its camera poses reconstructs the scene a similarity transform away from the
scan's frame; even with fixed poses a small misregistration remains, and a Chamfer distance at DTU thresholds sees it.

    sim3 = align_cameras(current_poses(pose_net), c2w_ref)                  # Umeyama on the camera centres (host, float64)
    errs = pose_errors(c2w_est, c2w_ref, sim3)                              # rotation / position error after alignment
    res  = align_mesh(vertices, triangles, gt_points, spacing, max_dist, init=sim3)   # trimmed ICP on the device, from sim3

A transform is (s, R, t): x -> s R x + t, R [3,3] a proper rotation, float64 numpy. ICP runs ONE way, from the mesh's samples to
the scan: its accuracy on real data is bounded by the sample spacing (the scan's and the mesh's), and geometry the scan lacks
(the unobserved back of an object, a closed bottom) pulls the fit towards it unless max_dist / trim leave it out. No
point-to-plane or symmetric variant, no initialisation-free registration: start from the cameras."""
import math
import os

import numpy as np
import torch


def _poses(x, what):
    x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] not in (3, 4) or x.shape[2] != 4:
        raise ValueError("%s must be [N,4,4] (or [N,3,4]) camera-to-world matrices" % what)
    return x


def _sim3(sim3):
    s, R, t = sim3
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,) or not (math.isfinite(float(s)) and np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("a transform is (s, R [3,3], t [3]), all finite")
    return float(s), R, t


def umeyama(p, q, scale=True):
    """p, q [N,3] -> (s, R, t) minimising sum |s R p + t - q|^2 (Umeyama 1991), float64 on the host; s = 1 with scale=False. The
    reflection guard keeps det R = +1. ValueError for N < 3 or for p on a line (the second singular value of its covariance
    <= 1e-12 of the first)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if p.shape != q.shape or p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("the two point sets must both be [N,3], got %r and %r" % (p.shape, q.shape))
    n = p.shape[0]
    if n < 3:
        raise ValueError("a similarity needs at least 3 points, got %d" % n)
    mp, mq = p.mean(0), q.mean(0)
    dp, dq = p - mp, q - mq
    sv = np.linalg.svd(dp.T @ dp / n, compute_uv=False)
    if not (sv[0] > 0.0 and sv[1] > 1e-12 * sv[0]):
        raise ValueError("the points are collinear (or coincide): no rotation is determined")
    U, D, Vt = np.linalg.svd(dq.T @ dp / n)
    if not D[1] > 1e-12 * D[0]:
        raise ValueError("the correspondences are degenerate: no rotation is determined")
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0])
    R = (U * S) @ Vt
    s = float((D * S).sum() / (dp * dp).sum() * n) if scale else 1.0
    return s, R, mq - s * (R @ mp)


def align_cameras(c2w_est, c2w_ref, scale=True):
    """(s, R, t) that maps the estimated cameras' centres onto the reference's: umeyama(c_est, c_ref). c2w_* [N,4,4], tensors or
    arrays. ValueError for N < 3, collinear centres or a shape mismatch."""
    a, b = _poses(c2w_est, "c2w_est"), _poses(c2w_ref, "c2w_ref")
    if a.shape[0] != b.shape[0]:
        raise ValueError("%d estimated cameras against %d reference cameras" % (a.shape[0], b.shape[0]))
    return umeyama(a[:, :3, 3], b[:, :3, 3], scale=scale)


def pose_errors(c2w_est, c2w_ref, sim3):
    """The cameras' errors after the alignment sim3 = (s, R, t), float64 on the host -> dict:
      rotation_deg [N]   the angle of D = R_ref^T R R_est: arccos(c), c = (trace D - 1) / 2 clamped to [-1, 1] - taken as
                         atan2(|a|, c) with a = (D32 - D23, D13 - D31, D21 - D12) / 2, the same angle, which keeps its digits
                         near 0 where arccos loses half of them (an exact alignment gives 1e-14 degrees, not 1e-6)
      position [N]       |s R c_est + t - c_ref|
      rotation_deg_mean / _median / _max, position_mean / _median / _max, position_rmse (the absolute trajectory error)"""
    a, b = _poses(c2w_est, "c2w_est"), _poses(c2w_ref, "c2w_ref")
    if a.shape[0] != b.shape[0] or a.shape[0] == 0:
        raise ValueError("%d estimated cameras against %d reference cameras" % (a.shape[0], b.shape[0]))
    s, R, t = _sim3(sim3)
    rel = np.einsum("nji,jk,nkl->nil", b[:, :3, :3], R, a[:, :3, :3])
    cos = np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    axial = 0.5 * np.stack([rel[:, 2, 1] - rel[:, 1, 2], rel[:, 0, 2] - rel[:, 2, 0], rel[:, 1, 0] - rel[:, 0, 1]], 1)
    rot = np.degrees(np.arctan2(np.linalg.norm(axial, axis=1), cos))
    pos = np.linalg.norm(s * a[:, :3, 3] @ R.T + t - b[:, :3, 3], axis=1)
    out = {"rotation_deg": rot, "position": pos, "position_rmse": float(np.sqrt((pos * pos).mean()))}
    for k, v in (("rotation_deg", rot), ("position", pos)):
        out[k + "_mean"], out[k + "_median"], out[k + "_max"] = float(v.mean()), float(np.median(v)), float(v.max())
    return out


def current_poses(pose_net):
    """[N,4,4] tensor: pose_net(i) of every camera of a dpt_models.poses.LearnPose (or a LearnableRays, or a DataParallel
    wrapper of either), detached, on the module's device."""
    pose_net = getattr(pose_net, "pose_net", pose_net)          # (LearnableRays)
    pose_net = getattr(pose_net, "module", pose_net)
    was_training = pose_net.training
    pose_net.eval()
    try:
        with torch.no_grad():
            return torch.stack([pose_net(i) for i in range(pose_net.num_cams)]).detach()
    finally:
        pose_net.train(was_training)


def store_current_pose(pose_net, base_exp_dir, iter_step):
    """The reference's store_current_pose: <base_exp_dir>/cam_poses/pose_{iter_step:0>6d}.npy with the [N,4,4] fp32 array of
    current_poses. -> the path."""
    path = os.path.join(base_exp_dir, "cam_poses", "pose_{:0>6d}.npy".format(int(iter_step)))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, current_poses(pose_net).cpu().numpy())
    return path


def apply_sim3(vertices, sim3):
    """vertices [V,3] tensor -> s R v + t in float64, rounded to fp32, on the vertices' device."""
    s, R, t = _sim3(sim3)
    v = vertices.detach().double()
    return (v @ torch.from_numpy(s * R.T).to(v.device) + torch.from_numpy(t).to(v.device)).float()


def align_mesh(vertices, triangles, gt_points, spacing, max_dist, init=None, scale=False, thin=None, **icp_options):
    """Registers a mesh to a scanned cloud: area-weighted samples of the surface (sample_surface at `spacing`; triangles None:
    the vertices themselves), optionally thinned to pairwise more than `thin` apart (thin_points), then vdn_hip.nn.icp from the
    samples to gt_points starting at init = (s, R, t) (typically align_cameras(...); None: the identity) with matches up to
    max_dist. icp_options: max_rounds, tol, trim. gt_points may be a vdn_hip.nn.PointGrid built before.
    -> icp's dict plus n_samples and `vertices`: the input's vertices through the result, float64 rounded to fp32."""
    from vdn_hip import mesh as hmesh, nn
    if not (torch.is_tensor(vertices) and vertices.is_cuda and vertices.dim() == 2 and vertices.shape[1] == 3):
        raise ValueError("vertices must be a [V,3] CUDA tensor")
    if not (float(spacing) > 0.0 and math.isfinite(float(spacing))):
        raise ValueError("spacing must be positive and finite, got %r" % (spacing,))
    unknown = set(icp_options) - {"max_rounds", "tol", "trim"}
    if unknown:
        raise TypeError("align_mesh: unknown options %r" % sorted(unknown))
    samples = vertices.detach().float().contiguous() if triangles is None else hmesh.sample_surface(vertices, triangles, spacing)[0]
    if thin is not None:
        samples = samples[nn.thin_points(samples, thin)]
    if samples.shape[0] < 3:
        raise ValueError("the mesh gives %d samples at spacing %r" % (samples.shape[0], spacing))
    res = nn.icp(samples, gt_points, init=init, max_dist=max_dist, scale=scale, **icp_options)
    res["n_samples"] = int(samples.shape[0])
    res["vertices"] = apply_sim3(vertices, (res["s"], res["R"], res["t"]))
    return res


def summary(res):
    """The plain-JSON part of an align_mesh / icp result: the transform, the rounds, the last round's n_pairs and rms."""
    return {"s": float(res["s"]), "R": np.asarray(res["R"]).tolist(), "t": np.asarray(res["t"]).tolist(),
            "matrix": np.asarray(res["matrix"]).tolist(), "rounds": int(res["rounds"]), "converged": bool(res["converged"]),
            "n_pairs": int(res["n_pairs"][-1]), "rms": float(res["rms"][-1])}


# ---- camera files (tools/align_mesh.py) -------------------------------------------------------------------------------------------
def load_estimated_poses(path):
    """[N,4,4] float64 from a pose_*.npy of store_current_pose, or from a pose checkpoint (pnf_*.pth: its pose_param_net)."""
    if str(path).endswith(".npy"):
        return _poses(np.load(path), path)
    from dpt_models.poses import LearnPose
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("pose_param_net", sd)
    net = LearnPose(sd["r"].shape[0], False, False, init_c2w=sd.get("init_c2w"))
    net.load_state_dict(sd)
    return _poses(current_poses(net), path)


def load_reference_poses(path):
    """cameras_sphere.npz -> (c2w [N,4,4] float64 in the world frame, from world_mat_<i> alone, in the order of the names' numbers;
    scale_mat_0 [4,4]: the object frame's placement in the world)."""
    from .dataset import load_K_Rt_from_P
    cams = np.load(path)
    names = sorted((k[len("world_mat_"):] for k in cams.files if k.startswith("world_mat_") and not k.startswith("world_mat_inv")),
                   key=lambda n: (len(n), n))
    if not names:
        raise ValueError("%s has no world_mat_<name>" % path)
    c2w = np.stack([load_K_Rt_from_P(cams["world_mat_" + n].astype(np.float64)[:3, :4])[1].astype(np.float64) for n in names])
    key = "scale_mat_" + names[0]
    return c2w, (cams[key].astype(np.float64) if key in cams.files else np.eye(4))


def poses_to_world(c2w, scale_mat):
    """Camera-to-world matrices of the normalised object frame -> the world frame: centres through scale_mat, rotations kept."""
    c2w = _poses(c2w, "c2w").copy()
    c2w[:, :3, 3] = c2w[:, :3, 3] @ scale_mat[:3, :3].T + scale_mat[:3, 3]
    return c2w
