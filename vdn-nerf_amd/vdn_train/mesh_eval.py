"""Geometry figures of an extracted surface against a ground-truth point cloud: accuracy, completeness, Chamfer distance and
F-scores - what the NeuS / VDN-NeRF family reports on DTU-style scans. All of it on the device: area-weighted surface samples
(vdn_hip.mesh.sample_surface), one uniform grid per side and one exact nearest-neighbour query in each direction (vdn_hip.nn),
reductions in float64 through torch.

The DTU protocol's three extra steps are optional arguments of evaluate_mesh: `thin` brings the mesh samples to a fixed density
(vdn_hip.nn.thin_points, greedy and exact), `obs_mask` leaves samples in voxels no scanner view observed out of the accuracy
(observed_mask), `plane` leaves the table the scan stands on out of the completeness (above_plane). The last two are element-wise
torch ops that run on any device. With none of them the figures are those of the plain comparison; the ground-truth cloud is never
thinned (the published scans already are)."""
import json
import math
import os

import numpy as np
import torch


def _check_args(spacing, max_dist, thresholds):
    if not (float(spacing) > 0.0 and math.isfinite(float(spacing))):
        raise ValueError("spacing must be positive and finite, got %r" % (spacing,))
    if not (float(max_dist) >= 0.0):
        raise ValueError("max_dist must be >= 0, got %r" % (max_dist,))
    thresholds = tuple(float(t) for t in thresholds)
    for t in thresholds:
        if not (t >= 0.0):
            raise ValueError("a threshold must be >= 0, got %r" % (t,))
        if t > float(max_dist):
            raise ValueError("threshold %r is beyond max_dist %r: distances are only searched up to max_dist" % (t, max_dist))
    return thresholds


def _side(dist, max_dist):
    """mean of the distances <= max_dist (nan over nothing) and how many there are; dist is fp32 with +inf beyond max_dist."""
    used = torch.isfinite(dist)
    n = int(used.sum().item())
    mean = float(dist[used].double().sum().item()) / n if n > 0 else float("nan")
    return mean, n


def observed_mask(points, obs_mask, bb, res, patch=60.0):
    """points [N,3] -> (inbound [N] bool, observed [N] bool), the DTU evaluation's two sample filters, on the points' device:
      inbound  = all(p >= bb[0] - patch) & all(p < bb[1] + 2 * patch)     (the `2 *` on the upper side only is the published DTU
                                                                           evaluation code's own; kept, so the figures compare)
      g        = rint((p - bb[0]) / res), in fp32, halves to even
      observed = inbound & all(0 <= g < obs_mask.shape) & obs_mask[gx, gy, gz]
    obs_mask: 3-D bool or uint8 indexed [x, y, z] (nonzero = some scanner view observed the voxel); bb [2,3]: the voxel grid's
    corners; res: the voxel pitch; patch: the band around the box. Arrays or tensors; the bounds are formed in fp32."""
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a float [N,3] tensor")
    dev = points.device
    p = points.detach().float()
    m = torch.as_tensor(obs_mask, device=dev)
    if m.dim() != 3 or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError("obs_mask must be a 3-D bool or uint8 array")
    bb = torch.as_tensor(bb, device=dev).float()
    if tuple(bb.shape) != (2, 3):
        raise ValueError("bb must be [2,3]")
    res, patch = float(res), float(patch)
    if not (res > 0.0 and math.isfinite(res)) or not (patch >= 0.0 and math.isfinite(patch)):
        raise ValueError("res must be positive and patch >= 0, both finite; got %r, %r" % (res, patch))
    f32 = lambda x: torch.tensor([x], dtype=torch.float32, device=dev)          # (a tensor operand: one fp32 op, no scalar shortcut)
    inbound = (p >= bb[0] - f32(patch)).all(1) & (p < bb[1] + f32(2.0) * f32(patch)).all(1)
    g = torch.round((p - bb[0]) / f32(res))
    shape = torch.tensor(list(m.shape), dtype=torch.float32, device=dev)
    inside = ((g >= 0) & (g < shape)).all(1)                    # (nan fails both)
    gi = torch.where(inside[:, None], g, torch.zeros_like(g)).long()
    observed = inbound & inside & (m[gi[:, 0], gi[:, 1], gi[:, 2]] != 0)
    return inbound, observed


def above_plane(points, plane):
    """points [N,3], plane (a, b, c, d) -> [N] bool: a x + b y + c z + d > 0, summed in float64 in that order (the DTU ground
    plane P: the scan's points on the positive side are the object, the others the table)."""
    if not (torch.is_tensor(points) and points.dim() == 2 and points.shape[1] == 3 and points.is_floating_point()):
        raise ValueError("points must be a float [N,3] tensor")
    pl = [float(x) for x in np.asarray(plane.detach().cpu() if torch.is_tensor(plane) else plane, dtype=np.float64).reshape(-1)]
    if len(pl) != 4 or not all(math.isfinite(x) for x in pl):
        raise ValueError("plane must be 4 finite numbers")
    p = points.detach().double()
    return pl[0] * p[:, 0] + pl[1] * p[:, 1] + pl[2] * p[:, 2] + pl[3] > 0


def evaluate_mesh(vertices, triangles, gt_points, spacing, max_dist, thresholds=(), thin=None, obs_mask=None, patch=60.0, plane=None,
                  align=None):
    """vertices [V,3], triangles [F,3] (or None: `vertices` is evaluated as a bare cloud), gt_points [G,3], all CUDA tensors ->
    dict of
      n_mesh_samples, n_gt
      accuracy, n_accuracy_used          mean distance mesh sample -> ground truth over the samples within max_dist, and their number
      completeness, n_completeness_used  the same from the ground truth to the mesh samples
      chamfer                            (accuracy + completeness) / 2, the DTU "overall" figure
      precision, recall, fscore          one dict each, keyed by threshold t: the share of ALL mesh samples / of ALL ground-truth
                                         points within t, and 2 P R / (P + R) (0 where P + R = 0)
    A mean over nothing is nan. The mesh is sampled once per spacing^2 of area (sample_surface). A threshold beyond max_dist
    raises: nothing is searched further than max_dist.

    The DTU protocol's steps, each optional (with none of them the dict is exactly the one above):
      thin      a radius: the mesh samples are thinned to samples[thin_points(samples, thin)] - pairwise more than `thin` apart
      obs_mask  (ObsMask, BB, Res): inbound, observed = observed_mask(samples, ObsMask, BB, Res, patch). ACCURACY runs from
                samples[observed] to all of gt_points, COMPLETENESS to samples[inbound] (not the observed ones: the protocol's)
      plane     (a, b, c, d): completeness runs from gt_points[above_plane(gt_points, plane)] only
    precision / recall are then shares of those two query sets (samples[observed], gt above the plane), max_dist stays inclusive.
    Further keys: n_thinned (samples the thinning removed), thin_rounds, n_inbound, n_observed, n_gt_above_plane; n_mesh_samples
    counts the samples after thinning. ValueError when a filter leaves a side empty.

    align (vdn_train/mesh_align.py): None, or what brings the mesh into the ground truth's frame BEFORE it is sampled - a transform
    (s, R, t) applied to the vertices, or a dict of align_mesh options (init, scale, thin, max_rounds, tol, trim, and spacing /
    max_dist where the registration's differ from the evaluation's): the mesh is registered to gt_points by ICP first. The dict
    then gains the key `align`: s, R, t, matrix, and with a registration rounds, converged and the last round's n_pairs / rms."""
    from vdn_hip import mesh as hmesh, nn
    thresholds = _check_args(spacing, max_dist, thresholds)
    for x, what in ((vertices, "vertices"), (gt_points, "gt_points")):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.shape[1] == 3):
            raise ValueError("%s must be a [N,3] CUDA tensor" % what)
    aligned = None
    if align is not None:
        from . import mesh_align
        if isinstance(align, dict):
            opts = dict(align)
            res = mesh_align.align_mesh(vertices, triangles, gt_points, opts.pop("spacing", spacing), opts.pop("max_dist", max_dist), **opts)
            vertices, aligned = res["vertices"], mesh_align.summary(res)
        else:
            vertices = mesh_align.apply_sim3(vertices, align)
            s_, R_, t_ = mesh_align._sim3(align)
            aligned = {"s": s_, "R": R_.tolist(), "t": t_.tolist(), "matrix": np.vstack([np.c_[s_ * R_, t_], [0.0, 0.0, 0.0, 1.0]]).tolist()}
    if triangles is None:
        samples = vertices.detach().float().contiguous()
    else:
        samples = hmesh.sample_surface(vertices, triangles, spacing)[0]
    gt = gt_points.detach().float().contiguous()
    S, G = samples.shape[0], gt.shape[0]
    if S == 0 or G == 0:
        raise ValueError("nothing to compare: %d mesh samples, %d ground-truth points" % (S, G))
    protocol = thin is not None or obs_mask is not None or plane is not None
    extra = {}
    acc_from, comp_to, comp_from = samples, samples, gt       # accuracy: acc_from -> gt; completeness: comp_from -> comp_to
    if protocol:
        extra = {"n_thinned": 0, "thin_rounds": 0, "n_inbound": S, "n_observed": S, "n_gt_above_plane": G}
        if thin is not None:
            keep, extra["thin_rounds"] = nn.thin_points(samples, thin, return_rounds=True)
            samples = samples[keep]
            extra["n_thinned"], S = S - samples.shape[0], samples.shape[0]
            extra["n_inbound"] = extra["n_observed"] = S
            acc_from = comp_to = samples
        if obs_mask is not None:
            if not (isinstance(obs_mask, (tuple, list)) and len(obs_mask) == 3):
                raise ValueError("obs_mask must be (ObsMask, BB, Res)")
            inbound, observed = observed_mask(samples, obs_mask[0], obs_mask[1], obs_mask[2], patch)
            acc_from, comp_to = samples[observed], samples[inbound]
            extra["n_inbound"], extra["n_observed"] = comp_to.shape[0], acc_from.shape[0]
        if plane is not None:
            comp_from = gt[above_plane(gt, plane)]
            extra["n_gt_above_plane"] = comp_from.shape[0]
        if min(acc_from.shape[0], comp_to.shape[0], comp_from.shape[0]) == 0:
            raise ValueError("a filter left a side empty: %d observed and %d inbound mesh samples, %d ground-truth points above the plane"
                             % (acc_from.shape[0], comp_to.shape[0], comp_from.shape[0]))
    d_acc = nn.PointGrid(gt).query(acc_from, max_dist)[0]
    d_comp = nn.PointGrid(comp_to).query(comp_from, max_dist)[0]
    acc, n_acc = _side(d_acc, max_dist)
    comp, n_comp = _side(d_comp, max_dist)
    out = {"n_mesh_samples": S, "n_gt": G, "accuracy": acc, "n_accuracy_used": n_acc, "completeness": comp,
           "n_completeness_used": n_comp, "chamfer": 0.5 * (acc + comp), "precision": {}, "recall": {}, "fscore": {}}
    out.update(extra)
    for t in thresholds:
        t32 = nn._fp32_at_most(t)          # (an fp32 distance is <= t exactly when it is <= the largest fp32 below t)
        p, r = int((d_acc <= t32).sum().item()) / acc_from.shape[0], int((d_comp <= t32).sum().item()) / comp_from.shape[0]
        out["precision"][t], out["recall"][t] = p, r
        out["fscore"][t] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    if aligned is not None:
        out["align"] = aligned
    return out


def evaluate_ply(mesh_path, gt_path, spacing, max_dist, thresholds=(), device="cuda:0", thin=None, obs_mask=None, patch=60.0, plane=None,
                 align=None):
    """evaluate_mesh on files: a mesh written by vdn_train.meshio.write_ply (validate_mesh(world_space=True) leaves one in the
    ground truth's frame) against the vertex positions of a scanned-cloud PLY (meshio.read_points_ply). obs_mask and plane may be
    paths of DTU auxiliary files (meshio.read_dtu_aux: ObsMask, BB and Res from the first, P from the second) or what
    evaluate_mesh takes; align is evaluate_mesh's."""
    from . import meshio
    _check_args(spacing, max_dist, thresholds)
    if isinstance(obs_mask, (str, os.PathLike)):
        aux = meshio.read_dtu_aux(obs_mask)
        if not all(k in aux for k in ("ObsMask", "BB", "Res")):
            raise ValueError("%s: needs ObsMask, BB and Res, has %r" % (obs_mask, sorted(aux)))
        obs_mask = (aux["ObsMask"], aux["BB"], aux["Res"])
    if isinstance(plane, (str, os.PathLike)):
        aux = meshio.read_dtu_aux(plane)
        if "P" not in aux:
            raise ValueError("%s: needs P, has %r" % (plane, sorted(aux)))
        plane = aux["P"]
    m = meshio.read_ply(mesh_path)
    gt = meshio.read_points_ply(gt_path)
    dev = torch.device(device)
    return evaluate_mesh(torch.from_numpy(np.ascontiguousarray(m["vertices"])).to(dev), torch.from_numpy(np.ascontiguousarray(m["triangles"])).to(dev),
                         torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).to(dev), spacing, max_dist, thresholds,
                         thin=thin, obs_mask=obs_mask, patch=patch, plane=plane, align=align)


def to_json(result):
    """One JSON line of an evaluate_mesh result (threshold keys as strings, nan as null)."""
    clean = lambda v: None if isinstance(v, float) and not math.isfinite(v) else v
    return json.dumps({k: (v if k == "align" else {repr(t): clean(x) for t, x in v.items()} if isinstance(v, dict) else clean(v))
                       for k, v in result.items()})
