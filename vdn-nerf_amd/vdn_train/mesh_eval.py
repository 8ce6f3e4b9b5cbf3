"""Geometry figures of an extracted surface against a ground-truth point cloud: accuracy, completeness, Chamfer distance and
F-scores - what the NeuS / VDN-NeRF family reports on DTU-style scans. All of it on the device: area-weighted surface samples
(vdn_hip.mesh.sample_surface), one uniform grid per side and one exact nearest-neighbour query in each direction (vdn_hip.nn),
reductions in float64 through torch.

Out of scope, on purpose: the DTU protocol's observation masks, its ground-plane cut and the thinning of either cloud to a fixed
density. The caller passes points that are already filtered; `spacing` sets the mesh's sampling density, nothing is thinned."""
import json
import math

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


def evaluate_mesh(vertices, triangles, gt_points, spacing, max_dist, thresholds=()):
    """vertices [V,3], triangles [F,3] (or None: `vertices` is evaluated as a bare cloud), gt_points [G,3], all CUDA tensors ->
    dict of
      n_mesh_samples, n_gt
      accuracy, n_accuracy_used          mean distance mesh sample -> ground truth over the samples within max_dist, and their number
      completeness, n_completeness_used  the same from the ground truth to the mesh samples
      chamfer                            (accuracy + completeness) / 2, the DTU "overall" figure
      precision, recall, fscore          one dict each, keyed by threshold t: the share of ALL mesh samples / of ALL ground-truth
                                         points within t, and 2 P R / (P + R) (0 where P + R = 0)
    A mean over nothing is nan. The mesh is sampled once per spacing^2 of area (sample_surface). A threshold beyond max_dist
    raises: nothing is searched further than max_dist. The DTU observation-mask, ground-plane and point-thinning steps are not
    applied - pass points that are already filtered."""
    from vdn_hip import mesh as hmesh, nn
    thresholds = _check_args(spacing, max_dist, thresholds)
    for x, what in ((vertices, "vertices"), (gt_points, "gt_points")):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.shape[1] == 3):
            raise ValueError("%s must be a [N,3] CUDA tensor" % what)
    if triangles is None:
        samples = vertices.detach().float().contiguous()
    else:
        samples = hmesh.sample_surface(vertices, triangles, spacing)[0]
    gt = gt_points.detach().float().contiguous()
    S, G = samples.shape[0], gt.shape[0]
    if S == 0 or G == 0:
        raise ValueError("nothing to compare: %d mesh samples, %d ground-truth points" % (S, G))
    d_acc = nn.PointGrid(gt).query(samples, max_dist)[0]
    d_comp = nn.PointGrid(samples).query(gt, max_dist)[0]
    acc, n_acc = _side(d_acc, max_dist)
    comp, n_comp = _side(d_comp, max_dist)
    out = {"n_mesh_samples": S, "n_gt": G, "accuracy": acc, "n_accuracy_used": n_acc, "completeness": comp,
           "n_completeness_used": n_comp, "chamfer": 0.5 * (acc + comp), "precision": {}, "recall": {}, "fscore": {}}
    for t in thresholds:
        t32 = nn._fp32_at_most(t)          # (an fp32 distance is <= t exactly when it is <= the largest fp32 below t)
        p, r = int((d_acc <= t32).sum().item()) / S, int((d_comp <= t32).sum().item()) / G
        out["precision"][t], out["recall"][t] = p, r
        out["fscore"][t] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return out


def evaluate_ply(mesh_path, gt_path, spacing, max_dist, thresholds=(), device="cuda:0"):
    """evaluate_mesh on files: a mesh written by vdn_train.meshio.write_ply (validate_mesh(world_space=True) leaves one in the
    ground truth's frame) against the vertex positions of a scanned-cloud PLY (meshio.read_points_ply)."""
    from . import meshio
    _check_args(spacing, max_dist, thresholds)
    m = meshio.read_ply(mesh_path)
    gt = meshio.read_points_ply(gt_path)
    dev = torch.device(device)
    return evaluate_mesh(torch.from_numpy(np.ascontiguousarray(m["vertices"])).to(dev), torch.from_numpy(np.ascontiguousarray(m["triangles"])).to(dev),
                         torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).to(dev), spacing, max_dist, thresholds)


def to_json(result):
    """One JSON line of an evaluate_mesh result (threshold keys as strings, nan as null)."""
    clean = lambda v: None if isinstance(v, float) and not math.isfinite(v) else v
    return json.dumps({k: ({repr(t): clean(x) for t, x in v.items()} if isinstance(v, dict) else clean(v)) for k, v in result.items()})
