"""One ICP round on the device, fused (vdn_icp_round) against the same round composed from the launches the tree had
before it, and a whole vdn_hip.nn.icp call:

    python tools/time_mesh_align.py --out profiles/mesh_align.json

The scene is an icosphere pushed onto a lobed ellipsoid (no symmetry a registration could slide along). The source is about
--samples (default 10^6) surface samples of it (sample_surface), moved by a small rigid motion (--degrees about (1, 2, 3), --shift
along each axis); the target clouds are samples of the same surface at the spacings that give about each of --clouds points
(default 10^6 and 10^7). Matches are searched up to --max-dist. Per cloud:
  fused      IcpRound(M, max_dist) and the read of the 19 doubles: two launches, one host read. The visiting order is made once
             per icp call, outside the round: its time is reported as order_s.
  composed   the round from torch and PointGrid.query, written here: y = fp32(M p) by a float64 torch matmul, PointGrid.query(y,
             max_dist) (bin, two sorts, vdn_nn_query writing dist and idx), the gather of the matches, the mask, the 19 float64 sums
             by torch reductions (the nine of q p^T as one broadcast product and sum), their read. Its sums are compared with the fused round's (they agree to rounding).
  icp        a whole nn.icp call from the identity (the grid built outside), its rounds, the time per round.
Times are host-clock seconds with the device synchronised, the median of --repeats calls after one warm-up call. Prints one JSON
line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--clouds", type=int, nargs="*", default=[1000000, 10000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subdivisions", type=int, default=5)
    ap.add_argument("--degrees", type=float, default=0.5)
    ap.add_argument("--shift", type=float, default=0.003)
    ap.add_argument("--max-dist", type=float, default=0.03)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-5, help="icp's stopping tolerance (two samplings of one surface keep jittering below it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from time_mesh_thin import icosphere
    from vdn_hip import mesh, nn
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_align.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    v, f = icosphere(a.subdivisions)
    d = v.astype(np.float64)
    r = 1.0 + 0.3 * np.sin(3.0 * d[:, 0] + 1.0) + 0.25 * np.cos(4.0 * d[:, 1] * d[:, 2] + 0.5) + 0.2 * d[:, 2]
    v = (d * r[:, None] * [1.0, 0.8, 0.6]).astype(np.float32)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    vv = v.astype(np.float64)
    area = float(0.5 * np.linalg.norm(np.cross(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]]), axis=1).sum())
    cloud = lambda n: mesh.sample_surface(tv, tf, math.sqrt(area / n))[0]

    ax = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    th = math.radians(a.degrees)
    R = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    src = (cloud(a.samples).double() @ torch.from_numpy(R.T).to(dev) + a.shift).float().contiguous()
    M = nn.sim3_matrix(1.0, np.eye(3), np.zeros(3))

    def timed(fn):
        fn()                                                      # warm-up: code objects, the allocator's blocks for this size
        out = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t)
        return statistics.median(out), out, r

    def composed(grid):
        Mt = torch.from_numpy(M).to(dev)
        y = (src.double() @ Mt[:, :3].T + Mt[:, 3]).float()
        dist, idx = grid.query(y, a.max_dist)
        hit = idx >= 0
        p, q, yy = src[hit].double(), grid.ref[idx[hit]].double(), y[hit].double()
        e = yy - q
        sums = torch.cat([hit.sum().double().reshape(1), p.sum(0), q.sum(0), (p * p).sum().reshape(1), (q * q).sum().reshape(1),
                          (q[:, :, None] * p[:, None, :]).sum(0).reshape(-1), (e * e).sum().reshape(1)])
        return sums.cpu().numpy()

    rows = []
    for n in a.clouds:
        ref = cloud(n)
        grid = nn.PointGrid(ref)
        t_order, _, order = timed(lambda: nn.query_order(grid, src))
        op = nn.IcpRound(src, grid, order=order)
        t_fused, all_fused, x = timed(lambda: op(M, a.max_dist).cpu().numpy())
        t_comp, all_comp, xc = timed(lambda: composed(grid))
        t_icp, all_icp, res = timed(lambda: nn.icp(src, grid, max_dist=a.max_dist, max_rounds=a.max_rounds, tol=a.tol))
        row = {"samples": int(src.shape[0]), "cloud": int(ref.shape[0]), "cells": grid.n_cells, "pairs": int(x[0]),
               "fused_round_s": t_fused, "fused_round_s_all": all_fused, "composed_round_s": t_comp, "composed_round_s_all": all_comp,
               "composed_over_fused": t_comp / t_fused, "order_s": t_order,
               "sums_max_relative_difference": float(np.max(np.abs(x - xc) / np.maximum(np.abs(x), 1e-300))),
               "icp_s": t_icp, "icp_s_all": all_icp, "icp_rounds": res["rounds"], "icp_converged": res["converged"],
               "icp_s_per_round": t_icp / res["rounds"], "icp_rms_first": res["rms"][0], "icp_rms_last": res["rms"][-1]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del ref, grid, op, order
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "timer": "host clock, device synchronised, median of %d calls after one warm-up call" % a.repeats,
           "scene": "icosphere(%d) pushed onto r(d) = 1 + 0.3 sin(3 dx + 1) + 0.25 cos(4 dy dz + 0.5) + 0.2 dz, axes scaled (1, 0.8, 0.6), sampled by sample_surface; source moved by %g degrees about (1, 2, 3) and %g along each axis; "
                    "max_dist %g; round timed at the identity; icp with tol %g, at most %d rounds" % (a.subdivisions, a.degrees, a.shift, a.max_dist, a.tol, a.max_rounds),
           "rows": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
