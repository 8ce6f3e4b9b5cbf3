"""Timing of the grid nearest-neighbour path (vdn_hip.nn, DESIGN.md "Mesh evaluation"): points on two concentric spheres
(queries on radius 0.5, reference on radius 0.52 - a mesh's samples against a scanned cloud), the grid path end to end (binning,
sorts, cell table, query; HIP events, median of --reps after --warmup) at each size of --sizes, the query alone at a sweep of cell
sizes (factor x L_max / sqrt(R)), the occupied cells' occupancy histogram and the mean ring count. The baseline is NOT the code
under test: chunked torch.cdist(...).min(1) in the same process on the first size, whose distances the grid's must match.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def sphere(n, radius, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (radius * d / d.norm(dim=1, keepdim=True)).float().to(dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def cdist_min(q, ref, chunk, mode="use_mm_for_euclid_dist_if_necessary"):
    """torch.cdist's default mode takes the matrix-product form at these sizes (fast, cancels); the other is the difference form"""
    out = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    for s in range(0, q.shape[0], chunk):
        out[s:s + chunk] = torch.cdist(q[s:s + chunk], ref, compute_mode=mode).min(1).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 18, 1 << 21])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--factors", type=float, nargs="+", default=[1.0, 1.5, 2.0, math.sqrt(8.0), 4.0, 6.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vdn_hip import nn
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "default_cell_factor": nn.DEFAULT_CELL_FACTOR, "sizes": []}
    for n_i, n in enumerate(a.sizes):
        q, ref = sphere(n, 0.5, 1, dev), sphere(n, 0.52, 2, dev)
        end_to_end = lambda: nn.PointGrid(ref).query(q)
        ms = [timed(end_to_end)[0] for _ in range(a.warmup + a.reps)][a.warmup:]
        grid = nn.PointGrid(ref)
        build = [timed(lambda: nn.PointGrid(ref))[0] for _ in range(a.reps)]
        dist, idx, rings = grid.query(q, return_rings=True)
        occ = grid.cell_count[grid.cell_count > 0]
        hist = torch.bincount(occ.clamp(max=32), minlength=33).tolist()
        entry = {"Q": n, "R": n, "grid_end_to_end": stats(ms), "grid_build": stats(build), "cell_size": grid.h, "dims": grid.dims,
                 "occupied_cells": int(occ.numel()), "mean_points_per_occupied_cell": float(occ.double().mean()),
                 "occupancy_histogram_1_to_32plus": hist[1:], "mean_rings": float(rings.double().mean()), "max_rings": int(rings.max()),
                 "mean_dist": float(dist.double().mean()), "query_by_cell_factor": {}}
        for f in a.factors:
            gf = nn.PointGrid(ref, cell_size=f * 1.04 / math.sqrt(n))
            t = [timed(lambda: gf.query(q))[0] for _ in range(a.warmup + a.reps)][a.warmup:]
            d2, i2 = gf.query(q)
            entry["query_by_cell_factor"]["%.3f" % f] = dict(stats(t), equal_to_default=bool(torch.equal(d2, dist) and torch.equal(i2, idx)))
        if n_i == 0:
            base = [timed(lambda: cdist_min(q, ref, a.chunk))[0] for _ in range(1 + a.baseline_reps)][1:]
            exact = "donot_use_mm_for_euclid_dist"
            base_exact = [timed(lambda: cdist_min(q, ref, a.chunk, exact))[0] for _ in range(1 + a.baseline_reps)][1:]
            want = cdist_min(q, ref, a.chunk, exact)
            entry["cdist_baseline"] = dict(stats(base), chunk=a.chunk)
            entry["cdist_difference_form"] = stats(base_exact)
            entry["speedup_over_cdist"] = float(np.median(base) / np.median(ms))
            entry["max_rel_diff_to_cdist"] = float(((dist - want).abs() / want.clamp_min(1e-30)).max())
        res["sizes"].append(entry)
        del q, ref, grid
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
