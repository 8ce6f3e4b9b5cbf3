"""Greedy radius thinning on the device (vdn_hip.nn.thin_points) on a sphere's surface samples:

    python tools/time_mesh_thin.py --out profiles/mesh_thin.json

For each size of --sizes (default 10^6 and 10^7) an icosphere is sampled by sample_surface at the spacing that gives about that many
samples, and the cloud is thinned at radius = spacing (the DTU ratio), once in the samples' own index order (triangle by triangle,
a low-discrepancy sequence inside each: it behaves like a hashed order, not like strips; tools/count_thin_rounds.py counts what a
strip order costs) and once in one fixed permutation of it (seed 0). Per arm: the number of rounds, how many points are kept, the wall time of the whole call (host clock, device synchronised: the grid's sort and tables, every round with its host read of the
counter, the scatter back - what a caller waits for) as the median of --repeats calls after one warm-up call, and from one more,
instrumented call the time of every round's launch between device events: the first round, the median of the later ones, their sum.
The sequential numpy loop of the definition runs once at --cpu-size points (default 10^5) on the same host, and the device's mask at
that size is compared with it (near-ties at the radius may legally differ; the count is reported, nothing is asserted).
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def icosphere(subdivisions):
    import numpy as np
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v).astype(np.float32), np.array(f, np.int64)


def sequential_loop(p, radius):
    """the definition (fp32 difference form, inclusive); a kept point only has to look at the points behind it"""
    import numpy as np
    r2 = np.float32(radius) * np.float32(radius)
    keep = np.ones(len(p), bool)
    for i in range(len(p)):
        if keep[i]:
            d = p[i + 1:] - p[i]
            keep[i + 1:][d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= r2] = False
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000000, 10000000])
    ap.add_argument("--cpu-size", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--subdivisions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from vdn_hip import mesh, nn
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_thin.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    v, f = icosphere(a.subdivisions)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    vv = v.astype(np.float64)
    area = float(0.5 * np.linalg.norm(np.cross(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]]), axis=1).sum())

    def cloud(n):
        spacing = math.sqrt(area / n)
        return mesh.sample_surface(tv, tf, spacing)[0], spacing

    def wall(points, radius):
        torch.cuda.synchronize()
        t = time.perf_counter()
        keep, rounds = nn.thin_points(points, radius, return_rounds=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t, keep, rounds

    def round_times(points, radius):
        """ms of every round's launch, between device events, in one instrumented call"""
        events, real = [], nn._call_sized

        def timed(name, *args):
            if name != "vdn_thin_round":
                return real(name, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            real(name, *args)
            e1.record()
            events.append((e0, e1))
        nn._call_sized = timed
        try:
            nn.thin_points(points, radius)
        finally:
            nn._call_sized = real
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in events]

    def arm(points, radius):
        wall(points, radius)                                     # warm-up: code objects, the allocator's blocks for this size
        runs = [wall(points, radius) for _ in range(a.repeats)]
        ms = round_times(points, radius)
        keep, rounds = runs[0][1], runs[0][2]
        later = ms[1:] or [0.0]
        return {"rounds": rounds, "kept": int(keep.sum()), "wall_s_median": statistics.median(r[0] for r in runs), "wall_s_all": [r[0] for r in runs],
                "first_round_ms": ms[0], "later_round_ms_median": statistics.median(later), "later_round_ms_max": max(later),
                "rounds_ms_sum": sum(ms), "wall_ms_per_round": 1e3 * statistics.median(r[0] for r in runs) / rounds}

    rows = []
    for n in a.sizes:
        points, spacing = cloud(n)
        perm = torch.from_numpy(np.random.default_rng(0).permutation(points.shape[0])).to(dev)
        row = {"samples": int(points.shape[0]), "spacing": spacing, "radius": spacing, "index_order": arm(points, spacing),
               "permuted": arm(points[perm].contiguous(), spacing)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del points, perm
        torch.cuda.empty_cache()
    cpu = None
    if a.cpu_size > 0:
        points, spacing = cloud(a.cpu_size)
        host = points.cpu().numpy()
        t = time.perf_counter()
        want = sequential_loop(host, spacing)
        cpu_s = time.perf_counter() - t
        dt, keep, rounds = wall(points, spacing)
        dt, keep, rounds = wall(points, spacing)                 # (the second call: warmed)
        cpu = {"samples": len(host), "radius": spacing, "numpy_loop_s": cpu_s, "device_wall_s": dt, "device_rounds": rounds,
               "kept_numpy": int(want.sum()), "kept_device": int(keep.sum()), "masks_differ_at": int((keep.cpu().numpy() != want).sum())}
    out = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "timer": "wall: host clock around thin_points, device synchronised, median of %d calls after one warm-up; rounds: device events "
                    "around each vdn_thin_round launch in one further call" % a.repeats,
           "scene": "icosphere(%d) of radius 1, sample_surface at the spacing for the size, radius = spacing; permutation: numpy default_rng(0)" % a.subdivisions,
           "rows": rows, "sequential_numpy_loop": cpu}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
