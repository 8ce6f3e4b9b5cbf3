"""How many rounds the parallel form of greedy radius thinning (vdn_hip.nn.thin_points) needs in different index
orders, counted on the CPU (numpy and scipy's cKDTree, no device):

    python tools/count_thin_rounds.py --out profiles/mesh_thin_rounds_cpu.json

For each size of --sizes, N points uniform on the unit sphere (numpy default_rng(--seed), normalised normal deviates) are thinned at
radius = sqrt(4 pi / N), the mean sample spacing, in two orders: as drawn (a random order) and "strips" - sorted into bands of
width 2 * radius along z and by longitude inside a band, the order of a raster scan. Rounds are SYNCHRONOUS here: every undecided
point looks at the states of the round before (removed if a lower-index neighbour is kept, kept if all of them are removed). The
device kernel updates in place and can only need as many rounds or fewer. The figures belong to these clouds: another seed, band
width or sampling moves them by a few rounds. Prints one JSON line."""
import argparse
import json
import math
import os


def count_rounds(p, radius):
    """-> (synchronous rounds, points kept)"""
    import numpy as np
    from scipy.spatial import cKDTree
    n = len(p)
    pairs = cKDTree(p).query_pairs(radius, output_type="ndarray")
    lo, hi = pairs.min(1), pairs.max(1)                       # lo is a lower-index neighbour of hi
    state, rounds = np.zeros(n, np.int8), 0                   # 0 undecided, 1 kept, 2 removed
    while (state == 0).any():
        kept_lower, waiting_lower = np.zeros(n, bool), np.zeros(n, bool)
        np.logical_or.at(kept_lower, hi, state[lo] == 1)
        np.logical_or.at(waiting_lower, hi, state[lo] == 0)
        undecided = state == 0
        state[undecided & kept_lower] = 2
        state[undecided & ~kept_lower & ~waiting_lower] = 1
        rounds += 1
    return rounds, int((state == 1).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 200000])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    rng = np.random.default_rng(a.seed)
    rows = []
    for n in a.sizes:
        d = rng.normal(size=(n, 3))
        p = d / np.linalg.norm(d, axis=1, keepdims=True)
        radius = math.sqrt(4.0 * math.pi / n)
        strips = p[np.lexsort((np.arctan2(p[:, 1], p[:, 0]), np.floor(p[:, 2] / (2.0 * radius))))]
        (r0, k0), (r1, k1) = count_rounds(p, radius), count_rounds(strips, radius)
        rows.append({"points": n, "radius": radius, "random_order": {"rounds": r0, "kept": k0}, "strip_order": {"rounds": r1, "kept": k1}})
    line = json.dumps({"what": "synchronous rounds of greedy radius thinning, uniform points on the unit sphere, radius = sqrt(4 pi / N)",
                       "seed": a.seed, "rows": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
