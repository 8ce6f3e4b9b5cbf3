"""Dense against brick-sparse extract_geometry on the synthetic SDF network:

    python tools/time_mesh_extract.py --out profiles/mesh_extract_sparse.json

For each resolution of --both (default 256 512 1024) extract_geometry (with NeuSRenderer's query_func) runs once densely and once with `sparse`; for
each of --sparse-only (default 2048, where the dense lattice no longer fits) the sparse arm alone. Per arm: wall time (host clock
around the whole call, device synchronised, the copy of the mesh to the host included - what a caller waits for), the peak of
torch.cuda.max_memory_allocated above what was allocated before the call, the points handed to the network and the fraction of
bricks kept. Where both arms ran, whether the two array pairs are equal. One warm-up pair at the smallest resolution first; every
figure after that is ONE run.

The bound: --lipschitz, default 2 x the largest |gradient| of the network over the nodes of the --gradient-resolution lattice (what
tests/test_gpu_mesh_sparse.py does); that largest gradient is recorded, so a reader can judge the margin of the package default
(vdn_hip.mesh.SPARSE_LIPSCHITZ = 2.0, a policy). Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--both", type=int, nargs="*", default=[256, 512, 1024])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[2048])
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--lipschitz", type=float, default=None)
    ap.add_argument("--gradient-resolution", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from dpt_models.renderer import extract_geometry
    from vdn_hip import mesh
    from vdn_train import factory, synth
    dev = torch.device("cuda:0")
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0, variance=0.4), precision=a.precision)
    lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)

    # the largest |gradient| on the lattice nodes
    g1 = torch.linspace(-1.01, 1.01, a.gradient_resolution).to(dev)
    gmax = 0.0
    with torch.no_grad():
        for xs in g1.split(4):
            pts = torch.stack(torch.meshgrid(xs, g1, g1, indexing="ij"), dim=-1).reshape(-1, 3)
            gmax = max(gmax, float(rend.sdf_network.gradient(pts).reshape(-1, 3).float().norm(dim=-1).max()))
    L = a.lipschitz if a.lipschitz is not None else 2.0 * gmax
    opts = {"brick": a.brick, "lipschitz": L}

    counted = [0]

    def query(pts):
        counted[0] += pts.shape[0]
        return -rend.sdf_network.sdf(pts)                  # NeuSRenderer.extract_geometry's query_func

    def run(res, sparse):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before, counted[0] = torch.cuda.memory_allocated(), 0
        t = time.perf_counter()
        try:
            v, f = extract_geometry(lo, hi, res, 0.0, query, sparse=opts if sparse else None)
        except (mesh.SparseExtractionError, ValueError, torch.OutOfMemoryError) as e:
            return None, {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        torch.cuda.synchronize()
        row = {"wall_s": time.perf_counter() - t, "peak_bytes": torch.cuda.max_memory_allocated() - before,
               "points_evaluated": counted[0], "points_of_dense": counted[0] / float(res) ** 3, "vertices": int(v.shape[0]), "faces": int(f.shape[0])}
        if sparse:
            # points = bricks + active bricks * (B + 1)^3  (vdn_hip.mesh.marching_cubes_sparse)
            B = min(a.brick, res - 1)
            bricks = (-(-(res - 1) // B)) ** 3
            active = (counted[0] - bricks) // (B + 1) ** 3
            row.update(bricks=bricks, active_bricks=active, active_fraction=active / float(bricks))
        return (v, f), row

    if a.both or a.sparse_only:
        warm = min(a.both + a.sparse_only)
        run(warm, False), run(warm, True)
    rows = []
    for res in a.both:
        (m0, d), (m1, s) = run(res, False), run(res, True)
        row = {"resolution": res, "dense": d, "sparse": s}
        if m0 is not None and m1 is not None:
            row["equal"] = bool(np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del m0, m1
    for res in a.sparse_only:
        m1, s = run(res, True)
        del m1
        rows.append({"resolution": res, "sparse": s})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "timer": "host clock around extract_geometry, device synchronised, one run after a warm-up pair",
           "scene": "synth (seed 0, variance 0.4), %s, box [-1.01, 1.01]^3" % a.precision, "brick": a.brick, "lipschitz": L,
           "max_gradient_on_lattice": gmax, "gradient_resolution": a.gradient_resolution, "package_default_lipschitz": mesh.SPARSE_LIPSCHITZ,
           "rows": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
