"""Mesh simplification on the device (vdn_hip.mesh.simplify_mesh) on an extracted synthetic surface:

    python tools/time_mesh_simplify.py --out profiles/mesh_simplify.json

The surface is vdn_hip.mesh.marching_cubes of a rippled sphere on a --resolution^3 lattice (default 512: about 1.6 million
triangles), in lattice-index coordinates, cast to fp32. For each cell size of --cell-sizes (default 2 and 4 lattice spacings): the
wall time of the whole call (host clock, device synchronised: every launch, every torch sort / unique / scan between them, the three
host reads - what a caller waits for) as the median of --repeats calls after one warm-up call, for quadric and for mean placement and
for the count-only pass a face budget is searched with; and from one more, instrumented call of the quadric arm the device time of
every kernel launch and of every torch.sort / torch.unique call between device events, with the sorts' share of the whole.
--adaptive adds one leg on the same surface: the adaptive call (--adaptive-cell-size, --levels, --tolerance) against
the uniform call at that cell size, its parts as calls of their own - the level-0 stages (cluster_quadrics), the whole tree
(cluster_octree: the merges are the difference), select and assign (select_octree), one count pass (count_octree_faces), the call
on a built tree (select, records, emit) - the instrumented stages of one adaptive call, and one target_faces search at half the
uniform call's faces (vdn_train.mesh_simplify):

    python tools/time_mesh_simplify.py --cell-sizes --adaptive --out profiles/mesh_simplify_adaptive.json

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--cell-sizes", type=float, nargs="*", default=[2.0, 4.0], help="in lattice spacings")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adaptive", action="store_true", help="add the adaptive leg")
    ap.add_argument("--adaptive-cell-size", type=float, default=1.0, help="the adaptive leg's finest cell, in lattice spacings")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=0.05, help="in lattice spacings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vdn_hip import mesh
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_simplify.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    R = a.resolution
    g = torch.linspace(-1.0, 1.0, R, device=dev)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    u = torch.sqrt(x * x + y * y + z * z) - 0.7 - 0.05 * torch.sin(9.0 * x) * torch.sin(7.0 * y) * torch.sin(8.0 * z)
    del x, y, z
    v, t = mesh.marching_cubes(u.contiguous(), 0.0)
    del u
    v = v.float().contiguous()
    torch.cuda.empty_cache()

    def wall(fn):
        torch.cuda.synchronize()
        s = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - s, out

    def median_wall(fn):
        wall(fn)                                             # warm-up: code objects, the allocator's blocks for this size
        runs = [wall(fn)[0] for _ in range(a.repeats)]
        return {"wall_ms_median": 1e3 * statistics.median(runs), "wall_ms_all": [1e3 * r for r in runs]}

    def stages(fn):
        """ms of every kernel launch and of every torch.sort / torch.unique call, between device events, in one instrumented call"""
        events, real_call, real_sort, real_unique = [], mesh._call_sized, torch.sort, torch.unique

        def timed(label, real):
            def run(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = real(*args, **kw)
                e1.record()
                events.append((label if label else args[0], e0, e1))
                return out
            return run
        mesh._call_sized, torch.sort, torch.unique = timed(None, real_call), timed("torch.sort", real_sort), timed("torch.unique", real_unique)
        try:
            total, _ = wall(fn)
        finally:
            mesh._call_sized, torch.sort, torch.unique = real_call, real_sort, real_unique
        torch.cuda.synchronize()
        ms = {}
        for label, e0, e1 in events:
            ms[label] = ms.get(label, 0.0) + e0.elapsed_time(e1)
        sorts = ms.get("torch.sort", 0.0) + ms.get("torch.unique", 0.0)
        return {"stage_ms": ms, "instrumented_wall_ms": 1e3 * total, "kernels_ms": sum(x for k, x in ms.items() if k.startswith("vdn_")),
                "sort_and_unique_ms": sorts, "sort_and_unique_share_of_wall": sorts / (1e3 * total)}

    rows = []
    for h in a.cell_sizes:
        res = mesh.simplify_mesh(v, t, h)
        row = {"cell_size": h, "report": res["report"],
               "quadric": median_wall(lambda: mesh.simplify_mesh(v, t, h)),
               "mean": median_wall(lambda: mesh.simplify_mesh(v, t, h, placement="mean")),
               "count_only": median_wall(lambda: mesh.count_simplified_faces(v, t, h)),
               "quadric_stages": stages(lambda: mesh.simplify_mesh(v, t, h))}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del res
    adaptive = None
    if a.adaptive:
        from vdn_train import mesh_simplify
        h0, L, tol = a.adaptive_cell_size, a.levels, a.tolerance
        kw = {"tolerance": tol, "levels": L}
        res, uni = mesh.simplify_mesh(v, t, h0, **kw), mesh.simplify_mesh(v, t, h0)
        tree = mesh.cluster_octree(v, t, h0, L)
        budget = uni["report"]["faces_out"] // 2
        adaptive = {"cell_size": h0, "levels": L, "tolerance": tol, "report": res["report"], "uniform_report": uni["report"],
                    "nodes_in_tree_per_level": [int(x["cell"].shape[0]) for x in tree["levels"]],
                    "adaptive": median_wall(lambda: mesh.simplify_mesh(v, t, h0, **kw)),
                    "uniform_at_cell_size": median_wall(lambda: mesh.simplify_mesh(v, t, h0)),
                    "level0_stages": median_wall(lambda: mesh.cluster_quadrics(v, t, h0)),
                    "tree": median_wall(lambda: mesh.cluster_octree(v, t, h0, L)),
                    "select_assign": median_wall(lambda: mesh.select_octree(tree, tol)),
                    "count_pass": median_wall(lambda: mesh.count_octree_faces(tree, tol)),
                    "emit_on_built_tree": median_wall(lambda: mesh.simplify_mesh(v, t, h0, tree=tree, **kw)),
                    "adaptive_stages": stages(lambda: mesh.simplify_mesh(v, t, h0, **kw))}
        del res, uni
        search_s, found = wall(lambda: mesh_simplify.simplify_mesh(v, t, cell_size=h0, levels=L, target_faces=budget))
        adaptive["target_search"] = {"target_faces": budget, "wall_ms_one_call": 1e3 * search_s, "count_passes": len(found["report"]["tried"]),
                                     "tolerance_found": found["report"]["tolerance"], "faces_out": found["report"]["faces_out"]}
        print(json.dumps(adaptive), file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "timer": "wall: host clock around the call, device synchronised, median of %d calls after one warm-up; stages: device events around "
                    "each launch and each torch.sort / torch.unique in one further call (torch.unique sorts inside)" % a.repeats,
           "scene": "marching_cubes of a rippled sphere on a %d^3 lattice, lattice-index coordinates, fp32" % R,
           "vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "rows": rows}
    if adaptive is not None:
        out["adaptive"] = adaptive
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
