"""Texture baking on the device (vdn_hip.mesh.bake_texture and its parts) on the synthetic renderer's own surface:

    python tools/time_mesh_texture.py --out profiles/mesh_texture.json

The mesh is extract_geometry of the synthetic SDF network (vdn_train.synth.make_all_states(0), bf16 kernels) on a --resolution^3
lattice (default 256), simplified to about --target-faces faces (default 100 000), baked into a --texture-size^2 atlas (default
4096) with the largest patch that fits. For each entry of --project (default 0 and 2 rounds): the seconds of every stage - texel
points, each projection round split into its field evaluation (shade_points) and its Newton step, the shading pass, the gather -
on the host clock with the device synchronised around the stage, as the median of --repeats bakes after one warm-up bake; and the
median |sdf| at the texel points before and after the projection. Prints one JSON line."""
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
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target-faces", type=int, default=100000)
    ap.add_argument("--texture-size", type=int, default=4096)
    ap.add_argument("--project", type=int, nargs="*", default=[0, 2])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vdn_hip import mesh
    from vdn_train import factory, mesh_simplify, synth
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_texture.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0), precision="bf16")
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    v, t = rend.extract_geometry(lo, hi, resolution=a.resolution, threshold=0.0)
    faces_in = int(t.shape[0])
    res = mesh_simplify.simplify_mesh(v, t, target_faces=a.target_faces)
    v, t = torch.from_numpy(res["vertices"]).to(dev), torch.from_numpy(res["triangles"].astype("int64")).to(dev)
    layout = mesh.texture_layout(t.shape[0], a.texture_size)
    r = mesh.mean_edge_length(v, t)

    def bake(rounds):
        """one bake, stage by stage -> (seconds per stage, median |sdf| before, after)"""
        sec = {}

        def stage(name, fn):
            torch.cuda.synchronize()
            s = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            sec[name] = sec.get(name, 0.0) + time.perf_counter() - s
            return out
        x0, _ = stage("points", lambda: mesh.texel_points(v, t, layout))
        x, before = x0, None
        for k in range(rounds):
            sdf, g, _ = stage("project_field_%d" % k, lambda: mesh.shade_points(rend, x))
            if before is None:
                before = float(sdf.abs().median())
            x = stage("project_step_%d" % k, lambda: mesh.project_step(x, x0, sdf, g, r))
        sdf, _, col = stage("shade", lambda: mesh.shade_points(rend, x))
        stage("gather", lambda: mesh.gather_atlas(col, layout))
        after = float(sdf.abs().median())
        return sec, (after if before is None else before), after

    rows = []
    with torch.no_grad():
        for rounds in a.project:
            bake(rounds)                                         # warm-up: code objects, the allocator's blocks for this size
            runs = [bake(rounds) for _ in range(a.repeats)]
            names = list(runs[0][0])
            sec = {n: statistics.median(x[0][n] for x in runs) for n in names}
            new = sum(s for n, s in sec.items() if n in ("points", "gather") or n.startswith("project_step"))
            row = {"project": rounds, "seconds_median": sec, "seconds_all": [x[0] for x in runs], "total_seconds": sum(sec.values()),
                   "shade_seconds": sec["shade"], "new_kernels_seconds": new, "new_kernels_share_of_shade": new / sec["shade"],
                   "median_abs_sdf_before": runs[0][1], "median_abs_sdf_after": runs[0][2]}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(),
           "timer": "host clock around each stage, device synchronised before and after, median of %d bakes after one warm-up bake" % a.repeats,
           "scene": "extract_geometry of the synthetic SDF network (seed 0, bf16) on a %d^3 lattice, simplified with target_faces = %d"
                    % (a.resolution, a.target_faces),
           "faces_extracted": faces_in, "vertices": int(v.shape[0]), "faces": int(t.shape[0]), "cell_size": res["report"]["cell_size"],
           "texture_size": layout["S"], "patch": layout["n"], "texels_shaded": layout["points"], "max_offset": r, "rows": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
