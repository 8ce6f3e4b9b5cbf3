"""Device time of the mesh-cleaning primitives on extractions of the synthetic scene:

    python tools/time_mesh_clean.py --resolutions 256 512 --out profiles/mesh_clean_timing.json

connected_components, component_table and filter_mesh (keeping the largest component) on the marching-cubes mesh of the
`synth` SDF network at each lattice resolution: HIP events around each call, warm, the median of --repeats runs. The calls
include their host reads (the error flag, the output sizes), as a user of vdn_hip.mesh sees them."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, repeats):
    import torch
    fn()                                                    # warm
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vdn_hip import mesh
    from vdn_train import factory, mesh_clean, synth
    dev = torch.device("cuda:0")
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0, variance=0.4), precision="bf16")
    rows = []
    for res in a.resolutions:
        lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
        v, t = rend.extract_geometry(lo, hi, resolution=res, threshold=0.0)
        v, t = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
        V, F = v.shape[0], t.shape[0]
        labels, ms_cc = timed(lambda: mesh.connected_components(t, V), a.repeats)
        table, ms_table = timed(lambda: mesh.component_table(v, t, labels), a.repeats)
        keep = mesh_clean.select_components(table)[table["face_component"]]
        out, ms_filter = timed(lambda: mesh.filter_mesh(v, t, keep_faces=keep), a.repeats)
        rows.append({"resolution": res, "vertices": V, "faces": F, "components": int(table["root"].numel()), "faces_kept": int(out[1].shape[0]),
                     "connected_components_ms": ms_cc, "component_table_ms": ms_table, "filter_mesh_ms": ms_filter,
                     "total_ms": ms_cc + ms_table + ms_filter})
        print(json.dumps(rows[-1]), flush=True)
        del v, t, labels, table, keep, out
    res = {"device": torch.cuda.get_device_name(0), "timer": "HIP events, warm, median of %d" % a.repeats, "scene": "synth (seed 0, variance 0.4), bf16",
           "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
