"""Device time of the visibility stage of clean_mesh next to its mask-vote and component stages, on extractions of the synthetic
scene with its own cameras:

    python tools/time_mesh_visibility.py --resolutions 256 --out profiles/mesh_visibility_timing.json

The three stages as clean_mesh runs them, one after the other on what the stage before left: HIP events around each, warm, the
median of --repeats runs, host reads included. The masks are all set (the synthetic scene has none), so the mask stage only drops
what is in no image. Also reported: the grid's geometry and memory, and the ray-triangle tests per camera-vertex segment (cast
again through MeshGrid.cast for one camera, closest hit off: the any-hit walk the votes use)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cell-size", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from time_mesh_clean import timed
    from vdn_hip import mesh
    from vdn_train import factory, mesh_clean, synth
    dev = torch.device("cuda:0")
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0, variance=0.4), precision="bf16")
    K = np.linalg.inv(synth.intrinsics_inv())
    P = np.stack([K @ np.linalg.inv(c)[:3] for c in synth.make_cameras(0)])
    H, W = synth.H, synth.W_IMG
    masks = torch.ones(len(P), H, W, dtype=torch.uint8, device=dev)
    rows = []
    for res in a.resolutions:
        lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
        v, t = rend.extract_geometry(lo, hi, resolution=res, threshold=0.0)
        v, t = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
        row = {"resolution": res, "vertices": int(v.shape[0]), "faces": int(t.shape[0]), "cameras": len(P), "image": [H, W]}

        def stage_masks():
            n_img, n_msk = mesh.mask_votes(v, P, masks)
            return mesh.filter_mesh(v, t, keep_vertices=mesh_clean.vote_keep(n_img, n_msk))
        (v1, t1, _), row["mask_stage_ms"] = timed(stage_masks, a.repeats)

        def stage_components():
            table = mesh.component_table(v1, t1, mesh.connected_components(t1, v1.shape[0]))
            return mesh.filter_mesh(v1, t1, keep_faces=mesh_clean.select_components(table)[table["face_component"]])
        (v2, t2, _), row["component_stage_ms"] = timed(stage_components, a.repeats)

        grid, row["grid_build_ms"] = timed(lambda: mesh.MeshGrid(v2, t2, cell_size=a.cell_size), a.repeats)
        (n_img, n_vis), row["visibility_votes_ms"] = timed(lambda: mesh.visibility_votes(v2, t2, P, (H, W), grid=grid), a.repeats)
        (v3, t3, _), row["visibility_filter_ms"] = timed(lambda: mesh.filter_mesh(v2, t2, keep_vertices=mesh_clean.visible_keep(n_vis)), a.repeats)
        row["visibility_stage_ms"] = row["grid_build_ms"] + row["visibility_votes_ms"] + row["visibility_filter_ms"]
        c = torch.from_numpy(mesh.camera_centres(P[:1])).to(dev)
        tests = grid.cast(c.expand(v2.shape[0], 3), v2.double() - c, t_max=1.0 - 1e-4, any_hit=True,
                          skip_vertex=torch.arange(v2.shape[0], device=dev), return_tests=True)[2]
        row.update(vertices_after_components=int(v2.shape[0]), faces_after_components=int(t2.shape[0]), vertices_seen=int(v3.shape[0]),
                   faces_seen=int(t3.shape[0]), segments=int(n_img.sum().item()), cell_size=grid.h, cells=grid.dims, references=grid.n_refs,
                   grid_bytes=grid.nbytes, tests_per_segment_camera_0=float(tests.double().mean().item()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "timer": "HIP events, warm, median of %d" % a.repeats,
           "scene": "synth (seed 0, variance 0.4), bf16; its %d cameras, masks all set" % len(P), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
