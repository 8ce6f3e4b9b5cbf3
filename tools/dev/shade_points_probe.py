"""Timing of vertex shading (vdn_hip.mesh.shade_points, DESIGN.md "Meshes on disk"): the fused launch (vdn_shade_points_bf16,
csrc/k_sdf_fwd2.h MODE 4) against the separate launches (VDN_SHADE_POINTS_FUSED=0) on 2^20 points of the shell 0.3 <= |x| <= 1 in
bf16, and the two bare kernels of that arm (one SDF launch + the colour head, no layout round trip), alternating in one process,
HIP events around each call, median of --reps calls after --warmup; and the share of a resolution-512 validate_mesh call that
vertex shading takes. Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "vdn-nerf_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def shell_points(n, seed=0):
    from vdn_train import synth
    d = synth.normal(seed, "shade_points_probe/dir", (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (0.3 + 0.7 * synth.uniform(seed, "shade_points_probe/radius", (n, 1)))).astype(np.float32)


def timed(fn):
    """-> (milliseconds between two HIP events around fn(), its result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vdn_hip import mesh
    from vdn_train import factory, synth, validate
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dev = torch.device("cuda:0")
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0, variance=0.4), precision="bf16")
    x = torch.from_numpy(shell_points(a.points)).to(dev)

    def arm(fused):
        os.environ["VDN_SHADE_POINTS_FUSED"] = "1" if fused else "0"
        return mesh.shade_points(rend, x)

    def lean():
        """The least the separate kernels can do: ONE mode-1 SDF launch and the colour head on its feature plane as written (no
        row-major round trip of the plane, no second SDF launch for .gradient), the view direction in torch."""
        with torch.no_grad():
            sdf, feat, g = rend.sdf_network._run(1, pts=x)
            return sdf, g, rend.color_network._run(g, feat, pts=x, dirs=mesh.view_from_gradient(g))
    times = {True: [], False: [], "lean": []}
    for i in range(a.warmup + a.reps):
        for fused in (True, False, "lean"):
            ms, _ = timed(lean if fused == "lean" else (lambda: arm(fused)))
            if i >= a.warmup:
                times[fused].append(ms)
    f, s = arm(True), arm(False)
    res = {"points": a.points, "reps": a.reps,
           "fused_ms_median": float(np.median(times[True])), "fused_ms_min": float(np.min(times[True])), "fused_ms_max": float(np.max(times[True])),
           "separate_ms_median": float(np.median(times[False])), "separate_ms_min": float(np.min(times[False])),
           "separate_ms_max": float(np.max(times[False])), "two_kernels_ms_median": float(np.median(times["lean"])),
           "two_kernels_ms_min": float(np.min(times["lean"])), "two_kernels_ms_max": float(np.max(times["lean"])),
           "sdf_equal": bool(torch.equal(f[0], s[0])), "gradient_equal": bool(torch.equal(f[1], s[1])),
           "colour_max_abs_diff": float((f[2] - s[2]).abs().max())}
    del f, s
    os.environ["VDN_SHADE_POINTS_FUSED"] = "1"
    # the share of a whole validate_mesh call (lattice, marching cubes, vertex shading, the file) that vertex shading takes
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(2):        # (the first call warms every launch's code)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, V, F = validate.validate_mesh(rend, lo, hi, os.path.join(tmp, "m.ply"), resolution=a.resolution)
            torch.cuda.synchronize()
            whole = time.perf_counter() - t0
            t0 = time.perf_counter()
            validate.validate_mesh(rend, lo, hi, os.path.join(tmp, "bare.ply"), resolution=a.resolution, vertex_colors=False, vertex_normals=False)
            torch.cuda.synchronize()
            bare = time.perf_counter() - t0
    v, _ = rend.extract_geometry(lo, hi, resolution=a.resolution)
    xv = torch.from_numpy(v.astype(np.float32)).to(dev)
    shade = [timed(lambda: mesh.shade_points(rend, xv))[0] for _ in range(a.warmup + a.reps)][a.warmup:]
    res.update({"resolution": a.resolution, "vertices": V, "faces": F, "validate_mesh_s": whole, "validate_mesh_bare_s": bare,
                "vertex_shading_ms_median": float(np.median(shade)), "vertex_shading_share": float(np.median(shade)) * 1e-3 / whole})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
