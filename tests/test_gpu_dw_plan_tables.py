"""The ray engine's weight-gradient descriptor tables are unchanged by the per-network entry builders of vdn_hip/train.py
(sdf_dw_entries / rendering_dw_entries / nerf_dw_entries / dw_layout / dw_tables / weightnorm_table), which the point engine of
the standalone networks (vdn_hip/points.py) shares.

Every table of a TrainEngine (GEMM, finalize, weight-norm; whole and per launch group) is reduced to a canonical form - device
pointers as (buffer name, byte offset), the buffers named by the engine's own workspace keys - and hashed. The digests in
tests/golden/dw_plan_tables.json were made with this file's dump at the commit before the refactor:
    python tests/test_gpu_dw_plan_tables.py --dump OUT.json [--pkg DIR_OF_vdn_hip]
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dw_plan_tables.json")
CONFIGS = {"wdepth_fp32": dict(wdepth=True, precision="fp32"), "wdepth_bf16": dict(wdepth=True, precision="bf16"),
           "plain_bf16": dict(wdepth=False, precision="bf16"), "dbc_bf16": dict(wdepth=True, precision="bf16", depth_before_color=True)}
B = 64


def _storages(eng):
    named = []
    for k, v in eng.w.items():
        for i, t in enumerate(v if isinstance(v, tuple) else (v,)):
            if t is not None:
                named.append(("w.%s.%d" % (k, i), t))
    named += [("slab", eng.slab), ("colsum", eng.colsum), ("maps", eng.maps), ("grad_flat", eng._grad_flat), ("var_map", eng._var_map)]
    for key, net in eng.nets.items():
        named += [(key + ".dweff", net.dweff), (key + ".inv_norm", net.img.inv_norm)]
    named += [("param%d" % i, p) for i, p in enumerate(eng.params)]
    out, seen = [], set()
    for n, t in named:
        s = t.untyped_storage()
        if s.data_ptr() not in seen:
            seen.add(s.data_ptr())
            out.append((s.data_ptr(), s.nbytes(), n))
    return out


def _canon(tab, struct, stor):
    from vdn_hip import lib
    import ctypes
    ptr_fields = [f for f, t in lib.STRUCTS[struct]._fields_ if t is ctypes.c_void_p]
    arr = np.frombuffer(tab.cpu().numpy().tobytes(), dtype=lib.struct_dtype(struct))

    def rel(p):
        p = int(p)
        if p == 0:
            return 0
        for base, nb, n in stor:
            if base <= p < base + nb:
                return "%s+%d" % (n, p - base)
        return "?"
    rows = []
    for r in arr:
        rows.append({f: (rel(r[f]) if f in ptr_fields else repr(r[f].item())) for f in arr.dtype.names})
    return rows


def engine_digests(eng):
    stor = _storages(eng)
    tabs = {"dw": (eng.dw_table, "VdnDwDesc"), "fin": (eng.fin_table, "VdnDwFinalizeDesc"), "wn": (eng.wn_table, "VdnWeightNormBwdDesc")}
    for g, v in eng.dw_groups.items():
        tabs["dw." + g] = (v[0], "VdnDwDesc")
    for g, v in eng.fin_groups.items():
        tabs["fin." + g] = (v[0], "VdnDwFinalizeDesc")
    for g, v in eng.wn_groups.items():
        tabs["wn." + g] = (v[0], "VdnWeightNormBwdDesc")
    out = {}
    for k, (t, struct) in sorted(tabs.items()):
        body = json.dumps(_canon(t, struct, stor), sort_keys=True)
        out[k] = hashlib.sha256(body.encode()).hexdigest()
    out["scalars"] = [eng.dw_total_wgs, eng.n_dw, eng.n_fin, eng.fin_max_M, eng.n_wn, eng.wn_max_rows, eng.fin_has_phase1,
                      sorted((g, v[1], v[2]) for g, v in eng.dw_groups.items()),
                      sorted((g, v[1], v[2], v[3]) for g, v in eng.fin_groups.items())]
    out["maps"] = hashlib.sha256(eng.maps.cpu().numpy().tobytes()).hexdigest()
    return out


def all_digests(dev):
    from vdn_train import synth, factory
    from vdn_hip.train import TrainEngine
    res = {}
    for name, kw in CONFIGS.items():
        st = synth.make_all_states(0, wdepth=kw["wdepth"], depth_before_color=kw.get("depth_before_color", False))
        rend = factory.build_renderer(device=dev, states=st, **kw)
        res[name] = engine_digests(TrainEngine(rend, B, dev))
    return json.loads(json.dumps(res))


@pytest.mark.gpu
def test_ray_engine_tables_unchanged():
    import torch
    got = all_digests(torch.device("cuda:0"))
    want = json.load(open(GOLDEN))
    bad = ["%s/%s" % (c, k) for c in want for k in want[c] if got[c].get(k) != want[c][k]]
    assert not bad, bad


if __name__ == "__main__":
    args = sys.argv[1:]
    pkg = args[args.index("--pkg") + 1] if "--pkg" in args else os.path.join(ROOT, "vdn-nerf_amd")
    sys.path[:0] = [pkg, ROOT]
    import torch
    json.dump(all_digests(torch.device("cuda:0")), open(args[args.index("--dump") + 1], "w"), indent=1, sort_keys=True)
