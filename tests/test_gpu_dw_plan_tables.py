"""The ray engine's weight-gradient descriptor tables are unchanged by the per-network entry builders of vdn_hip/train.py
(sdf_dw_entries / rendering_dw_entries / nerf_dw_entries / dw_layout / dw_tables / weightnorm_table), which the point engine of
the standalone networks (vdn_hip/points.py) shares.

Every table of a TrainEngine (GEMM, finalize, weight-norm; whole and per launch group) is reduced to a canonical form - device
pointers as (buffer name, byte offset), the buffers named by the engine's own workspace keys - and hashed. The digests in
tests/golden/dw_plan_tables.json were made with this file's dump at the commit before the refactor:
    python tests/test_gpu_dw_plan_tables.py --dump OUT.json [--pkg DIR_OF_vdn_hip]

The launch groups (TrainEngine.groups: one DwGroup each) are also checked against each other: they cut the tables of `all` into
ranges of entries, nothing lost, nothing twice.
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
    structs = {"dw": "VdnDwDesc", "fin": "VdnDwFinalizeDesc", "wn": "VdnWeightNormBwdDesc"}
    tabs = {}
    for g, grp in eng.groups.items():
        for kind, struct in structs.items():
            if getattr(grp, "n_" + kind):
                tabs[kind if g == "all" else kind + "." + g] = (getattr(grp, kind), struct)
    out = {}
    for k, (t, struct) in sorted(tabs.items()):
        body = json.dumps(_canon(t, struct, stor), sort_keys=True)
        out[k] = hashlib.sha256(body.encode()).hexdigest()
    a, parts = eng.groups["all"], {g: grp for g, grp in eng.groups.items() if g != "all"}
    out["scalars"] = [a.wgs, a.n_dw, a.n_fin, a.max_m, a.n_wn, a.wn_rows, a.phase1,
                      sorted((g, v.n_dw, v.wgs) for g, v in parts.items()),
                      sorted((g, v.n_fin, v.max_m, v.phase1) for g, v in parts.items())]
    out["maps"] = hashlib.sha256(eng.maps.cpu().numpy().tobytes()).hexdigest()
    return out


def make_engines(dev):
    from vdn_train import synth, factory
    from vdn_hip.train import TrainEngine
    res = {}
    for name, kw in CONFIGS.items():
        st = synth.make_all_states(0, wdepth=kw["wdepth"], depth_before_color=kw.get("depth_before_color", False))
        rend = factory.build_renderer(device=dev, states=st, **kw)
        res[name] = TrainEngine(rend, B, dev)
    return res


def all_digests(engines):
    return json.loads(json.dumps({name: engine_digests(eng) for name, eng in engines.items()}))


@pytest.fixture(scope="module")
def engines():
    import torch
    return make_engines(torch.device("cuda:0"))


@pytest.mark.gpu
def test_ray_engine_tables_unchanged(engines):
    got = all_digests(engines)
    want = json.load(open(GOLDEN))
    bad = ["%s/%s" % (c, k) for c in want for k in want[c] if got[c].get(k) != want[c][k]]
    assert not bad, bad
    extra = ["%s/%s" % (c, k) for c in want for k in got[c] if k not in want[c]]
    assert not extra and sorted(got) == sorted(want), extra


def _rows(grp, kind):
    from vdn_hip import lib
    struct = {"dw": "VdnDwDesc", "fin": "VdnDwFinalizeDesc", "wn": "VdnWeightNormBwdDesc"}[kind]
    n = getattr(grp, "n_" + kind)
    if not n:
        return np.zeros(0, dtype=lib.struct_dtype(struct))
    # (the first n descriptors: the SDF group's GEMM table is the device copy of the whole table, used with its own count)
    return np.frombuffer(getattr(grp, kind).cpu().numpy().tobytes(), dtype=lib.struct_dtype(struct))[:n].copy()


def _same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


@pytest.mark.gpu
def test_launch_groups_partition_the_tables(engines):
    """The launch groups of every engine cut the tables of `all` into ranges of entries: sdf + heads + nerf (and sdf + rest, rest =
    heads + nerf) carry every GEMM descriptor once, in order, with workgroups numbered from each group's own zero; the finalize
    rows of sdf + rest and the weight-norm rows of sdf + heads + nerf are those of `all`."""
    for name, eng in engines.items():
        G = eng.groups
        assert set(G) == {"all", "sdf", "rest", "heads", "nerf"}, name

        def chain(kind, *groups):
            parts, wg0 = [], 0
            for g in groups:
                r = _rows(G[g], kind)
                if kind == "dw":
                    assert len(r) and int(r["wg_begin"][0]) == 0, (name, g)
                    r["wg_begin"] += wg0             # back to the whole table's numbering
                    wg0 += G[g].wgs
                parts.append(r)
            return np.concatenate(parts)
        assert _same(chain("dw", "sdf", "heads", "nerf"), _rows(G["all"], "dw")), name
        assert _same(chain("dw", "heads", "nerf"), _rows(G["rest"], "dw")), name
        assert G["sdf"].wgs + G["heads"].wgs + G["nerf"].wgs == G["all"].wgs and G["heads"].wgs + G["nerf"].wgs == G["rest"].wgs, name
        multiset = lambda rows: sorted(r.tobytes() for r in rows)
        assert multiset(chain("fin", "sdf", "rest")) == multiset(_rows(G["all"], "fin")), name
        assert multiset(chain("fin", "heads", "nerf")) == multiset(_rows(G["rest"], "fin")), name
        assert _same(chain("wn", "sdf", "heads", "nerf"), _rows(G["all"], "wn")), name
        assert _same(chain("wn", "heads", "nerf"), _rows(G["rest"], "wn")), name


if __name__ == "__main__":
    args = sys.argv[1:]
    pkg = args[args.index("--pkg") + 1] if "--pkg" in args else os.path.join(ROOT, "vdn-nerf_amd")
    sys.path[:0] = [pkg, ROOT]
    import torch
    json.dump(all_digests(make_engines(torch.device("cuda:0"))), open(args[args.index("--dump") + 1], "w"), indent=1, sort_keys=True)
