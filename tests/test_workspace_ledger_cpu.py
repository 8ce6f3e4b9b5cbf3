"""The workspace ledger (tests/poison.py) held to the source without a GPU: every buffer the engine, the Trainer and a launch group
create has a row, the rows are well-formed, and the poison generators produce what they claim."""
import inspect
import os
import re

import pytest
import torch

import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_PY = os.path.join(ROOT, "vdn-nerf_amd", "vdn_hip", "train.py")


def _assignments(src):
    """[(left side, right side)] of the plain assignment statements of `src` (one per logical line; continuation lines join)."""
    out, cur = [], ""
    for line in src.splitlines():
        code = line.split("#")[0].rstrip()
        if not code.strip():
            continue
        cur = (cur + " " + code.strip()) if cur else code.strip()
        if cur.count("(") + cur.count("[") > cur.count(")") + cur.count("]") or cur.endswith("\\"):
            continue
        m = re.match(r"^([^=]+?)\s=\s(?!=)(.*)$", cur)
        if m and not cur.startswith(("if ", "for ", "while ", "return ", "assert ", "elif ")):
            out.append((m.group(1), m.group(2)))
        cur = ""
    return out


def _makes_tensor(rhs):
    """The right side allocates or moves a tensor (and no stream, event or device object)."""
    if re.search(r"Event|Stream|torch\.device|lambda", rhs):
        return False
    return bool(re.search(r"torch\.(empty|zeros|ones|full|rand|from_numpy|zeros_like|empty_like)|\bf\(|\bfz\(|\bfs\(|\.to\((self\.)?dev\)", rhs))


def _has_row(table, key):
    return key in table or any(k.startswith(key + ".") for k in table)


def test_every_workspace_key_of_the_engine_has_a_row():
    src = open(TRAIN_PY).read()
    keys = set()
    for lhs, rhs in _assignments(src):
        keys.update(re.findall(r'\bw\["(\w+)"\]', lhs))
    assert len(keys) > 80 and {"slab", "colsum"}.isdisjoint(keys), sorted(keys)
    missing = sorted(k for k in keys if not _has_row(poison.W_LEDGER, k))
    assert not missing, "w[...] keys of vdn_hip/train.py without a row in tests/poison.py W_LEDGER: %s" % missing
    # ... and no row for a key the source no longer has
    gone = sorted(k for k in poison.W_LEDGER if k.split(".")[0] not in keys)
    assert not gone, gone


def _self_attrs(fn, accept=_makes_tensor):
    attrs = set()
    for lhs, rhs in _assignments(inspect.getsource(fn)):
        if accept(rhs):
            attrs.update(re.findall(r"\bself\.(\w+)", lhs))
    return attrs


def test_every_buffer_attribute_has_a_row():
    from vdn_hip.train import DwGroup, TrainEngine, _Net
    from vdn_train.trainer import Trainer
    tr = _self_attrs(Trainer.__init__) | _self_attrs(Trainer._init_cameras) | _self_attrs(Trainer._set_intrinsics)
    assert {"_param_flat", "_exp_avg", "g_color", "scalars", "_rows", "_near", "_far", "_pose_flat", "_intrin_inv", "_eik_partial"} <= tr, sorted(tr)
    missing = sorted(a for a in tr if not _has_row(poison.TRAINER_LEDGER, a))
    assert not missing, "Trainer attributes without a row in TRAINER_LEDGER: %s" % missing
    # created later, on first use (trainer.py: _pose_scratch, _g_log, _fg_cnt_g, _jitter, _last_pixels)
    lazy = set(re.findall(r"self\.(_pose_scratch|_g_log|_fg_cnt_g|_jitter|_last_pixels)\b", inspect.getsource(Trainer)))
    assert len(lazy) == 5 and all(_has_row(poison.TRAINER_LEDGER, a) for a in lazy), lazy
    eng = _self_attrs(TrainEngine.__init__) | _self_attrs(TrainEngine._build_dw_plan) | _self_attrs(_Net.__init__)
    eng.discard("_out_slots")             # (assigned beside the arena: a host-side dict of offsets and shapes)
    assert {"_out_arena", "_fg_cnt", "_grad_flat", "slab", "colsum", "maps", "_var_map", "dweff"} <= eng, sorted(eng)
    missing = sorted(a for a in eng if not _has_row(poison.ENGINE_LEDGER, a))
    assert not missing, "TrainEngine attributes without a row in ENGINE_LEDGER: %s" % missing
    # a launch group: its three device tables and the row cap (every attribute that is not a plain count)
    grp = _self_attrs(DwGroup.__init__, accept=lambda rhs: True)
    counts = {a for a in grp if a.startswith("n_")} | {"wgs", "max_m", "phase1", "wn_rows"}
    assert grp - counts == {"dw", "fin", "wn", "cap"}, sorted(grp - counts)
    assert all(_has_row(poison.DWGROUP_LEDGER, a) for a in grp - counts)


def test_rows_are_well_formed():
    seen = set()
    for pattern, cls, how, cite in poison.LEDGER:
        assert pattern not in seen, pattern
        seen.add(pattern)
        assert cls in poison.CLASSES, (pattern, cls)
        if cls in poison.POISONED:
            assert how in ("ones", "stale") or (isinstance(how, tuple) and how[0] in ("index", "count") and callable(how[1])), (pattern, how)
            assert re.search(r"\w+\.py:\d+", cite), (pattern, "a rewritten / masked row cites the line that justifies it", cite)
            if cls == "masked":
                assert how == "stale", pattern
        else:
            assert how is None and len(cite) > 10, (pattern, "a state / const row names the owner")
    assert all(p in seen for p in poison.REFERENCES)
    # a cited line exists in the cited file
    files = {"train.py": "vdn_hip/train.py", "trainer.py": "vdn_train/trainer.py", "renderer.py": "dpt_models/renderer.py",
             "fields.py": "dpt_models/fields.py", "points.py": "vdn_hip/points.py", "k_composite_row.h": "csrc/k_composite_row.h"}
    lines = {k: len(open(os.path.join(ROOT, "vdn-nerf_amd", v)).read().splitlines()) for k, v in files.items()}
    cited = 0
    for pattern, cls, how, cite in poison.LEDGER:
        for name, first in re.findall(r"(\w+\.(?:py|h)):(\d+)", cite):
            if name in lines:
                cited += 1
                assert 0 < int(first) <= lines[name], (pattern, name, first)
    assert cited > 100
    # descriptor tables hold raw device addresses: never a poisoned class
    for key in ("dw", "fin", "wn"):
        assert poison.DWGROUP_LEDGER[key][0] == "const"
    for pattern, cls, how, cite in poison.LEDGER:
        if any(s in pattern for s in ("_img_tables", "_img_cache", "._img.", ".img.", "group.")):
            assert cls in ("state", "const"), pattern


class _Eng:
    P, Q, N, T = 12, 20, 4, 5


def test_walker_names_views_once_and_wants_a_row_for_everything():
    lin = torch.nn.Linear(3, 2)
    flat = torch.zeros(10)
    holder = {"flat": flat, "pair": (flat[2:5], flat[2:5]), "again": flat, "other": [torch.ones(2, dtype=torch.int32)], "lin": lin,
              "skipped": "text", 7: torch.zeros(1)}
    found = poison.walk({"root": holder}, device_only=False)
    names = [f.name for f in found]
    assert names == ["root.flat", "root.pair.0", "root.other.0", "root.lin._parameters.weight", "root.lin._parameters.bias", "root.7"]
    assert found[0].aliases == ["root.again"] and found[1].aliases == ["root.pair.1"]
    assert found[1].span == (flat.untyped_storage().data_ptr(), 8, 20)
    assert poison.walk({"root": holder}) == []                               # nothing on a device
    ledger = [("root.flat", "rewritten", "ones", "x.py:1"), ("root.pair.*", "state", None, "owner: the test"), ("*._parameters.*", "state", None, "the module"),
              ("root.other.*", "rewritten", ("index", lambda e: e.P), "x.py:2")]
    with pytest.raises(AssertionError, match="root.7"):
        poison.classify(found, ledger)
    ledger.append(("root.7", "const", None, "a constant of the test"))
    poison.classify(found, ledger)
    assert [f.row[1] for f in found] == ["rewritten", "state", "rewritten", "state", "state", "const"]
    # poisoning the container covers the state view inside it: coverage reports the clobbered bytes
    found[2].engine = _Eng
    done = poison.apply(found)
    cov = poison.coverage(found, done)
    assert sorted(done) == ["root.flat", "root.other.0"] and cov["clobbered"] == 12
    assert cov["non_state_bytes"] == 40 - 12 + 8 and cov["poisoned_bytes"] == cov["non_state_bytes"]
    assert torch.isnan(flat).all() and int(found[2].tensor.max()) < 12


def test_a_reference_gives_way_to_the_owner():
    t = torch.zeros(4)
    found = poison.walk({"eng": {"_ctx": (t,)}, "tr": {"g_color": t}}, device_only=False)
    assert [f.name for f in found] == ["eng._ctx.0"]
    poison.classify(found)
    assert found[0].name == "tr.g_color" and found[0].row[1] == "rewritten" and found[0].aliases == ["eng._ctx.0"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8])
def test_all_ones_bytes(dtype):
    t = torch.zeros(5, 7, dtype=dtype)
    poison.ones_bytes_(t)
    assert (t == 255).all() if dtype == torch.uint8 else torch.isnan(t).all()
    base = torch.zeros(6, 8, dtype=dtype)
    view = base[1:5, 2:6]                                                      # not contiguous: only the view is written
    poison.ones_bytes_(view)
    hit = (base == 255) if dtype == torch.uint8 else torch.isnan(base)
    assert hit[1:5, 2:6].all() and int(hit.sum()) == 16
    poison.ones_bytes_(torch.zeros(0, dtype=dtype))
    scalar = torch.zeros((), dtype=dtype)                                      # a 0-dim view (the variance's gradient)
    poison.ones_bytes_(scalar)
    assert int(scalar) == 255 if dtype == torch.uint8 else bool(torch.isnan(scalar))
    with pytest.raises(AssertionError):
        poison.ones_bytes_(torch.zeros(3, dtype=torch.int32))                  # an integer list never gets all-ones bytes


@pytest.mark.parametrize("capacity", [0, 1, 2, 7, 20480])
@pytest.mark.parametrize("kind", ["index", "count"])
def test_integer_poison_stays_in_range(kind, capacity):
    lo, hi = poison.int_range(kind, capacity)
    assert lo == 0 and hi == (max(capacity - 1, 0) if kind == "index" else capacity)
    t = torch.full((4096,), -5, dtype=torch.int32)
    poison.int_poison_(t, kind, capacity, poison.generator(3))
    assert int(t.min()) >= lo and int(t.max()) <= hi
    if capacity >= 2:
        assert len(t.unique()) > 1
        if capacity <= 7:
            assert int(t.min()) == lo and int(t.max()) == hi                   # the whole range is used, both ends included
    with pytest.raises(AssertionError):
        poison.int_poison_(torch.zeros(3), kind, capacity, poison.generator(0))


@pytest.mark.parametrize("shape", [(0,), (1,), (257,), (33, 3), (4, 16, 8)])
def test_shuffled_stale_is_a_permutation(shape):
    src = torch.arange(int(torch.tensor(shape).prod()), dtype=torch.float32).reshape(shape)
    out = poison.shuffled_stale(src, poison.generator(5))
    assert out.shape == src.shape and (src.numel() == 0 or out.data_ptr() != src.data_ptr())
    assert torch.equal(out.reshape(-1).sort().values, src.reshape(-1).sort().values)
    if len(shape) >= 2:                                                        # whole rows change places
        rows = {tuple(r.tolist()) for r in src.reshape(-1, shape[-1])}
        assert all(tuple(r.tolist()) in rows for r in out.reshape(-1, shape[-1]))
    if src.numel() > 100:
        assert not torch.equal(out, src)
    assert torch.equal(out, poison.shuffled_stale(src, poison.generator(5)))   # the same seed, the same stale rows


def test_interval_measure():
    assert poison._minus([(0, 10), (5, 20)], []) == 20
    assert poison._minus([(0, 10), (30, 40)], [(5, 35)]) == 10
    assert poison._minus([(0, 10)], [(0, 4), (4, 10)]) == 0
