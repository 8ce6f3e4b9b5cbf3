"""The run-time switches (vdn_hip/switches.py): every parse rule against a literal table written out from the expressions the
read sites used to spell themselves, the environment read in one place only, DESIGN.md 11 held to the table, and the graph
plans' keys derived from it."""
import glob
import os
import re

import pytest

from conftest import PKG, ROOT
from vdn_hip import switches

VALUES = (None, "", "0", "1", "2", "off")        # None: unset
VE = ValueError

# on unless exactly "0" (`os.environ.get(NAME, "1") != "0"`)
ON = ("VDN_FUSE_ROUNDS", "VDN_FUSE_SDF_ROUNDS", "VDN_BG_COMPACT", "VDN_RENDER_FG_COMPACT", "VDN_SHADE_FUSED", "VDN_FG_COMPACT",
      "VDN_FUSED_PREP", "VDN_BWD_SPLIT_DW", "VDN_SDF_BWD_SPLIT", "VDN_SHADE_POINTS_FUSED", "VDN_FUSED_COMPOSITE", "VDN_DP_FUSED",
      "VDN_SPLIT_REST", "VDN_EVENT_TRIM", "VDN_RENDER_GRAPHS", "VDN_RELU_MASK", "VDN_OVERLAP", "VDN_DP_SIDE_GROUP", "VDN_DP_INSTREAM")
# (name, default the caller supplies or None) -> the result for each of VALUES
FLAGS = {(n, None): (True, True, False, True, True, True) for n in ON}
FLAGS.update({
    ("VDN_SDF_TAIL", "1"): (True, True, False, True, True, True),          # (no side stream)
    ("VDN_SDF_TAIL", "0"): (False, True, False, True, True, True),         # (with one)
    ("VDN_SIDE_STREAM", None): (True, False, False, True, False, False),   # `os.environ.get(NAME, "1") == "1"`
    ("VDN_TRAIN_COLOR_FUSED", None): (False, False, False, True, False, False),      # `os.environ.get(NAME, "0") == "1"`
    ("VDN_RENDER_GRAPH", None): (False, False, False, True, False, False),
})
# `int(os.environ.get(NAME, default))`; VDN_RENDER_ENGINES: `min(3, max(1, int(os.environ.get(NAME, "3") or 3)))`
INTS = {
    ("VDN_DW_SPLIT_PTS", None): (4096, VE, 0, 1, 2, VE),
    ("VDN_DW_SPLIT_PTS_SDF", 2048): (2048, VE, 0, 1, 2, VE),
    ("VDN_DW_SPLIT_PTS_REST", 2048): (2048, VE, 0, 1, 2, VE),
    ("VDN_DW_SPLIT_PTS_NERF", "4096"): (4096, VE, 0, 1, 2, VE),
    ("VDN_DW_SPLIT_PTS_HEADS", "4096"): (4096, VE, 0, 1, 2, VE),
    ("VDN_SDF_TAIL_ROW0", 128 * 256): (32768, VE, 0, 1, 2, VE),
    ("VDN_SDF_TAIL_MAX", None): (8192, VE, 0, 1, 2, VE),
    ("VDN_RENDER_ENGINES", None): (3, 3, 1, 1, 2, VE),
}
VALID = {"VDN_RENDER_ENGINES": (("7", 3), ("-4", 1), ("2", 2))}          # other int switches: "5000" -> 5000
# _pts_per_split: (precision, the one variable of the family set to "1000" or None) -> rows for the sdf / nerf / heads launches
CHAIN = {
    ("bf16", None): (6144, 4096, 4096),
    ("bf16", "VDN_DW_SPLIT_PTS"): (1000, 4096, 4096),          # (the rest group's fallback is the value read at import)
    ("bf16", "VDN_DW_SPLIT_PTS_SDF"): (1000, 4096, 4096),
    ("bf16", "VDN_DW_SPLIT_PTS_REST"): (6144, 1000, 1000),
    ("bf16", "VDN_DW_SPLIT_PTS_NERF"): (6144, 1000, 4096),
    ("bf16", "VDN_DW_SPLIT_PTS_HEADS"): (6144, 4096, 1000),
    ("fp32", None): (2048, 2048, 2048),
    ("fp32", "VDN_DW_SPLIT_PTS"): (2048, 2048, 2048),
    ("fp32", "VDN_DW_SPLIT_PTS_SDF"): (1000, 2048, 2048),
    ("fp32", "VDN_DW_SPLIT_PTS_REST"): (2048, 1000, 1000),
    ("fp32", "VDN_DW_SPLIT_PTS_NERF"): (2048, 2048, 2048),
    ("fp32", "VDN_DW_SPLIT_PTS_HEADS"): (2048, 2048, 2048),
}
# name -> ((value or None, result), ...)
TEXTS = {
    "VDN_PRECISION": ((None, None), ("", None), ("  ", None), ("bf16", "bf16"), (" BF16\n", "bf16"), ("Half", "half")),
    "VDN_MESH_METHOD": ((None, "cubes"), ("", ""), ("tets", "tets"), (" Tets", " Tets")),
    "VDN_MESH_SPARSE": ((None, ""), ("", ""), ("0", "0"), ("8:2.5", "8:2.5")),
    "VDN_LIB": ((None, ""), ("", ""), ("/x/lib.so", "/x/lib.so")),
    "VDN_BUILD_VARIANT": ((None, ""), ("", ""), ("a:-DX=1 -DY", "a:-DX=1 -DY")),
}
NATIVE = ("VDN_SDF2_WARM", "VDN_PLANE_PREFETCH", "VDN_SDF0_SPLIT_MAX")
# the hand-kept tuple _TrainPlan keyed on before the table existed
TRAIN = ("VDN_RENDER_FG_COMPACT", "VDN_FG_COMPACT", "VDN_BG_COMPACT", "VDN_FUSED_PREP", "VDN_TRAIN_COLOR_FUSED", "VDN_SDF_TAIL",
         "VDN_SDF_TAIL_ROW0", "VDN_SDF_TAIL_MAX", "VDN_BWD_SPLIT_DW", "VDN_SDF_BWD_SPLIT", "VDN_FUSE_ROUNDS", "VDN_FUSE_SDF_ROUNDS")
# what render() without grad reads in _sample / render / _shade
RENDER = ("VDN_FUSE_ROUNDS", "VDN_FUSE_SDF_ROUNDS", "VDN_BG_COMPACT", "VDN_SHADE_FUSED")


@pytest.fixture
def env(monkeypatch):
    for name in switches.TABLE:
        monkeypatch.delenv(name, raising=False)

    def put(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return put


def _check(read, name, default, value, want, env):
    env(name, value)
    if want is VE:
        with pytest.raises(ValueError):
            read(name, default)
    else:
        got = read(name, default)
        assert got == want and type(got) is type(want), (name, default, value, got, want)
    env(name, None)


def test_every_switch_is_covered_by_the_literal_tables():
    literal = {n for n, _ in FLAGS} | {n for n, _ in INTS} | set(TEXTS) | set(NATIVE)
    assert literal == set(switches.TABLE) and len(switches.TABLE) == 39
    for s in switches.TABLE.values():
        assert s.read in ("import", "construct", "call") and set(s.regions) <= {"train", "render"} and s.doc, s.name
    assert {s.name for s in switches.TABLE.values() if s.kind == switches.NATIVE} == set(NATIVE)


def test_flags_parse_as_their_read_sites_did(env):
    for (name, default), wants in FLAGS.items():
        for value, want in zip(VALUES, wants):
            _check(switches.flag, name, default, value, want, env)
    env("VDN_FG_COMPACT", "off")
    env("VDN_SIDE_STREAM", "2")
    assert switches.flag("VDN_FG_COMPACT") is True and switches.flag("VDN_SIDE_STREAM") is False
    with pytest.raises(TypeError):
        switches.flag("VDN_SDF_TAIL")                      # (its default is the engine's to give)


def test_ints_parse_as_their_read_sites_did(env):
    for (name, default), wants in INTS.items():
        for value, want in zip(VALUES, wants):
            _check(switches.integer, name, default, value, want, env)
        for value, want in VALID.get(name, (("5000", 5000),)):
            _check(switches.integer, name, default, value, want, env)
    with pytest.raises(TypeError):
        switches.integer("VDN_SDF_TAIL_ROW0")


def test_weight_gradient_split_chain(env, monkeypatch):
    from vdn_hip import train
    monkeypatch.setattr(train, "PTS_PER_SPLIT", 4096)     # (VDN_DW_SPLIT_PTS as read at import, the default)
    for (precision, name), want in CHAIN.items():
        if name is not None:
            env(name, "1000")
        assert tuple(train._pts_per_split(net, precision) for net in ("sdf", "nerf", "heads")) == want, (precision, name)
        if name is not None:
            env(name, None)
    # only the value that is used is parsed
    env("VDN_DW_SPLIT_PTS", "off")
    env("VDN_DW_SPLIT_PTS_SDF", "512")
    assert train._pts_per_split("sdf", "bf16") == 512
    env("VDN_DW_SPLIT_PTS_SDF", None)
    with pytest.raises(ValueError):
        train._pts_per_split("sdf", "bf16")


def test_strings_parse_as_their_read_sites_did(env):
    for name, cases in TEXTS.items():
        for value, want in cases:
            _check(lambda n, _: switches.text(n), name, None, value, want, env)


def test_undeclared_names_raise_at_the_read_site(env):
    for read in (switches.flag, switches.integer, switches.text, switches.raw):
        with pytest.raises(KeyError):
            read("VDN_NO_SUCH_SWITCH")
    for read, name in ((switches.flag, "VDN_RENDER_ENGINES"), (switches.integer, "VDN_FG_COMPACT"), (switches.text, "VDN_SDF_TAIL_MAX"),
                       (switches.raw, "VDN_SDF2_WARM"), (switches.flag, "VDN_PLANE_PREFETCH"), (switches.signature, "bench")):
        with pytest.raises(KeyError):
            read(name)


def test_call_time_switches_are_live(env):
    assert switches.flag("VDN_SHADE_FUSED")
    env("VDN_SHADE_FUSED", "0")
    assert not switches.flag("VDN_SHADE_FUSED")
    env("VDN_SHADE_FUSED", None)
    assert switches.flag("VDN_SHADE_FUSED")


def _csrc_text():
    return "\n".join(open(p, errors="replace").read() for p in sorted(glob.glob(os.path.join(PKG, "csrc", "**", "*"), recursive=True)) if os.path.isfile(p))


def test_the_environment_is_read_in_one_place():
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) > 20
    hits = []
    for p in files:
        if os.path.basename(p) == "switches.py":
            continue
        for i, line in enumerate(open(p).read().splitlines(), 1):
            if re.search(r"\b(environ|getenv|putenv)\b", line) and not (p.endswith(os.path.join("vdn_hip", "build.py")) and "MAX_JOBS" in line):
                hits.append("%s:%d: %s" % (os.path.relpath(p, ROOT), i, line.strip()))
    assert not hits, hits
    own = open(os.path.join(PKG, "vdn_hip", "switches.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s.*$", own, flags=re.M) == ["import os", "from collections import namedtuple"]      # (no torch)
    assert set(re.findall(r'getenv\(\s*"(VDN_[A-Z0-9_]+)"', _csrc_text())) == set(NATIVE)


def test_design_table_lists_the_declared_switches():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec = text[text.index("\n## 11. Run-time switches"):]
    sec = sec[:sec.index("\n## ", 1)]
    rows = [l for l in sec.splitlines() if l.startswith("|")]
    closing = [i for i, l in enumerate(rows) if "no longer in the tree" in l]
    assert len(closing) == 1 and closing[0] == len(rows) - 1
    live = set(re.findall(r"VDN_[A-Z0-9_]+", "\n".join(rows[:-1])))
    gone = set(re.findall(r"VDN_[A-Z0-9_]+", rows[-1]))
    assert set(switches.TABLE) <= live, sorted(set(switches.TABLE) - live)
    csrc = _csrc_text()
    for name in sorted(live - set(switches.TABLE)):
        assert re.search(r"\b%s\b" % name, csrc), name + " is neither a declared switch nor a macro of csrc/"
    assert len(gone) == 14 and not gone & set(switches.TABLE)
    for name in gone:                                     # ... and nothing in the package reads them
        assert not re.search(r"\b%s\b" % name, csrc), name


def test_plan_keys_come_from_the_table(env):
    for region, names in (("train", TRAIN), ("render", RENDER)):
        declared = tuple(s.name for s in switches.TABLE.values() if region in s.regions)
        assert set(declared) == set(names) and len(declared) == len(names)
        base = switches.signature(region)
        assert base == (None,) * len(names)
        for name in names:
            env(name, "0")
            sig = switches.signature(region)
            assert sig != base and sig[declared.index(name)] == "0" and sig.count(None) == len(names) - 1, (region, name)
            env(name, "")                                 # (the raw strings: "" is not unset)
            assert switches.signature(region) != base
            env(name, None)
            assert switches.signature(region) == base
        for name in set(switches.TABLE) - set(names):
            env(name, "0")
            assert switches.signature(region) == base, (region, name)
            env(name, None)
    assert "VDN_EVENT_TRIM" not in TRAIN + RENDER and "VDN_RENDER_ENGINES" not in TRAIN + RENDER
