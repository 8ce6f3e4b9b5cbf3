"""The gate of the run-time switches' arms (tests/switch_arms.py: ARMS): every switch of vdn_hip/switches.py has a row, every
row names a value the switch's kind accepts and that is not the default, and a test that runs it - the matrix of
tests/test_gpu_switch_arms.py, or an existing GPU test whose own source names the switch. No GPU, no library: a switch added to
the table without a row fails here."""
import os
import re

import pytest

import switch_arms
from conftest import ROOT
from switch_arms import ARMS
from vdn_hip import switches

NOT_AN_ARM = {"VDN_LIB", "VDN_BUILD_VARIANT"}


def test_one_row_per_declared_switch():
    assert set(ARMS) == set(switches.TABLE), (sorted(set(switches.TABLE) - set(ARMS)), sorted(set(ARMS) - set(switches.TABLE)))


def _parsed(s, value):
    """What the switch's kind makes of `value` (ValueError where it declines it)."""
    if s.kind == switches.ON:
        return value != "0"
    if s.kind == switches.ONLY1:
        return value == "1"
    if s.kind == switches.INT:
        v = int(value)
        return v if s.clamp is None else min(s.clamp[1], max(s.clamp[0], v))
    if s.kind == switches.WORD:
        v = value.strip().lower()
        if v not in ("bf16", "fp32"):
            raise ValueError(value)
        return v
    if not value:
        raise ValueError("an empty string is the unset switch")
    return value


def test_values_are_accepted_by_the_kind_and_are_not_the_default():
    for name, row in ARMS.items():
        s = switches.TABLE[name]
        assert isinstance(row["values"], tuple), name
        if row["held_by"] is None:
            assert row["values"] == (), name
            continue
        assert row["values"], name
        assert row["relation"] in ("bits", "rounding"), name
        for v in row["values"]:
            assert isinstance(v, str), (name, v)
            got = _parsed(s, v)                                   # (raises where the kind declines the string)
            if s.default is not switches.CALLER and s.default != "":
                assert got != _parsed(s, str(s.default)), (name, v, "is the default arm")
            if s.kind == switches.INT and s.clamp is not None:
                assert str(got) == v, (name, v, "is clamped to", got)
        assert len(set(row["values"])) == len(row["values"]), name


def _function_source(path, func):
    """The text of top-level function `func` of `path`, from its def to the next top-level statement (None: not defined)."""
    lines = open(path, encoding="utf-8").read().splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r"def %s\(" % re.escape(func), l)]
    if len(start) != 1:
        return None
    end = next((i for i in range(start[0] + 1, len(lines)) if lines[i] and not lines[i][0].isspace() and not lines[i].startswith("#")),
               len(lines))
    return "\n".join(lines[start[0]:end])


def held_by_problem(name, node, both):
    """None, or why `node` does not hold switch `name`: it must name the switch, and contain `both` - the line that builds the
    default-arm side as well as the arm's (a test that sets the arm on every side it compares has no such line)."""
    m = re.fullmatch(r"(tests/test_gpu_[a-z0-9_]+\.py)::(test_[A-Za-z0-9_]+)", node)
    if not m:
        return "not the node id of a GPU test: %r" % node
    path = os.path.join(ROOT, m.group(1))
    if not os.path.isfile(path):
        return "no such file: " + m.group(1)
    src = _function_source(path, m.group(2))
    if src is None:
        return "%s does not define %s" % (m.group(1), m.group(2))
    if not re.search(r"\b%s\b" % name, src):
        return "the source of %s does not name %s" % (node, name)
    if not both or both not in src:
        return "the source of %s does not hold the line that builds both sides: %r" % (node, both)
    return None


def test_held_by_names_a_test_that_runs_the_arm():
    held = {n: (r["held_by"], r["both"]) for n, r in ARMS.items() if r["held_by"] not in (None, "matrix")}
    assert len(held) >= 15
    bad = {n: held_by_problem(n, *nb) for n, nb in held.items()}
    assert not {n: p for n, p in bad.items() if p}, {n: p for n, p in bad.items() if p}


def test_matrix_rows_name_scenarios_and_a_predicate():
    natives = {s.name for s in switches.TABLE.values() if s.kind == switches.NATIVE}
    for name, row in ARMS.items():
        if row["held_by"] != "matrix":
            continue
        assert row["scenario"] and set(row["scenario"]) <= set(switch_arms.SCENARIO_NAMES), (name, row["scenario"])
        assert row["how"] in ("monkeypatch", "child", "dp_child"), name
        s = switches.TABLE[name]
        if s.read == "import" or s.kind == switches.NATIVE:
            assert row["how"] == "child", (name, "is read once per process: a running process cannot reach it")
        assert (row["how"] == "dp_child") == (row["scenario"] == ("dp_one_rank",)), name
        if name in natives:
            # the library reads it itself: the row points at the line of C++ that selects the arm
            m = re.fullmatch(r"(csrc/[a-z0-9_.]+):(\d+)", row["native"])
            line = open(os.path.join(ROOT, "vdn-nerf_amd", m.group(1))).read().splitlines()[int(m.group(2)) - 1]
            assert row["taken"] is None and 'getenv("%s")' % name in line, (name, line)
        else:
            assert callable(row["taken"]) and row["native"] is None, name
    assert {n for n, r in ARMS.items() if r["held_by"] == "matrix" and r["taken"] is None} == natives
    for (name, value), sel in switch_arms.FP64_UNDER_ARM.items():
        assert name in natives and value in ARMS[name]["values"]
        for arg in sel:
            if arg.startswith("tests/"):
                assert os.path.isfile(os.path.join(ROOT, arg)), arg
    assert {n for n, _ in switch_arms.FP64_UNDER_ARM} == natives


def test_only_the_other_builds_are_not_an_arm():
    assert {n for n, r in ARMS.items() if r["held_by"] is None} == NOT_AN_ARM
    for n in NOT_AN_ARM:
        assert ARMS[n]["reason"]


def test_the_gate_bites():
    """A held_by that points at a test which never names the switch, at a function that does not exist, at a missing file."""
    good, both = ARMS["VDN_FUSED_COMPOSITE"]["held_by"], ARMS["VDN_FUSED_COMPOSITE"]["both"]
    assert held_by_problem("VDN_FUSED_COMPOSITE", good, both) is None
    assert "does not name" in held_by_problem("VDN_RENDER_GRAPH", good, both)
    assert "does not define" in held_by_problem("VDN_FUSED_COMPOSITE", good + "_no_such", both)
    assert "no such file" in held_by_problem("VDN_FUSED_COMPOSITE", "tests/test_gpu_no_such_file.py::test_x", both)
    # a test that names the switch but runs the arm on both sides (tests/stream_skew.py sets VDN_BWD_SPLIT_DW in the delayed and the
    # serial arm alike): nothing in it builds a default side
    node = "tests/test_gpu_stream_order.py::test_drop_in_flow_equals_the_one_stream_run"
    assert "both sides" in held_by_problem("VDN_BWD_SPLIT_DW", node, 'for mode in ("1", "0"):')
    assert "both sides" in held_by_problem("VDN_BWD_SPLIT_DW", node, "")
    assert ARMS["VDN_BWD_SPLIT_DW"]["held_by"] == "matrix"
    with pytest.raises(ValueError):
        _parsed(switches.TABLE["VDN_DW_SPLIT_PTS"], "many")


def test_the_fp64_fallback_rule():
    """further_than_twice (the rounding relation's fallback in tests/test_gpu_switch_arms.py, reached only when an arm misses its
    bound against the default arm): at most 2 x the default arm's distance to fp64, per tensor."""
    rule = switch_arms.further_than_twice
    assert rule([("a", 1e-7, 2e-7), ("b", 0.0, 0.0), ("c", 3e-9, 1e-9)]) == []
    assert rule([("a", 1e-7, 2.0001e-7), ("b", 1e-8, 1e-8)]) == [("a", 1e-7, 2.0001e-7)]
    assert rule([("z", 0.0, 1e-30)]) == [("z", 0.0, 1e-30)]                       # exact on the default, off on the arm
    assert [n for n, _, _ in rule([("n", 1e-7, float("nan")), ("i", 1e-7, float("inf"))])] == ["n", "i"]
    # the measured pairs of the one-split fp32 arm before the kernel fix (record)
    seen = [("sdf.lin2.weight_v", 9.570e-08, 3.211e-07), ("sdf.lin3.weight_v", 7.853e-08, 1.512e-07), ("color.lin4.bias", 1.155e-08, 1.003e-07)]
    assert [n for n, _, _ in rule(seen)] == ["sdf.lin2.weight_v", "color.lin4.bias"]


def test_design_table_names_who_holds_each_switch():
    """the fourth column ("held by") names, for every row, the matrix and / or the files of the tests ARMS points at."""
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec = text[text.index("\n## 11. Run-time switches"):]
    sec = sec[:sec.index("\n## ", 1)]
    rows = [l for l in sec.splitlines() if l.startswith("|")]
    assert rows[0].rstrip().endswith("| held by |")
    seen = set()
    for l in rows[2:-1]:
        cells = [c.strip() for c in l.strip().strip("|").split("|")]
        assert len(cells) == 4, l[:60]
        seen |= {n for n in re.findall(r"VDN_[A-Z0-9_]+", l) if n in ARMS and ARMS[n]["held_by"] is None}
        for name in re.findall(r"VDN_[A-Z0-9_]+", cells[0]):
            if name not in ARMS:
                continue
            seen.add(name)
            held = ARMS[name]["held_by"]
            if held == "matrix":
                assert "test_gpu_switch_arms" in cells[3], name
            elif held is not None:
                assert held in cells[3], (name, held)
    assert seen == set(ARMS), sorted(set(ARMS) - seen)
