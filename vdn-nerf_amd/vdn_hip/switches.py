"""The package's run-time switches (environment variables): ONE table, and the only place that reads the environment.

Each switch selects the launches a step issues - the A/B arm of a measurement, the reference arm of a bit-identity test, or a
memory bound - and every arm ships. A row states how the value is parsed, its default, when it is read and which captured
region (the graphs of NeuSRenderer's _TrainPlan: "train", of RenderPlan: "render") it selects launches in; signature(region)
is what those plans key on. DESIGN.md 11 is the same table for users (tests/test_switches_cpu.py holds the two together).

Kinds:  ON      a flag that is on unless the value is exactly "0" ("", "2", "off" are all ON)
        ONLY1   a flag that is on only if the value is exactly "1"
        INT     int(value): anything int() declines raises ValueError, the empty string included; with a `clamp` the empty
                string counts as unset and the value is clamped
        STR     the raw string;  WORD  stripped and lower-cased, empty: None
        NATIVE  read by the library itself (getenv in csrc/, once per process): declared here, never read from Python
Default CALLER: the read site supplies it (it depends on the engine or the device). Switches read per `call` are live: a test
flips them between two calls of one process, nothing here caches a value. This module imports nothing but os (build.py and
lib.py read theirs before torch may be imported).
"""
import os
from collections import namedtuple

ON, ONLY1, INT, STR, WORD, NATIVE = "on", "only1", "int", "str", "word", "native"
CALLER = None
Switch = namedtuple("Switch", "name kind default read regions doc clamp", defaults=(None,))
_T, _R, _TR = ("train",), ("render",), ("train", "render")

TABLE = {s.name: s for s in (
    # ---- the sampler and the step preparation
    Switch("VDN_FUSE_ROUNDS", ON, "1", "import", _TR, "0: merge and up-sample of a sampler round as two launches (vdn_merge_upsample: one)"),
    Switch("VDN_FUSE_SDF_ROUNDS", ON, "1", "call", _TR, "0: a sampler round as SDF pass + merge/up-sample instead of one launch"),
    Switch("VDN_BG_COMPACT", ON, "1", "call", _TR, "0: every background sample is evaluated, as the reference does"),
    Switch("VDN_FG_COMPACT", ON, "1", "call", _T, "0: no foreground work list, every inside sample is evaluated"),
    Switch("VDN_RENDER_FG_COMPACT", ON, "1", "call", _T, "0: render()'s autograd node evaluates every sample (the Trainer keeps its list)"),
    Switch("VDN_FUSED_PREP", ON, "1", "call", _T, "0: the step preparation as separate launches instead of vdn_train_prep"),
    # ---- forward
    Switch("VDN_SHADE_FUSED", ON, "1", "call", _R, "0: inference shading as SDF kernel, colour head, compositor, eikonal reduce"),
    Switch("VDN_TRAIN_COLOR_FUSED", ONLY1, "0", "call", _T, "1: the colour head rides in the training SDF launch (slower on two streams)"),
    Switch("VDN_SDF_TAIL", ON, CALLER, "call", _T, "tail split of the fused SDF forward; default 1 without a side stream, 0 with one"),
    Switch("VDN_SDF_TAIL_ROW0", INT, CALLER, "call", _T, "first row the tail kernel may take; default 128 x the device's CU count"),
    Switch("VDN_SDF_TAIL_MAX", INT, 8192, "call", _T, "longest tail the split kernel takes, in rows"),
    Switch("VDN_SHADE_POINTS_FUSED", ON, "1", "call", (), "0: mesh vertices are shaded by the module calls instead of one launch per batch"),
    # ---- backward and the weight-gradient GEMM
    Switch("VDN_BWD_SPLIT_DW", ON, "1", "call", _T, "0: one weight-gradient GEMM behind the autograd node's whole backward"),
    Switch("VDN_SDF_BWD_SPLIT", ON, "1", "call", _T, "0: the SDF backward as sdf_rbar + sdf_fbar instead of one feature-split launch"),
    Switch("VDN_RELU_MASK", ON, "1", "construct", (), "0: bf16 ReLU chains read the saved planes instead of 1-bit masks"),
    Switch("VDN_DW_SPLIT_PTS", INT, 4096, "import", (), "rows per K split of the weight-gradient GEMM (the bf16 SDF group falls back to it, then 6144)"),
    Switch("VDN_DW_SPLIT_PTS_SDF", INT, CALLER, "construct", (), "... of the SDF group (vdn_hip.train._pts_per_split holds the fallback chain)"),
    Switch("VDN_DW_SPLIT_PTS_REST", INT, CALLER, "construct", (), "... of the rest group: the fp32 value, the bf16 fallback of _NERF / _HEADS"),
    Switch("VDN_DW_SPLIT_PTS_NERF", INT, CALLER, "construct", (), "... of the background network's launch (bf16)"),
    Switch("VDN_DW_SPLIT_PTS_HEADS", INT, CALLER, "construct", (), "... of the heads' launch (bf16)"),
    # ---- the Trainer's schedule and data parallelism
    Switch("VDN_SIDE_STREAM", ONLY1, "1", "construct", (), "anything but 1: the whole step on the caller's stream (kernel traces)"),
    Switch("VDN_OVERLAP", ON, "1", "construct", (), "0: the in-order step schedule"),
    Switch("VDN_SPLIT_REST", ON, "1", "call", (), "0: one rest-group GEMM instead of two halves"),
    Switch("VDN_EVENT_TRIM", ON, "1", "call", (), "0: every cross-stream event and wait is recorded"),
    Switch("VDN_FUSED_COMPOSITE", ON, "1", "call", (), "0: compositor, loss gradients and adjoint as separate launches"),
    Switch("VDN_DP_FUSED", ON, "1", "call", (), "0: at N > 1 the early eikonal all-reduce and the separate launches"),
    Switch("VDN_DP_SIDE_GROUP", ON, "1", "construct", (), "0: side-stream gradient slices on the one process group"),
    Switch("VDN_DP_INSTREAM", ON, "1", "construct", (), "0: every gradient sum goes through the backend's stream"),
    # ---- graphs, engines, precision
    Switch("VDN_RENDER_GRAPHS", ON, "1", "call", (), "0: render() under grad issues every launch from Python (no _TrainPlan)"),
    Switch("VDN_RENDER_GRAPH", ONLY1, "0", "call", (), "1: the image loops replay a captured RenderPlan"),
    Switch("VDN_RENDER_ENGINES", INT, 3, "call", (), "training engines kept per renderer", clamp=(1, 3)),
    Switch("VDN_PRECISION", WORD, "", "construct", (), "bf16 / fp32 for all four networks of a NeuSRenderer built without `precision`"),
    # ---- meshes
    Switch("VDN_MESH_METHOD", STR, "cubes", "call", (), "tets: marching tetrahedra"),
    Switch("VDN_MESH_SPARSE", STR, "", "call", (), "1 or brick:lipschitz: brick-sparse extraction (dpt_models.renderer.parse_sparse)"),
    # ---- development: another build of the library
    Switch("VDN_LIB", STR, "", "import", (), "path of the library to load; empty: the in-tree one"),
    Switch("VDN_BUILD_VARIANT", STR, "", "import", (), "name:-DFLAG..: vdn_hip.build makes a side copy of the library with extra flags"),
    # ---- read by the library
    Switch("VDN_SDF2_WARM", NATIVE, "1", "import", (), "0: no L2 warm-up of cold weight streams"),
    Switch("VDN_PLANE_PREFETCH", NATIVE, "2", "import", (), "1: the SDF backward prefetches one chunk step instead of two"),
    Switch("VDN_SDF0_SPLIT_MAX", NATIVE, "8192", "import", (), "sdf-only launches up to this many points use the feature-split kernel"),
)}

_REGIONS = {r: tuple(s.name for s in TABLE.values() if r in s.regions) for r in ("train", "render")}
_FLAGS = {s.name: (s.default, s.kind == ONLY1) for s in TABLE.values() if s.kind in (ON, ONLY1)}
_get = os.environ.get


def flag(name, default=CALLER):
    """An ON / ONLY1 switch -> bool. KeyError: `name` is not a declared flag."""
    dflt, only1 = _FLAGS[name]
    v = _get(name, dflt if default is None else default)
    if v is None:
        raise TypeError("%s has no default of its own: the caller supplies one" % name)
    return v == "1" if only1 else v != "0"


def raw(name, default=CALLER):
    """The string in the environment, else the caller's default, else the table's (unparsed: the fallback chains)."""
    s = TABLE[name]
    if s.kind == NATIVE:
        raise KeyError("%s is read by the library itself, not from Python" % name)
    v = _get(name, s.default if default is None else default)
    if v is None:
        raise TypeError("%s has no default of its own: the caller supplies one" % name)
    return v


def integer(name, default=CALLER):
    s = TABLE[name]
    if s.kind != INT:
        raise KeyError("%s is not an int switch" % name)
    if s.clamp is None:
        return int(raw(name, default))
    return min(s.clamp[1], max(s.clamp[0], int(raw(name, default) or s.default)))


def text(name):
    s = TABLE[name]
    if s.kind not in (STR, WORD):
        raise KeyError("%s is not a string switch" % name)
    return raw(name) if s.kind == STR else raw(name).strip().lower() or None


def signature(region):
    """The raw environment strings (None: unset) of the switches that select launches in `region`, in table order."""
    return tuple(map(_get, _REGIONS[region]))
