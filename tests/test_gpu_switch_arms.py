"""Every shipped arm of the run-time switch table runs, and equals the default arm (tests/switch_arms.py: the ledger ARMS, the
scenarios, the `taken` predicates; tests/test_switch_arms_cpu.py holds the ledger to vdn_hip/switches.py).

For every row of ARMS with held_by = "matrix" and every value of it: the row's scenarios on the default arm, then under the arm;
`taken` (the arm ran and was not silently the default); then the relation.
  * arms read per call or when an object is built: in this process, the variable set in front of the scenario (which builds its
    renderer, engine and Trainer itself);
  * arms read at import or by the library itself: ONE switch per fresh child, `python -m switch_arms SCENARIO OUT.npz`, against the
    default environment's child of the same scenario (one per scenario and module);
  * the library's own three also run the existing fp64 plane tests under the arm in a child pytest, which must pass as many tests as
    the same selection collects;
  * the data-parallel switches: the one-rank child of tests/test_gpu_dp.py (four steps in lockstep with a Trainer without
    collectives, bit for bit) under the arm.

Relations. "bits": torch.equal on every returned tensor, every tensor finite. "rounding" (the K-split partition of the
weight-gradient GEMM, vdn_hip/train.py:204-206): the first step's scalars bit for bit - they are formed before the weight-gradient
GEMMs; the later steps' follow parameters that already differ in their last bits and are held finite - every gradient tensor of step
1 to max|d| <= 2e-5 max|default| + 1e-12 (the bound of tests/test_gpu_heads_inside_list.py for the same class of difference: the same
fp32-accumulated products in another split order), the parameters after the last step to |d| < 1e-3 |default| (the bound that file
takes from tests/test_gpu_train_parity.py). Where a gradient tensor misses the first bound, the bound is not widened: both arms are
measured against the fp64 oracle's gradients (_gpu_grads and _oracle_grads of tests/test_gpu_grads.py, on the step scenarios' rays), and the arm may stand at most
2 x as far from fp64 as the default arm does, per tensor - a reordering of the same terms cannot double the error unless terms are
lost. VDN_MESH_METHOD=tets is another triangulation: bit for bit extract_geometry(method="tets"),
the default bit for bit method="cubes". VDN_PRECISION=bf16 as a default: bit for bit the renderer built with precision="bf16".

Children. One at a time, each under its own timeout = 3 x the wall time below + 60 s (interpreter, torch, the library). A child that
ends by a signal, by exit status 124 / 134 / 137 / 139 or by the timeout sets a module flag: every later test of this module fails at
once and starts nothing. Nothing is retried.

Wall times, one MI355X, default environment, measured once in one run of this file (the whole child, python start to exit):
    python -m switch_arms step_bf16              2.2 s        render_inf   2.4 s
    python -m switch_arms step_fp32              2.2 s        step_bf16_two_chain   2.2 s
    the one-rank data-parallel child             6.6 s (the arms: 3.6 - 4.2 s)
    pytest --collect-only of a selection         3.3 - 4.0 s
    the fp64 selections under their arm          9.9 s (VDN_PLANE_PREFETCH=1, 38 tests), 5.4 s (VDN_SDF2_WARM=0, 17),
                                                 5.5 s (VDN_SDF0_SPLIT_MAX=0, 74)
The whole file: 37 tests in 88 s, the in-process cases 0.02 - 0.5 s each.

What the matrix exposed (one split of the fp32 weight-gradient GEMM, and the kernel fix) is in DESIGN.md, "Switch-arm matrix: record".
"""
import os
import re
import subprocess
import sys
import time

import pytest
import torch

import switch_arms as sa
from switch_arms import ARMS
from vdn_hip import switches

pytestmark = pytest.mark.gpu

# seconds, the whole child in the default environment (the module docstring's measurements)
WALL = {"step_bf16": 2.2, "step_fp32": 2.2, "step_bf16_two_chain": 2.2, "render_inf": 2.4, "dp_one_rank": 6.6,
        "fp64/VDN_PLANE_PREFETCH": 9.9, "fp64/VDN_SDF2_WARM": 5.4, "fp64/VDN_SDF0_SPLIT_MAX": 5.5, "collect": 4.0}

FAULT_STATUS = (124, 134, 137, 139)
_DEAD = []
DEV = torch.device("cuda:0")


def _timeout(key):
    return 3.0 * WALL[key] + 60.0


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _DEAD:
        pytest.fail("a child of this module faulted, hung or was killed (%s): nothing more is started" % _DEAD[0])


def _clean_env(**arm):
    # (VDN_LIB / VDN_BUILD_VARIANT stay: a suite run against a side build tests that build in its children too)
    env = {k: v for k, v in os.environ.items() if k not in switches.TABLE or ARMS[k]["held_by"] is None}
    env.update(arm)
    return env


def _ended_badly(what, code):
    """code: the child's exit status, None = it outlived its timeout."""
    if code is None or code < 0 or code in FAULT_STATUS:
        _DEAD.append("%s: %s" % (what, "timeout" if code is None else "exit status %d" % code))
        pytest.fail("child %s ended by %s" % (what, "its timeout" if code is None else "status %d" % code))


def _child(what, cmd, env, timeout, cwd):
    t0 = time.time()
    try:
        p = subprocess.run(cmd, env=env, timeout=timeout, capture_output=True, text=True, cwd=cwd)
    except subprocess.TimeoutExpired:
        _ended_badly(what, None)
    print("child %s: %.1f s, exit status %d" % (what, time.time() - t0, p.returncode))
    _ended_badly(what, p.returncode)
    return p


def _scenario_child(scenario, arm, folder):
    tag = "-".join([scenario] + ["%s=%s" % kv for kv in arm.items()]) or scenario
    path = os.path.join(folder, tag + ".npz")
    p = _child(tag, [sys.executable, "-m", "switch_arms", scenario, path], _clean_env(**arm), _timeout(scenario), sa.TESTS)
    assert p.returncode == 0, (tag, p.stdout[-1500:], p.stderr[-3000:])
    return sa.load(path)


def _check_scene(scenario, obs):
    """The step scenarios' precondition: both work lists strict, non-empty subsets, the foreground list with both classes."""
    if scenario.startswith("step_"):
        assert 0 < obs["fg_inner"] < obs["fg_listed"] < obs["P"] and 0 < obs["bg_listed"] < obs["Q"], obs
        assert obs["side"] and obs["overlap"], obs


class _Defaults:
    """The default arm of each scenario, run once per module: in this process, or as a fresh child."""

    def __init__(self, folder):
        self.folder, self.here, self.child = folder, {}, {}

    def in_process(self, scenario):
        if scenario not in self.here:
            assert not [k for k in switches.TABLE if k in os.environ and ARMS[k]["held_by"] is not None]
            self.here[scenario] = sa.run(scenario, DEV)
            _check_scene(scenario, self.here[scenario][1])
        return self.here[scenario]

    def in_child(self, scenario):
        if scenario not in self.child:
            self.child[scenario] = _scenario_child(scenario, {}, self.folder)
            _check_scene(scenario, self.child[scenario][1])
        return self.child[scenario]


@pytest.fixture(scope="module")
def defaults(tmp_path_factory):
    return _Defaults(str(tmp_path_factory.mktemp("switch_arms")))


@pytest.fixture
def clean(monkeypatch):
    for name in switches.TABLE:
        if ARMS[name]["held_by"] is not None:            # (not VDN_LIB / VDN_BUILD_VARIANT: which build is under test)
            monkeypatch.delenv(name, raising=False)
    return monkeypatch


# ------------------------------------------------------------------------------------------------------------------------
# relations
# ------------------------------------------------------------------------------------------------------------------------
def _finite(t):
    return bool(torch.isfinite(t).all()) if t.is_floating_point() else True


def _bits(got, ref, what, keys=None):
    if keys is None:
        assert set(got) == set(ref), (what, sorted(set(got) ^ set(ref)))
        keys = sorted(ref)
    assert len(keys) > 0, what
    for k in keys:
        assert _finite(got[k]) and _finite(ref[k]), (what, k, "not finite")
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, ref[k].shape)
        assert torch.equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), float((got[k].double() - ref[k].double()).abs().max()))


_ORACLE = {}


def _grads_fixture(wdepth):
    """A fixture in the format of tests/test_gpu_grads.py (what its _gpu_grads and _oracle_grads take) on the rays of the step
    scenarios' first step: the golden fixtures of that file hold 16 - 24 rays, at most two K splits at the default, where these
    160 rays' 20 480 rows make ten (fp32) - the partitions that missed the bound. z is the sampler's (a no-grad stage), injected into both sides."""
    if wdepth not in _ORACLE:
        import stream_skew as sk
        import test_gpu_grads as tg
        from vdn_train import synth, factory
        seed, B = 11, sk.B
        o, d = synth.random_pixel_batch(seed, 0, 0, B, cams=synth.make_cameras(seed))
        near, far = synth.near_far_from_sphere(o, d)
        t1, t2 = synth.jitter(seed, 0, B)
        rend = factory.build_renderer(wdepth=wdepth, device=DEV, states=synth.make_all_states(seed, wdepth=wdepth, variance=0.3))
        with torch.no_grad():
            z, _ = rend._sample(*(tg.g(x, DEV) for x in (o, d, near.reshape(-1), far.reshape(-1))), 1.0, tg.g(t1, DEV), tg.g(t2, DEV), None)
        fx = dict(wdepth=wdepth, seed=seed, variance=0.3, n_importance=64, rays_o=o, rays_d=d, near=near, far=far, perturb=1.0, white=True,
                  cos_anneal=0.5, t_rand=t1, t_rand_out=t2, z_vals_inside=z.cpu().numpy(), true_rgb=synth.target_colors(o, d, 0.5),
                  gt_feats=synth.uniform(seed, "T2/feats", (B, 96)).astype("float32"))
        _ORACLE[wdepth] = (fx, tg._oracle_grads(fx, torch.float64)[1])
    return _ORACLE[wdepth]


def _fp64_distances(name, value, precision, wdepth):
    """Where an arm misses the bound against the default arm: both arms against the fp64 oracle's gradients, with the functions
    of tests/test_gpu_grads.py (_gpu_grads: render() under grad + loss.backward() on the kernels; _oracle_grads: the oracle's autograd
    in float64) -> [(tensor name, max|default - fp64|, max|arm - fp64|)] in parameter order. In this process: the arm must be
    one that is read when an engine is built."""
    import stream_skew as sk
    import test_gpu_grads as tg
    assert switches.TABLE[name].read == "construct", name
    (fx, ref), grads = _grads_fixture(wdepth), []
    held = os.environ.pop(name, None)              # (the test's own setting of the arm: the first run is the default arm)
    try:
        for env in ({}, {name: value}):
            with sk.environ(**env):
                _, named, _ = tg._gpu_grads(fx, DEV, precision=precision)
            grads.append([(n, p.grad.detach().cpu().double()) for n, p in named])
    finally:
        if held is not None:
            os.environ[name] = held
    assert any(not torch.equal(a, b) for (_, a), (_, b) in zip(*grads)), "the arm changed no gradient of the fixture"
    return [(n, float((a - ref[n].double()).abs().max()), float((b - ref[n].double()).abs().max())) for (n, a), (_, b) in zip(*grads)]


def _rounding(got, ref, obs, what, arm=None):
    assert set(got) == set(ref), what
    for k in got:
        assert _finite(got[k]), (what, k)
    assert torch.equal(got["scalars/0"], ref["scalars/0"]), (what, got["scalars/0"].tolist(), ref["scalars/0"].tolist())
    sizes = obs["param_sizes"]
    assert sum(sizes) == got["grad_flat"].numel() == ref["grad_flat"].numel()
    worst, missed = 0.0, []
    for i, (a, b) in enumerate(zip(torch.split(got["grad_flat"], sizes), torch.split(ref["grad_flat"], sizes))):
        d, bound = float((a - b).abs().max()), 2e-5 * float(b.abs().max()) + 1e-12
        worst = max(worst, d / bound)
        if d > bound:
            missed.append((i, d, bound))
    if missed:
        # not a wider bound: both arms against fp64. A reordering of the same terms cannot double the error unless terms are lost:
        # per tensor, the arm may stand at most 2x as far from the fp64 gradient as the default arm does
        print("%s: gradient tensors beyond 2e-5 of the default's largest entry: %s" % (what, missed))
        assert arm is not None and switches.TABLE[arm[0]].read == "construct", (what, missed)
        dist = _fp64_distances(arm[0], arm[1], obs["precision"], obs["wdepth"])
        for n, d0, d1 in dist:
            print("%s: fp64 fixture %-40s default %.3e  arm %.3e  ratio %.3f" % (what, n, d0, d1, d1 / d0 if d0 else float(d1 > 0)))
        bad = sa.further_than_twice(dist)
        assert not bad, (what, "further than 2x the default arm from the fp64 gradients", bad, "missed against the default arm", missed)
    assert float(ref["grad_flat"].abs().max()) > 0
    a, b = got["param_flat"].double(), ref["param_flat"].double()
    rel = float((a - b).norm() / b.norm())
    print("%s: worst gradient tensor at %.3f of its bound, %d of %d gradient elements differ, parameters %.2e of their norm apart"
          % (what, worst, int((got["grad_flat"] != ref["grad_flat"]).sum()), ref["grad_flat"].numel(), rel))
    assert rel < 1e-3, (what, rel)


def _relate(name, value, scenario, got, ref, obs):
    what = "%s=%s %s" % (name, value, scenario)
    if name == "VDN_MESH_METHOD":
        for part in ("vertices", "faces"):
            assert torch.equal(got["env/" + part], got[value + "/" + part]), (what, part)
            assert torch.equal(ref["env/" + part], ref["cubes/" + part]), (what, part)
        assert got["env/faces"].shape != ref["env/faces"].shape or not torch.equal(got["env/faces"], ref["env/faces"])
        _bits(got, ref, what, [k for k in sorted(ref) if not k.startswith("env/")])
    elif name == "VDN_PRECISION":
        env = [k for k in sorted(ref) if k.startswith("env/")]
        _bits({k: got[k] for k in env}, {k: ref[value + k[3:]] for k in env}, what + " (against precision=%r)" % value)
        _bits({k: ref[k] for k in env}, {k: ref["fp32" + k[3:]] for k in env}, what + " (unset: the networks' own fp32)")
        _bits(got, ref, what, [k for k in sorted(ref) if not k.startswith("env/")])
    elif ARMS[name]["relation"] == "rounding":
        _rounding(got, ref, obs, what, (name, value))
    else:
        _bits(got, ref, what)


def _cases(how):
    return [(n, v, s) for n, r in ARMS.items() if r["held_by"] == "matrix" and r["how"] == how for v in r["values"] for s in r["scenario"]]


def _ids(cases):
    return ["%s=%s-%s" % c for c in cases]


# ------------------------------------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------------------------------------
_HERE = _cases("monkeypatch")


@pytest.mark.parametrize("name,value,scenario", _HERE, ids=_ids(_HERE))
def test_arm_read_per_call_or_at_construction(clean, defaults, name, value, scenario):
    ref, ref_obs = defaults.in_process(scenario)
    clean.setenv(name, value)
    got, obs = sa.run(scenario, DEV)
    assert ARMS[name]["taken"](value, obs, ref_obs), (name, value, {k: v for k, v in obs.items() if not k.startswith("log")})
    _relate(name, value, scenario, got, ref, obs)


_CHILD = _cases("child")


@pytest.mark.parametrize("name,value,scenario", _CHILD, ids=_ids(_CHILD))
def test_arm_read_at_import_or_by_the_library(defaults, name, value, scenario):
    ref, ref_obs = defaults.in_child(scenario)
    got, obs = _scenario_child(scenario, {name: value}, defaults.folder)
    taken = ARMS[name]["taken"]
    if taken is None:
        # the library reads it (ARMS[name]["native"]): same launches from Python, whatever kernel they picked
        assert switches.TABLE[name].kind == switches.NATIVE and obs["log"] == ref_obs["log"]
    else:
        assert taken(value, obs, ref_obs), (name, value, {k: v for k, v in obs.items() if not k.startswith("log")})
    _relate(name, value, scenario, got, ref, obs)


_FP64 = sorted(sa.FP64_UNDER_ARM)


@pytest.mark.parametrize("name,value", _FP64, ids=["%s=%s" % c for c in _FP64])
def test_fp64_plane_tests_pass_under_the_library_arm(name, value):
    """Bit equality with the default says the arm is no worse, not that it is right: the existing fp64 tests of the kernels the
    arm selects, in a child pytest under the arm. It must pass exactly the tests the selection collects."""
    sel = sa.FP64_UNDER_ARM[(name, value)]
    col = _child("collect " + name, [sys.executable, "-m", "pytest", "--collect-only", "-q"] + sel, _clean_env(), _timeout("collect"), sa.ROOT)
    assert col.returncode == 0, col.stdout[-2000:]
    want = len([l for l in col.stdout.splitlines() if "::" in l])
    assert want > 0, col.stdout[-2000:]
    p = _child("fp64 under %s=%s" % (name, value), [sys.executable, "-m", "pytest", "-q", "-x"] + sel, _clean_env(**{name: value}),
               _timeout("fp64/" + name), sa.ROOT)
    tail = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    assert p.returncode == 0, (p.stdout[-4000:], p.stderr[-2000:])
    m = re.search(r"\b(\d+) passed\b", tail)
    assert m and int(m.group(1)) == want and not re.search(r"skipped|failed|error|xfailed|xpassed", tail), (want, tail)


@pytest.fixture(scope="module")
def dp_default():
    old = {k: os.environ.pop(k) for k in switches.TABLE if k in os.environ and ARMS[k]["held_by"] is not None}
    try:
        return _dp("default")
    finally:
        os.environ.update(old)


def _dp(what):
    t0 = time.time()
    code, res, obs = sa.dp_one_rank("nccl", timeout=_timeout("dp_one_rank"))
    print("child dp_one_rank %s: %.1f s, exit status %s" % (what, time.time() - t0, code))
    _ended_badly("dp_one_rank " + what, code)
    assert code == 0 and res is not None, (what, code)
    same, loss, gmax = res
    assert same and loss == loss and abs(loss) != float("inf") and gmax > 0, (what, res)       # bit for bit, every step
    return obs


_DP = [(n, v) for n, v, _ in _cases("dp_child")]


@pytest.mark.parametrize("name,value", _DP, ids=["%s=%s" % c for c in _DP])
def test_data_parallel_arm_on_a_one_rank_group(clean, dp_default, name, value):
    clean.setenv(name, value)
    obs = _dp("%s=%s" % (name, value))
    assert ARMS[name]["taken"](value, obs, dp_default), (name, {k: v for k, v in obs.items() if k != "log"})
