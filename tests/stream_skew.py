"""Stream-skew harness for the training step's four-stream schedule (tests/test_gpu_stream_order.py holds the assertions and the
hand-over table this enforces).

Every launch of the package goes through vdn_hip.lib.call / lib.try_call with the raw stream handle as its last positional
argument. `Skew` replaces the two for its duration: it logs (step, entry point, stream role) per launch and, in front of every launch
a rule (role, entry point or None) selects, enqueues ONE torch.cuda._sleep(cycles) on that launch's own stream - one workgroup, no
data, no host synchronisation. A consumer that is not ordered behind a delayed producer then overtakes it with certainty instead
of losing the race at natural timing.

The delay D = max(2 T_step, 1 ms): T_step is one whole un-delayed step of the configuration's serial arm (events around its third
step), so everything the other streams can do before they reach an unordered consumer fits inside one delay. cycles per ms of the
delay kernel are measured once per process. Both scale the tool; neither is a pass bar.

An "arm" is one Trainer (or renderer) built from torch.manual_seed(0), stepped S times on inputs uploaded beforehand; nothing
inside an arm synchronises the host except the serial arm, which does so after every step. `run_case(spec)` -> a dict of CPU tensors,
either called in-process or, when the process's streams do not run concurrently (two of them on one hardware queue), by `main()`
in ONE fresh child process that creates the four streams first and leaves every case's result on disk."""
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vdn-nerf_amd")
for _p in (PKG, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

S = 6                    # steps per arm
B = 160                  # rays per step: full-frame pixels, both work lists strict non-empty subsets (asserted by the tests)
DROPIN_CALLS = 3
ROLES = ("main", "side", "side2", "log")

_DEPTH = dict(extract_depth=True, depth_start_iter=2)           # the depth term (and its Adam ranges) switch on at step 3
_BASE = dict(warm_up_end=4, end_iter=300, anneal_end=40)
CONFIGS = {
    "T1": dict(precision="bf16", wdepth=False, conf={}, roles=("main", "side", "log")),
    "T2": dict(precision="bf16", wdepth=True, conf=_DEPTH, roles=ROLES),
    "T3": dict(precision="fp32", wdepth=True, conf=_DEPTH, roles=ROLES),
    "T4": dict(precision="bf16", wdepth=False, conf=dict(mask_weight=0.1), mask=True, roles=("main", "side")),
    "T5": dict(precision="bf16", wdepth=False, conf={}, user_stream=True, roles=("main", "side", "log")),
    # learnable cameras: steps 0-2 are fixed-pose steps (side-stream halves pending), steps 3-5 pose steps
    "T6": dict(precision="bf16", wdepth=False, conf=dict(start_refine_pose_iter=2), pose=True, roles=("main", "side", "log")),
}
# schedule switches (T2): environment of both arms / the Trainer's overlap flag. VDN_SPLIT_REST, VDN_FUSED_PREP and overlap select
# LAUNCHES as well as streams (one rest-group GEMM or two, seven preparation launches or one), so the serial arm carries them too
SWITCHES = {"trim0": dict(env={"VDN_EVENT_TRIM": "0"}), "split0": dict(env={"VDN_SPLIT_REST": "0"}),
            "ovl0": dict(env={}, overlap=False), "prep0": dict(env={"VDN_FUSED_PREP": "0"})}

DEV = torch.device("cuda:0")
_STATE = {}


def dev_streams():
    """{role: torch stream} of the package's shared streams, created in this order (the user stream of the user-stream
    configuration is chosen by concurrency_precondition)."""
    from vdn_hip.train import shared_stream
    if "streams" not in _STATE:
        _STATE["streams"] = {r: shared_stream(DEV, r) for r in ("side", "side2", "log")}
    return _STATE["streams"]


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------------------
# calibration and the concurrency precondition
# ------------------------------------------------------------------------------------------------------------------------
def cycles_per_ms():
    """Cycles of torch.cuda._sleep per millisecond, from event timing (once per process)."""
    if "cpm" not in _STATE:
        n, ms = 1_000_000, 0.0
        torch.cuda._sleep(n)                     # (the first launch loads the kernel)
        torch.cuda.synchronize()
        for _ in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 4.0:
                break
            n *= 4
        assert ms >= 0.5, ("the delay kernel does not delay", n, ms)
        _STATE["cpm"] = n / ms
    return _STATE["cpm"]


def _overtakes(sa, sb, cyc, x):
    """A delay on stream sa, then a trivial kernel and an event on sb: did sb's event complete while the delay was still running?"""
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(sa):
        torch.cuda._sleep(cyc)
        ea.record(sa)
    with torch.cuda.stream(sb):
        x.add_(1.0)
        eb.record(sb)
    while not eb.query() and not ea.query():      # (bounded by the delay kernel)
        pass
    ok = bool(eb.query() and not ea.query())
    sa.synchronize()
    sb.synchronize()
    return ok


def concurrency_precondition():
    """For every ordered pair (A, B) of the streams an arm uses - (default, side, side2, log) and, for the user-stream configuration,
    (user, side, side2, log) - a delay on A, then a trivial kernel and an event on B: B's event must complete while A's delay is
    still running. -> {"A>B": True / False}. (Two streams on one hardware queue serialise, and a skew between them would do nothing.)
    Every stream has launched once before it is checked (a stream's first launch sets up its queue). HIP maps streams onto four
    hardware queues, so a fifth stream shares one: the user stream is the first of up to eight new streams that overtakes and is
    overtaken by side, side2 and log (it then shares the default stream's queue, which is idle in that configuration)."""
    if "pairs" in _STATE:
        return _STATE["pairs"]
    st = dev_streams()
    cyc = int(20.0 * cycles_per_ms())
    x = torch.zeros(64, device=DEV)

    def warm(s):
        with torch.cuda.stream(s):
            x.add_(1.0)
        s.synchronize()

    def check(group, only=""):
        return {"%s>%s" % (a, b): _overtakes(sa, sb, cyc, x) for a, sa in group.items() for b, sb in group.items()
                if a != b and only in (a, b, "")}
    group = dict(main=torch.cuda.default_stream(DEV), side=st["side"], side2=st["side2"], log=st["log"])
    for s in group.values():
        warm(s)
    torch.cuda.synchronize()
    pairs = check(group)
    for _ in range(8):
        user = torch.cuda.Stream(device=DEV)
        warm(user)
        got = check(dict(user=user, side=st["side"], side2=st["side2"], log=st["log"]), only="user")
        if all(got.values()):
            break
    st["user"] = user
    pairs.update(got)
    _STATE["pairs"] = pairs
    return pairs


# ------------------------------------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------------------------------------
class Skew:
    """with Skew(main_stream, rule, cycles) as h: ... h.step = i ...; h.log = [(step, entry point, role)]."""

    def __init__(self, main, rule=None, cycles=0):
        self.main, self.rule, self.cycles = main, rule, int(cycles)
        self.log, self.step, self.delays = [], 0, 0

    def _resolve(self, handle):
        from vdn_hip import train
        if not isinstance(handle, int) and handle is not None:
            return "other", None
        handle = handle or 0
        if handle == self.main.cuda_stream:
            return "main", self.main
        for (d, role), s in train._SHARED_STREAMS.items():
            if d == DEV.index and s.cuda_stream == handle:
                return role, s
        return "other", None

    def _before(self, fn_name, args):
        role, stream = self._resolve(args[-1] if args else None)
        if self.rule is not None and role == self.rule[0] and self.rule[1] in (None, fn_name):
            with torch.cuda.stream(stream):
                torch.cuda._sleep(self.cycles)
            self.delays += 1
        return role

    def __enter__(self):
        from vdn_hip import lib
        self._lib, self._call, self._try = lib, lib.call, lib.try_call

        def call(fn_name, *args):
            role = self._before(fn_name, args)
            self._call(fn_name, *args)
            self.log.append((self.step, fn_name, role))

        def try_call(fn_name, *args, **kw):
            role = self._before(fn_name, args)
            done = self._try(fn_name, *args, **kw)
            if done:                                  # (a declined shape launched nothing)
                self.log.append((self.step, fn_name, role))
            return done
        lib.call, lib.try_call = call, try_call
        return self

    def __exit__(self, *exc):
        self._lib.call, self._lib.try_call = self._call, self._try
        return False


# ------------------------------------------------------------------------------------------------------------------------
# inputs (uploaded before an arm starts: a host-to-device copy from pageable memory synchronises)
# ------------------------------------------------------------------------------------------------------------------------
def _g(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()


def _step_inputs(seed, steps, tag, feats=False, mask=False):
    from vdn_train import synth
    cams = synth.make_cameras(seed)
    out = []
    for it in range(steps):
        o, d = synth.random_pixel_batch(seed, it, it % 40, B, cams=cams)           # full-frame pixels: no crop
        near, far = synth.near_far_from_sphere(o, d)
        t1, t2 = synth.jitter(seed, it, B)
        out.append(dict(args=[_g(o), _g(d), _g(near), _g(far), _g(synth.target_colors(o, d, 0.5))], t_rand=_g(t1), t_rand_out=_g(t2)))
    extra = {}
    if feats:
        extra["gt_feats"] = _g(synth.uniform(seed, tag + "/feats", (B, 96)))
    if mask:
        extra["mask"] = _g((synth.uniform(seed, tag + "/mask", (B, 1)) > 0.5).astype(np.float32))
    return out, extra


def _pose_scene():
    """The resident images, cameras and intrinsics of the learnable-camera configuration (read-only: shared by its arms)."""
    if "pose_scene" not in _STATE:
        from vdn_train import synth
        from vdn_train.rays import RaysGenerator
        from dpt_models.poses import LearnIntrin
        n, H, W = 2, 800, 800
        cams = np.asarray(synth.make_cameras(6)[:n], np.float32)
        intr = LearnIntrin(H, W, req_grad=True, order=2, init_focal=torch.tensor(1111.0)).to(DEV)
        images = synth.uniform(6, "pose/images", (n, H, W, 3)).astype(np.float32)
        fixed = RaysGenerator(images, None, cams, intr().detach().cpu().numpy(), device=DEV)
        r0 = torch.tensor((synth.uniform(6, "pose/r0", (n, 3)) - 0.5).astype(np.float32) * 0.02)
        t0 = torch.tensor((synth.uniform(6, "pose/t0", (n, 3)) - 0.5).astype(np.float32) * 0.04)
        px = [_g(np.floor(synth.uniform(6, "pose/px/%d" % it, (B,)) * W)) for it in range(S)]
        py = [_g(np.floor(synth.uniform(6, "pose/py/%d" % it, (B,)) * H)) for it in range(S)]
        jit = [tuple(_g(t) for t in synth.jitter(6, it, B)) for it in range(S)]
        _STATE["pose_scene"] = (cams, intr, fixed, r0, t0, px, py, jit)
    return _STATE["pose_scene"]


def _rule(arm):
    """arm: "ref" | "none" | a role | "role:entry_point" (the narrowed form) -> rule or None."""
    if arm in ("ref", "none"):
        return None
    role, _, fn = arm.partition(":")
    assert role in ROLES, arm
    return (role, fn or None)


def _cpu(t):
    return t.detach().clone().cpu()


# ------------------------------------------------------------------------------------------------------------------------
# arms of the Trainer's step
# ------------------------------------------------------------------------------------------------------------------------
def train_arm(cfg_name, arm, switch=None, steps=S, no_forward_join=False, between_steps=None, env_extra=None):
    """One arm of configuration `cfg_name`: "ref" = the serial arm (VDN_SIDE_STREAM=0, the logging launches on the caller's stream
    as well, torch.cuda.synchronize() after every step), else the shipped schedule under the rule of `arm`.
    no_forward_join: TrainEngine._join clears _pending WITHOUT waiting during forward() (the harness-bites case only).
    between_steps(tr, it): called in front of every step it = 0 .. steps-1 and once more behind the last one (it = steps), on the arm's
    stream (tests/test_gpu_workspace_poison.py: it joins, snapshots and poisons there). env_extra: more switches for both arms."""
    from vdn_train import factory
    from vdn_train.trainer import Trainer
    from vdn_hip.train import TrainEngine
    cfg, sw = CONFIGS[cfg_name], SWITCHES.get(switch, dict(env={}))
    serial = arm == "ref"
    env = dict(VDN_SDF_TAIL="0", VDN_SIDE_STREAM="0" if serial else "1")
    env.update(sw["env"])
    env.update(env_extra or {})
    cycles = 0
    if _rule(arm) is not None:
        cycles = int(run_case(ref_spec(dict(kind="train", cfg=cfg_name, switch=switch)))["D_ms"] * cycles_per_ms())
    streams = dev_streams()
    main = streams["user"] if cfg.get("user_stream") else torch.cuda.default_stream(DEV)
    conf = dict(_BASE)
    conf.update(cfg["conf"])
    with environ(**env):
        torch.manual_seed(0)
        rend = factory.build_renderer(wdepth=cfg["wdepth"], device=DEV, precision=cfg["precision"])
        cameras = None
        if cfg.get("pose"):
            from dpt_models.poses import LearnPose, LearnableRays
            cams, intr, fixed, r0, t0, px, py, jit = _pose_scene()
            pn = LearnPose(len(cams), True, True, init_c2w=torch.tensor(cams)).to(DEV)
            with torch.no_grad():
                pn.r.copy_(r0)
                pn.t.copy_(t0)
            cameras = LearnableRays(pn, intr, fixed)
        else:
            inputs, extra = _step_inputs(11, steps, cfg_name, feats=cfg["wdepth"], mask=cfg.get("mask", False))
        tr = Trainer(rend, B, DEV, conf=conf, overlap=sw.get("overlap", True), cameras=cameras)
        assert (tr.engine._side is None) == serial
        if serial:
            tr._log_stream = main          # (the loss scalars' launches: on the caller's stream too, behind an event of that stream)
        torch.cuda.synchronize()
        scalars, counts, t_step = [], None, None
        orig_fwd, orig_join = TrainEngine.forward, TrainEngine._join
        if no_forward_join:
            def fwd(self, *a, **k):
                TrainEngine._join = lambda eng: setattr(eng, "_pending", False)
                try:
                    return orig_fwd(self, *a, **k)
                finally:
                    TrainEngine._join = orig_join
            TrainEngine.forward = fwd
        try:
            with torch.cuda.stream(main), Skew(main, _rule(arm), cycles) as h:
                for it in range(steps):
                    h.step = it
                    if between_steps is not None:
                        between_steps(tr, it)
                    if serial and it == 2:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                    if cfg.get("pose"):
                        sc = tr.train_step_at(it % len(cams), px[it], py[it], t_rand=jit[it][0], t_rand_out=jit[it][1])
                    else:
                        x = inputs[it]
                        sc = tr.train_step(*x["args"], t_rand=x["t_rand"], t_rand_out=x["t_rand_out"], **extra)
                    scalars.append(sc.clone())           # on the caller's stream, no join
                    if serial:
                        if it == 2:
                            e1.record()
                        torch.cuda.synchronize()
                        if it == 2:
                            t_step = e0.elapsed_time(e1)
                        if it == 0:
                            w = tr.engine.w
                            counts = [int(w["fg_active"][1].item()), tr.engine.P, int(w["bg_active"][1].item()), tr.engine.Q]
                if between_steps is not None:
                    between_steps(tr, steps)
                torch.cuda.synchronize()
                res = dict(scalars=_cpu(torch.stack(scalars)), param_flat=_cpu(tr.param_flat), exp_avg=_cpu(tr.exp_avg),
                           exp_avg_sq=_cpu(tr.exp_avg_sq), grad_flat=_cpu(tr.engine.grad_flat), log=list(h.log), delays=h.delays)
                if cfg.get("pose"):
                    res["pose_flat"] = _cpu(tr._pose_flat)
        finally:
            TrainEngine.forward, TrainEngine._join = orig_fwd, orig_join
    if serial:
        res["counts"], res["T_step_ms"] = counts, t_step
        res["D_ms"] = max(2.0 * t_step, 1.0) if t_step is not None else None
    res["cycles"] = cycles
    return res


# ------------------------------------------------------------------------------------------------------------------------
# arms of the drop-in flow: NeuSRenderer.render under grad + loss.backward(), eager
# ------------------------------------------------------------------------------------------------------------------------
def dropin_arm(wdepth, split_dw, arm, between_steps=None, env_extra=None, calls=DROPIN_CALLS):
    """between_steps(rend, it): as train_arm's, with the renderer, in front of every call and once behind the last."""
    from vdn_train import factory
    serial = arm == "ref"
    env = dict(VDN_RENDER_GRAPHS="0", VDN_SDF_TAIL="0", VDN_SIDE_STREAM="0" if serial else "1")
    if not split_dw:
        env["VDN_BWD_SPLIT_DW"] = "0"
    env.update(env_extra or {})
    cycles = 0
    if _rule(arm) is not None:
        cycles = int(run_case(ref_spec(dict(kind="dropin", wdepth=wdepth, split_dw=split_dw)))["D_ms"] * cycles_per_ms())
    main = torch.cuda.default_stream(DEV)
    inputs, extra = _step_inputs(13, calls, "dropin", feats=wdepth)
    bg = torch.ones(1, 3, device=DEV)
    with environ(**env):
        torch.manual_seed(0)
        rend = factory.build_renderer(wdepth=wdepth, device=DEV, precision="bf16")
        params = rend._all_parameters()
        torch.cuda.synchronize()
        outs, grads, t_step = [], [], None
        with torch.cuda.stream(main), Skew(main, _rule(arm), cycles) as h:
            for it in range(calls):
                h.step = it
                if between_steps is not None:
                    between_steps(rend, it)
                if serial and it == 1:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                o, d, near, far, rgb = inputs[it]["args"]
                out = rend.render(o, d, near, far, background_rgb=bg, cos_anneal_ratio=0.5, t_rand=inputs[it]["t_rand"],
                                  t_rand_out=inputs[it]["t_rand_out"])
                loss = (out["color_fine"] - rgb).abs().sum() / B + 0.1 * out["gradient_error"]
                if wdepth:
                    loss = loss + 0.3 * (out["render_feats"] - extra["gt_feats"]).abs().sum() / B
                for p in params:
                    p.grad = None
                loss.backward()
                outs.append({k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)})
                gl = [torch.zeros_like(p) if p.grad is None else p.grad for p in params]
                grads.append(torch.cat([g.reshape(-1) for g in gl]))
                with torch.no_grad():            # a plain descent step: the next call rebuilds every weight image
                    torch._foreach_add_(list(params), gl, alpha=-1e-3)
                if serial:
                    if it == 1:
                        e1.record()
                    torch.cuda.synchronize()
                    if it == 1:
                        t_step = e0.elapsed_time(e1)
            if between_steps is not None:
                between_steps(rend, calls)
            torch.cuda.synchronize()
            res = dict(outs=[{k: _cpu(v) for k, v in o_.items()} for o_ in outs], grads=[_cpu(g) for g in grads],
                       params=_cpu(torch.cat([p.detach().reshape(-1) for p in params])), log=list(h.log), delays=h.delays)
    if serial:
        res["T_step_ms"], res["D_ms"] = t_step, max(2.0 * t_step, 1.0)
    res["cycles"] = cycles
    return res


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
def case_id(spec):
    if spec["kind"] == "train":
        parts = [spec["cfg"]] + ([spec["switch"]] if spec.get("switch") else []) + [spec["arm"]]
        if spec.get("no_forward_join"):
            parts.append("nojoin")
    elif spec["kind"] == "dropin":
        parts = ["dropin", "vdn" if spec["wdepth"] else "plain", "split" if spec["split_dw"] else "nosplit", spec["arm"]]
    else:
        parts = [spec["kind"]]
    return "-".join(parts).replace(":", "@")


def ref_spec(spec):
    """The serial arm a case is compared with (same configuration, same launch-selecting switches)."""
    r = {k: v for k, v in spec.items() if k not in ("arm", "no_forward_join", "steps")}
    r["arm"] = "ref"
    return r


_CACHE = {}


def run_case(spec):
    """-> the case's result (a dict of CPU tensors, lists and floats). Serial arms are cached per process and never changed."""
    cid = case_id(spec)
    if cid in _CACHE:
        return _CACHE[cid]
    concurrency_precondition()                    # (first of all: it creates the streams and picks the user stream)
    if spec["kind"] == "train":
        res = train_arm(spec["cfg"], spec["arm"], spec.get("switch"), spec.get("steps", S), spec.get("no_forward_join", False))
    elif spec["kind"] == "dropin":
        res = dropin_arm(spec["wdepth"], spec["split_dw"], spec["arm"])
    elif spec["kind"] == "precondition":
        res = dict(pairs=concurrency_precondition(), cycles_per_ms=cycles_per_ms())
    else:
        raise ValueError(spec)
    if spec.get("arm") == "ref" or spec["kind"] == "precondition":
        _CACHE[cid] = res
    return res


def all_cases():
    """Every case of tests/test_gpu_stream_order.py (the child process runs them all; serial arms come with their first user)."""
    cases = []
    for name, cfg in CONFIGS.items():
        for arm in ("none",) + tuple(cfg["roles"]):
            cases.append(dict(kind="train", cfg=name, arm=arm))
    for sw in SWITCHES:
        for arm in ("main", "side"):
            cases.append(dict(kind="train", cfg="T2", switch=sw, arm=arm))
    for name in CONFIGS:
        cases.append(dict(kind="train", cfg=name, switch="ovl0", arm="ref"))
    for wdepth in (False, True):
        for split_dw in (True, False):
            for arm in ("main", "side"):
                cases.append(dict(kind="dropin", wdepth=wdepth, split_dw=split_dw, arm=arm))
    cases.append(dict(kind="train", cfg="T1", arm="side", steps=1, no_forward_join=True))
    return cases


def main(out_dir):
    """The child process: the four streams first, the precondition, then every case and its serial arm -> out_dir/<case id>.pt."""
    dev_streams()
    torch.save(run_case(dict(kind="precondition")), os.path.join(out_dir, "precondition.pt"))
    for spec in all_cases():
        for s in (ref_spec(spec), spec):
            path = os.path.join(out_dir, case_id(s) + ".pt")
            if not os.path.exists(path):
                torch.save(run_case(s), path)
    with open(os.path.join(out_dir, "done.json"), "w") as f:
        json.dump({"cases": len(all_cases()), "wall_s": time.time() - _T0}, f)


_T0 = time.time()

if __name__ == "__main__":
    main(sys.argv[1])
