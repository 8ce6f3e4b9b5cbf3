"""No launch of a step reads a row that this step did not write: every persistent workspace is poisoned between steps and the
step is held to the un-poisoned run bit for bit.

tests/poison.py holds the ledger (every persistent device tensor and its class), the walker and the poison. Here, per
configuration, two arms run from the same seed: a clean one and a poisoned one. In front of EVERY step - step 0 included, which
catches reliance on what the allocator returned - both arms call tr.join() and torch.cuda.synchronize() and walk the objects; the
poisoned arm then writes all-ones bytes (NaN / 0xFF) into every `rewritten` buffer, shuffled stale rows (the clean arm's contents
after the same step) into every `masked` one and in-range integers into the work lists and counters. After every step the six
scalars, grad_flat, param_flat, both moment buffers, pose_flat and the work lists' counters are compared with torch.equal. There is
no tolerance: test_gpu_train_parity.py::test_training_is_bitwise_reproducible establishes that two clean arms agree bit for bit.

Configurations (B = 160, S = 6 of tests/stream_skew.py, whose inputs make both work lists strict, changing subsets; the depth term
comes on at step 3, T6 moves from fixed-pose to pose steps at step 3): T1 - T6 on the serial arm and on the shipped schedule;
T2 with VDN_FUSED_COMPOSITE=0 and with VDN_TRAIN_COLOR_FUSED=1; a renderer without background (n_outside = 0); B = 96 after
B = 160 on one renderer whose cached engines alternate; the drop-in flow (plain / VDN head, eager / VDN_RENDER_GRAPHS=1); the
inference render() in bf16 and fp32; the standalone networks of vdn_hip/points.py at two row counts inside one padded block.

The harness bites: poison written between forward and backward into a plane the backward reads changes the gradient, once per
dtype; every `masked` row filled with NaN instead of stale values changes the step (so the class is not vacuous: those rows are
truly read under a zero factor); and the poisoned share of the non-state bytes is 100 %.

Record (MI355X, whole-suite order). No stale read was found: every configuration is bit-identical under the poison. T2: 82
`rewritten` tensors / 995 MB, 5 `masked` / 10.6 MB (sdf, normals, bg_density, bg_rgb, bg_feat), 202 `state`, 31 `const`; T3 (fp32)
2.1 GB poisoned per step; T6 85 `rewritten` with the ray-adjoint buffers; two cached engines 1.38 GB; the inference path keeps ONE
workspace, the background network's masked scratch buffer; the standalone networks keep none (868 MB of free allocator blocks
poisoned instead). Classes that changed while this was written: col_out and vdn_out are torch.zeros and were entered as `masked`;
NaN behind the heads' prefix changes nothing (a select stands in front of the load, csrc/k_composite_row.h:84-85, :155), so they are
`rewritten`. The flat gradient was tried as `rewritten` and is so wherever a network has weight-gradient entries, but with
n_outside = 0 the background network's 606 596 elements are written by no launch and keep the zeros of their allocation: `state`.
The module's 36 cases take 12 s, beside 11 s of test_gpu_stream_order.py in the same run."""
import pytest
import torch

import poison
import stream_skew as sk

pytestmark = pytest.mark.gpu

DEV = sk.DEV


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is sticky: once a synchronisation fails, nothing more of this file runs on the device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping the module: %s" % e, returncode=3)


# ------------------------------------------------------------------------------------------------------------------------
# the hook both arms run between steps
# ------------------------------------------------------------------------------------------------------------------------
def _observe_trainer(tr):
    eng = tr.engine
    got = dict(scalars=tr.scalars, grad_flat=eng.grad_flat, param_flat=tr.param_flat, exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq,
               fg_counts=eng._fg_cnt[:3])
    if "bg_active" in eng.w:
        got["bg_count"] = eng.w["bg_active"][1]
    if tr.cameras is not None:
        got["pose_flat"] = tr._pose_flat
    return {k: v.detach().clone().cpu() for k, v in got.items()}


class Hook:
    """between_steps of one arm. clean=None: the clean arm (it keeps the stale sources behind every step); else the poisoned arm,
    which takes its stale rows from `clean`. only / override: poison.apply's (narrowing and the bite checks)."""

    def __init__(self, n_steps, clean=None, only=None, override=None):
        self.n_steps, self.clean, self.only, self.override = n_steps, clean, only, override
        self.steps, self.stale, self.cov, self.done, self.found = [], [], None, {}, None

    def __call__(self, obj, it):
        is_trainer = hasattr(obj, "engine")
        if is_trainer:
            obj.join()
        torch.cuda.synchronize()
        found = poison.classify(poison.walk(poison.roots_of(tr=obj) if is_trainer else poison.roots_of(rend=obj)))
        if it > 0:
            if is_trainer:
                self.steps.append(_observe_trainer(obj))
            self.stale.append(poison.snapshot_stale_sources(found))
        if self.clean is not None and it < self.n_steps:
            done = poison.apply(found, stale=self.clean.stale[it], seed=it, only=self.only, override=self.override)
            self.done.update(done)
            self.cov, self.found = poison.coverage(found, done), [(f.name, f.row[1]) for f in found]
            torch.cuda.synchronize()


def _assert_coverage(h, what):
    """The poisoned arm's last walk: every byte outside state / const tensors was poisoned, nothing of a state / const tensor was,
    and the tensors left alone are exactly the ledger's state / const rows."""
    c = h.cov
    print("%s: %s; non-state bytes %d, poisoned %d" % (what, ", ".join("%s %d tensors / %d bytes" % (k, n, b) for k, (n, b) in c["classes"].items()),
                                                       c["non_state_bytes"], c["poisoned_bytes"]))
    assert c["non_state_bytes"] > 0 and c["poisoned_bytes"] == c["non_state_bytes"], (what, c)
    assert c["clobbered"] == 0, (what, c)
    left = sorted(n for n, cls in h.found if n not in h.done)
    assert left == sorted(n for n, cls in h.found if cls in ("state", "const")), what
    assert c["classes"]["rewritten"][0] + c["classes"]["masked"][0] > 0


def _first_difference(clean, pois):
    """-> None, or (step, key, differing elements) of the first observation of the poisoned arm that differs."""
    assert len(clean.steps) == len(pois.steps) > 0
    for it, (a, b) in enumerate(zip(clean.steps, pois.steps)):
        assert a.keys() == b.keys()
        for k in a:
            if a[k].dtype.is_floating_point:
                assert torch.isfinite(a[k]).all(), ("the clean arm", it, k)
            if not torch.equal(a[k], b[k]):
                return it, k, int((a[k] != b[k]).sum())
    return None


# ------------------------------------------------------------------------------------------------------------------------
# arms
# ------------------------------------------------------------------------------------------------------------------------
_CLEAN = {}


def _train_pair(cfg, arm, env=None, steps=sk.S, only=None, override=None):
    """(clean hook, poisoned hook) of one Trainer configuration; the clean arm is run once per (cfg, arm, env, steps)."""
    key = (cfg, arm, tuple(sorted((env or {}).items())), steps)
    if key not in _CLEAN:
        sk.concurrency_precondition()
        h = Hook(steps)
        sk.train_arm(cfg, arm, steps=steps, between_steps=h, env_extra=env)
        _CLEAN[key] = h
    clean = _CLEAN[key]
    pois = Hook(steps, clean=clean, only=only, override=override)
    sk.train_arm(cfg, arm, steps=steps, between_steps=pois, env_extra=env)
    return clean, pois


_T = [(c, a) for c in sk.CONFIGS for a in ("ref", "none")]


@pytest.mark.parametrize("cfg,arm", _T, ids=["%s-%s" % (c, "serial" if a == "ref" else "shipped") for c, a in _T])
def test_training_step_reads_no_stale_row(cfg, arm):
    clean, pois = _train_pair(cfg, arm)
    assert _first_difference(clean, pois) is None, (cfg, arm, _first_difference(clean, pois))
    _assert_coverage(pois, "%s-%s" % (cfg, arm))


@pytest.mark.parametrize("switch", ["VDN_FUSED_COMPOSITE=0", "VDN_TRAIN_COLOR_FUSED=1"])
def test_other_owners_of_the_compositor_and_colour_buffers(switch):
    """T2 where other launches own the compositor's and the colour head's buffers: the separate compositor / loss / adjoint launches,
    and the colour head inside the SDF kernel's launch."""
    k, v = switch.split("=")
    clean, pois = _train_pair("T2", "none", env={k: v})
    assert _first_difference(clean, pois) is None, (switch, _first_difference(clean, pois))
    _assert_coverage(pois, switch)


def _no_background_arm(hook, steps=4):
    """A Trainer on a renderer with n_outside = 0: no background list, no work lists at all (TrainEngine.forward: nothing may be skipped)."""
    from vdn_train import factory
    from vdn_train.trainer import Trainer
    inputs, _ = sk._step_inputs(11, steps, "noout")
    with sk.environ(VDN_SDF_TAIL="0"):
        torch.manual_seed(0)
        rend = factory.build_renderer(wdepth=False, device=DEV, precision="bf16", n_outside=0)
        tr = Trainer(rend, sk.B, DEV, conf=dict(sk._BASE))
        torch.cuda.synchronize()
        for it in range(steps):
            hook(tr, it)
            x = inputs[it]
            tr.train_step(*x["args"], t_rand=x["t_rand"])
        hook(tr, steps)
    torch.cuda.synchronize()
    return sum(p.numel() for p in rend.nerf.parameters())


def test_renderer_without_background():
    clean = Hook(4)
    _no_background_arm(clean)
    pois = Hook(4, clean=clean)
    _no_background_arm(pois)
    assert _first_difference(clean, pois) is None, _first_difference(clean, pois)
    _assert_coverage(pois, "n_outside=0")
    assert "bg_count" not in clean.steps[0]


def _render_flow(hook, batches, wdepth, env, grad=True, precision="bf16"):
    """render() on ONE renderer over `batches` (ray counts; the first rays of stream_skew's 160-ray inputs): under grad with the
    drop-in flow's loss and a plain descent step, or under no_grad. -> per call {name: CPU tensor} of every output (+ "grads")."""
    from vdn_train import factory
    inputs, extra = sk._step_inputs(13, len(batches), "flow", feats=wdepth)
    bg = torch.ones(1, 3, device=DEV)
    res = []
    with sk.environ(**env):
        torch.manual_seed(0)
        rend = factory.build_renderer(wdepth=wdepth, device=DEV, precision=precision)
        params = rend._all_parameters()
        torch.cuda.synchronize()
        for it, B in enumerate(batches):
            hook(rend, it)
            o, d, near, far, rgb = (t[:B].contiguous() for t in inputs[it]["args"])
            kw = dict(background_rgb=bg, cos_anneal_ratio=0.5, t_rand=inputs[it]["t_rand"][:B].contiguous(),
                      t_rand_out=inputs[it]["t_rand_out"][:B].contiguous())
            if not grad:
                with torch.no_grad():
                    out = rend.render(o, d, near, far, **kw)
                torch.cuda.synchronize()
                res.append({k: v.detach().clone().cpu() for k, v in out.items() if torch.is_tensor(v)})
                continue
            out = rend.render(o, d, near, far, **kw)
            loss = (out["color_fine"] - rgb).abs().sum() / B + 0.1 * out["gradient_error"]
            if wdepth:
                loss = loss + 0.3 * (out["render_feats"] - extra["gt_feats"][:B]).abs().sum() / B
            for p in params:
                p.grad = None
            loss.backward()
            gl = [torch.zeros_like(p) if p.grad is None else p.grad for p in params]
            one = {k: v.detach().clone().cpu() for k, v in out.items() if torch.is_tensor(v)}
            one["grads"] = torch.cat([g.reshape(-1) for g in gl]).cpu()
            with torch.no_grad():
                torch._foreach_add_(list(params), gl, alpha=-1e-3)
            torch.cuda.synchronize()
            res.append(one)
        hook(rend, len(batches))
    return res


def _render_pair(batches, wdepth, env, grad=True, precision="bf16"):
    clean = Hook(len(batches))
    a = _render_flow(clean, batches, wdepth, env, grad, precision)
    pois = Hook(len(batches), clean=clean)
    b = _render_flow(pois, batches, wdepth, env, grad, precision)
    assert len(a) == len(b) == len(batches)
    for it, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys() and len(x) >= 6
        for k in x:
            if x[k].dtype.is_floating_point:
                assert torch.isfinite(x[k]).all(), ("the clean arm", it, k)
            assert torch.equal(x[k], y[k]), (it, k, int((x[k] != y[k]).sum()))
    return clean, pois, a


_EAGER = dict(VDN_RENDER_GRAPHS="0", VDN_SDF_TAIL="0")


@pytest.mark.parametrize("wdepth", [False, True], ids=["plain", "vdn"])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_drop_in_flow_reads_no_stale_row(wdepth, graphs):
    """render() under grad + loss.backward() + a descent step, four calls: eager, and with VDN_RENDER_GRAPHS=1 (calls 1 - 3 replay
    the captured forward, 2 - 3 the captured backward) - the poison then lands on the replayed graphs' own buffers."""
    env = dict(VDN_RENDER_GRAPHS="1" if graphs else "0")
    sk.concurrency_precondition()
    clean = Hook(4)
    ref = sk.dropin_arm(wdepth, True, "none", between_steps=clean, env_extra=env, calls=4)
    pois = Hook(4, clean=clean)
    got = sk.dropin_arm(wdepth, True, "none", between_steps=pois, env_extra=env, calls=4)
    assert len(ref["outs"]) == len(got["outs"]) == len(ref["grads"]) == len(got["grads"]) == 4
    for it in range(4):
        a, b = ref["outs"][it], got["outs"][it]
        assert a.keys() == b.keys() and len(a) >= 6
        for k in a:
            assert torch.isfinite(a[k]).all(), ("the clean arm", it, k)
            assert torch.equal(a[k], b[k]), (it, k, int((a[k] != b[k]).sum()))
        assert torch.isfinite(ref["grads"][it]).all() and float(ref["grads"][it].abs().max()) > 0
        assert torch.equal(ref["grads"][it], got["grads"][it]), (it, "grads", int((ref["grads"][it] != got["grads"][it]).sum()))
    assert torch.equal(ref["params"], got["params"])
    _assert_coverage(pois, "drop-in %s %s" % ("vdn" if wdepth else "plain", "graphs" if graphs else "eager"))
    names = [n for n, _ in pois.found]
    assert any("._plans." in n for n in names) == graphs
    if graphs:                                                                 # the captured backward exists too: it was replayed
        assert any("._plans." in n and ".bwd." in n for n in names)


def test_alternating_batch_sizes_on_one_renderer():
    """B = 96 after B = 160 and back: the renderer's cached engines alternate, each keeps its workspaces while the other runs."""
    clean, pois, res = _render_pair([160, 96, 160, 96], False, _EAGER)
    _assert_coverage(pois, "B = 160 / 96")
    assert sum(1 for n, _ in pois.found if n.endswith(".w.sdf")) == 2          # both engines were walked and poisoned


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_inference_render_reads_no_stale_row(precision):
    """Four render() calls under no_grad on batches whose work lists differ: every tensor of the output dict."""
    clean, pois, res = _render_pair([sk.B] * 4, True, _EAGER, grad=False, precision=precision)
    _assert_coverage(pois, "inference " + precision)
    assert any("._scratch." in n for n, _ in pois.found)
    assert not torch.equal(res[0]["weights"], res[1]["weights"])


def _points_arm(poisoned):
    """SDFNetwork, RenderingNetwork and NeRF under autograd (vdn_hip/points.py), bf16, P = 1000 then P = 999 on the same modules:
    both counts share one padded block of 1024 plane rows. The plans these calls cache hold maps and descriptor tables only
    (`const`); the saves, deltas, slabs and column sums are per-call allocations, so the poison goes into the allocator's free
    blocks. -> (per call the gradients of every parameter, bytes poisoned, the modules)."""
    from test_gpu_module_autograd import _clear, _nerf_inputs, _rand, _rend, _rn_inputs
    r = _rend(DEV, "bf16")
    nets = (r.sdf_network, r.color_network, r.nerf)
    for m in nets:
        m.differentiable = True
    out, total = [], 0
    for P in (1000, 999):
        x, R = _rand("wp%d" % P, (P, 3), -1.1, 1.1).to(DEV), _rand("wpr%d" % P, (P, 257)).to(DEV)
        ins = [t.to(DEV) for t in _rn_inputs(P, 256)]
        p4, d = (t.to(DEV) for t in _nerf_inputs(P))
        torch.cuda.synchronize()
        found = poison.classify(poison.walk(dict(zip(("sdf_network", "color_network", "nerf"), nets))))
        assert all(f.row[1] in ("state", "const") for f in found), [f.name for f in found if f.row[1] in poison.POISONED]
        if poisoned:
            total += poison.poison_free_blocks_(DEV)[1]
        _clear(*nets)
        sdf, col, nerf = nets
        (sdf(x) * R).sum().backward()
        (col(*ins) * R[:, :3]).sum().backward()
        sum((t * R[:, :t.shape[1]]).sum() for t in nerf(p4, d)).backward()
        torch.cuda.synchronize()
        out.append([p.grad.detach().clone().cpu() for m in nets for p in m.parameters()])
    return out, total, [f.name for f in found]


def test_standalone_networks_read_no_recycled_row():
    clean, _, names = _points_arm(False)
    got, total, _ = _points_arm(True)
    print("points: %d bytes of free allocator blocks poisoned over two calls; %d persistent tensors, all state / const" % (total, len(names)))
    assert any("._pt_plans." in n for n in names)
    assert total >= 2 * 2 * 8 * 1024 * 256 * 2                                 # at least the H and V planes of one SDF call, twice
    for a, b in zip(clean, got):
        assert len(a) == len(b) > 20
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(clean[0], clean[1]))      # (row 999 enters the P = 1000 sums)


@pytest.mark.parametrize("cfg", ["T2", "T6"])
def test_flat_gradient_is_overwritten_where_a_network_has_entries(cfg):
    """The flat gradient is `state` in the ledger for ONE reason, shown by the second test below. Everywhere else the step
    overwrites it: NaN in all of it in front of every step changes nothing (T2: all four networks, the depth term coming on;
    T6: fixed-pose and pose steps)."""
    name = "tr.engine._grad_flat"
    clean, pois = _train_pair(cfg, "ref", only={name}, override={name: "ones"})
    assert list(pois.done) == [name]
    assert _first_difference(clean, pois) is None, _first_difference(clean, pois)


def test_flat_gradient_keeps_its_zeros_without_background():
    """n_outside = 0: the engine has no weight-gradient entries for the background network, whose slice of the flat gradient is
    written by no launch and relies on the zeros of its allocation - NaN there stays, and only there."""
    name = "tr.engine._grad_flat"
    clean = Hook(2)
    n_nerf = _no_background_arm(clean, steps=2)
    pois = Hook(2, clean=clean, only={name}, override={name: "ones"})
    _no_background_arm(pois, steps=2)
    assert list(pois.done) == [name]
    for a, b in zip(clean.steps, pois.steps):
        diff = a["grad_flat"] != b["grad_flat"]
        assert int(diff.sum()) == n_nerf and bool(torch.isnan(b["grad_flat"][diff]).all()) and float(a["grad_flat"][diff].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# the harness bites
# ------------------------------------------------------------------------------------------------------------------------
_SEAM = {"f32": ("tr.engine.w.mid_z", "ones"), "bf16": ("tr.engine.w.col_h", "ones"), "uint8-mask": ("tr.engine.w.col_mask", "ones"),
         "int32-list": ("tr.engine.w.fg_active.0", None)}


def _seam_arm(target):
    """One T2 step on the serial arm whose TrainEngine.backward is preceded by a poison write into `target` (name, poison): the
    poison lands BETWEEN forward and backward, on a plane the backward reads. -> grad_flat on the CPU."""
    def hook(tr, it):
        if it != 0 or target is None:
            return
        eng, inner = tr.engine, tr.engine.backward

        def backward(*a, **k):
            torch.cuda.synchronize()
            found = poison.classify(poison.walk(poison.roots_of(tr=tr)))
            done = poison.apply(found, seed=1, only={target[0]}, override={target[0]: target[1]} if target[1] else None)
            assert list(done) == [target[0]], done
            torch.cuda.synchronize()
            return inner(*a, **k)
        eng.backward = backward
    return sk.train_arm("T2", "ref", steps=1, between_steps=hook)["grad_flat"]


@pytest.mark.parametrize("dtype", list(_SEAM))
def test_poison_between_forward_and_backward_changes_the_gradient(dtype):
    """Writes land where kernels read: NaN in the f32 mid-points, NaN in a bf16 saved plane of the colour head, 0xFF in its 1-bit
    ReLU masks, other (valid) row ids in the int32 foreground list - each changes the gradient of the step."""
    if "seam" not in _CLEAN:
        _CLEAN["seam"] = _seam_arm(None)
    clean, got = _CLEAN["seam"], _seam_arm(_SEAM[dtype])
    assert torch.isfinite(clean).all() and float(clean.abs().max()) > 0
    assert not torch.equal(clean, got), dtype


_MASKED_T2 = sorted("tr.engine.w." + k for k, row in poison.W_LEDGER.items() if row[0] == "masked")


@pytest.mark.parametrize("name", _MASKED_T2)
def test_masked_rows_are_truly_read(name):
    """`masked` is not vacuous: with NaN instead of stale finite values in the rows off the lists, the step changes - the rows are
    read, under a zero factor. (A buffer this did not change would be `rewritten`.)"""
    clean, pois = _train_pair("T2", "ref", steps=4, only={name}, override={name: "ones"})
    assert list(pois.done) == [name]
    assert _first_difference(clean, pois) is not None, name


def test_masked_scratch_of_the_inference_path_is_truly_read():
    """The background network's per-stream scratch buffer (dpt_models/fields.py NeRF._run): NaN off the list reaches the output."""
    clean = Hook(3)
    a = _render_flow(clean, [sk.B] * 3, True, _EAGER, grad=False)
    name = next(n for n in clean.stale[-1] if "._scratch." in n)
    pois = Hook(3, clean=clean, only={name}, override={name: "ones"})
    b = _render_flow(pois, [sk.B] * 3, True, _EAGER, grad=False)
    assert list(pois.done) == [name]
    assert any(not torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
