"""The ORDER in which the training step's kernels run across its four streams, held to a serial execution bit for bit.

Every arm (tests/stream_skew.py) builds the same Trainer from torch.manual_seed(0), feeds it the same synth.* inputs for S = 6 steps
and is compared with the configuration's serial arm - VDN_SIDE_STREAM=0, the logging launches on the caller's stream too,
torch.cuda.synchronize() after every step: the scalars of every step, param_flat, exp_avg, exp_avg_sq and engine.grad_flat with
torch.equal, all finite, and the multiset of entry points per step equal. The test arms run the shipped default schedule with no
delay and with ONE stream at a time held back: a delay D = max(2 T_step, 1 ms) (one torch.cuda._sleep, no data, no host
synchronisation) in front of every launch on `main`, `side`, `side2` or `log`. A consumer that is not ordered behind a delayed
producer then passes it with certainty, so a missing or over-trimmed wait fails here deterministically instead of on a busy
machine.

Pinned in both arms: VDN_SDF_TAIL=0 (its default flips on without a side stream, TrainEngine._tail_wanted), and the switches that
select LAUNCHES as well as streams - the Trainer's `overlap` (with it the rest group's weight-gradient GEMM, Adam step and image
build are two launches each, background network / heads; without it one), VDN_SPLIT_REST (the same) and VDN_FUSED_PREP. The serial
arm therefore keeps overlap=True (without a side stream the flag moves nothing to another stream);
test_serial_arm_is_the_same_with_overlap_off holds it to the overlap=False serial arm, bit for bit, for every configuration.

Hand-overs the schedule rests on (vdn_hip/train.py TrainEngine, vdn_train/trainer.py Trainer.train_step / join). RAW = the waiter
reads what the recorder's stream wrote, WAR = the waiter rewrites what the recorder's stream still reads.

  event      recorded (stream)                                   waited for by                          protects
  _ev_fork   _fork(): caller's, behind the step preparation      side, in front of the background       RAW z_feed, bg_mid, bg_dists, bg_active (prep -> network);
             (forward) / the compositor's adjoint (backward,     network's forward / backward           RAW d_bg_density, d_bg_rgb, d_bg_feat (adjoint -> its backward);
             when no fork_event is handed in)                                                           WAR bg_density / bg_rgb / bg_feat, nf_* saves (last step's readers
                                                                                                        on the caller's stream)
  _ev_join   _side_done(): side, behind the background           caller's, _join(): in front of the     RAW bg_density, bg_rgb, bg_feat (-> compositor); RAW nf_d* deltas,
             network's forward / its backward (+ its GEMM        compositor; in backward() in front of  nf_* saves and the background slice of grad_flat (-> "all" GEMM,
             in render()'s backward)                             the "all" group / behind the heads'    param_grads)
  _ev_fork2  forward: caller's, behind join() and the SDF        side2, in front of the VDN head        RAW feat, normals, mid_z, fg_active, the head's weight image;
             kernel                                                                                     WAR vdn_out, vdn_h, vdn_small, vdn_mask (last step's heads' GEMM,
                                                                                                        ordered on the caller's stream by _ev_ws)
  _ev_join2  forward: side2, behind the VDN head                 caller's, in front of the compositor   RAW vdn_out (and the head's saves for backward)
  _ev_comp   train_step: caller's, behind the fused compositor   log; side in front of the background   RAW color, weights, eik_partial, feat_out (-> loss scalars);
                                                                 network's backward (fork_event: no     RAW d_bg_* (vdn_composite_train's adjoint -> background backward)
                                                                 VDN head, VDN_EVENT_TRIM on)
  _ev_log    train_step: log, behind vdn_loss_fwd_bwd            caller's, at the end of the step       RAW scalars, eik; WAR color, weights, eik_partial, feat_out, true_rgb,
                                                                                                        gt_feats (next forward / the caller's buffers)
  _ev_heads  backward: caller's, behind the heads' backward      side, side_weight_grads without        RAW col_dh, col_dout, vdn_dh, vdn_dout, d_featvec (-> heads' GEMM)
             (only with heads_event: VDN_EVENT_TRIM=0)           `after` (the Trainer always hands one)
  _ev_gemm   backward: caller's, behind the SDF group's GEMM     side, in front of the one-launch rest  RAW the heads' deltas (covers their backward); keeps the two
             (overlap and not (split and TRIM))                  group (VDN_SPLIT_REST=0)               HBM-bound GEMMs apart
  _ev_tail   train_step: caller's, behind the SDF update         side, in front of the heads' GEMM      RAW the heads' deltas (covers their backward)
  _ev_ws     side, right behind the heads' / rest group's GEMM   caller's, next step, in front of the   WAR feat, col_h, col_small, vdn_h, vdn_small, col_dh, col_dout, vdn_dh,
                                                                 step preparation                       vdn_dout, nf_* and fg_active[1] / bg_active[1] (prep and forward rewrite)
  _ev_rest   side, behind the heads' (rest) Adam + image build   join(): caller's in front of the       RAW param_flat / exp_avg* / weight images of the heads and the background
                                                                 heads' forward (before_heads), of a    network, their slices of grad_flat
                                                                 pose step, of any outside reader

No ordering bug was found: every arm below is bit-identical to its serial arm, and the removed-join case differs.

Measured on the MI355X (figures scale the tool, they are no pass bar). The delay kernel: 2.40e6 cycles per ms. T_step / D of the
serial arms: T1 1.06 / 2.12 ms, T2 1.13 / 2.26, T3 (fp32) 5.55 / 11.1, T4 1.05 / 2.10, T5 1.06 / 2.11, T6 1.04 / 2.08, the T2 switches
1.04 - 1.18 / 2.08 - 2.37, the drop-in flow 1.7 - 2.8 / 3.4 - 5.6. B = 160 full-frame rays, the starting value, is strict at once: the
foreground list holds 16 468 of 20 480 rows and the background list 14 846 of 25 600 after the first step (T1, T4, T5; T2 14 756,
T3 14 759; T6, other cameras: 15 025 and 16 640). The 18 stream pairs ran concurrently in-process, alone and in whole-suite order
(the user stream is chosen among new streams for that, stream_skew.concurrency_precondition); the module's 49 cases take 13 s
(16 s when they go through the child process).
"""
import collections
import os
import subprocess
import sys

import pytest
import torch

import stream_skew as sk

pytestmark = pytest.mark.gpu


class _Cases:
    """Results by case: computed in this process, or read from what the one child process left on disk."""

    def __init__(self, folder=None):
        self.folder = folder
        pre = self.get(dict(kind="precondition"))
        self.pairs, self.cycles_per_ms = pre["pairs"], pre["cycles_per_ms"]

    def get(self, spec):
        if self.folder is None:
            return sk.run_case(spec)
        name = "precondition" if spec["kind"] == "precondition" else sk.case_id(spec)
        return torch.load(os.path.join(self.folder, name + ".pt"), weights_only=False)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    here = _Cases()
    if all(here.pairs.values()):
        return here
    # two of this process's streams share a hardware queue (the streams earlier tests made took the others): all arms in ONE fresh
    # child process, which creates the four streams first
    folder = str(tmp_path_factory.mktemp("stream_order"))
    p = subprocess.run([sys.executable, os.path.abspath(sk.__file__), folder], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    print("stream-order arms ran in a child process; in this process:", {k: v for k, v in here.pairs.items() if not v})
    return _Cases(folder)


def _per_step(log):
    out = collections.defaultdict(collections.Counter)
    for step, name, role in log:
        out[step][name] += 1
    return dict(out)


def _check_serial(ref, cfg_name):
    fg, P, bg, Q = ref["counts"]
    print("%s serial arm: fg_active %d of %d, bg_active %d of %d, T_step %.3f ms, D %.3f ms" % (cfg_name, fg, P, bg, Q, ref["T_step_ms"], ref["D_ms"]))
    assert 0 < fg < P and 0 < bg < Q, (cfg_name, ref["counts"])              # both work lists: strict, non-empty subsets
    assert {role for _, _, role in ref["log"]} == {"main"}                    # truly serial: every launch on the caller's stream
    assert ref["D_ms"] >= 2.0 * ref["T_step_ms"] and ref["D_ms"] >= 1.0


def _check_train(got, ref, what, buffers=("param_flat", "exp_avg", "exp_avg_sq", "grad_flat"), launches=True):
    assert got["scalars"].shape == ref["scalars"].shape
    for it in range(ref["scalars"].shape[0]):
        assert torch.equal(got["scalars"][it], ref["scalars"][it]), (what, "scalars of step", it, got["scalars"][it].tolist(), ref["scalars"][it].tolist())
    for k in buffers + (("pose_flat",) if "pose_flat" in ref else ()):
        assert torch.isfinite(got[k]).all(), (what, k)
        assert torch.equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), float((got[k] - ref[k]).abs().max()))
    assert torch.isfinite(got["scalars"]).all(), what
    if launches:
        assert _per_step(got["log"]) == _per_step(ref["log"]), what


def _check_delays(got, arm):
    role, _, fn = arm.partition(":")
    n = sum(1 for _, name, r in got["log"] if r == role and (not fn or name == fn))
    # (try_call launches that declined a shape were delayed as well: at least one delay per logged launch)
    assert got["delays"] >= n > 0 and got["cycles"] > 0, (arm, got["delays"], n)


def test_streams_of_an_arm_run_concurrently(cases):
    """The precondition of every delayed arm: for each ordered pair of (caller's, side, side2, log) and of (user, side, side2, log), a
    kernel on B completes while a delay on A is still running - in this process, or in the child process the arms ran in."""
    print("cycles per ms of the delay kernel: %.0f; pairs: %s" % (cases.cycles_per_ms, cases.pairs))
    assert len(cases.pairs) == 18                                            # 12 + the 6 pairs with the user stream: none left out
    assert all(cases.pairs.values()), {k: v for k, v in cases.pairs.items() if not v}


_ARMS = [(name, arm) for name, cfg in sk.CONFIGS.items() for arm in ("none",) + tuple(cfg["roles"])]


@pytest.mark.parametrize("cfg_name,arm", _ARMS, ids=["%s-%s" % a for a in _ARMS])
def test_schedule_equals_the_serial_arm(cases, cfg_name, arm):
    """T1 - T6 (stream_skew.CONFIGS) on the shipped default schedule: un-delayed, and with every launch of one stream delayed,
    against the VDN_SIDE_STREAM=0 arm."""
    spec = dict(kind="train", cfg=cfg_name, arm=arm)
    ref, got = cases.get(sk.ref_spec(spec)), cases.get(spec)
    _check_serial(ref, cfg_name)
    roles = collections.Counter(role for _, _, role in got["log"])
    if arm == "none":
        print(cfg_name, "launches per stream:", dict(roles))
        # the arms this configuration leaves out are exactly the streams it never launches on; and it does use several
        assert set(roles) == set(sk.CONFIGS[cfg_name]["roles"]) and len(roles) >= 2, roles
    else:
        _check_delays(got, arm)
    _check_train(got, ref, (cfg_name, arm))


_SW = [(sw, arm) for sw in sk.SWITCHES for arm in ("main", "side")]


@pytest.mark.parametrize("switch,arm", _SW, ids=["%s-%s" % a for a in _SW])
def test_schedule_switches_equal_the_serial_arm(cases, switch, arm):
    """T2 under VDN_EVENT_TRIM=0, VDN_SPLIT_REST=0, overlap=False with the side stream on, VDN_FUSED_PREP=0."""
    spec = dict(kind="train", cfg="T2", switch=switch, arm=arm)
    ref, got = cases.get(sk.ref_spec(spec)), cases.get(spec)
    _check_serial(ref, "T2-" + switch)
    _check_delays(got, arm)
    assert {"main", "side", "side2"} <= {role for _, _, role in got["log"]}
    _check_train(got, ref, (switch, arm))


@pytest.mark.parametrize("cfg_name", list(sk.CONFIGS))
def test_serial_arm_is_the_same_with_overlap_off(cases, cfg_name):
    """The serial arm the cases above compare with keeps overlap=True (launch selection only); with overlap=False - one rest-group
    GEMM, Adam step and image build instead of two - every value is the same."""
    a = cases.get(dict(kind="train", cfg=cfg_name, arm="ref"))
    b = cases.get(dict(kind="train", cfg=cfg_name, switch="ovl0", arm="ref"))
    _check_train(a, b, (cfg_name, "overlap"), launches=False)


_DROPIN = [(wd, sp, arm) for wd in (False, True) for sp in (True, False) for arm in ("main", "side")]


@pytest.mark.parametrize("wdepth,split_dw,arm", _DROPIN, ids=["%s-%s-%s" % ("vdn" if w else "plain", "split" if s else "nosplit", a) for w, s, a in _DROPIN])
def test_drop_in_flow_equals_the_one_stream_run(cases, wdepth, split_dw, arm):
    """NeuSRenderer.render under grad + loss.backward(), eager (VDN_RENDER_GRAPHS=0), three calls on one renderer whose workspaces
    are reused call to call, bf16, at the default and at VDN_BWD_SPLIT_DW=0: every returned tensor and every parameter's .grad of
    every call against the VDN_SIDE_STREAM=0 run."""
    spec = dict(kind="dropin", wdepth=wdepth, split_dw=split_dw, arm=arm)
    ref, got = cases.get(sk.ref_spec(spec)), cases.get(spec)
    print("drop-in serial arm: T_step %.3f ms, D %.3f ms" % (ref["T_step_ms"], ref["D_ms"]))
    assert {role for _, _, role in ref["log"]} == {"main"}
    assert "side" in {role for _, _, role in got["log"]}
    _check_delays(got, arm)
    for it, (a, b) in enumerate(zip(got["outs"], ref["outs"])):
        assert a.keys() == b.keys() and len(a) >= 6
        for k in b:
            assert torch.equal(a[k], b[k]), (it, k)
            assert torch.isfinite(a[k]).all(), (it, k)
    assert len(got["grads"]) == len(ref["grads"]) == sk.DROPIN_CALLS
    for it, (a, b) in enumerate(zip(got["grads"], ref["grads"])):
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0
        assert torch.equal(a, b), (it, int((a != b).sum()), float((a - b).abs().max()))
    assert torch.equal(got["params"], ref["params"])


def test_harness_detects_a_removed_join(cases):
    """The method bites: T1, side stream delayed, TrainEngine._join clearing _pending WITHOUT waiting during forward() - the
    compositor reads bg_density / bg_rgb (float planes only: no index list, no row count) before the background network wrote them,
    and the scalars of that one step differ from the serial arm's."""
    spec = dict(kind="train", cfg="T1", arm="side", steps=1, no_forward_join=True)
    ref, got = cases.get(sk.ref_spec(spec)), cases.get(spec)
    _check_delays(got, "side")
    assert not torch.equal(got["scalars"][0], ref["scalars"][0]), (got["scalars"][0].tolist(), ref["scalars"][0].tolist())
