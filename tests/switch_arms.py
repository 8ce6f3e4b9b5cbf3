"""Every arm of the run-time switch table (vdn_hip/switches.py) and the test that runs it: the ledger `ARMS`, the scenarios
the matrix of tests/test_gpu_switch_arms.py runs under an arm, and the child process of the arms a running process cannot reach
(tests/test_switch_arms_cpu.py holds the ledger to the table without a GPU).

A row of ARMS:
  values    the non-default value(s) of the switch that are run
  relation  "bits": every tensor a scenario returns equals the default arm's, torch.equal; "rounding": the arm changes a summation
            order by construction (the row's comment cites the line) - scalars of the first step bit for bit, every gradient tensor
            of the first step within 2e-5 of the default's largest entry, the parameters after the last step within 1e-3 of their norm
  held_by   "matrix" (tests/test_gpu_switch_arms.py runs `scenario` under the arm, `how` says in which process), the node id of
            an existing GPU test that runs the arm against the default (`both`: the line of it that builds both sides), or None
            with a `reason`
  taken     for "matrix": taken(value, arm_obs, default_obs) -> bool, a predicate on what `run` observed beside the tensors - the
            launch log of stream_skew.Skew (the vdn_hip.lib.call / try_call wrapper), attributes of the engine or Trainer - that
            proves the arm ran and was not silently the default. None only for the three switches the library reads itself
            (`native` points at the C++ line that selects the arm: nothing in Python sees which kernel a launch picked).

A scenario is `name(dev) -> {key: tensor}` on fixed seeds of vdn_train.synth at the smallest shapes that reach the paths; it leaves
what it observed in OBS. `run(name, dev)` -> (tensors on the CPU, observations). `python -m switch_arms SCENARIO OUT.npz`
(from tests/) is the child: one scenario under whatever the environment holds, tensors and observations in one .npz."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vdn-nerf_amd")
TESTS = os.path.join(ROOT, "tests")
for _p in (PKG, ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)


# ------------------------------------------------------------------------------------------------------------------------
# `taken` predicates: (value, observations under the arm, observations of the default arm) -> bool
# ------------------------------------------------------------------------------------------------------------------------
def _has(obs, part):
    return any(part in n for n in obs["log"])


def taken_fuse_rounds(value, arm, dflt):
    """The two launches of a sampler round appear, no launch that merges and up-samples in one does (vdn_merge_upsample, and the
    SDF pass that carries them, vdn_sdf_merge_upsample_bf16); the default arm has such launches."""
    return ("vdn_merge_sorted" in arm["log"] and "vdn_upsample_round" in arm["log"] and not _has(arm, "merge_upsample")
            and _has(dflt, "merge_upsample"))


def taken_fused_prep(value, arm, dflt):
    return "vdn_train_prep" in dflt["log"] and "vdn_train_prep" not in arm["log"] and len(arm["log"]) > len(dflt["log"])


def _gemms(obs):
    return sum(1 for n in obs["log"] if n.startswith("vdn_dw_gemm"))


def taken_split_rest(value, arm, dflt):
    """One rest-group GEMM instead of two halves: one weight-gradient GEMM launch per step less."""
    return _gemms(dflt) - _gemms(arm) == dflt["steps"] and _gemms(arm) == 2 * arm["steps"]


def taken_event_trim(value, arm, dflt):
    """Same launches, more events recorded (the SDF GEMM's and the heads' event of every step)."""
    return arm["log"] == dflt["log"] and arm["events"] > dflt["events"]


def taken_overlap(value, arm, dflt):
    return dflt["overlap"] is True and arm["overlap"] is False and _gemms(arm) < _gemms(dflt)


def expected_splits(P, segs, pps):
    """vdn_hip/train.py: dw_layout."""
    s = max(1, (P * segs + pps - 1) // pps)
    return s + s % 2 if segs == 2 else s


def _taken_splits(kinds_bf16, kinds_fp32):
    def taken(value, arm, dflt):
        want = int(value)
        nets = kinds_fp32 if arm["precision"] == "fp32" else kinds_bf16
        hit = 0
        for i, (kind, P, segs, splits) in enumerate(zip(arm["dw_kind"], arm["dw_P"], arm["dw_segs"], arm["dw_splits"])):
            on = kind in nets
            if arm["pps"][kind] != (want if on else dflt["pps"][kind]):
                return False
            if splits != expected_splits(P, segs, arm["pps"][kind]):
                return False
            if on:
                # 1 000 000 rows per split: one split, two for a two-segment entry; 1 024: sixteen and more
                if splits == dflt["dw_splits"][i] or (splits != segs if want >= 1000000 else splits < 16):
                    return False
                hit += 1
            elif splits != dflt["dw_splits"][i]:
                return False
        return hit > 0 and arm["dw_kind"] == dflt["dw_kind"] and arm["dw_P"] == dflt["dw_P"]
    return taken


def taken_render_graph(value, arm, dflt):
    """The image loop made one plan, captured once; its four full batches issued no launch from Python (the capture's own and the
    ragged batch's are all the log holds), where the default arm issues five renders' worth."""
    return dflt["plans"] == 0 and arm["plans"] == 1 and arm["captures"] == 1 and 0 < len(arm["log"]) < len(dflt["log"])


def taken_render_engines(value, arm, dflt):
    return dflt["engines"] == 2 and dflt["engines_built"] == 2 and arm["engines"] == 1 and arm["engines_built"] == 3


def taken_bwd_split_dw(value, arm, dflt):
    """The launches render_grad issued from Python (its eager calls and its graph captures, the same in both arms): one
    weight-gradient GEMM per backward under the arm, one per launch group - two or three - on the default."""
    return _gemms(arm) > 0 and _gemms(dflt) >= 2 * _gemms(arm) and _gemms(dflt) % _gemms(arm) == 0


def taken_mesh_method(value, arm, dflt):
    return ("vdn_mesh_count" in arm["log_env"] and "vdn_mesh_mc_count" not in arm["log_env"]
            and "vdn_mesh_mc_count" in dflt["log_env"] and "vdn_mesh_count" not in dflt["log_env"])


def taken_precision(value, arm, dflt):
    bf16 = lambda obs: sum(1 for n in obs["log"] if n.endswith("_bf16"))
    return dflt["env_precision"] == "fp32" and arm["env_precision"] == value and bf16(arm) > bf16(dflt)


def taken_dp_side_group(value, arm, dflt):
    return dflt["side_group_own"] is True and arm["side_group_own"] is False and arm["instream"] is True


def taken_dp_instream(value, arm, dflt):
    return dflt["instream"] is True and arm["instream"] is False and arm["side_group_own"] is True


def taken_dp_fused(value, arm, dflt):
    """The early eikonal all-reduce and the separate launches instead of the one-launch compositor of the collective path."""
    return "vdn_eikonal_terms" in arm["log"] and "vdn_eikonal_terms" not in dflt["log"]


# ------------------------------------------------------------------------------------------------------------------------
# the ledger
# ------------------------------------------------------------------------------------------------------------------------
def _held(node, both, relation="bits", values=("0",)):
    """both: the line of the test's own source that builds BOTH sides - the arm and the default - or the default-arm side next to
    a helper that sets the arm (the gate finds it in the function's text: a test that sets the arm on both sides has no such line)."""
    return dict(values=values, relation=relation, held_by=node, both=both)


def _matrix(values, scenario, how, taken, relation="bits", native=None):
    return dict(values=tuple(values), relation=relation, held_by="matrix", scenario=tuple(scenario), how=how, taken=taken, native=native)


_SPLIT_VALUES = ("1024", "1000000")

ARMS = {
    # ---- the sampler and the step preparation
    "VDN_FUSE_ROUNDS": _matrix(("0",), ("step_bf16", "render_inf"), "child", taken_fuse_rounds),                  # (read at import)
    "VDN_FUSE_SDF_ROUNDS": _held("tests/test_gpu_parity.py::test_fused_sampler_rounds_equal_the_two_launch_rounds", "for fused in (\"1\", \"0\"):"),
    # rounding: the work lists shorten the rows the weight-gradient GEMM contracts over (VdnDwDesc.P_dev, vdn_hip/train.py:234),
    # so a K split sums other rows; scalars bit for bit
    "VDN_BG_COMPACT": _held("tests/test_gpu_grads.py::test_trainer_work_lists_do_not_change_the_step", "for mode in (\"1\", \"0\"):", "rounding"),
    "VDN_FG_COMPACT": _held("tests/test_gpu_grads.py::test_trainer_work_lists_do_not_change_the_step", "for mode in (\"1\", \"0\"):", "rounding"),
    "VDN_RENDER_FG_COMPACT": _held("tests/test_gpu_runner_flow.py::test_render_under_grad_on_the_work_list_equals_every_sample", "os.environ[\"VDN_RENDER_FG_COMPACT\"] = \"1\" if compact else \"0\"", "rounding"),
    # (tests/test_gpu_stream_order.py runs VDN_FUSED_PREP / VDN_SPLIT_REST / VDN_EVENT_TRIM = 0 only against a serial arm under the
    # same setting, never against the default: they are run here)
    "VDN_FUSED_PREP": _matrix(("0",), ("step_bf16",), "monkeypatch", taken_fused_prep),
    # ---- forward
    "VDN_SHADE_FUSED": _held("tests/test_gpu_shade_fused.py::test_fused_shading_equals_the_separate_launches", "ref = _render(rend, batch, False, **kw)"),
    "VDN_TRAIN_COLOR_FUSED": _held("tests/test_gpu_train_parity.py::test_colour_head_inside_the_training_forward_launch", "for fused in (\"1\", \"0\"):", values=("1",)),
    "VDN_SDF_TAIL": _held("tests/test_gpu_parity.py::test_sdf_tail_kernel_equals_the_large_kernel_bit_for_bit", "for mode in (\"0\", \"1\"):", values=("0", "1")),
    "VDN_SDF_TAIL_ROW0": _held("tests/test_gpu_parity.py::test_sdf_tail_kernel_equals_the_large_kernel_bit_for_bit", "for mode in (\"0\", \"1\"):", values=("16384", "4096", "0")),
    "VDN_SDF_TAIL_MAX": _held("tests/test_gpu_parity.py::test_sdf_tail_kernel_equals_the_large_kernel_bit_for_bit", "for mode in (\"0\", \"1\"):", values=("40000",)),
    "VDN_SHADE_POINTS_FUSED": _held("tests/test_gpu_shade_points.py::test_fused_point_shading_equals_the_separate_launches", "sdf0, grad0, col0 = _shade(rend, x, False)"),
    # ---- backward and the weight-gradient GEMM
    # (tests/test_gpu_stream_order.py sets VDN_BWD_SPLIT_DW=0 in the delayed AND the serial arm: never against the default. Bits:
    # the one launch carries the same descriptors - entries, splits, slabs - as the launches per group, vdn_hip/train.py: dw_group)
    "VDN_BWD_SPLIT_DW": _matrix(("0",), ("render_grad",), "monkeypatch", taken_bwd_split_dw),
    "VDN_SDF_BWD_SPLIT": _held("tests/test_gpu_grads.py::test_one_launch_sdf_backward_equals_rbar_then_fbar", "for mode in (\"0\", \"1\"):"),
    "VDN_RELU_MASK": _held("tests/test_gpu_relu_masks.py::test_masked_step_is_bit_identical", "trs = [_trainer(monkeypatch, m, wdepth, B) for m in (False, True)]"),
    # rounding, all five: the value is the rows per K split, `splits = max(1, (K + pps - 1) // pps)` and `splits += splits % 2`
    # (vdn_hip/train.py:204-206) - the same fp32-accumulated products, partitioned into other slabs and summed by the finalize pass
    "VDN_DW_SPLIT_PTS": _matrix(_SPLIT_VALUES, ("step_bf16",), "child",                                            # (read at import)
                                _taken_splits(("fg", "heads", "bg"), ()), "rounding"),
    "VDN_DW_SPLIT_PTS_SDF": _matrix(_SPLIT_VALUES, ("step_bf16", "step_fp32"), "monkeypatch", _taken_splits(("fg",), ("fg",)), "rounding"),
    "VDN_DW_SPLIT_PTS_REST": _matrix(_SPLIT_VALUES, ("step_bf16", "step_fp32"), "monkeypatch",
                                     _taken_splits(("heads", "bg"), ("heads", "bg")), "rounding"),
    "VDN_DW_SPLIT_PTS_NERF": _matrix(_SPLIT_VALUES, ("step_bf16",), "monkeypatch", _taken_splits(("bg",), ()), "rounding"),
    "VDN_DW_SPLIT_PTS_HEADS": _matrix(_SPLIT_VALUES, ("step_bf16",), "monkeypatch", _taken_splits(("heads",), ()), "rounding"),
    # ---- the Trainer's schedule and data parallelism
    "VDN_SIDE_STREAM": _held("tests/test_gpu_stream_order.py::test_schedule_equals_the_serial_arm", "ref, got = cases.get(sk.ref_spec(spec)), cases.get(spec)"),
    "VDN_OVERLAP": _matrix(("0",), ("step_bf16",), "monkeypatch", taken_overlap),
    "VDN_SPLIT_REST": _matrix(("0",), ("step_bf16",), "monkeypatch", taken_split_rest),
    "VDN_EVENT_TRIM": _matrix(("0",), ("step_bf16",), "monkeypatch", taken_event_trim),
    "VDN_FUSED_COMPOSITE": _held("tests/test_gpu_train_parity.py::test_fused_compositor_launch_is_bit_identical_to_the_four_launches", "for fused in (\"1\", \"0\"):"),
    # (tests/test_gpu_dp.py runs VDN_DP_FUSED=0 at two ranks against one process, within a tolerance, not against the default arm)
    "VDN_DP_FUSED": _matrix(("0",), ("dp_one_rank",), "dp_child", taken_dp_fused),
    "VDN_DP_SIDE_GROUP": _matrix(("0",), ("dp_one_rank",), "dp_child", taken_dp_side_group),
    "VDN_DP_INSTREAM": _matrix(("0",), ("dp_one_rank",), "dp_child", taken_dp_instream),
    # ---- graphs, engines, precision
    "VDN_RENDER_GRAPHS": _held("tests/test_gpu_runner_flow.py::test_graph_replayed_steps_equal_eager_steps", "monkeypatch.setenv(\"VDN_RENDER_GRAPHS\", \"1\" if graphs else \"0\")"),
    "VDN_RENDER_GRAPH": _matrix(("1",), ("image_loop",), "monkeypatch", taken_render_graph),
    "VDN_RENDER_ENGINES": _matrix(("1",), ("render_grad",), "monkeypatch", taken_render_engines),
    # (as a default: render_inf builds one renderer without `precision`; bits against the renderer built WITH that precision)
    "VDN_PRECISION": _matrix(("bf16",), ("render_inf",), "child", taken_precision),
    # ---- meshes (tets is another triangulation: bits against extract_geometry(method="tets"), the default against method="cubes")
    "VDN_MESH_METHOD": _matrix(("tets",), ("geometry",), "monkeypatch", taken_mesh_method),
    "VDN_MESH_SPARSE": _held("tests/test_gpu_mesh_sparse.py::test_network_extraction_is_equal", "monkeypatch.delenv(\"VDN_MESH_SPARSE\", raising=False)", values=("8:2.5",)),
    # ---- development: another build of the library, not an arm of this one
    "VDN_LIB": dict(values=(), relation=None, held_by=None, reason="loads another build of the library: not an arm of this one"),
    "VDN_BUILD_VARIANT": dict(values=(), relation=None, held_by=None, reason="builds and loads a side copy of the library with other flags: not an arm of this one"),
    # ---- read by the library (getenv, once per process): a fresh child per arm; which kernel a launch picked is not visible from Python
    "VDN_SDF2_WARM": _matrix(("0",), ("step_bf16", "render_inf"), "child", None, native="csrc/k_sdf_fwd2.h:740"),
    "VDN_PLANE_PREFETCH": _matrix(("1",), ("step_fp32", "step_bf16_two_chain"), "child", None, native="csrc/k_sdf_bwd.h:285"),
    "VDN_SDF0_SPLIT_MAX": _matrix(("0",), ("render_inf", "step_bf16"), "child", None, native="csrc/sdf_bf16.hip:15"),
}

def further_than_twice(dist):
    """The fp64 fallback of the "rounding" relation: dist = [(tensor, max|default - fp64|, max|arm - fp64|)] -> the rows whose arm
    stands more than 2 x as far from fp64 as the default arm (a tensor both arms hit exactly passes; an arm off where the default is
    exact does not)."""
    return [(n, d0, d1) for n, d0, d1 in dist if not d1 <= 2.0 * d0]


# the fp64 tests the library's own arms run under as well (bit equality with the default says the arm is no worse; the plane models
# say it is right): (switch, value) -> pytest selection
FP64_UNDER_ARM = {
    ("VDN_PLANE_PREFETCH", "1"): ["-m", "gpu", "-k", "test_sdf_backward_blocks_vs_float64_layer_models",
                                  "tests/test_gpu_mlp_planes.py", "tests/test_gpu_mlp_planes_f32.py"],
    ("VDN_SDF2_WARM", "0"): ["-m", "gpu", "-k", "test_sdf_forward_planes_vs_float64_layer_models",
                             "tests/test_gpu_mlp_planes.py", "tests/test_gpu_mlp_planes_f32.py"],
    ("VDN_SDF0_SPLIT_MAX", "0"): ["-m", "gpu", "tests/test_gpu_sdf_value_launches.py"],
}


# ------------------------------------------------------------------------------------------------------------------------
# scenarios
# ------------------------------------------------------------------------------------------------------------------------
OBS = {}


def _g(x, dev):
    import numpy as np
    import torch
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev).contiguous()


def _dw_columns(eng):
    """The K splits of every entry of the engine's weight-gradient descriptor table, with what dw_layout sized them on."""
    import numpy as np
    from vdn_hip import lib, train
    grp = eng.groups["all"]
    rows = np.frombuffer(grp.dw.cpu().numpy().tobytes(), dtype=lib.struct_dtype("VdnDwDesc"))[:grp.n_dw]
    fin = np.frombuffer(grp.fin.cpu().numpy().tobytes(), dtype=lib.struct_dtype("VdnDwFinalizeDesc"))[:grp.n_dw]
    assert [int(x) for x in fin["splits"]] == [int(x) for x in rows["splits"]]          # the finalize pass sums what the GEMM wrote
    return dict(dw_kind=list(eng.dw_list_kind), dw_P=[int(x) for x in rows["P"]], dw_segs=[2 if int(x) else 1 for x in rows["A2"]],
                dw_splits=[int(x) for x in rows["splits"]],
                pps={k: train._pts_per_split(n, eng.precision) for k, n in (("fg", "sdf"), ("heads", "heads"), ("bg", "nerf"))})


def _step(dev, precision, wdepth, steps):
    """The Trainer on the scene of tests/stream_skew.py T2 (B = 160 full-frame rays: both work lists ragged, the foreground list
    with both classes), the depth term on from the first step."""
    import torch
    import stream_skew as sk
    from vdn_train import factory
    from vdn_train.trainer import Trainer
    conf = dict(sk._BASE)
    if wdepth:
        conf.update(extract_depth=True, depth_start_iter=-1)
    inputs, extra = sk._step_inputs(11, steps, "T2", feats=wdepth)
    torch.manual_seed(0)
    rend = factory.build_renderer(wdepth=wdepth, device=dev, precision=precision)
    tr = Trainer(rend, sk.B, dev, conf=conf)
    eng = tr.engine
    out = {}
    for it in range(steps):
        x = inputs[it]
        sc = tr.train_step(*x["args"], t_rand=x["t_rand"], t_rand_out=x["t_rand_out"], **extra)
        out["scalars/%d" % it] = sc.clone()
        if it == 0:
            out["grad_flat"] = eng.grad_flat.clone()
            cnt = eng._fg_cnt.tolist()
            OBS.update(fg_listed=cnt[0], fg_inner=cnt[1], bg_listed=int(eng.w["bg_active"][1].item()), P=eng.P, Q=eng.Q)
    out["param_flat"] = tr.param_flat.clone()
    OBS.update(_dw_columns(eng))
    OBS.update(steps=steps, precision=precision, wdepth=bool(wdepth), overlap=bool(tr.overlap), side=eng._side is not None, relu_mask=bool(eng.relu_mask),
               param_sizes=[int(p.numel()) for p in eng.params])
    return out


def step_bf16(dev):
    """Trainer, bf16, VDN head and depth term on, 3 steps: scalars of each step, grad_flat after step 1, param_flat after step 3."""
    return _step(dev, "bf16", True, 3)


def step_fp32(dev):
    """The same on the fp32 kernels without the VDN head, 1 step (vdn_sdf_bwd_rbar_f32 / fbar_f32)."""
    out = _step(dev, "fp32", False, 1)
    assert "vdn_sdf_bwd_rbar_f32" in _LOG_NOW() and "vdn_sdf_bwd_fbar_f32" in _LOG_NOW()
    return out


def step_bf16_two_chain(dev):
    """step_bf16 for 1 step with VDN_SDF_BWD_SPLIT=0: the bf16 rbar + fbar chains."""
    import stream_skew as sk
    with sk.environ(VDN_SDF_BWD_SPLIT="0"):
        out = _step(dev, "bf16", True, 1)
    assert "vdn_sdf_bwd_rbar_bf16" in _LOG_NOW() and "vdn_sdf_bwd_fbar_bf16" in _LOG_NOW()
    return out


def _rays(seed, step, B, dev):
    from vdn_train import synth
    cams = synth.make_cameras(seed)
    o, d = synth.random_pixel_batch(seed, step, step % len(cams), B, cams=cams)
    near, far = synth.near_far_from_sphere(o, d)
    t1, t2 = synth.jitter(seed, step, B)
    return [_g(x, dev) for x in (o, d, near, far)], dict(t_rand=_g(t1, dev), t_rand_out=_g(t2, dev)), (o, d)


def render_inf(dev):
    """render() under no_grad, VDN head on, bf16 and fp32, B = 77 and 130, injected jitter: every output. And one renderer built
    WITHOUT `precision` on the same weights (key "env": what VDN_PRECISION, or the networks' own fp32, gives), B = 77."""
    import torch
    from vdn_train import synth, factory
    from dpt_models.renderer import NeuSRenderer
    st = synth.make_all_states(3, wdepth=True)
    bg = torch.ones(1, 3, device=dev)
    out = {}

    def leg(tag, rend, sizes):
        for B in sizes:
            rays, jit, _ = _rays(3, 1, B, dev)
            with torch.no_grad():
                res = rend.render(*rays, background_rgb=bg, cos_anneal_ratio=0.6, **jit)
            for k, v in res.items():
                if torch.is_tensor(v):
                    out["%s/%d/%s" % (tag, B, k)] = v.clone()
    for precision in ("bf16", "fp32"):
        leg(precision, factory.build_renderer(wdepth=True, device=dev, states=st, precision=precision), (77, 130))
    r = factory.build_renderer(wdepth=True, device=dev, states=st, precision="fp32")
    plain = NeuSRenderer(r.nerf, r.sdf_network, r.deviation_network, r.color_network, r.depth_network, **factory.CONF["neus_renderer"])
    OBS["env_precision"] = plain.sdf_network.precision
    assert len({m.precision for m in (plain.nerf, plain.sdf_network, plain.color_network, plain.depth_network)}) == 1
    leg("env", plain, (77,))
    return out


def render_grad(dev):
    """The drop-in flow: render() under grad + the runner's loss + backward(), bf16 with the VDN head, twice at B = 77 (the second
    call is the _TrainPlan replay), twice at B = 130, once more at B = 77 (its engine is still alive, or has to be built again):
    the outputs and the flat .grad of every call."""
    import torch
    from vdn_train import synth, factory
    from vdn_hip import train
    torch.manual_seed(0)
    rend = factory.build_renderer(wdepth=True, device=dev, precision="bf16")
    params = rend._all_parameters()
    bg = torch.ones(1, 3, device=dev)
    built, init = [], train.TrainEngine.__init__

    def counted(self, *a, **k):
        built.append(1)
        init(self, *a, **k)
    train.TrainEngine.__init__ = counted
    out = {}
    try:
        for call, B in enumerate((77, 77, 130, 130, 77)):
            rays, jit, (o, d) = _rays(13, call, B, dev)
            rgb = _g(synth.target_colors(o, d, 0.5), dev)
            feats = _g(synth.uniform(13, "arms/feats/%d" % call, (B, 96)), dev)
            res = rend.render(*rays, background_rgb=bg, cos_anneal_ratio=0.5, **jit)
            loss = ((res["color_fine"] - rgb).abs().sum() / B + 0.1 * res["gradient_error"]
                    + 0.3 * (res["render_feats"] - feats).abs().sum() / B)
            for p in params:
                p.grad = None
            loss.backward()
            for k, v in res.items():
                if torch.is_tensor(v):
                    out["call%d/%s" % (call, k)] = v.detach().clone()
            out["call%d/grad" % call] = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).reshape(-1) for p in params])
    finally:
        train.TrainEngine.__init__ = init
    OBS.update(engines=len(rend._engines), engines_built=len(built))
    return out


def image_loop(dev):
    """validate.render_image on a 20 x 14 image in batches of 64 with the jitter off: four full batches and a ragged one of 24 rays
    (n >= 2 * batch_size holds) -> img_fine, gradient_error, weight_depth."""
    import numpy as np
    import torch
    from vdn_train import synth, factory, validate
    from vdn_train.rays import RaysGenerator
    H, W, BS = 14, 20, 64
    K = np.eye(4)
    K[0, 0] = K[1, 1] = synth.FOCAL * W / synth.W_IMG
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    gen = RaysGenerator(synth.uniform(7, "arms/images", (1, H, W, 3)).astype(np.float32), None, synth.make_cameras(7)[:1], K, device=dev)
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(7), precision="bf16")
    rend.perturb = 0
    plans, make = [], rend.plan

    def plan(*a, **k):
        plans.append(make(*a, **k))
        return plans[-1]
    rend.plan = plan
    assert H * W >= 2 * BS and H * W % BS == 24
    res = validate.render_image(rend, gen, 0, resolution_level=1, batch_size=BS, cos_anneal_ratio=0.8, gen_depth_for_finetune=True)
    OBS.update(plans=len(plans), captures=sum(p.captures for p in plans))
    return {k: torch.from_numpy(np.ascontiguousarray(res[k])) for k in ("img_fine", "gradient_error", "weight_depth")}


def geometry(dev):
    """extract_geometry at resolution 32, as the environment says ("env") and with `method` given: vertices and faces."""
    import numpy as np
    import torch
    import stream_skew as sk
    from vdn_train import synth, factory
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(5), precision="fp32")
    lo, hi = torch.tensor([-1.01, -1.01, -1.01]), torch.tensor([1.01, 1.01, 1.01])
    out = {}
    for tag, method in (("env", None), ("cubes", "cubes"), ("tets", "tets")):
        with sk.Skew(torch.cuda.current_stream(dev)) as h:
            v, f = rend.extract_geometry(lo, hi, resolution=32, threshold=0.0, method=method)
        OBS["log_" + tag] = [n for _, n, _ in h.log]
        assert v.shape[0] > 0 and f.shape[0] > 0, tag
        out[tag + "/vertices"], out[tag + "/faces"] = torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(f))
    return out


SCENARIOS = {f.__name__: f for f in (step_bf16, step_fp32, step_bf16_two_chain, render_inf, render_grad, image_loop, geometry)}
# (dp_one_rank is no function of this table: it is the one-rank child of tests/test_gpu_dp.py, started by dp_one_rank below)
SCENARIO_NAMES = tuple(SCENARIOS) + ("dp_one_rank",)

_RUN = {}


def _LOG_NOW():
    return [n for _, n, _ in _RUN["skew"].log]


def run(name, dev=None):
    """One scenario under the launch log -> ({key: CPU tensor}, observations). observations["log"]: the entry points in launch
    order; ["events"]: torch.cuda.Event.record calls; plus what the scenario left in OBS."""
    import torch
    import stream_skew as sk
    dev = torch.device("cuda:0") if dev is None else dev
    OBS.clear()
    record, n_ev = torch.cuda.Event.record, [0]

    def counting(self, *a, **k):
        n_ev[0] += 1
        return record(self, *a, **k)
    torch.cuda.Event.record = counting
    t0 = time.time()
    try:
        with sk.Skew(torch.cuda.current_stream(dev)) as h:
            _RUN["skew"] = h
            out = SCENARIOS[name](dev)
            torch.cuda.synchronize()
    finally:
        torch.cuda.Event.record = record
        _RUN.pop("skew", None)
    obs = dict(OBS, log=[n for _, n, _ in h.log], events=n_ev[0], wall_s=time.time() - t0)
    return {k: v.detach().cpu() for k, v in out.items()}, json.loads(json.dumps(obs))


def save(path, tensors, obs):
    import numpy as np
    arrays = {k.replace("/", "__"): v.numpy() for k, v in tensors.items()}
    np.savez(path, __obs__=np.array(json.dumps(obs)), **arrays)


def load(path):
    import numpy as np
    import torch
    with np.load(path, allow_pickle=False) as z:
        obs = json.loads(str(z["__obs__"]))
        return {k.replace("__", "/"): torch.from_numpy(z[k]) for k in z.files if k != "__obs__"}, obs


# ------------------------------------------------------------------------------------------------------------------------
# the one-rank data-parallel child: tests/test_gpu_dp.py's own worker, with the collectives' attributes and the launch log reported
# ------------------------------------------------------------------------------------------------------------------------
class _Sink:
    def __init__(self):
        self.items = []

    def put(self, x):
        self.items.append(x)


class _DefaultStream:
    cuda_stream = 0


def dp_one_rank_worker(port, q, backend):
    """_one_rank_worker of tests/test_gpu_dp.py (a one-rank group, four steps of a Trainer with the collective path forced on in
    lockstep with one without collectives, bit for bit) -> its own result + what the enabled Collectives was built as + the log."""
    import torch  # noqa: F401  (before the library)
    import stream_skew as sk
    import test_gpu_dp
    from vdn_train import dp
    seen, init = [], dp.Collectives.__init__

    def recording(self, *a, **k):
        init(self, *a, **k)
        seen.append(dict(enabled=bool(self.enabled), instream=bool(self.instream), side_group_own=self.side_group is not self.group))
    dp.Collectives.__init__ = recording
    sink = _Sink()
    # (the worker makes its process group before anything touches the GPU: the log's caller stream is named by its handle, 0)
    with sk.Skew(_DefaultStream()) as h:
        test_gpu_dp._one_rank_worker(port, sink, backend)
    on = [c for c in seen if c["enabled"]]
    assert len(seen) == 2 and len(on) == 1, seen
    q.put((sink.items[0], dict(on[0], log=[n for _, n, _ in h.log])))


def dp_one_rank(backend="nccl", timeout=600):
    """Start dp_one_rank_worker in a spawned process under the current environment -> (exit code or None if it did not end,
    (same, loss, gmax) or None, observations or None). Nothing is retried."""
    import queue
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=dp_one_rank_worker, args=(port, q, backend))
    p.start()
    deadline, got = time.time() + timeout, None
    while got is None and time.time() < deadline:
        try:
            got = q.get(timeout=0.2)
        except queue.Empty:
            if not p.is_alive():
                break
    p.join(timeout=max(1.0, deadline - time.time()))
    if p.is_alive():
        p.kill()
        p.join()
        return None, None, None
    return p.exitcode, (got[0] if got else None), (got[1] if got else None)


def main(argv):
    name, path = argv
    tensors, obs = run(name)
    save(path, tensors, obs)
    print("switch_arms: %s in %.2f s -> %s" % (name, obs["wall_s"], path))


if __name__ == "__main__":
    main(sys.argv[1:])
