"""The fp32 forms of the one-layer models (oracle/mlp_ops.py: sdf_plane_models_f32, sdf_bwd_models_f32, and the f32 = True forms of
the heads' and the background network's models), proven without a GPU, as tests/test_mlp_ops_model_cpu.py proves the bf16 forms:
the chains of fp32-form models on unrounded weight images, fed their own unrounded outputs in float64, ARE the networks of
oracle/neus_oracle.py and their torch autograd gradients (the double backward and the s_from_h = 1 form included) to 1e-10; the
fmt-0 chunk decoder inverts the documented layout; mfma_chain_f32 is the documented k order, one rounding per product; the
comparator accepts the float32 stand-in - the chain-ordered float32 model run through its own planes - in every case (the floors
are printed: pytest -rA) and rejects it with each planted defect at the plane the defect is in; the other weight state is rejected."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import mlp_cases, mlp_ops, neus_oracle as orc

SDF_NAMES = list(mlp_cases.SDF_CASES) + list(mlp_cases.SDF_F32_CASES)
F32, F64 = torch.float32, torch.float64
exact = lambda a: np.asarray(a, np.float64)


def _sdf_streams():
    from vdn_hip import images
    return images.sdf_streams(3, 257, 256, 8, (4,), 6, scaled=False)


@functools.lru_cache(maxsize=None)
def _sdf(state="init", rounded=True):
    """(ops, sweep ops, fbar ops, w8row) of an SDF state: as the fmt-0 blob holds them, or unrounded in float64."""
    sd = mlp_cases.states(state)["sdf_network_fine"]
    host = mlp_ops.HostImages.of_sdf_state(sd, _sdf_streams(), np.float32 if rounded else np.float64)
    return mlp_ops.sdf_ops_f32(host, rounded) + (host.weff["lin8"][0].astype(np.float64),)


def _copy(ops):
    return [dict(o, W=o["W"].copy(), b=o["b"].copy()) for o in ops]


# ---- the decoder and the chain ----------------------------------------------------------------------------------------------

def test_f32_chunk_decoder_inverts_the_documented_layout():
    """A chunk written element by element from the layout at the top of csrc/mlp_engine.h: [kt * 4 groups][64 lanes][4 f32], lane
    (i, h) of group g holding W[i][8 g + 4 h .. + 3]; 32 f32 of bias at byte kt * 4096."""
    from vdn_hip import layout
    kt = 3
    rs = np.random.RandomState(1)
    W, bias = rs.standard_normal((32, 32 * kt)).astype(np.float32), rs.standard_normal(32).astype(np.float32)
    words = np.zeros(kt * 4 * 64 * 4, np.float32)
    for g in range(kt * 4):
        for lane in range(64):
            i, h = lane & 31, lane >> 5
            for e in range(4):
                words[(g * 64 + lane) * 4 + e] = W[i, 8 * g + 4 * h + e]
    chunk = torch.cat([torch.from_numpy(words).view(torch.uint8), torch.from_numpy(bias).view(torch.uint8), torch.zeros(896, dtype=torch.uint8)])
    assert chunk.numel() == kt * 4096 + 1024
    Wd, bd = layout.decode_chunk_f32(chunk, kt)
    assert np.array_equal(Wd.numpy(), W) and np.array_equal(bd.numpy(), bias)


def test_the_chain_is_the_documented_k_order_one_rounding_per_product():
    assert mlp_ops.mfma_k_order(16).tolist() == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]
    rs = np.random.RandomState(2)
    x, W, b = ((rs.standard_normal(s) * 10.0 ** rs.randint(-3, 4, s)).astype(np.float32) for s in ((5, 64), (7, 64), (7,)))
    want = np.zeros((5, 7), np.float32)
    for p in range(5):
        for n in range(7):
            acc = np.float32(b[n])
            for g in range(8):
                for j in range(4):
                    for k in (8 * g + j, 8 * g + 4 + j):
                        acc = np.float32(float(acc) + float(W[n, k]) * float(x[p, k]))       # (the product is exact in float64)
            want[p, n] = acc
    assert np.array_equal(mlp_ops.mfma_chain_f32(x, W, b), want.astype(np.float64))
    # the order matters (so a floor from another order would not be this kernel's), and the chain's error is a float32 one
    plain = (torch.tensor(x) @ torch.tensor(W).T + torch.tensor(b)).double().numpy()
    ref = x.astype(np.float64) @ W.astype(np.float64).T + b
    assert not np.array_equal(plain, mlp_ops.mfma_chain_f32(x, W, b))
    assert np.abs(mlp_ops.mfma_chain_f32(x, W, b) - ref).max() <= 64 * 2.0 ** -24 * (np.abs(x.astype(np.float64)) @ np.abs(W.astype(np.float64)).T).max()


def test_fmt0_operand_weights_are_one_float32_rounding_of_the_scaled_weight():
    sd = mlp_cases.states()["sdf_network_fine"]
    host = mlp_ops.HostImages.of_sdf_state(sd, _sdf_streams())
    o4 = mlp_ops.operand_weights(host, "full", 4, fmt=0)
    w = host.weff["lin4"]
    assert o4["W"].shape == (256, 288) and o4["kt"] == 9
    assert np.array_equal(o4["W"][:, :217], (np.float32(1.0 / math.sqrt(2.0)) * w[:, :217]).astype(np.float64))
    assert np.array_equal(o4["W"][:, 224:263], (np.float32(1.0 / math.sqrt(2.0)) * w[:, 217:]).astype(np.float64))
    assert not o4["W"][:, 217:224].any() and not o4["W"][:, 263:].any() and o4["tail"] is None
    assert np.array_equal(o4["b"], sd["lin4.bias"].astype(np.float64))
    o3 = mlp_ops.operand_weights(host, "full", 3, fmt=0)       # nmap of lin3: rows 217..223 of the image are zero, bias too
    assert o3["W"].shape == (224, 256) and not o3["W"][217:].any() and not o3["b"][217:].any()


# ---- the chain of fp32-form models is the network and its gradients ---------------------------------------------------------

def _exact_forward(c, state="init"):
    ops, osw, ofb, w8 = _sdf(state, rounded=False)
    return mlp_ops.simulate_sdf_forward_f32(ops, osw, w8, c["pts"], c["scale"], F64, exact, aten_threshold=True)


@pytest.mark.parametrize("name", ["uniform-P33-s1.5", "lattice-P33-s1"])
def test_chain_of_f32_form_models_equals_the_oracle_and_its_gradient(name):
    c = mlp_cases.sdf_case(name)
    sd = mlp_cases.states()["sdf_network_fine"]
    planes = _exact_forward(c)
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in sd.items()}
    ref, grad = orc.sdf_forward(p, torch.tensor(c["pts"].astype(np.float64)), orc.SDFConf(scale=c["scale"]), with_gradient=True)
    for got, want in ((planes["sdf"], ref[:, 0].numpy()), (planes["feat"], ref[:, 1:].numpy()), (planes["normals"], grad.numpy())):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("s_mode", [0, 1])
@pytest.mark.parametrize("kind", mlp_cases.SDF_UPSTREAM)
def test_chain_of_f32_form_backward_models_equals_autograd_of_the_oracle(kind, s_mode):
    """pe_jacobian, sdf_rbar_step and sdf_fbar_step in the network's units (ex_factor = 100) with softplus' read from the S planes
    (s_mode 0) or formed as 1 - exp(-100 h) from the H planes (s_mode 1), fed the exact forward and their own outputs in float64:
    the column sums of the ab blocks are the bias gradients torch autograd gives for loss = g_sdf . sdf + g_feat . feat +
    g_n . (d sdf / d x) - a double backward -, and sdf_d_pts_model is d loss / d x."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    sd = mlp_cases.states()["sdf_network_fine"]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    p = {k: t(v, k.endswith(".bias")) for k, v in sd.items()}
    x = t(c["pts"], True)
    out, grad = orc.sdf_forward(p, x, orc.SDFConf(scale=c["scale"]), with_gradient=True)
    ((out[:, 0] * t(g_sdf)).sum() + (out[:, 1:] * t(g_feat)).sum() + (grad * t(g_n)).sum()).backward()
    ops, osw, ofb, w8 = _sdf("init", rounded=False)
    f = _exact_forward(c)
    S = [f["%s%d" % ("H" if s_mode else "S", l)] for l in range(8)]
    V = [f["V%d" % l] for l in range(8)]
    ub, EX, ab = mlp_ops.simulate_sdf_backward(ops, ofb, c["pts"], c["scale"], g_sdf, g_feat, g_n, S, V, rnd=exact, dtype=F64,
                                               ex_factor=100.0, s_mode=s_mode, aten_threshold=True)
    for l in range(8):
        want = p["lin%d.bias" % l].grad.numpy()
        got = ab[l].sum(0)[:len(want)]
        assert np.abs(got - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-300), (l, np.abs(got - want).max(), np.abs(want).max())
    want = p["lin8.bias"].grad.numpy()
    assert np.abs(np.concatenate([ab[8].sum(0)[256:257], ab[8].sum(0)[:256]]) - want).max() <= 1e-10 * np.abs(want).max()
    m = mlp_ops.sdf_d_pts_model(ofb, c["pts"], c["scale"], g_n, f["U_pe"], ab[0], ab[4], f32=True)
    assert np.abs(m["y64"] - x.grad.numpy()).max() <= 1e-10 * np.abs(x.grad.numpy()).max()
    if kind == "g_normals=0":
        assert all((b == 0).all() for b in ub) and all((e == 0).all() for e in EX)


# ---- the SDF forward: the stand-in passes, the planted defects do not -------------------------------------------------------

def _sim(c, ops=None, osw=None, **kw):
    o, s, _, w8 = _sdf(c["state"])
    return mlp_ops.simulate_sdf_forward_f32(ops or o, osw or s, w8, mlp_cases.rows_of(c), c["scale"], **kw)


def _promised(planes):
    return {k: (v[:, :217] if k in ("H3", "S3", "V3") else v) for k, v in planes.items()}


def _judged(c, planes):
    o, s, _, w8 = _sdf(c["state"])
    planes = _promised(planes)
    return mlp_ops.judge_planes(mlp_ops.sdf_plane_models_f32(o, s, w8, mlp_cases.rows_of(c), c["scale"], planes), planes)


@functools.lru_cache(maxsize=None)
def _sim_cached(name):
    c = mlp_cases.sdf_case(name)
    return c, _sim(c)


@pytest.mark.parametrize("name", SDF_NAMES)
def test_sdf_comparator_accepts_the_float32_stand_in_and_prints_the_floors(name):
    c, planes = _sim_cached(name)
    res = _judged(c, planes)
    assert len(res) == 29
    for k, j in res.items():
        print("%-22s %-7s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
        assert j["ok"] and j["err"] <= j["bound"], (name, k, j)


def test_a_pre_activation_of_exactly_zero_pins_h_and_s():
    """The silenced unit (state "silent"): a = 0 exactly, the float64 model gives S = 1/2 and H = ln 2 / 100, and the float32
    evaluation of the documented formula gives S = 0.5 and H = float32(ln 2 / 100) exactly: 2^-0 = 1, 1 / 2 and log2 2 are exact."""
    c, planes = _sim_cached("silent-P33-s1")
    l, u = mlp_cases.SDF_SILENT
    o, s, _, w8 = _sdf("silent")
    assert not o[l]["W"][u].any() and o[l]["b"][u] == 0
    assert (planes["S%d" % l][:, u] == 0.5).all() and (planes["H%d" % l][:, u] == np.float32(0.0069314718055994529)).all()
    m = mlp_ops.sdf_plane_models_f32(o, s, w8, c["pts"], c["scale"], _promised(planes))
    assert (m["S%d" % l]["y64"][:, u] == 0.5).all() and np.abs(m["H%d" % l]["y64"][:, u] - math.log(2.0) / 100.0).max() < 1e-18
    # the branch a >= 0 ? r : e r taken the other way at 0 still gives 1/2 (e = 1): the boundary is continuous, the value pinned


def _plant_k_column(o):
    o[2]["W"][:, 5] = 0.0
    return ["H2", "S2"]


def _plant_bias(o):
    o[5]["b"][:] = 0.0
    return ["H5", "S5"]


def _plant_skip_scale(o):
    o[4]["W"] = mlp_ops.f32_rne(o[4]["W"] * math.sqrt(2.0))
    return ["H4", "S4"]


FWD_PLANTS = {"dropped-k-column": _plant_k_column, "bias-left-out": _plant_bias, "layer-4-without-1/sqrt2": _plant_skip_scale}


@pytest.mark.parametrize("name", ["uniform-P33-s1.5", "lattice-P33-s1", "hot-P129-s1"])
@pytest.mark.parametrize("plant", list(FWD_PLANTS))
def test_sdf_comparator_rejects_each_planted_weight_defect(name, plant):
    """The stand-in evaluated with the defect in its forward operand weights, judged against the models of the true weights:
    rejected at the planes the defect is in and - teacher forcing - at no other."""
    c = mlp_cases.sdf_case(name)
    wrong = _copy(_sdf(c["state"])[0])
    where = FWD_PLANTS[plant](wrong)
    res = _judged(c, _sim(c, ops=wrong))
    for k, j in res.items():
        assert j["ok"] == (k not in where), (name, plant, k, j)


@pytest.mark.parametrize("defect,where", [("s-negated", "S0"), ("upe-without-u4", "U_pe"), ("hw-trig", "PE")])
def test_sdf_comparator_rejects_each_planted_formula_defect(defect, where):
    """S taken as sigmoid(-100 a); the PE part of u_4 left out of U_pe; the hardware-trig error the bf16 contract allows its
    encoding (2^-18 absolute), which the fp32 contract does not. One plane suffices; no plane BEFORE it complains."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    res = _judged(c, _sim(c, defect=defect))
    order = list(res)
    assert not res[where]["ok"], (defect, res[where])
    if defect != "s-negated":                            # (every S plane is wrong then, and with it every V plane)
        for k in order:
            if k != where and not (defect == "hw-trig" and k in ("H0", "S0", "H4", "S4", "normals")):
                assert res[k]["ok"], (defect, k, res[k])


def test_sdf_comparator_rejects_a_plane_rounded_to_bf16():
    """Any plane rounded to bf16 - here each in turn, the others left as they are -: a bf16 rounding moves an element by up to
    2^-9 of itself, tens of thousands of units."""
    c, base = _sim_cached("uniform-P33-s1.5")
    o, s, _, w8 = _sdf(c["state"])
    models = mlp_ops.sdf_plane_models_f32(o, s, w8, c["pts"], c["scale"], _promised(base))
    for k in base:
        planes = dict(_promised(base))
        planes[k] = mlp_ops.bf16_rne(planes[k])
        j = mlp_ops.judge_planes({k: models[k]}, planes)[k]
        assert not j["ok"] and j["err"] > 100.0, (k, j)


def test_sdf_comparator_rejects_work_list_saves_written_at_the_dense_row():
    """The work-list case with its saves where a dense launch would put them: row q holding point q instead of point
    active_idx[q]. Every plane behind another is consistent with it - teacher forcing -; the planes made from the inputs, PE and
    the normals (J_PE at the point), show it."""
    c = mlp_cases.sdf_case("worklist-P200-n77-s1")
    dense = dict(c, active_idx=None, n_active=None)
    planes = {k: v[:c["n_active"]] for k, v in _sim(dense).items()}
    res = _judged(c, planes)
    assert not res["PE"]["ok"] and not res["normals"]["ok"] and res["PE"]["err"] > 1e3


def test_the_other_sdf_weight_state_is_rejected():
    """What the GPU test's wiring check relies on."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    o, s, _, w8 = _sdf("other")
    res = _judged(c, mlp_ops.simulate_sdf_forward_f32(o, s, w8, c["pts"], c["scale"]))
    free = ("PE", "normals", "sdf", "V7")                # (no weights; the geometric init's constant row of W_8 in both states)
    assert res["PE"]["ok"] and res["normals"]["ok"] and all(not res[k]["ok"] and res[k]["err"] > 1e3 for k in res if k not in free)


# ---- the SDF backward ---------------------------------------------------------------------------------------------------------

def _bwd_args(c, kind):
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    return mlp_cases.rows_of(c), c["scale"], g_sdf[sel], g_feat[sel], g_n[sel]


def _bwd_judged(c, kind, s_mode, fwd, ub, EX, ab, d_pts=None, before=None):
    o, _, ofb, _ = _sdf(c["state"])
    S = [fwd["%s%d" % ("H" if s_mode else "S", l)] for l in range(8)]
    V = [fwd["V%d" % l] for l in range(8)]
    pts, scale, g_sdf, g_feat, g_n = _bwd_args(c, kind)
    models = mlp_ops.sdf_bwd_models_f32(o, ofb, pts, scale, g_sdf, g_feat, g_n, S, s_mode, V, ub, EX, ab)
    planes = {"ub0": ub[0][:, :39], "ub4pe": ub[4][:, 224:263], "ab8": ab[8][:, :257]}
    for l in range(8):
        w = 217 if l == 3 else 256
        planes["ub%d" % (l + 1)], planes["EX%d" % l], planes["ab%d" % l] = ub[l + 1][:, :w], EX[l][:, :w], ab[l][:, :w]
    if d_pts is not None:
        models["d_pts"] = mlp_ops.sdf_d_pts_model(ofb, pts, scale, g_n, fwd["U_pe"], ab[0], ab[4], f32=True, before=before)
        planes["d_pts"] = d_pts
    return mlp_ops.judge_planes(models, planes)


def _bwd_sim(c, kind, s_mode, fwd, ops=None, S=None, **kw):
    o, _, ofb, _ = _sdf(c["state"])
    S = S or [fwd["%s%d" % ("H" if s_mode else "S", l)] for l in range(8)]
    V = [fwd["V%d" % l] for l in range(8)]
    return mlp_ops.simulate_sdf_backward(ops or o, ofb, *_bwd_args(c, kind), S, V, rnd=mlp_ops.f32_rne, dtype=F32,
                                         **dict(dict(ex_factor=100.0, s_mode=s_mode, chain=True), **kw))


def _d_pts_sim(c, kind, fwd, ab, before=None):
    """The stand-in of fbar's ray adjoint: the float32 side of the model on the stand-in's own blocks."""
    _, _, ofb, _ = _sdf(c["state"])
    pts, scale, _, _, g_n = _bwd_args(c, kind)
    return mlp_ops.sdf_d_pts_model(ofb, pts, scale, g_n, fwd["U_pe"], ab[0], ab[4], f32=True, before=before)["y32"]


@pytest.mark.parametrize("s_mode", [0, 1])
@pytest.mark.parametrize("name,kind", [(n, "random") for n in SDF_NAMES] + [("uniform-P129-s1", "g_feat=0"), ("uniform-P129-s1", "g_normals=0")])
def test_sdf_backward_comparator_accepts_the_float32_stand_in(name, kind, s_mode):
    """rbar + fbar on the stand-in forward's planes with s_from_h = 0 and 1, acc_pts = 0 and 1: accepted; the floors printed."""
    c, fwd = _sim_cached(name)
    ub, EX, ab = _bwd_sim(c, kind, s_mode, fwd)
    res = _bwd_judged(c, kind, s_mode, fwd, ub, EX, ab, _d_pts_sim(c, kind, fwd, ab))
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    before = mlp_cases.sdf_d_pts_prefill(c)[sel]
    res["d_pts+acc"] = _bwd_judged(c, kind, s_mode, fwd, ub, EX, ab, _d_pts_sim(c, kind, fwd, ab, before), before)["d_pts"]
    for k, j in res.items():
        print("%-22s %-12s s_from_h=%d %-9s floor %.3f units  bound %.2f" % (name, kind, s_mode, k, j["floor"], j["bound"]))
        assert j["ok"], (name, kind, s_mode, k, j)


@pytest.mark.parametrize("s_mode", [0, 1])
def test_sdf_backward_comparator_rejects_planted_defects(s_mode):
    """ex_l without the 100; softplus' of layer 5 formed the other form's way (exp(-100 S) from an S plane, or the H plane taken for
    softplus' itself); a dropped k column of W_2; acc_pts overwriting instead of adding - each at the block it is in."""
    c, fwd = _sim_cached("uniform-P33-s1.5")
    kind = "random"
    only = lambda res, where: all(j["ok"] == (k not in where) for k, j in res.items())
    res = _bwd_judged(c, kind, s_mode, fwd, *_bwd_sim(c, kind, s_mode, fwd, ex_factor=1.0))
    assert only(res, ["EX%d" % l for l in range(8)]), {k: j["ok"] for k, j in res.items()}
    # the planes of the OTHER form handed to layer 5
    other = [fwd["%s%d" % ("S" if s_mode else "H", l)] if l == 5 else fwd["%s%d" % ("H" if s_mode else "S", l)] for l in range(8)]
    res = _bwd_judged(c, kind, s_mode, fwd, *_bwd_sim(c, kind, s_mode, fwd, S=other))
    assert only(res, ["ub6", "EX5", "ab5"]), {k: j["ok"] for k, j in res.items()}
    wrong = _copy(_sdf(c["state"])[0])
    wrong[2]["W"][:, 5] = 0.0
    res = _bwd_judged(c, kind, s_mode, fwd, *_bwd_sim(c, kind, s_mode, fwd, ops=wrong))
    assert only(res, ["ub3", "EX2"]), {k: j["ok"] for k, j in res.items()}
    ub, EX, ab = _bwd_sim(c, kind, s_mode, fwd)
    before = mlp_cases.sdf_d_pts_prefill(c)
    j = _bwd_judged(c, kind, s_mode, fwd, ub, EX, ab, _d_pts_sim(c, kind, fwd, ab), before)["d_pts"]
    assert not j["ok"] and j["err"] > 1e3


# ---- the heads and the background network -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _head_ops(net, state, stream):
    from vdn_hip import images
    d_out = 3 if net == "color_network" else 96
    d_feature = 352 if state == "heads352" and net == "color_network" else 256
    st = images.rendering_streams(d_feature=d_feature, mode="idr", d_in=9, d_out=d_out, d_hidden=256, n_layers=4, multires_view=4)
    img = mlp_ops.HostImages.of_sdf_state(mlp_cases.head_states(state)[mlp_cases.STATE_KEY[net]], st, np.float32, n_layers=5)
    return [mlp_ops.operand_weights(img, stream, l, fmt=0) for l in range(5)]


def _head_sim(c, ops=None):
    return mlp_ops.simulate_head_forward(ops or _head_ops(c["net"], c["state"], "fwd"), c["pts"], c["dirs"], c["normals"],
                                         c["feat"].astype(np.float64), c["squeeze"], c["d_out"], mlp_ops.f32_rne, extra=c["extra"], chain=True)


def _head_judged(c, planes):
    models = mlp_ops.head_plane_models(_head_ops(c["net"], c["state"], "fwd"), c["pts"], c["dirs"], c["normals"], c["feat"].astype(np.float64),
                                       planes, c["squeeze"], c["d_out"], extra=c["extra"], f32=True)
    return mlp_ops.judge_planes(models, planes), models


@pytest.mark.parametrize("name", list(mlp_cases.HEAD_CASES))
def test_head_comparators_accept_the_float32_stand_in_and_reject_planted_defects(name):
    """vdn_rendernet_fwd_f32 / _bwd_f32: the stand-in passes (floors printed). Rejected: the hardware-trig error in save_small; a
    plane rounded to bf16; a dropped k column; ReLU' at exactly 0 taken as 1 (the silenced unit of layer 2); acc_* overwriting."""
    c = mlp_cases.head_case(name)
    planes = _head_sim(c)
    res, models = _head_judged(c, planes)
    for k, j in res.items():
        print("%-14s %-9s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
        assert j["ok"], (name, k, j)
    u = mlp_cases.SILENT_UNIT
    for k in ("h0", "h2"):
        assert (models[k]["y64"][:, u] == 0).all() and (models[k]["unit"][:, u] == 0).all() and (planes[k][:, u] == 0).all()
    # the copied columns admit nothing but the input itself
    assert not models["small"]["unit"][:, :6].any() and not models["small"]["unit"][:, 30:].any()
    bad = dict(planes, small=planes["small"].copy())
    bad["small"][:, 6:30] += mlp_ops.TRIG_ABS
    assert not _head_judged(c, bad)[0]["small"]["ok"]
    assert not _head_judged(c, dict(planes, h1=mlp_ops.bf16_rne(planes["h1"])))[0]["h1"]["ok"]
    wrong = _copy(_head_ops(c["net"], c["state"], "fwd"))
    wrong[1]["W"][:, 5] = 0.0
    res, _ = _head_judged(c, _head_sim(c, ops=wrong))
    assert all(j["ok"] == (k != "h1") for k, j in res.items()), {k: j["ok"] for k, j in res.items()}
    if c["extra"] is not None:
        return
    # backward
    ob = _head_ops(c["net"], c["state"], "bwd")
    g_out, hs = mlp_cases.head_upstream(c), [planes["h%d" % l] for l in range(4)]
    judged = lambda p: mlp_ops.judge_planes(mlp_ops.head_bwd_plane_models(ob, g_out, planes["out"], hs, p, c["squeeze"], c["d_out"], f32=True), p)
    bwd = mlp_ops.simulate_head_backward(ob, g_out, planes["out"], hs, c["squeeze"], mlp_ops.f32_rne, chain=True)
    res = judged(bwd)
    for k, j in res.items():
        print("%-14s %-9s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
        assert j["ok"], (name, k, j)
    relu1 = [h.copy() for h in hs]
    relu1[2][:, u] = 1.0                                 # (ReLU' = 1 where the saved activation is exactly 0)
    res = judged(mlp_ops.simulate_head_backward(ob, g_out, planes["out"], relu1, c["squeeze"], mlp_ops.f32_rne, chain=True))
    assert not res["delta_h2"]["ok"] and all(j["ok"] for k, j in res.items() if k != "delta_h2"), {k: j["ok"] for k, j in res.items()}
    m = mlp_ops.head_bwd_plane_models(ob, g_out, planes["out"], hs, bwd, c["squeeze"], c["d_out"], f32=True)["d_normals"]
    pre = np.random.RandomState(5).standard_normal(m["y64"].shape).astype(np.float32)
    acc = dict(m, y64=m["y64"] + pre, y32=mlp_ops.f32_rne(m["y32"] + pre), unit=m["unit"] + mlp_ops.U24 * np.abs(m["y64"] + pre))
    assert mlp_ops.judge(mlp_ops.f32_rne(bwd["d_normals"] + pre), **acc)["ok"] and not mlp_ops.judge(bwd["d_normals"], **acc)["ok"]


@functools.lru_cache(maxsize=None)
def _nerf_ops(state, stream):
    from vdn_hip import images
    st = images.nerf_streams(D=8, W=256, d_in=4, d_in_view=3, multires=10, multires_view=4, skips=(4,), rgb_dims=3,
                             gen_depth_feats=state != "nodpt", dpt_dim=96)
    img = mlp_ops.HostImages.of_linear_state(mlp_cases.head_states(state)["nerf"], st, np.float32)
    return [mlp_ops.operand_weights(img, stream, l, fmt=0) for l in range(11)]


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_comparators_accept_the_float32_stand_in_and_reject_planted_defects(name):
    """vdn_nerf_mlp_fwd_f32 / _bwd_f32 / _bwd_input_f32: the stand-in passes (floors printed). Rejected: a dropped k column, a bias
    left out, a plane rounded to bf16, the other weight state (the wiring), work-list saves at the dense row."""
    c = mlp_cases.nerf_case(name)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    ops, ob = _nerf_ops(c["state"], "fwd"), _nerf_ops(c["state"], "bwd")
    judged = lambda p: mlp_ops.judge_planes(mlp_ops.nerf_plane_models(ops, pts4, dirs, p, f32=True), p)
    planes = mlp_ops.simulate_nerf_forward(ops, pts4, dirs, mlp_ops.f32_rne, chain=True)
    for k, j in judged(planes).items():
        print("%-24s %-9s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
        assert j["ok"], (name, k, j)
    assert (planes["h2"][:, mlp_cases.SILENT_UNIT] == 0).all()
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    g = [None if a is None else a[sel] for a in mlp_cases.nerf_upstream(c)]
    hs, hv = [planes["h%d" % l] for l in range(8)], planes["hv"]
    bwd = mlp_ops.simulate_nerf_backward(ob, *g, hs, hv, mlp_ops.f32_rne, chain=True)
    models = mlp_ops.nerf_bwd_plane_models(ob, *g, hs, hv, bwd, f32=True)
    adj = mlp_ops.nerf_input_adjoint_models(ob, pts4, dirs, bwd, f32=True)
    models.update(adj)
    bwd.update({k: m["y32"] for k, m in adj.items()})
    for k, j in mlp_ops.judge_planes(models, bwd).items():
        print("%-24s %-9s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
        assert j["ok"], (name, k, j)
    if name != "nerf-P33" and c["active_idx"] is None:
        return
    if c["active_idx"] is not None:                      # saves at the dense row
        dense = mlp_ops.simulate_nerf_forward(ops, c["pts4"][:c["n_active"]], c["dirs"][:c["n_active"]], mlp_ops.f32_rne, chain=True)
        res = judged(dense)
        assert not res["pe"]["ok"] and not res["vpe"]["ok"] and res["pe"]["err"] > 1e3
        return
    wrong = _copy(ops)
    wrong[3]["W"][:, 5] = 0.0
    res = judged(mlp_ops.simulate_nerf_forward(wrong, pts4, dirs, mlp_ops.f32_rne, chain=True))
    assert all(j["ok"] == (k != "h3") for k, j in res.items()), {k: j["ok"] for k, j in res.items()}
    wrong = _copy(ops)
    wrong[6]["b"][:] = 0.0
    res = judged(mlp_ops.simulate_nerf_forward(wrong, pts4, dirs, mlp_ops.f32_rne, chain=True))
    assert all(j["ok"] == (k != "h6") for k, j in res.items()), {k: j["ok"] for k, j in res.items()}
    assert not judged(dict(planes, feature=mlp_ops.bf16_rne(planes["feature"])))["feature"]["ok"]
    res = judged(mlp_ops.simulate_nerf_forward(_nerf_ops("heads-other", "fwd"), pts4, dirs, mlp_ops.f32_rne, chain=True))
    assert res["pe"]["ok"] and res["vpe"]["ok"] and all(not j["ok"] and j["err"] > 1e3 for k, j in res.items() if k not in ("pe", "vpe"))


def test_the_other_head_weight_state_is_rejected():
    c = mlp_cases.head_case("color-P33")
    res, _ = _head_judged(c, _head_sim(c, ops=_head_ops("color_network", "heads-other", "fwd")))
    assert res["small"]["ok"] and all(not j["ok"] and j["err"] > 1e3 for k, j in res.items() if k != "small")
