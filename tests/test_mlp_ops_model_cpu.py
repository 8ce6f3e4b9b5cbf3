"""The one-layer models of the bf16 forward and backward launches (oracle/mlp_ops.py: SDF network, heads, background network)
and their cases (oracle/mlp_cases.py), proven without a GPU: the chains of one-layer
models on unrounded weight images, fed their own unrounded outputs in float64, ARE the networks of oracle/neus_oracle.py
(sdf_forward with its gradient, rendering_forward, nerf_forward) and their torch autograd gradients, to 1e-10; the "init" state sits on the knee of softplus in every layer and the "hot" state reaches
every range switch; the comparator accepts a float32 evaluation rounded to bf16 either way and rejects it with each planted
structural error, in every case, at the plane the error is in and at no other; a pre-activation that is exactly zero admits
nothing but an exact zero; the chunk decoder inverts the documented layout. The float32 floors of every (case, plane) are printed
(pytest -rA). For the launches that save no planes (tests/test_gpu_sdf_value_launches.py, held bit for bit): the cases reach what
they claim, the "sdf" stream holds the first nine layers of "full", every planted ray / column / stride / weight / scale defect
moves the sdf of every row, and the ray-form models (pts_err) accept either way of forming the point and reject those defects."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import mlp_cases, mlp_ops, neus_oracle as orc

NAMES = list(mlp_cases.SDF_CASES)


def _streams():
    from vdn_hip import images
    return images.sdf_streams(3, 257, 256, 8, (4,), 6, scaled=True)


@functools.lru_cache(maxsize=None)
def _ops(state="init"):
    sd = mlp_cases.states(state)["sdf_network_fine"]
    return mlp_ops.sdf_ops(mlp_ops.HostImages.of_sdf_state(sd, _streams()))


@functools.lru_cache(maxsize=None)
def _sweep_ops(state="init"):
    sd = mlp_cases.states(state)["sdf_network_fine"]
    return mlp_ops.sdf_sweep_ops(mlp_ops.HostImages.of_sdf_state(sd, _streams()))


def _copy(ops):
    return [dict(o, W=o["W"].copy(), b=o["b"].copy()) for o in ops]


# ---- bf16 as a set of values ------------------------------------------------------------------------------------------------

def test_bf16_helpers_against_torch():
    rs = np.random.RandomState(0)
    x = (rs.standard_normal(20000) * 10.0 ** rs.uniform(-30, 30, 20000)).astype(np.float32)
    x[:5] = [0.0, 1.0, -1.0, 1.00390625, 255.5]                      # (two ties)
    want = torch.tensor(x).to(torch.bfloat16).double().numpy()
    assert np.array_equal(mlp_ops.bf16_rne(x), want)
    v = x.astype(np.float64) * (1.0 + 1e-9)
    dn, up = mlp_ops.bf16_down(v), mlp_ops.bf16_up(v)
    assert (dn <= v).all() and (up >= v).all()
    for a in (dn, up):                                                # bf16 values: unchanged by a further rounding
        assert np.array_equal(mlp_ops.bf16_rne(a), a)
    q = up - dn
    assert ((q == 0) | (np.abs(q) <= 2.0 ** -7 * np.abs(v) * 1.0000001)).all()       # neighbours
    t = mlp_ops.bf16_trunc(x)
    assert np.array_equal(t, np.where(x >= 0, mlp_ops.bf16_down(x), mlp_ops.bf16_up(x)))


def test_chunk_decoder_inverts_the_documented_layout():
    """A chunk written element by element by the layout's formula (include/vdn_render.h, csrc/prep.hip's comment)."""
    from vdn_hip import layout
    kt = 3
    rs = np.random.RandomState(1)
    W = torch.tensor(rs.standard_normal((32, 32 * kt)).astype(np.float32)).to(torch.bfloat16)
    bias = torch.tensor(rs.standard_normal(32).astype(np.float32))
    words = torch.zeros(2 * kt * 64 * 8, dtype=torch.bfloat16)
    for s in range(2 * kt):
        for lane in range(64):
            i, h = lane & 31, lane >> 5
            for j in range(8):
                words[(s * 64 + lane) * 8 + j] = W[i, 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)]
    chunk = torch.cat([words.view(torch.uint8), bias.view(torch.uint8), torch.zeros(896, dtype=torch.uint8)])
    Wd, bd = layout.decode_chunk_bf16(chunk, kt)
    assert torch.equal(Wd, W.float()) and torch.equal(bd, bias)


# ---- the chain of one-layer models is the network -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uniform-P33-s1.5", "lattice-P33-s1"])
def test_chain_of_one_layer_models_equals_the_oracle(name):
    c = mlp_cases.sdf_case(name)
    sd = mlp_cases.states()["sdf_network_fine"]
    ops = mlp_ops.sdf_ops(mlp_ops.HostImages.of_sdf_state(sd, _streams(), np.float64), rounded=False)
    x = mlp_ops.posenc_scaled(c["pts"], c["scale"])["y"]
    g = None
    for l in range(8):
        g = mlp_ops.sdf_hidden(l, g, (x, x) if l in (0, 4) else None, ops[l]["W"], ops[l]["b"])["y"]
    last = mlp_ops.sdf_last(g, ops[8]["W"], ops[8]["b"], ops[8]["tail"], c["scale"])
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in sd.items()}
    ref = orc.sdf_forward(p, torch.tensor(c["pts"].astype(np.float64)), orc.SDFConf(scale=c["scale"])).numpy()
    for got, want in ((last["sdf"], ref[:, 0]), (last["feat"], ref[:, 1:])):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("name", ["uniform-P33-s1.5", "lattice-P33-s1"])
def test_chain_of_sweep_models_equals_the_oracle_gradient(name):
    """sdf_sweep, sweep_u and pe_jacobian_T on the unrounded images of W_l^T, fed the unrounded forward chain and their own
    outputs in float64, against the reverse sweep of sdf_forward(with_gradient=True): d sdf / d x."""
    c = mlp_cases.sdf_case(name)
    sd = mlp_cases.states()["sdf_network_fine"]
    img = mlp_ops.HostImages.of_sdf_state(sd, _streams(), np.float64)
    ops, ows = mlp_ops.sdf_ops(img, rounded=False), mlp_ops.sdf_sweep_ops(img, rounded=False)
    x = mlp_ops.posenc_scaled(c["pts"], c["scale"])["y"]
    g, gs = None, []
    for l in range(8):
        g = mlp_ops.sdf_hidden(l, g, (x, x) if l in (0, 4) else None, ops[l]["W"], ops[l]["b"])["y"]
        gs.append(g)
    u = np.repeat(ops[8]["tail"][None, :] / c["scale"], c["P"], 0)
    pe4 = None
    for l in range(7, -1, -1):
        V = mlp_ops.sdf_sweep(l, u, gs[l], aten_threshold=True)["y"]       # (the oracle is torch's softplus: threshold 20)
        if l == 3:
            V = np.concatenate([V, np.zeros((c["P"], 224 - V.shape[1]))], -1)
        u = mlp_ops.sweep_u(l, V, ows[l]["W"])["u"]
        if l == 4:
            pe4, u = u[:, 224:224 + 39], u[:, :217]
    got = mlp_ops.pe_jacobian_T(c["pts"], c["scale"], u[:, :39] + pe4)["y"]
    p = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in sd.items()}
    _, ref = orc.sdf_forward(p, torch.tensor(c["pts"].astype(np.float64)), orc.SDFConf(scale=c["scale"]), with_gradient=True)
    assert np.abs(got - ref.numpy()).max() <= 1e-10 * np.abs(ref.numpy()).max()


# ---- coverage -----------------------------------------------------------------------------------------------------------------

def _chain_t(state, name):
    """Pre-activations t_l of the exact network (float64, nothing rounded) at a case's points, layer by layer."""
    c = mlp_cases.sdf_case(name)
    sd = mlp_cases.states(state)["sdf_network_fine"]
    ops = mlp_ops.sdf_ops(mlp_ops.HostImages.of_sdf_state(sd, _streams(), np.float64), rounded=False)
    x = mlp_ops.posenc_scaled(c["pts"], c["scale"])["y"]
    g, out = None, []
    for l in range(8):
        m = mlp_ops.sdf_hidden(l, g, (x, x) if l in (0, 4) else None, ops[l]["W"], ops[l]["b"])
        g = m["y"]
        n = 217 if l == 3 else 256
        out.append((m["t"][:, :n], m["sigma"][:, :n], m["y"][:, :n]))
    return out


def test_init_state_sits_on_the_knee_of_softplus_in_every_layer():
    """At the 300-point case at least 20 % of every hidden layer's units have 0.02 < sigma < 0.98: the logarithm, not its
    asymptotes, forms the value (and the sweep's 8-bit code is neither 0 nor 255)."""
    for l, (t, s, y) in enumerate(_chain_t("init", "uniform-P300-s1.5")):
        knee = float(((s > 0.02) & (s < 0.98)).mean())
        print("init layer %d: %.1f %% of the units on the knee" % (l, 100 * knee))
        assert knee >= 0.20


def test_hot_state_reaches_the_range_switches_in_every_layer():
    """From the float64 model alone: in every hidden layer at least 1 % of the units in each of t >= 128 (w = +inf), t <= -128,
    25 <= t < 128 (g = t) and |t| < 5 (the knee), and max |H| < 2^10."""
    for l, (t, s, y) in enumerate(_chain_t("hot", "hot-P300-s1.5")):
        share = [float((t >= 128).mean()), float((t <= -128).mean()), float(((t >= 25) & (t < 128)).mean()), float((np.abs(t) < 5).mean())]
        print("hot layer %d: t >= 128 %.1f %%, t <= -128 %.1f %%, 25 <= t < 128 %.1f %%, |t| < 5 %.1f %%; max H %.0f"
              % ((l,) + tuple(100 * v for v in share) + (np.abs(y).max(),)))
        assert min(share) >= 0.01 and np.abs(y).max() < 2.0 ** 10


def test_cases_reach_every_row_path():
    Ps = sorted(mlp_cases.SDF_CASES[n][0] for n in NAMES if mlp_cases.SDF_CASES[n][3] is None and mlp_cases.SDF_CASES[n][4] == "init")
    assert {1, 33, 129, 300} <= set(Ps) and {mlp_cases.SDF_CASES[n][1] for n in NAMES} == {1.0, 1.5}
    c = mlp_cases.sdf_case("worklist-P200-n77-s1")
    idx = c["active_idx"][:77]
    assert len(set(idx.tolist())) == 77 and (np.diff(idx) < 0).any() and (np.diff(idx) != 1).any() and (c["active_idx"][77:] == -1).all()
    lat = mlp_cases.sdf_case("lattice-P33-s1")["pts"]
    assert set(np.unique(lat).tolist()) == {-1.0, 0.0, 1.0} and (lat[0] == 0).all()


# ---- the comparator: accepts a rounding of the float32 evaluation, rejects each planted error ----------------------------------

def _judged(c, planes):
    pts = mlp_cases.rows_of(c)
    return mlp_ops.judge_planes(mlp_ops.sdf_plane_models(_ops(c["state"]), pts, c["scale"], planes, _sweep_ops(c["state"])), planes)


def _sim(c, ops=None, rnd=mlp_ops.bf16_rne, ops_sweep=None, **kw):
    return mlp_ops.simulate_sdf_forward(ops or _ops(c["state"]), mlp_cases.rows_of(c), c["scale"], rnd,
                                        ops_sweep or _sweep_ops(c["state"]), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_comparator_accepts_both_roundings_and_prints_the_floors(name):
    c = mlp_cases.sdf_case(name)
    pts = mlp_cases.rows_of(c)
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        res = _judged(c, _sim(c, rnd=rnd))
        for k, j in res.items():
            if k == "sdf" and rnd is mlp_ops.bf16_trunc:      # (its 2^-9 term presumes H[7] is the NEAREST bf16 of the activations)
                continue
            assert j["ok"], (name, rnd.__name__, k, j)
            assert j["err"] <= j["bound"]
    for k, j in res.items():
        print("%-22s %-5s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))


def _plant_bias_tile(ops):
    """Layer 2: the bias block of the 32-column tile 1 swapped with tile 2's."""
    b = ops[2]["b"]
    b[32:64], b[64:96] = b[64:96].copy(), b[32:64].copy()
    return "H2"


def _plant_skip_scale(ops):
    """Layer 4: 1 / sqrt 2 left off the encoded input's columns."""
    ops[4]["W"][:, 224:] = mlp_ops.bf16_rne(ops[4]["W"][:, 224:] * math.sqrt(2.0))
    return "H4"


def _plant_residue_columns(ops, l=0):
    """The residue slots' weights taken from padded columns 25..49 (layer 4: 224 + 25 ..) of the image."""
    k0 = 0 if l == 0 else 224
    ops[l]["W"][:, k0 + 39:k0 + 64] = ops[l]["W"][:, k0 + 25:k0 + 50].copy()
    return "H%d" % l


def _plant_network_units(ops):
    """Layer 5's bias in network units (without 100 log2 e)."""
    ops[5]["b"] = ops[5]["b"] / mlp_ops.C
    return "H5"


def _plant_feature_row(ops):
    """The feature rows of the last layer shifted by one (row j of the image = row j of W_8 instead of j + 1)."""
    W = ops[8]["W"]
    W[1:256] = W[0:255].copy()
    return "feat"


PLANTS = {"bias-tile": _plant_bias_tile, "skip-scale": _plant_skip_scale, "residue-l0": _plant_residue_columns,
          "residue-l4": lambda o: _plant_residue_columns(o, 4), "network-units": _plant_network_units, "feature-row": _plant_feature_row}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plant", list(PLANTS))
def test_comparator_rejects_each_planted_error(name, plant):
    """The stand-in launch evaluated with the planted error, judged against the models of the true weights: rejected at the
    plane the error is in, and - teacher forcing - at no other plane."""
    c = mlp_cases.sdf_case(name)
    wrong = _copy(_ops(c["state"]))
    where = PLANTS[plant](wrong)
    res = _judged(c, _sim(c, ops=wrong))
    assert not res[where]["ok"], (name, plant, res[where])
    for k, j in res.items():
        if k != where:
            assert j["ok"], (name, plant, k, j)


def _sweep_tile(ow):
    """The image of W_6^T with its 32-row tiles 2 and 3 swapped: u_6, seen in V[5]."""
    W = ow[6]["W"]
    W[64:96], W[96:128] = W[96:128].copy(), W[64:96].copy()
    return "V5"


def _sweep_skip_scale(ow):
    """1 / sqrt 2 left off the encoded input's rows of W_4^T: seen in U_pe alone."""
    ow[4]["W"][224:] = mlp_ops.bf16_rne(ow[4]["W"][224:] * math.sqrt(2.0))
    return "U_pe"


def _sweep_k_shift(ow):
    """W_2^T contracted against v_2 shifted by one feature."""
    ow[2]["W"] = np.roll(ow[2]["W"], 1, axis=1)
    return "V1"


SWEEP_PLANTS = {"sweep-tile": _sweep_tile, "sweep-skip-scale": _sweep_skip_scale, "sweep-k-shift": _sweep_k_shift}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("plant", list(SWEEP_PLANTS) + ["sigma-network-units", "sigma-neighbour"])
def test_comparator_rejects_each_planted_sweep_error(name, plant):
    """As above for the reverse sweep: a wrong image, and softplus' formed from H in the network's units instead of the scaled
    ones (layer 5), or taken from the neighbouring feature (layer 2)."""
    c = mlp_cases.sdf_case(name)
    if plant in SWEEP_PLANTS:
        wrong = _copy(_sweep_ops(c["state"]))
        where = SWEEP_PLANTS[plant](wrong)
        planes = _sim(c, ops_sweep=wrong)
    elif plant == "sigma-network-units":
        where = "V5"
        planes = _sim(c, sigma_of=lambda l, g: 1.0 - torch.exp2(-(g / mlp_ops.C if l == 5 else g)))
    else:
        where = "V2"
        planes = _sim(c, sigma_of=lambda l, g: 1.0 - torch.exp2(-(torch.roll(g, 1, 1) if l == 2 else g)))
    res = _judged(c, planes)
    assert not res[where]["ok"], (name, plant, res[where])
    for k, j in res.items():
        if k != where:
            assert j["ok"], (name, plant, k, j)


@pytest.mark.parametrize("name", NAMES)
def test_comparator_rejects_two_bf16_ulps(name):
    """One element of one plane moved by 2 bf16 ulps (the largest element of H[6]; the first feature; a PE cosine)."""
    c = mlp_cases.sdf_case(name)
    base = _sim(c)
    for k, pick in (("H6", None), ("feat", (0, 0)), ("PE", (0, 6))):
        planes = {n: v.copy() for n, v in base.items()}
        i = np.unravel_index(np.argmax(np.abs(planes[k])), planes[k].shape) if pick is None else pick
        v = planes[k][i]
        planes[k][i] = mlp_ops.bf16_up(np.nextafter(mlp_ops.bf16_up(np.nextafter(v, np.inf)), np.inf))
        models = mlp_ops.sdf_plane_models(_ops(c["state"]), mlp_cases.rows_of(c), c["scale"], base, _sweep_ops(c["state"]))   # (of the unmoved planes)
        j = mlp_ops.judge_planes({k: models[k]}, planes)[k]
        assert not j["ok"] and j["n_bad"] == 1 and j["worst"] == tuple(int(a) for a in i), (name, k, j)


def test_the_other_weight_state_is_rejected():
    """What the GPU test's wiring check relies on: the launch of the other state's weights does not pass this state's models."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    planes = _sim(c, ops=_ops("other"), ops_sweep=_sweep_ops("other"))
    res = _judged(c, planes)
    for k, j in res.items():
        print(k, j["ok"], "%.3g" % j["err"])
    # (the encoding and the Jacobian of the encoding have no weights; the sdf row of W_8, which also makes V[7], is the geometric
    # init's constant sqrt(pi) / 16 in both states)
    free = ("PE", "normals", "sdf", "V7")
    assert res["PE"]["ok"] and res["normals"]["ok"] and all(not res[k]["ok"] for k in res if k not in free)


# ---- the launches that save no planes (tests/test_gpu_sdf_value_launches.py): cases, premise, the ray form's anchor --------------------
# Those launches are held to the training launch bit for bit, so the comparator is torch.equal; what has to be proven here is that
# the cases reach what they claim, that the two streams hold the same network, that a wrong ray, column or stride moves the sdf of
# EVERY row by more than the last-layer model's whole allowance (so by far more than a bit), and that the models with which the GPU
# test holds the ray-form TRAINING launch - the anchor of the ray cases - accept either way of forming the point and reject each
# planted defect at the PE plane.

RAY_NAMES = list(mlp_cases.SDF_VALUE_RAY_CASES)


def test_sdf_value_cases_reach_what_they_claim():
    assert set(mlp_cases.SDF_VALUE_CASES) == set(mlp_cases.SDF_CASES) | set(RAY_NAMES) | set(mlp_cases.SDF_VALUE_LARGE_CASES)
    for n in mlp_cases.SDF_CASES:                            # the pts form: SDF_CASES as they are
        a, b = mlp_cases.sdf_case(n), mlp_cases.sdf_value_case(n)
        assert b["form"] == "pts" and all(np.array_equal(a[k], b[k]) for k in a)
    cs = {n: mlp_cases.sdf_value_case(n) for n in RAY_NAMES}
    assert [(c["B"], c["n_per_ray"]) for c in cs.values()] == [(1, 1), (3, 11), (5, 16), (2, 64), (3, 43), (8, 25)]
    assert cs["value-rays-3x43-s1.5"]["scale"] == 1.5 and cs["value-rays-3x43-s1.5"]["P"] == 129
    assert cs["value-rays-5x16-s1"]["P"] == 2 * 32 + 16      # the split kernel's two rays per workgroup, 2 1/2 workgroups
    for n, c in cs.items():
        B, k = c["B"], c["n_per_ray"]
        assert c["form"] == "rays" and "pts" not in c and c["state"] == "init"
        assert c["z_ld"] > k and c["sdf_ld"] > k and c["sdf_ld"] != c["z_ld"], n
        assert 0 < c["z_col0"] <= c["z_ld"] - k and 0 < c["sdf_col0"] <= c["sdf_ld"] - k, n
        assert c["z_wide"].shape == (B, c["z_ld"]) and c["z_wide"].dtype == np.float32
        assert np.array_equal(c["z_wide"][:, c["z_col0"]:c["z_col0"] + k], c["z"])
        gap = np.ones(c["z_ld"], bool)
        gap[c["z_col0"]:c["z_col0"] + k] = False
        assert gap.sum() == c["z_ld"] - k > 0                # non-empty, and no depth of the slice is a depth of the gap
        assert c["z_wide"][:, gap].min() >= mlp_cases.Z_GAP_FILL[0] > 1.0 >= c["z"].max()
        assert (c["rays_o"][0] == 0).all() and (c["rays_d"][0] == (1.0, 0.0, 0.0)).all(), n
        if B > 1:
            assert np.abs(np.diff(c["rays_d"], axis=0)).min() >= mlp_cases.DIR_GAP > 4 * 2.0 ** -7, n
        if c["P"] >= 3:
            assert (c["z"] == 0).sum() == 1 and (c["z"] < 0).sum() == 1, n
    assert all(32 % cs[n]["n_per_ray"] for n in ("value-rays-3x11-s1", "value-rays-3x43-s1.5", "value-rays-worklist-8x25-n77-s1"))   # ray boundaries inside a wave
    w = cs["value-rays-worklist-8x25-n77-s1"]
    idx = w["active_idx"][:77]
    assert w["P"] == 200 and len(set(idx.tolist())) == 77 and (np.diff(idx) < 0).any() and (w["active_idx"][77:] == -1).all()
    tile = mlp_cases.sdf_case(mlp_cases.SDF_VALUE_TILE)
    for n, (P, n_active) in mlp_cases.SDF_VALUE_LARGE_CASES.items():
        c = mlp_cases.sdf_value_case(n)
        assert c["P"] == P > 8192 and c["tile"] == tile["P"] == 300 and c["scale"] == tile["scale"] and c["state"] == tile["state"]
        assert np.array_equal(c["pts"], tile["pts"][np.arange(P) % 300])
        if n_active is None:
            assert P == 64 * 128 + 1
        else:
            idx = c["active_idx"][:n_active]
            assert len(set(idx.tolist())) == n_active == 77 and (np.diff(idx) < 0).any() and (c["active_idx"][n_active:] == -1).all()
            assert idx.max() >= 128 and len(set((idx % 300).tolist())) > 60       # beyond the first workgroup's points; many tile rows
    # cold_start = 1 reads ahead only from 128 workgroups on: 129 of the split kernel's (P <= 8192), 129 of the 128-point kernels'
    cold = {n: mlp_cases.sdf_value_case(n) for n in list(mlp_cases.SDF_COLD_TILED_CASES) + list(mlp_cases.SDF_COLD_RAY_CASES)}
    assert sorted((c["P"] + 31) // 32 for c in cold.values() if c["P"] <= 8192) == [129, 130]
    assert sorted((c["P"] + 127) // 128 for c in cold.values() if c["P"] > 8192) == [129, 129]
    assert {c["form"] for c in cold.values() if c["P"] <= 8192} == {c["form"] for c in cold.values() if c["P"] > 8192} == {"pts", "rays"}
    assert all(c["active_idx"] is None and c["tile"] == (300 if c["form"] == "pts" else None) for c in cold.values())
    for r0, rmax, n in mlp_cases.SDF_TAIL_SPLITS:            # the hand-off's every branch, at both workgroup boundaries
        assert r0 % 128 == 0 and n <= 300 < mlp_cases.SDF_TAIL_LIST_P
    assert [mlp_cases.handed_off(*s) for s in mlp_cases.SDF_TAIL_SPLITS] == [False, True, True, True, False]
    assert {s[0] for s in mlp_cases.SDF_TAIL_SPLITS if mlp_cases.handed_off(*s)} == {128, 256}
    t = mlp_cases.sdf_tail_case("list", 300)
    idx = t["active_idx"][:300]
    assert len(set(idx.tolist())) == 300 and (np.diff(idx) < 0).any() and (t["active_idx"][300:] == -1).all()
    assert np.array_equal(mlp_cases.sdf_tail_case("list", 129)["active_idx"][:129], idx[:129])
    assert np.array_equal(mlp_cases.sdf_tail_case("dense", 129)["pts"], tile["pts"][:129])


@pytest.mark.parametrize("state", ["init", "hot", "other"])
def test_the_sdf_stream_holds_the_first_nine_layers_of_the_full_stream(state):
    """The premise of mode 0 = mode 1 bit for bit, on the host: layers 0..7 of "sdf" are those of "full" (operand, bias, tail,
    k-tiles, chunk count); layer 8 of "sdf" is one chunk whose row 0 is the sdf row - row 256 of "full"'s layer 8 - with the same
    bias and tail, every other row zero."""
    host = mlp_ops.HostImages.of_sdf_state(mlp_cases.states(state)["sdf_network_fine"], _streams())
    assert len(host.streams["sdf"]) == 9 and len(host.streams["full"]) == 17
    for l in range(8):
        a, b = mlp_ops.operand_weights(host, "sdf", l), mlp_ops.operand_weights(host, "full", l)
        assert a["kt"] == b["kt"] and a["n_chunks"] == b["n_chunks"]
        assert all(np.array_equal(a[k], b[k]) for k in ("W", "b", "tail"))
    a, b = mlp_ops.operand_weights(host, "sdf", 8), mlp_ops.operand_weights(host, "full", 8)
    assert (a["n_chunks"], b["n_chunks"], a["kt"], b["kt"]) == (1, 9, 8, 8) and np.array_equal(a["tail"], b["tail"])
    assert np.array_equal(a["W"][0], b["W"][256]) and a["b"][0] == b["b"][256] and not a["W"][1:].any() and not a["b"][1:].any()
    assert a["W"][0].any() and a["b"][0] != 0


SHOWS = 2.0 ** -20              # 16 float32 steps at 1: what a defect has to move a row's sdf by to count as shown (|sdf| < 1.1 here)


def _value_sdf(c, pts, state="init"):
    """The sdf of the network the blob holds (bf16 operand weights) in float64, nothing else rounded, at the given points: a
    function of the point alone - the float32 stand-in's last bits depend on which rows share its matrix product."""
    ops = _ops(state)
    x = mlp_ops.posenc_scaled(pts, c["scale"])["y"]
    g = None
    for l in range(8):
        g = mlp_ops.sdf_hidden(l, g, (x, x) if l in (0, 4) else None, ops[l]["W"], ops[l]["b"])["y"]
    return mlp_ops.sdf_last(g, ops[8]["W"], ops[8]["b"], ops[8]["tail"], c["scale"])["sdf"]


def _ray_pts(c, z, rows, o=None, d=None):
    """o + d z in float32 (two roundings) at the dense point ids `rows`, z [B, n_per_ray]."""
    o, d = c["rays_o"] if o is None else o, c["rays_d"] if d is None else d
    r, s = rows // c["n_per_ray"], rows % c["n_per_ray"]
    return (o[r] + (d[r] * z[r, s][:, None]).astype(np.float32)).astype(np.float32)


def _value_defects(c):
    """{defect: float32 points [rows, 3] a launch with that defect would evaluate}, in the rows of the list."""
    rows = mlp_cases.value_rows_of(c)
    B, n, col0 = c["B"], c["n_per_ray"], c["z_col0"]
    flat = c["z_wide"].reshape(-1)
    out = {"z_ld taken as n_per_ray": _ray_pts(c, flat[col0:col0 + B * n].reshape(B, n), rows),
           "the column offset of z dropped": _ray_pts(c, c["z_wide"][:, :n], rows)}
    if B > 1:
        out["the neighbouring ray's z"] = _ray_pts(c, np.roll(c["z"], -1, axis=0), rows)
        out["the neighbouring ray's origin and direction"] = _ray_pts(c, c["z"], rows, np.roll(c["rays_o"], -1, axis=0), np.roll(c["rays_d"], -1, axis=0))
    if c["P"] > 1:
        out["the neighbouring sample's z"] = _ray_pts(c, np.roll(c["z"].reshape(-1), -1).reshape(B, n), rows)
    return out


@pytest.mark.parametrize("name", RAY_NAMES)
def test_value_ray_cases_show_a_wrong_ray_column_or_stride_in_every_row(name):
    """The GPU test's comparator is bit equality, so a defect shows in a row as soon as that row's sdf moves at all. Here, on the
    float64 network: each defect moves the point of EVERY row it can reach (with B = 1 there is no neighbouring ray; with z_ld
    taken as n_per_ray ray 0 still reads its own depths, every later ray reads others) and its sdf by more than SHOWS; so do the
    "other" weight state and, at scale 1.5, a missing 1 / scale; the share of rows moved beyond the last-layer model's whole
    allowance (sdf_last + last_units: what a comparison through a model would have needed) is printed; and the positions
    r sdf_ld + s of the outputs are not the dense ones."""
    c = mlp_cases.sdf_value_case(name)
    rows = mlp_cases.value_rows_of(c)
    pts = mlp_cases.value_points_of(c)[rows]
    sdf = _value_sdf(c, pts)
    assert np.abs(sdf).max() < 1.1
    planes = mlp_ops.simulate_sdf_forward(_ops(), pts, c["scale"])
    m = mlp_ops.sdf_plane_models(_ops(), pts, c["scale"], planes)["sdf"]
    allowance = 3.0 * m["unit"] + m["extra"]

    def shows(other, sel, what):
        d = np.abs(other - sdf)[sel]
        print("%-34s %-45s moved by >= %.2e, %3.0f %% of the rows beyond the model's allowance" % (name, what, d.min(), 100 * (d > allowance[sel]).mean()))
        assert d.size and (d > SHOWS).all(), (name, what, d.min())

    defects = _value_defects(c)
    assert len(defects) == (2 if c["P"] == 1 else 5)
    for what, bad_pts in defects.items():
        moved = np.abs(bad_pts - pts).max(1) > 0
        sel = np.ones(len(rows), bool)
        if what == "z_ld taken as n_per_ray":                # (ray 0 starts at the same column: it reads its own depths)
            sel = rows // c["n_per_ray"] > 0
            if c["B"] == 1:
                continue
        assert moved[sel].all() and not moved[~sel].any(), (name, what)
        shows(_value_sdf(c, bad_pts), sel, what)
    everywhere = np.ones(len(rows), bool)
    shows(_value_sdf(c, pts, state="other"), everywhere, "the other weight state")
    if c["scale"] != 1.0:
        shows(sdf * c["scale"], everywhere, "1 / scale omitted")
    r, s = rows // c["n_per_ray"], rows % c["n_per_ray"]
    assert (r * c["sdf_ld"] + s + c["sdf_col0"] != rows).all()      # a dense write lands elsewhere in the wide, NaN-filled buffer


def test_one_over_scale_and_the_other_state_show_in_every_row_of_the_point_cases():
    for name in ("uniform-P33-s1.5", "uniform-P300-s1.5", "uniform-P129-s1"):
        c = mlp_cases.sdf_case(name)
        sdf = _value_sdf(c, c["pts"])
        assert (np.abs(_value_sdf(c, c["pts"], state="other") - sdf) > SHOWS).all(), name
        if c["scale"] != 1.0:
            assert (np.abs(sdf * c["scale"] - sdf) > SHOWS).all(), name


@pytest.mark.parametrize("name", RAY_NAMES)
def test_ray_form_models_accept_either_point_and_reject_each_planted_defect(name):
    """The anchor of the ray cases is the ray-form TRAINING launch, which the GPU test holds to sdf_plane_models at the float64
    points o + d z with pts_err = ray_points' bound. Here: the stand-in passes at every plane whether it forms the point with two
    roundings or with one (a fused multiply-add); with each planted defect the PE plane is rejected."""
    c = mlp_cases.sdf_value_case(name)
    rows = mlp_cases.value_rows_of(c)
    p64, err = mlp_ops.ray_points(c["rays_o"], c["rays_d"], c["z"], rows)
    assert err.shape == p64.shape and (err <= 2.0 ** -24 * 4.0).all()
    two, one = _ray_pts(c, c["z"], rows), p64.astype(np.float32)
    assert np.abs(two - p64).max() > 0 or c["P"] == 1
    assert (np.abs(two - p64) <= err).all() and (np.abs(one - p64) <= err).all()
    for pts in (two, one):
        planes = mlp_ops.simulate_sdf_forward(_ops(), pts, c["scale"], ops_sweep=_sweep_ops())
        res = mlp_ops.judge_planes(mlp_ops.sdf_plane_models(_ops(), p64, c["scale"], planes, _sweep_ops(), pts_err=err), planes)
        assert all(j["ok"] for j in res.values()), (name, [k for k, j in res.items() if not j["ok"]])
    for what, bad_pts in _value_defects(c).items():
        if np.array_equal(bad_pts, two):                     # (one ray: its stride does not matter)
            assert c["B"] == 1 and what == "z_ld taken as n_per_ray"
            continue
        planes = mlp_ops.simulate_sdf_forward(_ops(), bad_pts, c["scale"])
        res = mlp_ops.judge_planes(mlp_ops.sdf_plane_models(_ops(), p64, c["scale"], planes, pts_err=err), planes)
        assert not res["PE"]["ok"] and res["PE"]["err"] > 1e3, (name, what, res["PE"])


# ---- the heads' forward -------------------------------------------------------------------------------------------------------

HEAD_NAMES = list(mlp_cases.HEAD_CASES)


@functools.lru_cache(maxsize=None)
def _head_ops(net, state="heads", exact=False):
    from vdn_hip import images
    d_out = 3 if net == "color_network" else 96
    d_feature = 352 if state == "heads352" and net == "color_network" else 256
    st = images.rendering_streams(d_feature=d_feature, mode="idr", d_in=9, d_out=d_out, d_hidden=256, n_layers=4, multires_view=4)
    sd = mlp_cases.head_states(state)[mlp_cases.STATE_KEY[net]]
    img = mlp_ops.HostImages.of_sdf_state(sd, st, np.float64 if exact else np.float32, n_layers=5)
    return [mlp_ops.operand_weights(img, "fwd", l, rounded=not exact) for l in range(5)]


def _head_sim(c, ops=None, rnd=mlp_ops.bf16_rne):
    return mlp_ops.simulate_head_forward(ops or _head_ops(c["net"], c["state"]), c["pts"], c["dirs"], c["normals"],
                                         mlp_ops.bf16_rne(c["feat"]), c["squeeze"], c["d_out"], rnd, extra=c["extra"])


def _head_judged(c, planes):
    models = mlp_ops.head_plane_models(_head_ops(c["net"], c["state"]), c["pts"], c["dirs"], c["normals"], mlp_ops.bf16_rne(c["feat"]),
                                       planes, c["squeeze"], c["d_out"], extra=c["extra"])
    return mlp_ops.judge_planes(models, planes), models


@pytest.mark.parametrize("name", ["color-P33", "vdn-P33", "color352-P129"])
def test_chain_of_head_models_equals_the_oracle(name):
    """small_inputs, head_layer0_input, dense_relu and dense_out on the unrounded image of the 'fwd' stream, fed their own outputs
    in float64, against rendering_forward on [points, view, normals, feature vector (+ the 96 appended channels)]."""
    c = mlp_cases.head_case(name)
    ops = _head_ops(c["net"], c["state"], exact=True)
    x = mlp_ops.head_layer0_input(c["feat"].astype(np.float64), mlp_ops.small_inputs(c["pts"], c["dirs"], c["normals"])["y"],
                                  None if c["extra"] is None else c["extra"].astype(np.float64))
    for l in range(4):
        x = mlp_ops.dense_relu(x, ops[l]["W"], ops[l]["b"])["y"]
    got = mlp_ops.dense_out(x, ops[4]["W"], ops[4]["b"], c["squeeze"], c["d_out"])["y"]
    sd = mlp_cases.head_states(c["state"])[mlp_cases.STATE_KEY[c["net"]]]
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    fv = c["feat"] if c["extra"] is None else np.concatenate([c["feat"], c["extra"]], -1)
    ref = orc.rendering_forward({k: t(v) for k, v in sd.items()}, t(c["pts"]), t(c["normals"]), t(c["dirs"]), t(fv),
                                orc.RenderingConf(d_feature=c["d_feature"], d_out=c["d_out"])).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()


@pytest.mark.parametrize("name", HEAD_NAMES)
def test_head_comparator_accepts_both_roundings_and_pins_relu_of_zero(name):
    c = mlp_cases.head_case(name)
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        planes = _head_sim(c, rnd=rnd)
        res, models = _head_judged(c, planes)
        for k, j in res.items():
            assert j["ok"], (name, rnd.__name__, k, j)
    for k, j in res.items():
        print("%-12s %-6s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
    # the silenced unit: pre-activation exactly zero, unit of the element zero, so nothing but an exact 0 passes
    u = mlp_cases.SILENT_UNIT
    for k in ("h0", "h2"):
        assert (models[k]["y64"][:, u] == 0).all() and (models[k]["unit"][:, u] == 0).all() and (planes[k][:, u] == 0).all()
        planes[k][0, u] = 2.0 ** -126
        assert not _head_judged(c, planes)[0][k]["ok"]
        planes[k][0, u] = 0.0
    assert (models["small"]["y64"][0, 7:30:6] == 0).all()               # row 0: sines of a zero component


def _head_bias_tile(ops):
    b = ops[1]["b"]
    b[32:64], b[64:96] = b[64:96].copy(), b[32:64].copy()
    return "h1"


def _head_small_columns(ops):
    """Layer 0: the normals' weight columns and the points' swapped."""
    W = ops[0]["W"]
    W[:, 256:259], W[:, 286:289] = W[:, 286:289].copy(), W[:, 256:259].copy()
    return "h0"


def _head_out_row(ops):
    """The output layer's rows 0 and 1 swapped."""
    ops[4]["W"][[0, 1]] = ops[4]["W"][[1, 0]]
    return "out"


HEAD_PLANTS = {"bias-tile": _head_bias_tile, "small-columns": _head_small_columns, "out-row": _head_out_row}


@pytest.mark.parametrize("name", HEAD_NAMES)
@pytest.mark.parametrize("plant", list(HEAD_PLANTS))
def test_head_comparator_rejects_each_planted_error(name, plant):
    c = mlp_cases.head_case(name)
    wrong = _copy(_head_ops(c["net"], c["state"]))
    where = HEAD_PLANTS[plant](wrong)
    res, _ = _head_judged(c, _head_sim(c, ops=wrong))
    assert not res[where]["ok"], (name, plant, res[where])
    for k, j in res.items():
        if k != where:
            assert j["ok"], (name, plant, k, j)


# ---- the colour head inside the fused SDF launches ------------------------------------------------------------------------------

FUSED_NAMES = list(mlp_cases.FUSED_CASES)


@functools.lru_cache(maxsize=None)
def _c2_host(state="heads"):
    from vdn_hip import images
    st = images.rendering_streams(d_feature=256, mode="idr", d_in=9, d_out=3, d_hidden=256, n_layers=4, multires_view=4)
    sd = mlp_cases.fused_states(state)["color_network_fine"]
    return mlp_ops.HostImages.of_sdf_state(sd, st, np.float32, n_layers=5)


@functools.lru_cache(maxsize=None)
def _c2_ops(state="heads"):
    return [mlp_ops.operand_weights(_c2_host(state), "c2", l) for l in range(5)]


@functools.lru_cache(maxsize=None)
def _fused_setup(name):
    """The case with the CPU stand-in of its SDF side (the float32 chain of simulate_sdf_forward on the case's SDF state): the
    feature plane, the same features unrounded, the f32 normals, per row of the saved planes."""
    c = mlp_cases.fused_case(name)
    host = mlp_ops.HostImages.of_sdf_state(mlp_cases.fused_states(c["state"])["sdf_network_fine"], _streams())
    ops, sweep = mlp_ops.sdf_ops(host), mlp_ops.sdf_sweep_ops(host)
    rows = mlp_cases.fused_rows_of(c)
    sp = mlp_ops.simulate_sdf_forward(ops, mlp_cases.fused_points_of(c)[rows], c["scale"], ops_sweep=sweep)
    raw = mlp_ops.sdf_last(sp["H7"], ops[8]["W"], ops[8]["b"], ops[8]["tail"], c["scale"], torch.float32)["feat"]
    rr = mlp_ops.ray_rows(c["rays_o"], c["rays_d"], c["z"], rows, torch.float32)
    return {"c": c, "rows": rows, "feat": sp["feat"], "feat_f32": raw, "normals": sp["normals"].astype(np.float32),
            "pts": rr["pts"], "dirs": rr["dirs"], "H_max": max(float(sp["H%d" % l].max()) for l in range(8))}


def _fused_sim(s, ops=None, rnd=mlp_ops.bf16_rne, **kw):
    a = dict(pts=s["pts"], dirs=s["dirs"], feat=s["feat"], nz=None)
    a.update(kw)
    return mlp_ops.simulate_fused_head_forward(ops or _c2_ops(), a["pts"], a["dirs"], s["normals"], a["feat"], True, rnd, nz=a["nz"])


def _fused_judged(s, planes):
    c = s["c"]
    models = mlp_ops.fused_head_plane_models(_c2_ops(), c["rays_o"], c["rays_d"], c["z"], s["rows"], s["normals"], s["feat"], planes,
                                             c["squeeze"], c["scale"])
    return mlp_ops.judge_planes(models, planes), models


def test_fused_cases_reach_every_row_path():
    cs = {n: mlp_cases.fused_case(n) for n in FUSED_NAMES}
    assert {c["P"] for c in cs.values() if c["active_idx"] is None} == {1, 33, 129, 300}
    assert {c["scale"] for c in cs.values()} == {1.0, 1.5} and cs["rays-12x25-s1.5"]["P"] == 300
    assert cs["rays-3x11-s1"]["n_per_ray"] == 11 and cs["rays-43x3-s1"]["n_per_ray"] == 3      # ray boundaries inside a wave
    w = cs["worklist-8x25-n77-s1"]
    idx = w["active_idx"][:77]
    assert w["P"] == 200 and len(set(idx.tolist())) == 77 and (np.diff(idx) < 0).any() and (w["active_idx"][77:] == -1).all()
    for n, c in cs.items():
        assert (c["rays_o"][0] == 0).all() and (c["rays_d"][0] == (1.0, 0.0, 0.0)).all(), n
        assert np.abs(np.linalg.norm(c["rays_d"], axis=1) - 1).max() < 1e-6
        if c["B"] > 1:          # far more than a bf16 step (2^-7 at 1) in every component of neighbouring rays
            assert np.abs(np.diff(c["rays_d"], axis=0)).min() >= mlp_cases.DIR_GAP > 4 * 2.0 ** -7, n
        if c["P"] >= 3:
            assert (c["z"] == 0).sum() == 1 and (c["z"] < 0).sum() == 1, n
    init, hot = _fused_setup("rays-43x3-s1"), _fused_setup("hot-43x3-s1")
    assert hot["H_max"] < 2.0 ** 10 and np.abs(hot["feat"]).max() > 4 * np.abs(init["feat"]).max()      # large features into the head
    for state in ("heads", "heads-other"):                   # the silenced unit's row of the tail column is zero as well
        o = _c2_ops(state)[0]
        u = mlp_cases.SILENT_UNIT
        assert o["W"].shape == (256, 288) and o["kt"] == 9 and o["tail"].shape == (256,)
        assert not o["W"][u].any() and o["b"][u] == 0 and o["tail"][u] == 0 and np.count_nonzero(o["tail"]) == 255
        assert np.array_equal(o["tail"], _c2_host(state).weff["lin0"][:, 32].astype(np.float64))
    flat = mlp_cases.fused_states("heads-flat")["sdf_network_fine"]
    assert flat["lin8.weight_g"][0] == 0 and np.count_nonzero(flat["lin8.weight_g"]) == flat["lin8.weight_g"].size - 1


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_fused_head_comparator_accepts_both_roundings_and_the_cases_cover(name):
    """No false alarm: the float32 stand-in passes every plane of every case, rounded either way. Coverage: the silenced unit gives
    exact zeros that admit nothing else; every hidden layer has relu inputs of both signs; on the init states no sigmoid output is
    saturated (all within [0.02, 0.98]), so that the output's unit measures the kernel."""
    s = _fused_setup(name)
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        planes = _fused_sim(s, rnd=rnd)
        res, models = _fused_judged(s, planes)
        assert set(res) == {"small", "h0", "h1", "h2", "h3", "out"}
        for k, j in res.items():
            assert j["ok"], (name, rnd.__name__, k, j)
    for k, j in res.items():
        print("%-22s %-6s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
    u = mlp_cases.SILENT_UNIT
    for k in ("h0", "h2"):
        assert (models[k]["y64"][:, u] == 0).all() and (models[k]["unit"][:, u] == 0).all() and (planes[k][:, u] == 0).all()
        assert np.all(np.broadcast_to(models[k]["extra"], models[k]["y64"].shape)[:, u] == 0)
        planes[k][0, u] = 2.0 ** -126
        assert not _fused_judged(s, planes)[0][k]["ok"]
        planes[k][0, u] = 0.0
    if s["c"]["P"] > 1:
        o = _c2_ops()
        t = [mlp_ops.fused_layer0(s["feat"], planes["small"], s["normals"][:, 2], o[0]["W"], o[0]["b"], o[0]["tail"])["t"]]
        t += [mlp_ops.dense_relu(planes["h%d" % (l - 1)], o[l]["W"], o[l]["b"])["t"] for l in (1, 2, 3)]
        assert all((a > 0).any() and (a < 0).any() for a in t)
    if s["c"]["state"] == "heads":
        assert planes["out"].min() >= 0.02 and planes["out"].max() <= 0.98, (planes["out"].min(), planes["out"].max())
    if name != "rays-1x1-s1":                               # ray 0: the sines of its zero components
        assert (models["small"]["y64"][s["rows"] < s["c"]["n_per_ray"]][:, [7, 8, 13, 14, 19, 20, 25, 26]] == 0).all()


def _fd_nz_bf16(s):
    return _fused_sim(s, nz=mlp_ops.bf16_rne(s["normals"][:, 2]))


def _fd_tail_column_31(s):
    ops = _copy(_c2_ops())
    ops[0]["tail"] = _c2_host().weff["lin0"][:, 31].astype(np.float64)
    return _fused_sim(s, ops=ops)


def _fd_small_30_31(s):
    planes = _fused_sim(s)
    # (the launch forms the tile once: the saved plane and the first layer's operand are swapped alike)
    sw = s["normals"].copy()
    sw[:, [0, 1]] = sw[:, [1, 0]]
    wrong = mlp_ops.simulate_fused_head_forward(_c2_ops(), s["pts"], s["dirs"], sw, s["feat"], True, nz=s["normals"][:, 2])
    assert np.array_equal(wrong["small"][:, :30], planes["small"][:, :30])
    return wrong


def _fd_next_rays_direction(s):
    c = s["c"]
    r = np.minimum((s["rows"] + 1) // c["n_per_ray"], c["B"] - 1)
    return _fused_sim(s, dirs=c["rays_d"][r].astype(np.float64))


def _fd_scaled_point(s):
    return _fused_sim(s, pts=s["pts"] * s["c"]["scale"]) if s["c"]["scale"] != 1.0 else None


def _fd_feature_unrounded(s):
    return _fused_sim(s, feat=s["feat_f32"])


def _fd_out_rows(s):
    ops = _copy(_c2_ops())
    ops[4]["W"][[0, 1]], ops[4]["b"][[0, 1]] = ops[4]["W"][[1, 0]], ops[4]["b"][[1, 0]]
    return _fused_sim(s, ops=ops)


def _fd_small_32_unwritten(s):
    planes = _fused_sim(s)
    planes["small"][:, 32] = np.nan                          # (what the NaN pre-fill of the GPU test leaves there)
    return planes


# planted defect -> (the plane that has to catch it, the stand-in with the defect; None where the case cannot show it)
FUSED_DEFECTS = {"nz-rounded-to-bf16": ("h0", _fd_nz_bf16), "tail-from-column-31": ("h0", _fd_tail_column_31),
                 "small-columns-30-31-swapped": ("small", _fd_small_30_31), "direction-of-the-next-ray": ("small", _fd_next_rays_direction),
                 "point-times-scale": ("small", _fd_scaled_point), "feature-operand-unrounded": ("h0", _fd_feature_unrounded),
                 "output-rows-permuted": ("out", _fd_out_rows), "small-column-32-unwritten": ("small", _fd_small_32_unwritten)}


@pytest.mark.parametrize("plant", list(FUSED_DEFECTS))
def test_fused_head_comparator_rejects_each_planted_defect(plant):
    """Each defect the fused head could have without the end-to-end tests noticing, planted into the float32 stand-in, is rejected on
    at least one committed case by the plane it is in (and wherever it is rejected, no plane BEFORE that one complains)."""
    where, make = FUSED_DEFECTS[plant]
    order = ["small", "h0", "h1", "h2", "h3", "out"]
    caught = []
    for name in FUSED_NAMES:
        s = _fused_setup(name)
        planes = make(s)
        if planes is None:
            continue
        res, _ = _fused_judged(s, planes)
        for k in order[:order.index(where)]:
            assert res[k]["ok"], (plant, name, k, res[k])
        if not res[where]["ok"]:
            caught.append(name)
        print("%-30s %-22s plane %-5s %s  error %.3g units (bound %.2f), %d of %d elements outside" % (
            plant, name, where, "REJECTED" if not res[where]["ok"] else "passes", res[where]["err"], res[where]["bound"],
            res[where]["n_bad"], res[where]["n"]))
    assert caught, "%s: plane %s rejects it on no case" % (plant, where)


# ---- the background network's forward -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nerf_ops(state="heads", exact=False):
    from vdn_hip import images
    st = images.nerf_streams(D=8, W=256, d_in=4, d_in_view=3, multires=10, multires_view=4, skips=(4,), rgb_dims=3,
                             gen_depth_feats=state != "nodpt", dpt_dim=96)
    img = mlp_ops.HostImages.of_linear_state(mlp_cases.head_states(state)["nerf"], st, np.float64 if exact else np.float32)
    return [mlp_ops.operand_weights(img, "fwd", l, rounded=not exact) for l in range(11)]


def _nerf_judged(c, planes):
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    models = mlp_ops.nerf_plane_models(_nerf_ops(c["state"]), pts4, dirs, planes)
    return mlp_ops.judge_planes(models, planes), models


@pytest.mark.parametrize("name", ["nerf-P33", "nerf-nodpt-P129"])
def test_chain_of_background_models_equals_the_oracle(name):
    """plain_encoding, nerf_inputs_of and the layers on the unrounded image of the 'fwd' stream, fed their own outputs in float64,
    against nerf_forward (with and without the dpt head)."""
    c = mlp_cases.nerf_case(name)
    ops = _nerf_ops(c["state"], exact=True)
    planes = {"pe": mlp_ops.plain_encoding(c["pts4"], 10)["y"], "vpe": mlp_ops.plain_encoding(c["dirs"], 4)["y"]}
    zero = {"h%d" % j: np.zeros((c["P"], 256)) for j in range(8)}
    for i in range(8):
        x = mlp_ops.nerf_inputs_of({**zero, "feature": zero["h0"], "hv": None, **planes})[i]
        planes["h%d" % i] = mlp_ops.dense_relu(x, ops[i]["W"], ops[i]["b"])["y"]
    y8, _ = mlp_ops._linear(planes["h7"], ops[8]["W"], ops[8]["b"], torch.float64)
    planes["feature"] = y8[:, :256]
    planes["hv"] = mlp_ops.dense_relu(mlp_ops.nerf_inputs_of({**planes, "hv": None})[9], ops[9]["W"], ops[9]["b"])["y"]
    y10, _ = mlp_ops._linear(planes["hv"], ops[10]["W"], ops[10]["b"], torch.float64)
    sd = mlp_cases.head_states(c["state"])["nerf"]
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    alpha, rgb, feat = orc.nerf_forward({k: t(v) for k, v in sd.items()}, t(c["pts4"]), t(c["dirs"]),
                                        orc.NeRFConf(gen_depth_feats=c["state"] != "nodpt"))
    pairs = [(y8[:, 256:257], alpha), (y10[:, :3], rgb)] + ([(y10[:, 32:128], feat)] if feat is not None else [])
    assert (feat is None) == (y10.shape[1] == 32)
    for got, want in pairs:
        assert got.shape == tuple(want.shape) and np.abs(got - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_comparator_accepts_both_roundings_and_pins_relu_of_zero(name):
    c = mlp_cases.nerf_case(name)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        planes = mlp_ops.simulate_nerf_forward(_nerf_ops(c["state"]), pts4, dirs, rnd)
        res, models = _nerf_judged(c, planes)
        for k, j in res.items():
            assert j["ok"], (name, rnd.__name__, k, j)
    for k, j in res.items():
        print("%-24s %-8s floor %.3f units  bound %.2f" % (name, k, j["floor"], j["bound"]))
    u = mlp_cases.SILENT_UNIT
    assert (models["h2"]["y64"][:, u] == 0).all() and (models["h2"]["unit"][:, u] == 0).all() and (planes["h2"][:, u] == 0).all()
    planes["h2"][0, u] = 2.0 ** -126
    assert not _nerf_judged(c, planes)[0]["h2"]["ok"]


def _nerf_bias_tile(ops):
    b = ops[3]["b"]
    b[32:64], b[64:96] = b[64:96].copy(), b[32:64].copy()
    return ["h3"]


def _nerf_skip_columns(ops):
    """Layer 5: the encoded input's weight columns behind the activations' instead of in front of them."""
    W = ops[5]["W"]
    ops[5]["W"] = np.concatenate([W[:, 96:352], W[:, :96]], -1)
    return ["h5"]


def _nerf_alpha_row(ops):
    """The density row of the head taken from row 0 of feature_linear."""
    ops[8]["W"][256] = ops[8]["W"][0]
    return ["density"]


def _nerf_view_columns(ops):
    """views_linears.0: the encoded view's columns shifted by one."""
    ops[9]["W"][:, 256:288] = np.roll(ops[9]["W"][:, 256:288], 1, axis=1)
    return ["hv"]


def _nerf_out_chunks(ops):
    """The output layer's dpt chunks 0 and 1 swapped."""
    W = ops[10]["W"]
    W[32:64], W[64:96] = W[64:96].copy(), W[32:64].copy()
    return ["feat"]


NERF_PLANTS = {"bias-tile": _nerf_bias_tile, "skip-columns": _nerf_skip_columns, "alpha-row": _nerf_alpha_row,
               "view-columns": _nerf_view_columns, "out-chunks": _nerf_out_chunks}


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
@pytest.mark.parametrize("plant", list(NERF_PLANTS))
def test_nerf_comparator_rejects_each_planted_error(name, plant):
    c = mlp_cases.nerf_case(name)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    wrong = _copy(_nerf_ops(c["state"]))
    where = NERF_PLANTS[plant](wrong)
    res, _ = _nerf_judged(c, mlp_ops.simulate_nerf_forward(wrong, pts4, dirs))
    for k, j in res.items():
        assert j["ok"] == (k not in where), (name, plant, k, j)


# ---- the heads' backward ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _head_bwd_ops(net, exact=False):
    from vdn_hip import images
    d_out = 3 if net == "color_network" else 96
    st = images.rendering_streams(d_feature=256, mode="idr", d_in=9, d_out=d_out, d_hidden=256, n_layers=4, multires_view=4)
    sd = mlp_cases.head_states("heads")[mlp_cases.STATE_KEY[net]]
    img = mlp_ops.HostImages.of_sdf_state(sd, st, np.float64 if exact else np.float32, n_layers=5)
    return [mlp_ops.operand_weights(img, "bwd", l, rounded=not exact) for l in range(5)]


@pytest.mark.parametrize("name", ["color-P33", "vdn-P33"])
def test_chain_of_head_backward_models_equals_autograd_of_the_oracle(name):
    """head_delta_out and relu_chain_step on the unrounded 'bwd' images, fed their own outputs in float64, against torch autograd
    of rendering_forward: d loss / d feature vector, d normals, d points for loss = sum(g_out . out)."""
    c = mlp_cases.head_case(name)
    sd = mlp_cases.head_states("heads")[mlp_cases.STATE_KEY[c["net"]]]
    t = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), requires_grad=grad)
    pts, nrm, fv = t(c["pts"], True), t(c["normals"], True), t(c["feat"], True)
    out = orc.rendering_forward({k: t(v) for k, v in sd.items()}, pts, nrm, t(c["dirs"]), fv, orc.RenderingConf(d_out=c["d_out"]))
    g_out = mlp_cases.head_upstream(c)
    (out * t(g_out)).sum().backward()
    # the forward's activations, from the exact forward chain
    ops = _head_ops(c["net"], "heads", exact=True)
    x = mlp_ops.head_layer0_input(c["feat"].astype(np.float64), mlp_ops.small_inputs(c["pts"], c["dirs"], c["normals"])["y"])
    hs = []
    for l in range(4):
        x = mlp_ops.dense_relu(x, ops[l]["W"], ops[l]["b"])["y"]
        hs.append(x)
    ob = _head_bwd_ops(c["net"], exact=True)
    d = mlp_ops.head_delta_out(g_out, out.detach().numpy(), c["squeeze"])["y"]
    for l in (3, 2, 1, 0):
        d = mlp_ops.relu_chain_step(d, ob[3 - l]["W"], hs[l] > 0)["y"]
    u = mlp_ops.relu_chain_step(d, ob[4]["W"], np.ones((c["P"], ob[4]["W"].shape[0])))["y"]
    for got, want in ((u[:, :256], fv.grad), (u[:, 286:289], nrm.grad), (u[:, 256:259], pts.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()


def _head_bwd_setup(c):
    """(g_out, out, the forward's h planes) of the CPU stand-in's forward."""
    fwd = _head_sim(c)
    return mlp_cases.head_upstream(c), fwd["out"], [fwd["h%d" % l] for l in range(4)]


def _head_bwd_judged(c, planes, g_out, out, hs):
    models = mlp_ops.head_bwd_plane_models(_head_bwd_ops(c["net"]), g_out, out, hs, planes, c["squeeze"], c["d_out"])
    return mlp_ops.judge_planes(models, planes)


@pytest.mark.parametrize("name", ["color-P33", "color-P129", "vdn-P33", "vdn-P300"])
def test_head_backward_comparator_accepts_both_roundings_and_rejects_planted_errors(name):
    c = mlp_cases.head_case(name)
    g_out, out, hs = _head_bwd_setup(c)
    ob = _head_bwd_ops(c["net"])
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        res = _head_bwd_judged(c, mlp_ops.simulate_head_backward(ob, g_out, out, hs, c["squeeze"], rnd), g_out, out, hs)
        for k, j in res.items():
            assert j["ok"], (name, rnd.__name__, k, j)
    # a mask taken from the neighbouring feature (layer 2); a 32-row tile of W_2^T swapped with its neighbour (delta_h1);
    # the normals' rows of W_0^T taken from the points'
    shifted = [h.copy() for h in hs]
    shifted[2] = np.roll(shifted[2], 1, axis=1)
    res = _head_bwd_judged(c, mlp_ops.simulate_head_backward(ob, g_out, out, shifted, c["squeeze"]), g_out, out, hs)
    assert not res["delta_h2"]["ok"] and all(j["ok"] for k, j in res.items() if k != "delta_h2"), res
    wrong = _copy(ob)
    W = wrong[2]["W"]
    W[32:64], W[64:96] = W[64:96].copy(), W[32:64].copy()
    res = _head_bwd_judged(c, mlp_ops.simulate_head_backward(wrong, g_out, out, hs, c["squeeze"]), g_out, out, hs)
    assert not res["delta_h1"]["ok"] and all(j["ok"] for k, j in res.items() if k != "delta_h1"), res
    wrong = _copy(ob)
    wrong[4]["W"][286:289] = wrong[4]["W"][256:259]
    res = _head_bwd_judged(c, mlp_ops.simulate_head_backward(wrong, g_out, out, hs, c["squeeze"]), g_out, out, hs)
    assert not res["d_normals"]["ok"] and all(j["ok"] for k, j in res.items() if k != "d_normals"), res


# ---- the background network's backward ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _nerf_bwd_ops(state="heads", exact=False):
    from vdn_hip import images
    st = images.nerf_streams(D=8, W=256, d_in=4, d_in_view=3, multires=10, multires_view=4, skips=(4,), rgb_dims=3,
                             gen_depth_feats=state != "nodpt", dpt_dim=96)
    img = mlp_ops.HostImages.of_linear_state(mlp_cases.head_states(state)["nerf"], st, np.float64 if exact else np.float32)
    return [mlp_ops.operand_weights(img, "bwd", l, rounded=not exact) for l in range(11)]


def _exact_rnd(a):
    return np.asarray(a, np.float64)


@pytest.mark.parametrize("name", ["nerf-P33", "nerf-nodpt-P129"])
def test_chain_of_background_backward_models_equals_autograd_of_the_oracle(name):
    """The delta chain on the unrounded 'bwd' images, fed the exact forward's activations and its own outputs in float64: the
    column sums of every delta plane are the bias gradients torch autograd gives for nerf_forward (loss = sum g . outputs)."""
    c = mlp_cases.nerf_case(name)
    sd = mlp_cases.head_states(c["state"])["nerf"]
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k.endswith(".bias")) for k, v in sd.items()}
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    g_density, g_rgb, g_feat = mlp_cases.nerf_upstream(c)
    alpha, rgb, feat = orc.nerf_forward(p, t(c["pts4"]), t(c["dirs"]), orc.NeRFConf(gen_depth_feats=g_feat is not None))
    loss = (alpha[:, 0] * t(g_density)).sum() + (rgb * t(g_rgb)).sum() + (0 if g_feat is None else (feat * t(g_feat)).sum())
    loss.backward()
    fwd = mlp_ops.simulate_nerf_forward(_nerf_ops(c["state"], exact=True), c["pts4"], c["dirs"], rnd=_exact_rnd, dtype=torch.float64)
    planes = mlp_ops.simulate_nerf_backward(_nerf_bwd_ops(c["state"], exact=True), g_density, g_rgb, g_feat,
                                            [fwd["h%d" % l] for l in range(8)], fwd["hv"], rnd=_exact_rnd, dtype=torch.float64)
    want = {"delta_h%d" % l: p["pts_linears.%d.bias" % l].grad for l in range(8)}
    want["delta_v"] = p["views_linears.0.bias"].grad
    want["delta_head"] = torch.cat([p["feature_linear.bias"].grad, p["alpha_linear.bias"].grad])
    for k, w in want.items():
        got = planes[k].sum(0)
        assert got.shape == tuple(w.shape) and np.abs(got - w.numpy()).max() <= 1e-10 * np.abs(w.numpy()).max(), k


@pytest.mark.parametrize("name", list(mlp_cases.NERF_CASES))
def test_nerf_backward_comparator_accepts_both_roundings_and_rejects_planted_errors(name):
    c = mlp_cases.nerf_case(name)
    pts4, dirs = mlp_cases.nerf_rows_of(c)
    g = [None if a is None else (a if c["active_idx"] is None else a[c["active_idx"][:c["n_active"]]]) for a in mlp_cases.nerf_upstream(c)]
    fwd = mlp_ops.simulate_nerf_forward(_nerf_ops(c["state"]), pts4, dirs)
    hs, hv, ob = [fwd["h%d" % l] for l in range(8)], fwd["hv"], _nerf_bwd_ops(c["state"])
    judged = lambda planes: mlp_ops.judge_planes(mlp_ops.nerf_bwd_plane_models(ob, *g, hs, hv, planes), planes)
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        res = judged(mlp_ops.simulate_nerf_backward(ob, *g, hs, hv, rnd))
        for k, j in res.items():
            assert j["ok"], (name, rnd.__name__, k, j)
    # the skip's rows of W_5^T read in the forward's unpadded order (h_4 from row 84); the mask of layer 2 from the neighbouring
    # feature; the density adjoint left out of the head's delta
    wrong = _copy(ob)
    wrong[5]["W"] = np.roll(wrong[5]["W"], 12, axis=0)
    res = judged(mlp_ops.simulate_nerf_backward(wrong, *g, hs, hv))
    assert not res["delta_h4"]["ok"] and all(j["ok"] for k, j in res.items() if k != "delta_h4"), res
    shifted = [h.copy() for h in hs]
    shifted[2] = np.roll(shifted[2], 1, axis=1)
    res = judged(mlp_ops.simulate_nerf_backward(ob, *g, shifted, hv))
    assert not res["delta_h2"]["ok"] and all(j["ok"] for k, j in res.items() if k != "delta_h2"), res
    if c["P"] > 1:                                       # (row 0's upstream gradients are zero)
        planes = mlp_ops.simulate_nerf_backward(ob, np.zeros_like(g[0]), g[1], g[2], hs, hv)
        res = judged(planes)
        assert not res["delta_head"]["ok"]


# ---- the SDF backward -----------------------------------------------------------------------------------------------------------

def _exact_sdf_chain(c, sd):
    """The exact forward and sweep (float64, unrounded images, the reference's thresholded softplus'): ops, fbar ops, H, V."""
    img = mlp_ops.HostImages.of_sdf_state(sd, _streams(), np.float64)
    ops, ows, ofb = mlp_ops.sdf_ops(img, rounded=False), mlp_ops.sdf_sweep_ops(img, rounded=False), mlp_ops.sdf_fbar_ops(img, rounded=False)
    x = mlp_ops.posenc_scaled(c["pts"], c["scale"])["y"]
    g, H = None, []
    for l in range(8):
        g = mlp_ops.sdf_hidden(l, g, (x, x) if l in (0, 4) else None, ops[l]["W"], ops[l]["b"], aten_threshold=True)["y"]
        H.append(np.concatenate([g, np.zeros((c["P"], 256 - g.shape[1]))], -1))
    u = np.repeat(ops[8]["tail"][None, :] / c["scale"], c["P"], 0)
    V = [None] * 8
    for l in range(7, -1, -1):
        v = mlp_ops.sdf_sweep(l, u, H[l], aten_threshold=True)["y"]
        V[l] = np.concatenate([v, np.zeros((c["P"], 256 - v.shape[1]))], -1)
        u = mlp_ops.sweep_u(l, V[l][:, :224] if l == 3 else V[l], ows[l]["W"])["u"]
        if l == 4:
            u = u[:, :217]
    return ops, ofb, H, V


@pytest.mark.parametrize("kind", mlp_cases.SDF_UPSTREAM)
def test_chain_of_sdf_backward_models_equals_autograd_of_the_oracle(kind):
    """pe_jacobian, sdf_rbar_step and sdf_fbar_step (the closed forms of DESIGN.md section 4) on unrounded images, fed the exact
    forward / sweep and their own outputs in float64: the column sums of the ab blocks are the bias gradients that torch autograd
    gives for loss = g_sdf . sdf + g_feat . feat + g_n . (d sdf / d x) of sdf_forward(with_gradient=True) - a double backward."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    sd = mlp_cases.states()["sdf_network_fine"]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k.endswith(".bias")) for k, v in sd.items()}
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    out, grad = orc.sdf_forward(p, t(c["pts"]), orc.SDFConf(scale=c["scale"]), with_gradient=True)
    ((out[:, 0] * t(g_sdf)).sum() + (out[:, 1:] * t(g_feat)).sum() + (grad * t(g_n)).sum()).backward()
    ops, ofb, H, V = _exact_sdf_chain(c, sd)
    ub, EX, ab = mlp_ops.simulate_sdf_backward(ops, ofb, c["pts"], c["scale"], g_sdf, g_feat, g_n, H, V, rnd=_exact_rnd,
                                               dtype=torch.float64, aten_threshold=True)
    for l in range(8):
        want = p["lin%d.bias" % l].grad.numpy()
        got = ab[l].sum(0)[:len(want)]
        assert np.abs(got - want).max() <= 1e-10 * max(np.abs(want).max(), 1e-300), (l, np.abs(got - want).max(), np.abs(want).max())
    want = p["lin8.bias"].grad.numpy()
    got = np.concatenate([ab[8].sum(0)[256:257], ab[8].sum(0)[:256]])
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    if kind == "g_normals=0":
        assert all((b == 0).all() for b in ub) and all((e == 0).all() for e in EX)


@functools.lru_cache(maxsize=None)
def _fbar_ops(state="init"):
    sd = mlp_cases.states(state)["sdf_network_fine"]
    return mlp_ops.sdf_fbar_ops(mlp_ops.HostImages.of_sdf_state(sd, _streams()))


def _sdf_bwd_judged(c, kind, H, V, ub, EX, ab):
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    models = mlp_ops.sdf_bwd_models(_ops(c["state"]), _fbar_ops(c["state"]), mlp_cases.rows_of(c), c["scale"], g_sdf[sel],
                                    mlp_ops.bf16_rne(g_feat[sel]), g_n[sel], H, V, ub, EX, ab)
    planes = {"ub0": ub[0][:, :39], "ub4pe": ub[4][:, 224:263], "ab8": ab[8][:, :257]}
    for l in range(8):
        w = 217 if l == 3 else 256
        planes["ub%d" % (l + 1)], planes["EX%d" % l], planes["ab%d" % l] = ub[l + 1][:, :w], EX[l][:, :w], ab[l][:, :w]
    return mlp_ops.judge_planes(models, planes)


@pytest.mark.parametrize("name,kind", [(n, "random") for n in NAMES] + [("uniform-P129-s1", "g_feat=0"), ("uniform-P129-s1", "g_normals=0")])
def test_sdf_backward_comparator_accepts_both_roundings_and_rejects_planted_errors(name, kind):
    """The stand-in of rbar + fbar on the stand-in forward's planes: accepted rounded either way; rejected with ex_l without the
    100 (ln 2 / 100 in scaled units), with sigma formed from H in the network's units, with a bias-free tile of W_2 swapped, and
    with the second-order term left out of ab_5 - each at the block the error is in and at no other."""
    c = mlp_cases.sdf_case(name)
    fwd = _sim(c)
    H, V = [fwd["H%d" % l] for l in range(8)], [fwd["V%d" % l] for l in range(8)]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c, kind)
    sel = np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    args = (mlp_cases.rows_of(c), c["scale"], g_sdf[sel], mlp_ops.bf16_rne(g_feat[sel]), g_n[sel], H, V)
    ops, ofb = _ops(c["state"]), _fbar_ops(c["state"])
    for rnd in (mlp_ops.bf16_rne, mlp_ops.bf16_trunc):
        res = _sdf_bwd_judged(c, kind, H, V, *mlp_ops.simulate_sdf_backward(ops, ofb, *args, rnd=rnd))
        for k, j in res.items():
            assert j["ok"], (name, kind, rnd.__name__, k, j)
    for k, j in res.items():
        print("%-22s %-12s %-6s floor %.3f units  bound %.2f" % (name, kind, k, j["floor"], j["bound"]))
    if kind == "g_normals=0":                            # (nothing but the forward's adjoint: the plants below have nothing to bite on)
        return
    only = lambda res, where: all(j["ok"] == (k not in where) for k, j in res.items())
    # ex_l without the 100: every EX plane wrong, nothing else (fbar is teacher-forced on the EX it is given)
    res = _sdf_bwd_judged(c, kind, H, V, *mlp_ops.simulate_sdf_backward(ops, ofb, *args, ex_factor=mlp_ops.LN2 / 100.0))
    assert only(res, ["EX%d" % l for l in range(8)]), {k: j["ok"] for k, j in res.items()}
    # sigma of layer 5 from H in the network's units
    Hn = [h / mlp_ops.C if l == 5 else h for l, h in enumerate(H)]
    res = _sdf_bwd_judged(c, kind, H, V, *mlp_ops.simulate_sdf_backward(ops, ofb, mlp_cases.rows_of(c), c["scale"], g_sdf[sel],
                                                                      mlp_ops.bf16_rne(g_feat[sel]), g_n[sel], Hn, V))
    assert only(res, ["ub6", "EX5", "ab5"]), {k: j["ok"] for k, j in res.items()}
    wrong = _copy(ops)
    W = wrong[2]["W"]
    W[32:64], W[64:96] = W[64:96].copy(), W[32:64].copy()
    res = _sdf_bwd_judged(c, kind, H, V, *mlp_ops.simulate_sdf_backward(wrong, ofb, *args))
    assert only(res, ["ub3", "EX2"]), {k: j["ok"] for k, j in res.items()}
    ub, EX, ab = mlp_ops.simulate_sdf_backward(ops, ofb, *args)
    EX0 = [e.copy() for e in EX]
    EX0[5][:] = 0.0
    ab5 = mlp_ops.bf16_rne(mlp_ops.sdf_fbar_step(6, ab[6], ofb[6]["W"], H[5], EX0[5], torch.float32)["y"])
    ab_wrong = list(ab)
    ab_wrong[5] = ab5
    res = _sdf_bwd_judged(c, kind, H, V, ub, EX, ab_wrong)
    assert only(res, ["ab5", "ab4"]) or only(res, ["ab5"]), {k: j["ok"] for k, j in res.items()}


@pytest.mark.parametrize("name", ["nerf-P33", "nerf-nodpt-P129"])
def test_background_input_adjoint_models_equal_autograd_of_the_oracle(name):
    """encoding_jacobian_T behind the exact delta chain: d loss / d input_pts and d loss / d input_views of nerf_forward."""
    c = mlp_cases.nerf_case(name)
    sd = mlp_cases.head_states(c["state"])["nerf"]
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    x, v = t(c["pts4"], True), t(c["dirs"], True)
    g_density, g_rgb, g_feat = mlp_cases.nerf_upstream(c)
    alpha, rgb, feat = orc.nerf_forward({k: t(a) for k, a in sd.items()}, x, v, orc.NeRFConf(gen_depth_feats=g_feat is not None))
    ((alpha[:, 0] * t(g_density)).sum() + (rgb * t(g_rgb)).sum() + (0 if g_feat is None else (feat * t(g_feat)).sum())).backward()
    fwd = mlp_ops.simulate_nerf_forward(_nerf_ops(c["state"], exact=True), c["pts4"], c["dirs"], rnd=_exact_rnd, dtype=torch.float64)
    ob = _nerf_bwd_ops(c["state"], exact=True)
    planes = mlp_ops.simulate_nerf_backward(ob, g_density, g_rgb, g_feat, [fwd["h%d" % l] for l in range(8)], fwd["hv"],
                                            rnd=_exact_rnd, dtype=torch.float64)
    m = mlp_ops.nerf_input_adjoint_models(ob, c["pts4"], c["dirs"], planes)
    for k, want in (("d_pts4", x.grad), ("d_dirs", v.grad)):
        assert np.abs(m[k]["y64"] - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max(), k


def test_sdf_d_pts_model_equals_autograd_of_the_oracle():
    """The ray adjoint of the SDF backward: d loss / d x of sdf_forward(with_gradient=True) under autograd (a double backward
    through the sweep), against sdf_d_pts_model on the exact chain's ab_0, ab_4 and U_pe."""
    c = mlp_cases.sdf_case("uniform-P33-s1.5")
    sd = mlp_cases.states()["sdf_network_fine"]
    g_sdf, g_feat, g_n = mlp_cases.sdf_upstream(c)
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    x = t(c["pts"], True)
    out, grad = orc.sdf_forward({k: t(v) for k, v in sd.items()}, x, orc.SDFConf(scale=c["scale"]), with_gradient=True)
    ((out[:, 0] * t(g_sdf)).sum() + (out[:, 1:] * t(g_feat)).sum() + (grad * t(g_n)).sum()).backward()
    ops, ofb, H, V = _exact_sdf_chain(c, sd)
    ub, EX, ab = mlp_ops.simulate_sdf_backward(ops, ofb, c["pts"], c["scale"], g_sdf, g_feat, g_n, H, V, rnd=_exact_rnd,
                                               dtype=torch.float64, aten_threshold=True)
    img = mlp_ops.HostImages.of_sdf_state(sd, _streams(), np.float64)
    ows = mlp_ops.sdf_sweep_ops(img, rounded=False)
    U_pe = mlp_ops.sweep_u(0, V[0], ows[0]["W"])["u"][:, :39] + mlp_ops.sweep_u(4, V[4], ows[4]["W"])["u"][:, 224:263]
    m = mlp_ops.sdf_d_pts_model(ofb, c["pts"], c["scale"], g_n, U_pe, ab[0], ab[4])
    assert np.abs(m["y64"] - x.grad.numpy()).max() <= 1e-10 * np.abs(x.grad.numpy()).max()
