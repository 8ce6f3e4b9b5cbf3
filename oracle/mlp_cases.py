"""Constructed inputs of the bf16 plane tests (oracle/mlp_ops.py, tests/test_gpu_mlp_planes.py), deterministic from the
case name: the SDF network first, then the heads, the colour head inside the fused SDF launches (tests/test_gpu_fused_head_planes.py),
the SDF launches that save no planes with the tail hand-off (tests/test_gpu_sdf_value_launches.py: SDF_VALUE_CASES, which alone go
beyond 300 rows - the entry point routes on P > 8192, the cold-start prologue reads ahead from 128 workgroups on) and the background
network. tests/test_mlp_ops_model_cpu.py proves their coverage without a GPU.

Row counts: 1 (one row), 33 (one row past a 32-row pad block), 129 (one row past a 128-row workgroup), 300 (two full workgroups
and a partial one whose last block is partial); one work list: 77 of 200 rows, not ascending, so that saves in compact rows
against outputs in dense rows shows. Nothing larger: these are the smallest shapes that reach every row path.
Points: uniform in [-1.1, 1.1]^3; one case on the lattice {-1, 0, 1}^3 (exact zeros and +-1). SDFNetwork scale 1 and 1.5.
Weights: "init" = synth.make_all_states(3, wdepth=True, variance=0.3), where every hidden layer has 22 - 30 % of its units on the knee
of softplus (0.02 < sigma < 0.98). "hot" = the same state with weight_g of the hidden SDF layers scaled by HOT_FACTORS, chosen per
layer on the CPU (float64 model, 300 points) so that every layer reaches the kernel's range switches (DESIGN.md 3a, round 3:
g = t from t >= 25, w = +inf from t = 128): at least 4 % of each layer's units in each of t >= 128, t <= -128, 25 <= t < 128 and
|t| < 5, with max H < 2^10 (one factor for all layers does not do it: activations compound and the knee empties). "other" (seed
4) is the state of the wiring check. The fp32 plane tests (tests/test_gpu_mlp_planes_f32.py) run the same cases and add only
SDF_F32_CASES (a pre-activation that is exactly 0) and sdf_d_pts_prefill (what d_pts holds before an acc_pts = 1 launch)."""
import numpy as np

from vdn_train import synth

SEED, OTHER_SEED = 3, 4
HOT_FACTORS = (4.0, 1.0, 1.0, 1.0, 1.4, 1.0, 1.0, 1.4)

# name: (P, scale, points, n_active, weight state)
SDF_CASES = {
    "uniform-P1-s1": (1, 1.0, "uniform", None, "init"),
    "uniform-P33-s1.5": (33, 1.5, "uniform", None, "init"),
    "lattice-P33-s1": (33, 1.0, "lattice", None, "init"),
    "uniform-P129-s1": (129, 1.0, "uniform", None, "init"),
    "uniform-P300-s1.5": (300, 1.5, "uniform", None, "init"),
    "worklist-P200-n77-s1": (200, 1.0, "uniform", 77, "init"),
    "hot-P129-s1": (129, 1.0, "uniform", None, "hot"),
    "hot-P300-s1.5": (300, 1.5, "uniform", None, "hot"),
}


# The fp32 plane tests (tests/test_gpu_mlp_planes_f32.py) run SDF_CASES as they are and this one more: state "silent" = "init" with
# unit 7 of lin2 silenced (weight_g = bias = 0), so that its pre-activation is exactly 0: H = ln 2 / 100 and S = 1/2 exactly - the
# boundary of the fp32 kernel's a >= 0 ? r : e r.
SDF_F32_CASES = {"silent-P33-s1": (33, 1.0, "uniform", None, "silent")}
SDF_SILENT = (2, 7)                                    # (layer, unit)


def states(state="init"):
    st = synth.make_all_states(OTHER_SEED if state == "other" else SEED, wdepth=True, variance=0.3)
    if state == "silent":
        sd = st["sdf_network_fine"]
        sd["lin%d.weight_g" % SDF_SILENT[0]][SDF_SILENT[1]] = 0.0
        sd["lin%d.bias" % SDF_SILENT[0]][SDF_SILENT[1]] = 0.0
    if state == "hot":
        sd = st["sdf_network_fine"]
        for l, f in enumerate(HOT_FACTORS):
            sd["lin%d.weight_g" % l] = sd["lin%d.weight_g" % l] * np.float32(f)
    return st


def sdf_case(name):
    P, scale, kind, n_active, state = SDF_CASES[name] if name in SDF_CASES else SDF_F32_CASES[name]
    if kind == "uniform":
        pts = (2.2 * synth.uniform(SEED, "mlp/%s/pts" % name, (P, 3)) - 1.1).astype(np.float32)
    else:
        pts = (np.floor(3.0 * synth.uniform(SEED, "mlp/%s/pts" % name, (P, 3))) - 1.0).astype(np.float32)
        pts[0] = 0.0                                   # the origin itself: every sine exactly zero
        pts[1], pts[2] = 1.0, -1.0
    c = {"name": name, "P": P, "scale": scale, "pts": pts, "active_idx": None, "n_active": None, "state": state}
    if n_active is not None:
        order = np.argsort(synth.uniform(SEED, "mlp/%s/order" % name, (P,)))      # a permutation: not ascending, not contiguous
        idx = np.full(P, -1, np.int32)
        idx[:n_active] = order[:n_active]
        c["active_idx"], c["n_active"] = idx, n_active
    return c


def rows_of(c):
    """The points behind the rows of the saved planes: the listed ones in list order, or all of them."""
    return c["pts"] if c["active_idx"] is None else c["pts"][c["active_idx"][:c["n_active"]]]


# ---- the heads ---------------------------------------------------------------------------------------------------------------
# name: (network, P). Inputs: points uniform in [-1.1, 1.1]^3, unit view directions, normals ~ N(0, 1), a feature plane of
# bf16 values ~ N(0, 0.3) (what the SDF forward leaves there). Row 0 looks along +x from the origin with a zero normal and a zero
# feature vector: every sine exactly zero. State "init" with unit 7 of layers 0 and 2 silenced (weight_g = bias = 0): a
# pre-activation that is exactly zero, so that relu(0) = 0 and its mask bit are pinned (background network: unit 7 of pts_linears.2).
# "color352": the d_feature = 352 colour network (13 k-tiles in its first layer, the 96 appended channels behind the small inputs).
HEAD_CASES = {"color-P33": ("color_network", 33), "color-P129": ("color_network", 129), "vdn-P33": ("depth_network", 33),
              "vdn-P300": ("depth_network", 300), "color352-P129": ("color_network", 129)}
SILENT_UNIT = 7
STATE_KEY = {"color_network": "color_network_fine", "depth_network": "depth_network_fine"}


def head_states(state="heads"):
    """"heads": the init state with the silenced units; "heads-other": seed 4 likewise (the wiring check); "heads352": with the
    d_feature = 352 colour network; "nodpt": without the VDN head and the background network's dpt head."""
    if state == "heads352":
        st = synth.make_all_states(SEED, wdepth=True, variance=0.3, depth_before_color=True)
    elif state == "nodpt":
        st = synth.make_all_states(SEED, wdepth=False, variance=0.3)
    else:
        st = states("other" if state == "heads-other" else "init")
    st["nerf"]["pts_linears.2.weight"][SILENT_UNIT] = 0.0
    st["nerf"]["pts_linears.2.bias"][SILENT_UNIT] = 0.0
    for key in STATE_KEY.values():
        if st[key] is None:
            continue
        for l in (0, 2):
            st[key]["lin%d.weight_g" % l][SILENT_UNIT] = 0.0
            st[key]["lin%d.bias" % l][SILENT_UNIT] = 0.0
    return st


def head_case(name):
    net, P = HEAD_CASES[name]
    u = lambda tag, shape: synth.uniform(SEED, "mlp/%s/%s" % (name, tag), shape)
    n = lambda tag, shape: synth.normal(SEED, "mlp/%s/%s" % (name, tag), shape)
    pts = (2.2 * u("pts", (P, 3)) - 1.1).astype(np.float32)
    dirs = n("dirs", (P, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    normals = n("normals", (P, 3)).astype(np.float32)
    feat = (0.3 * n("feat", (P, 256))).astype(np.float32)
    pts[0], dirs[0], normals[0], feat[0] = 0.0, (1.0, 0.0, 0.0), 0.0, 0.0
    wide = name.startswith("color352")
    return {"name": name, "net": net, "P": P, "pts": pts, "dirs": dirs, "normals": normals, "feat": feat,
            "d_out": 3 if net == "color_network" else 96, "squeeze": True, "state": "heads352" if wide else "heads",
            "d_feature": 352 if wide else 256, "extra": (0.3 * n("extra", (P, 96))).astype(np.float32) if wide else None}


def head_upstream(c):
    """g_out [P,d_out] ~ N(0, 1) of a head case (the backward's upstream gradient); row 0 zero."""
    g = synth.normal(SEED, "mlp/%s/g_out" % c["name"], (c["P"], c["d_out"])).astype(np.float32)
    g[0] = 0.0
    return g


# ---- the colour head inside the fused SDF launches (csrc/k_sdf_fwd2.h MODE 3 / 2 / 4) -------------------------------------------
# MODE 3 (vdn_sdf_color_train_bf16), name: (rays, samples per ray, SDFNetwork scale, n_active, weight state). Ray form only (the
# entry point rejects `pts`), the smallest shapes that reach every row path: 1 row; 33 rows with ray boundaries at lanes 11 and 22
# of a wave and one row past a pad block; 129 rows, one past a workgroup, the ray changing every 3 lanes; 300 rows at scale 1.5; a
# work list of 77 of 200 rows, not ascending; 129 rows on the "hot" SDF state (large features into the head, max H < 2^10).
# rays_o uniform in [-0.6, 0.6]^3, unit rays_d, every component of neighbouring rays at least DIR_GAP apart (a bf16 step at 1 is
# 2^-7: the direction of the wrong ray shows in every column), z uniform in [0.05, 1]. Ray 0 starts at the origin and looks along
# +x (the sines of its zero components are exactly zero). From 3 rows on the last depth is exactly 0 and the middle one negative.
# Weight states: fused_states below; the colour network always with unit 7 of layers 0 and 2 silenced (head_states), so that its
# row of the first layer's tail column is zero as well and h0[:, 7] is pinned to exactly 0.
FUSED_CASES = {
    "rays-1x1-s1": (1, 1, 1.0, None, "heads"),
    "rays-3x11-s1": (3, 11, 1.0, None, "heads"),
    "rays-43x3-s1": (43, 3, 1.0, None, "heads"),
    "rays-12x25-s1.5": (12, 25, 1.5, None, "heads"),
    "worklist-8x25-n77-s1": (8, 25, 1.0, 77, "heads"),
    "hot-43x3-s1": (43, 3, 1.0, None, "heads-hot"),
}
DIR_GAP = 0.05


def fused_states(state="heads"):
    """"heads" / "heads-other": head_states; "heads-hot": "heads" with the hot SDF network (HOT_FACTORS); "heads-flat": "heads"
    with lin8.weight_g[0] = 0 - row 0 of W_8 is zero, the sdf is the constant b_8[0] and its gradient exactly zero everywhere."""
    st = head_states("heads-other" if state == "heads-other" else "heads")
    sd = st["sdf_network_fine"]
    if state == "heads-hot":
        for l, f in enumerate(HOT_FACTORS):
            sd["lin%d.weight_g" % l] = sd["lin%d.weight_g" % l] * np.float32(f)
    elif state == "heads-flat":
        sd["lin8.weight_g"][0] = 0.0
    return st


def _unit_dirs(tag, n, first=None):
    """n unit directions, deterministic (the first one given, or drawn); each differs from the one before it by at least DIR_GAP
    in every component."""
    out = [] if first is None else [np.asarray(first, np.float32)]
    for r in range(len(out), n):
        for k in range(64):
            d = synth.normal(SEED, "mlp/%s/%d/%d" % (tag, r, k), (3,))
            d = (d / np.linalg.norm(d)).astype(np.float32)
            if not out or np.abs(d - out[-1]).min() >= DIR_GAP:
                break
        else:
            raise AssertionError("no direction found")
        out.append(d)
    return np.stack(out)


def _ray_case(name, B, n, scale, n_active, state):
    """The ray recipe of FUSED_CASES (and of the ray form of SDF_VALUE_CASES): see the comment above FUSED_CASES."""
    u = lambda tag, shape: synth.uniform(SEED, "mlp/%s/%s" % (name, tag), shape)
    rays_o = (1.2 * u("rays_o", (B, 3)) - 0.6).astype(np.float32)
    rays_d = _unit_dirs(name + "/rays_d", B, first=(1.0, 0.0, 0.0))
    rays_o[0] = 0.0
    z = (0.05 + 0.95 * u("z", (B, n))).astype(np.float32)
    if z.size >= 3:
        z.reshape(-1)[-1], z.reshape(-1)[z.size // 2] = 0.0, -0.25
    c = {"name": name, "B": B, "n_per_ray": n, "P": B * n, "scale": scale, "rays_o": rays_o, "rays_d": rays_d, "z": z,
         "active_idx": None, "n_active": None, "state": state, "squeeze": True}
    if n_active is not None:
        order = np.argsort(u("order", (B * n,)))
        idx = np.full(B * n, -1, np.int32)
        idx[:n_active] = order[:n_active]
        c["active_idx"], c["n_active"] = idx, n_active
    return c


def fused_case(name):
    return _ray_case(name, *FUSED_CASES[name])


def fused_rows_of(c):
    """The dense point ids (ray * n_per_ray + sample) behind the rows of the saved planes: the listed ones in list order, or all."""
    return np.arange(c["P"]) if c["active_idx"] is None else c["active_idx"][:c["n_active"]].astype(np.int64)


def fused_points_of(c):
    """The float32 points o + d z of every dense point id, as the reference forms them (renderer.py:233): for the CPU stand-in of
    the SDF side."""
    p = c["rays_o"][:, None, :] + c["rays_d"][:, None, :] * c["z"][:, :, None]
    return p.reshape(-1, 3).astype(np.float32)


# ---- the bf16 SDF launches that save no planes (tests/test_gpu_sdf_value_launches.py) ------------------------------------------
# vdn_sdf_mlp_fwd_bf16 mode 0 (csrc/k_sdf_fwd0_split.h up to 8192 points, csrc/k_sdf_fwd2.h MODE 0 beyond) and mode 1 without saves.
# SDF_VALUE_CASES = SDF_CASES as they are (explicit points), the ray cases and the large cases below.
# Ray form, name: (rays, samples per ray, SDFNetwork scale, n_active, (z_ld, first z column), (sdf_ld, first sdf column)). z and sdf
# are column slices of wider rows: z_ld > n_per_ray, sdf_ld > n_per_ray, sdf_ld != z_ld, both first columns non-zero; the columns of
# z outside the slice hold depths in [1.5, 2.5], which no sample has. Rays and depths: the recipe of FUSED_CASES (DIR_GAP; ray 0 from
# the origin along +x; the last depth 0, the middle one negative). 1 row; 33 rows with ray boundaries at lanes 11 and 22 of a wave;
# 5 rays of 16 = the split kernel's two rays per 32-point workgroup, 2 1/2 workgroups; 2 rays of 64 = one 128-point workgroup;
# 129 rows at scale 1.5 with the ray changing every 43 lanes; a work list of 77 of 200 rows, not ascending. Weight state "init".
SDF_VALUE_RAY_CASES = {
    "value-rays-1x1-s1": (1, 1, 1.0, None, (3, 1), (4, 2)),
    "value-rays-3x11-s1": (3, 11, 1.0, None, (16, 3), (13, 2)),
    "value-rays-5x16-s1": (5, 16, 1.0, None, (24, 5), (20, 3)),
    "value-rays-2x64-s1": (2, 64, 1.0, None, (80, 9), (72, 4)),
    "value-rays-3x43-s1.5": (3, 43, 1.5, None, (50, 6), (47, 1)),
    "value-rays-worklist-8x25-n77-s1": (8, 25, 1.0, 77, (32, 4), (29, 3)),
}
# The large kernel (the entry point routes on P > 8192), name: (P, n_active): 64 workgroups of 128 points and one row; a work list
# of 77 rows, not ascending, in P = 8200. Point i is point i % 300 of SDF_VALUE_TILE: only 300 rows need a model, and every
# repetition must carry the same bits.
SDF_VALUE_LARGE_CASES = {"value-tiled-P8193-s1.5": (8193, None), "value-tiled-worklist-P8200-n77-s1.5": (8200, 77)}
SDF_VALUE_TILE = "uniform-P300-s1.5"
SDF_VALUE_CASES = tuple(SDF_CASES) + tuple(SDF_VALUE_RAY_CASES) + tuple(SDF_VALUE_LARGE_CASES)
Z_GAP_FILL = (1.5, 2.5)
# cold_start = 1: the prologue only reads ahead in launches whose first round has at least 128 workgroups (csrc/vdn_common.h:
# warm_l2_issue), so these are the smallest shapes that run it - 129 workgroups of the split kernel (32 points each, P <= 8192) and
# of the 128-point kernels, on tiled points and in ray form (65 and 257 rays of 64). They are compared with cold_start = 0 only
# (and, tiled, with the 300-row case); not part of SDF_VALUE_CASES.
SDF_COLD_TILED_CASES = {"cold-tiled-P4097-s1.5": (4097, None), "cold-tiled-P16385-s1.5": (16385, None)}
SDF_COLD_RAY_CASES = {"cold-rays-65x64-s1": (65, 64, 1.0, None, (80, 9), (72, 4)), "cold-rays-257x64-s1": (257, 64, 1.0, None, (80, 9), (72, 4))}


def sdf_value_case(name):
    """A case of SDF_VALUE_CASES. "form" = "pts" (sdf_case's keys; "tile" = the period of a large case's points) or "rays" (the
    ray keys of fused_case, and z_wide [B, z_ld] with z = z_wide[:, z_col0 : z_col0 + n_per_ray], z_ld, z_col0, sdf_ld, sdf_col0)."""
    if name in SDF_CASES:
        return dict(sdf_case(name), form="pts", tile=None)
    if name in SDF_VALUE_LARGE_CASES or name in SDF_COLD_TILED_CASES:
        P, n_active = SDF_VALUE_LARGE_CASES[name] if name in SDF_VALUE_LARGE_CASES else SDF_COLD_TILED_CASES[name]
        t = sdf_case(SDF_VALUE_TILE)
        c = {"name": name, "form": "pts", "tile": t["P"], "P": P, "scale": t["scale"], "pts": t["pts"][np.arange(P) % t["P"]].copy(),
             "active_idx": None, "n_active": None, "state": t["state"]}
        if n_active is not None:
            order = np.argsort(synth.uniform(SEED, "mlp/%s/order" % name, (P,)))
            idx = np.full(P, -1, np.int32)
            idx[:n_active] = order[:n_active]
            c["active_idx"], c["n_active"] = idx, n_active
        return c
    B, n, scale, n_active, (z_ld, z_col0), (sdf_ld, sdf_col0) = SDF_VALUE_RAY_CASES[name] if name in SDF_VALUE_RAY_CASES else SDF_COLD_RAY_CASES[name]
    c = _ray_case(name, B, n, scale, n_active, "init")
    lo, hi = Z_GAP_FILL
    z_wide = (lo + (hi - lo) * synth.uniform(SEED, "mlp/%s/z_gap" % name, (B, z_ld))).astype(np.float32)
    z_wide[:, z_col0:z_col0 + n] = c["z"]
    c.update(form="rays", tile=None, z_wide=z_wide, z_ld=z_ld, z_col0=z_col0, sdf_ld=sdf_ld, sdf_col0=sdf_col0)
    del c["squeeze"]
    return c


def value_points_of(c):
    """The float32 points of every dense point id of a case of SDF_VALUE_CASES (ray form: o + d z, as fused_points_of)."""
    return c["pts"] if c["form"] == "pts" else fused_points_of(c)


def value_rows_of(c):
    """The dense point ids behind the rows of the saved planes: the listed ones in list order, or all."""
    return fused_rows_of(c)


# The tail hand-off (VdnSdfArgs.tail_row0 / tail_max_rows; csrc/k_sdf_fwd2.h MODE 1 against csrc/k_sdf_fwd1_split.h):
# (tail_row0, tail_max_rows, n_rows) - the tail idle (the list ends AT tail_row0), one row and 172 rows handed off, the second
# workgroup boundary, a list that ends beyond the window (the main kernel keeps every row). "dense": the first n_rows points of
# SDF_VALUE_TILE, P = n_rows; "list": 400 uniform points at scale 1 with a work list of n_rows rows, not ascending, whose
# count the kernels read on the device.
SDF_TAIL_SPLITS = ((128, 256, 128), (128, 256, 129), (128, 256, 300), (256, 256, 300), (128, 128, 300))
SDF_TAIL_LIST_P = 400


def sdf_tail_case(kind, n_rows):
    if kind == "dense":
        t = sdf_case(SDF_VALUE_TILE)
        return {"name": "tail-dense-n%d" % n_rows, "form": "pts", "tile": None, "P": n_rows, "scale": t["scale"], "pts": t["pts"][:n_rows].copy(),
                "active_idx": None, "n_active": None, "state": t["state"]}
    P = SDF_TAIL_LIST_P
    pts = (2.2 * synth.uniform(SEED, "mlp/tail-list/pts", (P, 3)) - 1.1).astype(np.float32)
    order = np.argsort(synth.uniform(SEED, "mlp/tail-list/order", (P,)))
    idx = np.full(P, -1, np.int32)
    idx[:n_rows] = order[:n_rows]
    return {"name": "tail-list-n%d" % n_rows, "form": "pts", "tile": None, "P": P, "scale": 1.0, "pts": pts, "active_idx": idx,
            "n_active": n_rows, "state": "init"}


def handed_off(tail_row0, tail_max_rows, n_rows):
    """Whether the rows from tail_row0 on are the tail launch's (include/vdn_render.h: VdnSdfArgs.tail_row0)."""
    return tail_max_rows > 0 and n_rows > tail_row0 and n_rows - tail_row0 <= tail_max_rows


# MODE 2 (vdn_shade_fused_bf16), name: (rays, T). One workgroup is one ray of 128 samples; T = 160 brings the background inputs
# and a background colour. Depths sorted in [0, 1.6] from origins within 0.7 of the centre: samples on both sides of the unit sphere.
SHADE_CASES = {"shade-B1-T128": (1, 128), "shade-B3-T160": (3, 160)}


def shade_case(name):
    B, T = SHADE_CASES[name]
    N = 128
    u = lambda tag, shape: synth.uniform(SEED, "mlp/%s/%s" % (name, tag), shape).astype(np.float32)
    z = np.sort(1.6 * u("z", (B, N)), axis=1).astype(np.float32)
    dists = np.concatenate([np.diff(z, axis=1), np.full((B, 1), 0.0125, np.float32)], 1).astype(np.float32)
    c = {"name": name, "B": B, "n_per_ray": N, "N": N, "T": T, "P": B * N, "scale": 1.0, "rays_o": (0.8 * u("rays_o", (B, 3)) - 0.4),
         "rays_d": _unit_dirs(name + "/rays_d", B), "z": z, "dists": dists, "variance": 0.3, "cos_anneal": 0.5,
         "active_idx": None, "n_active": None, "state": "heads", "squeeze": True,
         "bg_density": None, "bg_rgb": None, "bg_dists": None, "background_rgb": None}
    if T > N:
        c.update(bg_density=4.0 * u("bg_density", (B * T,)), bg_rgb=u("bg_rgb", (B * T, 3)), bg_dists=0.02 + 0.05 * u("bg_dists", (B, T)),
                 background_rgb=np.ones(3, np.float32))
    return c


# MODE 4 (vdn_shade_points_bf16), name: (P, weight state). Points uniform in [-1.1, 1.1]^3, the row counts of the SDF cases; once
# on the state whose sdf is constant: the gradient is exactly zero and the view direction must be zero, never NaN.
POINT_CASES = {"points-P1": (1, "heads"), "points-P33": (33, "heads"), "points-P129": (129, "heads"), "points-P300": (300, "heads"),
               "flat-P33": (33, "heads-flat")}


def point_case(name):
    P, state = POINT_CASES[name]
    pts = (2.2 * synth.uniform(SEED, "mlp/%s/pts" % name, (P, 3)) - 1.1).astype(np.float32)
    return {"name": name, "P": P, "scale": 1.0, "pts": pts, "active_idx": None, "n_active": None, "state": state, "squeeze": True}


# ---- the background network ---------------------------------------------------------------------------------------------------
# name: (P, n_active). Inverted-sphere points [x / r, 1 / r] with r in [1, 4] (renderer.py:112-115), unit view directions; row 0
# sits on the +x axis at r = 1 and looks along +x (exact zeros and ones).
NERF_CASES = {"nerf-P1": (1, None), "nerf-P33": (33, None), "nerf-P129": (129, None), "nerf-P300": (300, None),
              "nerf-worklist-P200-n77": (200, 77), "nerf-nodpt-P129": (129, None)}


def nerf_case(name):
    P, n_active = NERF_CASES[name]
    u = lambda tag, shape: synth.uniform(SEED, "mlp/%s/%s" % (name, tag), shape)
    n = lambda tag, shape: synth.normal(SEED, "mlp/%s/%s" % (name, tag), shape)
    d = n("x", (P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 1.0 + 3.0 * u("r", (P, 1))
    pts4 = np.concatenate([d, 1.0 / r], -1).astype(np.float32)
    dirs = n("dirs", (P, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    pts4[0], dirs[0] = (1.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    c = {"name": name, "P": P, "pts4": pts4, "dirs": dirs, "active_idx": None, "n_active": None,
         "state": "nodpt" if "nodpt" in name else "heads"}
    if n_active is not None:
        order = np.argsort(u("order", (P,)))
        idx = np.full(P, -1, np.int32)
        idx[:n_active] = order[:n_active]
        c["active_idx"], c["n_active"] = idx, n_active
    return c


def nerf_rows_of(c):
    sel = slice(None) if c["active_idx"] is None else c["active_idx"][:c["n_active"]]
    return c["pts4"][sel], c["dirs"][sel]


def nerf_upstream(c):
    """(g_density [P], g_rgb [P,3], g_feat [P,96] or None) ~ N(0, 1) of a background case; row 0 zero (but in the one-row case)."""
    n = lambda tag, shape: synth.normal(SEED, "mlp/%s/%s" % (c["name"], tag), shape).astype(np.float32)
    g = [n("g_density", (c["P"],)), n("g_rgb", (c["P"], 3)), None if c["state"] == "nodpt" else n("g_feat", (c["P"], 96))]
    for a in g:
        if a is not None and c["P"] > 1:
            a[0] = 0.0
    return g


# ---- the SDF backward ---------------------------------------------------------------------------------------------------------
# Upstream gradients of an SDF case: random, and each chain alone (g_feat = 0 with g_sdf = 0 leaves only the sweep's adjoint and its
# second-order term; g_normals = 0 leaves only the forward's adjoint: ub and EX exactly zero).
SDF_UPSTREAM = ("random", "g_feat=0", "g_normals=0")


def sdf_d_pts_prefill(c):
    """What d_pts [P,3] holds before a vdn_sdf_bwd_fbar_* launch with acc_pts = 1: ~ N(0, 1), finite, dense point order."""
    return synth.normal(SEED, "mlp/%s/d_pts_before" % c["name"], (c["P"], 3)).astype(np.float32)


def sdf_upstream(c, kind="random"):
    """(g_sdf [P], g_feat [P,256] bf16 values, g_normals [P,3]) ~ N(0, 1), dense point order."""
    n = lambda tag, shape: synth.normal(SEED, "mlp/%s/%s" % (c["name"], tag), shape).astype(np.float32)
    g_sdf, g_feat, g_n = n("g_sdf", (c["P"],)), n("g_feat", (c["P"], 256)), n("g_normals", (c["P"], 3))
    if kind == "g_feat=0":
        g_feat[:], g_sdf[:] = 0.0, 0.0
    elif kind == "g_normals=0":
        g_n[:] = 0.0
    return g_sdf, g_feat, g_n
