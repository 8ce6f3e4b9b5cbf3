"""The two-class foreground work list and the heads' prefix (DESIGN.md "Work lists", third consequence).

List kernel: vdn_foreground_active / vdn_train_prep with inner_radius 1.0 inside radius 1.2 write the ids with |p| < 1 first and
those with 1 <= |p| < 1.2 behind them, both ascending, by the compositor's own float32 norm; with the new fields zero the list is
the unpartitioned one. Step: the colour / VDN head on the first class only (TrainEngine._heads_inside) gives the scalars of the
whole-list arm bit for bit and its gradients up to the weight-gradient GEMM's summation order; nothing reads a head's output, save
or delta outside the evaluated prefix (NaN poison); rows that change class from step to step leave nothing stale behind.
tests/test_heads_inside_cpu.py holds the exactness claim itself to the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F12 = np.float32(1.2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _norms(o, d, mid):
    """|o + d z| as csrc/k_ray_rows.h sample_norm rounds it: float32, no contraction."""
    x = o[:, None, 0] + d[:, None, 0] * mid
    y = o[:, None, 1] + d[:, None, 1] * mid
    w = o[:, None, 2] + d[:, None, 2] * mid
    with np.errstate(invalid="ignore"):
        return np.sqrt(((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (w * w).astype(np.float32), dtype=np.float32)


def _inputs(kind, B, N, O=32):
    """rays and sorted inside depths z [B,N] whose section mid-points (z_i + (z_{i+1} - z_i) / 2) fall on both sides of both radii."""
    rng = np.random.default_rng(B * 1000 + N)
    d = rng.standard_normal((B, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if kind == "mixed":
        o = (rng.standard_normal((B, 3)) * 0.6).astype(np.float32)
        z = np.sort(rng.uniform(0.0, 3.0, (B, N)).astype(np.float32), axis=1)
        # ray 0: o = 0, d = e_x; the sections [0.875, 1.125] and [1.2f - 1/16, 1.2f + 1/16] have the mid-points 1.0 and float32(1.2)
        # exactly (every operation of the section is exact on these values), so |p| = 1.0 and 1.2f exactly at samples 1 and 3
        o[0], d[0] = 0.0, (1.0, 0.0, 0.0)
        z[0] = np.linspace(2.0, 3.0, N, dtype=np.float32)
        z[0, :5] = (0.25, 0.875, 1.125, F12 - np.float32(0.0625), F12 + np.float32(0.0625))
        if B > 1:
            z[B // 2, N // 3] = np.nan      # one NaN depth: its two sections have NaN mid-points, in neither class
    elif kind == "all_inner":
        o = (rng.standard_normal((B, 3)) * 0.05).astype(np.float32)
        z = np.sort(rng.uniform(0.0, 0.8, (B, N)).astype(np.float32), axis=1)
    else:                                   # none_inner: |p| >= 1.1 everywhere, many listed
        o = np.tile(np.asarray([[1.1, 0.0, 0.0]], np.float32), (B, 1))
        d = np.tile(np.asarray([[0.0, 1.0, 0.0]], np.float32), (B, 1))
        z = np.sort(rng.uniform(0.0, 0.6, (B, N)).astype(np.float32), axis=1)
    z_out = np.sort(rng.uniform(0.05, 0.95, (B, O)).astype(np.float32), axis=1)
    return o, d, z, z_out


def _train_prep(o, d, z, z_out, inner):
    """vdn_train_prep -> (mid_z [B,N] as the launch wrote it, idx, n_active, n_inner [2], ray_counts)."""
    from vdn_hip import lib
    B, N = z.shape
    T = N + z_out.shape[1]
    t = lambda a: torch.tensor(a).to(DEV).contiguous()
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)
    keep = dict(o=t(o), d=t(d), z=t(z), z_out=t(z_out), z_feed=f(B, T), dists=f(B, N), mid=f(B, N), bg_dists=f(B, T), bg_mid=f(B, T),
                fg_idx=i32(B * N), fg_n=i32(1), fg_cnt=i32(2 * B), fg_inner=i32(2), bg_idx=i32(B * T), bg_n=i32(1), bg_cnt=i32(B))
    tp = lib.VdnTrainPrepArgs()
    tp.rays_o, tp.rays_d, tp.z, tp.z_out, tp.z_feed = (keep[k].data_ptr() for k in ("o", "d", "z", "z_out", "z_feed"))
    tp.B, tp.N, tp.T, tp.z_ld, tp.sample_dist, tp.fg_radius = B, N, T, N, 2.0 / 64, 1.2
    tp.dists, tp.mid_z, tp.bg_dists, tp.bg_mid = (keep[k].data_ptr() for k in ("dists", "mid", "bg_dists", "bg_mid"))
    tp.fg_active_idx, tp.fg_n_active, tp.fg_ray_counts = (keep[k].data_ptr() for k in ("fg_idx", "fg_n", "fg_cnt"))
    tp.bg_active_idx, tp.bg_n_active, tp.bg_ray_counts = (keep[k].data_ptr() for k in ("bg_idx", "bg_n", "bg_cnt"))
    if inner:
        tp.fg_inner_radius, tp.fg_n_inner = inner, keep["fg_inner"].data_ptr()
    lib.call("vdn_train_prep", tp, _stream())
    torch.cuda.synchronize()
    return keep["mid"], keep["fg_idx"].cpu().numpy(), int(keep["fg_n"].item()), keep["fg_inner"].cpu().numpy(), keep["fg_cnt"].cpu().numpy()


def _fg_active(o, d, mid_dev, inner):
    from vdn_hip import lib
    B, N = mid_dev.shape
    to, td = torch.tensor(o).to(DEV), torch.tensor(d).to(DEV)
    idx = torch.full((B * N,), -7, dtype=torch.int32, device=DEV)
    n = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ni = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((2 * B,), -7, dtype=torch.int32, device=DEV)
    a = lib.VdnForegroundActiveArgs()
    a.rays_o, a.rays_d, a.mid_z, a.B, a.N, a.radius = to.data_ptr(), td.data_ptr(), mid_dev.data_ptr(), B, N, 1.2
    a.active_idx, a.n_active, a.ray_counts = idx.data_ptr(), n.data_ptr(), cnt.data_ptr()
    if inner:
        a.inner_radius, a.n_inner = inner, ni.data_ptr()
    lib.call("vdn_foreground_active", a, _stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), int(n.item()), ni.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("kind,B,N", [("mixed", 1, 128), ("mixed", 37, 128), ("mixed", 300, 130), ("all_inner", 37, 128), ("none_inner", 37, 128)])
def test_two_class_list_follows_the_compositors_norm(kind, B, N):
    o, d, z, z_out = _inputs(kind, B, N)
    mid_dev, idx_p, n_p, ni_p, cnt_p = _train_prep(o, d, z, z_out, 1.0)
    mid = mid_dev.cpu().numpy()
    pn = _norms(o, d, mid).reshape(-1)
    with np.errstate(invalid="ignore"):
        inner = np.flatnonzero(pn < np.float32(1.0)).astype(np.int32)
        shell = np.flatnonzero((pn < F12) & ~(pn < np.float32(1.0))).astype(np.int32)
        whole = np.flatnonzero(pn < F12).astype(np.int32)
    n0, n = len(inner), len(inner) + len(shell)
    # both entry points: ids and counts of the numpy restatement, both classes ascending, nothing behind the count
    idx_f, n_f, ni_f, cnt_f = _fg_active(o, d, mid_dev, 1.0)
    for idx, cnt_n, ni, cnt in ((idx_p, n_p, ni_p, cnt_p), (idx_f, n_f, ni_f, cnt_f)):
        assert cnt_n == n and ni[0] == n0 and ni[1] == min(n, (n0 + 127) // 128 * 128)
        assert np.array_equal(idx[:n0], inner) and np.array_equal(idx[n0:n], shell)
        assert (np.diff(idx[:n0]) > 0).all() and (np.diff(idx[n0:n]) > 0).all()
        assert np.array_equal(np.sort(idx[:n]), whole)                  # the union is the unpartitioned list
        assert (idx[n:] == -7).all()
        with np.errstate(invalid="ignore"):
            per_ray = lambda m: m.reshape(B, N).sum(1).astype(np.int32)
            assert np.array_equal(cnt[:B], per_ray(pn < np.float32(1.0))) and np.array_equal(cnt[B:], per_ray((pn < F12) & ~(pn < np.float32(1.0))))
    assert np.array_equal(idx_p, idx_f) and np.array_equal(ni_p, ni_f) and np.array_equal(cnt_p, cnt_f)     # the entry points agree bit for bit
    # the new fields zero: today's list, counters of the second class untouched
    for idx, cnt_n, ni, cnt in (_train_prep(o, d, z, z_out, 0.0)[1:], _fg_active(o, d, mid_dev, 0.0)):
        assert cnt_n == n and np.array_equal(idx[:n], whole) and (idx[n:] == -7).all()
        assert (ni == -7).all() and (cnt[B:] == -7).all()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(cnt[:B], (pn < F12).reshape(B, N).sum(1).astype(np.int32))
    if kind == "mixed":
        # ray 0 (o = 0, d = e_x): |p| = 1.0 exactly is listed but not inner; |p| = float32(1.2) exactly is not listed
        assert mid[0, 1] == np.float32(1.0) and mid[0, 3] == F12 and pn[1] == np.float32(1.0) and pn[3] == F12
        assert 1 in shell and 1 not in inner and 3 not in whole and 0 in inner
        assert 0 < n0 < n
        if B > 1:
            q = (B // 2) * N + N // 3
            assert np.isnan(pn[q]) and np.isnan(pn[q - 1]) and q not in idx_p[:n] and q - 1 not in idx_p[:n]
    elif kind == "all_inner":
        assert n0 == n == B * N
    else:
        assert n0 == 0 and n > B * N // 2


# ---- the training step ------------------------------------------------------------------------------------------------------

def _g(x):
    return torch.tensor(np.asarray(x, dtype=np.float32)).to(DEV)


def _step_inputs(seed, B, it=0, img=4):
    from vdn_train import synth
    cams = synth.make_cameras(seed)
    o, d = synth.random_pixel_batch(seed, it, img, B, cams=cams)            # full frame: listed samples on both sides of |p| = 1
    near, far = synth.near_far_from_sphere(o, d)
    t1, t2 = synth.jitter(seed, it, B)
    return [_g(x) for x in (o, d, near, far)], _g(t1), _g(t2)


def _trainer(st, precision, B, heads_inside):
    from vdn_train import factory
    from vdn_train.trainer import Trainer
    tr = Trainer(factory.build_renderer(wdepth=True, device=DEV, states=st, precision=precision), B, DEV,
                 conf=dict(extract_depth=True, depth_start_iter=-1))
    tr.iter_step = 10
    tr.engine._heads_inside = heads_inside
    return tr


def _heads_planes(eng):
    """(dense per-sample outputs, compact-row planes [layers, rows * ld] flat per layer with their ld, mask planes) of both heads."""
    w = eng.w
    dense = [w["col_out"], w["vdn_out"]]
    planes = [(w[k].view(w[k].shape[0] if w[k].dim() == 3 else 1, -1), w[k].shape[-1]) for k in
              ("col_h", "col_small", "col_dh", "col_dout", "vdn_h", "vdn_small", "vdn_dh", "vdn_dout")]
    masks = [w[k] for k in ("col_mask", "vdn_mask") if w.get(k) is not None]
    return dense, planes, masks


@pytest.mark.parametrize("precision,fused", [("fp32", False), ("bf16", False), ("bf16", True)], ids=["fp32", "bf16", "bf16_color_fused"])
def test_heads_on_the_inner_class_do_not_change_the_step(monkeypatch, precision, fused):
    """One step of the scene of test_trainer_work_lists_do_not_change_the_step with the heads on the first class against the heads
    on the whole list: scalars bit for bit, gradients within that test's bound (the arms differ by the summation order of the heads'
    weight-gradient entries); and a third run whose heads' outputs, saves, masks and deltas outside the evaluated prefix are NaN
    (0xFF) before the step gives the first run's scalars and gradients bit for bit."""
    from vdn_train import synth
    monkeypatch.setenv("VDN_TRAIN_COLOR_FUSED", "1" if fused else "0")
    B, seed = 256, 53
    st = synth.make_all_states(seed, wdepth=True)
    rays, t1, t2 = _step_inputs(seed, B)
    rgb, gtf = _g(synth.uniform(seed, "wl/rgb", (B, 3))), _g(synth.uniform(seed, "wl/f", (B, 96)))
    res = {}
    for arm in ("on", "off", "poisoned"):
        tr = _trainer(st, precision, B, arm != "off")
        eng = tr.engine
        if arm == "poisoned":
            n, n_in, n_heads, idx = res["on"][2:]
            assert n_heads % 128 == 0
            dense, planes, masks = _heads_planes(eng)
            off = torch.ones(eng.P, dtype=torch.bool, device=DEV)
            off[idx[:n_heads].long()] = False
            for t in dense:
                t[off] = float("nan")
            for p, ld in planes:                    # rows >= n_heads (a multiple of 32) of a row-major or tile-blocked plane: the flat tail
                p[:, n_heads * ld:] = float("nan")
            for m in masks:
                m[:, n_heads * 32:] = 0xFF
        sc = tr.train_step(*rays, rgb, gt_feats=gtf, t_rand=t1, t_rand_out=t2).cpu().numpy().copy()
        assert bool(eng._color_fused) == fused
        cnt = eng._fg_cnt.tolist()
        res[arm] = (sc, [x.clone() for x in eng.param_grads()], cnt[0], cnt[1], cnt[2], eng.w["fg_active"][0].clone())
    sc1, g1, n, n_in, n_heads, idx1 = res["on"]
    sc0, g0, n_off, n_in_off, n_heads_off, idx0 = res["off"]
    print("%s fused=%s: listed %d, inner %d, heads' rows %d of P = %d" % (precision, fused, n, n_in, n_heads, B * 128))
    assert 0 < n_in < n and n_heads == min(n, (n_in + 127) // 128 * 128)
    assert n_off == n and n_in_off == n and n_heads_off == n
    assert torch.equal(torch.sort(idx1[:n])[0], idx0[:n])
    assert np.isfinite(sc1).all() and np.array_equal(sc1, sc0)
    for a, b in zip(g1, g0):
        assert torch.isfinite(a).all()
        assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-12
    scp, gp = res["poisoned"][:2]
    assert res["poisoned"][2:5] == (n, n_in, n_heads)
    assert np.isfinite(scp).all() and np.array_equal(scp, sc1)
    for a, b in zip(gp, g1):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_rows_that_change_class_between_steps():
    """8 steps over different images (a compact row that was inner becomes shell and back): the parameters stay with the whole-list
    arm within the bound tests/test_gpu_train_parity.py uses for two arms that differ by rounding."""
    from vdn_train import synth
    B, seed = 256, 53
    st = synth.make_all_states(seed, wdepth=True)
    trs = [_trainer(st, "bf16", B, on) for on in (True, False)]
    gtf = _g(synth.uniform(seed, "wl/f", (B, 96)))
    fractions = []
    for it in range(8):
        rays, t1, t2 = _step_inputs(seed, B, it, (7 * it) % 40)
        rgb = _g(synth.target_colors(rays[0].cpu().numpy(), rays[1].cpu().numpy(), 0.5))
        for tr in trs:
            tr.train_step(*rays, rgb, gt_feats=gtf, t_rand=t1, t_rand_out=t2)
        cnt = trs[0].engine._fg_cnt.tolist()
        fractions.append(cnt[1] / max(cnt[0], 1))
        assert 0 < cnt[1] < cnt[0]
    assert max(fractions) - min(fractions) > 0.0            # the class boundary moved
    pa, pb = trs[0].param_flat, trs[1].param_flat
    assert torch.isfinite(pa).all() and (pa - pb).norm().item() < 1e-3 * pb.norm().item()


def test_without_a_background_pass_the_heads_keep_every_sample():
    from vdn_train import synth, factory
    from vdn_train.trainer import Trainer
    B, seed = 96, 59
    st = synth.make_all_states(seed, wdepth=False)
    rays, t1, _ = _step_inputs(seed, B, 0, 1)
    tr = Trainer(factory.build_renderer(device=DEV, states=st, n_outside=0), B, DEV)
    assert tr.engine._heads_inside
    tr.iter_step = 10
    sc = tr.train_step(*rays, _g(synth.uniform(seed, "nb/rgb", (B, 3))), t_rand=t1).cpu().numpy()
    assert np.isfinite(sc).all() and tr.engine._fg_cnt.tolist()[:3] == [B * 128] * 3


def test_ray_gradients_keep_the_heads_on_the_whole_list():
    """With ray gradients the heads stay on the whole list (TrainEngine._inner_radius): d loss / d rays_o, rays_d of a 96-ray step equal
    the attribute-off arm within the fp32 bound of tests/test_gpu_raygrads.py (1e-3 of the largest entry)."""
    from vdn_train import synth, factory
    from vdn_hip.train import TrainEngine
    seed, B = 4, 96
    rend = factory.build_renderer(device=DEV, states=synth.make_all_states(seed), precision="fp32")
    (o, d, near, far), t1, t2 = _step_inputs(seed, B, 0, 1)
    gen = torch.Generator(device="cpu").manual_seed(0)
    g_color, g_eik = _g(torch.randn(B, 3, generator=gen) * 1e-2), _g([0.1])
    res = {}
    for on in (True, False):
        eng = TrainEngine(rend, B, DEV)
        eng._heads_inside = on
        with torch.no_grad():
            z, z_out = rend._sample(o, d, near.reshape(B), far.reshape(B), rend.perturb, t1.view(B, 1), t2, None)
        w = eng.forward(o, d, z.contiguous(), z_out, torch.ones(3, device=DEV), 0.5, skip_far=True, ray_grads=True, ray_grads_compact=True)
        eng.backward(g_color, None, None, g_eik)
        cnt = eng._fg_cnt.tolist()
        assert eng._fg_compact and 0 < cnt[0] < eng.P and cnt[1] == cnt[2] == cnt[0]
        res[on] = {k: w[k].clone() for k in ("d_rays_o", "d_rays_d")}
    for k in ("d_rays_o", "d_rays_d"):
        a, b = res[True][k], res[False][k]
        assert torch.isfinite(a).all() and b.abs().max().item() > 0
        assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item() + 1e-12, k


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_row_cap_of_a_gemm_launch_equals_p_dev_on_the_capped_entries(precision):
    """vdn_dw_gemm_rows_*: descriptors [1, 3) of a 4-entry launch capped at 1000 + 13 rows give the slabs and column sums of the
    uncapped launch whose descriptors 1 and 2 carry that count as P_dev, bit for bit (same split ranges, same order); the entries
    outside the range keep their own row counts (entry 3 its larger P_dev)."""
    from vdn_hip import layout, lib
    sfx = "_bf16" if precision == "bf16" else "_f32"
    P, cap_rows, own_rows = 2048 + 77, 1000 + 13, 1500
    entries = [(256, 256, True, 2), (256, 64, False, 2), (96, 128, False, 3), (128, 256, False, 2)]
    gen = torch.Generator(device="cpu").manual_seed(5)
    dt = torch.bfloat16 if precision == "bf16" else torch.float32

    def plane(ld):
        x = torch.randn(P, ld, generator=gen)
        if precision == "fp32":
            return x.to(DEV).contiguous()
        full = torch.zeros(layout.rows(P, "bf16"), ld)
        full[:P] = x
        return layout.to_pt32(full.to(DEV).to(dt))
    ints = {k: torch.tensor([v], dtype=torch.int32, device=DEV) for k, v in (("cap", cap_rows), ("own", own_rows))}
    planes = [[(plane(M), plane(N)) for _ in range(2 if two else 1)] for M, N, two, _ in entries]
    outs = {}
    for arm in ("cap", "p_dev"):
        dw = np.zeros(len(entries), dtype=lib.struct_dtype("VdnDwDesc"))
        slabs, wg = [], 0
        for i, (M, N, two, splits) in enumerate(entries):
            d = dw[i]
            for s, (a, b) in enumerate(planes[i]):
                d["A%d" % (s + 1)], d["lda%d" % (s + 1)], d["B%d" % (s + 1)], d["ldb%d" % (s + 1)] = a.data_ptr(), M, b.data_ptr(), N
            slab = torch.full((splits, M, N), float("nan"), device=DEV)
            colsum = torch.full((splits, M), float("nan"), device=DEV)
            slabs.append((slab, colsum))
            d["P"], d["m_tiles"], d["n_tiles"], d["splits"], d["wg_begin"] = P, M // 32, N // 32, splits, wg
            d["slab"], d["colsum"] = slab.data_ptr(), colsum.data_ptr()
            if i == 3:
                d["P_dev"] = ints["own"].data_ptr()
            elif arm == "p_dev" and i in (1, 2):
                d["P_dev"] = ints["cap"].data_ptr()
            wg += lib.call_value("vdn_dw_entry_wgs" + sfx, M // 32, N // 32, splits)
        table = torch.from_numpy(dw.view(np.uint8)).to(DEV)
        if arm == "cap":
            lib.call("vdn_dw_gemm_rows" + sfx, lib.ptr(table), len(entries), wg, lib.ptr(ints["cap"]), 1, 3, _stream())
        else:
            lib.call("vdn_dw_gemm" + sfx, lib.ptr(table), len(entries), wg, _stream())
        torch.cuda.synchronize()
        outs[arm] = slabs
    for i, ((sa, ca), (sb, cb)) in enumerate(zip(outs["cap"], outs["p_dev"])):
        assert torch.isfinite(sa).all() and torch.isfinite(ca).all(), i
        assert torch.equal(sa, sb) and torch.equal(ca, cb), i
    # and the cap does bite: entry 1 against the product over its first cap_rows rows
    if precision == "fp32":
        a, b = planes[1][0]
        want = a[:cap_rows].double().T @ b[:cap_rows].double()
        got = outs["cap"][1][0].double().sum(0)
        assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
