"""The hierarchical sampler's launches as operators, through the C ABI (include/vdn_render.h), one launch per case, against the
float64 model of oracle/sampler_ops.py on the constructed inputs of oracle/sampler_cases.py (whose coverage, conditioning and
bite tests/test_sampler_model_cpu.py proves without a GPU).

Buffers: every output is pre-filled with NaN between two NaN guard bands (test_gpu_ray_ops.Bufs); every input row is NaN beyond
its M valid entries, so a kernel that reads there shows. After the launch every element the header promises is finite and
everything else is still NaN.

vdn_upsample_round against the float64 model (sampler_ops.judge, the comparator the CPU test proves): U = 1e-6 max(1, max|z|);
tight cases: every entry |z - z64| <= max(U, 3 F_z), none excluded, F_z recomputed here from the float32 CPU model (three times,
as in test_gpu_ray_ops.py: the kernel's operation order differs from torch's and one extra rounding per step may land the other
way); ill-conditioned cases: every entry's CDF residual <= 3 F_cdf (+ 1e-5 in the flat branch), the new depths ascending and
within [z[0], z[M-1]]. A branch-sensitive entry may match one of its candidates instead; they are counted and printed, with the
worst error per case in units of its bound (pytest -rA).

The fused launches promise bit-identity with the launches they replace, asserted exactly: vdn_merge_upsample = vdn_merge_sorted
+ vdn_upsample_round; vdn_sdf_upsample_bf16 / vdn_sdf_merge_upsample_bf16 = vdn_sdf_mlp_fwd_bf16(mode 0) + those; vdn_train_prep
with new_z / M_old = vdn_merge_sorted + vdn_train_prep without; and -10 with nothing written for what they decline. Their new
depths are also held to the float64 model fed the kernel's OWN SDF values, so the comparison does not depend on the bf16 error of
the SDF network (tests/test_gpu_bf16.py's subject). Last, the chain: the launches NeuSRenderer._sample makes, replayed unfused on
buffers the test owns, round by round against the model, and bit for bit against what _sample() returns.
"""
import numpy as np
import pytest
import torch

from oracle import sampler_cases as sc
from oracle import sampler_ops as so
from test_gpu_ray_ops import Bufs, _call, _status, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _padded(a, ld):
    """[B,n] -> [B,ld] with NaN behind the n valid columns."""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


def _row_buffer(b, name, rows, ld):
    """An in-place row buffer [B,ld] between guard bands: `rows` in its first columns, NaN behind. -> device pointer."""
    ptr = b.out(name, rows.shape[0], ld)
    b[name][:, :rows.shape[1]] = torch.as_tensor(np.ascontiguousarray(rows)).to(DEV)
    return ptr


def _upsample_args(b, B, M, ld, n_imp, inv_s, u, z=None, sdf=None, rays=None, weights=None, w_ld=0, out="new_z"):
    from vdn_hip import lib
    a = lib.VdnUpsampleArgs()
    if z is not None:
        a.z = b.inp(_padded(z, ld))
    if weights is not None:
        a.weights, a.w_ld = b.inp(_padded(weights, w_ld)), w_ld
    else:
        a.rays_o, a.rays_d = b.inp(rays[0]), b.inp(rays[1])
        if sdf is not None:
            a.sdf = b.inp(_padded(sdf, ld))
    a.u, a.new_z = b.inp(u), b.out(out, B, n_imp)
    a.inv_s, a.B, a.M, a.ld, a.n_imp = float(inv_s), B, M, ld, n_imp
    return a


def _model(cls, rays, z, sdf, u, inv_s, weights=None, exact_knots=False):
    """(case for judge, float64 stages, float32 stages) on the rows a launch was fed (numpy float32)."""
    case = {"cls": cls, "exact_knots": exact_knots}
    st = []
    for dt in (torch.float64, torch.float32):
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dt)
        st.append(so.upsample_stages(t(rays[0]) if rays else None, t(rays[1]) if rays else None, t(z), t(sdf), t(u), float(inv_s), t(weights)))
    return case, st[0], st[1]


def _hold(label, model, got, rows):
    case, s64, s32 = model
    j = so.judge(case, s64, s32, torch.as_tensor(got))
    rows.append("%-34s %-5s worst %.3f units of its bound (depth bound %.2e, F_z %.2e, F_cdf %.2e); branch-sensitive %d of %d, %d matched by candidate"
                % (label, case["cls"], j["worst"], j["bound_z"], j["F_z"], j["F_cdf"], j["n_sensitive"], got.size, j["n_by_candidate"]))
    print(rows[-1])
    assert j["ok"], "%s: %s" % (label, j["why"])
    return j


# ---- vdn_upsample_round -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.upsample_case_names())
def test_upsample_round_vs_float64_model(name):
    c = sc.upsample_case(name)
    B, M, n = c["B"], c["M"], c["n_imp"]
    b = Bufs()
    a = _upsample_args(b, B, M, c["ld"], n, c["inv_s"], c["u"], z=c["z"], sdf=c["sdf"], rays=(c["rays_o"], c["rays_d"]),
                       weights=c["weights"], w_ld=c["w_ld"])
    _call("vdn_upsample_round", a, _stream())
    b.check()
    model = (c, so.stages_of(c, torch.float64), so.stages_of(c, torch.float32))
    j = _hold(name, model, b.np("new_z"), [])
    if c["cls"] == "tight":
        assert j["n_sensitive"] == 0            # (the CPU test's condition, on the floors as the host running this test computes them)


@pytest.mark.parametrize("name", ["clean-B77-M64-n16", "noisy-B5-M112-n16", "graze-B77-M112-n16"])
def test_the_comparator_rejects_the_kernel_on_the_neighbouring_rounds_inv_s(name):
    """The wiring from the launch to the comparator: the same launch handed 2 x inv_s, judged against the model of the case's own
    inv_s, is rejected (what tests/test_sampler_model_cpu.py proves of the float32 model, here of the kernel's output)."""
    c = sc.upsample_case(name)
    b = Bufs()
    a = _upsample_args(b, c["B"], c["M"], c["ld"], c["n_imp"], 2.0 * c["inv_s"], c["u"], z=c["z"], sdf=c["sdf"], rays=(c["rays_o"], c["rays_d"]))
    _call("vdn_upsample_round", a, _stream())
    b.check()
    j = so.judge(c, so.stages_of(c, torch.float64), so.stages_of(c, torch.float32), torch.as_tensor(b.np("new_z")))
    assert not j["ok"] and j["worst"] > 10.0, j


# ---- vdn_merge_sorted -------------------------------------------------------------------------------------------------------

def _merge_args(b, B, M, K, ld, ld_out, z, new_z, sdf=None, new_sdf=None, in_place=False, tag=""):
    from vdn_hip import lib
    m = lib.VdnMergeArgs()
    if in_place:
        assert ld == ld_out
        m.z = m.z_out = _row_buffer(b, tag + "z", z, ld)
        if sdf is not None:
            m.sdf = m.sdf_out = _row_buffer(b, tag + "sdf", sdf, ld)
    else:
        m.z, m.z_out = b.inp(_padded(z, ld)), b.out(tag + "z", B, ld_out)
        if sdf is not None:
            m.sdf, m.sdf_out = b.inp(_padded(sdf, ld)), b.out(tag + "sdf", B, ld_out)
    m.new_z = b.inp(new_z)
    if sdf is not None:
        m.new_sdf = b.inp(new_sdf)
    m.B, m.M, m.K, m.ld, m.ld_out = B, M, K, ld, ld_out
    return m


def _check_rows(b, name, n):
    """The first n columns finite, the rest of the row still NaN, the guard bands untouched."""
    b.check(written=())
    v = b[name]
    assert torch.isfinite(v[:, :n]).all() and torch.isnan(v[:, n:]).all(), "%s: columns written beyond %d, or not up to it" % (name, n)


@pytest.mark.parametrize("name", list(sc.MERGE_CASES))
def test_merge_sorted_equals_the_stable_sort(name):
    c = sc.merge_case(name)
    B, M, K = c["B"], c["M"], c["K"]
    b = Bufs()
    m = _merge_args(b, B, M, K, c["ld"], c["ld_out"], c["z"], c["new_z"], c["sdf"], c["new_sdf"], c["in_place"])
    _call("vdn_merge_sorted", m, _stream())
    t = lambda k: None if c[k] is None else torch.as_tensor(c[k])
    want_z, want_s = so.merge(t("z"), t("sdf"), t("new_z"), t("new_sdf"))
    _check_rows(b, "z", M + K)
    assert torch.equal(b["z"][:, :M + K].cpu(), want_z)
    if c["sdf"] is not None:
        _check_rows(b, "sdf", M + K)
        assert torch.equal(b["sdf"][:, :M + K].cpu(), want_s)


# ---- vdn_merge_upsample -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,M,K,n_imp", sc.MERGE_UPSAMPLE_SHAPES)
def test_merge_upsample_equals_the_two_launches_and_the_model(B, M, K, n_imp):
    c = sc.merge_upsample_case(B, M, K, n_imp)
    ld = sc.LD_FIXED if M + K <= sc.LD_FIXED else 256          # (in place with ld = ld_out = 160; the rows of M = 240 need 256)
    rays = (c["rays_o"], c["rays_d"])
    # the two launches, in place
    two = Bufs()
    m = _merge_args(two, B, M, K, ld, ld, c["z"], c["new_z"], c["sdf"], c["new_sdf"], True)
    _call("vdn_merge_sorted", m, _stream())
    u = _upsample_args(two, B, M + K, ld, n_imp, c["inv_s"], c["u"], rays=rays)
    u.z, u.sdf = m.z_out, m.sdf_out
    _call("vdn_upsample_round", u, _stream())
    _check_rows(two, "z", M + K)
    _check_rows(two, "sdf", M + K)
    # the one launch; the up-sample args' z / sdf / ld are ignored (NULL, 0 here)
    one = Bufs()
    m1 = _merge_args(one, B, M, K, ld, ld, c["z"], c["new_z"], c["sdf"], c["new_sdf"], True)
    u1 = _upsample_args(one, B, M + K, 0, n_imp, c["inv_s"], c["u"], rays=rays)
    _call("vdn_merge_upsample", m1, u1, _stream())
    _check_rows(one, "z", M + K)
    _check_rows(one, "sdf", M + K)
    one.check(written=("new_z",))
    for k in ("z", "sdf", "new_z"):
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k          # (bit for bit, the NaN tails included)
    if K == n_imp:
        # as render() calls it: the new depths of the next round are written over those of this one
        al = Bufs()
        ma = _merge_args(al, B, M, K, ld, ld, c["z"], c["new_z"], c["sdf"], c["new_sdf"], True)
        ua = _upsample_args(al, B, M + K, 0, n_imp, c["inv_s"], c["u"], rays=rays)
        shared = torch.as_tensor(c["new_z"]).to(DEV).contiguous()
        ma.new_z = ua.new_z = shared.data_ptr()
        _call("vdn_merge_upsample", ma, ua, _stream())
        al.check(written=())
        assert torch.equal(shared, one["new_z"]) and torch.equal(al["z"].view(torch.int32), one["z"].view(torch.int32))
    want_z, want_s = so.merge(*(torch.as_tensor(c[k]) for k in ("z", "sdf", "new_z", "new_sdf")))
    assert torch.equal(one["z"][:, :M + K].cpu(), want_z) and torch.equal(one["sdf"][:, :M + K].cpu(), want_s)
    _hold(c["name"], _model("tight", rays, want_z.numpy(), want_s.numpy(), c["u"], c["inv_s"]), one.np("new_z"), [])


# ---- vdn_train_prep with the last round's merge ------------------------------------------------------------------------------

def _train_prep(c, with_new):
    """vdn_train_prep on a case; with_new False: the old row has been completed by vdn_merge_sorted beforehand."""
    from vdn_hip import lib
    B, N, M_old, ld, O = c["B"], c["N"], c["M_old"], c["z_ld"], c["O"]
    T = N + O
    b = Bufs()
    tp = lib.VdnTrainPrepArgs()
    tp.rays_o, tp.rays_d, tp.z_out = b.inp(c["rays_o"]), b.inp(c["rays_d"]), b.inp(c["z_out"])
    tp.z = _row_buffer(b, "z", c["z"], ld)
    if with_new:
        tp.new_z, tp.M_old = b.inp(c["new_z"]), M_old
    else:
        m = lib.VdnMergeArgs()
        m.z = m.z_out = tp.z
        m.new_z = b.inp(c["new_z"])
        m.B, m.M, m.K, m.ld, m.ld_out = B, M_old, N - M_old, ld, ld
        _call("vdn_merge_sorted", m, _stream())
    tp.B, tp.N, tp.T, tp.z_ld, tp.sample_dist, tp.fg_radius = B, N, T, ld, 2.0 / 64, 1.2
    tp.z_feed, tp.dists, tp.mid_z = b.out("z_feed", B, T), b.out("dists", B, N), b.out("mid_z", B, N)
    tp.bg_dists, tp.bg_mid = b.out("bg_dists", B, T), b.out("bg_mid", B, T)
    ints = {k: torch.full((n,), -7, dtype=torch.int32, device=DEV) for k, n in
            (("fg_idx", B * N), ("fg_n", 1), ("fg_cnt", B), ("bg_idx", B * T), ("bg_n", 1), ("bg_cnt", B))}
    tp.fg_active_idx, tp.fg_n_active, tp.fg_ray_counts = (ints[k].data_ptr() for k in ("fg_idx", "fg_n", "fg_cnt"))
    tp.bg_active_idx, tp.bg_n_active, tp.bg_ray_counts = (ints[k].data_ptr() for k in ("bg_idx", "bg_n", "bg_cnt"))
    _call("vdn_train_prep", tp, _stream())
    _check_rows(b, "z", N)
    b.check(written=("z_feed", "dists", "mid_z", "bg_dists", "bg_mid"))
    return b, ints


@pytest.mark.parametrize("B,N,M_old,z_ld", sc.TRAIN_PREP_SHAPES)
def test_train_prep_with_the_last_merge_equals_merge_then_train_prep(B, N, M_old, z_ld):
    c = sc.train_prep_case(B, N, M_old, z_ld)
    got, gi = _train_prep(c, True)
    ref, ri = _train_prep(c, False)
    want_z, _ = so.merge(torch.as_tensor(c["z"]), None, torch.as_tensor(c["new_z"]), None)
    assert torch.equal(ref["z"][:, :N].cpu(), want_z)
    for k in got.outs:
        assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), k
    for k in ("fg", "bg"):
        n = int(ri[k + "_n"].item())
        assert int(gi[k + "_n"].item()) == n and 0 < n <= ri[k + "_idx"].numel(), k
        assert torch.equal(gi[k + "_idx"][:n], ri[k + "_idx"][:n]) and torch.equal(gi[k + "_cnt"], ri[k + "_cnt"]), k
        assert (gi[k + "_idx"][n:] == -7).all(), k


# ---- the bf16 launches that evaluate the SDF themselves ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def renderers():
    from vdn_train import synth, factory
    st = synth.make_all_states(5)
    return {p: factory.build_renderer(device=torch.device(DEV), states=st, precision=p) for p in ("fp32", "bf16")}


def _sdf_args(net, b, rays, z_ptr, z_ld, n_per_ray, B, sdf_ptr, sdf_ld):
    from vdn_hip import lib
    img = net._images()
    a = lib.VdnSdfArgs()
    a.rays_o, a.rays_d, a.z, a.n_per_ray, a.z_ld = b.inp(rays[0]), b.inp(rays[1]), z_ptr, n_per_ray, z_ld
    a.P, a.scale, a.sdf, a.sdf_ld = B * n_per_ray, float(net.scale), sdf_ptr, sdf_ld
    a.w8row = img.weff_view("lin8").data_ptr()
    a.blob = img.blobs["sdf"].data_ptr()
    return a


def _coarse_rows(near, far, n=64):
    lin = torch.linspace(0.0, 1.0, n).numpy()
    return np.ascontiguousarray((near[:, None] + (far - near)[:, None] * lin[None, :]).astype(np.float32))


@pytest.mark.parametrize("B,ld", [(1, 64), (2, 128), (3, 64), (77, 128)])
def test_fused_bf16_rounds_equal_their_launches_and_the_model(renderers, B, ld):
    """vdn_sdf_upsample_bf16 on the coarse rows, then vdn_sdf_merge_upsample_bf16 on its result."""
    net = renderers["bf16"].sdf_network
    o, d, near, far = sc.network_rays(B)
    rays = (o, d)
    z64 = _coarse_rows(near, far)
    u16 = torch.linspace(0.5 / 16, 1.0 - 0.5 / 16, 16).numpy()
    rows = []
    with torch.no_grad():
        # -- the first pass + round 0: z / sdf rows of leading dimension ld
        f = Bufs()
        zin = f.inp(_padded(z64, ld))
        a = _sdf_args(net, f, rays, zin, ld, 64, B, f.out("sdf", B, ld), ld)
        up = _upsample_args(f, B, 64, 0, 16, 64.0, u16, rays=rays)
        _call("vdn_sdf_upsample_bf16", a, up, _stream())
        _check_rows(f, "sdf", 64)
        f.check(written=("new_z",))
        s = Bufs()                                       # the SDF pass alone, and the round alone on its values
        sa = _sdf_args(net, s, rays, zin, ld, 64, B, s.out("sdf", B, ld), ld)
        _call("vdn_sdf_mlp_fwd_bf16", 0, sa, _stream())
        _check_rows(s, "sdf", 64)
        assert torch.equal(f["sdf"][:, :64], s["sdf"][:, :64])
        sdf64 = f.np("sdf")[:, :64].astype(np.float32)
        r = Bufs()
        ra = _upsample_args(r, B, 64, 64, 16, 64.0, u16, z=z64, sdf=sdf64, rays=rays)
        _call("vdn_upsample_round", ra, _stream())
        r.check()
        assert torch.equal(f["new_z"], r["new_z"])
        _hold("sdf_upsample B%d ld%d" % (B, ld), _model("tight", rays, z64, sdf64, u16, 64.0), f.np("new_z"), rows)
        new_z = f.np("new_z").astype(np.float32)

        # -- round 1 in one launch: SDF of the 16 new samples, merge (in place, ld 128), up-sample at inv_s = 128
        def round_buffers():
            g = Bufs()
            m = _merge_args(g, B, 64, 16, 128, 128, z64, new_z, sdf64, np.zeros((B, 16), np.float32), True)
            m.new_sdf = g.out("new_sdf", B, 16)
            return g, m
        g, m = round_buffers()
        a2 = _sdf_args(net, g, rays, m.new_z, 16, 16, B, m.new_sdf, 16)
        up2 = _upsample_args(g, B, 80, 0, 16, 128.0, u16, rays=rays)
        _call("vdn_sdf_merge_upsample_bf16", a2, m, up2, _stream())
        _check_rows(g, "z", 80)
        _check_rows(g, "sdf", 80)
        g.check(written=("new_sdf", "new_z"))
        h, mh = round_buffers()                          # the launches it replaces
        ah = _sdf_args(net, h, rays, mh.new_z, 16, 16, B, mh.new_sdf, 16)
        _call("vdn_sdf_mlp_fwd_bf16", 0, ah, _stream())
        uh = _upsample_args(h, B, 80, 0, 16, 128.0, u16, rays=rays)
        _call("vdn_merge_upsample", mh, uh, _stream())
        for k in ("new_sdf", "z", "sdf", "new_z"):
            assert torch.equal(g[k].view(torch.int32), h[k].view(torch.int32)), k
        want_z, want_s = so.merge(torch.as_tensor(z64), torch.as_tensor(sdf64), torch.as_tensor(new_z), g["new_sdf"].cpu())
        assert torch.equal(g["z"][:, :80].cpu(), want_z) and torch.equal(g["sdf"][:, :80].cpu(), want_s)
        _hold("sdf_merge_upsample B%d" % B, _model("tight", rays, want_z.numpy(), want_s.numpy(), u16, 128.0), g.np("new_z"), rows)

        # -- what they decline: -10, nothing written
        pts = torch.zeros(B * 64, 3, device=DEV)
        idx = torch.zeros(B * 64, dtype=torch.int32, device=DEV)

        def declined(fn, build, change):
            q = Bufs()
            args = build(q)
            change(*args)
            assert _status(fn, *args, _stream()) == -10, fn
            q.check(unwritten=tuple(q.outs))

        def first(q):
            return (_sdf_args(net, q, rays, q.inp(_padded(z64, ld)), ld, 64, B, q.out("sdf", B, ld), ld), _upsample_args(q, B, 64, 0, 16, 64.0, u16, rays=rays))

        def first_63(a, up):
            a.n_per_ray, a.P, up.M = 63, B * 63, 63
        declined("vdn_sdf_upsample_bf16", first, first_63)
        declined("vdn_sdf_upsample_bf16", first, lambda a, up: setattr(a, "pts", pts.data_ptr()))
        declined("vdn_sdf_upsample_bf16", first, lambda a, up: setattr(a, "active_idx", idx.data_ptr()))

        def second(q):
            m = lib_merge(q)
            return (_sdf_args(net, q, rays, m.new_z, 16, 16, B, m.new_sdf, 16), m, _upsample_args(q, B, 80, 0, 16, 128.0, u16, rays=rays))

        def lib_merge(q):
            m = _merge_args(q, B, 64, 16, 128, 128, z64, new_z, sdf64, np.zeros((B, 16), np.float32), False)
            m.new_sdf = q.out("new_sdf", B, 16)
            return m

        def k15(a, m, up):
            m.K, up.M = 15, 79

        def n64(a, m, up):
            a.n_per_ray = 64
        declined("vdn_sdf_merge_upsample_bf16", second, k15)
        declined("vdn_sdf_merge_upsample_bf16", second, n64)
        declined("vdn_sdf_merge_upsample_bf16", second, lambda a, m, up: setattr(a, "pts", pts.data_ptr()))
        declined("vdn_sdf_merge_upsample_bf16", second, lambda a, m, up: setattr(a, "active_idx", idx.data_ptr()))


# ---- the chain ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 77])
@pytest.mark.parametrize("defer", [False, True], ids=["merged", "deferred"])
@pytest.mark.parametrize("fuse", ["0", "1"], ids=["two_launches", "fused"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_chain_round_by_round(renderers, monkeypatch, precision, fuse, defer, B):
    from vdn_hip import lib
    monkeypatch.setenv("VDN_FUSE_SDF_ROUNDS", fuse)
    rend = renderers[precision]
    net = rend.sdf_network
    S, I, O, steps = rend.n_samples, rend.n_importance, rend.n_outside, rend.up_sample_steps
    assert (S, I, O, steps) == (64, 64, 32, 4)
    N, n_imp = S + I, I // steps
    o, d, near, far = sc.network_rays(B, "chain")
    rays = (o, d)
    dv = lambda a: torch.as_tensor(a).to(DEV).contiguous()
    to, td, tn, tf = dv(o), dv(d), dv(near), dv(far)
    consts = rend._consts(torch.device(DEV))
    u = consts["u"].cpu().numpy()
    rows = []
    with torch.no_grad():
        # -- the launches of _sample, unfused, on buffers the test owns
        b = Bufs()
        ca = lib.VdnCoarseArgs()
        ca.near, ca.far, ca.lin_samples = tn.data_ptr(), tf.data_ptr(), consts["lin_samples"].data_ptr()
        ca.lin_outside, ca.out_lower, ca.out_upper = (consts[k].data_ptr() for k in ("lin_outside", "out_lower", "out_upper"))
        ca.z, ca.z_out = b.out("z", B, N), b.out("z_out", B, O)
        ca.B, ca.n_samples, ca.n_outside, ca.z_ld = B, S, O, N
        _call("vdn_coarse_z", ca, _stream())
        _check_rows(b, "z", S)
        b.out("sdf", B, N)
        coarse = b["z"][:, :S].clone()
        net._run(0, rays=(to, td, b["z"][:, :S]), sdf_out=b["sdf"][:, :S])
        _check_rows(b, "sdf", S)
        M = S
        for i in range(steps):
            inv_s = 64.0 * 2 ** i
            z_rows, sdf_rows = b.np("z")[:, :M].astype(np.float32), b.np("sdf")[:, :M].astype(np.float32)
            r = Bufs()
            ua = _upsample_args(r, B, M, N, n_imp, inv_s, u, rays=rays)
            ua.z, ua.sdf = b["z"].data_ptr(), b["sdf"].data_ptr()
            _call("vdn_upsample_round", ua, _stream())
            r.check()
            _hold("%s B%d round %d (M %d, inv_s %g)" % (precision, B, i, M, inv_s), _model("tight", rays, z_rows, sdf_rows, u, inv_s),
                  r.np("new_z"), rows)
            m = lib.VdnMergeArgs()
            m.z = m.z_out = b["z"].data_ptr()
            m.new_z = r["new_z"].data_ptr()
            m.B, m.M, m.K, m.ld, m.ld_out = B, M, n_imp, N, N
            if i + 1 < steps:
                new_sdf = net._run(0, rays=(to, td, r["new_z"])).view(B, n_imp)
                m.sdf = m.sdf_out = b["sdf"].data_ptr()
                m.new_sdf = new_sdf.data_ptr()
            _call("vdn_merge_sorted", m, _stream())
            M += n_imp
            _check_rows(b, "z", M)
            _check_rows(b, "sdf", M if i + 1 < steps else M - n_imp)
        final = b["z"]
        assert (final[:, 1:] >= final[:, :-1]).all()
        # -- what _sample() returns
        z, z_out = rend._sample(to, td, tn, tf, 0, None, None, None, defer_last_merge=defer)
        assert torch.equal(z_out, b["z_out"])
        if defer:
            new_z, M_old = rend._pending_merge
            assert M_old == N - n_imp and not torch.equal(z, final)
            tp = lib.VdnTrainPrepArgs()
            q = Bufs()
            tp.rays_o, tp.rays_d, tp.z, tp.new_z, tp.M_old, tp.z_out = to.data_ptr(), td.data_ptr(), z.data_ptr(), new_z.data_ptr(), M_old, z_out.data_ptr()
            tp.B, tp.N, tp.T, tp.z_ld, tp.sample_dist, tp.fg_radius = B, N, N + O, z.stride(0), 2.0 / S, 1.2
            tp.z_feed, tp.dists, tp.mid_z = q.out("z_feed", B, N + O), q.out("dists", B, N), q.out("mid_z", B, N)
            tp.bg_dists, tp.bg_mid = q.out("bg_dists", B, N + O), q.out("bg_mid", B, N + O)
            ints = [torch.empty(n, dtype=torch.int32, device=DEV) for n in (B * (N + O), 1, B)]
            tp.bg_active_idx, tp.bg_n_active, tp.bg_ray_counts = (t.data_ptr() for t in ints)
            _call("vdn_train_prep", tp, _stream())
            q.check()
        else:
            assert rend._pending_merge is None
        assert torch.equal(z, final), "_sample() and the unfused launches disagree"
        # the 64 coarse depths are carried through the four merges unchanged
        fin, co = final.cpu().numpy(), coarse.cpu().numpy()
        assert all(np.isin(co[k].view(np.int32), fin[k].view(np.int32)).all() for k in range(B))
