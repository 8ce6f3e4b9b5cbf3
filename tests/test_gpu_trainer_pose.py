"""Learnable camera poses in the fused Trainer (reference dpt_runner.py:197-259 with `*_learn_*` configurations):
vdn_gen_rays_pose against the reference's own rays at its shipped learned poses (tests/golden/pnf_rays.npz) and against
LearnableRays; vdn_pose_adjoint against the reference's autograd and fp64 autograd; ray gradients on the foreground work
list; one Trainer.train_step_at against the drop-in flow (LearnableRays + render() + loss.backward()); pose recovery; the
refine gating, the schedule, the pnf_* checkpoints."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _lib():
    from vdn_hip import lib
    return lib


def _gen_pose(px, py, Kinv, r, t, init, out_ld=6, fixed=None, idx=0):
    lib = _lib()
    B = px.numel()
    out = torch.zeros(B, out_ld, device=DEV)
    near, far = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    a = lib.VdnGenRaysPoseArgs()
    a.pixels_x, a.pixels_y, a.intrinsic_inv = px.data_ptr(), py.data_ptr(), Kinv.data_ptr()
    a.r, a.t = r.data_ptr(), t.data_ptr()
    a.init_c2w = init.data_ptr() if init is not None else None
    if fixed is not None:
        a.image = fixed.images[idx].data_ptr()
        if fixed.masks is not None:
            a.mask, a.mask_ch = fixed.masks[idx].data_ptr(), fixed.masks.shape[-1]
        if fixed.with_depth:
            a.feats, a.C = fixed.depth_feats[idx].data_ptr(), fixed.C
    a.out, a.near, a.far = out.data_ptr(), near.data_ptr(), far.data_ptr()
    a.B, a.H, a.W, a.out_ld = B, (fixed.H if fixed else 800), (fixed.W if fixed else 800), out_ld
    lib.call("vdn_gen_rays_pose", a, lib.stream_handle())
    return out, near, far


def _adjoint(px, py, Kinv, r, t, init, d_o, d_d, n_cams, cam, d_z=None, lin=None, d_z_out=None, z_out=None, n_samples=64, n_importance=64):
    lib = _lib()
    g = torch.full((6 * n_cams,), float("nan"), device=DEV)
    a = lib.VdnPoseAdjointArgs()
    a.pixels_x, a.pixels_y, a.intrinsic_inv = px.data_ptr(), py.data_ptr(), Kinv.data_ptr()
    a.r, a.t = r.data_ptr(), t.data_ptr()
    a.init_c2w = init.data_ptr() if init is not None else None
    a.d_rays_o, a.d_rays_d = d_o.data_ptr(), d_d.data_ptr()
    if d_z is not None:
        a.d_z, a.lin_samples, a.N = d_z.data_ptr(), lin.data_ptr(), d_z.shape[1]
    if d_z_out is not None:
        a.d_z_out, a.z_out, a.O = d_z_out.data_ptr(), z_out.data_ptr(), d_z_out.shape[1]
    a.grad_r, a.grad_t = g.data_ptr(), g[3 * n_cams:].data_ptr()
    scratch = torch.full((12 * px.numel(),), float("nan"), dtype=torch.float64, device=DEV)
    a.scratch = scratch.data_ptr()
    a.B, a.n_samples, a.n_importance, a.cam, a.n_cams = px.numel(), n_samples, n_importance, cam, n_cams
    lib.call("vdn_pose_adjoint", a, lib.stream_handle())
    return g[:3 * n_cams].view(n_cams, 3), g[3 * n_cams:].view(n_cams, 3)


def _golden_setups():
    from vdn_train.rays import RaysGenerator
    from dpt_models.poses import LearnPose, LearnIntrin
    fx = load_golden("pnf_rays")
    H, W = int(fx["H"]), int(fx["W"])
    for tag in fx["names"]:
        tag = str(tag)
        n = fx[tag + "/r"].shape[0]
        pose = LearnPose(n, True, True, torch.zeros(n, 4, 4))
        pose.load_state_dict({k: torch.tensor(fx["%s/%s" % (tag, k)]) for k in ("init_c2w", "r", "t")})
        intr = LearnIntrin(H, W, req_grad=True)
        intr.load_state_dict({"fx": torch.tensor(fx[tag + "/fx"])})
        bgra = fx[tag + "/bgra"].astype(np.float64) / 255.0
        img, a = bgra[..., :3], bgra[..., 3:]
        img = (img * a + (1 - a)).astype(np.float32)
        fixed = RaysGenerator(img, a.astype(np.float32), fx[tag + "/c2w"][:3], fx[tag + "/intrinsic"], device=DEV)
        yield fx, tag, pose.to(DEV), intr.to(DEV), fixed


def test_pose_rays_and_adjoint_on_the_reference_shipped_cameras():
    """Item 1 + 2 on tests/golden/pnf_rays.npz: the reference's rays at its ten shipped learned-pose sets, and its autograd's
    d (r, t) of a linear loss on the rays; through a Trainer with cameras, whose state comes from a pnf_* checkpoint written
    in the reference's format (dpt_runner.py:391-401)."""
    from vdn_train import synth, factory
    from vdn_train.trainer import Trainer
    from dpt_models.poses import LearnPose, LearnIntrin, LearnableRays
    rend = factory.build_renderer(device=DEV, states=synth.make_all_states(0))
    worst = {"o": 0.0, "d": 0.0, "gr": 0.0, "gt": 0.0}
    for fx, tag, pose_ref, intr_ref, fixed in _golden_setups():
        n = pose_ref.num_cams
        # a Trainer whose cameras start at zero deltas, then loads the reference-format checkpoint
        pose = LearnPose(n, True, True, pose_ref.init_c2w.detach().clone()).to(DEV)
        intr = LearnIntrin(fixed.H, fixed.W, req_grad=True).to(DEV)
        tr = Trainer(rend, 16, DEV, cameras=LearnableRays(pose, intr, fixed))
        ck = {"intrin_net": intr_ref.state_dict(), "pose_param_net": pose_ref.state_dict(),
              "optimizer_focal": torch.optim.Adam(intr_ref.parameters(), lr=5e-4).state_dict(),
              "optimizer_pose": torch.optim.Adam(pose_ref.parameters(), lr=5e-4).state_dict(),
              "poses_iter_step": int(fx[tag + "/poses_iter_step"])}
        tr.load_pnf_checkpoint(ck)
        assert tr.poses_iter_step == int(fx[tag + "/poses_iter_step"])
        assert torch.equal(pose.r.detach(), pose_ref.r.detach()) and torch.equal(pose.t.detach(), pose_ref.t.detach())
        for idx in (0, 1, 2):
            k = "%s/cam%d" % (tag, idx)
            want = fx[k + "/data"]
            px = torch.tensor(fx[k + "/pixels_x"].astype(np.float32), device=DEV)
            py = torch.tensor(fx[k + "/pixels_y"].astype(np.float32), device=DEV)
            rows, near, far = tr.gen_rays_at(idx, px, py)
            got = rows.cpu().numpy()
            worst["o"] = max(worst["o"], float(np.abs(got[:, :3] - want[:, :3]).max()))
            worst["d"] = max(worst["d"], float(np.abs(got[:, 3:6] - want[:, 3:6]).max()))
            assert np.array_equal(got[:, 6:], want[:, 6:]), (tag, idx)
            fr = fixed.gen_random_rays_at(idx, 16, pixels=(px, py))
            assert torch.equal(rows[:, 6:], fr[:, 6:])
            w = torch.tensor(fx[k + "/loss_weights"], device=DEV)
            gsum = tr.pose_adjoint(idx, px, py, w[:, :3].contiguous(), w[:, 3:6].contiguous(), None, None, None).clone()
            gr, gt = gsum[:3 * n].view(n, 3).cpu().numpy(), gsum[3 * n:].view(n, 3).cpu().numpy()
            worst["gr"] = max(worst["gr"], float(np.abs(gr[idx] - fx[k + "/grad_r"]).max() / (np.abs(fx[k + "/grad_r"]).max() + 1e-30)))
            worst["gt"] = max(worst["gt"], float(np.abs(gt[idx] - fx[k + "/grad_t"]).max() / (np.abs(fx[k + "/grad_t"]).max() + 1e-30)))
            others = np.ones(n, bool)
            others[idx] = False
            assert np.all(gr[others] == 0) and np.all(gt[others] == 0)
    assert worst["o"] < 1e-6 and worst["d"] < 2e-6, worst
    assert worst["gr"] < 2e-5 and worst["gt"] < 2e-5, worst


def _kinv():
    from dpt_models.poses import LearnIntrin
    intr = LearnIntrin(800, 800, req_grad=False, order=2, init_focal=torch.tensor(1111.0))
    K = intr()
    return intr, torch.inverse(K)[:3, :3].contiguous()


@pytest.mark.parametrize("rmag", [0.0, 1e-4, 0.05])
def test_pose_rays_equal_learnable_rays(rmag):
    """Item 1: vdn_gen_rays_pose against LearnableRays at random t and r = 0, |r| ~ 1e-4, |r| ~ 0.05; the pixel / mask / feature
    columns bit-identical to vdn_gen_rays."""
    from vdn_train import synth
    from vdn_train.rays import RaysGenerator
    from dpt_models.poses import LearnPose, LearnableRays
    rng = np.random.RandomState(3)
    n, H, W, C = 3, 40, 56, 5
    from dpt_models.poses import LearnIntrin
    intr = LearnIntrin(H, W, req_grad=False, order=2, init_focal=torch.tensor(60.0))
    cams = np.asarray(synth.make_cameras(3, n=n), np.float32)
    fixed = RaysGenerator(rng.rand(n, H, W, 3).astype(np.float32), rng.rand(n, H, W, 1).astype(np.float32), cams, intr().numpy(),
                          depth_feats=rng.rand(n, H, W, C).astype(np.float32), device=DEV)
    pose = LearnPose(n, True, True, torch.tensor(cams))
    with torch.no_grad():
        d = torch.tensor(rng.randn(n, 3).astype(np.float32))
        pose.r.copy_(d / d.norm(dim=1, keepdim=True) * rmag)
        pose.t.copy_(torch.tensor(rng.randn(n, 3).astype(np.float32) * 0.05))
    pose = pose.to(DEV)
    lr = LearnableRays(pose, intr.to(DEV), fixed)
    px = torch.tensor(rng.randint(0, W, 300).astype(np.float32), device=DEV)
    py = torch.tensor(rng.randint(0, H, 300).astype(np.float32), device=DEV)
    Kinv = torch.inverse(intr().cpu())[:3, :3].contiguous().to(DEV)
    for i in range(n):
        want = lr.gen_random_rays_at(i, 300, pixels=(px, py)).detach()
        got, near, far = _gen_pose(px, py, Kinv, pose.r.detach()[i].contiguous(), pose.t.detach()[i].contiguous(), pose.init_c2w[i].contiguous(),
                                   out_ld=10 + C, fixed=fixed, idx=i)
        assert (got[:, :6] - want[:, :6]).abs().max().item() <= 2e-6
        fr, nr, fa = fixed.gen_random_rays_at(i, 300, pixels=(px, py), return_near_far=True)
        assert torch.equal(got[:, 6:], fr[:, 6:])
        o, v = got[:, :3], got[:, 3:6]
        mid = 0.5 * (-(2.0 * (o * v).sum(-1))) / (v * v).sum(-1)
        assert (near - (mid - 1)).abs().max().item() < 1e-5 and (far - (mid + 1)).abs().max().item() < 1e-5


@pytest.mark.parametrize("rmag,n_importance", [(0.0, 64), (1e-4, 64), (0.05, 0), (0.0, 0), (1e-4, 0)])
def test_pose_adjoint_vs_fp64_autograd(rmag, n_importance):
    """Item 2: torch fp64 autograd of LearnPose -> rays -> near_far_from_sphere -> _attach_rays (z_out = far c + 1/n_samples;
    the inside depths near + (far - near) lin only with n_importance = 0) with random d_rays_o, d_rays_d, d_z, d_z_out; and
    the kernel run twice is bit-identical."""
    from vdn_train import synth
    from dpt_models.lie_group_helper import make_c2w
    rng = np.random.RandomState(11)
    n, cam, B, S, O = 4, 2, 2000, 64, 32
    N = S + n_importance
    cams = torch.tensor(np.asarray(synth.make_cameras(1, n=n), np.float32))
    _, Kinv = _kinv()
    d = rng.randn(3)
    r32 = torch.tensor((d / np.linalg.norm(d) * rmag).astype(np.float32))
    t32 = torch.tensor((rng.randn(3) * 0.05).astype(np.float32))
    px = torch.tensor(rng.randint(0, 800, B).astype(np.float32))
    py = torch.tensor(rng.randint(0, 800, B).astype(np.float32))
    c = torch.tensor(rng.rand(B, O).astype(np.float32) * 0.9 + 0.05)
    lin = torch.linspace(0, 1, S)
    d_o, d_d = torch.randn(B, 3), torch.randn(B, 3)
    d_z, d_zo = torch.randn(B, N) * 0.1, torch.randn(B, O) * 0.1

    # fp64 reference
    r = r32.double().requires_grad_(True)
    t = t32.double().requires_grad_(True)

    def exp64(v):
        K = torch.zeros(3, 3, dtype=torch.float64)
        K = torch.stack([torch.stack([K[0, 0], -v[2], v[1]]), torch.stack([v[2], K[0, 0], -v[0]]), torch.stack([-v[1], v[0], K[0, 0]])])
        nn_ = v.norm() + 1e-15
        return torch.eye(3, dtype=torch.float64) + (torch.sin(nn_) / nn_) * K + ((1 - torch.cos(nn_)) / nn_ ** 2) * (K @ K)
    c2w = torch.cat([torch.cat([exp64(r), t[:, None]], 1), torch.tensor([[0, 0, 0, 1.0]], dtype=torch.float64)], 0) @ cams[cam].double()
    p = torch.stack([px.double(), py.double(), torch.ones(B, dtype=torch.float64)], -1) @ Kinv.double().T
    v = p / p.norm(dim=-1, keepdim=True)
    rd = v @ c2w[:3, :3].T
    ro = c2w[:3, 3].expand(B, 3)
    mid = -(ro * rd).sum(-1, keepdim=True) / (rd * rd).sum(-1, keepdim=True)
    near, far = mid - 1, mid + 1
    zo = far * c.double() + 1.0 / S
    loss = (ro * d_o.double()).sum() + (rd * d_d.double()).sum() + (zo * d_zo.double()).sum()
    if n_importance == 0:
        z = near + (far - near) * lin.double()[None]
        loss = loss + (z * d_z.double()).sum()
    gr64, gt64 = torch.autograd.grad(loss, (r, t))

    # the kernel: the depths it reads are the fp32 ones of the rays it makes
    g = lambda x: x.contiguous().to(DEV)
    init = g(cams[cam])
    _, _, far32 = _gen_pose(g(px), g(py), g(Kinv), g(r32), g(t32), init)
    z_out32 = far32[:, None] * g(c) + 1.0 / S
    kw = dict(d_z=g(d_z), lin=g(lin), d_z_out=g(d_zo), z_out=z_out32.contiguous(), n_samples=S, n_importance=n_importance)
    pose_flat = torch.zeros(6 * n, device=DEV)
    pose_flat[3 * cam:3 * cam + 3], pose_flat[3 * n + 3 * cam:3 * n + 3 * cam + 3] = g(r32), g(t32)
    gr, gt = _adjoint(g(px), g(py), g(Kinv), pose_flat[3 * cam:], pose_flat[3 * n + 3 * cam:], init, g(d_o), g(d_d), n, cam, **kw)
    gr2, gt2 = _adjoint(g(px), g(py), g(Kinv), pose_flat[3 * cam:], pose_flat[3 * n + 3 * cam:], init, g(d_o), g(d_d), n, cam, **kw)
    assert torch.equal(gr, gr2) and torch.equal(gt, gt2)
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    assert rel(gr[cam], gr64) <= 1e-5 and rel(gt[cam], gt64) <= 1e-5, (rel(gr[cam], gr64), rel(gt[cam], gt64))
    others = [i for i in range(n) if i != cam]
    assert torch.all(gr[others] == 0) and torch.all(gt[others] == 0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_compacted_ray_gradients_equal_the_full_ones(precision):
    """Item 3: d_rays_o, d_rays_d, d_z, d_z_out with skip_far=True (ray_grads_compact) equal the skip_far=False ones."""
    from vdn_train import synth, factory
    from vdn_hip.train import TrainEngine
    seed, B = 4, 512
    rend = factory.build_renderer(device=DEV, states=synth.make_all_states(seed), precision=precision)
    cams = synth.make_cameras(seed)
    o, d = synth.random_pixel_batch(seed, 0, 1, B, cams=cams)
    near, far = synth.near_far_from_sphere(o, d)
    t1, t2 = synth.jitter(seed, 0, B)
    tt = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32).to(DEV).contiguous()
    o, d, near, far, t1, t2 = (tt(x) for x in (o, d, near, far, t1, t2))
    eng = TrainEngine(rend, B, DEV)
    gen = torch.Generator(device="cpu").manual_seed(0)
    g_color = tt(torch.randn(B, 3, generator=gen) * 1e-2)
    g_eik = tt([0.1])
    res = {}
    for skip in (False, True):
        with torch.no_grad():
            z, z_out = rend._sample(o, d, near.reshape(B), far.reshape(B), rend.perturb, t1.view(B, 1), t2, None)
        w = eng.forward(o, d, z.contiguous(), z_out, torch.ones(3, device=DEV), 0.5, skip_far=skip, ray_grads=True, ray_grads_compact=skip)
        if skip:
            assert eng._fg_compact and int(w["fg_active"][1].item()) < eng.P        # the list does skip samples
        eng.backward(g_color, None, None, g_eik)
        res[skip] = {k: w[k].clone() for k in ("d_rays_o", "d_rays_d", "d_z", "d_z_out")}
        res[skip]["grad"] = eng._grad_flat.clone()
    for k in ("d_rays_o", "d_rays_d", "d_z", "d_z_out"):
        a, b = res[True][k], res[False][k]
        err = float((a - b).abs().max() / (b.abs().max() + 1e-30))
        assert err <= 1e-6, (k, err)
    ga, gb = res[True]["grad"], res[False]["grad"]
    assert float((ga - gb).norm() / gb.norm()) < (1e-4 if precision == "fp32" else 1e-2)


def _scene(precision="fp32", seed=0, n=4, H=800, W=800, images=None, wdepth=False):
    from vdn_train import synth, factory
    from vdn_train.rays import RaysGenerator
    from dpt_models.poses import LearnIntrin
    rend = factory.build_renderer(device=DEV, states=synth.make_all_states(seed, wdepth=wdepth, variance=0.3), precision=precision)
    cams = np.asarray(synth.make_cameras(seed)[:n], np.float32)
    intr = LearnIntrin(H, W, req_grad=True, order=2, init_focal=torch.tensor(1111.0)).to(DEV)
    if images is None:
        images = np.random.RandomState(seed).rand(n, H, W, 3).astype(np.float32)
    fixed = RaysGenerator(images, None, cams, intr().cpu().numpy(), device=DEV)
    return rend, cams, intr, fixed


def _pose_net(cams, r0=None, t0=None, learn_R=True, learn_t=True):
    from dpt_models.poses import LearnPose
    pn = LearnPose(len(cams), learn_R, learn_t, init_c2w=torch.tensor(cams)).to(DEV)
    with torch.no_grad():
        if r0 is not None:
            pn.r.copy_(r0)
        if t0 is not None:
            pn.t.copy_(t0)
    return pn


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_pose_step_equals_the_drop_in_flow(precision):
    """Item 4: Trainer.train_step_at against LearnableRays + render() + the runner's loss + loss.backward() + torch.optim.Adam on
    the same pixels and jitter: the pose gradient of the first step, then parameters and (r, t) after three steps."""
    from vdn_train.trainer import Trainer
    from dpt_models.poses import LearnableRays
    B, cam, steps = 512, 1, 3
    conf = dict(warm_up_end=0, start_refine_pose_iter=-1, anneal_end=0)
    rng = np.random.RandomState(2)
    r0 = torch.tensor(rng.randn(4, 3).astype(np.float32) * 0.01)
    t0 = torch.tensor(rng.randn(4, 3).astype(np.float32) * 0.02)
    rend_a, cams, intr, fixed = _scene(precision)
    rend_b, _, _, _ = _scene(precision)
    pose_a, pose_b = _pose_net(cams, r0, t0), _pose_net(cams, r0, t0)
    tr = Trainer(rend_a, B, DEV, conf=conf, cameras=LearnableRays(pose_a, intr, fixed))
    lrays = LearnableRays(pose_b, intr, fixed)
    params_b = rend_b._all_parameters()
    opt = torch.optim.Adam(params_b, lr=tr.learning_rate())
    opt_pose = torch.optim.Adam(pose_b.parameters(), lr=5e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt_pose, milestones=range(0, tr.conf["end_iter"], 5000), gamma=0.9)
    sched.step()
    gen = torch.Generator(device="cpu").manual_seed(7)
    for it in range(steps):
        px = (torch.rand(B, generator=gen) * 500 + 150).floor().to(DEV)
        py = (torch.rand(B, generator=gen) * 500 + 150).floor().to(DEV)
        t1 = torch.rand(B, 1, generator=gen).to(DEV)
        t2 = torch.rand(B, 32, generator=gen).to(DEV)
        for grp in opt.param_groups:
            grp["lr"] = tr.learning_rate()
        tr.train_step_at(cam, px, py, t_rand=t1, t_rand_out=t2)
        data = lrays.gen_random_rays_at(cam, B, pixels=(px, py))
        # the graph from LearnableRays, the values of the rays / near / far the Trainer rendered: vdn_gen_rays_pose and the torch
        # ops differ by rounding, and a 1-ulp change of near / far moves the importance samples of some rays (2.6e-4 - 3.5e-4 of
        # the fp32 pose gradient with the values left to each path; below 1e-4 on the same values)
        kr = tr._rows.clone()
        ro = kr[:, :3] + (data[:, :3] - data[:, :3].detach())
        rd = kr[:, 3:6] + (data[:, 3:6] - data[:, 3:6].detach())
        rgb = data[:, 7:10]
        a2 = (rd ** 2).sum(-1, keepdim=True)
        mid = 0.5 * (-(2.0 * (ro * rd).sum(-1, keepdim=True))) / a2
        near = tr._near.clone() + (mid - mid.detach())
        far = tr._far.clone() + (mid - mid.detach())
        ro.retain_grad()
        rd.retain_grad()
        out = rend_b.render(ro, rd, near, far, background_rgb=torch.ones(1, 3, device=DEV), cos_anneal_ratio=1.0,
                            t_rand=t1, t_rand_out=t2)
        loss = (out["color_fine"] - rgb).abs().sum() / (B + 1e-5) + out["gradient_error"] * tr.conf["igr_weight"]
        opt.zero_grad()
        opt_pose.zero_grad()
        loss.backward()
        if it == 0:
            n = 4
            got = tr._pose_grad.clone()
            gr, gt = got[:3 * n].view(n, 3), got[3 * n:].view(n, 3)
            wr, wt = pose_b.r.grad, pose_b.t.grad
            assert torch.all(gr[[0, 2, 3]] == 0) and torch.all(gt[[0, 2, 3]] == 0)
            if precision == "fp32":
                rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
                w = tr.engine.w
                diag = (rel(w["d_rays_o"], ro.grad), rel(w["d_rays_d"], rd.grad))
                assert rel(gr[cam], wr[cam]) <= 1e-4 and rel(gt[cam], wt[cam]) <= 1e-4, (diag, gr[cam], wr[cam], gt[cam], wt[cam])
            else:
                cos = torch.nn.functional.cosine_similarity(torch.cat([gr[cam], gt[cam]]), torch.cat([wr[cam], wt[cam]]), dim=0).item()
                assert cos >= 0.999, cos
        opt.step()
        opt_pose.step()
        sched.step()
    tr.join()
    dr = (pose_a.r.detach() - pose_b.r.detach()).abs().max().item()
    dt = (pose_a.t.detach() - pose_b.t.detach()).abs().max().item()
    diff = torch.cat([(p - q).detach().reshape(-1).abs() for p, q in zip(tr.params, params_b)])
    frac = float((diff > 2e-5).float().mean())
    if precision == "fp32":
        assert dr < 2e-5 and dt < 2e-5, (dr, dt)
        # Adam's first steps move every weight by ~lr whatever the gradient size: sign decisions on ~0 gradients may differ
        assert frac < 1e-3 and float(diff.max()) < 6 * 5e-4, (frac, float(diff.max()))
    else:
        # bf16: the two paths' gradients agree to cosine 0.999, not to fp32 rounding (the compacted and the full backward sum
        # bf16 products in different orders), so Adam's normalised steps - at most 3 lr ~ 1.4e-3 per parameter over three
        # steps - can part where a gradient component is near zero. Bound: (r, t) within a tenth of that travel; weights as
        # in fp32, with a share of parting weights ten times larger
        assert dr < 1.4e-4 and dt < 1.4e-4, (dr, dt)
        assert frac < 1e-2 and float(diff.max()) < 6 * 5e-4, (frac, float(diff.max()))


def _render_targets(rend, cams, intr, cam, true_r, true_t, H=800, W=800, lo=150, hi=650):
    """The image of camera `cam` at its true pose over pixels [lo, hi)^2 (elsewhere white), rendered without jitter."""
    pn = _pose_net(cams)
    with torch.no_grad():
        pn.r[cam].copy_(true_r)
        pn.t[cam].copy_(true_t)
    Kinv = torch.inverse(intr().cpu())[:3, :3].to(DEV)
    img = torch.ones(len(cams), H, W, 3, device=DEV)
    ys, xs = torch.meshgrid(torch.arange(lo, hi, device=DEV).float(), torch.arange(lo, hi, device=DEV).float(), indexing="ij")
    px, py = xs.reshape(-1).contiguous(), ys.reshape(-1).contiguous()
    n = len(cams)
    with torch.no_grad():
        for s in range(0, px.numel(), 8192):
            qx, qy = px[s:s + 8192].contiguous(), py[s:s + 8192].contiguous()
            rows, near, far = _gen_pose(qx, qy, Kinv.contiguous(), pn.r[cam].contiguous(), pn.t[cam].contiguous(), pn.init_c2w[cam].contiguous())
            out = rend.render(rows[:, :3].contiguous(), rows[:, 3:6].contiguous(), near, far, perturb_overwrite=0,
                              background_rgb=torch.ones(1, 3, device=DEV), cos_anneal_ratio=1.0)
            img[cam, qy.long(), qx.long()] = out["color_fine"]
    return img.cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_recovers_a_perturbed_camera(precision):
    """Item 5: test_pose_refinement_recovers_a_perturbed_camera through the Trainer: networks fixed (learning_rate = 0), colour
    term only (igr_weight = 0), targets rendered from the true camera held by the resident RaysGenerator."""
    from vdn_train.trainer import Trainer
    from vdn_train.rays import RaysGenerator
    from dpt_models.poses import LearnableRays
    B, steps, cam = 512, 200, 2
    rend, cams, intr, _ = _scene(precision, images=np.ones((4, 8, 8, 3), np.float32), H=800, W=800)
    rend.perturb = 0.0
    true_r, true_t = torch.tensor([0.02, -0.015, 0.01], device=DEV), torch.tensor([0.05, -0.04, 0.03], device=DEV)
    img = _render_targets(rend, cams, intr, cam, true_r, true_t)
    fixed = RaysGenerator(img, None, cams, intr().cpu().numpy(), device=DEV)
    pose = _pose_net(cams)
    conf = dict(learning_rate=0.0, igr_weight=0.0, pose_lr=2e-3, pose_lr_gamma=1.0, start_refine_pose_iter=-1, warm_up_end=0,
                anneal_end=0)            # (cos_anneal_ratio 1, as the targets were rendered)
    tr = Trainer(rend, B, DEV, conf=conf, cameras=LearnableRays(pose, intr, fixed))
    gen = torch.Generator(device="cpu").manual_seed(1)
    first = None
    for it in range(steps):
        px = (torch.rand(B, generator=gen) * 500 + 150).floor().to(DEV)
        py = (torch.rand(B, generator=gen) * 500 + 150).floor().to(DEV)
        sc = tr.train_step_at(cam, px, py)
        if first is None:
            first = sc[1].item()
    last = sc[1].item()
    er = (pose.r[cam].detach() - true_r).norm().item()
    et = (pose.t[cam].detach() - true_t).norm().item()
    assert last < 0.05 * first and er < 0.1 * true_r.norm().item() and et < 0.1 * true_t.norm().item(), (first, last, er, et)


def test_gating_schedule_and_learn_flags():
    """Item 6: r / t and their moments unchanged through iter_step = start_refine_pose_iter; the pose lr drops by gamma at a
    milestone; learn_R = False leaves r untouched. Item 8: world_size = 2 with cameras raises."""
    from vdn_train.trainer import Trainer
    from dpt_models.poses import LearnableRays
    B, start = 256, 2
    rend, cams, intr, fixed = _scene(H=64, W=64, images=np.random.RandomState(0).rand(4, 64, 64, 3).astype(np.float32))
    pose = _pose_net(cams)
    conf = dict(start_refine_pose_iter=start, warm_up_end=3, step_size=1000, end_iter=10000, pose_lr_gamma=0.5)
    tr = Trainer(rend, B, DEV, conf=conf, cameras=LearnableRays(pose, intr, fixed))
    lrs = []
    for it in range(start + 1):
        lrs.append(tr.pose_lr())
        tr.train_step_at(0)
        assert torch.all(pose.r.detach() == 0) and torch.all(pose.t.detach() == 0)
        assert torch.all(tr._pose_exp_avg == 0) and torch.all(tr._pose_exp_avg_sq == 0)
    tr.train_step_at(0)                      # iter_step = start + 1: the first pose step
    assert pose.t.detach()[0].abs().sum() > 0 and pose.r.detach()[0].abs().sum() > 0
    # epochs: 1 at step 0 (the step() in front of the loop) ... milestone 3 = warm_up_end
    assert tr.pose_sched.last_epoch == start + 3
    assert tr.pose_lr() == pytest.approx(5e-4 * 0.5) and lrs[0] == pytest.approx(5e-4)
    # learn_R = False: r never moves and has no Adam state
    rend2, cams2, intr2, fixed2 = _scene(H=64, W=64, images=np.random.RandomState(0).rand(4, 64, 64, 3).astype(np.float32))
    pose2 = _pose_net(cams2, learn_R=False)
    tr2 = Trainer(rend2, B, DEV, conf=dict(start_refine_pose_iter=-1), cameras=LearnableRays(pose2, intr2, fixed2))
    for _ in range(3):
        tr2.train_step_at(1)
    assert torch.all(pose2.r.detach() == 0) and pose2.t.detach()[1].abs().sum() > 0
    st = tr2.pnf_state_dict()["optimizer_pose"]["state"]
    assert set(st) == {2}
    with pytest.raises(NotImplementedError):
        Trainer(rend2, B, DEV, world_size=2, cameras=LearnableRays(pose2, intr2, fixed2))


def test_pnf_checkpoint_round_trip():
    """Item 7: save_pnf_checkpoint -> torch.optim.Adam(LearnPose.parameters()).load_state_dict works and one torch step from that
    state equals the Trainer's next pose step; state_dict() keys are those of a Trainer without cameras."""
    import copy
    import os
    import tempfile
    from vdn_train.trainer import Trainer
    from dpt_models.poses import LearnableRays
    B = 256
    rend, cams, intr, fixed = _scene(H=64, W=64, images=np.random.RandomState(1).rand(4, 64, 64, 3).astype(np.float32))
    pose = _pose_net(cams)
    conf = dict(start_refine_pose_iter=-1, warm_up_end=0, step_size=2, pose_lr_gamma=0.5)      # the pose lr decays as it goes
    tr = Trainer(rend, B, DEV, conf=conf, cameras=LearnableRays(pose, intr, fixed))
    for _ in range(3):
        tr.train_step_at(2)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pnf_000003.pth")
        tr.save_pnf_checkpoint(path)
        ck = torch.load(path)
    assert set(ck) == {"intrin_net", "pose_param_net", "optimizer_focal", "optimizer_pose", "poses_iter_step"}
    assert ck["poses_iter_step"] == 3 and set(ck["optimizer_pose"]["state"]) == {1, 2}
    assert float(ck["optimizer_pose"]["state"][1]["step"]) == 3 and ck["optimizer_focal"]["state"] == {}
    twin = copy.deepcopy(pose)
    twin.load_state_dict(ck["pose_param_net"])
    opt = torch.optim.Adam(twin.parameters(), lr=5e-4)
    opt.load_state_dict(copy.deepcopy(ck["optimizer_pose"]))         # (torch steps the loaded `step` tensors in place)
    assert opt.param_groups[0]["lr"] == pytest.approx(tr.pose_lr()) and "initial_lr" in opt.param_groups[0]
    # the Trainer's next pose step on a fixed pixel set; torch's step on the gradient the Trainer used
    px = torch.arange(B, device=DEV).float() % 64
    py = (torch.arange(B, device=DEV).float() * 7) % 64
    tr.train_step_at(2, px, py)
    n = 4
    twin.r.grad, twin.t.grad = tr._pose_grad[:3 * n].view(n, 3).clone(), tr._pose_grad[3 * n:].view(n, 3).clone()
    opt.step()
    assert (twin.r.detach() - pose.r.detach()).abs().max().item() < 1e-7
    assert (twin.t.detach() - pose.t.detach()).abs().max().item() < 1e-7
    # the network checkpoint is the same with or without cameras
    rend2, _, _, _ = _scene(H=64, W=64, images=np.zeros((4, 64, 64, 3), np.float32))
    assert set(Trainer(rend2, B, DEV).state_dict()) == set(tr.state_dict())
    # load_pnf_checkpoint restores parameters and moments
    tr.train_step_at(2, px, py)
    tr.load_pnf_checkpoint(ck)
    assert torch.equal(tr._pose_exp_avg[:12].view(4, 3).cpu(), ck["optimizer_pose"]["state"][1]["exp_avg"].cpu())
    assert tr._pose_steps == 3 and tr.poses_iter_step == 3 and tr.pose_sched.last_epoch == 0
    # the epoch counter restarts, the decayed rate stays (the runner constructs its scheduler, then loads the optimizer state)
    saved_lr = ck["optimizer_pose"]["param_groups"][0]["lr"]
    assert saved_lr == pytest.approx(5e-4 * 0.5 ** 3) and tr.pose_lr() == saved_lr
    tr.train_step_at(2, px, py)               # epoch 1 (the step in front of the loop): not a milestone, the rate holds
    assert tr.pose_sched.last_epoch == 2 and tr.pose_lr() == pytest.approx(saved_lr * 0.5)
