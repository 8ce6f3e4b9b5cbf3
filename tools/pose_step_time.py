"""ms per training step at B = 512 on the same pixels, three paths: the learnable-pose Trainer step (Trainer.train_step_at after
start_refine_pose_iter), the fixed-pose Trainer.train_step, and the drop-in learnable flow (LearnableRays + render() under grad +
the runner's loss + loss.backward() + torch.optim.Adam). HIP events around each timed window.
usage: pose_step_time.py [--steps K] [--warmup W] [--precision fp32|bf16|both]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vdn-nerf_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vdn_train import synth, factory  # noqa: E402
from vdn_train.rays import RaysGenerator  # noqa: E402
from vdn_train.trainer import Trainer  # noqa: E402
from dpt_models.poses import LearnPose, LearnIntrin, LearnableRays  # noqa: E402

B, H, W, N_CAMS = 512, 800, 800, 8


def scene(precision, dev):
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(0), precision=precision)
    cams = np.asarray(synth.make_cameras(0)[:N_CAMS], np.float32)
    intr = LearnIntrin(H, W, req_grad=True, order=2, init_focal=torch.tensor(1111.0)).to(dev)
    imgs = np.random.RandomState(0).rand(N_CAMS, H, W, 3).astype(np.float32)
    fixed = RaysGenerator(imgs, None, cams, intr().cpu().numpy(), device=dev)
    pose = LearnPose(N_CAMS, True, True, init_c2w=torch.tensor(cams)).to(dev)
    return rend, intr, fixed, pose


def timed(fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(steps):
        fn(warmup + k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run(precision, steps, warmup, dev):
    gen = torch.Generator(device="cpu").manual_seed(0)
    pix = [((torch.rand(B, generator=gen) * W).floor().to(dev), (torch.rand(B, generator=gen) * H).floor().to(dev))
           for _ in range(steps + warmup)]
    res = {}
    # the pose step
    rend, intr, fixed, pose = scene(precision, dev)
    tr = Trainer(rend, B, dev, conf=dict(start_refine_pose_iter=-1), cameras=LearnableRays(pose, intr, fixed))
    res["pose_step_ms"] = timed(lambda k: tr.train_step_at(k % N_CAMS, *pix[k]), steps, warmup)
    # the fixed-pose step on the same pixels (rays from the resident generator)
    rend, intr, fixed, pose = scene(precision, dev)
    tr = Trainer(rend, B, dev)
    rows = []
    for k, (px, py) in enumerate(pix):
        out, near, far = fixed.gen_random_rays_at(k % N_CAMS, B, pixels=(px, py), return_near_far=True)
        rows.append((out[:, 0:3].contiguous(), out[:, 3:6].contiguous(), near, far, out[:, 7:10].contiguous()))
    res["fixed_step_ms"] = timed(lambda k: tr.train_step(*rows[k]), steps, warmup)
    # the drop-in learnable flow
    rend, intr, fixed, pose = scene(precision, dev)
    lr = LearnableRays(pose, intr, fixed)
    params = rend._all_parameters()
    opt, opt_pose = torch.optim.Adam(params, lr=5e-4), torch.optim.Adam(pose.parameters(), lr=5e-4)
    bg = torch.ones(1, 3, device=dev)

    def drop_in(k):
        data = lr.gen_random_rays_at(k % N_CAMS, B, pixels=pix[k])
        ro, rd, rgb = data[:, :3], data[:, 3:6], data[:, 7:10]
        mid = 0.5 * (-(2.0 * (ro * rd).sum(-1, keepdim=True))) / (rd * rd).sum(-1, keepdim=True)
        out = rend.render(ro, rd, mid - 1.0, mid + 1.0, background_rgb=bg, cos_anneal_ratio=0.5)
        loss = (out["color_fine"] - rgb).abs().sum() / (B + 1e-5) + out["gradient_error"] * 0.1
        opt.zero_grad()
        opt_pose.zero_grad()
        loss.backward()
        opt.step()
        opt_pose.step()
    res["drop_in_ms"] = timed(drop_in, steps, warmup)
    for k in ("pose_step", "fixed_step", "drop_in"):
        res[k + "_krays_s"] = B / res[k + "_ms"]          # B rays per ms = K rays / s
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--precision", default="both")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for p in (("bf16", "fp32") if a.precision == "both" else (a.precision,)):
        print(json.dumps(dict(precision=p, B=B, steps=a.steps, **{k: round(v, 4) for k, v in run(p, a.steps, a.warmup, dev).items()})), flush=True)


if __name__ == "__main__":
    main()
