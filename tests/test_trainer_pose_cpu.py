"""The learnable-pose Trainer's host-side semantics (no GPU): the pose / focal learning-rate schedules restated from
torch.optim.lr_scheduler.MultiStepLR as dpt_runner.py drives them, and the refine gating of the pose optimizer."""
import pytest
import torch

from vdn_train.trainer import DEFAULT_TRAIN_CONF, pose_schedules, refine_pose_now


def _runner_lrs(conf, iters, resume_at=None):
    """The reference's own objects: Adam + MultiStepLR constructed as dpt_runner.py:91-97, one step() in train() in front of the
    loop (update_learning_rate, :175), one after every iteration (:263). A resume constructs them afresh and THEN loads the
    optimizers' saved state (load_pnf_checkpoint, :383-389), which restores their decayed lr; no scheduler state is saved.
    -> [(pose lr, focal lr) used by iteration k]"""
    def fresh(saved=None):
        p = torch.nn.Parameter(torch.zeros(3))
        f = torch.nn.Parameter(torch.zeros(1))
        op, of = torch.optim.Adam([p], lr=conf["pose_lr"]), torch.optim.Adam([f], lr=conf["focal_lr"])
        sp = torch.optim.lr_scheduler.MultiStepLR(op, milestones=range(conf["warm_up_end"], conf["end_iter"], conf["step_size"]),
                                                  gamma=conf["pose_lr_gamma"])
        sf = torch.optim.lr_scheduler.MultiStepLR(of, milestones=(conf["warm_up_end"], conf["end_iter"], conf["step_size"]),
                                                  gamma=conf["focal_lr_gamma"])
        if saved is not None:
            op.load_state_dict(saved[0])
            of.load_state_dict(saved[1])
        sp.step()
        sf.step()
        return op, of, sp, sf
    op, of, sp, sf = fresh()
    out = []
    for k in range(iters):
        if k == resume_at:
            op, of, sp, sf = fresh((op.state_dict(), of.state_dict()))
        out.append((op.param_groups[0]["lr"], of.param_groups[0]["lr"]))
        sp.step()
        sf.step()
    return out


def _restated_lrs(conf, iters, resume_at=None):
    def fresh(saved=None):
        p, f = pose_schedules(conf, *(saved or (None, None)))
        p.step()
        f.step()
        return p, f
    p, f = fresh()
    out = []
    for k in range(iters):
        if k == resume_at:
            p, f = fresh((p.lr, f.lr))        # the lr the saved optimizer states hold
        out.append((p.lr, f.lr))
        p.step()
        f.step()
    return out


@pytest.mark.parametrize("warm,step,end,resume", [(50, 200, 2500, None), (7, 3, 3000, None), (100, 250, 2000, 1234), (0, 1000, 3000, 700),
                                                  (0, 100, 3000, 1000), (5, 1, 3000, 1500)])
def test_pose_and_focal_schedules_equal_multisteplr(warm, step, end, resume):
    conf = dict(DEFAULT_TRAIN_CONF, warm_up_end=warm, end_iter=end, step_size=step, pose_lr=5e-4, focal_lr=1e-3,
                pose_lr_gamma=0.9, focal_lr_gamma=0.5)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (torch warns about scheduler.step() without optimizer.step())
        want = _runner_lrs(conf, 3000, resume)
    got = _restated_lrs(conf, 3000, resume)
    assert got == want
    # the schedules do move: the pose lr has dropped by the end; a resume keeps the decayed lr (it does not go back to pose_lr)
    assert got[-1][0] < got[0][0]
    if resume is not None:
        assert got[resume][0] <= got[resume - 1][0]


@pytest.mark.parametrize("start", [-1, 0, 5])
def test_refine_gating_is_strictly_after_start(start):
    """dpt_runner.py:246-253: `if self.learnable and self.iter_step > self.start_refine_pose_iter` (> , not >=)."""
    steps = [k for k in range(10) if refine_pose_now(k, start)]
    assert steps == list(range(start + 1, 10))
    assert not refine_pose_now(start, start) and refine_pose_now(start + 1, start)
