"""The launch groups of the ray engine's weight-gradient tail (vdn_hip/train.py: DwGroup, TrainEngine.groups) give the same
gradients whichever of them carries an entry: `all` in one go, `sdf` then `rest`, `sdf` then `heads` then `nerf`.

Every entry keeps its own K splits, slab and column sums in every group's table, and the finalize pass sums the splits of one
entry in a fixed order, so the arms agree bit for bit (as they did before the groups became one record: measured there on the
same inputs, all four configurations of tests/test_gpu_dw_plan_tables.py, largest difference 0)."""
import numpy as np
import pytest
import torch

B = 64
ARMS = (("all",), ("sdf", "rest"), ("sdf", "heads", "nerf"))


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["wdepth_bf16", "wdepth_fp32"])
def test_grouping_does_not_change_gradients(config):
    from vdn_train import synth, factory
    from vdn_hip.train import TrainEngine, _stream
    dev = torch.device("cuda:0")
    seed = 33
    g = lambda x: torch.tensor(np.asarray(x, np.float32)).to(dev)
    rend = factory.build_renderer(device=dev, states=synth.make_all_states(seed, wdepth=True), wdepth=True, precision=config[-4:])
    eng = TrainEngine(rend, B, dev)
    assert set(eng.groups) == {"all", "sdf", "rest", "heads", "nerf"}
    o, d = synth.random_pixel_batch(seed, 0, 3, B, cams=synth.make_cameras(seed))
    near, far = synth.near_far_from_sphere(o, d)
    t1, t2 = synth.jitter(seed, 0, B)
    o, d, near, far, t1, t2 = (g(x) for x in (o, d, near, far, t1, t2))
    with torch.no_grad():
        z, z_out = rend._sample(o, d, near.reshape(B), far.reshape(B), 1.0, t1, t2, None)
    # one eager step: the workspaces then hold the saved planes, the deltas and the device-side row counts every arm reads
    eng.forward(o, d, z.contiguous(), z_out, torch.ones(3, device=dev), 0.3, skip_far=True)
    eng.backward(g(synth.uniform(seed, "groups/gc", (B, 3)) - 0.5), g(synth.uniform(seed, "groups/gf", (B, 96)) - 0.5), None,
                 torch.tensor([0.1], device=dev))
    torch.cuda.synchronize()
    snap = [(t, t.clone()) for t in [eng._grad_flat] + [net.dweff for net in eng.nets.values()]]
    got = []
    for arm in ARMS:
        for t, t0 in snap:           # (whether finalize overwrites or accumulates does not matter then)
            t.copy_(t0)
        for group in arm:
            eng.weight_grads(group, _stream())
        torch.cuda.synchronize()
        got.append(eng._grad_flat.clone())
    assert torch.isfinite(got[0]).all() and got[0].abs().max() > 0
    for arm, x in zip(ARMS, got):
        assert torch.equal(x, got[0]), (arm, (x - got[0]).abs().max().item())
