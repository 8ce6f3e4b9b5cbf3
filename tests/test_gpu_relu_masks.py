"""1-bit ReLU masks (csrc/mlp_engine.h: BF16::relu_bits): the bf16 forwards of the background network and of the colour / VDN
heads write them beside their saved planes, and the backward chains read them instead of the planes. The predicate is the one
the plane-reading chains evaluate, so the training step must not change by a single bit (VDN_RELU_MASK=0 is the reference)."""
import numpy as np
import pytest


def _bf16_positive(b):
    """What the plane-reading backward evaluates: the bf16 bits, widened to f32, > 0."""
    return (b.astype(np.uint32) << 16).view(np.float32) > 0.0


def test_mask_predicate_covers_every_bf16_value():
    # every 16-bit pattern: positive finite values, +inf and NaN with a clear sign pass; zeros, negatives and the other NaNs do not
    b = np.arange(1 << 16, dtype=np.uint32)
    ok = _bf16_positive(b)
    assert ok.sum() == 0x7F80
    assert ok[1] and ok[0x7F7F] and ok[0x7F80] and not ok[0] and not ok[0x7F81] and not ok[0x8000] and not ok[0xFF80]


def test_mask_layout_decode_roundtrip():
    import torch
    from vdn_hip import layout
    P, ld = 70, 256
    g = torch.Generator().manual_seed(0)
    m = torch.rand(P, ld, generator=g) > 0.5
    # encode by the documented layout: lane (c, h) of block blk, bit 16 tile + t, feature 32 tile + 16k + 8j + 4h + e
    Pp = layout.pad32(P)
    full = torch.zeros(Pp, ld, dtype=torch.bool)
    full[:P] = m
    bits = full.view(Pp // 32, 32, ld // 32, 2, 2, 2, 4).permute(0, 5, 1, 2, 3, 4, 6).reshape(Pp // 32, 2, 32, ld // 16, 8)
    buf = (bits.long() << torch.arange(8)).sum(-1).to(torch.uint8).reshape(-1)
    assert torch.equal(layout.mask_from_plane(buf, P, ld), m)


def _trainer(monkeypatch, mask, wdepth, B):
    import torch
    from vdn_train import factory
    from vdn_train.trainer import Trainer
    monkeypatch.setenv("VDN_RELU_MASK", "1" if mask else "0")
    torch.manual_seed(0)
    rend = factory.build_renderer(wdepth=wdepth, device=torch.device("cuda:0"), precision="bf16")
    return Trainer(rend, B, torch.device("cuda:0"), conf=dict(warm_up_end=20, end_iter=300, anneal_end=40, extract_depth=wdepth,
                                                              depth_start_iter=-1))


@pytest.mark.gpu
@pytest.mark.parametrize("wdepth,compact,B", [(False, True, 512), (True, True, 512), (False, False, 256), (True, True, 200)])
def test_masked_step_is_bit_identical(monkeypatch, wdepth, compact, B):
    """Two Trainers in lockstep, one built under VDN_RELU_MASK=0 (_trainer sets the switch), one under the default."""
    import torch
    from vdn_train import synth
    from vdn_hip import layout
    for k in ("VDN_FG_COMPACT", "VDN_BG_COMPACT"):
        monkeypatch.setenv(k, "1" if compact else "0")
    dev = torch.device("cuda:0")
    seed = 5
    cams = synth.make_cameras(seed)
    gg = lambda x: torch.tensor(x).to(dev)
    trs = [_trainer(monkeypatch, m, wdepth, B) for m in (False, True)]
    assert not trs[0].engine.relu_mask and trs[1].engine.relu_mask
    feats = gg(synth.uniform(seed, "relu_mask/feats", (B, 96)).astype(np.float32)) if wdepth else None
    for it in range(6):
        o, d = synth.random_pixel_batch(seed, it, it % 40, B, cams=cams, crop=420)
        near, far = synth.near_far_from_sphere(o, d)
        t1, t2 = synth.jitter(seed, it, B)
        args = [gg(o), gg(d), gg(near), gg(far), gg(synth.target_colors(o, d, 0.5))]
        losses = [tr.train_step(*args, gt_feats=feats, t_rand=gg(t1), t_rand_out=gg(t2)).clone() for tr in trs]
        torch.cuda.synchronize()
        assert torch.equal(losses[0], losses[1]), (it, losses)
        e0, e1 = trs[0].engine, trs[1].engine
        assert torch.equal(e0.grad_flat, e1.grad_flat), it
        nq, n_fg = int(e1.w["bg_active"][1].item()), int(e1.w["fg_active"][1].item())
        assert nq == int(e0.w["bg_active"][1].item()) and n_fg == int(e0.w["fg_active"][1].item())
        # the chains' deltas over the valid rows
        planes = (("nf_dh", nq, 256, 8), ("nf_dv", nq, 128, 0), ("col_dh", n_fg, 256, 4)) + ((("vdn_dh", n_fg, 256, 4),) if wdepth else ())
        for k, rows, ld, nl in planes:
            for l in range(max(nl, 1)):
                a, b = (e.w[k][l] if nl else e.w[k] for e in (e0, e1))
                assert torch.equal(layout.from_pt32(a, rows, ld), layout.from_pt32(b, rows, ld)), (it, k, l)
        # the masks, decoded, are the saved planes' ReLU' on every valid row
        w = e1.w
        for l in range(8):
            ref = layout.from_pt32(w["nf_h"][l], nq, 256) > 0
            assert torch.equal(layout.mask_from_plane(w["nf_mask"][l], nq, 256), ref), (it, "nerf", l)
        assert torch.equal(layout.mask_from_plane(w["nf_mask_v"], nq, 128), layout.from_pt32(w["nf_hv"], nq, 128) > 0), it
        for net in ("col",) + (("vdn",) if wdepth else ()):
            for l in range(4):
                ref = layout.from_pt32(w[net + "_h"][l], n_fg, 256) > 0
                assert torch.equal(layout.mask_from_plane(w[net + "_mask"][l], n_fg, 256), ref), (it, net, l)
    assert torch.equal(trs[0].param_flat, trs[1].param_flat)
