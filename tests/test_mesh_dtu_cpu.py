"""The DTU steps of mesh evaluation, the parts that need no device: the ctypes mirror of VdnThinArgs and the argument checks of
vdn_thin_round / thin_points, observed_mask and above_plane on CPU tensors against numpy restatements of their formulas (exact: the
inputs are asserted to sit clear of every rounding decision first), and read_dtu_aux."""
import ctypes
import re

import numpy as np
import pytest
import torch

from vdn_hip import lib
from vdn_train import mesh_eval, meshio


def test_thin_argument_block_is_a_c_layout_and_declared():
    structs, funcs = lib.parse_header()
    assert funcs["vdn_thin_round"] == [ctypes.c_void_p, ctypes.c_void_p]
    # VdnThinArgs {4 pointers, int64, 5 float, 3 int32}
    T = lib.VdnThinArgs
    assert ctypes.sizeof(T) == 4 * 8 + 8 + 5 * 4 + 3 * 4 == 72
    assert [f for f, _ in structs["VdnThinArgs"]] == ["rec", "cell_start", "state", "undecided", "N", "lo_x", "lo_y", "lo_z", "h", "radius",
                                                      "nx", "ny", "nz"]
    assert (T.rec.offset, T.cell_start.offset, T.state.offset, T.undecided.offset, T.N.offset) == (0, 8, 16, 24, 32)
    assert (T.lo_x.offset, T.lo_z.offset, T.h.offset, T.radius.offset, T.nx.offset, T.ny.offset, T.nz.offset) == (40, 48, 52, 56, 60, 64, 68)
    # additive: the nearest-neighbour block and the version are what they were
    assert ctypes.sizeof(lib.VdnNnArgs) == 120
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28
    assert lib.call_value("vdn_abi_version") == 28
    assert hasattr(lib.load(), "vdn_thin_round")                 # exported, not only declared


def _thin_args():
    a = lib.VdnThinArgs()
    a.rec = a.cell_start = a.state = a.undecided = 8             # never dereferenced on the host
    a.N, a.h, a.radius, a.nx, a.ny, a.nz = 1, 1.0, 0.5, 1, 1, 1
    return a


def test_thin_round_refuses_bad_argument_blocks_before_any_launch():
    with pytest.raises(lib.VdnError):
        lib.call("vdn_thin_round", lib.VdnThinArgs(), None)
    for field, bad in (("rec", None), ("cell_start", None), ("state", None), ("undecided", None), ("N", 0), ("nx", 0), ("ny", 0), ("nz", -1),
                       ("h", 0.0), ("h", float("inf")), ("h", float("nan")), ("radius", 0.0), ("radius", -1.0), ("radius", float("inf")),
                       ("radius", float("nan"))):
        a = _thin_args()
        setattr(a, field, bad)
        with pytest.raises(lib.VdnError):
            lib.call("vdn_thin_round", a, None)
    # sizes beyond 32-bit indexing: status -10, checked on the host
    a = _thin_args()
    a.N = 1 << 31
    assert lib.try_call("vdn_thin_round", a, None) is False
    a = _thin_args()
    a.nx, a.ny, a.nz = 2048, 2048, 512
    assert lib.try_call("vdn_thin_round", a, None) is False


def test_thin_points_argument_errors_that_need_no_device():
    from vdn_hip import nn
    p = torch.zeros(5, 3)
    with pytest.raises(ValueError):
        nn.thin_points(p, 0.1)                                   # a CPU tensor
    with pytest.raises(ValueError):
        nn.thin_points(p[:, :2], 0.1)
    with pytest.raises(ValueError):
        nn.thin_points(p.long(), 0.1)
    for r in (0.0, -1.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="radius"):        # checked before the tensor: reached without a device
            nn.thin_points(p, r)
    with pytest.raises(ValueError, match="cell_size"):
        nn.thin_points(p, 0.1, cell_size=0.0)
    # the smallest cell edge covers radius + margin at that edge, in fp32
    for radius, extent in ((0.03, 1.0), (1.0, 1000.0), (1e-6, 500.0), (5.0, 0.0)):
        h = nn._thin_min_cell(radius, extent)
        assert h == float(np.float32(h)) and h >= radius + float(np.float32(nn.MARGIN_ULPS * 2.0 ** -24 * (extent + h)))
        assert h <= radius * (1 + 1e-5) + 4e-6 * extent


def test_the_round_loop_raises_instead_of_spinning():
    from vdn_hip import nn
    feed = lambda seq: iter(seq).__next__
    assert nn._rounds_to_fixpoint(feed([0]), 10) == 1
    assert nn._rounds_to_fixpoint(feed([9, 4, 1, 0]), 10) == 4
    for seq in ([10], [5, 5], [5, 6], [5, -1], [3, 2, 2]):       # nothing decided, a count that rises, a count that makes no sense
        calls = []
        it = iter(seq)
        with pytest.raises(RuntimeError):
            nn._rounds_to_fixpoint(lambda: calls.append(1) or next(it), 10)
        assert len(calls) == len(seq)                             # raised at once, not a round later


# ---- observed_mask / above_plane ------------------------------------------------------------------------------------------------
SHAPE, RES, PATCH = (16, 12, 20), 0.25, 1.5
BB = np.float32([[-2.0, 1.0, 0.5], [-2.0 + 16 * 0.25, 1.0 + 12 * 0.25, 0.5 + 20 * 0.25]])
PLANE = (0.3, -0.5, 0.8, -0.9)


def dtu_inputs():
    rng = np.random.default_rng(11)
    lo, hi = BB[0].astype(np.float64), BB[1].astype(np.float64)
    parts = [rng.uniform(lo - 0.3, hi + 0.3, size=(3000, 3))]                         # around the grid
    for axis in range(3):
        for side in (0, 1):
            band = rng.uniform(lo - 0.2, hi + 0.2, size=(200, 3))                     # in the patch band of one face ...
            band[:, axis] = (hi[axis] + rng.uniform(0.3, 2 * PATCH - 0.01, 200)) if side else (lo[axis] - rng.uniform(0.3, PATCH - 0.01, 200))
            far = rng.uniform(lo - 0.2, hi + 0.2, size=(100, 3))                      # ... and outside that face's bound
            far[:, axis] = (hi[axis] + 2 * PATCH + rng.uniform(0.01, 3.0, 100)) if side else (lo[axis] - PATCH - rng.uniform(0.01, 3.0, 100))
            parts += [band, far]
    parts.append(rng.uniform(lo - 4.0, hi + 6.0, size=(176, 3)))                      # off edges and corners
    edge = rng.uniform(lo, hi, size=(24, 3))                                          # at bb[1] + 2 patch exactly (an excluded bound),
    for k in range(24):                                                               # and at bb[0] - patch exactly (an included one)
        edge[k, k % 3] = float(BB[1][k % 3] + np.float32(2.0) * np.float32(PATCH)) if k < 12 else float(BB[0][k % 3] - np.float32(PATCH))
    parts.append(edge)
    p = np.concatenate(parts)
    t = (p - lo) / RES                                                                # of 15 000 random coordinates a few land next to a
    p = np.where(np.abs(t - np.floor(t) - 0.5) < 1e-3, p + 0.01 * RES, p).astype(np.float32)      # half-integer: moved off it
    assert p.shape == (5000, 3)
    mask = rng.uniform(size=SHAPE) < 0.5
    return p, mask


def np_observed(p, mask, bb, res, patch):
    lo = bb[0] - np.float32(patch)
    hi = bb[1] + np.float32(2.0) * np.float32(patch)
    inbound = (p >= lo).all(1) & (p < hi).all(1)
    g = np.rint((p - bb[0]) / np.float32(res))
    assert g.dtype == np.float32
    inside = ((g >= 0) & (g < np.float32(mask.shape))).all(1)
    gi = np.where(inside[:, None], g, 0).astype(np.int64)
    return inbound, inbound & inside & (mask[gi[:, 0], gi[:, 1], gi[:, 2]] != 0)


def test_observed_mask_and_above_plane_match_the_formulas_exactly():
    p, mask = dtu_inputs()
    # no decision hinges on rounding: no voxel coordinate near a half-integer, no plane value near 0
    t = (p.astype(np.float64) - BB[0].astype(np.float64)) / RES
    assert np.abs(t - np.floor(t) - 0.5).min() > 1e-4
    pv = PLANE[0] * p[:, 0].astype(np.float64) + PLANE[1] * p[:, 1].astype(np.float64) + PLANE[2] * p[:, 2].astype(np.float64) + PLANE[3]
    assert np.abs(pv).min() > 1e-9
    want_in, want_obs = np_observed(p, mask, BB, RES, PATCH)
    # every region is populated: outside, in the band only, inside and observed, inside and not observed, and the exact bounds
    assert 0 < want_obs.sum() < want_in.sum() < len(p)
    inside_box = ((p >= BB[0]) & (p < BB[1])).all(1)
    assert (want_in & ~inside_box).sum() > 500 and (inside_box & ~want_obs).sum() > 500
    assert not want_in[-24:-12].any() and want_in[-12:].all()
    for m in (mask, mask.astype(np.uint8) * 255):
        got_in, got_obs = mesh_eval.observed_mask(torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(BB), RES, PATCH)
        assert got_in.dtype == got_obs.dtype == torch.bool
        assert np.array_equal(got_in.numpy(), want_in) and np.array_equal(got_obs.numpy(), want_obs)
    # arrays in place of tensors, doubles in place of fp32 points
    got_in, got_obs = mesh_eval.observed_mask(torch.from_numpy(p).double(), mask, BB.tolist(), RES, PATCH)
    assert np.array_equal(got_in.numpy(), want_in) and np.array_equal(got_obs.numpy(), want_obs)
    above = mesh_eval.above_plane(torch.from_numpy(p), PLANE)
    assert above.dtype == torch.bool and np.array_equal(above.numpy(), pv > 0) and 500 < (pv > 0).sum() < 4500
    assert np.array_equal(mesh_eval.above_plane(torch.from_numpy(p), torch.tensor(PLANE, dtype=torch.float64)).numpy(), pv > 0)
    assert np.array_equal(mesh_eval.above_plane(torch.from_numpy(p), np.float64(PLANE).reshape(1, 4)).numpy(), pv > 0)


def test_observed_mask_and_above_plane_argument_errors():
    p, mask = dtu_inputs()
    tp = torch.from_numpy(p)
    for args in ((p, mask, BB, RES), (tp[:, :2], mask, BB, RES), (tp, mask[0], BB, RES), (tp, mask.astype(np.float32), BB, RES),
                 (tp, mask, BB[0], RES), (tp, mask, BB, 0.0), (tp, mask, BB, float("nan")), (tp, mask, BB, RES, -1.0)):
        with pytest.raises(ValueError):
            mesh_eval.observed_mask(*args)
    for args in ((p, PLANE), (tp, PLANE[:3]), (tp, (1.0, 0.0, float("nan"), 0.0)), (tp[:, :2], PLANE)):
        with pytest.raises(ValueError):
            mesh_eval.above_plane(*args)
    empty = mesh_eval.observed_mask(tp[:0], mask, BB, RES)
    assert empty[0].shape == empty[1].shape == (0,) and mesh_eval.above_plane(tp[:0], PLANE).shape == (0,)


def test_evaluate_mesh_still_refuses_cpu_tensors_with_the_new_arguments():
    v, t, g = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(5, 3)
    with pytest.raises(ValueError):
        mesh_eval.evaluate_mesh(v, t, g, 0.1, 0.5, thin=0.1, obs_mask=(np.ones((2, 2, 2), bool), BB, RES), plane=PLANE)


# ---- read_dtu_aux ---------------------------------------------------------------------------------------------------------------
def _aux():
    rng = np.random.default_rng(5)
    return {"ObsMask": rng.uniform(size=(7, 5, 9)) < 0.4, "BB": BB.astype(np.float64), "Res": np.float64(RES), "P": np.float64(PLANE)}


def _check_aux(out, want, keys):
    assert sorted(out) == sorted(keys)
    if "ObsMask" in keys:
        assert out["ObsMask"].dtype == np.bool_ and np.array_equal(out["ObsMask"], want["ObsMask"])
    if "BB" in keys:
        assert out["BB"].dtype == np.float32 and out["BB"].shape == (2, 3) and np.array_equal(out["BB"], want["BB"].astype(np.float32))
    if "Res" in keys:
        assert type(out["Res"]) is float and out["Res"] == float(want["Res"])
    if "P" in keys:
        assert out["P"].dtype == np.float64 and out["P"].shape == (4,) and np.array_equal(out["P"], want["P"])


def test_read_dtu_aux_round_trips_an_npz(tmp_path):
    want = _aux()
    np.savez(tmp_path / "all.npz", other=np.arange(3), **want)
    _check_aux(meshio.read_dtu_aux(str(tmp_path / "all.npz")), want, ("ObsMask", "BB", "Res", "P"))
    np.savez(tmp_path / "plane.npz", P=want["P"].reshape(1, 4))
    _check_aux(meshio.read_dtu_aux(tmp_path / "plane.npz"), want, ("P",))
    np.savez(tmp_path / "mask.npz", ObsMask=want["ObsMask"].astype(np.uint8), BB=want["BB"].astype(np.float32), Res=np.float32([[RES]]))
    _check_aux(meshio.read_dtu_aux(str(tmp_path / "mask.npz")), want, ("ObsMask", "BB", "Res"))
    assert meshio.read_dtu_aux(_save(tmp_path / "none.npz", other=np.arange(3))) == {}


def _save(path, **arrays):
    np.savez(path, **arrays)
    return str(path)


def test_read_dtu_aux_round_trips_a_mat(tmp_path):
    sio = pytest.importorskip("scipy.io")
    want = _aux()
    sio.savemat(str(tmp_path / "all.mat"), {"ObsMask": want["ObsMask"], "BB": want["BB"], "Res": want["Res"], "P": want["P"].reshape(4, 1)})
    _check_aux(meshio.read_dtu_aux(str(tmp_path / "all.mat")), want, ("ObsMask", "BB", "Res", "P"))
    sio.savemat(str(tmp_path / "plane.mat"), {"P": want["P"]})
    _check_aux(meshio.read_dtu_aux(str(tmp_path / "plane.mat")), want, ("P",))


def test_read_dtu_aux_refuses_a_v73_mat_with_advice(tmp_path):
    pytest.importorskip("scipy.io")
    # the 128-byte header of a MATLAB v7.3 (HDF5) file: text, subsystem offset, version 0x0200, endian mark
    head = b"MATLAB 7.3 MAT-file, Platform: GLNXA64".ljust(116, b" ") + b"\0" * 8 + b"\x00\x02" + b"IM"
    (tmp_path / "v73.mat").write_bytes(head + b"\0" * 512)
    with pytest.raises(ValueError, match="v7.3"):
        meshio.read_dtu_aux(str(tmp_path / "v73.mat"))


def test_read_dtu_aux_says_when_scipy_is_missing(tmp_path, monkeypatch):
    import sys
    (tmp_path / "x.mat").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "scipy.io", None)           # `from scipy.io import loadmat` now raises ImportError
    monkeypatch.setitem(sys.modules, "scipy", None)
    with pytest.raises(ValueError, match="scipy"):
        meshio.read_dtu_aux(str(tmp_path / "x.mat"))


def test_read_dtu_aux_refuses_wrong_shapes(tmp_path):
    want = _aux()
    bad = {"mask2d": {"ObsMask": want["ObsMask"][0]}, "mask_float": {"ObsMask": want["ObsMask"].astype(np.float32)},
           "bb_t": {"BB": want["BB"].T}, "bb_flat": {"BB": want["BB"].reshape(6)}, "res2": {"Res": np.float64([0.1, 0.2])},
           "p3": {"P": want["P"][:3]}, "p5": {"P": np.zeros(5)}, "p3d": {"P": want["P"].reshape(1, 2, 2)}, "bb_bool": {"BB": np.ones((2, 3), bool)}}
    for name, arrays in bad.items():
        with pytest.raises(ValueError):
            meshio.read_dtu_aux(_save(tmp_path / (name + ".npz"), **arrays))
    (tmp_path / "aux.txt").write_text("ObsMask")
    with pytest.raises(ValueError):
        meshio.read_dtu_aux(str(tmp_path / "aux.txt"))
