"""Mesh alignment, the parts that need no device: the declaration and argument checks of vdn_icp_round, solve_sim3 on sums formed in
numpy, align_cameras / pose_errors on a synthetic ring of cameras, store_current_pose, and the float64 model of the ICP loop
(tests/align_model.py) on the three cases the device tests run - a case the model itself failed could not pass there.

Tolerances. solve_sim3 / align_cameras: float64 closed forms on exact correspondences, recovery to 1e-12. Pose errors: 1e-9, degrees
and lengths alike (pose_errors takes the angle by atan2, which keeps its digits at 0). The model ICP: every round matches exactly the 1 500 inliers and the
transform is recovered to 1e-6 (the model reaches about 1e-9: the fp32 rounding of the stored source, averaged over 1 500 points)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import align_model as am
from vdn_hip import lib, nn
from vdn_train import mesh_align


def _known(seed=0, s=1.7):
    rng = np.random.default_rng(seed)
    R = am.rotation(rng.normal(size=3), 37.0)
    return s, R, rng.normal(size=3)


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_round_and_the_library_exports_it():
    structs, funcs = lib.parse_header()
    assert funcs["vdn_icp_round"] == [ctypes.c_void_p, ctypes.c_void_p] and funcs["vdn_icp_round_blocks"] == [ctypes.c_int64]
    text = open(lib.HEADER).read()
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", text).group(1)) == 28                 # additive: no bump
    l = lib.load()
    assert hasattr(l, "vdn_icp_round") and hasattr(l, "vdn_icp_round_blocks") and l.vdn_abi_version() == 28
    # {8 pointers, 12 doubles, 3 int64, 6 floats, 4 int32}
    A = lib.VdnIcpArgs
    assert ctypes.sizeof(A) == 8 * 8 + 12 * 8 + 3 * 8 + 6 * 4 + 4 * 4 == 224
    assert (A.result.offset, A.m00.offset, A.m23.offset, A.N.offset, A.partials_rows.offset, A.lo_x.offset, A.max_dist.offset, A.nx.offset) == \
        (56, 64, 152, 160, 176, 184, 204, 208)
    # the slots' names and count
    slots = {k: int(v) for k, v in re.findall(r"#define\s+VDN_ICP_(\w+)\s+(\d+)", text)}
    assert slots == {"N": 0, "P": 1, "Q": 4, "PP": 7, "QQ": 8, "QP": 9, "RES": 18, "SUMS": 19}
    assert (nn.ICP_N, nn.ICP_P, nn.ICP_Q, nn.ICP_PP, nn.ICP_QQ, nn.ICP_QP, nn.ICP_RES, nn.ICP_SUMS) == (0, 1, 4, 7, 8, 9, 18, 19)
    assert (am.S_N, am.S_P, am.S_Q, am.S_PP, am.S_QQ, am.S_QP, am.S_RES, am.N_SUMS) == (0, 1, 4, 7, 8, 9, 18, 19)
    assert lib.call_value("vdn_icp_round_blocks", 1) == 1 and lib.call_value("vdn_icp_round_blocks", 256) == 1
    assert lib.call_value("vdn_icp_round_blocks", 257) == 2 and lib.call_value("vdn_icp_round_blocks", 0) == 0
    assert lib.call_value("vdn_icp_round_blocks", 1 << 31) == 0


def _valid_block():
    """every check passes on this block; the pointers are never dereferenced on the host"""
    a = lib.VdnIcpArgs()
    a.src = a.ref = a.cell_start = a.partials = a.result = 8
    a.m00 = a.m11 = a.m22 = 1.0
    a.N, a.R, a.partials_rows = 300, 10, 2
    a.h, a.margin, a.max_dist = 1.0, 0.0, 1.0
    a.nx = a.ny = a.nz = 1
    return a


def _status(a):
    return getattr(lib.load(), "vdn_icp_round")(ctypes.byref(a), None)


def test_malformed_argument_blocks_are_refused_before_any_launch():
    with pytest.raises(lib.VdnError):
        lib.call("vdn_icp_round", lib.VdnIcpArgs(), None)
    assert lib.load().vdn_icp_round(None, None) == -1
    edits = {"src": 0, "ref": 0, "cell_start": 0, "partials": 0, "result": 0, "N": 0, "R": 0, "nx": 0, "ny": -1, "nz": 0, "h": 0.0,
             "margin": -1.0, "max_dist": -1.0, "partials_rows": 1, "m13": float("nan"), "m00": float("inf")}
    for field, value in edits.items():
        a = _valid_block()
        setattr(a, field, value)
        assert _status(a) == -1, field
    for field in ("h", "margin", "max_dist"):
        a = _valid_block()
        setattr(a, field, float("nan"))
        assert _status(a) == -1, field
    # sizes beyond 32-bit indexing: -10, as vdn_nn_query
    a = _valid_block()
    a.N, a.partials_rows = 1 << 31, 1 << 40
    assert _status(a) == -10 and lib.try_call("vdn_icp_round", a, None) is False
    a = _valid_block()
    a.R = 1 << 31
    assert _status(a) == -10
    a = _valid_block()
    a.nx, a.ny, a.nz = 2048, 2048, 512
    assert _status(a) == -10


def test_python_argument_errors_that_need_no_device():
    g = torch.zeros(5, 3)
    with pytest.raises(ValueError):
        nn.icp(g, g, max_dist=1.0)                            # CPU tensors
    with pytest.raises(ValueError):
        nn.IcpRound(g, None)
    with pytest.raises(ValueError):
        nn.sim3_matrix(1.0, np.eye(2), np.zeros(3))
    with pytest.raises(ValueError):
        nn.sim3_matrix(float("nan"), np.eye(3), np.zeros(3))
    with pytest.raises(ValueError):
        mesh_align.align_mesh(g, None, g, 0.1, 0.5)           # CPU tensors
    from vdn_train import mesh_eval
    with pytest.raises(ValueError):
        mesh_eval.evaluate_mesh(g, None, g, 0.1, 0.5, align=(1.0, np.eye(3), np.zeros(3)))


# ---- the solve ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [True, False])
def test_solve_sim3_recovers_a_known_transform(scale):
    s, R, t = _known(1, 1.7 if scale else 1.0)
    p = np.random.default_rng(2).normal(size=(200, 3))
    q = s * p @ R.T + t
    for solve in (nn.solve_sim3, am.solve_sim3):
        s1, R1, t1 = solve(am.sums_of_pairs(p, q), scale)
        assert abs(s1 - s) <= 1e-12 * s and np.abs(R1 - R).max() <= 1e-12 and np.abs(t1 - t).max() <= 1e-12
        assert (s1 == 1.0) or scale
    # scale=False on pairs that DO differ in scale: a rigid fit, s exactly 1, the same rotation
    q2 = 1.3 * p @ R.T + t
    s1, R1, t1 = nn.solve_sim3(am.sums_of_pairs(p, q2), scale=False)
    assert s1 == 1.0 and np.abs(R1 - R).max() <= 1e-12
    # a device tensor-like input: a torch tensor of the sums
    s1, R1, t1 = nn.solve_sim3(torch.from_numpy(am.sums_of_pairs(p, q)), scale)
    assert np.abs(R1 - R).max() <= 1e-12


def test_solve_sim3_keeps_a_proper_rotation_on_a_mirrored_target():
    s, R, t = _known(3, 1.0)
    p = np.random.default_rng(4).normal(size=(300, 3)) * [1.0, 0.7, 0.05]       # nearly flat: the mirror image fits almost as well
    q = (p * [1.0, 1.0, -1.0]) @ R.T + t
    for solve in (nn.solve_sim3, am.solve_sim3):
        s1, R1, t1 = solve(am.sums_of_pairs(p, q), True)
        assert abs(np.linalg.det(R1) - 1.0) <= 1e-12 and np.abs(R1 @ R1.T - np.eye(3)).max() <= 1e-12
        assert s1 > 0
    # and an exact mirror of a full-rank cloud
    p = np.random.default_rng(5).normal(size=(50, 3))
    s1, R1, t1 = nn.solve_sim3(am.sums_of_pairs(p, p * [-1.0, 1.0, 1.0]), True)
    assert abs(np.linalg.det(R1) - 1.0) <= 1e-12


def test_solve_sim3_refuses_degenerate_pairs():
    p = np.random.default_rng(6).normal(size=(10, 3))
    with pytest.raises(ValueError):
        nn.solve_sim3(am.sums_of_pairs(p[:2], p[:2]))                          # fewer than 3 pairs
    with pytest.raises(ValueError):
        nn.solve_sim3(np.zeros(19))                                            # none
    line = np.outer(np.linspace(-1, 1, 20), [1.0, 2.0, 3.0]) + [0.5, 0.0, -0.5]
    with pytest.raises(ValueError):
        nn.solve_sim3(am.sums_of_pairs(line, line))                            # collinear
    same = np.tile([0.3, 0.2, 0.1], (5, 1))
    with pytest.raises(ValueError):
        nn.solve_sim3(am.sums_of_pairs(same, same))                            # one point
    with pytest.raises(ValueError):
        nn.solve_sim3(np.zeros(18))


# ---- cameras --------------------------------------------------------------------------------------------------------------------
def _ring(n=12):
    """n cameras on a tilted ring looking at the origin -> [n,4,4] camera-to-world"""
    out = []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        c = np.array([2.0 * math.cos(a), 2.0 * math.sin(a), 0.6 + 0.3 * math.sin(2 * a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, c
        out.append(m)
    return np.stack(out)


def _moved(c2w, s, R, t):
    out = c2w.copy()
    out[:, :3, :3] = R @ c2w[:, :3, :3]
    out[:, :3, 3] = s * c2w[:, :3, 3] @ R.T + t
    return out


def test_align_cameras_and_pose_errors_on_a_ring_of_cameras():
    est = _ring()
    s, R, t = _known(7, 2.5)
    ref = _moved(est, s, R, t)
    s1, R1, t1 = mesh_align.align_cameras(est, ref)
    assert abs(s1 - s) <= 1e-12 * s and np.abs(R1 - R).max() <= 1e-12 and np.abs(t1 - t).max() <= 1e-12
    e = mesh_align.pose_errors(torch.from_numpy(est), ref, (s1, R1, t1))                    # tensors or arrays
    assert e["rotation_deg"].shape == e["position"].shape == (12,)
    assert e["rotation_deg_max"] <= 1e-9 and e["position_max"] <= 1e-9 and e["position_rmse"] <= 1e-9
    # rigid: the same cameras at scale 1
    ref1 = _moved(est, 1.0, R, t)
    s1, R1, t1 = mesh_align.align_cameras(est, ref1, scale=False)
    assert s1 == 1.0 and np.abs(R1 - R).max() <= 1e-12 and np.abs(t1 - t).max() <= 1e-12
    # one camera off by a known 2 degrees and a known shift, errors measured with the TRUE alignment: exactly those figures
    bad = est.copy()
    bad[5, :3, :3] = am.rotation((0.3, -1.0, 0.5), 2.0) @ est[5, :3, :3]
    shift = np.array([0.01, -0.02, 0.02])
    bad[5, :3, 3] += shift
    e = mesh_align.pose_errors(bad, ref, (s, R, t))
    want_pos = s * np.linalg.norm(shift)
    assert abs(e["rotation_deg"][5] - 2.0) <= 1e-9 and abs(e["position"][5] - want_pos) <= 1e-9
    others = np.arange(12) != 5
    assert e["rotation_deg"][others].max() <= 1e-9 and e["position"][others].max() <= 1e-9
    assert abs(e["rotation_deg_max"] - 2.0) <= 1e-9 and abs(e["rotation_deg_mean"] - 2.0 / 12) <= 1e-9 and e["rotation_deg_median"] <= 1e-9
    assert abs(e["position_max"] - want_pos) <= 1e-9 and abs(e["position_mean"] - want_pos / 12) <= 1e-9
    assert abs(e["position_rmse"] - want_pos / math.sqrt(12)) <= 1e-9 and e["position_median"] <= 1e-9


def test_align_cameras_refusals():
    est = _ring()
    with pytest.raises(ValueError):
        mesh_align.align_cameras(est[:2], est[:2])                             # N < 3
    with pytest.raises(ValueError):
        mesh_align.align_cameras(est, est[:11])                                # a shape mismatch
    with pytest.raises(ValueError):
        mesh_align.align_cameras(est[:, :3, :3], est[:, :3, :3])
    line = est.copy()
    line[:, :3, 3] = np.outer(np.linspace(0, 1, 12), [1.0, -2.0, 0.5]) + [3.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        mesh_align.align_cameras(line, est)                                    # collinear centres
    with pytest.raises(ValueError):
        mesh_align.pose_errors(est, est[:11], (1.0, np.eye(3), np.zeros(3)))


def test_store_current_pose_writes_the_reference_file(tmp_path):
    from dpt_models.poses import LearnPose, LearnIntrin, LearnableRays
    init = torch.from_numpy(_ring(5).astype(np.float32))
    net = LearnPose(5, True, True, init_c2w=init)
    with torch.no_grad():
        net.r.copy_(torch.from_numpy(np.random.default_rng(8).normal(size=(5, 3)).astype(np.float32) * 0.05))
        net.t.copy_(torch.from_numpy(np.random.default_rng(9).normal(size=(5, 3)).astype(np.float32) * 0.1))
    net.train()
    want = torch.stack([net(i) for i in range(5)]).detach().numpy()
    path = mesh_align.store_current_pose(net, str(tmp_path), 1234)
    assert path == os.path.join(str(tmp_path), "cam_poses", "pose_001234.npy") and os.path.exists(path)
    got = np.load(path)
    assert got.dtype == np.float32 and got.shape == (5, 4, 4) and np.array_equal(got, want)
    assert net.training                                                         # left as it was
    poses = mesh_align.current_poses(net)
    assert torch.is_tensor(poses) and not poses.requires_grad and np.array_equal(poses.numpy(), want)

    class Pixels:
        H = W = 4
        device = "cpu"
    rays = LearnableRays(net, LearnIntrin(4, 4, False), Pixels())
    assert np.array_equal(rays.current_poses().numpy(), want)
    path = rays.store_current_pose(str(tmp_path), 7)
    assert path.endswith(os.path.join("cam_poses", "pose_000007.npy")) and np.array_equal(np.load(path), want)
    assert np.array_equal(mesh_align.load_estimated_poses(path), want.astype(np.float64))
    # a pose checkpoint gives the same cameras
    ck = str(tmp_path / "pnf_000007.pth")
    torch.save({"pose_param_net": net.state_dict()}, ck)
    assert np.array_equal(mesh_align.load_estimated_poses(ck), want.astype(np.float64))


# ---- the model of the loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(am.CASES))
def test_the_model_icp_converges_on_the_cases(name):
    c = am.case(name)
    assert c["src"].dtype == c["ref"].dtype == np.float32 and c["src"].shape == (1650, 3) and c["ref"].shape == (4000, 3)
    m = am.case_model(name, 1e-10)
    print(name, "rounds", m["rounds"], "errors", am.pose_error(m, c["truth"]), "rms", m["rms"][0], m["rms"][-1])
    assert m["converged"] and m["rounds"] <= 60
    # every round matched exactly the 1 500 inliers: no outlier on the radius-3 sphere is ever within max_dist
    assert all(n == 1500 for n in m["n_pairs"])
    assert all((d[:1500] <= c["max_dist"]).all() and (d[1500:] > 2.0).all() for d in m["dists"])
    eR, et, es = am.pose_error(m, c["truth"])
    assert eR <= 1e-6 and et <= 1e-6 and es <= 1e-6
    assert c["scale"] or m["s"] == 1.0
    assert m["rms"][-1] <= 1e-6 and m["rms"][0] > 1e-3 and m["threshold"] == [c["max_dist"]] * m["rounds"]


def test_the_model_round_forms_y_by_the_documented_expression():
    c = am.case("rigid")
    M = am.matrix(*c["truth"])
    y = am.transform_y(M, c["src"])
    p = c["src"].astype(np.float64)
    for r in range(3):
        assert np.array_equal(y[:, r], (((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]).astype(np.float32))
    r = am.round_model(c["src"], c["ref"], M, c["max_dist"])
    assert r["sums"][am.S_N] == 1500 and np.array_equal(r["idx"][:1500], c["pick"])
    s, R, t = am.solve_sim3(r["sums"], False)
    assert np.abs(R - c["truth"][1]).max() <= 1e-6 and np.abs(t - c["truth"][2]).max() <= 1e-6


def test_camera_files_give_the_start_of_the_tools(tmp_path):
    """tools/align_mesh.py's camera path: pose_*.npy in the object frame + cameras_sphere.npz -> the start transform and the errors"""
    import argparse
    import sys
    from vdn_train.dataset import write_cameras_npz
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import align_mesh as tool
    obj = _ring(8)                                                              # the cameras in the normalised object frame
    scale_mat = np.diag([150.0, 150.0, 150.0, 1.0])
    scale_mat[:3, 3] = [20.0, -35.0, 600.0]
    world = mesh_align.poses_to_world(obj, scale_mat)
    assert np.allclose(world[:, :3, 3], 150.0 * obj[:, :3, 3] + scale_mat[:3, 3], rtol=0, atol=1e-12) and np.array_equal(world[:, :3, :3], obj[:, :3, :3])
    K = np.array([[900.0, 0.0, 320.0], [0.0, 900.0, 240.0], [0.0, 0.0, 1.0]])
    world_mats = []
    for c2w in world:
        w = np.eye(4)
        w[:3, :4] = K @ np.linalg.inv(c2w)[:3, :4]
        world_mats.append(w)
    npz = str(tmp_path / "cameras_sphere.npz")
    write_cameras_npz(npz, [str(i) for i in range(8)], world_mats, [scale_mat] * 8)
    ref, sm = mesh_align.load_reference_poses(npz)
    assert np.array_equal(sm, scale_mat) and np.abs(ref - world).max() <= 1e-3        # (the loader's poses are fp32: 2^-24 of 600)
    # the estimate: the object-frame cameras, drifted by a similarity
    s, R, t = 1.1, am.rotation((0.2, 1.0, -0.4), 12.0), np.array([0.05, -0.1, 0.02])
    est = _moved(obj, s, R, t)
    pose_file = str(tmp_path / "pose_000100.npy")
    np.save(pose_file, est.astype(np.float32))
    a = argparse.Namespace(cameras_est=pose_file, cameras_ref=npz, est_frame="object", scale=True)
    init, cams = tool.camera_start(a)
    rep = tool.pose_report(cams, init)
    assert rep["position_max"] <= 1e-3 and rep["rotation_deg_max"] <= 1e-3 and abs(init[0] * s - 1.0) <= 1e-5
    assert isinstance(rep["rotation_deg"], list) and len(rep["position"]) == 8
    a.cameras_ref = None
    with pytest.raises(SystemExit):
        tool.camera_start(a)
    a.cameras_est = None
    assert tool.camera_start(a) == (None, None)
