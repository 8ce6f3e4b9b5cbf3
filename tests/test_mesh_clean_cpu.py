"""Mesh cleaning, the parts that need no device: the ctypes mirrors of the new argument blocks and their host-side refusals, the
component policy and the vote rule on hand-written tables, SceneData.projection_matrices, the argument errors of the Python layer,
and the numpy restatements the GPU tests compare against (cross-checked against scipy where it imports)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from vdn_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vdn_cc_union", "vdn_cc_flatten", "vdn_tri_area", "vdn_mask_dilate", "vdn_mask_votes", "vdn_mesh_filter_mark",
                "vdn_mesh_filter_remap")


# ---- numpy restatements (test_gpu_mesh_clean.py imports them) -------------------------------------------------------------------
def np_labels(tri, V):
    """Plain union-find, then the canonical label of each vertex: the minimum index of its set."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in np.asarray(tri).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    root = np.array([find(v) for v in range(V)], dtype=np.int64)
    low = np.full(V, V, dtype=np.int64)
    np.minimum.at(low, root, np.arange(V))
    return low[root].astype(np.int32) if V else np.zeros(0, np.int32)


def np_dilate(m, r):
    """Brute-force window maximum, pixels outside the image = 0."""
    N, H, W = m.shape
    out = np.zeros_like(m)
    for y in range(H):
        for x in range(W):
            out[:, y, x] = m[:, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].reshape(N, -1).max(axis=1)
    return out


def np_project(v32, P):
    """float64 projection of fp32 vertices -> (u [N,V], v [N,V], w [N,V])."""
    x = np.concatenate([np.asarray(v32, np.float32).astype(np.float64), np.ones((len(v32), 1))], axis=1)
    q = np.einsum("nij,vj->niv", np.asarray(P, np.float64), x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], q[:, 2]


def np_votes(v32, P, masks):
    u, v, w = np_project(v32, P)
    N, H, W = masks.shape
    with np.errstate(invalid="ignore"):
        px, py = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = (w > 0) & np.isfinite(u) & np.isfinite(v) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    ix, iy = np.where(inside, px, 0).astype(np.int64), np.where(inside, py, 0).astype(np.int64)
    hit = inside & (masks[np.arange(N)[:, None], iy, ix] != 0)
    return inside.sum(axis=0).astype(np.int32), hit.sum(axis=0).astype(np.int32)


def test_restatements_agree_with_scipy():
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    for V, F in ((1, 0), (40, 13), (300, 257)):
        tri = rng.integers(0, V, (F, 3))
        e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]]])
        g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
        _, lab = csgraph.connected_components(g, directed=False)
        low = np.full(V, V)
        np.minimum.at(low, lab, np.arange(V))
        assert np.array_equal(np_labels(tri, V), low[lab])
    m = (rng.random((2, 9, 11)) > 0.8).astype(np.uint8) * 255
    for r in (0, 1, 3, 12):
        want = np.stack([ndimage.grey_dilation(p, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0) for p in m])
        assert np.array_equal(np_dilate(m, r), want)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_argument_blocks_are_c_layouts_and_declared():
    structs, funcs = lib.parse_header()
    for fn in ENTRY_POINTS:
        assert funcs[fn] == [ctypes.c_void_p, ctypes.c_void_p]
    # VdnCcArgs {4 pointers, 2 int64, 2 int32}
    C = lib.VdnCcArgs
    assert ctypes.sizeof(C) == 4 * 8 + 2 * 8 + 2 * 4 == 56
    assert (C.triangles.offset, C.parent.offset, C.label.offset, C.error.offset, C.V.offset, C.F.offset, C.index_bytes.offset) == (0, 8, 16, 24, 32, 40, 48)
    # VdnTriAreaArgs {4 pointers, 2 int64, 2 int32}
    A = lib.VdnTriAreaArgs
    assert ctypes.sizeof(A) == 56 and (A.vertices.offset, A.area.offset, A.error.offset, A.V.offset, A.index_bytes.offset) == (0, 16, 24, 32, 48)
    # VdnMaskDilateArgs {3 pointers, int64, 4 int32}
    D = lib.VdnMaskDilateArgs
    assert ctypes.sizeof(D) == 3 * 8 + 8 + 4 * 4 == 48
    assert (D.src.offset, D.scratch.offset, D.dst.offset, D.N.offset, D.H.offset, D.W.offset, D.radius.offset) == (0, 8, 16, 24, 32, 36, 40)
    # VdnMaskVotesArgs {5 pointers, 2 int64, 2 int32}
    M = lib.VdnMaskVotesArgs
    assert ctypes.sizeof(M) == 5 * 8 + 2 * 8 + 2 * 4 == 64
    assert (M.P.offset, M.masks.offset, M.n_in_image.offset, M.n_in_mask.offset, M.V.offset, M.N.offset, M.H.offset, M.W.offset) == (8, 16, 24, 32, 40, 48, 56, 60)
    # VdnMeshFilterArgs {9 pointers, 3 int64, 2 int32}
    R = lib.VdnMeshFilterArgs
    assert ctypes.sizeof(R) == 9 * 8 + 3 * 8 + 2 * 4 == 104
    assert (R.keep_face.offset, R.keep_vertex.offset, R.face_alive.offset, R.vertex_used.offset, R.error.offset, R.face_offsets.offset,
            R.vertex_new.offset, R.out_triangles.offset, R.V.offset, R.F.offset, R.F_out.offset, R.index_bytes.offset) == (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96)
    assert int(re.search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28     # additive: no bump


def test_new_entry_points_are_exported_at_abi_28():
    so = lib.load()
    for fn in ENTRY_POINTS:
        assert getattr(so, fn) is not None
    assert lib.call_value("vdn_abi_version") == 28


def test_new_entry_points_refuse_empty_argument_blocks():
    for name, args in (("vdn_cc_union", lib.VdnCcArgs()), ("vdn_cc_flatten", lib.VdnCcArgs()), ("vdn_tri_area", lib.VdnTriAreaArgs()),
                       ("vdn_mask_dilate", lib.VdnMaskDilateArgs()), ("vdn_mask_votes", lib.VdnMaskVotesArgs()),
                       ("vdn_mesh_filter_mark", lib.VdnMeshFilterArgs()), ("vdn_mesh_filter_remap", lib.VdnMeshFilterArgs())):
        with pytest.raises(lib.VdnError):
            lib.call(name, args, None)
        with pytest.raises(lib.VdnError):
            lib.call(name, None, None)
    # one missing pointer or a bad index width is refused too
    c = lib.VdnCcArgs()
    c.triangles = c.parent = c.label = c.error = 8
    c.V, c.F, c.index_bytes = 3, 1, 2
    with pytest.raises(lib.VdnError):
        lib.call("vdn_cc_union", c, None)
    d = lib.VdnMaskDilateArgs()
    d.src = d.dst = 8
    d.scratch, d.N, d.H, d.W, d.radius = 16, 1, 4, 4, -1
    with pytest.raises(lib.VdnError):
        lib.call("vdn_mask_dilate", d, None)
    d.radius, d.scratch = 1, 8                                 # the scratch plane must be one of its own
    with pytest.raises(lib.VdnError):
        lib.call("vdn_mask_dilate", d, None)


def test_sizes_beyond_32_bit_indexing_are_status_minus_10():
    """checked on the host before anything is launched (the pointers are never dereferenced there)"""
    big = 1 << 31
    c = lib.VdnCcArgs()
    c.triangles = c.parent = c.label = c.error = 8
    c.index_bytes = 8
    for V, F in ((big, 1), (3, big)):
        c.V, c.F = V, F
        assert lib.try_call("vdn_cc_union", c, None) is False and lib.try_call("vdn_cc_flatten", c, None) is False
    a = lib.VdnTriAreaArgs()
    a.vertices = a.triangles = a.area = a.error = 8
    a.index_bytes = 4
    for V, F in ((big, 1), (3, big)):
        a.V, a.F = V, F
        assert lib.try_call("vdn_tri_area", a, None) is False
    d = lib.VdnMaskDilateArgs()
    d.src = d.dst = 8
    d.scratch, d.radius = 16, 1
    for N, H, W in ((big, 1, 1), (1, 1 << 16, 1 << 15), (4, 1 << 15, 1 << 14), (1 << 20, 64, 32)):
        d.N, d.H, d.W = N, H, W
        assert lib.try_call("vdn_mask_dilate", d, None) is False, (N, H, W)
    m = lib.VdnMaskVotesArgs()
    m.vertices = m.P = m.masks = m.n_in_image = m.n_in_mask = 8
    for V, N, H, W in ((big, 1, 4, 4), (5, 4, 1 << 15, 1 << 14), (5, 1, 1 << 16, 1 << 15)):
        m.V, m.N, m.H, m.W = V, N, H, W
        assert lib.try_call("vdn_mask_votes", m, None) is False, (V, N, H, W)
    f = lib.VdnMeshFilterArgs()
    f.triangles = f.face_alive = f.vertex_used = f.error = f.face_offsets = f.vertex_new = f.out_triangles = 8
    f.index_bytes, f.F_out = 8, 1
    for V, F in ((big, 1), (3, big)):
        f.V, f.F = V, F
        assert lib.try_call("vdn_mesh_filter_mark", f, None) is False and lib.try_call("vdn_mesh_filter_remap", f, None) is False


# ---- policy -----------------------------------------------------------------------------------------------------------------------
def _table(n_faces, area):
    return {"n_faces": np.asarray(n_faces, np.int64), "area": np.asarray(area, np.float64)}


def test_select_components_on_hand_written_tables():
    from vdn_train.mesh_clean import select_components as sel
    # the most faces and the largest area disagree
    t = _table([10, 50, 7, 50], [9.0, 1.0, 0.5, 2.0])
    assert sel(t).tolist() == [False, True, False, False]                         # 50 faces twice: the lower root
    assert sel(t, by="area").tolist() == [True, False, False, False]
    assert sel(_table([3, 3], [1.0, 1.0]), by="area").tolist() == [True, False]
    # thresholds
    assert sel(t, keep="all").tolist() == [True] * 4
    assert sel(t, keep="all", min_faces=10).tolist() == [True, True, False, True]
    assert sel(t, keep="all", min_faces=51).tolist() == [False] * 4
    assert sel(t, keep="all", min_area_fraction=0.1).tolist() == [True, False, False, True]      # of 12.5: 1.25
    # (area equal to the threshold stays: 1.0 >= 0.25 * 4.0)
    assert sel(_table([1, 1, 1, 1], [2.0, 1.0, 0.5, 0.5]), keep="all", min_area_fraction=0.25).tolist() == [True, True, False, False]
    assert sel(t, keep="all", min_faces=8, min_area_fraction=0.1).tolist() == [True, False, False, True]
    # the largest still has to pass them
    assert sel(t, min_area_fraction=0.1).tolist() == [False] * 4
    assert sel(t, by="area", min_faces=10).tolist() == [True, False, False, False]
    # components without faces (isolated vertices) never win, and stay only under keep="all" without thresholds
    z = _table([0, 4, 0], [0.0, 1.0, 0.0])
    assert sel(z).tolist() == [False, True, False] and sel(z, keep="all", min_faces=1).tolist() == [False, True, False]
    # an empty table, numpy in -> numpy out, tensors in -> tensors out
    e = sel(_table([], []))
    assert isinstance(e, np.ndarray) and e.dtype == np.bool_ and e.shape == (0,)
    assert sel(_table([], []), keep="all").shape == (0,)
    tt = {k: torch.as_tensor(x) for k, x in t.items()}
    out = sel(tt)
    assert torch.is_tensor(out) and out.dtype == torch.bool and out.tolist() == [False, True, False, False]
    for kw in (dict(keep="biggest"), dict(by="volume"), dict(min_faces=-1), dict(min_area_fraction=1.5), dict(min_area_fraction=-0.1)):
        with pytest.raises(ValueError):
            sel(t, **kw)


def test_vote_rule_on_hand_written_counts():
    from vdn_train.mesh_clean import vote_keep
    n_img = np.array([0, 1, 1, 3, 3, 3, 6, 6])
    n_msk = np.array([0, 0, 1, 3, 2, 1, 6, 4])
    assert vote_keep(n_img, n_msk).tolist() == [False, False, True, True, False, False, True, False]
    assert vote_keep(n_img, n_msk, min_inside=0).tolist() == [True, False, True, True, False, False, True, False]       # unseen vertices stay
    assert vote_keep(n_img, n_msk, min_inside=2, max_outside=1).tolist() == [False, False, False, True, True, False, True, False]
    assert vote_keep(n_img, n_msk, min_inside=1, max_outside=2).tolist() == [False, False, True, True, True, True, True, True]
    out = vote_keep(torch.as_tensor(n_img), torch.as_tensor(n_msk))
    assert torch.is_tensor(out) and out.tolist() == vote_keep(n_img, n_msk).tolist()
    with pytest.raises(ValueError):
        vote_keep(n_img, n_msk, min_inside=-1)
    with pytest.raises(ValueError):
        vote_keep(n_img, n_msk, max_outside=-1)


def test_masks_of_every_kind_become_bytes():
    from vdn_train.mesh_clean import masks_to_uint8
    rng = np.random.default_rng(2)
    b = rng.random((2, 5, 7)) > 0.5
    for m in (b, b.astype(np.uint8) * 255, b.astype(np.int32) * -3, b.astype(np.float32) * 0.6 + 0.2, torch.from_numpy(b),
              np.repeat((b.astype(np.float32))[..., None], 3, 3), b.astype(np.float64)[..., None]):
        out = masks_to_uint8(m)
        assert out.dtype == torch.uint8 and out.shape == (2, 5, 7) and np.array_equal(out.numpy(), b.astype(np.uint8))
    three = np.zeros((1, 2, 2, 3), np.float32)
    three[..., 1:] = 1.0                                        # only channel 0 counts
    assert masks_to_uint8(three).sum() == 0
    with pytest.raises(ValueError):
        masks_to_uint8(np.zeros((4, 4)))


def test_projection_matrices_against_a_float64_product(tmp_path):
    from PIL import Image
    from vdn_train import dataset, synth
    root, n, H, W = str(tmp_path), 3, 6, 8
    os.makedirs(os.path.join(root, "image", "mask"))
    names = ["%03d" % i for i in range(n)]
    K4 = np.eye(4)
    K4[:3, :3] = [[21.3, 0.1, 3.5], [0, 20.7, 2.5], [0, 0, 1]]
    scale_mat = np.diag([1.7, 1.7, 1.7, 1.0])
    scale_mat[:3, 3] = [0.2, -0.1, 0.05]
    world = [K4 @ np.linalg.inv(c) @ np.linalg.inv(scale_mat) for c in synth.make_cameras(1)[:n]]
    dataset.write_cameras_npz(os.path.join(root, "cameras_sphere.npz"), names, world, [scale_mat] * n)
    for nm in names:
        Image.fromarray(np.full((H, W, 3), 90, np.uint8), "RGB").save(os.path.join(root, "image", nm + ".png"))
        Image.fromarray(np.full((H, W, 3), 255, np.uint8), "RGB").save(os.path.join(root, "image", "mask", nm + ".png"))
    scene = dataset.SceneData(root)
    P_obj, P_world = scene.projection_matrices(), scene.projection_matrices(world_space=True)
    assert P_obj.dtype == P_world.dtype == np.float64 and P_obj.shape == P_world.shape == (n, 3, 4)
    for i in range(n):
        w32, s32 = np.asarray(world[i]).astype(np.float32), scale_mat.astype(np.float32)
        assert np.array_equal(P_obj[i], (w32.astype(np.float64) @ s32.astype(np.float64))[:3])         # the float64 product of the stored float32
        assert not np.array_equal(P_obj[i], (w32 @ s32)[:3].astype(np.float64))                        # (not the float32 one)
        assert np.array_equal(P_world[i], w32.astype(np.float64)[:3])
        # an object-space point and its world-space image land on the same pixel
        x = np.array([0.1, -0.2, 0.3, 1.0])
        a, b = P_obj[i] @ x, P_world[i] @ (s32.astype(np.float64) @ x)
        assert np.allclose(a[:2] / a[2], b[:2] / b[2], rtol=0, atol=1e-9)


# ---- Python layer -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_that_need_no_device():
    from vdn_hip import mesh
    from vdn_train import mesh_clean
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    m, P = torch.zeros(2, 4, 4, dtype=torch.uint8), np.zeros((2, 3, 4))
    for call in (lambda: mesh.connected_components(t, 4), lambda: mesh.connected_components(t.numpy(), 4),
                 lambda: mesh.triangle_areas(v, t), lambda: mesh.component_table(v, t, torch.zeros(4, dtype=torch.int32)),
                 lambda: mesh.dilate_masks(m, 1), lambda: mesh.mask_votes(v, P, m), lambda: mesh.filter_mesh(v, t)):
        with pytest.raises(ValueError):
            call()                                           # CPU tensors
    for kw in (dict(keep="some"), dict(by="volume"), dict(min_faces=-1), dict(min_area_fraction=2.0), dict(cameras=P), dict(masks=m),
               dict(dilate=-1), dict(dilate=1.5), dict(cameras=P, masks=m, min_inside=-1), dict(cameras=P, masks=m, max_outside=-1)):
        with pytest.raises(ValueError):
            mesh_clean.clean_mesh(v.numpy(), t.numpy(), **kw)
    for vv, tt in ((np.zeros((4, 2)), t.numpy()), (v.numpy(), np.zeros((2, 4), np.int64)), (np.zeros(12), t.numpy())):
        with pytest.raises(ValueError):
            mesh_clean.clean_mesh(vv, tt)
    with pytest.raises(ValueError):
        mesh_clean.clean_mesh(v.numpy(), t.numpy(), attributes=[np.zeros((3, 3))])


def test_validate_mesh_signature_defaults_to_no_cleaning():
    from vdn_train import validate
    for fn in (validate.validate_mesh, validate.validate_scene_mesh):
        assert inspect.signature(fn).parameters["clean"].default is None


def test_command_line_tool_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "clean_mesh.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--keep", "--by", "--min-faces", "--min-area-fraction", "--scene", "--dilate", "--min-inside", "--max-outside", "--world-space"):
        assert opt in r.stdout
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import clean_mesh as tool
    finally:
        sys.path.pop(0)
    a = tool.parser().parse_args(["in.ply", "out.ply", "--keep", "all", "--by", "area", "--min-faces", "5", "--scene", "d", "--dilate", "3", "--world-space"])
    assert (a.mesh, a.out, a.keep, a.by, a.min_faces, a.scene, a.dilate, a.world_space, a.min_inside, a.max_outside) == ("in.ply", "out.ply", "all", "area", 5, "d", 3, True, 1, 0)
