"""Mesh evaluation, the parts that need no device: read_points_ply (the scanned-cloud reader of vdn_train.meshio), the ctypes
mirrors of the new argument blocks, and the argument errors of sample_surface / PointGrid / evaluate_mesh."""
import ctypes

import numpy as np
import pytest
import torch

from vdn_hip import lib
from vdn_train import meshio


def _cloud(n=37, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), rng.normal(size=(n, 3)).astype(np.float32), rng.integers(0, 256, size=(n, 3)).astype(np.uint8)


def _write(path, header_lines, *blobs):
    with open(path, "wb") as f:
        f.write(("\n".join(header_lines) + "\n").encode("ascii"))
        for b in blobs:
            f.write(b)
    return str(path)


def _scan_file(path, pos, nrm, col, pos_type="float", extra=()):
    """positions + normals + uchar colours, no faces: what a scanned ground-truth cloud looks like on disk."""
    ft = "<f4" if pos_type == "float" else "<f8"
    rec = np.empty(len(pos), dtype=[("x", ft), ("y", ft), ("z", ft), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for d, n in enumerate("xyz"):
        rec[n] = pos[:, d]
        rec["n" + n] = nrm[:, d]
    for d, n in enumerate(("red", "green", "blue")):
        rec[n] = col[:, d]
    head = ["ply", "format binary_little_endian 1.0", "comment a scan", "element vertex %d" % len(pos)]
    head += ["property %s %s" % (pos_type, n) for n in "xyz"] + ["property float n%s" % n for n in "xyz"]
    head += ["property uchar %s" % n for n in ("red", "green", "blue")] + list(extra) + ["end_header"]
    return _write(path, head, rec.tobytes()), rec


def test_read_points_ply_positions_only(tmp_path):
    pos = _cloud()[0].astype(np.float32)
    p = _write(tmp_path / "a.ply", ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(pos),
                                    "property float x", "property float y", "property float z", "end_header"], pos.astype("<f4").tobytes())
    out = meshio.read_points_ply(p)
    assert out.dtype == np.float32 and np.array_equal(out, pos)


def test_read_points_ply_scanned_cloud_layout(tmp_path):
    pos, nrm, col = _cloud()
    p, _ = _scan_file(tmp_path / "scan.ply", pos.astype(np.float32), nrm, col)
    out = meshio.read_points_ply(p)
    assert out.dtype == np.float32 and out.shape == (37, 3) and np.array_equal(out, pos.astype(np.float32))


def test_read_points_ply_double_positions_and_aliases(tmp_path):
    pos, nrm, col = _cloud()
    p, _ = _scan_file(tmp_path / "d.ply", pos, nrm, col, pos_type="double")
    out = meshio.read_points_ply(p)
    assert out.dtype == np.float64 and np.array_equal(out, pos)
    # the int8 .. float64 spellings, the coordinates not first and a short in between
    rec = np.empty(5, dtype=[("q", "<i2"), ("z", "<f4"), ("x", "<f8"), ("k", "u1"), ("y", "<f4")])
    rec["q"], rec["k"] = 7, 9
    rec["x"], rec["y"], rec["z"] = pos[:5, 0], pos[:5, 1].astype(np.float32), pos[:5, 2].astype(np.float32)
    p = _write(tmp_path / "alias.ply", ["ply", "format binary_little_endian 1.0", "element vertex 5", "property int16 q", "property float32 z",
                                        "property float64 x", "property uint8 k", "property float32 y", "end_header"], rec.tobytes())
    out = meshio.read_points_ply(p)
    assert out.dtype == np.float64
    assert np.array_equal(out[:, 0], pos[:5, 0]) and np.array_equal(out[:, 1], pos[:5, 1].astype(np.float32).astype(np.float64))
    assert np.array_equal(out[:, 2], pos[:5, 2].astype(np.float32).astype(np.float64))


def test_read_points_ply_ignores_later_elements(tmp_path):
    """a mesh of write_ply (face element behind the vertices) gives its vertices; read_ply still reads the same file whole"""
    pos = _cloud(6)[0].astype(np.float32)
    tri = np.array([[0, 1, 2], [3, 4, 5]])
    p = meshio.write_ply(str(tmp_path / "m.ply"), pos, tri, colors=_cloud(6)[2])
    assert np.array_equal(meshio.read_points_ply(p), pos)
    assert np.array_equal(meshio.read_ply(p)["triangles"], tri)
    # zero vertices
    p = _write(tmp_path / "e.ply", ["ply", "format binary_little_endian 1.0", "element vertex 0", "property float x", "property float y",
                                    "property float z", "end_header"])
    assert meshio.read_points_ply(p).shape == (0, 3)


def test_read_points_ply_refusals(tmp_path):
    pos, nrm, col = _cloud()
    xyz = ["property float x", "property float y", "property float z"]
    body = pos.astype("<f4").tobytes()
    n = "element vertex %d" % len(pos)
    cases = {
        "ascii": (["ply", "format ascii 1.0", n] + xyz + ["end_header"], body),
        "big_endian": (["ply", "format binary_big_endian 1.0", n] + xyz + ["end_header"], body),
        "list_in_vertex": (["ply", "format binary_little_endian 1.0", n] + xyz + ["property list uchar int k", "end_header"], body),
        "truncated": (["ply", "format binary_little_endian 1.0", n] + xyz + ["end_header"], body[:-1]),
        "no_z": (["ply", "format binary_little_endian 1.0", n] + xyz[:2] + ["property float w", "end_header"], body),
        "face_first": (["ply", "format binary_little_endian 1.0", "element face 1", "property list uchar int vertex_indices", n] + xyz + ["end_header"], body),
        "unknown_type": (["ply", "format binary_little_endian 1.0", n] + xyz + ["property half w", "end_header"], body),
        "no_header": (["ply", "format binary_little_endian 1.0", n] + xyz, body),
    }
    for name, (head, blob) in cases.items():
        p = _write(tmp_path / (name + ".ply"), head, blob)
        with pytest.raises(ValueError):
            meshio.read_points_ply(p)
    # read_ply stays strict: the scanned-cloud layout is not one of its files
    p, _ = _scan_file(tmp_path / "scan.ply", pos.astype(np.float32), nrm, col)
    with pytest.raises(ValueError):
        meshio.read_ply(p)


def test_new_argument_blocks_are_c_layouts_and_declared():
    structs, funcs = lib.parse_header()
    for fn in ("vdn_surf_count", "vdn_surf_emit", "vdn_nn_bin", "vdn_nn_query"):
        assert funcs[fn] == [ctypes.c_void_p, ctypes.c_void_p]
    # VdnSurfArgs {2 pointers, double, 3 int64, 2 int32, 5 pointers}
    S = lib.VdnSurfArgs
    assert ctypes.sizeof(S) == 2 * 8 + 8 + 3 * 8 + 2 * 4 + 5 * 8 == 96
    assert (S.spacing.offset, S.V.offset, S.S.offset, S.index_bytes.offset, S.counts.offset, S.face.offset) == (16, 24, 40, 48, 56, 88)
    # VdnNnArgs {8 pointers, 2 int64, 6 float, 4 int32}
    N = lib.VdnNnArgs
    assert ctypes.sizeof(N) == 8 * 8 + 2 * 8 + 6 * 4 + 4 * 4 == 120
    assert (N.rings.offset, N.N.offset, N.R.offset, N.lo_x.offset, N.max_dist.offset, N.nx.offset, N.nz.offset) == (56, 64, 72, 80, 100, 104, 112)
    assert int(__import__("re").search(r"#define\s+VDN_ABI_VERSION\s+(\d+)", open(lib.HEADER).read()).group(1)) == 28     # additive: no bump


def test_new_entry_points_refuse_empty_argument_blocks():
    for name, args in (("vdn_surf_count", lib.VdnSurfArgs()), ("vdn_surf_emit", lib.VdnSurfArgs()),
                       ("vdn_nn_bin", lib.VdnNnArgs()), ("vdn_nn_query", lib.VdnNnArgs())):
        with pytest.raises(lib.VdnError):
            lib.call(name, args, None)


def test_sizes_beyond_32_bit_indexing_are_status_minus_10():
    """checked on the host before anything is launched (the pointers are never dereferenced there)"""
    a = lib.VdnNnArgs()
    a.pts = a.cell = a.ref = a.cell_start = a.dist = a.idx = 8
    a.N, a.R, a.h, a.nx, a.ny, a.nz, a.max_dist = 1 << 31, 1, 1.0, 1, 1, 1, 1.0
    assert lib.try_call("vdn_nn_bin", a, None) is False and lib.try_call("vdn_nn_query", a, None) is False
    a.N, a.nx, a.ny, a.nz = 1, 2048, 2048, 512
    assert lib.try_call("vdn_nn_bin", a, None) is False
    a.nx, a.R = 1, 1 << 31
    assert lib.try_call("vdn_nn_query", a, None) is False
    s = lib.VdnSurfArgs()
    s.vertices = s.triangles = s.counts = s.error = s.offsets = s.points = s.face = 8
    s.spacing, s.V, s.F, s.S, s.index_bytes = 1.0, 3, 1 << 31, 1, 8
    assert lib.try_call("vdn_surf_count", s, None) is False and lib.try_call("vdn_surf_emit", s, None) is False
    s.F, s.S = 1, 1 << 31
    assert lib.try_call("vdn_surf_emit", s, None) is False


def test_argument_errors_that_need_no_device():
    from vdn_hip import mesh, nn
    from vdn_train import mesh_eval
    v, t, g = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(5, 3)
    with pytest.raises(ValueError):
        mesh.sample_surface(v, t, 0.1)                       # CPU tensors
    with pytest.raises(ValueError):
        nn.PointGrid(g)
    with pytest.raises(ValueError):
        nn.nearest(g, g)
    for kw in (dict(spacing=0.0, max_dist=1.0), dict(spacing=-1.0, max_dist=1.0), dict(spacing=0.1, max_dist=-1.0),
               dict(spacing=0.1, max_dist=0.5, thresholds=(0.1, 0.6)), dict(spacing=0.1, max_dist=0.5, thresholds=(-0.1,)),
               dict(spacing=0.1, max_dist=0.5)):             # the last: valid numbers, CPU tensors
        with pytest.raises(ValueError):
            mesh_eval.evaluate_mesh(v, t, g, **kw)
    with pytest.raises(ValueError):
        mesh_eval.evaluate_mesh(v, None, g, 0.1, 0.5)


def test_result_line_is_plain_json():
    import json
    from vdn_train import mesh_eval
    r = {"n_gt": 3, "accuracy": float("nan"), "chamfer": 0.25, "precision": {0.5: 1.0}, "recall": {0.5: 0.0}, "fscore": {0.5: 0.0}}
    d = json.loads(mesh_eval.to_json(r))
    assert d == {"n_gt": 3, "accuracy": None, "chamfer": 0.25, "precision": {"0.5": 1.0}, "recall": {"0.5": 0.0}, "fscore": {"0.5": 0.0}}
