"""Meshes on disk, the parts that need no GPU: the binary PLY writer / reader (vdn_train/meshio.py), the colour quantisation rule
of the vertex colours (vdn_hip/mesh.py) and the boundary of the point-shading entry point (vdn_shade_points_bf16)."""
import os

import numpy as np
import pytest

from vdn_hip import lib, mesh
from vdn_train import meshio

# a hand-made mesh: a unit square in the z = 0.25 plane, two triangles
VERTS = np.array([[0.0, 0.0, 0.25], [1.0, 0.0, 0.25], [1.0, 1.0, 0.25], [0.0, 1.0, 0.25]], dtype=np.float64)
TRIS = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
NORMALS = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8], [-1.0, 0.0, 0.0]], dtype=np.float32)
COLORS = np.array([[255, 0, 0], [0, 128, 1], [3, 2, 254], [17, 18, 19]], dtype=np.uint8)


def _expected_header(V, F, with_n, with_c):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % V, "property float x", "property float y", "property float z"]
    if with_n:
        lines += ["property float nx", "property float ny", "property float nz"]
    if with_c:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += ["element face %d" % F, "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


@pytest.mark.parametrize("with_n", [False, True])
@pytest.mark.parametrize("with_c", [False, True])
def test_ply_round_trip_header_and_size(tmp_path, with_n, with_c):
    path = str(tmp_path / "m.ply")
    assert meshio.write_ply(path, VERTS, TRIS, normals=NORMALS if with_n else None, colors=COLORS if with_c else None) == path
    raw = open(path, "rb").read()
    head = _expected_header(4, 2, with_n, with_c)
    assert raw[:len(head)] == head                                   # the header text, line for line
    stride = 12 + (12 if with_n else 0) + (3 if with_c else 0)
    assert len(raw) == len(head) + 4 * stride + 2 * 13 == os.path.getsize(path)
    # the first vertex record and the first face record, byte for byte
    assert raw[len(head):len(head) + 12] == np.array([0.0, 0.0, 0.25], "<f4").tobytes()
    assert raw[len(head) + 4 * stride:len(head) + 4 * stride + 13] == b"\x03" + np.array([0, 1, 2], "<i4").tobytes()
    got = meshio.read_ply(path)
    assert got["vertices"].dtype == np.float32 and np.array_equal(got["vertices"], VERTS.astype(np.float32))
    assert got["triangles"].shape == (2, 3) and np.array_equal(got["triangles"], TRIS)
    if with_n:
        assert got["normals"].dtype == np.float32 and np.array_equal(got["normals"], NORMALS)
    else:
        assert got["normals"] is None
    if with_c:
        assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], COLORS)
    else:
        assert got["colors"] is None


@pytest.mark.parametrize("with_attr", [False, True])
def test_empty_mesh_is_a_valid_file(tmp_path, with_attr):
    path = str(tmp_path / "empty.ply")
    e3 = np.zeros((0, 3))
    meshio.write_ply(path, e3, np.zeros((0, 3), np.int64), normals=e3.astype(np.float32) if with_attr else None,
                     colors=e3.astype(np.uint8) if with_attr else None)
    assert open(path, "rb").read() == _expected_header(0, 0, with_attr, with_attr)
    got = meshio.read_ply(path)
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3)
    assert (got["normals"] is not None) == with_attr and (got["colors"] is not None) == with_attr


def test_read_ply_raises_on_what_write_ply_does_not_write(tmp_path):
    good = str(tmp_path / "good.ply")
    meshio.write_ply(good, VERTS, TRIS, normals=NORMALS, colors=COLORS)
    raw = open(good, "rb").read()

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p
    with pytest.raises(ValueError):
        meshio.read_ply(variant("ascii.ply", raw.replace(b"format binary_little_endian 1.0", b"format ascii 1.0")))
    with pytest.raises(ValueError):
        meshio.read_ply(variant("big.ply", raw.replace(b"binary_little_endian", b"binary_big_endian")))
    with pytest.raises(ValueError):
        meshio.read_ply(variant("double.ply", raw.replace(b"property float x", b"property double x")))
    with pytest.raises(ValueError):
        meshio.read_ply(variant("short.ply", raw[:-1]))                # one byte short of what the header announces
    with pytest.raises(ValueError):
        meshio.read_ply(variant("noheader.ply", b"not a ply file"))
    assert np.array_equal(meshio.read_ply(good)["colors"], COLORS)


def test_write_ply_checks_its_arguments(tmp_path):
    p = str(tmp_path / "x.ply")
    with pytest.raises(ValueError):
        meshio.write_ply(p, VERTS, np.array([[0, 1, 4]]))            # index past the last vertex
    with pytest.raises(ValueError):
        meshio.write_ply(p, VERTS, TRIS, normals=NORMALS[:3])
    with pytest.raises(ValueError):
        meshio.write_ply(p, VERTS, TRIS, colors=COLORS.astype(np.float32))


def test_colour_quantisation_rule():
    """BGR float -> RGB uint8 = rint(clip(c, 0, 1) * 255), channels reversed: values outside [0, 1] saturate, a quarter step either
    side of a level rounds to that level, and the exact tie 0.5 * 255 = 127.5 goes to the even neighbour 128."""
    c = np.array([[0.0, 0.5, 1.0],                       # B, G, R
                  [-0.25, 1.75, 1e-9],
                  [(10 - 0.25) / 255, (10 + 0.25) / 255, (10 + 0.75) / 255],
                  [np.nextafter(np.float32(0.5), np.float32(0)), 0.5, np.nextafter(np.float32(0.5), np.float32(1))]], dtype=np.float32)
    q = mesh.quantize_colors_bgr(c)
    assert q.dtype == np.uint8 and q.flags["C_CONTIGUOUS"]
    assert q.tolist() == [[255, 128, 0], [0, 255, 0], [11, 10, 10], [128, 128, 127]]
    assert mesh.quantize_colors_bgr(c.astype(np.float64)).tolist() == q.tolist()
    with pytest.raises(ValueError):
        mesh.quantize_colors_bgr(np.zeros((4, 4), np.float32))


def test_library_exports_the_point_shading_entry_point():
    l = lib.load()
    assert "vdn_shade_points_bf16" in lib.FUNCTIONS and hasattr(l, "vdn_shade_points_bf16")
    assert len(lib.FUNCTIONS["vdn_shade_points_bf16"]) == 5
    assert l.vdn_abi_version() == 28                    # additive: no version bump


def test_point_shading_argument_errors_are_reported_not_ignored():
    """An empty argument block / null pointers are refused with a negative status before anything is launched (no GPU is touched:
    this runs on a machine without one)."""
    s = lib.VdnSdfArgs()
    with pytest.raises(lib.VdnError):
        lib.call("vdn_shade_points_bf16", s, None, 1, None, None)
    with pytest.raises(lib.VdnError):
        lib.call("vdn_shade_points_bf16", None, None, 1, None, None)
    s.P = 4                                             # points, but no blob / buffers
    with pytest.raises(lib.VdnError):
        lib.call("vdn_shade_points_bf16", s, None, 1, None, None)
