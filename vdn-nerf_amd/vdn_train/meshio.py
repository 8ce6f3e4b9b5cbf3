"""Triangle meshes on disk: the binary PLY Runner.validate_mesh leaves behind (dpt_runner.py:699-713 exports through the
third-party `trimesh`; this module writes the same kind of file with numpy alone), with optional vertex normals and colours.

Layout (`binary_little_endian 1.0`):
  element vertex V:  float x y z, [float nx ny nz], [uchar red green blue]
  element face F:    property list uchar int vertex_indices   (always 3 indices: 13 bytes per face)
Both elements are written from numpy structured arrays; read_ply reads exactly this layout and raises on anything else.
read_points_ply reads the positions of a scanned cloud, read_dtu_aux the arrays the DTU evaluation keeps beside one.
write_obj / read_obj: a textured mesh as a Wavefront OBJ with its material library and its PNG (vdn_hip.mesh.bake_texture's atlas)."""
import os

import numpy as np

_POS = ("x", "y", "z")
_NRM = ("nx", "ny", "nz")
_COL = ("red", "green", "blue")
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])          # packed: 13 bytes


def vertex_dtype(normals=False, colors=False):
    """The packed little-endian record of one vertex."""
    fields = [(n, "<f4") for n in _POS]
    if normals:
        fields += [(n, "<f4") for n in _NRM]
    if colors:
        fields += [(n, "u1") for n in _COL]
    return np.dtype(fields)


def ply_header(n_vertices, n_faces, normals=False, colors=False):
    """The header text of a file of write_ply, line for line."""
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n_vertices]
    lines += ["property float %s" % n for n in _POS]
    if normals:
        lines += ["property float %s" % n for n in _NRM]
    if colors:
        lines += ["property uchar %s" % n for n in _COL]
    lines += ["element face %d" % n_faces, "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """vertices [V,3] (stored as float32), triangles [F,3] integer, normals [V,3] float or None, colors [V,3] uint8 RGB or None."""
    vertices = np.asarray(vertices).reshape(-1, 3)
    triangles = np.asarray(triangles).reshape(-1, 3)
    V, F = vertices.shape[0], triangles.shape[0]
    if not np.issubdtype(triangles.dtype, np.integer) and F > 0:
        raise ValueError("triangles must be integers, got %s" % triangles.dtype)
    if F > 0 and (triangles.min() < 0 or triangles.max() >= V or triangles.max() > np.iinfo(np.int32).max):
        raise ValueError("triangle indices must lie in [0, V)")
    vert = np.empty(V, dtype=vertex_dtype(normals is not None, colors is not None))
    for d, n in enumerate(_POS):
        vert[n] = vertices[:, d]
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != (V, 3):
            raise ValueError("normals must be [V,3] = %s, got %s" % ((V, 3), normals.shape))
        for d, n in enumerate(_NRM):
            vert[n] = normals[:, d]
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != (V, 3) or colors.dtype != np.uint8:
            raise ValueError("colors must be uint8 [V,3] = %s, got %s %s" % ((V, 3), colors.dtype, colors.shape))
        for d, n in enumerate(_COL):
            vert[n] = colors[:, d]
    face = np.empty(F, dtype=FACE_DTYPE)
    face["n"] = 3
    face["v"] = triangles
    with open(path, "wb") as f:
        f.write(ply_header(V, F, normals is not None, colors is not None).encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())
    return path


_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
                "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def read_points_ply(path):
    """-> vertex positions [V,3] (float32, or float64 where the file stores doubles) of any `binary_little_endian 1.0` file whose
    first element is `vertex` with scalar properties that include x, y, z - the layout of scanned ground-truth clouds (positions,
    normals, uchar colours, no faces). The other properties and every later element are ignored. ValueError on ASCII or big-endian
    files, a list property in the vertex element, missing coordinates or a truncated file. (read_ply stays the strict reader of
    write_ply's own files.)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError("%s: no PLY header" % path)
    n_head = end + len(b"end_header\n")
    try:
        lines = [ln.strip() for ln in data[:n_head].decode("ascii").split("\n")]
    except UnicodeDecodeError:
        raise ValueError("%s: the PLY header is not ASCII text" % path)
    if lines[0] != "ply":
        raise ValueError("%s: not a PLY file" % path)
    lines = [ln for ln in lines[1:] if ln and not ln.startswith(("comment", "obj_info"))]
    if not lines or lines[0].split() != ["format", "binary_little_endian", "1.0"]:
        raise ValueError("%s: only `format binary_little_endian 1.0` files are read, got %r" % (path, lines[:1]))
    V, fields, n_elements = None, [], 0
    for ln in lines[1:]:
        tok = ln.split()
        if tok[0] == "element":
            n_elements += 1
            if n_elements == 1:
                try:
                    assert tok[1] == "vertex" and len(tok) == 3
                    V = int(tok[2])
                    assert V >= 0
                except (AssertionError, ValueError, IndexError):
                    raise ValueError("%s: the first element must be `element vertex V`, got %r" % (path, ln))
        elif tok[0] == "property" and n_elements == 1:
            if len(tok) >= 2 and tok[1] == "list":
                raise ValueError("%s: a list property in the vertex element: %r" % (path, ln))
            if len(tok) != 3 or tok[1] not in _PLY_SCALARS:
                raise ValueError("%s: unknown vertex property %r" % (path, ln))
            fields.append((tok[2], _PLY_SCALARS[tok[1]]))
    if V is None:
        raise ValueError("%s: no vertex element" % path)
    names = [n for n, _ in fields]
    if len(set(names)) != len(names) or not all(n in names for n in _POS):
        raise ValueError("%s: the vertex element needs one x, y and z each, got %r" % (path, names))
    vd = np.dtype(fields)
    if len(data) < n_head + V * vd.itemsize:
        raise ValueError("%s: %d bytes, the vertex element alone needs %d" % (path, len(data), n_head + V * vd.itemsize))
    vert = np.frombuffer(data, dtype=vd, count=V, offset=n_head)
    out = np.float64 if any(vd[n] == np.dtype("<f8") for n in _POS) else np.float32
    return np.stack([vert[n].astype(out) for n in _POS], axis=1) if V > 0 else np.zeros((0, 3), out)


def read_ply(path):
    """-> dict(vertices [V,3] float32, triangles [F,3] int32, normals [V,3] float32 | None, colors [V,3] uint8 | None) of a file
    written by write_ply; ValueError on any other header (ASCII, big-endian, other properties) or a size that does not match."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError("%s: no PLY header" % path)
    n_head = end + len(b"end_header\n")
    try:
        head = data[:n_head].decode("ascii")
    except UnicodeDecodeError:
        raise ValueError("%s: the PLY header is not ASCII text" % path)
    lines = head.split("\n")
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError("%s: only `format binary_little_endian 1.0` files are read, got %r" % (path, lines[1:2]))
    try:
        kind, what, V = lines[2].split()
        V = int(V)
        assert (kind, what) == ("element", "vertex") and V >= 0
    except (ValueError, AssertionError):
        raise ValueError("%s: expected `element vertex V`, got %r" % (path, lines[2]))
    F = None
    for has_n in (False, True):
        for has_c in (False, True):
            face_line = 3 + 3 * (1 + has_n + has_c)
            if len(lines) > face_line and lines[face_line].startswith("element face "):
                try:
                    F = int(lines[face_line].split()[2])
                except (ValueError, IndexError):
                    F = -1
                if F >= 0 and head == ply_header(V, F, has_n, has_c):
                    vd = vertex_dtype(has_n, has_c)
                    if len(data) != n_head + V * vd.itemsize + F * FACE_DTYPE.itemsize:
                        raise ValueError("%s: %d bytes, the header announces %d" %
                                         (path, len(data), n_head + V * vd.itemsize + F * FACE_DTYPE.itemsize))
                    vert = np.frombuffer(data, dtype=vd, count=V, offset=n_head)
                    face = np.frombuffer(data, dtype=FACE_DTYPE, count=F, offset=n_head + V * vd.itemsize)
                    if F > 0 and not (face["n"] == 3).all():
                        raise ValueError("%s: a face that is not a triangle" % path)
                    col = lambda names: np.stack([vert[n] for n in names], axis=1) if V > 0 else np.zeros((0, 3), vert[names[0]].dtype)
                    return {"vertices": col(_POS), "triangles": face["v"].astype(np.int32).reshape(F, 3),
                            "normals": col(_NRM) if has_n else None, "colors": col(_COL) if has_c else None}
    raise ValueError("%s: the header is not one write_ply writes" % path)


def _obj_paths(path):
    stem, ext = os.path.splitext(str(path))
    if ext.lower() != ".obj":
        raise ValueError("%s: an OBJ path ends in .obj" % path)
    return stem + ".obj", stem + ".mtl", stem + ".png"


def write_obj(path, vertices, triangles, uv, texture, normals=None):
    """A textured mesh as the trio <stem>.obj, <stem>.mtl (one material, `map_Kd <stem>.png`) and <stem>.png -> the .obj path.
    vertices [V,3] float, triangles [F,3] integer, uv [F,3,2] float (one texture coordinate per face corner, v = 0 at the bottom:
    vdn_hip.mesh.bake_texture's "uv"), texture uint8 [S,S,3] RGB with row 0 at the top, normals [V,3] float or None. Faces are
    written as `f v/vt` or `f v/vt/vn`, 1-based, face f using the texture coordinates 3 f + 1 .. 3 f + 3. Positions and
    normals are stored as fp32 and printed with %.9g, the coordinates with %.17g: read_obj returns those arrays bit for bit."""
    from PIL import Image
    obj, mtl, png = _obj_paths(path)
    vertices = np.asarray(vertices).reshape(-1, 3)
    triangles = np.asarray(triangles).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64)
    texture = np.asarray(texture)
    V, F = vertices.shape[0], triangles.shape[0]
    if not np.issubdtype(triangles.dtype, np.integer) and F > 0:
        raise ValueError("triangles must be integers, got %s" % triangles.dtype)
    if F > 0 and (triangles.min() < 0 or triangles.max() >= V):
        raise ValueError("triangle indices must lie in [0, V)")
    if uv.shape != (F, 3, 2):
        raise ValueError("uv must be [F,3,2] = %s, got %s" % ((F, 3, 2), uv.shape))
    if texture.ndim != 3 or texture.shape[2] != 3 or texture.dtype != np.uint8 or texture.shape[0] < 1 or texture.shape[1] < 1:
        raise ValueError("texture must be uint8 [H,W,3], got %s %s" % (texture.dtype, texture.shape))
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != (V, 3):
            raise ValueError("normals must be [V,3] = %s, got %s" % ((V, 3), normals.shape))
    name = os.path.basename(png)
    lines = ["mtllib %s" % os.path.basename(mtl)]
    lines += ["v %.9g %.9g %.9g" % tuple(p) for p in vertices.astype(np.float32).tolist()]
    if normals is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(p) for p in normals.astype(np.float32).tolist()]
    lines += ["vt %.17g %.17g" % tuple(p) for p in uv.reshape(-1, 2).tolist()]
    lines.append("usemtl material_0")
    tri = (triangles.astype(np.int64) + 1).tolist()
    if normals is None:
        lines += ["f %d/%d %d/%d %d/%d" % (a, 3 * f + 1, b, 3 * f + 2, c, 3 * f + 3) for f, (a, b, c) in enumerate(tri)]
    else:
        lines += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, 3 * f + 1, a, b, 3 * f + 2, b, c, 3 * f + 3, c) for f, (a, b, c) in enumerate(tri)]
    with open(obj, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(mtl, "w") as f:
        f.write("newmtl material_0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s\n" % name)
    Image.fromarray(np.ascontiguousarray(texture)).save(png)
    return obj


def read_obj(path):
    """-> dict(vertices [V,3] float32, triangles [F,3] int32, uv [T,2] float64 (the file's vt lines), uv_index [F,3] int32,
    normals [V,3] float32 | None, normal_index [F,3] int32 | None, mtllib, texture_path (the map_Kd of the material library, beside
    the file; None without one)) of a file of write_obj: triangles only, `f v/vt` or `f v/vt/vn`, indices 0-based on return.
    ValueError on anything else."""
    path = str(path)
    v, vn, vt, fv, ft, fn, mtllib = [], [], [], [], [], [], None
    with open(path) as f:
        for ln in f:
            tok = ln.split()
            if not tok or tok[0].startswith("#"):
                continue
            try:
                if tok[0] == "v" and len(tok) == 4:
                    v.append([float(x) for x in tok[1:]])
                elif tok[0] == "vn" and len(tok) == 4:
                    vn.append([float(x) for x in tok[1:]])
                elif tok[0] == "vt" and len(tok) == 3:
                    vt.append([float(x) for x in tok[1:]])
                elif tok[0] == "f" and len(tok) == 4:
                    parts = [[int(x) - 1 for x in c.split("/")] for c in tok[1:]]
                    if len({len(p) for p in parts}) != 1 or len(parts[0]) not in (2, 3):
                        raise ValueError
                    fv.append([p[0] for p in parts])
                    ft.append([p[1] for p in parts])
                    if len(parts[0]) == 3:
                        fn.append([p[2] for p in parts])
                elif tok[0] == "mtllib" and len(tok) == 2:
                    mtllib = tok[1]
                elif tok[0] in ("usemtl", "o", "g", "s"):
                    continue
                else:
                    raise ValueError
            except ValueError:
                raise ValueError("%s: not a line write_obj writes: %r" % (path, ln.rstrip("\n")))
    if fn and len(fn) != len(fv):
        raise ValueError("%s: some faces carry normals and some do not" % path)
    arr = lambda x, dt, w: np.asarray(x, dtype=dt).reshape(-1, w)
    tri, uvi = arr(fv, np.int32, 3), arr(ft, np.int32, 3)
    if len(tri) and (tri.min() < 0 or tri.max() >= len(v) or uvi.min() < 0 or uvi.max() >= len(vt)):
        raise ValueError("%s: a face refers to a vertex or a texture coordinate the file does not hold" % path)
    texture_path = None
    if mtllib is not None:
        mtl = os.path.join(os.path.dirname(path), mtllib)
        if os.path.exists(mtl):
            with open(mtl) as f:
                for ln in f:
                    tok = ln.split()
                    if len(tok) == 2 and tok[0] == "map_Kd":
                        texture_path = os.path.join(os.path.dirname(path), tok[1])
    return {"vertices": arr(v, np.float32, 3), "triangles": tri, "uv": arr(vt, np.float64, 2), "uv_index": uvi,
            "normals": arr(vn, np.float32, 3) if vn else None, "normal_index": arr(fn, np.int32, 3) if fn else None,
            "mtllib": mtllib, "texture_path": texture_path}


def read_dtu_aux(path):
    """-> dict with those of ObsMask (bool [X,Y,Z]), BB (float32 [2,3]), Res (float), P (float64 [4]) the file holds: the arrays
    the DTU evaluation reads beside a scan (the observation mask with its box and voxel pitch, the ground plane), for
    vdn_train.mesh_eval's observed_mask / above_plane. `.npz`: numpy's archive with those names; `.mat`: a MATLAB file with the same
    names, read through scipy.io.loadmat - a ValueError says so where scipy is not installed (convert the file to .npz elsewhere).
    ValueError on a v7.3 (HDF5) .mat file, on any other suffix and on an array of the wrong shape; other names in the file are ignored."""
    p = str(path)
    if p.lower().endswith(".npz"):
        with np.load(p, allow_pickle=False) as z:
            raw = {k: z[k] for k in ("ObsMask", "BB", "Res", "P") if k in z.files}
    elif p.lower().endswith(".mat"):
        try:
            from scipy.io import loadmat
        except ImportError:
            raise ValueError("%s: a .mat file needs scipy (scipy.io.loadmat), which cannot be imported; convert it to .npz" % p)
        try:
            m = loadmat(p)
        except NotImplementedError:
            raise ValueError("%s: a MATLAB v7.3 (HDF5) file, which scipy.io.loadmat does not read; save it with -v7 or convert it to .npz" % p)
        raw = {k: np.asarray(m[k]) for k in ("ObsMask", "BB", "Res", "P") if k in m}
    else:
        raise ValueError("%s: expected a .npz or .mat file" % p)
    out = {}
    if "ObsMask" in raw:
        a = raw["ObsMask"]
        if a.ndim != 3 or a.dtype.kind not in "bui":
            raise ValueError("%s: ObsMask must be a 3-D bool or integer array, got %s %r" % (p, a.dtype, a.shape))
        out["ObsMask"] = np.ascontiguousarray(a != 0)
    if "BB" in raw:
        a = raw["BB"]
        if a.shape != (2, 3) or a.dtype.kind not in "fui":
            raise ValueError("%s: BB must be [2,3] numbers, got %s %r" % (p, a.dtype, a.shape))
        out["BB"] = np.ascontiguousarray(a, dtype=np.float32)
    if "Res" in raw:
        a = raw["Res"]
        if a.size != 1 or a.dtype.kind not in "fui":
            raise ValueError("%s: Res must be one number, got %s %r" % (p, a.dtype, a.shape))
        out["Res"] = float(a.reshape(-1)[0])
    if "P" in raw:
        a = raw["P"]
        if a.size != 4 or a.ndim > 2 or a.dtype.kind not in "fui":
            raise ValueError("%s: P must be 4 numbers, got %s %r" % (p, a.dtype, a.shape))
        out["P"] = np.ascontiguousarray(a, dtype=np.float64).reshape(4)
    return out
