"""The VTU writers (orc_write_vtu, orc_write_vtu_faces; orc_amd/csrc/vtk_io.cpp) read back with the standard library only
(xml.etree, struct): both encodings, bit-for-bit arrays with NaN, infinities, -0.0 and denormals, VTK's node order and orientation
of every tetrahedron and hexahedron (signed volume against the mesh's cell volume), the type counts of the mesh, every polyhedron's
face stream, the absence of unused points, and the status codes of bad arguments and an unwritable path.  CPU only."""
import ctypes as C
import struct
import xml.etree.ElementTree as ET

import numpy as np
import pytest

BAD_ARGUMENT, IO = 10, 13
TETRA, HEXAHEDRON, POLYHEDRON, POLYGON = 10, 12, 42, 7
_STRUCT = {"Float64": "d", "Int64": "q", "UInt8": "B"}


def read_vtu(path):
    """{'n_points', 'n_cells', 'arrays': {name: (list of values, components)}} of a .vtu in either encoding"""
    raw = open(path, "rb").read()
    k = raw.find(b"<AppendedData")
    blob = b""
    if k >= 0:
        assert b'encoding="raw"' in raw[k:raw.index(b">", k)]
        blob = raw[raw.index(b"_", raw.index(b">", k)) + 1:]
        raw = raw[:k] + b"</VTKFile>"
    root = ET.fromstring(raw)
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid" and root.get("version") == "1.0"
    assert root.get("byte_order") == "LittleEndian" and root.get("header_type") == "UInt64"
    piece = root.find("UnstructuredGrid/Piece")
    out = {"n_points": int(piece.get("NumberOfPoints")), "n_cells": int(piece.get("NumberOfCells")), "arrays": {}, "cell_data": []}
    for section in piece:
        for da in section.findall("DataArray"):
            code = _STRUCT[da.get("type")]
            if da.get("format") == "appended":
                off = int(da.get("offset"))
                (nbytes,) = struct.unpack_from("<Q", blob, off)
                size = struct.calcsize(code)
                assert nbytes % size == 0
                vals = list(struct.unpack_from("<%d%s" % (nbytes // size, code), blob, off + 8))
            else:
                assert da.get("format") == "ascii"
                vals = [float(t) if code == "d" else int(t) for t in (da.text or "").split()]
            out["arrays"][da.get("Name")] = (vals, int(da.get("NumberOfComponents") or 1))
            if section.tag == "CellData":
                out["cell_data"].append(da.get("Name"))
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def cell_array(out, name, n):
    """a CellData array back as ndarray [n] or [n, k]"""
    vals, k = out["arrays"][name]
    a = np.array(vals, dtype=np.float64)
    assert len(a) == n * k
    return a if k == 1 else a.reshape(n, k)


# ------------------------------------------------------------------ the cases
@pytest.fixture(scope="module", params=["hex", "mixed", "poly"])
def case(request, tmp_path_factory):
    from orc_amd import io as orc_io
    from orc_amd.mesh import write_hex_channel_msh, write_mixed_channel_msh
    d = tmp_path_factory.mktemp("vtu_" + request.param)
    path = str(d / "m.msh")
    if request.param == "hex":
        write_hex_channel_msh(path, 3, 2, 2)
    else:  # the channels of tests/test_gpu_surface.py::mixed_case
        write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=request.param == "poly")
    md = orc_io.read_mesh(path)
    return request.param, md, md.arrays(), md.nodes(), d


def special_arrays(n):
    rng = np.random.default_rng(7)
    s = rng.standard_normal(n)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -2.2250738585072009e-308, 1.7976931348623157e308, 0.1, -1.0 / 3.0]
    s[:min(n, len(special))] = special[:min(n, len(special))]
    vec = rng.standard_normal((n, 3))
    vec[n // 2] = (-0.0, np.nan, 4.9406564584124654e-324)
    return {"s": s, "velocity": vec}


def mesh_kinds(a, nodes):
    """per cell: the VTK type the mesh itself calls for, and its faces' node lists"""
    vert, fnp, fn = nodes
    cfp, cf = np.asarray(a["cell_face_ptr"]), np.asarray(a["cell_faces"])
    kinds, faces = [], []
    for c in range(len(cfp) - 1):
        fl = [fn[fnp[f]:fnp[f + 1]].tolist() for f in cf[cfp[c]:cfp[c + 1]]]
        distinct = len(set(v for f in fl for v in f))
        if len(fl) == 4 and all(len(f) == 3 for f in fl) and distinct == 4:
            kinds.append(TETRA)
        elif len(fl) == 6 and all(len(f) == 4 for f in fl) and distinct == 8:
            kinds.append(HEXAHEDRON)
        else:
            kinds.append(POLYHEDRON)
        faces.append(fl)
    return np.array(kinds), faces


HEX_FACES = ((0, 4, 7, 3), (1, 2, 6, 5), (0, 1, 5, 4), (3, 7, 6, 2), (0, 3, 2, 1), (4, 5, 6, 7))  # VTK's, outward


def signed_volume(kind, x):
    if kind == TETRA:
        return float(np.dot(np.cross(x[1] - x[0], x[2] - x[0]), x[3] - x[0])) / 6.0
    vol = 0.0
    for f in HEX_FACES:  # divergence theorem, every quadrilateral as four triangles about its centre
        q = x[list(f)]
        c = q.mean(axis=0)
        for i in range(4):
            vol += float(np.dot(c, np.cross(q[i], q[(i + 1) % 4]))) / 6.0
    return vol


@pytest.mark.parametrize("encoding", ["ascii", "raw"])
def test_volume_file_round_trip(case, encoding):
    from orc_amd import io as orc_io
    name, md, a, nodes, d = case
    vert, fnp, fn = nodes
    n = md.n_cells
    arrays = special_arrays(n)
    path = str(d / ("vol_%s.vtu" % encoding))
    orc_io.write_vtu(path, md, arrays, encoding=encoding)
    out = read_vtu(path)
    assert out["n_cells"] == n and out["cell_data"] == ["s", "velocity"]
    for k, want in arrays.items():  # bit for bit
        assert np.array_equal(bits(cell_array(out, k, n)), bits(want)), k
    # only the used points, ascending, with their coordinates
    kinds, cell_faces = mesh_kinds(a, nodes)
    used = np.array(sorted(set(v for fl in cell_faces for f in fl for v in f)))
    assert out["n_points"] == len(used)
    pts = np.array(out["arrays"]["Points"][0]).reshape(-1, 3)
    assert out["arrays"]["Points"][1] == 3 and np.array_equal(bits(pts), bits(vert[used]))
    # types and their counts
    types = np.array(out["arrays"]["types"][0])
    assert np.array_equal(types, kinds)
    if name == "hex":
        assert set(types.tolist()) == {HEXAHEDRON}
    else:
        assert set(types.tolist()) == {TETRA, HEXAHEDRON, POLYHEDRON}
    conn, offs = np.array(out["arrays"]["connectivity"][0]), np.array(out["arrays"]["offsets"][0])
    assert len(offs) == n and offs[-1] == len(conn) and conn.min() >= 0 and conn.max() < len(used)
    vol = np.asarray(a["cell_volume"])
    begin = np.concatenate([[0], offs[:-1]])
    for c in range(n):
        ids = conn[begin[c]:offs[c]]
        assert set(used[ids].tolist()) == set(v for f in cell_faces[c] for v in f)
        if types[c] in (TETRA, HEXAHEDRON):
            assert len(ids) == (4 if types[c] == TETRA else 8)
            sv = signed_volume(types[c], pts[ids])
            assert sv > 0 and abs(sv - vol[c]) <= 1e-12 * vol[c], (c, int(types[c]), sv, vol[c])
    # the face streams
    if POLYHEDRON in types:
        stream, foff = out["arrays"]["faces"][0], out["arrays"]["faceoffsets"][0]
        assert len(foff) == n
        pos = 0
        for c in range(n):
            if types[c] != POLYHEDRON:
                assert foff[c] == -1
                continue
            nf = stream[pos]
            pos += 1
            got = []
            for _ in range(nf):
                k = stream[pos]
                got.append(used[stream[pos + 1:pos + 1 + k]].tolist())
                pos += 1 + k
            assert foff[c] == pos
            assert got == cell_faces[c], c  # the faces in the cell's order, the nodes in the face's
        assert pos == len(stream)
    else:
        assert "faces" not in out["arrays"]


@pytest.mark.parametrize("encoding", ["ascii", "raw"])
def test_face_file_round_trip(case, encoding):
    from orc_amd import io as orc_io
    from orc_amd.solver import BoundaryFields
    name, md, a, nodes, d = case
    vert, fnp, fn = nodes
    c1, fz = np.asarray(a["face_c1"]), np.asarray(a["face_zone"])
    Z = len(a["zone_type"])
    zones = [np.flatnonzero((c1 < 0) & (fz == z)) for z in range(Z)]
    faces = np.concatenate(zones).astype(np.int32)
    zp = np.concatenate([[0], np.cumsum([len(f) for f in zones])]).astype(np.int64)
    nb = len(faces)
    sp = special_arrays(nb)
    bf = BoundaryFields(zp, faces, {"pressure": sp["s"], "traction_x": sp["velocity"][:, 0], "traction_y": sp["velocity"][:, 1],
                                    "traction_z": sp["velocity"][:, 2]}, a["zone_names"])
    path = str(d / ("faces_%s.vtu" % encoding))
    orc_io.write_vtu_boundary(path, md, bf, extra_arrays={"extra": sp["s"][::-1]}, encoding=encoding)
    out = read_vtu(path)
    assert out["n_cells"] == nb and set(out["arrays"]["types"][0]) == {POLYGON}
    assert np.array_equal(bits(cell_array(out, "pressure", nb)), bits(sp["s"]))
    assert np.array_equal(bits(cell_array(out, "traction", nb)), bits(sp["velocity"]))
    assert np.array_equal(bits(cell_array(out, "extra", nb)), bits(sp["s"][::-1]))
    assert np.array_equal(cell_array(out, "zone", nb), np.repeat(np.arange(Z), np.diff(zp)).astype(np.float64))
    used = np.array(sorted(set(fn[fnp[f]:fnp[f + 1]][k] for f in faces for k in range(fnp[f + 1] - fnp[f]))))
    assert out["n_points"] == len(used) < len(vert)  # the interior points are absent
    pts = np.array(out["arrays"]["Points"][0]).reshape(-1, 3)
    assert np.array_equal(bits(pts), bits(vert[used]))
    conn, offs = out["arrays"]["connectivity"][0], out["arrays"]["offsets"][0]
    begin = [0] + offs[:-1]
    for i, f in enumerate(faces):
        assert used[conn[begin[i]:offs[i]]].tolist() == fn[fnp[f]:fnp[f + 1]].tolist()


# ------------------------------------------------------------------ the C entry directly: status codes
def c_call(nodes, a, path, **over):
    from orc_amd._lib import lib
    vert, fnp, fn = nodes
    F64, I64, I32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    n = len(a["cell_volume"])
    arg = dict(path=path.encode() if path is not None else None, n_points=len(vert), points=np.ascontiguousarray(vert),
               n_cells=n, cfp=np.ascontiguousarray(a["cell_face_ptr"], np.int64), cf=np.ascontiguousarray(a["cell_faces"], np.int64),
               fnp=np.ascontiguousarray(fnp, np.int64), fn=np.ascontiguousarray(fn, np.int64), n_arrays=1, names=[b"s"],
               components=np.array([1], np.int32), data=[np.arange(n, dtype=np.float64)], encoding=0)
    arg.update(over)
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
    names = None if arg["names"] is None else (C.c_char_p * len(arg["names"]))(*arg["names"])
    data = None if arg["data"] is None else (F64 * len(arg["data"]))(*[ptr(x, F64) for x in arg["data"]])
    return lib().orc_write_vtu(arg["path"], arg["n_points"], ptr(arg["points"], F64), arg["n_cells"], ptr(arg["cfp"], I64), ptr(arg["cf"], I64),
                               ptr(arg["fnp"], I64), ptr(arg["fn"], I64), arg["n_arrays"], names, ptr(arg["components"], I32), data, arg["encoding"])


def test_bad_arguments_and_unwritable_path(tmp_path):
    from orc_amd import io as orc_io
    from orc_amd.mesh import write_hex_channel_msh
    msh = str(tmp_path / "m.msh")
    write_hex_channel_msh(msh, 3, 2, 2)
    md = orc_io.read_mesh(msh)
    a, nodes = md.arrays(), md.nodes()
    vert, fnp, fn = nodes
    good = str(tmp_path / "ok.vtu")
    assert c_call(nodes, a, good) == 0
    assert c_call(nodes, a, good, n_arrays=0, names=None, components=None, data=None) == 0  # geometry alone
    # an unused point appended: absent from the file
    assert c_call((np.vstack([vert, [[9.0, 9.0, 9.0]]]), fnp, fn), a, good) == 0
    assert read_vtu(good)["n_points"] == len(vert)
    assert c_call(nodes, a, None) == BAD_ARGUMENT
    for over in (dict(points=None), dict(cfp=None), dict(cf=None), dict(fnp=None), dict(fn=None), dict(names=None),
                 dict(components=None), dict(data=None), dict(data=[None]), dict(encoding=2), dict(encoding=-1), dict(n_arrays=-1),
                 dict(components=np.array([0], np.int32)), dict(names=[b""]), dict(names=[b"a<b"]), dict(n_points=-1), dict(n_cells=-1)):
        assert c_call(nodes, a, good, **over) == BAD_ARGUMENT, over
    bad_fn = fn.copy(); bad_fn[5] = len(vert)
    assert c_call((vert, fnp, bad_fn), a, good) == BAD_ARGUMENT
    bad_fn[5] = -1
    assert c_call((vert, fnp, bad_fn), a, good) == BAD_ARGUMENT
    assert c_call(nodes, a, good, n_points=len(vert) - 1) == BAD_ARGUMENT  # the last node is out of range now
    bad_cf = np.asarray(a["cell_faces"], np.int64).copy(); bad_cf[3] = -2
    assert c_call(nodes, a, good, cf=bad_cf) == BAD_ARGUMENT
    bad_cfp = np.asarray(a["cell_face_ptr"], np.int64).copy(); bad_cfp[2] = bad_cfp[1] - 1
    assert c_call(nodes, a, good, cfp=bad_cfp) == BAD_ARGUMENT
    bad_fnp = fnp.copy(); bad_fnp[4] = bad_fnp[3] - 1
    assert c_call((vert, bad_fnp, fn), a, good) == BAD_ARGUMENT
    assert c_call(nodes, a, str(tmp_path / "no_such_dir" / "x.vtu")) == IO
    assert c_call(nodes, a, str(tmp_path)) == IO  # a directory
    with pytest.raises(Exception):
        orc_io.write_vtu(str(tmp_path / "no_such_dir" / "x.vtu"), md, {})
    with pytest.raises(ValueError):
        orc_io.write_vtu(good, md, {"short": np.zeros(md.n_cells - 1)})
