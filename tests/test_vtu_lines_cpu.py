"""orc_write_vtu_lines (orc_amd/csrc/vtk_io.cpp): polylines with point data as a VTK XML UnstructuredGrid — the ASCII file parsed back
with xml.etree, the appended-raw file holding the same arrays, and the refusals.  Host only."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np

BAD_ARGUMENT, IO = 10, 13
DTYPES = {"Float64": np.float64, "Int64": np.int64, "UInt8": np.uint8}


def three_lines():
    """lines of 1, 2 and 7 points, one scalar and one 3-component array per point, none of the values short in decimal"""
    rng = np.random.RandomState(5)
    lines = [rng.standard_normal((m, 3)) / 3.0 for m in (1, 2, 7)]
    return lines, {"age": rng.standard_normal(10) * 1e-3, "velocity": rng.standard_normal((10, 3)) / 7.0}


def read_ascii(path):
    root = ET.parse(path).getroot()
    piece = root.find("UnstructuredGrid/Piece")
    out = {"n_points": int(piece.get("NumberOfPoints")), "n_cells": int(piece.get("NumberOfCells"))}
    for da in piece.iter("DataArray"):
        assert da.get("format") == "ascii"
        out[da.get("Name")] = np.array([float(t) if da.get("type") == "Float64" else int(t) for t in da.text.split()], DTYPES[da.get("type")])
    out["point_data"] = [da.get("Name") for da in piece.find("PointData")]
    return out


def read_raw(path):
    blob = open(path, "rb").read()
    mark = b'<AppendedData encoding="raw">\n_'
    head, data = blob[:blob.index(mark)], blob[blob.index(mark) + len(mark):]
    piece = ET.fromstring(head + b"</VTKFile>").find("UnstructuredGrid/Piece")
    out = {"n_points": int(piece.get("NumberOfPoints")), "n_cells": int(piece.get("NumberOfCells"))}
    for da in piece.iter("DataArray"):
        assert da.get("format") == "appended"
        o = int(da.get("offset"))
        nbytes = int(np.frombuffer(data[o:o + 8], np.uint64)[0])
        out[da.get("Name")] = np.frombuffer(data[o + 8:o + 8 + nbytes], DTYPES[da.get("type")])
    return out


def test_ascii_round_trip_of_three_lines(tmp_path):
    from orc_amd import io as orc_io
    lines, data = three_lines()
    path = str(tmp_path / "lines.vtu")
    orc_io.write_vtu_lines(path, lines, data, encoding="ascii")
    got = read_ascii(path)
    assert got["n_points"] == 10 and got["n_cells"] == 3
    assert np.array_equal(got["connectivity"], np.arange(10)) and np.array_equal(got["offsets"], [1, 3, 10])
    assert np.array_equal(got["types"], [1, 4, 4])  # VTK_VERTEX, VTK_POLY_LINE
    assert np.array_equal(got["Points"].view(np.uint64), np.concatenate(lines).ravel().view(np.uint64))  # %.17g: exact
    assert np.array_equal(got["age"].view(np.uint64), data["age"].view(np.uint64))
    assert np.array_equal(got["velocity"].view(np.uint64), data["velocity"].ravel().view(np.uint64))
    assert got["point_data"] == ["age", "velocity"]
    root = ET.parse(path).getroot()
    comps = {da.get("Name"): da.get("NumberOfComponents") for da in root.iter("DataArray")}
    assert comps["velocity"] == "3" and comps["Points"] == "3"


def test_appended_raw_file_has_the_same_arrays(tmp_path):
    from orc_amd import io as orc_io
    lines, data = three_lines()
    pa, pr = str(tmp_path / "a.vtu"), str(tmp_path / "r.vtu")
    orc_io.write_vtu_lines(pa, lines, data, encoding="ascii")
    orc_io.write_vtu_lines(pr, lines, data)  # raw is the default
    a, r = read_ascii(pa), read_raw(pr)
    for k in ("Points", "connectivity", "offsets", "types", "age", "velocity"):
        assert a[k].dtype == r[k].dtype and np.array_equal(a[k].view(np.uint8), r[k].view(np.uint8)), k
    assert (a["n_points"], a["n_cells"]) == (r["n_points"], r["n_cells"])
    orc_io.write_vtu_lines(str(tmp_path / "bare.vtu"), lines, encoding="ascii")  # no arrays at all
    assert read_ascii(str(tmp_path / "bare.vtu"))["point_data"] == []


def test_refusals(tmp_path):
    from orc_amd._lib import lib
    L = lib()
    pts = np.zeros((10, 3))
    f64, i64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)), lambda v: v.ctypes.data_as(C.POINTER(C.c_int64))
    path = str(tmp_path / "x.vtu").encode()
    good, decreasing, empty = np.array([0, 1, 3, 10], np.int64), np.array([0, 3, 1, 10], np.int64), np.array([0, 3, 3, 10], np.int64)
    assert L.orc_write_vtu_lines(path, 3, i64(decreasing), f64(pts), 0, None, None, None, 0) == BAD_ARGUMENT
    assert L.orc_write_vtu_lines(path, 3, i64(empty), f64(pts), 0, None, None, None, 0) == BAD_ARGUMENT
    assert L.orc_write_vtu_lines(path, 3, i64(good), None, 0, None, None, None, 0) == BAD_ARGUMENT
    assert L.orc_write_vtu_lines(path, 3, None, f64(pts), 0, None, None, None, 0) == BAD_ARGUMENT
    assert L.orc_write_vtu_lines(None, 3, i64(good), f64(pts), 0, None, None, None, 0) == BAD_ARGUMENT
    assert L.orc_write_vtu_lines(path, 3, i64(good), f64(pts), 0, None, None, None, 2) == BAD_ARGUMENT  # unknown encoding
    assert not (tmp_path / "x.vtu").exists()
    nowhere = str(tmp_path / "no_such_directory" / "x.vtu").encode()
    assert L.orc_write_vtu_lines(nowhere, 3, i64(good), f64(pts), 0, None, None, None, 0) == IO
    assert L.orc_write_vtu_lines(path, 3, i64(good), f64(pts), 0, None, None, None, 0) == 0
