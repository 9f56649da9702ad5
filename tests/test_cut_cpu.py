"""Cut surfaces without a device: the restatement (tests/cut_restatement.py) closes its loops and its surface is closed; the inputs of
test_gpu_cut.py stay within the caps, so that its comparisons are not vacuous; the noisy iso-surface is as hard as it claims; the
polygon writer round-trips; every compute entry reports the missing device; orc_mesh_set_nodes checks its arrays (on the device
machine: there the host checks are reached)."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import cut_cases as K
import cut_restatement as CR
from test_vtu_cpu import bits, read_vtu

BAD_ARGUMENT, NO_DEVICE = 10, 11
F64, I64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)


def p(x, t=F64):
    return x.ctypes.data_as(t)


@pytest.fixture(scope="module", params=["hex_13x7x5", "mixed", "poly"])
def case(request, tmp_path_factory):
    a, nodes, md = K.host_case(tmp_path_factory.mktemp("cut_" + request.param), request.param)
    return request.param, a, nodes


def surfaces(name, a, nodes):
    """every plane and field test_gpu_cut.py cuts this mesh with -> [(label, restated surface)]"""
    out = [("oblique%d" % i, K.restated_plane(a, nodes, o, n)) for i, (o, n) in enumerate(K.oblique_planes(nodes))]
    if name.startswith("hex"):
        out += [(lab, K.restated_plane(a, nodes, o, n)) for lab, (o, n) in zip(("on_layer", "between"), K.axis_planes(nodes))]
        phi, level = K.distance_field(a, nodes)
        out.append(("smooth", CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, phi), level), K.max_points())))
        out.append(("noisy", CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, K.noisy_field(a)), 0.0), K.max_points())))
    return out


def test_limits_need_no_device():
    from orc_amd.mesh import cut_limits
    lim = cut_limits()
    assert lim["max_points"] >= 32 and lim["scan_chunk"] >= 64


def test_surfaces_are_closed_within_the_caps_and_the_noisy_case_is_hard(case):
    name, a, nodes = case
    fnp, fn = nodes[1], nodes[2]
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    # which faces hold a mesh edge (pair of consecutive cycle nodes)
    edge_faces = {}
    for f in range(len(fnp) - 1):
        cyc = [int(v) for v in fn[fnp[f]:fnp[f + 1]]]
        for j in range(len(cyc)):
            edge_faces.setdefault((min(cyc[j - 1], cyc[j]), max(cyc[j - 1], cyc[j])), set()).add(f)
    for label, s in surfaces(name, a, nodes):
        assert s["nonfinite"] == [] and s["overflow"] == [], label  # within the caps: the device comparisons are not vacuous
        assert len(s["cell"]) > 0, label
        assert np.all(np.diff(s["cell"]) >= 0) and np.all(np.diff(s["poly_ptr"]) >= 3), label
        # a polygon edge joins two cut points of ONE face; inside an interior face it occurs once in each direction (the two cells
        # see the face from opposite sides), in a boundary face once
        count = Counter(CR.welded_edges(s))
        for (ka, kb), k in count.items():
            shared = edge_faces[ka] & edge_faces[kb]
            assert len(shared) >= 1, (label, ka, kb)
            interior = [f for f in shared if c1[f] >= 0]
            if interior:
                assert k == 1 and count.get((kb, ka), 0) == 1, (label, ka, kb)
            else:
                assert k == 1 and (kb, ka) not in count, (label, ka, kb)
        if label == "noisy":
            assert s["faces_with_four_cuts"] >= 1 and s["cells_with_two_loops"] >= 1
        if label in ("on_layer", "between"):  # every cell of one layer once, every polygon a quadrilateral
            nx, ny, nz = (int(t) for t in name[4:].split("x"))
            assert len(s["cell"]) == ny * nz == len(set(s["cell"].tolist())) and np.all(np.diff(s["poly_ptr"]) == 4)


def test_prism_stack_counts():
    for n in (12, K.max_points() + 1):
        arrays, nodes = CR.prism_stack(n)
        s = CR.cut(arrays, nodes, CR.plane_d(nodes, (0.0, 0.0, 0.4e-3), (0.0, 0.0, 1.0)), K.max_points())
        if n == 12:
            assert s["overflow"] == [] and np.array_equal(s["poly_ptr"], [0, 12]) and s["cell"].tolist() == [0]
            assert s["area_vector"][0, 2] > 0  # the normal points toward increasing d
        else:
            assert s["overflow"] == [0] and len(s["cell"]) == 0
        both = CR.cut(arrays, nodes, CR.plane_d(nodes, (0.0, 0.0, 1e-3), (0.3, 0.0, 1.0)), 2 * n)  # oblique through the interior face
        assert sorted(set(both["cell"].tolist())) == [0, 1]


@pytest.mark.parametrize("encoding", ["ascii", "raw"])
def test_polygon_writer_round_trip(tmp_path, encoding):
    from orc_amd._lib import lib
    a, nodes, md = K.host_case(tmp_path, "hex_3x2x2")
    o, n = K.oblique_planes(nodes)[0]
    s = K.restated_plane(a, nodes, o, n)
    uniq, first, inv = np.unique(s["keys"], axis=0, return_index=True, return_inverse=True)
    pts = np.ascontiguousarray(s["points"][first])
    conn = np.ascontiguousarray(np.asarray(inv).reshape(-1), np.int64)
    ptr = np.ascontiguousarray(s["poly_ptr"], np.int64)
    P, M = len(s["cell"]), len(pts)
    rng = np.random.default_rng(5)
    special = np.array([np.nan, np.inf, -0.0, 5e-324])
    cell_s = rng.standard_normal(P)
    cell_s[:min(P, 4)] = special[:min(P, 4)]
    cell_v = np.ascontiguousarray(rng.standard_normal((3, P)))  # component-major
    point_s = rng.standard_normal(M)
    point_s[-min(M, 4):] = special[:min(M, 4)]
    path = str(tmp_path / ("cut_%s.vtu" % encoding))
    cn = (C.c_char_p * 2)(b"area", b"flux")
    cc = np.array([1, 3], np.int32)
    cd = (F64 * 2)(p(cell_s), p(cell_v))
    pn = (C.c_char_p * 1)(b"phi")
    pc = np.array([1], np.int32)
    pd = (F64 * 1)(p(point_s))
    call = lambda **kw: lib().orc_write_vtu_polygons(kw.get("path", path).encode(), M, p(pts), P, p(kw.get("ptr", ptr), I64), p(kw.get("conn", conn), I64), 2, cn, p(cc, C.POINTER(C.c_int32)), cd, 1, pn,
                                                     p(pc, C.POINTER(C.c_int32)), pd, {"ascii": 0, "raw": 1}[encoding])
    assert call() == 0
    out = read_vtu(path)
    assert out["n_points"] == M and out["n_cells"] == P
    arr = out["arrays"]
    assert np.array_equal(bits(arr["Points"][0]), bits(pts.reshape(-1))) and arr["Points"][1] == 3
    assert arr["connectivity"][0] == conn.tolist() and arr["offsets"][0] == ptr[1:].tolist() and arr["types"][0] == [7] * P
    assert np.array_equal(bits(arr["area"][0]), bits(cell_s)) and arr["area"][1] == 1
    assert np.array_equal(bits(arr["flux"][0]), bits(cell_v.T.reshape(-1))) and arr["flux"][1] == 3
    assert np.array_equal(bits(arr["phi"][0]), bits(point_s))
    assert sorted(out["cell_data"]) == ["area", "flux"]
    # refused: a node past the points, a polygon of two nodes, a point no polygon uses, an unwritable path
    bad = conn.copy()
    bad[0] = M
    assert call(conn=bad) == BAD_ARGUMENT
    short = ptr.copy()
    short[1] = 2
    assert call(ptr=short) == BAD_ARGUMENT
    unused = np.where(conn == conn[0], conn[1], conn)
    assert call(conn=np.ascontiguousarray(unused)) == BAD_ARGUMENT
    assert call(path=str(tmp_path / "no_such_dir" / "x.vtu")) == 13


def test_entries_report_a_missing_device_or_check_their_arguments():
    """without a device every compute entry returns ORC_ERR_NO_DEVICE whatever the arguments; with one, the same null arguments are
    ORC_ERR_BAD_ARGUMENT"""
    import orc_amd
    from orc_amd._lib import lib
    L = lib()
    want = NO_DEVICE if orc_amd.device_count() == 0 else BAD_ARGUMENT
    st = C.c_int(0)
    v = (C.c_double * 3)(0.0, 0.0, 1.0)
    assert L.orc_mesh_set_nodes(None, 1, v, 0, None, None) == want
    assert L.orc_mesh_node_average(None, None, None) == want
    for make in (lambda: L.orc_cut_plane(None, v, v, C.byref(st)), lambda: L.orc_cut_node_level(None, v, 0.0, C.byref(st)),
                 lambda: L.orc_cut_cell_field(None, v, 0.0, C.byref(st)), lambda: L.orc_solver_cut_field(None, 1, 0.0, C.byref(st))):
        st.value = 0
        assert make() is None and st.value == want
    assert L.orc_cut_sizes(None, None, None, None, None) == want
    assert L.orc_cut_get(None, None, None, None, None, None, None) == want
    assert L.orc_solver_sample_cut(None, None, 1, 0, None) == want
    assert L.orc_cut_sample_cells(None, 1, None, None) == want
    ms = (C.c_double * 4)()
    assert L.orc_bench_cut(None, None, v, v, 1, ms) == want
    L.orc_cut_destroy(None)
    cap, chunk = C.c_int32(0), C.c_int32(0)
    assert L.orc_cut_limits(C.byref(cap), C.byref(chunk)) == 0 and cap.value >= 32 and chunk.value >= 64  # host only: no device needed
