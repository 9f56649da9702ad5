"""Volume reports without a device: the numpy restatement (tests/group_restatement.py) against exact facts on the hex channel and the
polyhedral writer's mesh, the bin and box labels against brute force, the Python mirror (GroupReport, the label checks) and every
refusal that needs no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import group_restatement as R
from conftest import ROOT, splitmix64_uniform


def hex_arrays(nx=6, ny=8, nz=3):
    from orc_amd.mesh import hex_channel
    return hex_channel(nx, ny, nz)


def poly_arrays(tmp_path):
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, write_mixed_channel_msh
    path = str(tmp_path / "poly.msh")
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=True)
    return MeshArrays(orc_io.read_mesh(path).arrays())


@pytest.fixture(params=["hex", "poly"])
def arrays(request, tmp_path):
    return hex_arrays() if request.param == "hex" else poly_arrays(tmp_path)


def scattered_ids(n, n_groups, seed=11, free=0.2):
    """labels in [-1, n_groups) from splitmix64 noise: about `free` of the cells in no group"""
    r = 0.5 * (splitmix64_uniform(n, seed) + 1.0)
    ids = np.floor(r * n_groups / (1.0 - free)).astype(np.int32)
    ids[ids >= n_groups] = -1
    return ids


# ------------------------------------------------------------------ the restatement against exact facts
def test_lists_ascend_in_orc_id_and_partition_the_listed_cells(arrays):
    n = arrays.n_cells
    ids = scattered_ids(n, 5)
    gp, cells = R.lists(ids, 5)
    assert gp[0] == 0 and gp[-1] == np.count_nonzero(ids >= 0) == len(cells)
    for g in range(5):
        c = cells[gp[g]:gp[g + 1]]
        assert np.all(np.diff(c) > 0) and np.all(ids[c] == g)
    assert np.array_equal(np.sort(cells), np.flatnonzero(ids >= 0))
    assert np.array_equal(R.chunks_of(np.array([0, 0, 1, 2049, 4097]), 2048), [0, 1, 1, 1])


def test_weights_of_the_groups_and_the_rest_make_the_total_volume(arrays):
    n, vol = arrays.n_cells, np.asarray(arrays["cell_volume"])
    ids = scattered_ids(n, 7)
    rep = R.report(ids, 7, vol, np.ones((1, n)))
    total = math.fsum(rep["W"].tolist() + vol[ids < 0].tolist())
    exact = math.fsum(vol.tolist())
    assert abs(total - exact) <= 8 * R.EPS * exact  # seven exactly rounded partial sums and their exactly rounded sum
    # x = 1: t1 = w * 1 = w and t2 = t1 * 1 = w, bit for bit, so SUM = SUM_SQ = W
    assert np.array_equal(rep["S"][:, 0, R.SUM], rep["W"]) and np.array_equal(rep["S"][:, 0, R.SUM_SQ], rep["W"])
    assert np.array_equal(rep["count"], np.bincount(ids[ids >= 0], minlength=7))
    unit = R.report(ids, 7, vol, np.ones((1, n)), "unit")
    assert np.array_equal(unit["W"], rep["count"].astype(np.float64))


def test_centroid_coordinate_gives_the_group_centroid(arrays):
    n, vol, cc = arrays.n_cells, np.asarray(arrays["cell_volume"]), np.asarray(arrays["cell_centroid"])
    ids = scattered_ids(n, 3)
    rep = R.report(ids, 3, vol, cc.T.copy())
    for g in range(3):
        sel = ids == g
        want = (vol[sel, None] * cc[sel]).sum(axis=0) / vol[sel].sum()
        got = rep["S"][g, :, R.SUM] / rep["W"][g]
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)


def test_centroid_of_a_box_on_the_hex_mesh_is_analytic():
    from orc_amd.mesh import box_ids
    nx, ny, nz, lx, ly = 8, 6, 4, 0.002, 0.001
    a = hex_arrays(nx, ny, nz)
    lz = 1e-4 * nz
    cc, vol = np.asarray(a["cell_centroid"]), np.asarray(a["cell_volume"])
    # the box of the cells i in [2, 6), j in [1, 4), k in [0, 2): its faces lie on cell faces, so its centroid is the box's centre
    lo = np.array([2 * lx / nx, 1 * ly / ny, 0.0]) - 1e-12
    hi = np.array([6 * lx / nx, 4 * ly / ny, 2 * lz / nz]) - 1e-12
    ids = box_ids(cc, lo, hi)
    assert np.count_nonzero(ids == 0) == 4 * 3 * 2
    rep = R.report(ids, 1, vol, cc.T.copy())
    centre = np.array([4 * lx / nx, 2.5 * ly / ny, 1 * lz / nz])
    assert np.allclose(rep["S"][0, :, R.SUM] / rep["W"][0], centre, rtol=1e-12, atol=0.0)
    assert math.isclose(rep["W"][0], 24 * (lx / nx) * (ly / ny) * (lz / nz), rel_tol=1e-12)


def test_unit_weighting_of_integer_fields_is_integer_arithmetic(arrays):
    n = arrays.n_cells
    ids = scattered_ids(n, 4)
    x = np.round(1024 * splitmix64_uniform(n, 5)).astype(np.int64)
    rep = R.report(ids, 4, arrays["cell_volume"], x.astype(np.float64)[None, :], "unit")
    for g in range(4):
        sel = ids == g
        assert rep["W"][g] == np.count_nonzero(sel)
        assert rep["S"][g, 0, R.SUM] == int(x[sel].sum()) and rep["S"][g, 0, R.SUM_SQ] == int((x[sel] * x[sel]).sum())
        assert rep["S"][g, 0, R.MIN] == x[sel].min() and rep["S"][g, 0, R.MAX] == x[sel].max()
        assert rep["where"][g, 0, 0] == np.flatnonzero(sel & (x == x[sel].min()))[0]
        assert rep["where"][g, 0, 1] == np.flatnonzero(sel & (x == x[sel].max()))[0]


def test_extrema_rules_of_the_restatement():
    ids = np.array([0, 0, 0, 1, 1, 2, 2, -1], np.int32)
    x = np.array([3.0, 1.0, 1.0, np.nan, np.nan, np.nan, -0.0, -9.0])
    rep = R.report(ids, 4, np.ones(8), x[None, :])
    assert rep["S"][0, 0, R.MIN] == 1.0 and rep["where"][0, 0, 0] == 1  # equal values: the smallest ORC id
    assert rep["S"][0, 0, R.MAX] == 3.0 and rep["where"][0, 0, 1] == 0
    assert rep["S"][1, 0, R.MIN] == np.inf and rep["S"][1, 0, R.MAX] == -np.inf and list(rep["where"][1, 0]) == [-1, -1]  # NaN only
    assert np.isnan(rep["S"][1, 0, R.SUM]) and np.isnan(rep["S"][2, 0, R.SUM_SQ])
    assert rep["S"][2, 0, R.MIN] == 0.0 and list(rep["where"][2, 0]) == [6, 6]  # a NaN never wins
    assert rep["S"][3, 0, R.MIN] == np.inf and rep["S"][3, 0, R.MAX] == -np.inf and list(rep["where"][3, 0]) == [-1, -1]  # no cell
    assert rep["count"][3] == 0 and rep["W"][3] == 0.0 and rep["S"][3, 0, R.SUM] == 0.0


def test_depth_counts_the_association():
    # one chunk: the lane's slots, the wave tree, the waves, fsum; 5 chunks: three levels of the pairwise fold more
    assert R.depth(np.array([1, 2048, 2049, 5 * 2048]), 2048, 8).tolist() == [19.0, 19.0, 20.0, 22.0]
    assert R.bound(np.array([[1.0, 2.0]]), np.array([1]), 2048, 8).tolist() == [[19 * R.EPS, 38 * R.EPS]]


# ------------------------------------------------------------------ bins and boxes against brute force
def test_bin_ids_against_brute_force_with_edge_values(arrays):
    from orc_amd.mesh import bin_ids
    cc = np.asarray(arrays["cell_centroid"])
    y = np.unique(cc[:, 1])
    # edges ON centroid values: the lower edge belongs to the bin, the upper one to the next; the last edge is outside
    edges = np.array([y[0], y[len(y) // 3], y[len(y) // 2], y[-1]])
    ids, nb = bin_ids(cc, (0.0, 1.0, 0.0), edges)
    assert nb == 3 and ids.dtype == np.int32
    for c in range(len(cc)):
        s = cc[c, 1]
        want = -1
        for k in range(3):
            if edges[k] <= s < edges[k + 1]:
                want = k
        assert ids[c] == want, (c, s)
    assert np.all(ids[cc[:, 1] == y[-1]] == -1) and np.all(ids[cc[:, 1] == y[0]] == 0)
    assert np.all(ids[cc[:, 1] == y[len(y) // 3]] == 1)
    # an oblique direction is normalised; s is formed as (x dx + y dy) + z dz
    d = np.array([1.0, 2.0, -0.5])
    dn = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    s = (cc[:, 0] * dn[0] + cc[:, 1] * dn[1]) + cc[:, 2] * dn[2]
    edges = np.linspace(s.min(), s.max(), 6)
    ids, nb = bin_ids(cc, d, edges)
    want = np.full(len(cc), -1)
    for k in range(5):
        want[(edges[k] <= s) & (s < edges[k + 1])] = k
    assert nb == 5 and np.array_equal(ids, want) and ids[np.argmax(s)] == -1
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, np.nan]):
        with pytest.raises(ValueError):
            bin_ids(cc, (0, 1, 0), bad)
    with pytest.raises(ValueError):
        bin_ids(cc, (0, 0, 0), [0.0, 1.0])


def test_box_ids_against_brute_force_with_edge_values(arrays):
    from orc_amd.mesh import box_ids
    cc = np.asarray(arrays["cell_centroid"])
    lo, hi = cc[len(cc) // 3].copy(), cc.max(axis=0)  # lo ON a centroid (inside), hi ON the largest coordinates (outside)
    ids = box_ids(cc, lo, hi)
    want = np.array([0 if all(lo[k] <= c[k] < hi[k] for k in range(3)) else -1 for c in cc])
    assert np.array_equal(ids, want) and ids.dtype == np.int32
    assert ids[len(cc) // 3] == 0 or np.any(cc[len(cc) // 3] >= hi)
    assert np.all(ids[np.any(cc == hi[None, :], axis=1)] == -1)


# ------------------------------------------------------------------ the Python mirror
def test_group_report_object_views_and_derived_values():
    from orc_amd.solver import GroupReport
    sums = np.zeros((3, 2, 4))
    sums[0, 0] = [6.0, 14.0, 1.0, 3.0]   # w = 1, x = 1, 2, 3
    sums[0, 1] = [-4.0, 8.0, -2.0, 0.0]
    sums[1, 0] = [1.0, 0.5, 0.5, 0.5]    # w = 2, x = 0.5
    sums[2] = [0.0, 0.0, np.inf, -np.inf]
    weight = np.array([[3.0, 3], [2.0, 1], [0.0, 0]])
    where = np.array([[[0, 2], [5, 7]], [[4, 4], [4, 4]], [[-1, -1], [-1, -1]]])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an empty group gives NaN without a warning
        r = GroupReport(["u", "p"], sums, weight, where)
        assert r.names == ["u", "p"] and r.column("p") == 1
        assert r.weight.tolist() == [3.0, 2.0, 0.0] and r.count.tolist() == [3, 1, 0] and r.count.dtype == np.int64
        assert r.sum[0].tolist() == [6.0, -4.0] and r.sum_sq[0, 0] == 14.0 and r.min[0, 1] == -2.0 and r.max[0, 0] == 3.0
        assert r.argmin[0].tolist() == [0, 5] and r.argmax[0].tolist() == [2, 7] and r.argmin[2].tolist() == [-1, -1]
        assert r.mean[0, 0] == 2.0 and r.variance[0, 0] == 14.0 / 3.0 - 4.0 and r.rms[0, 0] == math.sqrt(14.0 / 3.0)
        assert r.mean[1, 0] == 0.5 and r.variance[1, 0] == 0.0
        assert np.all(np.isnan(r.mean[2])) and np.all(np.isnan(r.variance[2])) and np.all(np.isnan(r.rms[2]))


def test_label_checks_of_the_python_mirror():
    from orc_amd.mesh import check_group_ids
    from orc_amd.solver import _weighting
    ids, G = check_group_ids(np.array([0, 2, -1, 1]), 4)
    assert G == 3 and ids.dtype == np.int32 and ids.flags.c_contiguous
    assert check_group_ids(np.array([-1, -1]), 2)[1] == 1
    assert check_group_ids(np.array([0, 0]), 2, n_groups=5)[1] == 5
    for bad_ids, n, g in ((np.array([0, 1]), 3, None), (np.array([0, -2]), 2, None), (np.array([0, 3]), 2, 3), (np.array([0.0, 1.0]), 2, None),
                          (np.array([0, 0]), 2, 0), (np.zeros((2, 1), int), 2, None)):
        with pytest.raises(ValueError):
            check_group_ids(bad_ids, n, g)
    assert _weighting("volume") == 0 and _weighting("Unit") == 1 and _weighting(1) == 1
    with pytest.raises(KeyError):
        _weighting("mass")


# ------------------------------------------------------------------ the library without a device
def test_library_exports_the_group_entries():
    """fails on a library built before the volume reports existed"""
    import orc_amd
    from orc_amd._lib import lib
    from orc_amd.mesh import group_limits
    L = lib()
    names = ("orc_cell_groups_create", "orc_cell_groups_destroy", "orc_cell_groups_count", "orc_cell_groups_get", "orc_group_limits",
             "orc_solver_group_report", "orc_group_integrals", "orc_solver_group_statistics", "orc_solver_set_group_history",
             "orc_solver_record_groups", "orc_solver_group_history_count", "orc_solver_group_history", "orc_bench_group_report")
    for name in names:
        assert hasattr(L, name), name
    # the header's enums and the Python mirror agree
    txt = open(os.path.join(ROOT, "include", "orc_types.h")).read()
    for name, value in (("SUM", R.SUM), ("SUM_SQ", R.SUM_SQ), ("MIN", R.MIN), ("MAX", R.MAX), ("WEIGHT_VOLUME", 0), ("WEIGHT_UNIT", 1)):
        assert "ORC_GROUP_%s = %d" % (name, value) in txt, name
    lim = group_limits()  # needs no device
    assert lim["fields"] >= 1 and lim["chunk"] == 256 * lim["slots"] and lim["max_groups"] >= 1 << 16
    # argument checks that need no mesh: without a device every compute entry says so, with one a null argument is a bad argument
    want = 11 if orc_amd.device_count() < 1 else 10
    st = C.c_int(0)
    assert L.orc_cell_groups_create(None, C.c_int32(1), None, C.byref(st)) is None and st.value == want
    assert L.orc_solver_group_report(None, None, C.c_uint32(1), C.c_int32(0), None, None, None) == want
    assert L.orc_group_integrals(None, None, C.c_int32(1), None, C.c_int32(0), None, None, None) == want
    assert L.orc_solver_group_statistics(None, None, C.c_uint32(1), C.c_int32(0), C.c_int32(0), None, None, None) == want
    assert L.orc_solver_set_group_history(None, None, C.c_uint32(1), C.c_int32(0), C.c_uint64(1)) == want
    assert L.orc_solver_record_groups(None, C.c_double(0.0)) == want
    assert L.orc_solver_group_history_count(None) == -1
    assert L.orc_solver_group_history(None, C.c_uint64(0), C.c_uint64(0), None, None, None, None) == want
    assert L.orc_cell_groups_count(None) == 0 and L.orc_cell_groups_get(None, None, None, None) == 10
    L.orc_cell_groups_destroy(None)
