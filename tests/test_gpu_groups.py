"""Volume reports on the device (orc_amd/csrc/groups.hip) against the numpy restatement of tests/group_restatement.py: the lists at the
chunk and lane edges, the sums within the derived bound, exact integer sums, the extrema and their cells bit for bit, independence of
the mesh's numbering and of the labels, the live solver, the running statistics, the history of a transient run, arguments.

Every comparison of a sum with the restatement uses the DERIVED bound of group_restatement.bound():
    |device - fsum| <= D * 2^-53 * sum |term|,   D = lane slots + 6 + waves + ceil(log2(chunks)) + 1
counted there from the association (a lane's slots in sequence, the wave tree, the four waves in sequence, the pairwise fold of the
chunks, fsum's own rounding); both sides form a term with the same rounded multiplies.  Bit for bit means equal uint64 views."""
import ctypes as C

import numpy as np
import pytest

import group_restatement as R
from conftest import splitmix64_uniform
from test_gpu_surface import hex_case, mixed_case, seeded_fields
from test_gpu_transient import channel_flow, settings, transient

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
BICGSTAB = 3
RHO, MU = 1000.0, 1e-3
N_EDGE_GROUPS = 12


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def same_report(a, b):
    return (same_bits(a.raw, b.raw) and same_bits(a.weight, b.weight) and np.array_equal(a.count, b.count) and
            np.array_equal(a.where, b.where))


def limits():
    from orc_amd.mesh import group_limits
    return group_limits()


def edge_ids(n, chunk, seed=71):
    """groups of 0, 1, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 cells, the cells handed out along a seeded
    permutation (scattered lists); the cells left over are in no group"""
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert sum(sizes) < n, (sum(sizes), n)
    perm = np.argsort(splitmix64_uniform(n, seed), kind="stable")
    ids = np.full(n, -1, np.int32)
    at = 0
    for g, k in enumerate(sizes):
        ids[perm[at:at + k]] = g
        at += k
    return ids, sizes


def scattered_ids(n, n_groups, seed=11, free=0.15):
    r = 0.5 * (splitmix64_uniform(n, seed) + 1.0)
    ids = np.floor(r * n_groups / (1.0 - free)).astype(np.int32)
    ids[ids >= n_groups] = -1
    return ids


def rough_fields(a, F):
    """F fields: splitmix64 noise on a rough (per-cell oscillating) base, different scales and signs"""
    n = a.n_cells
    y = np.asarray(a["cell_centroid"])[:, 1]
    out = []
    for k in range(F):
        base = (0.05 * (k + 1)) * (np.sin(1.7 * np.arange(n) + k) + 0.3 * k - 0.2) + 40.0 * (k % 2) * y
        out.append(base * (1.0 + 0.5 * splitmix64_uniform(n, 100 + k)))
    return np.array(out)


def named(fields):
    return {"f%d" % k: x for k, x in enumerate(fields)}


@pytest.fixture(scope="module")
def cases(gpu, tmp_path_factory):
    """the two meshes, their label sets and group sets, built once"""
    lim = limits()
    a_hex, m_hex = hex_case(24, 24, 20)
    ids_hex, sizes = edge_ids(a_hex.n_cells, lim["chunk"])
    a_poly, m_poly = mixed_case(tmp_path_factory.mktemp("groups"), True)
    ids_poly = scattered_ids(a_poly.n_cells, 5)
    return dict(lim=lim, sizes=sizes,
                hex=(a_hex, m_hex, ids_hex, N_EDGE_GROUPS, m_hex.cell_groups(ids_hex, N_EDGE_GROUPS)),
                poly=(a_poly, m_poly, ids_poly, 5, m_poly.cell_groups(ids_poly, 5)))


_WANT = {}


def restated(cases, name, weighting):
    """the restatement of the case's KF + 1 rough fields, computed once per (mesh, weighting) and never changed"""
    key = (name, weighting)
    if key not in _WANT:
        a, _, ids, G, _ = cases[name]
        f = rough_fields(a, cases["lim"]["fields"] + 1)
        _WANT[key] = (f, R.report(ids, G, a["cell_volume"], f, weighting))
    return _WANT[key]


def columns(want, F):
    out = dict(want)
    out["S"], out["Sabs"], out["where"] = want["S"][:, :F], want["Sabs"][:, :F], want["where"][:, :F]
    return out


# ------------------------------------------------------------------ 1. chunk and lane edges
def test_lists_at_the_chunk_and_lane_edges_equal_the_restatement(cases):
    a, m, ids, G, groups = cases["hex"]
    lim = cases["lim"]
    assert groups.chunk == lim["chunk"] and len(groups) == G == len(cases["sizes"])
    assert a.n_cells <= 11520 and np.count_nonzero(ids < 0) > 0
    gp, cells = R.lists(ids, G)
    assert np.array_equal(np.diff(gp), cases["sizes"])
    assert np.array_equal(groups.group_ptr, gp) and np.array_equal(groups.cells, cells)
    assert groups.group_ptr.dtype == np.int64 and groups.cells.dtype == np.int64
    for g in range(G):
        assert np.all(np.diff(groups.cells[gp[g]:gp[g + 1]]) > 0)  # ascending in ORC id, though handed out by a permutation
    assert not np.all(np.diff(np.flatnonzero(ids == 11)) == 1)     # the lists are scattered over the mesh
    # the same labels on a reordered mesh give the same lists: they speak ORC order
    _, m_rcm = hex_case(24, 24, 20, ordering=1)
    g_rcm = m_rcm.cell_groups(ids, G)
    assert np.array_equal(g_rcm.group_ptr, gp) and np.array_equal(g_rcm.cells, cells)


# ------------------------------------------------------------------ 2. sums within the derived bound
@pytest.mark.parametrize("n_fields", ["one", "launch", "launch_plus_one"])
@pytest.mark.parametrize("weighting", ["volume", "unit"])
@pytest.mark.parametrize("name", ["hex", "poly"])
def test_sums_lie_within_the_derived_bound(cases, name, weighting, n_fields):
    from orc_amd.solver import group_integrals
    a, m, ids, G, groups = cases[name]
    lim = cases["lim"]
    F = {"one": 1, "launch": lim["fields"], "launch_plus_one": lim["fields"] + 1}[n_fields]
    f, want = restated(cases, name, weighting)
    rep = group_integrals(m, groups, named(f[:F]), weighting)
    assert rep.raw.shape == (G, F, 4) and rep.names == ["f%d" % k for k in range(F)]
    worst = R.check(rep, columns(want, F), lim["chunk"], lim["slots"])
    print("%s %s F=%d: worst error / bound = %.3f" % (name, weighting, F, worst))
    if weighting == "unit":
        assert np.array_equal(rep.weight, rep.count.astype(np.float64))
    # the derived values of the Python mirror
    full = rep.count > 0
    assert np.all(np.isnan(rep.mean[~full])) and np.all(np.isfinite(rep.mean[full]))
    assert np.allclose(rep.mean[full], want["S"][full, :F, R.SUM] / want["W"][full, None], rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------ 3. exactness
def test_unit_weighting_of_integer_fields_is_exact_in_every_bit(cases):
    from orc_amd.solver import group_integrals
    a, m, ids, G, groups = cases["hex"]
    n = a.n_cells
    F = cases["lim"]["fields"] + 1
    x = np.array([np.round(1024 * splitmix64_uniform(n, 40 + k)) for k in range(F)])
    assert np.abs(x).max() <= 1024 and np.abs(x).max() > 1000
    rep = group_integrals(m, groups, named(x), "unit")
    xi = x.astype(np.int64)
    for g in range(G):
        sel = ids == g
        assert rep.weight[g] == rep.count[g] == np.count_nonzero(sel)
        for k in range(F):
            assert rep.sum[g, k] == int(xi[k][sel].sum()) and rep.sum_sq[g, k] == int((xi[k][sel] * xi[k][sel]).sum()), (g, k)


# ------------------------------------------------------------------ 4. extrema and their cells
def test_extrema_and_their_cells_bit_for_bit(cases):
    from orc_amd.solver import group_integrals
    a, m, ids, G, groups = cases["hex"]
    lim = cases["lim"]
    n = a.n_cells
    noise = splitmix64_uniform(n, 51)
    coarse = np.round(4 * splitmix64_uniform(n, 52)) / 4  # nine values: ties everywhere
    const = np.full(n, -0.75)
    nan_one = noise.copy()
    victim = int(np.flatnonzero(ids == 9)[17])   # one NaN in the group of `chunk` cells
    nan_one[victim] = np.nan
    nan_all = noise.copy()
    nan_all[ids == 5] = np.nan                   # the group of 255 cells holds NaN only
    inf = coarse.copy()
    inf[ids == 3] = np.inf                       # +inf in every cell of a group: the minimum is +inf AT its first cell
    f = np.array([noise, coarse, const, nan_one, nan_all, inf])
    want = R.report(ids, G, a["cell_volume"], f, "volume")
    rep = group_integrals(m, groups, named(f), "volume")
    R.check(rep, want, lim["chunk"], lim["slots"])
    gp = groups.group_ptr
    for g in range(1, G):
        first = groups.cells[gp[g]]
        assert rep.argmin[g, 2] == first and rep.argmax[g, 2] == first  # a constant field: the group's smallest ORC id
        assert rep.min[g, 2] == rep.max[g, 2] == -0.75
    assert list(rep.where[0].ravel()) == [-1] * 12 and np.all(rep.min[0] == np.inf) and np.all(rep.max[0] == -np.inf)  # no cell
    assert rep.argmin[9, 3] != victim and rep.argmax[9, 3] != victim and np.isfinite(rep.min[9, 3]) and np.isfinite(rep.max[9, 3])
    assert np.isnan(rep.sum[9, 3]) and np.isnan(rep.sum_sq[9, 3]) and not np.isnan(rep.sum[8, 3])
    assert rep.min[5, 4] == np.inf and rep.max[5, 4] == -np.inf and list(rep.where[5, 4]) == [-1, -1] and np.isnan(rep.sum[5, 4])
    assert rep.min[3, 5] == np.inf and rep.argmin[3, 5] == groups.cells[gp[3]]


# ------------------------------------------------------------------ 5. independence
def test_reports_do_not_depend_on_numbering_labels_or_the_call(cases):
    from orc_amd.solver import group_integrals
    a, m, ids, G, groups = cases["hex"]
    f, _ = restated(cases, "hex", "volume")
    fields = named(f)
    first = group_integrals(m, groups, fields, "volume")
    assert same_report(group_integrals(m, groups, fields, "volume"), first)  # two calls, the same bits
    for ordering in (1, 2):
        _, mo = hex_case(24, 24, 20, ordering=ordering)
        assert not np.array_equal(mo.cell_order(), np.arange(a.n_cells))
        assert same_report(group_integrals(mo, mo.cell_groups(ids, G), fields, "volume"), first), ordering
    # relabelled groups give the permuted rows
    new_of_old = np.argsort(splitmix64_uniform(G, 5), kind="stable").astype(np.int32)
    ids2 = np.where(ids >= 0, new_of_old[np.maximum(ids, 0)], -1).astype(np.int32)
    rep2 = group_integrals(m, m.cell_groups(ids2, G), fields, "volume")
    assert same_bits(rep2.raw[new_of_old], first.raw) and same_bits(rep2.weight[new_of_old], first.weight)
    assert np.array_equal(rep2.where[new_of_old], first.where) and np.array_equal(rep2.count[new_of_old], first.count)


# ------------------------------------------------------------------ 6. the live solver
def live_solver(arms=False):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import ScalarSettings, Viscosity, ViscosityModel
    from orc_amd.solver import Solver
    a = set_channel_bcs(hex_channel(12, 10, 8))
    m = Mesh(a)
    s = Solver(m, settings(solver_type=BICGSTAB, iterations=20), RHO, MU)
    s.set_fields(*seeded_fields(a, scale=0.01))
    extra = {}
    if arms:
        extra["mu"] = MU * (1.5 + splitmix64_uniform(a.n_cells, 61))
        extra["phi"] = splitmix64_uniform(a.n_cells, 62)
        s.set_viscosity_field(extra["mu"])
        s.set_viscosity(Viscosity.make(ViscosityModel.FIELD))
        s.set_scalar(ScalarSettings.default())
        s.set_scalar_field(extra["phi"])
    return a, m, s, extra


def test_live_solver_report_equals_the_integrals_of_its_fields_and_reads_only(gpu):
    from orc_amd.solver import group_integrals
    a, m, s, _ = live_solver()
    groups = m.bin_cells((0, 1, 0), np.linspace(0.0, 0.001, 6))
    assert len(groups) == 5 and groups.count.sum() == a.n_cells
    s.set_monitors(True)
    s.iterate(3)
    before = (s.get_fields(), s.surface_report().raw.copy(), s.residual_history().copy())
    names = ("u", "v", "w", "p")
    for weighting in ("volume", "unit"):
        rep = s.group_report(groups, names, weighting)
        assert rep.names == list(names)
        assert same_report(rep, group_integrals(m, groups, dict(zip(names, before[0])), weighting))
    assert same_report(s.group_report(groups, ("p", "u")), group_integrals(m, groups, dict(u=before[0][0], p=before[0][3])))  # mask order
    # MU while the viscosity arm is off: the constant in every cell, through the same rounded products
    assert same_report(s.group_report(groups, ("w", "mu")), group_integrals(m, groups, dict(w=before[0][2], mu=np.full(a.n_cells, MU))))
    assert same_report(s.group_report(groups, "mu", "unit"), group_integrals(m, groups, dict(mu=np.full(a.n_cells, MU)), "unit"))
    for g, w in zip(s.get_fields(), before[0]):
        assert same_bits(g, w)
    assert same_bits(s.surface_report().raw, before[1]) and same_bits(s.residual_history(), before[2])
    # a steady run records on demand
    s.set_group_history(groups, ("u", "p"))
    assert s.group_history_count() == 0
    s.iterate(1)
    s.record_groups(3.0)
    times, values, weight = s.group_history()
    now = s.group_report(groups, ("u", "p"))
    assert times.tolist() == [3.0] and same_bits(values[0], now.raw) and same_bits(weight, now.weight)
    _, full = s.group_history(full=True)
    assert same_report(full[0], now)


def test_live_solver_phi_and_mu_with_their_arms_on(gpu):
    from orc_amd.solver import group_integrals
    a, m, s, extra = live_solver(arms=True)
    groups = m.box_cells((0.0005, 0.0002, 0.0), (0.0015, 0.0008, 0.001))
    assert len(groups) == 1 and 0 < groups.count[0] < a.n_cells
    s.iterate(2)
    u, v, w, p = s.get_fields()
    all_six = dict(u=u, v=v, w=w, p=p, phi=s.get_scalar_field(), mu=s.viscosity())  # six fields: two launches
    assert same_report(s.group_report(groups, ("u", "v", "w", "p", "phi", "mu")), group_integrals(m, groups, all_six))
    assert same_report(s.group_report(groups, ("phi", "mu"), "unit"), group_integrals(m, groups, dict(phi=all_six["phi"], mu=all_six["mu"]), "unit"))


# ------------------------------------------------------------------ 7. the running statistics
def test_group_statistics_equal_the_integrals_of_the_statistics(cases):
    from orc_amd.settings import StatGroup, TimeStatistics
    from orc_amd.solver import Solver, group_integrals
    a, m, ids, G, groups = cases["poly"]
    s = Solver(m, settings(solver_type=BICGSTAB), RHO, MU)
    s.set_time_statistics(TimeStatistics.make(groups=StatGroup.MEAN | StatGroup.STRESS))
    for k, wt in enumerate((1.0, 0.25, 3.0, 0.7)):
        s.set_fields(*seeded_fields(a, scale=0.05 * (k + 1)))
        s.sample_statistics(wt)
    names = s.statistics_fields()
    assert len(names) == 11 > 2 * cases["lim"]["fields"]  # three launches
    for form, normalised in (("normalised", True), ("raw", False)):
        host = s.statistics(names, normalised=normalised)
        rep = s.group_statistics(groups, None, form)
        assert rep.names == names
        assert same_report(rep, group_integrals(m, groups, {k: host[k] for k in names}))
        some = ("uv", "p", "ww")  # a sub-mask, in the order of the statistics' fields
        assert same_report(s.group_statistics(groups, some, form, "unit"), group_integrals(m, groups, {k: host[k] for k in ("p", "ww", "uv")}, "unit"))
    assert not same_bits(s.group_statistics(groups, "uu", "raw").raw, s.group_statistics(groups, "uu", "normalised").raw)


# ------------------------------------------------------------------ 8. the history
@pytest.mark.parametrize("interval", [1, 2])
def test_history_of_four_euler_steps(gpu, interval):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = m.n_cells
    y = np.asarray(a["cell_centroid"])[:, 1]
    groups = m.bin_cells((0, 1, 0), np.linspace(y.min(), y.max() * (1 + 1e-9), 5))
    probes = m.locate(np.asarray(a["cell_centroid"])[:: max(n // 40, 1)].copy())
    names = ("u", "v", "w", "p")

    def fresh():
        s = Solver(m, settings(solver_type=BICGSTAB, iterations=30), RHO, MU)
        z = np.zeros(n)
        s.set_fields(z, z, z, z)
        s.set_transient(transient(1e-3, 0, 2))
        s.set_probe_history(probes, names, "cell")
        return s

    # the second, identical run: no group history, stepped one at a time, a report after every step
    t = fresh()
    assert t.group_history_count() == -1
    reps_t, reports = [], []
    for _ in range(4):
        reps_t.append(t.advance(1, report=True)[0])
        reports.append(t.group_report(groups, names))
    reps_t = np.array(reps_t)

    s = fresh()
    s.set_group_history(groups, names, interval=interval)
    assert s.group_history_count() == 0
    reps_s = s.advance(4, report=True)
    due = [k for k in range(4) if (k + 1) % interval == 0]
    times, values, weight = s.group_history()
    assert len(times) == len(due) == s.group_history_count() and values.shape == (len(due), len(groups), 4, 4)
    assert same_bits(times, reps_s[due, 9])
    _, full = s.group_history(full=True)
    for row, step in enumerate(due):
        assert same_bits(values[row], reports[step].raw), step
        assert same_report(full[row], reports[step]), step
    assert same_bits(weight, reports[0].weight)
    # the run with the history on is the run with it off, in every bit: step reports, fields, probe history
    assert same_bits(reps_s, reps_t)
    for g, w in zip(s.get_fields(), t.get_fields()):
        assert same_bits(g, w)
    (ts, hs), (tt, ht) = s.probe_history(), t.probe_history()
    assert same_bits(ts, tt) and all(same_bits(hs[k], ht[k]) for k in names)
    assert same_report(s.group_report(groups, names), reports[-1])
    t1, v1, _ = s.group_history(first=len(due) - 1, count=1)
    assert same_bits(t1, times[-1:]) and same_bits(v1, values[-1:])
    # turning it off drops it
    s.set_group_history(None)
    assert s.group_history_count() == -1
    s.advance(1)
    assert s.group_history_count() == -1


# ------------------------------------------------------------------ 9. arguments
def test_refused_arguments_leave_everything_alone(gpu):
    from orc_amd import parallel
    from orc_amd._lib import OrcError, lib
    from orc_amd.mesh import Mesh
    from orc_amd.settings import StatGroup, TimeStatistics
    from orc_amd.solver import group_integrals
    L = lib()
    a, m, s, _ = live_solver()
    n = a.n_cells
    other = Mesh(a)
    ids = scattered_ids(n, 3)
    i32 = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    st = C.c_int(0)
    assert L.orc_cell_groups_create(None, 3, i32(ids), C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_cell_groups_create(m.ptr, 3, None, C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_cell_groups_create(m.ptr, 0, i32(ids), C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_cell_groups_create(m.ptr, limits()["max_groups"] + 1, i32(ids), C.byref(st)) is None and st.value == BAD_ARGUMENT
    for bad in (-2, 3):
        wrong = ids.copy()
        wrong[7] = bad
        assert L.orc_cell_groups_create(m.ptr, 3, i32(wrong), C.byref(st)) is None and st.value == BAD_ARGUMENT
    ap, halo, _ = parallel.partition_arrays(a, 2, 0)
    pm = parallel.PartitionedMesh(ap, halo)
    with pytest.raises(OrcError) as e:
        pm.cell_groups(np.zeros(pm.n_cells, np.int32))
    assert e.value.status == BAD_ARGUMENT and "partitioned" in str(e.value)
    groups, foreign = m.cell_groups(ids, 3), other.cell_groups(ids, 3)
    assert L.orc_cell_groups_get(groups.ptr, None, None, None) == 0  # every output may be NULL
    f = s.get_fields()
    surface = s.surface_report().raw.copy()
    good = s.group_report(groups, "u")
    assert L.orc_solver_group_report(s.ptr, groups.ptr, 1, 0, None, None, None) == 0  # every output may be NULL
    block = np.ascontiguousarray(np.array(f[:1]))
    f64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    refused = [
        lambda: L.orc_solver_group_report(None, groups.ptr, 1, 0, None, None, None),
        lambda: s.group_report(None, "u", raise_on_error=False)[0],
        lambda: s.group_report(foreign, "u", raise_on_error=False)[0],
        lambda: s.group_report(groups, 0, raise_on_error=False)[0],
        lambda: s.group_report(groups, 1 << 6, raise_on_error=False)[0],
        lambda: s.group_report(groups, "phi", raise_on_error=False)[0],  # no scalar arm
        lambda: s.group_report(groups, "u", 2, raise_on_error=False)[0],  # unknown weighting
        lambda: group_integrals(m, foreign, dict(u=f[0]), raise_on_error=False)[0],
        lambda: group_integrals(m, None, dict(u=f[0]), raise_on_error=False)[0],
        lambda: group_integrals(m, groups, dict(u=f[0]), 5, raise_on_error=False)[0],
        lambda: L.orc_group_integrals(m.ptr, groups.ptr, 1, None, 0, None, None, None),
        lambda: L.orc_group_integrals(None, groups.ptr, 1, f64(block), 0, None, None, None),
        lambda: L.orc_group_integrals(m.ptr, groups.ptr, 0, f64(block), 0, None, None, None),
        lambda: s.group_statistics(groups, "u", raise_on_error=False)[0],  # the statistics arm is off
        lambda: L.orc_solver_set_group_history(None, groups.ptr, 1, 0, 1),
        lambda: s.set_group_history(groups, "u", interval=0, raise_on_error=False),
        lambda: s.set_group_history(groups, 0, raise_on_error=False),
        lambda: s.set_group_history(groups, "phi", raise_on_error=False),
        lambda: s.set_group_history(groups, "u", weighting=9, raise_on_error=False),
        lambda: s.set_group_history(foreign, "u", raise_on_error=False),
        lambda: s.record_groups(1.0, raise_on_error=False),  # the history is off
        lambda: L.orc_solver_group_history(s.ptr, 0, 0, None, None, None, None),
    ]
    for k, call in enumerate(refused):
        assert call() == BAD_ARGUMENT, k
    assert s.group_history_count() == -1
    # the statistics arm on: a field whose group is off, NORMALISED without a sample, an unknown form
    s.set_time_statistics(TimeStatistics.make(groups=StatGroup.MEAN))
    for call in (lambda: s.group_statistics(groups, "uu", raise_on_error=False)[0],
                 lambda: s.group_statistics(groups, "u", "normalised", raise_on_error=False)[0],
                 lambda: s.group_statistics(groups, "u", 7, raise_on_error=False)[0],
                 lambda: s.group_statistics(foreign, "u", "raw", raise_on_error=False)[0],
                 lambda: s.group_statistics(groups, "u", "raw", 3, raise_on_error=False)[0]):
        assert call() == BAD_ARGUMENT
    assert s.group_statistics(groups, "u", "raw", raise_on_error=False)[0] == 0
    # a history that is on stays as it was when a second set call is refused, and a range past it is refused
    s.set_group_history(groups, ("u", "p"), interval=3)
    s.record_groups(1.5)
    assert s.set_group_history(foreign, "u", raise_on_error=False) == BAD_ARGUMENT
    assert s.set_group_history(groups, "u", interval=0, raise_on_error=False) == BAD_ARGUMENT
    assert s.group_history_count() == 1 and s.group_history()[1].shape == (1, 3, 2, 4)
    assert L.orc_solver_group_history(s.ptr, 1, 1, None, None, None, None) == BAD_ARGUMENT
    assert L.orc_solver_group_history(s.ptr, 0, 1, None, None, None, None) == 0
    # nothing moved
    for g, w in zip(s.get_fields(), f):
        assert same_bits(g, w)
    assert same_bits(s.surface_report().raw, surface) and same_report(s.group_report(groups, "u"), good)
