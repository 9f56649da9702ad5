"""Point probes on the device (orc_amd/csrc/probes.hip): the locate against the numpy restatement of tests/probe_restatement.py in
every output, culled and un-culled and with forced slab counts; the edges of a wave, a cell tile and a slab; the tie rule; points
outside; both samplers bit for bit; the history of a BDF2 run; arguments.

Bit for bit means equal uint64 views."""
import ctypes as C

import numpy as np
import pytest

import probe_restatement as PR
from conftest import splitmix64_uniform
from test_gpu_surface import mixed_case, seeded_fields
from test_gpu_transient import channel_flow, settings, transient
from test_gpu_wall import hex_mesh
from test_probes_cpu import bounding_box, seeded_points

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
BICGSTAB = 3
RHO, MU = 1000.0, 1e-3
GREEN_GAUSS, LEAST_SQUARES = 0, 2
VARIANTS = [dict(), dict(cull=False), dict(slabs=1), dict(slabs=2), dict(slabs=7), dict(cull=False, slabs=7)]
OUTPUTS = ("cell", "status", "steps", "zone")


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def assert_located(p, want, what=""):
    for k in OUTPUTS:
        assert np.array_equal(getattr(p, k), want[k]), (what, k, int(np.count_nonzero(getattr(p, k) != want[k])))
    assert same_bits(p.excess, want["excess"]), (what, "excess")
    assert np.array_equal(p.inside, want["status"] == PR.INSIDE) and len(p) == len(want["cell"])


def mesh_of(name, tmp_path, ordering=None):
    if name.startswith("hex"):
        return hex_mesh(*{"hex_small": (5, 4, 3), "hex_large": (32, 16, 12)}[name], ordering=ordering)
    return mixed_case(tmp_path, name == "poly")


# ------------------------------------------------------------------ 1. locate equals the restatement
@pytest.mark.parametrize("name", ["hex_small", "hex_large", "mixed", "poly"])
def test_locate_equals_the_restatement_culled_unculled_and_in_slabs(gpu, tmp_path, name):
    a, m = mesh_of(name, tmp_path)
    x = seeded_points(a)
    want = PR.locate(a, x)
    if name in ("mixed", "poly"):
        assert np.mean(want["steps"] > 0) >= 0.10  # a nearest-centroid answer alone fails here
    for kw in VARIANTS:
        assert_located(m.locate(x, **kw), want, kw)
    st = m.probe_search_stats()
    assert st["tiles"] == (m.n_cells + st["tile"] - 1) // st["tile"] and st["slabs"] == 7


def test_reordered_meshes_give_the_same_cells_in_orc_numbering(gpu):
    from orc_amd.mesh import Mesh
    a, m = hex_mesh(32, 16, 12)
    x = seeded_points(a, 1000, seed=7)
    want = PR.locate(a, x)
    assert_located(m.locate(x), want)
    for ordering in (1, 2):  # RCM, GEOMETRIC
        mo = Mesh(a, ordering=ordering)
        assert not np.array_equal(mo.cell_order(), np.arange(m.n_cells))
        for kw in (dict(), dict(cull=False, slabs=3)):
            assert_located(mo.locate(x, **kw), want, (ordering, kw))


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_point_counts_at_the_wave_and_block_edges(gpu, n):
    a, m = hex_mesh(5, 4, 3)
    x = seeded_points(a, n, seed=31)
    want = PR.locate(a, x)
    for kw in (dict(), dict(cull=False, slabs=2)):
        assert_located(m.locate(x, **kw), want, kw)


@pytest.mark.parametrize("k", ["1", "T-1", "T", "T+1", "2T+1"])
def test_cell_counts_at_the_tile_edges_and_more_slabs_than_tiles(gpu, k):
    from orc_amd.mesh import probe_search_stats
    T = probe_search_stats()["tile"]
    n_cells = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[k]
    a, m = hex_mesh(n_cells, 1, 1)
    assert m.n_cells == n_cells
    x = seeded_points(a, 130, seed=41)
    want = PR.locate(a, x)
    assert np.all(want["status"] == PR.INSIDE)
    for kw in (dict(), dict(cull=False), dict(slabs=2), dict(slabs=5), dict(cull=False, slabs=5)):  # 5 slabs, at most 3 tiles
        assert_located(m.locate(x, **kw), want, kw)
    assert m.probe_search_stats()["tiles"] == (n_cells + T - 1) // T


# ------------------------------------------------------------------ 3. the tie rule
def test_ties_go_to_the_smallest_orc_id_whatever_the_numbering_and_the_point_order(gpu):
    from orc_amd.mesh import Mesh
    a, m = hex_mesh(4, 4, 4, lx=4.0, ly=4.0, lz=4.0)  # spacing 1: centroids at k + 1/2, face centres exact
    cc = np.asarray(a["cell_centroid"])
    assert np.array_equal(np.sort(np.unique(cc)), [0.5, 1.5, 2.5, 3.5])
    g = np.arange(1.0, 4.0)
    faces = np.array([[i, 0.5 + j, 0.5 + k] for i in g for j in range(4) for k in range(4)])          # between 2 cells
    edges = np.array([[i, j, 0.5 + k] for i in g for j in g for k in range(4)])                        # between 4
    verts = np.array([[i, j, k] for i in g for j in g for k in g])                                     # between 8
    x = np.concatenate([faces, faces[:, [1, 0, 2]], faces[:, [2, 1, 0]], edges, edges[:, [2, 0, 1]], verts])
    s = ((x[:, None, :] - cc[None, :, :]) ** 2).sum(axis=2)
    tied = s == s.min(axis=1)[:, None]
    assert sorted(set(tied.sum(axis=1))) == [2, 4, 8]
    smallest = np.argmax(tied, axis=1)
    want = PR.locate(a, x)
    assert np.array_equal(want["cell"], smallest) and np.all(want["steps"] == 0) and np.all(want["status"] == PR.INSIDE)
    assert np.all(want["excess"] == 0.0)
    perm = np.argsort(splitmix64_uniform(len(x), 9), kind="stable")
    for mesh in (m, Mesh(a, ordering=1)):
        for kw in VARIANTS:
            assert_located(mesh.locate(x, **kw), want, kw)
        p = mesh.locate(x[perm])
        assert np.array_equal(p.cell, smallest[perm]) and np.all(p.status == PR.INSIDE) and np.all(p.steps == 0)


# ------------------------------------------------------------------ 4. outside, and the order of the points
def test_points_beyond_each_side_are_outside_through_the_right_zone(gpu):
    a, m = hex_mesh(5, 4, 3)
    lo, hi = bounding_box(a)
    mid, span = 0.5 * (lo + hi), hi - lo
    sides = {"INLET": (0, -1), "OUTLET": (0, 1), "BOTTOM_WALL": (1, -1), "TOP_WALL": (1, 1), "PERIODIC_-Z": (2, -1), "PERIODIC_+Z": (2, 1)}
    x = np.tile(mid, (6, 1))
    for i, (axis, sign) in enumerate(sides.values()):
        x[i, axis] = (hi if sign > 0 else lo)[axis] + sign * 0.37 * span[axis]
    want = PR.locate(a, x)
    assert np.all(want["status"] == PR.OUTSIDE) and np.all(want["excess"] > 0)
    assert list(want["zone"]) == [a.get_face_zone(z) for z in sides]
    p = m.locate(x)
    assert_located(p, want)
    assert not p.inside.any()
    far = np.concatenate([x, mid[None, :] + 40.0 * span[None, :] * np.array([[1.0, 0.3, -0.2]])])  # far off: outside after a few moves
    assert_located(m.locate(far), PR.locate(a, far))


def test_the_order_of_the_points_does_not_matter(gpu, tmp_path):
    a, m = mixed_case(tmp_path, True)
    x = seeded_points(a)
    perm = np.argsort(splitmix64_uniform(len(x), 55), kind="stable")
    p, q = m.locate(x), m.locate(x[perm])
    for k in OUTPUTS:
        assert np.array_equal(getattr(q, k), getattr(p, k)[perm]), k
    assert same_bits(q.excess, p.excess[perm])


# ------------------------------------------------------------------ 5. sampling
def solver_of(a, m, recon, arms=False):
    from orc_amd.settings import ScalarSettings, Viscosity, ViscosityModel
    from orc_amd.solver import Solver
    st = settings(gradient_reconstruction=recon, solver_type=BICGSTAB)
    s = Solver(m, st, RHO, MU)
    f = seeded_fields(a)
    s.set_fields(*f)
    extra = {}
    if arms:
        extra["mu"] = MU * (1.5 + splitmix64_uniform(a.n_cells, 61))
        extra["phi"] = splitmix64_uniform(a.n_cells, 62)
        s.set_viscosity_field(extra["mu"])
        s.set_viscosity(Viscosity.make(ViscosityModel.FIELD))
        s.set_scalar(ScalarSettings.default())
        s.set_scalar_field(extra["phi"])
    return s, st, f, extra


@pytest.mark.parametrize("recon", [GREEN_GAUSS, LEAST_SQUARES], ids=["green_gauss", "least_squares"])
@pytest.mark.parametrize("name", ["hex_large", "poly"])
def test_both_samplers_equal_the_restatement_bit_for_bit(gpu, tmp_path, name, recon):
    from orc_amd.solver import calculate_gradients
    a, m = mesh_of(name, tmp_path)
    s, st, f, extra = solver_of(a, m, recon, arms=True)
    x = seeded_points(a, 1500, seed=13)
    loc = PR.locate(a, x)
    p = m.locate(x)
    assert_located(p, loc)
    gp, gu = calculate_gradients(m, *f, st)
    before = s.get_fields()
    names = ("u", "v", "w", "p", "phi", "mu")
    cell = s.sample(p, names, "cell")
    lin = s.sample(p, names, "linear")
    assert list(cell) == list(lin) == list(names)
    grads = {"u": gu[:, 0, :], "v": gu[:, 1, :], "w": gu[:, 2, :], "p": gp}
    for k, phi in zip("uvwp", f):
        assert same_bits(cell[k], PR.sample_cell(phi, loc)), k
        assert same_bits(lin[k], PR.sample_linear(phi, grads[k], loc)), k
        assert not same_bits(lin[k], cell[k])
    for k in ("phi", "mu"):  # cell values in either mode
        assert same_bits(cell[k], extra[k][loc["cell"]]) and same_bits(lin[k], cell[k]), k
    one = s.sample(p, ("p", "u"), "linear")  # a selection, in the order asked for
    assert list(one) == ["p", "u"] and same_bits(one["p"], lin["p"]) and same_bits(one["u"], lin["u"])
    for b, c in zip(before, s.get_fields()):
        assert same_bits(b, c)
    # the viscosity arm off: MU is the constant
    s2, _, _, _ = solver_of(a, m, recon)
    assert same_bits(s2.sample(p, "mu")["mu"], np.full(len(x), MU))


def test_a_field_linear_in_x_is_reproduced_in_interior_cells(gpu):
    """u_P = a + b x_P on the hex channel, Green-Gauss, LINEAR at points in cells without a boundary face: a + b x up to rounding.
    With M = |a| + |b| max|x| >= every value involved and e = 2^-53: the inputs u_P carry 2 roundings each (b x, + a), which reach the
    result through u_P itself (2 e M) and through G.r (|r_d| <= h_d / 2, G_d from two cells over 2 h_d: e M per direction) — 5 e M.
    The gradient: per direction two non-zero face terms f (A / V) n_d of size <= M / h_d with 5 roundings each (the face mean 2, A / V,
    n (A / V), the product) and one rounding add, the terms of the four other faces are exact zeros: 11 e M / h_d, times |r_d| <= h_d / 2,
    three directions — 16.5 e M.  r = x - x_P: e M.  The three products G_d r_d and their two adds: 5 e M; the last add: e M; the two
    roundings of the expected a + b x itself: 2 e M.  30.5 e M in all; the test asks for 32 e M = 16 * 2^-52 M."""
    a, m = hex_mesh(8, 6, 5)
    cc = np.asarray(a["cell_centroid"])
    a0, b0 = 1.0, 100.0
    z = np.zeros(a.n_cells)
    from orc_amd.solver import Solver
    s = Solver(m, settings(gradient_reconstruction=GREEN_GAUSS, solver_type=BICGSTAB), RHO, MU)
    s.set_fields(a0 + b0 * cc[:, 0], z, z, z)
    x = seeded_points(a, 2000, seed=17)
    p = m.locate(x)
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    boundary_cell = np.zeros(a.n_cells, bool)
    boundary_cell[c0[c1 < 0]] = True
    keep = p.inside & ~boundary_cell[p.cell]
    assert keep.sum() > 200
    got = s.sample(p, "u", "linear")["u"]
    M = abs(a0) + abs(b0) * np.abs(x[:, 0]).max()
    err = np.abs(got - (a0 + b0 * x[:, 0]))[keep].max()
    print("linear field: worst error %.2f x 2^-52 M" % (err / (2.0 ** -52 * M)))
    assert err <= 16 * 2.0 ** -52 * M
    assert np.abs(s.sample(p, "u", "cell")["u"] - (a0 + b0 * x[:, 0]))[keep].max() > 1e-6 * M  # the cell value alone is far off


# ------------------------------------------------------------------ 6. the history
@pytest.mark.parametrize("interval", [1, 2])
def test_history_of_five_bdf2_steps(gpu, interval):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = m.n_cells
    x = seeded_points(a, 100, seed=23)
    p = m.locate(x)
    names = ("u", "v", "w", "p")

    def fresh():
        s = Solver(m, settings(solver_type=BICGSTAB, iterations=30), RHO, MU)
        z = np.zeros(n)
        s.set_fields(z, z, z, z)
        s.set_transient(transient(1e-3, 1, 2))
        return s

    plain = fresh()
    rep0 = plain.advance(5, report=True)
    f0 = plain.get_fields()

    s = fresh()
    assert s.probe_history_count() == -1
    s.set_probe_history(p, names, "linear", interval=interval)
    assert s.probe_history_count() == 0
    reps, samples = [], []
    for step in range(5):
        reps.append(s.advance(1, report=True)[0])
        samples.append(s.sample(p, names, "linear"))
        if step == 2:  # snapshot and restore leave the history alone
            s.snapshot()
            s.restore()
            assert s.probe_history_count() == (step + 1) // interval
    reps = np.array(reps)
    due = [k for k in range(5) if (k + 1) % interval == 0]
    times, hist = s.probe_history()
    assert len(times) == len(due) == s.probe_history_count()
    assert same_bits(times, reps[due, 9])
    for k in names:
        assert hist[k].shape == (len(due), len(x))
        for row, step in enumerate(due):
            assert same_bits(hist[k][row], samples[step][k]), (k, step)
    # the run is the run without probes, in every bit
    assert same_bits(reps, rep0)
    for g, w in zip(s.get_fields(), f0):
        assert same_bits(g, w)
    # record_probes appends the current state under its tag
    s.record_probes(-7.5)
    times, hist = s.probe_history()
    assert len(times) == len(due) + 1 and times[-1] == -7.5
    for k in names:
        assert same_bits(hist[k][-1], samples[-1][k])
    t1, h1 = s.probe_history(first=1, count=1)
    assert same_bits(t1, times[1:2]) and same_bits(h1["p"], hist["p"][1:2])
    # several steps in one call, then off
    s.advance(2 * interval)
    assert s.probe_history_count() == len(due) + 3
    s.set_probe_history(None)
    assert s.probe_history_count() == -1


# ------------------------------------------------------------------ 7. arguments
def test_refused_arguments_leave_mesh_and_solver_alone(gpu):
    from orc_amd._lib import OrcError, lib
    from orc_amd.mesh import Mesh
    from orc_amd.solver import Solver
    L = lib()
    a, m = hex_mesh(5, 4, 3)
    other = Mesh(a)
    x = seeded_points(a, 10)
    st = C.c_int(0)
    f64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.orc_probes_create(None, 10, f64(x), C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_probes_create(m.ptr, 10, None, C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_probes_create(m.ptr, 0, f64(x), C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_debug_probes_locate(m.ptr, 10, f64(x), 1, -1, C.byref(st)) is None and st.value == BAD_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[3, 1] = bad
        with pytest.raises(OrcError) as e:
            m.locate(y)
        assert e.value.status == BAD_ARGUMENT
    assert L.orc_probes_get(None, None, None, None, None, None) == BAD_ARGUMENT
    # a partitioned mesh is refused, and the message says why
    from orc_amd import parallel
    ap, halo, _ = parallel.partition_arrays(a, 2, 0)
    with pytest.raises(OrcError) as e:
        parallel.PartitionedMesh(ap, halo).locate(x)
    assert e.value.status == BAD_ARGUMENT and "partitioned" in str(e.value)
    p = m.locate(x)
    assert L.orc_probes_get(p.ptr, None, None, None, None, None) == 0  # every output may be NULL
    s = Solver(m, settings(solver_type=BICGSTAB), RHO, MU)
    f = seeded_fields(a)
    s.set_fields(*f)
    out = np.zeros((6, 10))
    refused = [
        lambda: L.orc_solver_sample_probes(None, p.ptr, 1, 0, f64(out)),
        lambda: L.orc_solver_sample_probes(s.ptr, None, 1, 0, f64(out)),
        lambda: L.orc_solver_sample_probes(s.ptr, p.ptr, 1, 0, None),
        lambda: s.sample(p, 0, "cell", raise_on_error=False)[0],
        lambda: s.sample(p, 1 << 6, "cell", raise_on_error=False)[0],
        lambda: s.sample(p, "phi", "cell", raise_on_error=False)[0],  # no scalar arm
        lambda: s.sample(p, "u", 2, raise_on_error=False)[0],
        lambda: s.sample(other.locate(x), "u", "cell", raise_on_error=False)[0],
        lambda: L.orc_solver_set_probe_history(None, p.ptr, 1, 0, 1),
        lambda: s.set_probe_history(p, "u", "cell", interval=0, raise_on_error=False),
        lambda: s.set_probe_history(p, 0, "cell", raise_on_error=False),
        lambda: s.set_probe_history(p, "phi", "cell", raise_on_error=False),
        lambda: s.set_probe_history(p, "u", 7, raise_on_error=False),
        lambda: s.set_probe_history(other.locate(x), "u", "cell", raise_on_error=False),
        lambda: s.record_probes(1.0, raise_on_error=False),  # the history is off
        lambda: L.orc_solver_probe_history(s.ptr, 0, 0, None, None),
        lambda: L.orc_solver_record_probes(None, 0.0),
    ]
    for i, call in enumerate(refused):
        assert call() == BAD_ARGUMENT, i
        assert s.probe_history_count() == -1
        for g, w in zip(s.get_fields(), f):
            assert same_bits(g, w)
    assert s.sample(p, "mu", "cell")["mu"][0] == MU  # MU is selectable always
    s.set_probe_history(p, ("u", "p"), "cell")
    s.record_probes(2.0)
    times = np.zeros(4)
    assert L.orc_solver_probe_history(s.ptr, 0, 2, f64(times), None) == BAD_ARGUMENT  # a range past the history
    assert L.orc_solver_probe_history(s.ptr, 2, 0, f64(times), None) == BAD_ARGUMENT
    assert L.orc_solver_probe_history(s.ptr, 1, 0, f64(times), None) == 0
    assert s.probe_history_count() == 1
    s.set_probe_history(None)
