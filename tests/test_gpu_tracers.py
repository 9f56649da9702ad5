"""Tracer particles on the device (orc_amd/csrc/tracers.hip) against the numpy restatement of tests/tracer_restatement.py, bit for bit in
every output: both schemes, both interpolations, both gradient arms, both directions, both step modes, with and without a path; the edges
of a wave and of the substep count; the invariances; the order of accuracy on a solid-body rotation; the sampler; tracking inside advance.

Bit for bit means equal uint64 views of the doubles and equal integers."""
import ctypes as C

import numpy as np
import pytest

import probe_restatement as PR
import tracer_restatement as TR
from conftest import splitmix64_uniform
from test_gpu_probes import same_bits
from test_gpu_surface import mixed_case
from test_gpu_transient import channel_flow, settings, transient
from test_gpu_wall import hex_mesh
from test_probes_cpu import bounding_box, seeded_points
from test_tracers_cpu import SUBSTEPS, U0, length_step, tracer_fields, tracer_seeds

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
BICGSTAB = 3
RHO, MU = 1000.0, 1e-3
GREEN_GAUSS, LEAST_SQUARES = 0, 2
RECON = {"green_gauss": GREEN_GAUSS, "least_squares": LEAST_SQUARES}


def gpu_mesh(name, tmp_path, ordering=None):
    """the meshes of tests/test_tracers_cpu.py::host_mesh on the device"""
    return hex_mesh(12, 8, 6, ordering=ordering) if name == "hex" else mixed_case(tmp_path, name == "poly")


def solver_with(a, m, recon, fields=None):
    """-> (solver, (u, v, w), the velocity gradients [n, 3, 3] of orc_calculate_gradients for this arm)"""
    from orc_amd.solver import Solver, calculate_gradients
    st = settings(gradient_reconstruction=recon, solver_type=BICGSTAB)
    s = Solver(m, st, RHO, MU)
    f = tracer_fields(a) if fields is None else fields
    p = np.zeros(a.n_cells)
    s.set_fields(*f, p)
    _, gu = calculate_gradients(m, *f, p, st)
    return s, f, gu


def make(step=0.0, **kw):
    from orc_amd.settings import TracerSettings
    return TracerSettings.make(step, **kw)


def assert_set(t, want, what=""):
    got = t.get()
    assert same_bits(got["positions"], want["x"]), (what, "positions", int(np.count_nonzero(got["positions"] != want["x"])))
    for k in ("cell", "status", "zone", "steps"):
        assert np.array_equal(got[k], want[k]), (what, k, int(np.count_nonzero(got[k] != want[k])))
    assert same_bits(got["age"], want["age"]), (what, "age")
    assert np.array_equal(t.active, want["status"] == TR.ACTIVE) and len(t) == len(want["cell"])


def run_both(a, m, T, s, f, gu, seeds, n_sub, stride, what, **kw):
    """the same advection on the device and in the restatement, compared in every output -> (tracers, restatement state, its report)"""
    c = make(kw.pop("step"), **kw)
    t = m.seed(seeds)
    want = TR.seed(T, seeds)
    assert_set(t, want, (what, "seeded"))
    out = TR.advect(T, want, f, gu, c.scheme, c.interpolation, c.step_mode, c.direction, c.step, c.min_speed, n_sub, record_stride=stride)
    res = s.advect(t, c, n_sub, record_stride=stride)
    assert_set(t, want, what)
    if stride:
        path, plen = res
        assert same_bits(path, out["path"]), (what, "path")
        assert np.array_equal(plen, out["path_len"]), (what, "path_len")
    else:
        assert res is None
    return t, want, out


# ------------------------------------------------------------------ 1. equals the restatement
@pytest.mark.parametrize("recon", list(RECON), ids=list(RECON))
@pytest.mark.parametrize("name", ["hex", "mixed", "poly"])
def test_advection_equals_the_restatement(gpu, tmp_path, name, recon):
    a, m = gpu_mesh(name, tmp_path)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, RECON[recon])
    seeds, step, n_sub = tracer_seeds(a), length_step(a), SUBSTEPS[name]
    for scheme in (TR.EULER, TR.RK2):
        for interpolation in (TR.CELL, TR.LINEAR):
            if interpolation == TR.CELL and recon == "least_squares":
                continue  # the cell value does not depend on the gradient arm
            for direction in (1, -1):
                what = (name, recon, scheme, interpolation, direction)
                t, want, out = run_both(a, m, T, s, f, gu, seeds, n_sub, 1, what, step=step, scheme=scheme, interpolation=interpolation,
                                        step_mode=TR.LENGTH, direction=direction)
                if direction == 1:  # the comparison is not empty, with this arm's gradients too (tests/test_tracers_cpu.py)
                    active, left = want["status"] == TR.ACTIVE, want["status"] == TR.LEFT
                    assert active.mean() >= 0.25 and left.mean() >= 0.25 and out["longest"] >= 3, what
                    assert not np.any(want["status"] >= TR.WALK_LIMIT), what
    # paths at a stride, and none: 32 substeps
    kw = dict(step=step, scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.LENGTH, direction=1)
    for stride in (4, 0, 32):
        run_both(a, m, T, s, f, gu, seeds, 32, stride, (name, recon, "stride", stride), **kw)
    # TIME mode once per mesh
    run_both(a, m, T, s, f, gu, seeds, n_sub, 1, (name, recon, "time"), step=step / U0, scheme=TR.RK2, interpolation=TR.LINEAR,
             step_mode=TR.TIME, direction=1)


# ------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_particle_counts_at_the_wave_and_block_edges(gpu, n):
    a, m = hex_mesh(5, 4, 3)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    t, want, out = run_both(a, m, T, s, f, gu, tracer_seeds(a, n, seed=31), 6, 1, n, step=length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR,
                            step_mode=TR.LENGTH, direction=1)
    assert want["steps"].max() > 0


@pytest.mark.parametrize("n_sub", [0, 1])
def test_zero_and_one_substep(gpu, n_sub):
    a, m = hex_mesh(5, 4, 3)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, LEAST_SQUARES)
    seeds = tracer_seeds(a, 100, seed=5)
    kw = dict(step=length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.LENGTH, direction=1)
    for stride in (0, 1):
        t, want, out = run_both(a, m, T, s, f, gu, seeds, n_sub, stride, (n_sub, stride), **kw)
        assert np.all(want["steps"] <= n_sub)
        if n_sub == 0:
            assert same_bits(t.positions, seeds) and np.all(t.age == 0.0)
    path, plen = s.advect(m.seed(seeds), make(**kw), 0, record_stride=7)  # 0 is a multiple of every stride
    assert path.shape == (1, 100, 3) and same_bits(path[0], seeds) and np.all(plen == 1)


def test_every_moving_particle_leaves_a_one_cell_mesh(gpu):
    a, m = hex_mesh(1, 1, 1)
    assert m.n_cells == 1
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, GREEN_GAUSS, fields=(np.array([U0]), np.array([0.3 * U0]), np.array([-0.05 * U0])))
    seeds = tracer_seeds(a, 70, seed=3)
    for scheme in (TR.EULER, TR.RK2):
        for interpolation in (TR.CELL, TR.LINEAR):
            for direction in (1, -1):
                t, want, out = run_both(a, m, T, s, f, gu, seeds, 32, 4, (scheme, interpolation, direction), step=length_step(a), scheme=scheme,
                                        interpolation=interpolation, step_mode=TR.LENGTH, direction=direction)
                assert np.all(want["status"] == TR.LEFT) and len(set(want["zone"].tolist())) >= 2


def test_seeds_outside_are_left_from_creation_and_never_move(gpu):
    a, m = hex_mesh(5, 4, 3)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    lo, hi = bounding_box(a)
    inside = tracer_seeds(a, 40, seed=9)
    outside = inside.copy()
    outside[:, 1] = hi[1] + 0.2 * (hi - lo)[1] * (1.0 + np.arange(40) / 40.0)  # above the top wall
    outside[::2, 0] = lo[0] - 0.3 * (hi - lo)[0]                                # or before the inlet, further away than above
    seeds = np.concatenate([inside, outside])[np.argsort(splitmix64_uniform(80, 4), kind="stable")]
    t, want, out = run_both(a, m, T, s, f, gu, seeds, 3, 1, "outside", step=length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR,
                            step_mode=TR.LENGTH, direction=1)
    born_left = PR.locate(a, seeds)["status"] == PR.OUTSIDE
    assert born_left.sum() == 40
    got = t.get()
    assert np.all(got["status"][born_left] == TR.LEFT) and np.all(got["zone"][born_left] >= 0)
    assert same_bits(got["positions"][born_left], seeds[born_left]) and np.all(got["steps"][born_left] == 0) and np.all(got["age"][born_left] == 0.0)
    assert np.all(out["path_len"][born_left] == 1) and got["steps"][~born_left].max() == 3


def test_min_speed_above_every_speed_and_a_cell_at_rest(gpu):
    a, m = hex_mesh(5, 4, 3)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    seeds = tracer_seeds(a, 90, seed=17)
    kw = dict(step=length_step(a), scheme=TR.RK2, step_mode=TR.LENGTH, direction=1)
    for interpolation in (TR.CELL, TR.LINEAR):
        t, want, out = run_both(a, m, T, s, f, gu, seeds, 5, 1, ("min_speed", interpolation), interpolation=interpolation, min_speed=10.0, **kw)
        assert np.all(want["status"] == TR.STAGNANT) and same_bits(t.positions, seeds) and np.all(t.steps == 0)
        assert np.all(out["path_len"] == 1)
    # a third of the cells at rest, min_speed 0: a particle there (from the start, or on arrival) is STAGNANT, and nothing is NaN
    rest = np.arange(a.n_cells) % 3 == 0
    f0 = tuple(np.where(rest, 0.0, x) for x in f)
    s0, f0, gu0 = solver_with(a, m, GREEN_GAUSS, fields=f0)
    for scheme in (TR.EULER, TR.RK2):
        t, want, out = run_both(a, m, T, s0, f0, gu0, seeds, 8, 1, ("rest", scheme), interpolation=TR.CELL, **dict(kw, scheme=scheme))
        got = t.get()
        assert np.any(got["status"] == TR.STAGNANT) and np.all(rest[got["cell"][got["status"] == TR.STAGNANT]])
        assert np.all(np.isfinite(got["positions"])) and np.all(np.isfinite(got["age"]))
        assert np.all(np.isfinite(s0.advect(m.seed(seeds), make(interpolation=TR.CELL, **dict(kw, scheme=scheme)), 8, record_stride=2)[0]))


# ------------------------------------------------------------------ 3. invariances
def test_split_permutation_and_repetition(gpu, tmp_path):
    a, m = gpu_mesh("poly", tmp_path)
    s, f, gu = solver_with(a, m, LEAST_SQUARES)
    seeds = tracer_seeds(a)
    c = make(length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.LENGTH, direction=1)

    def run(x, parts):
        t = m.seed(x)
        for k in parts:
            s.advect(t, c, k)
        return t.get()

    one, two, again = run(seeds, [32]), run(seeds, [10, 22]), run(seeds, [32])
    perm = np.argsort(splitmix64_uniform(len(seeds), 55), kind="stable")
    shuffled = run(seeds[perm], [32])
    assert not same_bits(run(seeds, [10])["positions"], one["positions"])
    for k in one:
        eq = same_bits if one[k].dtype == np.float64 else np.array_equal
        assert eq(two[k], one[k]), ("split", k)
        assert eq(again[k], one[k]), ("again", k)
        assert eq(shuffled[k], one[k][perm]), ("permutation", k)


def test_reordered_meshes_give_the_same_particles_in_orc_numbering(gpu):
    from orc_amd.mesh import Mesh
    a, m = hex_mesh(32, 16, 12)
    T = TR.Tables(a)
    seeds = seeded_points(a, 1000, seed=7)
    kw = dict(step=length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.LENGTH, direction=1)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    t, want, out = run_both(a, m, T, s, f, gu, seeds, 14, 0, "orc order", **kw)
    assert (want["status"] == TR.ACTIVE).mean() > 0.25 and out["changes"].max() >= 4
    for ordering in (1, 2):  # RCM, GEOMETRIC
        mo = Mesh(a, ordering=ordering)
        assert not np.array_equal(mo.cell_order(), np.arange(m.n_cells))
        so, _, _ = solver_with(a, mo, GREEN_GAUSS)
        to = mo.seed(seeds)
        so.advect(to, make(**kw), 14)
        assert_set(to, want, ordering)


# ------------------------------------------------------------------ 4. order of accuracy
@pytest.mark.parametrize("recon", list(RECON), ids=list(RECON))
def test_solid_body_rotation_follows_the_closed_forms(gpu, recon):
    """u = -(y - 1/2), v = x - 1/2 (omega = 1), LINEAR, TIME mode, one revolution in N substeps of h = 2 pi / N: every substep multiplies the
    offset z = (x - 1/2) + i (y - 1/2) by 1 + i theta (EULER) or 1 + i theta - theta^2 / 2 (RK2), theta = 2 pi / N.  No visited cell has a
    boundary face, where the reconstruction of a linear field is exact up to rounding: 256 substeps of a few dozen roundings of 2^-53 each,
    relative to the box, are about 1e-12 — the test asks for 1e-9 of the radius.  The distance to the seed after one revolution then falls
    by 4.000 (RK2) and 2.079 (EULER) from 128 to 256 substeps."""
    a, m = hex_mesh(16, 16, 4, lx=1.0, ly=1.0, lz=0.25)
    cc = np.asarray(a["cell_centroid"])
    s, f, gu = solver_with(a, m, RECON[recon], fields=(-(cc[:, 1] - 0.5), cc[:, 0] - 0.5, np.zeros(a.n_cells)))
    k = np.arange(64)
    radius, angle = 0.1 + 0.2 * k / 63.0, 2.0 * np.pi * k / 64.0
    seeds = np.stack([0.5 + radius * np.cos(angle), 0.5 + radius * np.sin(angle), np.full(64, 0.25 * 1.5 / 4.0)], axis=1)
    z0 = (seeds[:, 0] - 0.5) + 1j * (seeds[:, 1] - 0.5)
    radius = np.abs(z0)
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    boundary_cell = np.zeros(a.n_cells, bool)
    boundary_cell[c0[c1 < 0]] = True
    dist, worst = {}, 0.0
    for scheme in (TR.EULER, TR.RK2):
        for N in (128, 256):
            theta = 2.0 * np.pi / N
            t = m.seed(seeds)
            path, plen = s.advect(t, make(theta, scheme=scheme, interpolation=TR.LINEAR, step_mode=TR.TIME, direction=1), N, record_stride=8)
            got = t.get()
            assert np.all(got["status"] == TR.ACTIVE) and np.all(got["steps"] == N) and np.all(plen == N // 8 + 1)
            visited = PR.locate(a, path.reshape(-1, 3))
            assert np.all(visited["status"] == PR.INSIDE) and not np.any(boundary_cell[visited["cell"]])
            factor = (1.0 + 1j * theta) if scheme == TR.EULER else (1.0 + 1j * theta - theta * theta / 2.0)
            want = z0 * factor ** N
            z = (got["positions"][:, 0] - 0.5) + 1j * (got["positions"][:, 1] - 0.5)
            dev = np.abs(z - want) / radius
            worst = max(worst, float(dev.max()))
            assert same_bits(got["positions"][:, 2], seeds[:, 2])
            assert same_bits(got["age"], np.cumsum(np.full((N, 64), theta), axis=0)[-1])  # the sum of the accepted h, in order
            dist[scheme, N] = np.abs(z - z0) / radius
    print("solid-body rotation, %s: largest deviation from the closed form %.3e radii" % (recon, worst))
    print("distance to the seed after one revolution, radii: EULER %.4f -> %.4f, RK2 %.3e -> %.3e"
          % (dist[TR.EULER, 128].max(), dist[TR.EULER, 256].max(), dist[TR.RK2, 128].max(), dist[TR.RK2, 256].max()))
    assert worst <= 1e-9
    r2, r1 = dist[TR.RK2, 128] / dist[TR.RK2, 256], dist[TR.EULER, 128] / dist[TR.EULER, 256]
    assert np.all((r2 >= 3.9) & (r2 <= 4.1)), (r2.min(), r2.max())
    assert np.all((r1 >= 2.0) & (r1 <= 2.2)), (r1.min(), r1.max())


# ------------------------------------------------------------------ 5. the sampler
@pytest.mark.parametrize("recon", list(RECON), ids=list(RECON))
def test_sample_tracers_equals_the_probes_at_the_same_points(gpu, tmp_path, recon):
    a, m = gpu_mesh("poly", tmp_path)
    s, f, gu = solver_with(a, m, RECON[recon])
    t = m.seed(tracer_seeds(a))
    s.advect(t, make(length_step(a), scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.LENGTH, direction=1), 20)
    got = t.get()
    active = got["status"] == TR.ACTIVE
    assert active.sum() >= 100
    loc = PR.locate(a, got["positions"])
    keep = active & (loc["excess"] < 0.0)  # a particle exactly on a face may be claimed by either side
    assert np.all(loc["status"][active] == PR.INSIDE) and np.mean(~keep[active]) < 0.01
    assert np.array_equal(loc["cell"][keep], got["cell"][keep])  # the walk from the nearest centroid ends in the carried cell
    p = m.locate(got["positions"])
    names = ("u", "v", "w", "p")
    for interpolation in ("cell", "linear"):
        want, have = s.sample(p, names, interpolation), s.sample_tracers(t, names, interpolation)
        assert list(have) == list(names)
        for k in names:
            assert same_bits(have[k][keep], want[k][keep]), (interpolation, k)
    assert not same_bits(s.sample_tracers(t, "u", "linear")["u"][keep], s.sample_tracers(t, "u", "cell")["u"][keep])
    assert same_bits(s.sample_tracers(t, "u", "cell")["u"], f[0][got["cell"]])


def test_streamlines_join_the_backward_half_to_the_forward_half(gpu, tmp_path):
    from orc_amd import io as orc_io
    a, m = hex_mesh(12, 8, 6)
    T = TR.Tables(a)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    seeds, step = tracer_seeds(a, 50, seed=8), length_step(a)
    both, forward = s.streamlines(seeds, step, 14, both_directions=True), s.streamlines(seeds, step, 14)
    half = {}
    for direction in (1, -1):
        out = TR.advect(T, TR.seed(T, seeds), f, gu, TR.RK2, TR.LINEAR, TR.LENGTH, direction, step, 0.0, 14, record_stride=1)
        half[direction] = [out["path"][:out["path_len"][i], i] for i in range(50)]
    assert len(both) == len(forward) == 50
    for i in range(50):
        assert same_bits(forward[i], half[1][i]), i
        assert same_bits(both[i], np.concatenate([half[-1][i][:0:-1], half[1][i]])), i
        assert len(both[i]) == len(half[1][i]) + len(half[-1][i]) - 1
    euler = s.streamlines(seeds, step, 14, scheme=TR.EULER, interpolation=TR.CELL)
    assert any(len(x) != len(y) or not same_bits(x, y) for x, y in zip(euler, forward))
    path = tmp_path / "streamlines.vtu"
    orc_io.write_vtu_lines(str(path), both, {"index": np.concatenate([np.arange(len(x), dtype=np.float64) for x in both])})
    assert path.stat().st_size > 24 * sum(len(x) for x in both)


# ------------------------------------------------------------------ 6. tracking inside advance
def test_tracking_equals_advection_by_hand_after_every_step_and_changes_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = m.n_cells
    x = seeded_points(a, 100, seed=23)
    p = m.locate(x)
    names = ("u", "v", "w", "p")
    dt = 1e-3

    def fresh():
        s = Solver(m, settings(solver_type=BICGSTAB, iterations=30), RHO, MU)
        z = np.zeros(n)
        s.set_fields(z, z, z, z)
        s.set_transient(transient(dt, 1, 2))
        s.set_probe_history(p, names, "linear")
        return s

    kw = dict(scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.TIME, direction=1)
    tracked, by_hand = fresh(), fresh()
    t1, t2 = m.seed(x), m.seed(x)
    tracked.set_tracer_tracking(t1, make(0.0, **kw), substeps=2)  # the step is ignored
    rep1, rep2 = [], []
    for step in range(4):
        rep1.append(tracked.advance(1, report=True)[0])
        if step == 1:  # snapshot and restore leave the set alone
            before = t1.get()
            tracked.snapshot()
            tracked.restore()
            after = t1.get()
            assert all(np.array_equal(before[k], after[k]) for k in before)
        rep2.append(by_hand.advance(1, report=True)[0])
        by_hand.advect(t2, make(dt / 2, **kw), 2)
    g1, g2 = t1.get(), t2.get()
    assert np.any(g1["steps"] == 8) and not same_bits(g1["positions"], x)
    for k in g1:
        eq = same_bits if g1[k].dtype == np.float64 else np.array_equal
        assert eq(g1[k], g2[k]), k
    # the tracked run is the untracked run, in every bit
    assert same_bits(np.array(rep1), np.array(rep2))
    for u1, u2 in zip(tracked.get_fields(), by_hand.get_fields()):
        assert same_bits(u1, u2)
    assert same_bits(tracked.surface_report().raw, by_hand.surface_report().raw)
    (times1, h1), (times2, h2) = tracked.probe_history(), by_hand.probe_history()
    assert len(times1) == 4 and same_bits(times1, times2)
    for k in names:
        assert same_bits(h1[k], h2[k]), k
    # off again: the set stays where it is
    tracked.set_tracer_tracking(None)
    tracked.advance(1)
    assert same_bits(t1.positions, g1["positions"])


# ------------------------------------------------------------------ 7. arguments
def test_refused_arguments_leave_solver_and_set_alone(gpu):
    from orc_amd._lib import OrcError, lib
    from orc_amd import parallel
    from orc_amd.mesh import Mesh
    from orc_amd.solver import Solver
    L = lib()
    a, m = hex_mesh(5, 4, 3)
    s, f, gu = solver_with(a, m, GREEN_GAUSS)
    seeds = tracer_seeds(a, 10)
    t = m.seed(seeds)
    st = C.c_int(0)
    f64 = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.orc_tracers_create(None, 10, f64(seeds), C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_tracers_create(m.ptr, 10, None, C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_tracers_create(m.ptr, 0, f64(seeds), C.byref(st)) is None and st.value == BAD_ARGUMENT
    for bad in (np.nan, np.inf):
        y = seeds.copy()
        y[3, 1] = bad
        with pytest.raises(OrcError) as e:
            m.seed(y)
        assert e.value.status == BAD_ARGUMENT
    ap, halo, _ = parallel.partition_arrays(a, 2, 0)
    with pytest.raises(OrcError) as e:
        parallel.PartitionedMesh(ap, halo).seed(seeds)
    assert e.value.status == BAD_ARGUMENT and "partitioned" in str(e.value)
    assert L.orc_tracers_get(None, None, None, None, None, None, None) == BAD_ARGUMENT
    assert L.orc_tracers_get(t.ptr, None, None, None, None, None, None) == 0  # every output may be NULL
    other = Mesh(a).seed(seeds)
    good = dict(step=length_step(a))
    path = np.zeros((3, 3, 10))
    refused = [
        lambda: L.orc_solver_advect_tracers(None, t.ptr, C.byref(make(**good)), 1, 0, None, None),
        lambda: L.orc_solver_advect_tracers(s.ptr, None, C.byref(make(**good)), 1, 0, None, None),
        lambda: L.orc_solver_advect_tracers(s.ptr, t.ptr, None, 1, 0, None, None),
        lambda: s.advect(other, make(**good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(scheme=2, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(interpolation=2, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(step_mode=2, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(direction=0, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(0.0), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(-1.0), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(np.inf), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(np.nan), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(min_speed=-1.0, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(min_speed=np.nan, **good), 1, raise_on_error=False)[0],
        lambda: s.advect(t, make(**good), 5, record_stride=2, raise_on_error=False)[0],
        lambda: L.orc_solver_advect_tracers(s.ptr, t.ptr, C.byref(make(**good)), 4, 2, None, None),
        lambda: L.orc_solver_sample_tracers(s.ptr, None, 1, 0, f64(path)),
        lambda: L.orc_solver_sample_tracers(s.ptr, t.ptr, 1, 0, None),
        lambda: s.sample_tracers(t, 0, "cell", raise_on_error=False)[0],
        lambda: s.sample_tracers(t, "phi", "cell", raise_on_error=False)[0],  # no scalar arm
        lambda: s.sample_tracers(other, "u", "cell", raise_on_error=False)[0],
        lambda: s.set_tracer_tracking(t, make(step_mode=TR.TIME), 1, raise_on_error=False),  # no transient arm
        lambda: L.orc_solver_set_tracer_tracking(None, t.ptr, C.byref(make(**good)), 1),
        lambda: L.orc_bench_tracers(s.ptr, t.ptr, C.byref(make(0.0)), 1, 1, f64(path)),
    ]
    for i, call in enumerate(refused):
        assert call() == BAD_ARGUMENT, i
        assert same_bits(t.positions, seeds) and np.all(t.steps == 0)
    s.set_transient(transient(1e-3, 1, 2))
    tracking = [
        lambda: s.set_tracer_tracking(t, make(step_mode=TR.LENGTH), 1, raise_on_error=False),
        lambda: s.set_tracer_tracking(t, make(step_mode=TR.TIME, direction=-1), 1, raise_on_error=False),
        lambda: s.set_tracer_tracking(t, make(step_mode=TR.TIME), 0, raise_on_error=False),
        lambda: s.set_tracer_tracking(other, make(step_mode=TR.TIME), 1, raise_on_error=False),
        lambda: s.set_tracer_tracking(t, None, 1, raise_on_error=False),
    ]
    for i, call in enumerate(tracking):
        assert call() == BAD_ARGUMENT, i
    for g, w in zip(s.get_fields(), list(f) + [np.zeros(a.n_cells)]):
        assert same_bits(g, w)
    assert s.set_tracer_tracking(t, make(step_mode=TR.TIME), 3) == 0 and s.set_tracer_tracking(None) == 0
    assert s.bench_tracers(t, make(**good), 4, reps=2) > 0.0


def test_a_refused_zone_type_leaves_the_set_as_it_was(gpu):
    """LINEAR on a mesh with a zone type the assembly refuses: ORC_ERR_UNSUPPORTED_BC as the probes' sampler, the set untouched; CELL goes"""
    from orc_amd.solver import Solver
    a, m = hex_mesh(5, 4, 3)
    s = Solver(m, settings(solver_type=BICGSTAB), RHO, MU)
    f = tracer_fields(a)
    s.set_fields(*f, np.zeros(a.n_cells))
    a.set_zone("TOP_WALL", 36)  # OUTFLOW: a type the assembly refuses (tests/surface_restatement.py); a solver is not created on it
    m.update_zones()
    seeds = tracer_seeds(a, 200, seed=2)
    t = m.seed(seeds)
    c = make(length_step(a))
    st, _ = s.advect(t, c, 6, record_stride=2, raise_on_error=False)
    assert st == 7  # ORC_ERR_UNSUPPORTED_BC
    got = t.get()
    assert same_bits(got["positions"], seeds) and np.all(got["steps"] == 0) and np.all(got["age"] == 0.0) and np.all(got["status"] == TR.ACTIVE)
    s.advect(t, make(length_step(a), interpolation=TR.CELL), 6)
    assert t.steps.max() == 6
