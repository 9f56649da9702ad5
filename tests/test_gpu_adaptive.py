"""Adaptive time stepping on the device (orc_amd/csrc/courant.hip, api_transient.cpp): the Courant reduction against the derived field
bit for bit, the variable-step time term of the momentum and scalar systems exactly, fixed steps through the new paths, start-up
Couette with changing steps against the variable-step model (tests/adaptive_restatement.py), its temporal order, the controller inside
advance against the law applied by hand, the arms that follow the step actually taken, the time state, the refusals, two ranks.

Bit for bit means equal uint64 views of the doubles."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_restatement as A
import helpers as H
import stats_restatement as SR
import transient_restatement as R
from conftest import ROOT, splitmix64_uniform
from test_gpu_transient import (HGT, MU, NY, RHO, U_TOP, channel_flow, couette_mesh, diag_slots, poiseuille_start, poly_channel, row_of,
                                settings, transient)

pytestmark = pytest.mark.gpu

BICGSTAB = 3
BAD_ARGUMENT = 10
GREEN_GAUSS, LEAST_SQUARES = 0, 2
HEX_SHAPES = {"hex255": (17, 5, 3), "hex256": (8, 8, 4), "hex2048": (16, 16, 8), "hex2057": (11, 11, 17)}
REDUCTION_MESHES = ["channel_flow", "poly", "couette"] + list(HEX_SHAPES)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def control(**kw):
    from orc_amd.settings import TimeStepControl
    return TimeStepControl.make(**kw)


def hex_case(shape, ordering=None):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    a = set_channel_bcs(hex_channel(*shape), dp_dx=5.0)
    return a, Mesh(a, ordering=ordering)


def reduction_mesh(name, tmp_path, ordering=None):
    if name == "channel_flow":
        return channel_flow(ordering=ordering)
    if name == "poly":
        return poly_channel(tmp_path)
    if name == "couette":
        return couette_mesh()
    return hex_case(HEX_SHAPES[name], ordering)


def first_attaining(rate):
    """the smallest index whose rate is the maximum, a NaN ranking above every number"""
    nan = np.isnan(rate)
    return int(np.flatnonzero(nan)[0]) if nan.any() else int(np.flatnonzero(rate == rate.max())[0])


# ------------------------------------------------------------------ 1. the reduction
@pytest.mark.parametrize("arm", [GREEN_GAUSS, LEAST_SQUARES], ids=["green_gauss", "least_squares"])
@pytest.mark.parametrize("mesh_name", REDUCTION_MESHES)
def test_courant_is_the_maximum_of_the_derived_rate_bit_for_bit(gpu, tmp_path, mesh_name, arm):
    from orc_amd.solver import Solver
    a, m = reduction_mesh(mesh_name, tmp_path)
    n = m.n_cells
    if mesh_name in HEX_SHAPES:
        assert n == int(mesh_name[3:])
    base = H.rough_fields(np.asarray(a["cell_centroid"]))
    last_group = 256 * ((n - 1) // 256)  # the first cell of the last, possibly ragged, workgroup
    cases = {"rough": {}, "spike_first": {0: 50.0}, "spike_last": {n - 1: 50.0}, "spike_last_group": {last_group: 50.0},
             "two_spikes": {n // 3: 50.0, (2 * n) // 3: 50.0}, "at_rest": None, "one_nan": {n // 2: float("nan")}}
    s = Solver(m, settings(solver_type=BICGSTAB, gradient_reconstruction=arm), 1000.0, 1e-3)
    for what, spikes in cases.items():
        f = [x.copy() for x in base]
        if spikes is None:  # every rate is 0: every cell attains the maximum
            f[0][:], f[1][:], f[2][:] = 0.0, 0.0, 0.0
        else:
            for c, v in spikes.items():
                f[0][c] = v if v != v else f[0][c] + v
        s.set_fields(*f)
        report = s.surface_report().raw.copy()
        want = s.derived_fields("convective_rate")["convective_rate"]
        r1, c1, field = s.courant(field=True)
        r2, c2 = s.courant()
        r3, c3, field3 = s.courant(field=True)
        assert same_bits(field, want) and same_bits(field3, want), (mesh_name, what)
        if what == "one_nan":
            assert np.isnan(want).any() and np.isnan(r1) and np.isnan(r2)
        else:
            assert np.isfinite(want).all() and same_bits(r1, want.max()), (mesh_name, what, r1, want.max())
        if what == "at_rest":
            assert r1 == 0.0 and c1 == 0
        assert c1 == first_attaining(want), (mesh_name, what, c1, first_attaining(want))
        assert same_bits(r1, r2) and same_bits(r1, r3) and c1 == c2 == c3  # with and without the field, and repeated
        for x, y in zip(s.get_fields(), f):
            assert same_bits(x, y)
        assert same_bits(s.surface_report().raw, report)


@pytest.mark.parametrize("mesh_name", ["channel_flow", "hex2057"])
def test_a_reordered_mesh_gives_the_same_rate_and_the_same_orc_cell(gpu, tmp_path, mesh_name):
    from orc_amd.solver import Solver
    a, m = reduction_mesh(mesh_name, tmp_path)
    _, mr = reduction_mesh(mesh_name, tmp_path, ordering=1)
    assert not np.array_equal(mr.cell_order(), np.arange(m.n_cells))
    f = H.rough_fields(np.asarray(a["cell_centroid"]))
    for spike in (None, 7, m.n_cells - 2):
        g = [x.copy() for x in f]
        if spike is not None:
            g[1][spike] += 30.0
        out = []
        for mesh in (m, mr):
            s = Solver(mesh, settings(solver_type=BICGSTAB), 1000.0, 1e-3)
            s.set_fields(*g)
            out.append(s.courant(field=True))
        assert same_bits(out[0][0], out[1][0]) and out[0][1] == out[1][1] and same_bits(out[0][2], out[1][2])


# ------------------------------------------------------------------ 2. exact assembly
@pytest.mark.parametrize("mesh_name", ["channel_flow", "channel_flow_rcm", "poly"])
def test_variable_step_assembly_is_the_steady_assembly_plus_the_time_term(gpu, tmp_path, mesh_name):
    from orc_amd.solver import Solver
    if mesh_name == "poly":
        a, m = poly_channel(tmp_path)
    else:
        a, m = channel_flow(ordering=1 if mesh_name.endswith("rcm") else None)
    n = m.n_cells
    g = m.cell_order()
    vol = np.asarray(a["cell_volume"])[g]
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    lv = [fields[k] * (1 + 0.1 * splitmix64_uniform(n, 11 + k)) for k in range(3)]
    lv1 = [fields[k] * (1 - 0.07 * splitmix64_uniform(n, 21 + k)) for k in range(3)]
    rho, mu, dt0 = 1000.0, 1e-3, 3.7e-3
    ds = diag_slots(m)
    kw = dict(momentum=5, solver_type=BICGSTAB)
    steady = Solver(m, settings(**kw), rho, mu)
    steady.set_fields(*fields)
    ref = steady.assemble_momentum()
    for scheme, ratio in ((1, 1.5), (1, 0.5), (1, 1.0), (0, 1.5)):
        s = Solver(m, settings(**kw), rho, mu)
        s.set_fields(*fields)
        s.set_transient(transient(dt0, scheme))
        s.set_time_levels(*lv, *lv1)
        dt = ratio * dt0
        s.set_time_step(dt)
        state = s.time_state()
        assert (state["dt_next"], state["dt_last"], state["time"]) == (dt, dt0, 0.0)
        got = s.assemble_momentum()
        c = (rho * vol) / dt
        if scheme == 1:
            a0, a1, a2 = A.coefficients(dt / dt0)
            add, rhs = a0 * c, [c * (a1 * lv[k][g] - a2 * lv1[k][g]) for k in range(3)]
        else:
            add, rhs = c, [c * lv[k][g] for k in range(3)]
        for k in range(3):
            want = ref[k].copy()
            want[ds] = ref[k][ds] + add
            assert np.array_equal(got[k], want), (mesh_name, scheme, ratio, k)
            assert np.array_equal(got[3 + k], ref[3 + k] + rhs[k]), (mesh_name, scheme, ratio, k)
        assert got[6] == ref[6]


@pytest.mark.parametrize("mesh_name", ["hex", "hex_rcm", "poly"])
def test_variable_step_scalar_assembly_is_the_steady_one_plus_the_time_term(gpu, tmp_path, mesh_name):
    import scalar_restatement as S
    from orc_amd.settings import Transient
    from test_gpu_scalar import ASSEMBLY_BCS, ASSEMBLY_TYPES, hex_mesh, make_solver, mixed_mesh, scalar_settings, seeded_flow
    if mesh_name == "poly":
        a, m = mixed_mesh(tmp_path, True, ASSEMBLY_TYPES)
    else:
        a, m = hex_mesh(8, 6, 4, ordering=1 if mesh_name == "hex_rcm" else None, types=ASSEMBLY_TYPES)
    n = a.n_cells
    g = m.cell_order()
    vol = np.asarray(a["cell_volume"])[g]
    ds = diag_slots(m)
    flow = seeded_flow(a)
    rho, gamma, dt0 = 1.3, 2.5e-4, 2.7e-3
    phi = 0.5 + 0.5 * splitmix64_uniform(n, 7)
    src = 3.0 * splitmix64_uniform(n, 8)
    lv = [phi * (1 + 0.1 * splitmix64_uniform(n, 9)), phi * (1 - 0.1 * splitmix64_uniform(n, 10))]

    def solver():
        s, _, _ = make_solver(m, a, scalar_settings(scheme=S.CD1, diffusivity=gamma), ASSEMBLY_BCS, flow, rho=rho)
        s.set_scalar_field(phi)
        s.set_scalar_source(src)
        return s

    ref_a, ref_b = solver().assemble_scalar()
    for ratio in (1.5, 0.5):
        s = solver()
        s.set_transient(Transient.make(dt0, S.BDF2, 1))
        s.set_scalar_levels(lv[0], lv[1])
        dt = ratio * dt0
        s.set_time_step(dt)
        got_a, got_b = s.assemble_scalar()
        c = (rho * vol) / dt
        a0, a1, a2 = A.coefficients(dt / dt0)
        want_a = ref_a.copy()
        want_a[ds] = ref_a[ds] + a0 * c
        assert np.array_equal(got_a, want_a), (mesh_name, ratio)
        assert np.array_equal(got_b, ref_b + c * (a1 * lv[0][g] - a2 * lv[1][g])), (mesh_name, ratio)


# ------------------------------------------------------------------ 3. a fixed step through the new paths
def poiseuille_solver(m, a, scheme, dt=0.01, inner=4):
    from orc_amd.solver import Solver
    s = Solver(m, settings(momentum=1, solver_type=BICGSTAB, iterations=50, relative_convergence_threshold=1e-10), 1000.0, 1e-3)
    s.set_fields(*poiseuille_start(a))
    s.set_transient(transient(dt, scheme, inner))
    return s


@pytest.mark.parametrize("scheme", [0, 1])
def test_a_fixed_step_through_the_new_paths_keeps_every_bit(gpu, scheme):
    a, m = channel_flow()
    dt, steps = 0.01, 5
    plain = poiseuille_solver(m, a, scheme, dt)
    want = plain.advance(steps, report=True)
    held = poiseuille_solver(m, a, scheme, dt)
    held.set_time_step_control(control(target_courant=0.5, dt_min=dt, dt_max=dt))
    got_held = held.advance(steps, report=True)
    manual = poiseuille_solver(m, a, scheme, dt)
    rows = []
    for _ in range(steps):
        manual.set_time_step(dt)
        rows.append(manual.advance(1, report=True)[0])
    assert want.shape == (steps, 10)
    for s, rep in ((held, got_held), (manual, np.array(rows))):
        assert same_bits(rep, want)
        for x, y in zip(s.get_fields(), plain.get_fields()):
            assert same_bits(x, y)
        h = s.time_step_history()
        assert h.shape == (steps, 4) and np.all(h[:, 1] == dt) and same_bits(h[:, 0], want[:, 9])
    assert np.all(held.time_step_history()[:, 2] > 0.0) and np.isnan(manual.time_step_history()[:, 2]).all()
    assert plain.time_step_history().shape == (0, 4)


# ------------------------------------------------------------------ 4.-5. start-up Couette with changing steps
def couette_var(mesh, scheme, dts, inner=2):
    from orc_amd.solver import Solver
    kw = dict(momentum=0, solver_type=BICGSTAB, iterations=100, relative_convergence_threshold=1e-13)
    s = Solver(mesh, settings(**kw), RHO, MU)
    z = np.zeros(mesh.n_cells)
    s.set_fields(z, z, z, z)
    s.set_transient(transient(float(dts[0]), scheme, inner))
    rows = []
    for dt in dts:
        s.set_time_step(float(dt))
        rows.append(s.advance(1, report=True)[0])
    return s.get_fields(), np.array(rows), s


@pytest.mark.parametrize("scheme", [0, 1])
def test_startup_couette_with_changing_steps_matches_the_variable_step_model(gpu, scheme):
    a, m = couette_mesh()
    nu = MU / RHO
    steps = 12
    dts = 0.01 * HGT ** 2 / nu * np.array([1.0, 1.5] * (steps // 2))
    (u, v, w, p), rep, s = couette_var(m, scheme, dts)
    K, f = R.operator(NY, HGT, nu, u_top=U_TOP)
    model = A.march_var(K, f, np.zeros(NY), dts, scheme)
    want = model[-1][row_of(a)]
    err = H.rel_l2(u, want)
    kept = H.rel_l2(A.march_var(K, f, np.zeros(NY), dts, scheme, coef=lambda w: (1.5, 2.0, 0.5))[-1][row_of(a)], want)
    print("scheme %d: rel-L2 to the variable-step model %.3e; coefficients kept at 1.5 / 2 / 0.5 would be off by %.3e" % (scheme, err, kept))
    assert err <= 1e-8, err
    assert scheme == 0 or kept > 1e-5  # the bound tells the two apart by orders of magnitude
    t, run = 0.0, []
    for dt in dts:
        t += float(dt)
        run.append(t)
    assert same_bits(rep[:, 9], run)
    h = s.time_step_history()
    assert same_bits(h[:, 0], run) and same_bits(h[:, 1], dts) and np.isnan(h[:, 2]).all() and np.all(h[:, 3] == -1)
    assert np.all(rep[:, 8] == 2)


@pytest.mark.parametrize("scheme, lo, hi", [(0, 0.9, 1.1), (1, 1.8, 2.2)])
def test_temporal_order_with_changing_steps(gpu, scheme, lo, hi):
    a, m = couette_mesh()
    nu = MU / RHO
    T = 0.2 * HGT ** 2 / nu
    K, f = R.operator(NY, HGT, nu, u_top=U_TOP)
    exact = R.semi_discrete(K, f, np.zeros(NY), T)[row_of(a)]
    errs = []
    for steps in (20, 40, 80):
        (u, _, _, _), rep, _ = couette_var(m, scheme, A.pattern_steps((1, 1.5), steps, T))
        assert abs(rep[-1, 9] - T) <= 1e-12 * T
        errs.append(H.rel_l2(u, exact))
    order = R.observed_order(errs)
    print("scheme %d: errors %s, orders %s" % (scheme, errs, order))
    assert np.all((order >= lo) & (order <= hi)), (errs, order)


# ------------------------------------------------------------------ 6. the controller in the loop
POISEUILLE_CONTROL = dict(target_courant=0.02, dt_min=2e-3, dt_max=5e-2, max_growth=1.2, max_shrink=0.5)


@pytest.mark.parametrize("interval", [1, 3])
def test_the_controller_inside_advance_is_the_law_applied_by_hand(gpu, interval):
    a, m = channel_flow()
    dt0, steps = 0.01, 12
    c = control(interval=interval, **POISEUILLE_CONTROL)
    s = poiseuille_solver(m, a, 1, dt0)
    s.set_time_step_control(c)
    rep = s.advance(steps, report=True)
    h = s.time_step_history()
    assert h.shape == (steps, 4)
    twin = poiseuille_solver(m, a, 1, dt0)
    twin.set_time_step_control(c)
    dt, t = dt0, 0.0
    for k in range(steps):
        assert h[k, 1] == dt, (k, h[k, 1], dt)
        t += dt
        assert h[k, 0] == t and rep[k, 9] == t
        twin.advance(1)
        if (k + 1) % interval == 0:
            rate, cell = twin.courant()
            assert same_bits(h[k, 2], rate) and h[k, 3] == cell and rate > 0.0
            dt = A.step_next(c, dt, h[k, 2])
            from orc_amd.solver import time_step_next
            assert dt == time_step_next(c, h[k, 1], h[k, 2])
        else:
            assert np.isnan(h[k, 2]) and h[k, 3] == -1
    assert s.time_state()["dt_next"] == dt
    assert np.all((h[:, 1] >= c.dt_min) & (h[:, 1] <= c.dt_max))
    assert len(np.unique(h[:, 1])) > 2  # the step did change
    if interval == 3:
        assert np.all(h[0::3, 1] == h[1::3, 1]) and np.all(h[0::3, 1] == h[2::3, 1])
    for x, y in zip(s.get_fields(), twin.get_fields()):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 7. the arms follow the step taken
def test_statistics_probes_and_tracers_see_the_step_actually_taken(gpu):
    from orc_amd.settings import TimeStatistics
    from test_gpu_tracers import make as tracer_settings
    from test_probes_cpu import seeded_points
    import tracer_restatement as TR
    a, m = channel_flow()
    n = m.n_cells
    x = seeded_points(a, 64, seed=23)
    probes = m.locate(x)
    dts = 1e-3 * np.array([1.0, 1.5, 2.25, 1.5, 1.0, 0.5])
    kw = dict(scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.TIME, direction=1)

    def fresh():
        s = poiseuille_solver(m, a, 1, float(dts[0]), inner=2)
        s.set_fields(*H.rough_fields(np.asarray(a["cell_centroid"])))
        return s

    s, by_hand = fresh(), fresh()
    s.set_time_statistics(TimeStatistics.make(groups=SR.MEAN, start_step=1, interval=1))
    s.set_probe_history(probes, ("u", "p"), "linear")
    t1, t2 = m.seed(x), m.seed(x)
    s.set_tracer_tracking(t1, tracer_settings(0.0, **kw), substeps=2)
    run = SR.Running(SR.MEAN, n)
    for dt in dts:
        for solver in (s, by_hand):
            solver.set_time_step(float(dt))
            solver.advance(1)
        u, v, w, p = by_hand.get_fields()
        run.sample(float(dt), dict(u=u, v=v, w=w, p=p))
        by_hand.advect(t2, tracer_settings(float(dt) / 2, **kw), 2)
    h = s.time_step_history()
    assert same_bits(h[:, 1], dts)
    got = s.statistics(normalised=False)
    for k in ("u", "v", "w", "p"):
        assert same_bits(got[k], run.acc[k]), k
    info = s.statistics_info()
    assert info["samples"] == len(dts) and info["weight_sum"] == run.W
    times, _ = s.probe_history()
    assert same_bits(times, h[:, 0])
    g1, g2 = t1.get(), t2.get()
    assert not same_bits(g1["positions"], x)
    for k in g1:
        eq = same_bits if g1[k].dtype == np.float64 else np.array_equal
        assert eq(g1[k], g2[k]), k
    for f1, f2 in zip(s.get_fields(), by_hand.get_fields()):
        assert same_bits(f1, f2)


@pytest.mark.parametrize("scheme", [0, 1])
def test_scalar_conduction_with_changing_steps_matches_its_model(gpu, scheme):
    import scalar_restatement as S
    from test_gpu_scalar import ALPHA, HY, slab, slab_solver
    from test_gpu_scalar import NY as SLAB_NY
    from test_gpu_scalar import row_of as slab_rows
    a, m = slab()
    K = S.conduction_operator(SLAB_NY, HY, ALPHA)
    T, steps = 0.05 * HY ** 2 / ALPHA, 20
    dts = A.pattern_steps((1, 1.5), steps, T)
    s = slab_solver(m, a, scheme, float(dts[0]))
    s.set_scalar_field(np.ones(a.n_cells))
    for dt in dts:
        s.set_time_step(float(dt))
        s.advance(1)
    model = A.march_var(K, np.zeros(SLAB_NY), np.ones(SLAB_NY), dts, scheme)[-1]
    err = np.abs(s.get_scalar_field() - model[slab_rows(a)]).max()
    print("scheme %d: max |phi - model| = %.3e" % (scheme, err))
    assert err <= 1e-11, err


# ------------------------------------------------------------------ 8. state and arguments
def test_snapshot_and_restore_carry_the_time_state(gpu):
    a, m = channel_flow()
    s = poiseuille_solver(m, a, 1, 0.01)
    s.set_time_step_control(control(interval=2, **POISEUILLE_CONTROL))
    s.advance(3)
    s.snapshot()
    state = s.time_state()
    r1 = s.advance(4, report=True)
    f1, e1 = s.get_fields(), s.time_state()
    assert e1 != state
    s.restore()
    assert s.time_state() == state
    r2 = s.advance(4, report=True)
    assert same_bits(r1, r2) and s.time_state() == e1
    for x, y in zip(f1, s.get_fields()):
        assert same_bits(x, y)
    h = s.time_step_history()
    assert h.shape == (11, 4) and same_bits(h[3:7], h[7:11])  # the history is left alone: both passes are in it


def test_time_levels_and_time_state_continue_a_run_bit_for_bit(gpu):
    a, m = channel_flow()
    c = control(**POISEUILLE_CONTROL)
    whole = poiseuille_solver(m, a, 1, 0.01)
    whole.set_time_step_control(c)
    want = whole.advance(6, report=True)
    s = poiseuille_solver(m, a, 1, 0.01)
    s.set_time_step_control(c)
    levels = []
    for _ in range(3):
        s.advance(1)
        levels.append(s.get_fields()[:3])
    state = s.time_state()
    s.set_transient(transient(0.01, 1, 4))  # the arm from scratch: no levels, time 0, control off, history empty
    assert s.time_step_history().shape == (0, 4) and s.time_state() == dict(time=0.0, dt_next=0.01, dt_last=0.01, dt_before_last=0.01)
    s.set_time_levels(*levels[1], *levels[0])  # the levels the fourth step shifts: it reads fields and n = step 2
    s.set_time_state(state)
    assert s.time_state() == state
    s.set_time_step_control(c)
    got = s.advance(3, report=True)
    assert same_bits(got, want[3:])
    for x, y in zip(s.get_fields(), whole.get_fields()):
        assert same_bits(x, y)
    assert same_bits(s.time_step_history(), whole.time_step_history()[3:])


def test_refusals_return_their_code_and_change_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    nan, inf = float("nan"), float("inf")
    good = control(**POISEUILLE_CONTROL)
    bad_controls = [control(**dict(POISEUILLE_CONTROL, **kw)) for kw in (
        dict(target_courant=0.0), dict(target_courant=nan), dict(dt_min=0.0), dict(dt_min=1.0), dict(dt_max=inf), dict(max_growth=0.9),
        dict(max_growth=2.5), dict(max_shrink=0.0), dict(max_shrink=1.5), dict(interval=0), dict(reserved0=1), dict(reserved1=1),
        dict(dt_min=2e-3, dt_max=5e-3), dict(dt_min=2e-2, dt_max=5e-2))]  # the last two do not contain the first step

    def make(on, poke):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        s.set_fields(*fields)
        if on:
            s.set_transient(transient(1e-2, 1, 5, 1e-3))
            s.set_time_levels(*fields[:3], *fields[:3])
        if poke:
            if not on:
                assert s.set_time_step(1e-3, raise_on_error=False) == BAD_ARGUMENT
                assert s.set_time_step_control(good, raise_on_error=False) == BAD_ARGUMENT
                assert s.set_time_state(1.0, 1e-3, 1e-3, raise_on_error=False) == BAD_ARGUMENT
            for dt in (0.0, -1e-3, nan, inf):
                assert s.set_time_step(dt, raise_on_error=False) == BAD_ARGUMENT, dt
                assert s.set_time_state(0.5, dt, 1e-3, raise_on_error=False) == BAD_ARGUMENT, dt
                assert s.set_time_state(0.5, 1e-3, dt, raise_on_error=False) == BAD_ARGUMENT, dt
            for t in (-1.0, nan, inf):
                assert s.set_time_state(t, 1e-3, 1e-3, raise_on_error=False) == BAD_ARGUMENT, t
            for k, c in enumerate(bad_controls):
                assert s.set_time_step_control(c, raise_on_error=False) == BAD_ARGUMENT, k
            if on:
                assert s.time_state() == dict(time=0.0, dt_next=1e-2, dt_last=1e-2, dt_before_last=1e-2)
                assert s.time_step_history().shape == (0, 4)
        return s

    for on in (False, True):
        got, want = make(on, True).assemble_momentum(), make(on, False).assemble_momentum()
        for x, y in zip(got[:6], want[:6]):
            assert np.array_equal(x, y)
    from orc_amd._lib import lib
    s = make(True, False)
    out = np.zeros(8)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib().orc_solver_time_step_history(s.ptr, 0, 1, p) == BAD_ARGUMENT  # a range past the history
    assert lib().orc_solver_time_step_history(s.ptr, 1, 0, p) == BAD_ARGUMENT
    assert lib().orc_solver_time_step_history(s.ptr, 0, 0, p) == 0
    assert lib().orc_solver_courant(None, None, None, None) == BAD_ARGUMENT


def test_solve_transient_takes_a_control(gpu):
    from orc_amd.solver import solve_transient
    a, m = channel_flow()
    c = control(**POISEUILLE_CONTROL)
    t = transient(0.01, 1, 4)
    f = [x.copy() for x in poiseuille_start(a)]
    seen = []
    st, hist = solve_transient(m, *f, settings(momentum=1, solver_type=BICGSTAB, iterations=50, relative_convergence_threshold=1e-10), 1000.0,
                               1e-3, t, 5, reporting_interval=1, report=lambda *r: seen.append(r[0]), control=c)
    s = poiseuille_solver(m, a, 1, 0.01)
    s.set_time_step_control(c)
    s.advance(5)
    assert st == 0 and seen == [1, 2, 3, 4, 5] and same_bits(hist, s.time_step_history())
    for x, y in zip(f, s.get_fields()):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 9. two ranks
def test_two_ranks_on_one_gpu_choose_the_same_steps_as_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "adaptive_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "ADAPTIVE_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
