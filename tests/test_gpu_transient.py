"""Implicit time stepping (orc_solver_set_transient / advance / orc_solve_transient) on the device: the assembled systems
exactly, start-up Couette against the 1-D finite-volume restatement (tests/transient_restatement.py), observed temporal
order, start-up Poiseuille against the analytical series and the steady solution, the default Multigrid path, steady
behaviour untouched, argument checking and two ranks on one GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import transient_restatement as R
from conftest import GOLDEN, ROOT, splitmix64_uniform

pytestmark = pytest.mark.gpu

JACOBI, MULTIGRID, BICGSTAB = 1, 2, 3
BAD_ARGUMENT = 10


def channel_flow(dp_dx=5.0, ordering=None):
    """channel_flow.msh with the boundary conditions of tests.rs:60-76 (H.channel_bcs)"""
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays
    d = orc_io.read_mesh(os.path.join(GOLDEN, "meshes", "channel_flow.msh"))
    H.channel_bcs(_ZoneAdapter(d), dp_dx=dp_dx)
    a = MeshArrays(d.arrays())
    return a, Mesh(a, ordering=ordering)


class _ZoneAdapter:
    def __init__(self, d):
        self.d = d

    def zone_names(self):
        return self.d.arrays()["zone_names"]

    def set_zone(self, name, zt, scalar=0.0, vector=(0.0, 0.0, 0.0)):
        self.d.set_zone(name, zt, scalar, vector)


def poly_channel(tmp_path):
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays, set_mixed_channel_bcs, write_mixed_channel_msh
    path = str(tmp_path / "poly.msh")
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=True)
    a = set_mixed_channel_bcs(MeshArrays(orc_io.read_mesh(path).arrays()))
    return a, Mesh(a)


def transient(dt, scheme=0, inner=3, tol=0.0):
    from orc_amd.settings import Transient
    return Transient.make(dt, scheme, inner, tol)


def settings(**kw):
    from orc_amd.settings import NumericalSettings
    return NumericalSettings.default(**kw)


def diag_slots(mesh):
    rp, ci = mesh.matrix_pattern()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    d = np.nonzero(ci == rows)[0]
    assert len(d) == mesh.n_cells
    return d


# ------------------------------------------------------------------ 1. exact assembly
@pytest.mark.parametrize("mesh_name", ["channel_flow", "channel_flow_rcm", "poly"])
def test_transient_assembly_is_the_steady_assembly_plus_the_time_term(gpu, tmp_path, mesh_name):
    from orc_amd.solver import Solver
    if mesh_name == "poly":
        a, m = poly_channel(tmp_path)
    else:
        a, m = channel_flow(ordering=1 if mesh_name.endswith("rcm") else None)
    n = m.n_cells
    g = m.cell_order()  # internal row r holds ORC cell g[r]; fields and levels go in in ORC order
    vol = np.asarray(a["cell_volume"])[g]
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    lv = [fields[k] * (1 + 0.1 * splitmix64_uniform(n, 11 + k)) for k in range(3)]
    lv1 = [fields[k] * (1 - 0.07 * splitmix64_uniform(n, 21 + k)) for k in range(3)]
    rho, mu, dt = 1000.0, 1e-3, 3.7e-3
    ds = diag_slots(m)
    kw = dict(momentum=5, solver_type=BICGSTAB)
    for scheme, levels in ((0, 1), (1, 2), (1, 1), (0, 0)):
        steady = Solver(m, settings(**kw), rho, mu)
        steady.set_fields(*fields)
        ref = steady.assemble_momentum()
        s = Solver(m, settings(**kw), rho, mu)
        s.set_fields(*fields)
        s.set_transient(transient(dt, scheme))
        if levels:
            s.set_time_levels(*lv, *(lv1 if levels == 2 else (None, None, None)))
        got = s.assemble_momentum()
        c = (rho * vol) / dt
        if levels == 0:
            add, rhs = np.zeros(n), [np.zeros(n)] * 3
        elif scheme == 1 and levels == 2:
            add, rhs = 1.5 * c, [c * (2.0 * lv[k][g] - 0.5 * lv1[k][g]) for k in range(3)]
        else:
            add, rhs = c, [c * lv[k][g] for k in range(3)]
        for k in range(3):
            want = ref[k].copy()
            want[ds] = ref[k][ds] + add if levels else ref[k][ds]
            assert np.array_equal(got[k], want), (mesh_name, scheme, levels, k)
            assert np.array_equal(got[3 + k], ref[3 + k] + rhs[k] if levels else ref[3 + k]), (mesh_name, scheme, levels, k)
        assert got[6] == ref[6]  # the Peclet statistics are taken before the time term


# ------------------------------------------------------------------ 2.-3. start-up Couette against the discrete model
# rho = mu = 1 and U = 1e-6 m/s: the cell Reynolds number is 1e-12.  ORC's pressure inlet drops the momentum that enters
# through it (the boundary face's a_nb u_b term goes nowhere, discretization.rs:226, 294-307), so the inlet column of an
# x-uniform flow loses rho u^2 A per cell, and UD carries that deficit downstream; it is second order in U against the first
# order viscous and time terms.  At this Reynolds number it is ~4e-12 of them and the flow is 1-D to round-off.
NX, NY, NZ = 8, 32, 1
HGT, RHO, MU, U_TOP = 1e-3, 1.0, 1.0, 1e-6


def couette_mesh():
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    a = set_channel_bcs(hex_channel(NX, NY, NZ), top_wall_velocity=U_TOP, dp_dx=0.0)
    return a, Mesh(a)


def couette_run(mesh, scheme, dt, steps, method=BICGSTAB, inner=2):
    from orc_amd.solver import Solver
    kw = dict(momentum=0, solver_type=method, iterations=100, relative_convergence_threshold=1e-13)
    s = Solver(mesh, settings(**kw), RHO, MU)
    z = np.zeros(mesh.n_cells)
    s.set_fields(z, z, z, z)
    s.set_transient(transient(dt, scheme, inner))
    rep = s.advance(steps, report=True)
    return s.get_fields(), rep


def row_of(a):
    y = np.asarray(a["cell_centroid"])[:, 1]
    return np.floor(y / (HGT / NY)).astype(int)


@pytest.mark.parametrize("scheme", [0, 1])
def test_startup_couette_matches_the_discrete_model(gpu, scheme):
    a, m = couette_mesh()
    nu = MU / RHO
    dt, steps = 0.01 * HGT ** 2 / nu, 12
    (u, v, w, p), rep = couette_run(m, scheme, dt, steps)
    K, f = R.operator(NY, HGT, nu, u_top=U_TOP)
    model = R.march(K, f, np.zeros(NY), dt, steps, scheme)
    want = model[-1][row_of(a)]
    assert H.rel_l2(u, want) <= 1e-8, H.rel_l2(u, want)
    for x in (v, w):  # round-off and the O(Re) inlet deficit above: both far below 1e-8 of the scales
        assert np.abs(x).max() <= 1e-8 * U_TOP, np.abs(x).max()
    assert np.abs(p).max() <= 1e-8 * MU * U_TOP / HGT, np.abs(p).max()
    assert np.allclose(rep[:, 9], dt * np.arange(1, steps + 1), rtol=1e-12)
    assert np.all(rep[:, 8] == 2)
    # and after every step, not only the last (u of the mean row profile)
    assert abs(rep[-1, 0] - want.mean()) <= 1e-8 * abs(want.mean())


@pytest.mark.parametrize("scheme, lo, hi", [(0, 0.9, 1.1), (1, 1.8, 2.2)])
def test_temporal_order(gpu, scheme, lo, hi):
    a, m = couette_mesh()
    nu = MU / RHO
    T = 0.2 * HGT ** 2 / nu
    K, f = R.operator(NY, HGT, nu, u_top=U_TOP)
    exact = R.semi_discrete(K, f, np.zeros(NY), T)[row_of(a)]
    errs = []
    for steps in (20, 40, 80):
        (u, _, _, _), _ = couette_run(m, scheme, T / steps, steps)
        errs.append(H.rel_l2(u, exact))
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), (errs, order)


# ------------------------------------------------------------------ 4. physics: start-up Poiseuille
# The start is u = v = w = 0 with the linear pressure of the boundary values, p = -dp_dx lx (1 - x / lx).  Not the
# pressure of initialize_pressure_field: its ten Jacobi sweeps at relaxation 0.1 (solver.rs:414-509) leave p on this mesh
# almost where it started (rel-L2 0.997 from the linear field), and with the default pressure relaxation of 0.01 SIMPLE
# needs hundreds of iterations to build the gradient up, so the flow would not be driven by the constant G of the series.
def poiseuille_start(a, dp_dx=5.0, lx=0.002):
    x = np.asarray(a["cell_centroid"])[:, 0]
    z = np.zeros(len(x))
    return z.copy(), z.copy(), z.copy(), -dp_dx * lx * (1.0 - x / lx)


def test_startup_poiseuille_follows_the_series(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    y = np.asarray(a["cell_centroid"])[:, 1]
    rho, mu = 1000.0, 1e-3
    s = Solver(m, settings(momentum=1, solver_type=BICGSTAB, iterations=50, relative_convergence_threshold=1e-10), rho, mu)
    s.set_fields(*poiseuille_start(a))
    s.set_transient(transient(0.01, 1, 30, 1e-4))
    errs = []
    for t_end, steps in ((0.1, 10), (0.3, 20)):
        rep = s.advance(steps, report=True)
        assert abs(rep[-1, 9] - t_end) < 1e-12
        u = s.get_fields()[0]
        errs.append(H.rel_l2(u, R.poiseuille_series(y, t_end, HGT, mu, rho, -5.0)))
    assert max(errs) < 0.01, errs


def test_long_transient_run_ends_at_the_steady_solution(gpu):
    """Large steps from the start of test_gpu_solve_steady's converged-fields test (from rest, steady SIMPLE with CD1 and the
    reference's relaxation runs off to infinity on this mesh): the time term vanishes at a fixed point, and so does its trace in
    Rhie-Chow's V/a weights, which multiply (p_i - p_j)/|d| - grad p . d/|d|, zero for the linear pressure of this flow."""
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = m.n_cells
    cc = np.asarray(a["cell_centroid"])
    start = (H.analytical_poiseuille(cc[:, 1]) * (1 + 0.02 * splitmix64_uniform(n, 1)), 1e-7 * splitmix64_uniform(n, 2),
             1e-12 * splitmix64_uniform(n, 3), -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4)))
    kw = dict(momentum=1, solver_type=BICGSTAB, iterations=50)
    steady = Solver(m, settings(**kw), 1000.0, 1e-3)
    steady.set_fields(*start)
    steady.iterate(1500)
    us, vs, ws, ps = steady.get_fields()
    assert np.isfinite(us).all() and H.rel_l2(us, H.analytical_poiseuille(cc[:, 1])) < 0.01
    s = Solver(m, settings(**kw), 1000.0, 1e-3)
    s.set_fields(*start)
    s.set_transient(transient(100.0, 0, 20))
    s.advance(75)
    u, v, w, p = s.get_fields()
    assert np.isfinite(u).all()
    du, dp = H.rel_l2(u, us), H.rel_l2(p, ps)
    assert du < 1e-6 and dp < 1e-6, (du, dp)
    assert np.linalg.norm(v - vs) < 1e-6 * np.linalg.norm(us) and np.linalg.norm(w - ws) < 1e-6 * np.linalg.norm(us)


# ------------------------------------------------------------------ 5. default solver path
def test_multigrid_arm_agrees_with_bicgstab_and_repeats_bit_for_bit(gpu):
    a, m = couette_mesh()
    nu = MU / RHO
    dt, steps = 0.01 * HGT ** 2 / nu, 6
    K, f = R.operator(NY, HGT, nu, u_top=U_TOP)
    want = R.march(K, f, np.zeros(NY), dt, steps, 1)[-1][row_of(a)]
    (ub, *_), _ = couette_run(m, 1, dt, steps, method=BICGSTAB, inner=4)
    runs = [couette_run(m, 1, dt, steps, method=MULTIGRID, inner=4) for _ in range(2)]
    (um, vm, wm, pm), rep = runs[0]
    assert H.rel_l2(um, ub) <= 1e-8 and H.rel_l2(um, want) <= 1e-8, (H.rel_l2(um, ub), H.rel_l2(um, want))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(runs[0][1], runs[1][1])
    # the same on a flow with a pressure field: start-up Poiseuille
    from orc_amd.solver import Solver
    a, m = channel_flow()
    out = []
    for method in (BICGSTAB, MULTIGRID):
        s = Solver(m, settings(momentum=1, solver_type=method, iterations=100, relative_convergence_threshold=1e-12), 1000.0, 1e-3)
        s.set_fields(*poiseuille_start(a))
        s.set_transient(transient(0.05, 1, 40))
        s.advance(3)
        out.append(s.get_fields())
    # a fixed count of SIMPLE iterations: the arms agree to what the Multigrid arm's single cycle per solve leaves behind, which
    # SIMPLE (pressure relaxation 0.01) relaxes only slowly — measured 5.2e-6 (u) and 3.0e-6 (p) after 3 x 40 iterations
    assert H.rel_l2(out[1][0], out[0][0]) < 1e-5 and H.rel_l2(out[1][3], out[0][3]) < 1e-5, \
        (H.rel_l2(out[1][0], out[0][0]), H.rel_l2(out[1][3], out[0][3]))


# ------------------------------------------------------------------ 6. steady behaviour unchanged; snapshots
def test_enabling_and_disabling_leaves_steady_iterations_bit_identical(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    out = []
    for toggle in (False, True):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        if toggle:
            s.set_transient(transient(1e-3, 1))
            s.set_time_levels(*fields[:3])
            s.set_transient(None)
        s.set_fields(*fields)
        st, rep = s.iterate(3, report=True)
        out.append((s.get_fields(), rep))
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(out[0][1], out[1][1])


def test_snapshot_restore_includes_the_time_levels(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    s = Solver(m, settings(momentum=1, solver_type=BICGSTAB), 1000.0, 1e-3)
    s.set_fields(*poiseuille_start(a))
    s.set_transient(transient(0.01, 1, 3))
    s.advance(2)
    s.snapshot()
    r1 = s.advance(2, report=True)
    f1 = s.get_fields()
    s.restore()
    r2 = s.advance(2, report=True)
    f2 = s.get_fields()
    assert np.array_equal(r1, r2)
    for x, y in zip(f1, f2):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 7. arguments
def test_invalid_arguments_are_rejected_and_change_nothing(gpu):
    from orc_amd.settings import Transient
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    good = transient(1e-3, 1, 5, 1e-3)
    bad = [Transient(dt=0.0, scheme=0, inner_iterations=1), Transient(dt=-1.0, scheme=0, inner_iterations=1),
           Transient(dt=float("inf"), scheme=0, inner_iterations=1), Transient(dt=float("nan"), scheme=0, inner_iterations=1),
           Transient(dt=1e-3, scheme=2, inner_iterations=1), Transient(dt=1e-3, scheme=-1, inner_iterations=1),
           Transient(dt=1e-3, scheme=0, inner_iterations=0),
           Transient(dt=1e-3, scheme=0, inner_iterations=1, inner_tolerance=-1e-3),
           Transient(dt=1e-3, scheme=0, inner_iterations=1, inner_tolerance=float("nan")),
           Transient(dt=1e-3, scheme=0, reserved0=1, inner_iterations=1)]
    def make(on, poke):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        s.set_fields(*fields)
        if on:
            s.set_transient(good)
            s.set_time_levels(*fields[:3])
        if poke:
            if not on:
                assert s.advance(1, raise_on_error=False) == BAD_ARGUMENT
                assert s.set_time_levels(*fields[:3], raise_on_error=False) == BAD_ARGUMENT
            for t in bad:
                assert s.set_transient(t, raise_on_error=False) == BAD_ARGUMENT, (t.dt, t.scheme, t.inner_iterations, t.inner_tolerance)
        return s

    # an assembly moves the state on (Rhie-Chow reads the diagonals it wrote), so the unchanged state is checked against a
    # solver brought to the same point without the rejected calls: the first assemblies of the two agree bit for bit
    for on in (False, True):
        got, want = make(on, True).assemble_momentum(), make(on, False).assemble_momentum()
        for x, y in zip(got[:6], want[:6]):
            assert np.array_equal(x, y)
    s = Solver(m, settings(momentum=5, frozen_diagonals=0), 1000.0, 1e-3)
    assert s.set_transient(good, raise_on_error=False) == BAD_ARGUMENT


def test_solve_transient_matches_the_solver_object(gpu):
    from orc_amd.solver import Solver, solve_transient
    a, m = channel_flow()
    kw = dict(momentum=1, solver_type=BICGSTAB)
    t = transient(0.02, 1, 4)
    f = [x.copy() for x in poiseuille_start(a)]
    reports = []
    solve_transient(m, *f, settings(**kw), 1000.0, 1e-3, t, 5, reporting_interval=1, report=lambda *r: reports.append(r))
    s = Solver(m, settings(**kw), 1000.0, 1e-3)
    s.set_fields(*poiseuille_start(a))
    s.set_transient(t)
    rep = s.advance(5, report=True)
    for x, y in zip(f, s.get_fields()):
        assert np.array_equal(x, y)
    assert [r[0] for r in reports] == [1, 2, 3, 4, 5]
    assert [r[1][0] for r in reports] == list(rep[:, 0])


# ------------------------------------------------------------------ 8. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "transient_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "TRANSIENT_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
