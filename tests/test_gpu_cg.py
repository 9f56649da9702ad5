"""The CG arm (ORC_SOLVER_CG, extension; orc_amd/csrc/cg.hip) on the device against its numpy restatement
(tests/cg_restatement.py) over the case table of tests/cg_cases.py, and the pressure-correction solver override
(orc_solver_set_pressure_solver) in solve_steady, the transient arm, the scalar arm and a partitioned run.

Iterates: the reference is the longdouble restatement, the bound 50 d_case, d_case being the rounding scale of the case
measured from the references alone (tests/test_cg_cpu.py holds it under 1e-10 for every case): the device's tree association
is a third float64 association beside the two d_case is taken from.  A pre-scaled view (CG nested inside another arm) is
refused by cg_dev with ORC_ERR_BAD_ARGUMENT but cannot be reached from the public surface, so no test drives it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import cg_cases as G
import cg_restatement as R
import helpers as H
from conftest import ROOT

pytestmark = pytest.mark.gpu
JACOBI_ARM, MULTIGRID, BICGSTAB, GMRES, CG = 1, 2, 3, 19, 20
NONE, JACOBI = 0, 1
BAD_ARGUMENT, STRUCTURAL_ZERO = 10, 6


def device_solve(a, b, iters, precond, threshold=0.0, x0=None):
    from orc_amd.linear_algebra import iterative_solve, last_cg_stats
    x = np.zeros(a.shape[0]) if x0 is None else x0.copy()
    st = iterative_solve(a, b, x, iters, CG, 0.5, threshold, precond, raise_on_error=False)
    return st, x, last_cg_stats()


def check_x(label, x, x_ref, d_case):
    err = G.rel(x, x_ref)
    print("%s: device error %.3e, d_case %.3e, ratio %.2f" % (label, err, d_case, err / d_case))
    assert err <= 50 * d_case, (label, err, d_case)


def check_stats(stats, sr, d_res=None):
    """iterations, event, beta0 and the final |r| against a restatement's, the residuals to 1e-10 relative.  d_res: given only for
    the cases of cg_cases.RESIDUAL_AT_ROUNDING, whose float64 references do not determine |r| themselves (cg_cases' docstring)"""
    its, beta0, res, event = stats
    assert (its, event) == (sr["iterations"], sr["event"]), (stats, sr["iterations"], sr["event"])
    assert abs(beta0 - float(sr["beta0"])) <= 1e-10 * float(sr["beta0"]), (beta0, sr["beta0"])
    ref = float(sr["residual"])
    print("|r|: device %.6e, restatement %.6e, relative difference %.3e, d_res %s" % (res, ref, abs(res - ref) / ref if ref else 0.0, d_res))
    allowance = 0.0 if d_res is None else 50 * max(d_res, 1e-15 * float(sr["beta0"]))
    assert abs(res - ref) <= 1e-10 * ref + allowance, (res, ref, d_res)


# ------------------------------------------------------------------ 1. iterates
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_iterates(gpu, c):
    a, b = G.system(c.family, c.n)
    x0 = G.start_vector(c)
    st, x, stats = device_solve(a, b, c.iterations, c.precond, x0=x0)
    assert st == 0
    if c.n in G.LARGE_SIZES:
        x_ref = np.zeros(c.n) if x0 is None else x0.copy()
        sr = R.cg(a, b, x_ref, c.iterations, c.precond)
        d_case, d_res = G.large_case_d(c), None
    else:
        r = G.case_references(c)
        x_ref, sr, d_case = r["x_ld"], r["st_ld"], r["d_case"]
        d_res = r["d_res"] if G.case_id(c) in G.RESIDUAL_AT_ROUNDING else None
    check_stats(stats, sr, d_res)
    check_x(G.case_id(c), x, x_ref, d_case)


@pytest.mark.parametrize("c", G.PAST_END_CASES, ids=G.case_id)
def test_more_iterations_than_unknowns(gpu, c):
    """CG is through after n iterations; what follows works on rounding noise, or meets p.q = 0 of a vanished direction (event 1).
    The bound on x: the direct solution's own rounding, eps * condition (< 10 here) * iterations (<= 50) < 1e-13, with margin."""
    a, b = G.system(c.family, c.n)
    st, x, (its, beta0, res, event) = device_solve(a, b, c.iterations, c.precond, x0=G.start_vector(c))
    assert st == 0 and event in (0, 1) and c.n <= its <= c.iterations, (st, its, event)
    ref = np.linalg.solve(a.toarray(), b)
    assert np.isfinite(x).all() and np.isfinite(res) and np.linalg.norm(x - ref) <= 1e-10 * np.linalg.norm(ref), (x, ref)


# ------------------------------------------------------------------ 2. stops and events
@pytest.mark.parametrize("t", G.THRESHOLD_CASES, ids=lambda t: "%s-%s" % (t.family, t.where))
def test_threshold_stops_at_the_restatements_iteration(gpu, t):
    a, b = G.system(t.family, t.n)
    thr, k = G.threshold_of(t)
    r = G.threshold_references(t)
    assert r["st_ld"]["iterations"] == k
    st, x, stats = device_solve(a, b, t.iterations, t.precond, threshold=thr)
    assert st == 0
    check_stats(stats, r["st_ld"])
    check_x("%s %s" % (t.family, t.where), x, r["x_ld"], r["d_case"])


@pytest.mark.parametrize("t", G.EVENT_CASES, ids=lambda t: "%s-n%d" % t)
def test_events(gpu, t):
    a, b, x0, precond = G.event_system(t)
    r = G.event_references(t)
    st, x, (its, beta0, res, event) = device_solve(a, b, G.EVENT_ITERATIONS, precond, x0=x0)
    assert st == 0
    sr = r["st_ld"]
    assert (its, event) == (sr["iterations"], sr["event"]), (its, event, sr["iterations"], sr["event"])
    if t.name == "zero_rhs":
        assert not x.any() and beta0 == 0.0 and res == 0.0
    elif t.name == "solved_start":
        # r0 is rounding noise, of which every association has its own: beta0 is compared in size only
        assert 0 <= beta0 <= 1e-12 * np.linalg.norm(b)
        check_x("solved start", x, r["x_ld"], r["d_case"])
    else:
        assert abs(beta0 - float(sr["beta0"])) <= 1e-10 * float(sr["beta0"])
        check_x("indefinite n=%d" % t.n, x, r["x_ld"], r["d_case"])


def test_edge_rules(gpu):
    from orc_amd.linear_algebra import iterative_solve
    a, b = G.system("lap1", 129)
    x0 = np.full(129, 0.25)
    # beta0 = 0 leaves x untouched, which differs from zeroed: a diagonal matrix of powers of two and a dyadic start, b = A x0
    # without rounding on the host or the device, r0 = 0 exactly
    ad = sp.diags(2.0 ** (np.arange(129) % 5 - 2), format="csr")
    xd = 0.25 * (np.arange(129) % 7 + 1)
    for precond in (NONE, JACOBI):
        st, x, (its, beta0, res, event) = device_solve(ad, ad @ xd, 5, precond, x0=xd)
        assert st == 0 and np.array_equal(x, xd) and (its, event, beta0, res) == (0, 0, 0.0, 0.0)
    # iterations = 0: what the other extension arm does today — ORC_OK, x untouched
    xg, xc = x0.copy(), x0.copy()
    st_g = iterative_solve(a, b, xg, 0, GMRES, 0.5, 0.0, JACOBI, raise_on_error=False)
    st_c = iterative_solve(a, b, xc, 0, CG, 0.5, 0.0, JACOBI, raise_on_error=False)
    assert st_c == st_g == 0 and np.array_equal(xc, xg) and np.array_equal(xc, x0)
    # a non-finite right-hand side: event 2 before anything is written
    bn = b.copy()
    bn[7] = np.nan
    st, x, (its, _, _, event) = device_solve(a, bn, 5, JACOBI, x0=x0)
    assert st == 0 and (its, event) == (0, 2) and np.array_equal(x, x0)
    # unknown preconditioner
    st, x, _ = device_solve(a, b, 5, 7, x0=x0)
    assert st == BAD_ARGUMENT and np.array_equal(x, x0)
    # a zero diagonal entry under the Jacobi preconditioner; without it the same matrix is solved (and meets p.q <= 0 or not)
    az = a.copy()
    az.data[az.indptr[40] + 1] = 0.0  # row 40: columns 39, 40, 41
    assert az[40, 40] == 0.0
    st, x, _ = device_solve(az, b, 5, JACOBI, x0=x0)
    assert st == STRUCTURAL_ZERO and np.array_equal(x, x0)
    st, x, _ = device_solve(az, b, 5, NONE, x0=x0)
    assert st == 0 and np.isfinite(x).all()


# ------------------------------------------------------------------ 3. the preconditioner keeps the operator symmetric
def test_jacobi_is_applied_inside_the_recurrence_not_as_a_left_scaling(gpu):
    a, b = G.system("p", 1008)
    al, bl = R.left_scaled(a, b)
    for k in (3, 7):
        st, x, _ = device_solve(a, b, k, JACOBI)
        assert st == 0
        xl = np.zeros(1008, G.LD)
        R.cg(a, b, xl, k, 1, dtype=G.LD)
        x64, xc = np.zeros(1008), np.zeros(1008)
        R.cg(a, b, x64, k, 1)
        R.cg(a, b, xc, k, 1, chunk=128)
        d_case = max(G.rel(x64, xl), G.rel(xc, xl), 1e-15)
        check_x("PCG, M = D, k = %d" % k, x, xl, d_case)
        xs = np.zeros(1008)
        R.cg(al, bl, xs, k, 0)
        far = G.rel(x, xs.astype(G.LD))
        print("k = %d: distance from CG on the left-scaled system %.3e" % (k, far))
        assert far > 1e-3 and far > 1e6 * 50 * d_case


# ------------------------------------------------------------------ 4. reproducible, and as good as the restatement at size
def test_bit_reproducible_and_reduces_the_midsize_residual(gpu):
    import test_gpu_gmres as TG
    a, b = TG.midsize_pressure_system()
    assert G.is_bit_symmetric(a)
    st1, x1, s1 = device_solve(a, b, 50, JACOBI)
    st2, x2, s2 = device_solve(a, b, 50, JACOBI)
    assert st1 == 0 and st2 == 0 and s1[0] == 50 and s1[3] == 0
    assert np.array_equal(x1, x2) and s1 == s2
    xr = np.zeros(a.shape[0])
    R.cg(a, b, xr, 50, 1)
    dev, ref = np.linalg.norm(b - a @ x1), np.linalg.norm(b - a @ xr)
    print("midsize p': |b - A x| / |b| after 50 iterations: device %.3e, restatement %.3e" % (dev / np.linalg.norm(b), ref / np.linalg.norm(b)))
    assert dev <= 10 * ref and ref < np.linalg.norm(b)


# ------------------------------------------------------------------ 5. the p' override in solve_steady
def couette_8x8(oracle, mesh_path):
    from orc_amd.mesh import Mesh, MeshArrays
    om = oracle.Mesh.read(mesh_path("couette_flow_8x8x1"))
    H.channel_bcs(om)
    a = MeshArrays(om.arrays())
    return a, Mesh(a)


# relaxations at which SIMPLE on this mesh converges in 200 iterations (the oracle with BiCGSTAB: velocity correction 1.7e-11 of
# |u| = 4e-3 at iteration 200; the reference's defaults 0.01 / 0.5 are at 6e-5 after 600)
STEADY_KW = dict(momentum=1, solver_type=BICGSTAB, iterations=50, frozen_diagonals=1, pressure_relaxation=0.3, momentum_relaxation=0.7)


def steady_run(a, m, iterations, prepare=None, **kw):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    s = Solver(m, NumericalSettings.default(**dict(STEADY_KW, **kw)), 1000.0, 1e-3)
    if prepare:
        prepare(s)
    s.set_fields(*H.seeded_fields(a, seed=2, w_zero=True))
    st, rep = s.iterate(iterations, report=True, raise_on_error=False)
    assert st == 0
    return s, s.get_fields(), rep


def test_override_unset_cleared_or_equal_to_the_settings_changes_no_bit(gpu, oracle, mesh_path):
    a, m = couette_8x8(oracle, mesh_path)
    _, plain, _ = steady_run(a, m, 3)

    def set_and_clear(s):
        s.set_pressure_solver(CG, JACOBI, 200, 1e-12)
        assert s.pressure_solver()[0]
        s.set_pressure_solver(None)
        assert not s.pressure_solver()[0]

    _, cleared, _ = steady_run(a, m, 3, set_and_clear)
    # (b) the settings' own five fields as the override: the plumbing by itself changes nothing
    _, same, _ = steady_run(a, m, 3, lambda s: s.set_pressure_solver(BICGSTAB, JACOBI, 50, 1e-3, 0.5))
    for f, g, h in zip(plain, cleared, same):
        assert np.array_equal(f, g) and np.array_equal(f, h)
    assert any(np.abs(f).max() > 0 for f in plain)


def test_override_cg_converges_to_the_same_fixed_point(gpu, oracle, mesh_path):
    from orc_amd.linear_algebra import last_cg_stats
    a, m = couette_8x8(oracle, mesh_path)
    _, ref, rep0 = steady_run(a, m, 200)
    s, got, rep1 = steady_run(a, m, 200, lambda s: s.set_pressure_solver(CG, JACOBI, 200, 1e-12))
    its, beta0, res, event = last_cg_stats()
    print("last p' solve: %d CG iterations, |r| %.3e -> %.3e, event %d; velocity corrections %.3e / %.3e" % (its, beta0, res, event, rep0[-1][6], rep1[-1][6]))
    assert 0 < its <= 200 and event == 0 and res <= 1e-12 * beta0
    un = np.linalg.norm(ref[0])
    assert rep0[-1][6] <= 1e-7 * un and rep1[-1][6] <= 1e-7 * un  # both runs are converged
    assert H.rel_l2(got[0], ref[0]) < 1e-6 and H.rel_l2(got[3], ref[3]) < 1e-6, (H.rel_l2(got[0], ref[0]), H.rel_l2(got[3], ref[3]))
    assert np.linalg.norm(got[1] - ref[1]) < 1e-6 * un and np.linalg.norm(got[2] - ref[2]) < 1e-6 * un


def test_override_cg_under_multigrid_momentum_builds_no_pressure_hierarchy(gpu, oracle, mesh_path):
    from orc_amd.linear_algebra import last_cg_stats
    a, m = couette_8x8(oracle, mesh_path)
    s, f, _ = steady_run(a, m, 3, solver_type=MULTIGRID)
    built = s.debug_pressure_hierarchies()
    assert built >= 3
    s, g, _ = steady_run(a, m, 3, lambda s: s.set_pressure_solver(CG, JACOBI, 200, 1e-12), solver_type=MULTIGRID)
    assert s.debug_pressure_hierarchies() == 0
    assert last_cg_stats()[0] > 0 and all(np.isfinite(x).all() for x in g)
    # and the override may itself name a Multigrid arm: the hierarchy is set up as without it
    s, h, _ = steady_run(a, m, 3, lambda s: s.set_pressure_solver(MULTIGRID, JACOBI, 50, 1e-3, 0.5), solver_type=MULTIGRID)
    assert s.debug_pressure_hierarchies() == built
    for x, y in zip(f, h):
        assert np.array_equal(x, y)


def test_override_round_trip_and_bad_fields(gpu, oracle, mesh_path):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    a, m = couette_8x8(oracle, mesh_path)
    s = Solver(m, NumericalSettings.default(**STEADY_KW), 1000.0, 1e-3)
    assert s.pressure_solver() == (False, dict(solver_type=BICGSTAB, preconditioner=JACOBI, iterations=50, threshold=1e-3, relaxation=0.5))
    s.set_pressure_solver(CG, NONE, 123, 1e-9, 0.75)
    want = (True, dict(solver_type=CG, preconditioner=NONE, iterations=123, threshold=1e-9, relaxation=0.75))
    assert s.pressure_solver() == want
    for bad in (dict(iterations=0), dict(threshold=-1e-3), dict(threshold=float("nan")), dict(solver_type=21), dict(solver_type=-1),
                dict(preconditioner=2), dict(relaxation=float("inf"))):
        kw = dict(dict(solver_type=CG, preconditioner=JACOBI, iterations=50, threshold=0.0, relaxation=0.5), **bad)
        assert s.set_pressure_solver(raise_on_error=False, **kw) == BAD_ARGUMENT, bad
        assert s.pressure_solver() == want  # a refusal leaves the solver unchanged
    s.snapshot()
    s.set_pressure_solver(None)
    s.restore()
    assert not s.pressure_solver()[0]  # snapshot / restore do not touch the override


# ------------------------------------------------------------------ 6. transient
def test_one_time_step_with_the_override_agrees_with_the_step_without(gpu):
    import test_gpu_transient as TT
    from orc_amd.solver import Solver
    a, m = TT.couette_mesh()
    nu = TT.MU / TT.RHO
    dt = 0.01 * TT.HGT ** 2 / nu
    out = []
    for override in (False, True):
        kw = dict(momentum=0, solver_type=BICGSTAB, iterations=500, relative_convergence_threshold=1e-13)
        s = Solver(m, TT.settings(**kw), TT.RHO, TT.MU)
        if override:
            s.set_pressure_solver(CG, JACOBI, 500, 1e-13)
        z = np.zeros(m.n_cells)
        s.set_fields(z, z, z, z)
        s.set_transient(TT.transient(dt, 0, 2))
        s.advance(1)
        out.append(s.get_fields())
    (u0, v0, w0, p0), (u1, v1, w1, p1) = out
    assert np.abs(u0).max() > 0
    assert H.rel_l2(u1, u0) <= 1e-8, H.rel_l2(u1, u0)
    for x, y in ((v0, v1), (w0, w1)):
        assert np.abs(x - y).max() <= 1e-8 * TT.U_TOP
    assert np.abs(p1 - p0).max() <= 1e-8 * TT.MU * TT.U_TOP / TT.HGT


# ------------------------------------------------------------------ 7. scalar
def test_pure_conduction_with_the_cg_arm(gpu):
    import scalar_restatement as SR
    import test_gpu_scalar as TS
    from orc_amd.linear_algebra import last_cg_stats
    a, m = TS.hex_mesh(2, 16, 2)  # every boundary zone a wall: no flow, the system is the symmetric Gamma part
    z = np.zeros(a.n_cells)
    s, _, _ = TS.make_solver(m, a, TS.scalar_settings(diffusivity=0.7, iterations=200, solver_type=CG, relative_convergence_threshold=1e-14),
                             {"BOTTOM_WALL": (SR.VALUE, 0.0), "TOP_WALL": (SR.VALUE, 1.0)}, (z, z, z, z))
    sa, _ = s.assemble_scalar()
    assert G.is_bit_symmetric(m.csr(sa))
    s.solve_scalar()
    phi = s.get_scalar_field()
    y = np.asarray(a["cell_centroid"])[:, 1]
    assert np.abs(phi - y / 0.001).max() <= 1e-9, np.abs(phi - y / 0.001).max()
    its, _, _, event = last_cg_stats()
    assert 0 < its < 200 and event == 0


# ------------------------------------------------------------------ 8. two ranks on one GPU
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "cg_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    print(r.stdout[-2000:])
    assert "CG_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
