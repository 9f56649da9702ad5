"""Residual monitors on the device (orc_solver_set_monitors and its companions) against the numpy restatement
(tests/residual_restatement.py): the momentum residuals and the mass imbalance of an iteration, the host slots, read-only and
repeatable, the stopping rule, argument checking, the transient arm and two ranks on one GPU.

The per-row residuals of the restatement are the kernel's bit for bit (same order, separate multiply and add), so the maxima are
compared as uint64; a sum of n non-negative terms in any association lies within n EPS sum(term) of the exact one, a sum of
squares within (n + 1) EPS sum(term) (residual_restatement.py): those are the bounds, nothing measured."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import residual_restatement as R
from conftest import MESHES, ROOT, splitmix64_uniform
from test_gpu_surface import channel_solver, hex_case, mixed_case, seeded_fields

pytestmark = pytest.mark.gpu

BICGSTAB, MULTIGRID = 3, 2
UD, CD1, TVD_UMIST = 0, 1, 5
BAD_ARGUMENT = 10
RHO, MU = 1.3, 2e-3
F64 = C.POINTER(C.c_double)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def case(name, tmp_path):
    if name == "hex":
        return hex_case(13, 7, 5)       # 455 rows: two workgroups, a last slice of 7 live rows
    if name == "hex_rcm":
        return hex_case(13, 7, 5, ordering=1)
    if name == "hex211":
        return hex_case(2, 1, 1)        # two rows, one slice
    return mixed_case(tmp_path, polyhedra=(name == "poly"))  # rows of different length within a slice


def monitored_first_iteration(a, m, momentum):
    """(solver, first record, A_u/v/w, b_u/v/w, u/v/w in the mesh's internal order) of seeded fields"""
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    s = Solver(m, NumericalSettings.default(solver_type=BICGSTAB, momentum=momentum), RHO, MU)
    f = seeded_fields(a)
    s.set_fields(*f)
    s.snapshot()
    au, av, aw, bu, bv, bw, _ = s.assemble_momentum()
    s.restore()
    s.set_monitors()
    s.iterate(1)
    h = s.residual_history()
    assert h.shape == (1, R.N)
    g = m.cell_order()
    return s, h[0], (au, av, aw), (bu, bv, bw), [x[g] for x in f[:3]]


def check_sums(rec, want, bound, slots):
    for k in slots:
        print("slot %2d: device %.17g restatement %.17g |diff| %.3e bound %.3e" % (k, rec[k], want[k], abs(rec[k] - want[k]), bound[k]))
        assert np.isfinite(rec[k]) and abs(rec[k] - want[k]) <= bound[k], k


# ------------------------------------------------------------------ 1. momentum residuals against the restatement
@pytest.mark.parametrize("momentum", [UD, TVD_UMIST], ids=["ud", "tvd_umist"])
@pytest.mark.parametrize("mesh_name", ["hex", "hex_rcm", "hex211", "mixed", "poly"])
def test_momentum_residuals_equal_the_restatement(gpu, tmp_path, mesh_name, momentum):
    a, m = case(mesh_name, tmp_path)
    s, rec, A, b, x = monitored_first_iteration(a, m, momentum)
    pattern = m.matrix_pattern()
    if mesh_name in ("mixed", "poly"):
        lens = np.diff(pattern[0])
        assert len(set(lens[:64])) > 1 or len(set(lens)) > 2  # ragged inside a slice
    if momentum == TVD_UMIST and mesh_name == "hex":
        assert not np.array_equal(A[0], A[1]) or not np.array_equal(A[0], A[2])  # the limiter differs by component: three value streams
    systems = [R.momentum(A[k], b[k], x[k], pattern) for k in range(3)]
    want, bound = R.momentum_slots(systems)
    assert np.array_equal(bits(rec[R.MAX:R.MAX + 3]), bits(want[R.MAX:R.MAX + 3])), (rec[R.MAX:R.MAX + 3], want[R.MAX:R.MAX + 3])
    check_sums(rec, want, bound, range(R.L1, R.MAX))
    assert np.all(rec[R.L1:R.MAX + 3] > 0.0)  # a kernel that writes zeros fails
    for k in range(3):                        # slots 16..18: the stated quotient of the recorded doubles
        assert bits(rec[R.SCALED + k]) == bits(rec[R.L1 + k] / rec[R.SCALE + k])


# ------------------------------------------------------------------ 2. continuity
@pytest.mark.parametrize("mesh_name", ["hex", "hex_rcm", "poly"])
def test_mass_imbalance_and_host_slots(gpu, tmp_path, mesh_name):
    a, m = case(mesh_name, tmp_path)
    s, rec, _, _, _ = monitored_first_iteration(a, m, UD)
    want, bound = R.continuity_slots(s.pressure_rhs())
    assert bits(rec[R.C_MAX]) == bits(want[R.C_MAX])
    check_sums(rec, want, bound, (R.C_L1, R.C_SQ))
    assert rec[R.C_L1] > 0.0 and rec[R.C_SQ] > 0.0 and rec[R.C_MAX] > 0.0
    for _ in range(6):
        s.iterate(1)
        w2, b2 = R.continuity_slots(s.pressure_rhs())
        last = s.residual_history(first=s.residual_history().shape[0] - 1)[0]
        assert bits(last[R.C_MAX]) == bits(w2[R.C_MAX]) and abs(last[R.C_L1] - w2[R.C_L1]) <= b2[R.C_L1]
    h = s.residual_history()
    assert h.shape == (7, R.N)
    assert np.array_equal(bits(h[:, R.C_SCALE]), bits(np.concatenate([np.maximum.accumulate(h[:5, R.C_L1]), np.full(2, h[:5, R.C_L1].max())])))
    assert np.array_equal(bits(h[:, R.C_SCALED]), bits(h[:, R.C_L1] / h[:, R.C_SCALE]))
    assert np.array_equal(bits(h), bits(R.finish(h)))
    assert np.array_equal(bits(s.residual_history(first=2, count=3)), bits(h[2:5]))


# ------------------------------------------------------------------ 3. read-only and repeatable
def test_monitoring_changes_no_bit_and_repeats(gpu):
    from orc_amd._lib import lib
    a, m, s = channel_solver()
    s.snapshot()
    rep_off = s.iterate(3, report=True)[1]
    f_off = s.get_fields()
    assert s.residual_history().shape == (0, R.N)
    s.restore()
    s.set_monitors()
    rep_on = s.iterate(3, report=True)[1]
    f_on = s.get_fields()
    for x, y in zip(f_off, f_on):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(rep_off), bits(rep_on))
    h1 = s.residual_history()
    assert h1.shape == (3, R.N) and np.all(np.isfinite(h1)) and np.all(h1[:, :R.C_SCALE] > 0.0)
    s.restore()  # neither snapshot nor restore touch the history
    assert np.array_equal(bits(s.residual_history()), bits(h1))
    s.set_monitors()  # clears it
    assert s.residual_history().shape == (0, R.N)
    s.iterate(3)
    assert np.array_equal(bits(s.residual_history()), bits(h1))
    # guard words behind the output
    buf = np.full(3 * R.N + 8, -7.25)
    assert lib().orc_solver_residual_history(s.ptr, 1, 2, buf.ctypes.data_as(F64)) == 0
    assert np.array_equal(bits(buf[:2 * R.N]), bits(h1[1:].ravel())) and np.all(buf[2 * R.N:] == -7.25)
    # switching off: later iterations record nothing and keep their bits
    s.set_monitors(False)
    s.restore()
    s.iterate(3)
    assert s.residual_history().shape == (0, R.N)
    for x, y in zip(f_off, s.get_fields()):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------ 4. the stopping rule, no tolerance fixed in advance
# The 8 x 8 x 1 Couette fixture with the settings of tests/golden/make_golden_couette_multigrid.py (CD1, Multigrid + Jacobi, 50 smoother
# iterations, moving top wall, its start fields).  COUETTE_N and the pressure relaxation: DESIGN.md §3 "Residual monitors" has the
# measured history they were chosen from.
COUETTE_N = 20
COUETTE_PRESSURE_RELAXATION = 0.3


def couette_solver():
    import helpers as H
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays, set_channel_bcs
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    a = set_channel_bcs(MeshArrays(orc_io.read_mesh(os.path.join(MESHES, "couette_flow_8x8x1.msh")).arrays()), top_wall_velocity=5e-4, dp_dx=10.0)
    m = Mesh(a)
    cc = np.asarray(a["cell_centroid"])
    n = len(cc)
    ua = H.analytical_poiseuille(cc[:, 1], dp_dx=10.0, u_top=5e-4)
    start = (ua * (1 + 0.02 * splitmix64_uniform(n, 1)), 1e-7 * splitmix64_uniform(n, 2), 1e-12 * splitmix64_uniform(n, 3),
             -0.02 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4)))
    s = Solver(m, NumericalSettings.default(momentum=CD1, solver_type=MULTIGRID, iterations=50,
                                            pressure_relaxation=COUETTE_PRESSURE_RELAXATION), 1000.0, 1e-3)
    s.set_fields(*start)
    return a, m, s


def first_passing(scaled, tol, start):
    for i in range(start, len(scaled)):
        if np.all(scaled[i] <= tol):
            return i
    return None


def test_iterate_until_stops_where_the_history_says(gpu):
    from orc_amd.settings import Convergence
    N = COUETTE_N
    a, m, s = couette_solver()
    s.snapshot()
    s.set_monitors()
    s.iterate(N)
    h = s.residual_history()
    scaled = h[:, R.SCALED:R.SCALED + 4]
    for i in range(N):
        print("it %3d scaled u %.6e v %.6e w %.6e continuity %.6e" % (i, *scaled[i]))
    assert np.all(np.isfinite(h))
    j = next((i for i in range(5, N) if np.all(scaled[i] < scaled[:i].min(axis=0))), None)
    assert j is not None and j < N - 1, j
    tol = np.sqrt(scaled[j] * scaled[:j].min(axis=0))
    print("j = %d, tolerances %s" % (j, tol))
    c = Convergence.make(momentum=tol[:3], continuity=tol[3])
    s.restore()
    s.set_monitors()
    st, done, conv, rep = s.iterate_until(N, c, report=True)
    assert (st, done, conv) == (0, j + 1, True)
    f_until = s.get_fields()
    assert np.array_equal(bits(s.residual_history()), bits(h[:j + 1]))
    s.restore()
    s.set_monitors()
    rep_fixed = s.iterate(j + 1, report=True)[1]
    for x, y in zip(f_until, s.get_fields()):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(rep), bits(rep_fixed[-1]))
    # all tolerances 0: the whole budget, not converged
    s.restore()
    s.set_monitors()
    assert s.iterate_until(N, Convergence.make(momentum=0.0, continuity=0.0)) == (0, N, False)
    assert np.array_equal(bits(s.residual_history()), bits(h))
    # min_iterations: no check before it
    s.restore()
    s.set_monitors()
    c.min_iterations = j + 3
    i = first_passing(scaled, tol, j + 2)
    assert s.iterate_until(N, c) == ((0, i + 1, True) if i is not None else (0, N, False))
    assert s.residual_history().shape[0] >= j + 3
    # a budget of 0 iterations runs none
    assert s.iterate_until(0, c) == (0, 0, False)


def test_solve_steady_converged_equals_iterate_until(gpu):
    from orc_amd.settings import Convergence, NumericalSettings
    from orc_amd.solver import solve_steady, solve_steady_converged
    a, m, s = couette_solver()
    start = s.get_fields()
    s.set_monitors()
    s.iterate(8)
    h = s.residual_history()
    tol = h[5, R.SCALED:R.SCALED + 4]  # met by record 5 (<=); whether an earlier one meets it too is read from the history
    i = first_passing(h[:, R.SCALED:R.SCALED + 4], tol, 0)
    settings = NumericalSettings.default(momentum=CD1, solver_type=MULTIGRID, iterations=50, pressure_relaxation=COUETTE_PRESSURE_RELAXATION)
    f = [x.copy() for x in start]
    st, done, conv, rec = solve_steady_converged(m, *f, settings, 1000.0, 1e-3, Convergence.make(momentum=tol[:3], continuity=tol[3]), 8)
    assert (st, done, conv) == (0, i + 1, True)
    assert np.array_equal(bits(rec), bits(h[i]))
    g = [x.copy() for x in start]
    solve_steady(m, *g, settings, 1000.0, 1e-3, i + 1)
    for x, y in zip(f, g):
        assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------ 5. arguments
def test_bad_arguments_leave_the_solver_unchanged(gpu):
    from orc_amd._lib import lib
    from orc_amd.settings import Convergence
    L = lib()
    a, m, s = channel_solver()
    s.snapshot()
    s.iterate(1)
    want = s.get_fields()
    s.restore()
    good = Convergence.make(1.0, 1.0)
    done, conv = C.c_uint64(99), C.c_int32(99)
    assert s.iterate_until(3, good, raise_on_error=False)[0] == BAD_ARGUMENT  # monitoring is off
    s.set_monitors()
    bad = [Convergence.make(momentum=(1.0, -1e-9, 1.0)), Convergence.make(momentum=(1.0, 1.0, float("nan"))),
           Convergence.make(continuity=-1.0), Convergence.make(continuity=float("nan"))]
    r0 = Convergence.make()
    r0.reserved0 = 3
    for c in bad + [r0]:
        assert L.orc_solver_iterate_until(s.ptr, 3, C.byref(c), None, C.byref(done), C.byref(conv)) == BAD_ARGUMENT
    assert L.orc_solver_iterate_until(s.ptr, 3, None, None, C.byref(done), C.byref(conv)) == BAD_ARGUMENT
    assert L.orc_solver_iterate_until(None, 3, C.byref(good), None, C.byref(done), C.byref(conv)) == BAD_ARGUMENT
    assert (done.value, conv.value) == (99, 99)
    assert L.orc_solver_set_monitors(None, 1) == BAD_ARGUMENT
    assert L.orc_solver_get_pressure_rhs(s.ptr, None) == BAD_ARGUMENT and L.orc_solver_get_pressure_rhs(None, None) == BAD_ARGUMENT
    out = np.full(2 * R.N, -7.25)
    assert s.residual_history().shape == (0, R.N)
    assert L.orc_solver_residual_history(s.ptr, 0, 1, out.ctypes.data_as(F64)) == BAD_ARGUMENT  # nothing recorded yet
    s.iterate(1)
    for x, y in zip(want, s.get_fields()):  # the next iteration's bits are the same
        assert np.array_equal(bits(x), bits(y))
    assert L.orc_solver_residual_history(s.ptr, 0, 2, out.ctypes.data_as(F64)) == BAD_ARGUMENT
    assert L.orc_solver_residual_history(s.ptr, 1, 1, out.ctypes.data_as(F64)) == BAD_ARGUMENT
    assert L.orc_solver_residual_history(s.ptr, 2 ** 63, 2 ** 63, out.ctypes.data_as(F64)) == BAD_ARGUMENT
    assert L.orc_solver_residual_history(s.ptr, 0, 1, None) == BAD_ARGUMENT
    assert L.orc_solver_residual_history(None, 0, 1, out.ctypes.data_as(F64)) == BAD_ARGUMENT
    assert np.all(out == -7.25)
    assert L.orc_solver_residual_history(s.ptr, 1, 0, None) == 0  # an empty range at the end is a range
    assert s.residual_history().shape == (1, R.N)


# ------------------------------------------------------------------ 6. transient
def test_advance_records_every_inner_iteration(gpu):
    from orc_amd.settings import Transient
    a, m, s = channel_solver()
    s.set_transient(Transient.make(1e-3, 0, 4, 0.5))
    s.snapshot()
    rep_off = s.advance(2, report=True)
    f_off = s.get_fields()
    s.restore()
    s.set_monitors()
    rep = s.advance(2, report=True)
    used = int(rep[:, 8].sum())
    assert 2 <= used <= 8 and s.residual_history().shape == (used, R.N)
    assert np.array_equal(bits(rep), bits(rep_off))  # its own stopping rule is unchanged
    for x, y in zip(f_off, s.get_fields()):
        assert np.array_equal(bits(x), bits(y))
    assert np.all(np.isfinite(s.residual_history()))


# ------------------------------------------------------------------ 7. two ranks
def test_two_ranks_on_one_gpu_hold_the_same_records(gpu, tmp_path):
    import socket
    import residuals_mp_worker as W
    from orc_amd.mesh import Mesh
    from orc_amd.solver import Solver
    ag = W.whole_mesh_arrays()
    s = Solver(Mesh(ag), W.settings(), W.RHO, W.MU)  # the single-rank record of the same state
    s.set_fields(*W.fields(ag.n_cells))
    s.set_monitors()
    s.iterate(1)
    single = str(tmp_path / "single.npy")
    np.save(single, s.residual_history())
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "residuals_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1", ORC_TEST_RESIDUALS_SINGLE=single))
    print(r.stdout[-3000:])
    assert "RESIDUALS_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
