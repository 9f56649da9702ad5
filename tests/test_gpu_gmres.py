"""The GMRES arm (ORC_SOLVER_GMRES, extension) on the device against its numpy restatement (tests/gmres_restatement.py):
iterates after k steps, reported steps / cycles, convergence, edge rules, reproducibility, SIMPLE to convergence through
solve_steady's one-system-per-solve path, and a partitioned run over two ranks on one GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_restatement as R
import helpers as H
from conftest import GOLDEN, ROOT, splitmix64_uniform

pytestmark = pytest.mark.gpu
GMRES = 19


def channel_systems():
    d = np.load(os.path.join(GOLDEN, "channel_flow.npz"))
    rp, col = d["row_ptr"], d["col"]
    n = len(rp) - 1
    return {"u": (sp.csr_matrix((d["a_uvw_frozen_it1"][0], col, rp), shape=(n, n)), d["b_uvw_frozen_it1"][0].copy()),
            "p": (sp.csr_matrix((d["a_p_frozen"], col, rp), shape=(n, n)), d["b_p_frozen"].copy())}


_MIDSIZE = {}


def midsize_pressure_system():
    """the p' system of the 128 x 64 x 64 hex channel (the bench_midsize shape), assembled through the Solver API"""
    if "p" not in _MIDSIZE:
        from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
        from orc_amd.settings import NumericalSettings
        from orc_amd.solver import Solver
        a = set_channel_bcs(hex_channel(128, 64, 64))
        m = Mesh(a)
        s = Solver(m, NumericalSettings.default(momentum=5), 1000.0, 1e-3)
        s.set_fields(*H.rough_fields(np.asarray(a["cell_centroid"])))
        s.assemble_momentum()
        ap, bp = s.assemble_pressure()
        _MIDSIZE["p"] = (m.csr(ap), bp)
    return _MIDSIZE["p"]


def device_solve(a, b, iters, restart, precond, threshold=0.0, x0=None):
    from orc_amd.linear_algebra import iterative_solve, last_gmres_stats, set_gmres_restart
    set_gmres_restart(restart)
    x = np.zeros(a.shape[0]) if x0 is None else x0.copy()
    try:
        st = iterative_solve(a, b, x, iters, GMRES, 0.5, threshold, precond, raise_on_error=False)
    finally:
        set_gmres_restart(0)
    return st, x, last_gmres_stats()


def host_solve(a, b, iters, restart, precond, threshold=0.0, x0=None, guard=True):
    if precond:
        a, b = R.jacobi_scaled(a, b)
    x = np.zeros(a.shape[0]) if x0 is None else x0.copy()
    return x, R.gmres(a, b, x, iters, restart=restart, threshold=threshold, guard=guard)


@pytest.mark.parametrize("name", ["u", "p", "midsize_p"])
def test_iterates_agree_with_the_restatement(gpu, name):
    a, b = midsize_pressure_system() if name == "midsize_p" else channel_systems()[name]
    for restart in (8, 30):
        for precond in (0, 1):
            for k in (1, 5, restart, restart + 7):
                st, x, (steps, cycles, beta0, est) = device_solve(a, b, k, restart, precond)
                xr, sr = host_solve(a, b, k, restart, precond)
                assert st == 0
                err = np.linalg.norm(x - xr) / np.linalg.norm(xr)
                assert err <= (1e-9 if k > restart else 1e-10), (name, restart, precond, k, err)
                assert (steps, cycles) == (sr["steps"], sr["cycles"]), (name, restart, precond, k, steps, cycles, sr)
                assert abs(beta0 - sr["beta0"]) <= 1e-12 * sr["beta0"]


# the u system takes about 750 steps of GMRES(30) to 1e-10, the p' system about 140: "well past convergence" is 2000 / 500 steps.
# A restart forms b - A x explicitly, with the rounding of |A| |x|: on the u system that is about 1e-5 of a residual of 1e-10 |b|,
# so the estimate is held to 1e-6 there only on the p' system.
@pytest.mark.parametrize("name,past,est_tol", [("u", 2000, 1e-4), ("p", 500, 1e-6)])
def test_converges_and_stays_converged(gpu, name, past, est_tol):
    a, b = channel_systems()[name]
    for precond in (0, 1):
        aa, bb = R.jacobi_scaled(a, b) if precond else (a, b)
        st, x, (steps, cycles, beta0, est) = device_solve(a, b, 3000, 30, precond, threshold=1e-10)
        assert st == 0
        true = np.linalg.norm(bb - aa @ x)
        assert true <= 1e-9 * np.linalg.norm(bb), (name, precond, true)
        assert steps < 3000
        # the estimate of the last cycle is its true residual
        assert abs(est - true) <= est_tol * true, (est, true)
        # far past convergence with no stopping test: finite and still converged
        st, x, _ = device_solve(a, b, past, 30, precond, threshold=0.0)
        assert st == 0 and np.isfinite(x).all()
        assert np.linalg.norm(bb - aa @ x) <= 1e-10 * np.linalg.norm(bb)


def test_edge_rules(gpu):
    from orc_amd.linear_algebra import breakdown_guard_events, set_breakdown_guard
    a, b = channel_systems()["p"]
    n = a.shape[0]
    st, x, (steps, _, _, _) = device_solve(a, np.zeros(n), 10, 8, 1)
    assert st == 0 and not x.any() and steps == 0
    ident = sp.identity(n, format="csr")
    st, x, (steps, cycles, _, _) = device_solve(ident, b, 10, 8, 0)
    assert st == 0 and steps == 1 and cycles == 1 and np.isfinite(x).all()
    assert np.linalg.norm(x - b) <= 1e-14 * np.linalg.norm(b)
    st, x, _ = device_solve(a, b, 10, 65, 0)
    assert st == 10
    st, x, _ = device_solve(a, b, 10, -1, 0)
    assert st == 10
    bn = b.copy()
    bn[7] = np.nan
    set_breakdown_guard(True)
    breakdown_guard_events(reset=True)
    x0 = np.full(n, 0.25)
    st, x, _ = device_solve(a, bn, 10, 8, 1, x0=x0)
    assert st == 0 and np.array_equal(x, x0)
    assert breakdown_guard_events(reset=True) == 1
    set_breakdown_guard(False)
    try:
        st, x, _ = device_solve(a, bn, 10, 8, 1, x0=x0)
    finally:
        set_breakdown_guard(True)
    assert st == 0 and np.isnan(x).any()
    assert breakdown_guard_events(reset=True) == 0


def test_bit_reproducible(gpu):
    a, b = midsize_pressure_system()
    _, x1, s1 = device_solve(a, b, 45, 30, 1)
    _, x2, s2 = device_solve(a, b, 45, 30, 1)
    assert np.array_equal(x1, x2) and s1 == s2


def test_simple_with_gmres_converges_to_the_reference_fixed_point(gpu, oracle, mesh_path):
    """channel_flow.msh as in test_gpu_solve_steady's reference-mode test: the oracle runs BiCGSTAB in the reference's mode for
    1500 iterations, the device solve_steady with the GMRES arm (50 steps, default threshold).  Inexact inner solves leave the
    SIMPLE fixed point where it is."""
    from orc_amd.mesh import Mesh, MeshArrays
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    om = oracle.Mesh.read(mesh_path("channel_flow"))
    H.channel_bcs(om)
    a = MeshArrays(om.arrays())
    dm = Mesh(a)
    n = dm.n_cells
    cc = np.asarray(a["cell_centroid"])
    u0 = H.analytical_poiseuille(cc[:, 1]) * (1 + 0.02 * splitmix64_uniform(n, 1))
    v0 = 1e-7 * splitmix64_uniform(n, 2)
    w0 = 1e-12 * splitmix64_uniform(n, 3)
    p0 = -0.01 * (1 - cc[:, 0] / 0.002) * (1 + 0.01 * splitmix64_uniform(n, 4))
    uo, vo, wo, po_ = (x.copy() for x in (u0, v0, w0, p0))
    st, rep = oracle.solve_steady(om, uo, vo, wo, po_, oracle.default_settings(frozen_diagonals=0, momentum=1, solver_type=3, iterations=50),
                                  1000.0, 1e-3, 1500, report=True)
    assert st == 0 and rep[-1][4] < 1e-8
    s = Solver(dm, NumericalSettings.default(frozen_diagonals=1, momentum=1, solver_type=GMRES, iterations=50), 1000.0, 1e-3)
    s.set_fields(u0, v0, w0, p0)
    s.iterate(1500)
    u, v, w, p = s.get_fields()
    assert H.rel_l2(u, uo) < 1e-6 and H.rel_l2(p, po_) < 1e-6, (H.rel_l2(u, uo), H.rel_l2(p, po_))
    assert np.linalg.norm(v - vo) < 1e-6 * np.linalg.norm(uo) and np.linalg.norm(w - wo) < 1e-6 * np.linalg.norm(uo)


def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "gmres_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "GMRES_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
