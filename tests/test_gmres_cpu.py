"""The GMRES arm's restatement (tests/gmres_restatement.py) against scipy on the channel_flow systems, and its C ABI
(enum value, settings field, exported symbols, no CPU fallback).  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_restatement as R
from conftest import GOLDEN


def channel_systems():
    d = np.load(os.path.join(GOLDEN, "channel_flow.npz"))
    rp, col = d["row_ptr"], d["col"]
    n = len(rp) - 1
    out = {}
    for name, vals, rhs in (("u", d["a_uvw_frozen_it1"][0], d["b_uvw_frozen_it1"][0]), ("p", d["a_p_frozen"], d["b_p_frozen"])):
        out[name] = (sp.csr_matrix((vals, col, rp), shape=(n, n)), rhs.copy())
    return out


SYSTEMS = channel_systems()
CASES = [(name, jac) for name in ("u", "p") for jac in (False, True)]


def system(name, jac):
    a, b = SYSTEMS[name]
    if jac:
        a, b = R.jacobi_scaled(a, b)
    return a, b


@pytest.mark.parametrize("name,jac", CASES)
def test_unrestarted_restatement_is_a_direct_solve(name, jac):
    a, b = system(name, jac)
    n = a.shape[0]
    ref = spla.spsolve(a.tocsc(), b)
    # restart 64 is the longest cycle the arm takes: run to n steps (16 cycles), stopping once converged
    x = np.zeros(n)
    R.gmres(a, b, x, n, restart=64, threshold=1e-15)
    assert np.linalg.norm(x - ref) <= 1e-10 * np.linalg.norm(ref)


@pytest.mark.parametrize("name,jac", CASES)
def test_estimate_is_the_true_residual_and_never_increases(name, jac):
    a, b = system(name, jac)
    n = a.shape[0]
    for restart in (8, 30, 64):
        x = np.zeros(n)
        # replay step by step: the estimate after k steps of one cycle against |b - A x_k| of a solve stopped there
        st = R.gmres(a, b, x, restart, restart=restart, threshold=0.0)
        ests = st["estimates"][0]
        assert all(ests[i + 1] <= ests[i] * (1 + 1e-12) for i in range(len(ests) - 1))
        beta0 = st["beta0"]
        for k in (1, 3, restart // 2, restart):
            xk = np.zeros(n)
            sk = R.gmres(a, b, xk, k, restart=restart, threshold=0.0)
            true = np.linalg.norm(b - a @ xk)
            if true > 1e-8 * beta0:
                assert abs(sk["estimate"] - true) <= 1e-8 * true, (restart, k, sk["estimate"], true)


@pytest.mark.parametrize("name,jac", CASES)
def test_restarted_restatement_agrees_with_scipy_gmres(name, jac):
    a, b = system(name, jac)
    n = a.shape[0]
    restart = 30
    x = np.zeros(n)
    R.gmres(a, b, x, 30 * 200, restart=restart, threshold=1e-12)
    xs, info = spla.gmres(a, b, x0=np.zeros(n), restart=restart, maxiter=400, rtol=1e-12, atol=0.0)
    assert info == 0
    assert np.linalg.norm(b - a @ x) <= 1e-11 * np.linalg.norm(b)
    assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs)


def test_restatement_edge_rules():
    n = 50
    a = sp.identity(n, format="csr")
    b = np.arange(1.0, n + 1)
    x = np.zeros(n)
    st = R.gmres(a, b, x, 10, restart=8)
    assert st["steps"] == 1 and st["cycles"] == 1 and np.allclose(x, b, rtol=1e-15, atol=0)
    z = np.zeros(n)
    st = R.gmres(a, np.zeros(n), z, 10)
    assert st["steps"] == 0 and not z.any()
    bn = b.copy()
    bn[3] = np.nan
    x = np.ones(n)
    st = R.gmres(a, bn, x, 10, guard=True)
    assert st["event"] == 1 and np.all(x == 1.0)
    st = R.gmres(a, bn, x, 10, guard=False)
    assert np.isnan(x).all()


def test_gmres_abi():
    from orc_amd.settings import NumericalSettings, SolutionMethod
    import orc_amd
    assert SolutionMethod.GMRES == 19
    s = NumericalSettings.default()
    assert s.gmres_restart == 0 and C.sizeof(s) == 88
    lib = orc_amd._lib.lib()
    assert hasattr(lib, "orc_set_gmres_restart") and hasattr(lib, "orc_last_gmres_stats")
    from orc_amd.linear_algebra import last_gmres_stats, set_gmres_restart
    set_gmres_restart(12)
    set_gmres_restart(0)
    assert last_gmres_stats()[0] >= 0


def test_gmres_without_device_is_status_11():
    import orc_amd
    from orc_amd import OrcError
    from orc_amd.linear_algebra import iterative_solve
    from orc_amd.settings import SolutionMethod
    if orc_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(OrcError) as e:
        iterative_solve(sp.identity(4, format="csr"), np.ones(4), np.zeros(4), 5, SolutionMethod.GMRES, 0.5, 1e-6, 0)
    assert e.value.status == 11
