"""The transient arm without a GPU: the OrcTransient layout from C and from ctypes, the exported entry points, and the numpy
restatement (tests/transient_restatement.py) the GPU tests compare against — its series solutions, its convergence to
them under refinement and its observed temporal order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import transient_restatement as R
from conftest import ROOT

NEW_SYMBOLS = ["orc_solver_set_transient", "orc_solver_set_time_levels", "orc_solver_advance", "orc_solve_transient"]


@pytest.fixture(scope="module")
def lib():
    import orc_amd
    if not os.path.exists(orc_amd._lib.LIB_PATH):
        orc_amd.build()
    return orc_amd._lib.lib()


def test_transient_struct_layout_matches_c(tmp_path):
    from orc_amd.settings import TimeScheme, Transient
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu %d %d", sizeof(OrcTransient), offsetof(OrcTransient, scheme), '
           'offsetof(OrcTransient, reserved0), offsetof(OrcTransient, inner_iterations), offsetof(OrcTransient, inner_tolerance), '
           '(int)ORC_TIME_EULER, (int)ORC_TIME_BDF2);return 0;}')
    exe = str(tmp_path / "sizeof_transient")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    size, o_scheme, o_res, o_inner, o_tol, euler, bdf2 = map(int, subprocess.check_output([exe]).split())
    assert size == C.sizeof(Transient) == 32
    assert (o_scheme, o_res, o_inner, o_tol) == (Transient.scheme.offset, Transient.reserved0.offset,
                                                 Transient.inner_iterations.offset, Transient.inner_tolerance.offset)
    assert (euler, bdf2) == (TimeScheme.Euler, TimeScheme.BDF2) == (0, 1)


def test_settings_struct_unchanged():
    from orc_amd.settings import NumericalSettings
    assert C.sizeof(NumericalSettings) == 88


def test_new_symbols_are_exported(lib):
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "orc_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr


def test_python_api_present():
    from orc_amd import solver
    for name in ("set_transient", "set_time_levels", "advance"):
        assert callable(getattr(solver.Solver, name))
    assert callable(solver.solve_transient)


def test_operator_is_the_fv_stencil():
    K, f = R.operator(4, 1.0, 2.0, u_top=3.0, body=0.5)
    c = 2.0 / 0.25 ** 2
    assert np.allclose(np.diag(K), c * np.array([3, 2, 2, 3]))
    assert np.allclose(np.diag(K, 1), -c) and np.allclose(K, K.T)
    assert np.allclose(f, [0.5, 0.5, 0.5, 0.5 + 2 * c * 3.0])
    # the steady state of the Couette operator is the linear profile through the wall values
    K, f = R.operator(16, 1e-3, 1e-6, u_top=2.0)
    y = R.centroids(16, 1e-3)
    assert np.allclose(np.linalg.solve(K, f), 2.0 * y / 1e-3, rtol=1e-12, atol=1e-14)


def test_semi_discrete_solution_solves_the_ode():
    K, f = R.operator(12, 1.0, 1.0, u_top=1.0, body=0.3)
    u0 = np.linspace(0, 1, 12) ** 2
    t, e = 0.05, 1e-6
    d = (R.semi_discrete(K, f, u0, t + e) - R.semi_discrete(K, f, u0, t - e)) / (2 * e)
    ut = R.semi_discrete(K, f, u0, t)
    assert np.allclose(d, -K @ ut + f, rtol=1e-6, atol=1e-8)
    assert np.allclose(R.semi_discrete(K, f, u0, 0.0), u0, atol=1e-14)


def test_series_solutions():
    h, nu, U = 1e-3, 1e-6, 0.5
    y = np.linspace(0, h, 41)
    assert np.allclose(R.couette_series(y, 1e9, h, nu, U), U * y / h, atol=1e-12)
    assert np.allclose(R.couette_series(y[1:33], 1e-9, h, nu, U), 0.0, atol=1e-3 * U)  # from rest (truncated series: away from the moving wall)
    mu, rho, G = 1e-3, 1000.0, 5.0
    steady = G / (2 * mu) * y * (h - y)
    assert np.allclose(R.poiseuille_series(y, 1e9, h, mu, rho, G), steady, atol=1e-15)
    assert np.allclose(R.poiseuille_series(y, 0.0, h, mu, rho, G), 0.0, atol=1e-6 * steady.max())
    # the series satisfies the PDE: u_t = nu u_yy + G / rho
    t, e, dy = 0.05, 1e-6, 1e-6
    yy = np.linspace(0.1 * h, 0.9 * h, 9)
    ut = (R.poiseuille_series(yy, t + e, h, mu, rho, G) - R.poiseuille_series(yy, t - e, h, mu, rho, G)) / (2 * e)
    uyy = (R.poiseuille_series(yy + dy, t, h, mu, rho, G) - 2 * R.poiseuille_series(yy, t, h, mu, rho, G)
           + R.poiseuille_series(yy - dy, t, h, mu, rho, G)) / dy ** 2
    assert np.allclose(ut, nu * uyy + G / rho, rtol=1e-4, atol=1e-6 * steady.max())


@pytest.mark.parametrize("scheme, lo, hi", [(R.EULER, 0.9, 1.1), (R.BDF2, 1.8, 2.2)])
def test_observed_temporal_order(scheme, lo, hi):
    """the step sizes and end time of tests/test_gpu_transient.py::test_temporal_order"""
    ny, h, nu, U = 32, 1e-3, 1.0, 1.0
    K, f = R.operator(ny, h, nu, u_top=U)
    T = 0.2 * h * h / nu
    exact = R.semi_discrete(K, f, np.zeros(ny), T)
    errs = []
    for steps in (20, 40, 80):
        u = R.march(K, f, np.zeros(ny), T / steps, steps, scheme)[-1]
        errs.append(np.linalg.norm(u - exact) / np.linalg.norm(exact))
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), order


def test_bdf2_with_two_given_levels_is_second_order_from_the_start():
    K, f = R.operator(16, 1.0, 1.0, u_top=1.0)
    u0 = R.semi_discrete(K, f, np.zeros(16), 0.02)
    errs = []
    for steps in (10, 20, 40):
        dt = 0.1 / steps
        um1 = R.semi_discrete(K, f, np.zeros(16), 0.02 - dt)
        u = R.march(K, f, u0, dt, steps, R.BDF2, u_prev=um1)[-1]
        errs.append(np.linalg.norm(u - R.semi_discrete(K, f, np.zeros(16), 0.12)))
    assert np.all(R.observed_order(errs) > 1.9)


@pytest.mark.parametrize("case", ["couette", "poiseuille"])
def test_discrete_model_converges_to_the_series(case):
    """refining space and time together, the restatement approaches the analytical series"""
    h, mu, rho = 1e-3, 1e-3, 1000.0
    nu = mu / rho
    t = 0.1 * h * h / nu
    errs = []
    for ny in (8, 16, 32, 64):
        y = R.centroids(ny, h)
        if case == "couette":
            K, f = R.operator(ny, h, nu, u_top=1.0)
            ref = R.couette_series(y, t, h, nu, 1.0)
        else:
            K, f = R.operator(ny, h, nu, body=5.0 / rho)
            ref = R.poiseuille_series(y, t, h, mu, rho, 5.0)
        steps = ny * ny // 8
        u = R.march(K, f, np.zeros(ny), t / steps, steps, R.BDF2)[-1]
        errs.append(np.linalg.norm(u - ref) / np.linalg.norm(ref))
    assert errs[-1] < 2e-3 and all(a > b for a, b in zip(errs, errs[1:])), errs
    assert np.all(R.observed_order(errs) > 1.5), errs
