"""The passive scalar arm without a GPU: the OrcScalarSettings layout from C and from ctypes, the exported entry points, the
Python API, and the numpy restatement (tests/scalar_restatement.py) the GPU tests compare against — its 1-D models against
the analytic solutions, and the observed spatial and temporal orders that fix the GPU tests' bands."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scalar_restatement as R
from conftest import ROOT

NEW_SYMBOLS = ["orc_scalar_settings_default", "orc_solver_set_scalar", "orc_solver_set_scalar_bc", "orc_solver_set_scalar_field",
               "orc_solver_get_scalar_field", "orc_solver_set_scalar_source", "orc_solver_set_scalar_levels",
               "orc_solver_solve_scalar", "orc_solver_last_scalar_report", "orc_solver_assemble_scalar",
               "orc_solver_scalar_boundary_flux"]
FIELDS = ["diffusivity", "scheme", "solver_type", "preconditioner", "reserved0", "iterations", "relative_convergence_threshold",
          "relaxation", "outer_iterations", "outer_tolerance"]


@pytest.fixture(scope="module")
def lib():
    import orc_amd
    if not os.path.exists(orc_amd._lib.LIB_PATH):
        orc_amd.build()
    return orc_amd._lib.lib()


def test_scalar_struct_layout_matches_c(tmp_path):
    from orc_amd.settings import ScalarBc, ScalarSettings
    offs = ", ".join("offsetof(OrcScalarSettings, %s)" % f for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\n'
           'int main(){printf("%%zu %%zu' + ' %zu' * len(FIELDS) + ' %%d %%d %%d %%d", sizeof(OrcScalarSettings), _Alignof(OrcScalarSettings), '
           + offs + ', (int)ORC_SCALAR_BC_DEFAULT, (int)ORC_SCALAR_BC_VALUE, (int)ORC_SCALAR_BC_FLUX, (int)ORC_SCALAR_BC_ZERO_GRADIENT);return 0;}')
    src = src.replace("%%", "%")
    exe = str(tmp_path / "sizeof_scalar")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    out = list(map(int, subprocess.check_output([exe]).split()))
    size, align, offsets, kinds = out[0], out[1], out[2:2 + len(FIELDS)], out[2 + len(FIELDS):]
    assert size == C.sizeof(ScalarSettings) == 64 and align == 8
    assert offsets == [getattr(ScalarSettings, f).offset for f in FIELDS]
    # no implicit padding: every field ends where the next begins
    sizes = [C.sizeof(t) for _, t in ScalarSettings._fields_]
    assert [o + z for o, z in zip(offsets, sizes)] == offsets[1:] + [size]
    assert kinds == [ScalarBc.DEFAULT, ScalarBc.VALUE, ScalarBc.FLUX, ScalarBc.ZERO_GRADIENT] == [0, 1, 2, 3]


def test_settings_structs_unchanged():
    from orc_amd.settings import NumericalSettings, Transient
    assert C.sizeof(NumericalSettings) == 88 and C.sizeof(Transient) == 32


def test_new_symbols_are_exported(lib):
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "orc_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr


def test_scalar_settings_defaults(lib):
    from orc_amd.settings import ScalarSettings
    c = ScalarSettings.default()
    assert (c.diffusivity, c.scheme, c.solver_type, c.preconditioner, c.reserved0) == (1e-3, 0, 3, 1, 0)
    assert (c.iterations, c.relative_convergence_threshold, c.relaxation, c.outer_iterations, c.outer_tolerance) == (500, 1e-10, 0.5, 30, 1e-8)
    assert ScalarSettings.default(scheme=5, diffusivity=2.0).scheme == 5
    with pytest.raises(AttributeError):
        ScalarSettings.default(no_such_field=1)


def test_python_api_present():
    from orc_amd import solver
    for name in ("set_scalar", "set_scalar_bc", "set_scalar_field", "get_scalar_field", "set_scalar_source", "set_scalar_levels",
                 "solve_scalar", "last_scalar_report", "assemble_scalar", "scalar_boundary_flux"):
        assert callable(getattr(solver.Solver, name)), name


def test_default_conditions_resolve_from_the_zone_type():
    zt = [R.INTERIOR, R.WALL, R.SYMMETRY, R.VELOCITY_INLET, R.PRESSURE_INLET, R.PRESSURE_OUTLET, R.WALL]
    k, v = R.resolve_bcs(zt, [0, 0, 0, 0, 0, 0, R.VALUE], [0, 9, 9, 9, 9, 9, 3.5])
    assert list(k[1:]) == [R.FLUX, R.FLUX, R.VALUE, R.VALUE, R.ZERO_GRADIENT, R.VALUE]
    assert list(v[1:]) == [0, 0, 0, 0, 0, 3.5]


def test_conduction_between_plates_is_linear():
    # no flow, VALUE 0 and 1 at the ends: the discrete solution is the linear profile exactly (to round-off)
    for N in (4, 17, 64):
        A, b = R.fv1d(N, 2.0, 0.0, 0.3, 1.0, R.UD, 0.0, 1.0)
        x = R.centroids(N, 2.0)
        assert np.allclose(np.linalg.solve(A, b), x / 2.0, rtol=0, atol=1e-13)


def test_plug_flow_converges_to_the_exponential_profile():
    for s in (R.UD, R.CD1):
        e = [R.plug_flow_error(N, s) for N in R.PLUG_N]
        assert e[-1] < (2e-2 if s == R.UD else 2e-4), (s, e)


@pytest.mark.parametrize("scheme", [R.UD, R.CD1])
def test_observed_spatial_order_is_in_the_band(scheme):
    lo, hi = R.ORDER_BAND[scheme]
    order = R.observed_order([R.plug_flow_error(N, scheme) for N in R.PLUG_N])
    assert np.all((order >= lo) & (order <= hi)), order


def test_fv1d_is_bounded_and_conservative():
    for s in (R.UD, R.CD1):
        A, b = R.fv1d(40, 1.0, 1.0, 0.5, 1.0, s, 0.0, 1.0)
        phi = np.linalg.solve(A, b)
        assert phi.min() >= 0.0 and phi.max() <= 1.0
        # every interior face moves as much phi out of one cell as into the other: the row sums of the convective part
        # telescope to the boundary terms
        A0, _ = R.fv1d(40, 1.0, 1.0, 0.0, 1.0, s, 0.0, 1.0)
        assert abs(A0.sum()) < 1e-12


def test_slab_series_and_semi_discrete_solution_agree():
    # second order in space: the error at t quarters when the cells halve
    L, alpha = 1.0, 1.0
    for t in (0.02, 0.1):
        errs = []
        for N in (32, 64, 128):
            K = R.conduction_operator(N, L, alpha)
            errs.append(np.abs(R.semi_discrete(K, np.ones(N), t) - R.slab_series(R.centroids(N, L), t, L, alpha)).max())
        assert errs[-1] < 1e-4 and np.all(np.abs(R.observed_order(errs) - 2.0) < 0.05), errs
    x = R.centroids(64, L)
    assert np.allclose(R.slab_series(x, 0.02, L, alpha), R.slab_series(x, 0.02, L, alpha, terms=8001), atol=1e-12)


@pytest.mark.parametrize("scheme", [R.EULER, R.BDF2])
def test_observed_temporal_order_is_in_the_band(scheme):
    lo, hi = R.TIME_ORDER_BAND[scheme]
    N, T = 32, 0.05
    K = R.conduction_operator(N, 1.0, 1.0)
    exact = R.semi_discrete(K, np.ones(N), T)
    errs = [np.abs(R.march(K, np.ones(N), T / k, k, scheme) - exact).max() for k in (20, 40, 80)]
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), (errs, order)


def _line_mesh(N, L=1.0):
    """N cells in a row along x, unit cross-section, as MeshArrays-like dict (inlet zone 1 at x = 0, outlet zone 2, walls 3)"""
    h = L / N
    faces = []  # (c0, c1, zone, area, normal, centroid)
    for i in range(N + 1):
        x = i * h
        if i == 0:
            faces.append((0, -1, 1, 1.0, (-1.0, 0.0, 0.0), (x, 0.5, 0.5)))
        elif i == N:
            faces.append((N - 1, -1, 2, 1.0, (1.0, 0.0, 0.0), (x, 0.5, 0.5)))
        else:
            faces.append((i - 1, i, 0, 1.0, (1.0, 0.0, 0.0), (x, 0.5, 0.5)))
    for i in range(N):
        for nrm, ctr in (((0, -1, 0), (0, 0, .5)), ((0, 1, 0), (0, 1, .5)), ((0, 0, -1), (0, .5, 0)), ((0, 0, 1), (0, .5, 1))):
            faces.append((i, -1, 3, h, nrm, ((i + 0.5) * h, ctr[1], ctr[2])))
    per = [[] for _ in range(N)]
    for f, (c0, c1, *_rest) in enumerate(faces):
        per[c0].append(f)
        if c1 >= 0:
            per[c1].append(f)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in per])])
    return dict(face_c0=np.array([f[0] for f in faces]), face_c1=np.array([f[1] for f in faces]),
                face_zone=np.array([f[2] for f in faces], dtype=np.int32), face_area=np.array([f[3] for f in faces]),
                face_normal=np.array([f[4] for f in faces], dtype=float), face_centroid=np.array([f[5] for f in faces], dtype=float),
                cell_centroid=np.array([((i + 0.5) * h, 0.5, 0.5) for i in range(N)]), cell_volume=np.full(N, h),
                cell_face_ptr=ptr, cell_faces=np.concatenate([sorted(p) for p in per]),
                zone_type=np.array([R.INTERIOR, R.VELOCITY_INLET, R.PRESSURE_OUTLET, R.SYMMETRY], dtype=np.int32),
                zone_vector=np.array([[0, 0, 0], [1.0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=float))


@pytest.mark.parametrize("scheme", [R.UD, R.CD1, R.TVD_UD])
def test_mesh_assembly_reduces_to_the_1d_model(scheme):
    N, U, gamma, rho = 12, 1.0, 0.05, 1.0
    a = _line_mesh(N)
    u = np.full(N, U)
    z = np.zeros(N)
    flux = R.face_flux_linear(a, u, z, z)
    k, v = R.resolve_bcs(a["zone_type"], [0, R.VALUE, R.VALUE, 0], [0, 0.0, 1.0, 0])
    rows, cols, vals, b = R.assemble(a, flux, rho, gamma, scheme, k, v, phi=np.linspace(0, 1, N))
    A = np.zeros((N, N))
    np.add.at(A, (rows, cols), vals)
    A1, b1 = R.fv1d(N, 1.0, U, gamma, rho, R.UD if scheme == R.TVD_UD else scheme, 0.0, 1.0)
    assert np.allclose(A, A1, rtol=1e-14, atol=1e-14) and np.allclose(b, b1, rtol=1e-14, atol=1e-14)


def test_tvd_cd1_correction_turns_ud_into_cd1_at_the_fixed_point():
    N, gamma = 12, 0.05
    a = _line_mesh(N)
    flux = R.face_flux_linear(a, np.ones(N), np.zeros(N), np.zeros(N))
    k, v = R.resolve_bcs(a["zone_type"], [0, R.VALUE, R.VALUE, 0], [0, 0.0, 1.0, 0])
    A1, b1 = R.fv1d(N, 1.0, 1.0, gamma, 1.0, R.CD1, 0.0, 1.0)
    phi_cd1 = np.linalg.solve(A1, b1)
    rows, cols, vals, b = R.assemble(a, flux, 1.0, gamma, R.TVD_CD1, k, v, phi=phi_cd1)
    A = np.zeros((N, N))
    np.add.at(A, (rows, cols), vals)
    assert np.allclose(np.linalg.solve(A, b), phi_cd1, rtol=0, atol=1e-13)


def test_boundary_flux_balances_the_source():
    N, gamma = 16, 0.05
    a = _line_mesh(N)
    flux = R.face_flux_linear(a, np.ones(N), np.zeros(N), np.zeros(N))
    k, v = R.resolve_bcs(a["zone_type"], [0, R.VALUE, R.FLUX, 0], [0, 0.3, 0.7, 0])
    S = np.linspace(1, 2, N)
    rows, cols, vals, b = R.assemble(a, flux, 1.0, gamma, R.UD, k, v, source=S)
    A = np.zeros((N, N))
    np.add.at(A, (rows, cols), vals)
    phi = np.linalg.solve(A, b)
    bf = R.boundary_flux(a, flux, 1.0, gamma, k, v, phi)
    assert abs(bf.sum() + (S * a["cell_volume"]).sum()) < 1e-12
