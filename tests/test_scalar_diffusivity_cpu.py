"""The scalar arm's variable diffusivity without a GPU: the OrcScalarDiffusivity layout from C and from ctypes, the exported entry
points and the Python API, and the numpy restatement (tests/scalar_diffusivity_restatement.py) the GPU tests compare against — the
face formula, the constant-Gamma identity with tests/scalar_restatement.py in every bit, two-layer conduction against its exact
profile and LINEAR conduction against its closed form with the observed order.

Recorded on the 1-D models (the GPU tests hold the device to them):
  two layers Gamma | 4 Gamma, N = 16: HARMONIC max |phi - exact| = 7.8e-16 (rounding), ARITHMETIC 1.73e-2 (0.288 / N to first order);
  LINEAR, beta = 2, ARITHMETIC faces, the cell's Gamma at the VALUE faces, Picard from phi = 0 to 1e-8:
      N = 16  relative L2 error 1.93e-3, 11 rounds;  N = 32  5.3e-4, 12 rounds;  N = 64  1.4e-4, 12 rounds; orders 1.86, 1.92."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scalar_diffusivity_restatement as R
import scalar_restatement as S
from conftest import ROOT, splitmix64_uniform

NEW_SYMBOLS = ["orc_scalar_diffusivity_default", "orc_solver_set_scalar_diffusivity", "orc_solver_set_scalar_diffusivity_field",
               "orc_solver_get_scalar_diffusivity", "orc_bench_scalar_diffusivity"]
FIELDS = ["model", "face_interpolation", "schmidt_t", "beta", "phi_ref", "gamma_min", "gamma_max", "reserved0"]


@pytest.fixture(scope="module")
def lib():
    import orc_amd
    if not os.path.exists(orc_amd._lib.LIB_PATH):
        orc_amd.build()
    return orc_amd._lib.lib()


def test_struct_layout_matches_c(tmp_path):
    from orc_amd.settings import ScalarDiffusivity, ScalarDiffusivityModel as M
    offs = ", ".join("offsetof(OrcScalarDiffusivity, %s)" % f for f in FIELDS)
    enums = "ORC_SCALAR_GAMMA_CONSTANT", "ORC_SCALAR_GAMMA_FIELD", "ORC_SCALAR_GAMMA_EDDY", "ORC_SCALAR_GAMMA_LINEAR"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\n'
           'int main(){printf("%zu %zu' + " %zu" * len(FIELDS) + " %d" * len(enums) + '", sizeof(OrcScalarDiffusivity), '
           "_Alignof(OrcScalarDiffusivity), " + offs + ", " + ", ".join("(int)" + e for e in enums) + ");return 0;}")
    exe = str(tmp_path / "sizeof_scalar_diffusivity")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    out = list(map(int, subprocess.check_output([exe]).split()))
    size, align, offsets, models = out[0], out[1], out[2:2 + len(FIELDS)], out[2 + len(FIELDS):]
    assert size == C.sizeof(ScalarDiffusivity) == 56 and align == 8
    assert offsets == [getattr(ScalarDiffusivity, f).offset for f in FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48]
    sizes = [C.sizeof(t) for _, t in ScalarDiffusivity._fields_]
    assert [o + z for o, z in zip(offsets, sizes)] == offsets[1:] + [size]  # no implicit padding
    assert models == [M.CONSTANT, M.FIELD, M.EDDY, M.LINEAR] == [R.CONSTANT, R.FIELD, R.EDDY, R.LINEAR] == [0, 1, 2, 3]


def test_new_symbols_are_exported_and_the_python_api_is_present(lib):
    from orc_amd import solver
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "orc_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr
    for name in ("set_scalar_diffusivity", "set_scalar_diffusivity_field", "scalar_diffusivity", "bench_scalar_diffusivity"):
        assert callable(getattr(solver.Solver, name)), name


def test_defaults_and_make(lib):
    from orc_amd.settings import ScalarDiffusivity, ScalarDiffusivityModel as M, ViscosityFace
    c = ScalarDiffusivity.make(M.CONSTANT)
    want = R.params(R.CONSTANT)
    assert {f: getattr(c, f) for f in FIELDS} == want
    c = ScalarDiffusivity.make(M.EDDY, ViscosityFace.HARMONIC, schmidt_t=0.5, gamma_max=3.0)
    assert (c.model, c.face_interpolation, c.schmidt_t, c.gamma_min, c.gamma_max) == (2, 1, 0.5, 1e-12, 3.0)
    assert ScalarDiffusivity.make(M.LINEAR, beta=2.0, phi_ref=0.25).beta == 2.0
    with pytest.raises(AttributeError):
        ScalarDiffusivity.make(M.FIELD, no_such_field=1)


def test_face_formula_is_symmetric_and_exact_for_equal_cells():
    g = R.log_uniform(splitmix64_uniform(4000, 11))
    h = R.log_uniform(splitmix64_uniform(4000, 12))
    for mode in (R.ARITHMETIC, R.HARMONIC):
        assert np.array_equal(R.face_gamma(mode, g, h), R.face_gamma(mode, h, g))
        assert np.array_equal(R.face_gamma(mode, g, g), g)
        f = R.face_gamma(mode, g, h)
        assert np.all(f >= np.fmin(g, h) * (1 - 4e-16)) and np.all(f <= np.fmax(g, h) * (1 + 4e-16))
    assert np.all(R.face_gamma(R.HARMONIC, g, h) <= R.face_gamma(R.ARITHMETIC, g, h) * (1 + 4e-16))
    # the harmonic mean 2 g h / (g + h)
    assert np.allclose(R.face_gamma(R.HARMONIC, g, h), 2 * g * h / (g + h), rtol=1e-14, atol=0)


def test_laws_follow_the_written_order_and_the_clamp():
    mu = np.array([1e-3, 5e-4, 3e-3, 1.0])
    p = R.params(R.EDDY, schmidt_t=0.5, gamma_max=0.1)
    got = R.law(p, 2e-3, mu=mu, mu_lam=1e-3)
    assert np.array_equal(got, [2e-3, 2e-3, 2e-3 + (3e-3 - 1e-3) / 0.5, 0.1])
    p = R.params(R.LINEAR, beta=2.0, phi_ref=0.5, gamma_min=1e-4)
    phi = np.array([0.5, 1.0, 0.0, -1.0])
    assert np.array_equal(R.law(p, 1e-3, phi=phi), [1e-3, 1e-3 * (1.0 + 2.0 * 0.5), 1e-4, 1e-4])
    assert np.array_equal(R.law(R.params(R.FIELD), 1e-3, field=mu), mu)
    assert np.array_equal(R.law(R.params(R.CONSTANT), 1e-3, n=3), np.full(3, 1e-3))
    # LINEAR with beta = 0 and EDDY without an eddy part are gamma0 exactly
    assert np.array_equal(R.law(R.params(R.LINEAR), 7e-4, phi=phi), np.full(4, 7e-4))
    assert np.array_equal(R.law(R.params(R.EDDY), 7e-4, mu=np.full(4, 1e-3), mu_lam=1e-3), np.full(4, 7e-4))


def assembly_case(a, n):
    from test_gpu_scalar import ASSEMBLY_BCS, ASSEMBLY_TYPES, scalar_bcs, seeded_flow, set_zone_types
    set_zone_types(a, ASSEMBLY_TYPES)
    k, v = scalar_bcs(a, ASSEMBLY_BCS)
    kr, vr = S.resolve_bcs(a["zone_type"], k, v)
    flow = seeded_flow(a)
    return kr, vr, S.face_flux_linear(a, *flow[:3])


@pytest.mark.parametrize("mesh_name", ["hex", "poly"])
def test_constant_gamma_reproduces_the_scalar_restatement_in_every_bit(tmp_path, mesh_name):
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, hex_channel, set_mixed_channel_bcs, write_mixed_channel_msh
    if mesh_name == "poly":
        path = str(tmp_path / "poly.msh")
        write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=True)
        a = set_mixed_channel_bcs(MeshArrays(orc_io.read_mesh(path).arrays()))
    else:
        a = hex_channel(8, 6, 4)
    n = a.n_cells
    kr, vr, flux = assembly_case(a, n)
    rho, gamma = 1.3, 2.5e-4
    phi = 0.5 + 0.5 * splitmix64_uniform(n, 7)
    src = 3.0 * splitmix64_uniform(n, 8)
    lv = [phi * (1 + 0.1 * splitmix64_uniform(n, 9)), phi * (1 - 0.1 * splitmix64_uniform(n, 10))]
    for scheme, time in ((S.UD, None), (S.CD1, (2.7e-3, S.BDF2, lv[0], lv[1])), (S.TVD_UMIST, (2.7e-3, S.EULER, lv[0], None))):
        want = S.assemble(a, flux, rho, gamma, scheme, kr, vr, phi=phi, source=src, time=time)
        for mode in (R.ARITHMETIC, R.HARMONIC):
            got = R.assemble(a, flux, rho, np.full(n, gamma), mode, scheme, kr, vr, phi=phi, source=src, time=time)
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (mesh_name, scheme, mode)
    assert np.array_equal(R.boundary_flux(a, flux, rho, np.full(n, gamma), kr, vr, phi), S.boundary_flux(a, flux, rho, gamma, kr, vr, phi))
    # and a variable Gamma is another system, with another boundary flux
    g = R.log_uniform(splitmix64_uniform(n, 13))
    assert not np.array_equal(R.assemble(a, flux, rho, g, R.ARITHMETIC, S.UD, kr, vr)[2], want[2])
    assert not np.array_equal(R.boundary_flux(a, flux, rho, g, kr, vr, phi), S.boundary_flux(a, flux, rho, gamma, kr, vr, phi))


def test_two_layer_conduction_harmonic_is_exact_and_arithmetic_is_not():
    L, g1 = 1e-3, 0.7
    for N in (16, 32):
        x = S.centroids(N, L)
        exact = R.two_layer_exact(x, L, g1, 4 * g1)
        eh = np.abs(R.two_layer_model(N, L, g1, 4 * g1, R.HARMONIC) - exact).max()
        ea = np.abs(R.two_layer_model(N, L, g1, 4 * g1, R.ARITHMETIC) - exact).max()
        print("two layers, N = %d: HARMONIC %.3e, ARITHMETIC %.3e" % (N, eh, ea))
        assert eh <= 1e-14, eh  # rounding: the harmonic face value carries the interface flux exactly
        # ARITHMETIC gives the interface face the resistance h / (2.5 g1) where the two half cells have 0.625 h / g1: the total
        # resistance 0.625 L / g1 is short by 0.225 h / g1, the flux too large by the factor 1 / (1 - 0.36 / N), and the profile
        # just below the interface (phi = 0.8 there) off by 0.8 * 0.36 / N = 0.288 / N to first order in 1 / N
        assert 0.2 / N < ea < 0.4 / N, ea
    # the flux is one constant across the interface: q = (phi_{i+1} - phi_i) Gamma_f / h on both sides of it
    phi = R.two_layer_model(16, L, g1, 4 * g1, R.HARMONIC)
    q = np.diff(phi) / (L / 16) * R.face_gamma(R.HARMONIC, R.two_layer_gamma(16, g1, 4 * g1)[:-1], R.two_layer_gamma(16, g1, 4 * g1)[1:])
    assert np.allclose(q, q[0], rtol=1e-12, atol=0)


def test_linear_conduction_picard_model_and_its_observed_order():
    p = R.params(R.LINEAR, beta=2.0)
    errs, rounds = [], []
    for N in (16, 32, 64):
        phi, k = R.linear_picard(N, 1.0, 1.0, p, tol=1e-8)
        errs.append(R.rel_l2(phi, R.linear_exact(S.centroids(N, 1.0), 1.0, 2.0)))
        rounds.append(k)
    order = S.observed_order(errs)
    print("LINEAR conduction: errors %s, rounds %s, orders %s" % (errs, rounds, order))
    assert rounds == [11, 12, 12]
    assert abs(errs[0] - 1.93e-3) <= 0.01e-3 and abs(errs[1] - 5.3e-4) <= 0.1e-4 and abs(errs[2] - 1.4e-4) <= 0.1e-4, errs
    assert abs(order[0] - 1.86) <= 0.01 and abs(order[1] - 1.92) <= 0.01, order
    assert np.all(order > 1.7)
    assert abs(errs[0] / errs[1] - 3.64) <= 0.01
    assert max(rounds) <= 30  # inside the default outer_iterations
    # the closed form satisfies its equation and its ends
    x = np.linspace(0.0, 1.0, 11)
    e = R.linear_exact(x, 1.0, 2.0)
    assert np.allclose(e + 2.0 * e * e / 2.0, 2.0 * x, rtol=0, atol=1e-15) and e[0] == 0.0 and abs(e[-1] - 1.0) <= 1e-15
