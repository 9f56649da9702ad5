"""Variable scalar diffusivity (orc_solver_set_scalar_diffusivity*, orc_amd/csrc/scalar.hip) on the device: the plain arm's bits
where Gamma is the constant, the Gamma part and the system bit for bit against tests/scalar_diffusivity_restatement.py at the launch
edges of the XCD-contiguous block walk, two-layer conduction and LINEAR conduction against their 1-D models, the eddy diffusivity in
a Smagorinsky BDF2 run, refusals, repeatability, the bench hook and two ranks on one GPU.

Bit for bit means equal uint64 views.  Tolerances: 1e-9 (max norm) for a converged conduction solve, the bar of
test_conduction_between_plates_is_linear in tests/test_gpu_scalar.py; 1e-8 of the summed magnitudes for the boundary fluxes, the bar
of that file's conservation test; 1e-10 between one and two ranks, the bar of tests/scalar_mp_worker.py.  The renumbered (RCM) mesh
visits a cell's faces in another order, so its sums round differently: 1e-14 relative there, as tests/test_gpu_scalar.py has it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scalar_diffusivity_restatement as R
import scalar_restatement as S
from conftest import ROOT, splitmix64_uniform
from test_gpu_scalar import (ASSEMBLY_BCS, ASSEMBLY_TYPES, LINEAR as VINTERP_LINEAR, PLUG_TYPES, hex_mesh, make_solver, mixed_mesh,
                             scalar_settings, seeded_flow, settings)
from test_gpu_transient import channel_flow, transient

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
CG = 20
VIS_FIELD, VIS_POWER_LAW, VIS_CARREAU, VIS_SMAGORINSKY = 1, 2, 3, 4
RHO, MU, GAMMA0 = 1.3, 1e-3, 2.5e-4
CONDUCTION_TOL = 1e-9
# channel_flow.msh: VALUE on the inlet and on the walls (every D_b sees its cell's Gamma), the rest DEFAULT
CHANNEL_BCS = {"INLET": (S.VALUE, 0.3), "WALL": (S.VALUE, 1.0), "PERIODIC_-Z": (S.ZERO_GRADIENT, 0.0)}


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def gam(model, face=R.ARITHMETIC, **kw):
    from orc_amd.settings import ScalarDiffusivity
    return ScalarDiffusivity.make(model, face, **kw)


def visc(model, **kw):
    from orc_amd.settings import Viscosity
    return Viscosity.make(model, **kw)


def case_mesh(tmp_path, name):
    """(arrays, mesh, scalar conditions by zone name)"""
    if name == "channel_flow":
        a, m = channel_flow()
        return a, m, CHANNEL_BCS
    if name == "poly":
        a, m = mixed_mesh(tmp_path, True, ASSEMBLY_TYPES)
    elif name == "hex_rcm":
        a, m = hex_mesh(8, 6, 4, ordering=1, types=ASSEMBLY_TYPES)
    else:
        a, m = hex_mesh(*name, types=ASSEMBLY_TYPES)
    return a, m, ASSEMBLY_BCS


def scalar_state(s):
    return s.assemble_scalar() + (s.get_scalar_field(), s.scalar_boundary_flux(), s.scalar_diffusivity())


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("scheme", [S.UD, S.TVD_UMIST], ids=["ud", "umist"])
@pytest.mark.parametrize("mesh_name", ["channel_flow", "poly"])
def test_constant_gamma_gives_the_plain_arm_bit_for_bit(gpu, tmp_path, mesh_name, scheme):
    """FIELD with every entry gamma0 (both face modes), LINEAR with beta = 0 and EDDY over Smagorinsky with cs = 0 (mu_c = mu exactly).
    UD with one outer round, since LINEAR runs the Picard loop where the plain UD arm solves once; UMIST with three for all."""
    a, m, bcs = case_mesh(tmp_path, mesh_name)
    n = a.n_cells
    flow = seeded_flow(a)
    phi = 0.5 + 0.5 * splitmix64_uniform(n, 7)
    sc = scalar_settings(scheme=scheme, diffusivity=GAMMA0, outer_iterations=1 if scheme == S.UD else 3)

    def run(configure):
        s, _, _ = make_solver(m, a, sc, bcs, flow, rho=RHO, mu=MU)
        configure(s)
        s.set_scalar_field(phi)
        asm, bf0 = s.assemble_scalar(), s.scalar_boundary_flux()
        rep = s.solve_scalar()
        return s, asm + (bf0, rep, s.get_scalar_field(), s.scalar_boundary_flux(), s.scalar_diffusivity())

    def field(face):
        def f(s):
            s.set_scalar_diffusivity_field(np.full(n, GAMMA0))
            s.set_scalar_diffusivity(gam(R.FIELD, face))
        return f

    def eddy(s):
        s.set_viscosity(visc(VIS_SMAGORINSKY, cs=0.0))
        s.set_scalar_diffusivity(gam(R.EDDY, R.HARMONIC, schmidt_t=0.5))

    _, plain = run(lambda s: None)
    assert same_bits(plain[6], np.full(n, GAMMA0)) and not same_bits(plain[2], plain[5])
    variants = {"field_arithmetic": field(R.ARITHMETIC), "field_harmonic": field(R.HARMONIC),
                "linear_beta_0": lambda s: s.set_scalar_diffusivity(gam(R.LINEAR, R.HARMONIC, beta=0.0, phi_ref=0.3)), "eddy_cs_0": eddy}
    for name, configure in variants.items():
        s, got = run(configure)
        for k, (x, y) in enumerate(zip(got, plain)):
            assert same_bits(x, y), (mesh_name, scheme, name, k)
    # a field that is not the constant is another system; switching the model off puts the constant Gamma part back bit for bit
    s.set_scalar_diffusivity_field(R.log_uniform(splitmix64_uniform(n, 13), 1e-5, 1e-3))
    s.set_scalar_diffusivity(gam(R.FIELD, R.HARMONIC))
    s.set_scalar_field(phi)
    assert not same_bits(s.assemble_scalar()[0], plain[0])
    for off in (None, gam(R.CONSTANT)):
        s.set_scalar_diffusivity(gam(R.FIELD, R.ARITHMETIC))
        s.assemble_scalar()
        s.set_scalar_diffusivity(off)
        for x, y in zip(s.assemble_scalar(), plain[:2]):
            assert same_bits(x, y), (mesh_name, scheme, off)
        assert same_bits(s.scalar_boundary_flux(), plain[2]) and same_bits(s.scalar_diffusivity(), plain[6])


# ------------------------------------------------------------------ 2. the rebuild, bit for bit
# hex channels at the launch edges of a 256-thread block, of the XCD walk (on for a grid that is a multiple of 8) and of the
# 2048-workgroup clamp: the list of tests/test_gpu_viscosity.py for diffusion_var_k
REBUILD_MESHES = ["channel_flow", "poly", "hex_rcm", (15, 17, 1), (16, 16, 1), (257, 1, 1), (23, 89, 1), (81, 81, 80)]
N_CELLS = {(15, 17, 1): 255, (16, 16, 1): 256, (257, 1, 1): 257, (23, 89, 1): 2047, (81, 81, 80): 524880}


@pytest.mark.parametrize("mesh_name", REBUILD_MESHES, ids=lambda s: s if isinstance(s, str) else "%dx%dx%d" % s)
def test_system_equals_the_restatement_bit_for_bit(gpu, tmp_path, mesh_name):
    a, m, bcs = case_mesh(tmp_path, mesh_name)
    n = a.n_cells
    large = mesh_name == (81, 81, 80)
    if not isinstance(mesh_name, str):
        assert n == N_CELLS[mesh_name]
    exact = mesh_name != "hex_rcm"
    g = m.cell_order()
    assert np.array_equal(g, np.arange(n)) == exact
    rp, ci = m.matrix_pattern()
    flow = seeded_flow(a)
    flux = S.face_flux_linear(a, *flow[:3])
    phi = 0.5 + 0.5 * splitmix64_uniform(n, 7)
    src = 3.0 * splitmix64_uniform(n, 8)
    field = R.log_uniform(splitmix64_uniform(n, 0x47414d4d), 1e-6, 1e2)
    assert field.min() < 1e-5 and field.max() > 10.0
    laws = {R.FIELD: R.params(R.FIELD),
            R.EDDY: R.params(R.EDDY, schmidt_t=0.7, gamma_min=1e-6, gamma_max=1e2),  # over a log-uniform viscosity FIELD
            R.LINEAR: R.params(R.LINEAR, beta=1e6, phi_ref=0.5, gamma_min=1e-6, gamma_max=1e2)}  # both clamps bind
    combos = [(sch, model, face) for sch in (S.UD, S.TVD_UMIST) for model in (R.FIELD, R.EDDY, R.LINEAR) for face in (R.ARITHMETIC, R.HARMONIC)]
    if large:  # the assembly only, one law that gathers the field and one that gathers the viscosity
        combos = [(S.UD, R.FIELD, R.HARMONIC), (S.UD, R.EDDY, R.ARITHMETIC)]
    solvers, seen = {}, []
    for sch, model, face in combos:
        if sch not in solvers:
            s, k, v = make_solver(m, a, scalar_settings(scheme=sch, diffusivity=GAMMA0), bcs, flow, rho=RHO, mu=MU)
            s.set_viscosity_field(field[::-1].copy())
            s.set_viscosity(visc(VIS_FIELD))
            s.set_scalar_field(phi)
            s.set_scalar_source(src)
            s.set_scalar_diffusivity_field(field)
            solvers[sch] = (s, S.resolve_bcs(a["zone_type"], k, v))
        s, (kr, vr) = solvers[sch]
        p = dict(laws[model], face_interpolation=face)
        s.set_scalar_diffusivity(gam(model, face, **{f: p[f] for f in ("schmidt_t", "beta", "phi_ref", "gamma_min", "gamma_max")}))
        got_a, got_b = s.assemble_scalar()
        mu_c = s.viscosity()
        assert same_bits(mu_c, field[::-1])
        gamma_c = R.law(p, GAMMA0, field=field, mu=mu_c, mu_lam=MU, phi=phi)
        if model != R.FIELD:
            assert gamma_c.min() == 1e-6 if model == R.LINEAR else gamma_c.min() == GAMMA0
            assert gamma_c.max() == 1e2 and len(np.unique(gamma_c)) > n // 4
        assert same_bits(s.scalar_diffusivity(), gamma_c), (mesh_name, sch, model, face)
        rows, cols, vals, b = R.assemble(a, flux, RHO, gamma_c, face, sch, kr, vr, phi=phi, source=src)
        want_a, want_b = S.on_pattern(rows, cols, vals, rp, ci, g), b[g]
        if exact:
            assert same_bits(got_a, want_a), (mesh_name, sch, model, face, int(np.count_nonzero(got_a != want_a)))
            assert same_bits(got_b, want_b), (mesh_name, sch, model, face, int(np.count_nonzero(got_b != want_b)))
        else:
            assert np.all(np.abs(got_a - want_a) <= 1e-14 * np.abs(want_a)), (sch, model, face)
            assert np.all(np.abs(got_b - want_b) <= 1e-14 * np.abs(want_b).max()), (sch, model, face)
        bf, want_bf = s.scalar_boundary_flux(), R.boundary_flux(a, flux, RHO, gamma_c, kr, vr, phi)
        assert np.all(np.abs(bf - want_bf) <= 1e-8 * np.abs(want_bf).sum()), (mesh_name, sch, model, face, bf, want_bf)
        seen.append(got_a)
    assert not same_bits(seen[0], seen[1])  # the face modes, or the laws, differ
    if large:
        return
    # a solve on the rebuilt system: UD with a FIELD over two decades and a source; at convergence the boundary fluxes balance the
    # source (the conservation identity holds with the cell's Gamma in the boundary term)
    s, _, _ = make_solver(m, a, scalar_settings(diffusivity=GAMMA0, iterations=2000, relative_convergence_threshold=1e-13), bcs, flow,
                          rho=RHO, mu=MU)
    s.set_scalar_source(src)
    s.set_scalar_diffusivity_field(R.log_uniform(splitmix64_uniform(n, 17), 1e-4, 1e-2))
    s.set_scalar_diffusivity(gam(R.FIELD, R.HARMONIC))
    s.solve_scalar()
    bf = s.scalar_boundary_flux()
    sv = float((src * np.asarray(a["cell_volume"])).sum())
    print("conservation %s: sum of boundary fluxes %.6e, source %.6e" % (mesh_name, bf.sum(), sv))
    assert abs(bf.sum() + sv) <= 1e-8 * (np.abs(bf).sum() + abs(sv)), (bf, sv)


# ------------------------------------------------------------------ 3.-4. conduction through a column at rest
LX = 0.002
REST_TYPES = dict(PLUG_TYPES, INLET=(S.VELOCITY_INLET, (0.0, 0.0, 0.0)))
ENDS = {"INLET": (S.VALUE, 0.0), "OUTLET": (S.VALUE, 1.0)}


def column(N, sc, mu=MU):
    """a hex column of N cells along x, flow at rest, VALUE 0 at x = 0 and VALUE 1 at x = LX (plug_solve's column).  The callers
    solve with the CG arm: at rest the system is symmetric positive definite.  (Measured on this column with two layers: the default
    BiCGSTAB + Jacobi arm stops at a relative residual of 1.8e-2 whatever its iteration count, where CG, GMRES and BiCGSTAB without
    the preconditioner reach 1e-15 on the same, bit-identical system.)"""
    a, m = hex_mesh(N, 1, 1, lx=LX, types=REST_TYPES)
    z = np.zeros(a.n_cells)
    s, _, _ = make_solver(m, a, sc, ENDS, (z, z, z, z), rho=1.0, mu=mu)
    x = np.asarray(a["cell_centroid"])[:, 0]
    return s, x, np.floor(x / (LX / N)).astype(int)


@pytest.mark.parametrize("source", ["field", "eddy"])
def test_two_layer_conduction(gpu, source):
    """Gamma | 4 Gamma, as a FIELD and as EDDY over a viscosity FIELD mu | 4 mu with schmidt_t = 0.5 and mu = gamma0 / 2"""
    N, g0 = 16, 0.7
    errs = {}
    for face in (R.HARMONIC, R.ARITHMETIC):
        s, x, row = column(N, scalar_settings(diffusivity=g0, iterations=200, solver_type=CG), mu=g0 / 2)
        lower = x < LX / 2
        if source == "field":
            s.set_scalar_diffusivity_field(np.where(lower, g0, 4 * g0))
            s.set_scalar_diffusivity(gam(R.FIELD, face))
            want_gamma = np.where(lower, g0, 4 * g0)
        else:
            s.set_viscosity_field(np.where(lower, g0 / 2, 4 * (g0 / 2)))
            s.set_viscosity(visc(VIS_FIELD))
            p = R.params(R.EDDY, face, schmidt_t=0.5)
            s.set_scalar_diffusivity(gam(R.EDDY, face, schmidt_t=0.5))
            want_gamma = R.law(p, g0, mu=s.viscosity(), mu_lam=g0 / 2)
            assert np.allclose(want_gamma, np.where(lower, g0, 4 * g0), rtol=1e-15, atol=0)
        rep = s.solve_scalar()
        phi = s.get_scalar_field()
        gamma = s.scalar_diffusivity()
        assert same_bits(gamma, want_gamma) and rep[0] == 1
        g_row = np.empty(N)
        g_row[row] = gamma
        A, b = R.conduction_1d(g_row, face, LX, 0.0, 1.0)
        model = np.linalg.solve(A, b)
        exact = R.two_layer_exact(x, LX, g0, 4 * g0)
        errs[face] = (np.abs(phi - model[row]).max(), np.abs(phi - exact).max(), np.abs(model[row] - exact).max())
        print("two layers (%s), face mode %d: |device - model| %.3e, |device - exact| %.3e, |model - exact| %.3e" % ((source, face) + errs[face]))
        assert errs[face][0] <= CONDUCTION_TOL, errs
    assert errs[R.HARMONIC][1] <= CONDUCTION_TOL, errs
    # ARITHMETIC is off from the exact profile by what the 1-D model says (tests/test_scalar_diffusivity_cpu.py: 0.288 / N to first order)
    assert abs(errs[R.ARITHMETIC][1] - errs[R.ARITHMETIC][2]) <= CONDUCTION_TOL and 0.2 / N < errs[R.ARITHMETIC][2] < 0.4 / N, errs


def test_linear_conduction_follows_the_picard_model(gpu):
    """Gamma = gamma0 (1 + 2 phi) between phi = 0 and phi = 1: the device against the 1-D Picard model round for round, its rounds
    against the model's own stopping round, and the error ratio of N = 16 and 32 against the model's 3.64"""
    g0, beta = 0.7, 2.0
    p = R.params(R.LINEAR, R.ARITHMETIC, beta=beta)
    errs, model_errs = [], []
    for N in (16, 32):
        s, x, row = column(N, scalar_settings(diffusivity=g0, iterations=400, solver_type=CG, relative_convergence_threshold=1e-12,
                                              outer_tolerance=1e-8))
        s.set_scalar_diffusivity(gam(R.LINEAR, R.ARITHMETIC, beta=beta, phi_ref=0.0))
        rep = s.solve_scalar()
        phi = s.get_scalar_field()
        stop_phi, stop_rounds = R.linear_picard(N, LX, g0, p, tol=1e-8)
        model, _ = R.linear_picard(N, LX, g0, p, rounds=int(rep[0]))
        exact = R.linear_exact(x, LX, beta)
        errs.append(R.rel_l2(phi, exact))
        model_errs.append(R.rel_l2(stop_phi[row], exact))
        print("LINEAR conduction N = %d: rounds %d (model %d), |device - model| %.3e, relative L2 error %.6e (model %.6e)" %
              (N, rep[0], stop_rounds, np.abs(phi - model[row]).max(), errs[-1], model_errs[-1]))
        assert np.abs(phi - model[row]).max() <= CONDUCTION_TOL
        assert abs(int(rep[0]) - stop_rounds) <= 2 and rep[1] <= 1e-8, (rep, stop_rounds)
        assert same_bits(s.scalar_diffusivity(), R.law(p, g0, phi=phi))
    want = model_errs[0] / model_errs[1]
    assert abs(want - 3.64) <= 0.01
    assert abs(errs[0] / errs[1] - want) <= 0.1 * want, (errs, model_errs)


# ------------------------------------------------------------------ 5. the eddy diffusivity in a Smagorinsky BDF2 run
def test_eddy_diffusivity_follows_the_viscosity_through_time_steps(gpu):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.solver import Solver
    a = set_channel_bcs(hex_channel(12, 8, 4))
    m = Mesh(a)
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    start = (1e-3 * (1 + 0.1 * splitmix64_uniform(n, 1)), 1e-6 * splitmix64_uniform(n, 2), 1e-7 * splitmix64_uniform(n, 3),
             -0.01 * (1 - cc[:, 0] / 0.002))
    rho, mu, g0 = 1000.0, 1e-3, 5e-4
    p = R.params(R.EDDY, R.HARMONIC, schmidt_t=0.7)
    out = []
    for eddy in (False, True):
        s = Solver(m, settings(), rho, mu)  # the default stack: UMIST, Rhie-Chow, Multigrid arm
        s.set_fields(*start)
        s.set_viscosity(visc(VIS_SMAGORINSKY, cs=1.0))
        s.set_transient(transient(1e-3, 1, 2))  # BDF2
        s.set_scalar(scalar_settings(diffusivity=g0))
        s.set_scalar_bc("INLET", S.VALUE, 1.0)
        if eddy:
            s.set_scalar_diffusivity(gam(R.EDDY, R.HARMONIC, schmidt_t=0.7))
        steps = []
        for _ in range(2):
            rep = s.advance(1, report=True)
            gamma, mu_c = s.scalar_diffusivity(), s.viscosity()
            if eddy:
                assert same_bits(gamma, R.law(p, g0, mu=mu_c, mu_lam=mu))
                assert gamma.min() >= g0 and gamma.max() > g0 and len(np.unique(gamma)) > n // 2
            else:
                assert same_bits(gamma, np.full(n, g0))
            steps.append((rep, mu_c) + tuple(s.get_fields()))
        out.append((steps, s.get_scalar_field()))
    for on, off in zip(out[1][0], out[0][0]):
        for x, y in zip(on, off):
            assert same_bits(x, y)  # the flow's fields, reports and viscosity never see the scalar's model
    assert not same_bits(out[0][1], out[1][1])  # and the scalar does see it


# ------------------------------------------------------------------ 6. refusals
def test_refusals_change_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = a.n_cells
    flow = seeded_flow(a)
    nan, inf = float("nan"), float("inf")
    bad = [gam(-1), gam(4), gam(R.FIELD, 2), gam(R.LINEAR, -1), gam(R.CONSTANT, 2)]
    for model in (R.CONSTANT, R.FIELD, R.EDDY, R.LINEAR):
        for name in ("schmidt_t", "beta", "phi_ref", "gamma_min", "gamma_max", "reserved0"):
            for x in (nan, inf, -inf):
                bad.append(gam(model, **{name: x}))
        bad += [gam(model, schmidt_t=0.0), gam(model, schmidt_t=-0.7), gam(model, gamma_min=0.0), gam(model, gamma_min=-1.0),
                gam(model, gamma_min=2.0, gamma_max=1.0), gam(model, reserved0=1.0), gam(model, reserved0=-1e-300)]
    bad_fields = [np.zeros(n), np.full(n, -1.0), np.where(np.arange(n) == n - 1, nan, 1.0), np.where(np.arange(n) == 0, inf, 1.0)]
    # the scalar arm off: every entry refuses
    s = Solver(m, settings(velocity_interpolation=VINTERP_LINEAR), RHO, MU)
    assert s.set_scalar_diffusivity(gam(R.LINEAR, beta=1.0), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_scalar_diffusivity(None, raise_on_error=False) == BAD_ARGUMENT
    assert s.set_scalar_diffusivity_field(np.ones(n), raise_on_error=False) == BAD_ARGUMENT
    with pytest.raises(Exception):
        s.scalar_diffusivity()
    for on in (False, True):
        s, _, _ = make_solver(m, a, scalar_settings(scheme=S.TVD_UMIST, diffusivity=GAMMA0), CHANNEL_BCS, flow, rho=RHO, mu=MU)
        s.set_scalar_field(0.5 + 0.5 * splitmix64_uniform(n, 3))
        if on:
            s.set_scalar_diffusivity(gam(R.LINEAR, R.HARMONIC, beta=0.5, phi_ref=0.2))
        before = scalar_state(s) + (s.viscosity(),) + s.diffusion()
        for c in bad:
            assert s.set_scalar_diffusivity(c, raise_on_error=False) == BAD_ARGUMENT, [getattr(c, f) for f, _ in c._fields_]
        assert s.set_scalar_diffusivity(gam(R.FIELD), raise_on_error=False) == BAD_ARGUMENT  # FIELD without a field
        for f in bad_fields:
            assert s.set_scalar_diffusivity_field(f, raise_on_error=False) == BAD_ARGUMENT
        assert s.set_scalar_diffusivity(gam(R.FIELD), raise_on_error=False) == BAD_ARGUMENT  # the refused fields were not kept
        # EDDY needs the viscosity arm on with an eddy part: off, power law and Carreau are refused
        assert s.set_scalar_diffusivity(gam(R.EDDY), raise_on_error=False) == BAD_ARGUMENT
        for x, y in zip(before, scalar_state(s) + (s.viscosity(),) + s.diffusion()):
            assert same_bits(x, y)
        for model in (VIS_POWER_LAW, VIS_CARREAU):
            s.set_viscosity(visc(model, k=0.02, n=0.6, mu_min=1e-5, mu_max=1.0))
            assert s.set_scalar_diffusivity(gam(R.EDDY), raise_on_error=False) == BAD_ARGUMENT
            s.set_viscosity(None)
        for x, y in zip(before, scalar_state(s) + (s.viscosity(),) + s.diffusion()):
            assert same_bits(x, y)
    # while EDDY is on, the viscosity arm keeps a model with an eddy part
    s.set_viscosity_field(R.log_uniform(splitmix64_uniform(n, 5), 1e-4, 1e-2))
    s.set_viscosity(visc(VIS_FIELD))
    s.set_scalar_diffusivity(gam(R.EDDY, R.HARMONIC))
    before = scalar_state(s) + (s.viscosity(),) + s.diffusion()
    assert s.set_viscosity(None, raise_on_error=False) == BAD_ARGUMENT
    for model in (VIS_POWER_LAW, VIS_CARREAU):
        assert s.set_viscosity(visc(model, k=0.02, n=0.6, mu_min=1e-5, mu_max=1.0), raise_on_error=False) == BAD_ARGUMENT
    for x, y in zip(before, scalar_state(s) + (s.viscosity(),) + s.diffusion()):
        assert same_bits(x, y)
    s.set_viscosity(visc(VIS_SMAGORINSKY))  # allowed: it has an eddy part
    s.set_scalar_diffusivity(None)
    s.set_viscosity(None)  # and with EDDY off the arm may go


# ------------------------------------------------------------------ 7. repeatability
def test_two_solves_from_one_snapshot_give_the_same_bits(gpu, tmp_path):
    a, m, bcs = case_mesh(tmp_path, "poly")
    n = a.n_cells
    s, _, _ = make_solver(m, a, scalar_settings(scheme=S.TVD_UMIST, diffusivity=GAMMA0, outer_iterations=6), bcs, seeded_flow(a), rho=RHO, mu=MU)
    s.set_scalar_field(0.5 + 0.5 * splitmix64_uniform(n, 7))
    # the wall fluxes of ASSEMBLY_BCS drive phi to some tens: a small beta keeps Gamma inside the clamp, where it varies with phi
    s.set_scalar_diffusivity(gam(R.LINEAR, R.HARMONIC, beta=0.01, phi_ref=0.1, gamma_min=1e-5))
    s.snapshot()
    runs = []
    for _ in range(2):
        rep = s.solve_scalar()
        runs.append((rep,) + scalar_state(s))
        s.restore()
    for x, y in zip(*runs):
        assert same_bits(x, y)
    assert runs[0][0][0] > 1 and len(np.unique(runs[0][5])) > n // 2  # Picard rounds on a Gamma that varies


# ------------------------------------------------------------------ 8. the bench hook
def test_bench_hook_times_three_passes_and_changes_nothing(gpu):
    a, m = channel_flow()
    n = a.n_cells
    s, _, _ = make_solver(m, a, scalar_settings(scheme=S.TVD_UMIST, diffusivity=GAMMA0), CHANNEL_BCS, seeded_flow(a), rho=RHO, mu=MU)
    s.set_scalar_field(0.5 + 0.5 * splitmix64_uniform(n, 7))
    with pytest.raises(Exception):
        s.bench_scalar_diffusivity(2)  # no model is on
    s.set_scalar_diffusivity_field(R.log_uniform(splitmix64_uniform(n, 5), 1e-5, 1e-3))
    s.set_scalar_diffusivity(gam(R.FIELD, R.HARMONIC))
    s.solve_scalar()
    before = scalar_state(s)
    ms = s.bench_scalar_diffusivity(3)
    assert len(ms) == 3 and all(0 < t < 100 for t in ms), ms
    for x, y in zip(before, scalar_state(s)):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 9. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "scalar_diffusivity_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "SCALAR_DIFFUSIVITY_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
