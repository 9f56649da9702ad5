"""Variable viscosity (orc_solver_set_viscosity*, orc_amd/csrc/viscosity.hip) on the device: the plain solver's bits where the
viscosity is the constant, the diffusion rebuild bit for bit against tests/viscosity_restatement.py at the launch edges of the
XCD-contiguous block walk, the laws against their longdouble restatement at the strain rate of the derived fields, a two-layer
Couette flow with its wall shear, power-law and Carreau Poiseuille flow against the 1-D model, snapshots, argument checking and
two ranks on one GPU.

Bit for bit means equal uint64 views.  The tolerances are the issue's: 16 * 2^-52 relative for a law (g is exact; at most two
library calls and six roundings per formula, no cancellation for mu_zero > mu_inf >= 0), 1e-8 for the Couette profile and its wall
forces (the bar of tests/test_gpu_transient.py for the same flow), 1e-6 for the converged Poiseuille profiles.
Accuracy of the device's pow and cbrt: the ROCm documentation tree installed with the toolchain carries no accuracy table (it holds
licences and the runtime API reference only); the published HIP math API reference lists both at 1 ULP in double precision, i.e.
2^-52 relative each, well inside the sixteen units of the bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import viscosity_restatement as R
from conftest import ROOT, splitmix64_uniform
from test_gpu_surface import hex_case, mixed_case
from test_gpu_transient import channel_flow, poly_channel, poiseuille_start, settings, transient

pytestmark = pytest.mark.gpu

BICGSTAB = 3
BAD_ARGUMENT = 10
GREEN_GAUSS, LEAST_SQUARES = 0, 2
HGT, LX = 1e-3, 2e-3


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def visc(model, face=R.ARITHMETIC, **kw):
    from orc_amd.settings import Viscosity
    return Viscosity.make(model, face, **kw)


def field_solver(m, mu_field, face, rho=1000.0, mu=1e-3, **kw):
    from orc_amd.solver import Solver
    s = Solver(m, settings(**kw), rho, mu)
    s.set_viscosity_field(mu_field)
    s.set_viscosity(visc(R.FIELD, face))
    return s


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("face", [R.ARITHMETIC, R.HARMONIC], ids=["arithmetic", "harmonic"])
@pytest.mark.parametrize("mesh_name", ["channel_flow", "poly"])
def test_constant_field_is_the_plain_solver_bit_for_bit(gpu, tmp_path, mesh_name, face):
    from orc_amd.solver import Solver
    a, m = poly_channel(tmp_path) if mesh_name == "poly" else channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    rho, mu = 1000.0, 1e-3
    out = []
    for on in (False, True):
        s = Solver(m, settings(momentum=5), rho, mu)
        if on:
            s.set_viscosity_field(np.full(m.n_cells, mu))
            s.set_viscosity(visc(R.FIELD, face))
            assert same_bits(s.viscosity(), np.full(m.n_cells, mu))
        s.set_fields(*fields)
        asm = s.assemble_momentum()
        dif = s.diffusion()
        s.set_fields(*fields)
        st, rep = s.iterate(3, report=True)
        out.append((asm[:6], dif, s.get_fields(), rep))
    for k in range(3):
        for x, y in zip(out[0][k], out[1][k]):
            assert same_bits(x, y), (mesh_name, face, k)
    assert same_bits(out[0][3], out[1][3])


def test_switching_off_puts_the_constant_diffusion_back(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    fresh = Solver(m, settings(momentum=5), 1000.0, 1e-3)
    s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
    s.set_fields(*fields)
    s.set_viscosity(visc(R.POWER_LAW, R.HARMONIC, k=0.02, n=0.6, mu_min=1e-6, mu_max=1.0))
    assert not same_bits(s.diffusion()[0], fresh.diffusion()[0])
    s.iterate(1)
    s.set_viscosity(None)
    for x, y in zip(s.diffusion(), fresh.diffusion()):
        assert same_bits(x, y)
    assert same_bits(s.viscosity(), np.full(m.n_cells, 1e-3))
    assert s.evaluate_viscosity(raise_on_error=False)[0] == BAD_ARGUMENT  # no law to evaluate


def test_smagorinsky_with_cs_zero_is_the_plain_solver_through_the_law_kernel(gpu):
    """m = mu + (rho (l l)) g with l = 0 * cbrt(V) = 0: mu + 0 = mu exactly, in every SIMPLE iteration and BDF2 step"""
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    out = []
    for on in (False, True):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        s.set_fields(*fields)
        if on:
            s.set_viscosity(visc(R.SMAGORINSKY, R.HARMONIC, cs=0.0))
        st, rep = s.iterate(3, report=True)
        steady = s.get_fields()
        s.set_transient(transient(1e-3, 1, 2))
        adv = s.advance(2, report=True)
        out.append((steady, rep, s.get_fields(), adv))
        if on:
            assert same_bits(s.viscosity(), np.full(m.n_cells, 1e-3))
    for x, y in zip(out[0][0] + out[0][2], out[1][0] + out[1][2]):
        assert same_bits(x, y)
    assert same_bits(out[0][1], out[1][1]) and same_bits(out[0][3], out[1][3])


# ------------------------------------------------------------------ 2. the diffusion rebuild, bit for bit
# hex channels at the launch edges of a 256-thread block and of the XCD walk (on for a grid that is a multiple of 8)
REBUILD_MESHES = ["channel_flow", "poly", (15, 17, 1), (16, 16, 1), (257, 1, 1), (23, 89, 1), (81, 81, 80)]


@pytest.mark.parametrize("mesh_name", REBUILD_MESHES, ids=lambda s: s if isinstance(s, str) else "%dx%dx%d" % s)
def test_diffusion_rebuild_equals_the_restatement_bit_for_bit(gpu, tmp_path, mesh_name):
    if mesh_name == "channel_flow":
        a, m = channel_flow()
    elif mesh_name == "poly":
        a, m = mixed_case(tmp_path, True)  # every supported zone type, non-zero wall and inlet vectors
    else:
        a, m = hex_case(*mesh_name)
        assert m.n_cells == {(15, 17, 1): 255, (16, 16, 1): 256, (257, 1, 1): 257, (23, 89, 1): 2047, (81, 81, 80): 524880}[mesh_name]
    n = m.n_cells
    assert np.array_equal(m.cell_order(), np.arange(n))
    mu = R.log_uniform(splitmix64_uniform(n, 0x56495343), 1e-6, 1e2)
    assert mu.min() < 1e-5 and mu.max() > 10.0
    rp, ci = m.matrix_pattern()
    plain = None
    for face in (R.ARITHMETIC, R.HARMONIC):
        s = field_solver(m, mu, face, momentum=5)
        if plain is None:
            plain = field_solver(m, np.full(n, 1e-3), face, momentum=5).diffusion()
        got = s.diffusion()
        want = R.diffusion(a, mu, face, rp, ci)
        assert same_bits(s.viscosity(), mu)
        for k, (x, y) in enumerate(zip(got, want)):
            assert same_bits(x, y), (mesh_name, face, k, int(np.count_nonzero(x != y)))
        assert not same_bits(got[0], plain[0])
        if mesh_name != "channel_flow":  # walls at rest there: the wall terms are zeros
            assert np.abs(got[1]).max() > 0
    # the two modes differ, and a later assembly rebuilds the same bits (the rebuild runs ahead of every assembly)
    assert not same_bits(R.diffusion(a, mu, R.ARITHMETIC, rp, ci)[0], want[0])
    s.assemble_momentum_only()
    for x, y in zip(s.diffusion(), want):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 3. the laws
def law_fields(a):
    """H.rough_fields, and the same with the velocity at rest in the upstream half: g = 0 exactly there"""
    cc = np.asarray(a["cell_centroid"])
    rough = H.rough_fields(cc)
    rest = cc[:, 0] < 0.5 * LX
    patch = tuple(np.where(rest, 0.0, f) for f in rough[:3]) + (rough[3],)
    return {"rough": rough, "patch": patch}


@pytest.mark.parametrize("arm", [GREEN_GAUSS, LEAST_SQUARES], ids=["green_gauss", "least_squares"])
@pytest.mark.parametrize("mesh_name", ["channel_flow", "poly"])
def test_laws_at_the_derived_strain_rate(gpu, tmp_path, mesh_name, arm):
    from orc_amd.solver import Solver
    a, m = poly_channel(tmp_path) if mesh_name == "poly" else channel_flow()
    vol = np.asarray(a["cell_volume"])
    rho, mu_lam = 1000.0, 1e-3
    for name, f in law_fields(a).items():
        s = Solver(m, settings(momentum=5, gradient_reconstruction=arm), rho, mu_lam)
        s.set_fields(*f)
        g = s.derived_fields("strain_rate_mag")["strain_rate_mag"]
        assert np.all(np.isfinite(g)) and g.max() > 0
        if name == "patch":
            assert np.count_nonzero(g == 0.0) > 10
        pos = g[g > 0]
        # clamps inside the range of the unclamped law, so that both are hit (and, with g = 0 and n < 1, pow's +inf)
        pl = R.params(R.POWER_LAW, k=0.02, n=0.5)
        raw = R.law(dict(pl, mu_min=1e-300, mu_max=1e300), pos)
        laws = [dict(pl, mu_min=float(np.quantile(raw, 0.2)), mu_max=float(np.quantile(raw, 0.8))),
                R.params(R.POWER_LAW, k=0.02, n=1.5, mu_min=float(np.quantile(0.02 * np.sqrt(pos), 0.2)), mu_max=float(np.quantile(0.02 * np.sqrt(pos), 0.8))),
                R.params(R.CARREAU, mu_zero=0.056, mu_inf=0.0035, lambda_=float(1.0 / np.median(pos)), n=0.3568),
                R.params(R.SMAGORINSKY, cs=0.17, mu_max=float(np.quantile(mu_lam + rho * (0.17 * np.cbrt(vol)) ** 2 * g, 0.9)))]
        for p in laws:
            v = visc(p["model"], R.HARMONIC, **{k: p[k] for k in p if k != "model"})
            s.set_viscosity(v)
            mu, g_dev = s.evaluate_viscosity()
            assert same_bits(g_dev, g), (mesh_name, arm, name, p["model"])
            want = R.law(p, g, vol, rho, mu_lam, dtype=np.longdouble)
            err = np.abs(mu.astype(np.longdouble) - want) / want
            print("%s %s arm %d model %d: worst error %.2f x 2^-52, clamped low %d high %d of %d" % (
                mesh_name, name, arm, p["model"], float(err.max()) / R.EPS, np.count_nonzero(mu == p["mu_min"]),
                np.count_nonzero(mu == p["mu_max"]), len(mu)))
            assert float(err.max()) <= 16 * R.EPS, (mesh_name, arm, name, p["model"], float(err.max()) / R.EPS)
            assert same_bits(s.viscosity(), mu)  # the set call evaluated the same law on the same fields
            if p["model"] != R.CARREAU:
                assert np.count_nonzero(mu == p["mu_max"]) > 0
            if p["model"] == R.POWER_LAW:
                assert np.count_nonzero(mu == p["mu_min"]) > 0
                if p["n"] < 1 and name == "patch":
                    assert np.all(mu[g == 0.0] == p["mu_max"])
        # n = 1: k (clamped) everywhere, g = 0 included
        s.set_viscosity(visc(R.POWER_LAW, k=0.02, n=1.0))
        assert same_bits(s.evaluate_viscosity()[0], np.full(m.n_cells, 0.02))
        s.set_viscosity(visc(R.POWER_LAW, k=0.02, n=1.0, mu_max=0.01))
        assert same_bits(s.evaluate_viscosity()[0], np.full(m.n_cells, 0.01))


def test_relaxation_after_two_assemblies(gpu):
    """the first evaluation of an assembly after set_viscosity takes the law's value, the second is relaxed: mu0 + w (m - mu0)"""
    from orc_amd.solver import Solver
    a, m = channel_flow()
    f = law_fields(a)
    s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
    s.set_fields(*f["patch"])
    s.set_viscosity(visc(R.POWER_LAW, R.ARITHMETIC, k=0.02, n=0.6, mu_min=1e-4, mu_max=5.0, relaxation=0.5))
    s.assemble_momentum_only()
    mu0 = s.viscosity()
    assert same_bits(mu0, s.evaluate_viscosity()[0])
    s.set_fields(*f["rough"])
    m_new = s.evaluate_viscosity()[0]
    assert same_bits(s.viscosity(), mu0)  # evaluating changes no state
    s.assemble_momentum_only()
    got = s.viscosity()
    assert same_bits(got, mu0 + 0.5 * (m_new - mu0))
    assert not same_bits(got, m_new) and not same_bits(got, mu0)
    rp, ci = m.matrix_pattern()
    for x, y in zip(s.diffusion(), R.diffusion(a, got, R.ARITHMETIC, rp, ci)):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 4. two-layer Couette
# rho = mu1 = 1 and U = 1e-6 m/s as the start-up Couette of tests/test_gpu_transient.py: the pressure inlet's momentum deficit is
# second order in U and below every tolerance here
def couette(face):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.solver import Solver
    u_top, mu1 = 1e-6, 1.0
    a = set_channel_bcs(hex_channel(4, 16, 1), top_wall_velocity=u_top, dp_dx=0.0)
    m = Mesh(a)
    y = np.asarray(a["cell_centroid"])[:, 1]
    mu = np.where(y < HGT / 2, mu1, 4 * mu1)
    s = Solver(m, settings(momentum=0, solver_type=BICGSTAB, iterations=100, relative_convergence_threshold=1e-13), 1.0, mu1)
    z = np.zeros(m.n_cells)
    s.set_fields(z, z, z, z)
    s.set_viscosity_field(mu)
    s.set_viscosity(visc(R.FIELD, face))
    s.iterate(4)
    exact, tau = R.two_layer_couette(y, HGT, mu1, 4 * mu1, u_top)
    return a, s, exact, tau


def test_two_layer_couette_profile_and_wall_shear(gpu):
    a, s, exact, tau = couette(R.HARMONIC)
    u, v, w, p = s.get_fields()
    err = H.rel_l2(u, exact)
    print("two-layer Couette, harmonic: rel-L2 %.2e" % err)
    assert err <= 1e-8, err
    rep = s.surface_report()
    bf = s.boundary_fields(["traction_x", "shear_mag"])
    for name, sign in (("TOP_WALL", -1.0), ("BOTTOM_WALL", 1.0)):
        z = a.get_face_zone(name)
        want = sign * tau * rep.area[z]
        assert abs(rep.area[z] - LX * 1e-4) <= 1e-12 * rep.area[z]
        assert abs(rep.viscous_force[z, 0] - want) <= 1e-8 * abs(want), (name, rep.viscous_force[z], want)
        t = bf.zone(name)
        assert len(t["traction_x"]) == 4
        assert np.all(np.abs(t["traction_x"] - sign * tau) <= 1e-8 * tau), (name, t["traction_x"], tau)
        assert np.all(np.abs(t["shear_mag"] - tau) <= 1e-8 * tau)
    # with the solver's constant mu (= mu1) the top wall, which lies in the 4 mu1 layer, would report a quarter of its force
    from orc_amd.solver import surface_integrals
    const = surface_integrals(s.mesh, u, v, w, p, 1.0, 1.0)
    zt = a.get_face_zone("TOP_WALL")
    assert abs(const.viscous_force[zt, 0] * 4 - rep.viscous_force[zt, 0]) <= 1e-8 * abs(rep.viscous_force[zt, 0])


def test_two_layer_couette_arithmetic_is_off(gpu):
    a, s, exact, tau = couette(R.ARITHMETIC)
    err = H.rel_l2(s.get_fields()[0], exact)
    print("two-layer Couette, arithmetic: rel-L2 %.2e (1.08e-2 in the 1-D model)" % err)
    assert err > 1e-3 and abs(err - 1.08e-2) < 1e-3, err


# ------------------------------------------------------------------ 5. power-law and Carreau Poiseuille against the 1-D model
# G = 5 Pa/m over h = 0.5 mm: the wall stress is G h = 2.5e-3 Pa.  k is chosen so that the wall viscosity is ~1 Pa s
# (g_w = 2.5e-3 / s); with rho = 1e-3 and the clamp's floor of 0.02 the cell Reynolds number rho |u| dy / mu stays below
# 1e-3 * (G h^2 / (2 * 0.02)) * 3.1e-5 / 0.02 = 4.9e-11 even while the viscosity sits on the floor.
# Velocity interpolation: Linear.  With Rhie-Chow the solver's own start-up at the inlet and outlet columns — the constant-mu solver
# shows it from this very start, arm off: p moves 8.4e-3 of the inlet pressure away from the linear field within 60 iterations, |v| is
# 8e-4 |u| — decays at the default pressure relaxation of 0.01 over thousands of iterations (2.8e-5 per iteration after 60), so the
# change of u never comes near 1e-10 within a test's seconds, whatever the viscosity.  With Linear face velocities the flow of this
# start is one-dimensional to round-off (p within 2e-14, |v| < 1e-14 |u|) and the iteration is the model's Picard iteration.
LINEAR_VELOCITY = 0  # settings.VelocityInterpolation.Linear
NY_P = 32
POISEUILLE = {"power_law_n0.5": R.params(R.POWER_LAW, k=0.05, n=0.5, mu_min=0.02, mu_max=1e3, relaxation=0.5),
              "power_law_n1.5": R.params(R.POWER_LAW, k=20.0, n=1.5, mu_min=0.02, mu_max=1e3, relaxation=0.5),
              "carreau": R.params(R.CARREAU, mu_zero=4.0, mu_inf=0.5, lambda_=400.0, n=0.5, mu_min=0.02, mu_max=1e3, relaxation=0.5)}


@pytest.mark.parametrize("case", list(POISEUILLE))
def test_poiseuille_converges_to_the_one_dimensional_model(gpu, case):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.solver import Solver
    p = POISEUILLE[case]
    rho, mu_lam, G = 1e-3, 1.0, 5.0
    a = set_channel_bcs(hex_channel(8, NY_P, 1))
    m = Mesh(a)
    s = Solver(m, settings(momentum=0, solver_type=BICGSTAB, iterations=100, relative_convergence_threshold=1e-13,
                           velocity_interpolation=LINEAR_VELOCITY), rho, mu_lam)
    s.set_fields(*poiseuille_start(a))
    s.set_viscosity(visc(p["model"], R.ARITHMETIC, **{k: p[k] for k in p if k != "model"}))
    u_old, rounds, change = np.zeros(m.n_cells), 0, np.inf
    cap = 300
    while rounds < cap:
        s.iterate(1)
        rounds += 1
        u = s.get_fields()[0]
        change = np.linalg.norm(u - u_old) / max(np.linalg.norm(u), 1e-300)
        u_old = u
        if change < 1e-10:
            break
    assert change < 1e-10, (case, rounds, change)  # the cap fails the test
    mu = s.viscosity()
    y = np.asarray(a["cell_centroid"])[:, 1]
    dy = HGT / NY_P
    assert rho * np.abs(u).max() * dy / mu.min() <= 1e-10
    u1, mu1, it = R.channel_picard(p, R.ARITHMETIC, NY_P, HGT, G, w=0.5, tol=1e-13, mu_lam=mu_lam, rho=rho)
    assert it < 400
    row = np.floor(y / dy).astype(int)
    err = H.rel_l2(u, -u1[row])  # set_channel_bcs drives the flow towards -x
    err_mu = H.rel_l2(mu, mu1[row])
    print("%s: %d iterations, u rel-L2 %.2e, mu rel-L2 %.2e against the 1-D model (%d Picard rounds)" % (case, rounds, err, err_mu, it))
    assert err <= 1e-6, (case, err)
    if p["model"] == R.POWER_LAW:  # and the model itself follows the analytic profile (tests/test_viscosity_cpu.py: second order)
        assert H.rel_l2(u1, R.power_law_profile((np.arange(NY_P) + 0.5) * dy, HGT, G, p["k"], p["n"])) < 1e-2


# ------------------------------------------------------------------ 6. snapshots
def test_snapshot_restore_and_repeatability(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    v = visc(R.POWER_LAW, R.HARMONIC, k=0.02, n=0.6, mu_min=1e-5, mu_max=1.0, relaxation=0.5)
    runs = []
    for _ in range(2):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        s.set_fields(*fields)
        s.set_viscosity(v)
        s.snapshot()  # the next evaluation is the first one: the flag travels with the snapshot
        s.iterate(1)
        first = s.get_fields() + (s.viscosity(),)
        s.restore()
        s.iterate(1)
        for x, y in zip(first, s.get_fields() + (s.viscosity(),)):
            assert same_bits(x, y)
        s.iterate(1)
        s.snapshot()
        st, r1 = s.iterate(2, report=True)
        f1 = s.get_fields() + (s.viscosity(),) + s.diffusion()
        s.restore()
        st, r2 = s.iterate(2, report=True)
        f2 = s.get_fields() + (s.viscosity(),) + s.diffusion()
        assert same_bits(r1, r2)
        for x, y in zip(f1, f2):
            assert same_bits(x, y)
        runs.append(f2)
    for x, y in zip(*runs):
        assert same_bits(x, y)
    assert not same_bits(runs[0][4], np.full(m.n_cells, 1e-3))


def test_bench_hook_times_both_passes_and_changes_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
    s.set_fields(*H.rough_fields(np.asarray(a["cell_centroid"])))
    with pytest.raises(Exception):
        s.bench_viscosity(2)  # the arm is off
    s.set_viscosity(visc(R.POWER_LAW, R.HARMONIC, k=0.02, n=0.6, mu_min=1e-5, mu_max=1.0, relaxation=0.5))
    s.iterate(1)
    before = s.get_fields() + (s.viscosity(),) + s.diffusion()
    cell_ms, rebuild_ms = s.bench_viscosity(3)
    assert 0 < cell_ms < 100 and 0 < rebuild_ms < 100
    for x, y in zip(before, s.get_fields() + (s.viscosity(),) + s.diffusion()):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 7. arguments
def test_refusals_change_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = m.n_cells
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    nan, inf = float("nan"), float("inf")
    good = dict(k=0.02, n=0.6, mu_min=1e-5, mu_max=1.0, relaxation=0.5)
    bad = [visc(0), visc(5), visc(-1), visc(R.POWER_LAW, 2), visc(R.POWER_LAW, -1)]
    for model in (R.POWER_LAW, R.CARREAU, R.SMAGORINSKY):
        for name in ("k", "n", "mu_zero", "mu_inf", "lambda_", "cs", "mu_min", "mu_max", "relaxation"):
            for x in (nan, inf, -inf):
                bad.append(visc(model, **{name: x}))
        bad += [visc(model, cs=-1e-3), visc(model, mu_min=0.0), visc(model, mu_min=-1.0), visc(model, mu_min=2.0, mu_max=1.0),
                visc(model, relaxation=0.0), visc(model, relaxation=-0.5), visc(model, relaxation=1.0 + 1e-12)]
    bad += [visc(R.POWER_LAW, k=0.0), visc(R.POWER_LAW, k=-1.0), visc(R.CARREAU, mu_zero=-1.0), visc(R.CARREAU, mu_inf=-1.0),
            visc(R.CARREAU, lambda_=-1.0)]
    bad_fields = [np.zeros(n), np.full(n, -1.0), np.where(np.arange(n) == n - 1, nan, 1.0), np.where(np.arange(n) == 0, inf, 1.0)]
    for on in (False, True):
        s = Solver(m, settings(momentum=5), 1000.0, 1e-3)
        s.set_fields(*fields)
        if on:
            s.set_viscosity(visc(R.POWER_LAW, R.HARMONIC, **good))
        before = (s.viscosity(),) + s.diffusion()
        for v in bad:
            assert s.set_viscosity(v, raise_on_error=False) == BAD_ARGUMENT, [getattr(v, f) for f, _ in v._fields_]
        assert s.set_viscosity(visc(R.FIELD), raise_on_error=False) == BAD_ARGUMENT  # FIELD without a field
        for mu in bad_fields:
            assert s.set_viscosity_field(mu, raise_on_error=False) == BAD_ARGUMENT
        assert s.set_viscosity(visc(R.FIELD), raise_on_error=False) == BAD_ARGUMENT  # the refused fields were not kept
        for x, y in zip(before, (s.viscosity(),) + s.diffusion()):
            assert same_bits(x, y)
    s = Solver(m, settings(momentum=5, frozen_diagonals=0), 1000.0, 1e-3)
    before = s.diffusion()
    s.set_viscosity_field(np.full(n, 1e-3))
    assert s.set_viscosity(visc(R.FIELD), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_viscosity(visc(R.POWER_LAW, **good), raise_on_error=False) == BAD_ARGUMENT
    for x, y in zip(before, s.diffusion()):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 8. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "viscosity_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "VISCOSITY_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
