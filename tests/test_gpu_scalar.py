"""Passive scalar transport (orc_solver_set_scalar and companions) on the device: the assembled system against the numpy
restatement (tests/scalar_restatement.py), conduction between plates, plug-flow convection-diffusion and its observed
orders, the TVD arm, boundedness on a mixed mesh, conservation, transient conduction and its temporal orders, the flow left
untouched, the solver arms, argument checking and two ranks on one GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scalar_restatement as R
from conftest import ROOT, splitmix64_uniform

pytestmark = pytest.mark.gpu

JACOBI, MULTIGRID, BICGSTAB, GMRES = 1, 2, 3, 19
LINEAR, RHIE_CHOW = 0, 2
BAD_ARGUMENT, UNSUPPORTED_SCHEME = 10, 8


def settings(**kw):
    from orc_amd.settings import NumericalSettings
    return NumericalSettings.default(**kw)


def scalar_settings(**kw):
    from orc_amd.settings import ScalarSettings
    return ScalarSettings.default(**kw)


def set_zone_types(a, types):
    """types: {zone name: (OrcFaceConditionType, vector)}; a name ending in '*' also sets its '_TRI' twin"""
    for name in list(a["zone_names"]):
        base = name[:-4] if name.endswith("_TRI") else name
        for key, (zt, vec) in types.items():
            if base == key or (key.endswith("*") and base.startswith(key[:-1])):
                a.set_zone(name, zt, 0.0, vec)
    return a


def hex_mesh(nx, ny, nz, ordering=None, lx=0.002, ly=0.001, lz=None, types=None):
    from orc_amd.mesh import Mesh, hex_channel
    a = hex_channel(nx, ny, nz, lx=lx, ly=ly, lz=lz)
    if types:
        set_zone_types(a, types)
    return a, Mesh(a, ordering=ordering)


def mixed_mesh(tmp_path, polyhedra, types=None):
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays, set_mixed_channel_bcs, write_mixed_channel_msh
    path = str(tmp_path / ("poly.msh" if polyhedra else "mixed.msh"))
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=polyhedra)
    a = set_mixed_channel_bcs(MeshArrays(orc_io.read_mesh(path).arrays()))
    if types:
        set_zone_types(a, types)
    return a, Mesh(a)


ASSEMBLY_TYPES = {"INLET": (R.VELOCITY_INLET, (0.4, 0.05, 0.0)), "OUTLET": (R.PRESSURE_OUTLET, (0, 0, 0)),
                  "PERIODIC*": (R.SYMMETRY, (0, 0, 0)), "TOP_WALL": (R.WALL, (0, 0, 0)), "BOTTOM_WALL": (R.WALL, (0, 0, 0)),
                  "WALL": (R.WALL, (0, 0, 0))}
# every kind: explicit VALUE, FLUX and ZERO_GRADIENT and the DEFAULT of each flow zone type present
ASSEMBLY_BCS = {"INLET": (R.VALUE, 0.3), "TOP_WALL": (R.FLUX, 2.0), "BOTTOM_WALL": (R.VALUE, 1.0), "PERIODIC_-Z": (R.ZERO_GRADIENT, 0.0),
                "WALL": (R.FLUX, -1.5)}


def scalar_bcs(a, bcs):
    """(kinds, values) per zone from {name: (kind, value)}; names also match their '_TRI' twins; the rest DEFAULT"""
    names = list(a["zone_names"])
    k, v = np.zeros(len(names), np.int64), np.zeros(len(names))
    for z, name in enumerate(names):
        base = name[:-4] if name.endswith("_TRI") else name
        if base in bcs:
            k[z], v[z] = bcs[base]
    return k, v


def make_solver(m, a, sc, bcs, flow=None, rho=1.3, mu=1e-3, vinterp=LINEAR, **flow_kw):
    from orc_amd.solver import Solver
    s = Solver(m, settings(velocity_interpolation=vinterp, **flow_kw), rho, mu)
    if flow is not None:
        s.set_fields(*flow)
    s.set_scalar(sc)
    k, v = scalar_bcs(a, bcs)
    for z in range(len(k)):
        if k[z] != R.DEFAULT:
            s.set_scalar_bc(z, int(k[z]), float(v[z]))
    return s, k, v


def seeded_flow(a, scale=0.05):
    n = a.n_cells
    return (scale * (1 + 0.5 * splitmix64_uniform(n, 1)), 0.3 * scale * splitmix64_uniform(n, 2),
            0.2 * scale * splitmix64_uniform(n, 3), 0.01 * splitmix64_uniform(n, 4))


# ------------------------------------------------------------------ 1. exact assembly
@pytest.mark.parametrize("mesh_name", ["hex", "hex_rcm", "poly"])
def test_assembly_equals_the_restatement(gpu, tmp_path, mesh_name):
    from orc_amd.settings import Transient
    if mesh_name == "poly":
        a, m = mixed_mesh(tmp_path, True, ASSEMBLY_TYPES)
    else:
        a, m = hex_mesh(8, 6, 4, ordering=1 if mesh_name == "hex_rcm" else None, types=ASSEMBLY_TYPES)
    exact = mesh_name != "hex_rcm"  # the renumbered mesh visits a cell's faces in another order: sums round differently
    n = a.n_cells
    g = m.cell_order()
    rp, ci = m.matrix_pattern()
    flow = seeded_flow(a)
    rho, gamma = 1.3, 2.5e-4
    phi = 0.5 + 0.5 * splitmix64_uniform(n, 7)
    src = 3.0 * splitmix64_uniform(n, 8)
    lv = [phi * (1 + 0.1 * splitmix64_uniform(n, 9)), phi * (1 - 0.1 * splitmix64_uniform(n, 10))]
    flux = R.face_flux_linear(a, *flow[:3])
    cases = [(sch, None) for sch in (R.UD, R.CD1, R.TVD_LUD, R.TVD_QUICK, R.TVD_UMIST, R.TVD_UD, R.TVD_CD1)]
    cases += [(R.TVD_UMIST, (R.EULER, 1)), (R.CD1, (R.BDF2, 2)), (R.UD, (R.BDF2, 1))]
    dt = 2.7e-3
    for sch, tm in cases:
        s, k, v = make_solver(m, a, scalar_settings(scheme=sch, diffusivity=gamma), ASSEMBLY_BCS, flow, rho=rho)
        kr, vr = R.resolve_bcs(a["zone_type"], k, v)
        s.set_scalar_field(phi)
        s.set_scalar_source(src)
        time = None
        if tm:
            s.set_transient(Transient.make(dt, tm[0], 1))
            s.set_scalar_levels(lv[0], lv[1] if tm[1] == 2 else None)
            time = (dt, tm[0], lv[0], lv[1] if tm[1] == 2 else None)
        got_a, got_b = s.assemble_scalar()
        rows, cols, vals, b = R.assemble(a, flux, rho, gamma, sch, kr, vr, phi=phi, source=src, time=time)
        want_a, want_b = R.on_pattern(rows, cols, vals, rp, ci, g), b[g]
        if exact:
            assert np.array_equal(got_a, want_a), (mesh_name, sch, tm, np.abs(got_a - want_a).max())
            assert np.array_equal(got_b, want_b), (mesh_name, sch, tm, np.abs(got_b - want_b).max())
        else:
            assert np.all(np.abs(got_a - want_a) <= 1e-14 * np.abs(want_a)), (sch, tm)
            # b sums terms of both signs: 1e-14 of its largest entry
            assert np.all(np.abs(got_b - want_b) <= 1e-14 * np.abs(want_b).max()), (sch, tm)


# ------------------------------------------------------------------ 2. conduction between plates
def test_conduction_between_plates_is_linear(gpu):
    a, m = hex_mesh(2, 16, 2)  # every boundary zone a wall: no flow, DEFAULT = adiabatic
    z = np.zeros(a.n_cells)
    s, _, _ = make_solver(m, a, scalar_settings(diffusivity=0.7, iterations=200), {"BOTTOM_WALL": (R.VALUE, 0.0), "TOP_WALL": (R.VALUE, 1.0)},
                          (z, z, z, z))
    rep = s.solve_scalar()
    phi = s.get_scalar_field()
    y = np.asarray(a["cell_centroid"])[:, 1]
    assert np.abs(phi - y / 0.001).max() <= 1e-9, np.abs(phi - y / 0.001).max()
    assert rep[0] == 1 and abs(rep[2] - phi.min()) == 0 and rep[3] == phi.max()


# ------------------------------------------------------------------ 3.-4. plug flow
PLUG_TYPES = {"INLET": (R.VELOCITY_INLET, (1.0, 0.0, 0.0)), "OUTLET": (R.PRESSURE_OUTLET, (0, 0, 0)),
              "PERIODIC*": (R.SYMMETRY, (0, 0, 0)), "TOP_WALL": (R.SYMMETRY, (0, 0, 0)), "BOTTOM_WALL": (R.SYMMETRY, (0, 0, 0)),
              "WALL": (R.SYMMETRY, (0, 0, 0))}
PLUG_BCS = {"INLET": (R.VALUE, 0.0), "OUTLET": (R.VALUE, 1.0)}
LX = 0.002


def plug_solve(N, scheme, **kw):
    a, m = hex_mesh(N, 1, 1, lx=LX, types=PLUG_TYPES)
    n = a.n_cells
    u = np.ones(n)
    z = np.zeros(n)
    gamma = 1.0 * 1.0 * LX / R.PLUG_PE
    s, _, _ = make_solver(m, a, scalar_settings(scheme=scheme, diffusivity=gamma, **kw), PLUG_BCS, (u, z, z, z), rho=1.0)
    rep = s.solve_scalar()
    x = np.asarray(a["cell_centroid"])[:, 0]
    return s.get_scalar_field(), x, rep


@pytest.mark.parametrize("scheme", [R.UD, R.CD1])
def test_plug_flow_profile_and_observed_order(gpu, scheme):
    errs = []
    for N in R.PLUG_N:
        phi, x, _ = plug_solve(N, scheme)
        A1, b1 = R.fv1d(N, LX, 1.0, LX / R.PLUG_PE, 1.0, scheme, 0.0, 1.0)
        assert np.abs(phi - np.linalg.solve(A1, b1)).max() <= 1e-10  # the 1-D finite-volume model
        errs.append(np.abs(phi - R.plug_flow_exact(x, LX, R.PLUG_PE)).max())
    lo, hi = R.ORDER_BAND[scheme]
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), (errs, order)


def test_tvd_arms_on_plug_flow(gpu):
    N = 40
    ud, _, _ = plug_solve(N, R.UD)
    tud1, _, rep1 = plug_solve(N, R.TVD_UD, outer_iterations=1)
    assert rep1[0] == 1 and np.array_equal(tud1, ud)  # psi = 0: the deferred correction is exactly zero
    tud, _, _ = plug_solve(N, R.TVD_UD)
    assert np.abs(tud - ud).max() <= 1e-12
    cd1, _, _ = plug_solve(N, R.CD1)
    tcd1, _, rep = plug_solve(N, R.TVD_CD1, outer_tolerance=1e-11, outer_iterations=60)
    assert rep[0] < 60 and rep[1] <= 1e-11, rep
    assert np.linalg.norm(tcd1 - cd1) <= 1e-9 * np.linalg.norm(cd1), np.linalg.norm(tcd1 - cd1)
    umist, _, rep = plug_solve(N, R.TVD_UMIST, outer_tolerance=1e-10, outer_iterations=60)
    assert rep[1] <= 1e-10, rep
    assert umist.min() >= -1e-10 and umist.max() <= 1.0 + 1e-10, (umist.min(), umist.max())
    assert rep[2] == umist.min() and rep[3] == umist.max()


# ------------------------------------------------------------------ 5. boundedness on the mixed tet / prism / hex mesh
def test_ud_plug_flow_on_the_mixed_mesh_is_bounded(gpu, tmp_path):
    a, m = mixed_mesh(tmp_path, False, PLUG_TYPES)
    n = a.n_cells
    z = np.zeros(n)
    gamma = LX / R.PLUG_PE
    s, _, _ = make_solver(m, a, scalar_settings(diffusivity=gamma), PLUG_BCS, (np.ones(n), z, z, z), rho=1.0)
    s.solve_scalar()
    phi = s.get_scalar_field()
    assert phi.min() >= -1e-12 and phi.max() <= 1.0 + 1e-12, (phi.min(), phi.max())
    assert phi.max() - phi.min() > 0.5  # a real profile between the two boundary values


# ------------------------------------------------------------------ 6. conservation on the polyhedral channel
def test_conservation_with_rhie_chow_and_a_source(gpu, tmp_path):
    from orc_amd.solver import Solver
    a, m = mixed_mesh(tmp_path, True)
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    s = Solver(m, settings(momentum=1, solver_type=BICGSTAB), 1000.0, 1e-3)
    s.set_fields(1e-3 * (1 + 0.1 * splitmix64_uniform(n, 1)), 1e-6 * splitmix64_uniform(n, 2), 1e-6 * splitmix64_uniform(n, 3),
                 -0.01 * (1 - cc[:, 0] / 0.002))
    s.iterate(3)
    s.set_scalar(scalar_settings(diffusivity=2e-3, iterations=800))
    s.set_scalar_bc("INLET", R.VALUE, 1.0)
    src = 50.0 * (1.5 + splitmix64_uniform(n, 5))
    s.set_scalar_source(src)
    s.solve_scalar()
    bf = s.scalar_boundary_flux()
    sv = float((src * np.asarray(a["cell_volume"])).sum())
    scale = np.abs(bf).sum() + abs(sv)
    assert abs(bf.sum() + sv) <= 1e-8 * scale, (bf, sv)
    assert bf[0] == 0.0  # the interior zone


# ------------------------------------------------------------------ 7. transient conduction
NY, HY, ALPHA = 32, 1.0, 1.0


def slab():
    a, m = hex_mesh(1, NY, 1, lx=1.0, ly=HY, lz=1.0)  # every zone a wall: no flow
    return a, m


def slab_solver(m, a, scheme, dt):
    from orc_amd.settings import Transient
    z = np.zeros(a.n_cells)
    s, _, _ = make_solver(m, a, scalar_settings(diffusivity=ALPHA, iterations=80), {"BOTTOM_WALL": (R.VALUE, 0.0), "TOP_WALL": (R.VALUE, 0.0)},
                          (z, z, z, z), rho=1.0, solver_type=BICGSTAB)
    s.set_transient(Transient.make(dt, scheme, 1))
    return s


def row_of(a):
    return np.floor(np.asarray(a["cell_centroid"])[:, 1] / (HY / NY)).astype(int)


def slab_march(m, a, scheme, dt, steps):
    s = slab_solver(m, a, scheme, dt)
    phi = np.ones(a.n_cells)
    s.set_scalar_field(phi)
    prev = None
    for _ in range(steps):
        s.set_scalar_levels(phi, prev if scheme == R.BDF2 else None)
        s.solve_scalar()
        prev, phi = phi, s.get_scalar_field()
    return phi


@pytest.mark.parametrize("scheme", [R.EULER, R.BDF2])
def test_transient_conduction_series_and_temporal_order(gpu, scheme):
    a, m = slab()
    K = R.conduction_operator(NY, HY, ALPHA)
    T = 0.05 * HY ** 2 / ALPHA
    rows = row_of(a)
    errs = []
    for steps in (20, 40, 80):
        phi = slab_march(m, a, scheme, T / steps, steps)
        model = R.march(K, np.ones(NY), T / steps, steps, scheme)
        assert np.abs(phi - model[rows]).max() <= 1e-11
        errs.append(np.abs(phi - R.semi_discrete(K, np.ones(NY), T)[rows]).max())
    lo, hi = R.TIME_ORDER_BAND[scheme]
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), (errs, order)
    # and the series: the spatial error of 32 cells at this time
    assert np.abs(phi - R.slab_series(np.asarray(a["cell_centroid"])[:, 1], T, HY, ALPHA)).max() < 2e-3


def test_advance_shifts_the_scalar_levels_and_snapshots_cover_them(gpu):
    a, m = slab()
    dt, steps = 2e-3, 4
    want = slab_march(m, a, R.BDF2, dt, steps)
    s = slab_solver(m, a, R.BDF2, dt)
    s.set_scalar_field(np.ones(a.n_cells))
    s.advance(steps)
    assert np.array_equal(s.get_scalar_field(), want)
    assert s.last_scalar_report()[3] == want.max()
    s.snapshot()
    s.advance(2)
    f1, r1 = s.get_scalar_field(), s.last_scalar_report()
    s.restore()
    s.advance(2)
    assert np.array_equal(s.get_scalar_field(), f1) and np.array_equal(s.last_scalar_report(), r1)


# ------------------------------------------------------------------ 8. the flow is untouched
def test_scalar_solves_leave_the_flow_bit_identical(gpu):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.solver import Solver
    a = set_channel_bcs(hex_channel(12, 8, 4))
    m = Mesh(a)
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    start = (1e-3 * (1 + 0.1 * splitmix64_uniform(n, 1)), 1e-6 * splitmix64_uniform(n, 2), 1e-7 * splitmix64_uniform(n, 3),
             -0.01 * (1 - cc[:, 0] / 0.002))
    out = []
    for with_scalar in (False, True):
        s = Solver(m, settings(), 1000.0, 1e-3)  # the default stack: UMIST, Rhie-Chow, Multigrid arm
        s.set_fields(*start)
        reps = []
        if with_scalar:
            s.set_scalar(scalar_settings(scheme=R.TVD_UMIST, solver_type=MULTIGRID, iterations=50, outer_iterations=3))
            s.set_scalar_bc("INLET", R.VALUE, 1.0)
        for it in range(3):
            reps.append(s.iterate(1, report=True)[1])
            if with_scalar:
                s.solve_scalar()
        out.append((s.get_fields(), np.concatenate(reps)))
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ 9. solver arms
def test_solver_arms_agree_and_repeat(gpu, tmp_path):
    a, m = mixed_mesh(tmp_path, True, PLUG_TYPES)
    n = a.n_cells
    flow = seeded_flow(a, 1.0)
    res = {}
    for method in (BICGSTAB, GMRES, MULTIGRID):
        s, _, _ = make_solver(m, a, scalar_settings(scheme=R.TVD_QUICK, diffusivity=5e-4, solver_type=method, iterations=600,
                                                    relative_convergence_threshold=1e-13, outer_tolerance=1e-11, outer_iterations=60),
                              PLUG_BCS, flow, rho=1.0)
        runs = []
        for _ in range(2):
            s.set_scalar_field(np.zeros(n))
            rep = s.solve_scalar()
            runs.append((s.get_scalar_field(), rep))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), method
        assert runs[0][1][1] <= 1e-11, (method, runs[0][1])
        res[method] = runs[0][0]
    ref = res[BICGSTAB]
    for method in (GMRES, MULTIGRID):
        assert np.linalg.norm(res[method] - ref) <= 1e-8 * np.linalg.norm(ref), (method, np.linalg.norm(res[method] - ref))


# ------------------------------------------------------------------ 10. arguments
def test_invalid_arguments_are_refused_and_change_nothing(gpu):
    from orc_amd.settings import ScalarSettings
    from orc_amd.solver import Solver
    a, m = hex_mesh(6, 4, 3, types=ASSEMBLY_TYPES)
    n = a.n_cells
    flow = seeded_flow(a)
    good = scalar_settings(scheme=R.TVD_UMIST, diffusivity=1e-3)

    def make(poke):
        s, _, _ = make_solver(m, a, good, ASSEMBLY_BCS, flow)
        s.set_scalar_field(0.5 + 0.5 * splitmix64_uniform(n, 3))
        if poke:
            for kw, code in ((dict(diffusivity=0.0), BAD_ARGUMENT), (dict(diffusivity=-1.0), BAD_ARGUMENT),
                             (dict(diffusivity=float("inf")), BAD_ARGUMENT), (dict(diffusivity=float("nan")), BAD_ARGUMENT),
                             (dict(scheme=R.CD2), UNSUPPORTED_SCHEME), (dict(scheme=9), UNSUPPORTED_SCHEME),
                             (dict(reserved0=1), BAD_ARGUMENT), (dict(iterations=0), BAD_ARGUMENT),
                             (dict(outer_iterations=0), BAD_ARGUMENT), (dict(solver_type=0), BAD_ARGUMENT),
                             (dict(preconditioner=5), BAD_ARGUMENT), (dict(outer_tolerance=-1.0), BAD_ARGUMENT)):
                assert s.set_scalar(ScalarSettings.default(**kw), raise_on_error=False) == code, kw
            assert s.set_scalar_bc(0, R.VALUE, 1.0, raise_on_error=False) == BAD_ARGUMENT  # the interior zone
            assert s.set_scalar_bc(1, 4, 1.0, raise_on_error=False) == BAD_ARGUMENT
            assert s.set_scalar_bc(1, -1, 1.0, raise_on_error=False) == BAD_ARGUMENT
            assert s.set_scalar_bc(99, R.VALUE, 1.0, raise_on_error=False) == BAD_ARGUMENT
            assert s.set_scalar_levels(np.ones(n), raise_on_error=False) == BAD_ARGUMENT  # no transient arm
        return s

    got, want = make(True), make(False)
    assert np.array_equal(got.get_scalar_field(), want.get_scalar_field())
    for x, y in zip(got.assemble_scalar(), want.assemble_scalar()):
        assert np.array_equal(x, y)
    # Rhie-Chow before any momentum assembly: refused, and fine once the diagonals exist
    s = Solver(m, settings(), 1.0, 1e-3)
    s.set_fields(*flow)
    s.set_scalar(good)
    st, _ = s.solve_scalar(raise_on_error=False)
    assert st == BAD_ARGUMENT and "diagonals" in __import__("orc_amd")._lib.last_error()
    assert s.assemble_scalar(raise_on_error=False) == BAD_ARGUMENT
    s.assemble_momentum()
    s.solve_scalar()
    # off: every entry but set_scalar refuses; turning it off frees the arm
    s.set_scalar(None)
    assert s.solve_scalar(raise_on_error=False)[0] == BAD_ARGUMENT


# ------------------------------------------------------------------ 11. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "scalar_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "SCALAR_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
