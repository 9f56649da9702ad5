"""Surface reports (orc_solver_surface_report, orc_surface_integrals, orc_mesh_boundary_index) on the device against the numpy
restatement (tests/surface_restatement.py): the boundary index, the chunk edges, every zone type on the mixed and polyhedral
meshes, the analytic facts of tests/test_surface_cpu.py, the live solver state, read-only and repeatable, the field-level entry,
argument checking and two ranks on one GPU.

Every comparison with the restatement uses the DERIVED bound of surface_restatement.bound():
    |device - restatement| <= (c_ops + ceil(log2(faces in zone)) + ceil(log2(chunks)) + 2) EPS sum|term|,  EPS = 2^-53
c_ops per quantity (surface_restatement.C_OPS, counted there from the operator order): AREA 0, MASS_FLOW 7, PRESSURE_FORCE 2,
VISCOUS_FORCE 13, MOMENTUM_FLOW 8, MOMENT 16, PRESSURE_AREA 1, FACES 0.  The rest is the depth of the device's tree: per chunk a
lane's eight slots pairwise (3), the wave tree (6), the four waves in sequence (3, one more than a tree: the first unit of the
"+ 2"), over the chunks a pairwise tree; the second unit is the restatement's own exactly rounded sum.  Exact zeros by definition
are compared with == 0.0, FACES and zone_ptr exactly."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_restatement as R
from conftest import ROOT, splitmix64_uniform

pytestmark = pytest.mark.gpu

BICGSTAB = 3
BAD_ARGUMENT, UNSUPPORTED_BC = 10, 7
RHO, MU = 1.3, 2e-3
ORIGIN = (3e-4, -2e-4, 1.5e-4)

# every supported type on the hex channel's six zones: non-zero wall and inlet vectors, non-zero inlet / outlet scalars
HEX_TYPES = {"INLET": (R.VELOCITY_INLET, 0.0, (0.4, 0.05, -0.02)), "OUTLET": (R.PRESSURE_OUTLET, 0.3, (0, 0, 0)),
             "PERIODIC_-Z": (R.SYMMETRY, 0.0, (0, 0, 0)), "PERIODIC_+Z": (R.PRESSURE_INLET, -0.2, (0, 0, 0)),
             "TOP_WALL": (R.WALL, 0.0, (0.1, 0.0, 0.03)), "BOTTOM_WALL": (R.WALL, 0.0, (-0.02, 0.01, 0.0))}
# the mixed writer's zones and their "_TRI" twins: the twins get another type or other values
MIXED_TYPES = {"INLET": (R.VELOCITY_INLET, 0.0, (0.4, 0.05, -0.02)), "OUTLET": (R.PRESSURE_OUTLET, 0.3, (0, 0, 0)),
               "WALL": (R.WALL, 0.0, (0.1, 0.0, 0.03)), "WALL_TRI": (R.WALL, 0.0, (-0.02, 0.01, 0.0)),
               "PERIODIC_-Z": (R.SYMMETRY, 0.0, (0, 0, 0)), "PERIODIC_-Z_TRI": (R.SYMMETRY, 0.0, (0, 0, 0)),
               "PERIODIC_+Z": (R.PRESSURE_INLET, -0.2, (0, 0, 0)), "PERIODIC_+Z_TRI": (R.VELOCITY_INLET, 0.0, (0.0, 0.02, -0.3))}


def apply_types(a, types):
    for name in a["zone_names"]:
        if name in types:
            zt, sc, vec = types[name]
            a.set_zone(name, zt, sc, vec)
    return a


def hex_case(nx, ny, nz, ordering=None, types=HEX_TYPES):
    from orc_amd.mesh import Mesh, hex_channel
    a = apply_types(hex_channel(nx, ny, nz), types)
    return a, Mesh(a, ordering=ordering)


def mixed_case(tmp_path, polyhedra, types=MIXED_TYPES):
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays, set_mixed_channel_bcs, write_mixed_channel_msh
    path = str(tmp_path / ("poly.msh" if polyhedra else "mixed.msh"))
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=polyhedra)
    a = apply_types(set_mixed_channel_bcs(MeshArrays(orc_io.read_mesh(path).arrays())), types)
    return a, Mesh(a)


def seeded_fields(a, scale=0.05):
    n = a.n_cells
    return (scale * (1 + 0.5 * splitmix64_uniform(n, 1)), 0.3 * scale * splitmix64_uniform(n, 2),
            0.2 * scale * splitmix64_uniform(n, 3), 0.01 * splitmix64_uniform(n, 4))


def integrals(m, f, origin=ORIGIN, rho=RHO, mu=MU):
    from orc_amd.solver import surface_integrals
    return surface_integrals(m, *f, rho, mu, origin=origin)


# ------------------------------------------------------------------ 1. the index
@pytest.mark.parametrize("mesh_name", ["hex", "hex_rcm", "poly"])
def test_boundary_index_equals_the_numpy_list(gpu, tmp_path, mesh_name):
    if mesh_name == "poly":
        a, m = mixed_case(tmp_path, True)
    else:
        a, m = hex_case(9, 5, 4, ordering=1 if mesh_name == "hex_rcm" else None)
    want = R.boundary_faces(a)  # a reordered mesh renumbers its cells, not its faces: the internal face numbering is the file's
    zp, faces, builds, chunk = m.boundary_index()
    assert builds == 1 and chunk >= 256
    assert np.array_equal(zp, np.concatenate([[0], np.cumsum([len(f) for f in want])]))
    assert np.array_equal(faces, np.concatenate(want))
    for z in range(len(want)):
        assert np.all(np.diff(faces[zp[z]:zp[z + 1]]) > 0)
    if mesh_name == "hex_rcm":  # the cells behind the faces are the renumbered ones: the report reads the right cells
        assert not np.array_equal(m.cell_order(), np.arange(a.n_cells))
    f = seeded_fields(a)
    first = integrals(m, f).raw
    for _ in range(2):
        assert np.array_equal(integrals(m, f).raw, first)
    a.set_zone("OUTLET", R.PRESSURE_OUTLET, 0.9)
    m.update_zones()
    after = integrals(m, f)
    assert after.zone("OUTLET")[R.PRESSURE_AREA] != first[a.get_face_zone("OUTLET"), R.PRESSURE_AREA]  # read at report time
    zp2, faces2, builds2, _ = m.boundary_index()
    assert builds2 == 1 and np.array_equal(zp2, zp) and np.array_equal(faces2, faces)
    R.check(after.raw, a, *f, RHO, MU, ORIGIN, chunk)


# ------------------------------------------------------------------ 2. chunk edges
# wall zones (nx * nz faces) of chunk - 1, chunk, chunk + 1, 2 chunk + 1 faces for chunk = 2048; ny = 2; the smallest channel
CHUNK_SHAPES = [(23, 2, 89), (64, 2, 32), (2049, 2, 1), (683, 2, 3), (4097, 2, 1), (2, 2, 1)]


@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_chunk_edges_all_sixteen_quantities(gpu, shape):
    nx, ny, nz = shape
    a, m = hex_case(nx, ny, nz)
    zp, faces, _, chunk = m.boundary_index()
    if chunk == 2048 and shape != (2, 2, 1):
        assert nx * nz in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1)
        assert zp[a.get_face_zone("TOP_WALL") + 1] - zp[a.get_face_zone("TOP_WALL")] == nx * nz
    f = seeded_fields(a)
    rep = integrals(m, f)
    worst = R.check(rep.raw, a, *f, RHO, MU, ORIGIN, chunk)
    print("shape %s: worst error / bound %.3f" % (shape, worst))


# ------------------------------------------------------------------ 3. every zone type, the mixed and the polyhedral mesh
@pytest.mark.parametrize("polyhedra", [False, True], ids=["mixed", "poly"])
def test_every_zone_type_on_the_mixed_meshes(gpu, tmp_path, polyhedra):
    from orc_amd.solver import surface_integrals
    a, m = mixed_case(tmp_path, polyhedra)
    nf = np.array([len(f) for f in R.boundary_faces(a)])
    present = set(int(t) for t, k in zip(a["zone_type"], nf) if k)
    assert present == set(R.SUPPORTED), present
    assert nf[a.get_face_zone("FLUID")] == 0 and np.count_nonzero(nf) >= 8  # the interior zone(s) and the twins
    chunk = m.boundary_index()[3]
    f = seeded_fields(a)
    rep = integrals(m, f)
    worst = R.check(rep.raw, a, *f, RHO, MU, ORIGIN, chunk)
    print("worst error / bound %.3f" % worst)
    assert np.all(rep.raw[nf == 0] == 0.0)
    assert np.all(np.isnan(rep.mean_pressure[nf == 0])) and np.all(np.isfinite(rep.mean_pressure[nf > 0]))
    assert np.array_equal(rep.force, rep.pressure_force + rep.viscous_force)
    # a type the assembly refuses, then the next valid call
    a.set_zone("OUTLET", R.OUTFLOW)
    m.update_zones()
    st, _ = surface_integrals(m, *f, RHO, MU, origin=ORIGIN, raise_on_error=False)
    assert st == UNSUPPORTED_BC
    zt, sc, vec = MIXED_TYPES["OUTLET"]
    a.set_zone("OUTLET", zt, sc, vec)
    m.update_zones()
    assert np.array_equal(integrals(m, f).raw, rep.raw)


# ------------------------------------------------------------------ 4. the analytic facts, on the device
GEOMETRY_OPS = 64  # tests/test_surface_cpu.py: the stored A n of a face is within about 64 EPS |A n| of the exact one


def all_boundary(a, zone_type, scalar=0.0, vector=(0.0, 0.0, 0.0)):
    nf = [len(f) for f in R.boundary_faces(a)]
    for z, name in enumerate(a["zone_names"]):
        if nf[z]:
            a.set_zone(name, zone_type, scalar, vector)
    return a


def device_and_bound(a, m, f, origin=None):
    """the device report, the restatement's bound per entry, and sum|term| per entry"""
    chunk = m.boundary_index()[3]
    rep = integrals(m, f, origin=origin)
    R.check(rep.raw, a, *f, RHO, MU, origin, chunk)
    S, Sabs, nf = R.report(a, *f, RHO, MU, origin)
    return rep, R.bound(Sabs, nf, chunk), Sabs


def test_closed_surface_and_constant_pressure(gpu, tmp_path):
    """sum over the zones of PRESSURE_FORCE = 0 under constant pressure (walls, and pressure zones carrying the same constant):
    the analytic tolerance of the CPU file plus the device's derived bound per zone"""
    from orc_amd.mesh import Mesh
    for a in (hex_case(7, 5, 3)[0], mixed_case(tmp_path, True)[0]):
        all_boundary(a, R.WALL)
        a.set_zone("INLET", R.PRESSURE_INLET, 3.75)
        a.set_zone("OUTLET", R.PRESSURE_OUTLET, 3.75)
        m = Mesh(a)
        z = np.zeros(a.n_cells)
        rep, B, Sabs = device_and_bound(a, m, (z, z, z, np.full(a.n_cells, 3.75)))
        total = np.array([math.fsum(rep.raw[:, k].tolist()) for k in (2, 3, 4)])
        tol = (R.C_OPS[R.PRESSURE_FORCE] + 2 + GEOMETRY_OPS) * R.EPS * Sabs[:, 2:5].sum(axis=0) + B[:, 2:5].sum(axis=0)
        assert np.all(np.abs(total) <= tol), (total, tol)
        has = rep.faces > 0
        assert np.all(np.abs(rep.mean_pressure[has] - 3.75) <= 4 * R.EPS * 3.75 + (B[has, 14] + 3.75 * B[has, 0]) / rep.area[has])


def test_uniform_flow_mass_balance(gpu, tmp_path):
    from orc_amd.mesh import Mesh
    U0 = np.array([0.31, 0.07, -0.11])
    for a in (hex_case(7, 5, 3)[0], mixed_case(tmp_path, True)[0]):
        all_boundary(a, R.PRESSURE_OUTLET)
        a.set_zone("INLET", R.VELOCITY_INLET, 0.0, tuple(U0))
        m = Mesh(a)
        n = a.n_cells
        rep, B, Sabs = device_and_bound(a, m, tuple(np.full(n, U0[k]) for k in range(3)) + (np.zeros(n),))
        total = math.fsum(rep.mass_flow.tolist())
        tol = (R.C_OPS[R.MASS_FLOW] + 2 + GEOMETRY_OPS) * R.EPS * Sabs[:, 1].sum() + B[:, 1].sum()
        assert abs(total) <= tol, (total, tol)
        zi = a.get_face_zone("INLET")
        faces = R.boundary_faces(a)[zi]
        An = np.asarray(a["face_area"])[faces, None] * np.asarray(a["face_normal"]).reshape(-1, 3)[faces]
        want = RHO * float(U0 @ np.array([math.fsum(An[:, k].tolist()) for k in range(3)]))
        assert want < 0 and abs(rep.mass_flow[zi] - want) <= (R.C_OPS[R.MASS_FLOW] + 1 + 6) * R.EPS * Sabs[zi, 1] + B[zi, 1]


def test_couette_wall_force_and_moment_of_a_plane(gpu):
    """tests/test_surface_cpu.py's Couette and moment facts with the device's derived bound added to their tolerances"""
    from orc_amd.mesh import Mesh, hex_channel
    nx, ny, nz = 5, 8, 3
    U, h = 0.4, 0.001
    a = all_boundary(hex_channel(nx, ny, nz), R.SYMMETRY)
    a.set_zone("TOP_WALL", R.WALL, 0.0, (U, 0.0, 0.0))
    a.set_zone("BOTTOM_WALL", R.WALL)
    m = Mesh(a)
    y = np.asarray(a["cell_centroid"])[:, 1]
    z = np.zeros(a.n_cells)
    rep, B, Sabs = device_and_bound(a, m, (U * y / h, z, z, z))
    top, bot = a.get_face_zone("TOP_WALL"), a.get_face_zone("BOTTOM_WALL")
    want = MU * U / h * rep.area[top]
    tol = (R.C_OPS[R.VISCOUS_FORCE] + 1 + 4 * 2 * ny + 3) * R.EPS * want
    assert abs(rep.viscous_force[top, 0] + want) <= tol + B[top, 5]
    assert abs(rep.viscous_force[bot, 0] - want) <= tol + B[bot, 5]
    assert np.all(rep.viscous_force[:, 1:] == 0.0) and np.all(rep.mass_flow == 0.0)
    # the moment of the inlet plane under constant pressure
    a = all_boundary(hex_channel(nx, ny, nz), R.WALL)
    m = Mesh(a)
    x0 = np.array(ORIGIN)
    rep, B, Sabs = device_and_bound(a, m, (z, z, z, np.full(a.n_cells, 2.5)), origin=ORIGIN)
    zi = a.get_face_zone("INLET")
    faces = R.boundary_faces(a)[zi]
    A = np.asarray(a["face_area"])[faces]
    xf = np.asarray(a["face_centroid"]).reshape(-1, 3)[faces]
    xbar = np.array([math.fsum((A * xf[:, k]).tolist()) for k in range(3)]) / math.fsum(A.tolist())
    F = rep.force[zi]
    arm = np.abs(xbar - x0).max()
    scale = Sabs[zi, 11:14] + arm * np.abs(F).max()
    tol = (R.C_OPS[R.MOMENT] + 2 + 8 + GEOMETRY_OPS) * R.EPS * scale + B[zi, 11:14] + arm * B[zi, 2:5].max()
    assert np.all(np.abs(rep.moment[zi] - np.cross(xbar - x0, F)) <= tol)


# ------------------------------------------------------------------ 5. the live state
def channel_solver(ordering=None, **kw):
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    a = set_channel_bcs(hex_channel(16, 8, 4), top_wall_velocity=0.01)
    m = Mesh(a, ordering=ordering)
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    start = (1e-3 * (1 + 0.1 * splitmix64_uniform(n, 1)), 1e-6 * splitmix64_uniform(n, 2), 1e-7 * splitmix64_uniform(n, 3),
             -0.01 * (1 - cc[:, 0] / 0.002))
    s = Solver(m, NumericalSettings.default(solver_type=BICGSTAB, **kw), 1000.0, 1e-3)  # Rhie-Chow is the default
    s.set_fields(*start)
    return a, m, s


@pytest.mark.parametrize("ordering", [None, 1], ids=["orc", "rcm"])
def test_report_reads_the_live_state(gpu, ordering):
    a, m, s = channel_solver(ordering)
    chunk = m.boundary_index()[3]
    s.snapshot()
    before = s.surface_report(ORIGIN)
    R.check(before.raw, a, *s.get_fields(), 1000.0, 1e-3, ORIGIN, chunk)
    s.iterate(3)
    rep = s.surface_report(ORIGIN)
    assert not np.array_equal(rep.raw, before.raw)
    R.check(rep.raw, a, *s.get_fields(), 1000.0, 1e-3, ORIGIN, chunk)
    s.restore()
    back = s.surface_report(ORIGIN)
    R.check(back.raw, a, *s.get_fields(), 1000.0, 1e-3, ORIGIN, chunk)
    assert np.array_equal(back.raw, before.raw)
    assert m.boundary_index()[2] == 1


# ------------------------------------------------------------------ 6. read-only and repeatable
def test_reports_are_repeatable_and_change_nothing(gpu):
    runs = []
    for with_reports in (False, True):
        a, m, s = channel_solver()
        reps = []
        for _ in range(3):
            if with_reports:
                f0 = s.get_fields()
                r1, r2 = s.surface_report(ORIGIN), s.surface_report(ORIGIN)
                assert np.array_equal(r1.raw, r2.raw)
                for x, y in zip(f0, s.get_fields()):
                    assert np.array_equal(x, y)
            reps.append(s.iterate(1, report=True)[1])
        runs.append((s.get_fields(), np.concatenate(reps)))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(runs[0][1], runs[1][1])


def test_scalar_boundary_flux_is_untouched_by_a_report(gpu):
    from orc_amd.settings import ScalarSettings
    out = []
    for with_reports in (False, True):
        a, m, s = channel_solver()
        s.iterate(1)
        s.set_scalar(ScalarSettings.default(diffusivity=2e-3, iterations=100))
        s.set_scalar_bc("INLET", 1, 1.0)
        if with_reports:
            s.surface_report()
        s.solve_scalar()
        if with_reports:
            s.surface_report(ORIGIN)
        b1 = s.scalar_boundary_flux()
        if with_reports:
            s.surface_report()
        out.append((b1, s.scalar_boundary_flux(), s.get_scalar_field()))
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 7. the field-level entry
@pytest.mark.parametrize("ordering", [None, 1], ids=["orc", "rcm"])
def test_field_level_entry_equals_the_solver_report(gpu, ordering):
    a, m, s = channel_solver(ordering)
    s.iterate(2)
    rep = s.surface_report(ORIGIN)
    got = integrals(m, s.get_fields(), rho=1000.0, mu=1e-3)
    assert np.array_equal(got.raw, rep.raw)
    assert np.array_equal(rep.zone("TOP_WALL"), rep.raw[a.get_face_zone("TOP_WALL")])


# ------------------------------------------------------------------ 8. arguments
def test_bad_arguments_are_refused_and_the_next_call_is_right(gpu):
    from orc_amd._lib import lib
    from orc_amd.solver import surface_integrals
    a, m, s = channel_solver()
    f = s.get_fields()
    good = s.surface_report(ORIGIN)
    F64 = C.POINTER(C.c_double)
    p = lambda x: x.ctypes.data_as(F64)
    out = np.zeros(len(a["zone_type"]) * 16)
    L = lib()
    o = np.array(ORIGIN)
    assert L.orc_solver_surface_report(None, p(o), p(out)) == BAD_ARGUMENT
    assert L.orc_solver_surface_report(s.ptr, p(o), None) == BAD_ARGUMENT
    assert L.orc_surface_integrals(None, p(f[0]), p(f[1]), p(f[2]), p(f[3]), 1.0, 1.0, p(o), p(out)) == BAD_ARGUMENT
    assert L.orc_surface_integrals(m.ptr, p(f[0]), p(f[1]), p(f[2]), p(f[3]), 1.0, 1.0, p(o), None) == BAD_ARGUMENT
    assert L.orc_surface_integrals(m.ptr, None, p(f[1]), p(f[2]), p(f[3]), 1.0, 1.0, p(o), p(out)) == BAD_ARGUMENT
    assert L.orc_mesh_boundary_index(None, None, None, None, None) == BAD_ARGUMENT
    for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
        assert s.surface_report(bad, raise_on_error=False)[0] == BAD_ARGUMENT
        assert surface_integrals(m, *f, 1000.0, 1e-3, origin=bad, raise_on_error=False)[0] == BAD_ARGUMENT
        assert np.array_equal(s.surface_report(ORIGIN).raw, good.raw)
    for rho, mu in ((0.0, 1e-3), (-1.0, 1e-3), (float("nan"), 1e-3), (float("inf"), 1e-3), (1000.0, 0.0), (1000.0, -1e-3),
                    (1000.0, float("nan")), (1000.0, float("inf"))):
        assert surface_integrals(m, *f, rho, mu, origin=ORIGIN, raise_on_error=False)[0] == BAD_ARGUMENT, (rho, mu)
        assert np.array_equal(surface_integrals(m, *f, 1000.0, 1e-3, origin=ORIGIN).raw, good.raw)
    # origin None = (0, 0, 0)
    assert np.array_equal(s.surface_report().raw, s.surface_report((0.0, 0.0, 0.0)).raw)
    for x, y in zip(f, s.get_fields()):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 9. two ranks
def test_two_ranks_on_one_gpu_receive_the_global_sums(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "surface_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "SURFACE_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
