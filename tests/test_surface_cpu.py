"""The numpy restatement of the surface reports (tests/surface_restatement.py) against facts that need no device — a closed
surface, uniform flow, the Couette profile, the moment of a loaded plane — on the hex channel and on the polyhedral writer's
mesh; the Python report object; and the three C entries in the built library.  CPU only.

Tolerances: a sum of k terms formed with c rounded operations each is within (c + k_sum) EPS sum|term| of the exact sum of the
exact terms, k_sum = 1 for the restatement's exactly rounded math.fsum.  What each test adds for its INPUTS' rounding (stored
areas, normals and centroids come out of the mesh generator in floating point) is written next to it."""
import ctypes as C
import math

import numpy as np
import pytest

import surface_restatement as R

RHO, MU = 1.3, 2e-3


def hex_arrays(nx=6, ny=8, nz=3):
    from orc_amd.mesh import hex_channel
    return hex_channel(nx, ny, nz)


def poly_arrays(tmp_path):
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, write_mixed_channel_msh
    path = str(tmp_path / "poly.msh")
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=True)
    return MeshArrays(orc_io.read_mesh(path).arrays())


@pytest.fixture(params=["hex", "poly"])
def arrays(request, tmp_path):
    return hex_arrays() if request.param == "hex" else poly_arrays(tmp_path)


def set_all_boundary(a, zone_type, scalar=0.0, vector=(0.0, 0.0, 0.0)):
    nf = [len(f) for f in R.boundary_faces(a)]
    for z, name in enumerate(a["zone_names"]):
        if nf[z]:
            a.set_zone(name, zone_type, scalar, vector)
    return a


# Geometry allowance: a face's area is a triangle fan about the node mean (per triangle a cross product and a norm, about 15
# operations, up to 6 triangles) and its normal a normalised cross product (about 15): the stored A n of a face is within about
# 64 EPS |A n| of the exact one, and the exact ones of a closed surface sum to zero.
GEOMETRY_OPS = 64


def test_the_boundary_is_a_closed_surface(arrays):
    """sum over all boundary zones of A n = 0: PRESSURE_FORCE with p = 1 everywhere (walls carry the cell pressure)"""
    a = set_all_boundary(arrays, R.WALL)
    n = a.n_cells
    z, one = np.zeros(n), np.ones(n)
    S, Sabs, nf = R.report(a, z, z, z, one, RHO, MU)
    assert nf.sum() > 0 and nf[0] == 0  # zone 0 is the interior zone
    assert np.all(S[0] == 0.0)
    total = np.array([math.fsum(S[:, k].tolist()) for k in (2, 3, 4)])
    scale = Sabs[:, 2:5].sum(axis=0)
    tol = (R.C_OPS[R.PRESSURE_FORCE] + 2 + GEOMETRY_OPS) * R.EPS * scale  # + 2: the sums per zone and over the zones
    assert np.all(np.abs(total) <= tol), (total, tol)
    assert scale.min() > 0


def test_constant_pressure_exerts_no_net_force(arrays):
    """constant p in the cells and the same constant as the scalar of the pressure zones: sum PRESSURE_FORCE = 0"""
    a = set_all_boundary(arrays, R.WALL)
    p0 = 3.75
    a.set_zone("INLET", R.PRESSURE_INLET, p0)
    a.set_zone("OUTLET", R.PRESSURE_OUTLET, p0)
    n = a.n_cells
    z = np.zeros(n)
    S, Sabs, nf = R.report(a, z, z, z, np.full(n, p0), RHO, MU)
    total = np.array([math.fsum(S[:, k].tolist()) for k in (2, 3, 4)])
    tol = (R.C_OPS[R.PRESSURE_FORCE] + 2 + GEOMETRY_OPS) * R.EPS * Sabs[:, 2:5].sum(axis=0)
    assert np.all(np.abs(total) <= tol), (total, tol)
    # and the mean pressure of every zone with faces is p0 to the rounding of its two sums and the quotient
    mean = S[nf > 0, R.PRESSURE_AREA] / S[nf > 0, R.AREA]
    assert np.all(np.abs(mean - p0) <= 4 * R.EPS * p0), mean


def test_uniform_flow_balances_its_mass(arrays):
    """uniform U0 in the cells, a VelocityInlet carrying U0, every other boundary zone a PressureOutlet (which carries the cell
    velocity): sum MASS_FLOW = rho U0 . sum A n = 0, and the inlet's is rho (U0 . n) A with n out of the domain, i.e. negative"""
    U0 = np.array([0.31, 0.07, -0.11])
    a = set_all_boundary(arrays, R.PRESSURE_OUTLET)
    a.set_zone("INLET", R.VELOCITY_INLET, 0.0, tuple(U0))
    n = a.n_cells
    u, v, w = (np.full(n, U0[k]) for k in range(3))
    S, Sabs, nf = R.report(a, u, v, w, np.zeros(n), RHO, MU)
    total = math.fsum(S[:, R.MASS_FLOW].tolist())
    tol = (R.C_OPS[R.MASS_FLOW] + 2 + GEOMETRY_OPS) * R.EPS * Sabs[:, R.MASS_FLOW].sum()
    assert abs(total) <= tol, (total, tol)
    zi = a.get_face_zone("INLET")
    faces = R.boundary_faces(a)[zi]
    An = np.asarray(a["face_area"])[faces, None] * np.asarray(a["face_normal"]).reshape(-1, 3)[faces]
    want = RHO * float(U0 @ np.array([math.fsum(An[:, k].tolist()) for k in range(3)]))
    assert want < 0  # entering
    # the same products in another association: c_ops of the term, the sum, and 6 operations of `want`
    assert abs(S[zi, R.MASS_FLOW] - want) <= (R.C_OPS[R.MASS_FLOW] + 1 + 6) * R.EPS * Sabs[zi, R.MASS_FLOW]
    # momentum flow of the inlet = mass flow times U0
    assert np.all(np.abs(S[zi, 8:11] - want * U0) <= (R.C_OPS[R.MOMENTUM_FLOW] + 1 + 7) * R.EPS * Sabs[zi, 8:11])


def test_couette_profile_gives_the_wall_shear():
    """u = U y / h in the cells: the moving wall feels -mu U / h A in x, the fixed wall +mu U / h A (the one-sided difference
    is exact for a linear profile).  Input rounding: u_P and y_P carry 2 and 1 roundings, and U_P - U_f at the moving wall is a
    difference of numbers 2 ny times its size, as is x_f - x_P against y: (2 + 1 + 1) (2 ny) EPS on top of the term's own."""
    nx, ny, nz = 5, 8, 3
    U, h = 0.4, 0.001
    a = set_all_boundary(hex_arrays(nx, ny, nz), R.SYMMETRY)
    a.set_zone("TOP_WALL", R.WALL, 0.0, (U, 0.0, 0.0))
    a.set_zone("BOTTOM_WALL", R.WALL)
    n = a.n_cells
    y = np.asarray(a["cell_centroid"])[:, 1]
    z = np.zeros(n)
    S, Sabs, nf = R.report(a, U * y / h, z, z, z, RHO, MU)
    top, bot = a.get_face_zone("TOP_WALL"), a.get_face_zone("BOTTOM_WALL")
    assert nf[top] == nx * nz and nf[bot] == nx * nz
    want = MU * U / h * S[top, R.AREA]
    tol = (R.C_OPS[R.VISCOUS_FORCE] + 1 + 4 * 2 * ny + 3) * R.EPS * want  # + 3: `want` itself
    assert abs(S[top, R.VISCOUS_FORCE] + want) <= tol, (S[top, 5], want, tol)
    assert abs(S[bot, R.VISCOUS_FORCE] - want) <= tol, (S[bot, 5], want, tol)
    assert np.all(S[[top, bot], 6:8] == 0.0)  # no shear in y or z
    assert np.all(S[:, R.MASS_FLOW] == 0.0)   # walls and symmetry planes only: exact zeros


def test_moment_of_a_plane_under_constant_pressure(arrays):
    """a planar zone (the inlet, x = 0) under constant pressure: MOMENT = (xbar - x_0) x F with xbar the area centroid.
    Both sides are sums of the same products r A p n in another association: the term's 16 operations, the sums, and about 8
    operations of the right-hand side, against sum |r| |F| per face (no cancellation inside a term here: F is along x)."""
    a = set_all_boundary(arrays, R.WALL)
    n = a.n_cells
    z = np.zeros(n)
    x0 = np.array([3e-4, -2e-4, 1e-4])
    S, Sabs, nf = R.report(a, z, z, z, np.full(n, 2.5), RHO, MU, origin=x0)
    zi = a.get_face_zone("INLET")
    faces = R.boundary_faces(a)[zi]
    A = np.asarray(a["face_area"])[faces]
    xf = np.asarray(a["face_centroid"]).reshape(-1, 3)[faces]
    xbar = np.array([math.fsum((A * xf[:, k]).tolist()) for k in range(3)]) / math.fsum(A.tolist())
    F = S[zi, 2:5]
    assert np.all(S[zi, 5:8] == 0.0) and abs(F[0]) > 0
    want = np.cross(xbar - x0, F)
    scale = Sabs[zi, 11:14] + np.abs(xbar - x0).max() * np.abs(F).max()
    tol = (R.C_OPS[R.MOMENT] + 2 + 8 + GEOMETRY_OPS) * R.EPS * scale  # the plane is planar only to the generator's rounding
    assert np.all(np.abs(S[zi, 11:14] - want) <= tol), (S[zi, 11:14], want, tol)


def test_every_supported_type_follows_the_face_rules(arrays):
    """U_f, p_f and phi_f per zone type as oracle/solver.c get_face_velocity (None) / get_face_pressure / get_face_flux state
    them, and an unsupported type is refused"""
    from conftest import splitmix64_uniform
    a = set_all_boundary(arrays, R.WALL, 0.0, (0.2, -0.1, 0.05))
    n = a.n_cells
    u, v, w, p = (splitmix64_uniform(n, s) for s in (1, 2, 3, 4))
    zi = a.get_face_zone("INLET")
    faces = R.boundary_faces(a)[zi]
    P = np.asarray(a["face_c0"])[faces]
    nrm = np.asarray(a["face_normal"]).reshape(-1, 3)[faces]
    UP = np.stack([u[P], v[P], w[P]], axis=1)
    zv = np.array([0.2, -0.1, 0.05])
    for zt, vec, scal, flux in ((R.WALL, True, False, False), (R.VELOCITY_INLET, True, False, True), (R.PRESSURE_INLET, False, True, True),
                                (R.PRESSURE_OUTLET, False, True, True), (R.SYMMETRY, False, False, False)):
        a.set_zone("INLET", zt, 0.7, tuple(zv))
        Uf, pf, phi = R.face_values(a, u, v, w, p, faces)
        assert np.array_equal(Uf, np.broadcast_to(zv, Uf.shape) if vec else UP)
        assert np.array_equal(pf, np.full(len(faces), 0.7) if scal else p[P])
        assert np.all(phi == 0.0) if not flux else np.allclose(phi, (nrm * Uf).sum(axis=1), rtol=1e-14, atol=0)
    a.set_zone("INLET", R.OUTFLOW)
    with pytest.raises(ValueError):
        R.report(a, u, v, w, p, RHO, MU)


def test_report_object_views():
    from orc_amd.solver import SurfaceReport
    raw = np.arange(3 * R.N, dtype=np.float64).reshape(3, R.N)
    raw[0] = 0.0
    r = SurfaceReport(raw.ravel(), ["FLUID", "INLET", "WALL"])
    assert r.raw.shape == (3, 16)
    assert np.array_equal(r.area, raw[:, 0]) and np.array_equal(r.mass_flow, raw[:, 1]) and np.array_equal(r.faces, raw[:, 15])
    assert np.array_equal(r.pressure_force, raw[:, 2:5]) and np.array_equal(r.viscous_force, raw[:, 5:8])
    assert np.array_equal(r.force, raw[:, 2:5] + raw[:, 5:8])
    assert np.array_equal(r.momentum_flow, raw[:, 8:11]) and np.array_equal(r.moment, raw[:, 11:14])
    mp = r.mean_pressure
    assert np.isnan(mp[0]) and np.array_equal(mp[1:], raw[1:, 14] / raw[1:, 0])
    assert np.array_equal(r.zone("WALL"), raw[2])
    with pytest.raises(KeyError):
        SurfaceReport(raw).zone("WALL")


def test_library_exports_the_surface_entries():
    """fails on a library built before the surface reports existed"""
    import orc_amd
    from orc_amd._lib import lib
    L = lib()
    for name in ("orc_solver_surface_report", "orc_surface_integrals", "orc_mesh_boundary_index"):
        assert hasattr(L, name), name
    # the header's enum and the Python mirror agree on the layout
    txt = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "orc_types.h")).read()
    for name, value in (("AREA", R.AREA), ("MASS_FLOW", R.MASS_FLOW), ("PRESSURE_FORCE", R.PRESSURE_FORCE), ("VISCOUS_FORCE", R.VISCOUS_FORCE),
                        ("MOMENTUM_FLOW", R.MOMENTUM_FLOW), ("MOMENT", R.MOMENT), ("PRESSURE_AREA", R.PRESSURE_AREA), ("FACES", R.FACES), ("N", R.N)):
        assert "ORC_SURFACE_%s = %d" % (name, value) in txt, name
    # argument checks that need no mesh: without a device every compute entry says so, with one a null mesh is a bad argument
    want = 11 if orc_amd.device_count() < 1 else 10
    out = np.zeros(16)
    assert L.orc_surface_integrals(None, None, None, None, None, C.c_double(1.0), C.c_double(1.0), None,
                                   out.ctypes.data_as(C.POINTER(C.c_double))) == want
    assert L.orc_mesh_boundary_index(None, None, None, None, None) == want
    assert L.orc_solver_surface_report(None, None, out.ctypes.data_as(C.POINTER(C.c_double))) == want
