"""The numpy restatement of the derived cell fields (tests/derived_restatement.py) against analytic facts, and the compute entries'
behaviour without a device.  CPU only.

The mesh is a uniform hex channel 7 x 5 x 4 with a cell edge of 1/8 in every direction: every coordinate and every face area is a
binary fraction and exact, the generator's cell volumes are within one rounding of h^3 (printed), so Green-Gauss with midpoint face
values reproduces a linear field's gradient on every cell without a boundary face up to rounding.  That rounding is bounded by the
restatement's DERIVED bound: (faces + 3) EPS sum_f |U_f.i n.j| A / V per gradient entry, carried through the table formulas
(field_bounds).  The field values themselves are rounded when they are formed (u = Omega x x: two products and a difference per
component) and so is V; each is one more rounding of the size of a unit of the same sum, inside the slack of a worst case over
6 + 3 roundings.  The bound is not tuned to what the code gives: the largest error / bound ratio is printed."""
import ctypes as C

import numpy as np
import pytest

import derived_restatement as D

NX, NY, NZ, H = 7, 5, 4, 0.125


@pytest.fixture(scope="module")
def cube():
    from orc_amd.mesh import hex_channel
    import surface_restatement as R
    a = hex_channel(NX, NY, NZ, lx=NX * H, ly=NY * H, lz=NZ * H)
    for name in a["zone_names"][1:]:
        a.set_zone(name, R.SYMMETRY)
    inner = np.ones(a.n_cells, bool)
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    inner[c0[c1 < 0]] = False
    assert inner.sum() == (NX - 2) * (NY - 2) * (NZ - 2)
    vol, area = np.asarray(a["cell_volume"]), np.asarray(a["face_area"])
    print("geometry: max |V / h^3 - 1| = %.2e, max |A / h^2 - 1| = %.2e" % (np.abs(vol / H ** 3 - 1).max(), np.abs(area / H ** 2 - 1).max()))
    return a, inner


def evaluate(a, U):
    G, conv, Gabs, convabs, faces = D.gg_gradient(a, U[:, 0], U[:, 1], U[:, 2])
    vol = np.asarray(a["cell_volume"])
    F = D.fields(G, conv, vol)
    B = D.field_bounds(G, D.gradient_bound(Gabs, faces), conv, convabs, faces, vol)
    return F, B


def within(F, B, inner, k, want, what):
    err = np.abs(F[k][inner] - want)
    ratio = float(np.max(err / B[k][inner])) if np.all(B[k][inner] > 0) else float(np.max(err))
    print("%s: worst error %.3e, worst error / bound %.3f" % (what, err.max(), ratio))
    assert np.all(err <= B[k][inner]), (what, err.max(), B[k][inner].min())


def test_rigid_rotation(cube):
    a, inner = cube
    om = np.array([0.3, -0.2, 0.5])
    x = np.asarray(a["cell_centroid"]).reshape(-1, 3)
    U = np.cross(om[None, :], x)
    F, B = evaluate(a, U)
    for k in range(3):
        within(F, B, inner, k, 2 * om[k], D.NAMES[k])
    within(F, B, inner, D.VORTICITY_MAG, 2 * np.sqrt(om @ om), "vorticity_mag")
    within(F, B, inner, D.STRAIN_RATE_MAG, 0.0, "strain_rate_mag")
    within(F, B, inner, D.Q_CRITERION, om @ om, "q_criterion")
    within(F, B, inner, D.DIVERGENCE, 0.0, "divergence")


def test_simple_shear(cube):
    a, inner = cube
    gamma = -0.7
    x = np.asarray(a["cell_centroid"]).reshape(-1, 3)
    U = np.zeros_like(x)
    U[:, 0] = gamma * x[:, 1]
    F, B = evaluate(a, U)
    within(F, B, inner, D.VORTICITY_Z, -gamma, "vorticity_z")
    within(F, B, inner, D.VORTICITY_X, 0.0, "vorticity_x")
    within(F, B, inner, D.VORTICITY_Y, 0.0, "vorticity_y")
    within(F, B, inner, D.STRAIN_RATE_MAG, abs(gamma), "strain_rate_mag")
    within(F, B, inner, D.Q_CRITERION, 0.0, "q_criterion")
    within(F, B, inner, D.DIVERGENCE, 0.0, "divergence")
    within(F, B, inner, D.CONVECTIVE_RATE, np.abs(U[inner, 0]) / H, "convective_rate")


def test_packing_helpers_and_boundary_restatement_shapes(cube):
    a, _ = cube
    n = a.n_cells
    z = np.zeros(n)
    allf = D.cell_fields(a, z + 1.0, z, z)
    assert allf.shape == (8, n) and np.array_equal(D.select(allf, 0b10100101), allf[[0, 2, 5, 7]])
    zp, faces, vals = D.boundary_fields(a, z + 1.0, z, z, z, 1.0, 1.0)
    assert zp[-1] == len(faces) == 2 * (NX * NY + NX * NZ + NY * NZ) and vals.shape == (8, len(faces))
    assert np.all(vals[D.B_TRACTION_X:D.B_Y_PLUS + 1] == 0.0)  # symmetry everywhere: no wall, no traction
    assert np.all(np.abs(vals[D.B_AREA] - H * H) <= 8 * D.EPS * H * H)


def test_compute_entries_need_a_device(cube):
    import orc_amd
    from orc_amd._lib import lib
    from orc_amd.settings import NumericalSettings
    want = 11 if orc_amd.device_count() == 0 else 10  # NO_DEVICE; with a device the null arguments are BAD_ARGUMENT
    L = lib()
    F64 = C.POINTER(C.c_double)
    x = np.zeros(8)
    p = x.ctypes.data_as(F64)
    s = NumericalSettings.default()
    # the device comes first, whatever the arguments
    assert L.orc_solver_derived_fields(None, 1, p) == want
    assert L.orc_derived_fields(None, p, p, p, C.byref(s), 1, p) == want
    assert L.orc_solver_boundary_fields(None, 1, p) == want
    assert L.orc_boundary_fields(None, p, p, p, p, 1.0, 1.0, 1, p) == want
