"""Wall distance and wall damping without a device: the struct's layout against the header, the numpy restatement of the search
(tests/wall_restatement.py) on the host generators against exact distances, its invariances, and the damped Smagorinsky law in
float64 against longdouble.

The bound of the law, 16 * 2^-52 relative: two library calls (cbrt, expm1) at 1 ULP each and at most eight roundings (cs cbrt, rho
u_tau, times d, / mu, / a_plus, l0 times the factor, l l, rho (l l), times g, mu + ...: the additions of positive terms never cancel,
and expm1 keeps 1 - exp(-x) free of cancellation at the wall)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wall_restatement as W
from conftest import ROOT, splitmix64_uniform

FIELDS = ["mode", "reserved0", "kappa", "a_plus", "u_tau"]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_struct_layout_matches_the_header(tmp_path):
    from orc_amd.settings import WallDamping, WallDampingMode
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\nint main(){printf("%zu", sizeof(OrcWallDamping));\n'
    src += "".join('printf(" %%zu", offsetof(OrcWallDamping, %s));\n' % f for f in FIELDS)
    src += 'printf(" %d %d %d", ORC_WALL_DAMPING_NONE, ORC_WALL_DAMPING_MIN, ORC_WALL_DAMPING_VAN_DRIEST);return 0;}'
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert [n for n, _ in WallDamping._fields_] == FIELDS
    assert got[0] == C.sizeof(WallDamping) == 32
    assert got[1:6] == [getattr(WallDamping, n).offset for n in FIELDS] == [0, 4, 8, 16, 24]
    assert got[6:] == [WallDampingMode.NONE, WallDampingMode.MIN, WallDampingMode.VAN_DRIEST] == [0, 1, 2]


def test_default_values_and_make():
    """orc_wall_damping_default needs no device"""
    from orc_amd.settings import WallDamping, WallDampingMode
    w = WallDamping.make(WallDampingMode.NONE)
    assert (w.mode, w.reserved0, w.kappa, w.a_plus, w.u_tau) == (0, 0, 0.41, 26.0, 0.0)
    w = WallDamping.make(WallDampingMode.VAN_DRIEST, u_tau=0.05, a_plus=25.0)
    assert (w.mode, w.reserved0, w.kappa, w.a_plus, w.u_tau) == (2, 0, 0.41, 25.0, 0.05)
    with pytest.raises(AttributeError):
        WallDamping.make(WallDampingMode.MIN, nope=1.0)


# ------------------------------------------------------------------ the search's restatement on the host generators
def box(nx, ny, nz, lx, ly, lz, walls):
    from orc_amd.mesh import hex_channel
    from orc_amd.settings import FaceConditionTypes as T
    a = hex_channel(nx, ny, nz, lx, ly, lz)
    for name in a["zone_names"][1:]:
        a.set_zone(name, T.Wall if name in walls else T.Symmetry)
    return a


SIDES = {"INLET": (0, 0), "OUTLET": (0, 1), "BOTTOM_WALL": (1, 0), "TOP_WALL": (1, 1), "PERIODIC_-Z": (2, 0), "PERIODIC_+Z": (2, 1)}


def plane_distance(a, walls):
    """min over the wall planes of |coordinate - plane|, the plane's coordinate read from the zone's face centroids"""
    cc, fc, fz = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"]), np.asarray(a["face_zone"])
    out = np.full(len(cc), np.inf)
    for name in walls:
        axis, _ = SIDES[name]
        plane = np.unique(fc[fz == a.get_face_zone(name), axis])
        assert len(plane) == 1, (name, plane)
        out = np.minimum(out, np.abs(cc[:, axis] - plane[0]))
    return out


def tied_cells(a):
    """cells whose smallest s is reached by more than one wall face"""
    cc = np.asarray(a["cell_centroid"])
    fc, _ = W.wall_table(a)
    r = cc[:, None, :] - fc[None, :, :]
    s = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
    return np.count_nonzero((s == s.min(axis=1)[:, None]).sum(axis=1) > 1)


def test_channel_is_min_y_h_minus_y_bit_for_bit():
    from orc_amd.mesh import hex_channel, set_channel_bcs
    a = set_channel_bcs(hex_channel(7, 10, 3))
    y = np.asarray(a["cell_centroid"])[:, 1]
    fy = np.asarray(a["face_centroid"])[:, 1]
    fz = np.asarray(a["face_zone"])
    assert np.all(fy[fz == a.get_face_zone("BOTTOM_WALL")] == 0.0)
    h = np.unique(fy[fz == a.get_face_zone("TOP_WALL")])
    assert len(h) == 1
    d = W.mesh_wall_distance(a)
    assert same_bits(d, np.minimum(y, h[0] - y))
    assert len(W.wall_faces(a)) == 2 * 7 * 3


def test_six_wall_box_and_two_wall_corner_are_exact_with_tied_cells():
    all6 = list(SIDES)
    a = box(4, 4, 4, 1.0, 1.0, 1.0, all6)  # a cube of cubes: the diagonal cells tie in s
    assert tied_cells(a) > 0
    assert same_bits(W.mesh_wall_distance(a), plane_distance(a, all6))
    b = box(5, 4, 3, 2e-3, 1e-3, 3e-4, all6)  # anisotropic cells
    assert same_bits(W.mesh_wall_distance(b), plane_distance(b, all6))
    corner = ["INLET", "BOTTOM_WALL"]
    c = box(4, 4, 3, 1.0, 1.0, 0.75, corner)
    assert tied_cells(c) > 0
    d = W.mesh_wall_distance(c)
    cc = np.asarray(c["cell_centroid"])
    assert same_bits(d, plane_distance(c, corner)) and same_bits(d, np.minimum(cc[:, 0], cc[:, 1]))
    # an explicit mask is the same as the types
    assert same_bits(W.mesh_wall_distance(c, zones=corner), d) and same_bits(W.mesh_wall_distance(c, zones=[1, 6]), d)


def test_no_walls_gives_inf():
    a = box(3, 2, 2, 1.0, 1.0, 1.0, [])
    assert len(W.wall_faces(a)) == 0
    assert np.all(np.isposinf(W.mesh_wall_distance(a)))


def test_invariance_under_cell_renumbering_and_table_order():
    from orc_amd.mesh import renumber_cells
    a = box(6, 5, 4, 2e-3, 1e-3, 4e-4, ["TOP_WALL", "BOTTOM_WALL", "INLET"])
    d = W.mesh_wall_distance(a)
    n = a.n_cells
    new_of_old = np.argsort(splitmix64_uniform(n, 11), kind="stable").astype(np.int64)
    b = renumber_cells(a, new_of_old)
    db = W.mesh_wall_distance(b)
    assert same_bits(db[new_of_old], d)
    fc, fn = W.wall_table(a)
    perm = np.argsort(splitmix64_uniform(len(fc), 12), kind="stable")
    assert same_bits(W.mesh_wall_distance(a, table=(fc[perm], fn[perm])), d)
    assert same_bits(W.mesh_wall_distance(a, table=(fc[::-1], fn[::-1])), d)


# ------------------------------------------------------------------ the damped law
def law_inputs(n=8192):
    from viscosity_restatement import log_uniform
    d = log_uniform(splitmix64_uniform(n, 21), 1e-9, 1e1)
    g = log_uniform(splitmix64_uniform(n, 22), 1e-8, 1e8)
    vol = log_uniform(splitmix64_uniform(n, 23), 1e-15, 1e-3)
    return d, g, vol


@pytest.mark.parametrize("mode", [W.MIN, W.VAN_DRIEST])
def test_damped_law_against_longdouble_and_its_limits(mode):
    d, g, vol = law_inputs()
    kw = dict(rho=1000.0, mu=1e-3, cs=0.17, kappa=0.41, a_plus=26.0, u_tau=0.05)
    m = W.damped_law(mode, g, vol, d, **kw)
    ml = W.damped_law(mode, g, vol, d, dtype=np.longdouble, **kw)
    err = np.abs(m.astype(np.longdouble) - ml) / ml
    print("mode %d: worst error %.2f x 2^-52" % (mode, float(err.max()) / W.EPS))
    assert float(err.max()) <= 16 * W.EPS
    plain = W.damped_law(W.NONE, g, vol, d, **kw)
    assert np.all(m <= plain) and np.count_nonzero(m < plain) > len(m) // 4
    # d = inf: the undamped value in every bit; NONE is the Smagorinsky law of tests/viscosity_restatement.py
    assert same_bits(W.damped_law(mode, g, vol, np.full(len(g), np.inf), **kw), plain)
    import viscosity_restatement as V
    assert same_bits(plain, V.law(V.params(V.SMAGORINSKY, cs=0.17), g, vol, 1000.0, 1e-3))
    # at the wall the eddy viscosity vanishes
    assert same_bits(W.damped_law(mode, g, vol, np.zeros(len(g)), **kw), np.full(len(g), 1e-3))
