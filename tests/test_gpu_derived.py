"""Derived cell fields and boundary-face maps (orc_solver_derived_fields, orc_derived_fields, orc_solver_boundary_fields,
orc_boundary_fields; orc_amd/csrc/derived.hip) on the device against the numpy restatement (tests/derived_restatement.py), bit for
bit: both gradient arms, every mask's packing with guard words, every supported zone type on the hex, mixed and polyhedral meshes,
the per-zone sums against the surface report, the live solver state (read-only, repeatable), argument checking, two ranks on one GPU
and a solve written to .vtu files and read back.

Bit for bit means equal uint64 views.  The only tolerances are derived: the per-zone sums of face values against the surface
report within (faces + 4) EPS sum|term| (the report's tree and two more roundings per term: the traction is the viscous term over A,
summed here times A again), and the two-rank run within twice derived_restatement.field_bounds().
Two ranks: the owned-cell results were bit-identical to the single-rank restatement in the run recorded in DESIGN.md §3."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import derived_restatement as D
import surface_restatement as R
from conftest import ROOT
from test_gpu_surface import HEX_TYPES, MIXED_TYPES, RHO, MU, channel_solver, hex_case, mixed_case, seeded_fields
from test_vtu_cpu import bits, cell_array, read_vtu

pytestmark = pytest.mark.gpu

BICGSTAB = 3
BAD_ARGUMENT, UNSUPPORTED_BC = 10, 7
GREEN_GAUSS, LEAST_SQUARES = 0, 2
F64 = C.POINTER(C.c_double)
GUARD = 16
MASKS = [1 << k for k in range(8)] + [0xFF, 0b10100101]
MESHES = ["hex", "hex_rcm", "hex211", "mixed", "poly"]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def build(tmp_path, name):
    if name == "hex":
        return hex_case(13, 7, 5)
    if name == "hex_rcm":
        return hex_case(13, 7, 5, ordering=1)
    if name == "hex211":
        return hex_case(2, 1, 1)
    return mixed_case(tmp_path, name == "poly")


def settings_for(arm):
    from orc_amd.settings import NumericalSettings
    return NumericalSettings.default(solver_type=BICGSTAB, gradient_reconstruction=arm)


def p64(x):
    return x.ctypes.data_as(F64)


def raw_derived(m, f, settings, mask):
    """the C entry with guard words behind popcount(mask) * n doubles -> (status, the block [k, n])"""
    from orc_amd._lib import lib
    n, k = m.n_cells, bin(mask).count("1")
    buf = np.full(k * n + GUARD, -77.25)
    u, v, w = (np.ascontiguousarray(x) for x in f[:3])
    st = lib().orc_derived_fields(m.ptr, p64(u), p64(v), p64(w), C.byref(settings), C.c_uint32(mask), p64(buf))
    assert np.all(buf[k * n:] == -77.25), "memory past popcount * n was written"
    return st, buf[:k * n].reshape(k, n)


# ------------------------------------------------------------------ 1. cell fields, both arms, every mask
@pytest.mark.parametrize("arm", [GREEN_GAUSS, LEAST_SQUARES], ids=["green_gauss", "least_squares"])
@pytest.mark.parametrize("mesh_name", MESHES)
def test_cell_fields_equal_the_restatement_bit_for_bit(gpu, tmp_path, mesh_name, arm):
    from orc_amd.mesh import Mesh
    from orc_amd.solver import calculate_gradients, derived_fields
    a, m = build(tmp_path, mesh_name)
    if mesh_name == "hex_rcm":
        assert not np.array_equal(m.cell_order(), np.arange(a.n_cells))
    assert a.n_cells > 256 or mesh_name == "hex211"  # two workgroups and a ragged tail
    f = seeded_fields(a)
    s = settings_for(arm)
    # the gradient orc_calculate_gradients returns (on the mesh in ORC's own numbering), through the table formulas
    _, gu = calculate_gradients(Mesh(a), *f, s)
    vol = np.asarray(a["cell_volume"])
    want = D.fields(gu, D.convective_sum(a, *f[:3]), vol)
    if arm == GREEN_GAUSS:  # and the independent restatement of the gradient itself
        own = D.cell_fields(a, *f[:3])
        assert same_bits(own, want)
    assert np.all(np.isfinite(want)) and np.all(np.abs(want).max(axis=1) > 0)
    for mask in MASKS:
        st, got = raw_derived(m, f, s, mask)
        assert st == 0
        assert same_bits(got, D.select(want, mask)), (mesh_name, arm, bin(mask))
    # the Python surface: names, the (n, 3) vorticity
    d = derived_fields(m, *f[:3], s, ["vorticity", "q_criterion", "convective_rate"])
    assert same_bits(d["vorticity"], want[:3].T) and same_bits(d["q_criterion"], want[D.Q_CRITERION])
    assert same_bits(d["convective_rate"], want[D.CONVECTIVE_RATE])
    assert list(derived_fields(m, *f[:3], s, 0b101)) == ["vorticity_x", "vorticity_z"]


# ------------------------------------------------------------------ 2. boundary maps
@pytest.mark.parametrize("mesh_name", MESHES)
def test_boundary_fields_equal_the_restatement_and_sum_to_the_report(gpu, tmp_path, mesh_name):
    from orc_amd._lib import lib
    from orc_amd.solver import BOUNDARY_NAMES, boundary_fields, surface_integrals
    a, m = build(tmp_path, mesh_name)
    f = seeded_fields(a)
    zp, faces, want = D.boundary_fields(a, *f, RHO, MU)
    bf = boundary_fields(m, *f, RHO, MU)
    assert np.array_equal(bf.zone_ptr, zp) and np.array_equal(bf.faces, faces)
    assert np.array_equal(m.boundary_index()[1], faces)
    for k, name in enumerate(BOUNDARY_NAMES):
        assert same_bits(bf[name], want[k]), (mesh_name, name)
    present = set(int(t) for z, t in enumerate(a["zone_type"]) if zp[z + 1] > zp[z])
    if mesh_name != "hex211":
        assert present == set(R.SUPPORTED)
    assert np.abs(want[D.B_SHEAR_MAG]).max() > 0 and np.abs(want[D.B_Y_PLUS]).max() > 0 and np.abs(want[D.B_MASS_FLUX]).max() > 0
    # masks: packing, order, guard words
    nb = len(faces)
    fields = [np.ascontiguousarray(x) for x in f]
    for mask in (0b1, 0b10000000, 0b10100101, 0xFF):
        k = bin(mask).count("1")
        buf = np.full(k * nb + GUARD, -77.25)
        assert lib().orc_boundary_fields(m.ptr, *[p64(x) for x in fields], RHO, MU, C.c_uint32(mask), p64(buf)) == 0
        assert np.all(buf[k * nb:] == -77.25)
        assert same_bits(buf[:k * nb].reshape(k, nb), D.select(want, mask)), bin(mask)
    # per zone: the sums of the face values times A are the surface report's, within (faces + 4) EPS sum|term|
    rep = surface_integrals(m, *f, RHO, MU)
    A = want[D.B_AREA]
    nrm = np.asarray(a["face_normal"]).reshape(-1, 3)[faces]
    zt = np.asarray(a["zone_type"])
    worst = 0.0
    for z in range(len(zt)):
        sl = slice(int(zp[z]), int(zp[z + 1]))
        nf = zp[z + 1] - zp[z]
        if nf == 0:
            continue
        if zt[z] not in (R.WALL, R.VELOCITY_INLET):  # d_f = 0: exact zeros
            assert np.all(want[D.B_TRACTION_X:D.B_Y_PLUS + 1, sl] == 0.0) and np.all(bf["shear_mag"][sl] == 0.0)
            assert np.all(bf["y_plus"][sl] == 0.0) and np.all(bf["traction_x"][sl] == 0.0)
        pairs = [(bf["mass_flux"][sl] * A[sl], rep.mass_flow[z])]
        for c in range(3):
            pairs.append((bf["traction_" + "xyz"[c]][sl] * A[sl], rep.viscous_force[z, c]))
            pairs.append(((bf["pressure"][sl] * A[sl]) * nrm[sl, c], rep.pressure_force[z, c]))
        for term, total in pairs:
            tol = (nf + 4) * R.EPS * math.fsum(np.abs(term).tolist())
            err = abs(math.fsum(term.tolist()) - total)
            assert err <= tol, (mesh_name, z, err, tol)
            worst = max(worst, err / tol if tol > 0 else 0.0)
    print("%s: worst zone-sum error / bound %.3f" % (mesh_name, worst))


# ------------------------------------------------------------------ 3. the live solver state
@pytest.mark.parametrize("ordering", [None, 1], ids=["orc", "rcm"])
def test_solver_form_equals_the_host_form_and_repeats(gpu, ordering):
    from orc_amd.solver import boundary_fields, derived_fields
    a, m, s = channel_solver(ordering)
    s.iterate(2)
    f = s.get_fields()
    from orc_amd.settings import NumericalSettings
    st = NumericalSettings.default(solver_type=BICGSTAB)
    d1, d2 = s.derived_fields(0xFF), s.derived_fields(0xFF)
    host = derived_fields(m, *f[:3], st, 0xFF)
    want = D.cell_fields(a, *f[:3])
    for k, name in enumerate(D.NAMES):
        assert same_bits(d1[name], d2[name]) and same_bits(d1[name], host[name]) and same_bits(d1[name], want[k]), name
    b1, b2 = s.boundary_fields(), s.boundary_fields()
    hostb = boundary_fields(m, *f, 1000.0, 1e-3)
    _, _, wantb = D.boundary_fields(a, *f, 1000.0, 1e-3)
    for k, name in enumerate(D.B_NAMES):
        assert same_bits(b1[name], b2[name]) and same_bits(b1[name], hostb[name]) and same_bits(b1[name], wantb[k]), name
    assert same_bits(b1.zone("TOP_WALL")["shear_mag"], b1["shear_mag"][b1.zone_ptr[a.get_face_zone("TOP_WALL")]:b1.zone_ptr[a.get_face_zone("TOP_WALL") + 1]])
    for x, y in zip(f, s.get_fields()):
        assert same_bits(x, y)


def test_calls_change_no_bit_of_the_solver(gpu):
    """a snapshot, the calls, an iterate — against an iterate from the same snapshot without the calls"""
    a, m, s = channel_solver()
    s.iterate(1)
    s.snapshot()
    st1, rep1 = s.iterate(2, report=True)
    plain = s.get_fields()
    s.restore()
    s.derived_fields(0xFF)
    s.boundary_fields()
    s.derived_fields("vorticity")
    st2, rep2 = s.iterate(2, report=True)
    assert st1 == st2 == 0 and same_bits(rep1, rep2)
    for x, y in zip(plain, s.get_fields()):
        assert same_bits(x, y)


# ------------------------------------------------------------------ 4. arguments and refused zones
def test_bad_arguments_and_refused_zone_types(gpu, tmp_path):
    from orc_amd._lib import lib
    from orc_amd.solver import boundary_fields, derived_fields
    a, m, s = channel_solver()
    f = [np.ascontiguousarray(x) for x in s.get_fields()]
    st = settings_for(GREEN_GAUSS)
    L = lib()
    out = np.zeros(8 * max(m.n_cells, int(m.boundary_index()[0][-1])))
    u, v, w, p = (p64(x) for x in f)
    for mask in (0, 1 << 8, 0x1FF, 1 << 31):
        assert L.orc_solver_derived_fields(s.ptr, C.c_uint32(mask), p64(out)) == BAD_ARGUMENT, mask
        assert L.orc_derived_fields(m.ptr, u, v, w, C.byref(st), C.c_uint32(mask), p64(out)) == BAD_ARGUMENT
        assert L.orc_solver_boundary_fields(s.ptr, C.c_uint32(mask), p64(out)) == BAD_ARGUMENT
        assert L.orc_boundary_fields(m.ptr, u, v, w, p, 1.0, 1.0, C.c_uint32(mask), p64(out)) == BAD_ARGUMENT
    assert L.orc_solver_derived_fields(None, 1, p64(out)) == BAD_ARGUMENT
    assert L.orc_solver_derived_fields(s.ptr, 1, None) == BAD_ARGUMENT
    assert L.orc_derived_fields(None, u, v, w, C.byref(st), 1, p64(out)) == BAD_ARGUMENT
    assert L.orc_derived_fields(m.ptr, None, v, w, C.byref(st), 1, p64(out)) == BAD_ARGUMENT
    assert L.orc_derived_fields(m.ptr, u, v, w, None, 1, p64(out)) == BAD_ARGUMENT
    assert L.orc_derived_fields(m.ptr, u, v, w, C.byref(st), 1, None) == BAD_ARGUMENT
    assert L.orc_solver_boundary_fields(None, 1, p64(out)) == BAD_ARGUMENT
    assert L.orc_solver_boundary_fields(s.ptr, 1, None) == BAD_ARGUMENT
    assert L.orc_boundary_fields(m.ptr, u, v, w, None, 1.0, 1.0, 1, p64(out)) == BAD_ARGUMENT
    for rho, mu in ((0.0, 1e-3), (float("nan"), 1e-3), (1.0, -1.0), (1.0, float("inf"))):
        assert L.orc_boundary_fields(m.ptr, u, v, w, p, rho, mu, 1, p64(out)) == BAD_ARGUMENT
    good = s.derived_fields(0xFF)
    goodb = s.boundary_fields()
    # a type the assembly refuses, then the next valid call
    a.set_zone("OUTLET", R.OUTFLOW)
    m.update_zones()
    assert s.derived_fields(0xFF, raise_on_error=False)[0] == UNSUPPORTED_BC
    assert s.boundary_fields(raise_on_error=False)[0] == UNSUPPORTED_BC
    assert derived_fields(m, *f[:3], settings_for(LEAST_SQUARES), 1, raise_on_error=False)[0] == UNSUPPORTED_BC
    assert boundary_fields(m, *f, 1000.0, 1e-3, raise_on_error=False)[0] == UNSUPPORTED_BC
    a.set_zone("OUTLET", R.PRESSURE_OUTLET, 0.0)
    m.update_zones()
    again = s.derived_fields(0xFF)
    for name in D.NAMES:
        assert same_bits(again[name], good[name])
    for name in D.B_NAMES:
        assert same_bits(s.boundary_fields()[name], goodb[name])


# ------------------------------------------------------------------ 5. two ranks
def test_two_ranks_on_one_gpu(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "derived_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    print(r.stdout[-1500:])
    assert "DERIVED_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ 6. end to end: a solve, two files, read back
@pytest.mark.parametrize("encoding", ["raw", "ascii"])
def test_solve_write_and_read_back(gpu, tmp_path, encoding):
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, set_channel_bcs, write_hex_channel_msh
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    msh = str(tmp_path / "c.msh")
    write_hex_channel_msh(msh, 13, 7, 5)
    md = orc_io.read_mesh(msh)
    a = set_channel_bcs(MeshArrays(md.arrays()), top_wall_velocity=0.01)
    from orc_amd.mesh import Mesh
    m = Mesh(a)
    s = Solver(m, NumericalSettings.default(solver_type=BICGSTAB), 1000.0, 1e-3)
    n = a.n_cells
    s.set_fields(1e-3 * np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n))
    s.iterate(3)
    u, v, w, p = s.get_fields()
    d = s.derived_fields(["vorticity", "vorticity_mag", "strain_rate_mag", "q_criterion", "divergence", "convective_rate"])
    b = s.boundary_fields()
    vol_path, face_path = str(tmp_path / "volume.vtu"), str(tmp_path / "boundary.vtu")
    arrays = dict(d, velocity=np.stack([u, v, w], axis=1), pressure=p)
    orc_io.write_vtu(vol_path, md, arrays, encoding=encoding)
    orc_io.write_vtu_boundary(face_path, md, b, encoding=encoding)
    out = read_vtu(vol_path)
    assert out["n_cells"] == n and set(out["arrays"]["types"][0]) == {12}
    for name, want in arrays.items():
        assert np.array_equal(bits(cell_array(out, name, n)), bits(want)), name
    assert np.abs(d["vorticity_mag"]).max() > 0
    outb = read_vtu(face_path)
    nb = len(b.faces)
    assert outb["n_cells"] == nb and set(outb["arrays"]["types"][0]) == {7}
    for name, want in b.arrays.items():
        assert np.array_equal(bits(cell_array(outb, name, nb)), bits(want)), name
    assert np.array_equal(bits(cell_array(outb, "traction", nb)), bits(np.stack([b["traction_x"], b["traction_y"], b["traction_z"]], axis=1)))
    assert np.abs(b["shear_mag"]).max() > 0
