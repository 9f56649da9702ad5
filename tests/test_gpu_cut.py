"""Cut surfaces on the device (orc_amd/csrc/cut.hip) against the restatement of tests/cut_restatement.py bit for bit in poly_ptr, owner
cells, points, keys and area vectors: planes through hex, mixed and polyhedral meshes in ORC and RCM numbering, a plane on a node
layer, the scan's chunk edge, the node average, smooth and noisy iso-surfaces, the solver's own field, the n-gon prisms at and past
ORC_CUT_MAX_POINTS, NaN, both samplers, flow through a plane, repeatability, arguments and the file of a slice.

Bit for bit means equal uint64 views."""
import ctypes as C
import math

import numpy as np
import pytest

import cut_cases as K
import cut_restatement as CR
from conftest import splitmix64_uniform
from cut_cases import same_bits
from test_vtu_cpu import bits, read_vtu

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
BICGSTAB = 3
RHO, MU = 1000.0, 1e-3
GREEN_GAUSS, LEAST_SQUARES = 0, 2
GUARD, GUARD_VALUE = 16, -77.25
F64, I64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)


def p64(x):
    return x.ctypes.data_as(F64)


def device_case(tmp_path, name, ordering=None):
    from orc_amd.mesh import Mesh
    a, nodes, md = K.host_case(tmp_path, name)
    return a, nodes, md, Mesh(a, ordering=ordering, nodes=md)


def assert_surface(cut, want, what=""):
    assert (cut.n_polygons, cut.n_points) == (len(want["cell"]), len(want["points"])), what
    assert cut.skipped == dict(nonfinite=len(want["nonfinite"]), overflow=len(want["overflow"])), what
    assert np.array_equal(cut.poly_ptr, want["poly_ptr"]), what
    assert np.array_equal(cut.cell, want["cell"]), what
    assert np.array_equal(cut.keys, want["keys"]), what
    assert same_bits(cut.points, want["points"]), (what, "points")
    assert same_bits(cut.area_vector, want["area_vector"]), (what, "area")


def assert_same_cut(x, y):
    assert np.array_equal(x.poly_ptr, y.poly_ptr) and np.array_equal(x.cell, y.cell) and np.array_equal(x.keys, y.keys)
    assert same_bits(x.points, y.points) and same_bits(x.area_vector, y.area_vector) and x.skipped == y.skipped


# ------------------------------------------------------------------ 1. planes
def test_two_hexahedra_cut_through_both_through_one_and_through_none(gpu, tmp_path):
    a, nodes, md, m = device_case(tmp_path, "hex_2x1x1")
    lo, hi = K.box(nodes)
    mid = 0.5 * (lo + hi)
    both = m.slice(mid, (0.0, 1.0, 0.1))
    assert_surface(both, K.restated_plane(a, nodes, mid, (0.0, 1.0, 0.1)))
    assert both.cell.tolist() == [0, 1]
    o = lo + (hi - lo) * np.array([0.2, 0.5, 0.5])
    one = m.slice(o, (1.0, 0.0, 0.0))
    assert_surface(one, K.restated_plane(a, nodes, o, (1.0, 0.0, 0.0)))
    assert len(one) == 1
    none = m.slice(hi + (hi - lo), (1.0, 0.0, 0.0))
    assert (none.n_polygons, none.n_points) == (0, 0) and none.poly_ptr.tolist() == [0]
    assert none.cell.shape == (0,) and none.points.shape == (0, 3) and none.area_vector.shape == (0, 3) and none.keys.shape == (0, 2)
    assert none.welded()[0].shape == (0, 3) and none.integrate(np.zeros((0, 3))) == 0.0


def test_hex_planes_in_both_numberings_and_the_area_of_the_axis_planes(gpu, tmp_path):
    """The area bound.  An axis plane's cut points carry exact node coordinates across the plane, so the polygons tile the cross-section
    exactly and only the fan sums round.  A polygon of k points has k - 2 fan terms ay bz - az by: four coordinate differences, two
    products, their difference and the accumulation, at most 6 roundings of 2^-53 each acting on a part no larger than the polygon's
    own doubled area (the polygons are rectangles, one product of every term is an exact zero) — 3 (k - 2) 2^-52 of the polygon's own
    area, k = 4: 6 2^-52, and summed over the polygons 6 2^-52 of the whole.  math.fsum adds the polygon areas without a further
    rounding.  The cross-section is formed from the node coordinates with two differences and a product: 3 roundings, under 2 2^-52.
    Together 8 2^-52 of the area, whatever P and NP (the issue's (NP + P) 2^-52 is 175 2^-52 here)."""
    a, nodes, md, m = device_case(tmp_path, "hex_13x7x5")
    _, _, _, rcm = device_case(tmp_path, "hex_13x7x5", ordering=1)
    assert not np.array_equal(rcm.cell_order(), np.arange(a.n_cells))
    planes = K.oblique_planes(nodes)[:1] + list(K.axis_planes(nodes))
    for i, (o, n) in enumerate(planes):
        want = K.restated_plane(a, nodes, o, n)
        got = m.slice(o, n)
        assert_surface(got, want, i)
        assert_surface(rcm.slice(o, n), want, (i, "rcm"))
        if i >= 1:
            area = K.cross_section(nodes, 0)
            total = math.fsum(got.area_vector[:, 0].tolist())
            assert np.all(np.diff(got.poly_ptr) == 4)
            print("axis plane %d: |total - area| / area = %.3g x 2^-52" % (i, abs(total - area) / area * 2.0 ** 52))
            assert abs(total - area) <= (3 * (4 - 2) + 2) * 2.0 ** -52 * area, (i, total, area)
            assert np.all(got.area_vector[:, 0] > 0) and len(set(got.cell.tolist())) == len(got) == 7 * 5
    # on the node layer: every cut point is a node of the layer (x_lo + t (x_hi - x_lo) with t = 0 or 1: exact across the plane, one
    # rounding of the difference and one of the sum along it), each polygon once
    on = m.slice(*planes[1])
    x_layer = planes[1][0][0]
    assert np.all(np.abs(on.points[:, 0] - x_layer) <= 2.0 ** -52 * x_layer)
    vert = np.asarray(nodes[0]).reshape(-1, 3)
    on_nodes = np.where(vert[:, 0] == x_layer)[0]
    assert len(on_nodes) == 8 * 6
    assert set(map(tuple, on.welded()[0][:, 1:])) == set(map(tuple, vert[on_nodes][:, 1:]))


@pytest.mark.parametrize("name", ["mixed", "poly"])
def test_mixed_and_polyhedral_channel_two_oblique_planes(gpu, tmp_path, name):
    a, nodes, md, m = device_case(tmp_path, name)
    for o, n in K.oblique_planes(nodes):
        want = K.restated_plane(a, nodes, o, n)
        assert len(want["cell"]) > 20 and want["overflow"] == []
        assert_surface(m.slice(o, n), want)


@pytest.mark.parametrize("extra", [0, 1])
def test_cut_cells_at_the_scan_chunk_and_one_more(gpu, tmp_path, extra):
    """nx x ny x 2 cells with nx ny = the scan's chunk (+ 1), sized from orc_cut_limits, and a plane through one of the two layers: as
    many cut cells as the chunk holds entries (and one more), beside as many cells that are not cut — whole chunks of zero entries
    or zeros between the cut ones, whichever way the layers are numbered."""
    from orc_amd.mesh import cut_limits
    count = cut_limits()["scan_chunk"] + extra
    ny = max(k for k in range(1, 65) if count % k == 0)
    nx = count // ny
    a, nodes, md, m = device_case(tmp_path, "hex_%dx%dx2" % (nx, ny))
    lo, hi = K.box(nodes)
    o = lo + (hi - lo) * np.array([0.5, 0.5, 0.27])
    n = (0.01, -0.02, 1.0)
    want = K.restated_plane(a, nodes, o, n)
    assert len(want["cell"]) == count and a.n_cells == 2 * count and 4 * count > cut_limits()["scan_chunk"]
    assert_surface(m.slice(o, n), want)


def test_more_chunks_than_one_workgroup_of_the_scan_takes_at_once(gpu):
    """96 x 80 x 70 = 537 600 cells: 525 scan chunks (the top scan's workgroup carries over twice), more cells and faces than one pass
    of the grids of the classify and face passes covers (2 048 workgroups of 256), and for the noisy cut more than 256 chunks of points
    as well.  The reference is vectorised numpy on the lattice nodes: cut edges per face, half their sum per cell.  A plane cuts a
    convex cell in one loop, so there poly_ptr and the owners follow from the counts; for noisy node values the polygons of a cell must
    add up to its count."""
    from orc_amd.mesh import Mesh, cut_limits, hex_channel, hex_channel_nodes
    dims = (96, 80, 70)
    a = hex_channel(*dims)
    nodes = hex_channel_nodes(a, *dims)
    m = Mesh(a, nodes=nodes)
    n, chunk = a.n_cells, cut_limits()["scan_chunk"]
    assert n > 256 * chunk and n > 2048 * 256
    vert, fnp, fn = nodes
    quads = fn.reshape(-1, 4)
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])

    def counts_of(d):
        above = d[quads] >= 0.0
        cuts = (above != np.roll(above, 1, axis=1)).sum(axis=1)
        per_cell = np.bincount(c0, weights=cuts, minlength=n) + np.bincount(c1[c1 >= 0], weights=cuts[c1 >= 0], minlength=n)
        assert np.all(per_cell % 2 == 0)
        return (per_cell // 2).astype(np.int64)

    lo, hi = K.box(nodes)
    o, nrm = K.oblique_planes(nodes)[0]
    count = counts_of(CR.plane_d(nodes, o, nrm))
    cut = m.slice(o, nrm)
    cells = np.nonzero(count)[0]
    assert len(cells) > 5000 and cells[-1] - cells[0] > 256 * chunk  # the cut cells lie more than one carry apart
    assert np.array_equal(cut.cell, cells)
    assert np.array_equal(cut.poly_ptr, np.concatenate([[0], np.cumsum(count[cells])]))
    assert cut.skipped == dict(nonfinite=0, overflow=0)
    above = CR.plane_d(nodes, o, nrm) >= 0.0
    assert np.all(above[cut.keys[:, 0]] != above[cut.keys[:, 1]])
    unit = np.asarray(nrm) / np.linalg.norm(nrm)
    assert np.allclose(np.abs((cut.points - o) @ unit).max(), 0.0, atol=1e-12)  # every point on the plane (the box is 2 mm long)
    noise = splitmix64_uniform(len(vert), 31)
    count = counts_of(noise)
    cut = m.cut_nodes(noise, 0.0)
    assert cut.skipped == dict(nonfinite=0, overflow=0) and count.max() <= 12
    assert cut.n_points == count.sum() > 256 * chunk
    sizes = np.diff(cut.poly_ptr)
    assert np.all(sizes >= 3) and np.all(np.diff(cut.cell) >= 0)
    assert np.array_equal(np.bincount(cut.cell, weights=sizes, minlength=n).astype(np.int64), count)
    above = noise >= 0.0
    assert np.all(above[cut.keys[:, 0]] != above[cut.keys[:, 1]])


# ------------------------------------------------------------------ 2. node values and iso-surfaces
@pytest.mark.parametrize("name,ordering", [("hex_13x7x5", None), ("hex_13x7x5", 1), ("mixed", None), ("poly", None), ("poly", 1)])
def test_node_average_bit_for_bit(gpu, tmp_path, name, ordering):
    a, nodes, md, m = device_case(tmp_path, name, ordering)
    phi = 0.3 + splitmix64_uniform(a.n_cells, 17)
    assert same_bits(m.node_average(phi), CR.node_average(a, nodes, phi))


def test_smooth_and_noisy_iso_surfaces(gpu, tmp_path):
    a, nodes, md, m = device_case(tmp_path, "hex_13x7x5")
    table = CR.node_cells(a, nodes)
    phi, level = K.distance_field(a, nodes)
    want = CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, phi, table), level), K.max_points())
    assert len(want["cell"]) > 30
    got = m.isosurface(phi, level)
    assert_surface(got, want, "smooth")
    assert_same_cut(m.cut_nodes(m.node_average(phi), level), got)
    noise = K.noisy_field(a)
    want = CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, noise, table), 0.0), K.max_points())
    assert want["faces_with_four_cuts"] >= 1 and want["cells_with_two_loops"] >= 1
    assert_surface(m.isosurface(noise, 0.0), want, "noisy")
    _, _, _, rcm = device_case(tmp_path, "hex_13x7x5", ordering=1)
    assert_surface(rcm.isosurface(noise, 0.0), want, "noisy rcm")
    # a sphere given at the nodes
    vert = np.asarray(nodes[0]).reshape(-1, 3)
    lo, hi = K.box(nodes)
    r = np.sqrt(((vert - 0.5 * (lo + hi)) ** 2).sum(axis=1))
    assert_surface(m.cut_nodes(r, 2e-4), CR.cut(a, nodes, CR.level_d(r, 2e-4), K.max_points()), "sphere")


def channel_solver(tmp_path, **kw):
    """test_gpu_surface.channel_solver on the 16 x 8 x 4 channel read back from its file, so that the mesh has its nodes"""
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    a, nodes, md, m = device_case(tmp_path, "hex_16x8x4")
    n = a.n_cells
    cc = np.asarray(a["cell_centroid"])
    start = (1e-3 * (1 + 0.1 * splitmix64_uniform(n, 1)), 1e-6 * splitmix64_uniform(n, 2), 1e-7 * splitmix64_uniform(n, 3), -0.01 * (1 - cc[:, 0] / 0.002))
    s = Solver(m, NumericalSettings.default(solver_type=BICGSTAB, **kw), RHO, MU)
    s.set_fields(*start)
    return a, nodes, md, m, s


def test_the_solvers_own_field_without_leaving_the_device(gpu, tmp_path):
    a, nodes, md, m, s = channel_solver(tmp_path)
    s.iterate(3)
    before, report = s.get_fields(), s.surface_report()
    assert np.any(report.raw != 0.0)
    u = before[0]
    level = float(np.median(u))
    mine = s.isosurface("u", level)
    assert len(mine) > 10
    assert_same_cut(mine, m.isosurface(u, level))
    assert_surface(mine, CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, u), level), K.max_points()))
    for b, c in zip(before, s.get_fields()):
        assert same_bits(b, c)
    assert same_bits(s.surface_report().raw, report.raw)


@pytest.mark.parametrize("n", [12, "max+1"])
def test_prism_stack_at_and_past_the_point_cap(gpu, n):
    from orc_amd.mesh import Mesh, MeshArrays
    n = K.max_points() + 1 if n == "max+1" else n
    arrays, nodes = CR.prism_stack(n)
    a = MeshArrays(arrays)
    m = Mesh(a, nodes=nodes)
    o, nrm = (0.0, 0.0, 0.4e-3), (0.0, 0.0, 1.0)
    want = K.restated_plane(a, nodes, o, nrm)
    got = m.slice(o, nrm)
    assert_surface(got, want)
    if n == 12:
        # the base's area from the ring's own coordinates in exact rational arithmetic (shoelace): the cut points of the vertical edges
        # carry those coordinates exactly, so only the fan sum rounds
        from fractions import Fraction
        ring = [(Fraction(float(x)), Fraction(float(y))) for x, y, _ in np.asarray(nodes[0])[:n]]
        base = abs(sum(ring[k][0] * ring[(k + 1) % n][1] - ring[(k + 1) % n][0] * ring[k][1] for k in range(n))) / 2
        assert got.n_polygons == 1 and got.n_points == 12
        assert abs(Fraction(float(got.area_vector[0, 2])) - base) <= (12 + 1) * Fraction(2) ** -52 * base
        assert got.area_vector[0, 0] == 0.0 and got.area_vector[0, 1] == 0.0
    else:
        assert got.n_polygons == 0 and got.skipped == dict(nonfinite=0, overflow=1)
        o2, n2 = (0.0, 0.0, 1e-3), (0.3, 0.0, 1.0)  # oblique through the interior face: each cell carries about half the ring
        assert_surface(m.slice(o2, n2), K.restated_plane(a, nodes, o2, n2))
        ring_of = np.arange(3 * n) // n
        both = m.cut_nodes(np.where(ring_of == 1, 1.0, -1.0), 0.0)  # the middle ring above: every vertical edge of both cells is cut
        assert both.n_polygons == 0 and both.n_points == 0 and both.skipped == dict(nonfinite=0, overflow=2)


def test_a_nan_cell_value_skips_exactly_the_cells_around_its_nodes(gpu, tmp_path):
    a, nodes, md, m = device_case(tmp_path, "hex_13x7x5")
    table = CR.node_cells(a, nodes)
    phi, level = K.distance_field(a, nodes)
    clean = m.isosurface(phi, level)
    bad_cell = int(clean.cell[len(clean) // 2])
    dirty = phi.copy()
    dirty[bad_cell] = np.nan
    want = CR.cut(a, nodes, CR.level_d(CR.node_average(a, nodes, dirty, table), level), K.max_points())
    touched = sorted({c for v, cells in enumerate(table) if bad_cell in cells for c in cells})
    assert want["nonfinite"] == touched and 8 < len(touched) <= 27
    got = m.isosurface(dirty, level)
    assert_surface(got, want)
    keep = ~np.isin(clean.cell, touched)  # the rest of the surface is unchanged
    assert np.array_equal(clean.cell[keep], got.cell)
    rows = np.repeat(keep, np.diff(clean.poly_ptr))
    assert same_bits(clean.points[rows], got.points) and same_bits(clean.area_vector[keep], got.area_vector)


# ------------------------------------------------------------------ 3. sampling
def raw_sample(s, cut, mask, interpolation):
    from orc_amd._lib import lib
    k, n = bin(mask).count("1"), cut.n_points if interpolation else cut.n_polygons
    buf = np.full(k * n + GUARD, GUARD_VALUE)
    assert lib().orc_solver_sample_cut(s.ptr, cut.ptr, C.c_uint32(mask), C.c_int32(interpolation), p64(buf)) == 0
    assert np.all(buf[k * n:] == GUARD_VALUE), "memory past popcount * n was written"
    return buf[:k * n].reshape(k, n)


@pytest.mark.parametrize("recon", [GREEN_GAUSS, LEAST_SQUARES], ids=["green_gauss", "least_squares"])
def test_both_samplers_equal_the_restatement_with_guard_words(gpu, tmp_path, recon):
    from orc_amd._lib import lib
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver, calculate_gradients
    from helpers import seeded_fields
    a, nodes, md, m = device_case(tmp_path, "poly")
    st = NumericalSettings.default(gradient_reconstruction=recon, solver_type=BICGSTAB)
    s = Solver(m, st, RHO, MU)
    f = seeded_fields(a)
    s.set_fields(*f)
    o, n = K.oblique_planes(nodes)[0]
    want = K.restated_plane(a, nodes, o, n)
    cut = m.slice(o, n)
    assert_surface(cut, want)
    gp, gu = calculate_gradients(m, *f, st)
    grads = {"u": gu[:, 0, :], "v": gu[:, 1, :], "w": gu[:, 2, :], "p": gp}
    cell, lin = raw_sample(s, cut, 0xF, 0), raw_sample(s, cut, 0xF, 1)
    for q, (k, phi) in enumerate(zip("uvwp", f)):
        assert same_bits(cell[q], CR.sample_cell(phi, want)), k
        assert same_bits(lin[q], CR.sample_linear(a, phi, grads[k], want)), k
    named = s.sample_cut(cut, ("p", "u"), "linear")
    assert list(named) == ["p", "u"] and same_bits(named["p"], lin[3]) and same_bits(named["u"], lin[0])
    # LINEAR is what orc_solver_sample_probes gives for that cell and point: where the locate of a polygon vertex ends in its owner
    # (a vertex lies on the owner's boundary, so the walk may also stop in a neighbour), the two entries return the same bits
    owner = np.repeat(want["cell"], np.diff(want["poly_ptr"]))
    probes = m.locate(cut.points)
    same_cell = probes.cell == owner
    assert np.count_nonzero(same_cell) > len(owner) // 10
    at_probes = s.sample(probes, ("u", "v", "w", "p"), "linear")
    for q, k in enumerate("uvwp"):
        assert same_bits(at_probes[k][same_cell], lin[q][same_cell]), k
    # the host gather of any cell array
    got = cut.sample_cells({"u": f[0], "p": f[3]})
    assert same_bits(got["u"], cell[0]) and same_bits(got["p"], cell[3])
    buf = np.full(2 * len(cut) + GUARD, GUARD_VALUE)
    src = np.ascontiguousarray(np.stack([f[1], f[2]]))
    assert lib().orc_cut_sample_cells(cut.ptr, 2, p64(src), p64(buf)) == 0
    assert np.all(buf[2 * len(cut):] == GUARD_VALUE) and same_bits(buf[:2 * len(cut)].reshape(2, -1), cell[1:3])
    for b, c in zip(f, s.get_fields()):
        assert same_bits(b, c)


def test_read_out_respects_its_buffers(gpu, tmp_path):
    from orc_amd._lib import lib
    a, nodes, md, m = device_case(tmp_path, "hex_3x2x2")
    o, n = K.oblique_planes(nodes)[0]
    cut = m.slice(o, n)
    P, NP = cut.n_polygons, cut.n_points
    ptr, cell, lo, hi = (np.full(k + GUARD, -7, np.int64) for k in (P + 1, P, NP, NP))
    pts, area = np.full(3 * NP + GUARD, GUARD_VALUE), np.full(3 * P + GUARD, GUARD_VALUE)
    i64 = lambda x: x.ctypes.data_as(I64)
    assert lib().orc_cut_get(cut.ptr, i64(ptr), i64(cell), p64(pts), i64(lo), i64(hi), p64(area)) == 0
    assert np.all(ptr[P + 1:] == -7) and np.all(cell[P:] == -7) and np.all(lo[NP:] == -7) and np.all(hi[NP:] == -7)
    assert np.all(pts[3 * NP:] == GUARD_VALUE) and np.all(area[3 * P:] == GUARD_VALUE)
    assert np.array_equal(ptr[:P + 1], cut.poly_ptr) and same_bits(pts[:3 * NP].reshape(-1, 3), cut.points)
    assert lib().orc_cut_get(cut.ptr, None, None, None, None, None, None) == 0  # every output may be NULL


def test_flow_through_a_plane(gpu, tmp_path):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    from helpers import seeded_fields
    a, nodes, md, m = device_case(tmp_path, "hex_13x7x5")
    s = Solver(m, NumericalSettings.default(solver_type=BICGSTAB), RHO, MU)
    f = seeded_fields(a)
    s.set_fields(*f)
    o, n = K.axis_planes(nodes)[1]
    cut = m.slice(o, n)
    want = K.restated_plane(a, nodes, o, n)
    uvw = s.sample_cut(cut, ("u", "v", "w"), "cell")
    vec = RHO * np.stack([uvw["u"], uvw["v"], uvw["w"]], axis=1)
    terms = CR.flux_terms(RHO * np.stack([f[0][want["cell"]], f[1][want["cell"]], f[2][want["cell"]]], axis=1), want)
    exact = math.fsum(terms.tolist())
    assert abs(cut.integrate(vec) - exact) <= len(cut) * 2.0 ** -52 * math.fsum(np.abs(terms).tolist())
    assert exact > 0  # the normal points toward increasing x, where the seeded u flows


def test_two_cuts_of_one_state_are_bit_identical(gpu, tmp_path):
    a, nodes, md, m = device_case(tmp_path, "poly")
    o, n = K.oblique_planes(nodes)[1]
    assert_same_cut(m.slice(o, n), m.slice(o, n))
    phi = K.noisy_field(a)
    assert_same_cut(m.isosurface(phi, 0.1), m.isosurface(phi, 0.1))


# ------------------------------------------------------------------ 4. arguments and the file
def test_refused_arguments_leave_mesh_and_solver_alone(gpu, tmp_path):
    from orc_amd import parallel
    from orc_amd._lib import OrcError, lib
    from orc_amd.mesh import Mesh
    L = lib()
    a, nodes, md, m, s = channel_solver(tmp_path)
    f = s.get_fields()
    vert, fnp, fn = (np.ascontiguousarray(x) for x in nodes)
    V, F = len(vert), len(fnp) - 1
    i64 = lambda x: x.ctypes.data_as(I64)
    bare = Mesh(a)
    st = C.c_int(0)
    o, n = (C.c_double * 3)(1e-3, 5e-4, 2e-4), (C.c_double * 3)(1.0, 0.0, 0.0)
    # a cut before orc_mesh_set_nodes
    assert L.orc_cut_plane(bare.ptr, o, n, C.byref(st)) is None and st.value == BAD_ARGUMENT
    assert L.orc_mesh_node_average(bare.ptr, p64(f[0]), p64(np.zeros(V))) == BAD_ARGUMENT
    # orc_mesh_set_nodes checks its arrays
    assert L.orc_mesh_set_nodes(bare.ptr, V, p64(vert), F - 1, i64(fnp), i64(fn)) == BAD_ARGUMENT  # F mismatch
    wrong = fn.copy()
    wrong[5] = V
    assert L.orc_mesh_set_nodes(bare.ptr, V, p64(vert), F, i64(fnp), i64(wrong)) == BAD_ARGUMENT  # an index out of range
    wrong[5] = -1
    assert L.orc_mesh_set_nodes(bare.ptr, V, p64(vert), F, i64(fnp), i64(wrong)) == BAD_ARGUMENT
    two = fnp.copy()
    two[1:] -= 2  # the first face keeps 2 nodes
    assert L.orc_mesh_set_nodes(bare.ptr, V, p64(vert), F, i64(two), i64(fn[2:].copy())) == BAD_ARGUMENT
    assert L.orc_mesh_set_nodes(bare.ptr, V, None, F, i64(fnp), i64(fn)) == BAD_ARGUMENT
    assert L.orc_mesh_set_nodes(None, V, p64(vert), F, i64(fnp), i64(fn)) == BAD_ARGUMENT
    assert L.orc_cut_plane(bare.ptr, o, n, C.byref(st)) is None and st.value == BAD_ARGUMENT  # still none
    # a second call on a mesh that has its nodes is checked as the first was: the same arrays change nothing, bad or other ones are refused
    assert L.orc_mesh_set_nodes(m.ptr, V, p64(vert), F, i64(fnp), i64(fn)) == 0
    assert L.orc_mesh_set_nodes(m.ptr, V, p64(vert), F, i64(fnp), i64(wrong)) == BAD_ARGUMENT
    assert L.orc_mesh_set_nodes(m.ptr, V + 1, p64(np.vstack([vert, vert[:1]])), F, i64(fnp), i64(fn)) == BAD_ARGUMENT
    # a partitioned mesh, and the message says why
    ap, halo, _ = parallel.partition_arrays(a, 2, 0)
    with pytest.raises(OrcError) as e:
        parallel.PartitionedMesh(ap, halo).set_nodes(nodes)
    assert e.value.status == BAD_ARGUMENT and "partitioned" in str(e.value)
    other = Mesh(a, nodes=nodes)
    good = m.slice((1e-3, 5e-4, 2e-4), (1.0, 0.0, 0.0))
    foreign = other.slice((1e-3, 5e-4, 2e-4), (1.0, 0.0, 0.0))
    out = np.zeros((6, max(good.n_points, 1)))
    vals = np.zeros(V)

    def made(call):
        st.value = 0
        assert call() is None
        return st.value

    refused = [
        lambda: made(lambda: L.orc_cut_plane(None, o, n, C.byref(st))),
        lambda: made(lambda: L.orc_cut_plane(m.ptr, None, n, C.byref(st))),
        lambda: made(lambda: L.orc_cut_plane(m.ptr, o, (C.c_double * 3)(0.0, 0.0, 0.0), C.byref(st))),
        lambda: made(lambda: L.orc_cut_plane(m.ptr, o, (C.c_double * 3)(0.0, np.nan, 1.0), C.byref(st))),
        lambda: made(lambda: L.orc_cut_plane(m.ptr, o, (C.c_double * 3)(np.inf, 0.0, 1.0), C.byref(st))),
        lambda: made(lambda: L.orc_cut_node_level(m.ptr, None, 0.0, C.byref(st))),
        lambda: made(lambda: L.orc_cut_node_level(m.ptr, p64(vals), np.nan, C.byref(st))),
        lambda: made(lambda: L.orc_cut_cell_field(m.ptr, None, 0.0, C.byref(st))),
        lambda: made(lambda: L.orc_cut_cell_field(m.ptr, p64(f[0]), np.inf, C.byref(st))),
        lambda: made(lambda: L.orc_solver_cut_field(None, 1, 0.0, C.byref(st))),
        lambda: made(lambda: L.orc_solver_cut_field(s.ptr, 0, 0.0, C.byref(st))),
        lambda: made(lambda: L.orc_solver_cut_field(s.ptr, 3, 0.0, C.byref(st))),        # two bits
        lambda: made(lambda: L.orc_solver_cut_field(s.ptr, 1 << 6, 0.0, C.byref(st))),   # an unknown bit
        lambda: made(lambda: L.orc_solver_cut_field(s.ptr, 1 << 4, 0.0, C.byref(st))),   # PHI without the scalar arm
        lambda: made(lambda: L.orc_solver_cut_field(s.ptr, 1, np.nan, C.byref(st))),
        lambda: L.orc_cut_sizes(None, None, None, None, None),
        lambda: L.orc_cut_get(None, None, None, None, None, None, None),
        lambda: L.orc_solver_sample_cut(None, good.ptr, 1, 0, p64(out)),
        lambda: L.orc_solver_sample_cut(s.ptr, None, 1, 0, p64(out)),
        lambda: L.orc_solver_sample_cut(s.ptr, good.ptr, 1, 0, None),
        lambda: s.sample_cut(good, 0, "cell", raise_on_error=False)[0],
        lambda: s.sample_cut(good, 1 << 6, "cell", raise_on_error=False)[0],
        lambda: s.sample_cut(good, "phi", "cell", raise_on_error=False)[0],
        lambda: s.sample_cut(good, "u", 2, raise_on_error=False)[0],
        lambda: s.sample_cut(foreign, "u", "cell", raise_on_error=False)[0],  # a cut of another mesh
        lambda: L.orc_cut_sample_cells(good.ptr, 0, p64(f[0]), p64(out)),
        lambda: L.orc_cut_sample_cells(good.ptr, 1, None, p64(out)),
    ]
    for i, call in enumerate(refused):
        assert call() == BAD_ARGUMENT, i
        for g, w in zip(s.get_fields(), f):
            assert same_bits(g, w)
    assert_same_cut(m.slice((1e-3, 5e-4, 2e-4), (1.0, 0.0, 0.0)), good)  # the mesh cuts as before
    assert_same_cut(m.slice((1e-3, 5e-4, 2e-4), (2.0, 0.0, 0.0)), good)  # the normal need not have unit length (a power of two: the same t)


@pytest.mark.parametrize("encoding", ["ascii", "raw"])
def test_a_slice_of_a_short_solve_written_and_read_back(gpu, tmp_path, encoding):
    from orc_amd import io as orc_io
    a, nodes, md, m, s = channel_solver(tmp_path)
    s.iterate(3)
    o, n = K.oblique_planes(nodes)[0]
    cut = m.slice(o, n)
    cell = s.sample_cut(cut, ("u", "p"), "cell")
    lin = s.sample_cut(cut, ("u", "v", "w"), "linear")
    vel = np.stack([lin["u"], lin["v"], lin["w"]], axis=1)
    path = str(tmp_path / ("slice_%s.vtu" % encoding))
    orc_io.write_vtu_cut(path, cut, cell_data={"u": cell["u"], "p": cell["p"], "area": cut.area}, point_data={"velocity": vel, "u_linear": lin["u"]},
                         encoding=encoding)
    out = read_vtu(path)
    pts, conn, first = cut.welded()
    arr = out["arrays"]
    assert out["n_points"] == len(pts) < cut.n_points and out["n_cells"] == len(cut)
    assert np.array_equal(bits(arr["Points"][0]), bits(pts.reshape(-1)))
    assert arr["connectivity"][0] == conn.tolist() and arr["offsets"][0] == cut.poly_ptr[1:].tolist() and arr["types"][0] == [7] * len(cut)
    assert same_bits(pts[conn], cut.points)  # a key gives the same bits in every cell that shares its edge
    for k in ("u", "p"):
        assert np.array_equal(bits(arr[k][0]), bits(cell[k])), k
    assert np.array_equal(bits(arr["u_linear"][0]), bits(lin["u"][first]))
    assert sorted(out["cell_data"]) == ["area", "p", "u"]
    assert np.array_equal(bits(arr["area"][0]), bits(cut.area))
    assert np.array_equal(bits(arr["velocity"][0]), bits(vel[first].reshape(-1))) and arr["velocity"][1] == 3  # the first polygon in order wins
    # data per welded point, said so: written as given
    per_point = np.arange(len(pts), dtype=np.float64)
    orc_io.write_vtu_cut(path, cut, point_data={"id": per_point}, encoding=encoding, per="point")
    assert np.array_equal(bits(read_vtu(path)["arrays"]["id"][0]), bits(per_point))
    with pytest.raises(ValueError):
        orc_io.write_vtu_cut(path, cut, point_data={"id": per_point}, encoding=encoding)  # per vertex is the default: NP values
