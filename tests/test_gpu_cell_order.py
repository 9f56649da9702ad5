"""The cell-order boundary of the library (orc_amd/csrc/cell_order.hpp) on an internally reordered mesh: every entry that takes or
returns a per-cell array speaks the caller's ORC order although orc_mesh_create_reordered renumbers the cells inside.

One 7 x 6 x 5 channel (210 cells) whose cells were renumbered by a fixed permutation, once as it is (`plain`) and once with the
internal RCM ordering (`reordered`).  Every input holds pairwise distinct values (splitmix64 of the cell index), so that a wrong or a
missing permutation cannot pass by accident.  Round trips are bit for bit; results on `reordered` against `plain` are bit for bit as
well, because renumber_cells and the internal reordering keep the face ids and every cell's ascending face list: each cell sums the
same terms in the same order.  The assembly entries and calculate_gradients answer in the INTERNAL order (include/orc_amd.h): their
row c on `reordered` is row g[c] on `plain`, g = cell_order()."""
import numpy as np
import pytest

from conftest import splitmix64_uniform

pytestmark = pytest.mark.gpu

RHO, MU = 1000.0, 1e-3
ORIGIN = (1e-3, 5e-4, 2e-4)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def distinct(n, seed, scale=1.0, offset=0.0):
    x = offset + scale * splitmix64_uniform(n, seed)
    assert len(np.unique(x)) == n
    return x


@pytest.fixture(scope="module")
def case(gpu):
    from orc_amd.mesh import Mesh, hex_channel, renumber_cells, set_channel_bcs
    a = set_channel_bcs(hex_channel(7, 6, 5))
    n = a.n_cells
    assert n == 210
    sh = renumber_cells(a, np.argsort(splitmix64_uniform(n, 5), kind="stable").astype(np.int64))
    plain, reordered = Mesh(sh), Mesh(sh, ordering=1)
    g = reordered.cell_order()
    assert not np.array_equal(g, np.arange(n)) and np.array_equal(np.sort(g), np.arange(n))
    assert np.array_equal(plain.cell_order(), np.arange(n))
    fields = (distinct(n, 1, 0.025, 0.05), distinct(n, 2, 0.015), distinct(n, 3, 0.01), distinct(n, 4, 0.01))
    return sh, plain, reordered, g, fields


def solver(mesh, fields=None, **kw):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import Solver
    s = Solver(mesh, NumericalSettings.default(**kw), RHO, MU)
    if fields is not None:
        s.set_fields(*fields)
    return s


# ------------------------------------------------------------------ 1. round trips on the reordered mesh, bit for bit
def test_fields_round_trip(case):
    _, _, reordered, _, fields = case
    s = solver(reordered, fields)
    for got, want in zip(s.get_fields(), fields):
        assert same_bits(got, want)


def test_scalar_field_round_trip(case):
    from orc_amd.settings import ScalarSettings
    _, _, reordered, _, fields = case
    s = solver(reordered, fields)
    s.set_scalar(ScalarSettings.default())
    phi = distinct(reordered.n_cells, 21, 0.5, 0.5)
    s.set_scalar_field(phi)
    assert same_bits(s.get_scalar_field(), phi)


def test_viscosity_field_round_trip(case):
    from orc_amd.settings import Viscosity, ViscosityModel
    _, _, reordered, _, fields = case
    s = solver(reordered, fields)
    mu = distinct(reordered.n_cells, 22, 4e-4, 1e-3)
    s.set_viscosity_field(mu)
    s.set_viscosity(Viscosity.make(ViscosityModel.FIELD))
    assert same_bits(s.viscosity(), mu)
    mu2 = distinct(reordered.n_cells, 23, 4e-4, 1e-3)  # the arm is on: the new field is the assembly's at once
    s.set_viscosity_field(mu2)
    assert same_bits(s.viscosity(), mu2)


def test_statistics_state_round_trip(case):
    from orc_amd.settings import TimeStatistics
    _, _, reordered, _, fields = case
    n = reordered.n_cells
    s = solver(reordered, fields)
    s.set_time_statistics(TimeStatistics.make())
    names = s.statistics_fields()
    assert len(names) == 11  # MEAN | STRESS
    raw = distinct(len(names) * n, 24).reshape(len(names), n)
    s.set_statistics_state(dict(samples=3, weight_sum=1.5, names=names, raw=raw, boundary=None))
    state = s.statistics_state()
    assert state["samples"] == 3 and state["weight_sum"] == 1.5 and state["names"] == names and state["boundary"] is None
    assert same_bits(state["raw"], raw)
    got = s.statistics(normalised=False)
    for k, name in enumerate(names):
        assert same_bits(got[name], raw[k]), name


# ------------------------------------------------------------------ 2. results on the reordered mesh against the plain one, ORC order
def test_derived_fields_equal_the_plain_mesh(case):
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import DERIVED_NAMES, derived_fields
    _, plain, reordered, _, fields = case
    st = NumericalSettings.default()
    want, got = derived_fields(plain, *fields[:3], st, DERIVED_NAMES), derived_fields(reordered, *fields[:3], st, DERIVED_NAMES)
    resident = solver(reordered, fields).derived_fields(DERIVED_NAMES)
    assert list(want) == list(DERIVED_NAMES)
    for name in DERIVED_NAMES:
        assert np.any(want[name] != 0.0), name
        assert same_bits(got[name], want[name]), name
        assert same_bits(resident[name], want[name]), name


def test_surface_integrals_equal_the_plain_mesh(case):
    from orc_amd.solver import surface_integrals
    _, plain, reordered, g, fields = case
    want, got = surface_integrals(plain, *fields, RHO, MU, origin=ORIGIN), surface_integrals(reordered, *fields, RHO, MU, origin=ORIGIN)
    assert np.all(want.faces[1:] > 0)  # every boundary zone reports
    assert same_bits(got.raw, want.raw)
    # the report sees the cell order: the fields of the internal order, unpermuted, give another one
    assert not same_bits(surface_integrals(plain, *[f[g] for f in fields], RHO, MU, origin=ORIGIN).raw, want.raw)


def test_boundary_fields_equal_the_plain_mesh(case):
    from orc_amd.solver import BOUNDARY_NAMES, boundary_fields
    _, plain, reordered, _, fields = case
    want, got = boundary_fields(plain, *fields, RHO, MU), boundary_fields(reordered, *fields, RHO, MU)
    assert np.array_equal(got.zone_ptr, want.zone_ptr) and np.array_equal(got.faces, want.faces) and len(want.faces) > 0
    for name in BOUNDARY_NAMES:
        assert same_bits(got[name], want[name]), name


# ------------------------------------------------------------------ 3. one-way setters, seen through a per-cell result (internal order)
def test_time_levels_reach_the_momentum_assembly(case):
    from orc_amd.settings import TimeScheme, Transient
    _, plain, reordered, g, fields = case
    n = plain.n_cells
    levels = [distinct(n, 31 + k, 0.02, 0.03) for k in range(6)]
    b = []
    for mesh in (plain, reordered):
        s = solver(mesh, fields)
        s.set_transient(Transient.make(2.5e-3, TimeScheme.BDF2, 1))
        s.set_time_levels(*levels)
        b.append(s.assemble_momentum()[3:6])
    for k in range(3):
        assert len(np.unique(b[0][k])) == n
        assert same_bits(b[1][k], b[0][k][g]), "b_" + "uvw"[k]
    # the levels are in those right-hand sides: without them (0 known levels, no time term) they are others
    s = solver(plain, fields)
    s.set_transient(Transient.make(2.5e-3, TimeScheme.BDF2, 1))
    assert not same_bits(s.assemble_momentum()[3], b[0][0])


def test_scalar_source_and_levels_reach_the_scalar_assembly(case):
    from orc_amd.settings import ScalarSettings, TimeScheme, Transient
    _, plain, reordered, g, fields = case
    n = plain.n_cells
    phi, src = distinct(n, 41, 0.5, 0.5), distinct(n, 42, 3.0)
    lv = [distinct(n, 43, 0.4, 0.6), distinct(n, 44, 0.4, 0.6)]

    def rhs(mesh, source, levels):
        s = solver(mesh, fields, velocity_interpolation=0)  # Linear: Rhie-Chow would need a momentum assembly's diagonals first
        s.set_scalar(ScalarSettings.default())
        s.set_scalar_field(phi)
        s.set_transient(Transient.make(2.5e-3, TimeScheme.BDF2, 1))
        if source is not None:
            s.set_scalar_source(source)
        if levels is not None:
            s.set_scalar_levels(*levels)
        return s.assemble_scalar()[1]

    want, got = rhs(plain, src, lv), rhs(reordered, src, lv)
    assert len(np.unique(want)) == n
    assert same_bits(got, want[g])
    # each of the two setters is in that right-hand side
    assert not same_bits(rhs(plain, None, lv), want) and not same_bits(rhs(plain, src, None), want)
    assert same_bits(rhs(reordered, None, lv), rhs(plain, None, lv)[g])
    assert same_bits(rhs(reordered, src, None), rhs(plain, src, None)[g])


# ------------------------------------------------------------------ 4. entries that stay mixed
def test_calculate_gradients_takes_orc_order_and_answers_in_internal_order(case):
    """orc_calculate_gradients on a reordered mesh: fields in ORC order in, gradients in the mesh's internal order out."""
    from orc_amd.settings import NumericalSettings
    from orc_amd.solver import calculate_gradients
    _, plain, reordered, g, fields = case
    st = NumericalSettings.default()
    gp0, gu0 = calculate_gradients(plain, *fields, st)
    gp1, gu1 = calculate_gradients(reordered, *fields, st)
    assert np.all(np.any(gp0 != 0.0, axis=1)) and np.all(np.any(gu0.reshape(-1, 9) != 0.0, axis=1))
    assert same_bits(gp1, gp0[g]) and same_bits(gu1, gu0[g])
    assert not same_bits(gp1, gp0)
