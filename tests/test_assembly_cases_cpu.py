"""What makes a green run of tests/test_gpu_assembly_cases.py mean something, checked without a GPU: every mesh of tests/assembly_cases.py has
the property it is listed for, the fields reach every branch of the limiters, no least-squares system is singular, any two arms of the table
give different bits on the oracle (a device that ignored a setting could not pass), and NaN diagonals (where the existing assembly test
returns before the p' comparison; the new one compares NaN positions instead) occur with the planted fields only."""
import itertools

import numpy as np
import pytest

import assembly_cases as AC
import helpers as H


@pytest.fixture(scope="module")
def cases(oracle):
    """builds the oracle library before assembly_cases imports it"""
    return AC


# ---------------------------------------------------------------- mesh properties
@pytest.mark.parametrize("name", AC.MESHES)
def test_mesh_has_the_property_it_is_listed_for(cases, name):
    om, a = AC.mesh(name)
    why = AC.WHY[name]
    n = om.n_cells
    nf = np.diff(np.asarray(a["cell_face_ptr"]))
    assert set(np.unique(nf).tolist()) == why["faces"]
    if "n" in why:
        assert n == why["n"]
    n_blk = -(-n // AC.BLOCK)
    if "grid" in why:  # grid_for: ceil(n / 256) up to 2 048; a multiple of 8 takes the XCD walk of momentum_k<false>
        assert n_blk == why["grid"] and n_blk <= AC.MAX_GRID and n_blk % 8 == 0
    if "last_block" in why:
        assert n - (n_blk - 1) * AC.BLOCK == why["last_block"]
    if "n_blk" in why:  # more blocks than workgroups: a second round for some, and the last XCD's range cut by n_blk
        per = (n_blk + 7) // 8
        assert n_blk == why["n_blk"] > AC.MAX_GRID and AC.MAX_GRID % 8 == 0
        assert per > AC.MAX_GRID // 8  # 260 (258) blocks per XCD against 256 workgroups: a second round
        assert (8 * per > n_blk) == why["cut"] and (per != n_blk // 8) == why["cut"]  # the last XCD's range ends at n_blk, not at 8 * per
        assert len(a["face_area"]) > AC.MAX_GRID * AC.BLOCK  # the face kernels take a second round too
    if "tri_zone_types" in why:
        assert AC.triangular_zone_types(a) == why["tri_zone_types"]
    if "non_orthogonal" in why:
        f = AC.interior_faces(a)
        d = np.asarray(a["cell_centroid"])[np.asarray(a["face_c1"])[f]] - np.asarray(a["cell_centroid"])[np.asarray(a["face_c0"])[f]]
        cos = np.einsum("ij,ij->i", np.asarray(a["face_normal"])[f], d) / np.linalg.norm(d, axis=1)
        assert cos.min() < 0.98 and (cos < 0.999).mean() > 0.25
    if "reversed_faces" in why:
        f = AC.interior_faces(a)
        assert (np.asarray(a["face_c0"])[f] > np.asarray(a["face_c1"])[f]).mean() > why["reversed_faces"]


def test_every_zone_type_sits_on_triangles_and_on_quadrilaterals(cases):
    every = {H.BC_WALL, H.BC_PINLET, H.BC_POUTLET, H.BC_SYMMETRY, H.BC_VINLET}
    tri, quad = set(), set()
    for name in AC.SMALL_MESHES:
        a = AC.mesh(name)[1]
        tri |= AC.triangular_zone_types(a)
        quad |= AC.quadrilateral_zone_types(a)
    assert tri == every and quad == every
    moving = [np.abs(np.asarray(AC.mesh(name)[1]["zone_vector"])[np.asarray(AC.mesh(name)[1]["zone_type"]) == H.BC_WALL]).max() > 0 for name in AC.MESHES]
    assert all(moving)


def test_the_zones_named_tri_hold_the_triangles(cases, oracle):
    """triangular_zone_types goes by the zone names: a face of three nodes lies in a *_TRI zone and nowhere else"""
    for name in ("tets", "poly_x8", "skew"):
        om = AC.mesh(name)[0]
        c = om.ptr.contents
        nn = np.diff(np.ctypeslib.as_array(c.face_node_ptr, shape=(c.n_faces + 1,)))
        fz = np.ctypeslib.as_array(c.face_zone, shape=(c.n_faces,))
        tri_zone = np.array([nm.endswith("_TRI") for nm in om.zone_names()])
        assert set(np.unique(nn).tolist()) == {3, 4} and np.array_equal(nn == 3, tri_zone[fz])


def test_shuffled_numbering_and_schedule_depth(cases):
    """The generator's numbering has c0 < c1 on every interior face; the shuffled one has both orders, and its level schedule is the
    SHALLOWER one (a random order has short ascending chains): 12 levels against 27."""
    a, s = AC.mesh("poly")[1], AC.mesh("poly_shuffled")[1]
    f = AC.interior_faces(a)
    assert (np.asarray(a["face_c0"])[f] < np.asarray(a["face_c1"])[f]).all()
    assert np.array_equal(np.sort(np.asarray(a["cell_volume"])), np.sort(np.asarray(s["cell_volume"])))
    deep, shallow = AC.level_depth(a), AC.level_depth(s)
    assert deep == 27 and 8 <= shallow < deep, (deep, shallow)


@pytest.mark.parametrize("name", sorted(AC.WEIGHTED_SHARE))
def test_linear_weighted_weights_are_far_from_one_half(cases, name):
    w = AC.weighted_weights(AC.mesh(name)[1])
    assert (np.abs(w - 0.5) > 1e-3).mean() > AC.WEIGHTED_SHARE[name]
    assert w.min() < 0.3 and w.max() > 0.7


def test_linear_weighted_reduces_to_one_half_on_the_hexahedra(cases):
    w = AC.weighted_weights(AC.mesh("hex_x16")[1])
    assert np.abs(w - 0.5).max() < 1e-12


# ---------------------------------------------------------------- limiter census
def _census_cells(name):
    if name not in AC.LARGE_MESHES:
        return None
    n = AC.mesh(name)[0].n_cells  # a sample: every 64th cell and the last 2 048 (the second round of the grid-stride kernels)
    return np.unique(np.concatenate([np.arange(0, n, 64), np.arange(n - 2048, n)]))


@pytest.mark.parametrize("name", AC.MESHES)
def test_rough_fields_reach_every_outcome_of_umist(cases, name):
    a = AC.mesh(name)[1]
    cen = AC.limiter_census(name, AC.fields("rough", a), _census_cells(name))
    for k, label in enumerate(AC.UMIST_OUTCOMES):
        assert (cen["outcome"] == k).sum() >= 20, label
    assert (cen["flux"] > 0).sum() >= 100 and (cen["flux"] < 0).sum() >= 100
    assert not cen["equal"].any()  # no two neighbours share a velocity unless planted


@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_planted_fields_hit_the_intended_cells(cases, name):
    a = AC.mesh(name)[1]
    pl = AC.planted_cells(a)
    nf = np.diff(np.asarray(a["cell_face_ptr"]))
    assert nf[pl["few"][0]] == nf.min() and nf[pl["many"][0]] == nf.max()
    cen = AC.limiter_census(name, AC.fields("planted", a))
    pairs = set(zip(cen["cell"][cen["equal"]].tolist(), cen["nb"][cen["equal"]].tolist()))
    # the flux decides from which side the neighbour is downstream: one of the two visits of each planted face
    assert len(pairs) == 2 and {frozenset(p) for p in pairs} == {frozenset(pl["few"]), frozenset(pl["many"])}
    part = (cen["dv"] == 0).any(axis=1) & ~(cen["dv"] == 0).all(axis=1)
    assert part.sum() == 1
    i = int(np.flatnonzero(part)[0])
    assert {int(cen["cell"][i]), int(cen["nb"][i])} == set(pl["component"])
    assert cen["dv"][i, 0] == 0.0 and not np.isfinite(cen["r"][i, 0]) and np.isfinite(cen["r"][i, 1:]).all()


# ---------------------------------------------------------------- least-squares systems
@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_no_least_squares_system_is_singular(cases, name):
    """oracle_gradients asserts status 0 cell by cell (a singular normal matrix is status != 0); a 4-face cell gives 4 rows for 3 unknowns"""
    a = AC.mesh(name)[1]
    for kind in AC.FIELD_KINDS:
        g = AC.oracle_gradients(name, AC.fields(kind, a))
        assert np.isfinite(g["lsq_p"]).all() and np.isfinite(g["lsq_u"]).all()


def test_no_least_squares_system_is_singular_on_the_large_mesh(cases):
    a = AC.mesh("hex_round2")[1]
    g = AC.oracle_gradients("hex_round2", AC.fields("rough", a), _census_cells("hex_round2"))
    assert np.isfinite(g["lsq_p"]).all() and np.isfinite(g["lsq_u"]).all()


# ---------------------------------------------------------------- arms are distinguishable; the NaN early return is capped
@pytest.fixture(scope="module")
def assembled(cases):
    """{(mesh, kind): {arm: (digest, momentum matrices finite, p' system finite)}}, every oracle run once"""
    out = {}
    for name in AC.SMALL_MESHES:
        a = AC.mesh(name)[1]
        for kind in AC.FIELD_KINDS:
            f = AC.fields(kind, a)
            table = {}
            for arm in AC.ARMS:
                r = AC.oracle_assembly(name, f, arm)
                table[arm] = (AC.digest(r), all(np.isfinite(x).all() for x in r.a), np.isfinite(r.ap).all() and np.isfinite(r.bp).all())
            out[name, kind] = table
    return out


@pytest.mark.parametrize("kind", ["seeded", "rough"])
@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_any_two_arms_differ_in_at_least_one_bit(assembled, name, kind):
    groups = {}
    for arm, (d, _, _) in assembled[name, kind].items():
        groups.setdefault(d, []).append(arm)
    same = {frozenset(g) for g in groups.values() if len(g) > 1}
    assert same == {frozenset(g) for g in AC.IDENTICAL_ARMS}, [[AC.arm_name(x) for x in g] for g in same]


@pytest.mark.parametrize("kind", ["seeded", "rough"])
@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_no_arm_takes_the_nan_path_without_planted_fields(assembled, name, kind):
    bad = [AC.arm_name(arm) for arm, (_, finite, pp_finite) in assembled[name, kind].items() if not (finite and pp_finite)]
    assert not bad


@pytest.mark.parametrize("name", AC.SMALL_MESHES)
def test_planted_fields_give_the_reference_nan_in_lud_and_quick_alone(assembled, name):
    """dv.x == 0 makes r.x infinite; LUD (psi = r) and QUICK ((3 + r) / 4) carry it into a_nb and the diagonal sum turns it
    into NaN; UMIST clamps r, the other schemes never form it.  24 arms of 84."""
    nan = {arm for arm, (_, finite, _) in assembled[name, "planted"].items() if not finite}
    assert nan == {arm for arm in AC.ARMS if arm.momentum in (AC.TVD_LUD, AC.TVD_QUICK)}


@pytest.mark.parametrize("name", AC.LARGE_MESHES)
def test_large_mesh_arm_is_finite(cases, name):
    a = AC.mesh(name)[1]
    r = AC.oracle_assembly(name, AC.fields("rough", a), AC.ROUND2_ARM)
    assert all(np.isfinite(x).all() for x in list(r.a) + list(r.b) + [r.ap, r.bp]) and np.isfinite(r.pe).all()


def test_arm_table_shape():
    assert len(AC.ARMS) == 84 and len(AC.ITERATION_ARMS) == 10
    assert {a.momentum for a in AC.ARMS_A} == set(AC.MOMENTUM) and len({(a.vinterp, a.pinterp) for a in AC.ARMS_A}) == 9
    assert all(a != b for a, b in itertools.combinations(AC.ARMS, 2))
