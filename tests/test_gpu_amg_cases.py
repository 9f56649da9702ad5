"""The AMG set-up on user matrices (tests/amg_cases.py): every LDS tier of the Galerkin merge, the candidate limit and its refusal, rows far
longer than the lanes that walk them, preference lists hundreds of entries deep, ties — pairing and coarse operator bit for bit.

Per case, through amg_coarsen (one level of the set-up: da_first_k / da_chase_k / agg_verify_k, galerkin_bound_k / galerkin_merge_k):
  * the pairing equals the Python restatement of the reference's loop (amg_cases.greedy_pairing) exactly;
  * the coarse operator equals the oracle's (R a) R^T in pattern, column order and every bit (zeros and their signs included), and on the
    dyadic cases scipy's exact product as well;
  * orc_debug_amg_setup_stats says the pairing was CERTIFIED, not rescued — no chain cut, no row the certifying pass would change, no
    fallback sweep: aggregate() repairs a wrong pairing by slice-sequential sweeps, so the result alone cannot show a broken da_chase_k —
    with the lanes per chain, the coarse rows per tier and the largest candidate count that amg_cases.predicted derives from the matrix.
The forms (ORC_AMG_DA=0, ORC_AMG_DA_STEPS=3, ORC_AMG_DA_GROUP, ORC_GALERKIN_GROUPS), the second level and two whole Multigrid solves in the
reference's reduction order follow.  Every comparison is exact.  tests/test_amg_cases_cpu.py guards what each case is in the table for."""
import numpy as np
import pytest

import amg_cases as AC
from conftest import fv_like_matrix

pytestmark = pytest.mark.gpu

MULTIGRID, PRE_JACOBI = 2, 1
ORC_ERR_BAD_ARGUMENT = 10

_ORACLE = {}
_DEVICE = {}


def oracle_coarse(oracle, key, a):
    """(R, (R a) R^T) of the oracle as scipy matrices, computed once per key"""
    if key not in _ORACLE:
        A = oracle.Csr.from_scipy(a)
        R = oracle.build_restriction_matrix(A)
        ref = R.matmul(A).matmul(R.transpose()).to_scipy()
        for x in (ref.data, ref.indices, ref.indptr):
            x.setflags(write=False)
        _ORACLE[key] = (R.to_scipy(), ref)
    return _ORACLE[key]


def coarsen(a):
    """(partner, coarse operator, rounds, statistics of that set-up)"""
    from orc_amd.linear_algebra import amg_coarsen, amg_setup_stats
    amg_setup_stats(reset=True)
    partner, ac, rounds = amg_coarsen(a)
    return partner, ac, rounds, amg_setup_stats()


def default_form(name):
    """the case through the set-up as it ships (no switch set), once"""
    if name not in _DEVICE:
        _DEVICE[name] = coarsen(AC.CASES[name].build())
    return _DEVICE[name]


def assert_same_csr(x, y, what):
    assert x.shape == y.shape, what
    assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices), what + ": pattern or column order"
    assert np.array_equal(x.data, y.data), what + ": values"
    assert np.array_equal(x.data == 0.0, y.data == 0.0) and np.array_equal(np.signbit(x.data), np.signbit(y.data)), what + ": zeros or their signs"


def expected_lanes(a):
    """amg_pairing.hip aggregate(): 4 lanes per chain when the SELL-64 image holds at most 24 entries per row on average, else 8"""
    n = a.shape[0]
    lens = np.zeros(((n + 63) // 64) * 64, np.int64)
    lens[:n] = np.diff(a.indptr)
    padded = int(lens.reshape(-1, 64).max(axis=1).sum()) * 64
    return 4 if padded / n <= 24.0 else 8


def assert_certified(stats, lanes=None):
    assert stats["overflow"] == 0 and stats["changed"] == 0 and stats["fallback"] == 0 and stats["fallback_sweeps"] == 0, stats
    if lanes is not None:
        assert stats["lanes"] == lanes, stats


def assert_level(oracle, key, a, partner, ac, dyadic):
    """partner and ac against the restatement, the oracle and (dyadic) exact arithmetic; returns the restatement's pairing"""
    want, _ = AC.pairing(key) if key in AC.CASES else AC.greedy_pairing(a)
    assert np.array_equal(partner, want), "%s: %d rows paired differently" % (key, int((partner != want).sum()))
    R, ref = oracle_coarse(oracle, key, a)
    r = AC.restriction(partner, a.shape[0])
    R.sort_indices()
    assert np.array_equal(r.indptr, R.indptr) and np.array_equal(r.indices, R.indices) and np.array_equal(r.data, R.data)
    assert_same_csr(ac, ref, "%s against the oracle" % key)
    if dyadic:
        assert_same_csr(ac, AC.exact_coarse(a, want), "%s against the exact product" % key)
    return want


def assert_tiers(stats, a, want):
    c, hist, _ = AC.predicted(a, want)
    tiers = hist[:AC.N_TIERS].copy()
    tiers[AC.N_TIERS - 1] += hist[AC.REFUSED]  # galerkin_bound_k's tier stops at the last one
    assert stats["tiers"] == tiers.tolist(), (stats["tiers"], tiers.tolist())
    assert stats["max_cand"] == int(c.max(initial=0)), stats


# ------------------------------------------------------------------ every case, as the set-up ships
@pytest.mark.parametrize("name", AC.COARSENED)
def test_pairing_and_coarse_operator_bit_exact_and_certified(gpu, oracle, name):
    case = AC.CASES[name]
    a = case.build()
    partner, ac, rounds, stats = default_form(name)
    print(name, stats)
    want = assert_level(oracle, name, a, partner, ac, case.expect["dyadic"])
    assert_certified(stats, expected_lanes(a))
    assert rounds == 1
    assert_tiers(stats, a, want)
    assert stats["steps"] >= stats["scans"] >= 0 and stats["longest"] <= stats["steps"]
    if name in AC.SCANNING:
        assert stats["scans"] > 0, stats
    if case.expect.get("empty_coarse"):
        assert (np.diff(ac.indptr) == 0).any()


def test_every_tier_is_reported_non_empty(gpu):
    total = np.zeros(AC.N_TIERS, np.int64)
    for name in AC.COARSENED:
        total += np.array(default_form(name)[3]["tiers"])
    assert (total > 0).all(), total.tolist()
    assert default_form("ladder_shared")[3]["tiers"] == AC.prediction("ladder_shared")[1][:AC.N_TIERS].tolist() and min(default_form("ladder_shared")[3]["tiers"]) > 0
    assert default_form("dense_at_limit")[3]["max_cand"] == AC.CAND_LIMIT and default_form("dense_at_limit")[3]["tiers"][6] == 256


def test_refusal_above_the_candidate_limit_and_the_next_set_up(gpu, oracle):
    """dense_over_limit: coarse rows of 2056 candidates do not fit the widest LDS tier; the set-up refuses before any merge launch (the
    check precedes the tier loop of galerkin()) with ORC_ERR_BAD_ARGUMENT, and the next set-up of the process is as good as ever"""
    from orc_amd._lib import OrcError
    from orc_amd.linear_algebra import amg_setup_stats
    a = AC.CASES[AC.REFUSED_CASE].build()
    with pytest.raises(OrcError) as err:
        coarsen(a)
    assert err.value.status == ORC_ERR_BAD_ARGUMENT
    assert "too long" in str(err.value) and "2056" in str(err.value)
    stats = amg_setup_stats()
    assert_certified(stats, expected_lanes(a))  # the pairing itself went through
    assert stats["scans"] > 0
    assert_tiers(stats, a, AC.pairing(AC.REFUSED_CASE)[0])
    assert stats["max_cand"] == 2056 and stats["tiers"][6] == 257
    b = fv_like_matrix(7, 5, 3)
    partner, ac, rounds, stats = coarsen(b)
    want = assert_level(oracle, "fv_7_5_3", b, partner, ac, False)
    assert_certified(stats, 4)
    assert_tiers(stats, b, want)


# ------------------------------------------------------------------ the forms of the set-up
FORMS = {
    "da_off": {"ORC_AMG_DA": "0"},
    "da_steps_3": {"ORC_AMG_DA_STEPS": "3"},
    "da_group_4": {"ORC_AMG_DA_GROUP": "4"},    # two-sweep scan beyond 32 entries
    "da_group_8": {"ORC_AMG_DA_GROUP": "8"},    # ... 64
    "da_group_16": {"ORC_AMG_DA_GROUP": "16"},  # ... 128
    "merge_64": {"ORC_GALERKIN_GROUPS": "64,64,64,64,64,64,64"},
    "merge_16": {"ORC_GALERKIN_GROUPS": "16,16,16,16,16,16,16"},  # (widened where a wavefront's lists would not fit the LDS)
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", AC.FORM_CASES)
def test_set_up_forms_agree_on_user_matrices(gpu, oracle, monkeypatch, name, form):
    """every form bit-identical to the default form and to the oracle; the statistics tell the forms apart — with every chain cut after
    three proposals the hook must SHOW the rescue (overflow, fallback sweeps), which proves it can see one"""
    case = AC.CASES[name]
    a = case.build()
    p0, a0, _, _ = default_form(name)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    partner, ac, rounds, stats = coarsen(a)
    print(name, form, stats)
    assert np.array_equal(partner, p0)
    assert_same_csr(ac, a0, "%s %s against the default form" % (name, form))
    want = assert_level(oracle, name, a, partner, ac, case.expect["dyadic"])
    assert_tiers(stats, a, want)
    if form == "da_off":
        assert stats["lanes"] == 0 and stats["steps"] == 0 and stats["fallback"] == 1 and rounds == stats["fallback_sweeps"] >= 1, stats
    elif form == "da_steps_3":
        assert stats["overflow"] > 0 and stats["fallback"] == 1 and rounds == stats["fallback_sweeps"] >= 1, stats
        assert stats["longest"] <= 3
    elif form.startswith("da_group_"):
        assert_certified(stats, int(form.rsplit("_", 1)[1]))
        assert rounds == 1
    else:
        assert_certified(stats, expected_lanes(a))


# ------------------------------------------------------------------ the second level
@pytest.mark.parametrize("name", AC.SECOND_LEVEL)
def test_second_level_bit_exact_and_certified(gpu, oracle, name):
    """the coarse operator of the case through the set-up again: rows that mix the fine level's short and long rows"""
    case = AC.CASES[name]
    _, a1, _, _ = default_form(name)
    assert_same_csr(a1, oracle_coarse(oracle, name, case.build())[1], name)
    partner, a2, rounds, stats = coarsen(a1)
    print(name, "level 2", stats)
    want = assert_level(oracle, name + "/2", a1, partner, a2, case.expect["dyadic"])
    assert_certified(stats, expected_lanes(a1))
    assert rounds == 1
    assert_tiers(stats, a1, want)


# ------------------------------------------------------------------ the whole arm on a user matrix
@pytest.mark.parametrize("name", AC.END_TO_END)
def test_multigrid_arm_reference_order_bit_exact_on_a_user_matrix(gpu, oracle, name):
    """band_33 and ladder_random made strictly diagonally dominant, b = a x*: three iterations of the Multigrid arm with the Jacobi
    preconditioner in the reference's reduction order, status and every bit of x against the oracle — the scaled views (s1, s2) through the
    long-row scan and the wide tiers.  The second case is skipped if the oracle does not finish it with status 0 (as built here the oracle
    returns 0 for both, tests/test_amg_cases_cpu.py::test_dominant_systems_of_the_end_to_end_runs holds the systems: the skip does not fire)."""
    from orc_amd.linear_algebra import amg_setup_stats, iterative_solve, set_breakdown_guard, set_reduction_order
    a, b, x0 = AC.end_to_end_system(name)
    xo = x0.copy()
    sto = oracle.iterative_solve(oracle.Csr.from_scipy(a), b, xo, 3, MULTIGRID, 0.5, 1e-3, PRE_JACOBI)
    if name == AC.END_TO_END[1] and sto != 0:
        pytest.skip("the oracle ends %s with status %d" % (name, sto))
    assert sto == 0 and np.isfinite(xo).all()
    set_reduction_order(1)
    set_breakdown_guard(False)  # the reference has no guard (linear_algebra.rs:255-268)
    try:
        x = x0.copy()
        amg_setup_stats(reset=True)
        st = iterative_solve(a, b, x, 3, MULTIGRID, 0.5, 1e-3, PRE_JACOBI, raise_on_error=False)
        stats = amg_setup_stats()
    finally:
        set_reduction_order(0)
        set_breakdown_guard(True)
    assert st == 0
    assert np.array_equal(x.view(np.uint64), xo.view(np.uint64)), "%d of %d entries differ" % (int((x != xo).sum()), len(x))
    assert_certified(stats)  # the last (coarsest) set-up of the hierarchy
    assert sum(stats["tiers"]) > 0
