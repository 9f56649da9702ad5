"""The CG arm's restatement (tests/cg_restatement.py) against scipy and against itself in longdouble over the case table of
tests/cg_cases.py, and the C ABI of the arm and of the p' solver override (enum value, struct size, declared and exported
symbols, no CPU fallback).  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cg_cases as G
import cg_restatement as R
from conftest import ROOT

FAMILIES = [("lap1", 4097), ("lap3", 4097), ("p", 1008)]


def scipy_cg(a, b, x0, k, precond):
    m = sp.diags(1.0 / a.diagonal()) if precond else None
    tol = {"rtol": 0.0} if "rtol" in inspect.signature(spla.cg).parameters else {"tol": 0.0}
    x, _ = spla.cg(a, b, x0=x0.copy(), maxiter=k, M=m, atol=0.0, **tol)
    return x


@pytest.mark.parametrize("family,n", FAMILIES)
@pytest.mark.parametrize("precond", [0, 1])
def test_restatement_converges(family, n, precond):
    a, b = G.system(family, n)
    x = np.zeros(n)
    st = R.cg(a, b, x, 2000, precond, threshold=1e-12)
    assert st["event"] == 0 and st["iterations"] < 2000
    assert np.linalg.norm(b - a @ x) <= 1e-11 * np.linalg.norm(b)
    # the recurrence residual is the true one to rounding, and the direct solve is reached
    assert abs(st["residual"] - np.linalg.norm(b - a @ x)) <= 1e-3 * st["residual"] + 1e-15 * np.linalg.norm(b)
    ref = spla.spsolve(a.tocsc(), b)
    assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref)


@pytest.mark.parametrize("family,n", FAMILIES)
@pytest.mark.parametrize("precond", [0, 1])
def test_restatement_agrees_with_scipy_cg(family, n, precond):
    a, b = G.system(family, n)
    x0 = 0.1 * G.splitmix64_uniform(n, 5) * np.abs(b).max() / np.abs(a.diagonal()).max()
    for k in (1, 2, 3, 7, 50):
        x = x0.copy()
        st = R.cg(a, b, x, k, precond)
        xs = scipy_cg(a, b, x0, k, precond)
        assert st["iterations"] == k and st["event"] == 0
        assert np.linalg.norm(x - xs) <= 1e-12 * np.linalg.norm(xs), (family, precond, k)


def test_every_matrix_of_the_table_is_bit_symmetric():
    seen = set()
    for c in G.CASES:
        if (c.family, c.n) not in seen:
            seen.add((c.family, c.n))
            a, _ = G.system(c.family, c.n)
            assert G.is_bit_symmetric(a), (c.family, c.n)
            assert np.all(a.diagonal() > 0)
    assert {s for _, s in seen} >= set(G.SIZES) | set(G.LARGE_SIZES)
    for t in G.EVENT_CASES:
        assert G.is_bit_symmetric(G.event_system(t)[0])


@pytest.mark.parametrize("c", G.SMALL_CASES, ids=G.case_id)
def test_d_case_is_small(c):
    """the float64 restatements stay within 1e-10 of the longdouble one on every case (the fixture's own value, measured: 8e-16
    at 200 iterations), the three agree on what they report, and no case meets an event"""
    r = G.case_references(c)
    assert r["d_case"] <= 1e-10, r["d_case"]
    for st in (r["st64"], r["st_chunk"], r["st_ld"]):
        assert st["iterations"] == c.iterations and st["event"] == 0


def test_the_final_residual_is_undetermined_in_the_listed_cases_only():
    """the device's |r| is held to 1e-10 relative except where the float64 references themselves differ from the longdouble |r|
    by more than 1e-11 of it: that set is the list of cg_cases and cannot grow unnoticed"""
    loose = {G.case_id(c) for c in G.SMALL_CASES if G.case_references(c)["res_at_rounding"]}
    assert loose == set(G.RESIDUAL_AT_ROUNDING), loose ^ set(G.RESIDUAL_AT_ROUNDING)
    for c in G.LARGE_CASES:  # a large case has no longdouble run of its own: its family at D_FAMILY_N stands for it
        assert not G.case_references(c._replace(n=G.D_FAMILY_N))["res_at_rounding"]
    for t in G.THRESHOLD_CASES:
        assert not G.threshold_references(t)["res_at_rounding"]


def test_past_end_cases_are_the_rest_of_the_table():
    got = {(c.n, c.iterations) for c in G.CASES + G.PAST_END_CASES if c.n in G.SIZES}
    assert got == {(n, k) for n in G.SIZES for k in G.ITERATIONS}
    for c in G.PAST_END_CASES:
        a, b = G.system(c.family, c.n)
        x = np.zeros(c.n) if G.start_vector(c) is None else G.start_vector(c).copy()
        st = R.cg(a, b, x, c.iterations, c.precond)
        assert st["event"] in (0, 1) and st["iterations"] >= c.n
        ref = np.linalg.solve(a.toarray(), b)
        assert np.linalg.norm(x - ref) <= 1e-10 * np.linalg.norm(ref)


def test_case_table_covers_the_dimensions():
    assert {c.n for c in G.CASES} == set(G.SIZES) | set(G.LARGE_SIZES) | {1008}
    assert {c.iterations for c in G.CASES} == set(G.ITERATIONS)
    for key in ("precond", "x0"):
        assert {getattr(c, key) for c in G.CASES} == {0, 1}
    assert {(c.family, c.precond, c.x0) for c in G.CASES if c.n >= 63} >= {(f, p, x) for f in ("lap1", "lap3") for p in (0, 1) for x in (0, 1)}
    # the large sizes are odd and lie above the clamps of the kernels' grids (cg_cases' docstring)
    assert all(n % 2 == 1 for n in G.LARGE_SIZES) and min(G.LARGE_SIZES) > 2048 * 256 and max(G.LARGE_SIZES) > 2 * 2048 * 256
    for c in G.LARGE_CASES:
        assert G.large_case_d(c) <= 1e-10


@pytest.mark.parametrize("t", G.THRESHOLD_CASES, ids=lambda t: "%s-%s" % (t.family, t.where))
def test_threshold_cases_stop_where_they_say(t):
    thr, k = G.threshold_of(t)
    r = G.threshold_references(t)
    assert {"first": k == 1, "middle": 10 <= k <= 40, "last": k == t.iterations}[t.where], k
    for st in (r["st64"], r["st_chunk"], r["st_ld"]):
        assert st["iterations"] == k and st["event"] == 0
    assert r["d_case"] <= 1e-10


@pytest.mark.parametrize("t", G.EVENT_CASES, ids=lambda t: "%s-n%d" % t)
def test_event_cases(t):
    a, b, x0, precond = G.event_system(t)
    r = G.event_references(t)
    sts = (r["st64"], r["st_chunk"], r["st_ld"])
    assert r["d_case"] <= 1e-10
    if t.name == "indefinite":
        want = 0 if t.n == 2 else 2
        assert t.n <= 1009 or t.n > 2 * 2048 * 256  # the large one grid-strides: late workgroups meet a raised flag
        for st in sts:
            assert (st["iterations"], st["event"]) == (want, 1)
            pq = np.array([float(v) for v in st["pq"]])
            # far from a tie: no association of the sum changes the sign of any p.q
            assert np.all(pq[:-1] > 1.0) and pq[-1] < -1.0
    elif t.name == "zero_rhs":
        for st in sts:
            assert (st["iterations"], st["event"], float(st["beta0"])) == (0, 0, 0.0)
        assert not r["x64"].any()
    else:
        for st in sts:
            assert (st["iterations"], st["event"]) == (G.EVENT_ITERATIONS, 0)
            assert 0 < st["beta0"] <= 1e-12 * np.linalg.norm(b)


def test_restatement_edge_rules():
    a, b = G.system("lap1", 65)
    x = np.full(65, 0.25)
    assert R.cg(a, b, x, 0)["iterations"] == 0 and np.all(x == 0.25)
    bn = b.copy()
    bn[7] = np.nan
    st = R.cg(a, bn, x, 5, 1)
    assert (st["iterations"], st["event"]) == (0, 2) and np.all(x == 0.25)
    st = R.cg(sp.identity(65, format="csr"), b, np.zeros(65), 5)
    assert st["iterations"] == 5 or st["event"] == 1  # converged in one iteration: the rest is p = 0 or rounding noise
    # not symmetric: the recurrence still runs, as on the device
    al, bl = R.left_scaled(*G.system("p", 1008))
    assert not G.is_bit_symmetric(al)
    assert R.cg(al, bl, np.zeros(1008), 7)["iterations"] == 7


def test_pcg_differs_measurably_from_cg_on_the_left_scaled_system():
    a, b = G.system("p", 1008)
    al, bl = R.left_scaled(a, b)
    for k in (3, 7):
        x1, x2 = np.zeros(1008), np.zeros(1008)
        R.cg(a, b, x1, k, 1)
        R.cg(al, bl, x2, k, 0)
        assert G.rel(x2, x1.astype(G.LD)) > 1e-3


def test_cg_abi():
    import orc_amd
    from orc_amd.settings import LinearSolver, NumericalSettings, SolutionMethod
    assert SolutionMethod.CG == 20
    assert C.sizeof(NumericalSettings.default()) == 88
    assert C.sizeof(LinearSolver) == 32
    assert [(f, getattr(LinearSolver, f).offset) for f, _ in LinearSolver._fields_] == [
        ("solver_type", 0), ("preconditioner", 4), ("iterations", 8), ("relative_convergence_threshold", 16), ("relaxation", 24)]
    api = open(os.path.join(ROOT, "orc_amd", "csrc", "api_solver.cpp")).read()  # the C struct itself is pinned where it is compiled
    assert re.search(r"static_assert\(sizeof\(OrcLinearSolver\) == 32", api)
    types = open(os.path.join(ROOT, "include", "orc_types.h")).read()
    assert re.search(r"ORC_SOLVER_CG\s*=\s*20\b", types) and "typedef struct OrcLinearSolver" in types
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orc_amd.h")).read(), flags=re.S)
    lib = orc_amd._lib.lib()
    for name in ("orc_last_cg_stats", "orc_solver_set_pressure_solver", "orc_solver_get_pressure_solver"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    from orc_amd.linear_algebra import last_cg_stats
    its, beta0, res, event = last_cg_stats()
    assert its >= 0 and event in (0, 1, 2)


def test_cg_without_device_is_status_11():
    import orc_amd
    from orc_amd import OrcError
    from orc_amd.linear_algebra import iterative_solve
    from orc_amd.settings import SolutionMethod
    if orc_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(OrcError) as e:
        iterative_solve(sp.identity(4, format="csr"), np.ones(4), np.zeros(4), 5, SolutionMethod.CG, 0.5, 1e-6, 0)
    assert e.value.status == 11
