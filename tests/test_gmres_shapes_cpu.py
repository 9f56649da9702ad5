"""The conditions tests/test_gpu_gmres_shapes.py relies on, proved from the references of tests/gmres_cases.py alone: every
case is well enough conditioned to test a kernel with (d_case <= 1e-12), the references agree on the step and cycle
counts, no stopping decision sits where rounding could move it, and the lucky-breakdown matrices break down where they
are meant to.  CPU only."""
import numpy as np
import pytest

import gmres_cases as G


def test_case_table_covers_what_it_claims():
    cases = G.CASES
    assert len(cases) == 358 and len(set(cases)) == len(cases)
    small = set(G.SIZES)
    assert {c.n for c in cases if c.family in ("cd1", "cd3")} == small | set(G.LARGE_SIZES)
    for n in G.SIZES:
        assert {5, 33, 64} <= {c.restart for c in cases if c.n == n}
    for n in (129, 1009):
        assert set(G.RESTARTS) <= {c.restart for c in cases if c.n == n}
    lo, mid, hi = G.LARGE_SIZES
    assert 131072 < lo <= 262144 < mid <= 1048576 < hi and all(n % 2 for n in G.LARGE_SIZES)
    for n in G.LARGE_SIZES:
        assert {c.restart for c in cases if c.n == n} == {8, 64}
    for r in {c.restart for c in cases}:
        ks = {c.steps for c in cases if c.restart == r}
        assert {r, r + 1, 2 * r + 3} <= ks and (r < 5 or r - 1 in ks)
    assert 2 * sum(c.precond for c in cases) >= len(cases) - 2 and 2 * sum(c.x0 for c in cases) >= len(cases)
    assert {c.family for c in cases} == {"cd1", "cd3", "u", "p"}


def test_synthetic_matrices_are_what_the_table_says():
    for fam in ("cd1", "cd3"):
        a, _ = G.system(fam, 1009)
        d = a.diagonal()
        off = a - G.sp.diags(d)
        assert abs(a - a.T).max() > 0.1, "non-symmetric"
        assert d.max() - d.min() > 0.01, "a diagonal Jacobi scaling changes"
        dom = d - np.asarray(abs(off).sum(axis=1)).ravel()
        assert dom.min() > 0 and np.median(dom) < 0.2 * np.median(d), "weakly diagonally dominant"


@pytest.mark.parametrize("c", G.SMALL_CASES, ids=G.case_id)
def test_references_agree_among_themselves(c):
    r = G.case_references(c)
    # a condition on the inputs: a case above it is too ill-conditioned to test a kernel with (replace the matrix, not the bound)
    assert r["d_case"] <= 1e-12, r["d_case"]
    counts = (r["st64"]["steps"], r["st64"]["cycles"])
    assert (r["st_chunk"]["steps"], r["st_chunk"]["cycles"]) == counts
    assert (r["st_ld"]["steps"], r["st_ld"]["cycles"]) == counts
    # no step's hn / |column| within a factor 5 of the breakdown rule's 1e-14: a ratio of 5e-14 or more carries a rounding error of
    # a few 1e-16, under one percent of itself, and cannot cross the rule in another association
    for k in ("st_chunk", "st_ld"):
        for cyc in r[k]["ratios"]:
            assert all(q < 2e-15 or q > 5e-14 for q in cyc), (k, cyc)


@pytest.mark.parametrize("t", G.THRESHOLD_CASES, ids=lambda t: "%s-r%d-%s" % (t.family, t.restart, t.where))
def test_threshold_stops_cannot_be_moved_by_rounding(t):
    thr = G.threshold_of(t)
    r = G.threshold_references(t)
    assert r["d_case"] <= 1e-12
    want = ((t.cycle - 1) * t.restart + t.step, t.cycle)
    assert t.step > 1 or t.cycle > 1
    for k in ("st64", "st_chunk", "st_ld"):
        s = r[k]
        assert (s["steps"], s["cycles"]) == want, (k, s["steps"], s["cycles"], want)
        for cyc in s["estimates"]:
            for e in cyc:
                q = float(e / (thr * s["beta0"]))
                assert not (1 - 1e-6 <= q <= 1 + 1e-6), (k, q)
    assert abs(float(r["st_ld"]["estimate"]) - r["st64"]["estimate"]) <= 1e-8 * r["st64"]["estimate"]


@pytest.mark.parametrize("t", G.BREAKDOWN_CASES, ids=lambda t: "n%d-d%d" % t)
def test_breakdown_matrices_break_down_at_step_d(t):
    r = G.breakdown_references(t)
    _, _, exact = G.breakdown_system(t)
    assert (r["st64"]["steps"], r["st64"]["cycles"]) == (t.d, 1)
    for k in ("st_chunk", "st_ld"):
        s = r[k]
        assert (s["steps"], s["cycles"]) == (t.d, 1)
        ratios = s["ratios"][0]
        assert ratios[-1] <= 1e-15, (k, ratios[-1])  # a decade under the rule's 1e-14
        assert all(q >= 1e-10 for q in ratios[:-1]), (k, ratios)
    for k in ("x64", "x_chunk", "x_ld"):
        assert G.rel(r[k], exact) <= 1e-14
