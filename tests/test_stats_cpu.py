"""Running time statistics on the host: the numpy restatement of the recurrence (tests/stats_restatement.py) against its longdouble
form and against the two-pass definitions, the cases that must be exact, and the Python mirror of the ABI.  No GPU.

The bound between the fp64 recurrence and its longdouble form is gamma * 2^-52 * S, S = the sum of the absolute values of the terms
added to that accumulator (kept by the longdouble run).  gamma = the roundings on the path from a sample to the accumulator's new
value, counted from the operator order of DESIGN.md §3 "Time statistics":
    a mean          W' = W + w | r = w / W' | dx = x - m | r * dx | m + (r dx)                                    gamma = 5
    a co-moment     the five above (ey reads m') | ey = x - m' | w * dx | (w dx) * ey | C + ((w dx) ey)              gamma = 9
The count bounds the roundings made in forming and adding ONE term; what a term inherits from the error the means already carry is
(w dm) ey + (w dx) dm', of the size 2^-53 |m| w (|ex| + |dx|).  That is inside the count while the fluctuations are not small against
the mean, which holds for the samples used here — the GPU test's: H.rough_fields times splitmix64 noise in [-1, 1), zero-mean — and not
for a small fluctuation on a large mean: measured with the same seven weights on fields * (1 + a * noise), the largest error of a
co-moment over 2^-52 S is 17 for a = 0.3, 127 for a = 0.05 and 5.9e3 for a = 1e-3 (the means stay below 1.4 throughout).  West's
update shares this with every one-pass variance; DESIGN.md says so."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import stats_restatement as R
from conftest import ROOT, splitmix64_uniform

GAMMA_MEAN, GAMMA_COMOMENT = 5, 9  # roundings per term: the docstring's count
WEIGHTS = (1.0, 0.5, 2.25, 0.125, 3.0, 0.75, 1.5)  # seven samples, unequal weights
GROUPS = R.MEAN | R.STRESS | R.VISCOSITY | R.SCALAR


def cloud(n):
    """cell centroids scattered over the channel's box: what H.rough_fields wants"""
    return np.stack([1e-3 * (1 + splitmix64_uniform(n, 1)), 0.5e-3 * (1 + splitmix64_uniform(n, 2)), 1e-4 * splitmix64_uniform(n, 3)], axis=1)


def noisy_states(n, count=len(WEIGHTS), seed=100):
    """sample k: rough_fields times noise in [-1, 1); mu positive, phi in [-1, 1)"""
    base = H.rough_fields(cloud(n))
    out = []
    for k in range(count):
        s = {name: base[i] * splitmix64_uniform(n, seed + 10 * k + i) for i, name in enumerate("uvwp")}
        s["mu"] = 1e-3 * (1.5 + splitmix64_uniform(n, seed + 10 * k + 5))
        s["phi"] = splitmix64_uniform(n, seed + 10 * k + 6)
        out.append(s)
    return out


@pytest.fixture(scope="module")
def runs():
    n = 1008
    states = noisy_states(n)
    f64, ld = R.Running(GROUPS, n), R.Running(GROUPS, n, np.longdouble, track=True)
    for w, s in zip(WEIGHTS, states):
        f64.sample(w, s)
        ld.sample(w, s)
    return states, f64, ld


def test_fp64_recurrence_against_its_longdouble_form(runs):
    _, f64, ld = runs
    assert f64.names == list(R.NAMES) and float(ld.W) == f64.W == sum(WEIGHTS)
    for k in f64.names:
        gamma = GAMMA_COMOMENT if k in R.PAIRS else GAMMA_MEAN
        err = np.abs(f64.acc[k].astype(np.longdouble) - ld.acc[k])
        bound = gamma * np.longdouble(2.0) ** -52 * ld.abs_terms[k]
        print("%-7s gamma %d: worst error / (2^-52 S) = %.3f" % (k, gamma, float(np.max(err / (bound / gamma)))))
        assert np.all(ld.abs_terms[k] > 0) and np.all(err <= bound), k


def test_longdouble_recurrence_equals_the_two_pass_definitions(runs):
    """West's update is the two-pass definition in exact arithmetic; in longdouble the two differ by its rounding: at most a few
    hundred units of eps_L (seven samples, nine roundings each, against sum w |x| for a mean and sum w |dx dy| for a co-moment)"""
    states, _, ld = runs
    want, W = R.two_pass(GROUPS, WEIGHTS, states)
    eps = np.finfo(np.longdouble).eps
    assert abs(ld.W - W) <= 8 * eps * W
    for k in ld.names:
        if k in R.PAIRS:
            x, y = R.PAIRS[k]
            scale = sum(np.longdouble(w) * np.abs((np.asarray(s[x], dtype=np.longdouble) - want[x]) * (np.asarray(s[y], dtype=np.longdouble) - want[y]))
                        for w, s in zip(WEIGHTS, states))
        else:
            scale = sum(np.longdouble(w) * np.abs(np.asarray(s[k], dtype=np.longdouble)) for w, s in zip(WEIGHTS, states)) / W
        assert np.all(np.abs(ld.acc[k] - want[k]) <= 256 * eps * scale), k


def test_constant_samples_are_exact():
    n = 27
    s = noisy_states(n, 1)[0]
    run = R.Running(GROUPS, n)
    for w in WEIGHTS:
        run.sample(w, s)
        for k in run.names:
            want = np.zeros(n) if k in R.PAIRS else s[k]
            assert np.array_equal(run.acc[k], want), k
    assert run.samples == len(WEIGHTS)


@pytest.mark.parametrize("w", [1.0, 0.3, 1e-9, 7.25e11])
def test_the_first_sample_is_exact_for_any_weight(w):
    n = 8
    s = noisy_states(n, 1, seed=7)[0]
    run = R.Running(GROUPS, n)
    run.sample(w, s)
    assert run.W == w
    for k in run.names:
        assert np.array_equal(run.acc[k], np.zeros(n) if k in R.PAIRS else s[k]), k


def test_doubling_every_weight_changes_no_bit_of_a_mean():
    """r = w / W' is a ratio: powers of two cancel exactly; C doubles exactly, so C / W keeps its bits too"""
    n = 480
    states = noisy_states(n)
    one, two = R.Running(GROUPS, n), R.Running(GROUPS, n)
    for w, s in zip(WEIGHTS, states):
        one.sample(w, s)
        two.sample(2.0 * w, s)
    a, b = one.result(R.NORMALISED), two.result(R.NORMALISED)
    for k in one.names:
        assert np.array_equal(a[k], b[k]), k
        if k in R.PAIRS:
            assert np.array_equal(2.0 * one.acc[k], two.acc[k]), k


def test_python_mirror_and_header_agree():
    from orc_amd import solver as S
    from orc_amd.settings import StatForm, StatGroup, TimeStatistics
    assert C.sizeof(TimeStatistics) == 24
    assert [(f, TimeStatistics.__dict__[f].offset) for f, _ in TimeStatistics._fields_] == [("groups", 0), ("reserved0", 4), ("start_step", 8), ("interval", 16)]
    txt = open(os.path.join(ROOT, "include", "orc_types.h")).read()
    for name, value in (("MEAN", StatGroup.MEAN), ("STRESS", StatGroup.STRESS), ("VISCOSITY", StatGroup.VISCOSITY), ("SCALAR", StatGroup.SCALAR),
                        ("BOUNDARY", StatGroup.BOUNDARY)):
        assert "ORC_STAT_GROUP_%s = %d" % (name, value) in txt, name
    assert (R.MEAN, R.STRESS, R.VISCOSITY, R.SCALAR, R.BOUNDARY) == (1, 2, 4, 8, 16) and StatGroup.ALL == R.ALL
    assert "ORC_STAT_RAW = %d" % StatForm.RAW in txt and "ORC_STAT_NORMALISED = %d" % StatForm.NORMALISED in txt
    # the field enum is written as a plain list from ORC_STAT_U = 0: its order is the names' order
    body = txt[txt.index("enum OrcStatField {"):txt.index("ORC_STAT_N /* 17 */")]
    listed = [t.strip().split(" ")[0] for t in body[body.index("{") + 1:].split(",") if t.strip()]
    assert listed == ["ORC_STAT_" + n.upper() for n in S.STATISTIC_NAMES] and "ORC_STAT_U = 0" in body
    assert S.STATISTIC_NAMES == R.NAMES and len(S.STATISTIC_NAMES) == 17
    assert S.STAT_BOUNDARY_NAMES == R.BOUNDARY_NAMES == S.BOUNDARY_NAMES[:5] and "#define ORC_STAT_BOUNDARY_N 5" in txt
    for k, (x, y) in R.PAIRS.items():
        assert k == x + y


def test_library_exports_the_statistics_entries():
    """fails on a library built before the statistics existed"""
    import orc_amd
    from orc_amd._lib import lib
    from orc_amd.settings import TimeStatistics
    L = lib()
    for name in ("orc_time_statistics_default", "orc_solver_set_time_statistics", "orc_solver_sample_statistics", "orc_solver_reset_statistics",
                 "orc_solver_statistics_info", "orc_solver_get_statistics", "orc_solver_set_statistics_state", "orc_solver_get_boundary_statistics",
                 "orc_bench_time_statistics"):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    c = TimeStatistics.make()
    assert (c.groups, c.reserved0, c.start_step, c.interval) == (3, 0, 1, 1)
    c = TimeStatistics.make(groups=R.ALL, start_step=5, interval=3)
    assert (c.groups, c.start_step, c.interval) == (31, 5, 3)
    # without a device every compute entry says so; with one a null solver is a bad argument
    want = 11 if orc_amd.device_count() < 1 else 10
    assert L.orc_solver_set_time_statistics(None, None) == want
    assert L.orc_solver_sample_statistics(None, 1.0) == want
    assert L.orc_solver_get_statistics(None, 1, 0, None) == want
