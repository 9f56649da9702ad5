"""The life cycle of the post-processing arms (orc_amd/csrc/deferred.hpp, postproc_state.hpp): the probe history, the group history and
tracer tracking each send a record to pinned host memory behind a step and read it one step later.  Here all three run on one stream,
an arm is set again or switched off while its record is still on its way, and a refused set call has to leave the arm as it was.

Every expected value comes from the public calls themselves at the same state (sample, group_report, advect), so every comparison is bit
for bit: equal uint64 views of the doubles and equal integers."""
import numpy as np
import pytest

from test_gpu_groups import same_bits, same_report
from test_gpu_transient import channel_flow, settings, transient
from test_probes_cpu import seeded_points

pytestmark = pytest.mark.gpu

BICGSTAB = 3
RHO, MU = 1000.0, 1e-3
DT = 1e-3
NAMES = ("u", "v", "w", "p")
N_POINTS = 100  # more than one wave, not a multiple of 64


@pytest.fixture(scope="module")
def flow(gpu):
    """the small channel, its points and its three groups (the middle one empty), built once"""
    a, m = channel_flow()
    x = seeded_points(a, N_POINTS, seed=23)
    y = np.asarray(a["cell_centroid"])[:, 1]
    ids = np.where(y < np.median(y), 0, 2).astype(np.int32)
    ids[::7] = -1  # some cells in no group
    groups = m.cell_groups(ids, 3)
    assert list(groups.count > 0) == [True, False, True]
    return dict(a=a, m=m, x=x, probes=m.locate(x), groups=groups)


def fresh(flow):
    from orc_amd.solver import Solver
    n = flow["m"].n_cells
    s = Solver(flow["m"], settings(solver_type=BICGSTAB, iterations=30), RHO, MU)
    z = np.zeros(n)
    s.set_fields(z, z, z, z)
    s.set_transient(transient(DT, 0, 2))
    return s


def tracking_settings(step=0.0):
    from orc_amd.settings import TracerSettings
    import tracer_restatement as TR
    return TracerSettings.make(step, scheme=TR.RK2, interpolation=TR.LINEAR, step_mode=TR.TIME, direction=1)


def same_set(t1, t2):
    g1, g2 = t1.get(), t2.get()
    return all((same_bits if g1[k].dtype == np.float64 else np.array_equal)(g1[k], g2[k]) for k in g1)


def probe_rows(h, names):
    return np.array([h[k] for k in names])


# ------------------------------------------------------------------ 1. the three deferred copies on one stream
def test_all_three_arms_together_record_what_the_direct_calls_give(flow):
    m, p, groups = flow["m"], flow["probes"], flow["groups"]
    # no arm on, stepped one at a time: the direct sample and report after every step
    plain = fresh(flow)
    reps, samples, reports = [], [], []
    for _ in range(4):
        reps.append(plain.advance(1, report=True)[0])
        samples.append(probe_rows(plain.sample(p, NAMES, "linear"), NAMES))
        reports.append(plain.group_report(groups, NAMES))
    # tracking alone
    alone, t_alone = fresh(flow), m.seed(flow["x"])
    alone.set_tracer_tracking(t_alone, tracking_settings(), substeps=2)
    alone.advance(4)
    # everything on, four steps in one call
    s, t = fresh(flow), m.seed(flow["x"])
    s.set_probe_history(p, NAMES, "linear", interval=2)
    s.set_group_history(groups, NAMES, interval=1)
    s.set_tracer_tracking(t, tracking_settings(), substeps=2)
    reps_s = s.advance(4, report=True)

    assert not same_bits(samples[1], samples[3]) and not same_report(reports[2], reports[3])  # the flow moves: a stale row would show
    times, h = s.probe_history()
    assert s.probe_history_count() == 2 and same_bits(times, reps_s[[1, 3], 9])
    for row, step in enumerate((1, 3)):
        assert same_bits(probe_rows(h, NAMES)[:, row], samples[step]), step
    times, full = s.group_history(full=True)
    assert s.group_history_count() == 4 and same_bits(times, reps_s[:, 9])
    for step in range(4):
        assert same_report(full[step], reports[step]), step
    assert same_set(t, t_alone) and np.any(t.get()["steps"] == 8)
    assert same_bits(reps_s, np.array(reps))
    for g, w in zip(s.get_fields(), plain.get_fields()):
        assert same_bits(g, w)


# ------------------------------------------------------------------ 2. set again while a record is on its way
def test_probe_history_set_again_with_a_record_in_flight(flow):
    p = flow["probes"]
    s = fresh(flow)
    s.set_probe_history(p, NAMES, "linear", interval=1)
    s.advance(1)  # its record is on its way and unread
    s.set_probe_history(p, ("u", "p"), "cell", interval=2)
    assert s.probe_history_count() == 0
    direct, reps = [], []
    for _ in range(4):
        reps.append(s.advance(1, report=True)[0])
        direct.append(probe_rows(s.sample(p, ("u", "p"), "cell"), ("u", "p")))
    times, h = s.probe_history()
    assert s.probe_history_count() == 2 and sorted(h) == ["p", "u"]
    assert same_bits(times, np.array(reps)[[1, 3], 9])
    assert h["u"].shape == (2, N_POINTS)
    for row, step in enumerate((1, 3)):
        assert same_bits(probe_rows(h, ("u", "p"))[:, row], direct[step]), step


def test_group_history_set_again_with_a_record_in_flight(flow):
    groups = flow["groups"]
    s = fresh(flow)
    s.set_group_history(groups, NAMES, interval=1)
    s.advance(1)  # its record is on its way and unread
    s.set_group_history(groups, ("u", "p"), interval=2, weighting="unit")
    assert s.group_history_count() == 0
    direct, reps = [], []
    for _ in range(4):
        reps.append(s.advance(1, report=True)[0])
        direct.append(s.group_report(groups, ("u", "p"), "unit"))
    times, full = s.group_history(full=True)
    assert s.group_history_count() == 2 and len(full) == 2
    assert same_bits(times, np.array(reps)[[1, 3], 9])
    for row, step in enumerate((1, 3)):
        assert full[row].raw.shape == (3, 2, 4) and same_report(full[row], direct[step]), step


# ------------------------------------------------------------------ 3. off while a record is on its way, then on again
def test_histories_off_with_a_record_in_flight_then_on_again(flow):
    p, groups = flow["probes"], flow["groups"]
    s = fresh(flow)
    s.set_probe_history(p, NAMES, "linear")
    s.set_group_history(groups, NAMES)
    s.advance(1)
    s.set_probe_history(None)
    s.set_group_history(None)
    assert s.probe_history_count() == -1 and s.group_history_count() == -1
    s.set_probe_history(p, NAMES, "linear")
    s.set_group_history(groups, NAMES)
    assert s.probe_history_count() == 0 and s.group_history_count() == 0
    s.advance(1)
    _, h = s.probe_history()
    _, full = s.group_history(full=True)
    assert s.probe_history_count() == 1 and s.group_history_count() == 1
    assert same_bits(probe_rows(h, NAMES)[:, 0], probe_rows(s.sample(p, NAMES, "linear"), NAMES))
    assert same_report(full[0], s.group_report(groups, NAMES))


def test_tracking_off_with_a_word_in_flight_then_on_again(flow):
    m = flow["m"]
    s, t = fresh(flow), m.seed(flow["x"])
    s.set_tracer_tracking(t, tracking_settings(), substeps=2)
    s.advance(1)
    assert s.set_tracer_tracking(None) == 0
    s.set_tracer_tracking(t, tracking_settings(), substeps=2)
    s.advance(1)
    by_hand, t2 = fresh(flow), m.seed(flow["x"])
    for _ in range(2):
        by_hand.advance(1)
        by_hand.advect(t2, tracking_settings(DT / 2), 2)
    assert same_set(t, t2) and np.any(t.get()["steps"] == 4)


# ------------------------------------------------------------------ 4. a refused set call changes nothing
def test_a_refused_set_call_leaves_the_history_as_it_was(flow):
    from orc_amd._lib import OrcError
    from orc_amd.mesh import Mesh
    p, groups = flow["probes"], flow["groups"]
    other = Mesh(flow["a"])
    ids = np.zeros(other.n_cells, np.int32)
    s = fresh(flow)
    s.set_probe_history(p, NAMES, "linear")
    s.set_group_history(groups, NAMES)
    s.advance(2)
    pt, ph = s.probe_history()
    gt, gf = s.group_history(full=True)
    assert len(pt) == 2 and len(gt) == 2
    refused = [
        lambda: s.set_probe_history(p, 1 << 6, "cell"),                  # unknown mask bit
        lambda: s.set_probe_history(p, "phi", "cell"),                   # no scalar arm
        lambda: s.set_probe_history(p, "u", "cell", interval=0),
        lambda: s.set_probe_history(other.locate(flow["x"]), "u", "cell"),
        lambda: s.set_group_history(groups, 1 << 6),
        lambda: s.set_group_history(groups, "phi"),
        lambda: s.set_group_history(groups, "u", interval=0),
        lambda: s.set_group_history(other.cell_groups(ids, 1), "u"),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(OrcError):
            call()
        assert s.probe_history_count() == 2 and s.group_history_count() == 2, k
        pt2, ph2 = s.probe_history()
        gt2, gf2 = s.group_history(full=True)
        assert same_bits(pt2, pt) and all(same_bits(ph2[n], ph[n]) for n in NAMES), k
        assert same_bits(gt2, gt) and all(same_report(x, y) for x, y in zip(gf2, gf)), k
