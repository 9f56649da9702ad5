"""Running time statistics (orc_solver_set_time_statistics, orc_amd/csrc/time_stats.hip) on the device: every enabled field bit for
bit against the numpy restatement (tests/stats_restatement.py) for every legal set of groups, the cases that must be exact, sampling
inside advance() against a twin solver without the arm, the boundary means and the friction velocity, the restart path, reset / off /
refusals, and two ranks on one GPU.

Bit for bit means equal uint64 views.  The meshes are the smallest on which the pass can go wrong: 3x3_cube (27 cells: odd, less than
one wave), 2D_2x4 (8 cells), channel_flow (1008 cells: four workgroups) in file and RCM order (internal order differs from ORC order)
and the 24 x 5 x 4 polyhedral channel.  The bound of the alternating state is the CPU test's (tests/test_stats_cpu.py): gamma * 2^-52
* S with gamma = 5 for a mean and 9 for a co-moment, S the longdouble run's sum of absolute terms."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import stats_restatement as R
from conftest import GOLDEN, ROOT, splitmix64_uniform
from test_gpu_transient import _ZoneAdapter, channel_flow, poly_channel, settings, transient
from test_stats_cpu import GAMMA_COMOMENT, GAMMA_MEAN, WEIGHTS

pytestmark = pytest.mark.gpu

BICGSTAB = 3
BAD_ARGUMENT = 10
RHO, MU = 1000.0, 1e-3
MESHES = ["3x3_cube", "2D_2x4", "channel_flow", "channel_flow_rcm", "poly"]
# every legal set of groups: MEAN with any of the other four
SUBSETS = [R.MEAN | sum(c) for k in range(5) for c in itertools.combinations((R.STRESS, R.VISCOSITY, R.SCALAR, R.BOUNDARY), k)]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def small_mesh(stem, bcs=None):
    from orc_amd import io as orc_io
    from orc_amd.mesh import Mesh, MeshArrays
    d = orc_io.read_mesh(os.path.join(GOLDEN, "meshes", stem + ".msh"))
    if bcs is not None:
        bcs(_ZoneAdapter(d))
    a = MeshArrays(d.arrays())
    return a, Mesh(a)


def mesh_of(name, tmp_path):
    if name == "3x3_cube":
        return small_mesh(name, H.cube_bcs_mixed)
    if name == "2D_2x4":
        return small_mesh(name)  # the file's own zone types: pressure inlet and outlet, two walls
    if name == "poly":
        return poly_channel(tmp_path)
    return channel_flow(ordering=1 if name.endswith("rcm") else None)


def stat_settings(groups, start_step=1, interval=1):
    from orc_amd.settings import TimeStatistics
    return TimeStatistics.make(groups=groups, start_step=start_step, interval=interval)


def sample_states(a, count=len(WEIGHTS), seed=100):
    """sample k: H.rough_fields times splitmix64 noise; a positive viscosity field; phi in [-1, 1)"""
    n = a.n_cells
    base = H.rough_fields(np.asarray(a["cell_centroid"]))
    out = []
    for k in range(count):
        s = {name: base[i] * splitmix64_uniform(n, seed + 10 * k + i) for i, name in enumerate("uvwp")}
        s["mu"] = MU * (1.5 + splitmix64_uniform(n, seed + 10 * k + 5))
        s["phi"] = splitmix64_uniform(n, seed + 10 * k + 6)
        out.append(s)
    return out


def full_solver(m, first):
    """a solver with the viscosity arm (FIELD) and the scalar arm on, so that every group is legal"""
    from orc_amd.settings import ScalarSettings, Viscosity, ViscosityModel
    from orc_amd.solver import Solver
    s = Solver(m, settings(momentum=5, solver_type=BICGSTAB), RHO, MU)
    s.set_viscosity_field(first["mu"])
    s.set_viscosity(Viscosity.make(ViscosityModel.FIELD))
    s.set_scalar(ScalarSettings.default())
    return s


def push(s, state):
    s.set_fields(state["u"], state["v"], state["w"], state["p"])
    s.set_viscosity_field(state["mu"])
    s.set_scalar_field(state["phi"])


def boundary_now(s):
    b = s.boundary_fields(list(R.BOUNDARY_NAMES))
    return np.stack([b[k] for k in R.BOUNDARY_NAMES])


def check_against(s, run, bnd=None):
    names = run.names
    for form, normalised in ((R.RAW, False), (R.NORMALISED, True)):
        got, want = s.statistics(normalised=normalised), run.result(form)
        assert list(got) == names
        for k in names:
            assert same_bits(got[k], want[k]), (k, form)
    one = s.statistics(names[-1], normalised=False)  # a selection: the last row of the buffer alone
    assert list(one) == [names[-1]] and same_bits(one[names[-1]], run.acc[names[-1]])
    if bnd is not None:
        b = s.boundary_statistics()
        for i, k in enumerate(R.BOUNDARY_NAMES):
            assert same_bits(b[k], bnd.m[i]), k


# ------------------------------------------------------------------ 1. bit for bit against the restatement
@pytest.mark.parametrize("mesh_name", MESHES)
def test_seven_unequal_samples_equal_the_restatement_for_every_set_of_groups(gpu, tmp_path, mesh_name):
    a, m = mesh_of(mesh_name, tmp_path)
    n = a.n_cells
    assert (n % 2 == 1) == (mesh_name == "3x3_cube")  # an odd and several even cell counts
    states = sample_states(a)
    s = full_solver(m, states[0])
    nb = int(m.boundary_index()[0][-1])
    assert len(SUBSETS) == 16
    for groups in SUBSETS:
        s.set_time_statistics(stat_settings(groups))
        run = R.Running(groups, n)
        bnd = R.BoundaryMean(nb) if groups & R.BOUNDARY else None
        for w, state in zip(WEIGHTS, states):
            push(s, state)
            s.sample_statistics(w)
            run.sample(w, state)
            if bnd is not None:
                bnd.sample(w, boundary_now(s))
        info = s.statistics_info()
        assert info == dict(samples=7, weight_sum=run.W, n_fields=len(run.names), n_boundary_faces=nb if bnd is not None else 0), groups
        check_against(s, run, bnd)
        if bnd is not None:
            assert np.any(bnd.m[4] != 0.0)  # there is a wall shear to average


# ------------------------------------------------------------------ 2. exactness on the device
@pytest.mark.parametrize("mesh_name", ["3x3_cube", "channel_flow_rcm"])
def test_a_constant_state_is_its_own_mean_with_zero_co_moments(gpu, tmp_path, mesh_name):
    a, m = mesh_of(mesh_name, tmp_path)
    state = sample_states(a, 1)[0]
    s = full_solver(m, state)
    groups = R.ALL
    s.set_time_statistics(stat_settings(groups))
    push(s, state)
    now = boundary_now(s)
    for w in WEIGHTS[:5]:
        s.sample_statistics(w)
    got = s.statistics(normalised=False)
    for k in R.enabled(groups):
        assert same_bits(got[k], np.zeros(a.n_cells) if k in R.PAIRS else state[k]), k
    b = s.boundary_statistics()
    for i, k in enumerate(R.BOUNDARY_NAMES):
        assert same_bits(b[k], now[i]), k


def test_an_alternating_state_gives_its_mean_and_variance_within_the_bound(gpu):
    """x + a, x - a, ... six times with equal weights: the mean is x and C = W a^2 in exact arithmetic; a is a good fraction of |x|
    (0.25 .. 0.75), the regime the bound is stated for (tests/test_stats_cpu.py)"""
    a_, m = channel_flow()
    n = a_.n_cells
    x = sample_states(a_, 1)[0]
    amp = {k: np.abs(x[k]) * (0.5 + 0.25 * splitmix64_uniform(n, 900 + i)) for i, k in enumerate(R.MEANS)}
    s = full_solver(m, x)
    groups = R.MEAN | R.STRESS | R.VISCOSITY | R.SCALAR
    s.set_time_statistics(stat_settings(groups))
    ld = R.Running(groups, n, np.longdouble, track=True)
    w, count = 0.75, 6
    for j in range(count):
        state = {k: x[k] + amp[k] if j % 2 == 0 else x[k] - amp[k] for k in R.MEANS}
        push(s, state)
        s.sample_statistics(w)
        ld.sample(w, state)
    got = s.statistics(normalised=False)
    L = np.longdouble
    unit = L(2.0) ** -52
    for k in R.enabled(groups):
        if k in R.PAIRS:
            p, q = R.PAIRS[k]
            # the state as fed: the rounded sums x + a, x - a around their own midpoint
            hi = {z: (x[z] + amp[z]).astype(L) for z in (p, q)}
            lo = {z: (x[z] - amp[z]).astype(L) for z in (p, q)}
            want = L(w) * count * ((hi[p] - lo[p]) / 2) * ((hi[q] - lo[q]) / 2)
            gamma = GAMMA_COMOMENT
        else:
            want = ((x[k] + amp[k]).astype(L) + (x[k] - amp[k]).astype(L)) / 2
            gamma = GAMMA_MEAN
        err = np.abs(got[k].astype(L) - want)
        print("%-7s worst error / (2^-52 S) = %.3f" % (k, float(np.max(err / (unit * ld.abs_terms[k])))))
        assert np.all(err <= gamma * unit * ld.abs_terms[k]), k
    assert same_bits(s.statistics("uu")["uu"], got["uu"] / s.statistics_info()["weight_sum"])  # NORMALISED: one division by W


# ------------------------------------------------------------------ 3. inside advance
def test_advance_samples_the_due_steps_and_leaves_the_flow_alone(gpu):
    from orc_amd.settings import ScalarBc, ScalarSettings
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = a.n_cells
    start = H.rough_fields(np.asarray(a["cell_centroid"]))
    dt = 1e-3
    groups = R.MEAN | R.STRESS | R.SCALAR | R.BOUNDARY
    pair = []
    for on in (True, False):
        s = Solver(m, settings(momentum=5, solver_type=BICGSTAB), RHO, MU)
        s.set_fields(*start)
        s.set_scalar(ScalarSettings.default())
        s.set_scalar_bc("INLET", ScalarBc.VALUE, 1.0)
        s.set_scalar_field(0.5 + 0.3 * splitmix64_uniform(n, 77))
        s.set_transient(transient(dt, 1, 3))  # BDF2, three inner iterations
        if on:
            s.set_time_statistics(stat_settings(groups, start_step=2, interval=2))
        pair.append(s)
    s, twin = pair
    run, bnd = R.Running(groups, n), R.BoundaryMean(int(m.boundary_index()[0][-1]))
    for step in range(1, 7):
        s.advance(1)
        twin.advance(1)
        if step in (2, 4, 6):
            u, v, w, p = twin.get_fields()
            run.sample(dt, dict(u=u, v=v, w=w, p=p, phi=twin.get_scalar_field()))
            bnd.sample(dt, boundary_now(twin))
        assert s.statistics_info()["samples"] == step // 2
    info = s.statistics_info()
    assert info["samples"] == 3 and info["weight_sum"] == (0.0 + dt) + dt + dt
    check_against(s, run, bnd)
    for x, y in zip(s.get_fields() + (s.get_scalar_field(),), twin.get_fields() + (twin.get_scalar_field(),)):
        assert same_bits(x, y)  # the arm reads only
    assert len(np.unique(run.acc["uu"])) > n // 2 and np.all(run.acc["uu"] >= 0.0)  # the flow moved between the samples


# ------------------------------------------------------------------ 4. the boundary group
def test_boundary_means_and_the_mean_friction_velocity(gpu):
    a, m = channel_flow()
    states = sample_states(a)
    s = full_solver(m, states[0])
    s.set_time_statistics(stat_settings(R.MEAN | R.BOUNDARY))
    zp, faces, _, _ = m.boundary_index()
    bnd = R.BoundaryMean(int(zp[-1]))
    for w, state in zip(WEIGHTS, states):
        push(s, state)
        s.sample_statistics(w)
        bnd.sample(w, boundary_now(s))
    b = s.boundary_statistics()
    assert np.array_equal(b.zone_ptr, zp) and np.array_equal(b.faces, faces) and list(b.arrays) == list(R.BOUNDARY_NAMES)
    for i, k in enumerate(R.BOUNDARY_NAMES):
        assert same_bits(b[k], bnd.m[i]), k
    z = list(a["zone_names"]).index("WALL")
    lo, hi = int(zp[z]), int(zp[z + 1])
    area = np.asarray(a["face_area"])[faces[lo:hi]]
    want = np.sqrt((np.sum(area * bnd.m[4][lo:hi]) / np.sum(area)) / RHO)
    assert hi - lo > 0 and want > 0.0
    assert s.mean_friction_velocity("WALL") == want == s.mean_friction_velocity(z)
    assert same_bits(b.zone("WALL")["shear_mag"], bnd.m[4][lo:hi])


# ------------------------------------------------------------------ 5. restart
@pytest.mark.parametrize("mesh_name", ["3x3_cube", "channel_flow_rcm"])
def test_a_restored_state_continues_bit_for_bit(gpu, tmp_path, mesh_name):
    a, m = mesh_of(mesh_name, tmp_path)
    states = sample_states(a, 6)
    weights = WEIGHTS[:6]
    groups = R.ALL
    whole = full_solver(m, states[0])
    whole.set_time_statistics(stat_settings(groups))
    for w, state in zip(weights, states):
        push(whole, state)
        whole.sample_statistics(w)
    first = full_solver(m, states[0])
    first.set_time_statistics(stat_settings(groups))
    for w, state in zip(weights[:3], states[:3]):
        push(first, state)
        first.sample_statistics(w)
    saved = first.statistics_state()
    assert saved["samples"] == 3 and saved["raw"].shape == (17, a.n_cells) and saved["boundary"].shape[0] == 5
    del first
    second = full_solver(m, states[0])
    second.set_time_statistics(stat_settings(groups))
    second.set_statistics_state(saved)
    assert second.statistics_info() == dict(whole.statistics_info(), samples=3, weight_sum=saved["weight_sum"])
    for w, state in zip(weights[3:], states[3:]):
        push(second, state)
        second.sample_statistics(w)
    assert second.statistics_info() == whole.statistics_info()
    x, y = second.statistics_state(), whole.statistics_state()
    assert same_bits(x["raw"], y["raw"]) and same_bits(x["boundary"], y["boundary"]) and x["names"] == y["names"] == list(R.NAMES)


# ------------------------------------------------------------------ 6. reset, off, refusals
def test_reset_keeps_the_settings_and_off_frees_the_arm(gpu):
    from orc_amd import OrcError
    a, m = channel_flow()
    states = sample_states(a, 3)
    s = full_solver(m, states[0])
    s.set_time_statistics(stat_settings(R.ALL, start_step=3, interval=2))
    for w, state in zip(WEIGHTS, states):
        push(s, state)
        s.sample_statistics(w)
    before = s.statistics_info()
    assert before["samples"] == 3 and before["n_fields"] == 17 and before["n_boundary_faces"] > 0
    s.reset_statistics()
    assert s.statistics_info() == dict(before, samples=0, weight_sum=0.0)
    raw = s.statistics(normalised=False)
    assert list(raw) == list(R.NAMES) and all(same_bits(v, np.zeros(a.n_cells)) for v in raw.values())  # RAW with 0 samples: zeros
    assert not np.any(s.boundary_statistics()["shear_mag"])
    assert s.statistics(raise_on_error=False)[0] == BAD_ARGUMENT  # NORMALISED with 0 samples
    push(s, states[1])
    s.sample_statistics(2.0)  # the first sample after a reset is exact again
    assert same_bits(s.statistics("u")["u"], states[1]["u"]) and not np.any(s.statistics("uv")["uv"])
    s.set_time_statistics(None)
    with pytest.raises(OrcError) as e:
        s.statistics()
    assert e.value.status == BAD_ARGUMENT
    assert s.sample_statistics(1.0, raise_on_error=False) == BAD_ARGUMENT and s.reset_statistics(raise_on_error=False) == BAD_ARGUMENT
    assert s.statistics_info(raise_on_error=False)[0] == BAD_ARGUMENT and s.boundary_statistics(raise_on_error=False)[0] == BAD_ARGUMENT
    s.set_scalar(None)  # with the arm off nothing holds the scalar or the viscosity arm
    s.set_viscosity(None)


def test_refusals_change_nothing(gpu):
    from orc_amd.settings import TimeStatistics
    from orc_amd.solver import Solver
    a, m = channel_flow()
    n = a.n_cells
    states = sample_states(a, 2)
    nan, inf = float("nan"), float("inf")

    def snapshot_of(s):
        return s.statistics_info(), s.statistics(normalised=False)

    def unchanged(s, before):
        info, raw = snapshot_of(s)
        return info == before[0] and all(same_bits(raw[k], before[1][k]) for k in raw)

    # a plain solver: neither the viscosity nor the scalar arm
    s = Solver(m, settings(momentum=5, solver_type=BICGSTAB), RHO, MU)
    s.set_time_statistics(stat_settings(R.MEAN | R.STRESS))
    for w, state in zip(WEIGHTS, states):
        s.set_fields(state["u"], state["v"], state["w"], state["p"])
        s.sample_statistics(w)
    before = snapshot_of(s)
    bad = [stat_settings(R.STRESS), stat_settings(0), stat_settings(R.MEAN | 32), stat_settings(R.MEAN | (1 << 31)),
           TimeStatistics(groups=3, reserved0=1, start_step=1, interval=1), stat_settings(3, interval=0),
           stat_settings(R.MEAN | R.VISCOSITY), stat_settings(R.MEAN | R.SCALAR), stat_settings(R.ALL)]
    for c in bad:
        assert s.set_time_statistics(c, raise_on_error=False) == BAD_ARGUMENT, (c.groups, c.reserved0, c.interval)
        assert unchanged(s, before)
    for w in (0.0, -1.0, nan, inf, -inf):
        assert s.sample_statistics(w, raise_on_error=False) == BAD_ARGUMENT
    for mask in (0, 1 << R.NAMES.index("mu"), 1 << R.NAMES.index("phi"), 1 | 1 << R.NAMES.index("wphi"), 1 << 17, 1 << 31):
        assert s.statistics(mask, raise_on_error=False)[0] == BAD_ARGUMENT, mask
    from orc_amd._lib import lib
    import ctypes as C
    out = np.zeros(n)
    for form in (2, -1):
        assert lib().orc_solver_get_statistics(s.ptr, 1, form, out.ctypes.data_as(C.POINTER(C.c_double))) == BAD_ARGUMENT
    assert s.boundary_statistics(raise_on_error=False)[0] == BAD_ARGUMENT  # the BOUNDARY group is off
    state = s.statistics_state()
    assert s.set_statistics_state(dict(state, names=state["names"][:4], raw=state["raw"][:4]), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_statistics_state(dict(state, boundary=np.zeros((5, 4))), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_statistics_state(dict(state, weight_sum=-1.0), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_statistics_state(dict(state, weight_sum=nan), raise_on_error=False) == BAD_ARGUMENT
    assert s.set_statistics_state(dict(state, samples=0), raise_on_error=False) == BAD_ARGUMENT
    assert unchanged(s, before)
    # the arms a group reads cannot be switched off under it
    s = full_solver(m, states[0])
    s.set_time_statistics(stat_settings(R.MEAN | R.VISCOSITY | R.SCALAR))
    push(s, states[0])
    s.sample_statistics(1.0)
    before = snapshot_of(s)
    assert s.set_scalar(None, raise_on_error=False) == BAD_ARGUMENT
    assert s.set_viscosity(None, raise_on_error=False) == BAD_ARGUMENT
    assert same_bits(s.get_scalar_field(), states[0]["phi"]) and same_bits(s.viscosity(), states[0]["mu"])
    push(s, states[1])
    s.sample_statistics(1.0)  # both arms are still there to be read
    assert not unchanged(s, before) and s.statistics_info()["samples"] == 2


# ------------------------------------------------------------------ 7. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "stats_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "STATS_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
