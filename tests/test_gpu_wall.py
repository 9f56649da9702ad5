"""Wall distance (orc_mesh_wall_distance, orc_amd/csrc/wall_distance.hip) and wall damping of the Smagorinsky length
(orc_solver_set_wall_damping, viscosity.hip) on the device: the search bit for bit against the brute-force restatement of
tests/wall_restatement.py, culled and un-culled, at the edges of a tile, a wave and a block; the cache; the counters of the culled
walk; the damped law against its longdouble restatement; identity with the undamped solver; snapshots, arguments and two ranks.

Bit for bit means equal uint64 views.  The law's bound is the issue's: 16 * 2^-52 relative (tests/test_wall_cpu.py has the count)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import viscosity_restatement as V
import wall_restatement as W
from conftest import ROOT, splitmix64_uniform
from test_gpu_surface import mixed_case
from test_gpu_transient import channel_flow, settings, transient

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = 10
K_BLOCK = 256  # common.hpp kBlock
RHO, MU = 1000.0, 1e-3
ALL_SIX = ["INLET", "OUTLET", "PERIODIC_-Z", "PERIODIC_+Z", "TOP_WALL", "BOTTOM_WALL"]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def tile():
    from orc_amd.mesh import wall_search_stats
    return wall_search_stats()["tile"]


def hex_mesh(nx, ny, nz, walls=ALL_SIX, ordering=None, **kw):
    from orc_amd.mesh import Mesh, hex_channel
    from orc_amd.settings import FaceConditionTypes as T
    a = hex_channel(nx, ny, nz, **kw)
    for name in a["zone_names"][1:]:
        a.set_zone(name, T.Wall if name in walls else T.Symmetry)
    return a, Mesh(a, ordering=ordering)


def check_search(a, m, zones=None):
    """the cached field and both walks of the uncached search against the restatement"""
    want = W.mesh_wall_distance(a, zones)
    for cull in (True, False):
        got = m.debug_wall_distance(zones, cull)
        assert same_bits(got, want), (cull, int(np.count_nonzero(got != want)), len(want))
    assert same_bits(m.wall_distance(zones), want)
    return want


# ------------------------------------------------------------------ 1. the search, bit for bit
@pytest.mark.parametrize("k", ["1", "T-1", "T", "T+1", "2T+1"])
def test_bottom_wall_alone_at_the_tile_edges(gpu, k):
    T = tile()
    n_wall = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[k]
    a, m = hex_mesh(n_wall, 3, 1)
    assert len(W.wall_faces(a, ["BOTTOM_WALL"])) == n_wall
    d = check_search(a, m, ["BOTTOM_WALL"])
    assert same_bits(d, np.asarray(a["cell_centroid"])[:, 1])
    from orc_amd.mesh import wall_search_stats
    st = wall_search_stats()
    assert st["wall_faces"] == n_wall and st["tiles"] == (n_wall + T - 1) // T


@pytest.mark.parametrize("shape", [(5, 4, 3), (32, 16, 12)], ids=lambda s: "%dx%dx%d" % s)
def test_six_walls(gpu, shape):
    a, m = hex_mesh(*shape)
    nx, ny, nz = shape
    assert len(W.wall_faces(a)) == 2 * (nx * ny + ny * nz + nx * nz)
    check_search(a, m)


@pytest.mark.parametrize("polyhedra", [False, True], ids=["mixed", "poly"])
def test_skewed_meshes(gpu, tmp_path, polyhedra):
    a, m = mixed_case(tmp_path, polyhedra)
    d = check_search(a, m)
    assert np.all(np.isfinite(d)) and d.min() > 0
    # not wall-aligned: the plane distance differs from the centroid distance somewhere
    fc, _ = W.wall_table(a)
    cc = np.asarray(a["cell_centroid"])
    nearest = np.sqrt(((cc[:, None, :] - fc[None, :, :]) ** 2).sum(axis=2).min(axis=1))
    assert np.count_nonzero(np.abs(d - nearest) > 1e-3 * nearest) > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, K_BLOCK - 1, K_BLOCK + 1])
def test_partial_last_wave_and_block(gpu, n):
    a, m = hex_mesh(n, 1, 1)
    assert m.n_cells == n
    check_search(a, m)


def test_no_walls_and_an_inlet_mask(gpu):
    a, m = hex_mesh(6, 5, 4)
    assert np.all(np.isposinf(m.wall_distance(zones=[])))
    assert np.all(np.isposinf(m.debug_wall_distance([], cull=False)))
    d = check_search(a, m, ["INLET"])
    assert same_bits(d, np.asarray(a["cell_centroid"])[:, 0])
    assert same_bits(check_search(a, m, [a.get_face_zone("INLET")]), d)
    b, mb = hex_mesh(6, 5, 4, walls=[])  # by type: no zone is a wall
    assert np.all(np.isposinf(mb.wall_distance()))


def test_update_zones_rebuilds_the_cached_field(gpu):
    from orc_amd.mesh import wall_search_stats
    from orc_amd.settings import FaceConditionTypes as T
    a, m = hex_mesh(9, 8, 3, walls=["TOP_WALL", "BOTTOM_WALL"])
    both = m.wall_distance()
    assert same_bits(both, W.mesh_wall_distance(a))
    wall_search_stats(reset=True)
    assert same_bits(m.wall_distance(), both)
    assert wall_search_stats()["waves"] == 0  # the second call is the cache's
    a.set_zone("TOP_WALL", T.Symmetry)
    m.update_zones()
    bottom = m.wall_distance()
    assert wall_search_stats()["waves"] > 0
    assert same_bits(bottom, W.mesh_wall_distance(a, ["BOTTOM_WALL"]))
    assert same_bits(bottom, np.asarray(a["cell_centroid"])[:, 1]) and not same_bits(bottom, both)
    # a change that leaves every wall a wall keeps the field
    wall_search_stats(reset=True)
    a.set_zone("INLET", T.PressureInlet, 0.5)
    m.update_zones()
    assert same_bits(m.wall_distance(), bottom) and wall_search_stats()["waves"] == 0


def test_reordered_mesh_returns_orc_order(gpu):
    from orc_amd.mesh import Mesh, hex_channel, renumber_cells
    a0 = hex_channel(7, 6, 5)
    n = a0.n_cells
    a = renumber_cells(a0, np.argsort(splitmix64_uniform(n, 5), kind="stable").astype(np.int64))
    m = Mesh(a, ordering=1)
    assert not np.array_equal(m.cell_order(), np.arange(n))
    want = W.mesh_wall_distance(a)
    assert same_bits(m.wall_distance(), want)
    assert same_bits(m.debug_wall_distance(None, cull=False), want)
    assert same_bits(Mesh(a).wall_distance(), want)


# ------------------------------------------------------------------ 2. the counters
def test_counters_of_both_walks(gpu):
    from orc_amd.mesh import wall_search_stats
    a, m = hex_mesh(64, 16, 8, walls=["TOP_WALL", "BOTTOM_WALL"])
    T = tile()
    n = m.n_cells
    wall_search_stats(reset=True)
    plain = m.debug_wall_distance(None, cull=False)
    st = wall_search_stats(reset=True)
    assert st["wall_faces"] == 1024 and st["tile"] == T and st["tiles"] == 1024 // T
    assert st["waves"] == (n + 63) // 64 and st["tile_visits"] == st["waves"] * st["tiles"]
    culled = m.debug_wall_distance(None, cull=True)
    sc = wall_search_stats(reset=True)
    print("64x16x8 channel: tile visits per wave %.2f culled, %d un-culled" % (sc["tile_visits"] / sc["waves"], st["tiles"]))
    assert sc["waves"] == st["waves"] and sc["waves"] <= sc["tile_visits"] < st["tile_visits"]
    assert same_bits(culled, plain)
    assert wall_search_stats()["tile_visits"] == 0 and wall_search_stats()["waves"] == 0
    ms = m.bench_wall_distance(cull=True, reps=2)
    assert 0 < ms < 100
    assert wall_search_stats()["waves"] > 0  # the bench's launches are counted too


# ------------------------------------------------------------------ 3. the damping
def smagorinsky(**kw):
    from orc_amd.settings import Viscosity
    return Viscosity.make(V.SMAGORINSKY, V.HARMONIC, cs=0.17, **kw)


def damping(mode, **kw):
    from orc_amd.settings import WallDamping
    return WallDamping.make(mode, **kw)


U_TAU = float(np.sqrt(0.5e-3 * 5.0 / RHO))  # the channel's friction velocity sqrt(h |dp/dx| / rho)
MODES = {"min": dict(mode=W.MIN), "van_driest": dict(mode=W.VAN_DRIEST, u_tau=U_TAU), "van_driest_fast": dict(mode=W.VAN_DRIEST, u_tau=0.05)}


def thin_channel():
    """cells flat enough that kappa d < cs cbrt(V) in the wall-adjacent row: 0.41 * dy / 2 = 1.28e-5 < 0.17 * 1.16e-4"""
    from orc_amd.mesh import Mesh, hex_channel, set_channel_bcs
    a = set_channel_bcs(hex_channel(8, 16, 4))
    return a, Mesh(a)


def run_three(s, fields):
    s.set_fields(*fields)
    st, rep = s.iterate(3, report=True)
    return (s.viscosity(),) + s.diffusion() + s.get_fields() + (rep,)


def state_after(m, fields, configure):
    from orc_amd.solver import Solver
    s = Solver(m, settings(momentum=5), RHO, MU)
    s.set_fields(*fields)
    configure(s)
    return (s.viscosity(),) + s.diffusion() + run_three(s, fields)


def test_off_and_wall_free_meshes_are_the_undamped_solver_bit_for_bit(gpu):
    a, m = thin_channel()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    plain = state_after(m, fields, lambda s: s.set_viscosity(smagorinsky()))

    def none_mode(s):
        s.set_viscosity(smagorinsky())
        s.set_wall_damping(damping(W.NONE))

    def on_then_off(s):
        s.set_wall_damping(damping(W.MIN))
        s.set_viscosity(smagorinsky())
        assert not same_bits(s.viscosity(), plain[0])
        s.set_wall_damping(None)
        assert s.wall_damping()[1] is False

    for configure in (none_mode, on_then_off):
        for k, (x, y) in enumerate(zip(state_after(m, fields, configure), plain)):
            assert same_bits(x, y), (configure.__name__, k)
    # no wall anywhere: d = +inf, both modes give l0
    from orc_amd.settings import FaceConditionTypes as T
    b, mb = thin_channel()
    b.set_zone("TOP_WALL", T.Symmetry)
    b.set_zone("BOTTOM_WALL", T.Symmetry)
    mb.update_zones()
    assert np.all(np.isposinf(mb.wall_distance()))
    free = state_after(mb, fields, lambda s: s.set_viscosity(smagorinsky()))
    assert np.all(np.isfinite(free[0])) and free[0].max() > MU
    for name in ("min", "van_driest"):
        def damped(s):
            s.set_viscosity(smagorinsky())
            s.set_wall_damping(damping(**MODES[name]))
            assert s.wall_damping()[1] is True
        for k, (x, y) in enumerate(zip(state_after(mb, fields, damped), free)):
            assert same_bits(x, y), (name, k)


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("mesh_name", ["channel_flow", "poly", "thin"])
def test_damped_law_at_the_devices_own_strain_rate_and_distance(gpu, tmp_path, mesh_name, name):
    from orc_amd.solver import Solver
    a, m = {"channel_flow": channel_flow, "poly": lambda: mixed_case(tmp_path, True), "thin": thin_channel}[mesh_name]()
    vol = np.asarray(a["cell_volume"])
    s = Solver(m, settings(momentum=5), RHO, MU)
    s.set_fields(*H.rough_fields(np.asarray(a["cell_centroid"])))
    s.set_viscosity(smagorinsky())
    plain, g0 = s.evaluate_viscosity()
    p = MODES[name]
    s.set_wall_damping(damping(**p))
    mu, g = s.evaluate_viscosity()
    d = m.wall_distance()
    assert same_bits(g, g0) and same_bits(d, W.mesh_wall_distance(a)) and np.all(np.isfinite(d))
    assert same_bits(s.viscosity(), mu)  # the set call evaluated the same law on the same fields
    kw = {k: v for k, v in p.items() if k != "mode"}
    want = W.damped_law(p["mode"], g, vol, d, RHO, MU, dtype=np.longdouble, **kw)
    err = np.abs(mu.astype(np.longdouble) - want) / want
    print("%s %s: worst error %.2f x 2^-52, damped in %d of %d cells" % (mesh_name, name, float(err.max()) / W.EPS,
                                                                      np.count_nonzero(mu < plain), len(mu)))
    assert float(err.max()) <= 16 * W.EPS, (mesh_name, name, float(err.max()) / W.EPS)
    assert np.all(mu <= plain)
    if p["mode"] == W.VAN_DRIEST or mesh_name != "poly":  # MIN damps only where kappa d < cs cbrt(V): flat cells at a wall
        assert np.count_nonzero(mu < plain) > 0
    if mesh_name == "thin":  # strictly smaller in every cell that owns a wall face
        c0 = np.asarray(a["face_c0"])[W.wall_faces(a)]
        assert len(np.unique(c0)) == 2 * 8 * 4 and np.all(g[c0] > 0)
        assert np.all(mu[c0] < plain[c0])
    # the setting survives the arm going off and on
    s.set_viscosity(None)
    assert s.wall_damping()[1] is True
    s.set_viscosity(smagorinsky())
    assert same_bits(s.viscosity(), mu)


@pytest.mark.parametrize("name", ["min", "van_driest"])
def test_damped_runs_are_finite_repeatable_and_survive_snapshots(gpu, name):
    from orc_amd.solver import Solver
    a, m = thin_channel()
    fields = H.rough_fields(np.asarray(a["cell_centroid"]))
    runs = []
    for _ in range(2):
        s = Solver(m, settings(momentum=5), RHO, MU)
        s.set_fields(*fields)
        s.set_viscosity(smagorinsky(relaxation=0.5))
        s.set_wall_damping(damping(**MODES[name]))
        s.snapshot()
        st, rep = s.iterate(3, report=True)
        steady = s.get_fields() + (s.viscosity(),)
        s.restore()
        st, rep2 = s.iterate(3, report=True)
        for x, y in zip(steady + (rep,), s.get_fields() + (s.viscosity(), rep2)):
            assert same_bits(x, y)
        s.set_transient(transient(1e-3, 1, 2))
        adv = s.advance(2, report=True)
        out = steady + s.get_fields() + (s.viscosity(), rep, adv)
        assert all(np.all(np.isfinite(x)) for x in out)
        runs.append(out)
    for x, y in zip(*runs):
        assert same_bits(x, y)
    assert runs[0][4].max() > MU  # the law is live


# ------------------------------------------------------------------ 4. arguments
def test_bad_damping_is_refused_with_status_10_and_changes_nothing(gpu):
    from orc_amd.solver import Solver
    a, m = thin_channel()
    s = Solver(m, settings(momentum=5), RHO, MU)
    s.set_fields(*H.rough_fields(np.asarray(a["cell_centroid"])))
    s.set_viscosity(smagorinsky())
    s.set_wall_damping(damping(W.MIN, kappa=0.3))
    before = (s.viscosity(),) + s.diffusion()
    nan, inf = float("nan"), float("inf")
    bad = [damping(3), damping(-1), damping(W.MIN, reserved0=1), damping(W.MIN, kappa=0.0), damping(W.MIN, kappa=-0.41),
           damping(W.VAN_DRIEST), damping(W.VAN_DRIEST, u_tau=-1.0), damping(W.VAN_DRIEST, u_tau=0.05, a_plus=0.0),
           damping(W.VAN_DRIEST, u_tau=0.05, a_plus=-26.0)]
    for mode in (W.NONE, W.MIN, W.VAN_DRIEST):
        for field in ("kappa", "a_plus", "u_tau"):
            for x in (nan, inf, -inf):
                bad.append(damping(mode, **dict(dict(u_tau=0.05), **{field: x})))
    for w in bad:
        assert s.set_wall_damping(w, raise_on_error=False) == BAD_ARGUMENT, [getattr(w, f) for f, _ in w._fields_]
        assert "wall damping" in gpu._lib.last_error()
    w, on = s.wall_damping()
    assert on and (w.mode, w.kappa) == (W.MIN, 0.3)
    for x, y in zip(before, (s.viscosity(),) + s.diffusion()):
        assert same_bits(x, y)
    # a mode ignores what it does not use
    assert s.set_wall_damping(damping(W.MIN, u_tau=0.0, a_plus=-1.0), raise_on_error=False) == 0
    assert s.set_wall_damping(damping(W.NONE, kappa=-1.0), raise_on_error=False) == 0


# ------------------------------------------------------------------ 5. two ranks
def test_two_ranks_on_one_gpu_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "wall_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert "WALL_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
