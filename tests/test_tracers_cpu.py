"""Tracer particles without a device: the settings' layout and the enums against the header, the exported symbols, the entries without a
device, and the numpy restatement (tests/tracer_restatement.py) against itself on the hex, mixed and polyhedral channels — the conditions
that keep the device comparison of tests/test_gpu_tracers.py from being empty, and the invariance under a split of the substeps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tracer_restatement as TR
from conftest import ROOT, splitmix64_uniform
from test_probes_cpu import bounding_box

NO_DEVICE = 11
U0 = 0.05
N_SEEDS = 300
SUBSTEPS = {"hex": 14, "mixed": 32, "poly": 32}
MIN_CHANGES = {"hex": 4, "mixed": 8, "poly": 8}
SYMBOLS = ["orc_tracer_settings_default", "orc_tracers_create", "orc_tracers_destroy", "orc_tracers_count", "orc_tracers_get",
           "orc_solver_advect_tracers", "orc_solver_sample_tracers", "orc_solver_set_tracer_tracking", "orc_write_vtu_lines", "orc_bench_tracers"]


# ------------------------------------------------------------------ 1. layout and symbols
def test_settings_layout_and_enums_match_the_header(tmp_path):
    from orc_amd import settings as S
    names = ["ORC_TRACER_ACTIVE", "ORC_TRACER_LEFT", "ORC_TRACER_WALK_LIMIT", "ORC_TRACER_STAGNANT", "ORC_TRACER_EULER", "ORC_TRACER_RK2",
             "ORC_TRACER_STEP_TIME", "ORC_TRACER_STEP_LENGTH", "sizeof(OrcTracerSettings)", "offsetof(OrcTracerSettings, direction)",
             "offsetof(OrcTracerSettings, step)", "offsetof(OrcTracerSettings, min_speed)"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "orc_types.h"\nint main(){' + "".join('printf("%%d ", (int)%s);' % n for n in names)
           + "return 0;}")
    exe = str(tmp_path / "enums")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    T, K, M, X = S.TracerStatus, S.TracerScheme, S.TracerStepMode, S.TracerSettings
    assert got == [T.ACTIVE, T.LEFT, T.WALK_LIMIT, T.STAGNANT, K.EULER, K.RK2, M.TIME, M.LENGTH, C.sizeof(X), X.direction.offset, X.step.offset,
                   X.min_speed.offset]
    assert got == [0, 1, 2, 3, 0, 1, 0, 1, 32, 12, 16, 24]
    assert (TR.ACTIVE, TR.LEFT, TR.WALK_LIMIT, TR.STAGNANT, TR.EULER, TR.RK2, TR.TIME, TR.LENGTH, TR.CELL, TR.LINEAR) == (0, 1, 2, 3, 0, 1, 0, 1, 0, 1)
    c = X.make(2.5e-5)  # host only: no device needed
    assert (c.scheme, c.interpolation, c.step_mode, c.direction, c.step, c.min_speed) == (K.RK2, S.ProbeInterpolation.LINEAR, M.LENGTH, 1, 2.5e-5, 0.0)
    assert X.make().step == 0.0 and X.make(1.0, direction=-1, scheme=K.EULER).direction == -1
    with pytest.raises(AttributeError):
        X.make(1.0, nonsense=1)


def test_every_new_symbol_is_exported():
    from orc_amd._lib import lib
    L = lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_compute_entries_return_no_device_without_a_device():
    import orc_amd
    from orc_amd._lib import lib
    if orc_amd.device_count() > 0:
        pytest.skip("a device is present")
    L = lib()
    st = C.c_int(0)
    xyz = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert L.orc_tracers_create(None, 1, xyz, C.byref(st)) is None and st.value == NO_DEVICE
    assert L.orc_tracers_get(None, None, None, None, None, None, None) == NO_DEVICE
    assert L.orc_solver_advect_tracers(None, None, None, 1, 0, None, None) == NO_DEVICE
    assert L.orc_solver_sample_tracers(None, None, 1, 0, None) == NO_DEVICE
    assert L.orc_solver_set_tracer_tracking(None, None, None, 1) == NO_DEVICE
    ms = C.c_double(0.0)
    assert L.orc_bench_tracers(None, None, None, 1, 1, C.byref(ms)) == NO_DEVICE
    assert L.orc_tracers_count(None) == 0
    L.orc_tracers_destroy(None)


# ------------------------------------------------------------------ 2. the restatement against itself
def host_mesh(name, tmp_path):
    """hex = hex_channel(12, 8, 6); mixed and poly: the meshes of tests/test_probes_cpu.py::host_mesh"""
    from orc_amd.mesh import hex_channel
    from test_probes_cpu import host_mesh as probe_mesh
    return hex_channel(12, 8, 6) if name == "hex" else probe_mesh(name, tmp_path)


def tracer_fields(a):
    """u = U0 (1 + 0.5 sin 2 pi xi_y + 0.1 r_1), v = U0 (0.3 cos 2 pi xi_x + 0.1 r_2), w = U0 (0.2 sin 2 pi xi_x + 0.1 r_3) with xi the
    cell centroid's fractions of the bounding box -> (u, v, w)"""
    lo, hi = bounding_box(a)
    xi = (np.asarray(a["cell_centroid"]) - lo) / (hi - lo)
    n = a.n_cells
    r = [splitmix64_uniform(n, k) for k in (1, 2, 3)]
    two_pi = 2.0 * np.pi
    return (np.ascontiguousarray(U0 * (1.0 + 0.5 * np.sin(two_pi * xi[:, 1]) + 0.1 * r[0])),
            np.ascontiguousarray(U0 * (0.3 * np.cos(two_pi * xi[:, 0]) + 0.1 * r[1])),
            np.ascontiguousarray(U0 * (0.2 * np.sin(two_pi * xi[:, 0]) + 0.1 * r[2])))


def analytic_gradients(a):
    """the gradient of the smooth part of tracer_fields at the centroids [n, 3, 3]: what stands in for LINEAR without a device"""
    lo, hi = bounding_box(a)
    xi = (np.asarray(a["cell_centroid"]) - lo) / (hi - lo)
    two_pi = 2.0 * np.pi
    g = np.zeros((a.n_cells, 3, 3))
    g[:, 0, 1] = U0 * 0.5 * two_pi * np.cos(two_pi * xi[:, 1]) / (hi - lo)[1]
    g[:, 1, 0] = -U0 * 0.3 * two_pi * np.sin(two_pi * xi[:, 0]) / (hi - lo)[0]
    g[:, 2, 0] = U0 * 0.2 * two_pi * np.cos(two_pi * xi[:, 0]) / (hi - lo)[0]
    return g


def tracer_seeds(a, n=N_SEEDS, seed=11):
    """n seeds at lo + (0.05 + 0.9 t)(hi - lo), t_k = 0.5 (splitmix64_uniform(n, seed + k) + 1)"""
    lo, hi = bounding_box(a)
    t = np.stack([0.5 * (splitmix64_uniform(n, seed + k) + 1.0) for k in range(3)], axis=1)
    return lo + (0.05 + 0.9 * t) * (hi - lo)


def length_step(a):
    return 0.4 * float(np.cbrt(np.median(np.asarray(a["cell_volume"]))))


def boundary_zones(a):
    return sorted(set(np.asarray(a["face_zone"])[np.asarray(a["face_c1"]) < 0].tolist()))


def assert_conditions(name, a, state, out):
    """what keeps a comparison on this input from being empty, for one direction -> the zones left through.  u > 0 in every cell
    (u >= 0.4 U0), so no particle can leave through the inlet with the flow, nor through the outlet against it: every boundary zone
    is asked of the two directions together (assert_every_zone)."""
    status, n = state["status"], len(state["status"])
    active, left = status == TR.ACTIVE, status == TR.LEFT
    print("%s: %.1f %% left, %.1f %% active, fewest cell changes of an active particle %d, longest walk %d moves"
          % (name, 100.0 * left.mean(), 100.0 * active.mean(), int(out["changes"][active].min()), out["longest"]))
    assert active.sum() >= 0.25 * n and left.sum() >= 0.25 * n
    assert out["changes"][active].min() >= MIN_CHANGES[name]
    assert out["longest"] >= 3
    assert not np.any(status == TR.WALK_LIMIT) and not np.any(status == TR.STAGNANT)
    assert np.all(state["zone"][~left] == -1)
    return set(state["zone"][left].tolist())


def assert_every_zone(a, forward, backward):
    assert sorted(forward | backward) == boundary_zones(a), (sorted(forward), sorted(backward))


@pytest.mark.parametrize("interpolation", [TR.CELL, TR.LINEAR], ids=["cell", "linear"])
@pytest.mark.parametrize("scheme", [TR.EULER, TR.RK2], ids=["euler", "rk2"])
@pytest.mark.parametrize("name", ["hex", "mixed", "poly"])
def test_restatement_moves_leaves_and_crosses_cells(tmp_path, name, scheme, interpolation):
    a = host_mesh(name, tmp_path)
    T = TR.Tables(a)
    f, g = tracer_fields(a), analytic_gradients(a)
    state = TR.seed(T, tracer_seeds(a))
    assert np.all(state["status"] == TR.ACTIVE)  # all seeds INSIDE
    seeds = state["x"].copy()
    n_sub = SUBSTEPS[name]
    out = TR.advect(T, state, f, g, scheme, interpolation, TR.LENGTH, 1, length_step(a), 0.0, n_sub, record_stride=1)
    zones = assert_conditions(name, a, state, out)
    back = TR.seed(T, tracer_seeds(a))  # against the flow: for the zones only
    TR.advect(T, back, f, g, scheme, interpolation, TR.LENGTH, -1, length_step(a), 0.0, n_sub)
    assert_every_zone(a, zones, set(back["zone"][back["status"] == TR.LEFT].tolist()))
    assert np.all(back["age"] < 0.0) and np.all(state["age"] > 0.0)
    # the path is the state's history: record 0 the seeds, the last record the final positions, a stopped particle repeating itself
    path, plen = out["path"], out["path_len"]
    assert path.shape == (n_sub + 1, N_SEEDS, 3) and np.array_equal(path[0], seeds) and np.array_equal(path[-1], state["x"])
    assert np.array_equal(plen, np.minimum(n_sub + 1, 1 + state["steps"]))
    for i in np.nonzero(plen <= n_sub)[0][:20]:
        assert np.all(path[plen[i] - 1:, i] == path[plen[i] - 1, i])
    # every accepted substep is `step` long up to rounding (LENGTH mode): the age is the path's length over the speed, not checked; the
    # segment lengths are
    seg = np.linalg.norm(np.diff(path, axis=0), axis=2)
    moved = np.arange(n_sub)[:, None] < (plen - 1)[None, :]
    if scheme == TR.EULER:
        assert np.allclose(seg[moved], length_step(a), rtol=1e-12)
    assert np.all(seg[~moved] == 0.0)


# ------------------------------------------------------------------ 3. split invariance
@pytest.mark.parametrize("scheme", [TR.EULER, TR.RK2], ids=["euler", "rk2"])
def test_ten_plus_twenty_two_substeps_equal_thirty_two(tmp_path, scheme):
    a = host_mesh("poly", tmp_path)
    T = TR.Tables(a)
    f, g = tracer_fields(a), analytic_gradients(a)
    one, two = TR.seed(T, tracer_seeds(a)), TR.seed(T, tracer_seeds(a))
    args = (f, g, scheme, TR.LINEAR, TR.LENGTH, 1, length_step(a), 0.0)
    TR.advect(T, one, *args, 32)
    TR.advect(T, two, *args, 10)
    assert not np.array_equal(one["x"], two["x"])
    TR.advect(T, two, *args, 22)
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    assert np.array_equal(one["x"].view(np.uint64), two["x"].view(np.uint64)) and np.array_equal(one["age"].view(np.uint64), two["age"].view(np.uint64))
