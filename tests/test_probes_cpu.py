"""Point probes without a device: the enums against the header, the entries without a device, and the numpy restatement of the
locate (tests/probe_restatement.py: nearest centroid, then the half-space walk) against an independent brute-force container — the
argmin over all cells of max_f g_f — on a small and a larger hex channel and on the mixed and polyhedral channels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import probe_restatement as PR
from conftest import ROOT, splitmix64_uniform

N_POINTS = 3000
SEED = 101
NO_DEVICE = 11


def test_enums_match_the_header(tmp_path):
    from orc_amd import settings as S
    names = ["ORC_PROBE_STATUS_INSIDE", "ORC_PROBE_STATUS_OUTSIDE", "ORC_PROBE_STATUS_WALK_LIMIT", "ORC_PROBE_U", "ORC_PROBE_V", "ORC_PROBE_W",
             "ORC_PROBE_P", "ORC_PROBE_PHI", "ORC_PROBE_MU", "ORC_PROBE_N", "ORC_PROBE_CELL", "ORC_PROBE_LINEAR", "ORC_PROBE_WALK_LIMIT"]
    src = '#include <stdio.h>\n#include "orc_types.h"\nint main(){' + "".join('printf("%%d ", (int)%s);' % n for n in names) + "return 0;}"
    exe = str(tmp_path / "enums")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    F, I, T = S.ProbeField, S.ProbeInterpolation, S.ProbeStatus
    assert got == [T.INSIDE, T.OUTSIDE, T.WALK_LIMIT, F.U, F.V, F.W, F.P, F.PHI, F.MU, F.N, I.CELL, I.LINEAR, S.PROBE_WALK_LIMIT]
    assert got == [0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 0, 1, 64]
    assert (PR.INSIDE, PR.OUTSIDE, PR.WALK_LIMIT, PR.WALK_LIMIT_MOVES) == (0, 1, 2, 64)
    from orc_amd.solver import PROBE_NAMES
    assert PROBE_NAMES == ("u", "v", "w", "p", "phi", "mu")


def test_entries_return_no_device_without_a_device():
    import orc_amd
    from orc_amd._lib import lib
    if orc_amd.device_count() > 0:
        pytest.skip("a device is present")
    L = lib()
    st = C.c_int(0)
    xyz = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert L.orc_probes_create(None, 1, xyz, C.byref(st)) is None and st.value == NO_DEVICE
    st = C.c_int(0)
    assert L.orc_debug_probes_locate(None, 1, xyz, 0, 2, C.byref(st)) is None and st.value == NO_DEVICE
    assert L.orc_probes_get(None, None, None, None, None, None) == NO_DEVICE
    assert L.orc_solver_sample_probes(None, None, 1, 0, None) == NO_DEVICE
    assert L.orc_solver_set_probe_history(None, None, 1, 0, 1) == NO_DEVICE
    assert L.orc_solver_record_probes(None, 0.0) == NO_DEVICE
    assert L.orc_solver_probe_history_count(None) == -1
    assert L.orc_solver_probe_history(None, 0, 0, None, None) == NO_DEVICE
    ms = (C.c_double * 2)()
    assert L.orc_bench_probe_locate(None, None, 1, 1, ms) == NO_DEVICE
    assert L.orc_probes_count(None) == 0
    L.orc_probes_destroy(None)
    out = (C.c_longlong * 6)()
    assert L.orc_debug_probe_search(out, 0) == 0 and out[0] >= 1  # host counters: no device needed


# ------------------------------------------------------------------ the restatement against the brute-force container
def host_mesh(name, tmp_path):
    from orc_amd import io as orc_io
    from orc_amd.mesh import MeshArrays, hex_channel, write_mixed_channel_msh
    if name.startswith("hex"):
        return hex_channel(*{"hex_small": (5, 4, 3), "hex_large": (32, 16, 12)}[name])
    path = str(tmp_path / (name + ".msh"))
    write_mixed_channel_msh(path, 24, 5, 4, lz=4e-4 * 1.3, polyhedra=name == "poly")  # the mesh of test_gpu_surface.mixed_case
    return MeshArrays(orc_io.read_mesh(path).arrays())


def bounding_box(a):
    fc = np.asarray(a["face_centroid"])
    b = np.asarray(a["face_c1"]) < 0
    return fc[b].min(axis=0), fc[b].max(axis=0)


def seeded_points(a, n=N_POINTS, seed=SEED):
    """n points at fractions 0.001 .. 0.999 of the bounding box"""
    lo, hi = bounding_box(a)
    t = np.stack([0.5 * (splitmix64_uniform(n, seed + k) + 1.0) for k in range(3)], axis=1)
    return lo + (0.001 + 0.998 * t) * (hi - lo)


@pytest.mark.parametrize("name", ["hex_small", "hex_large", "mixed", "poly"])
def test_restatement_agrees_with_the_brute_force_container(tmp_path, name):
    a = host_mesh(name, tmp_path)
    x = seeded_points(a)
    best, count = PR.containers(a, x)
    assert np.all(count == 1), "condition 1: %d points without exactly one containing cell" % np.count_nonzero(count != 1)
    start = PR.start_cells(a, x)
    loc = PR.walk(a, x, start)
    assert np.all(loc["status"] == PR.INSIDE) and np.array_equal(loc["cell"], best)  # condition 2
    assert np.all(loc["excess"] <= 0.0) and np.all(loc["zone"] == -1)
    print("%s: most moves %d, start cell differs from the container for %.1f %% of the points"
          % (name, int(loc["steps"].max()), 100.0 * np.mean(start != best)))
    assert loc["steps"].max() <= 8  # condition 3
    assert np.array_equal(loc["steps"] == 0, start == best)
    if name in ("mixed", "poly"):
        assert np.mean(start != best) >= 0.10  # condition 4: the walk is exercised


def test_points_outside_the_box_end_outside_with_the_zone_they_left_through():
    from orc_amd.mesh import hex_channel
    a = hex_channel(5, 4, 3)
    lo, hi = bounding_box(a)
    mid, span = 0.5 * (lo + hi), hi - lo
    sides = {"INLET": (0, -1), "OUTLET": (0, 1), "BOTTOM_WALL": (1, -1), "TOP_WALL": (1, 1), "PERIODIC_-Z": (2, -1), "PERIODIC_+Z": (2, 1)}
    for zone, (axis, sign) in sides.items():
        x = mid.copy()
        x[axis] = (hi if sign > 0 else lo)[axis] + sign * 0.37 * span[axis]
        loc = PR.locate(a, x[None, :])
        assert loc["status"][0] == PR.OUTSIDE and loc["zone"][0] == a.get_face_zone(zone), zone
        assert loc["excess"][0] > 0.0
        assert abs(loc["excess"][0] - 0.37 * span[axis]) <= 1e-12 * span[axis]
