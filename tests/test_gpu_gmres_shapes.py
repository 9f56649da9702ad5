"""The GMRES kernels (orc_amd/csrc/gmres.hip) over the shapes of tests/gmres_cases.py: restart lengths 1..64 (both tiles of
gmres_update_dots_k, the 64 KB LDS image at restart 59, every edge of the basis-vector-to-wave map), odd n and n below one
tile (the single-element tail of load2 / store2), the three grid-stride bands, step counts below the restart length, stops
by the threshold inside a cycle, lucky breakdowns at a step d > 1, and two ranks with an odd number of owned rows.  The
reference is the longdouble restatement; the bound is 50 d_case, d_case being the rounding scale of the case measured from
the references alone (tests/test_gmres_shapes_cpu.py proves the conditions this file relies on).

What the bound cannot see: dropping the second pass's coefficients from the Hessenberg (h = h1) while keeping its vector
update changes H by eps |h1| only, because the basis stays orthonormal; restated in float64 it moves x by at most 10 d_case."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gmres_cases as G
import gmres_restatement as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
GMRES = 19
_RATIOS = {}


def device_solve(a, b, iters, restart, precond, threshold=0.0, x0=None):
    from orc_amd.linear_algebra import iterative_solve, last_gmres_stats, set_gmres_restart
    set_gmres_restart(restart)
    x = np.zeros(a.shape[0]) if x0 is None else x0.copy()
    try:
        st = iterative_solve(a, b, x, iters, GMRES, 0.5, threshold, precond, raise_on_error=False)
    finally:
        set_gmres_restart(0)
    return st, x, last_gmres_stats()


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    if _RATIOS:
        print("\ndevice error / d_case, maximum per case family:")
        for key in sorted(_RATIOS):
            print("  %-28s %8.2f  (%d cases)" % (key, _RATIOS[key][0], _RATIOS[key][1]))


def check_x(key, label, x, x_ref, d_case):
    err = G.rel(x, x_ref)
    ratio = err / d_case
    worst, count = _RATIOS.get(key, (0.0, 0))
    _RATIOS[key] = (max(worst, ratio), count + 1)
    print("%s: device error %.3e, d_case %.3e, ratio %.2f" % (label, err, d_case, ratio))
    # measured on an MI355X: the largest ratio over every case of this file is 5.4 (cd3, n = 1009, restart 32, 67 steps); the
    # synthetic 1-D family and the p' system stay under 1.6, the u system under 4.1
    assert err <= 50 * d_case, (label, err, d_case, ratio)


def tile_of(restart, steps):
    nq = min(restart, steps)
    return "tile64" if nq > 59 else ("tile128-hi" if nq > 30 else "tile128-lo")


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_iterates(gpu, c):
    a, b = G.system(c.family, c.n)
    x0 = G.start_vector(c)
    st, x, (steps, cycles, beta0, est) = device_solve(a, b, c.steps, c.restart, c.precond, x0=x0)
    assert st == 0
    if c.n in G.LARGE_SIZES:
        ah, bh = G.host_system(c)
        x_ref = np.zeros(c.n) if x0 is None else x0.copy()
        sr = R.gmres(ah, bh, x_ref, c.steps, restart=c.restart)
        d_case = G.large_case_d(c)
    else:
        r = G.case_references(c)
        x_ref, sr, d_case = r["x_ld"], r["st64"], r["d_case"]
    assert (steps, cycles) == (sr["steps"], sr["cycles"]), (steps, cycles, sr["steps"], sr["cycles"])
    assert abs(beta0 - sr["beta0"]) <= 1e-13 * sr["beta0"], (beta0, sr["beta0"])
    size = "large" if c.n in G.LARGE_SIZES else ("n<128" if c.n < 128 else "mid")
    check_x("%s %s %s" % (c.family, size, tile_of(c.restart, c.steps)), G.case_id(c), x, x_ref, d_case)


@pytest.mark.parametrize("t", G.THRESHOLD_CASES, ids=lambda t: "%s-r%d-%s" % (t.family, t.restart, t.where))
def test_threshold_stop_inside_a_cycle(gpu, t):
    a, b = G.system(t.family, t.n)
    thr = G.threshold_of(t)
    r = G.threshold_references(t)
    sr = r["st64"]
    assert (sr["steps"], sr["cycles"]) == ((t.cycle - 1) * t.restart + t.step, t.cycle)
    st, x, (steps, cycles, beta0, est) = device_solve(a, b, t.steps, t.restart, t.precond, threshold=thr)
    assert st == 0
    assert (steps, cycles) == (sr["steps"], sr["cycles"]), (steps, cycles, sr["steps"], sr["cycles"])
    assert abs(est - sr["estimate"]) <= 1e-6 * sr["estimate"], (est, sr["estimate"])
    check_x("threshold %s" % t.family, "%s r%d %s" % (t.family, t.restart, t.where), x, r["x_ld"], r["d_case"])


@pytest.mark.parametrize("t", G.BREAKDOWN_CASES, ids=lambda t: "n%d-d%d" % t)
def test_lucky_breakdown_at_step_d(gpu, t):
    a, b, exact = G.breakdown_system(t)
    st, x, (steps, cycles, _, _) = device_solve(a, b, G.BREAKDOWN_RESTART + 7, G.BREAKDOWN_RESTART, 0)
    assert st == 0
    assert (steps, cycles) == (t.d, 1), (steps, cycles)
    err = G.rel(x, exact)
    print("n %d d %d: error %.3e" % (t.n, t.d, err))
    assert err <= 1e-12, err


def test_restart_64_is_accepted(gpu):
    # 65 is refused: test_gpu_gmres.py::test_edge_rules
    a, b = G.system("cd1", 129)
    st, x, (steps, cycles, _, _) = device_solve(a, b, 64, 64, 0)
    assert st == 0 and (steps, cycles) == (64, 1) and np.isfinite(x).all()


def test_bit_reproducible_at_restart_64_and_odd_n(gpu):
    n = G.LARGE_SIZES[1]
    assert n > 262144 and n % 2 == 1
    a, b = G.system("cd3", n)
    st1, x1, s1 = device_solve(a, b, 70, 64, 1)
    st2, x2, s2 = device_solve(a, b, 70, 64, 1)
    assert st1 == 0 and st2 == 0 and s1[:2] == (70, 2)
    assert np.array_equal(x1, x2) and s1 == s2


def test_two_ranks_with_an_odd_owned_count_match_the_single_rank_run(gpu):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "gmres_shapes_mp_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    print(r.stdout[-2000:])
    assert "GMRES_SHAPES_MP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
