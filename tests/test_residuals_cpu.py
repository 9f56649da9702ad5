"""Residual monitors without a device: the ABI of OrcConvergence against its ctypes mirror, the stopping rule
(orc_convergence_check: pure host arithmetic), the new entries' answer where there is no device, and the numpy restatement
(tests/residual_restatement.py) against a dense b - A x on a hand-built system."""
import ctypes as C
import os
import re

import numpy as np

import residual_restatement as R
from conftest import ROOT

F64 = C.POINTER(C.c_double)
BAD_ARGUMENT, NO_DEVICE = 10, 11


def record(scaled):
    rec = np.zeros(R.N)
    rec[R.SCALED:R.SCALED + 4] = scaled
    return rec


def test_convergence_struct_matches_the_header():
    from orc_amd.settings import Convergence
    assert C.sizeof(Convergence) == 48
    assert [(getattr(Convergence, f).offset, getattr(Convergence, f).size) for f, _ in Convergence._fields_] == [(0, 24), (24, 8), (32, 8), (40, 4)]
    txt = open(os.path.join(ROOT, "include", "orc_types.h")).read()
    body = re.search(r"typedef struct OrcConvergence \{(.*?)\} OrcConvergence;", txt, re.S).group(1)
    names = re.findall(r"^\s*(?:double|uint64_t|int32_t)\s+(\w+)", body, re.M)
    assert names == [f for f, _ in Convergence._fields_]
    from orc_amd.solver import RESIDUAL_NAMES
    assert len(RESIDUAL_NAMES) == R.N and "ORC_RESIDUAL_N = %d" % R.N in txt
    for name, value in (("MOMENTUM_L1", R.L1), ("MOMENTUM_SCALE", R.SCALE), ("MOMENTUM_SQ", R.SQ), ("MOMENTUM_MAX", R.MAX),
                        ("CONTINUITY_L1", R.C_L1), ("CONTINUITY_SQ", R.C_SQ), ("CONTINUITY_MAX", R.C_MAX),
                        ("CONTINUITY_SCALE", R.C_SCALE), ("MOMENTUM_SCALED", R.SCALED), ("CONTINUITY_SCALED", R.C_SCALED)):
        assert "ORC_RESIDUAL_%s = %d," % (name, value) in txt, name
    src = open(os.path.join(ROOT, "orc_amd", "csrc", "api_solver.cpp")).read()
    assert "sizeof(OrcConvergence) == 48" in src  # pinned on the C side too


def test_convergence_check_rule():
    from orc_amd.settings import Convergence
    from orc_amd.solver import convergence_check
    c = Convergence.make(momentum=(1e-3, 2e-3, 4e-3), continuity=1e-2)
    assert convergence_check(c, record([5e-4, 1e-3, 2e-3, 5e-3])) == (1, 0)          # all below
    assert convergence_check(c, record([1e-3, 2e-3, 4e-3, 1e-2])) == (1, 0)          # equal to the tolerance: <=
    for k, bad in enumerate(([2e-3, 1e-3, 2e-3, 5e-3], [5e-4, 3e-3, 2e-3, 5e-3], [5e-4, 1e-3, 5e-3, 5e-3], [5e-4, 1e-3, 2e-3, 2e-2])):
        assert convergence_check(c, record(bad)) == (0, 1 << k), k                   # one above: its bit alone
    above = np.nextafter(1e-3, 1.0)
    assert convergence_check(c, record([above, 1e-3, 2e-3, 5e-3])) == (0, 1)
    assert convergence_check(c, record([1.0, 1.0, 2e-3, 1.0])) == (0, 0b1011)
    for k in range(4):                                                               # NaN and inf never converge
        for v in (float("nan"), float("inf")):
            r = [5e-4, 1e-3, 2e-3, 5e-3]
            r[k] = v
            assert convergence_check(c, record(r)) == (0, 1 << k), (k, v)
    huge = Convergence.make(momentum=float("inf"), continuity=float("inf"))          # not even under infinite tolerances a NaN
    assert convergence_check(huge, record([1e300, 0.0, 5.0, 1e-300])) == (1, 0)
    assert convergence_check(huge, record([float("nan")] * 4)) == (0, 15)
    # a tolerance of 0: never satisfied by that equation, not even at a residual of exactly 0
    z = Convergence.make(momentum=(0.0, 1.0, 1.0), continuity=1.0)
    assert convergence_check(z, record([0.0, 0.5, 0.5, 0.5])) == (0, 1)
    assert convergence_check(Convergence.make(momentum=0.0, continuity=0.0), record([0.0] * 4)) == (0, 15)
    # min_iterations is the loop's business, not the check's
    assert convergence_check(Convergence.make(momentum=1.0, continuity=1.0, min_iterations=10 ** 6), record([0.5] * 4)) == (1, 0)
    # only slots 16..19 are read
    rec = np.full(R.N, float("nan"))
    rec[R.SCALED:] = 0.5
    assert convergence_check(Convergence.make(momentum=1.0, continuity=1.0), rec) == (1, 0)


def test_invalid_rules_are_refused_by_the_check():
    from orc_amd._lib import lib
    from orc_amd.settings import Convergence
    from orc_amd.solver import convergence_check
    rec = record([0.0] * 4)
    for bad in (Convergence.make(momentum=(-1e-9, 1, 1)), Convergence.make(momentum=(1, float("nan"), 1)),
                Convergence.make(continuity=-1.0), Convergence.make(continuity=float("nan"))):
        assert convergence_check(bad, rec) == (-1, 15)
    r0 = Convergence.make()
    r0.reserved0 = 1
    assert convergence_check(r0, rec) == (-1, 15)
    assert convergence_check(None, rec) == (-1, 15)
    assert lib().orc_convergence_check(C.byref(Convergence.make()), None, None) == -1
    assert lib().orc_convergence_check(C.byref(Convergence.make(1.0, 1.0)), rec.ctypes.data_as(F64), None) == 1  # the mask is optional


def test_new_entries_look_for_a_device_first():
    """fails on a library built before the monitors existed; without a device every compute entry says so whatever the arguments,
    with one a null solver is a bad argument"""
    import orc_amd
    from orc_amd._lib import lib
    from orc_amd.settings import Convergence
    L = lib()
    for name in ("orc_solver_set_monitors", "orc_solver_residual_count", "orc_solver_residual_history", "orc_convergence_check",
                 "orc_solver_iterate_until", "orc_solve_steady_converged", "orc_solver_get_pressure_rhs"):
        assert hasattr(L, name), name
    want = NO_DEVICE if orc_amd.device_count() < 1 else BAD_ARGUMENT
    out = np.zeros(R.N)
    c = Convergence.make()
    done, conv = C.c_uint64(7), C.c_int32(7)
    assert L.orc_solver_set_monitors(None, 1) == want
    assert L.orc_solver_residual_history(None, 0, 1, out.ctypes.data_as(F64)) == want
    assert L.orc_solver_iterate_until(None, 3, C.byref(c), None, C.byref(done), C.byref(conv)) == want
    assert L.orc_solve_steady_converged(None, None, None, None, None, None, 1.0, 1.0, C.byref(c), 3, 0, None, None, C.byref(done),
                                        C.byref(conv), out.ctypes.data_as(F64)) == want
    assert L.orc_solver_get_pressure_rhs(None, out.ctypes.data_as(F64)) == want
    assert L.orc_solver_residual_count(None) == 0
    assert (done.value, conv.value) == (7, 7) and not out.any()  # a refused call writes nothing


def test_restatement_equals_dense_on_a_hand_built_system():
    """5 rows: row 1 stores no diagonal, row 3 is empty; exactly representable values, so dense b - A @ x is exact too"""
    row_ptr = np.array([0, 2, 4, 7, 7, 9])
    col = np.array([0, 2, 0, 4, 1, 2, 3, 0, 4])
    val = np.array([4.0, -1.0, 0.5, -2.0, -0.25, 3.0, 1.5, -0.75, 2.0])
    x = np.array([1.0, -2.0, 0.5, 4.0, -1.5])
    b = np.array([3.0, 0.25, -1.0, 7.0, 0.125])
    A = np.zeros((5, 5))
    for i in range(5):
        A[i, col[row_ptr[i]:row_ptr[i + 1]]] = val[row_ptr[i]:row_ptr[i + 1]]
    r, d = R.momentum(val, b, x, (row_ptr, col))
    assert np.array_equal(r, b - A @ x)
    assert np.array_equal(d, np.array([4.0 * 1.0, 0.0, 3.0 * 0.5, 0.0, 2.0 * -1.5]))
    assert r[3] == b[3]  # the empty row's residual is its right-hand side
    rec, bound = R.momentum_slots([(r, d)] * 3)
    assert rec[R.L1] == np.abs(r).sum() and rec[R.SCALE] == np.abs(d).sum() and rec[R.SQ] == (r * r).sum() and rec[R.MAX] == np.abs(r).max()
    assert np.array_equal(rec[R.L1:R.L1 + 3], np.full(3, rec[R.L1])) and np.all(bound[R.MAX:R.MAX + 3] == 0.0)
    # owned rows only: a partitioned rank's ghost rows take no part
    r3, d3 = R.momentum(val, b, x, (row_ptr, col), n_rows=3)
    assert np.array_equal(r3, r[:3]) and np.array_equal(d3, d[:3])
    crec, _ = R.continuity_slots(b, n_rows=4)
    assert (crec[R.C_L1], crec[R.C_SQ], crec[R.C_MAX]) == (11.25, 9.0 + 0.0625 + 1.0 + 49.0, 7.0)


def test_host_slots_of_a_history():
    """slot 15 = the largest slot 12 of the first min(k, 5) records, then fixed; the quotients and their zero-scale rules"""
    h = np.zeros((7, R.N))
    h[:, R.C_L1] = [2.0, 3.0, 1.0, 0.5, 4.0, 9.0, 0.25]
    h[:, R.L1:R.L1 + 3] = [[1.0, 2.0, 3.0]] * 7
    h[:, R.SCALE:R.SCALE + 3] = [[4.0, 0.0, 6.0]] * 7
    f = R.finish(h)
    assert list(f[:, R.C_SCALE]) == [2.0, 3.0, 3.0, 3.0, 4.0, 4.0, 4.0]
    assert list(f[:, R.C_SCALED]) == [1.0, 1.0, 1.0 / 3.0, 0.5 / 3.0, 1.0, 9.0 / 4.0, 0.25 / 4.0]
    assert np.array_equal(f[0, R.SCALED:R.SCALED + 3], [0.25, 2.0, 0.5])  # a zero scale: the residual itself
    assert np.all(R.finish(np.zeros((3, R.N)))[:, R.C_SCALED] == 0.0)     # a zero continuity scale: 0
