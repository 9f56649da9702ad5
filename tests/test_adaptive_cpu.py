"""Adaptive time stepping without a device: the new symbols, the layout and defaults of OrcTimeStepControl, orc_time_step_next against
the plain-Python law (tests/adaptive_restatement.py) bit for bit, its refusals, and the restatement's own self-checks."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import adaptive_restatement as A
import transient_restatement as R

BAD_ARGUMENT = 10
SYMBOLS = ("orc_solver_courant", "orc_bench_courant", "orc_time_step_control_default", "orc_time_step_next", "orc_solver_set_time_step",
           "orc_solver_set_time_step_control", "orc_solver_get_time_state", "orc_solver_set_time_state", "orc_solver_time_step_history",
           "orc_solver_time_step_count", "orc_bench_derived_rate")


@pytest.fixture(scope="module")
def lib():
    import orc_amd
    if not os.path.exists(orc_amd._lib.LIB_PATH):
        orc_amd.build()
    return orc_amd._lib.lib()


def control(**kw):
    from orc_amd.settings import TimeStepControl
    return TimeStepControl.make(**kw)


def test_the_new_symbols_exist(lib):
    assert [s for s in SYMBOLS if not hasattr(lib, s)] == []


def test_control_layout_and_defaults(lib):
    from orc_amd.settings import TimeStepControl
    T = TimeStepControl
    assert C.sizeof(T) == 56
    want = dict(target_courant=0, dt_min=8, dt_max=16, max_growth=24, max_shrink=32, interval=40, reserved0=48, reserved1=52)
    assert {k: getattr(T, k).offset for k in want} == want
    c = T()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    lib.orc_time_step_control_default(C.byref(c))
    assert (c.target_courant, c.dt_min, c.dt_max, c.max_growth, c.max_shrink, c.interval, c.reserved0, c.reserved1) == \
        (0.5, 1e-12, 1e12, 1.2, 0.5, 1, 0, 0)
    d = control(target_courant=0.8, dt_min=1e-4, dt_max=2.0, max_growth=1.5, interval=3)
    assert (d.target_courant, d.dt_min, d.dt_max, d.max_growth, d.max_shrink, d.interval) == (0.8, 1e-4, 2.0, 1.5, 0.5, 3)
    with pytest.raises(TypeError):
        control(no_such_field=1)


def test_time_step_next_equals_the_law_bit_for_bit(lib):
    from orc_amd.solver import time_step_next
    seen = set()
    for target, (lo, hi), grow, shrink in itertools.product((0.3, 0.5, 1.7), ((1e-4, 1e-2), (3e-3, 3e-3), (1e-9, 1e3)), (1.0, 1.2, 2.0),
                                                            (0.1, 0.5, 1.0)):
        c = control(target_courant=target, dt_min=lo, dt_max=hi, max_growth=grow, max_shrink=shrink)
        for dt in (1e-4, 7.3e-4, 3e-3, 1e-2, 0.37):
            for rate in (0.0, 1e-300, 0.013, 1.0, 97.3, 161.80339887, 1e4, 3.3e7, 1e300):
                got, want = time_step_next(c, dt, rate), A.step_next(c, dt, rate)
                assert got == want, (target, lo, hi, grow, shrink, dt, rate, got, want)
                raw = target / rate if rate > 0 else hi
                seen.add("rate0" if rate == 0 else "inside" if got == raw else "dt_min" if got == lo and raw < lo else
                         "dt_max" if got == hi and raw > hi else "growth" if got == dt * grow else "shrink" if got == dt * shrink else "other")
    assert {"rate0", "inside", "dt_min", "dt_max", "growth", "shrink"} <= seen, seen


def test_invalid_controls_and_rates_are_refused_and_leave_the_output_alone(lib):
    good = dict(target_courant=0.5, dt_min=1e-4, dt_max=1e-2, max_growth=1.2, max_shrink=0.5, interval=1, reserved0=0, reserved1=0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(target_courant=x) for x in (0.0, -1.0, nan, inf)]
    bad += [dict(dt_min=x) for x in (0.0, -1e-4, nan, inf, 2e-2)] + [dict(dt_max=x) for x in (0.0, -1.0, nan, inf, 1e-5)]
    bad += [dict(max_growth=x) for x in (0.99, 2.01, nan, inf)] + [dict(max_shrink=x) for x in (0.0, -0.5, 1.01, nan)]
    bad += [dict(interval=0), dict(reserved0=1), dict(reserved1=-1)]
    out = C.c_double(-7.25)

    def call(c, dt, rate):
        return lib.orc_time_step_next(C.byref(c) if c is not None else None, C.c_double(dt), C.c_double(rate), C.byref(out))

    for change in bad:
        assert call(control(**dict(good, **change)), 1e-3, 10.0) == BAD_ARGUMENT, change
        assert out.value == -7.25
    c = control(**good)
    for rate in (nan, -1.0, -0.0 - 1e-300, inf, -inf):
        assert call(c, 1e-3, rate) == BAD_ARGUMENT, rate
        assert out.value == -7.25
    for dt in (0.0, -1e-3, nan, inf):
        assert call(c, dt, 10.0) == BAD_ARGUMENT, dt
        assert out.value == -7.25
    assert call(None, 1e-3, 10.0) == BAD_ARGUMENT and out.value == -7.25
    assert lib.orc_time_step_next(C.byref(c), C.c_double(1e-3), C.c_double(10.0), None) == BAD_ARGUMENT
    assert call(c, 1e-3, 10.0) == 0 and out.value == A.step_next(c, 1e-3, 10.0)
    # without a solver the solver entries refuse as well
    assert lib.orc_solver_set_time_step(None, C.c_double(1e-3)) == BAD_ARGUMENT
    assert lib.orc_solver_set_time_step_control(None, C.byref(c)) == BAD_ARGUMENT
    assert lib.orc_solver_time_step_count(None) == 0


def test_unit_ratio_gives_the_fixed_step_coefficients_exactly():
    assert A.coefficients(1.0) == (1.5, 2.0, 0.5)
    for dt in (3.7e-3, 0.01, 1e-7, 123.456):  # the ratio of a step to itself is 1 exactly
        assert A.coefficients(dt / dt) == (1.5, 2.0, 0.5)


@pytest.mark.parametrize("rows", [8, 16, 20])
@pytest.mark.parametrize("scheme", [A.EULER, A.BDF2])
def test_march_var_with_equal_steps_is_march_bit_for_bit(rows, scheme):
    h, nu = 1e-3, 1.0
    K, f = R.operator(rows, h, nu, u_top=1e-6, body=0.3)
    dt, steps = 0.01 * h ** 2 / nu, 12
    u0 = 1e-7 * np.sin(np.arange(rows))
    assert np.array_equal(A.march_var(K, f, u0, [dt] * steps, scheme), R.march(K, f, u0, dt, steps, scheme))


@pytest.mark.parametrize("rows", [8, 16, 20])
@pytest.mark.parametrize("pattern", [(1, 1.5), (1, 2), (1, 1.5, 2.25, 1.5)])
@pytest.mark.parametrize("scheme, lo, hi", [(A.EULER, 0.9, 1.1), (A.BDF2, 1.8, 2.2)])
def test_march_var_keeps_the_order_under_changing_steps(rows, pattern, scheme, lo, hi):
    h, nu = 1e-3, 1.0
    K, f = R.operator(rows, h, nu, u_top=1e-6)
    T = 0.2 * h ** 2 / nu
    exact = R.semi_discrete(K, f, np.zeros(rows), T)
    errs = []
    for steps in (20, 40, 80):
        dts = A.pattern_steps(pattern, steps, T)
        assert abs(dts.sum() - T) <= 1e-12 * T
        u = A.march_var(K, f, np.zeros(rows), dts, scheme)[-1]
        errs.append(np.linalg.norm(u - exact) / np.linalg.norm(exact))
    order = R.observed_order(errs)
    assert np.all((order >= lo) & (order <= hi)), (errs, order)
