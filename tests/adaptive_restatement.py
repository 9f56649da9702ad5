"""Adaptive time stepping restated in numpy / plain Python (tests/test_adaptive_cpu.py checks it, the GPU tests compare the device
against it).

    coefficients(w)            variable-step BDF2, w = dt / dt_last:  a0 = (1 + 2w)/(1 + w), a1 = 1 + w, a2 = (w w)/(1 + w)
                               (w = 1: 1.5, 2, 0.5 exactly)
    step_next(c, dt, rate)     the controller law, operator for operator:
                                   want = rate > 0 ? target_courant / rate : dt_max
                                   next = min(max(want, dt * max_shrink), dt * max_growth)
                                   next = min(max(next, dt_min), dt_max)
    march_var(K, f, u0, dts, scheme)
                               variable-step Euler / BDF2 on du/dt = -K u + f, the operator of tests/transient_restatement.py:
                                   Euler:  (I/dt + K) u1 = u0/dt + f
                                   BDF2:   (a0 I/dt + K) u1 = (a1 u0 - a2 um1)/dt + f,  an Euler step first
    pattern_steps(pattern, steps, T)
                               `steps` steps whose sizes repeat `pattern` and sum to T
"""
import numpy as np

EULER, BDF2 = 0, 1


def coefficients(w):
    return (1.0 + 2.0 * w) / (1.0 + w), 1.0 + w, (w * w) / (1.0 + w)


def step_next(c, dt, rate):
    """c: anything with the fields of OrcTimeStepControl"""
    want = c.target_courant / rate if rate > 0.0 else c.dt_max
    nxt = min(max(want, dt * c.max_shrink), dt * c.max_growth)
    return min(max(nxt, c.dt_min), c.dt_max)


def march_var(K, f, u0, dts, scheme, u_prev=None, dt_prev=None, coef=coefficients):
    """one implicit step per entry of dts from u0 (u_prev, dt_prev: the level before u0 and the step that led from it to u0);
    coef: the BDF2 coefficients as a function of w (a test passes the fixed-step ones to see what they would cost)"""
    n = len(u0)
    I = np.eye(n)
    u, um1, last = np.array(u0, dtype=float), (None if u_prev is None else np.array(u_prev, dtype=float)), dt_prev
    out = []
    for dt in dts:
        if scheme == BDF2 and um1 is not None:
            a0, a1, a2 = coef(dt / last)
            u1 = np.linalg.solve(a0 * I / dt + K, (a1 * u - a2 * um1) / dt + f)
        else:
            u1 = np.linalg.solve(I / dt + K, u / dt + f)
        um1, u, last = u, u1, dt
        out.append(u.copy())
    return np.array(out)


def pattern_steps(pattern, steps, T):
    p = np.array([pattern[k % len(pattern)] for k in range(steps)], dtype=float)
    return p * (T / p.sum())
