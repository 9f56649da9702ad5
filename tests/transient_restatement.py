"""numpy restatement of the transient arm on a channel cross-section (tests/test_transient_cpu.py checks it, the GPU tests
compare the device against it).

A hex channel that is uniform in y, with walls at y = 0 and y = h, pressure inlet and outlet and symmetry in z, carries a
1-D flow u(y, t) when nothing varies along x.  The finite-volume discretisation the library applies to it is then a
tridiagonal operator: ny cells of height dy, face coefficient nu / dy^2 between neighbours and 2 nu / dy^2 to a wall (the
wall lies half a cell from the centroid, discretization.rs:70-79).  With K that operator and f the wall and body forcing,
    du/dt = -K u + f,
and a time step of the arm is  Euler:  (I/dt + K) u1 = u0/dt + f;  BDF2:  (1.5 I/dt + K) u1 = (2 u0 - 0.5 um1)/dt + f,
BDF2 taking an Euler step first while only one level is known."""
import numpy as np

EULER, BDF2 = 0, 1


def centroids(ny, h):
    dy = h / ny
    return (np.arange(ny) + 0.5) * dy


def operator(ny, h, nu, u_top=0.0, body=0.0):
    """(K, f): du/dt = -K u + f on ny uniform cells; u_top = velocity of the wall at y = h, body = G / rho (G = -dp/dx)"""
    dy = h / ny
    c = nu / dy ** 2
    K = np.zeros((ny, ny))
    for j in range(ny):
        if j > 0:
            K[j, j - 1] = -c
            K[j, j] += c
        if j < ny - 1:
            K[j, j + 1] = -c
            K[j, j] += c
    K[0, 0] += 2 * c
    K[-1, -1] += 2 * c
    f = np.full(ny, float(body))
    f[-1] += 2 * c * u_top
    return K, f


def march(K, f, u0, dt, steps, scheme, u_prev=None):
    """`steps` implicit steps from u0 (u_prev: the level before u0 for BDF2's first step, else it starts as Euler)"""
    n = len(u0)
    I = np.eye(n)
    A_e = I / dt + K
    A_b = 1.5 * I / dt + K
    u, um1 = np.array(u0, dtype=float), (None if u_prev is None else np.array(u_prev, dtype=float))
    out = []
    for _ in range(steps):
        if scheme == BDF2 and um1 is not None:
            u1 = np.linalg.solve(A_b, (2.0 * u - 0.5 * um1) / dt + f)
        else:
            u1 = np.linalg.solve(A_e, u / dt + f)
        um1, u = u, u1
        out.append(u.copy())
    return np.array(out)


def semi_discrete(K, f, u0, t):
    """exact-in-time solution of du/dt = -K u + f (K symmetric) at time t"""
    lam, Q = np.linalg.eigh(K)
    us = np.linalg.solve(K, f)
    coef = Q.T @ (np.asarray(u0, dtype=float) - us)
    return us + Q @ (coef * np.exp(-lam * t))


def couette_series(y, t, h, nu, U, terms=2000):
    """start-up Couette from rest: u = U y/h - (2U/pi) sum_k (-1)^(k+1)/k sin(k pi y/h) exp(-k^2 pi^2 nu t/h^2)"""
    y = np.asarray(y, dtype=float)
    k = np.arange(1, terms + 1)[:, None]
    s = ((-1.0) ** (k + 1) / k * np.sin(k * np.pi * y / h) * np.exp(-k ** 2 * np.pi ** 2 * nu * t / h ** 2)).sum(axis=0)
    return U * y / h - 2 * U / np.pi * s


def poiseuille_series(y, t, h, mu, rho, G, terms=2001):
    """start-up Poiseuille from rest under G = -dp/dx:
    u = (G/2mu) y(h-y) - (4 G h^2/(mu pi^3)) sum_{k odd} k^-3 sin(k pi y/h) exp(-k^2 pi^2 nu t/h^2)"""
    y = np.asarray(y, dtype=float)
    nu = mu / rho
    k = np.arange(1, terms + 1, 2)[:, None]
    s = (k ** -3.0 * np.sin(k * np.pi * y / h) * np.exp(-k ** 2 * np.pi ** 2 * nu * t / h ** 2)).sum(axis=0)
    return G / (2 * mu) * y * (h - y) - 4 * G * h ** 2 / (mu * np.pi ** 3) * s


def observed_order(errors):
    """log2 of successive error ratios for step sizes dt, dt/2, dt/4, ..."""
    e = np.asarray(errors, dtype=float)
    return np.log2(e[:-1] / e[1:])
