"""numpy restatement of the device's restarted GMRES arm (include/orc_amd.h, orc_set_gmres_restart), line for line:
CGS2 Arnoldi, Givens rotations from hypot, restarts, the stopping rules and the breakdown rule.  The device sums in a
different association, so the two agree to rounding, not bit for bit."""
import numpy as np


def jacobi_scaled(a, b):
    """the Jacobi preconditioner of every arm: p_inv * a, p_inv * b (linear_algebra.rs:159-167)"""
    import scipy.sparse as sp
    dinv = 1.0 / a.diagonal()
    return (sp.diags(dinv) @ a).tocsr(), dinv * b


def gmres(a, b, x, iteration_count, restart=30, threshold=0.0, guard=True):
    """x is updated in place.  Returns dict(steps, cycles, beta0, estimate, event, estimates=[|g| per step, per cycle])."""
    restart = 30 if restart == 0 else restart
    if not 1 <= restart <= 64:
        raise ValueError("restart")
    st = dict(steps=0, cycles=0, beta0=0.0, estimate=0.0, event=0, estimates=[])
    n = len(b)
    if iteration_count == 0 or n == 0:
        return st
    m = min(restart, iteration_count)
    left = iteration_count
    first = True
    while left > 0:
        k = min(m, left)
        left -= k
        r = b - a @ x
        beta = np.sqrt(r @ r)
        if first:
            st["beta0"] = beta
            first = False
        st["estimate"] = beta
        if not np.isfinite(beta) and guard:
            st["event"] = 1
            return st
        if beta == 0.0:
            return st
        st["cycles"] += 1
        V = np.zeros((m + 1, n))
        Hm = np.zeros((m + 1, m))
        cs, sn = np.zeros(m), np.zeros(m)
        g = np.zeros(m + 1)
        g[0] = beta
        V[0] = r / beta
        cols, stop, apply = 0, False, True
        ests = []
        for j in range(k):
            w = a @ V[j]
            h1 = V[: j + 1] @ w
            w = w - V[: j + 1].T @ h1
            h2 = V[: j + 1] @ w
            w = w - V[: j + 1].T @ h2
            h = h1 + h2
            hn = np.sqrt(w @ w)
            st["steps"] += 1
            cols = j + 1
            col = np.concatenate([h, [hn]])
            if not np.all(np.isfinite(col)):
                stop = True
                st["estimate"] = np.nan
                if guard:
                    st["event"] = 1
                    apply = False
                else:
                    Hm[: j + 2, j] = col
                break
            happy = hn <= 1e-14 * np.sqrt(col @ col)
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            d = np.hypot(col[j], col[j + 1])
            c, s = (1.0, 0.0) if d == 0.0 else (col[j] / d, col[j + 1] / d)
            cs[j], sn[j] = c, s
            col[j], col[j + 1] = d, 0.0
            Hm[: j + 2, j] = col
            g[j + 1] = -s * g[j]
            g[j] = c * g[j]
            est = abs(g[j + 1])
            st["estimate"] = est
            ests.append(est)
            if happy or (threshold > 0 and est <= threshold * st["beta0"]):
                stop = True
                break
            V[j + 1] = w / hn
        st["estimates"].append(ests)
        if apply:
            y = np.zeros(cols)
            for i in range(cols - 1, -1, -1):
                y[i] = (g[i] - Hm[i, i + 1: cols] @ y[i + 1:]) / Hm[i, i]
            x += V[:cols].T @ y
        if stop:
            return st
    return st
