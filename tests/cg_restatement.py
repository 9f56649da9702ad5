"""numpy restatement of the device's preconditioned conjugate-gradient arm (include/orc_amd.h, orc_last_cg_stats), line for
line: the recurrence, the stop rules and the event codes.  The device sums in a different association, so the two agree to
rounding, not bit for bit.

    start:      r = b - A x, z = M^-1 r, p = z, rho = r.z, beta0 = |r|
    iteration:  q = A p; alpha = rho / p.q; x += alpha p; r -= alpha q; z = M^-1 r; rho' = r.z; p = z + (rho' / rho) p

M = D (precond = 1, z = r / diag(A)) or the identity (precond = 0): the operator itself is never scaled.  Stops: beta0 == 0
(no iteration); event 2 (rho or p.q non-finite), else event 1 (p.q <= 0), else event 2 (alpha non-finite), tested before the update, so that x keeps the last
completed iterate and the iteration does not count; after the update of an iteration, which counts: event 2 when r.z or
r.r is non-finite, |r| <= threshold * beta0 (threshold > 0 only), or the iteration count."""
import numpy as np


def matvec(a, dtype):
    """CSR product in `dtype` (longdouble: by np.add.reduceat, every sum in longdouble)"""
    if dtype is np.float64:
        return lambda v: a @ v
    data, indices, starts = a.data.astype(dtype), a.indices, a.indptr[:-1]
    assert np.all(np.diff(a.indptr) > 0), "reduceat needs a non-empty row everywhere"
    return lambda v: np.add.reduceat(data * v[indices], starts)


def dot_of(chunk):
    """(u, v) -> u . v; chunk: partial sums over chunks of that many elements, folded afterwards (the device's shape of association)"""
    if not chunk:
        return lambda u, v: u @ v

    def dot(u, v):
        p = u * v
        pad = -len(p) % chunk
        if pad:
            p = np.concatenate([p, np.zeros(pad, p.dtype)])
        return p.reshape(-1, chunk).sum(axis=1).sum()

    return dot


def cg(a, b, x, iteration_count, precond=0, threshold=0.0, dtype=np.float64, chunk=0):
    """x (of `dtype`) is updated in place.  Returns dict(iterations, beta0, residual, event, residuals=[|r| after each
    completed iteration], pq=[p.q of each iteration entered])."""
    st = dict(iterations=0, beta0=dtype(0), residual=dtype(0), event=0, residuals=[], pq=[])
    n = len(b)
    if iteration_count == 0 or n == 0:
        return st
    mv, dot = matvec(a, dtype), dot_of(chunk)
    b = b.astype(dtype)
    dinv = (dtype(1) / a.diagonal().astype(dtype)) if precond else None
    with np.errstate(all="ignore"):
        r = b - mv(x)
        beta0 = np.sqrt(dot(r, r))
        st["beta0"] = st["residual"] = beta0
        if not np.isfinite(beta0):
            st["event"] = 2
            return st
        if beta0 == 0:
            return st
        z = dinv * r if precond else r.copy()
        p = z.copy()
        rho = dot(r, z)
        for it in range(iteration_count):
            q = mv(p)
            pq = dot(p, q)
            st["pq"].append(pq)
            if not (np.isfinite(rho) and np.isfinite(pq)):
                st["event"] = 2
                return st
            if pq <= 0:
                st["event"] = 1
                return st
            alpha = rho / pq
            if not np.isfinite(alpha):
                st["event"] = 2
                return st
            x += alpha * p
            r = r - alpha * q
            z = dinv * r if precond else r
            rho_new = dot(r, z)
            rr = dot(r, r)
            res = np.sqrt(rr)
            st["iterations"] += 1
            st["residual"] = res
            st["residuals"].append(res)
            if not (np.isfinite(rho_new) and np.isfinite(rr)):
                st["event"] = 2
                return st
            if threshold > 0 and res <= dtype(threshold) * beta0:
                return st
            p = z + (rho_new / rho) * p
            rho = rho_new
    return st


def left_scaled(a, b):
    """what the other arms solve under the Jacobi preconditioner: D^-1 A, D^-1 b (linear_algebra.rs:159-167) — not symmetric"""
    import scipy.sparse as sp
    dinv = 1.0 / a.diagonal()
    return (sp.diags(dinv) @ a).tocsr(), dinv * b
