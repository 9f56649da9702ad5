"""numpy restatement of the BiCGSTAB arm (orc_amd/csrc/bicgstab.hip, oracle/linear_algebra.c:194-220) and of the Multigrid arm
around it (oracle/linear_algebra.c:58-94, :221-235), parametrised by the dtype of the vectors and by the association of the
sums.  The device sums in a tree of its own, so the two agree to rounding, not bit for bit.

    start:      r = b - A x; p = r; rho = sum(r)                                   (r_hat_0 = 1)
    iteration:  nu = A p; alpha = rho / sum(nu); s = r - alpha nu; t = A s; omega = (t.s) / (t.t);
                x = (x + alpha p) + omega s; r = s - omega t; rho' = sum(r); beta = rho' / rho * alpha / omega;
                p = r + beta (p - omega nu)

No test of any denominator: the reference has none, and the device's breakdown guard changes nothing while none is 0.

The Jacobi preconditioner is the left scaling of linear_algebra.c:104-127: row i of A times 1 / a_ii, one product per entry,
b_i times 1 / a_ii; a row whose diagonal is not stored becomes EMPTY and its b entry 0.  The scaled matrix and the inverse
diagonal are float64 data in every variant (one rounding per entry, the same on the device and in the oracle); matrices never
change dtype, only vectors and sums do.

Sums (class Sums):  "ld" / "pairwise": numpy's .sum() in the dtype of the vector;  "chunk": partial sums over chunks of 512
elements folded afterwards, the device's shape (a vector workgroup holds 256 lanes of two elements);  "oracle": or_dot's eight
accumulators (oracle/sparse.c), which makes the float64 restatement the oracle's arithmetic bit for bit.
Two wrong forms for tests/test_bicg_cpu.py: drop="last" leaves the last element out of every sum (a lost n & 1 tail),
drop="block" leaves one chunk of 512 elements out (a lost partial sum): the middle one, chunk (count // 2), of a sum over
more than one chunk; a sum over a single chunk stays whole (losing its only partial sum is losing the sum)."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
CHUNK = 512
MAX_LEVELS = 3      # MULTIGRID_COARSENING_LEVELS (linear_algebra.c:14): with the fine level, four levels
MIN_ROWS = 16       # a coarse operator of <= 16 rows is not coarsened further (:79)


def matvec(a, dtype):
    """v -> A v in `dtype`.  float64: scipy's CSR product (every row in ascending column order from 0.0, what the device's
    products do bit for bit).  longdouble: products and row sums in longdouble; np.add.reduceat over the rows that hold
    entries only, since it cannot express an empty row (it would return the entry at the row's start instead of 0)."""
    if dtype is np.float64:
        return lambda v: a @ v
    n = a.shape[0]
    data, indices = a.data.astype(dtype), a.indices
    lens = np.diff(a.indptr)
    live = np.flatnonzero(lens > 0)
    starts = a.indptr[:-1][live]

    def mv(v):
        out = np.zeros(n, dtype)
        if len(live):
            out[live] = np.add.reduceat(data * v[indices], starts)
        return out

    return mv


class Sums:
    """sum(u) and dot(u, v) in one association (module docstring)"""

    def __init__(self, kind="pairwise", drop=None):
        assert kind in ("ld", "pairwise", "chunk", "oracle") and drop in (None, "last", "block")
        self.kind, self.drop = kind, drop

    def _fold(self, p):
        n = len(p)
        if self.drop == "last":
            p = p[:-1]
        elif self.drop == "block" and n > CHUNK:
            j = ((n + CHUNK - 1) // CHUNK) // 2
            p = np.concatenate([p[:j * CHUNK], p[(j + 1) * CHUNK:]])
        if self.kind == "chunk":
            pad = -len(p) % CHUNK
            if pad:
                p = np.concatenate([p, np.zeros(pad, p.dtype)])
            return p.reshape(-1, CHUNK).sum(axis=1).sum()
        if self.kind == "oracle":
            m = len(p) // 8 * 8
            acc = np.zeros(8, p.dtype)
            for row in p[:m].reshape(-1, 8):  # eight running sums, one addition each per row
                acc = acc + row
            res = p.dtype.type(0)
            for k in range(4):
                res = res + (acc[k] + acc[k + 4])
            for v in p[m:]:
                res = res + v
            return res
        return p.sum()

    def sum(self, u):
        return self._fold(u)

    def dot(self, u, v):
        return self._fold(u * v)


def jacobi_scaled(a):
    """(D^-1 A, 1 / diag) as float64 data (linear_algebra.c:104-127); a row without a stored diagonal comes out empty and its
    inverse diagonal 0, which turns its b entry into 0"""
    a = a.tocsr()
    n = a.shape[0]
    lens = np.diff(a.indptr)
    rid = np.repeat(np.arange(n), lens)
    on_diag = a.indices == rid
    dinv = np.zeros(n)
    dinv[rid[on_diag]] = 1.0 / a.data[on_diag]
    has = np.zeros(n, bool)
    has[rid[on_diag]] = True
    keep = has[rid]
    vals = 0.0 + dinv[rid[keep]] * a.data[keep]
    indptr = np.concatenate([[0], np.cumsum(np.where(has, lens, 0))])
    return sp.csr_matrix((vals, a.indices[keep], indptr), shape=a.shape), dinv


def bicgstab(a, b, x, iterations, dtype=np.float64, sums=None, keep=()):
    """fixed-count BiCGSTAB on (a, b) as they stand; x (of `dtype`) is updated in place.  keep: iteration counts after which
    a copy of x is returned, {count: x}."""
    S = sums or Sums()
    mv = matvec(a, dtype)
    b = b.astype(dtype)
    kept = {}
    with np.errstate(all="ignore"):
        r = b - mv(x)
        rho = S.sum(r)
        p = r.copy()
        for it in range(iterations):
            nu = mv(p)
            alpha = rho / S.sum(nu)
            s = r - alpha * nu
            t = mv(s)
            omega = S.dot(t, s) / S.dot(t, t)
            x[:] = (x + alpha * p) + omega * s
            r = s - omega * t
            rho_prev = rho
            rho = S.sum(r)
            beta = rho / rho_prev * alpha / omega
            p = r + beta * (p - omega * nu)
            if it + 1 in keep:
                kept[it + 1] = x.copy()
    return kept


def solve(a, b, x, iterations, precond, dtype=np.float64, sums=None, keep=()):
    """iterative_solve(..., BICGSTAB, preconditioner): the scaling, then the recurrence.  b may be of `dtype` already."""
    if precond:
        a, dinv = jacobi_scaled(a)
        b = dinv.astype(dtype) * b.astype(dtype)
    return bicgstab(a, b, x, iterations, dtype, sums, keep)


# ------------------------------------------------------------------ Multigrid arm
def hierarchy(oracle, a):
    """[(R, R^T, (R a) R^T)] of every level below `a` — the operator the arm coarsens: the once-scaled system under the Jacobi
    preconditioner — from the oracle, as float64 scipy matrices: a level is coarsened while it is one of the first three
    coarse ones and the one before it has more than 16 rows"""
    out = []
    A = oracle.Csr.from_scipy(a)
    level = 1
    while True:
        R = oracle.build_restriction_matrix(A)
        Rt = R.transpose()
        Ac = R.matmul(A).matmul(Rt)
        out.append((R.to_scipy(), Rt.to_scipy(), Ac.to_scipy()))
        if not (level < MAX_LEVELS and Ac.shape[0] > MIN_ROWS):
            return out
        A, level = Ac, level + 1


def _coarse(levels, k, r, iterations, precond, dtype, sums):
    """multigrid_solve (linear_algebra.c:58-94) on level k of `levels` with the residual r passed down"""
    R, Rt, ac = levels[k]
    r_prime = matvec(R, dtype)(r)
    e = np.zeros(ac.shape[0], dtype)
    solve(ac, r_prime, e, iterations, precond, dtype, sums)
    if k + 1 < len(levels):
        e += _coarse(levels, k + 1, r_prime, iterations, precond, dtype, sums)  # r', not the residual of e
        solve(ac, r_prime, e, iterations, precond, dtype, sums)  # at threshold / 10, which BiCGSTAB never reads
    return matvec(Rt, dtype)(e)


def scaled_operator(a, precond):
    """the operator the Multigrid arm smooths and coarsens"""
    return jacobi_scaled(a)[0] if precond else a.tocsr()


def multigrid(a, b, x, iterations, precond, levels, dtype=np.float64, sums=None):
    """iterative_solve(..., MULTIGRID, preconditioner) with BiCGSTAB as the smoother; levels: hierarchy(oracle, scaled_operator(a,
    precond)).  Every smoothing solve scales the system it is given once more (nested rescaling)."""
    b = b.astype(dtype)
    if precond:
        a, dinv = jacobi_scaled(a)
        b = dinv.astype(dtype) * b
    solve(a, b, x, iterations, precond, dtype, sums)
    r = b - matvec(a, dtype)(x)
    x += _coarse(levels, 0, r, iterations, precond, dtype, sums)
