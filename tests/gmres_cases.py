"""Case table and references of the GMRES shape tests (tests/test_gmres_shapes_cpu.py, tests/test_gpu_gmres_shapes.py).

Matrices (generated here, nothing committed): "cd1" a non-symmetric 1-D convection-diffusion tridiagonal, "cd3" the leading
n x n block of a non-symmetric 3-D 7-point convection-diffusion stencil with a skew convective part (unequal off-diagonals,
a varying diagonal, weak diagonal dominance), and the "u" / "p" systems of golden/channel_flow.npz (n = 1008).  Right-hand
sides and starting vectors come from conftest.splitmix64_uniform.

References of one case, all the algorithm of gmres_restatement.gmres:
  * gmres_restatement.gmres itself, float64 (unchanged);
  * gmres_variant(..., dtype=numpy.longdouble): CSR products by np.add.reduceat, every sum in longdouble;
  * gmres_variant(..., chunk=128): float64 whose dot products and norms are partial sums over chunks of 128 elements
    folded afterwards, the device's shape of association.
d_case = the larger relative difference in x of the two float64 variants from the longdouble result, floored at 1e-15.

CASES: 358 iterate cases (328 with a longdouble reference, 30 at the three large sizes).  Every size of SIZES with restarts 5, 33, 64 (the three large sizes: 8 and 64), every restart of
RESTARTS with n = 129 and 1009, the channel systems with restarts 5, 33, 59, 64; per (system, restart) the step counts
r, r + 1, 2 r + 3 and, for r >= 5, r - 1 and r // 2.  Family, preconditioner and starting vector alternate over the pairs,
so half of the cases are preconditioned and half start from a non-zero x0.
THRESHOLD_CASES: 12 (restarts 30 and 64 on p' and on cd3 at n = 4097, three stop positions each);
BREAKDOWN_CASES: 6 (d in 2, 5, 17 at n = 129 and 1009)."""
import functools
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import gmres_restatement as R
from conftest import GOLDEN, splitmix64_uniform

LD = np.longdouble
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 1009, 4097)
LARGE_SIZES = (196_613, 524_289, 1_200_001)  # odd, one in each grid-stride band: (131 072, 262 144], (262 144, 1 048 576], above
RESTARTS = (1, 2, 4, 5, 16, 17, 31, 32, 33, 58, 59, 60, 61, 63, 64)
D_FAMILY_N = 4097  # a large case takes its d_case from the same family at this size

Case = namedtuple("Case", "family n restart steps precond x0")


def step_counts(r):
    s = [r, r + 1, 2 * r + 3]
    if r >= 5:
        s += [r - 1, r // 2]
    return s


def _pairs():
    out = []
    for n in SIZES:
        for r in (5, 33, 64):
            out.append((n, r))
    for r in RESTARTS:
        for n in (129, 1009):
            if (n, r) not in out:
                out.append((n, r))
    for n in LARGE_SIZES:
        for r in (8, 64):
            out.append((n, r))
    return out


def _cases():
    out = []
    for i, (n, r) in enumerate(_pairs()):
        family = ("cd1", "cd3")[i % 2]
        for k, steps in enumerate(step_counts(r)):
            out.append(Case(family, n, r, steps, (i // 2 + k) % 2, (i + k) % 2))
    for i, (name, r) in enumerate((nm, r) for nm in ("u", "p") for r in (5, 33, 59, 64)):
        for k, steps in enumerate(step_counts(r)):
            out.append(Case(name, 1008, r, steps, (i + k) % 2, (i // 2 + k) % 2))
    return out


CASES = _cases()
SMALL_CASES = [c for c in CASES if c.n not in LARGE_SIZES]
LARGE_CASES = [c for c in CASES if c.n in LARGE_SIZES]


def case_id(c):
    return "%s-n%d-r%d-k%d-pc%d-x%d" % c


# ------------------------------------------------------------------ matrices
def convdiff_1d(n):
    """-(0.5 + c) u_{i-1} + d_i u_i - (0.5 - c) u_{i+1}, c = 0.3, d_i in [1.02, 1.22): non-symmetric, weakly dominant"""
    d = 1.02 + 0.2 * np.abs(splitmix64_uniform(n, 11))
    a = sp.diags([np.full(max(n - 1, 0), -0.8), d, np.full(max(n - 1, 0), -0.2)], [-1, 0, 1], format="csr")
    a.sort_indices()
    return a


def convdiff_3d(n):
    """the leading n x n block of a 7-point stencil on the smallest cube-like grid with at least n points: diffusion -1 per
    face plus a skew convective part (+s towards the lower neighbour, -s towards the upper one, s = 0.45, 0.3, 0.15 along
    x, y, z, modulated by position); the diagonal of a row is the sum of its off-diagonal magnitudes plus [0.002, 0.032):
    weakly dominant in every row, those at the boundary and at the cut included"""
    nx = max(int(np.ceil(n ** (1.0 / 3.0))), 1)
    while nx ** 3 < n:
        nx += 1
    ny = nz = nx
    N = nx * ny * nz
    idx = np.arange(N).reshape(nz, ny, nx)
    mod = 1.0 + 0.25 * splitmix64_uniform(N, 23)
    rows, cols, vals = [], [], []
    for ax, s in ((2, 0.45), (1, 0.3), (0, 0.15)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        i, j = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()  # j is the upper neighbour of i
        rows += [i, j]
        cols += [j, i]
        vals += [-1.0 + s * mod[i], -1.0 - s * mod[i]]
    a = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))[:n, :n].tocsr()
    d = np.asarray(abs(a).sum(axis=1)).ravel() + 0.002 + 0.03 * np.abs(splitmix64_uniform(n, 29))
    a = (a + sp.diags(d)).tocsr()
    a.sort_indices()
    return a


@functools.lru_cache(maxsize=None)
def _channel():
    d = np.load(os.path.join(GOLDEN, "channel_flow.npz"))
    rp, col = d["row_ptr"], d["col"]
    n = len(rp) - 1
    return {"u": (sp.csr_matrix((d["a_uvw_frozen_it1"][0], col, rp), shape=(n, n)), d["b_uvw_frozen_it1"][0].copy()),
            "p": (sp.csr_matrix((d["a_p_frozen"], col, rp), shape=(n, n)), d["b_p_frozen"].copy())}


@functools.lru_cache(maxsize=8)
def system(family, n):
    """(a, b) as the device receives them (unscaled)"""
    if family in ("u", "p"):
        a, b = _channel()[family]
        assert n == a.shape[0]
        return a, b
    a = convdiff_1d(n) if family == "cd1" else convdiff_3d(n)
    return a, splitmix64_uniform(n, 101 + n % 89)


def start_vector(c):
    """the non-zero starting vector of a case (None: zero), of the size of the solution"""
    if not c.x0:
        return None
    a, b = system(c.family, c.n)
    xs = np.abs(b).max() / np.abs(a.diagonal()).max()
    return xs * splitmix64_uniform(c.n, 7 + c.restart)


def host_system(c):
    """the system the algorithm sees: Jacobi-scaled in float64 when the case is preconditioned"""
    a, b = system(c.family, c.n)
    return R.jacobi_scaled(a, b) if c.precond else (a, b)


# ------------------------------------------------------------------ references
def _matvec(a, dtype):
    if dtype is np.float64:
        return lambda v: a @ v
    data, indices, starts = a.data.astype(dtype), a.indices, a.indptr[:-1]
    assert np.all(np.diff(a.indptr) > 0), "reduceat needs a non-empty row everywhere"
    return lambda v: np.add.reduceat(data * v[indices], starts)


def _dots(chunk):
    """(V, w) -> V w and (w) -> w . w; chunk: partial sums over chunks of that many elements, folded afterwards"""
    if not chunk:
        return (lambda V, w: V @ w), (lambda w: w @ w)

    def many(V, w):
        n = len(w)
        pad = -n % chunk
        p = V * w
        if pad:
            p = np.concatenate([p, np.zeros((len(V), pad), p.dtype)], axis=1)
        return p.reshape(len(V), -1, chunk).sum(axis=2).sum(axis=1)

    return many, (lambda w: many(w[None, :], w)[0])


def gmres_variant(a, b, x, iteration_count, restart=30, threshold=0.0, dtype=np.float64, chunk=0):
    """gmres_restatement.gmres (finite inputs, guard irrelevant) in `dtype`, with the dot products of _dots(chunk).  x (of
    `dtype`) is updated in place.  Besides the restatement's statistics: ratios = [hn / |column| per step, per cycle]."""
    mv = _matvec(a, dtype)
    many, norm2 = _dots(chunk)
    b = b.astype(dtype)
    st = dict(steps=0, cycles=0, beta0=dtype(0), estimate=dtype(0), estimates=[], ratios=[])
    n = len(b)
    if iteration_count == 0 or n == 0:
        return st
    m = min(restart, iteration_count)
    left = iteration_count
    first = True
    while left > 0:
        k = min(m, left)
        left -= k
        r = b - mv(x)
        beta = np.sqrt(norm2(r))
        if first:
            st["beta0"] = beta
            first = False
        st["estimate"] = beta
        if beta == 0:
            return st
        st["cycles"] += 1
        V = np.zeros((m + 1, n), dtype)
        Hm = np.zeros((m + 1, m), dtype)
        cs, sn = np.zeros(m, dtype), np.zeros(m, dtype)
        g = np.zeros(m + 1, dtype)
        g[0] = beta
        V[0] = r / beta
        cols, stop = 0, False
        ests, ratios = [], []
        for j in range(k):
            w = mv(V[j])
            h1 = many(V[: j + 1], w)
            w = w - V[: j + 1].T @ h1
            h2 = many(V[: j + 1], w)
            w = w - V[: j + 1].T @ h2
            h = h1 + h2
            hn = np.sqrt(norm2(w))
            st["steps"] += 1
            cols = j + 1
            col = np.concatenate([h, [hn]])
            assert np.all(np.isfinite(col))
            cn = np.sqrt(col @ col)
            ratios.append(float(hn / cn) if cn > 0 else 0.0)
            happy = hn <= dtype(1e-14) * cn
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            d = np.hypot(col[j], col[j + 1])
            c, s = (dtype(1), dtype(0)) if d == 0 else (col[j] / d, col[j + 1] / d)
            cs[j], sn[j] = c, s
            col[j], col[j + 1] = d, 0
            Hm[: j + 2, j] = col
            g[j + 1] = -s * g[j]
            g[j] = c * g[j]
            est = abs(g[j + 1])
            st["estimate"] = est
            ests.append(est)
            if happy or (threshold > 0 and est <= dtype(threshold) * st["beta0"]):
                stop = True
                break
            V[j + 1] = w / hn
        st["estimates"].append(ests)
        st["ratios"].append(ratios)
        y = np.zeros(cols, dtype)
        for i in range(cols - 1, -1, -1):
            y[i] = (g[i] - Hm[i, i + 1: cols] @ y[i + 1:]) / Hm[i, i]
        x += V[:cols].T @ y
        if stop:
            return st
    return st


def _x0(x0, n, dtype):
    return np.zeros(n, dtype) if x0 is None else x0.astype(dtype)


def rel(x, ref):
    """|x - ref| / |ref| (|x - ref| itself where ref is zero), as a float"""
    d = np.sqrt(np.sum((x.astype(LD) - ref) ** 2))
    nr = np.sqrt(np.sum(ref.astype(LD) ** 2))
    return float(d / nr) if nr > 0 else float(d)


def references(a, b, x0, steps, restart, threshold=0.0):
    """the three references of one solve on the system the algorithm sees.  Returns dict(x_ld, x64, x_chunk, st_ld, st64,
    st_chunk, d_case)."""
    n = a.shape[0]
    x64 = _x0(x0, n, np.float64)
    st64 = R.gmres(a, b, x64, steps, restart=restart, threshold=threshold)
    xc = _x0(x0, n, np.float64)
    stc = gmres_variant(a, b, xc, steps, restart, threshold, np.float64, chunk=128)
    xl = _x0(x0, n, LD)
    stl = gmres_variant(a, b, xl, steps, restart, threshold, LD)
    return dict(x_ld=xl, x64=x64, x_chunk=xc, st_ld=stl, st64=st64, st_chunk=stc, d_case=max(rel(x64, xl), rel(xc, xl), 1e-15))


@functools.lru_cache(maxsize=None)
def case_references(c):
    """references() of a case of SMALL_CASES"""
    a, b = host_system(c)
    return references(a, b, start_vector(c), c.steps, c.restart)


def large_case_d(c):
    """d_case of a large case: that of the same family, restart, step count and settings at n = D_FAMILY_N"""
    return case_references(c._replace(n=D_FAMILY_N))["d_case"]


# ------------------------------------------------------------------ threshold stops inside a cycle
ThresholdCase = namedtuple("ThresholdCase", "family n restart precond where steps cycle step")
_WHERE = ("first-cycle", "later-cycle-first-step", "later-cycle-middle")


def _threshold_table():
    """p' converges fast (about 140 steps to 1e-10), the synthetic system slowly: the stops are placed in cycle 1 at step
    r // 3, in cycle 2 at step 1 and in cycle 2 at step r // 2, with 3 r steps allowed"""
    out = []
    for family, n, precond in (("p", 1008, 1), ("cd3", 4097, 0)):
        for r in (30, 64):
            for where, (cycle, step) in zip(_WHERE, ((1, r // 3), (2, 1), (2, r // 2))):
                out.append(ThresholdCase(family, n, r, precond, where, 3 * r, cycle, step))
    return out


THRESHOLD_CASES = _threshold_table()


@functools.lru_cache(maxsize=None)
def _free_run(family, n, restart, precond, steps):
    a, b = host_system(Case(family, n, restart, steps, precond, 0))
    return R.gmres(a, b, np.zeros(n), steps, restart=restart, threshold=0.0)


def threshold_of(t):
    """the threshold that stops case t at (cycle, step): the geometric mean of the float64 restatement's estimate there and
    the one before it (the last of the previous cycle for a first step), over beta0"""
    st = _free_run(t.family, t.n, t.restart, t.precond, t.steps)
    e = st["estimates"]
    here = e[t.cycle - 1][t.step - 1]
    before = e[t.cycle - 1][t.step - 2] if t.step > 1 else e[t.cycle - 2][-1]
    assert here < before
    return float(np.sqrt(here * before) / st["beta0"])


@functools.lru_cache(maxsize=None)
def threshold_references(t):
    a, b = host_system(Case(t.family, t.n, t.restart, t.steps, t.precond, 0))
    return references(a, b, None, t.steps, t.restart, threshold=threshold_of(t))


# ------------------------------------------------------------------ lucky breakdown at a step d > 1
BreakdownCase = namedtuple("BreakdownCase", "n d")
BREAKDOWN_CASES = [BreakdownCase(n, d) for n in (129, 1009) for d in (2, 5, 17)]
BREAKDOWN_RESTART = 30


def breakdown_system(t):
    """diagonal matrix with the d eigenvalues 1 + i / d in turn (row i: eigenvalue i mod d); the right-hand side is constant
    over the rows of one eigenvalue, so every vector of the iteration is, and so is every rounding error of an element-wise
    pass: the error of w stays in the d-dimensional Krylov space and the second orthogonalisation pass removes it.  Returns
    (a, b, exact solution)."""
    cls = np.arange(t.n) % t.d
    lam = 1.0 + cls / float(t.d)
    b = (0.5 + np.abs(splitmix64_uniform(t.d, 41 + t.d)))[cls] * np.where(cls % 2 == 0, 1.0, -1.0)
    a = sp.diags(lam, format="csr")
    return a, b, (b.astype(LD) / lam.astype(LD))


@functools.lru_cache(maxsize=None)
def breakdown_references(t):
    a, b, _ = breakdown_system(t)
    return references(a, b, None, BREAKDOWN_RESTART + 7, BREAKDOWN_RESTART)
