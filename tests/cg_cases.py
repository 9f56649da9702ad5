"""Case table and references of the CG tests (tests/test_cg_cpu.py, tests/test_gpu_cg.py).

Matrices (generated here, nothing committed), all symmetric in every bit: "lap1" an SPD tridiagonal with a varying diagonal,
"lap3" the leading n x n block of a symmetric 7-point stencil whose face coefficients vary by position, with a weakly
dominant diagonal, and "p", the pressure-correction system of golden/channel_flow.npz (n = 1008).  Right-hand sides and
starting vectors come from conftest.splitmix64_uniform.

References of one case, all the algorithm of cg_restatement.cg: float64, longdouble (CSR products by np.add.reduceat), and
float64 whose dot products are partial sums over chunks of 128 elements folded afterwards, the device's shape of association.
d_case = the larger relative difference in x of the two float64 variants from the longdouble result, floored at 1e-15.
d_res = the same for the reported final residual norm: the larger difference of the two float64 variants' |r| from the
longdouble one.  The device's |r| is held to 1e-10 relative.  The exception is a case whose float64 references do not
determine |r| to a tenth of that themselves (res_at_rounding: d_res > 1e-11 |r|): CG through after k = n iterations on n = 1, 2, 3
(|r| is the rounding of r - alpha q, 1e-20 beta0 in longdouble) and lap3 on 64 to 256 unknowns at 50 iterations, where CG is
nearly through and the float64 recurrences differ among themselves by up to the residual's own size.  RESIDUAL_AT_ROUNDING
names them; tests/test_cg_cpu.py holds the set to exactly that list, and there the device's |r| is held to 1e-10 relative plus
50 max(d_res, 1e-15 beta0): 1e-15 beta0 is the rounding of the last update of r (half an ulp of |alpha q| <= beta0 per entry,
over k <= 3 iterations where the float64 variants happen to end at exactly 0).

CASES: every size of SIZES with every iteration count of ITERATIONS that does not exceed it (CG on n unknowns is through after
n iterations; what follows works on rounding noise and has no reference iterate), the channel system with all five, and the two
large sizes with 3 and 50 iterations.  Family, preconditioner and starting vector alternate over the cases.
PAST_END_CASES: the remaining combinations, n = 1, 2, 3 with more iterations than unknowns, as set_pressure_solver(CG, JACOBI, 50, 0)
meets them on a tiny mesh: held to the direct solution, a clean status and event 0 or 1 (p.q of a vanished direction is 0).
LARGE_SIZES: the vector kernels of cg.hip (cg_start_k, cg_update_k, cg_direction_k) take two elements per lane and their grid
is clamped at 2048 workgroups of 256, so they grid-stride above 1 048 576 rows; the product's grid (one slice of 64 rows per
wave, four per workgroup) and cg_diag_inverse_k (one row per lane) are clamped above 524 288 rows.  One odd size above each.
THRESHOLD_CASES: on "p" and on "lap3" at n = 4097, 50 iterations allowed, stops at the first, a middle and the last one.
EVENT_CASES: indefinite diagonal systems at n = 2, 129, 1009 and at the larger of LARGE_SIZES (workgroups of the launch that raises
the stop flag still start while it is raised) whose p.q turns negative at a known iteration; b = 0; a starting vector that
solves the system to rounding."""
import functools
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import cg_restatement as R
from conftest import GOLDEN, splitmix64_uniform

LD = np.longdouble
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1009, 4097)
LARGE_SIZES = (600_001, 1_200_001)
ITERATIONS = (1, 2, 3, 7, 50)
D_FAMILY_N = 4097  # a large case takes its d_case from the same family at this size

Case = namedtuple("Case", "family n iterations precond x0")


def _cases():
    out = []
    i = 0
    for n in SIZES:
        for k in ITERATIONS:
            if k <= n:
                out.append(Case(("lap1", "lap3")[i % 2], n, k, (i // 2) % 2, (i // 4) % 2))
                i += 1
    for k in ITERATIONS:
        out.append(Case("p", 1008, k, i % 2, (i // 2) % 2))
        i += 1
    for n in LARGE_SIZES:
        for k in (3, 50):
            out.append(Case(("lap1", "lap3")[i % 2], n, k, (i // 2) % 2, (i // 4) % 2))
            i += 1
    return out


CASES = _cases()
PAST_END_CASES = [Case(("lap1", "lap3")[i % 2], n, k, (i // 2) % 2, (i // 4) % 2)
                  for i, (n, k) in enumerate((n, k) for n in (1, 2, 3) for k in ITERATIONS if k > n)]
# (docstring, d_res) the cases whose float64 references leave the final |r| undetermined at 1e-11 relative
RESIDUAL_AT_ROUNDING = frozenset(("lap1-n1-k1-pc0-x0", "lap1-n2-k2-pc1-x0", "lap3-n3-k3-pc0-x1", "lap3-n64-k50-pc1-x1", "lap3-n127-k50-pc0-x0",
                                  "lap3-n129-k50-pc1-x0", "lap3-n256-k50-pc0-x1"))
SMALL_CASES = [c for c in CASES if c.n not in LARGE_SIZES]
LARGE_CASES = [c for c in CASES if c.n in LARGE_SIZES]


def case_id(c):
    return "%s-n%d-k%d-pc%d-x%d" % c


# ------------------------------------------------------------------ matrices
def lap1(n):
    """-u_{i-1} + d_i u_i - u_{i+1}, d_i in [2.1, 2.6): symmetric, strictly dominant"""
    d = 2.1 + 0.5 * np.abs(splitmix64_uniform(n, 11))
    off = np.full(max(n - 1, 0), -1.0)
    a = sp.diags([off, d, off], [-1, 0, 1], format="csr")
    a.sort_indices()
    return a


def lap3(n):
    """the leading n x n block of a 7-point stencil on the smallest cube with at least n points: the coefficient of a face is
    -(1 + 0.5 u) with u in [0, 1) by the position of the face, the same in both rows it joins; the diagonal of a row is the
    sum of its off-diagonal magnitudes plus [0.1, 0.3), 1 to 4 % of it: weakly dominant in every row, those at the cut included
    (condition number 76 at n = 4097).  With [0.02, 0.05) the cases n = 128, 129 at 50 iterations without a preconditioner broke
    the d_case bound of tests/test_cg_cpu.py (1.4e-10): CG on so few unknowns is then in its superlinear phase, where rounding
    delays convergence and the iterates of two precisions differ by the size of the current error."""
    nx = max(int(np.ceil(n ** (1.0 / 3.0))), 1)
    while nx ** 3 < n:
        nx += 1
    N = nx ** 3
    idx = np.arange(N).reshape(nx, nx, nx)
    rows, cols, vals = [], [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax] = slice(0, -1)
        hi[ax] = slice(1, None)
        i, j = idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()
        c = -(1.0 + 0.5 * np.abs(splitmix64_uniform(N, 23 + ax)[i]))
        rows += [i, j]
        cols += [j, i]
        vals += [c, c]
    if rows and len(np.concatenate(rows)):
        a = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))[:n, :n].tocsr()
    else:
        a = sp.csr_matrix((n, n))
    d = np.asarray(abs(a).sum(axis=1)).ravel() + 0.1 + 0.2 * np.abs(splitmix64_uniform(n, 29))
    a = (a + sp.diags(d)).tocsr()
    a.sort_indices()
    return a


@functools.lru_cache(maxsize=None)
def _channel_p():
    d = np.load(os.path.join(GOLDEN, "channel_flow.npz"))
    rp, col = d["row_ptr"], d["col"]
    n = len(rp) - 1
    a = sp.csr_matrix((d["a_p_frozen"], col, rp), shape=(n, n))
    a.sort_indices()
    return a, d["b_p_frozen"].copy()


@functools.lru_cache(maxsize=8)
def system(family, n):
    """(a, b) as the device receives them"""
    if family == "p":
        a, b = _channel_p()
        assert n == a.shape[0]
        return a, b
    a = lap1(n) if family == "lap1" else lap3(n)
    return a, splitmix64_uniform(n, 101 + n % 89)


def start_vector(c):
    """the non-zero starting vector of a case (None: zero)"""
    if not c.x0:
        return None
    a, b = system(c.family, c.n)
    xs = np.abs(b).max() / np.abs(a.diagonal()).max()
    return xs * splitmix64_uniform(c.n, 7 + c.iterations)


def is_bit_symmetric(a):
    t = a.T.tocsr()
    t.sort_indices()
    return np.array_equal(a.indptr, t.indptr) and np.array_equal(a.indices, t.indices) and np.array_equal(a.data, t.data)


# ------------------------------------------------------------------ references
def _x0(x0, n, dtype):
    return np.zeros(n, dtype) if x0 is None else x0.astype(dtype)


def rel(x, ref):
    """|x - ref| / |ref| (|x - ref| itself where ref is zero), as a float"""
    d = np.sqrt(np.sum((x.astype(LD) - ref) ** 2))
    nr = np.sqrt(np.sum(ref.astype(LD) ** 2))
    return float(d / nr) if nr > 0 else float(d)


def references(a, b, x0, iterations, precond, threshold=0.0):
    """the three references of one solve.  Returns dict(x_ld, x64, x_chunk, st_ld, st64, st_chunk, d_case, d_res, res_at_rounding)."""
    n = a.shape[0]
    x64 = _x0(x0, n, np.float64)
    st64 = R.cg(a, b, x64, iterations, precond, threshold)
    xc = _x0(x0, n, np.float64)
    stc = R.cg(a, b, xc, iterations, precond, threshold, chunk=128)
    xl = _x0(x0, n, LD)
    stl = R.cg(a, b, xl, iterations, precond, threshold, dtype=LD)
    d_res = max(abs(float(st64["residual"] - stl["residual"])), abs(float(stc["residual"] - stl["residual"])))
    return dict(x_ld=xl, x64=x64, x_chunk=xc, st_ld=stl, st64=st64, st_chunk=stc, d_case=max(rel(x64, xl), rel(xc, xl), 1e-15), d_res=d_res,
                res_at_rounding=d_res > 1e-11 * float(stl["residual"]))


@functools.lru_cache(maxsize=None)
def case_references(c):
    """references() of a case of SMALL_CASES"""
    a, b = system(c.family, c.n)
    return references(a, b, start_vector(c), c.iterations, c.precond)


def large_case_d(c):
    """d_case of a large case: that of the same family, iteration count and settings at n = D_FAMILY_N"""
    return case_references(c._replace(n=D_FAMILY_N))["d_case"]


# ------------------------------------------------------------------ threshold stops
ThresholdCase = namedtuple("ThresholdCase", "family n precond where iterations target")
THRESHOLD_ITERATIONS = 50
THRESHOLD_CASES = [ThresholdCase(family, n, precond, where, THRESHOLD_ITERATIONS, target)
                   for family, n, precond in (("p", 1008, 1), ("lap3", 4097, 0))
                   for where, target in (("first", 1), ("middle", 25), ("last", 50))]


@functools.lru_cache(maxsize=None)
def _free_run(family, n, precond, iterations):
    a, b = system(family, n)
    return R.cg(a, b, np.zeros(n), iterations, precond)


def threshold_of(t):
    """(threshold, iteration): CG's residual norm is not monotone, so the stop is placed at the iteration closest to the
    target (at or below it) at which the float64 restatement's |r| is below every earlier one by at least a tenth; the
    threshold is the geometric mean of that |r| and the smallest earlier one (beta0 included), over beta0"""
    st = _free_run(t.family, t.n, t.precond, t.iterations)
    res = np.concatenate([[st["beta0"]], np.asarray(st["residuals"], np.float64)])
    for k in range(t.target, 0, -1):
        before = res[:k].min()
        if res[k] <= 0.9 * before:
            return float(np.sqrt(res[k] * before) / res[0]), k
    raise AssertionError("no strict minimum of |r| at or below iteration %d" % t.target)


@functools.lru_cache(maxsize=None)
def threshold_references(t):
    a, b = system(t.family, t.n)
    return references(a, b, None, t.iterations, t.precond, threshold=threshold_of(t)[0])


# ------------------------------------------------------------------ events
EventCase = namedtuple("EventCase", "name n")
EVENT_CASES = [EventCase("indefinite", 2), EventCase("indefinite", 129), EventCase("indefinite", 1009), EventCase("indefinite", LARGE_SIZES[-1]),
               EventCase("zero_rhs", 129), EventCase("solved_start", 1009)]
EVENT_ITERATIONS = 7


@functools.lru_cache(maxsize=None)
def event_system(t):
    """(a, b, x0, precond).
    indefinite: a diagonal matrix with the eigenvalues 1, 2, 3 and -4 in turn (n = 2: 1 and -4) and a right-hand side that is
    constant over the rows of one eigenvalue and small on the negative one: every vector of the iteration is constant per
    class, p.q = sum lambda p^2 starts positive (n = 2: negative at once) and turns negative once the positive part of the
    residual is reduced.
    zero_rhs: lap1, b = 0, x0 = 0.  solved_start: lap3 started from its float64 direct solution: r0 is rounding noise."""
    if t.name == "indefinite":
        lam_of = np.array([1.0, -4.0]) if t.n == 2 else np.array([1.0, 2.0, 3.0, -4.0])
        w_of = np.array([1.0, 2.0]) if t.n == 2 else np.array([1.0, -0.75, 0.5, 0.05])
        cls = np.arange(t.n) % len(lam_of)
        return sp.diags(lam_of[cls], format="csr"), w_of[cls], None, 0
    if t.name == "zero_rhs":
        return lap1(t.n), np.zeros(t.n), None, 1
    import scipy.sparse.linalg as spla
    a, b = system("lap3", t.n)
    return a, b, spla.spsolve(a.tocsc(), b), 1


@functools.lru_cache(maxsize=None)
def event_references(t):
    a, b, x0, precond = event_system(t)
    return references(a, b, x0, EVENT_ITERATIONS, precond)
