"""Case table and references of the default-order BiCGSTAB and Multigrid tests (tests/test_bicg_cpu.py, tests/test_gpu_bicg.py).

Systems (generated here, nothing committed; callers must not modify what they get):
  "fv"      conftest.fv_like_matrix(nx, ny, nz), b = A u7, starting vector 0.1 u8 (u: conftest.splitmix64_uniform by seed);
            (n, 1, 1) is a 1-D chain;
  "triple"  system k of three systems on the pattern of "fv": the first is fv_like_matrix itself, the others its values times
            1 + 1e-3 u, b = A_k u(7 + k), starting vector 0.1 u(20 + k) — test_gpu_triple.three_systems' default form;
  "user"    product_cases.solve_system(name) of the four product_cases.S_CASES.

References of one case, all of them the algorithm of tests/bicg_restatement.py: longdouble; float64 with numpy's pairwise
sums; float64 with partial sums over chunks of 512 elements folded afterwards, the device's shape.
d_case = max(rel(x64, x_ld), rel(x_chunk, x_ld), 1e-15), rel the relative L2 distance: the rounding scale of the case, taken
from the references alone.  tests/test_bicg_cpu.py holds it under 1e-10 for every case (a condition on the inputs) and shows
that a restatement which loses the last element or one chunk of every sum is more than 1e6 x 50 d_case away.
A fixed-count BiCGSTAB run of k iterations is a prefix of the run of k' > k iterations on the same inputs: the cases of one
system, preconditioner and starting vector share one run per variant (`solutions`).

SMALL_CASES   chains n = 2, 3, 63, 64, 65, 511, 512, 513, 1009, 4097 and the shapes (7,5,3), (13,11,5), (65,3,1), iterations
              1, 2, 3, 8 below n; preconditioner and starting vector alternate over the cases.  Under the Jacobi preconditioner
              3 iterations carry the scalings on the fly, 8 materialise them (ORC_MATERIALIZE_SCALING = 4).
BAND_CASES    one odd n just above each boundary of the launch geometry, 1 and 3 iterations.  With
                  vector_grid(n)  = min(ceil(ceil(n / 2) / 256), 2048)                      grid_for((n + 1) / 2), common.hpp
                  product_grid(n) = min(ceil(ceil(n / 64) / 4), 2048), rounded down to a multiple of 8 from 8 on   spmv_grid, spmv.hip
              and a fold (fold_partials_block, linalg_kernels.hpp) of 16 virtual wavefronts of 64 virtual threads, thread vt adding
              partials[vt] and partials[vt + 1024]:
                  n = 32 769      vector_grid 64 -> 65: the fold of the vector kernels' sums enters a second virtual wavefront
                  n = 263 937     product_grid 1024 -> 1032: the fold of a product's sums takes a second element per virtual thread.
                                  (NOT 262 145: spmv_grid rounds 1025 ... 1031 workgroups down to 1024, the next grid is 1032, first
                                  reached with 4 125 slices = 263 937 rows)
                  n = 524 289     product_grid clamped at 2048 (8 193 slices want 2 049), and vector_grid 1024 -> 1025: the fold of the
                                  vector kernels' sums takes a second element per virtual thread
                  n = 1 048 579   vector_grid clamped at 2048 AND a second grid-stride pass: the clamp itself is reached at
                                  1 048 577, but there the 2048 x 256 lanes hold exactly the n >> 1 = 524 288 pairs and only the
                                  single-element tail is left over; 1 048 579 has one pair in the second pass, plus the tail
                  129 x 129 x 127 = 2 113 407   two full passes of the vector kernels (2 x 524 288 pairs), 8 127 pairs in a third,
                                  plus the tail
              tests/test_bicg_cpu.py recomputes each of these from the two formulas and pins their constants to the sources.
USER_CASES    the four product_cases.S_CASES, both preconditioners, 3 and 8 iterations, starting vector of solve_system.  Three of
              the eight runs do not stand 8 iterations, and their counts are lowered (USER_COUNTS) instead of any bound:
                  S2 without preconditioner   BiCGSTAB with r_hat_0 = 1 loses the iterate on these 130 unknowns: the float64
                                              restatements are 1.2e-11 from longdouble after 4 iterations, 2e-8 after 5, 1e-3 after 6
                                              (cap 1e-10), and at 4 a lost last element moves x by 6.11e-4, a hair under 1e6 x 50
                                              d_case = 6.14e-4: counts 2 and 3 (no scaling to materialise without a preconditioner);
                  S2 with Jacobi              converged at 8 (|b - A x| = 1.4e-5 |b|): a lost last element moves x by 6.7e-7 < 1e6 x
                                              50 d_case = 1.05e-6; at 6 by 8.2e-5: counts 3 and 6 (6 still materialises);
                  S4 with Jacobi              the same: 9.4e-9 < 5e-8 at 8, 7.1e-7 at 6: counts 3 and 6.
MG_CASES      the Multigrid arm on (20,17,9) and (64,40,12), Jacobi, 3 and 5 smoothing iterations; R and (R a) R^T of every level come
              from the oracle as float64 data (`mg_references` takes the oracle module).
TRIPLE_CASES  what the lock-step tests of test_gpu_bicg.py need: the three "triple" systems on the chain of 1 048 577 rows with both
              preconditioners, and system 0 of (13,11,5) and of that chain without (the per-system guard scenario), 3 iterations.
              At 1 048 577 rows the pair loops of bicg_{s,xr,p}3_k are through after one pass (see 1 048 579 above), so the three
              systems are solved on the chain of 1 048 579 rows as well, without preconditioner.
GUARD_CASES   n = 1 with every iteration count, and the chains n = 2, 3 with n iterations: BiCGSTAB on n unknowns is through after n
              iterations, so the last half step meets s = 0 (the guard's x = h branch) or rounding noise.  Held to the direct
              solution, not to an iterate."""
import functools
from collections import namedtuple

import numpy as np

import bicg_restatement as R
import product_cases as PC
from conftest import fv_like_matrix, splitmix64_uniform

LD = np.longdouble
CHAINS = (2, 3, 63, 64, 65, 511, 512, 513, 1009, 4097)
SHAPES = ((7, 5, 3), (13, 11, 5), (65, 3, 1))
ITERATIONS = (1, 2, 3, 8)
BAND_SHAPES = ((32_769, 1, 1), (263_937, 1, 1), (524_289, 1, 1), (1_048_579, 1, 1), (129, 129, 127))
BAND_ITERATIONS = (1, 3)
LOCKSTEP_SHAPE = (1_048_577, 1, 1)
LOCKSTEP_RUNS = ((LOCKSTEP_SHAPE, 0), (LOCKSTEP_SHAPE, 1), ((1_048_579, 1, 1), 0))  # (shape, preconditioner)
GUARD3_SHAPES = ((13, 11, 5), LOCKSTEP_SHAPE)
MG_SHAPES = ((20, 17, 9), (64, 40, 12))
MG_ITERATIONS = (3, 5)
BOUND = 50  # the project's margin over the spread of the float64 associations (tests/test_gpu_cg.py)

# kind: "fv" | "triple" | "user"; key: a shape, (shape, k) or a name of product_cases.S_CASES
Case = namedtuple("Case", "kind key iterations precond x0")


def _small():
    out = []
    for j, shape in enumerate([(n, 1, 1) for n in CHAINS] + list(SHAPES)):
        n = shape[0] * shape[1] * shape[2]
        for q, k in enumerate(ITERATIONS):
            if k < n:  # every iteration count meets both preconditioners and both starting vectors over the sizes
                out.append(Case("fv", shape, k, (j + q) % 2, (j // 2 + q // 2) % 2))
    return out


SMALL_CASES = _small()
BAND_CASES = [Case("fv", shape, k, i % 2, (i // 2) % 2) for i, shape in enumerate(BAND_SHAPES) for k in BAND_ITERATIONS]
# (name, preconditioner) -> iteration counts where 3 and 8 do not serve (docstring)
USER_COUNTS = {("S2_long_ragged", 0): (2, 3), ("S2_long_ragged", 1): (3, 6), ("S4_far_short_ragged", 1): (3, 6)}
USER_CASES = [Case("user", c.name, k, pre, 1) for c in PC.S_CASES for pre in (0, 1)
              for k in USER_COUNTS.get((c.name, pre), (PC.BICG_ON_THE_FLY, PC.BICG_MATERIALISED))]
MG_CASES = [Case("fv", shape, k, 1, 1) for shape in MG_SHAPES for k in MG_ITERATIONS]
TRIPLE_CASES = ([Case("triple", (shape, s), 3, pre, 1) for shape, pre in LOCKSTEP_RUNS for s in range(3)]
                + [Case("triple", (GUARD3_SHAPES[0], 0), 3, 0, 1)])
ITERATE_CASES = SMALL_CASES + BAND_CASES + USER_CASES + TRIPLE_CASES
GUARD_CASES = [Case("fv", (1, 1, 1), k, i % 2, (i // 2) % 2) for i, k in enumerate(ITERATIONS)] + [
    Case("fv", (2, 1, 1), 2, 1, 0), Case("fv", (3, 1, 1), 3, 0, 1)]


def case_id(c):
    key = c.key if c.kind == "user" else "x".join(map(str, c.key if c.kind == "fv" else c.key[0])) + ("" if c.kind == "fv" else "-s%d" % c.key[1])
    return "%s-%s-k%d-pc%d-x%d" % (c.kind, key, c.iterations, c.precond, c.x0)


# ------------------------------------------------------------------ launch geometry (docstring)
K_BLOCK, K_MAX_GRID, SLICE_ROWS, SLICES_PER_WG = 256, 2048, 64, 4


def vector_grid(n):
    """grid_for((n + 1) / 2): the workgroups of bicg_{s,xr,p}_k and bicg_{s,xr,p}3_k, two elements per lane"""
    return max(1, min(((n + 1) // 2 + K_BLOCK - 1) // K_BLOCK, K_MAX_GRID))


def product_grid(n):
    """spmv_grid(ceil(n / 64)): the workgroups of a product on a user matrix, which is the number of its partial sums"""
    g = min(((n + SLICE_ROWS - 1) // SLICE_ROWS + SLICES_PER_WG - 1) // SLICES_PER_WG, K_MAX_GRID)
    if g >= 8:
        g = g // 8 * 8
    return max(1, g)


def vector_passes(n):
    """(full or partial passes of the two-element loop over the n >> 1 pairs, is there a single-element tail)"""
    lanes = vector_grid(n) * K_BLOCK
    return ((n >> 1) + lanes - 1) // lanes, bool(n & 1)


# ------------------------------------------------------------------ systems
@functools.lru_cache(maxsize=3)
def _fv(shape):
    return fv_like_matrix(*shape)


@functools.lru_cache(maxsize=4)
def system(kind, key):
    """(a, b, starting vector) as the device receives them"""
    if kind == "user":
        return PC.solve_system(key)
    if kind == "fv":
        a = _fv(key)
        n = a.shape[0]
        return a, a @ splitmix64_uniform(n, 7), 0.1 * splitmix64_uniform(n, 8)
    shape, k = key
    a0 = _fv(shape)
    n = a0.shape[0]
    a = a0
    if k:
        a = a0.copy()
        a.data = a0.data * (1.0 + 1e-3 * splitmix64_uniform(len(a0.data), 1 + 100 * k))
    return a, a @ splitmix64_uniform(n, 7 + k), 0.1 * splitmix64_uniform(n, 20 + k)


def three_systems(shape):
    """(mats, bs, xs) of the three "triple" systems of a shape, as fresh lists of copies"""
    ss = [system("triple", (shape, k)) for k in range(3)]
    return [s[0].copy() for s in ss], [s[1].copy() for s in ss], [s[2].copy() for s in ss]


def start(c, dtype=np.float64):
    a, _, x0 = system(c.kind, c.key)
    return x0.astype(dtype) if c.x0 else np.zeros(a.shape[0], dtype)


def rel(x, ref):
    """|x - ref| / |ref| (|x - ref| itself where ref is zero), as a float"""
    d = np.sqrt(np.sum((x.astype(LD) - ref) ** 2))
    nr = np.sqrt(np.sum(ref.astype(LD) ** 2))
    return float(d / nr) if nr > 0 else float(d)


# ------------------------------------------------------------------ references
def _counts(kind, key, precond, x0):
    """the iteration counts the table holds for one system, preconditioner and starting vector"""
    return tuple(sorted({c.iterations for c in ITERATE_CASES if (c.kind, c.key, c.precond, c.x0) == (kind, key, precond, x0)}))


def run(c, dtype, sums, keep=None):
    """{count: x} of one restatement run of the case's system up to max(keep) iterations (keep: default the case's own count)"""
    a, b, _ = system(c.kind, c.key)
    keep = keep or (c.iterations,)
    x = start(c, dtype)
    return R.solve(a, b, x, max(keep), c.precond, dtype, sums, keep)


@functools.lru_cache(maxsize=None)
def solutions(kind, key, precond, x0):
    """{count: (x_ld, d_case)} for every iteration count of the table on this system"""
    keep = _counts(kind, key, precond, x0)
    c = Case(kind, key, max(keep), precond, x0)
    ld = run(c, LD, R.Sums("ld"), keep)
    f64 = run(c, np.float64, R.Sums("pairwise"), keep)
    chunk = run(c, np.float64, R.Sums("chunk"), keep)
    out = {}
    for k in keep:
        ld[k].setflags(write=False)
        out[k] = (ld[k], max(rel(f64[k], ld[k]), rel(chunk[k], ld[k]), 1e-15))
    return out


def references(c):
    """(x_ld, d_case) of an iterate case"""
    return solutions(c.kind, c.key, c.precond, c.x0)[c.iterations]


def mg_system(shape):
    return system("fv", shape)


@functools.lru_cache(maxsize=None)
def _mg_levels(oracle, shape, precond):
    a, _, _ = mg_system(shape)
    return R.hierarchy(oracle, R.scaled_operator(a, precond))


def mg_run(oracle, c, dtype, sums):
    a, b, _ = mg_system(c.key)
    x = start(c, dtype)
    R.multigrid(a, b, x, c.iterations, c.precond, _mg_levels(oracle, c.key, c.precond), dtype, sums)
    return x


@functools.lru_cache(maxsize=None)
def mg_references(oracle, c):
    """(x_ld, d_case) of a Multigrid case; oracle: the oracle.pyoracle module, built"""
    xl = mg_run(oracle, c, LD, R.Sums("ld"))
    x64 = mg_run(oracle, c, np.float64, R.Sums("pairwise"))
    xc = mg_run(oracle, c, np.float64, R.Sums("chunk"))
    xl.setflags(write=False)
    return xl, max(rel(x64, xl), rel(xc, xl), 1e-15)
