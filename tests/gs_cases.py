"""Case table of the Gauss-Seidel tests (tests/test_gs_cases_cpu.py, tests/test_gpu_gs_cases.py).

The Gauss-Seidel arms of orc_amd/csrc/gs_*.hip (the multicolour sweep, the GS-preconditioned BiCGSTAB in row and in slot space,
the smoother of MULTIGRID_GS) colour the pattern on the device, sort it by colour into 64-row slices and sweep slice ranges.
The matrices here sit where that can go wrong on a USER matrix: patterns that are not structurally symmetric (a row with an
in-neighbour it does not store), colours of fewer than 64 rows, exactly 64 colours and one more, more than 1 024 row blocks and
colour-sorted slices (the carry branches of the two one-workgroup scans), rows of 1 ... 130 entries, an empty row, a last slice
with one live row.  Every claim of the table is re-derived from the matrix by the CPU test, without the library.

Nothing is committed: the builders are deterministic and cached — callers must not modify what they return.  No GPU, no oracle.
Values come from product_cases._finish(..., solve=True): a full diagonal, negative off-diagonals, strict diagonal dominance.

Where a case differs from a bare reading of its description:
  * G5: the tridiagonal tail behind the dense block takes three colours under the hash priorities (a chain needs two only when
    the priorities alternate), so colours 3 ... 63 hold one row each, not 2 ... 63; what matters stands: exactly 64 colours,
    none with 64 rows, so 64 colour-sorted slices hold the 101 rows and every slice is partly padding.
  * G9: row 70 of G3 lies in G1's diagonal-only slice and no other row stores column 70, so "its column kept in other rows" holds
    of no entry: emptying the row removes its diagonal and nothing else refers to it.  (Emptying a row that others do refer to
    would make the pattern non-symmetric; G9 is one of the cases whose colouring is pinned to the symmetric rule.)  The claim
    the CPU test derives is therefore: row 70 is the only empty row and every other row is G3's.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import product_cases as PC
from conftest import fv_like_matrix, splitmix64_uniform  # noqa: F401  (fv_like_matrix: re-exported for the tests)

MULTICOLOR_GS, BICGSTAB_GS, MULTIGRID_GS = 16, 17, 18
PRE_NONE, PRE_JACOBI = 0, 1
ERR_BAD_ARGUMENT = 10

# claims: structural facts the CPU test re-derives (test_gs_cases_cpu.py); seed: b = splitmix64_uniform(n, seed), x0 = (n, seed + 1)
Case = namedtuple("Case", "name build n symmetric seed claims")


def _rows_of(a):
    a = a.tocsr()
    return [a.indices[a.indptr[r]:a.indptr[r + 1]].astype(np.int64) for r in range(a.shape[0])]


def _pattern_union_transpose(a):
    p = sp.csr_matrix((np.ones(a.nnz), a.indices, a.indptr), shape=a.shape)
    p = (p + p.T).tocsr()
    p.sort_indices()
    return p


# ---------------------------------------------------------------- G3 / G9: G1's pattern made symmetric
@functools.lru_cache(maxsize=None)
def short_ragged_sym():
    p = _pattern_union_transpose(PC.short_ragged(True))
    return PC._finish(p.shape[0], _rows_of(p), 111, True)


EMPTY_ROW = 70


@functools.lru_cache(maxsize=None)
def short_ragged_sym_empty_row():
    """G3 with row 70 emptied (diagonal included); every other row is G3's"""
    a = short_ragged_sym().tolil(copy=True)
    a.rows[EMPTY_ROW], a.data[EMPTY_ROW] = [], []
    a = a.tocsr()
    a.sort_indices()
    return a


# ---------------------------------------------------------------- G4
@functools.lru_cache(maxsize=None)
def bidiagonal(n=200):
    return PC._finish(n, [np.array([r - 1, r] if r else [0], dtype=np.int64) for r in range(n)], 404, True)


# ---------------------------------------------------------------- G5 / G6
@functools.lru_cache(maxsize=None)
def clique_with_tail(m, tail=37):
    """rows 0 ... m-1 hold each other's columns; rows m ... m+tail-1 continue as a tridiagonal chain from row m-1"""
    n = m + tail
    rows = []
    for r in range(n):
        if r < m - 1:
            rows.append(np.arange(m, dtype=np.int64))
        elif r == m - 1:
            rows.append(np.arange(m + 1, dtype=np.int64))
        else:
            rows.append(np.array([c for c in (r - 1, r, r + 1) if c < n], dtype=np.int64))
    return PC._finish(n, rows, 505 + m, True)


# ---------------------------------------------------------------- G7
N_BAND = 65_601  # 1 025 * 64 + 1: 1 026 row blocks, the last with one live row
BAND_OFFSETS = (-257, -1, 0, 1, 257)


@functools.lru_cache(maxsize=None)
def far_band():
    n = N_BAND
    r = np.arange(n, dtype=np.int64)
    cols = np.stack([r + o for o in BAND_OFFSETS], axis=1)
    keep = (cols >= 0) & (cols < n)
    rows = [c[k] for c, k in zip(cols, keep)]
    return PC._finish(n, rows, 707, True)


# ---------------------------------------------------------------- G8
@functools.lru_cache(maxsize=None)
def tridiagonal(n):
    return PC._finish(n, [np.array([c for c in (r - 1, r, r + 1) if 0 <= c < n], dtype=np.int64) for r in range(n)], 800 + n, True)


TRIDIAGONAL_N = (1, 63, 64, 65)

G_CASES = (
    Case("G1_short_ragged", functools.partial(PC.short_ragged, True), 193, False, 11,
         dict(row_lens=(1, 13), diagonal_only_slice=1, last_slice_live=1)),
    Case("G2_long_ragged", functools.partial(PC.long_ragged, True), 130, False, 21,
         dict(full_rows=(9, 94), full_row_len=130, chunks_plus=(16, 2))),
    Case("G3_short_ragged_sym", short_ragged_sym, 193, True, 31, dict(ragged=True, last_slice_live=1)),
    Case("G4_bidiagonal", bidiagonal, 200, False, 41, dict(unseen_in_neighbour_rows=199)),
    Case("G5_clique64", functools.partial(clique_with_tail, 64), 101, True, 51, dict(clique=64, colors=64, single_row_colors=(3, 63), slices=64)),
    Case("G6_clique65", functools.partial(clique_with_tail, 65), 102, True, 61, dict(clique=65, colors=None)),
    Case("G7_far_band", far_band, N_BAND, True, 71, dict(row_blocks=1026, min_slices=1026, last_block_live=1)),
) + tuple(
    Case("G8_tridiagonal_%d" % n, functools.partial(tridiagonal, n), n, True, 80 + n, dict(tridiagonal=True))
    for n in TRIDIAGONAL_N
) + (
    Case("G9_empty_row", short_ragged_sym_empty_row, 193, True, 91, dict(empty_row=EMPTY_ROW)),
)

CASES = {c.name: c for c in G_CASES}
ERROR_CASE = "G6_clique65"
EMPTY_ROW_CASE = "G9_empty_row"
SOLVABLE = [c.name for c in G_CASES if c.name not in (ERROR_CASE,)]           # everything that can be coloured
SYMMETRIC = [c.name for c in G_CASES if c.symmetric and c.name != ERROR_CASE]  # today's colouring is pinned on these
NOT_SYMMETRIC = [c.name for c in G_CASES if not c.symmetric]
# both forms of the preconditioned BiCGSTAB, 3 iterations
BICG_CASES = ["G1_short_ragged", "G2_long_ragged", "G3_short_ragged_sym", "G4_bidiagonal", "G5_clique64", "G7_far_band", "G8_tridiagonal_65"]
BICG_ITERATIONS = 3
# case -> iterations after which the restatement (and then the device) has solved the system to 1e-8; a case that needs more gets
# its count raised HERE (test_gs_cases_cpu.py::test_reference_solves_the_convergence_cases is the condition)
CONVERGENCE_COUNTS = {"G1_short_ragged": 12, "G2_long_ragged": 12, "G3_short_ragged_sym": 12, "G5_clique64": 12}
MULTIGRID_CASES = ["G3_short_ragged_sym", "G4_bidiagonal"]
SWEEPS = 3
OMEGAS = (0.8, 1.0)


def preconditioners(name):
    """the Jacobi scaling divides by the diagonal: not on the case with an empty row"""
    return (PRE_NONE,) if name == EMPTY_ROW_CASE else (PRE_NONE, PRE_JACOBI)


def system(name):
    """(a, b, x0) of a case: b = splitmix64_uniform(n, s), x0 = splitmix64_uniform(n, s + 1), as product_cases seeds its vectors"""
    c = CASES[name]
    return c.build(), splitmix64_uniform(c.n, c.seed), splitmix64_uniform(c.n, c.seed + 1)


def convergence_system(name):
    """(a, b, xs) with b = a xs: the solves that start from zero and must find xs"""
    c = CASES[name]
    a = c.build()
    xs = splitmix64_uniform(c.n, c.seed + 2)
    return a, a @ xs, xs


def jacobi_scale(a):
    return 1.0 / a.diagonal()


def is_structurally_symmetric(a):
    p = sp.csr_matrix((np.ones(a.nnz), a.indices, a.indptr), shape=a.shape)
    return (p != p.T).nnz == 0
