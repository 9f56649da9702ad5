"""Case table of the product-dispatch tests (tests/test_product_cases_cpu.py, tests/test_gpu_product_cases.py).

launch_spmv (orc_amd/csrc/spmv.hip) picks a kernel by the matrix: the raggedness class of its SELL-64 image
(padded > 1.08 nnz ? (padded < 24 n ? 2 : 1) : 0), whether the all-or-nothing narrow column image exists (every slice and
depth spans <= 65 535 columns), and by the call (scalings carried or materialised, non-temporal policy).  The matrices here sit
on those thresholds and on the kernels' edges; every claim of the table (class, narrow kept / refused, which slice and depth is
over-wide, width-0 slices, empty rows, ...) is re-derived from the matrix by the CPU test, without the library.

Nothing is committed: the builders are deterministic (values from conftest.splitmix64_uniform) and cached — callers must not
modify what they return.  No GPU, no oracle import.

Product-only cases (P*) may lack diagonals.  Solve cases (S*) share the patterns of P1, P2, P4b, P4e, with a full diagonal,
negative off-diagonals and strict diagonal dominance as conftest.fv_like_matrix has them.

Where a case differs from a bare reading of its description:
  * P2 siblings: class 1 needs padded >= 24 n, i.e. at most width * 64 * slices / 24 rows — 20 rows (one slice) at width 8,
    23 rows at width 9, 70 rows (two slices) at width 24.
  * P4f: class 1 at n = 65 600 is reached with one row of 2 950 entries in each of the first 8 slices (padded 1 575 488 >=
    24 n = 1 574 400, 89 192 entries), so the n = 65 664 fallback is not needed.
  * S3: P4b's rows hold one diagonal entry; with a full diagonal alone the Jacobi-scaled operator is the identity, BiCGSTAB is
    exact after one iteration and the unguarded reference divides 0 by 0 in the second.  S3 therefore carries a sub-diagonal
    (r, r - 1) in every row, and P4b's far column sits at depth 2 (two rows reach it, 65 536 columns apart): still class 0,
    narrow image refused.
  * a depth below a slice's width that no row reaches cannot be built: the width IS the longest row.  The `cbase = 0` branch of
    the narrow image is unreachable for a well-formed SELL image; the width-0 slice of P1 is the nearest edge.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from conftest import splitmix64_uniform

N_FAR = 65_600  # 1 025 slices: the smallest multiple of 64 above 65 536 that leaves room for a column 65 536 + c

# class: 0 uniform, 1 long ragged (spmv_k), 2 short ragged; narrow: the 16-bit column image is kept
# family: the launch counter (orc_amd.linear_algebra.PRODUCT_FAMILIES) a plain product y = A x must hit, and no other
# claims: structural facts the CPU test re-derives (see test_product_cases_cpu.py)
Case = namedtuple("Case", "name build n cls narrow family claims")

# the P1 row pattern: the middle L of these offsets from the row (no diagonal: 0 is swapped for +2)
_OFFS = np.array([-37, -20, -9, -4, -3, -1, 0, 1, 3, 5, 11, 23, 41])


def _finish(n, rows, seed, solve):
    """rows: list of n ascending int arrays.  Product-only: values uniform[-1, 1).  Solve: every row gets its diagonal, the
    off-diagonals are -(0.5 + 0.5 |r|) and the diagonal is their absolute sum times (1 + 0.1 |r'|) plus 0.5 + 0.5 |r''| (a bare
    constant would give every off-diagonal-free row the same eigenvalue)."""
    if solve:
        rows = [np.union1d(c, [r]) for r, c in enumerate(rows)]
    lens = np.array([len(c) for c in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.asarray(c, dtype=np.int64) for c in rows] + [np.zeros(0, np.int64)])
    assert indices.min(initial=0) >= 0 and indices.max(initial=0) < n
    rid = np.repeat(np.arange(n), lens)
    u = splitmix64_uniform(len(indices), seed)
    if solve:
        vals = np.where(indices == rid, 0.0, -(0.5 + 0.5 * np.abs(u)))
        off = np.zeros(n)
        np.add.at(off, rid, np.abs(vals))
        d = off * (1.0 + 0.1 * np.abs(splitmix64_uniform(n, seed + 7))) + 0.5 + 0.5 * np.abs(splitmix64_uniform(n, seed + 11))
        vals = np.where(indices == rid, d[rid], vals)
    else:
        vals = np.where(u == 0.0, 0.5, u)  # no stored zero
    a = sp.csr_matrix((vals, indices, indptr), shape=(n, n))
    assert a.has_sorted_indices or not a.sort_indices()
    return a


def _cycle_row(r, n, length):
    """`length` columns around row r: the middle of _OFFS, slid (not wrapped) into [0, n); every fifth row has no diagonal"""
    if length == 0:
        return np.zeros(0, np.int64)
    lo = (len(_OFFS) - length) // 2
    offs = _OFFS[lo:lo + length].copy()
    if r % 5 == 2 and 0 in offs:
        offs[offs == 0] = 2
        offs.sort()
    c = r + offs
    if c[0] < 0:
        c = c - c[0]
    if c[-1] >= n:
        c = c - (c[-1] - (n - 1))
    return c.astype(np.int64)


def _cycle_rows(n):
    """P1's lengths: r % 13 (0 ... 12), the rows of slice 1 all empty"""
    return [_cycle_row(r, n, 0 if 64 <= r < 128 else r % 13) for r in range(n)]


# ---------------------------------------------------------------- P1 / S1
@functools.lru_cache(maxsize=None)
def short_ragged(solve=False):
    n = 193  # 3 * 64 + 1: the last slice has one live row
    return _finish(n, _cycle_rows(n), 101, solve)


# ---------------------------------------------------------------- P2 / S2 and siblings
def _long_rows(n, width, long_at, short_len=2):
    rows = []
    for r in range(n):
        if r in long_at:
            rows.append(np.arange(width, dtype=np.int64))
        elif r % 2:
            rows.append(np.unique(np.array([(r + 5) % n, (r + 17) % n]))[:short_len])  # no diagonal
        else:
            rows.append(np.unique(np.array([r, (r + 17) % n]))[:short_len])
    return rows


@functools.lru_cache(maxsize=None)
def long_ragged(solve=False):
    """n = 130: rows 9 and 64 + 30 hold all 130 columns (16 chunks + 2), every other row 2 entries; the last slice has two
    live rows, one of length 1 and one empty"""
    n = 130
    rows = _long_rows(n, 130, (9, 94))
    rows[128] = np.array([3], dtype=np.int64)
    rows[129] = np.zeros(0, np.int64)
    return _finish(n, rows, 202, solve)


@functools.lru_cache(maxsize=None)
def long_ragged_width(width):
    """slice widths exactly `width` with as many rows as class 1 (padded >= 24 n) allows"""
    n, long_at = {8: (20, (4,)), 9: (23, (22,)), 24: (70, (0, 69))}[width]
    return _finish(n, _long_rows(n, width, long_at), 210 + width, False)


# ---------------------------------------------------------------- P3: the class rule's edge
@functools.lru_cache(maxsize=None)
def class_edge(above):
    """n = 640, every slice 25 wide (padded = 16 000 = 25 n >= 24 n).  padded > 1.08 nnz flips between nnz = 14 815 (class 0)
    and 14 814 (class 1): 1 185 / 1 186 entries are taken off evenly, row 0 of each slice stays full."""
    n, w = 640, 25
    remove = 1186 if above else 1185
    per_slice = [remove // 10 + (1 if s < remove % 10 else 0) for s in range(10)]
    offs = (np.arange(w) - 12) * 5
    rows = []
    for r in range(n):
        s, i = divmod(r, 64)
        cut = 0
        if i > 0:  # 63 rows share the slice's removals: everyone q, the first `rem` rows one more
            q, rem = divmod(per_slice[s], 63)
            cut = q + (1 if i - 1 < rem else 0)
        # drop from the far end of the offset list, so the diagonal (offset 0) stays
        rows.append(np.sort((r + offs[:w - cut]) % n).astype(np.int64))
    return _finish(n, rows, 303 + int(above), False)


# ---------------------------------------------------------------- P4: the narrow image's edge
def _diag_rows(n):
    return [np.array([r], dtype=np.int64) for r in range(n)]


FAR_ROWS = (7, 40)  # rows of slice 0 that hold the far column of P4a / P4b


@functools.lru_cache(maxsize=None)
def far_depth0(col):
    """P4a (col = 65 535) / P4b (65 536): rows 7 and 40 hold that one column and no diagonal; row 0's diagonal is column 0"""
    rows = _diag_rows(N_FAR)
    for r in FAR_ROWS:
        rows[r] = np.array([col], dtype=np.int64)
    return _finish(N_FAR, rows, 404, False)


MID_SLICE = 512


@functools.lru_cache(maxsize=None)
def far_mid_depth1():
    """P4c: two rows of slice 512 reach depth 1, with columns 10 and 10 + 65 536 (their depth-0 columns 3 and 5 keep depth 0
    within 32 829 columns)"""
    rows = _diag_rows(N_FAR)
    rows[MID_SLICE * 64 + 3] = np.array([3, 10], dtype=np.int64)
    rows[MID_SLICE * 64 + 20] = np.array([5, 10 + 65536], dtype=np.int64)
    return _finish(N_FAR, rows, 405, False)


@functools.lru_cache(maxsize=None)
def far_last_slice():
    """P4d: row 65 540 (last slice, columns 65 536 ... 65 599 otherwise) holds column 0 alone"""
    rows = _diag_rows(N_FAR)
    rows[65540] = np.array([0], dtype=np.int64)
    return _finish(N_FAR, rows, 406, False)


@functools.lru_cache(maxsize=None)
def far_short_ragged(solve=False):
    """P4e / S4: P1's row-length cycle on 65 600 rows with P4b's far column in rows 7 and 40.  With the diagonal in front of it
    (S4) the far column sits at depth 1, where the slice's smallest column is 1 or more: there it is the last column, 65 599."""
    rows = _cycle_rows(N_FAR)
    for r in FAR_ROWS:
        rows[r] = np.array([N_FAR - 1 if solve else 65536], dtype=np.int64)
    return _finish(N_FAR, rows, 407, solve)


LONG_F = 2950  # 368 chunks + 6


@functools.lru_cache(maxsize=None)
def far_long_ragged():
    """P4f: row 64 s + 1 of the first 8 slices holds 2 950 columns (stride 22), P4b's far column in rows 7 and 40"""
    rows = _diag_rows(N_FAR)
    for s in range(8):
        rows[64 * s + 1] = (np.arange(LONG_F, dtype=np.int64) * 22 + s)
    for r in FAR_ROWS:
        rows[r] = np.array([65536], dtype=np.int64)
    return _finish(N_FAR, rows, 408, False)


@functools.lru_cache(maxsize=None)
def far_bidiagonal_solve():
    """S3: diagonal + sub-diagonal in every row; rows 7 and 40 are the only ones that reach depth 2, with columns 12 and
    12 + 65 536"""
    rows = [np.array([r - 1, r] if r else [0], dtype=np.int64) for r in range(N_FAR)]
    rows[7] = np.array([6, 7, 12], dtype=np.int64)            # depth 2: column 12
    rows[40] = np.array([39, 40, 12 + 65536], dtype=np.int64)  # depth 2: column 12 + 65 536
    return _finish(N_FAR, rows, 409, True)


P_CASES = (
    Case("P1_short_ragged", short_ragged, 193, 2, True, "narrow",
         dict(width0_slice=1, empty_row=True, missing_diag=True, last_slice_live=1)),
    Case("P2_long_ragged", long_ragged, 130, 1, True, "ragged",
         dict(widths=(130, 130, 1), width_mod8=2, last_slice_live=2, last_slice_lens=(1, 0), empty_row=True, missing_diag=True)),
    Case("P2_width8", functools.partial(long_ragged_width, 8), 20, 1, True, "ragged", dict(widths=(8,))),
    Case("P2_width9", functools.partial(long_ragged_width, 9), 23, 1, True, "ragged", dict(widths=(9,))),
    Case("P2_width24", functools.partial(long_ragged_width, 24), 70, 1, True, "ragged", dict(widths=(24, 24), last_slice_live=6)),
    Case("P3a_class_edge_below", functools.partial(class_edge, False), 640, 0, True, "narrow", dict(widths=(25,) * 10, nnz=14815)),
    Case("P3b_class_edge_above", functools.partial(class_edge, True), 640, 1, True, "ragged", dict(widths=(25,) * 10, nnz=14814)),
    Case("P4a_span_65535", functools.partial(far_depth0, 65535), N_FAR, 0, True, "narrow", dict(max_span=65535, max_span_at=(0, 0))),
    Case("P4b_span_65536", functools.partial(far_depth0, 65536), N_FAR, 0, False, "wide", dict(wide_at=[(0, 0)])),
    Case("P4c_mid_depth1", far_mid_depth1, N_FAR, 0, False, "wide", dict(wide_at=[(MID_SLICE, 1)])),
    Case("P4d_last_slice", far_last_slice, N_FAR, 0, False, "wide", dict(wide_at=[(1024, 0)])),
    Case("P4e_far_short_ragged", far_short_ragged, N_FAR, 2, False, "wide", dict(width0_slice=1, empty_row=True, missing_diag=True, wide_at=[(0, 0)])),
    Case("P4f_far_long_ragged", far_long_ragged, N_FAR, 1, False, "ragged", dict(width_mod8=LONG_F % 8, max_width=LONG_F, wide_at=[(0, 0)])),
)

S_CASES = (
    Case("S1_short_ragged", functools.partial(short_ragged, True), 193, 2, True, "narrow", dict(full_diag=True, last_slice_live=1)),
    Case("S2_long_ragged", functools.partial(long_ragged, True), 130, 1, True, "ragged", dict(full_diag=True, last_slice_live=2)),
    Case("S3_far_bidiagonal", far_bidiagonal_solve, N_FAR, 0, False, "wide", dict(full_diag=True, wide_at=[(0, 2)])),
    Case("S4_far_short_ragged", functools.partial(far_short_ragged, True), N_FAR, 2, False, "wide", dict(full_diag=True, wide_at=[(0, 1)])),
)

CASES = {c.name: c for c in P_CASES + S_CASES}

# ---------------------------------------------------------------- the solves of the GPU test
JACOBI, BICGSTAB = 1, 3
PRE_NONE, PRE_JACOBI = 0, 1
BICG_ON_THE_FLY, BICG_MATERIALISED = 3, 8  # below / at or above ORC_MATERIALIZE_SCALING = 4 iterations
# (case, preconditioner) -> BiCGSTAB iteration counts; a count the unguarded reference cannot finish finite would be lowered HERE
# (test_product_cases_cpu.py::test_oracle_finishes_every_listed_solve_finite is the condition)
BICG_COUNTS = {(c.name, pre): (BICG_ON_THE_FLY, BICG_MATERIALISED) for c in S_CASES for pre in (PRE_NONE, PRE_JACOBI)}
JACOBI_ARM_CASES = ("S1_short_ragged", "S2_long_ragged")
JACOBI_ARM_RUNS = ((1e-30, 25), (0.2, 50))  # (threshold, sweeps): never breaks / breaks on the residual ratio
JACOBI_RELAXATION = 0.7


def solve_system(name):
    """(a, b, x0) of a solve case"""
    a = CASES[name].build()
    n = a.shape[0]
    return a, a @ splitmix64_uniform(n, 7), 0.1 * splitmix64_uniform(n, 8)


def product_vector(name):
    return splitmix64_uniform(CASES[name].n, 8)


def solve_family(case, scaled_on_the_fly, nt):
    """The one family every product of a BiCGSTAB solve on a USER matrix (no mirrors, no persistent pattern) must hit, from the
    table's class and narrow columns: class 1 has one kernel whatever the call; scalings carried on the fly take the generic
    kernel; the non-temporal instantiation exists for the narrow image only."""
    if case.cls == 1:
        return "ragged"
    if scaled_on_the_fly:
        return "generic_scaled"
    if case.narrow:
        return "narrow_nt" if nt else "narrow"
    return "wide"


# ---------------------------------------------------------------- what the CPU test derives
def sell_stats(a):
    """SELL-64 facts of a CSR matrix, computed from the matrix alone: widths per slice, padded, the class by the rule above,
    and the column span (max - min) of every (slice, depth) that a row reaches, as a dict."""
    n = a.shape[0]
    lens = np.diff(a.indptr).astype(np.int64)
    n_slices = (n + 63) // 64
    padl = np.zeros(n_slices * 64, np.int64)
    padl[:n] = lens
    widths = padl.reshape(n_slices, 64).max(axis=1)
    padded = int(widths.sum() * 64)
    nnz = int(a.nnz)
    cls = (2 if padded < 24 * max(n, 1) else 1) if padded > 1.08 * max(nnz, 1) else 0
    rid = np.repeat(np.arange(n), lens)
    depth = np.arange(nnz) - np.repeat(a.indptr[:-1].astype(np.int64), lens)
    base = np.concatenate([[0], np.cumsum(widths)])
    key = base[rid >> 6] + depth
    lo = np.full(int(base[-1]) + 1, np.iinfo(np.int64).max)
    hi = np.full(int(base[-1]) + 1, -1)
    cols = a.indices.astype(np.int64)
    np.minimum.at(lo, key, cols)
    np.maximum.at(hi, key, cols)
    reached = hi >= 0
    span = np.where(reached, hi - lo, -1)
    slice_of = np.repeat(np.arange(n_slices), widths)
    depth_of = np.arange(int(base[-1])) - np.repeat(base[:-1], widths)
    spans = {(int(s), int(d)): int(v) for s, d, v in zip(slice_of, depth_of, span[:-1])}
    return dict(n=n, nnz=nnz, lens=lens, widths=widths, padded=padded, cls=cls, spans=spans,
                narrow=all(v <= 65535 for v in spans.values()), unreached=[k for k, v in spans.items() if v < 0])


def sequential_product(a, x):
    """y = A x, every row summed in ascending-column order from 0.0, one multiply and one add per step (numpy never fuses them)"""
    n = a.shape[0]
    rp, ci, v = a.indptr.astype(np.int64), a.indices, a.data
    lens = np.diff(rp)
    acc = np.zeros(n)
    idx = np.flatnonzero(lens > 0)
    k = 0
    while len(idx):
        p = rp[idx] + k
        acc[idx] = acc[idx] + v[p] * x[ci[p]]
        k += 1
        idx = idx[lens[idx] > k]
    return acc
