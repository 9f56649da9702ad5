"""Case table of the AMG set-up tests (tests/test_amg_cases_cpu.py, tests/test_gpu_amg_cases.py) and two plain references.

The Multigrid set-up (orc_amd/csrc/amg_pairing.hip, amg_galerkin.hip: the pairing da_first_k / da_chase_k / agg_verify_k, the Galerkin product galerkin_bound_k /
galerkin_merge_k) takes any user CSR matrix and branches on quantities a finite-volume matrix never moves:
  * the LDS tier of a coarse row: its candidate count c (the summed lengths of its <= 4 fine rows) goes to the narrowest tier t = 0..6 with
    64 << t >= 2 c, i.e. tier t holds c <= 32 << t; above c = 2048 the set-up refuses;
  * the lanes per coarse row of a tier (16, 16, 32, 64, ...) against the fine rows' lengths (first-G-entries prefetch);
  * the scan of a row whose four-entry preference list ran out: from registers up to 8 G entries (G = 4 lanes per chain when the mean padded
    row length is <= 24, else 8), in two sweeps beyond;
  * ties: the reference's strict `<` keeps the first of equal coefficients.
The matrices here sit on those limits.  What each case claims (`expect`) is re-derived from the matrix by the CPU test with the two references
below, without the library:
  * greedy_pairing: the reference's Strongest pairing (build_restriction_matrix, linear_algebra.rs:30-60), restated from the Rust;
  * with DYADIC values (integer multiples of 2^-10 below 2^12, integer diagonals) every sum of (R a) R^T is exact in double precision in any
    order, so scipy's `R @ a @ R.T` is an association-free exact reference (exact_coarse).

Nothing is committed: the builders are deterministic (conftest.splitmix64_uniform; random_doubles alone draws from numpy's default_rng) and
cached — callers must not modify what they return.  No GPU, no oracle import."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from conftest import splitmix64_uniform

FLOAT_MAX = np.finfo(np.float64).max
N_TIERS = 7
REFUSED = N_TIERS      # index of "refused" in predicted()'s histogram
CAND_LIMIT = 2048      # 2 c <= 64 << 6

# expect: dyadic (bool) and any of
#   tiers: tiers that must hold at least one coarse row       max_c: the largest candidate count, exactly
#   refused: True: some coarse row has c > CAND_LIMIT         deep_long: a row longer than 64 entries with depth > 3
#   max_len: the longest fine row, exactly                    deeper_than_list: at least this many rows with depth > 3
#   ties: a row whose chosen column ties with an earlier, taken one
#   weight2_only / unmatched / empty_coarse / positive: the shapes of R the case is named after
Case = namedtuple("Case", "name build expect")


# ---------------------------------------------------------------- the two references
def _pairing(a):
    """linear_algebra.rs:30-60 on a scipy CSR matrix with sorted columns: rows in ascending order; a row folds over its columns, skipping the
    diagonal and the columns in `combined_cells` (taken by an EARLIER row's choice — a row that has chosen is not thereby taken), and keeps
    the column whose coefficient is strictly below the strongest so far (Float::MAX at the start: that value and NaN are never chosen)."""
    n = a.shape[0]
    rp, ci, v = a.indptr.tolist(), a.indices.tolist(), a.data.tolist()
    taken = [False] * n
    partner = np.full(n, -1, np.int64)
    depth = np.zeros(n, np.int64)
    tie = np.zeros(n, bool)
    for i in range(n):
        strongest, acc, kc, passed = FLOAT_MAX, -1, -1, []
        for k in range(rp[i], rp[i + 1]):
            j = ci[k]
            if taken[j] or i == j:
                if i != j and v[k] < FLOAT_MAX:
                    passed.append((v[k], k))  # a candidate an earlier row holds
                continue
            if v[k] < strongest:
                strongest, acc, kc = v[k], j, k
        if acc >= 0:
            taken[acc] = True
            partner[i] = acc
            # better ranked (value ascending, position ascending) than the chosen entry: strictly below it, or equal and in front of it
            depth[i] = sum(1 for x, k in passed if x < strongest or (x == strongest and k < kc))
            tie[i] = any(x == strongest and k < kc for x, k in passed)
        else:
            depth[i] = len(passed)
    return partner, depth, tie


def greedy_pairing(a):
    """(partner, depth): partner[i] = the column row i takes (-1: nothing left), depth[i] = how many better-ranked candidates it found taken"""
    partner, depth, _ = _pairing(a)
    return partner, depth


def tie_rows(a):
    """rows whose chosen column has the value of an earlier (lower-position) candidate that was already taken"""
    return np.flatnonzero(_pairing(a)[2])


def restriction(partner, n):
    """R as the reference pushes its triplets (:56-57): (i // 2, i) and (i // 2, partner[i]) for every matched row, duplicates summed"""
    i = np.flatnonzero(np.asarray(partner) >= 0)
    rows = np.concatenate([i // 2, i // 2])
    cols = np.concatenate([i, np.asarray(partner)[i]])
    r = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=((n + 1) // 2, n)).tocsr()
    r.sum_duplicates()
    r.sort_indices()
    return r


def tier_of(c):
    """the narrowest tier with 64 << t >= 2 c (galerkin_bound_k); REFUSED above CAND_LIMIT"""
    if c > CAND_LIMIT:
        return REFUSED
    t = 0
    while (64 << t) < 2 * c:
        t += 1
    return t


def predicted(a, partner):
    """(c per coarse row, histogram over the 7 tiers + refused, longest fine row): c = the summed lengths of the distinct fine rows of row I
    of R; an empty coarse row has c = 0 and sits in tier 0"""
    n = a.shape[0]
    lens = np.diff(a.indptr).astype(np.int64)
    r = restriction(partner, n)
    c = np.zeros(r.shape[0], np.int64)
    np.add.at(c, np.repeat(np.arange(r.shape[0]), np.diff(r.indptr)), lens[r.indices])
    hist = np.bincount([tier_of(int(x)) for x in c], minlength=N_TIERS + 1).astype(np.int64)
    return c, hist, int(lens.max(initial=0))


def exact_coarse(a, partner):
    """(R a) R^T by scipy, columns sorted, stored zeros kept: exact for dyadic cases whatever the order of the sums"""
    r = restriction(partner, a.shape[0])
    ac = (r @ a @ r.T).tocsr()
    ac.sort_indices()
    return ac


def dominant(a):
    """`a` with every diagonal entry replaced by 1 + the row's absolute off-diagonal sum rounded up (strictly diagonally dominant; every
    row must hold its diagonal)"""
    a = a.copy()
    n = a.shape[0]
    rid = np.repeat(np.arange(n), np.diff(a.indptr))
    on = a.indices == rid
    assert on.sum() == n
    off = np.zeros(n)
    np.add.at(off, rid[~on], np.abs(a.data[~on]))
    a.data[on] = np.ceil(off) + 1.0
    return a


# ---------------------------------------------------------------- builders
def _dyadic(count, seed):
    """-k / 1024, k = 1 ... 4095"""
    return -(np.floor((splitmix64_uniform(count, seed) + 1.0) * 0.5 * 4095.0) + 1.0) / 1024.0


def _from_rows(n, rows, off_values, diag):
    """rows: ascending int arrays (diagonal included where the row has one); off_values(i, cols) -> the off-diagonal values of row i; diag[i]"""
    lens = np.array([len(c) for c in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.asarray(c, np.int64) for c in rows] + [np.zeros(0, np.int64)])
    data = np.zeros(len(indices))
    for i, c in enumerate(rows):
        c = np.asarray(c, np.int64)
        vals = np.empty(len(c))
        offm = c != i
        vals[offm] = off_values(i, c[offm])
        vals[~offm] = diag[i]
        data[indptr[i]:indptr[i + 1]] = vals
    a = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    assert a.has_sorted_indices or not a.sort_indices()
    return a


def _blocks(sizes):
    """[(offset, size)] and the dense block-diagonal row patterns"""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    rows = []
    for o, s in zip(offs[:-1], sizes):
        rows += [np.arange(o, o + s, dtype=np.int64)] * s
    return list(zip(offs[:-1].tolist(), sizes)), rows, int(offs[-1])


SHARED_SIZES = (6, 12, 20, 40, 72, 136, 264)
RANDOM_SIZES = (7, 13, 21, 41, 73, 137, 263)


def _shared(sizes, seed):
    """dense blocks; inside a block every row has the same off-diagonal values -(1 + perm(j) / 64): all rows want the same columns"""
    blocks, rows, n = _blocks(sizes)
    colval = np.zeros(n)
    diag = np.zeros(n)
    for b, (o, s) in enumerate(blocks):
        perm = np.argsort(splitmix64_uniform(s, seed + b), kind="stable")
        colval[o:o + s] = -(1.0 + perm / 64.0)
        diag[o:o + s] = 4.0 * s
    return _from_rows(n, rows, lambda i, c: colval[c], diag)


@functools.lru_cache(maxsize=None)
def ladder_shared():
    return _shared(SHARED_SIZES, 1100)


@functools.lru_cache(maxsize=None)
def dense_shared(size):
    return _shared((size,), 1200 + size)


def _ladder_random(values):
    blocks, rows, n = _blocks(RANDOM_SIZES)
    diag = np.concatenate([np.full(s, 4.0 * s) for _, s in blocks])
    ptr = np.concatenate([[0], np.cumsum([len(c) - 1 for c in rows])])
    return _from_rows(n, rows, lambda i, c: values[ptr[i]:ptr[i + 1]], diag)


def _ladder_random_off_count():
    return sum(s * (s - 1) for s in RANDOM_SIZES)


@functools.lru_cache(maxsize=None)
def ladder_random():
    return _ladder_random(_dyadic(_ladder_random_off_count(), 1300))


@functools.lru_cache(maxsize=None)
def all_ties():
    return _ladder_random(np.full(_ladder_random_off_count(), -1.0))


@functools.lru_cache(maxsize=None)
def random_doubles():
    return _ladder_random(-(0.5 + np.random.default_rng(1400).random(_ladder_random_off_count())))


def _band_rows(n, length):
    """odd length: symmetric half-width (length - 1) / 2; even: one more sub- than super-diagonal (structurally asymmetric)"""
    below, above = length // 2, (length - 1) // 2
    return [np.arange(max(0, i - below), min(n, i + above + 1), dtype=np.int64) for i in range(n)]


def _band(n, length, seed, values=None, sign=-1.0, isolate=()):
    rows = _band_rows(n, length)
    for i in isolate:
        rows[i] = np.array([i], dtype=np.int64)
    count = sum(len(c) - 1 for c in rows)
    vals = _dyadic(count, seed) if values is None else values(count)
    ptr = np.concatenate([[0], np.cumsum([len(c) - 1 for c in rows])])
    return _from_rows(n, rows, lambda i, c: -sign * vals[ptr[i]:ptr[i + 1]], np.full(n, sign * -4.0 * length))


BAND_N = 257
BAND_LENGTHS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def band(length, n=BAND_N):
    return _band(n, length, 1500 + length)


@functools.lru_cache(maxsize=None)
def few_values():
    """banded, 33 entries per row, n = 193; off-diagonals from {-1, -0.5}"""
    return _band(193, 33, 0, values=lambda count: np.where(splitmix64_uniform(count, 1600) < 0.0, -1.0, -0.5))


@functools.lru_cache(maxsize=None)
def mutual_pairs():
    """tridiagonal, n = 130: rows 2k and 2k + 1 hold each other as their strongest entry (-2 against -1)"""
    n = 130
    rows = [np.arange(max(0, i - 1), min(n, i + 2), dtype=np.int64) for i in range(n)]
    return _from_rows(n, rows, lambda i, c: np.where(c == (i ^ 1), -2.0, -1.0), np.full(n, 4.0))


ISOLATED_RUN = (100, 101, 102, 103)  # starts at an even index: coarse rows 50 and 51 are empty


def isolated_at(n=BAND_N):
    return tuple(sorted(set(r for r in range(n) if r % 11 == 3) | set(ISOLATED_RUN)))


@functools.lru_cache(maxsize=None)
def isolated_rows():
    """band(17) with the rows r % 11 == 3, and the run 100 ... 103, reduced to their diagonal (their columns stay in the other rows)"""
    return _band(BAND_N, 17, 1500 + 17, isolate=isolated_at())


@functools.lru_cache(maxsize=None)
def positive_offdiag():
    """band(17) with positive off-diagonals and a negative diagonal: the strongest entry is the SMALLEST positive one"""
    return _band(BAND_N, 17, 1500 + 17, sign=1.0)


SIZES = (1, 2, 3, 63, 64, 65, 127, 129)


def _expect(dyadic=True, **kw):
    return dict(dyadic=dyadic, **kw)


CASES_LIST = [
    Case("ladder_shared", ladder_shared, _expect(tiers=(0, 1, 2, 3, 4, 5, 6), max_len=264, deep_long=True, deeper_than_list=500)),
    Case("ladder_random", ladder_random, _expect(tiers=(0, 1, 2, 3, 4, 5, 6), max_len=263)),
    Case("dense_at_limit", functools.partial(dense_shared, 512), _expect(tiers=(6,), max_c=2048, max_len=512, deep_long=True)),
    Case("dense_over_limit", functools.partial(dense_shared, 514), _expect(refused=True, max_c=2056, max_len=514)),
]
CASES_LIST += [Case("band_%d" % length, functools.partial(band, length), _expect(max_len=length)) for length in BAND_LENGTHS]
CASES_LIST += [
    Case("all_ties", all_ties, _expect(ties=True, max_len=263, deep_long=True)),
    Case("few_values", few_values, _expect(ties=True, max_len=33)),
    Case("mutual_pairs", mutual_pairs, _expect(weight2_only=True, max_len=3)),
    Case("isolated_rows", isolated_rows, _expect(unmatched=True, empty_coarse=True, max_len=17)),
    Case("positive_offdiag", positive_offdiag, _expect(positive=True, max_len=17)),
]
CASES_LIST += [Case("sizes_%d" % n, functools.partial(band, 17, n), _expect(max_len=min(17, n if n < 9 else 17))) for n in SIZES]
CASES_LIST += [Case("random_doubles", random_doubles, _expect(dyadic=False, max_len=263))]

CASES = {c.name: c for c in CASES_LIST}
NAMES = [c.name for c in CASES_LIST]
REFUSED_CASE = "dense_over_limit"
COARSENED = [n for n in NAMES if n != REFUSED_CASE]              # cases the set-up completes
SCANNING = ("ladder_shared", "dense_at_limit", "all_ties")      # the chains must have scanned rows (scans > 0)
FORM_CASES = ("ladder_shared", "ladder_random", "all_ties", "band_65")
SECOND_LEVEL = ("ladder_random", "band_33")
END_TO_END = ("band_33", "ladder_random")


@functools.lru_cache(maxsize=None)
def pairing(name):
    """(partner, depth) of a case, computed once"""
    partner, depth = greedy_pairing(CASES[name].build())
    partner.setflags(write=False)
    depth.setflags(write=False)
    return partner, depth


@functools.lru_cache(maxsize=None)
def prediction(name):
    return predicted(CASES[name].build(), pairing(name)[0])


def end_to_end_system(name):
    """(a, b, x0): the case made strictly diagonally dominant, b = a x* """
    a = dominant(CASES[name].build())
    n = a.shape[0]
    return a, a @ splitmix64_uniform(n, 7), 0.1 * splitmix64_uniform(n, 8)
