"""Fine matrices whose coarse operator has a PRESCRIBED pattern (tests/test_gpu_xwin_compact.py, tests/test_xwin_compact_cpu.py).

The fine rows 2 I and 2 I + 1 hold each other as their strongest entry (-2 against off-diagonals in (-0.75, -0.25)), so the reference's
pairing (linear_algebra.rs:30-60, tests/amg_cases.py: greedy_pairing) joins exactly them, coarse row I = {2 I, 2 I + 1} and fine column j
becomes coarse column j // 2.  Fine row 2 I carries the columns 2 c of the prescribed coarse columns c of row I; row 2 I + 1 only its pair.
A coarse row listed as None is EMPTY: its two fine rows hold nothing but their diagonals, nothing pairs them.  The values are
not dyadic: the order of every sum matters, which is what a bit-for-bit comparison of products wants.  Builders are deterministic."""
import numpy as np
import scipy.sparse as sp

from conftest import splitmix64_uniform


def forced_pairs(coarse_cols, seed=5):
    """coarse_cols[I]: ascending distinct coarse columns of row I other than I itself (an int array, possibly empty), or None for an empty
    coarse row.  Returns the fine CSR matrix (2 len(coarse_cols) rows)."""
    nc = len(coarse_cols)
    rows, cols = [], []
    for I, c in enumerate(coarse_cols):
        if c is None:
            rows += [np.array([2 * I, 2 * I + 1])]
            cols += [np.array([2 * I, 2 * I + 1])]
            continue
        c = np.asarray(c, np.int64)
        assert np.all(c != I) and np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < nc))
        rows += [np.full(len(c) + 2, 2 * I), np.array([2 * I + 1, 2 * I + 1])]
        cols += [np.concatenate([2 * c, [2 * I, 2 * I + 1]]), np.array([2 * I, 2 * I + 1])]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    u = splitmix64_uniform(len(rows), seed)
    vals = -(0.5 + 0.25 * u)
    vals[(rows ^ 1) == cols] = -2.0
    vals[rows == cols] = 0.0
    a = sp.csr_matrix((vals, (rows, cols)), shape=(2 * nc, 2 * nc))
    d = -np.asarray(a.sum(axis=1)).ravel() * (1.0 + 0.1 * np.abs(splitmix64_uniform(2 * nc, seed + 7))) + 1.0
    a = (a + sp.diags(d)).tocsr()
    a.sort_indices()
    return a


def coarse_pattern(coarse_cols):
    """the prescription as (indptr, indices) of the coarse operator: row I holds I and coarse_cols[I], ascending; None rows are empty, and
    — their fine rows being unmatched, i.e. absent from R — so are their columns"""
    gone = np.array([I for I, c in enumerate(coarse_cols) if c is None], np.int64)
    out = [np.zeros(0, np.int64) if c is None else np.sort(np.concatenate([np.setdiff1d(np.asarray(c, np.int64), gone), [I]])) for I, c in enumerate(coarse_cols)]
    return np.concatenate([[0], np.cumsum([len(c) for c in out])]).astype(np.int64), np.concatenate(out + [np.zeros(0, np.int64)])


def _near(I, count, nc):
    """`count` columns next to I (alternating above and below), never I"""
    out, d = [], 1
    while len(out) < count:
        for c in (I + d, I - d):
            if 0 <= c < nc and len(out) < count:
                out.append(c)
        d += 1
    return np.array(sorted(out), np.int64)


SLICE_LENGTHS = (1, 7, 8, 9, 15, 16, 17)


def big_window(window, nc=4096 + 2 * 64 + 37):
    """Block 0 (rows 0 ... 255) references exactly the columns 0 ... window - 1 (window >= 1024, a multiple of 256), its largest column — window
    position window - 1 — as the LAST entry of eight rows whose lengths are 1 ... 8 modulo 8: the position lands in each of the eight slots of a
    chunk of positions.  Slice 4 (rows 256 ... 319) has rows of 1, 7, 8, 9, 15, 16 and 17 entries; row window + 40 is empty (its column leaves the
    operator with it, so it lies outside block 0's window); the other rows hold 2 - 12 entries next to their diagonal.  With the default nc the last block has three slices and the last slice 37 rows."""
    per = window // 256
    top = window - 1
    cc = []
    for I in range(256):
        c = set(range(per * I, per * I + per)) - {I}
        cc.append(c)
    for s in range(8):  # rows 8 ... 15: columns from their own range, then `top`; lengths (with the diagonal) 9 + s, i.e. last slot (8 + s) % 8
        I = 8 + s
        own = sorted(cc[I])
        keep = own[:7 + s]
        dropped = set(own) - set(keep)
        cc[I] = set(keep) | {top}
        cc[200 + s] |= dropped - {200 + s}  # ... and the columns they gave up stay in the window (a row's own column does as its diagonal)
    cols = [np.array(sorted(c), np.int64) for c in cc]
    want = dict(zip(range(256 + 3, 256 + 3 + 4 * len(SLICE_LENGTHS), 4), SLICE_LENGTHS))
    for I in range(256, nc):
        if I == window + 40:
            cols.append(None)
        elif I in want:
            cols.append(_near(I, want[I] - 1, nc))
        else:
            cols.append(_near(I, 1 + (I * 7) % 11, nc))
    return cols


def tridiagonal_with_far(nc, far):
    """Coarse rows hold their two neighbours: the window of block b is the contiguous run 256 b - 1 ... 256 b + 256.  far: {block: offset}; the
    last row of such a block gives up its upper neighbour and takes column 256 b + 255 + offset instead: the block's list has 257 contiguous
    entries — entry 256, the base of its fifth segment, is column 256 b + 255 — followed by ONE entry `offset` columns above that base."""
    cols = []
    for I in range(nc):
        c = [x for x in (I - 1, I + 1) if 0 <= x < nc]
        b = I // 256
        if b in far and I == 256 * b + 255:
            c = [I - 1, I + far[b]]
        cols.append(np.array(c, np.int64))
    return cols
