"""numpy restatement of the volume reports (DESIGN.md §3 "Volume reports", orc_types.h OrcGroupQuantity) from the labels alone.

The lists and chunks are built from the ids as the library builds them: the cells of a group ascending in ORC id, a group's list cut
from its start into chunks of `chunk` entries.  Every term is formed in float64 with the device's rounded multiplies, one IEEE operation
per numpy operation (numpy never fuses), so a term here and the device's term of the same cell are the same bits; only the summation
differs.  The sums are math.fsum (exactly rounded), and next to every sum comes sum |term|: the scale of the device's rounding.

Per listed cell with weight w (the stored volume, or 1.0) and field value x:
    t1 = w * x        t2 = t1 * x        W = sum w      SUM = sum t1      SUM_SQ = sum t2
    MIN / MAX: a NaN never wins; among equal values the smallest ORC id (= the smallest list position) wins; a group without a cell
    or with NaN only gives +inf, -inf and the cell -1.
"""
import math

import numpy as np

EPS = 2.0 ** -53  # unit roundoff of float64: the relative error of one rounded operation
SUM, SUM_SQ, MIN, MAX = 0, 1, 2, 3
WAVE_DEPTH = 6    # the __shfl_down tree over the 64 lanes of a wave
WAVES = 4         # waves of a workgroup, added in sequence


def lists(ids, n_groups):
    """(group_ptr [G + 1], cells [listed]): what CellGroups.group_ptr / .cells must equal — one stable sort of the ORC cell ids by label"""
    ids = np.asarray(ids)
    listed = np.flatnonzero(ids >= 0)
    order = listed[np.argsort(ids[listed], kind="stable")]
    counts = np.bincount(ids[listed], minlength=n_groups)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), order.astype(np.int64)


def chunks_of(group_ptr, chunk):
    """chunks per group: ceil(count / chunk)"""
    return (np.diff(group_ptr) + chunk - 1) // chunk


def weights(volume, weighting):
    v = np.asarray(volume, dtype=np.float64)
    return v if weighting == "volume" else np.ones(len(v))


def extremum(x, cells, largest):
    """(value, ORC cell) of the minimum (largest=False) or maximum under the rules above; the value's bits are the winning cell's"""
    ok = ~np.isnan(x)
    if not ok.any():
        return (-np.inf if largest else np.inf), -1
    m = np.max(x[ok]) if largest else np.min(x[ok])
    pos = int(np.flatnonzero(x == m)[0])  # == holds for -0.0 against 0.0 too: the first of them wins, as on the device
    return x[pos], int(cells[pos])


def report(ids, n_groups, volume, fields, weighting="volume"):
    """dict of W [G], count [G], S [G, F, 4] (SUM and SUM_SQ exactly rounded), Sabs [G, F, 2] = sum |t1|, sum |t2|, where [G, F, 2]"""
    fields = np.asarray(fields, dtype=np.float64).reshape(-1, len(ids))
    gp, cells = lists(ids, n_groups)
    w_all = weights(volume, weighting)
    G, F = n_groups, len(fields)
    out = dict(W=np.zeros(G), count=np.diff(gp), S=np.zeros((G, F, 4)), Sabs=np.zeros((G, F, 2)), where=np.full((G, F, 2), -1, np.int64),
               group_ptr=gp, cells=cells)
    for g in range(G):
        c = cells[gp[g]:gp[g + 1]]
        w = w_all[c]
        out["W"][g] = math.fsum(w.tolist())
        for f in range(F):
            x = fields[f][c]
            with np.errstate(invalid="ignore", over="ignore"):
                t1 = w * x
                t2 = t1 * x
            nan = bool(np.isnan(t1).any() or np.isnan(t2).any())
            out["S"][g, f, SUM] = np.nan if nan else math.fsum(t1.tolist())
            out["S"][g, f, SUM_SQ] = np.nan if nan else math.fsum(t2.tolist())
            out["Sabs"][g, f, 0] = np.nan if nan else math.fsum(np.abs(t1).tolist())
            out["Sabs"][g, f, 1] = np.nan if nan else math.fsum(np.abs(t2).tolist())
            out["S"][g, f, MIN], out["where"][g, f, 0] = extremum(x, c, False)
            out["S"][g, f, MAX], out["where"][g, f, 1] = extremum(x, c, True)
    return out


def depth(count, chunk, slots):
    """Rounded additions on the longest path of the device's tree over a group of `count` cells, counted from the association:
        slots          a lane adds its entries begin + tid + 256 k one after the other in ascending k (the first to 0.0, exactly)
        WAVE_DEPTH 6   the wave's __shfl_down tree, offsets 32 .. 1
        WAVES 4        ((w0 + w1) + w2) + w3 through LDS: three additions, bounded by the number of waves
        ceil(log2(chunks))   the pairwise fold of the group's chunks in chunk order
        + 1            math.fsum's own rounding of the exact sum"""
    n_chunks = np.maximum((np.asarray(count) + chunk - 1) // chunk, 1)
    return slots + WAVE_DEPTH + WAVES + np.ceil(np.log2(n_chunks)) + 1


def bound(Sabs, count, chunk, slots):
    """|device - fsum| <= D * 2^-53 * sum |term| per group (first axis of Sabs), D = depth()"""
    D = depth(count, chunk, slots)
    return D.reshape((-1,) + (1,) * (np.ndim(Sabs) - 1)) * EPS * np.asarray(Sabs)


def check(rep, want, chunk, slots):
    """assert a GroupReport against report(): count, extrema and their cells bit for bit; W, SUM and SUM_SQ within bound(), and NaN
    exactly where a term is NaN.  Returns the largest error / bound ratio seen (for printing)."""
    assert np.array_equal(rep.count, want["count"]), (rep.count, want["count"])
    assert np.array_equal(rep.min, want["S"][:, :, MIN]) and np.array_equal(rep.max, want["S"][:, :, MAX])
    assert np.array_equal(np.signbit(rep.min), np.signbit(want["S"][:, :, MIN]))
    assert np.array_equal(np.signbit(rep.max), np.signbit(want["S"][:, :, MAX]))
    assert np.array_equal(rep.argmin, want["where"][:, :, 0]), (rep.argmin, want["where"][:, :, 0])
    assert np.array_equal(rep.argmax, want["where"][:, :, 1]), (rep.argmax, want["where"][:, :, 1])
    worst = 0.0
    for name, got, ref, scale in (("W", rep.weight, want["W"], np.abs(want["W"])),
                                  ("SUM", rep.sum, want["S"][:, :, SUM], want["Sabs"][:, :, 0]),
                                  ("SUM_SQ", rep.sum_sq, want["S"][:, :, SUM_SQ], want["Sabs"][:, :, 1])):
        B = bound(scale, want["count"], chunk, slots)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (name, got, ref)
        with np.errstate(invalid="ignore"):
            err = np.where(nan | (got == ref), 0.0, np.abs(got - ref))  # an infinite sum is met exactly or not at all
            B = np.where(nan, 0.0, B)
        assert np.all(err <= B), (name, want["count"], got, ref, err, B)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.max(np.where(B > 0, err / B, 0.0), initial=0.0)))
    return worst
