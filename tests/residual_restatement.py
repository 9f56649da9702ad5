"""Numpy restatement of the residual monitors (include/orc_types.h OrcResidual, DESIGN.md §3 "Residual monitors"); no device.

momentum(values, b, field, pattern): per owned row P of one momentum system, with CSR values in pattern order (as
Solver.assemble_momentum() returns them), b and the field in the mesh's INTERNAL cell order (Mesh.cell_order() maps a field of
get_fields() there: field_orc[mesh.cell_order()]):
    y_P = the row's sum of a_Pj phi_j in ascending stored order from 0.0, formed depth by depth as acc += a[:, k] * x[col[:, k]] —
          numpy multiplies and adds separately, as the kernel built with -ffp-contract=off does, so these are the kernel's numbers
          bit for bit;
    r_P = b_P - y_P;   d_P = a_PP phi_P, or 0 where the row stores no diagonal.
The reference sums are taken in np.longdouble.  A device sum of n non-negative terms in ANY association lies within
n EPS sum(term) of the exact sum (EPS = 2^-53: each of the at most n - 1 additions a term passes through rounds once); the sum of
squares has one more rounding per term, the square's own: (n + 1) EPS sum(term).  The maxima lose nothing."""
import numpy as np

EPS = 2.0 ** -53
N = 20  # ORC_RESIDUAL_N
L1, SCALE, SQ, MAX, C_L1, C_SQ, C_MAX, C_SCALE, SCALED, C_SCALED = 0, 3, 6, 9, 12, 13, 14, 15, 16, 19


def momentum(values, b, field, pattern, n_rows=None):
    """(r, d) per row of one system; pattern = (row_ptr, col) of Mesh.matrix_pattern(); n_rows: the owned rows (default: all)"""
    row_ptr, col = (np.asarray(x, dtype=np.int64) for x in pattern)
    n = len(row_ptr) - 1 if n_rows is None else int(n_rows)
    values, b, field = (np.asarray(x, dtype=np.float64) for x in (values, b, field))
    start, lens = row_ptr[:n], np.diff(row_ptr)[:n]
    acc, d = np.zeros(n), np.zeros(n)
    rows = np.arange(n, dtype=np.int64)
    for k in range(int(lens.max()) if n else 0):
        live = lens > k
        idx = start[live] + k
        t = values[idx] * field[col[idx]]
        acc[live] = acc[live] + t
        on_diag = col[idx] == rows[live]
        d[rows[live][on_diag]] = t[on_diag]
    return b[:n] - acc, d


def sums(x):
    """(sum |x|, sum x^2, max |x|) with the sums in long double; the squares are the doubles the kernel squares"""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    return float(np.sum(a.astype(np.longdouble))), float(np.sum((x * x).astype(np.longdouble))), (float(np.max(a)) if len(a) else 0.0)


def momentum_slots(systems):
    """slots 0..11 of a record from [(r, d)] of u, v, w, and the bound of every slot (0 for the maxima: exact)"""
    rec, bound = np.zeros(N), np.zeros(N)
    for k, (r, d) in enumerate(systems):
        n = len(r)
        l1, sq, mx = sums(r)
        sc = sums(d)[0]
        rec[L1 + k], rec[SCALE + k], rec[SQ + k], rec[MAX + k] = l1, sc, sq, mx
        bound[L1 + k], bound[SCALE + k], bound[SQ + k] = n * EPS * l1, n * EPS * sc, (n + 1) * EPS * sq
    return rec, bound


def continuity_slots(b_p, n_rows=None):
    """slots 12..14 from the right-hand side of the pressure correction (owned rows), and their bounds"""
    b_p = np.asarray(b_p, dtype=np.float64)
    b_p = b_p if n_rows is None else b_p[:int(n_rows)]
    rec, bound = np.zeros(N), np.zeros(N)
    rec[C_L1], rec[C_SQ], rec[C_MAX] = sums(b_p)
    bound[C_L1], bound[C_SQ] = len(b_p) * EPS * rec[C_L1], (len(b_p) + 1) * EPS * rec[C_SQ]
    return rec, bound


def finish(history):
    """slots 15..19 of every record of a history (k, 20) from its slots 0..14: plain double arithmetic, so exact"""
    h = np.array(history, dtype=np.float64, copy=True).reshape(-1, N)
    scale = 0.0
    for i in range(len(h)):
        if i < 5 and (i == 0 or h[i, C_L1] > scale):
            scale = h[i, C_L1]
        h[i, C_SCALE] = scale
        for k in range(3):
            h[i, SCALED + k] = h[i, L1 + k] if h[i, SCALE + k] == 0.0 else h[i, L1 + k] / h[i, SCALE + k]
        h[i, C_SCALED] = 0.0 if scale == 0.0 else h[i, C_L1] / scale
    return h
