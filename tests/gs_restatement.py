"""Plain numpy restatements of what orc_amd/csrc/gs_*.hip compute (colouring: gs_coloring.hip, sweep and row-space arm: gs_sweep.hip), for tests/test_gs_cases_cpu.py and tests/test_gpu_gs_cases.py.
The library is not imported.

  color_today(a)    the colouring rule that looks at a row's own line alone (the rule of the library before it learned about
                    patterns that are not structurally symmetric): proper on symmetric patterns, whose colourings it pins
  color_proper(a)   the library's rule: the same rounds, plus the knock-out stores and the forbidden-colour mask
  sweep(...)        one multicolour Gauss-Seidel sweep, bit for bit the kernels' arithmetic
  bicgstab_gs(...)  the Gauss-Seidel-preconditioned BiCGSTAB recurrences of the row-space arm
  is_proper(a, c)   no stored off-diagonal entry inside a colour
"""
import math

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def hash32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def _priority(n):
    """prio_greater(a, b) == key[a] > key[b]: the hash, then the row index"""
    i = np.arange(n, dtype=np.uint64)
    return (hash32(i) << np.uint64(32)) | i


def _color(a, knock_out):
    a = a.tocsr()
    n = a.shape[0]
    lens = np.diff(a.indptr)
    rid = np.repeat(np.arange(n, dtype=np.int64), lens)
    cj = a.indices.astype(np.int64)
    off = rid != cj
    rid, cj = rid[off], cj[off]
    key = _priority(n)
    one = np.uint64(1)
    col = np.full(n, -1, dtype=np.int64)
    forbid = np.zeros(n, dtype=np.uint64)
    for _ in range(10000):
        new = col < 0
        # assign: the smallest colour outside the final colours of the stored neighbours (and the forbidden mask)
        used = forbid.copy()
        m = new[rid] & (col[cj] >= 0)
        np.bitwise_or.at(used, rid[m], one << col[cj[m]].astype(np.uint64))
        free = ~used
        if (free[new] == 0).any():
            return None
        low = free & (~free + one)  # lowest set bit; a power of two is exact in float64
        tent = np.where(new, np.log2(low.astype(np.float64)).astype(np.int64), col)
        # resolve
        same = new[cj] & (tent[cj] == tent[rid])
        lose = np.zeros(n, dtype=bool)
        both = same & new[rid]
        lose[rid[both & (key[cj] > key[rid])]] = True
        if knock_out:
            lose[cj[both & ~(key[cj] > key[rid])]] = True
            fin = same & ~new[rid]
            lose[cj[fin]] = True
            np.bitwise_or.at(forbid, cj[fin], one << tent[rid[fin]].astype(np.uint64))
        col = np.where(new & lose, -1, tent)
        if not (col < 0).any():
            return col.astype(np.int32)
    raise RuntimeError("colouring did not finish")


def color_today(a):
    """Jacobi-style assign and resolve rounds over a row's OWN line: the smallest free colour of a 64-bit mask, conflicts of a
    round settled by the hash32 priority with the row index as tie-break.  None: more than 64 colours."""
    return _color(a, False)


def color_proper(a):
    """color_today plus what makes the result proper on A united with its transpose: a row that sees a conflict settles it
    for the row that cannot see it (a flag), and a final row's colour enters that row's forbidden mask"""
    return _color(a, True)


def is_proper(a, colors):
    coo = a.tocoo()
    off = coo.row != coo.col
    colors = np.asarray(colors)
    return bool(np.all(colors[coo.row[off]] != colors[coo.col[off]]))  # (a_ij and a_ji: the test is symmetric in i, j)


def _row_sums(rp, ci, val, lens, rows, x, skip_diag, scale=None):
    """sum_k v_k x[c_k] of the rows `rows`, every sum from 0.0 in ascending-column order, one multiply and one add per entry;
    the diagonal adds the literal 0.0 where skip_diag"""
    acc = np.zeros(len(rows))
    live = np.arange(len(rows))
    k = 0
    live = live[lens[rows] > 0]
    while len(live):
        r = rows[live]
        p = rp[r] + k
        j = ci[p]
        v = val[p] if scale is None else scale[r] * val[p]
        term = v * x[j]
        if skip_diag:
            term = np.where(j == r, 0.0, term)
        acc[live] = acc[live] + term
        k += 1
        live = live[lens[r] > k]
    return acc


def sweep(a, b, x, omega, colors, scale=None, rhs_scaled=False):
    """x_i = x_i (1 - w) + w (b_i - sum_{j != i} a_ij x_j) / a_ii, Gauss-Seidel in colour order: colour after colour, inside a colour
    row after row.  Rows of a colour that no stored entry joins do not see each other's updates, so they are taken at once
    (vectorised); a colour with such an entry — an improper colouring — is walked row by row, which is what a sweep in that
    order means and what no parallel launch over the colour computes.  Rows without entries are skipped.  With a Jacobi
    scaling the entries are scale[i] * a_ij and the right-hand side is 0.0 + scale[i] * b_i (rhs_scaled: b is a vector of the
    scaled system already, as the residuals the preconditioner is applied to are).  No fused multiply-add."""
    a = a.tocsr()
    n = a.shape[0]
    rp, ci, val = a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data
    lens = np.diff(rp)
    rid = np.repeat(np.arange(n, dtype=np.int64), lens)
    dpos = np.full(n, -1, dtype=np.int64)
    at = np.flatnonzero(ci == rid)
    dpos[rid[at]] = at
    assert ((dpos >= 0) | (lens == 0)).all(), "a non-empty row without a diagonal is an error of the arm, not a case of this restatement"
    x = np.array(x, dtype=np.float64)
    colors = np.asarray(colors)
    coupled = set(colors[rid[(rid != ci) & (colors[rid] == colors[ci])]].tolist())
    for c in range(int(colors.max()) + 1 if n else 0):
        rows = np.flatnonzero((colors == c) & (lens > 0))
        for part in ([rows[k:k + 1] for k in range(len(rows))] if c in coupled else [rows] if len(rows) else []):
            s = _row_sums(rp, ci, val, lens, part, x, True, scale)
            d = val[dpos[part]] if scale is None else scale[part] * val[dpos[part]]
            bi = b[part] if scale is None or rhs_scaled else 0.0 + scale[part] * b[part]
            x[part] = x[part] * (1.0 - omega) + omega * (bi - s) / d
    return x


def product(a, x, scale=None):
    a = a.tocsr()
    rp = a.indptr.astype(np.int64)
    return _row_sums(rp, a.indices.astype(np.int64), a.data, np.diff(rp), np.arange(a.shape[0], dtype=np.int64), x, False, scale)


def bicgstab_gs(a, b, x0, its, colors, scale=None, sums=math.fsum):
    """The recurrences of the row-space arm (gs_arm_dev): r = b - A x, p = r, rho = sum(r); per iteration p^ = M^-1 p, nu = A p^,
    alpha = rho / sum(nu), s = r - alpha nu, s^ = M^-1 s, t = A s^, omega = (t.s) / (t.t), x = (x + alpha p^) + omega s^,
    r = s - omega t, rho' = sum(r), beta = rho' / rho * alpha / omega, p = r + beta (p - omega nu).  M^-1 is one sweep from zero
    with omega = 1.  `sums` takes the four reductions: math.fsum (exactly rounded) or np.sum."""
    n = a.shape[0]
    bs = b if scale is None else 0.0 + scale * b
    zero = np.zeros(n)
    x = np.array(x0, dtype=np.float64)
    r = bs - product(a, x, scale)
    p = r.copy()
    rho = float(sums(r))
    for _ in range(its):
        ph = sweep(a, p, zero, 1.0, colors, scale, rhs_scaled=True)
        nu = product(a, ph, scale)
        alpha = rho / float(sums(nu))
        s = r - alpha * nu
        sh = sweep(a, s, zero, 1.0, colors, scale, rhs_scaled=True)
        t = product(a, sh, scale)
        omega = float(sums(t * s)) / float(sums(t * t))
        x = (x + alpha * ph) + omega * sh
        r = s - omega * t
        rho_new = float(sums(r))
        beta = rho_new / rho * alpha / omega
        p = r + beta * (p - omega * nu)
        rho = rho_new
    return x

