"""The inputs and the references of tests/test_gpu_gs_cases.py, guarded without a GPU: every claim of the case table
(tests/gs_cases.py) is derived here from the matrix itself, and the numpy restatements (tests/gs_restatement.py) are checked
against independent mathematics — one sweep with omega = 1 in colour order IS the forward substitution
(D + L_pi) x = b - U_pi x0 on the colour-permuted matrix — so that bit equality with them on the GPU means something.

Also recorded here, where anyone can see it without a GPU: the colouring rule that looks at a row's own line alone
(gs_restatement.color_today, the library's rule before this suite) is proper on every structurally symmetric case and IMPROPER
on G1, G2 and G4, whose rows have in-neighbours they do not store; the library's rule (color_proper) is proper on all of them
and equal to color_today on the symmetric ones.  orc_amd is not imported."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

import gs_cases as G
import gs_restatement as R

IDS = [c.name for c in G.G_CASES]


@pytest.fixture(scope="module")
def colors():
    """proper colourings by the restatement, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.color_proper(G.CASES[name].build())
        return cache[name]

    return get


def test_table_is_complete():
    names = " ".join(IDS)
    for want in ("G1_", "G2_", "G3_", "G4_", "G5_", "G6_", "G7_", "G8_tridiagonal_1 ", "G8_tridiagonal_63", "G8_tridiagonal_64", "G8_tridiagonal_65", "G9_"):
        assert want in names + " ", want
    assert len(set(IDS)) == len(IDS) == 12
    assert set(G.SOLVABLE) == set(IDS) - {G.ERROR_CASE}
    assert set(G.SYMMETRIC) | set(G.NOT_SYMMETRIC) == set(G.SOLVABLE) and not set(G.SYMMETRIC) & set(G.NOT_SYMMETRIC)
    assert set(G.BICG_CASES) | set(G.CONVERGENCE_COUNTS) | set(G.MULTIGRID_CASES) <= set(G.SOLVABLE)
    for f in (G, R):
        src = open(f.__file__).read()
        assert "import orc_amd" not in src and "from orc_amd" not in src, "table and restatement derive nothing from the library"


@pytest.mark.parametrize("case", G.G_CASES, ids=IDS)
def test_matrix_is_well_formed(case):
    a = case.build()
    n = case.n
    assert a.shape == (n, n) and a.has_sorted_indices
    assert G.is_structurally_symmetric(a) == case.symmetric
    lens = np.diff(a.indptr)
    rid = np.repeat(np.arange(n), lens)
    assert np.isfinite(a.data).all() and (a.data != 0).all()
    has_diag = np.bincount(rid[a.indices == rid], minlength=n) == 1
    assert has_diag.sum() == n - ("empty_row" in case.claims) and (has_diag | (lens == 0)).all(), "a diagonal in every non-empty row"
    row_off = np.zeros(n)
    np.add.at(row_off, rid, np.where(a.indices == rid, 0.0, np.abs(a.data)))
    assert (a.diagonal()[has_diag] > row_off[has_diag]).all(), "strictly diagonally dominant"
    assert (a.data[a.indices != rid] < 0).all(), "negative off-diagonals"
    _, b, x0 = G.system(case.name)
    assert len(b) == len(x0) == n and not np.array_equal(b, x0) and (x0 != 0).all()


@pytest.mark.parametrize("case", G.G_CASES, ids=IDS)
def test_structural_claims(case):
    a, cl, n = case.build(), case.claims, case.n
    lens = np.diff(a.indptr)
    if "row_lens" in cl:  # G1: rows of 1 ... 13 entries, every length present
        assert set(lens) == set(range(cl["row_lens"][0], cl["row_lens"][1] + 1))
        assert (lens % 8 != 0).any() and (lens > 8).any(), "widths that are no multiple of the chunk, rows longer than one chunk"
    if "diagonal_only_slice" in cl:
        s = cl["diagonal_only_slice"]
        assert (lens[64 * s:64 * s + 64] == 1).all()
    if "last_slice_live" in cl:
        assert n - 64 * ((n + 63) // 64 - 1) == cl["last_slice_live"]
    if "full_rows" in cl:  # G2
        assert tuple(np.flatnonzero(lens == cl["full_row_len"])) == cl["full_rows"] and cl["full_row_len"] == n
        assert divmod(n, 8) == cl["chunks_plus"]
        assert max(lens[[r for r in range(n) if r not in cl["full_rows"]]]) <= 3
        adj = (a + a.T).tocsr()
        for r in cl["full_rows"]:
            assert len(adj[r].indices) == n, "neighbours every row"
    if cl.get("ragged"):  # G3: G1's pattern united with its transpose, still ragged
        g1 = G.CASES["G1_short_ragged"].build()
        want = ((abs(g1) + abs(g1.T)) != 0).tocsr()
        assert ((a != 0) != want).nnz == 0
        assert len(set(lens)) > 8 and (lens % 8 != 0).any() and (lens > 8).any()
    if "unseen_in_neighbour_rows" in cl:  # G4: row r stores r - 1 only; r + 1 stores r
        assert (a != 0).tolil().rows.tolist() == [[0]] + [[r - 1, r] for r in range(1, n)]
        seen = {(i, j) for i, j in zip(*a.nonzero())}
        assert sum(1 for r in range(n) if any((j, r) in seen and (r, j) not in seen for j in (r - 1, r + 1))) == cl["unseen_in_neighbour_rows"]
    if "clique" in cl:  # G5 / G6
        m = cl["clique"]
        assert (a[:m, :m] != 0).nnz == m * m, "a dense block"
        tail = a[m:, :].tocsr()
        assert (np.diff(tail.indptr) <= 3).all() and n - m == 37
        assert (abs(a - sp.tril(sp.triu(a, -1), 1))[m:, :]).nnz == 0, "the tail is tridiagonal"
        c = R.color_today(a)
        if cl["colors"] is None:
            assert c is None and R.color_proper(a) is None, "65 rows that all neighbour each other need 65 colours"
        else:
            assert int(c.max()) + 1 == cl["colors"] == 64
            counts = np.bincount(c, minlength=64)
            lo, hi = cl["single_row_colors"]
            assert (counts[lo:hi + 1] == 1).all() and counts[:lo].sum() == n - (hi - lo + 1)
            assert int(((counts + 63) // 64).sum()) == cl["slices"], "64 slices hold 101 rows"
            assert (counts < 64).all()
    if "row_blocks" in cl:  # G7
        assert (n + 63) // 64 == cl["row_blocks"] > 1024 and n - 64 * (cl["row_blocks"] - 1) == cl["last_block_live"]
        c = R.color_today(a)
        counts = np.bincount(c)
        slices = int(((counts + 63) // 64).sum())
        print("G7: %d colours, rows per colour %s, %d colour-sorted slices" % (len(counts), counts.tolist(), slices))
        assert slices >= cl["min_slices"] > 1024, "both one-workgroup scans take their carry branch"
        offs = sorted(set((a.tocoo().col - a.tocoo().row).tolist()))
        assert tuple(offs) == G.BAND_OFFSETS
    if cl.get("tridiagonal"):  # G8
        assert (abs(a - sp.tril(sp.triu(a, -1), 1))).nnz == 0 and a.nnz == max(3 * n - 2, 1)
        if n > 1:
            counts = np.bincount(R.color_today(a))
            print("G8 n = %d: rows per colour %s" % (n, counts.tolist()))
            assert (counts < 64).all(), "every colour is one partly filled slice"
    if "empty_row" in cl:  # G9
        r = cl["empty_row"]
        g3 = G.CASES["G3_short_ragged_sym"].build()
        assert r == 70 and lens[r] == 0 and (np.delete(lens, r) > 0).all(), "the one empty row"
        keep = np.arange(n) != r
        assert (a[keep] != g3[keep]).nnz == 0, "every other row is G3's"
        assert a[:, r].nnz == g3[:, r].nnz - 1, "nothing but the row's own entries left with it"


def test_tridiagonal_sizes_straddle_one_slice():
    """G8: with n = 63, 64, 65 the row blocks are below, at and above one 64-row block; n = 1 has no off-diagonal at all"""
    assert G.TRIDIAGONAL_N == (1, 63, 64, 65)
    assert G.CASES["G8_tridiagonal_1"].build().nnz == 1
    assert [(n + 63) // 64 for n in G.TRIDIAGONAL_N] == [1, 1, 1, 2]


# ------------------------------------------------------------------ the colouring rules
@pytest.mark.parametrize("name", G.SYMMETRIC)
def test_own_line_rule_is_proper_on_symmetric_patterns(name):
    a = G.CASES[name].build()
    c = R.color_today(a)
    assert c is not None and R.is_proper(a, c)
    assert np.array_equal(np.unique(c), np.arange(c.max() + 1)), "colours 0 ... nc - 1, none empty"
    assert np.array_equal(c, R.color_proper(a)), "the library's rule leaves a symmetric pattern's colouring as it was"


@pytest.mark.parametrize("name", G.NOT_SYMMETRIC)
def test_own_line_rule_is_improper_without_symmetry(name):
    """THE DEFECT: a stored a_ij whose mirror a_ji is not stored — i sees j, j never sees i — leaves both in one colour when i has
    the higher priority or was coloured in an earlier round.  The library's rule settles the pair from i's side."""
    a = G.CASES[name].build()
    c = R.color_today(a)
    coo = a.tocoo()
    off = coo.row != coo.col
    inside = int(np.sum(c[coo.row[off]] == c[coo.col[off]]))
    print("%s: own-line rule %d colours, %d stored off-diagonals inside a colour" % (name, c.max() + 1, inside))
    assert inside > 0 and not R.is_proper(a, c)
    p = R.color_proper(a)
    assert R.is_proper(a, p) and p.max() + 1 <= 64
    assert np.array_equal(np.unique(p), np.arange(p.max() + 1))


def test_own_line_rule_matches_a_scalar_reading():
    """the vectorised rounds against a row-by-row reading of the same rule, on a case of every kind"""
    def scalar(a):
        n = a.shape[0]
        h = [int(v) for v in R.hash32(np.arange(n))]
        greater = lambda p, q: h[p] > h[q] or (h[p] == h[q] and p > q)  # noqa: E731
        col = [-1] * n
        while True:
            tent = list(col)
            for i in range(n):
                if col[i] < 0:
                    used = 0
                    for j in a.indices[a.indptr[i]:a.indptr[i + 1]]:
                        if j != i and col[j] >= 0:
                            used |= 1 << col[j]
                    tent[i] = next(c for c in range(65) if not used >> c & 1)
                    if tent[i] == 64:
                        return None
            out = list(tent)
            for i in range(n):
                if col[i] < 0 and any(j != i and col[j] < 0 and tent[j] == tent[i] and greater(j, i) for j in a.indices[a.indptr[i]:a.indptr[i + 1]]):
                    out[i] = -1
            col = out
            if min(col) >= 0:
                return np.array(col)

    for name in ("G1_short_ragged", "G4_bidiagonal", "G5_clique64", "G6_clique65", "G8_tridiagonal_65", "G9_empty_row"):
        a = G.CASES[name].build()
        want, got = scalar(a), R.color_today(a)
        assert (want is None and got is None) or np.array_equal(want, got), name
    fv = G.fv_like_matrix(9, 7, 5)
    assert np.array_equal(scalar(fv), R.color_today(fv)) and int(R.color_today(fv).max()) == 4


# ------------------------------------------------------------------ the sweep against forward substitution
@pytest.mark.parametrize("name,pre", [pytest.param(n, p, id="%s-%s" % (n, "jacobi" if p else "none")) for n in G.SOLVABLE for p in G.preconditioners(n)])
def test_sweep_is_forward_substitution_in_colour_order(name, pre, colors):
    """omega = 1: x_new = (D + L_pi)^-1 (b - U_pi x0), pi = colour order; the bound comes from the two CPU computations (each row
    adds at most n_row_max products: 64 n_row_max 2^-53 of the solution's size)"""
    a, b, x0 = G.system(name)
    n = a.shape[0]
    c = colors(name)
    scale = G.jacobi_scale(a) if pre else None
    got = R.sweep(a, b, x0, 1.0, c, scale)
    a2, b2 = a.tocsr(), b.copy()
    if pre:
        a2, b2 = sp.diags(scale) @ a2, scale * b2
    empty = np.flatnonzero(np.diff(a.indptr) == 0)
    if len(empty):  # an empty row is skipped: x keeps its value — the identity row says the same
        a2 = (a2 + sp.csr_matrix((np.ones(len(empty)), (empty, empty)), shape=a.shape)).tocsr()
        b2[empty] = x0[empty]
    order = np.argsort(c, kind="stable")
    ap = a2[order][:, order].tocsr()
    lower, upper = sp.tril(ap, 0, format="csr"), sp.triu(ap, 1, format="csr")
    want = np.empty(n)
    want[order] = spsolve_triangular(lower, b2[order] - upper @ x0[order], lower=True)
    n_row_max = int(np.diff(a.indptr).max())
    err = np.abs(got - want).max() / np.abs(want).max()
    bound = 64 * n_row_max * 2.0 ** -53
    assert err < bound, "%s: %.3e against %.3e (n_row_max %d)" % (name, err, bound, n_row_max)


def test_sweep_equals_the_row_by_row_loop_bit_for_bit(colors):
    """the vectorised sweep against test_gpu_gauss_seidel.gs_numpy's scalar loop (rows one after another in colour order), with
    relaxation and scaling, on ragged rows"""
    def gs_numpy(a, b, x, sweeps, omega, cols, scale=None):
        x = x.copy()
        for _ in range(sweeps):
            for i in np.argsort(cols, kind="stable"):
                s, d = 0.0, None
                for q in range(a.indptr[i], a.indptr[i + 1]):
                    j = a.indices[q]
                    v = a.data[q] if scale is None else scale[i] * a.data[q]
                    if j == i:
                        d = v
                        s += 0.0
                    else:
                        s += v * x[j]
                if d is None:
                    continue
                bi = b[i] if scale is None else 0.0 + scale[i] * b[i]
                x[i] = x[i] * (1.0 - omega) + omega * (bi - s) / d
        return x

    # an improper colouring: the restatement still means "row after row in colour order" (and no longer what a launch per colour gives)
    a, b, x0 = G.system("G4_bidiagonal")
    bad = R.color_today(a)
    assert not R.is_proper(a, bad)
    assert np.array_equal(R.sweep(a, b, x0, 0.8, bad).view(np.uint64), gs_numpy(a, b, x0, 1, 0.8, bad).view(np.uint64))
    for name in ("G1_short_ragged", "G2_long_ragged", "G9_empty_row"):
        a, b, x0 = G.system(name)
        for pre in G.preconditioners(name):
            scale = G.jacobi_scale(a) if pre else None
            x = x0
            for _ in range(2):
                x = R.sweep(a, b, x, 0.8, colors(name), scale)
            assert np.array_equal(x.view(np.uint64), gs_numpy(a, b, x0, 2, 0.8, colors(name), scale).view(np.uint64)), (name, pre)


# ------------------------------------------------------------------ the BiCGSTAB restatement
@pytest.mark.parametrize("pre", [G.PRE_NONE, G.PRE_JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("name", sorted(G.CONVERGENCE_COUNTS))
def test_reference_solves_the_convergence_cases(name, pre, colors):
    """from zero with b = A xs, the exactly-summed restatement reaches a relative residual below 1e-8 (and xs within 1e-8) in the
    table's count: agreement with it means agreement with something that solves the system"""
    a, b, xs = G.convergence_system(name)
    its = G.CONVERGENCE_COUNTS[name]
    x = R.bicgstab_gs(a, b, np.zeros(len(xs)), its, colors(name), G.jacobi_scale(a) if pre else None, sums=math.fsum)
    res = np.linalg.norm(b - a @ x) / np.linalg.norm(b)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print("%s pre %d: relative residual %.3e, error %.3e after %d iterations" % (name, pre, res, err, its))
    assert np.isfinite(x).all() and res < 1e-8 and err < 1e-8


@pytest.mark.parametrize("pre", [G.PRE_NONE, G.PRE_JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("name", G.BICG_CASES)
def test_three_iterations_stay_finite_and_depend_little_on_the_summation(name, pre, colors):
    """what the GPU test's bound is made of: d_ref, the distance between exactly rounded sums and numpy's pairwise sums"""
    a, b, x0 = G.system(name)
    scale = G.jacobi_scale(a) if pre else None
    xf = R.bicgstab_gs(a, b, x0, G.BICG_ITERATIONS, colors(name), scale, sums=math.fsum)
    xn = R.bicgstab_gs(a, b, x0, G.BICG_ITERATIONS, colors(name), scale, sums=np.sum)
    d_ref = np.linalg.norm(xf - xn) / np.linalg.norm(xf)
    print("%s pre %d: d_ref %.3e, n 2^-53 %.3e" % (name, pre, d_ref, a.shape[0] * 2.0 ** -53))
    assert np.isfinite(xf).all() and np.isfinite(xn).all() and not np.array_equal(xf, x0)
    assert d_ref < 1e-9, "a reference whose own summation order moved it this far would bound nothing"
