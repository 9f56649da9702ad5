"""Guards the case table of tests/bicg_cases.py and the restatement of tests/bicg_restatement.py.  CPU only.

  * every case: the longdouble result is finite and d_case <= 1e-10.  The cap is a condition on the inputs, not a measurement: a
    case that breaks it is changed (fewer iterations, another seed), never the cap;
  * every iterate case: a restatement that leaves the last element out of every sum, and one that leaves one chunk of 512
    elements out, end more than 1e6 x 50 d_case from the longdouble result — the device bound of tests/test_gpu_bicg.py can see a
    lost tail or a lost partial sum with six orders of magnitude to spare.  (The lost chunk applies to sums over more than one
    chunk: it is asserted for n > 512; on the Multigrid cases the coarse levels of 512 rows or fewer keep their sums.);
  * every boundary the docstring of bicg_cases claims is recomputed from the grid formulas, whose constants are pinned to the sources;
  * the restatement in the oracle's own association is the oracle bit for bit: BiCGSTAB with and without the preconditioner, a
    matrix with empty rows and rows without a diagonal, and the Multigrid arm."""
import os
import re

import numpy as np
import pytest

import bicg_cases as G
import bicg_restatement as R
import product_cases as PC
from conftest import ROOT, fv_like_matrix, splitmix64_uniform

CAP = 1e-10
SEPARATION = 1e6
BICGSTAB, MULTIGRID = 3, 2


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("c", G.ITERATE_CASES, ids=G.case_id)
def test_case_is_determined_to_rounding(c):
    x, d = G.references(c)
    assert np.isfinite(x.astype(np.float64)).all()
    assert d <= CAP, d


def check_far(label, x_wrong, x_ld, d_case):
    far = G.rel(x_wrong, x_ld) if np.isfinite(x_wrong).all() else np.inf
    print("%s: %.3e from the longdouble result, bound %.3e" % (label, far, G.BOUND * d_case))
    assert far > SEPARATION * G.BOUND * d_case, (label, far, d_case)


@pytest.mark.parametrize("c", G.ITERATE_CASES, ids=G.case_id)
def test_a_lost_tail_or_partial_sum_is_far_outside_the_bound(c):
    x, d = G.references(c)
    check_far("last element lost", G.run(c, np.float64, R.Sums("pairwise", drop="last"))[c.iterations], x, d)
    if len(x) > R.CHUNK:
        check_far("one chunk lost", G.run(c, np.float64, R.Sums("chunk", drop="block"))[c.iterations], x, d)


@pytest.mark.parametrize("c", G.MG_CASES, ids=G.case_id)
def test_multigrid_case_is_determined_and_sees_a_lost_tail_or_partial_sum(oracle, c):
    x, d = G.mg_references(oracle, c)
    assert np.isfinite(x.astype(np.float64)).all()
    assert d <= CAP, d
    check_far("last element lost", G.mg_run(oracle, c, np.float64, R.Sums("pairwise", drop="last")), x, d)
    check_far("one chunk lost", G.mg_run(oracle, c, np.float64, R.Sums("chunk", drop="block")), x, d)


def test_table_covers_what_it_says():
    chains = {c.key[0] for c in G.SMALL_CASES if c.key[1:] == (1, 1)}
    assert chains == set(G.CHAINS)
    assert {c.key for c in G.SMALL_CASES} >= set(G.SHAPES)
    for c in G.SMALL_CASES:
        assert c.iterations in G.ITERATIONS and c.iterations < np.prod(c.key)
    assert {(np.prod(c.key), c.iterations) for c in G.SMALL_CASES if np.prod(c.key) > 8} == {(n, k) for n in list(G.CHAINS[2:]) + [105, 715, 195] for k in G.ITERATIONS}
    for key in ("precond", "x0"):
        assert {getattr(c, key) for c in G.SMALL_CASES} == {0, 1}
        assert {getattr(c, key) for c in G.BAND_CASES} == {0, 1}
    # both sides of the materialisation threshold under the preconditioner
    assert {c.iterations for c in G.SMALL_CASES if c.precond} == set(G.ITERATIONS) and PC.BICG_ON_THE_FLY < 4 <= PC.BICG_MATERIALISED
    want = {(s.name, p, k) for s in PC.S_CASES for p in (0, 1) for k in (3, 8)}
    got = {(c.key, c.precond, c.iterations) for c in G.USER_CASES}
    # three runs lowered (docstring of bicg_cases); under Jacobi each system still has a run on either side of the materialisation threshold
    assert got - want == {("S2_long_ragged", 0, 2), ("S2_long_ragged", 1, 6), ("S4_far_short_ragged", 1, 6)}
    assert want - got == {("S2_long_ragged", 0, 8), ("S2_long_ragged", 1, 8), ("S4_far_short_ragged", 1, 8)}
    for s in PC.S_CASES:
        ks = {k for name, p, k in got if name == s.name and p == 1}
        assert min(ks) < 4 <= max(ks)
    assert {(c.key, c.iterations, c.precond) for c in G.MG_CASES} == {(s, k, 1) for s in ((20, 17, 9), (64, 40, 12)) for k in (3, 5)}
    assert {c.iterations for c in G.BAND_CASES} == {1, 3} and len(G.BAND_CASES) == 2 * len(G.BAND_SHAPES)
    assert len({G.case_id(c) for c in G.ITERATE_CASES + G.MG_CASES + G.GUARD_CASES}) == len(G.ITERATE_CASES + G.MG_CASES + G.GUARD_CASES)


# ------------------------------------------------------------------ the launch geometry
def test_grid_formulas_are_the_sources():
    src = lambda name: open(os.path.join(ROOT, "orc_amd", "csrc", name)).read()
    common, spmv, bicg, kernels = src("common.hpp"), src("spmv.hip"), src("bicgstab.hip"), src("linalg_kernels.hpp")
    assert re.search(r"constexpr int kBlock = %d;" % G.K_BLOCK, common) and re.search(r"constexpr int kMaxGrid = %d;" % G.K_MAX_GRID, common)
    assert "constexpr int kMaxPartials = kMaxGrid;" in common
    assert "return clamp_partials_grid((work_items + per_block - 1) / per_block);" in common
    assert "int64_t g = ((int64_t)n_slices + 3) / 4;" in spmv and "if (g >= 8) g = (g / 8) * 8;" in spmv
    assert bicg.count("grid_for((n + 1) / 2)") == 2  # the one-system and the lock-step iteration
    # the fold: 16 virtual wavefronts, virtual thread vt adds partials[vt] and partials[vt + 1024]
    assert kernels.count("const int vt = (w + 4 * p) * 64 + lane;") == 4 and "vt + 1024 < count ? partials[vt + 1024]" in kernels


def test_every_boundary_of_the_band_sizes():
    vg, pg = G.vector_grid, G.product_grid
    assert all(np.prod(s) % 2 == 1 for s in G.BAND_SHAPES)
    n = [int(np.prod(s)) for s in G.BAND_SHAPES]
    # 32 769: the vector kernels' sums fill 64 virtual threads = one virtual wavefront of the fold up to 32 768 rows
    assert (vg(n[0] - 1), vg(n[0])) == (64, 65)
    # 263 937: the first product grid above 1024 partial sums (1025 ... 1031 are rounded down to 1024)
    assert (pg(n[1] - 1), pg(n[1])) == (1024, 1032) and pg(262_145) == 1024
    # 524 289: the product grid is clamped, and the vector kernels' sums pass 1024
    assert (pg(n[2] - 1), pg(n[2])) == (2048, 2048) and -(-n[2] // 64) == 8193 > 4 * 2048 >= -(-(n[2] - 1) // 64)
    assert (vg(n[2] - 1), vg(n[2])) == (1024, 1025)
    # 1 048 579: clamp and second pass; 1 048 577 is clamped but covered by one pass and the tail
    assert vg(1_048_576) == 2048 and -(-((1_048_577 + 1) // 2) // 256) == 2049
    assert G.vector_passes(1_048_577) == (1, True) and G.vector_passes(n[3]) == (2, True)
    assert (n[3] >> 1) - 2048 * 256 == 1
    # 129 x 129 x 127: two full passes, 8 127 pairs in the third, the tail
    assert n[4] == 2_113_407 > 2_097_152 and G.vector_passes(n[4]) == (3, True) and (n[4] >> 1) - 2 * 2048 * 256 == 8127
    # the lock-step and guard size of test_gpu_bicg.py: odd, grid clamped, per-element loops of the mixed-state branches in three passes
    m = int(np.prod(G.LOCKSTEP_SHAPE))
    assert m == 1_048_577 and vg(m) == 2048 and -(-m // (2048 * 256)) == 3
    assert int(np.prod(G.GUARD3_SHAPES[0])) == 715
    # the lock-step runs: 1 048 577 rows with both preconditioners, and the first odd size with a second pass of the pair loops
    assert G.LOCKSTEP_RUNS == ((G.LOCKSTEP_SHAPE, 0), (G.LOCKSTEP_SHAPE, 1), (G.BAND_SHAPES[3], 0))


# ------------------------------------------------------------------ the restatement is the algorithm
def test_oracle_association_in_numpy_is_or_dot(oracle):
    S = R.Sums("oracle")
    for n in list(range(0, 20)) + [105, 1000, 1009]:
        u, v = splitmix64_uniform(n, 3), splitmix64_uniform(n, 4)
        assert S.dot(u, v) == oracle.dot(u, v) and S.sum(u) == oracle.dot(u, np.ones(n))


@pytest.mark.parametrize("shape,iters,precond", [((7, 5, 3), 8, 1), ((65, 3, 1), 3, 0)])
def test_bicgstab_in_the_oracles_association_is_the_oracle_bit_for_bit(oracle, shape, iters, precond):
    a = fv_like_matrix(*shape)
    n = a.shape[0]
    b, x0 = splitmix64_uniform(n, 11), splitmix64_uniform(n, 12)
    x, xo = x0.copy(), x0.copy()
    R.solve(a, b, x, iters, precond, np.float64, R.Sums("oracle"))
    assert oracle.iterative_solve(oracle.Csr.from_scipy(a), b, xo, iters, BICGSTAB, 0.5, 1e-3, precond) == 0
    assert np.isfinite(xo).all() and not np.array_equal(xo, x0)
    assert same_bits(x, xo)
    # and the association matters at all: numpy's pairwise sums end elsewhere
    y = x0.copy()
    R.solve(a, b, y, iters, precond, np.float64, R.Sums("pairwise"))
    assert not np.array_equal(y, xo) and G.rel(y, xo.astype(G.LD)) < 1e-9


def test_rows_without_a_diagonal_become_empty_as_in_the_oracle(oracle):
    """the scaling on product_cases' P1 (empty rows, every fifth row without a diagonal): the oracle's two iterations bit for bit,
    whatever they hold, and the longdouble product copes with the empty rows"""
    a = PC.short_ragged(False)
    n = a.shape[0]
    scaled, dinv = R.jacobi_scaled(a)
    lens, slens = np.diff(a.indptr), np.diff(scaled.indptr)
    has = np.array([a[i, i] != 0 for i in range(n)])
    assert (~has).sum() > 20 and (lens == 0).sum() >= 64
    assert np.array_equal(slens, np.where(has, lens, 0)) and np.all(dinv[~has] == 0.0)
    b, x0 = splitmix64_uniform(n, 11), 0.1 * splitmix64_uniform(n, 12)
    x, xo = x0.copy(), x0.copy()
    R.solve(a, b, x, 2, 1, np.float64, R.Sums("oracle"))
    assert oracle.iterative_solve(oracle.Csr.from_scipy(a), b, xo, 2, BICGSTAB, 0.5, 1e-3, 1) == 0
    assert same_bits(x, xo)
    v = splitmix64_uniform(n, 5)
    y = R.matvec(scaled, G.LD)(v.astype(G.LD))
    assert y.dtype == G.LD and np.all(y[slens == 0] == 0)
    assert np.abs(y.astype(np.float64) - scaled @ v).max() <= 1e-14 * np.abs(v).max() * abs(scaled).sum(axis=1).max()


@pytest.mark.parametrize("shape,iters", [((7, 5, 3), 3), ((20, 17, 9), 4)])
def test_multigrid_in_the_oracles_association_is_the_oracle_bit_for_bit(oracle, shape, iters):
    a = fv_like_matrix(*shape)
    n = a.shape[0]
    b = a @ splitmix64_uniform(n, 7)
    x0 = 0.1 * splitmix64_uniform(n, 8)
    x, xo = x0.copy(), x0.copy()
    levels = R.hierarchy(oracle, R.scaled_operator(a, 1))
    halves = [(n + 1) // 2, ((n + 1) // 2 + 1) // 2, (((n + 1) // 2 + 1) // 2 + 1) // 2]
    assert [lv[2].shape[0] for lv in levels] == halves  # three coarse levels: the cap, none of the first two has 16 rows or fewer
    R.multigrid(a, b, x, iters, 1, levels, np.float64, R.Sums("oracle"))
    assert oracle.iterative_solve(oracle.Csr.from_scipy(a), b, xo, iters, MULTIGRID, 0.5, 1e-3, 1) == 0
    assert np.isfinite(xo).all()
    assert same_bits(x, xo)


@pytest.mark.parametrize("shape,iters,coarse", [((5, 3, 1), 3, [8]), ((11, 5, 1), 2, [28, 14])])
def test_multigrid_stops_coarsening_at_16_rows(oracle, shape, iters, coarse):
    """a coarse operator of 16 rows or fewer is solved and not coarsened again: the restatement follows the oracle there too"""
    a = fv_like_matrix(*shape)
    n = a.shape[0]
    b, x0 = a @ splitmix64_uniform(n, 7), 0.1 * splitmix64_uniform(n, 8)
    levels = R.hierarchy(oracle, R.scaled_operator(a, 1))
    assert [lv[2].shape[0] for lv in levels] == coarse
    x, xo = x0.copy(), x0.copy()
    R.multigrid(a, b, x, iters, 1, levels, np.float64, R.Sums("oracle"))
    assert oracle.iterative_solve(oracle.Csr.from_scipy(a), b, xo, iters, MULTIGRID, 0.5, 1e-3, 1) == 0
    assert same_bits(x, xo) and np.isfinite(xo).all()


# ------------------------------------------------------------------ guard sizes
@pytest.mark.parametrize("c", G.GUARD_CASES, ids=G.case_id)
def test_guard_cases_have_a_direct_solution_that_bounds_them(c):
    """iterations >= n: the device is held to the direct solution within 1e-10, which needs eps x condition x iterations far
    below that: condition < 1e3 gives 2.2e-16 x 1e3 x 8 < 2e-12"""
    a, b, _ = G.system(c.kind, c.key)
    n = a.shape[0]
    assert c.iterations >= n
    assert np.linalg.cond(a.toarray()) < 1e3
    ref = np.linalg.solve(a.toarray(), b)
    assert np.isfinite(ref).all()
    # the unguarded restatement: 0 / 0 where s vanishes exactly (n = 1: the guard's x = h branch is what the device needs), and
    # where it stays finite it has reached the direct solution with a tenth of the device's bound to spare
    for kind in ("pairwise", "chunk"):
        x = G.run(c, np.float64, R.Sums(kind))[c.iterations]
        if n == 1:
            assert np.isnan(x).all()
        else:
            assert np.isfinite(x).all() and np.linalg.norm(x - ref) <= 1e-11 * np.linalg.norm(ref)
