"""BiCGSTAB and the Multigrid arm in the DEFAULT (tree) reduction order against a longdouble restatement.

Every product, the benchmark and every solve_steady run sum in the default order: per-workgroup partial sums from the product
epilogues (EpiResidual, EpiStoreSum, EpiTs), folded by their consumers (fold_partials_block, fold_partials_multi<2|3|6>,
reduce_partials_k), in-launch folds of the window products (spmv_xwin_k, XWinDev::fold_scratch), and the two-elements-per-lane
vector kernels bicg_{s,xr,p}_k / bicg_{s,xr,p}3_k with their single-element tail and their grid-stride loop.  The bit-exact
comparisons with the oracle all run in reduction_order = REFERENCE, which replaces that whole path by dot_reference_k.  Here the
default order is held to the rounding scale of each case:

    rel(x_device, x_longdouble) <= 50 d_case

with the references, d_case and the case table of tests/bicg_cases.py (restatement: tests/bicg_restatement.py).  d_case is the
larger distance of two float64 restatements (pairwise sums; partial sums over 512 elements) from the longdouble one, floored at
1e-15; 50 is the project's margin over the spread of float64 associations (tests/test_gpu_cg.py): the device's tree is one more
association of the same terms.  tests/test_bicg_cpu.py holds d_case <= 1e-10 on every case and shows that a restatement which
loses the last element, or one 512-element partial, of every sum ends more than 1e6 x 50 d_case away.

The figures that motivated these tests (float64 associations 2e-16 ... 3e-13 from longdouble, 1.1e-12 at 2 113 407 rows and 8
iterations; a lost element moving x by 3e-4 ... 9; invisible at 50 iterations) came from a scipy restatement on the CPU, not
from the device.  Measured on the MI355X, error / d_case, largest per group (the bound is 50):

    small sizes            2.47   (chain of 64, 8 iterations, no preconditioner)
    band sizes             4.99   (263 937 rows, 3 iterations, Jacobi); 32 769: 0.46, 524 289: 0.42, 1 048 579: 1.03, 2 113 407: 2.17
    user matrices          2.83   (S4, 3 iterations, "wide"); by family: narrow 0.84, generic_scaled 0.99, ragged 1.36, wide 2.83
    Multigrid arm          1.60   ((20,17,9), 3 iterations, the same in both forms of the fold); (64,40,12): 0.59 / 0.59
    lock-step              3.97   (1 048 579 rows, system 0); 1 048 577 rows: 0.98
    per-system guard       1.43   (715 rows); 1 048 577 rows: 0.40
    guard sizes            n = 1: one guard event, the direct solution in every bit; n = 2, 3: no event, 3.5e-14 and 5.7e-16 from it

No kernel was found wrong: every case is within 5 d_case.
"""
import numpy as np
import pytest

import bicg_cases as G
import product_cases as PC

pytestmark = pytest.mark.gpu
MULTIGRID, BICGSTAB = 2, 3
PRE_NONE, PRE_JACOBI = 0, 1


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def check_x(label, x, x_ref, d_case):
    err = G.rel(x, x_ref)
    print("%s: device error %.3e, d_case %.3e, ratio %.2f" % (label, err, d_case, err / d_case))
    assert np.isfinite(x).all() and err <= G.BOUND * d_case, (label, err, d_case)


def device_solve(c, method=BICGSTAB):
    from orc_amd.linear_algebra import iterative_solve
    a, b, _ = G.system(c.kind, c.key)
    x = G.start(c)
    st = iterative_solve(a, b, x, c.iterations, method, 0.5, 1e-3, c.precond, raise_on_error=False)
    return st, x


# ------------------------------------------------------------------ 1. iterates
@pytest.mark.parametrize("c", G.SMALL_CASES + G.BAND_CASES, ids=G.case_id)
def test_iterates(gpu, c):
    st, x = device_solve(c)
    assert st == 0
    check_x(G.case_id(c), x, *G.references(c))


# ------------------------------------------------------------------ 2. user matrices: each bound names its kernel
@pytest.mark.parametrize("c", G.USER_CASES, ids=G.case_id)
def test_user_matrix_iterates_by_the_family_the_table_names(gpu, c):
    """the ragged, wide, narrow and generic scaled products write their partial sums in the default order: 1 + 2 k launches of
    the one family product_cases derives from the matrix, and x within the bound"""
    from orc_amd.linear_algebra import product_launches
    product_launches(reset=True)
    st, x = device_solve(c)
    fams = {k: v for k, v in product_launches(reset=True).items() if v}
    assert st == 0
    on_the_fly = c.precond == PRE_JACOBI and c.iterations < 4
    assert fams == {PC.solve_family(PC.CASES[c.key], on_the_fly, nt=False): 1 + 2 * c.iterations}, fams
    check_x("%s [%s]" % (G.case_id(c), ", ".join(fams)), x, *G.references(c))


# ------------------------------------------------------------------ 3. Multigrid arm, both forms of the window products' fold
@pytest.mark.parametrize("c", G.MG_CASES, ids=G.case_id)
def test_multigrid_arm(gpu, oracle, monkeypatch, c):
    """ORC_XWIN_WG_PER_BLOCK=1 (a workgroup per block, the last to arrive folds the partial sums in index order), again, then 0
    (persistent workgroups, one partial sum each, folded by the consumers): both within the bound, the two runs of the first form
    identical in every bit, and the levels did get windows"""
    from orc_amd.linear_algebra import xwin_counters
    x_ld, d_case = G.mg_references(oracle, c)
    out = []
    for mode in ("1", "1", "0"):
        monkeypatch.setenv("ORC_XWIN_WG_PER_BLOCK", mode)
        xwin_counters(reset=True)
        st, x = device_solve(c, MULTIGRID)
        blocks, over_cap, over_span = xwin_counters()
        print("ORC_XWIN_WG_PER_BLOCK=%s: %d blocks described, %d / %d without a window (cap / span)" % (mode, blocks, over_cap, over_span))
        assert st == 0
        assert blocks > 0 and blocks > over_cap + over_span
        check_x("%s, ORC_XWIN_WG_PER_BLOCK=%s" % (G.case_id(c), mode), x, x_ld, d_case)
        out.append(x)
    assert same_bits(out[0], out[1])


# ------------------------------------------------------------------ 4. lock-step against the one-system solve, at size
@pytest.mark.parametrize("shape,precond", G.LOCKSTEP_RUNS, ids=lambda v: str(v[0]) if isinstance(v, tuple) else "pc%d" % v)
def test_lock_step_at_a_million_rows(gpu, shape, precond):
    """three perturbed systems on the chain of 1 048 577 rows (vector grid clamped, one pass of the pair loops, single-element
    tail) with both preconditioners, and of 1 048 579 rows (a second pass) without, 3 iterations: every system as in its
    one-system solve bit for bit, and that within the bound of its own longdouble reference"""
    from orc_amd.linear_algebra import iterative_solve, iterative_solve3
    mats, bs, xs = G.three_systems(shape)
    x3 = [x.copy() for x in xs]
    st, st3 = iterative_solve3(mats, bs, x3, 3, BICGSTAB, 0.5, 1e-3, precond)
    assert st == 0 and st3 == [0, 0, 0]
    for k in range(3):
        x1 = xs[k].copy()
        assert iterative_solve(mats[k], bs[k], x1, 3, BICGSTAB, 0.5, 1e-3, precond, raise_on_error=False) == 0
        assert same_bits(x3[k], x1), "system %d" % k
        c = G.Case("triple", (shape, k), 3, precond, 1)
        check_x(G.case_id(c), x1, *G.references(c))


# ------------------------------------------------------------------ 5. the per-system guard at odd sizes
@pytest.mark.parametrize("shape", G.GUARD3_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_breakdown_guard_acts_per_system_at_odd_sizes(gpu, shape):
    """test_gpu_triple.test_breakdown_guard_acts_per_system (even n) at n = 715 and n = 1 048 577: system 1 has b = 0, x = 0 (rho = 0,
    frozen at once), system 2 is the identity (s vanishes in the first half step: x = h, then frozen), system 0 iterates on — the
    mixed-state branches of bicg_s3_k, bicg_xr3_k and bicg_p3_k with their n & 1 tails.  The same assertions at 12 iterations;
    at 3 the surviving system is within the bound of its longdouble reference."""
    from orc_amd.linear_algebra import breakdown_guard_events, iterative_solve, iterative_solve3
    mats, bs, xs = G.three_systems(shape)
    n = mats[0].shape[0]
    assert n % 2 == 1
    bs[1] = np.zeros(n)
    xs[1] = np.zeros(n)
    ident = mats[0].copy()
    ident.data = np.where(np.repeat(np.arange(n), np.diff(ident.indptr)) == ident.indices, 1.0, 0.0)
    mats[2] = ident
    xs[2] = np.zeros(n)
    for iters in (12, 3):
        ev0 = breakdown_guard_events()
        x3 = [x.copy() for x in xs]
        st, st3 = iterative_solve3(mats, bs, x3, iters, BICGSTAB, 0.5, 1e-3, PRE_NONE)
        assert st == 0 and st3 == [0, 0, 0]
        assert breakdown_guard_events() - ev0 == 2
        assert np.array_equal(x3[1], np.zeros(n))
        assert np.array_equal(x3[2], bs[2])  # x = h = x + alpha p = b exactly, and it stays there
        for k in range(3):
            x1 = xs[k].copy()
            assert iterative_solve(mats[k], bs[k], x1, iters, BICGSTAB, 0.5, 1e-3, PRE_NONE, raise_on_error=False) == 0
            assert same_bits(x3[k], x1), "system %d, %d iterations" % (k, iters)
        if iters == 12:
            assert np.isfinite(x3[0]).all() and np.linalg.norm(mats[0] @ x3[0] - bs[0]) < 1e-2 * np.linalg.norm(bs[0])  # system 0 carried on
        else:
            c = G.Case("triple", (shape, 0), 3, PRE_NONE, 1)
            check_x("surviving system, " + G.case_id(c), x3[0], *G.references(c))


# ------------------------------------------------------------------ 6. guard sizes
@pytest.mark.parametrize("c", G.GUARD_CASES, ids=G.case_id)
def test_as_many_iterations_as_unknowns(gpu, c):
    """BiCGSTAB on n unknowns is through after n iterations: the last half step meets s = 0 exactly (the guard takes x = h and the
    solve counts one event) or rounding noise.  Held to the direct solution: eps x condition (< 1e3, tests/test_bicg_cpu.py) x
    iterations (<= 8) < 2e-12, with margin."""
    from orc_amd.linear_algebra import breakdown_guard_events
    a, b, _ = G.system(c.kind, c.key)
    ev0 = breakdown_guard_events()
    st, x = device_solve(c)
    events = breakdown_guard_events() - ev0
    ref = np.linalg.solve(a.toarray(), b)
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print("%s: %d guard event(s), distance from the direct solution %.3e" % (G.case_id(c), events, err))
    assert st == 0 and events in (0, 1)
    assert np.isfinite(x).all() and err <= 1e-10, (x, ref)
