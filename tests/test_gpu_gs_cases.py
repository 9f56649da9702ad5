"""The Gauss-Seidel arms (orc_amd/csrc/gs_*.hip) on user matrices, at their edges: the matrices of tests/gs_cases.py — patterns that
are not structurally symmetric, colours of fewer than 64 rows, exactly 64 colours and one too many, more than 1 024 row blocks
and colour-sorted slices (the carry branches of gs_column_scan_k and gs_slice_ptr_k in gs_layout.hip), rows of 1 ... 130 entries, an empty row,
a last slice with one live row — against the numpy restatements of tests/gs_restatement.py, which tests/test_gs_cases_cpu.py
checks against forward substitution without a GPU.

  * the colouring is proper on A united with its transpose, repeatable, and on symmetric patterns bit for bit the colouring of
    the rule that looks at a row's own line alone (so cached mesh colourings and colour counts did not move); on the other
    patterns it is the restated rule with knock-out stores and forbidden-colour masks;
  * MULTICOLOR_GS sweeps are the restated sweep IN EVERY BIT, in the colours the device reports, and repeat bit for bit — with
    rows of one colour coupled through an entry only one of them stores, a colour's launch read x[j] while writing it and
    neither held;
  * more than 64 colours is ORC_ERR_BAD_ARGUMENT with x untouched, and leaves nothing behind for the next solve;
  * the preconditioned BiCGSTAB in slot space and in row space agree with each other and with the exactly-summed restatement
    within a bound made of the reference's own sensitivity to the summation order: 100 max(d_ref, n 2^-53), d_ref the distance
    between the restatement with math.fsum and with np.sum (the device's wave tree is a third association; three iterations
    amplify the difference by the mechanism that produces d_ref).  A wrong gather, a dropped entry or a mis-skipped column of
    gsx_sweep0_k moves the result by many orders of magnitude more.

Three iterations, x0 != 0; relative L2 distances, measured on an MI355X (slot = slot space, row = row space, ref = restatement
with fsum):

  case                 precond  d_ref      bound      slot-row   slot-ref   row-ref
  G1_short_ragged      none     1.924e-16  2.143e-12  1.496e-16  1.908e-16  1.719e-16
  G1_short_ragged      jacobi   2.229e-16  2.143e-12  2.418e-16  2.252e-16  2.410e-16
  G2_long_ragged       none     2.675e-16  1.443e-12  2.668e-16  2.525e-16  2.689e-16
  G2_long_ragged       jacobi   8.902e-17  1.443e-12  1.540e-16  1.516e-16  1.424e-16
  G3_short_ragged_sym  none     5.535e-16  2.143e-12  7.444e-16  5.631e-16  6.340e-16
  G3_short_ragged_sym  jacobi   6.623e-17  2.143e-12  2.063e-16  5.441e-17  2.073e-16
  G4_bidiagonal        none     2.011e-15  2.220e-12  1.688e-15  2.057e-15  1.792e-15
  G4_bidiagonal        jacobi   7.509e-15  2.220e-12  7.463e-15  6.924e-15  6.828e-15
  G5_clique64          none     5.911e-15  1.121e-12  7.074e-14  4.704e-15  6.964e-14
  G5_clique64          jacobi   6.241e-14  6.241e-12  5.747e-13  5.286e-13  4.663e-14
  G7_far_band          none     6.345e-16  7.283e-10  5.832e-16  8.179e-16  9.520e-16
  G7_far_band          jacobi   6.901e-16  7.283e-10  7.900e-16  7.446e-16  8.981e-16
  G8_tridiagonal_65    none     1.686e-16  7.216e-13  4.152e-16  4.410e-16  4.001e-16
  G8_tridiagonal_65    jacobi   1.673e-16  7.216e-13  4.215e-16  4.495e-16  4.764e-16

(the bound is n 2^-53 times 100 everywhere but on G5 with the Jacobi scaling, whose d_ref is the larger term; G5 is also where the
device is closest to its bound, a factor 12 below it.)

The sweep reference is Gauss-Seidel in colour order whatever the colours (gs_restatement.sweep walks a colour with coupled rows
one row at a time), so with the colouring that looked at a row's own line alone the colouring AND the sweep tests of G1, G2 and
G4 fail: "a stored off-diagonal entry inside a colour", and 107 of 193 (G1), 24 of 130 (G2), 155 of 200 (G4) entries of x off.
"""
import math

import numpy as np
import pytest

import gs_cases as G
import gs_restatement as R
from gs_cases import BICGSTAB_GS, MULTICOLOR_GS, MULTIGRID_GS, PRE_JACOBI, PRE_NONE

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """identical bit patterns; NaNs must sit in the same places (their sign/payload is hardware business)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def rel_l2(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def pre_id(pre):
    return "jacobi" if pre else "none"


_COLORS = {}


def device_colors(name):
    """(colors, n_colors) of the library for a case, asked once"""
    from orc_amd.linear_algebra import debug_coloring
    if name not in _COLORS:
        c, nc = debug_coloring(G.CASES[name].build())
        c.setflags(write=False)
        _COLORS[name] = (c, nc)
    return _COLORS[name]


def solve(name, method, its, omega, pre, x):
    from orc_amd.linear_algebra import iterative_solve
    a, b, _ = G.system(name)
    return iterative_solve(a, b, x, its, method, omega, 1e-3, pre, raise_on_error=False)


# ------------------------------------------------------------------ colouring
@pytest.mark.parametrize("name", G.SOLVABLE)
def test_coloring_is_proper_repeatable_and_pinned(gpu, name):
    from orc_amd.linear_algebra import debug_coloring
    case = G.CASES[name]
    a = case.build()
    colors, nc = device_colors(name)
    assert R.is_proper(a, colors), "a stored off-diagonal entry inside a colour"
    assert nc <= 64 and np.array_equal(np.unique(colors), np.arange(nc)), "colours 0 ... nc - 1, none empty"
    again, nc2 = debug_coloring(a)
    assert nc2 == nc and np.array_equal(again, colors)
    if case.symmetric:
        assert np.array_equal(colors, R.color_today(a)), "a symmetric pattern keeps the colouring of the own-line rule"
    else:
        assert np.array_equal(colors, R.color_proper(a))
    if name == "G5_clique64":
        assert nc == 64


def test_coloring_of_65_mutual_neighbours_is_an_error(gpu):
    from orc_amd._lib import OrcError
    from orc_amd.linear_algebra import debug_coloring
    with pytest.raises(OrcError) as e:
        debug_coloring(G.CASES[G.ERROR_CASE].build())
    assert e.value.status == G.ERR_BAD_ARGUMENT


# ------------------------------------------------------------------ sweeps
def sweep_runs():
    return [pytest.param(n, w, p, id="%s-%.1f-%s" % (n, w, pre_id(p))) for n in G.SOLVABLE for w in G.OMEGAS for p in G.preconditioners(n)]


@pytest.mark.parametrize("name,omega,pre", sweep_runs())
def test_sweeps_bit_exact_and_repeatable(gpu, name, omega, pre):
    """3 sweeps from x0 != 0: every bit of the restated sweep in the device's colours, status 0, and the same bits again"""
    a, b, x0 = G.system(name)
    colors, _ = device_colors(name)
    x = x0.copy()
    st = solve(name, MULTICOLOR_GS, G.SWEEPS, omega, pre, x)
    ref = x0
    scale = G.jacobi_scale(a) if pre else None
    for _ in range(G.SWEEPS):
        ref = R.sweep(a, b, ref, omega, colors, scale)
    differ = int(np.sum(x.view(np.uint64) != ref.view(np.uint64)))
    print("%s omega %.1f pre %d: %d of %d entries differ from the restated sweep" % (name, omega, pre, differ, len(x)))
    assert st == 0
    assert same_bits(x, ref), "%d of %d entries differ" % (differ, len(x))
    assert a.shape[0] == 1 or not np.array_equal(x, x0)
    x2 = x0.copy()
    assert solve(name, MULTICOLOR_GS, G.SWEEPS, omega, pre, x2) == 0
    assert same_bits(x2, x), "two runs of the same sweeps"
    if name == G.EMPTY_ROW_CASE:
        assert x[G.EMPTY_ROW].view(np.uint64) == x0[G.EMPTY_ROW].view(np.uint64), "an empty row is skipped"


# ------------------------------------------------------------------ more than 64 colours
def test_more_than_64_colours_is_an_error_and_leaves_nothing_behind(gpu):
    """G6: ORC_ERR_BAD_ARGUMENT from both arms, x untouched; G3 before and after gives the same bits (arena and status word clean)"""
    def g3():
        out = []
        for method in (MULTICOLOR_GS, BICGSTAB_GS):
            x = G.system("G3_short_ragged_sym")[2].copy()
            assert solve("G3_short_ragged_sym", method, 3, 0.8, PRE_NONE, x) == 0
            out.append(x)
        return out

    before = g3()
    _, _, x0 = G.system(G.ERROR_CASE)
    for method in (MULTICOLOR_GS, BICGSTAB_GS):
        for pre in (PRE_NONE, PRE_JACOBI):
            x = x0.copy()
            assert solve(G.ERROR_CASE, method, 3, 0.8, pre, x) == G.ERR_BAD_ARGUMENT
            assert same_bits(x, x0), "x keeps every bit"
    after = g3()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert not np.array_equal(before[0], G.system("G3_short_ragged_sym")[2])


# ------------------------------------------------------------------ preconditioned BiCGSTAB, both forms
_BICG_REF = {}


def bicg_reference(name, pre):
    """(x with exactly rounded sums, d_ref, bound) of a case, from the CPU alone, computed once"""
    key = (name, pre)
    if key not in _BICG_REF:
        a, b, x0 = G.system(name)
        colors, _ = device_colors(name)
        scale = G.jacobi_scale(a) if pre else None
        xf = R.bicgstab_gs(a, b, x0, G.BICG_ITERATIONS, colors, scale, sums=math.fsum)
        xn = R.bicgstab_gs(a, b, x0, G.BICG_ITERATIONS, colors, scale, sums=np.sum)
        d_ref = rel_l2(xn, xf)
        xf.setflags(write=False)
        _BICG_REF[key] = (xf, d_ref, 100.0 * max(d_ref, a.shape[0] * 2.0 ** -53))
    return _BICG_REF[key]


@pytest.mark.parametrize("pre", [PRE_NONE, PRE_JACOBI], ids=pre_id)
@pytest.mark.parametrize("name", G.BICG_CASES)
def test_bicgstab_slot_space_row_space_and_restatement_agree(gpu, monkeypatch, name, pre):
    _, _, x0 = G.system(name)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("ORC_GS_SLOTSPACE", mode)
        x = x0.copy()
        assert solve(name, BICGSTAB_GS, G.BICG_ITERATIONS, 1.0, pre, x) == 0
        out[mode] = x
    xf, d_ref, bound = bicg_reference(name, pre)
    d_sr, d_s, d_r = rel_l2(out["1"], out["0"]), rel_l2(out["1"], xf), rel_l2(out["0"], xf)
    print("BICG %-20s %-6s d_ref %.3e bound %.3e slot-row %.3e slot-ref %.3e row-ref %.3e" % (name, pre_id(pre), d_ref, bound, d_sr, d_s, d_r))
    assert np.isfinite(out["1"]).all() and np.isfinite(out["0"]).all() and np.isfinite(xf).all()
    assert not np.array_equal(out["1"], x0)
    assert d_sr < bound and d_s < bound and d_r < bound, (d_ref, bound, d_sr, d_s, d_r)


@pytest.mark.parametrize("pre", [PRE_NONE, PRE_JACOBI], ids=pre_id)
@pytest.mark.parametrize("name", sorted(G.CONVERGENCE_COUNTS))
def test_bicgstab_gs_converges(gpu, name, pre):
    from orc_amd.linear_algebra import iterative_solve
    a, b, xs = G.convergence_system(name)
    x = np.zeros(len(xs))
    assert iterative_solve(a, b, x, G.CONVERGENCE_COUNTS[name], BICGSTAB_GS, 1.0, 1e-3, pre, raise_on_error=False) == 0
    err = rel_l2(x, xs)
    print("%s pre %d: |x - xs| / |xs| = %.3e after %d iterations" % (name, pre, err, G.CONVERGENCE_COUNTS[name]))
    assert err < 1e-8


# ------------------------------------------------------------------ the smoother of MULTIGRID_GS
@pytest.mark.parametrize("name", G.MULTIGRID_CASES)
def test_multigrid_gs_on_user_matrices(gpu, name):
    """10 cycles: finite, the residual below 0.1 |b| (the bound of the fv test), and the same bits twice — the coarse levels of
    G4 are not structurally symmetric either, and they are coloured anew in every solve"""
    a, b, x0 = G.system(name)
    xs = []
    for _ in range(2):
        x = x0.copy()
        assert solve(name, MULTIGRID_GS, 10, 1.0, PRE_JACOBI, x) == 0
        xs.append(x)
    res = np.linalg.norm(a @ xs[0] - b) / np.linalg.norm(b)
    print("%s: MULTIGRID_GS residual %.3e |b|" % (name, res))
    assert np.isfinite(xs[0]).all() and res < 0.1
    assert same_bits(xs[0], xs[1])
