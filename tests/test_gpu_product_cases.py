"""Every product kernel a user matrix can select (launch_spmv, orc_amd/csrc/spmv.hip), at its boundaries, bit for bit.

The matrices are those of tests/product_cases.py: on the raggedness-class thresholds, on the 65 535 / 65 536 column span of the
narrow image, with width-0 slices, empty rows, rows without a diagonal, last slices with one or two live rows and widths that
are no multiple of the 8-entry chunk (tests/test_product_cases_cpu.py derives each of those claims from the matrix).  Every
comparison is bit equality with the CPU oracle, and every run is asserted against the launch counter
(orc_debug_product_launches): the family the table names was launched, the expected number of times, and no other — so a
dispatch threshold that drifts fails here instead of silently moving a case to another kernel.

Which families orc_iterative_solve can reach on a user matrix (no mirrors, no persistent pattern), and what the switch runs
therefore assert:
  * class 1 (S2) has ONE kernel, spmv_k<Epi, kSpmvRagged>: it applies carried scalings itself and has no non-temporal
    instantiation, so ORC_SPMV_NT=1 and ORC_MATERIALIZE_SCALING=0 leave S2 in "ragged" (asserted);
  * the non-temporal instantiation exists for the narrow image only: ORC_SPMV_NT=1 moves S1 to "narrow_nt" and leaves the wide
    S3 / S4 in "wide" (asserted);
  * scalings carried on the fly (Jacobi preconditioner below 4 iterations, or ORC_MATERIALIZE_SCALING=0) take the generic
    scaled kernel "generic_scaled" on S1, S3 and S4 (asserted)."""
import numpy as np
import pytest

import product_cases as PC
from product_cases import BICGSTAB, JACOBI, PRE_JACOBI, PRE_NONE

pytestmark = pytest.mark.gpu

REFERENCE = 1
P_IDS = [c.name for c in PC.P_CASES]
S_IDS = [c.name for c in PC.S_CASES]


@pytest.fixture()
def reference_order(gpu):
    from orc_amd.linear_algebra import set_breakdown_guard, set_reduction_order
    set_reduction_order(REFERENCE)
    set_breakdown_guard(False)  # the reference has no guard (linear_algebra.rs:255-268)
    yield
    set_reduction_order(0)
    set_breakdown_guard(True)


def same_bits(a, b):
    """identical bit patterns; NaNs must sit in the same places (their sign/payload is hardware business)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def launched(fn):
    """(result of fn(), {family: launches} of the families fn() launched)"""
    from orc_amd.linear_algebra import product_launches
    product_launches(reset=True)
    out = fn()
    return out, {k: v for k, v in product_launches(reset=True).items() if v}


_ORACLE = {}


def oracle_product(oracle, name):
    key = ("y", name)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.Csr.from_scipy(PC.CASES[name].build()).spmv(PC.product_vector(name))
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def oracle_solve(oracle, name, method, its, relaxation, threshold, pre):
    """(status, x, jacobi sweeps) of the oracle, computed once per solve"""
    key = (name, method, its, relaxation, threshold, pre)
    if key not in _ORACLE:
        a, b, x0 = PC.solve_system(name)
        x = x0.copy()
        st = oracle.iterative_solve(oracle.Csr.from_scipy(a), b, x, its, method, relaxation, threshold, pre)
        x.setflags(write=False)
        _ORACLE[key] = (st, x, int(oracle.lib().or_last_jacobi_sweeps()))
    return _ORACLE[key]


def device_product(name):
    from orc_amd.linear_algebra import csr_spmv
    (y, _), fams = launched(lambda: csr_spmv(PC.CASES[name].build(), PC.product_vector(name)))
    return y, fams


# ------------------------------------------------------------------ products
@pytest.mark.parametrize("name", P_IDS + S_IDS)
def test_product_bits_and_kernel_family(gpu, oracle, name):
    """y = A x equals the oracle's product in every bit, computed by exactly the kernel family the table names"""
    y, fams = device_product(name)
    assert fams == {PC.CASES[name].family: 1}
    assert same_bits(y, oracle_product(oracle, name))


def test_class_edge_flips_the_kernel(gpu, oracle):
    """P3a and P3b differ by one entry: the uniform kernel on one side of padded = 1.08 nnz, spmv_k on the other"""
    (ya, fa), (yb, fb) = device_product("P3a_class_edge_below"), device_product("P3b_class_edge_above")
    assert fa == {"narrow": 1} and fb == {"ragged": 1}
    assert same_bits(ya, oracle_product(oracle, "P3a_class_edge_below")) and same_bits(yb, oracle_product(oracle, "P3b_class_edge_above"))


def test_offset_0xffff_rows_one_by_one(gpu, oracle):
    """P4a: rows 7 and 40 stream the 16-bit offset 0xFFFF (column 65 535 over the depth's base column 0)"""
    name = "P4a_span_65535"
    a, x = PC.CASES[name].build(), PC.product_vector(name)
    y, fams = device_product(name)
    assert fams == {"narrow": 1}
    yo = oracle_product(oracle, name)
    for r in PC.FAR_ROWS:
        want = 0.0 + a.data[a.indptr[r]] * x[65535]
        assert yo[r] == want
        assert y[r].view(np.uint64) == yo[r].view(np.uint64), "row %d (offset 0xFFFF): %r, oracle %r" % (r, y[r], yo[r])
    assert same_bits(y, yo)


@pytest.mark.parametrize("name", ["P1_short_ragged", "P4a_span_65535"])
def test_without_the_narrow_image_same_bits(gpu, oracle, monkeypatch, name):
    """ORC_SPMV_NARROW_COLS=0: the same matrices through the 32-bit columns"""
    y_narrow, fams = device_product(name)
    assert fams == {"narrow": 1}
    monkeypatch.setenv("ORC_SPMV_NARROW_COLS", "0")
    y, fams = device_product(name)
    assert fams == {"wide": 1}
    assert same_bits(y, oracle_product(oracle, name)) and same_bits(y, y_narrow)


@pytest.mark.parametrize("name", ["P4a_span_65535", "P4e_far_short_ragged"])
def test_small_grid_same_bits(gpu, oracle, monkeypatch, name):
    """ORC_SPMV_GRID=8: 32 wavefronts walk the 1 025 slices, about 32 each"""
    monkeypatch.setenv("ORC_SPMV_GRID", "8")
    y, fams = device_product(name)
    assert fams == {PC.CASES[name].family: 1}
    assert same_bits(y, oracle_product(oracle, name))


# ------------------------------------------------------------------ solves in reference order
SWITCHES = {"default": None, "nt": ("ORC_SPMV_NT", "1"), "no_materialise": ("ORC_MATERIALIZE_SCALING", "0")}


def expected_solve_family(case, pre, its, switch):
    on_the_fly = pre == PRE_JACOBI and (its < 4 or switch == "no_materialise")
    return PC.solve_family(case, on_the_fly, nt=(switch == "nt"))


def bicg_runs():
    out = []
    for c in PC.S_CASES:
        for pre in (PRE_NONE, PRE_JACOBI):
            for its in PC.BICG_COUNTS[(c.name, pre)]:
                for sw in SWITCHES:
                    out.append(pytest.param(c.name, pre, its, sw, id="%s-%s-%d-%s" % (c.name, "jacobi" if pre else "none", its, sw)))
    return out


@pytest.mark.parametrize("name,pre,its,switch", bicg_runs())
def test_bicgstab_reference_order_bit_exact(reference_order, oracle, monkeypatch, name, pre, its, switch):
    """BiCGSTAB with scalings on the fly (3 iterations) and materialised (8): status and every bit of x against the oracle; all
    1 + 2 its products (EpiResidual, EpiStoreSum, EpiTs) by the one family the table's class and narrow columns give, also with
    ORC_SPMV_NT=1 and ORC_MATERIALIZE_SCALING=0 (module docstring: which families those can reach)."""
    from orc_amd.linear_algebra import iterative_solve
    case = PC.CASES[name]
    if SWITCHES[switch]:
        monkeypatch.setenv(*SWITCHES[switch])
    a, b, x0 = PC.solve_system(name)
    x = x0.copy()
    st, fams = launched(lambda: iterative_solve(a, b, x, its, BICGSTAB, 0.5, 1e-3, pre, raise_on_error=False))
    sto, xo, _ = oracle_solve(oracle, name, BICGSTAB, its, 0.5, 1e-3, pre)
    assert fams == {expected_solve_family(case, pre, its, switch): 1 + 2 * its}
    assert st == sto == 0
    assert np.isfinite(xo).all()
    assert same_bits(x, xo)


def test_switch_runs_cover_the_reachable_families():
    """what the runs above assert, as sets: the non-temporal and the generic scaled kernels are reached, and where"""
    reach = {}
    for c in PC.S_CASES:
        reach[c.name] = {expected_solve_family(c, pre, its, sw) for pre in (PRE_NONE, PRE_JACOBI) for its in PC.BICG_COUNTS[(c.name, pre)] for sw in SWITCHES}
    assert reach["S1_short_ragged"] == {"narrow", "narrow_nt", "generic_scaled"}
    assert reach["S2_long_ragged"] == {"ragged"}
    assert reach["S3_far_bidiagonal"] == reach["S4_far_short_ragged"] == {"wide", "generic_scaled"}
    for c in PC.S_CASES:
        assert min(PC.BICG_COUNTS[(c.name, PRE_JACOBI)]) < 4 <= max(PC.BICG_COUNTS[(c.name, PRE_JACOBI)]), "both sides of the materialisation threshold"


# ------------------------------------------------------------------ Jacobi arm
@pytest.mark.parametrize("threshold,count", PC.JACOBI_ARM_RUNS)
@pytest.mark.parametrize("pre", [PRE_NONE, PRE_JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("name", PC.JACOBI_ARM_CASES)
def test_jacobi_arm_bit_exact(gpu, oracle, name, pre, threshold, count):
    """sweeps that never break (1e-30) and sweeps that break on the residual ratio (0.2): x and the sweep count"""
    from orc_amd.linear_algebra import iterative_solve, last_jacobi_sweeps
    a, b, x0 = PC.solve_system(name)
    x = x0.copy()
    st = iterative_solve(a, b, x, count, JACOBI, PC.JACOBI_RELAXATION, threshold, pre, raise_on_error=False)
    sto, xo, sweeps = oracle_solve(oracle, name, JACOBI, count, PC.JACOBI_RELAXATION, threshold, pre)
    assert st == sto == 0
    assert last_jacobi_sweeps() == sweeps
    assert same_bits(x, xo)


# ------------------------------------------------------------------ default (tree) order
@pytest.mark.parametrize("pre", [PRE_NONE, PRE_JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("name", ["S2_long_ragged", "S4_far_short_ragged"])
def test_tree_order_finite_and_repeatable(gpu, name, pre):
    """the product default: 8 BiCGSTAB iterations finish finite and repeat bit for bit"""
    from orc_amd.linear_algebra import iterative_solve
    a, b, x0 = PC.solve_system(name)
    xs = []
    for _ in range(2):
        x = x0.copy()
        st, fams = launched(lambda: iterative_solve(a, b, x, 8, BICGSTAB, 0.5, 1e-3, pre, raise_on_error=False))
        assert st == 0 and np.isfinite(x).all()
        assert fams == {PC.CASES[name].family: 17}
        assert not np.array_equal(x, x0)
        xs.append(x)
    assert same_bits(xs[0], xs[1])
