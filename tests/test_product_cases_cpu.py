"""The inputs of tests/test_gpu_product_cases.py, guarded without a GPU: every claim of the case table (tests/product_cases.py)
is derived here from the matrix itself — the SELL-64 padded count and from it the raggedness class, the column span of every
slice and depth and from them "narrow image kept / refused", and the structural edges (a width-0 slice, empty rows, rows
without a diagonal, the live rows of the last slice, widths that are no multiple of the 8-entry chunk).  A threshold in the
library that drifts is then caught by the GPU test's launch counter, and a builder that drifts is caught here.  The
classification is computed by product_cases.sell_stats from the documented rule; orc_amd is not imported.

Also here: the plain numpy product (sequential in depth, one multiply and one add per step) equals the oracle's product bit for
bit on every case, and the unguarded oracle finishes every solve the GPU test lists with a finite result — the condition
under which those solves can be compared bit for bit at all."""
import numpy as np
import pytest

import product_cases as PC

ALL = PC.P_CASES + PC.S_CASES
IDS = [c.name for c in ALL]


@pytest.fixture(scope="module")
def stats():
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = PC.sell_stats(case.build())
        return cache[case.name]

    return get


def test_table_is_complete():
    names = " ".join(IDS)
    for want in ("P1_", "P2_long", "P2_width8", "P2_width9", "P2_width24", "P3a_", "P3b_", "P4a_", "P4b_", "P4c_", "P4d_", "P4e_", "P4f_",
                 "S1_", "S2_", "S3_", "S4_"):
        assert want in names, want
    assert len(set(IDS)) == len(IDS) == 17
    assert set(PC.BICG_COUNTS) == {(c.name, pre) for c in PC.S_CASES for pre in (PC.PRE_NONE, PC.PRE_JACOBI)}
    src = open(PC.__file__).read()
    assert "import orc_amd" not in src and "from orc_amd" not in src, "the table derives nothing from the library"


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_matrix_is_well_formed(case):
    a = case.build()
    assert a.shape == (case.n, case.n)
    assert a.has_sorted_indices
    lens = np.diff(a.indptr)
    rid = np.repeat(np.arange(case.n), lens)
    inner = np.arange(a.nnz) > np.repeat(a.indptr[:-1], lens)  # not the first entry of its row
    assert (np.diff(a.indices.astype(np.int64))[inner[1:]] > 0).all(), "columns strictly ascending per row"
    assert np.isfinite(a.data).all() and (a.data != 0).all()
    if case.claims.get("full_diag"):  # a solve matrix
        d = a.diagonal()
        off = np.abs(a.data).copy()
        off[a.indices == rid] = 0.0
        row_off = np.zeros(case.n)
        np.add.at(row_off, rid, off)
        assert (np.bincount(rid[a.indices == rid], minlength=case.n) == 1).all(), "full diagonal"
        assert (d > row_off).all(), "strictly diagonally dominant"
        assert (a.data[a.indices != rid] < 0).all(), "negative off-diagonals"


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_class_and_narrow_image_follow_from_the_matrix(case, stats):
    st = stats(case)
    ratio, per_row = st["padded"] / st["nnz"], st["padded"] / st["n"]
    print("%s: n %d nnz %d padded %d padded/nnz %.6f padded/n %.4f" % (case.name, st["n"], st["nnz"], st["padded"], ratio, per_row))
    cls = (2 if per_row < 24 else 1) if ratio > 1.08 else 0
    assert cls == st["cls"] == case.cls
    assert st["narrow"] == case.narrow
    assert not st["unreached"], "a depth below the width is reached by the slice's longest row"
    wide = sorted(k for k, v in st["spans"].items() if v > 65535)
    assert bool(wide) != case.narrow
    if "wide_at" in case.claims:
        assert wide == sorted(case.claims["wide_at"]), "exactly these (slice, depth) exceed 65 535 columns"
    if "max_span" in case.claims:
        top = max(st["spans"].values())
        assert top == case.claims["max_span"]
        assert [k for k, v in st["spans"].items() if v == top] == [case.claims["max_span_at"]]


def test_class_edge_is_within_one_entry_per_slice(stats):
    """P3a / P3b: the same widths, one entry apart in ONE slice, on either side of padded = 1.08 nnz; both at padded = 25 n >= 24 n"""
    a, b = PC.CASES["P3a_class_edge_below"], PC.CASES["P3b_class_edge_above"]
    sa, sb = stats(a), stats(b)
    assert sa["padded"] == sb["padded"] == 25 * 640
    assert (sa["nnz"], sb["nnz"]) == (a.claims["nnz"], b.claims["nnz"]) == (14815, 14814)
    assert not sa["padded"] > 1.08 * sa["nnz"] and sb["padded"] > 1.08 * sb["nnz"]
    per_slice = (sa["lens"] - sb["lens"]).reshape(10, 64).sum(axis=1)
    assert sorted(per_slice.tolist()) == [0] * 9 + [1]
    for st in (sa, sb):
        removed = 25 * 64 - st["lens"].reshape(10, 64).sum(axis=1)
        assert removed.max() - removed.min() <= 1, "shortened evenly"


def test_far_column_rows(stats):
    """P4a streams the 16-bit offset 0xFFFF in exactly the rows the GPU test asserts one by one; P4b is one column further"""
    a, b = PC.far_depth0(65535), PC.far_depth0(65536)
    for r in PC.FAR_ROWS:
        assert a.indices[a.indptr[r]:a.indptr[r + 1]].tolist() == [65535]
        assert b.indices[b.indptr[r]:b.indptr[r + 1]].tolist() == [65536]
    lo = min(int(a.indices[a.indptr[r]]) for r in range(64))  # depth 0 of slice 0
    assert lo == 0 and 65535 - lo == 0xFFFF
    assert (a != b).nnz == 2 * len(PC.FAR_ROWS)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_structural_claims(case, stats):
    st, cl, a = stats(case), case.claims, case.build()
    lens, widths, n = st["lens"], st["widths"], st["n"]
    if "width0_slice" in cl:
        assert widths[cl["width0_slice"]] == 0
    if cl.get("empty_row"):
        assert (lens == 0).any()
    if cl.get("missing_diag"):
        rid = np.repeat(np.arange(n), lens)
        has = np.bincount(rid[a.indices == rid], minlength=n) > 0
        assert (~has & (lens > 0)).any(), "a non-empty row without a diagonal"
    if "last_slice_live" in cl:
        assert n - 64 * (len(widths) - 1) == cl["last_slice_live"]
    if "last_slice_lens" in cl:
        assert tuple(lens[64 * (len(widths) - 1):]) == cl["last_slice_lens"]
    if "widths" in cl:
        assert tuple(widths) == cl["widths"]
    if "max_width" in cl:
        assert widths.max() == cl["max_width"]
    if "width_mod8" in cl:
        assert widths.max() % 8 == cl["width_mod8"] != 0
    if case.cls == 1:  # spmv_k's clamp: some lane is shorter than its slice, some row is long
        assert (np.repeat(widths, 64)[:n] > lens).any()
    if case.name.startswith("P2_width"):
        assert set(widths) == {int(case.name[len("P2_width"):])}


def test_widths_cover_the_chunk_edges():
    """slice widths of the class-1 cases: below, at and just above one 8-entry chunk, three chunks, and chunks plus a remainder"""
    got = set()
    for c in ALL:
        if c.cls == 1:
            got |= set(int(w) for w in PC.sell_stats(c.build())["widths"])
    assert {1, 8, 9, 24, 25, 130, 2950} <= got


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_sequential_numpy_product_equals_the_oracle(case, oracle):
    a, x = case.build(), PC.product_vector(case.name)
    y = PC.sequential_product(a, x)
    yo = oracle.Csr.from_scipy(a).spmv(x)
    assert np.array_equal(y.view(np.uint64), yo.view(np.uint64))
    assert np.isfinite(y).all()


@pytest.mark.parametrize("pre", [PC.PRE_NONE, PC.PRE_JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("case", PC.S_CASES, ids=[c.name for c in PC.S_CASES])
def test_oracle_finishes_every_listed_solve_finite(case, pre, oracle):
    """The reference iterates without a breakdown guard: a solve that converges exactly divides 0 by 0.  Every solve the GPU test
    compares must stay finite in the oracle alone (a count that does not is lowered in product_cases.BICG_COUNTS)."""
    a, b, x0 = PC.solve_system(case.name)
    A = oracle.Csr.from_scipy(a)
    for its in PC.BICG_COUNTS[(case.name, pre)]:
        x = x0.copy()
        assert oracle.iterative_solve(A, b, x, its, PC.BICGSTAB, 0.5, 1e-3, pre) == 0
        assert np.isfinite(x).all(), "%d iterations" % its
        assert not np.array_equal(x, x0)
    if case.name in PC.JACOBI_ARM_CASES:
        sweeps = []
        for thr, count in PC.JACOBI_ARM_RUNS:
            x = x0.copy()
            assert oracle.iterative_solve(A, b, x, count, PC.JACOBI, PC.JACOBI_RELAXATION, thr, pre) == 0
            assert np.isfinite(x).all()
            sweeps.append(int(oracle.lib().or_last_jacobi_sweeps()))
        print(case.name, pre, "jacobi sweeps", sweeps)
        assert sweeps[0] == PC.JACOBI_ARM_RUNS[0][1], "threshold 1e-30 never breaks"
        assert 2 < sweeps[1] < PC.JACOBI_ARM_RUNS[1][1], "threshold 0.2 breaks on the residual ratio before the count runs out"


def test_launch_counter_mirror_matches_the_header():
    """orc_debug_product_launches is host-only: callable without a device, and the Python names follow the header's enum"""
    import os
    import re
    from conftest import ROOT
    from orc_amd.linear_algebra import PRODUCT_FAMILIES, product_launches
    txt = open(os.path.join(ROOT, "include", "orc_amd.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"ORC_PRODUCT_([A-Z_]+) = (\d+)", txt)}
    assert enum.pop("families") == len(PRODUCT_FAMILIES)
    assert [k for k, _ in sorted(enum.items(), key=lambda kv: kv[1])] == list(PRODUCT_FAMILIES)
    got = product_launches(reset=True)
    assert list(got) == list(PRODUCT_FAMILIES) and all(v >= 0 for v in got.values())
    assert set(product_launches().values()) == {0}
    assert {c.family for c in ALL} <= set(PRODUCT_FAMILIES)
