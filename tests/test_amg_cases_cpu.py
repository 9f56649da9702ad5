"""The inputs of tests/test_gpu_amg_cases.py, guarded without a GPU: every case of tests/amg_cases.py is what its table line claims.

For every case: the Python restatement of the reference's pairing (amg_cases.greedy_pairing, written from linear_algebra.rs:30-60) gives the
R of the oracle's build_restriction_matrix; on the dyadic cases scipy's exact `R @ a @ R.T` has the pattern, the column order and the values
of the oracle's R.matmul(A).matmul(R.transpose()) bit for bit; and what the case is in the table FOR — the LDS tier of its coarse rows, the
candidate limit 2048, rows deeper than the four-entry preference list, ties, weight-2 entries, unmatched rows, empty coarse rows — is derived
from the matrix by amg_cases.predicted and asserted, so that a later edit of a builder cannot quietly move a case off its branch.  orc_amd is
not imported."""
import numpy as np
import pytest

import amg_cases as AC

IDS = AC.NAMES


@pytest.fixture(scope="module")
def oracle_level(oracle):
    """(A, R, (R A) R^T as scipy) of the oracle per case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            A = oracle.Csr.from_scipy(AC.CASES[name].build())
            R = oracle.build_restriction_matrix(A)
            cache[name] = (R.to_scipy(), R.matmul(A).matmul(R.transpose()).to_scipy())
        return cache[name]

    return get


def test_table_is_complete():
    for want in ["ladder_shared", "ladder_random", "dense_at_limit", "dense_over_limit", "all_ties", "few_values", "mutual_pairs", "isolated_rows",
                 "positive_offdiag", "random_doubles"] + ["band_%d" % v for v in (15, 16, 17, 31, 32, 33, 63, 64, 65, 129)] + \
                ["sizes_%d" % n for n in (1, 2, 3, 63, 64, 65, 127, 129)]:
        assert want in AC.CASES, want
    assert len(set(IDS)) == len(IDS) == 28
    assert set(AC.SCANNING) | set(AC.FORM_CASES) | set(AC.SECOND_LEVEL) | set(AC.END_TO_END) <= set(AC.COARSENED)
    src = open(AC.__file__).read()
    assert "import orc_amd" not in src and "from orc_amd" not in src and "import oracle" not in src and "from oracle" not in src


@pytest.mark.parametrize("name", IDS)
def test_matrix_is_well_formed(name):
    case = AC.CASES[name]
    a = case.build()
    n = a.shape[0]
    assert a.shape == (n, n) and n <= 560 and a.nnz <= 270_000
    assert a.has_sorted_indices
    lens = np.diff(a.indptr)
    inner = np.arange(a.nnz) > np.repeat(a.indptr[:-1], lens)
    assert (np.diff(a.indices.astype(np.int64))[inner[1:]] > 0).all(), "columns strictly ascending per row"
    assert np.isfinite(a.data).all() and (a.data != 0).all()
    rid = np.repeat(np.arange(n), lens)
    assert (np.bincount(rid[a.indices == rid], minlength=n) == 1).all(), "full diagonal"
    assert AC.prediction(name)[2] == case.expect["max_len"]
    off = a.data[a.indices != rid]
    if case.expect["dyadic"]:
        assert np.array_equal(a.data * 1024.0, np.round(a.data * 1024.0)) and (np.abs(off) < 4096.0).all()
        d = a.diagonal()
        assert np.array_equal(d, np.round(d))
    else:
        assert not np.array_equal(off * 1024.0, np.round(off * 1024.0))
    if case.expect.get("positive"):
        assert (off > 0).all() and (a.diagonal() < 0).all()
    elif len(off):
        assert (off < 0).all() and (a.diagonal() > 0).all()


def test_band_patterns_are_what_the_table_says():
    """odd lengths: symmetric half-width; even lengths: one more sub- than super-diagonal (structurally asymmetric)"""
    for length in AC.BAND_LENGTHS:
        a = AC.band(length)
        coo = a.tocoo()
        d = coo.col.astype(np.int64) - coo.row
        assert d.min() == -(length // 2) and d.max() == (length - 1) // 2
        sym = (abs(a) > 0).astype(np.int8)
        assert ((sym != sym.T).nnz == 0) == (length % 2 == 1)
    for n in AC.SIZES:
        assert AC.CASES["sizes_%d" % n].build().shape == (n, n)
    assert AC.few_values().shape == (193, 193) and set(np.unique(AC.few_values().data)) == {-1.0, -0.5, 4.0 * 33}
    assert AC.isolated_at()[:3] == (3, 14, 25) and set(AC.ISOLATED_RUN) <= set(AC.isolated_at()) and AC.ISOLATED_RUN[0] % 2 == 0
    iso = AC.isolated_rows()
    assert all(iso.indptr[r + 1] - iso.indptr[r] == 1 for r in AC.isolated_at())


@pytest.mark.parametrize("name", IDS)
def test_python_pairing_gives_the_oracles_restriction(oracle_level, name):
    a = AC.CASES[name].build()
    partner, depth = AC.pairing(name)
    r = AC.restriction(partner, a.shape[0])
    ro, _ = oracle_level(name)
    ro.sort_indices()
    assert r.shape == ro.shape
    assert np.array_equal(r.indptr, ro.indptr) and np.array_equal(r.indices, ro.indices) and np.array_equal(r.data, ro.data)
    # a pairing: no column is taken twice, nobody takes itself, every partner is a stored off-diagonal of its row
    m = partner[partner >= 0]
    assert len(np.unique(m)) == len(m)
    assert (partner != np.arange(a.shape[0])).all()
    for i in np.flatnonzero(partner >= 0)[:: max(1, a.shape[0] // 50)]:
        assert partner[i] in a.indices[a.indptr[i]:a.indptr[i + 1]]
    assert (depth >= 0).all() and (depth[partner < 0] == np.diff(a.indptr)[partner < 0] - 1).all()


@pytest.mark.parametrize("name", [n for n in IDS if AC.CASES[n].expect["dyadic"]])
def test_exact_product_is_the_oracles_bit_for_bit(oracle_level, name):
    """dyadic values: every sum of (R a) R^T is exact, so scipy's product (another association) must equal the oracle's in pattern, column
    order and every bit, signs of zeros included"""
    a = AC.CASES[name].build()
    ac = AC.exact_coarse(a, AC.pairing(name)[0])
    _, ref = oracle_level(name)
    assert ac.shape == ref.shape
    assert np.array_equal(ac.indptr, ref.indptr) and np.array_equal(ac.indices, ref.indices)
    assert np.array_equal(ac.data, ref.data) and np.array_equal(np.signbit(ac.data), np.signbit(ref.data))


@pytest.mark.parametrize("name", IDS)
def test_case_meets_its_expectation(name):
    case = AC.CASES[name]
    a = case.build()
    partner, depth = AC.pairing(name)
    c, hist, max_len = AC.prediction(name)
    lens = np.diff(a.indptr)
    ex = case.expect
    assert hist.sum() == (a.shape[0] + 1) // 2
    for t in ex.get("tiers", ()):
        assert hist[t] > 0, "tier %d is empty: %s" % (t, hist.tolist())
    if "max_c" in ex:
        assert c.max() == ex["max_c"]
    assert (hist[AC.REFUSED] > 0) == bool(ex.get("refused")) == (name == AC.REFUSED_CASE)
    if not ex.get("refused"):
        assert c.max(initial=0) <= AC.CAND_LIMIT
    if ex.get("deep_long"):
        assert ((lens > 64) & (depth > 3)).any()
    if "deeper_than_list" in ex:
        assert (depth > 3).sum() >= ex["deeper_than_list"]
    if ex.get("ties"):
        assert len(AC.tie_rows(a)) > 0
    r = AC.restriction(partner, a.shape[0])
    if ex.get("weight2_only"):
        assert (r.data == 2.0).all() and (np.diff(r.indptr) == 2).all()
    if ex.get("unmatched"):
        assert set(AC.isolated_at()) <= set(np.flatnonzero(partner < 0))
    if ex.get("empty_coarse"):
        empty = np.flatnonzero(np.diff(r.indptr) == 0)
        assert {AC.ISOLATED_RUN[0] // 2, AC.ISOLATED_RUN[2] // 2} <= set(empty)
        assert (c[empty] == 0).all()


def test_table_covers_every_branch():
    """over the table: every tier 0-6 non-empty somewhere, c == 2048 occurs, c > 2048 only in dense_over_limit, rows on both sides of the
    lanes-per-row G = 16 / 32 / 64 of their coarse row's tier, rows beyond the register scan (8 G = 32 and 64 entries) that are deeper than
    their list, and the sizes around a 64-row slice"""
    total = np.zeros(AC.N_TIERS + 1, np.int64)
    at_limit = False
    for name in IDS:
        c, hist, _ = AC.prediction(name)
        total += hist
        at_limit |= bool((c == AC.CAND_LIMIT).any())
        assert (c > AC.CAND_LIMIT).any() == (name == AC.REFUSED_CASE)
    assert (total[:AC.N_TIERS] > 0).all() and at_limit
    assert AC.prediction("dense_at_limit")[1][6] == 256 and AC.prediction("dense_over_limit")[0].max() == 2056
    # the merge's first-G-entries prefetch: in the tier its coarse row lands in, a fine row shorter than G, of exactly G, longer than G, 2 G
    group = (16, 16, 32, 64, 64, 64, 64)
    seen = set()
    for name in AC.COARSENED:
        a = AC.CASES[name].build()
        lens = np.diff(a.indptr)
        r = AC.restriction(AC.pairing(name)[0], a.shape[0])
        c = AC.prediction(name)[0]
        for I in range(r.shape[0]):
            g = group[AC.tier_of(int(c[I]))]
            for i in r.indices[r.indptr[I]:r.indptr[I + 1]]:
                ln = int(lens[i])
                seen.add((g, "below" if ln < g else "at" if ln == g else "above" if ln <= 2 * g else "above2"))
    # (a coarse row holds at least two fine rows, so a row longer than 2 G cannot land in a tier of G = 16 or 32 lanes — c <= 64, 128 — by
    # itself: those meet only under ORC_GALERKIN_GROUPS, which the GPU test's forms set)
    for g in (16, 32, 64):
        for where in ("below", "at", "above") + (("above2",) if g == 64 else ()):
            assert (g, where) in seen, (g, where)
    # the chains' scan: rows longer than 8 G that run out of their list (G = 4: mean padded length <= 24, else 8)
    for name, limit in (("ladder_shared", 64), ("all_ties", 64), ("dense_at_limit", 64), ("band_129", 64), ("band_65", 64)):
        a = AC.CASES[name].build()
        assert ((np.diff(a.indptr) > limit) & (AC.pairing(name)[1] > 3)).any(), name
    assert {1, 2, 3, 63, 64, 65, 127, 129} == set(AC.SIZES)


def test_dominant_systems_of_the_end_to_end_runs():
    for name in AC.END_TO_END:
        a, b, x0 = AC.end_to_end_system(name)
        n = a.shape[0]
        rid = np.repeat(np.arange(n), np.diff(a.indptr))
        off = np.zeros(n)
        np.add.at(off, rid[a.indices != rid], np.abs(a.data[a.indices != rid]))
        assert (a.diagonal() > off).all()
        orig = AC.CASES[name].build()
        assert np.array_equal(a.indices, orig.indices) and np.array_equal(a.data[a.indices != rid], orig.data[a.indices != rid])
