"""The compact metadata of the window products (XWinDev in orc_amd/csrc/linalg.hpp, ORC_XWIN_COMPACT): 12-bit window positions on levels whose
LDS share is at most 4 096 entries, and per block 16-bit window columns behind a 32-bit base per 64 list entries unless a segment spans 65 536
columns or more.  Neither changes a result: every product here is compared bit for bit with ORC_XWIN_COMPACT=0 and with the oracle's CSR product
(linear_algebra.rs:82-97, ascending-column sums), plain and with the smoothing solves' materialised Jacobi scaling; the raw streams
(orc_debug_amg_xwin_raw) must decode to the wide image and weigh what the formats promise.  Coarse patterns are prescribed through fine matrices
with forced pairs (tests/xwin_cases.py)."""
import numpy as np
import pytest

import xwin_cases as X
from conftest import fv_like_matrix, splitmix64_uniform

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x).view(np.uint64)


def _decoded(raw):
    """(positions, [window columns per block]) of a raw image"""
    from orc_amd.linear_algebra import xwin_unpack_positions, xwin_unpack_window
    pos = xwin_unpack_positions(raw["pos_raw"], raw["pos_bits"])
    win = [xwin_unpack_window(raw["wcol_raw"][b], int(raw["wsize"][b]), int(raw["wfmt"][b])) for b in range(len(raw["wsize"]))]
    return pos, win


def _expected_wcol_bytes(raw):
    ws, fmt = raw["wsize"].astype(np.int64), raw["wfmt"]
    has = ws > 0
    return int(np.where(fmt[has] == 1, 2 * ws[has] + 4 * ((ws[has] + 63) // 64), 4 * ws[has]).sum())


def _check_products(oracle, monkeypatch, fine, coarse, seed):
    """y = a' x as the solves launch it, compact and wide, plain and scaled: the same bits, and the oracle's"""
    from orc_amd.linear_algebra import amg_coarse_product
    nc = coarse.shape[0]
    x = splitmix64_uniform(nc, seed)
    for scaled in (False, True):
        ref = coarse.copy()
        if scaled:  # p_inv * a (linear_algebra.rs:159-166); an empty coarse row has no diagonal: nothing of it is scaled
            with np.errstate(divide="ignore"):
                dinv = 1.0 / ref.diagonal()
            ref.data = np.repeat(dinv, np.diff(ref.indptr)) * ref.data
        yo = oracle.Csr.from_scipy(ref).spmv(x)
        y, mirror = amg_coarse_product(fine, x, scaled=scaled)
        assert mirror, "no window mirror"
        assert np.array_equal(_bits(y), _bits(yo)), "scaled=%s: compact product differs from the oracle" % scaled
        monkeypatch.setenv("ORC_XWIN_COMPACT", "0")
        yw, _ = amg_coarse_product(fine, x, scaled=scaled)
        monkeypatch.delenv("ORC_XWIN_COMPACT")
        assert np.array_equal(_bits(y), _bits(yw)), "scaled=%s: compact and wide products differ" % scaled


# ---------------------------------------------------------------- 1. layout
@pytest.fixture(scope="module")
def fv_levels(gpu):
    from orc_amd.linear_algebra import amg_coarsen
    out = [fv_like_matrix(96, 64, 16)]
    for _ in range(3):
        _, ac, _ = amg_coarsen(out[-1])
        out.append(ac.tocsr())
    return out


@pytest.mark.parametrize("lv", [1, 2])
def test_raw_streams_decode_to_the_wide_image_and_weigh_what_they_promise(gpu, fv_levels, monkeypatch, lv):
    from orc_amd.linear_algebra import amg_packed_mirror, amg_xwin_raw
    fine = fv_levels[lv]
    raw = amg_xwin_raw(fine)
    wide = amg_packed_mirror(fine)  # compact level: expanded by the library on the host
    assert raw is not None and wide is not None, "level %d has no packed mirror" % (lv + 1)
    monkeypatch.setenv("ORC_XWIN_COMPACT", "0")
    plain = amg_packed_mirror(fine)  # ... and stored wide in the first place
    raw_plain = amg_xwin_raw(fine)
    monkeypatch.delenv("ORC_XWIN_COMPACT")
    assert raw["pos_bits"] == 12 and raw["cap"] <= 4096
    assert raw_plain["pos_bits"] == 16 and raw_plain["blocks_col16"] == 0 and not raw_plain["wfmt"].any()
    pos, win = _decoded(raw)
    for img in (wide, plain):
        np.testing.assert_array_equal(raw["lptr"], img["lptr"])
        np.testing.assert_array_equal(raw["wsize"], img["wsize"])
        assert len(pos) == len(img["lidx"]) == raw["pos_slots"]
        np.testing.assert_array_equal(pos, img["lidx"])
        for b, w in enumerate(win):
            np.testing.assert_array_equal(w, img["wcol"][b, :len(w)])
    assert raw["wsize"].max() <= 4096  # (no position is stored modulo 4 096 here)
    # bytes: 1.5 per position slot; 2 per window entry and 4 per started segment of 64 in a 16-bit block (every block at this size)
    assert raw["pos_bytes"] == len(raw["pos_raw"]) == 3 * raw["pos_slots"] // 2
    assert raw_plain["pos_bytes"] == 2 * raw["pos_slots"]
    ws = raw["wsize"].astype(np.int64)
    assert raw["blocks_col16"] == int((ws > 0).sum()) and raw["blocks_col32"] == 0 and np.all(raw["wfmt"][ws > 0] == 1)
    assert raw["wcol_bytes"] == _expected_wcol_bytes(raw) == int((2 * ws[ws > 0] + 4 * ((ws[ws > 0] + 63) // 64)).sum())
    assert raw_plain["wcol_bytes"] == 4 * int(ws[ws > 0].sum())
    print("level %d: positions %d -> %d bytes, window columns %d -> %d bytes" % (lv + 1, raw_plain["pos_bytes"], raw["pos_bytes"], raw_plain["wcol_bytes"], raw["wcol_bytes"]))


# ---------------------------------------------------------------- 2. products bit for bit
@pytest.fixture(scope="module")
def big4096(gpu):
    """the 4 096-entry window (xwin_cases.big_window) and its coarse operator as the set-up builds it"""
    from orc_amd.linear_algebra import amg_coarsen
    cols = X.big_window(4096)
    fine = X.forced_pairs(cols)
    _, coarse, _ = amg_coarsen(fine)
    coarse = coarse.tocsr()
    coarse.sort_indices()
    indptr, indices = X.coarse_pattern(cols)
    np.testing.assert_array_equal(coarse.indptr, indptr)  # the pairing was the forced one: the pattern is the prescribed one
    np.testing.assert_array_equal(coarse.indices, indices)
    return fine, coarse


@pytest.mark.parametrize("cap", [4096, 2000, "median"])
def test_products_bit_exact_with_twelve_bit_positions(gpu, oracle, monkeypatch, big4096, cap):
    """cap 4096: block 0's window holds exactly 4 096 columns, position 4 095 (twelve one-bits) sits in every slot of a chunk; 2000: block 0
    gathers from global memory beside blocks with 12-bit positions; "median": the median window size of the other blocks, so about half of them do.  Row lengths 1, 7, 8, 9, 15, 16, 17 in
    slice 4, an empty row, a last slice of 37 rows, a last block of three slices."""
    from orc_amd.linear_algebra import amg_packed_mirror, amg_xwin_raw, xwin_counters
    fine, coarse = big4096
    nc = coarse.shape[0]
    lens = np.diff(coarse.indptr)
    assert nc % 64 == 37 and ((nc + 63) // 64) % 4 == 3
    assert set(X.SLICE_LENGTHS) <= set(lens[256:320].tolist()) and lens[4096 + 40] == 0
    monkeypatch.setenv("ORC_SPMV_XWIN_MIN_NNZ", "1")
    if cap == "median":
        sizes = amg_xwin_raw(fine)["wsize"][1:]
        cap = int(np.median(sizes))
        assert sizes.min() < cap < sizes.max()
    monkeypatch.setenv("ORC_XWIN_CAP", str(cap))
    raw = amg_xwin_raw(fine)
    assert raw["pos_bits"] == 12 and raw["cap"] == cap
    if cap == 4096:
        assert raw["wsize"][0] == 4096
        wide = amg_packed_mirror(fine)
        pos, _ = _decoded(raw)
        np.testing.assert_array_equal(pos, wide["lidx"])
        blk0 = pos[int(raw["lptr"][0]):int(raw["lptr"][4])]
        assert set((np.flatnonzero(blk0 == 4095) % 8).tolist()) == set(range(8)), "position 4095 does not reach every slot of a chunk"
    xwin_counters(reset=True)
    _check_products(oracle, monkeypatch, fine, coarse, 60 + cap % 50)
    blocks, over_cap, over_span = xwin_counters()
    assert over_span == 0
    if cap == 4096:
        assert over_cap == 0
    elif cap == 2000:
        assert over_cap == 4  # block 0 in each of the four set-ups (compact / wide, plain / scaled)
    else:
        assert 0.2 * blocks < over_cap < 0.8 * blocks


# ---------------------------------------------------------------- 3. mixed window-column formats
def test_blocks_take_their_column_format_by_the_span_of_a_segment(gpu, oracle, monkeypatch):
    """Block 3's list ends 65 535 columns above the base of its last segment (16 bits: fits), block 5's 65 536 above (does not): block 5 alone
    keeps 32-bit columns, its neighbours 4 and 6 and everybody else store 16-bit offsets; one launch multiplies both kinds."""
    from orc_amd.linear_algebra import amg_coarsen, amg_packed_mirror, amg_xwin_raw
    nc = 70000
    cols = X.tridiagonal_with_far(nc, {3: 65535, 5: 65536})
    fine = X.forced_pairs(cols)
    _, coarse, _ = amg_coarsen(fine)
    coarse = coarse.tocsr()
    coarse.sort_indices()
    indptr, indices = X.coarse_pattern(cols)
    np.testing.assert_array_equal(coarse.indptr, indptr)
    np.testing.assert_array_equal(coarse.indices, indices)
    monkeypatch.setenv("ORC_SPMV_XWIN_MIN_NNZ", "1")
    raw = amg_xwin_raw(fine)
    nb = (nc + 255) // 256
    assert len(raw["wfmt"]) == nb and np.all(raw["wsize"] > 0)
    for b, gap in ((3, 65535), (5, 65536)):
        w = coarse.indices[coarse.indptr[256 * b]:coarse.indptr[256 * b + 256]]
        w = np.unique(w)
        assert len(w) == 258 and w[257] - w[256] == gap and np.all(np.diff(w[:257]) == 1)  # entry 256 opens the fifth segment
    expect = np.ones(nb, np.int32)
    expect[5] = 0
    np.testing.assert_array_equal(raw["wfmt"], expect)
    assert raw["blocks_col16"] == nb - 1 and raw["blocks_col32"] == 1
    assert raw["wcol_bytes"] == _expected_wcol_bytes(raw)
    _, win = _decoded(raw)
    wide = amg_packed_mirror(fine)
    for b in (0, 2, 3, 4, 5, 6, nb - 1):
        np.testing.assert_array_equal(win[b], wide["wcol"][b, :len(win[b])])
        np.testing.assert_array_equal(win[b], np.unique(coarse.indices[coarse.indptr[256 * b]:coarse.indptr[min(nc, 256 * b + 256)]]))
    _check_products(oracle, monkeypatch, fine, coarse, 77)


# ---------------------------------------------------------------- 4. a level forced to the 5 000-entry share
def test_a_level_with_the_large_share_keeps_sixteen_bit_positions(gpu, oracle, monkeypatch):
    """Block 0's window holds 4 608 columns: more than 1 % of the level's blocks exceed every smaller share, the level takes 5 000 entries and
    its positions 16 bits (written by the set-up's second launch) — the window columns are 16-bit offsets all the same."""
    from orc_amd.linear_algebra import amg_coarsen, amg_packed_mirror, amg_xwin_raw
    cols = X.big_window(4608, nc=4608 + 2 * 64 + 37)
    fine = X.forced_pairs(cols, seed=9)
    _, coarse, _ = amg_coarsen(fine)
    coarse = coarse.tocsr()
    coarse.sort_indices()
    monkeypatch.setenv("ORC_SPMV_XWIN_MIN_NNZ", "1")
    raw = amg_xwin_raw(fine)
    assert raw["wsize"][0] == 4608 and raw["cap"] == 5000 and raw["pos_bits"] == 16
    assert raw["pos_bytes"] == 2 * raw["pos_slots"]
    ws = raw["wsize"]
    assert raw["blocks_col16"] == int((ws > 0).sum()) and raw["blocks_col32"] == 0
    wide = amg_packed_mirror(fine)
    pos, win = _decoded(raw)
    np.testing.assert_array_equal(pos, wide["lidx"])
    assert pos[int(raw["lptr"][0]):int(raw["lptr"][4])].max() == 4607
    for b, w in enumerate(win):
        np.testing.assert_array_equal(w, wide["wcol"][b, :len(w)])
    _check_products(oracle, monkeypatch, fine, coarse, 91)
    # The set-up now EXPECTS the large share of a level of this many rows and writes 16-bit positions first; a level of the same size with
    # small windows still ends up with 12 bits (rewritten), the same image and the same products.
    small = X.forced_pairs(X.big_window(1024, nc=len(cols)), seed=10)
    _, coarse_small, _ = amg_coarsen(small)
    coarse_small = coarse_small.tocsr()
    coarse_small.sort_indices()
    raw = amg_xwin_raw(small)
    assert raw["wsize"][0] == 1024 and raw["cap"] == 2048 and raw["pos_bits"] == 12 and raw["pos_bytes"] == 3 * raw["pos_slots"] // 2
    pos, _ = _decoded(raw)
    np.testing.assert_array_equal(pos, amg_packed_mirror(small)["lidx"])
    _check_products(oracle, monkeypatch, small, coarse_small, 92)
