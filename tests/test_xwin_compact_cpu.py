"""Host-side halves of the compact window formats' tests (no GPU): the decoders of the raw streams (orc_amd.linear_algebra.xwin_unpack_positions /
xwin_unpack_window) against encoders written out independently here, and the claims of tests/xwin_cases.py — the forced pairing, the
prescribed coarse pattern, the window sizes and where the largest position lands — re-derived with the plain references of tests/amg_cases.py."""
import numpy as np

import amg_cases as A
import xwin_cases as X


def _pack12(pos):
    """eight positions -> 12 bytes: one 96-bit little-endian integer, position u at bit 12 u"""
    out = bytearray()
    for g in range(0, len(pos), 8):
        out += sum(int(p) << (12 * u) for u, p in enumerate(pos[g:g + 8])).to_bytes(12, "little")
    return np.frombuffer(bytes(out), np.uint8)


def test_unpack_positions_inverts_the_twelve_bit_granules():
    from orc_amd.linear_algebra import xwin_unpack_positions
    rng = np.random.default_rng(3)
    pos = rng.integers(0, 4096, 64 * 8).astype(np.uint16)
    pos[:8] = 4095
    pos[8:16] = 0
    for u in range(8):  # one position of twelve one-bits among zeros, in every slot: the neighbours must stay zero
        pos[16 + 8 * u:24 + 8 * u] = 0
        pos[16 + 8 * u + u] = 4095
    np.testing.assert_array_equal(xwin_unpack_positions(_pack12(pos), 12), pos)
    np.testing.assert_array_equal(xwin_unpack_positions(pos.view(np.uint8), 16), pos)


def test_unpack_window_inverts_bases_and_offsets():
    from orc_amd.linear_algebra import xwin_unpack_window
    rng = np.random.default_rng(4)
    for ws in (1, 63, 64, 65, 127, 128, 129, 4999, 5000):
        nseg = (ws + 63) // 64
        segs = []
        for s in range(nseg):  # every segment of two or more entries spans exactly 65 535 columns
            m = min(64, ws - 64 * s)
            o = np.sort(rng.choice(np.arange(1, 65535), m, replace=False))
            o[0] = 0
            if m > 1:
                o[-1] = 65535
            segs.append(70000 * (s + 1) + o)
        cols = np.concatenate(segs).astype(np.int32)
        assert np.all(np.diff(cols) > 0)
        words = np.zeros(5000, np.int32)
        words[:nseg] = cols[::64]
        off = (cols - np.repeat(cols[::64], 64)[:ws]).astype(np.uint16)
        words[nseg:].view(np.uint16)[:ws] = off
        np.testing.assert_array_equal(xwin_unpack_window(words, ws, 1), cols)
        wide = np.zeros(5000, np.int32)
        wide[:ws] = cols
        np.testing.assert_array_equal(xwin_unpack_window(wide, ws, 0), cols)
    assert len(xwin_unpack_window(np.zeros(5000, np.int32), -1, 0)) == 0


def _coarse(cols):
    a = X.forced_pairs(cols)
    partner, _ = A.greedy_pairing(a)
    n = a.shape[0]
    empty = np.array([c is None for c in cols]).repeat(2)
    np.testing.assert_array_equal(partner[~empty], (np.arange(n) ^ 1)[~empty])  # the forced pairs
    assert np.all(partner[empty] == -1)
    ac = A.exact_coarse(a, partner)
    indptr, indices = X.coarse_pattern(cols)
    np.testing.assert_array_equal(ac.indptr, indptr)
    np.testing.assert_array_equal(ac.indices, indices)
    return ac


def _windows(ac):
    nc = ac.shape[0]
    return [np.unique(ac.indices[ac.indptr[b]:ac.indptr[min(nc, b + 256)]]) for b in range(0, nc, 256)]


def test_big_window_case_is_what_it_claims():
    for window in (4096, 4608):
        cols = X.big_window(window, nc=window + 2 * 64 + 37)
        ac = _coarse(cols)
        nc = ac.shape[0]
        assert nc % 64 == 37 and ((nc + 63) // 64) % 4 == 3
        win = _windows(ac)
        np.testing.assert_array_equal(win[0], np.arange(window))
        sizes = np.array([len(w) for w in win[1:]])
        assert sizes.max() < 2000 and sizes.min() < int(np.median(sizes)) < sizes.max()
        # the largest position is the last entry of rows whose last entry sits in slot 0 ... 7 of a chunk of eight
        lens = np.diff(ac.indptr)
        slots = {(lens[I] - 1) % 8 for I in range(256) if lens[I] and ac.indices[ac.indptr[I + 1] - 1] == window - 1}
        assert slots == set(range(8))
        assert set(X.SLICE_LENGTHS) <= set(lens[256:320].tolist()) and lens[window + 40] == 0


def test_far_column_case_is_what_it_claims():
    cols = X.tridiagonal_with_far(2048 + 65536 + 300, {3: 65535, 5: 65536})
    ac = _coarse(cols)
    win = _windows(ac)
    for b, w in enumerate(win[:8]):
        wide = any(w[j] - w[j & ~63] > 65535 for j in range(len(w)))
        assert wide == (b == 5)
    for b, gap in ((3, 65535), (5, 65536)):
        assert len(win[b]) == 258 and win[b][257] - win[b][256] == gap
