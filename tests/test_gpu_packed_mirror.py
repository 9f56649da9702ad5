"""The packed mirror of the coarse levels in its lane-major chunks (PackedDev, XWinDev in orc_amd/csrc/linalg.hpp), read back and
decoded on the host: it must hold exactly the (row, k, column, value) entries of the coarse operator — the depth-major mirror's
content, which is the CSR form amg_coarsen returns — with every window position pointing at the entry's column, and pay no more
bytes than the granules say: a row owns pairs of value slots (one padding slot when its length is odd) and chunks of 8 window
positions, a slice starts on 128 bytes."""
import numpy as np
import pytest

from conftest import fv_like_matrix

pytestmark = pytest.mark.gpu

CHUNK = 8


def _levels(shape):
    from orc_amd.linear_algebra import amg_coarsen
    out = [fv_like_matrix(*shape)]
    for _ in range(3):
        _, ac, _ = amg_coarsen(out[-1])
        out.append(ac.tocsr())
    return out


def _decode(m, n):
    """(rows, depths, value slots, position slots) of every stored entry, padding included, from the chunked layout"""
    row_len, pk_ptr, lptr = m["row_len"], m["pk_ptr"], m["lptr"]
    rows, ks, vslot, pslot = [], [], [], []
    for s in range(len(pk_ptr) - 1):
        lens = row_len[s * 64:min(n, s * 64 + 64)]
        width = int(lens.max()) if len(lens) else 0
        off, poff = int(pk_ptr[s]), int(lptr[s])
        for j in range(0, width, CHUNK):
            lanes = np.nonzero(lens > j)[0]
            for u in range(CHUNK):
                rows.append(s * 64 + lanes)
                ks.append(np.full(len(lanes), j + u))
                pslot.append(poff + CHUNK * np.arange(len(lanes)) + u)
            poff += CHUNK * len(lanes)
            for q in range(CHUNK // 2):
                lanes = np.nonzero(lens > j + 2 * q)[0]
                for t in range(2):
                    vslot.append(off + 2 * np.arange(len(lanes)) + t)
                off += 2 * len(lanes)
        assert off <= pk_ptr[s + 1] and poff <= lptr[s + 1]
    rows, ks, pslot = np.concatenate(rows), np.concatenate(ks), np.concatenate(pslot)
    # the value slots were listed per pair: re-key them by (row, depth) in the order of the position walk
    vrows, vks = [], []
    for s in range(len(pk_ptr) - 1):
        lens = row_len[s * 64:min(n, s * 64 + 64)]
        width = int(lens.max()) if len(lens) else 0
        for j in range(0, width, CHUNK):
            for q in range(CHUNK // 2):
                lanes = np.nonzero(lens > j + 2 * q)[0]
                for t in range(2):
                    vrows.append(s * 64 + lanes)
                    vks.append(np.full(len(lanes), j + 2 * q + t))
    return rows, ks, pslot, np.concatenate(vrows), np.concatenate(vks), np.concatenate(vslot)


@pytest.mark.parametrize("lv", [1, 2])
def test_chunked_mirror_holds_the_coarse_operator(gpu, lv):
    from orc_amd.linear_algebra import amg_packed_mirror
    levels = _levels((96, 64, 16))
    fine, coarse = levels[lv], levels[lv + 1]
    coarse.sort_indices()
    m = amg_packed_mirror(fine)
    assert m is not None, "level %d has no packed mirror" % (lv + 1)
    n = coarse.shape[0]
    lens = np.diff(coarse.indptr).astype(np.int64)
    np.testing.assert_array_equal(m["row_len"], lens)
    assert np.all(m["pk_ptr"] % 16 == 0) and np.all(m["lptr"] % 64 == 0)  # 128-byte slice starts

    prow, pk, pslot, vrow, vk, vslot = _decode(m, n)
    # values and columns: every (row, k < len) is the CSR's k-th entry of the row, bit for bit; the padding slot of an odd row is finite
    real = vk < lens[vrow]
    src = coarse.indptr[vrow[real]] + vk[real]
    np.testing.assert_array_equal(m["pk_col"][vslot[real]], coarse.indices[src])
    np.testing.assert_array_equal(m["pk_val"][vslot[real]].view(np.uint64), coarse.data[src].view(np.uint64))
    assert real.sum() == coarse.nnz and len(np.unique(vslot)) == len(vslot)
    pad = ~real
    assert np.all(vk[pad] == lens[vrow[pad]]) and np.all(lens[vrow[pad]] % 2 == 1)
    assert np.all(np.isfinite(m["pk_val"][vslot[pad]]))
    assert np.all((m["pk_col"][vslot[pad]] >= 0) & (m["pk_col"][vslot[pad]] < n))
    # window positions: in a block with a window, position -> the entry's column; past the row's end, 0
    blk = prow // 256
    ws = m["wsize"][blk]
    win = ws >= 0
    real = pk < lens[prow]
    pos = m["lidx"][pslot].astype(np.int64)
    sel = win & real
    np.testing.assert_array_equal(m["wcol"][blk[sel], pos[sel]], coarse.indices[coarse.indptr[prow[sel]] + pk[sel]])
    assert np.all(pos[sel] < ws[sel])
    assert np.all(pos[win & ~real] == 0)
    assert win.mean() > 0.9  # (the test-size default: every block has its window)

    # bytes against the depth-major mirror (per slice the entries rounded up to 16, 8 + 2 bytes each): what the granules add, and no more
    ns = len(m["pk_ptr"]) - 1
    old = sum(((int(lens[s * 64:s * 64 + 64].sum()) + 15) // 16) * 16 for s in range(ns)) * 10
    new = int(m["pk_ptr"][-1]) * 8 + int(m["lptr"][-1]) * 2
    granules = int((lens % 2).sum()) * 8 + int(((-lens) % CHUNK).sum()) * 2
    assert old <= new <= old + granules + ns * (15 * 8 + 63 * 2)
    print("level %d: %.1f entries per row, mirror %+.2f %% bytes (pairs %.2f %%, position chunks %.2f %%)"
          % (lv + 1, lens.mean(), 100. * (new / old - 1), 100. * (lens % 2).sum() * 8 / old, 100. * ((-lens) % CHUNK).sum() * 2 / old))
