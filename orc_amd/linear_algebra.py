"""linear_algebra::iterative_solve of the reference (src/linear_algebra.rs:144-299) on MI355X."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def iterative_solve(a, b, solution_vector, iteration_count, method, relaxation_factor, convergence_threshold,
                    preconditioner, raise_on_error=True):
    """a: scipy.sparse CSR (sorted columns); solution_vector (float64, contiguous) is updated in place,
    like `&mut DVector` in the reference. Returns the status code (0 = ok)."""
    a = a.tocsr()
    a.sort_indices()
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    b = _f64(b)
    assert solution_vector.dtype == np.float64 and solution_vector.flags.c_contiguous
    st = lib().orc_iterative_solve(C.c_int64(a.shape[0]), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double),
                                   _p(b, C.c_double), _p(solution_vector, C.c_double), C.c_uint64(iteration_count),
                                   C.c_int(method), C.c_double(relaxation_factor), C.c_double(convergence_threshold),
                                   C.c_int(preconditioner))
    if raise_on_error:
        check(st)
    return st


def iterative_solve3(a_list, b_list, x_list, iteration_count, method, relaxation_factor, convergence_threshold, preconditioner):
    """orc_iterative_solve3: three systems on ONE pattern (scipy CSR matrices with identical indptr / indices) in lock-step;
    x_list is updated in place.  Returns (status, [status per system])."""
    a0 = a_list[0]
    n = a0.shape[0]
    rp, ci = _i64(a0.indptr), _i64(a0.indices)
    for a in a_list[1:]:
        assert np.array_equal(a.indptr, a0.indptr) and np.array_equal(a.indices, a0.indices), "the three systems must share their pattern"
    vals = [_f64(a.data) for a in a_list]
    bs = [_f64(b) for b in b_list]
    for x in x_list:
        assert x.dtype == np.float64 and x.flags.c_contiguous and len(x) == n
    PD = C.POINTER(C.c_double)
    v3 = (PD * 3)(*[_p(v, C.c_double) for v in vals])
    b3 = (PD * 3)(*[_p(b, C.c_double) for b in bs])
    x3 = (PD * 3)(*[_p(x, C.c_double) for x in x_list])
    st3 = (C.c_int * 3)()
    st = lib().orc_iterative_solve3(C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), v3, b3, x3, C.c_uint64(iteration_count), C.c_int(method),
                                    C.c_double(relaxation_factor), C.c_double(convergence_threshold), C.c_int(preconditioner), st3)
    return st, [st3[0], st3[1], st3[2]]


def set_breakdown_guard(on):
    """process-wide OrcSettings.breakdown_guard for iterative_solve (default on); off = NaN like the reference"""
    check(lib().orc_set_breakdown_guard(C.c_int(1 if on else 0)))


def set_reduction_order(order):
    """process-wide OrcSettings.reduction_order for iterative_solve: 0 = wave trees (default), 1 = the reference's
    (nalgebra dotx) association, bit-identical iterates (verification mode)"""
    check(lib().orc_set_reduction_order(C.c_int(int(order))))


def breakdown_guard_events(reset=False):
    """BiCGSTAB solves in which the breakdown guard fired since the last reset (the reference would have returned NaN)"""
    lib().orc_breakdown_guard_events.restype = C.c_int64
    return int(lib().orc_breakdown_guard_events(C.c_int(1 if reset else 0)))


def last_jacobi_sweeps():
    return lib().orc_last_jacobi_sweeps()


def set_gmres_restart(m):
    """process-wide OrcSettings.gmres_restart for iterative_solve: 0 = the default (30), 1..64; anything else makes the GMRES
    arm fail with ORC_ERR_BAD_ARGUMENT"""
    check(lib().orc_set_gmres_restart(C.c_int(int(m))))


def last_gmres_stats():
    """(Arnoldi steps, cycles, beta0, final residual estimate |g|) of the last iterative_solve's GMRES arm"""
    steps, cycles = C.c_int64(0), C.c_int64(0)
    beta0, est = C.c_double(0.0), C.c_double(0.0)
    check(lib().orc_last_gmres_stats(C.byref(steps), C.byref(cycles), C.byref(beta0), C.byref(est)))
    return steps.value, cycles.value, beta0.value, est.value


def last_cg_stats():
    """(completed iterations, beta0, final recurrence residual |r|, event: 0 none, 1 p.q <= 0, 2 non-finite) of the last CG solve"""
    its, ev = C.c_int64(0), C.c_int32(0)
    beta0, res = C.c_double(0.0), C.c_double(0.0)
    check(lib().orc_last_cg_stats(C.byref(its), C.byref(beta0), C.byref(res), C.byref(ev)))
    return its.value, beta0.value, res.value, ev.value


def csr_spmv(a, x, reps=1):
    """y = A x on the device; returns (y, avg_ms_per_launch)."""
    a = a.tocsr()
    a.sort_indices()
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    x = _f64(x)
    y = np.empty(a.shape[0])
    ms = C.c_double(0.0)
    check(lib().orc_csr_spmv(C.c_int64(a.shape[0]), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double),
                             _p(x, C.c_double), _p(y, C.c_double), C.c_int(reps), C.byref(ms)))
    return y, ms.value


def amg_coarsen(a):
    """Test hook: (partner[n], coarse CSR a' = (R a) R^T, rounds) of the device Multigrid set-up."""
    import scipy.sparse as sp
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    partner = np.empty(n, np.int64)
    nc, nnz, rounds = C.c_int64(0), C.c_int64(0), C.c_int(0)
    args = (C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double), _p(partner, C.c_int64), C.byref(nc), C.byref(nnz))
    check(lib().orc_amg_coarsen(*args, None, None, None, C.byref(rounds)))
    orp, oci, ov = np.empty(nc.value + 1, np.int64), np.empty(nnz.value, np.int64), np.empty(nnz.value)
    check(lib().orc_amg_coarsen(*args, _p(orp, C.c_int64), _p(oci, C.c_int64), _p(ov, C.c_double), C.byref(rounds)))
    return partner, sp.csr_matrix((ov, oci, orp), shape=(nc.value, nc.value)), rounds.value


def debug_coloring(a):
    """Test hook: (colors[n], n_colors) of the multicolour Gauss-Seidel extension for the pattern of `a`."""
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci = _i64(a.indptr), _i64(a.indices)
    colors = np.empty(n, np.int32)
    nc = C.c_int32(0)
    check(lib().orc_debug_coloring(C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(colors, C.c_int32), C.byref(nc)))
    return colors, nc.value


def amg_coarse_product(a, x, scaled=False):
    """Test hook: y = a' x with a' = (R a) R^T launched as the Multigrid solves launch it (packed mirror + LDS x windows where the
    set-up builds them); x has ceil(n / 2) entries.  Returns (y, has_window_mirror)."""
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    x = _f64(x)
    assert len(x) == (n + 1) // 2
    y = np.empty(len(x))
    mirror = C.c_int(0)
    check(lib().orc_debug_amg_coarse_product(C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double), C.c_int(1 if scaled else 0),
                                             _p(x, C.c_double), _p(y, C.c_double), C.byref(mirror)))
    return y, bool(mirror.value)


def amg_packed_mirror(a):
    """Test hook: the coarse level of a (as amg_coarsen builds it) as its products read it — the packed mirror and the LDS x windows.
    Returns None when the level has no mirror, else a dict of row_len, pk_ptr, pk_col, pk_val, lptr, lidx, wcol ([blocks, 5000]), wsize."""
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    sizes = np.zeros(5, np.int64)
    f = lib().orc_debug_amg_packed_mirror
    null = [None] * 8
    check(f(C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double), _p(sizes, C.c_int64), *null))
    nc, ns, slots, pos_slots, nb = (int(t) for t in sizes)
    if slots == 0:
        return None
    out = dict(row_len=np.empty(nc, np.int32), pk_ptr=np.empty(ns + 1, np.int64), pk_col=np.empty(slots, np.int32), pk_val=np.empty(slots),
               lptr=np.empty(ns + 1, np.int64), lidx=np.empty(pos_slots, np.uint16), wcol=np.empty((nb, 5000), np.int32), wsize=np.empty(nb, np.int32))
    check(f(C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double), _p(sizes, C.c_int64), _p(out["row_len"], C.c_int32),
            _p(out["pk_ptr"], C.c_int64), _p(out["pk_col"], C.c_int32), _p(out["pk_val"], C.c_double), _p(out["lptr"], C.c_int64),
            _p(out["lidx"], C.c_uint16), _p(out["wcol"], C.c_int32), _p(out["wsize"], C.c_int32)))
    return out


def xwin_unpack_positions(raw, bits):
    """The window positions of a raw position stream (amg_xwin_raw) as uint16: 16-bit positions as they are; 12-bit ones from granules
    of 12 bytes that hold eight positions, position u in bits [12 u, 12 u + 12) of the granule's 96 (little-endian)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    if bits == 16:
        return raw.view(np.uint16).copy()
    assert bits == 12 and len(raw) % 12 == 0
    w = raw.view(np.uint32).reshape(-1, 3).astype(np.uint64)
    lo = w[:, 0] | (w[:, 1] << np.uint64(32))            # bits 0..63
    hi = (w[:, 1] >> np.uint64(16)) | (w[:, 2] << np.uint64(16))  # bits 48..95
    out = np.empty((len(w), 8), np.uint16)
    for u in range(4):
        out[:, u] = (lo >> np.uint64(12 * u)) & np.uint64(0xfff)
        out[:, 4 + u] = (hi >> np.uint64(12 * u)) & np.uint64(0xfff)
    return out.reshape(-1)


def xwin_unpack_window(words, wsize, fmt):
    """The wsize ascending columns of one block's window from its words of the raw column stream (amg_xwin_raw): fmt 0 — the columns
    themselves; fmt 1 — ceil(wsize / 64) bases, then wsize 16-bit offsets from the base of the entry's segment of 64."""
    words = np.ascontiguousarray(words, np.int32)
    if wsize <= 0:
        return np.empty(0, np.int32)
    if not fmt:
        return words[:wsize].copy()
    nseg = (wsize + 63) // 64
    off = words[nseg:nseg + (wsize + 1) // 2].view(np.uint16)[:wsize].astype(np.int32)
    return words[:nseg][np.arange(wsize) // 64] + off


def amg_xwin_raw(a):
    """Test hook: the window streams of the coarse level of a (as amg_coarsen builds it) byte for byte as its products read them.
    Returns None when the level has no mirror, else a dict: pos_bits (12 / 16), pos_bytes, cap (the level's LDS share), blocks_col16 /
    blocks_col32 (blocks with a window by column format), wcol_bytes (what a product reads of the column lists), pos_slots, lptr,
    pos_raw (uint8), wcol_raw ([blocks, 5000] int32 words), wsize, wfmt."""
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    rp, ci, v = _i64(a.indptr), _i64(a.indices), _f64(a.data)
    info = np.zeros(10, np.int64)
    f = lib().orc_debug_amg_xwin_raw
    head = (C.c_int64(n), _p(rp, C.c_int64), _p(ci, C.c_int64), _p(v, C.c_double), _p(info, C.c_int64))
    check(f(*head, None, None, None, None, None))
    nc, ns, nb, pos_slots, bits, pos_bytes = (int(t) for t in info[:6])
    if nb == 0:
        return None
    out = dict(lptr=np.empty(ns + 1, np.int64), pos_raw=np.empty(pos_bytes, np.uint8), wcol_raw=np.empty((nb, 5000), np.int32),
               wsize=np.empty(nb, np.int32), wfmt=np.empty(nb, np.int32))
    check(f(*head, _p(out["lptr"], C.c_int64), _p(out["pos_raw"], C.c_uint8), _p(out["wcol_raw"], C.c_int32), _p(out["wsize"], C.c_int32),
            _p(out["wfmt"], C.c_int32)))
    out.update(pos_bits=int(info[4]), pos_bytes=int(info[5]), cap=int(info[6]), blocks_col16=int(info[7]), blocks_col32=int(info[8]),
               wcol_bytes=int(info[9]), pos_slots=pos_slots)
    return out


def xwin_counters(reset=False):
    """Test hook: (blocks described, blocks without a window because of the cap, ... because of the column span) since the last reset"""
    out = (C.c_longlong * 3)()
    check(lib().orc_debug_xwin_counters(out, C.c_int(1 if reset else 0)))
    return out[0], out[1], out[2]


def shared_galerkin(reset=False):
    """Test hook: sibling coarse operators built by a shared Galerkin pass since the last reset (two per lock-step momentum solve)"""
    f = lib().orc_debug_shared_galerkin
    f.restype = C.c_longlong
    return int(f(C.c_int(1 if reset else 0)))


def amg_certification(reset=False):
    """Test hook: (aggregations certified after their cascades, certification rounds in total); equal = nothing was changed"""
    out = (C.c_longlong * 2)()
    check(lib().orc_debug_amg_certification(out, C.c_int(1 if reset else 0)))
    return out[0], out[1]


AMG_SETUP_FIELDS = ("list", "steps", "scans", "longest", "overflow", "changed", "fallback_sweeps", "lanes")  # include/orc_amd.h out[0..7]


def amg_setup_stats(reset=False):
    """Test hook: what the most recent pairing and Galerkin product of this process did (orc_debug_amg_setup_stats; not cumulative): the
    fields above, `fallback` (did the slice-sequential sweeps run?), `tiers` (coarse rows per LDS tier, 7 entries) and `max_cand`"""
    out = (C.c_longlong * 16)()
    check(lib().orc_debug_amg_setup_stats(out, C.c_int(1 if reset else 0)))
    d = dict(zip(AMG_SETUP_FIELDS, (int(v) for v in out[:8])))
    d["fallback"] = 1 if d["fallback_sweeps"] > 0 else 0
    d["tiers"] = [int(v) for v in out[8:15]]
    d["max_cand"] = int(out[15])
    return d


PRODUCT_FAMILIES = ("ragged", "packed", "window", "generic_scaled", "wide", "narrow", "narrow_nt", "mesh")  # include/orc_amd.h ORC_PRODUCT_*


def product_launches(reset=False):
    """Test hook: {family: product launches since the last reset} (orc_debug_product_launches; the families are launch_spmv's kernels)"""
    out = (C.c_longlong * len(PRODUCT_FAMILIES))()
    n = lib().orc_debug_product_launches(out, C.c_int(len(PRODUCT_FAMILIES)), C.c_int(1 if reset else 0))
    if n != len(PRODUCT_FAMILIES):
        raise RuntimeError("orc_debug_product_launches: %d families, %d expected" % (n, len(PRODUCT_FAMILIES)))
    return dict(zip(PRODUCT_FAMILIES, (int(v) for v in out)))
