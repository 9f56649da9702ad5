// amg_hooks.hip — test hooks: one level of the set-up (aggregate() + galerkin(), private functions of the reference) made observable.
//   amg_debug_coarsen   the pairing and the coarse operator in CSR, optionally a product with it as the solves multiply it (orc_amg_coarsen,
//                       orc_debug_amg_coarse_product)
//   amg_debug_packed    the level's packed mirror and windows copied to the host (orc_debug_amg_packed_mirror), compact streams expanded
//   amg_debug_xwin_raw  the windows' streams byte for byte as the products read them, and what they count (orc_debug_amg_xwin_raw)
// Both leave the arena as they found it on every exit (ArenaScope).
#include <algorithm>
#include <cstring>

#include "amg.hpp"

namespace orc {

// the first level of A's hierarchy, as multigrid_solve_dev builds it for itself
static int build_level(const MatView &A, Arena &arena, AmgHierarchy::Level &L) {
    const int64_t n = A.P.n;
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &L.choice));
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &L.chooser));
    ORC_TRY(aggregate(A, arena, L.choice, L.chooser, &L.rounds));
    return galerkin(A, arena, L);
}

// x_h / y_h (optional, [ceil(n / 2)]): y = Ac x with the coarse operator AS THE SOLVES MULTIPLY IT — launch_spmv on the level's view,
// i.e. the packed mirror + LDS window product wherever galerkin() built one.  scaled != 0: the view a smoothing solve launches
// (Jacobi scaling 1 / diag materialised into the streamed values: spmv_xwin_k<Epi, 0, false>), else the plain values
// (spmv_xwin_k<Epi>, what the residual checks launch).  *mirror_out: did the level get a window mirror at all?
int amg_debug_coarsen(const MatView &A, Arena &arena, std::vector<int> &choice_h, std::vector<int64_t> &row_ptr_h,
                      std::vector<int64_t> &col_h, std::vector<double> &val_h, int *rounds, const double *x_h, double *y_h, int scaled, int *mirror_out) {
    const int64_t n = A.P.n;
    hipStream_t st = ctx().stream;
    ArenaScope scope(arena);
    AmgHierarchy::Level L;
    ORC_TRY(build_level(A, arena, L));
    if (rounds) *rounds = L.rounds;
    choice_h.resize((size_t)n);
    ORC_HIP(hipMemcpyAsync(choice_h.data(), L.choice, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    const int64_t nc = L.n;
    if (mirror_out) *mirror_out = (L.pk.ptr && L.xw.lidx) ? 1 : 0;
    if (x_h && y_h && nc > 0) {
        MatView V = coarse_view(L, A.symmetric);
        double *x, *y, *d1;
        ORC_TRY(arena.alloc((size_t)nc, &x));
        ORC_TRY(arena.alloc((size_t)nc, &y));
        ORC_HIP(hipMemcpyAsync(x, x_h, sizeof(double) * (size_t)nc, hipMemcpyHostToDevice, st));
        if (scaled) {
            ORC_TRY(arena.alloc((size_t)nc, &d1));
            ORC_TRY(diag_inverse_dev(V, d1));
            V.s1 = d1;
            ORC_TRY(materialize_scaled_view(V, 50, arena));
        }
        ORC_TRY(spmv_dev(V, x, y));
        ORC_HIP(hipMemcpyAsync(y_h, y, sizeof(double) * (size_t)nc, hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
    }
    std::vector<int> row_len((size_t)nc), col((size_t)std::max<int64_t>(L.padded, 1));
    std::vector<int64_t> slice_ptr((size_t)L.P.n_slices + 1);
    std::vector<double> val((size_t)std::max<int64_t>(L.padded, 1));
    ORC_HIP(hipMemcpyAsync(row_len.data(), L.P.row_len, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(slice_ptr.data(), L.P.slice_ptr, sizeof(int64_t) * slice_ptr.size(), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(col.data(), L.P.col, sizeof(int) * (size_t)L.padded, hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(val.data(), L.val, sizeof(double) * (size_t)L.padded, hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    row_ptr_h.assign((size_t)nc + 1, 0);
    for (int64_t I = 0; I < nc; ++I) row_ptr_h[(size_t)I + 1] = row_ptr_h[(size_t)I] + row_len[(size_t)I];
    col_h.resize((size_t)row_ptr_h[(size_t)nc]);
    val_h.resize((size_t)row_ptr_h[(size_t)nc]);
    for (int64_t I = 0; I < nc; ++I) {
        const int64_t base = slice_ptr[(size_t)(I >> 6)] + (I & 63);
        for (int k = 0; k < row_len[(size_t)I]; ++k) {
            col_h[(size_t)(row_ptr_h[(size_t)I] + k)] = col[(size_t)(base + (int64_t)k * 64)];
            val_h[(size_t)(row_ptr_h[(size_t)I] + k)] = val[(size_t)(base + (int64_t)k * 64)];
        }
    }
    return ORC_OK;
}

// The compact window formats (XWinDev: pos12, wfmt) expanded on the host to the wide ones.  raw: the position stream, n_slots positions;
// words: one block's kXWinCap words of wcol.
static void expand_positions12(const unsigned *raw, int64_t n_slots, uint16_t *out) {
    for (int64_t g = 0; g < n_slots / kPackChunk; ++g) {
        const unsigned long long lo = raw[3 * g] | (unsigned long long)raw[3 * g + 1] << 32, hi = raw[3 * g + 1] >> 16 | (unsigned long long)raw[3 * g + 2] << 16;
        for (int u = 0; u < 4; ++u) {
            out[kPackChunk * g + u] = (uint16_t)(lo >> (12 * u) & 0xfffu);
            out[kPackChunk * g + 4 + u] = (uint16_t)(hi >> (12 * u) & 0xfffu);
        }
    }
}
static void expand_window16(int32_t *words, int ws) {
    const int nseg = (ws + kXWinSeg - 1) / kXWinSeg;
    const std::vector<int32_t> base(words, words + nseg);
    std::vector<uint16_t> off((size_t)ws);
    memcpy(off.data(), words + nseg, sizeof(uint16_t) * (size_t)ws);
    for (int j = 0; j < ws; ++j) words[j] = base[(size_t)(j / kXWinSeg)] + (int32_t)off[(size_t)j];
}
// bytes of a level's position stream
static size_t position_bytes(const XWinDev &xw, int64_t n_slots) { return (size_t)n_slots * (xw.pos12 ? 3 : 4) / 2; }

// One level of the set-up on A, as amg_debug_coarsen, and the level's packed mirror and windows copied to the host (PackedDev, XWinDev):
// sizes = {coarse rows, slices, value slots, position slots, blocks}; with any output pointer null only the sizes are written.
// lidx_h and wcol_h are the WIDE image whatever the level stores: 16-bit positions, 32-bit columns.
int amg_debug_packed(const MatView &A, Arena &arena, int64_t sizes[5], int32_t *row_len_h, int64_t *pk_ptr_h, int32_t *pk_col_h, double *pk_val_h,
                     int64_t *lptr_h, uint16_t *lidx_h, int32_t *wcol_h, int32_t *wsize_h) {
    hipStream_t st = ctx().stream;
    ArenaScope scope(arena);
    AmgHierarchy::Level L;
    ORC_TRY(build_level(A, arena, L));
    const bool mirror = L.pk.ptr && L.xw.lidx;
    const int64_t ns = L.P.n_slices, nb = (ns + 3) / 4;
    sizes[0] = L.n; sizes[1] = ns; sizes[2] = mirror ? L.pk.slots : 0; sizes[3] = 0; sizes[4] = mirror ? nb : 0;
    if (mirror) ORC_HIP(hipMemcpyAsync(&sizes[3], L.xw.lptr + ns, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    if (mirror && row_len_h && pk_ptr_h && pk_col_h && pk_val_h && lptr_h && lidx_h && wcol_h && wsize_h) {
        ORC_HIP(hipMemcpyAsync(row_len_h, L.P.row_len, sizeof(int32_t) * (size_t)L.n, hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(pk_ptr_h, L.pk.ptr, sizeof(int64_t) * (size_t)(ns + 1), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(pk_col_h, L.pk.col, sizeof(int32_t) * (size_t)sizes[2], hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(pk_val_h, L.pk.val, sizeof(double) * (size_t)sizes[2], hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(lptr_h, L.xw.lptr, sizeof(int64_t) * (size_t)(ns + 1), hipMemcpyDeviceToHost, st));
        std::vector<unsigned> raw(L.xw.pos12 ? position_bytes(L.xw, sizes[3]) / 4 : 0);
        std::vector<int32_t> wfmt((size_t)nb);
        if (L.xw.pos12) ORC_HIP(hipMemcpyAsync(raw.data(), L.xw.lidx, position_bytes(L.xw, sizes[3]), hipMemcpyDeviceToHost, st));
        else ORC_HIP(hipMemcpyAsync(lidx_h, L.xw.lidx, sizeof(uint16_t) * (size_t)sizes[3], hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(wcol_h, L.xw.wcol, sizeof(int32_t) * (size_t)(nb * kXWinCap), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(wsize_h, L.xw.wsize, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(wfmt.data(), L.xw.wfmt, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        if (L.xw.pos12) expand_positions12(raw.data(), sizes[3], lidx_h);
        for (int64_t b = 0; b < nb; ++b)
            if (wfmt[(size_t)b] && wsize_h[b] > 0) expand_window16(wcol_h + b * kXWinCap, wsize_h[b]);
    }
    return ORC_OK;
}

// The same level's window streams as they are stored.  info = {coarse rows, slices, blocks, position slots, bits per position (12 / 16; 0: no
// mirror), bytes of the position stream, the level's LDS share in entries, blocks with 16-bit columns, blocks with a window and 32-bit columns,
// bytes of window columns a product reads (4 per entry, or 2 per entry and 4 per started segment of 64)}; the arrays (lptr [slices + 1],
// pos_raw [bytes of the position stream], wcol_raw [blocks * kXWinCap words], wsize / wfmt [blocks]) are written only if none is null.
int amg_debug_xwin_raw(const MatView &A, Arena &arena, int64_t info[10], int64_t *lptr_h, unsigned char *pos_raw_h, int32_t *wcol_raw_h, int32_t *wsize_h, int32_t *wfmt_h) {
    hipStream_t st = ctx().stream;
    ArenaScope scope(arena);
    AmgHierarchy::Level L;
    ORC_TRY(build_level(A, arena, L));
    const bool mirror = L.pk.ptr && L.xw.lidx;
    const int64_t ns = L.P.n_slices, nb = (ns + 3) / 4;
    for (int i = 0; i < 10; ++i) info[i] = 0;
    info[0] = L.n; info[1] = ns;
    if (!mirror) return ORC_OK;
    std::vector<int32_t> wsize((size_t)nb), wfmt((size_t)nb);
    ORC_HIP(hipMemcpyAsync(&info[3], L.xw.lptr + ns, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(wsize.data(), L.xw.wsize, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(wfmt.data(), L.xw.wfmt, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    info[2] = nb; info[4] = L.xw.pos12 ? 12 : 16; info[5] = (int64_t)position_bytes(L.xw, info[3]); info[6] = L.xw.cap;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t ws = wsize[(size_t)b];
        if (ws <= 0) continue;
        if (wfmt[(size_t)b]) { ++info[7]; info[9] += 2 * ws + 4 * ((ws + kXWinSeg - 1) / kXWinSeg); }
        else { ++info[8]; info[9] += 4 * ws; }
    }
    if (lptr_h && pos_raw_h && wcol_raw_h && wsize_h && wfmt_h) {
        ORC_HIP(hipMemcpyAsync(lptr_h, L.xw.lptr, sizeof(int64_t) * (size_t)(ns + 1), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(pos_raw_h, L.xw.lidx, (size_t)info[5], hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(wcol_raw_h, L.xw.wcol, sizeof(int32_t) * (size_t)(nb * kXWinCap), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        std::copy(wsize.begin(), wsize.end(), wsize_h);
        std::copy(wfmt.begin(), wfmt.end(), wfmt_h);
    }
    return ORC_OK;
}

}  // namespace orc
