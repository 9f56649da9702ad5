// gs_layout.hip — the colour-sorted layout of a coloured pattern (SortedLayout, gs.hpp), built on the device, and the values of
// a solve in it.  Slot of a row = first slot of its colour + its rank inside the colour by ascending row; rank = rows of that
// colour in earlier 64-row blocks (column scan of a [blocks x colours] count table) + rows of that colour before it in its
// own block (ballot).
#include "gs.hpp"

namespace orc {

__global__ __launch_bounds__(64) void gs_block_counts_k(const int *__restrict__ color, int64_t n, int n_colors, int *__restrict__ table,
                                                        int *__restrict__ intra) {
    const int lane = threadIdx.x;
    const int64_t n_blocks = (n + 63) / 64;
    for (int64_t bidx = blockIdx.x; bidx < n_blocks; bidx += gridDim.x) {
        const int64_t i = bidx * 64 + lane;
        const int c = i < n ? color[i] : -1;
        for (int q = 0; q < n_colors; ++q) {
            const unsigned long long m = __ballot(c == q);
            if (c == q) intra[i] = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) table[bidx * n_colors + q] = __popcll(m);
        }
    }
}
// One step of a scan over more than a workgroup's width: *carry + the inclusive Hillis-Steele prefix sum of the workgroup's v
// (kWidth threads; buf: kWidth entries of LDS), and *carry grows by the workgroup's total.  Every thread of the workgroup calls it.
template <int kWidth, class T>
__device__ __forceinline__ T block_scan_carry(T v, T *buf, T *carry) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kWidth; off <<= 1) {
        const T t = (int)threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
        __syncthreads();
        buf[threadIdx.x] += t;
        __syncthreads();
    }
    const T out = *carry + buf[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == kWidth - 1) *carry += buf[kWidth - 1];
    __syncthreads();
    return out;
}
// exclusive scan down every column of the table: one workgroup per colour
__global__ __launch_bounds__(1024) void gs_column_scan_k(int *__restrict__ table, int64_t n_blocks, int n_colors) {
    __shared__ int carry;
    __shared__ int buf[1024];
    const int q = blockIdx.x;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_blocks; base += 1024) {
        const int64_t e = base + threadIdx.x;
        const int v = e < n_blocks ? table[e * n_colors + q] : 0;
        const int incl = block_scan_carry<1024>(v, buf, &carry);
        if (e < n_blocks) table[e * n_colors + q] = incl - v;
    }
}
__global__ void gs_assign_slots_k(SellDev P, const int *__restrict__ color, const int *__restrict__ table, const int *__restrict__ intra, int n_colors,
                                  const int *__restrict__ color_first_slot, int *__restrict__ slot_of_row, int *__restrict__ rowid, int *__restrict__ len_p) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = color[i];
        const int slot = color_first_slot[c] + table[(i >> 6) * n_colors + c] + intra[i];
        slot_of_row[i] = slot;
        rowid[slot] = (int)i;
        len_p[slot] = P.row_len[i];
    }
}
// slice_ptr[s + 1] = 64 x the widths (longest row) of the slices 0 .. s: one workgroup
__global__ __launch_bounds__(1024) void gs_slice_ptr_k(const int *__restrict__ len_p, int n_slices, int64_t *__restrict__ slice_ptr) {
    __shared__ long long carry;
    __shared__ long long buf[1024];
    if (threadIdx.x == 0) { carry = 0; slice_ptr[0] = 0; }
    __syncthreads();
    for (int base = 0; base < n_slices; base += 1024) {
        const int sidx = base + threadIdx.x;
        long long w = 0;
        if (sidx < n_slices) {
            int mx = 0;
            for (int l = 0; l < 64; ++l) mx = max(mx, len_p[(int64_t)sidx * 64 + l]);
            w = (long long)mx * 64;
        }
        const long long incl = block_scan_carry<1024>(w, buf, &carry);
        if (sidx < n_slices) slice_ptr[sidx + 1] = incl;
    }
}
// pattern of the view -> colour-sorted storage (thread per original row), diagonal offsets on the way, and the values too
// unless val_p is null (a cached layout: every solve brings its own values, gs_permute_values_k)
__global__ void gs_permute_all_k(MatView A, const int *__restrict__ slot_of_row, const int64_t *__restrict__ sp_p, int *__restrict__ col_p,
                                 double *__restrict__ val_p, int *__restrict__ diag_p, int *__restrict__ cslot_p) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.P.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int len = A.P.row_len[i];
        const int64_t src = A.P.slice_ptr[i >> 6] + (i & 63);
        const int64_t slot = slot_of_row[i];
        const int64_t dst = sp_p[slot >> 6] + (slot & 63);
        int d = -1;
        for (int k = 0; k < len; ++k) {
            const int j = A.P.col[src + (int64_t)k * 64];
            col_p[dst + (int64_t)k * 64] = j;
            cslot_p[dst + (int64_t)k * 64] = j < A.P.n ? slot_of_row[j] : -1;  // (ghost columns: the slot-space solver is single-GPU)
            if (val_p) val_p[dst + (int64_t)k * 64] = view_value(A, i, src + (int64_t)k * 64);
            if (j == i) d = (int)(dst + (int64_t)k * 64);
        }
        diag_p[slot] = d;
    }
}
// values of the matrix view -> colour-sorted storage: thread per original row (coalesced reads), the scalings applied
__global__ void gs_permute_values_k(MatView A, const int *__restrict__ slot_of_row, const int64_t *__restrict__ sp_p, double *__restrict__ val_p) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.P.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int len = A.P.row_len[i];
        const int64_t src = A.P.slice_ptr[i >> 6] + (i & 63);
        const int64_t slot = slot_of_row[i];
        const int64_t dst = sp_p[slot >> 6] + (slot & 63);
        for (int k = 0; k < len; ++k) val_p[dst + (int64_t)k * 64] = view_value(A, i, src + (int64_t)k * 64);
    }
}

// an array of the layout: in the buffer the cache owns, or in the solve's arena
template <class T>
static int layout_alloc(Arena &arena, bool cached, DevBuf<T> &own, size_t count, T **out) {
    if (!cached) return arena.alloc(count, out);
    ORC_TRY(own.alloc(count));
    *out = own.p;
    return ORC_OK;
}

int build_sorted_layout(const MatView &A, Coloring &C, Arena &arena, bool cached, const double **val) {
    const int64_t n = A.P.n;
    hipStream_t st = ctx().stream;
    const int nc = C.n_colors;
    C.layout = SortedLayout();
    if (val) *val = nullptr;
    C.color_slice.assign((size_t)nc + 1, 0);
    std::vector<int> first_slot((size_t)std::max(nc, 1), 0);
    for (int c = 0; c < nc; ++c) {  // every colour padded to whole slices
        const int64_t cnt = C.start[(size_t)c + 1] - C.start[(size_t)c];
        first_slot[(size_t)c] = C.color_slice[(size_t)c] * 64;
        C.color_slice[(size_t)c + 1] = C.color_slice[(size_t)c] + (int)((cnt + 63) / 64);
    }
    const int n_slices = C.color_slice[(size_t)nc];
    const int64_t n_slots = (int64_t)n_slices * 64, n_blocks = (n + 63) / 64;
    if (n_slices == 0) return ORC_OK;  // (n == 0: nothing to sweep)
    int *slot_of_row, *rowid, *len_p, *diag_p, *col_p, *cslot_p;
    int64_t *sp_p;
    double *val_p = nullptr;
    ORC_TRY(layout_alloc(arena, cached, C.own.slot_of_row, (size_t)n, &slot_of_row));
    ORC_TRY(layout_alloc(arena, cached, C.own.rowid, (size_t)n_slots, &rowid));
    ORC_TRY(layout_alloc(arena, cached, C.own.row_len, (size_t)n_slots, &len_p));
    ORC_TRY(layout_alloc(arena, cached, C.own.diag_off, (size_t)n_slots, &diag_p));
    ORC_TRY(layout_alloc(arena, cached, C.own.sp, (size_t)n_slices + 1, &sp_p));
    ORC_HIP(hipMemsetAsync(rowid, 0xff, sizeof(int) * (size_t)n_slots, st));
    ORC_HIP(hipMemsetAsync(len_p, 0, sizeof(int) * (size_t)n_slots, st));
    ORC_HIP(hipMemsetAsync(diag_p, 0xff, sizeof(int) * (size_t)n_slots, st));
    int64_t padded = 0;
    {
        ArenaScope scratch(arena);  // the stream is idle when the scope ends
        int *table, *intra, *first_dev;
        ORC_TRY(arena.alloc((size_t)(n_blocks * nc), &table));
        ORC_TRY(arena.alloc((size_t)n, &intra));
        ORC_TRY(arena.alloc((size_t)nc, &first_dev));
        ORC_HIP(hipMemcpyAsync(first_dev, first_slot.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gs_block_counts_k, dim3((unsigned)std::min<int64_t>(n_blocks, 8192)), dim3(64), 0, st, C.color, n, nc, table, intra);
        hipLaunchKernelGGL(gs_column_scan_k, dim3(nc), dim3(1024), 0, st, table, n_blocks, nc);
        hipLaunchKernelGGL(gs_assign_slots_k, dim3(grid_for(n)), dim3(kBlock), 0, st, A.P, C.color, table, intra, nc, first_dev, slot_of_row, rowid, len_p);
        hipLaunchKernelGGL(gs_slice_ptr_k, dim3(1), dim3(1024), 0, st, len_p, n_slices, sp_p);
        ORC_HIP(hipGetLastError());
        ORC_HIP(hipMemcpyAsync(&padded, sp_p + n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
    }
    if (padded >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "colour-sorted matrix too large for 32-bit offsets");
    const size_t np = (size_t)std::max<int64_t>(padded, 1);
    ORC_TRY(layout_alloc(arena, cached, C.own.col, np, &col_p));
    ORC_TRY(layout_alloc(arena, cached, C.own.cslot, np, &cslot_p));
    if (val) ORC_TRY(arena.alloc(np, &val_p));
    hipLaunchKernelGGL(gs_permute_all_k, dim3(grid_for(n)), dim3(kBlock), 0, st, A, slot_of_row, sp_p, col_p, val_p, diag_p, cslot_p);
    ORC_HIP(hipGetLastError());
    if (cached) ORC_HIP(hipStreamSynchronize(st));  // other threads (the momentum lanes, on their own streams) read a cached layout
    SortedLayout &L = C.layout;
    L.sp = sp_p; L.row_len = len_p; L.rowid = rowid; L.diag_off = diag_p; L.col = col_p; L.cslot = cslot_p; L.slot_of_row = slot_of_row;
    L.n_slices = n_slices; L.n_slots = n_slots; L.padded = padded;
    if (val) *val = val_p;
    return ORC_OK;
}

int sorted_values(const MatView &A, const SortedLayout &L, Arena &arena, const double **val) {
    double *v;
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(L.padded, 1), &v));
    hipLaunchKernelGGL(gs_permute_values_k, dim3(grid_for(A.P.n)), dim3(kBlock), 0, ctx().stream, A, L.slot_of_row, L.sp, v);
    ORC_HIP(hipGetLastError());
    *val = v;
    return ORC_OK;
}

}  // namespace orc
