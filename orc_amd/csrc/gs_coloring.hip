// gs_coloring.hip — the colouring of a pattern for the multicolour Gauss-Seidel (gs.hpp): speculative first-fit with conflict
// resolution by a deterministic hash priority (64-bit colour mask), on the device; the cache of the persistent patterns'
// colourings and colour-sorted layouts.
#include <map>
#include <mutex>

#include "gs.hpp"

namespace orc {

__device__ __forceinline__ unsigned hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ bool prio_greater(int a, int b) {  // strict total order on rows
    const unsigned ha = hash32((unsigned)a), hb = hash32((unsigned)b);
    return ha > hb || (ha == hb && a > b);
}

__device__ __forceinline__ int64_t row_base_sell(const SellDev &P, int64_t i) { return P.slice_ptr[i >> 6] + (i & 63); }

// Speculative first-fit colouring with conflict resolution (Gebremedhin-Manne), three kernels per round, Jacobi style so
// that the result does not depend on scheduling: every uncoloured row takes the smallest colour none of its neighbours
// holds in the previous round's state (tentative), then a row that shares its tentative colour with a neighbour coloured
// in the same round gives it up if the neighbour has the higher priority.  A handful of rounds whatever the row
// lengths, where one Jones-Plassmann colour per round needs ~160 rounds on the coarse AMG levels (150 neighbours).
// The pattern need not be structurally symmetric: a row j whose column sits in row i's line while i's does not sit in
// j's never sees i, so the row that does see the pair settles it for both.  Where both are new this round the one of
// lower priority loses — i by itself as ever, j through a store to its flag; where i is final already, j loses and
// i's colour enters j's forbidden mask, which the assignment adds to the colours in use (without it j would choose the
// same colour again in every round).  The stores are idempotent and the mask is an OR, so the outcome still does not
// depend on scheduling; on a symmetric pattern they only repeat what j finds by itself, and the colouring is bit for
// bit the one of the two-kernel form that looked at a row's own line alone.
__global__ void spec_assign_k(SellDev P, const int *__restrict__ color_in, const unsigned long long *__restrict__ forbid, int *__restrict__ color_out,
                              int *__restrict__ overflow) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = color_in[i];
        if (ci >= 0) { color_out[i] = ci; continue; }
        const int len = P.row_len[i];
        const int64_t base = row_base_sell(P, i);
        unsigned long long used = forbid[i];
        for (int k = 0; k < len; ++k) {
            const int j = P.col[base + (int64_t)k * 64];
            if (j == i || j >= P.n) continue;
            const int cj = color_in[j];
            if (cj >= 0) used |= 1ull << cj;
        }
        const unsigned long long freec = ~used;
        if (freec == 0ull) { atomicExch(overflow, 1); color_out[i] = -1; continue; }
        color_out[i] = __ffsll((long long)freec) - 1;
    }
}
// color_prev: state before this round (-1 = was uncoloured), color_tent: after the tentative assignment; the verdicts go
// to the flags (zero on entry), so every row sees the same tentative state whatever the scheduling.  Final rows scan
// their lines too: they are the only ones that see a new row which does not store them.
__global__ void spec_resolve_k(SellDev P, const int *__restrict__ color_prev, const int *__restrict__ color_tent, int *__restrict__ lose,
                               unsigned long long *__restrict__ forbid) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = color_tent[i];
        if (ci < 0) continue;  // (overflow: the round ends in an error)
        const bool final_i = color_prev[i] >= 0;
        const int len = P.row_len[i];
        const int64_t base = row_base_sell(P, i);
        bool lost = false;
        for (int k = 0; k < len; ++k) {
            const int j = P.col[base + (int64_t)k * 64];
            if (j == i || j >= P.n) continue;
            if (color_prev[j] >= 0 || color_tent[j] != ci) continue;
            // j is new this round and took i's colour
            if (final_i) { lose[j] = 1; atomicOr(&forbid[j], 1ull << ci); }
            else if (prio_greater(j, (int)i)) lost = true;
            else lose[j] = 1;
        }
        if (lost) lose[i] = 1;
    }
}
// the round's outcome, in place: a new row keeps its tentative colour unless it was flagged; the flags are left zero
__global__ void spec_commit_k(int64_t n, int *__restrict__ color, const int *__restrict__ color_tent, int *__restrict__ lose, int *__restrict__ remaining) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (color[i] >= 0) continue;
        const int ci = color_tent[i];
        if (lose[i] || ci < 0) { lose[i] = 0; atomicAdd(remaining, 1); continue; }
        color[i] = ci;
    }
}

__global__ void color_count_k(const int *__restrict__ color, int64_t n, int *__restrict__ counts) {
    __shared__ int local[64];  // per-workgroup histogram: 64 global atomics per workgroup instead of one per row
    if (threadIdx.x < 64) local[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) atomicAdd(&local[color[i]], 1);
    __syncthreads();
    if (threadIdx.x < 64 && local[threadIdx.x]) atomicAdd(&counts[threadIdx.x], local[threadIdx.x]);
}

int build_coloring(const SellDev &P, Coloring &C, Arena *arena) {
    const int64_t n = P.n;
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    hipStream_t st = ctx().stream;
    DevBuf<int> lose_b, tent_b, flags_b, counts_b;
    DevBuf<unsigned long long> forbid_b;
    int *color, *lose, *tent, *flags, *counts;
    unsigned long long *forbid;
    if (arena) {  // per-solve colouring: no hipMalloc / hipFree inside the SIMPLE loop
        ORC_TRY(arena->alloc(nn, &color));
        ORC_TRY(arena->alloc(nn, &lose));
        ORC_TRY(arena->alloc(nn, &tent));
        ORC_TRY(arena->alloc(nn, &forbid));
        ORC_TRY(arena->alloc((size_t)2, &flags));
        ORC_TRY(arena->alloc((size_t)64, &counts));
    } else {
        ORC_TRY(C.own.color.alloc(nn));
        ORC_TRY(lose_b.alloc(nn));
        ORC_TRY(tent_b.alloc(nn));
        ORC_TRY(forbid_b.alloc(nn));
        ORC_TRY(flags_b.alloc(2));
        ORC_TRY(counts_b.alloc(64));
        color = C.own.color.p; lose = lose_b.p; tent = tent_b.p; forbid = forbid_b.p; flags = flags_b.p; counts = counts_b.p;
    }
    C.color = color;
    ORC_HIP(hipMemsetAsync(color, 0xff, sizeof(int) * (size_t)n, st));
    ORC_HIP(hipMemsetAsync(lose, 0, sizeof(int) * (size_t)n, st));
    ORC_HIP(hipMemsetAsync(forbid, 0, sizeof(unsigned long long) * (size_t)n, st));
    const int g = grid_for(n);
    for (int round = 0; round < 10000; ++round) {
        ORC_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
        hipLaunchKernelGGL(spec_assign_k, dim3(g), dim3(kBlock), 0, st, P, color, forbid, tent, flags + 1);
        hipLaunchKernelGGL(spec_resolve_k, dim3(g), dim3(kBlock), 0, st, P, color, tent, lose, forbid);
        hipLaunchKernelGGL(spec_commit_k, dim3(g), dim3(kBlock), 0, st, n, color, tent, lose, flags);
        ORC_HIP(hipGetLastError());
        int h[2];
        ORC_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        if (h[1]) return set_error(ORC_ERR_BAD_ARGUMENT, "colouring needs more than 64 colours");
        if (h[0] == 0) break;
    }
    ORC_HIP(hipMemsetAsync(counts, 0, 64 * sizeof(int), st));
    hipLaunchKernelGGL(color_count_k, dim3(g), dim3(kBlock), 0, st, color, n, counts);
    int hc[64];
    ORC_HIP(hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    C.n_colors = 0;
    for (int c = 0; c < 64; ++c) if (hc[c] > 0) C.n_colors = c + 1;
    C.start.assign((size_t)C.n_colors + 1, 0);
    for (int c = 0; c < C.n_colors; ++c) C.start[(size_t)c + 1] = C.start[(size_t)c] + hc[c];
    return ORC_OK;
}

// colourings of persistent patterns (the mesh pattern of a solver) are kept, with their layouts; AMG levels are coloured and
// laid out per solve
static std::map<const void *, std::unique_ptr<Coloring>> &color_cache() {
    static std::map<const void *, std::unique_ptr<Coloring>> c;
    return c;
}
void gs_forget_pattern(const void *col_ptr) { color_cache().erase(col_ptr); }

int gs_prepare(const MatView &A, Arena &arena, std::unique_ptr<Coloring> &owned, const Coloring **out, const double **val) {
    if (!A.persistent_pattern) {
        owned = std::make_unique<Coloring>();
        ORC_TRY(build_coloring(A.P, *owned, &arena));
        ORC_TRY(build_sorted_layout(A, *owned, arena, false, val));
        *out = owned.get();
        return ORC_OK;
    }
    {
        static std::mutex cache_mutex;  // the momentum lanes solve on the same (mesh) pattern at the same time
        std::lock_guard<std::mutex> lock(cache_mutex);
        auto &cache = color_cache();
        auto it = cache.find((const void *)A.P.col);
        if (it == cache.end()) {
            auto c = std::make_unique<Coloring>();
            ORC_TRY(build_coloring(A.P, *c, nullptr));
            ORC_TRY(build_sorted_layout(A, *c, arena, true, nullptr));
            it = cache.emplace((const void *)A.P.col, std::move(c)).first;
        }
        *out = it->second.get();
    }
    return sorted_values(A, (*out)->layout, arena, val);
}

// test hook: the colouring of a pattern (host arrays out)
int gs_debug_coloring(const SellDev &P, std::vector<int> &colors, int *n_colors) {
    Coloring C;
    ORC_TRY(build_coloring(P, C, nullptr));
    colors.resize((size_t)P.n);
    ORC_HIP(hipMemcpy(colors.data(), C.color, sizeof(int) * (size_t)P.n, hipMemcpyDeviceToHost));
    *n_colors = C.n_colors;
    return ORC_OK;
}

}  // namespace orc
