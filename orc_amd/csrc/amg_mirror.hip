// amg_mirror.hip — what the products of a built coarse level stream besides its SELL image (formats: linalg.hpp).
//   xwin_build_k    the LDS x windows of a packed mirror (XWinDev): per block of 256 rows the distinct columns, per entry a 16-bit position
//   xwin_cap_k      how many blocks exceed each candidate LDS share (XWinDev::cap);  xwin_stats_k: ORC_DEBUG_XWIN's figures
//   narrow_build_k  2-byte column offsets for a level without a mirror (SellDev::col16 / colbase)
// and the two phases of galerkin() (amg_galerkin.hip) that launch them: narrow_image(), build_windows().  g_xwin_counters is touched by
// this file's kernels only.
#include <algorithm>

#include "amg.hpp"

namespace orc {

// ---- LDS x windows of the packed mirror (XWinDev, linalg.hpp): per block of 256 rows the ascending list of distinct
// columns and, per packed entry, the 16-bit position of its column in that list.  One workgroup per block: the columns
// set bits in an LDS bitmap over the block's column span, a prefix of the word population counts turns a bit into its
// rank.  A block whose span exceeds the bitmap or whose window exceeds kXWinCap gets wsize = -1 (global gathers).
constexpr int kXBitWords = 8192;  // 262144 columns of span
// [r04] The two limits are run-time arguments bounded by the compiled LDS sizes (win_cap <= kXWinCap, bit_words <= kXBitWords;
// ORC_XWIN_CAP / ORC_XWIN_BITWORDS, read per set-up): at bench size 1 % of level 3's blocks take the no-window path of the
// product and none the span branch, on test-sized meshes none at all — the tests shrink the limits to drive a chosen share of
// the blocks through both branches and compare with the oracle (tests/test_gpu_window_fallback.py).  g_xwin_counters: blocks
// built / without a window because of the cap / because of the span, since the last reset (orc_debug_xwin_counters).
__device__ unsigned long long g_xwin_counters[3];
// [r04] Two passes: the first with a bitmap of kXBitWordsSmall words (25 KB of LDS: six workgroups per CU instead of three) takes every block whose
// columns span at most 131 072 and marks the others pending (wsize = -2); the second, with the full bitmap, runs only if any block is pending and
// looks at those only.  (ORC_AMG_TRACE "[amg windows]": with 2 048 words half of the channel's level-2 / 3 blocks were left to the second pass.)
constexpr int kXBitWordsSmall = 4096;
template <int kWords, bool kSecond>
__global__ __launch_bounds__(kBlock) void xwin_build_k(SellDev P, const int64_t *__restrict__ lptr, int *__restrict__ wcol, int *__restrict__ wsize,
                                                       unsigned short *__restrict__ lidx, int64_t n_blocks, int win_cap, int bit_words, int pass_words,
                                                       int *__restrict__ pending /* blocks the first pass left to the second */) {
    if (kSecond && *pending == 0) return;
    __shared__ unsigned bits[kWords];
    __shared__ unsigned short wpre[kWords];  // exclusive prefix of the word population counts (windows hold <= 4096)
    __shared__ int s_min, s_max, s_part[kBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long n_built = 0, n_capped = 0, n_spanned = 0;  // thread 0's tallies: ONE atomic per counter and workgroup at the end
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        if (kSecond && wsize[b] != -2) continue;  // workgroup-uniform: done by the first pass
        const int64_t row = b * kXWinRows + tid;
        const bool live = row < P.n;
        const int len = live ? P.row_len[row] : 0;
        const int64_t rbase = live ? P.slice_ptr[row >> 6] + (row & 63) : 0;
        if (tid == 0) { s_min = 0x7fffffff; s_max = -1; }
        __syncthreads();
        if (len > 0) {  // columns ascend within a row
            atomicMin(&s_min, P.col[rbase]);
            atomicMax(&s_max, P.col[rbase + (int64_t)(len - 1) * 64]);
        }
        __syncthreads();
        const int cmin = s_min, span = s_max - s_min + 1;
        const int words = (span + 31) >> 5;
        if (s_max < 0) {  // empty block
            if (tid == 0) wsize[b] = 0;
            __syncthreads();
            continue;
        }
        if (!kSecond && words <= bit_words && words > pass_words) {  // the full bitmap's business (pass_words <= kWords: ORC_XWIN_SMALL_BITWORDS, a test hook)
            if (tid == 0) { wsize[b] = -2; atomicAdd(pending, 1); }
            __syncthreads();
            continue;
        }
        ++n_built;
        if (words > bit_words || words > kWords) {
            if (tid == 0) wsize[b] = -1;
            ++n_spanned;
            __syncthreads();
            continue;
        }
        for (int w = tid; w < words; w += kBlock) bits[w] = 0u;
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const int c = P.col[rbase + (int64_t)k * 64] - cmin;
            atomicOr(&bits[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
        // prefix over the words: thread t owns words [t * per, (t + 1) * per)
        const int per = (words + kBlock - 1) / kBlock;
        int local = 0;
        for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) local += __popc(bits[w]);
        s_part[tid] = local;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {  // Hillis-Steele inclusive scan of the 256 partial sums
            const int t = tid >= off ? s_part[tid - off] : 0;
            __syncthreads();
            s_part[tid] += t;
            __syncthreads();
        }
        const int total = s_part[kBlock - 1];
        if (total > win_cap) {
            __syncthreads();
            if (tid == 0) wsize[b] = -1;
            ++n_capped;
            __syncthreads();
            continue;
        }
        int run = s_part[tid] - local;  // exclusive
        int *wc = wcol + b * kXWinCap;
        for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) {
            wpre[w] = (unsigned short)run;
            unsigned m = bits[w];
            while (m) {
                const int bit = __ffs(m) - 1;
                wc[run++] = cmin + (w << 5) + bit;
                m &= m - 1;
            }
        }
        if (tid == 0) wsize[b] = total;
        __syncthreads();
        // window positions of the packed entries: wave per slice, chunk by chunk (XWinDev::lidx): 8 positions per lane whose row reaches the
        // chunk, one 16-byte store; the positions past the row's end are 0
        const int64_t slice = b * 4 + wave;
        if (slice < P.n_slices) {
            const int64_t sbase = P.slice_ptr[slice];
            const int width = (int)((P.slice_ptr[slice + 1] - sbase) >> 6);
            int64_t off = lptr[slice];
            for (int j0 = 0; j0 < width; j0 += kPackChunk) {
                const bool in = j0 < len;
                const unsigned long long m = __ballot(in);
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (in) {
                    u32x4_t w = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int u = 0; u < kPackChunk; ++u) {
                        if (j0 + u < len) {
                            const int c = P.col[sbase + (int64_t)(j0 + u) * 64 + lane] - cmin;
                            const unsigned pos = wpre[c >> 5] + __popc(bits[c >> 5] & ((1u << (c & 31)) - 1u));
                            w[u >> 1] |= pos << (16 * (u & 1));
                        }
                    }
                    *reinterpret_cast<u32x4_t *>(lidx + off + (int64_t)kPackChunk * rank) = w;
                }
                off += (int64_t)kPackChunk * __popcll(m);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (n_built) atomicAdd(&g_xwin_counters[0], n_built);
        if (n_capped) atomicAdd(&g_xwin_counters[1], n_capped);
        if (n_spanned) atomicAdd(&g_xwin_counters[2], n_spanned);
    }
}

// candidates for a level's LDS share (XWinDev::cap), ascending; over[q] = blocks whose window holds more than kXWinCapSize[q] entries
constexpr int kXWinCapSizes = 5;
__device__ __constant__ int kXWinCapSizeDev[kXWinCapSizes] = {2048, 2560, 3200, 4000, kXWinCap};
static const int kXWinCapSize[kXWinCapSizes] = {2048, 2560, 3200, 4000, kXWinCap};
__global__ __launch_bounds__(kBlock) void xwin_cap_k(const int *__restrict__ wsize, int64_t n_blocks, int *__restrict__ over) {
    int c[kXWinCapSizes] = {0, 0, 0, 0, 0};
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * blockDim.x) {
        const int ws = wsize[b];
#pragma unroll
        for (int q = 0; q < kXWinCapSizes; ++q) c[q] += ws > kXWinCapSizeDev[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < kXWinCapSizes; ++q)
        if (c[q]) atomicAdd(over + q, c[q]);
}

// ORC_DEBUG_XWIN / ORC_XWIN_STATS (measurement): how the windows of a level are made up — entries, maximal runs of consecutive columns, runs of eight or
// more, blocks whose columns span fewer than 65 536, blocks without a window
__global__ __launch_bounds__(kBlock) void xwin_stats_k(const int *__restrict__ wcol, const int *__restrict__ wsize, int64_t n_blocks, unsigned long long *__restrict__ out) {
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int ws = wsize[b];
        if (ws <= 0) { if (threadIdx.x == 0 && ws < 0) atomicAdd(out + 4, 1ull); continue; }
        const int *wc = wcol + b * kXWinCap;
        unsigned long long runs = 0, long_entries = 0;
        for (int j = threadIdx.x; j < ws; j += kBlock) {
            if (j == 0 || wc[j] != wc[j - 1] + 1) {
                ++runs;
                int e = j + 1;
                while (e < ws && wc[e] == wc[e - 1] + 1) ++e;
                if (e - j >= 8) long_entries += (unsigned long long)(e - j);
            }
        }
        atomicAdd(out + 1, runs);
        atomicAdd(out + 2, long_entries);
        if (threadIdx.x == 0) {
            atomicAdd(out + 0, (unsigned long long)ws);
            if (wc[ws - 1] - wc[0] < 65536) atomicAdd(out + 3, 1ull);
        }
    }
}

// ---- narrow column image of a coarse operator (SellDev::col16 / colbase, linalg.hpp): one wavefront per slice; per depth the
// smallest column among the rows that reach it and 16-bit offsets from it; *too_wide is raised if a depth spans 65 536 or more
__global__ __launch_bounds__(64) void narrow_build_k(SellDev P, unsigned short *__restrict__ col16, int *__restrict__ colbase, int *__restrict__ too_wide) {
    const int lane = threadIdx.x;
    for (int64_t slice = blockIdx.x; slice < P.n_slices; slice += gridDim.x) {
        const int64_t row = slice * 64 + lane;
        const int64_t sb = P.slice_ptr[slice];
        const int width = (int)((P.slice_ptr[slice + 1] - sb) >> 6);
        const int len = row < P.n ? P.row_len[row] : 0;
        for (int k = 0; k < width; ++k) {
            const bool in = k < len;
            const int c = in ? P.col[sb + (int64_t)k * 64 + lane] : 0;
            int lo = in ? c : 0x7fffffff, hi = in ? c : -1;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lo = min(lo, __shfl_xor(lo, off, 64));
                hi = max(hi, __shfl_xor(hi, off, 64));
            }
            if (hi < 0) lo = 0;  // nobody reaches this depth
            if (lane == 0) {
                colbase[(sb >> 6) + k] = lo;
                if (hi >= 0 && hi - lo > 65535) atomicOr(too_wide, 1);
            }
            col16[sb + (int64_t)k * 64 + lane] = in ? (unsigned short)(c - lo) : (unsigned short)0;
        }
    }
}

int debug_xwin_counters(long long out[3], bool reset) {
    unsigned long long h[3] = {0, 0, 0};
    ORC_HIP(hipDeviceSynchronize());
    ORC_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_xwin_counters), sizeof(h)));
    for (int i = 0; i < 3; ++i) out[i] = (long long)h[i];
    if (reset) {
        const unsigned long long z[3] = {0, 0, 0};
        ORC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_xwin_counters), z, sizeof(z)));
    }
    return ORC_OK;
}

// ------------------------------------------------------------------ the two phases of galerkin() that build these
int narrow_image(SellDev &Pc, Arena &arena, Arena &tmp) {
    const int64_t padded = Pc.padded;
    if (!cfg().spmv_narrow_cols || padded <= 0) return ORC_OK;
    hipStream_t st = ctx().stream;
    unsigned short *c16;
    int *cbase, *wide;
    ORC_TRY(arena.alloc((size_t)padded, &c16));
    ORC_TRY(arena.alloc((size_t)(padded / 64) + 1, &cbase));
    ORC_TRY(tmp.alloc((size_t)1, &wide));
    ORC_HIP(hipMemsetAsync(wide, 0, sizeof(int), st));
    hipLaunchKernelGGL(narrow_build_k, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(Pc.n_slices, 256 * 32))), dim3(64), 0, st, Pc, c16, cbase, wide);
    ORC_HIP(hipGetLastError());
    int h_wide = 1;
    ORC_HIP(hipMemcpyAsync(&h_wide, wide, sizeof(int), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    if (!h_wide) { Pc.col16 = c16; Pc.colbase = cbase; }  // all or nothing, decided on the host (the kernel variant is a template argument)
    return ORC_OK;
}

// sys[0].L (the leader's level, with its packed mirror) gets the windows; every system the same structure and fold scratch of its own
int build_windows(const GalerkinSibling *sys, int n_sys, const int64_t *lptr, int64_t pos_slots, Arena &tmp) {
    AmgHierarchy::Level &L = *sys[0].L;
    Arena &arena = *sys[0].arena;
    const SellDev &Pc = L.P;
    const int64_t nc = Pc.n;
    hipStream_t st = ctx().stream;
    const bool trace = cfg().amg_trace;
    const int64_t n_blocks = ((int64_t)Pc.n_slices + 3) / 4;
    int *wcol, *wsize;
    unsigned short *lidx;
    ORC_TRY(arena.alloc((size_t)n_blocks * kXWinCap, &wcol));
    ORC_TRY(arena.alloc((size_t)n_blocks, &wsize));
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(pos_slots, 1), &lidx));
    const int win_cap = cfg().xwin_cap > 0 ? std::min(kXWinCap, cfg().xwin_cap) : kXWinCap;  // (test hooks: forced fallbacks)
    const int bit_words = cfg().xwin_bitwords > 0 ? std::min(kXBitWords, cfg().xwin_bitwords) : kXBitWords;
    const int small_words = cfg().xwin_small_bitwords > 0 ? std::min(kXBitWordsSmall, cfg().xwin_small_bitwords) : kXBitWordsSmall;
    int *pending;
    ORC_TRY(tmp.alloc((size_t)1, &pending));
    ORC_HIP(hipMemsetAsync(pending, 0, sizeof(int), st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(xwin_build_k<kXBitWordsSmall, false>), dim3((unsigned)std::min<int64_t>(n_blocks, 2048)), dim3(kBlock), 0, st, Pc, lptr, wcol, wsize, lidx,
                       n_blocks, win_cap, bit_words, small_words, pending);
    if (bit_words > small_words)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(xwin_build_k<kXBitWords, true>), dim3((unsigned)std::min<int64_t>(n_blocks, 2048)), dim3(kBlock), 0, st, Pc, lptr, wcol, wsize, lidx,
                           n_blocks, win_cap, bit_words, kXBitWords, pending);
    if (trace) {
        int hp = 0;
        ORC_HIP(hipMemcpyAsync(&hp, pending, sizeof(int), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        fprintf(stderr, "[amg windows n=%lld] %lld blocks, %d left to the full bitmap\n", (long long)nc, (long long)n_blocks, hp);
    }
    ORC_HIP(hipGetLastError());
    L.xw.wcol = wcol; L.xw.wsize = wsize; L.xw.lidx = lidx; L.xw.lptr = lptr;
    // this level's LDS share per workgroup: the smallest of a few sizes that leaves <= 1 % of the blocks without a window
    // (+ whatever had none to begin with); one small kernel and one host read per level with windows
    int *over;
    ORC_TRY(tmp.alloc((size_t)kXWinCapSizes, &over));
    ORC_HIP(hipMemsetAsync(over, 0, kXWinCapSizes * sizeof(int), st));
    hipLaunchKernelGGL(xwin_cap_k, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_blocks + kBlock - 1) / kBlock, 64))), dim3(kBlock), 0, st, (const int *)wsize, n_blocks, over);
    int h_over[kXWinCapSizes];
    ORC_HIP(hipMemcpyAsync(h_over, over, sizeof(h_over), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    int cap = win_cap;
    for (int q = 0; q < kXWinCapSizes && cfg().xwin_level_cap; ++q)
        if (kXWinCapSize[q] <= win_cap && (int64_t)h_over[q] * 100 <= n_blocks) { cap = kXWinCapSize[q]; break; }
    L.xw.cap = cap;
    if (trace) fprintf(stderr, "[amg windows n=%lld] LDS share %d entries per workgroup (%d of %lld blocks have larger windows)\n", (long long)nc, cap,
                       cap < win_cap ? h_over[std::find(kXWinCapSize, kXWinCapSize + kXWinCapSizes, cap) - kXWinCapSize] : 0, (long long)n_blocks);
    // scratch of the in-launch fold of the level's products (spmv_xwin_k): two sums per workgroup of a one-workgroup-per-block launch; one per
    // system, as the systems' products run side by side
    for (int s = 0; s < n_sys; ++s) {
        XWinDev &xw = sys[s].L->xw;
        if (s > 0) xw = L.xw;
        const size_t n_wg = (size_t)((n_blocks + 7) / 8 * 8);
        double *fs;
        unsigned *fc;
        ORC_TRY(sys[s].arena->alloc(2 * n_wg, &fs));
        ORC_TRY(sys[s].arena->alloc((size_t)4, &fc));
        ORC_HIP(hipMemsetAsync(fc, 0, 4 * sizeof(unsigned), st));
        xw.fold_scratch = fs; xw.fold_counter = fc;
    }
    if (cfg().debug_xwin) {
        unsigned long long *d_st, h_st[5];
        ORC_TRY(tmp.alloc((size_t)5, &d_st));
        ORC_HIP(hipMemsetAsync(d_st, 0, sizeof(h_st), st));
        hipLaunchKernelGGL(xwin_stats_k, dim3((unsigned)std::min<int64_t>(n_blocks, 4096)), dim3(kBlock), 0, st, (const int *)wcol, (const int *)wsize, n_blocks, d_st);
        ORC_HIP(hipMemcpyAsync(h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        fprintf(stderr, "[orc xwin] rows %lld nnz %lld blocks %lld: window entries %llu (%.1f per row), runs %llu (%.1f entries per run), in runs >= 8: %.1f %%, span < 65536: %llu blocks, no window: %llu\n",
                (long long)nc, (long long)L.pk.total, (long long)n_blocks, h_st[0], (double)h_st[0] / (double)nc, h_st[1], (double)h_st[0] / (double)std::max<unsigned long long>(h_st[1], 1),
                100. * (double)h_st[2] / (double)std::max<unsigned long long>(h_st[0], 1), h_st[3], h_st[4]);
    }
    return ORC_OK;
}

}  // namespace orc
