// amg_mirror.hip — what the products of a built coarse level stream besides its SELL image (formats: linalg.hpp).
//   xwin_build_k    the LDS x windows of a packed mirror (XWinDev): per block of 256 rows the distinct columns (32 bits each, or 16-bit offsets from
//                   a base per 64), per entry a 12- or 16-bit position
//   xwin_cap_k      how many blocks exceed each candidate LDS share (XWinDev::cap);  xwin_stats_k: ORC_DEBUG_XWIN's figures
//   narrow_build_k  2-byte column offsets for a level without a mirror (SellDev::col16 / colbase)
// and the two phases of galerkin() (amg_galerkin.hip) that launch them: narrow_image(), build_windows().  g_xwin_counters is touched by
// this file's kernels only.
#include <algorithm>
#include <mutex>
#include <vector>

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
// [r08] fmt: the formats this launch writes (XWinDev, ORC_XWIN_COMPACT).  kXFmtPos12: 12-bit positions, 12 bytes per granule at 1.5 lptr — the host's
// guess, as the level's LDS share is chosen from the windows this kernel builds; where the share then exceeds 4 096 (more than 1 % of the blocks
// above 4 000 entries: none of the channel's levels) the host launches the kernel once more with kXFmtRedo, which rebuilds the bitmap of every
// block that has a window and writes 16-bit positions only — nothing else is touched or counted.  kXFmtCol16: a block whose list has no segment
// of 64 entries spanning 65 536 columns or more stores bases and 16-bit offsets (wfmt[b] = 1; wfmt is cleared by the host).
constexpr int kXFmtPos12 = 1, kXFmtCol16 = 2, kXFmtRedo = 4;
constexpr int kXWinSegs = (kXWinCap + kXWinSeg - 1) / kXWinSeg;
template <int kWords, bool kSecond>
__global__ __launch_bounds__(kBlock) void xwin_build_k(SellDev P, const int64_t *__restrict__ lptr, int *__restrict__ wcol, int *__restrict__ wsize, int *__restrict__ wfmt,
                                                       unsigned short *__restrict__ lidx, int64_t n_blocks, int win_cap, int bit_words, int pass_words,
                                                       int *__restrict__ pending /* blocks the first pass left to the second */, int fmt) {
    if (kSecond && *pending == 0) return;
    __shared__ unsigned bits[kWords];
    __shared__ unsigned short wpre[kWords];  // exclusive prefix of the word population counts (windows hold <= kXWinCap)
    __shared__ int s_min, s_max, s_part[kBlock];
    __shared__ int s_segbase[kXWinSegs], s_wide;  // kXFmtCol16: the column of list entry 64 s; does an entry lie 65 536 or more above its base?
    const bool redo = (fmt & kXFmtRedo) != 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long n_built = 0, n_capped = 0, n_spanned = 0;  // thread 0's tallies: ONE atomic per counter and workgroup at the end
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        if (kSecond && wsize[b] != -2) continue;  // workgroup-uniform: done by the first pass
        if (redo && wsize[b] <= 0) continue;      // (workgroup-uniform) no window, no positions
        const int64_t row = b * kXWinRows + tid;
        const bool live = row < P.n;
        const int len = live ? P.row_len[row] : 0;
        const int64_t rbase = live ? P.slice_ptr[row >> 6] + (row & 63) : 0;
        if (tid == 0) { s_min = 0x7fffffff; s_max = -1; s_wide = 0; }
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
        if (!kSecond && !redo && words <= bit_words && words > pass_words) {  // the full bitmap's business (pass_words <= kWords: ORC_XWIN_SMALL_BITWORDS, a test hook)
            if (tid == 0) { wsize[b] = -2; atomicAdd(pending, 1); }
            __syncthreads();
            continue;
        }
        if (!redo) ++n_built;
        if (words > bit_words || words > kWords) {  // (never with kXFmtRedo: the block has a window)
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
        if (total > win_cap) {  // (never with kXFmtRedo)
            __syncthreads();
            if (tid == 0) wsize[b] = -1;
            ++n_capped;
            __syncthreads();
            continue;
        }
        int run = s_part[tid] - local;  // exclusive
        int *wc = wcol + b * kXWinCap;
        bool col16 = false;
        if ((fmt & kXFmtCol16) && !redo) {
            // two walks over the thread's words before the one that writes: the bases of the segments, then every entry against its base
            int r = run;
            for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) {
                unsigned m = bits[w];
                while (m) {
                    if ((r & (kXWinSeg - 1)) == 0) s_segbase[r / kXWinSeg] = cmin + (w << 5) + (__ffs(m) - 1);
                    ++r;
                    m &= m - 1;
                }
            }
            __syncthreads();
            bool wide = false;
            r = run;
            for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) {
                unsigned m = bits[w];
                while (m) {
                    wide |= cmin + (w << 5) + (__ffs(m) - 1) - s_segbase[r / kXWinSeg] > 65535;
                    ++r;
                    m &= m - 1;
                }
            }
            if (wide) s_wide = 1;
            __syncthreads();
            col16 = s_wide == 0;
        }
        if (col16) {
            const int nseg = (total + kXWinSeg - 1) / kXWinSeg;
            unsigned short *w16 = reinterpret_cast<unsigned short *>(wc + nseg);
            for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) {
                wpre[w] = (unsigned short)run;
                unsigned m = bits[w];
                while (m) {
                    const int bit = __ffs(m) - 1;
                    w16[run] = (unsigned short)(cmin + (w << 5) + bit - s_segbase[run / kXWinSeg]);
                    ++run;
                    m &= m - 1;
                }
            }
            for (int sg = tid; sg < nseg; sg += kBlock) wc[sg] = s_segbase[sg];
        } else {
            for (int w = tid * per; w < words && w < (tid + 1) * per; ++w) {
                wpre[w] = (unsigned short)run;
                unsigned m = bits[w];
                while (m) {
                    const int bit = __ffs(m) - 1;
                    if (!redo) wc[run] = cmin + (w << 5) + bit;
                    ++run;
                    m &= m - 1;
                }
            }
        }
        if (tid == 0 && !redo) { wsize[b] = total; wfmt[b] = col16 ? 1 : 0; }
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
                    unsigned pos[kPackChunk];
#pragma unroll
                    for (int u = 0; u < kPackChunk; ++u) {
                        pos[u] = 0u;
                        if (j0 + u < len) {
                            const int c = P.col[sbase + (int64_t)(j0 + u) * 64 + lane] - cmin;
                            pos[u] = wpre[c >> 5] + __popc(bits[c >> 5] & ((1u << (c & 31)) - 1u));
                        }
                    }
                    if (fmt & kXFmtPos12) {  // position u in bits [12 u, 12 u + 12) of three words (a window above 4 096 entries: modulo, never read)
#pragma unroll
                        for (int u = 0; u < kPackChunk; ++u) pos[u] &= 0xfffu;
                        const u32x3_t w = {pos[0] | pos[1] << 12 | pos[2] << 24, pos[2] >> 8 | pos[3] << 4 | pos[4] << 16 | pos[5] << 28, pos[5] >> 4 | pos[6] << 8 | pos[7] << 20};
                        *reinterpret_cast<u32x3_a4_t *>(reinterpret_cast<unsigned *>(lidx) + ((off >> 3) + rank) * 3) = w;
                    } else {
                        const u32x4_t w = {pos[0] | pos[1] << 16, pos[2] | pos[3] << 16, pos[4] | pos[5] << 16, pos[6] | pos[7] << 16};
                        *reinterpret_cast<u32x4_t *>(lidx + off + (int64_t)kPackChunk * rank) = w;
                    }
                }
                off += (int64_t)kPackChunk * __popcll(m);
            }
        }
        __syncthreads();
    }
    if (tid == 0 && !redo) {
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
// more, blocks whose columns span fewer than 65 536, blocks without a window; [r08] blocks whose every segment of 64 list entries spans fewer than
// 65 536 (what the 16-bit column format asks of a block, counted whichever format the block has) and the window entries in those blocks
struct XWinList {  // a block's column list in either format (XWinDev::wfmt)
    const int *wc;
    int fmt, nseg;
    __device__ int operator[](int j) const { return fmt ? wc[j / kXWinSeg] + (int)reinterpret_cast<const unsigned short *>(wc + nseg)[j] : wc[j]; }
};
__global__ __launch_bounds__(kBlock) void xwin_stats_k(const int *__restrict__ wcol, const int *__restrict__ wsize, const int *__restrict__ wfmt, int64_t n_blocks,
                                                       unsigned long long *__restrict__ out) {
    __shared__ int s_wide;
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int ws = wsize[b];
        if (ws <= 0) { if (threadIdx.x == 0 && ws < 0) atomicAdd(out + 4, 1ull); continue; }
        const XWinList wc{wcol + b * kXWinCap, wfmt[b], (ws + kXWinSeg - 1) / kXWinSeg};
        if (threadIdx.x == 0) s_wide = 0;
        __syncthreads();
        unsigned long long runs = 0, long_entries = 0;
        bool wide = false;
        for (int j = threadIdx.x; j < ws; j += kBlock) {
            if (j == 0 || wc[j] != wc[j - 1] + 1) {
                ++runs;
                int e = j + 1;
                while (e < ws && wc[e] == wc[e - 1] + 1) ++e;
                if (e - j >= 8) long_entries += (unsigned long long)(e - j);
            }
            wide |= wc[j] - wc[j & ~(kXWinSeg - 1)] > 65535;
        }
        if (wide) s_wide = 1;
        atomicAdd(out + 1, runs);
        atomicAdd(out + 2, long_entries);
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd(out + 0, (unsigned long long)ws);
            if (wc[ws - 1] - wc[0] < 65536) atomicAdd(out + 3, 1ull);
            if (!s_wide) { atomicAdd(out + 5, 1ull); atomicAdd(out + 6, (unsigned long long)ws); }
        }
        __syncthreads();  // s_wide is cleared for the next block
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

// [r08] build_windows' expectation of a level's position format: the row counts of the levels whose last build took an LDS share above
// kXWinPos12Max.  A hint shared by the set-up threads of a process; a handful of entries (one per level and mesh in use).
static std::mutex g_large_share_mu;
static std::vector<int64_t> g_large_share_rows;
static bool large_share_expected(int64_t nc) {
    std::lock_guard<std::mutex> lk(g_large_share_mu);
    return std::find(g_large_share_rows.begin(), g_large_share_rows.end(), nc) != g_large_share_rows.end();
}
static void expect_large_share(int64_t nc, bool large) {
    std::lock_guard<std::mutex> lk(g_large_share_mu);
    const auto it = std::find(g_large_share_rows.begin(), g_large_share_rows.end(), nc);
    if (large && it == g_large_share_rows.end()) {
        if (g_large_share_rows.size() >= 64) g_large_share_rows.erase(g_large_share_rows.begin());
        g_large_share_rows.push_back(nc);
    } else if (!large && it != g_large_share_rows.end()) {
        g_large_share_rows.erase(it);
    }
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
    int *wcol, *wsize, *wfmt;
    unsigned short *lidx;
    ORC_TRY(arena.alloc((size_t)n_blocks * kXWinCap, &wcol));
    ORC_TRY(arena.alloc((size_t)n_blocks, &wsize));
    ORC_TRY(arena.alloc((size_t)n_blocks, &wfmt));
    ORC_HIP(hipMemsetAsync(wfmt, 0, sizeof(int) * (size_t)n_blocks, st));
    const int win_cap = cfg().xwin_cap > 0 ? std::min(kXWinCap, cfg().xwin_cap) : kXWinCap;  // (test hooks: forced fallbacks)
    const int bit_words = cfg().xwin_bitwords > 0 ? std::min(kXBitWords, cfg().xwin_bitwords) : kXBitWords;
    const int small_words = cfg().xwin_small_bitwords > 0 ? std::min(kXBitWordsSmall, cfg().xwin_small_bitwords) : kXBitWordsSmall;
    int *pending, *over;
    ORC_TRY(tmp.alloc((size_t)1, &pending));
    ORC_TRY(tmp.alloc((size_t)kXWinCapSizes, &over));
    ORC_HIP(hipMemsetAsync(pending, 0, sizeof(int), st));
    // [r08] The positions' format follows the level's LDS share (12 bits up to 4 096 entries), and the share is chosen from the windows the build
    // kernel is about to make: the kernel writes the format the host EXPECTS, and where the share then says otherwise a second launch rewrites
    // the positions alone (kXFmtRedo) into a stream of the right size that takes the first one's place (the position stream is the last thing
    // on the arena until the share is known; `tmp` may be the same arena).  Expected: 12 bits — every share but the compiled worst case
    // qualifies, and that one is taken only when more than 1 % of the blocks hold over 4 000 entries — unless the last level of this many rows
    // ended up with the large share (the channel's level 3 does in most of its hierarchies: a solver builds the hierarchy of the same system
    // iteration after iteration).  The expectation decides what the set-up costs, never what it produces.
    const bool compact = cfg().xwin_compact;
    const bool share_known = win_cap <= kXWinPos12Max || !cfg().xwin_level_cap;  // the share is win_cap, or every candidate is small
    const bool pos12_first = compact && (share_known ? win_cap <= kXWinPos12Max : !large_share_expected(nc));
    const int fmt = (pos12_first ? kXFmtPos12 : 0) | (compact ? kXFmtCol16 : 0);
    const size_t pos_units = (size_t)std::max<int64_t>(pos_slots, 1);  // 2 bytes each; 12-bit positions take three quarters (pos_slots is a multiple of 64)
    const Arena::Mark before_positions = arena.mark();
    ORC_TRY(arena.alloc(pos12_first ? pos_units / 4 * 3 + 2 : pos_units, &lidx));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(xwin_build_k<kXBitWordsSmall, false>), dim3((unsigned)std::min<int64_t>(n_blocks, 2048)), dim3(kBlock), 0, st, Pc, lptr, wcol, wsize, wfmt, lidx,
                       n_blocks, win_cap, bit_words, small_words, pending, fmt);
    if (bit_words > small_words)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(xwin_build_k<kXBitWords, true>), dim3((unsigned)std::min<int64_t>(n_blocks, 2048)), dim3(kBlock), 0, st, Pc, lptr, wcol, wsize, wfmt, lidx,
                           n_blocks, win_cap, bit_words, kXBitWords, pending, fmt);
    if (trace) {
        int hp = 0;
        ORC_HIP(hipMemcpyAsync(&hp, pending, sizeof(int), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        fprintf(stderr, "[amg windows n=%lld] %lld blocks, %d left to the full bitmap\n", (long long)nc, (long long)n_blocks, hp);
    }
    ORC_HIP(hipGetLastError());
    L.xw.wcol = wcol; L.xw.wsize = wsize; L.xw.wfmt = wfmt; L.xw.lidx = lidx; L.xw.lptr = lptr;
    // this level's LDS share per workgroup: the smallest of a few sizes that leaves <= 1 % of the blocks without a window
    // (+ whatever had none to begin with); one small kernel and one host read per level with windows
    ORC_HIP(hipMemsetAsync(over, 0, kXWinCapSizes * sizeof(int), st));
    hipLaunchKernelGGL(xwin_cap_k, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_blocks + kBlock - 1) / kBlock, 64))), dim3(kBlock), 0, st, (const int *)wsize, n_blocks, over);
    int h_over[kXWinCapSizes];
    ORC_HIP(hipMemcpyAsync(h_over, over, sizeof(h_over), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    int cap = win_cap;
    for (int q = 0; q < kXWinCapSizes && cfg().xwin_level_cap; ++q)
        if (kXWinCapSize[q] <= win_cap && (int64_t)h_over[q] * 100 <= n_blocks) { cap = kXWinCapSize[q]; break; }
    L.xw.cap = cap;
    L.xw.pos12 = compact && cap <= kXWinPos12Max ? 1 : 0;
    if (compact && !share_known) expect_large_share(nc, !L.xw.pos12);
    if ((L.xw.pos12 != 0) != pos12_first) {  // not what was expected (the first launch is over: the host has read its sizes)
        arena.release(before_positions);
        ORC_TRY(arena.alloc(L.xw.pos12 ? pos_units / 4 * 3 + 2 : pos_units, &lidx));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(xwin_build_k<kXBitWords, false>), dim3((unsigned)std::min<int64_t>(n_blocks, 2048)), dim3(kBlock), 0, st, Pc, lptr, wcol, wsize, wfmt, lidx,
                           n_blocks, win_cap, bit_words, kXBitWords, pending, kXFmtRedo | (L.xw.pos12 ? kXFmtPos12 : 0));
        ORC_HIP(hipGetLastError());
        L.xw.lidx = lidx;
        if (trace) fprintf(stderr, "[amg windows n=%lld] LDS share %d entries: positions rewritten in %d bits\n", (long long)nc, cap, L.xw.pos12 ? 12 : 16);
    }
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
        unsigned long long *d_st, h_st[7];
        ORC_TRY(tmp.alloc((size_t)7, &d_st));
        ORC_HIP(hipMemsetAsync(d_st, 0, sizeof(h_st), st));
        hipLaunchKernelGGL(xwin_stats_k, dim3((unsigned)std::min<int64_t>(n_blocks, 4096)), dim3(kBlock), 0, st, (const int *)wcol, (const int *)wsize, (const int *)wfmt, n_blocks, d_st);
        ORC_HIP(hipMemcpyAsync(h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        fprintf(stderr, "[orc xwin] rows %lld nnz %lld blocks %lld: window entries %llu (%.1f per row), runs %llu (%.1f entries per run), in runs >= 8: %.1f %%, span < 65536: %llu blocks, no window: %llu; every 64-entry segment < 65536: %llu blocks with %llu window entries (%.2f %%); positions %d bits\n",
                (long long)nc, (long long)L.pk.total, (long long)n_blocks, h_st[0], (double)h_st[0] / (double)nc, h_st[1], (double)h_st[0] / (double)std::max<unsigned long long>(h_st[1], 1),
                100. * (double)h_st[2] / (double)std::max<unsigned long long>(h_st[0], 1), h_st[3], h_st[4], h_st[5], h_st[6],
                100. * (double)h_st[6] / (double)std::max<unsigned long long>(h_st[0], 1), L.xw.pos12 ? 12 : 16);
    }
    return ORC_OK;
}

}  // namespace orc
