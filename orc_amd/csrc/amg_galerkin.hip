// amg_galerkin.hip — the coarse operator a' = (R A) R^T of one level (linear_algebra.rs:84) for up to three systems on one pattern.
//
// The candidates of T = (R A)[I,:] are <= 4 fine rows whose columns ascend, so T is a MERGE (binary searches; equal columns keep the order
// of the fine rows: the reference's order of accumulation); (T R^T)[I,J] runs over the <= 4 fine indices of row J of R; the survivors are
// ranked by counting.  Every sum associates like nalgebra-sparse's spmm_csr, so the operator is bit-identical to the CPU oracle's.
//   galerkin_bound_k       per coarse row the candidate bound, its scratch offset, its LDS tier (list capacity 64 << t)
//   galerkin_merge_k<G, S> G lanes per coarse row, S value sets through one symbolic pass; output to row-contiguous scratch rows
//   slice_sizes_k, scan_*  the slice tables of the SELL image, the packed mirror and the window positions
//   galerkin_pack_fused_k  scratch rows -> SELL-64 image and packed mirror;  rows_compact_k -> exact-size row-contiguous mirror
//   galerkin()             the one entry: bounds -> merge -> pack -> narrow image -> row mirror -> windows (the last but one and the
//                          narrow image live in amg_mirror.hip)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>

#include "amg.hpp"

namespace orc {

// ------------------------------------------------------------------ scan helpers
// exclusive prefix sum of one int per lane across the wavefront
__device__ __forceinline__ int wave_excl_scan(int v, int &total) {
    const int lane = threadIdx.x & 63;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    total = __shfl(x, 63, 64);
    return x - v;
}

// The candidates of T = (R A)[I,:] are <= 4 fine rows whose columns ascend, so T is a MERGE: every candidate finds its
// place by binary searches in the other lists (equal columns keep the order of the fine rows, i ascending, which is the
// reference's order of accumulation).  And (T R^T)[I,J] = sum_j T_j R_Jj is a sum over the <= 4 fine indices of row J
// of R (restriction_row(J), ascending j — again the reference's order): once the distinct J are known each output lane
// looks its <= 4 terms up in T.  The distinct J need no sort either: a fine column j reaches J = j >> 1 (when j has a
// partner) and J' = chooser[j] >> 1 (when it was chosen), and whether an earlier T entry reaches the same coarse column is
// decided by O(1) look-ups (the sibling 2J+1 / the sibling's partner).  The survivors are ranked by counting.
__device__ __forceinline__ int lds_lower_bound(const int *p, int len, int key) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int lds_upper_bound(const int *p, int len, int key) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// exclusive prefix sum of one int per lane across a group of G lanes
template <int G>
__device__ __forceinline__ int group_excl_scan(int v, int &total) {
    const int gl = threadIdx.x & (G - 1);
    int x = v;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) {
        const int y = __shfl_up(x, off, G);
        if (gl >= off) x += y;
    }
    total = __shfl(x, G - 1, G);
    return x - v;
}

// G lanes per coarse row (64 / G rows per wavefront): the passes of a narrow row (<= 32 candidates on the first coarse
// level) fill half a wavefront.
// Step 1 requests the descriptors of all <= 4 fine rows together, then their first G entries together, from the row-contiguous mirror
// where the matrix has one, and the next coarse row's index and pairing travel while the current row is merged: walked one after the
// other they are twelve dependent global round trips per coarse row.
// S systems on ONE fine pattern and ONE pairing (the u, v, w momentum matrices whenever v's and w's fine-level pairings verify as u's:
// SiblingPairing) share everything symbolic — which candidates there are, where each one merges to, which coarse columns come out and in
// which order — so one pass carries S value sets through the same LDS passes (MergeSiblings: the values, scalings and outputs of systems
// 1 .. S-1; system 0 travels in the ordinary arguments).  Per system the products and the order of every sum are those of its own pass:
// bit-identical (tests/test_gpu_triple.py).  The kernel waits for scattered look-ups most of its time; those are now paid once for three.
struct MergeSiblings {
    const double *val[2] = {nullptr, nullptr};    // fine values, addressed like system 0's (SELL image or row-contiguous mirror)
    const double *s1[2] = {nullptr, nullptr}, *s2[2] = {nullptr, nullptr};  // the views' row scalings (null where system 0 has none)
    double *s_val[2] = {nullptr, nullptr};        // scratch rows, same offsets as system 0's
};

template <int G, int S = 1>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(S == 1 ? 6 : 4))) void galerkin_merge_k(MatView A, const int *__restrict__ choice, const int *__restrict__ chooser, int64_t n_coarse,
                                                        int cap /* power of two >= 2 * candidates */, int *__restrict__ row_len_c,
                                                        const long long *__restrict__ slice_base, const int *__restrict__ intra_off, int *__restrict__ s_col,
                                                        double *__restrict__ s_val, const int *__restrict__ list, const int *__restrict__ list_count,
                                                        MergeSiblings X) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int kRows = 64 / G;  // coarse rows in flight per wavefront
    constexpr int kX = S - 1;      // sibling systems
    const int h = cap >> 1;
    const int lane = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    double *src_val = reinterpret_cast<double *>(smem + (size_t)grp * (size_t)cap * (size_t)(12 + 8 * kX));  // candidates in generation order, later T's values
    double *m_val = src_val + h;                          // merged candidates
    int *src_col = reinterpret_cast<int *>(m_val + h);    // ... later T's columns
    int *m_col = src_col + h;
    // [cap] distinct coarse columns, unsorted: written by step 4, when the merged candidates (last read by step 3) are dead — the list lives
    // in their values' place [r04: 12 instead of 16 bytes of LDS per list slot]
    int *U = reinterpret_cast<int *>(m_val);
    double *x_src = reinterpret_cast<double *>(m_col + h);  // siblings: [kX][h] candidates / T values, then [kX][h] merged candidates
    double *x_m = x_src + (size_t)(kX > 0 ? kX : 1) * h;
    const int n_fine = (int)A.P.n;
    const int64_t total_rows = list ? (int64_t)*list_count : n_coarse;
    const int64_t it_step = (int64_t)gridDim.x * kRows;
    // entry k of fine row i: the row-contiguous mirror where the matrix has one (RowWalk)
    const bool mirror = A.rows.col != nullptr;
    const int32_t *colp = mirror ? A.rows.col : A.P.col;
    const double *valp = mirror ? A.rows.val : A.val;
    const int64_t stride = mirror ? 1 : 64;
    // this iteration's row, loaded one iteration ahead
    int64_t it0 = (int64_t)blockIdx.x * kRows;
    bool active = it0 + grp < total_rows;
    int64_t I = active ? (list ? (int64_t)list[it0 + grp] : it0 + grp) : 0;
    int pair0 = (active && 2 * I < n_fine) ? choice[2 * I] : -1;
    int pair1 = (active && 2 * I + 1 < n_fine) ? choice[2 * I + 1] : -1;
    for (; it0 < total_rows; it0 += it_step) {
        // (the barriers below are reached by every group the same number of times)
        const int64_t it_n = it0 + it_step + grp;
        const bool active_n = it_n < total_rows;
        const int64_t I_n = active_n ? (list ? (int64_t)list[it_n] : it_n) : 0;  // in flight during steps 1-3
        RRow R;
        R.n = 0;
        if (active) R = restriction_row_from(I, pair0, pair1);
        // ---- 1. candidates, list after list (ghost columns dropped: coarse levels are per rank)
        int b1 = 0, b2 = 0, b3 = 0, b4 = 0;
        {
            int len[4];
            int64_t rb[4];
            double sc1[4], sc2[4];
            double xs1[kX > 0 ? kX : 1][4], xs2[kX > 0 ? kX : 1][4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {  // descriptors of all fine rows at once
                const bool on = a < R.n;
                const int i = on ? R.idx[a] : 0;
                len[a] = on ? A.P.row_len[i] : 0;
                rb[a] = mirror ? (int64_t)A.rows.slice_base[i >> 6] + A.rows.intra_off[i] : A.P.slice_ptr[i >> 6] + (i & 63);
                sc1[a] = A.s1 ? A.s1[i] : 1.;
                sc2[a] = A.s2 ? A.s2[i] : 1.;
#pragma unroll
                for (int x = 0; x < kX; ++x) {
                    xs1[x][a] = X.s1[x] ? X.s1[x][i] : 1.;
                    xs2[x][a] = X.s2[x] ? X.s2[x][i] : 1.;
                }
            }
            int c0[4];
            double v0[4];
            double xv0[kX > 0 ? kX : 1][4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {  // their first G entries at once
                const bool in = lane < len[a];
                const int64_t pos = rb[a] + (int64_t)(in ? lane : 0) * stride;
                c0[a] = in ? colp[pos] : -1;
                v0[a] = in ? valp[pos] : 0.;
#pragma unroll
                for (int x = 0; x < kX; ++x) xv0[x][a] = in ? X.val[x][pos] : 0.;
            }
            int base = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (a < R.n) {
                    const double w = R.w[a];
                    for (int k0 = 0; k0 < len[a]; k0 += G) {
                        const int k = k0 + lane;
                        int c = -1;
                        double v = 0.;
                        double xv[kX > 0 ? kX : 1];
#pragma unroll
                        for (int x = 0; x < kX; ++x) xv[x] = 0.;
                        if (k0 == 0) {
                            c = c0[a]; v = v0[a];
#pragma unroll
                            for (int x = 0; x < kX; ++x) xv[x] = xv0[x][a];
                        } else if (k < len[a]) {
                            const int64_t pos = rb[a] + (int64_t)k * stride;
                            c = colp[pos]; v = valp[pos];
#pragma unroll
                            for (int x = 0; x < kX; ++x) xv[x] = X.val[x][pos];
                        }
                        const int valid = (c >= 0 && c < n_fine) ? 1 : 0;
                        int tot;
                        const int slot = base + group_excl_scan<G>(valid, tot);
                        if (valid) {
                            if (A.s1) v = sc1[a] * v;  // view_value's order
                            if (A.s2) v = sc2[a] * v;
                            src_col[slot] = c;
                            src_val[slot] = w * v;
#pragma unroll
                            for (int x = 0; x < kX; ++x) {
                                double t = xv[x];
                                if (X.s1[x]) t = xs1[x][a] * t;
                                if (X.s2[x]) t = xs2[x][a] * t;
                                x_src[(size_t)x * h + slot] = w * t;
                            }
                        }
                        base += tot;
                    }
                }
                if (a == 0) b1 = base;
                if (a == 1) b2 = base;
                if (a == 2) b3 = base;
                if (a == 3) b4 = base;
            }
        }
        const int cnt = b4;
        __syncthreads();
        // ---- 2. merge: rank = own position + entries of earlier lists with column <= c + entries of later lists with column < c
        for (int e = lane; e < cnt; e += G) {
            const int a = (e >= b1) + (e >= b2) + (e >= b3);
            const int c = src_col[e];
            const int own_base = a == 0 ? 0 : (a == 1 ? b1 : (a == 2 ? b2 : b3));
            int rank = e - own_base;
            if (a != 0 && b1 > 0) rank += lds_upper_bound(src_col, b1, c);
            if (a != 1 && b2 > b1) rank += a > 1 ? lds_upper_bound(src_col + b1, b2 - b1, c) : lds_lower_bound(src_col + b1, b2 - b1, c);
            if (a != 2 && b3 > b2) rank += a > 2 ? lds_upper_bound(src_col + b2, b3 - b2, c) : lds_lower_bound(src_col + b2, b3 - b2, c);
            if (a != 3 && b4 > b3) rank += lds_lower_bound(src_col + b3, b4 - b3, c);
            m_col[rank] = c;
            m_val[rank] = src_val[e];
#pragma unroll
            for (int x = 0; x < kX; ++x) x_m[(size_t)x * h + rank] = x_src[(size_t)x * h + e];
        }
        __syncthreads();
        // ---- 3. runs of equal j -> T (sorted by j) into src_col / src_val
        int cntT = 0;
        for (int b0 = 0; b0 < cnt; b0 += G) {
            const int e = b0 + lane;
            int head = 0;
            if (e < cnt) head = (e == 0) || (m_col[e] != m_col[e - 1]);
            int tot;
            const int slot = cntT + group_excl_scan<G>(head, tot);
            if (head) {
                const int j = m_col[e];
                double acc = 0. + m_val[e];
                double xacc[kX > 0 ? kX : 1];
#pragma unroll
                for (int x = 0; x < kX; ++x) xacc[x] = 0. + x_m[(size_t)x * h + e];
                for (int q = e + 1; q < cnt && m_col[q] == j; ++q) {
                    acc += m_val[q];
#pragma unroll
                    for (int x = 0; x < kX; ++x) xacc[x] += x_m[(size_t)x * h + q];
                }
                src_col[slot] = j;
                src_val[slot] = acc;
#pragma unroll
                for (int x = 0; x < kX; ++x) x_src[(size_t)x * h + slot] = xacc[x];
            }
            cntT += tot;
        }
        __syncthreads();
        // the next row's pairing (its index has arrived by now): in flight during steps 4-5
        const int pair0_n = (active_n && 2 * I_n < n_fine) ? choice[2 * I_n] : -1;
        const int pair1_n = (active_n && 2 * I_n + 1 < n_fine) ? choice[2 * I_n + 1] : -1;
        const int *tj = src_col;
        const double *tv = src_val;
        // ---- 4. the distinct coarse columns, first occurrence only
        int nU = 0;
        for (int b0 = 0; b0 < cntT; b0 += G) {
            const int e = b0 + lane;
            int k0 = -1, k1 = -1;
            if (e < cntT) {
                const int j = tj[e];
                const int cj = choice[j], mj = chooser[j];
                if (cj >= 0) {  // J = j >> 1; its other fine row 2J comes first when it is here too
                    const bool dup = (j & 1) && e > 0 && tj[e - 1] == j - 1 && choice[j - 1] >= 0;
                    if (!dup) k0 = j >> 1;
                }
                if (mj >= 0) {  // J' = chooser[j] >> 1
                    const int Jp = mj >> 1;
                    bool drop = cj >= 0 && Jp == (j >> 1);
                    if (!drop) {  // reached through its own fine rows 2J', 2J'+1 (with a partner) by some T entry?
                        const int p = lds_lower_bound(tj, cntT, 2 * Jp);
                        const bool has_even = p < cntT && tj[p] == 2 * Jp;
                        if (has_even && choice[2 * Jp] >= 0) drop = true;
                        else {
                            const int q = has_even ? p + 1 : p;
                            if (q < cntT && tj[q] == 2 * Jp + 1 && choice[2 * Jp + 1] >= 0) drop = true;
                        }
                    }
                    if (!drop) {  // the sibling of chooser[j] chose an earlier T entry: that one keeps J'
                        const int sib = mj ^ 1;
                        if (sib < n_fine) {
                            const int js = choice[sib];
                            if (js >= 0 && js < j) {
                                const int p = lds_lower_bound(tj, cntT, js);
                                if (p < cntT && tj[p] == js) drop = true;
                            }
                        }
                    }
                    if (!drop) k1 = Jp;
                }
            }
            int tot;
            int slot = nU + group_excl_scan<G>((k0 >= 0 ? 1 : 0) + (k1 >= 0 ? 1 : 0), tot);
            if (k0 >= 0) U[slot++] = k0;
            if (k1 >= 0) U[slot] = k1;
            nU += tot;
        }
        __syncthreads();
        // ---- 5. every distinct J: position by counting, value from the <= 4 fine indices of row J of R (ascending)
        const long long off = active ? slice_base[I >> 6] + intra_off[I] : 0;
        for (int e = lane; e < nU; e += G) {
            const int u = U[e];
            int rank = 0;
            for (int q = 0; q < nU; ++q) rank += U[q] < u ? 1 : 0;
            const RRow RJ = restriction_row(choice, u, A.P.n);
            double acc = 0.;
            double xacc[kX > 0 ? kX : 1];
#pragma unroll
            for (int x = 0; x < kX; ++x) xacc[x] = 0.;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (a < RJ.n) {
                    const int p = lds_lower_bound(tj, cntT, RJ.idx[a]);
                    if (p < cntT && tj[p] == RJ.idx[a]) {
                        acc += tv[p] * RJ.w[a];
#pragma unroll
                        for (int x = 0; x < kX; ++x) xacc[x] += x_src[(size_t)x * h + p] * RJ.w[a];
                    }
                }
            }
            s_col[off + rank] = u;
            s_val[off + rank] = acc;
#pragma unroll
            for (int x = 0; x < kX; ++x) X.s_val[x][off + rank] = xacc[x];
        }
        if (active && lane == 0) row_len_c[I] = nU;
        __syncthreads();
        active = active_n; I = I_n; pair0 = pair0_n; pair1 = pair1_n;
    }
}

// scratch rows -> SELL-64 (columns, values, diagonal offsets, padding) and, when asked for, the packed mirror, in one
// pass.  The scratch rows are contiguous per ROW, the images are interleaved per SLICE: a thread copying its own row reads
// 64 different cache lines per instruction (the texture path serialises them: 3 ms per image at 5 M rows).  Here one
// wavefront moves one slice through an LDS tile of 16 depths x 64 rows: four rows at a time are read with 16 consecutive
// lanes each (a handful of lines per instruction), the tile is read back depth by depth with lane = row, and both images
// are written with full-width stores.
// kValuesOnly: a sibling system on the same coarse pattern (MergeSiblings) — only val_c / pk_val are written.
constexpr int kPackDepth = 16;
template <bool kValuesOnly = false>
__global__ __launch_bounds__(64) void galerkin_pack_fused_k(SellDev Pc, const long long *__restrict__ slice_base, const int *__restrict__ intra_off,
                                                            const int *__restrict__ s_col, const double *__restrict__ s_val, int *__restrict__ col_c,
                                                            double *__restrict__ val_c, int *__restrict__ diag_c, const int64_t *__restrict__ pk_ptr,
                                                            int *__restrict__ pk_col, double *__restrict__ pk_val) {
    __shared__ int t_col[kPackDepth * 65];
    __shared__ double t_val[kPackDepth * 65];
    const int lane = threadIdx.x;
    const int kk = lane & (kPackDepth - 1), rr = lane / kPackDepth;  // gather phase: depth inside the tile, row inside the group of 4
    for (int64_t slice = blockIdx.x; slice < Pc.n_slices; slice += gridDim.x) {
        const int64_t I = slice * 64 + lane;
        const bool live = I < Pc.n;
        const int len = live ? Pc.row_len[I] : 0;
        const long long src = live ? slice_base[slice] + intra_off[I] : 0;
        const int src_lo = (int)(unsigned)(src & 0xffffffffll), src_hi = (int)(src >> 32);
        const int64_t base = Pc.slice_ptr[slice];
        const int width = (int)((Pc.slice_ptr[slice + 1] - base) >> 6);
        int64_t pk_off = pk_ptr ? pk_ptr[slice] : 0;
        int d = -1;
        for (int kc = 0; kc < width; kc += kPackDepth) {
            // ---- gather: rows 4 rb + rr, depths kc + kk
#pragma unroll 4
            for (int rb = 0; rb < 64 / (64 / kPackDepth); ++rb) {
                const int row = rb * (64 / kPackDepth) + rr;
                const int rlen = __shfl(len, row, 64);
                const long long rsrc = ((long long)__shfl(src_hi, row, 64) << 32) | (long long)(unsigned)__shfl(src_lo, row, 64);
                const int k = kc + kk;
                if (k < rlen) {
                    if (!kValuesOnly) t_col[kk * 65 + row] = s_col[rsrc + k];
                    t_val[kk * 65 + row] = s_val[rsrc + k];
                }
            }
            __syncthreads();
            // ---- scatter: depth by depth, lane = row.  The packed mirror goes by pairs of depths (PackedDev): a lane whose row is longer than
            // the pair's first depth owns both slots, and a row of odd length fills its second one with padding (its own row as column, 0.0) —
            // so the depths run on to the even end of the slice width.
            const int kend = min(kPackDepth, width - kc);
            const int kend_pk = pk_ptr ? min(kPackDepth, ((width + 1) & ~1) - kc) : kend;  // (kc and kPackDepth are even: no pair straddles two tiles)
            int pair_rank = 0;
            int64_t pair_base = 0;
            for (int q = 0; q < kend_pk; ++q) {
                const int k = kc + q;
                const bool in = k < len;
                const int c = (in && !kValuesOnly) ? t_col[q * 65 + lane] : (int)I;
                const double v = in ? t_val[q * 65 + lane] : 0.;
                if (live && q < kend) {
                    const int64_t pos = base + (int64_t)k * 64 + lane;
                    if (!kValuesOnly) col_c[pos] = c;
                    val_c[pos] = v;
                    if (!kValuesOnly && in && c == (int)I) d = (int)pos;
                }
                if (pk_ptr) {
                    if ((k & 1) == 0) {  // wave-uniform
                        const unsigned long long m = __ballot(in);
                        pair_rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        pair_base = pk_off;
                        pk_off += 2 * (int64_t)__popcll(m);
                    }
                    if ((k & ~1) < len) {
                        const int64_t p = pair_base + 2 * pair_rank + (k & 1);
                        if (!kValuesOnly) pk_col[p] = c;
                        pk_val[p] = v;
                    }
                }
            }
            __syncthreads();
        }
        if (live && !kValuesOnly) diag_c[I] = d;
    }
}

// Per coarse row: candidate count c = sum of the lengths of its (<= 4) fine rows.  2c bounds the row's coarse
// entries (every candidate spawns <= 2 products), so the scratch offset of row I is the exclusive prefix sum of 2c:
// computed here per 64-row slice (wave scan) + slice totals, finished by scan_excl_dev.  No allocator atomics.
constexpr int kGalerkinTiers = 7;  // LDS list capacities 64 << t, t = 0..6 (2 KB .. 128 KB per wavefront)
// The tier lists are appended to behind one counter per tier, and same-address atomics retire at 11.4 ns per wave-instruction
// (scripts/microbench/atomic_rate.hip).  So a wavefront keeps the tiers of all its slices in LDS (kBoundIters of them at most: the launch is
// sized for that), counts them, reserves ONE range per tier and writes its rows there in a second walk over the LDS bytes.
constexpr int kBoundIters = 32;
__global__ __launch_bounds__(64) void galerkin_bound_k(SellDev P, const int *__restrict__ choice, int64_t n_coarse, int *__restrict__ out_max,
                                                       unsigned long long *__restrict__ out_sum, int *__restrict__ intra_off,
                                                       long long *__restrict__ slice_tot, int *__restrict__ tier_count, int *__restrict__ tier_list, int min_tier) {
    __shared__ signed char tiers[kBoundIters][64];
    const int lane = threadIdx.x;
    const int64_t n_slices = (n_coarse + 63) / 64;
    int mx = 0;
    unsigned long long sm = 0;
    int cnt[kGalerkinTiers];
#pragma unroll
    for (int t = 0; t < kGalerkinTiers; ++t) cnt[t] = 0;
    // (a wavefront takes ADJACENT slices, so that the tier lists come out in row order: neighbouring list entries — what concurrent merge
    // wavefronts work on — are neighbouring coarse rows)
    const int64_t per_wave = (n_slices + gridDim.x - 1) / gridDim.x;  // <= kBoundIters by the launch's size
    const int64_t s_lo = (int64_t)blockIdx.x * per_wave, s_hi = s_lo + per_wave < n_slices ? s_lo + per_wave : n_slices;
    int it = 0;
    for (int64_t s = s_lo; s < s_hi && it < kBoundIters; ++s, ++it) {
        const int64_t I = s * 64 + lane;
        int c = 0;
        if (I < n_coarse) {
            const RRow R = restriction_row(choice, I, P.n);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (a < R.n) c += P.row_len[R.idx[a]];
        }
        int tot;
        const int ex = wave_excl_scan(2 * c, tot);
        if (I < n_coarse) intra_off[I] = ex;
        if (lane == 0) slice_tot[s] = tot;
        mx = max(mx, c);
        sm += (unsigned long long)c;
        // the row's list never exceeds 2c entries: it goes to the narrowest tier that holds them (no overflow passes)
        int tier = -1;
        if (I < n_coarse) {
            tier = min_tier;  // sorting kernel: 128 slots (4 KB) at least, 16 wavefronts per CU already saturate the narrow rows
            while (tier < kGalerkinTiers - 1 && (64 << tier) < 2 * c) ++tier;
        }
        tiers[it][lane] = (signed char)tier;
#pragma unroll
        for (int t = 0; t < kGalerkinTiers; ++t) cnt[t] += __popcll(__ballot(tier == t));  // wave-uniform
    }
    int base[kGalerkinTiers];
#pragma unroll
    for (int t = 0; t < kGalerkinTiers; ++t) {
        base[t] = 0;
        if (cnt[t] > 0) {  // wave-uniform
            if (lane == 0) base[t] = atomicAdd(&tier_count[t], cnt[t]);
            base[t] = __shfl(base[t], 0, 64);
        }
    }
    it = 0;
    for (int64_t s = s_lo; s < s_hi && it < kBoundIters; ++s, ++it) {
        const int64_t I = s * 64 + lane;
        const int tier = tiers[it][lane];
#pragma unroll
        for (int t = 0; t < kGalerkinTiers; ++t) {
            const unsigned long long m = __ballot(tier == t);
            if (m == 0ull) continue;
            if (tier == t) tier_list[(int64_t)t * n_coarse + base[t] + __popcll(m & ((1ull << lane) - 1ull))] = (int)I;
            base[t] += __popcll(m);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, __shfl_down(mx, off, 64));
        sm += __shfl_down(sm, off, 64);
    }
    if (lane == 0) { atomicMax(out_max, mx); atomicAdd(out_sum, sm); }
}

// exclusive scan of one value per thread across a workgroup of kScanThreads (the building block of scan_excl_dev below).  256 threads, not
// 1024: beside the products of another stream a 16-wavefront workgroup waits for a CU with four free slots on every SIMD (100 us alone,
// 0.6-1.2 ms in the concurrent schedule, most of it before its first instruction).
constexpr int kScanThreads = 256;
__device__ __forceinline__ long long block_excl_scan(long long v, long long *buf /*[kScanThreads]*/, long long &total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const long long x = t >= off ? buf[t - off] : 0;
        __syncthreads();
        buf[t] += x;
        __syncthreads();
    }
    total = buf[kScanThreads - 1];
    const long long r = buf[t] - v;
    __syncthreads();
    return r;
}

// slice widths -> slice_ptr and packed sizes -> pk_ptr (and the window positions' sizes -> XWinDev::lptr).
// One wavefront per slice reduces its 64 row lengths (SELL width * 64; the packed slots: lengths rounded up to pairs, the slice to 16
// elements = 128 bytes; the positions: lengths rounded up to chunks of 8, the slice to 64 = 128 bytes; the entries rounded up to 16, what
// the launches decide by, PackedDev::total), then the tables are scanned (scan_excl_dev; a single workgroup reading all n row lengths
// itself took 0.9 + 1.4 ms per level at 5 M rows).
__global__ __launch_bounds__(kBlock) void slice_sizes_k(const int *__restrict__ row_len, int64_t n, int n_slices, int64_t *__restrict__ w_sell,
                                                        int64_t *__restrict__ w_pk, int64_t *__restrict__ w_pos, int64_t *__restrict__ w_tot) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t s = wave; s < n_slices; s += waves) {
        const int64_t r = s * 64 + lane;
        const int len = r < n ? row_len[r] : 0;
        int mx = len, sum = len, pairs = (len + 1) >> 1, chunks = (len + kPackChunk - 1) / kPackChunk;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mx = max(mx, __shfl_xor(mx, off, 64));
            sum += __shfl_xor(sum, off, 64);
            pairs += __shfl_xor(pairs, off, 64);
            chunks += __shfl_xor(chunks, off, 64);
        }
        if (lane == 0) {
            w_sell[s] = (int64_t)mx * 64;
            w_pk[s] = ((int64_t)pairs * 2 + 15) & ~(int64_t)15;
            w_pos[s] = ((int64_t)chunks * kPackChunk + 63) & ~(int64_t)63;
            w_tot[s] = ((int64_t)sum + 15) & ~(int64_t)15;
        }
    }
}
// The scans run over the whole chip (one workgroup's threads would read 64 different cache lines per load instruction, on the set-up's
// dependent chain, in front of a host read): per-chunk sums (coalesced), a scan of the <= kScanBlocks sums, per-chunk scans from their
// bases.  Integer sums: exact.
constexpr int kScanBlocks = 128;
__global__ __launch_bounds__(kScanThreads) void scan_part_k(const long long *__restrict__ in_a, const long long *__restrict__ in_b, int64_t n, int64_t chunk,
                                                            long long *__restrict__ part /* [2][kScanBlocks] sums, then [2] totals */) {
    __shared__ long long buf[kScanThreads];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = std::min<int64_t>(n, lo + chunk);
    long long sa = 0, sb = 0;
    for (int64_t e = lo + threadIdx.x; e < hi; e += kScanThreads) { sa += in_a[e]; if (in_b) sb += in_b[e]; }
    long long ta, tb;
    (void)block_excl_scan(sa, buf, ta);
    (void)block_excl_scan(sb, buf, tb);
    if (threadIdx.x == 0) { part[blockIdx.x] = ta; part[kScanBlocks + blockIdx.x] = tb; }
}
__global__ __launch_bounds__(kScanThreads) void scan_mid_k(long long *__restrict__ part, int n_blocks) {
    __shared__ long long buf[kScanThreads];
    const int t = threadIdx.x;
    const long long va = t < n_blocks ? part[t] : 0, vb = t < n_blocks ? part[kScanBlocks + t] : 0;
    long long ta, tb;
    const long long ra = block_excl_scan(va, buf, ta);
    const long long rb = block_excl_scan(vb, buf, tb);
    if (t < n_blocks) { part[t] = ra; part[kScanBlocks + t] = rb; }
    if (t == 0) { part[2 * kScanBlocks] = ta; part[2 * kScanBlocks + 1] = tb; }
}
__global__ __launch_bounds__(kScanThreads) void scan_write_k(const long long *__restrict__ in_a, const long long *__restrict__ in_b, int64_t n, int64_t chunk,
                                                             const long long *__restrict__ part, long long *__restrict__ out_a, long long *__restrict__ out_b,
                                                             int write_totals /* out[n] = total */) {
    __shared__ long long buf[kScanThreads];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = std::min<int64_t>(n, lo + chunk);
    long long base_a = part[blockIdx.x], base_b = part[kScanBlocks + blockIdx.x];
    for (int64_t t0 = lo; t0 < hi; t0 += kScanThreads) {  // (workgroup-uniform trip count)
        const int64_t e = t0 + threadIdx.x;
        const long long va = e < hi ? in_a[e] : 0, vb = (in_b && e < hi) ? in_b[e] : 0;
        long long ta, tb = 0;
        const long long ra = block_excl_scan(va, buf, ta);
        long long rb = 0;
        if (in_b) rb = block_excl_scan(vb, buf, tb);
        if (e < hi) { out_a[e] = base_a + ra; if (in_b) out_b[e] = base_b + rb; }
        base_a += ta;
        base_b += tb;
    }
    if (write_totals && blockIdx.x == 0 && threadIdx.x == 0) { out_a[n] = part[2 * kScanBlocks]; if (in_b) out_b[n] = part[2 * kScanBlocks + 1]; }
}
// out_a (and out_b) = exclusive prefix sums of in_a (in_b; null: one table); write_totals: out[n] = the sum.  `part`: 2 * kScanBlocks + 2 words.
static int scan_excl_dev(const long long *in_a, const long long *in_b, int64_t n, long long *out_a, long long *out_b, bool write_totals, long long *part, hipStream_t st) {
    const int64_t n1 = std::max<int64_t>(n, 1);
    int64_t chunk = (n1 + kScanBlocks - 1) / kScanBlocks;
    chunk = ((chunk + kScanThreads - 1) / kScanThreads) * kScanThreads;
    const int n_blocks = (int)((n1 + chunk - 1) / chunk);
    hipLaunchKernelGGL(scan_part_k, dim3(n_blocks), dim3(kScanThreads), 0, st, in_a, in_b, n, chunk, part);
    hipLaunchKernelGGL(scan_mid_k, dim3(1), dim3(kScanThreads), 0, st, part, n_blocks);
    hipLaunchKernelGGL(scan_write_k, dim3(n_blocks), dim3(kScanThreads), 0, st, in_a, in_b, n, chunk, (const long long *)part, out_a, out_b, write_totals ? 1 : 0);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// Row-contiguous mirror, compacted: the product's scratch rows (reserved at twice the candidate count per row: the bound of the
// symbolic step, about 3.7 times what the rows really hold) copied to exact size — entry k of coarse row r at
// new_base[r >> 6] + new_intra[r] + k — so that the scratch can be handed back.  One wavefront per slice of 64 coarse rows.
__global__ __launch_bounds__(64) void rows_compact_k(const int *__restrict__ row_len, int64_t n_rows, int n_slices, const long long *__restrict__ old_base,
                                                     const int *__restrict__ old_intra, const int *__restrict__ s_col, const double *__restrict__ s_val,
                                                     const int64_t *__restrict__ new_base, int *__restrict__ new_intra, int *__restrict__ out_col,
                                                     double *__restrict__ out_val) {
    const int lane = threadIdx.x;
    for (int64_t slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {
        const int64_t row = slice * 64 + lane;
        const bool live = row < n_rows;
        const int len = live ? row_len[row] : 0;
        int incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        const int excl = incl - len;
        if (live) new_intra[row] = excl;
        const long long ob = old_base[slice];
        const int64_t nb = new_base[slice];
        const int oi = live ? old_intra[row] : 0;
        for (int r = 0; r < 64; ++r) {
            const int n = __shfl(len, r, 64);
            const long long src = ob + __shfl(oi, r, 64);
            const int64_t dst = nb + __shfl(excl, r, 64);
            for (int e = lane; e < n; e += 64) {
                out_col[dst + e] = s_col[src + e];
                out_val[dst + e] = s_val[src + e];
            }
        }
    }
}

static std::atomic<long long> g_shared_galerkin{0};  // sibling operators built by a shared pass (orc_debug_shared_galerkin)
long long debug_shared_galerkin(bool reset) {
    const long long v = g_shared_galerkin.load(std::memory_order_relaxed);
    if (reset) g_shared_galerkin.store(0, std::memory_order_relaxed);
    return v;
}

// ------------------------------------------------------------------ galerkin(): the host side, phase by phase
// What flows between the phases of one product.  Systems 0 .. n_sys - 1: the leader (A, arena, L) and the siblings that share its pattern
// and pairing; everything symbolic exists once, the values once per system.
struct GalerkinPass {
    const MatView &A;
    const int *choice, *chooser;
    Arena &arena, &tmp;  // the leader's hierarchy arena; what is dead when the level is complete (`scratch`, else the arena itself)
    hipStream_t st;
    int64_t n, nc;
    int n_slices;
    size_t ncs;
    int n_sys;
    GalerkinSibling sys[3];
    // per coarse row / per slice; the scratch rows (s_col, sys[].s_val) start at slice_base[I >> 6] + intra_off[I]
    int *row_len, *diag, *intra_off, *s_col, *pk_col;
    long long *slice_tot, *slice_base, *scan_part;
    int64_t *slice_ptr, *pk_ptr, *lptr, *tot_ptr;  // tot_ptr: exact entries per slice, also the compacted row mirror's slice starts
    int *flags;                    // [0] = max candidates, [1] = overflow (cannot happen: rows are pre-sorted into tiers)
    unsigned long long *counters;  // [1] = sum of candidates
    int *tier_count, *tier_list;
    // host reads
    int htier[kGalerkinTiers], max_cand;
    // packed_total: the entries rounded up per slice to 16 (the mirror's size before its pairs: what the choices and the launches go by);
    // packed_slots / pos_slots: what the mirror's values and window positions occupy
    int64_t padded, packed_total, packed_slots, pos_slots;
    bool mirror;  // the level gets a packed mirror with LDS x windows
    SellDev Pc;
    double t_mark;
    void lap(const char *what) {  // ORC_AMG_TRACE only: wall time of the phase that just ended (drains the stream)
        if (!cfg().amg_trace) return;
        (void)hipStreamSynchronize(st);
        const double now = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
        if (what) fprintf(stderr, "[amg phase n=%lld] %s %.3f ms\n", (long long)n, what, now - t_mark);
        t_mark = now;
    }
};

// Bounds and tiers, up to the first host read: per coarse row the candidate count, its scratch offset and its LDS tier; the totals size
// the scratch rows (one set of columns, one set of values per system).
static int galerkin_bounds(GalerkinPass &g) {
    Arena &arena = g.arena, &tmp = g.tmp;
    hipStream_t st = g.st;
    const int n_slices = g.n_slices;
    ORC_TRY(arena.alloc(g.ncs, &g.row_len));
    ORC_TRY(arena.alloc(g.ncs, &g.diag));
    ORC_TRY(tmp.alloc(g.ncs, &g.intra_off));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &g.slice_tot));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &g.slice_base));
    ORC_TRY(arena.alloc((size_t)n_slices + 1, &g.slice_ptr));
    ORC_TRY(tmp.alloc((size_t)4, &g.flags));
    ORC_TRY(tmp.alloc((size_t)2, &g.counters));
    ORC_HIP(hipMemsetAsync(g.flags, 0, 4 * sizeof(int), st));
    ORC_HIP(hipMemsetAsync(g.counters, 0, 2 * sizeof(unsigned long long), st));
    ORC_TRY(tmp.alloc((size_t)kGalerkinTiers + 1, &g.tier_count));
    ORC_TRY(tmp.alloc((size_t)kGalerkinTiers * g.ncs, &g.tier_list));
    ORC_HIP(hipMemsetAsync(g.tier_count, 0, (kGalerkinTiers + 1) * sizeof(int), st));
    // (a wavefront walks at most kBoundIters slices: the grid grows with the level beyond 8 192 x kBoundIters slices = 16.8 M coarse rows)
    const int64_t bound_grid = std::max<int64_t>(std::min<int64_t>(std::max<int64_t>(n_slices, 1), 8192), ((int64_t)n_slices + kBoundIters - 1) / kBoundIters);
    hipLaunchKernelGGL(galerkin_bound_k, dim3((unsigned)bound_grid), dim3(64), 0, st, g.A.P, g.choice, g.nc, g.flags, g.counters + 1, g.intra_off,
                       g.slice_tot, g.tier_count, g.tier_list, 0);
    ORC_TRY(tmp.alloc((size_t)2 * kScanBlocks + 2, &g.scan_part));
    ORC_TRY(scan_excl_dev(g.slice_tot, nullptr, (int64_t)n_slices, g.slice_base, nullptr, false, g.scan_part, st));
    int hflags[4];
    unsigned long long hcount[2];
    ORC_HIP(hipMemcpyAsync(hflags, g.flags, sizeof(hflags), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(hcount, g.counters, sizeof(hcount), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(g.htier, g.tier_count, sizeof(g.htier), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    g.max_cand = std::max(hflags[0], 1);
    note_galerkin_stats(g.htier, hflags[0]);
    const long long scratch_cap = (long long)std::max<unsigned long long>(2ull * hcount[1], 64ull);
    ORC_TRY(tmp.alloc((size_t)scratch_cap, &g.s_col));
    const bool fine_mirror = g.A.rows.col != nullptr;
    for (int s = 0; s < g.n_sys; ++s) {
        const MatView &B = *g.sys[s].A;
        if (B.P.n != g.n || B.P.col != g.A.P.col || (B.rows.col != nullptr) != fine_mirror || (fine_mirror && B.rows.col != g.A.rows.col))
            return set_error(ORC_ERR_BAD_ARGUMENT, "galerkin: a sibling system does not share the leader's pattern");
        ORC_TRY(tmp.alloc((size_t)scratch_cap, &g.sys[s].s_val));
    }
    return ORC_OK;
}

// The merge: one launch of galerkin_merge_k per non-empty LDS tier (32 B per list slot: every row was assigned to the narrowest list that is
// guaranteed to hold it), all systems' value sets through the same pass.
static int galerkin_merge(GalerkinPass &g) {
    const int n_sib = g.n_sys - 1;
    // lanes per coarse row by LDS tier (list capacity 64 << t); ORC_GALERKIN_GROUPS="g0,g1,..." overrides
    int tier_group[kGalerkinTiers] = {16, 16, 32, 64, 64, 64, 64};  // measured at 10.24 M fine rows (levels of 7 / 15 / 34 entries per row)
    if (!cfg().galerkin_groups.empty()) {
        int t = 0;
        for (const char *q = cfg().galerkin_groups.c_str(); *q && t < kGalerkinTiers; ++t) {
            const int v = atoi(q);
            if (v == 16 || v == 32 || v == 64) tier_group[t] = v;
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
    }
    MergeSiblings X;
    const bool fine_mirror = g.A.rows.col != nullptr;
    for (int x = 0; x < n_sib; ++x) {
        const MatView &B = *g.sys[x + 1].A;
        X.val[x] = fine_mirror ? B.rows.val : B.val;
        X.s1[x] = B.s1;
        X.s2[x] = B.s2;
        X.s_val[x] = g.sys[x + 1].s_val;
    }
    // the nine instantiations: [sibling systems][16 / 32 / 64 lanes per coarse row]  (one system with narrow groups on the widest tiers: only
    // with ORC_GALERKIN_GROUPS — 16 lanes per row on tier 5, 32 on tier 6 keep 96 KB of lists per wavefront)
    using MergeKernel = decltype(&galerkin_merge_k<64, 1>);
    static const MergeKernel kMerge[3][3] = {{&galerkin_merge_k<16, 1>, &galerkin_merge_k<32, 1>, &galerkin_merge_k<64, 1>},
                                             {&galerkin_merge_k<16, 2>, &galerkin_merge_k<32, 2>, &galerkin_merge_k<64, 2>},
                                             {&galerkin_merge_k<16, 3>, &galerkin_merge_k<32, 3>, &galerkin_merge_k<64, 3>}};
    static std::once_flag attr_once;  // several lane threads reach this concurrently
    std::call_once(attr_once, [] {
        for (const auto &row : kMerge)
            for (const MergeKernel k : row) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    if ((size_t)2 * g.max_cand > (size_t)(64 << (kGalerkinTiers - 1))) return set_error(ORC_ERR_BAD_ARGUMENT, "Galerkin row too long for LDS (%d candidates)", g.max_cand);
    for (int t = 0; t < kGalerkinTiers; ++t) {
        if (g.htier[t] == 0) continue;
        const int cap = 64 << t;
        int G = tier_group[t];  // narrow rows: two or four coarse rows per wavefront
        // a wavefront's lists must fit the LDS of one workgroup: wider groups (fewer rows per wavefront) where the sibling value sets would not
        while (G < 64 && (size_t)cap * (size_t)(12 + 8 * n_sib) * (size_t)(64 / G) > (size_t)150 * 1024) G <<= 1;
        const int rows_per_wave = 64 / G;
        const size_t smem = (size_t)cap * (size_t)(12 + 8 * n_sib) * (size_t)rows_per_wave;
        if (smem > (size_t)160 * 1024) return set_error(ORC_ERR_BAD_ARGUMENT, "Galerkin row too long for a shared pass (%d candidates, %d systems)", g.max_cand, g.n_sys);
        // resident wavefronts per CU: one system 80 VGPRs (amdgpu_waves_per_eu(6)) and 12 bytes of LDS per list slot: six per SIMD; the shared
        // pass carries three value sets in 128 VGPRs: four per SIMD.  A launch that no longer fits leaves a tail that runs alone.
        const int merge_waves = n_sib == 0 ? 24 : 16;
        const int waves_per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)merge_waves, (size_t)(150 * 1024) / smem));
        const int grid = (int)std::min<int64_t>(((int64_t)g.htier[t] + rows_per_wave - 1) / rows_per_wave, (int64_t)256 * waves_per_cu);
        const int *tl = g.tier_list + (int64_t)t * g.nc, *tc = g.tier_count + t;
        hipLaunchKernelGGL(kMerge[n_sib][G == 16 ? 0 : (G == 32 ? 1 : 2)], dim3(grid), dim3(64), smem, g.st, g.A, g.choice, g.chooser, g.nc, cap, g.row_len,
                           (const long long *)g.slice_base, (const int *)g.intra_off, g.s_col, g.sys[0].s_val, tl, tc, X);
    }
    return ORC_OK;
}

// Sizes, scans and the pack: the coarse rows' lengths -> the slice tables of the SELL image, the packed mirror and its window positions; the
// second host read; then every system's scratch rows into its SELL image (and packed mirror, where the level gets one).
static int galerkin_pack(GalerkinPass &g) {
    Arena &arena = g.arena, &tmp = g.tmp;
    hipStream_t st = g.st;
    const int n_slices = g.n_slices;
    const int64_t nc = g.nc;
    int64_t *w_sell, *w_pk, *w_pos, *w_tot;
    ORC_TRY(arena.alloc((size_t)n_slices + 1, &g.pk_ptr));
    ORC_TRY(arena.alloc((size_t)n_slices + 1, &g.lptr));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &w_sell));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &w_pk));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &w_pos));
    ORC_TRY(tmp.alloc((size_t)n_slices + 1, &w_tot));
    ORC_TRY(arena.alloc((size_t)n_slices + 1, &g.tot_ptr));
    hipLaunchKernelGGL(slice_sizes_k, dim3((unsigned)std::min<int64_t>(((int64_t)n_slices + 3) / 4, 4096)), dim3(kBlock), 0, st, g.row_len, nc, n_slices, w_sell, w_pk,
                       w_pos, w_tot);
    static_assert(sizeof(long long) == sizeof(int64_t), "64-bit tables");
    ORC_TRY(scan_excl_dev(reinterpret_cast<const long long *>(w_sell), reinterpret_cast<const long long *>(w_pk), (int64_t)n_slices, reinterpret_cast<long long *>(g.slice_ptr),
                          reinterpret_cast<long long *>(g.pk_ptr), true, g.scan_part, st));
    ORC_TRY(scan_excl_dev(reinterpret_cast<const long long *>(w_pos), reinterpret_cast<const long long *>(w_tot), (int64_t)n_slices, reinterpret_cast<long long *>(g.lptr),
                          reinterpret_cast<long long *>(g.tot_ptr), true, g.scan_part, st));
    ORC_HIP(hipGetLastError());
    int hflags[4];
    ORC_HIP(hipMemcpyAsync(&g.packed_total, g.tot_ptr + n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(&g.packed_slots, g.pk_ptr + n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(&g.pos_slots, g.lptr + n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(&g.padded, g.slice_ptr + n_slices, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipMemcpyAsync(hflags, g.flags, sizeof(hflags), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    const int64_t padded = g.padded, packed_total = g.packed_total;
    if (hflags[1]) return set_error(ORC_ERR_BAD_ARGUMENT, "Galerkin overflow (%d)", hflags[1]);
    if (padded >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "coarse matrix too large for 32-bit offsets");
    // Packed mirror + LDS x windows for the levels whose rows are long enough for a window to be re-used (ORC_SPMV_XWIN_MIN_NNZ entries per
    // row; < 0 switches the mirror off) — or, from half that length on, whose padded image wastes what the windows cost: 15 % padding or more
    // (rows of a tet / hex / polyhedral mesh paired).  The measurements behind both thresholds: HISTORY.md, "amg.hip split".
    const int xwin_min = cfg().spmv_xwin_min_nnz;
    const bool long_rows = packed_total >= (int64_t)xwin_min * nc;
    const bool ragged_rows = 2 * packed_total >= (int64_t)xwin_min * nc && (double)padded >= 1.15 * (double)packed_total;
    g.mirror = xwin_min >= 0 && packed_total > 0 && (long_rows || ragged_rows);
    const int64_t *pk_ptr = g.mirror ? g.pk_ptr : nullptr;
    const unsigned pack_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_slices, 256 * 12));
    for (int s = 0; s < g.n_sys; ++s) {  // system 0 writes the pattern too; the siblings their values on the same images
        GalerkinSibling &sy = g.sys[s];
        int *col = nullptr, *pk_col = nullptr;  // the pattern: system 0's business (kValuesOnly for the others)
        if (s == 0) ORC_TRY(sy.arena->alloc((size_t)std::max<int64_t>(padded, 1), &col));
        ORC_TRY(sy.arena->alloc((size_t)std::max<int64_t>(padded, 1), &sy.val));
        if (g.mirror && s == 0) ORC_TRY(sy.arena->alloc((size_t)g.packed_slots, &pk_col));
        if (g.mirror) ORC_TRY(sy.arena->alloc((size_t)g.packed_slots, &sy.pk_val));
        if (s == 0) {
            SellDev &Pc = g.Pc;
            Pc.n = nc; Pc.ncols = nc; Pc.n_slices = n_slices; Pc.ragged = padded < 24 * nc ? 2 : 1; Pc.padded = padded;
            Pc.slice_ptr = g.slice_ptr; Pc.row_len = g.row_len; Pc.col = col; Pc.diag_pos = g.diag;
            g.pk_col = pk_col;
        }
        hipLaunchKernelGGL(s == 0 ? galerkin_pack_fused_k<false> : galerkin_pack_fused_k<true>, dim3(pack_grid), dim3(64), 0, st, g.Pc, (const long long *)g.slice_base,
                           (const int *)g.intra_off, (const int *)g.s_col, (const double *)sy.s_val, col, sy.val, s == 0 ? g.diag : nullptr, pk_ptr, pk_col, sy.pk_val);
        ORC_HIP(hipGetLastError());
    }
    return ORC_OK;
}

// The levels as their owners will see them.  (A sibling's level is written by this thread while its owner waits: SiblingPairing.)
static void galerkin_publish(GalerkinPass &g) {
    const AmgHierarchy::Level &lead = *g.sys[0].L;
    for (int s = 0; s < g.n_sys; ++s) {
        AmgHierarchy::Level &L = *g.sys[s].L;
        if (s > 0) {
            L = AmgHierarchy::Level();
            L.choice = lead.choice; L.chooser = lead.chooser; L.rounds = lead.rounds;
        }
        L.P = g.Pc; L.val = g.sys[s].val; L.n = g.nc; L.padded = g.padded;
        L.pk = g.mirror ? PackedDev{g.pk_ptr, g.pk_col, g.sys[s].pk_val, g.packed_total, g.packed_slots} : PackedDev();
        L.xw = XWinDev();
        L.rows = RowsDev();
    }
}

// The row-contiguous mirror the NEXT level's aggregation and product walk.  Without `scratch` the scratch rows themselves (reserved at twice
// the candidate count per row, about 3.7 times what the rows hold) stay alive as the mirror.  With it: an exact-size copy per system, the
// slices starting at the entries' offsets (tot_ptr).  The mirror of the level below (A.rows) is dead now that this product's kernels are
// queued (same stream): both take turns in the scratch arena's companion, so a hierarchy keeps no mirror once it is built (2 GB of 10.3 GB
// per hierarchy at 10.24 M rows).  A whole copy per sibling: the leader's is gone when ITS next level is built.
static int galerkin_row_mirror(GalerkinPass &g, bool compact) {
    AmgHierarchy::Level &lead = *g.sys[0].L;
    if (!compact) {
        lead.rows = RowsDev{g.slice_base, g.intra_off, g.s_col, g.sys[0].s_val};
        return ORC_OK;
    }
    for (int s = 0; s < g.n_sys; ++s) {
        GalerkinSibling &sy = g.sys[s];
        Arena &ra = sy.rows_arena ? *sy.rows_arena : *sy.arena;
        if (sy.rows_arena) ra.release(Arena::Mark{0, 0});
        int *r_col, *r_intra;
        double *r_val;
        ORC_TRY(ra.alloc((size_t)g.packed_total, &r_col));
        ORC_TRY(ra.alloc((size_t)g.packed_total, &r_val));
        ORC_TRY(ra.alloc(g.ncs, &r_intra));
        hipLaunchKernelGGL(rows_compact_k, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(g.n_slices, 256 * 16))), dim3(64), 0, g.st, (const int *)g.row_len, g.nc, g.n_slices,
                           (const long long *)g.slice_base, (const int *)g.intra_off, (const int *)g.s_col, (const double *)sy.s_val, (const int64_t *)g.tot_ptr, r_intra, r_col, r_val);
        ORC_HIP(hipGetLastError());
        sy.L->rows = RowsDev{reinterpret_cast<const long long *>(g.tot_ptr), r_intra, r_col, r_val};
        sy.L->rows_transient = sy.rows_arena != nullptr;
    }
    return ORC_OK;
}

int galerkin(const MatView &A, Arena &arena, AmgHierarchy::Level &L, Arena *scratch, bool last_level, const GalerkinSibling *sib, int n_sib) {
    if (n_sib < 0 || n_sib > 2 || (n_sib > 0 && (!scratch || !sib))) return set_error(ORC_ERR_BAD_ARGUMENT, "galerkin: bad sibling arguments");
    Arena &tmp = scratch ? *scratch : arena;
    ArenaScope tmp_scope(tmp);  // with `scratch`: unwinds it on every exit; without: re-marked below so that nothing is released
    const int64_t n = A.P.n, nc = n / 2 + n % 2;  // :13
    GalerkinPass g{A, L.choice, L.chooser, arena, tmp, ctx().stream, n, nc, (int)((nc + 63) / 64), (size_t)std::max<int64_t>(nc, 1), n_sib + 1};
    g.sys[0] = GalerkinSibling{&A, &arena, scratch ? &scratch->companion() : nullptr, &L};
    for (int x = 0; x < n_sib; ++x) g.sys[x + 1] = sib[x];
    g.lap(nullptr);
    ORC_TRY(galerkin_bounds(g));
    g.lap("galerkin bounds");
    ORC_TRY(galerkin_merge(g));
    g.lap("galerkin product");
    ORC_TRY(galerkin_pack(g));
    g.lap("galerkin pack");
    if (!g.mirror) ORC_TRY(narrow_image(g.Pc, arena, tmp));  // the first coarse level: the uniform kernels multiply it
    galerkin_publish(g);
    if (!scratch || (g.packed_total > 0 && !last_level)) ORC_TRY(galerkin_row_mirror(g, scratch != nullptr));
    if (g.mirror) ORC_TRY(build_windows(g.sys, g.n_sys, g.lptr, g.pos_slots, tmp));
    g.lap("galerkin mirrors");
    if (!scratch) tmp_scope.mark = tmp.mark();  // the scratch rows ARE the mirror: everything stays
    if (n_sib > 0) g_shared_galerkin.fetch_add(n_sib, std::memory_order_relaxed);
    return ORC_OK;
}

}  // namespace orc
