// amg_pairing.hip — build_restriction_matrix's pairing (Strongest; linear_algebra.rs:12-63) on the device.
//
// What has to be reproduced: a SEQUENTIAL greedy pairing — row i takes the most negative off-diagonal a_ij whose column j no
// earlier row has taken; rows 2k and 2k+1 both land in coarse row k, so R is not a partition and carries weights of 2.
//   * aggregate(): the pairing by deferred acceptance (da_first_k, da_chase_k, da_finish_k: below), certified by ONE
//     verification pass (agg_verify_k) and one host read; slice-sequential sweeps (agg_init_k, agg_sweep_k, agg_rotate_k) behind it for a
//     pairing the certification rejects, a chain the step budget cuts, or ORC_AMG_DA=0;
//   * pairing_mismatches(): is a given pairing the fixed point of other matrices on the same pattern too?
//   * SiblingPairing (linalg.hpp): how the u, v, w set-up threads hand a pairing and a shared Galerkin pass to each other;
//   * the certification counters and the set-up statistics behind orc_debug_amg_certification / orc_debug_amg_setup_stats.
#include <algorithm>
#include <atomic>
#include <mutex>

#include "amg.hpp"

namespace orc {

struct AggCounters {
    int changed;  // rows whose choice changed in the current sweep
    int rounds;
};

// ---- the pairing as a fixed point: first-taker table, row evaluation, the sweeps of the fallback
// State: choice[i] (partner of row i or -1).  A column j is "in combined_cells when row i is visited"
// (linear_algebra.rs:41) iff some row m < i chose it, i.e. iff taken_by[j] = min{m : choice[m] = j} < i.
// Every round rebuilds taken_by from choice (reset + atomicMin scatter), then sweeps: one thread
// walks one 64-row slice IN ORDER, like the reference's loop, seeing its own updates immediately
// (Gauss-Seidel inside the slice) and the other slices' as they land (chaotic relaxation).  A
// sweep that changes nothing has evaluated every row against a taken_by that is exact for the
// final choice, so the state is the unique solution of the triangular system = the sequential
// result.  Chains inside a slice resolve in one sweep; a chain that crosses k slices needs ~k
// sweeps (an x-line of 400 cells: ~7).  Slices that cannot be affected by the last sweep's changes
// are skipped.
__global__ void agg_reset_k(int *__restrict__ taken_by, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) taken_by[i] = 0x7fffffff;
}
__global__ void agg_scatter_k(const int *__restrict__ choice, int *__restrict__ taken_by, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (choice[i] >= 0) atomicMin(&taken_by[choice[i]], (int)i);
}

// arg-min over j != i of a_ij among columns not taken by an earlier row (strict <, first wins: :37-52)
__device__ __forceinline__ int agg_eval_row(const MatView &A, const int *__restrict__ taken_by, int64_t i, bool constrained) {
    const int len = A.P.row_len[i];
    const int64_t base = A.P.slice_ptr[i >> 6] + (i & 63);
    double best = 1.7976931348623157e308;  // Float::MAX
    int bj = -1;
    for (int k = 0; k < len; ++k) {
        const int64_t pos = base + (int64_t)k * 64;
        const int j = A.P.col[pos];
        if (j == i || j >= A.P.n) continue;  // ghost columns (partitioned level 0) are never partners: aggregates stay on the rank
        if (constrained && taken_by[j] < i) continue;
        const double a = view_value(A, i, pos);
        if (a < best) { best = a; bj = j; }
    }
    return bj;
}

__global__ void agg_init_k(MatView A, int *__restrict__ choice) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.P.n; i += (int64_t)gridDim.x * blockDim.x) choice[i] = agg_eval_row(A, nullptr, i, false);
}

// Preference lists: a row's order of preference (value ascending, position ascending: the strict <, first-wins scan of linear_algebra.rs:37-52)
// does not change while a pairing is sought; da_first_k keeps every row's kPrefs most preferred columns (-1 = fewer; bit 30 of the last entry =
// the row has more candidates than listed).  Four: one 16-byte line per row (lists of three straddle cache lines).
constexpr int kPrefs = 4;
constexpr int kPrefMore = 1 << 30;

// one thread = one slice, rows in ascending order (the fallback of aggregate(): works on any pattern, symmetric or not)
__global__ void agg_sweep_k(MatView A, int *__restrict__ choice, int *__restrict__ taken_by, AggCounters *C) {
    const int64_t n = A.P.n;
    int changed = 0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < A.P.n_slices; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = s * 64, hi = lo + 64 < n ? lo + 64 : n;
        for (int64_t i = lo; i < hi; ++i) {
            const int old = choice[i];
            const int nv = agg_eval_row(A, taken_by, i, true);
            if (nv == old) continue;
            ++changed;
            choice[i] = nv;
            if (nv >= 0) atomicMin(&taken_by[nv], (int)i);
            // `old` may still be taken by another row; leaving taken_by[old] <= i is only ever too pessimistic for rows > i and is repaired
            // by the next sweep's rebuild, which cannot be skipped because this sweep counted a change.
        }
    }
    if (changed) atomicAdd(&C->changed, changed);
}

__global__ void agg_rotate_k(AggCounters *C, int *snapshot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *snapshot = C->changed;
        C->changed = 0;
        C->rounds += 1;
    }
}

// Is `choice` the fixed point?  Every row is evaluated against the exact first-taker table of `choice` itself; a state in
// which no row would choose differently is the sequential greedy pairing (the fixed point is unique).  Thread per row:
// coalesced reads of the interleaved image.  Counts the rows that would change.
__global__ void agg_verify_k(MatView A, const int *__restrict__ choice, const int *__restrict__ taken_by, AggCounters *C) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.P.n; i += (int64_t)gridDim.x * blockDim.x)
        if (agg_eval_row(A, taken_by, i, true) != choice[i]) ++bad;
    if (bad) atomicAdd(&C->changed, bad);  // rare: a verified pairing has none
}

// One atomicAdd per wavefront instead of one per lane: the lanes that want a slot are counted with a ballot, the
// lowest of them reserves the block of slots and every lane takes its rank inside it.  The work lists of a round hold
// tens of thousands of rows; their appends all hit ONE counter, and same-address atomics retire at ~12 ns each on
// this chip — that serialisation, not the row work, was most of a round's 50-60 us.
__device__ __forceinline__ int wave_append_slot(int *counter, bool want) {
    const unsigned long long m = __ballot(want);
    if (!want) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader, 64);
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void chooser_k(const int *__restrict__ choice, int *__restrict__ chooser, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (choice[i] >= 0) chooser[choice[i]] = (int)i;  // a column is taken at most once (:41, :55)
}

// ------------------------------------------------------------------ the pairing by deferred acceptance
// The reference's loop (linear_algebra.rs:30-60) is a SERIAL DICTATORSHIP: row i takes the column it prefers most — value ascending, position
// ascending: the strict <, first-wins scan, with the diagonal, NaNs and Float::MAX left out — among the columns no EARLIER row holds.  Give every
// column the same priority order over the rows (the lower index wins) and that allocation is the unique stable matching, which row-proposing
// deferred acceptance reaches from ANY order of proposals: a row proposes down its list; a column keeps the lowest row that ever proposed to it;
// a row that loses a column (rejected at once, or displaced later by a lower row) goes on to ITS next preference and never back up — a column,
// once held, is held by ever lower rows.  The whole mutable state is holder[j] = the lowest row that has proposed to column j, and one
// returning atomicMin IS a proposal: it returns a lower row -> rejected; a higher one -> accepted, and that row is displaced and becomes the
// lane's next proposer; nobody -> the chain ends.  A displaced row's next column needs no per-row state: it is the preference after the column
// just lost.  One lane per row starts a chain; the chains of the channel (a triangle of displaced rows at the end of every grid line: DESIGN §6)
// are followed by the lanes that run into them, thousands at a time, each step two dependent accesses (the atomic, the next row's preference
// list).  No fences: holder is touched by device-scope atomics only, everything else is read-only while the kernel runs.
// The slice sweeps above stay as the fallback for a pairing the verification pass rejects or a chain that exceeds the step budget — neither
// has been seen outside the tests that force them (scripts/analysis/deferred_acceptance.py: the argument, checked on the CPU).
struct DaCounters {
    int overflow;  // chains cut off by the step budget (the fallback then runs)
    int steps;     // proposals made by da_chase_k: statistics
    int list;      // rows the first pass left to the chains
    int scans;     // (statistics: proposals found by a scan of the row, the list having run out)
    int longest;   // (statistics: proposals of the longest chain)
};

// A look at the holder table before proposing: holder[j] only ever DECREASES, so a value below r — however stale the copy a load returns —
// means the proposal would be rejected, and the row passes the column by without an atomic.  (A stale copy errs towards "free": the atomic
// that follows is the authority.)  Relaxed agent-scope loads: past the vector L1, which would never show another CU's atomics.
__device__ __forceinline__ int da_peek(const int *holder, int j) { return __hip_atomic_load(holder + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// First pass: one thread per row, the SELL image (lane = row: coalesced).  The row's most preferred column that no lower row is seen to hold
// (agg_eval_row's scan with the holder table as the first-taker table) gets the row's proposal.  Whoever loses — the row itself, when a lower
// row got in between the look and the atomic; or the higher row it displaces — goes on the list of the chains: (row, the column it lost on).
// The scan also leaves the row's kPrefs most preferred columns behind (value ascending, position ascending; bit 30 of the
// last entry: the row has more candidates): a chain that displaces the row finds its next proposal in ONE 16-byte line at a known address.
__global__ __launch_bounds__(kBlock) void da_first_k(MatView A, int *holder, int2 *__restrict__ list, DaCounters *C, int *__restrict__ prefs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int loser = -1, lost_on = -1;
    if (i < A.P.n) {
        const int len = A.P.row_len[i];
        const int64_t base = A.P.slice_ptr[i >> 6] + (i & 63);
        double bv[kPrefs];
        int bj[kPrefs];
#pragma unroll
        for (int q = 0; q < kPrefs; ++q) { bv[q] = 1.7976931348623157e308; bj[q] = -1; }
        double best = 1.7976931348623157e308;  // Float::MAX
        int fj = -1, cand = 0;
        for (int k = 0; k < len; ++k) {
            const int64_t pos = base + (int64_t)k * 64;
            const int j = A.P.col[pos];
            if (j == i || j >= A.P.n) continue;  // ghost columns (partitioned level 0) are never partners
            const double a = view_value(A, i, pos);
            if (!(a < 1.7976931348623157e308)) continue;  // never chosen (nor a NaN)
            ++cand;
            int pos_q = kPrefs;  // its place in the list: in front of the first listed entry it is STRICTLY smaller than
#pragma unroll
            for (int q = kPrefs - 1; q >= 0; --q)
                if (a < bv[q]) pos_q = q;
#pragma unroll
            for (int q = kPrefs - 1; q >= 1; --q)
                if (q > pos_q) { bv[q] = bv[q - 1]; bj[q] = bj[q - 1]; }
#pragma unroll
            for (int q = 0; q < kPrefs; ++q)
                if (q == pos_q) { bv[q] = a; bj[q] = j; }
            if (!(a < best)) continue;
            if (da_peek(holder, j) < (int)i) continue;
            best = a; fj = j;
        }
        int4 pl;
        pl.x = bj[0]; pl.y = bj[1]; pl.z = bj[2];
        pl.w = (cand > kPrefs && bj[3] >= 0) ? (bj[3] | kPrefMore) : bj[3];
        reinterpret_cast<int4 *>(prefs)[i] = pl;
        if (fj >= 0) {
            const int old = atomicMin(&holder[fj], (int)i);
            if (old < (int)i) { loser = (int)i; lost_on = fj; }
            else if (old != 0x7fffffff) { loser = old; lost_on = fj; }
        }
    }
    const int slot = wave_append_slot(&C->list, loser >= 0);
    if (loser >= 0) list[slot] = make_int2(loser, lost_on);
}

// The chains: a group of G lanes takes a listed row and follows what its proposals set off — propose; if a higher row is displaced, go on as
// that row — until a proposal meets a free column or a row runs out of candidates; then it takes the next listed row.  No state but the holder
// table; no group waits for another.
//
// ONE flat loop per wavefront, the same straight-line code for its 64 / G groups in every pass: a group that is through with its chain takes
// its next row in the same pass in which the others make their next step (nested "for every listed row { follow the chain }" leaves a group
// whose chain has ended masked off until the longest chain of its wavefront ends).  Loads are unconditional at clamped addresses (a
// conditional load is a branch with a wait of its own behind it), the results masked.  A pass:
//   1. the row's LIST (da_first_k: its kPrefs most preferred columns): lanes 0-3 look at the holders of the listed columns behind `after`;
//   2. only if some group of the wavefront found them all taken and its row has more candidates: the SCAN of the row — descriptor, then
//      columns and values (<= kDaRegs entries per lane in registers, only the slots the wavefront's longest scanned row needs; longer rows:
//      two sweeps), then every candidate's holder, two reductions;
//   3. the proposal (one returning atomicMin per group) — beside it, already on its way, the list of the row it will most likely displace
//      (the holder just seen).
// Two dependent round trips per step where the list reaches, five where the row is scanned.  What bounds the coarse levels is the LONGEST
// chain times those trips, not the number of proposals.
constexpr int kDaRegs = 8;
template <int G>
__global__ __launch_bounds__(kBlock) void da_chase_k(MatView A, int *holder, const int2 *__restrict__ list, DaCounters *C, int max_steps, const int *__restrict__ prefs) {
    const int gl = threadIdx.x & (G - 1);
    const int shift = (threadIdx.x & 63) & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (((1ull << G) - 1ull) << shift);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) / G;
    const int count = C->list;
    const int4 *pl4 = reinterpret_cast<const int4 *>(prefs);
    const int n = (int)A.P.n;
    const bool mirror = A.rows.col != nullptr;
    const int32_t *colp = mirror ? A.rows.col : A.P.col;
    const double *valp = mirror ? A.rows.val : A.val;
    const int64_t stride = mirror ? 1 : 64;
    int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    bool have = e < count;
    int r = 0, after = -1;
    int4 pl = make_int4(-1, -1, -1, -1);
    if (have) {
        const int2 it = list[e];
        r = it.x; after = it.y;
        pl = pl4[r];
    }
    int steps = 0, scans = 0, chain_steps = 0, longest = 0;
    bool cut = false;
    while (__ballot(have) != 0ull) {
        // ---- 1. the list
        const int p3 = pl.w >= 0 ? (pl.w & ~kPrefMore) : -1;
        const bool more = pl.w >= 0 && (pl.w & kPrefMore) != 0;
        const int pq = gl == 0 ? pl.x : (gl == 1 ? pl.y : (gl == 2 ? pl.z : (gl == 3 ? p3 : -1)));
        const int first = after == pl.x ? 1 : (after == pl.y ? 2 : (after == pl.z ? 3 : 4));  // the first listed preference behind `after`
        const bool beyond = first == 4 && after != p3;                                         // `after` lies behind the whole list already
        const bool look = have && !beyond && gl < kPrefs && gl >= first && pq >= 0;
        int h = da_peek(holder, look ? pq : 0);
        h = look ? h : -1;
        const unsigned long long free_all = __ballot(look && h >= r);
        const unsigned free_mine = (unsigned)((free_all & gmask) >> shift);
        int cand = -1, seen = 0x7fffffff;
        if (free_mine) {
            const int q = __ffs((int)free_mine) - 1;
            cand = __shfl(pq, q, G);
            seen = __shfl(h, q, G);
        }
        const bool need_scan = have && (beyond || (!free_mine && more));
        const int scan_after = beyond ? after : p3;  // (a row's unlisted candidates all rank behind its last listed one)
        // ---- 2. the scan, for the groups whose list ran out (wave-uniform branch; inside, every lane runs the same code)
        if (__ballot(need_scan) != 0ull) {
            const int rs = need_scan ? r : 0;
            int len = A.P.row_len[rs];
            const int64_t base = mirror ? (int64_t)A.rows.slice_base[rs >> 6] + A.rows.intra_off[rs] : A.P.slice_ptr[rs >> 6] + (rs & 63);
            const double s1 = A.s1 ? A.s1[rs] : 1., s2 = A.s2 ? A.s2[rs] : 1.;
            len = need_scan ? len : 0;
            int k_c = -1;
            double v_c = 0.;
            double best = 1.7976931348623157e308;  // Float::MAX
            int bk = 0x7fffffff, bj = -1, bh = 0x7fffffff;
            int len_max = len;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) len_max = max(len_max, __shfl_xor(len_max, off, 64));
            if (len_max <= G * kDaRegs) {
                const int u_max = (len_max + G - 1) / G;  // wave-uniform
                int cj[kDaRegs], hp[kDaRegs];
                double cv[kDaRegs];
#pragma unroll
                for (int u = 0; u < kDaRegs; ++u) {
                    cj[u] = -1;
                    if (u < u_max) {
                        const int k = gl + u * G;
                        const int c = colp[base + (int64_t)(k < len ? k : 0) * stride];
                        cj[u] = k < len ? c : -1;
                    }
                }
#pragma unroll
                for (int u = 0; u < kDaRegs; ++u) {
                    cv[u] = 0.;
                    if (u < u_max) {
                        const int k = gl + u * G;
                        cv[u] = valp[base + (int64_t)(k < len ? k : 0) * stride];
                    }
                }
#pragma unroll
                for (int u = 0; u < kDaRegs; ++u) {
                    hp[u] = -1;
                    if (u >= u_max) continue;
                    const bool ok = cj[u] >= 0 && cj[u] != rs && cj[u] < n;
                    const int hh = da_peek(holder, ok ? cj[u] : 0);
                    hp[u] = ok ? hh : -1;  // (-1: not a candidate)
                    double t = cv[u];
                    if (A.s1) t = s1 * t;  // RowWalk::value's order
                    if (A.s2) t = s2 * t;
                    cv[u] = t;
                    if (cj[u] == scan_after && cj[u] >= 0) { k_c = gl + u * G; v_c = t; }
                }
#pragma unroll
                for (int off = G / 2; off > 0; off >>= 1) {
                    const int ok = __shfl_xor(k_c, off, G);
                    const double ov = __shfl_xor(v_c, off, G);
                    if (ok > k_c) { k_c = ok; v_c = ov; }
                }
#pragma unroll
                for (int u = 0; u < kDaRegs; ++u) {  // (a lane's positions ascend with u: strict < keeps the earlier one)
                    const int k = gl + u * G;
                    const double a = cv[u];
                    if (hp[u] < rs) continue;                                         // not a candidate, or held by a lower row
                    if (k_c >= 0 && !(a > v_c || (a == v_c && k > k_c))) continue;    // at or before `scan_after`: refused already
                    if (a < best) { best = a; bk = k; bj = cj[u]; bh = hp[u]; }
                }
            } else {  // rows beyond G * kDaRegs entries: the same in two sweeps over the row
                const int sweeps = (len_max + G - 1) / G;
                for (int u = 0; u < sweeps; ++u) {
                    const int k = gl + u * G;
                    const int64_t pos = base + (int64_t)(k < len ? k : 0) * stride;
                    const int c = colp[pos];
                    double t = valp[pos];
                    if (A.s1) t = s1 * t;
                    if (A.s2) t = s2 * t;
                    if (k < len && c == scan_after) { k_c = k; v_c = t; }
                }
#pragma unroll
                for (int off = G / 2; off > 0; off >>= 1) {
                    const int ok = __shfl_xor(k_c, off, G);
                    const double ov = __shfl_xor(v_c, off, G);
                    if (ok > k_c) { k_c = ok; v_c = ov; }
                }
                for (int u = 0; u < sweeps; ++u) {
                    const int k = gl + u * G;
                    const int64_t pos = base + (int64_t)(k < len ? k : 0) * stride;
                    const int c = colp[pos];
                    double t = valp[pos];
                    if (A.s1) t = s1 * t;
                    if (A.s2) t = s2 * t;
                    const bool ok = k < len && c != rs && c < n;
                    const int hh = da_peek(holder, ok ? c : 0);
                    if (!ok || hh < rs) continue;
                    if (k_c >= 0 && !(t > v_c || (t == v_c && k > k_c))) continue;
                    if (t < best) { best = t; bk = k; bj = c; bh = hh; }
                }
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, G);
                const int ok = __shfl_xor(bk, off, G);
                const int oj = __shfl_xor(bj, off, G);
                const int oh = __shfl_xor(bh, off, G);
                if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; bj = oj; bh = oh; }
            }
            if (need_scan) { cand = bj; seen = bh; ++scans; }
        }
        // ---- 3. the proposal; beside it the list of the row it will most likely displace
        const bool propose = have && cand >= 0;
        int old = 0;
        if (gl == 0 && propose) old = atomicMin(&holder[cand], r);
        const int guess = (propose && seen != 0x7fffffff && seen > r) ? seen : r;
        const int4 pl_guess = pl4[guess];
        old = __shfl(old, 0, G);
        bool done = have && !propose;  // the row has no candidate left: unmatched, the chain ends
        if (propose) {
            ++steps;
            ++chain_steps;
            after = cand;
            if (old > r) {
                if (old == 0x7fffffff) done = true;  // a free column: the chain ends
                else {
                    r = old;                         // accepted; `old` is displaced and goes on from the column it lost
                    pl = old == guess ? pl_guess : pl4[old];
                }
            }
            if (!done && chain_steps >= max_steps) { cut = true; done = true; }
        }
        // ---- the next listed row, in the same pass
        if (done) {
            longest = max(longest, chain_steps);
            e += groups;
            have = e < count;
            chain_steps = 0;
            if (have) {
                const int2 it = list[e];
                r = it.x; after = it.y;
                pl = pl4[r];
            }
        }
    }
    if (gl == 0) {
        if (cut) atomicAdd(&C->overflow, 1);
        if (steps) atomicAdd(&C->steps, steps);
        if (scans) atomicAdd(&C->scans, scans);
        if (longest) atomicMax(&C->longest, longest);
    }
}

// holder -> the pairing: chooser[j] = the row that holds column j (-1: nobody), choice[that row] = j (choice preset to -1)
__global__ void da_finish_k(const int *__restrict__ holder, int *__restrict__ choice, int *__restrict__ chooser, int64_t n) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int h = holder[j];
        chooser[j] = h == 0x7fffffff ? -1 : h;
        if (h != 0x7fffffff) choice[h] = (int)j;  // a row holds one column at most
    }
}

SiblingPairing::~SiblingPairing() {
    for (auto &e : ready)
        if (e) (void)hipEventDestroy(e);
    for (auto &o : offer)
        if (o.view_ready) (void)hipEventDestroy(o.view_ready);
    if (ops_ready) (void)hipEventDestroy(ops_ready);
}
void SiblingPairing::begin(bool leader_will_run) {
    std::lock_guard<std::mutex> lk(mu);
    for (auto &p : published) p = false;
    leader_done = !leader_will_run;
    expected_offers = 0;
    for (auto &o : offer) { o.made = o.ok = o.answered = o.adopted = false; o.view = nullptr; o.arena = o.rows_arena = nullptr; o.level = nullptr; }
    lead_choice = lead_chooser = nullptr;
}
int SiblingPairing::publish(int level, const int *choice, int64_t rows, hipStream_t stream) {
    if (level < 0 || level >= kLevels) return ORC_OK;
    int st = ORC_OK;
    if (buf[level].n < (size_t)std::max<int64_t>(rows, 1)) st = buf[level].alloc((size_t)std::max<int64_t>(rows, 1));
    if (st == ORC_OK && !ready[level] && hipEventCreateWithFlags(&ready[level], hipEventDisableTiming) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventCreate failed");
    if (st == ORC_OK && rows > 0 && hipMemcpyAsync(buf[level].p, choice, sizeof(int) * (size_t)rows, hipMemcpyDeviceToDevice, stream) != hipSuccess)
        st = set_error(ORC_ERR_HIP, "hipMemcpyAsync failed");
    if (st == ORC_OK && hipEventRecord(ready[level], stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    {
        std::lock_guard<std::mutex> lk(mu);
        if (st == ORC_OK) { n[level] = rows; published[level] = true; }
        else leader_done = true;  // nobody waits for a level that will not come
    }
    cv.notify_all();
    return st;
}
const int *SiblingPairing::wait(int level, int64_t rows, hipStream_t stream) {
    if (level < 0 || level >= kLevels) return nullptr;
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return published[level] || leader_done; });
    if (!published[level] || n[level] != rows) return nullptr;
    if (hipStreamWaitEvent(stream, ready[level], 0) != hipSuccess) return nullptr;
    return buf[level].p;
}
void SiblingPairing::finish() {
    {
        std::lock_guard<std::mutex> lk(mu);
        leader_done = true;
    }
    cv.notify_all();
}
void SiblingPairing::set_expected(int n) {
    std::lock_guard<std::mutex> lk(mu);
    expected_offers = n;
}
int SiblingPairing::make_offer(int slot, const MatView *view, Arena *arena, Arena *rows_arena, AmgHierarchy::Level *level, hipStream_t stream) {
    if (slot < 0 || slot > 1) return ORC_OK;
    int st = ORC_OK;
    Offer &o = offer[slot];
    if (!o.view_ready && hipEventCreateWithFlags(&o.view_ready, hipEventDisableTiming) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventCreate failed");
    if (st == ORC_OK && hipEventRecord(o.view_ready, stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    {
        std::lock_guard<std::mutex> lk(mu);
        o.made = true;
        o.ok = st == ORC_OK;
        o.view = view; o.arena = arena; o.rows_arena = rows_arena; o.level = level;
    }
    cv.notify_all();
    return st;
}
void SiblingPairing::withdraw(int slot) {
    if (slot < 0 || slot > 1) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        offer[slot].made = true;
        offer[slot].ok = false;
    }
    cv.notify_all();
}
bool SiblingPairing::wait_answer(int slot, hipStream_t stream) {
    if (slot < 0 || slot > 1) return false;
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return offer[slot].answered || leader_done; });
    if (!offer[slot].answered || !offer[slot].adopted) return false;
    return hipStreamWaitEvent(stream, ops_ready, 0) == hipSuccess;
}
int SiblingPairing::collect_offers(Offer *out[2]) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return (int)offer[0].made + (int)offer[1].made >= expected_offers; });
    int n = 0;
    for (int q = 0; q < 2; ++q)
        if (offer[q].made && offer[q].ok) out[n++] = &offer[q];
    return n;
}
int SiblingPairing::answer(const bool adopted[2], const int *choice, const int *chooser, hipStream_t stream) {
    int st = ORC_OK;
    if (!ops_ready && hipEventCreateWithFlags(&ops_ready, hipEventDisableTiming) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventCreate failed");
    if (st == ORC_OK && hipEventRecord(ops_ready, stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    {
        std::lock_guard<std::mutex> lk(mu);
        lead_choice = choice; lead_chooser = chooser;
        for (int q = 0; q < 2; ++q) {
            offer[q].answered = true;
            offer[q].adopted = st == ORC_OK && adopted[q];
        }
    }
    cv.notify_all();
    return st;
}

// orc_debug_amg_certification: aggregations whose pairing was certified, and how many certifying passes / sweeps that took in total (equal =
// every certification found nothing to change: the deferred-acceptance chains had reached the fixed point by themselves)
static std::atomic<long long> g_cert_aggregations{0}, g_cert_rounds{0};
void debug_amg_certification(long long out[2], bool reset) {
    out[0] = g_cert_aggregations.load(std::memory_order_relaxed);
    out[1] = g_cert_rounds.load(std::memory_order_relaxed);
    if (reset) { g_cert_aggregations.store(0); g_cert_rounds.store(0); }
}
// orc_debug_amg_setup_stats: what the newest aggregate() and the galerkin() behind it did, from the counters both already copy to the host (no
// device read, no synchronisation of its own): [0..4] DaCounters list, steps, scans, longest, overflow; [5] agg_verify_k's `changed` after the
// chains; [6] sweeps of the fallback (0: it did not run); [7] lanes per chain (0: no chains, ORC_AMG_DA=0); [8..14] coarse rows per LDS tier;
// [15] the largest candidate count of a coarse row.  Not cumulative: aggregate() overwrites [0..7] and clears the rest, galerkin() fills [8..15].
static std::mutex g_setup_stats_mu;
static long long g_setup_stats[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
void note_aggregate_stats(const long long ag[8]) {
    std::lock_guard<std::mutex> lk(g_setup_stats_mu);
    for (int i = 0; i < 16; ++i) g_setup_stats[i] = i < 8 ? ag[i] : 0;
}
void note_galerkin_stats(const int *htier, int max_cand) {
    std::lock_guard<std::mutex> lk(g_setup_stats_mu);
    for (int t = 0; t < 7; ++t) g_setup_stats[8 + t] = htier[t];
    g_setup_stats[15] = max_cand;
}
void debug_amg_setup_stats(long long out[16], bool reset) {
    std::lock_guard<std::mutex> lk(g_setup_stats_mu);
    for (int i = 0; i < 16; ++i) {
        out[i] = g_setup_stats[i];
        if (reset) g_setup_stats[i] = 0;
    }
}

// Every row of every view is evaluated against the exact first-taker table of `choice` itself (rebuilt here: reset + scatter); a state in
// which no row would choose differently is that matrix's sequential greedy pairing.
int pairing_mismatches(const int *choice, int64_t n, const PairingCheckView *views, int n_views, Arena &arena, int changed[2]) {
    if (n < 1 || n_views < 1 || n_views > 2) return set_error(ORC_ERR_BAD_ARGUMENT, "pairing_mismatches: bad arguments");
    hipStream_t st = ctx().stream;
    ArenaScope scope(arena);
    int *taken_by;
    AggCounters *C;
    ORC_TRY(arena.alloc((size_t)n, &taken_by));
    ORC_TRY(arena.alloc((size_t)2, &C));
    ORC_HIP(hipMemsetAsync(C, 0, 2 * sizeof(AggCounters), st));
    const int g = grid_for(n);
    hipLaunchKernelGGL(agg_reset_k, dim3(g), dim3(kBlock), 0, st, taken_by, n);
    hipLaunchKernelGGL(agg_scatter_k, dim3(g), dim3(kBlock), 0, st, choice, taken_by, n);
    for (int q = 0; q < n_views; ++q) {
        if (views[q].ready) ORC_HIP(hipStreamWaitEvent(st, views[q].ready, 0));
        hipLaunchKernelGGL(agg_verify_k, dim3(g), dim3(kBlock), 0, st, *views[q].A, choice, (const int *)taken_by, C + q);
    }
    ORC_HIP(hipGetLastError());
    AggCounters hc[2];
    ORC_HIP(hipMemcpyAsync(hc, C, sizeof(hc), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < n_views; ++q) changed[q] = hc[q].changed;
    return ORC_OK;
}

// build_restriction_matrix's pairing (linear_algebra.rs:30-60) for the matrix behind `A`: choice[i] = the column row i takes (-1: none),
// chooser[j] = the row that took column j (-1: nobody).
//   warm (optional): a sibling system's pairing of THIS iteration — taken if it IS this matrix's fixed point (pairing_mismatches: one pass,
//     nothing to iterate), dropped otherwise (a pairing that is off in a few per cent of the rows is a worse start than none).
//   1. deferred acceptance (da_first_k, da_chase_k): the pairing, read off the holder table, certified by ONE verification pass and ONE host read;
//   2. only if that pass finds a row that would choose differently, or a chain was cut by the step budget (ORC_AMG_DA_STEPS: a test hook) —
//      never seen otherwise —, or with ORC_AMG_DA=0: slice-sequential sweeps against the rebuilt first-taker table until a sweep changes
//      nothing.  Slow (one sweep per slice a chain crosses) and as simple as the reference's loop: a fallback, not a path to tune.
int aggregate(const MatView &A, Arena &arena, int *choice, int *chooser, int *rounds_out, const int *warm) {
    const int64_t n = A.P.n;
    const int g = grid_for(n);
    const int gs = grid_for(A.P.n_slices, 64);  // one thread per slice, 64-thread workgroups spread the slices over the CUs
    int *taken_by, *snap;
    AggCounters *C;
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &taken_by));
    ORC_TRY(arena.alloc((size_t)1, &C));
    ORC_TRY(arena.alloc((size_t)64, &snap));
    hipStream_t st = ctx().stream;
    const bool trace = cfg().amg_trace;
    ORC_HIP(hipMemsetAsync(C, 0, sizeof(AggCounters), st));
    long long ag[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // orc_debug_amg_setup_stats [0..7]
    auto done = [&](int rounds) {  // what the statistics and the caller are told on every way out
        note_aggregate_stats(ag);
        if (rounds_out) *rounds_out = rounds;
    };
    if (n == 0) { done(0); return ORC_OK; }
    auto finish_from_choice = [&]() -> int {
        ORC_HIP(hipMemsetAsync(chooser, 0xff, sizeof(int) * (size_t)n, st));
        hipLaunchKernelGGL(chooser_k, dim3(g), dim3(kBlock), 0, st, (const int *)choice, chooser, n);
        ORC_HIP(hipGetLastError());
        return ORC_OK;
    };
    if (warm) {  // a sibling's pairing: this matrix's too?
        const PairingCheckView self{&A, nullptr};
        int changed[2] = {0, 0};
        ORC_HIP(hipMemcpyAsync(choice, warm, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
        ORC_TRY(pairing_mismatches(choice, n, &self, 1, arena, changed));
        if (trace) fprintf(stderr, "[amg sibling n=%lld] rows that would change: %d\n", (long long)n, changed[0]);
        if (changed[0] == 0) { done(1); return finish_from_choice(); }  // else not this matrix's pairing: from scratch
    }
    if (cfg().amg_da) {
        ArenaScope da_scope(arena);  // the list is dead when the pairing is known
        DaCounters *D;
        int2 *list;
        int *da_prefs;
        ORC_TRY(arena.alloc((size_t)1, &D));
        ORC_TRY(arena.alloc((size_t)n, &list));
        ORC_TRY(arena.alloc((size_t)n * kPrefs, &da_prefs));
        ORC_HIP(hipMemsetAsync(D, 0, sizeof(DaCounters), st));
        hipLaunchKernelGGL(agg_reset_k, dim3(g), dim3(kBlock), 0, st, taken_by, n);  // holder = taken_by: nobody
        hipLaunchKernelGGL(da_first_k, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, A, taken_by, list, D, da_prefs);
        // lanes per chain: the list needs four; a scan reads the row G entries at a time (kDaRegs slots per lane in registers)
        const double da_avg = (double)A.P.padded / (double)n;
        const int da_group = cfg().amg_da_group > 0 ? cfg().amg_da_group : (da_avg <= 24. ? 4 : 8);
        const int da_steps = cfg().amg_da_steps;
        if (da_group == 4) hipLaunchKernelGGL(da_chase_k<4>, dim3(kMaxGrid), dim3(kBlock), 0, st, A, taken_by, (const int2 *)list, D, da_steps, (const int *)da_prefs);
        else if (da_group == 8) hipLaunchKernelGGL(da_chase_k<8>, dim3(kMaxGrid), dim3(kBlock), 0, st, A, taken_by, (const int2 *)list, D, da_steps, (const int *)da_prefs);
        else hipLaunchKernelGGL(da_chase_k<16>, dim3(kMaxGrid), dim3(kBlock), 0, st, A, taken_by, (const int2 *)list, D, da_steps, (const int *)da_prefs);
        ORC_HIP(hipMemsetAsync(choice, 0xff, sizeof(int) * (size_t)n, st));
        hipLaunchKernelGGL(da_finish_k, dim3(g), dim3(kBlock), 0, st, (const int *)taken_by, choice, chooser, n);
        // is it the fixed point?  every row against the exact first-taker table (= holder): the sequential pairing is the only state that passes
        hipLaunchKernelGGL(agg_verify_k, dim3(g), dim3(kBlock), 0, st, A, (const int *)choice, (const int *)taken_by, C);
        ORC_HIP(hipGetLastError());
        AggCounters hc;
        DaCounters hd;
        ORC_HIP(hipMemcpyAsync(&hc, C, sizeof(hc), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipMemcpyAsync(&hd, D, sizeof(hd), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        if (trace) fprintf(stderr, "[amg da n=%lld] rows left to the chains %d, their proposals %d (%d by a scan of the row), longest chain %d, chains cut %d, rows that would change %d\n",
                           (long long)n, hd.list, hd.steps, hd.scans, hd.longest, hd.overflow, hc.changed);
        ag[0] = hd.list; ag[1] = hd.steps; ag[2] = hd.scans; ag[3] = hd.longest; ag[4] = hd.overflow; ag[5] = hc.changed; ag[7] = da_group == 4 || da_group == 8 ? da_group : 16;
        if (hd.overflow == 0 && hc.changed == 0) {
            g_cert_aggregations.fetch_add(1, std::memory_order_relaxed);  // certified by one pass that changed nothing
            g_cert_rounds.fetch_add(1, std::memory_order_relaxed);
            done(1);
            return ORC_OK;
        }
        ORC_HIP(hipMemsetAsync(C, 0, sizeof(AggCounters), st));
    }
    // ---- the fallback: sweeps from the unconstrained arg-min state, four per host read
    hipLaunchKernelGGL(agg_init_k, dim3(g), dim3(kBlock), 0, st, A, choice);
    constexpr int kBulk = 4;
    int rounds = 0;
    for (bool done = false; !done;) {
        for (int b = 0; b < kBulk; ++b) {
            hipLaunchKernelGGL(agg_reset_k, dim3(g), dim3(kBlock), 0, st, taken_by, n);
            hipLaunchKernelGGL(agg_scatter_k, dim3(g), dim3(kBlock), 0, st, choice, taken_by, n);
            hipLaunchKernelGGL(agg_sweep_k, dim3(gs), dim3(64), 0, st, A, choice, taken_by, C);
            hipLaunchKernelGGL(agg_rotate_k, dim3(1), dim3(1), 0, st, C, snap + b);
        }
        ORC_HIP(hipGetLastError());
        int h[kBulk];
        ORC_HIP(hipMemcpyAsync(h, snap, sizeof(int) * kBulk, hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        for (int b = 0; b < kBulk; ++b) {
            ++rounds;
            if (h[b] == 0) { done = true; break; }  // a sweep that changed nothing has evaluated every row against the exact table
        }
        if (rounds > 8 * 1000 * 1000) return set_error(ORC_ERR_BAD_ARGUMENT, "aggregation did not reach its fixed point");
    }
    if (trace) fprintf(stderr, "[amg fallback n=%lld] %d sweeps\n", (long long)n, rounds);
    g_cert_aggregations.fetch_add(1, std::memory_order_relaxed);
    g_cert_rounds.fetch_add(rounds, std::memory_order_relaxed);
    ag[6] = rounds;
    done(rounds);
    return finish_from_choice();
}

}  // namespace orc
