// amg.hpp — what the amg_*.hip files share, and nothing the rest of the library calls (that is declared in arms.hpp / linalg.hpp).
// The Multigrid arm (linear_algebra.rs:12-141, :270-296) is cut by concern:
//   amg_pairing.hip   build_restriction_matrix's pairing: deferred acceptance, its certification, the sweeps behind it; SiblingPairing
//   amg_galerkin.hip  the coarse operator (R A) R^T: bounds and LDS tiers, the merge, the pack into SELL image and packed mirror
//   amg_mirror.hip    what a built level's products stream besides: narrow column image, LDS x windows
//   amg_cycle.hip     transfer kernels, multigrid_solve's recursion, the set-up on its own, the arms for one and for three systems
//   amg_hooks.hip     one level of the set-up made observable (orc_amg_coarsen, orc_debug_amg_*)
// The library is built without relocatable device code: a __device__ function that kernels of two files call lives here; a __device__
// variable stays in the one file whose kernels touch it.
#pragma once
#include "linalg_kernels.hpp"

namespace orc {

// Row I of R (linear_algebra.rs:53-58 after COO->CSR): up to 4 (fine index, weight) pairs, ascending, duplicates summed.
struct RRow {
    int idx[4];
    double w[4];
    int n;
};
// Every array index below is a compile-time constant (fixed sorting network, unrolled merges), so the row lives in
// registers; a dynamically indexed idx[]/w[] would be spilled to scratch memory.
// (pair0, pair1 = choice[2I], choice[2I + 1], -1 where the fine row does not exist: loaded by the caller, ahead of time)
__device__ __forceinline__ RRow restriction_row_from(int64_t I, int pair0, int pair1) {
    constexpr int kNone = 0x7fffffff;
    int v[4] = {kNone, kNone, kNone, kNone};
    if (pair0 >= 0) { v[0] = (int)(2 * I); v[1] = pair0; }
    if (pair1 >= 0) { v[2] = (int)(2 * I + 1); v[3] = pair1; }
    // sorting network for 4 keys (absent entries sort last)
#define ORC_CSWAP(x, y) { const int lo__ = min(v[x], v[y]), hi__ = max(v[x], v[y]); v[x] = lo__; v[y] = hi__; }
    ORC_CSWAP(0, 1) ORC_CSWAP(2, 3) ORC_CSWAP(0, 2) ORC_CSWAP(1, 3) ORC_CSWAP(1, 2)
#undef ORC_CSWAP
    // merge equal indices: out[m-1] absorbs a repeat (weights 1 -> 2; a fine row can appear at most twice)
    RRow r;
    r.n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { r.idx[q] = 0; r.w[q] = 0.; }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const bool present = v[a] != kNone;
        const bool repeat = present && a > 0 && v[a] == v[a > 0 ? a - 1 : 0];
        if (present && !repeat) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == r.n) { r.idx[q] = v[a]; r.w[q] = 1.; }
            r.n++;
        } else if (repeat) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == r.n - 1) r.w[q] += 1.;
        }
    }
    return r;
}
__device__ __forceinline__ RRow restriction_row(const int *__restrict__ choice, int64_t I, int64_t n_fine) {
    const int pair0 = 2 * I < n_fine ? choice[2 * I] : -1;
    const int pair1 = 2 * I + 1 < n_fine ? choice[2 * I + 1] : -1;
    return restriction_row_from(I, pair0, pair1);
}

// Row j of R^T: (coarse index, weight) pairs, ascending
__device__ __forceinline__ int rt_row(const int *__restrict__ choice, const int *__restrict__ chooser, int j, int J[2], double W[2]) {
    const int own = choice[j] >= 0 ? (j >> 1) : -1;
    const int oth = chooser[j] >= 0 ? (chooser[j] >> 1) : -1;
    int n = 0;
    if (own >= 0 && oth >= 0) {
        if (own == oth) { J[0] = own; W[0] = 2.; n = 1; }
        else if (own < oth) { J[0] = own; W[0] = 1.; J[1] = oth; W[1] = 1.; n = 2; }
        else { J[0] = oth; W[0] = 1.; J[1] = own; W[1] = 1.; n = 2; }
    } else if (own >= 0) { J[0] = own; W[0] = 1.; n = 1; }
    else if (oth >= 0) { J[0] = oth; W[0] = 1.; n = 1; }
    return n;
}

// ------------------------------------------------------------------ host functions that cross between the files
// amg_pairing.hip.  build_restriction_matrix's pairing for the matrix behind `A`: choice[i] = the column row i takes (-1: none),
// chooser[j] = the row that took column j (-1: nobody); `warm` (optional): a sibling system's pairing, taken if it is this matrix's too.
int aggregate(const MatView &A, Arena &arena, int *choice, int *chooser, int *rounds_out, const int *warm = nullptr);
// Is `choice` (n >= 1 rows) the pairing of these matrices — up to two views on ONE pattern?  changed[q] = rows of view q that would choose
// differently (0: it is that matrix's fixed point, which is unique).  `ready` (optional): an event the view's data waits for.  One host read.
struct PairingCheckView {
    const MatView *A = nullptr;
    hipEvent_t ready = nullptr;
};
int pairing_mismatches(const int *choice, int64_t n, const PairingCheckView *views, int n_views, Arena &arena, int changed[2]);
// orc_debug_amg_setup_stats: [0..7] from aggregate() (which clears the rest), [8..15] from the galerkin() behind it
void note_aggregate_stats(const long long ag[8]);
void note_galerkin_stats(const int *htier, int max_cand);

// amg_galerkin.hip.  A sibling system on A's pattern that verified the leader's pairing as its own (SiblingPairing): its coarse operator
// shares the pattern the leader's product builds and gets its own values in its own arenas; every kernel runs on the calling thread's stream.
// Inside galerkin() the leader is system 0 of the same kind, and every system carries the values made for it.
struct GalerkinSibling {
    const MatView *A = nullptr;        // same pattern (and mirror structure) as the leader's view, its own values and scalings
    Arena *arena = nullptr;            // the system's hierarchy arena: its coarse values
    Arena *rows_arena = nullptr;       // where its copy of the transient row-contiguous mirror goes (the companion of its scratch arena)
    AmgHierarchy::Level *L = nullptr;  // out: its level
    double *s_val = nullptr, *val = nullptr, *pk_val = nullptr;  // galerkin()'s own: its scratch rows' values; its coarse values: SELL image, packed mirror
};
// L (in: choice, chooser, rounds of the pairing of A's rows) -> the level's operator.
// `scratch` (optional): a second arena for everything that is dead when the level is complete — the symbolic bounds, the tier lists and the
// product's scratch rows, 11 GB of a 10.24 M-row hierarchy's 23 GB — released before returning; the row-contiguous mirror is then a compacted
// copy in scratch's companion (L.rows_transient).  Without it the scratch rows themselves stay alive in `arena` as the mirror.
// `sib` / n_sib (<= 2): needs `scratch`.  last_level: the level is never aggregated, so it gets no row mirror.
int galerkin(const MatView &A, Arena &arena, AmgHierarchy::Level &L, Arena *scratch = nullptr, bool last_level = false, const GalerkinSibling *sib = nullptr, int n_sib = 0);

// amg_mirror.hip: two phases of galerkin().  narrow_image: 2-byte columns for a level the uniform kernels multiply (Pc.col16 / colbase, all
// or nothing; one host read).  build_windows: the LDS x windows of the leader's packed mirror, each system's fold scratch, and the LDS share.
int narrow_image(SellDev &Pc, Arena &arena, Arena &tmp);
int build_windows(const GalerkinSibling *sys, int n_sys, const int64_t *lptr, int64_t pos_slots, Arena &tmp);

}  // namespace orc
