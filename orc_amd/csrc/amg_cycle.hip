// amg_cycle.hip — the Multigrid arm (linear_algebra.rs:66-141 multigrid_solve, :270-296 the arm of iterative_solve) on built levels.
//   restrict[3]_k, prolong[3]_k, vec_add3_k   r' = R r, x += R^T e for one system and for three interleaved ones; count_diff_k, nan_to_status[3]_k
//   multigrid_solve_dev        one level of the V-recursion: pairing and operator (from a prepared hierarchy, or built here by
//                              aggregate() / galerkin()), a fixed-count smoothing solve before and after the recursion, which re-solves the
//                              restricted right-hand side r' 
//   multigrid_prepare_dev      the set-up on its own: levels 1..3 for a matrix, the u / v / w threads sharing pairing and product
//   multigrid_coarse_part_dev, multigrid_arm_dev, multigrid_arm3_dev   the arm from level 1 on, for one system, for u, v, w in lock-step
#include <algorithm>
#include <thread>

#include "amg.hpp"

namespace orc {

// r' = R r (:82)
__global__ void restrict_k(const int *__restrict__ choice, int64_t n_fine, int64_t n_coarse, const double *__restrict__ r, double *__restrict__ rc) {
    for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < n_coarse; I += (int64_t)gridDim.x * blockDim.x) {
        const RRow R = restriction_row(choice, I, n_fine);
        double acc = 0.;
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (a < R.n) acc += R.w[a] * r[R.idx[a]];
        rc[I] = acc;
    }
}

// out = R^T e (:140); when `add_to` is set: add_to += R^T e (x += multigrid_solve(...), :284)
__global__ void prolong_k(const int *__restrict__ choice, const int *__restrict__ chooser, int64_t n_fine, const double *__restrict__ e,
                          double *__restrict__ out, double *__restrict__ add_to) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_fine; j += (int64_t)gridDim.x * blockDim.x) {
        int J[2];
        double W[2];
        const int n = rt_row(choice, chooser, (int)j, J, W);
        double acc = 0.;
        for (int a = 0; a < n; ++a) acc += W[a] * e[J[a]];
        if (out) out[j] = acc;
        if (add_to) add_to[j] += acc;
    }
}

// ---- the same for three systems that share a pairing (interleaved vectors, linalg.hpp MatView3): one row of R / R^T per thread,
// applied to the three systems in the one-system order of additions
__global__ void restrict3_k(const int *__restrict__ choice, int64_t n_fine, int64_t n_coarse, const double *__restrict__ r3, double *__restrict__ rc3) {
    for (int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; I < n_coarse; I += (int64_t)gridDim.x * blockDim.x) {
        const RRow R = restriction_row(choice, I, n_fine);
        double a0 = 0., a1 = 0., a2 = 0.;
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (a < R.n) {
                const int64_t e = 3 * (int64_t)R.idx[a];
                a0 += R.w[a] * r3[e];
                a1 += R.w[a] * r3[e + 1];
                a2 += R.w[a] * r3[e + 2];
            }
        rc3[3 * I] = a0; rc3[3 * I + 1] = a1; rc3[3 * I + 2] = a2;
    }
}
// add_to3 += R^T e3
__global__ void prolong3_k(const int *__restrict__ choice, const int *__restrict__ chooser, int64_t n_fine, const double *__restrict__ e3,
                           double *__restrict__ add_to3) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_fine; j += (int64_t)gridDim.x * blockDim.x) {
        int J[2];
        double W[2];
        const int n = rt_row(choice, chooser, (int)j, J, W);
        double a0 = 0., a1 = 0., a2 = 0.;
        for (int a = 0; a < n; ++a) {
            const int64_t e = 3 * (int64_t)J[a];
            a0 += W[a] * e3[e];
            a1 += W[a] * e3[e + 1];
            a2 += W[a] * e3[e + 2];
        }
        add_to3[3 * j] += a0; add_to3[3 * j + 1] += a1; add_to3[3 * j + 2] += a2;
    }
}
// x3[3 i + s] += y_s[i]  (the corrections of the coarser levels, one contiguous vector per system)
__global__ void vec_add3_k(double *__restrict__ x3, const double *__restrict__ y0, const double *__restrict__ y1, const double *__restrict__ y2, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        x3[3 * i] += y0[i]; x3[3 * i + 1] += y1[i]; x3[3 * i + 2] += y2[i];
    }
}
// counts the entries in which two int arrays differ (pairings / row lengths of sibling systems)
__global__ void count_diff_k(const int *__restrict__ a, const int *__restrict__ b, int64_t n, int *__restrict__ counter) {
    int d = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d += a[i] != b[i];
    if (d) atomicAdd(counter, d);
}
__global__ void nan_to_status3_k(const double *__restrict__ value3, int *status3, int code) {
    if (blockIdx.x == 0 && threadIdx.x < 3 && isnan(value3[threadIdx.x])) atomicCAS(status3 + threadIdx.x, 0, code);
}

__global__ void nan_to_status_k(const double *__restrict__ value, int *status, int code) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && isnan(value[0])) atomicCAS(status, 0, code);
}

struct MgParams {
    uint64_t max_levels, iters;
    int smoother, preconditioner;
    double relaxation, threshold;
};

// Runs the enclosed calls on the solve-side stream (see SolveSide) by making it the context's current stream.
struct StreamSwitch {
    hipStream_t saved;
    bool on;
    StreamSwitch(SolveSide *side) : saved(ctx().stream), on(side != nullptr) { if (on) ctx().stream = side->stream; }
    ~StreamSwitch() { if (on) ctx().stream = saved; }
};
// B waits for what A has queued so far / A waits for what B has queued so far
static int side_wait_setup(SolveSide *side, hipStream_t setup_stream) {
    if (!side) return ORC_OK;
    ORC_HIP(hipEventRecord(side->ev_setup, setup_stream));
    ORC_HIP(hipStreamWaitEvent(side->stream, side->ev_setup, 0));
    return ORC_OK;
}
static int setup_wait_side(SolveSide *side, hipStream_t setup_stream) {
    if (!side) return ORC_OK;
    ORC_HIP(hipEventRecord(side->ev_solve, side->stream));
    ORC_HIP(hipStreamWaitEvent(setup_stream, side->ev_solve, 0));
    return ORC_OK;
}

// Leaves a level of the Multigrid arm on every exit path: what the side stream still reads (pairing, coarse matrix,
// vectors) must outlive it, so the set-up stream first waits for the side stream, then both arenas unwind.
struct SideScope {
    SolveSide *side;
    hipStream_t setup_stream;
    Arena &arena, &varena;
    Arena::Mark mk, vmk;
    bool release_varena;
    SideScope(SolveSide *sd, hipStream_t st, Arena &a, Arena &va, bool rel_v)
        : side(sd), setup_stream(st), arena(a), varena(va), mk(a.mark()), vmk(va.mark()), release_varena(rel_v) {}
    ~SideScope() {
        if (side) (void)setup_wait_side(side, setup_stream);
        if (release_varena) varena.release(vmk);
        arena.release(mk);
    }
    SideScope(const SideScope &) = delete;
    SideScope &operator=(const SideScope &) = delete;
};

// linear_algebra.rs:66-141.  `add_to`: the fine vector the prolonged correction is added to.
// With a SolveSide the vector work of a level (restriction, smoothing solves, residual check, prolongation) is queued
// on the side stream in exactly the order below, and the recursion's set-up overlaps this level's smoothing.
static int multigrid_solve_dev(const MatView &A, const double *r, uint64_t level, const MgParams &mp, double threshold, Arena &arena,
                               SolveStats *stats, int *dev_status, double *out, double *add_to, SolveSide *side) {
    const int64_t n = A.P.n;
    hipStream_t st = ctx().stream;
    Arena &varena = side ? *side->arena : arena;  // vectors and solver work space
    SideScope scope(side, st, arena, varena, side != nullptr);  // runs on every return below
    AmgHierarchy::Level L;
    const AmgHierarchy *hier = stats ? stats->hierarchy : nullptr;
    if (hier && (int)level <= hier->n_levels && (level == 1 ? hier->n_fine : hier->level[level - 2].n) == n) {
        // :80, :84 were done ahead of time (multigrid_prepare_dev) for exactly this matrix
        L = hier->level[level - 1];
    } else {
        ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &L.choice));
        ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &L.chooser));
        const int *warm = nullptr;
        SiblingPairing *sib = stats ? stats->sibling : nullptr;
        if (sib && stats->sibling_role == 2 && level == 1) warm = sib->wait((int)level, n, st);  // the fine level only: there the systems share their pattern
        const int agg_st = aggregate(A, arena, L.choice, L.chooser, &L.rounds, warm);  // :80 (scratch is released with the level)
        if (sib && stats->sibling_role == 1 && level == 1) {
            if (agg_st == ORC_OK) ORC_TRY(sib->publish((int)level, L.choice, n, st));
            sib->finish();  // nothing more will be published
        }
        ORC_TRY(agg_st);
        ORC_TRY(galerkin(A, arena, L));  // :84
    }
    const int64_t nc = L.n;
    if (stats && level < 8) {
        stats->amg_levels = std::max(stats->amg_levels, (int)level);
        stats->amg_rows[level] = nc;
        stats->amg_nnz[level] = L.padded;
        stats->amg_rounds[level] = L.rounds;
    }
    ORC_TRY(side_wait_setup(side, st));  // the coarse matrix and the pairing are complete
    const MatView Ac = coarse_view(L, A.symmetric);
    double *r_prime, *e_prime, *partials, *scal;
    const bool shared_scaling = cfg().amg_shared_scaling && mp.smoother == ORC_SOLVER_BICGSTAB && mp.preconditioner == ORC_PRECOND_JACOBI;
    ScaledOperator scaled;
    {
        StreamSwitch sw(side);
        hipStream_t vs = ctx().stream;
        ORC_TRY(varena.alloc((size_t)std::max<int64_t>(nc, 1), &r_prime));
        ORC_TRY(varena.alloc((size_t)std::max<int64_t>(nc, 1), &e_prime));
        ORC_TRY(varena.alloc((size_t)kMaxPartials, &partials));
        ORC_TRY(varena.alloc((size_t)4, &scal));
        double *r_check = nullptr;  // reference-order norm (verification mode): the residual is materialised
        if (ctx().reduction_order == ORC_REDUCTION_REFERENCE) ORC_TRY(varena.alloc((size_t)std::max<int64_t>(nc, 1), &r_check));
        hipLaunchKernelGGL(restrict_k, dim3(grid_for(nc)), dim3(kBlock), 0, vs, L.choice, n, nc, r, r_prime);  // :82
        ORC_HIP(hipGetLastError());
        ORC_TRY(vec_fill(e_prime, 0., nc));  // :86
        // both smoothing solves of this level scale Ac the same way (:159-166): prepared once, held in varena until the level unwinds
        if (shared_scaling) ORC_TRY(jacobi_scaling_prepare_dev(Ac, mp.iters, varena, scaled));
        ORC_TRY(shared_scaling ? bicgstab_scaled_dev(scaled, r_prime, e_prime, varena)
                               : iterative_solve_dev(Ac, r_prime, e_prime, mp.iters, mp.smoother, mp.relaxation, threshold, mp.preconditioner, varena, stats));  // :87-96
        // :97-105  |r' - a' e'| is NaN -> "Multigrid diverged"
        ORC_TRY(residual_norm2_dev(Ac, r_prime, e_prime, partials, scal, r_check));
        hipLaunchKernelGGL(nan_to_status_k, dim3(1), dim3(64), 0, vs, scal, dev_status, (int)ORC_ERR_MULTIGRID_DIVERGED);
    }
    if (level < mp.max_levels && nc > 16) {  // :109
        // :110-121 — the recursion receives r', not the residual; its set-up runs beside the smoothing above
        ORC_TRY(multigrid_solve_dev(Ac, r_prime, level + 1, mp, threshold, arena, stats, dev_status, nullptr, e_prime, side));
        StreamSwitch sw(side);
        ORC_TRY(shared_scaling ? bicgstab_scaled_dev(scaled, r_prime, e_prime, varena)
                               : iterative_solve_dev(Ac, r_prime, e_prime, mp.iters, mp.smoother, mp.relaxation, threshold / 10., mp.preconditioner, varena, stats));  // :123-132
    }
    {
        StreamSwitch sw(side);
        hipLaunchKernelGGL(prolong_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, L.choice, L.chooser, n, e_prime, out, add_to);  // :140
        ORC_HIP(hipGetLastError());
    }
    return ORC_OK;
}

// The leader, through with its fine aggregation, collects the followers' offers and decides which to adopt: the systems on A's pattern
// whose matrices have `choice` as their fixed point too (one verification pass each, one host read) join its Galerkin pass as gs[0 .. *n_sib);
// took[slot] is what the followers are answered.
static int adopt_offers(SiblingPairing &sibling, const MatView &A, const int *choice, Arena &scratch, GalerkinSibling gs[2], bool took[2], int *n_sib) {
    *n_sib = 0;
    SiblingPairing::Offer *offers[2] = {nullptr, nullptr}, *cand[2] = {nullptr, nullptr};
    const int n_off = sibling.collect_offers(offers);
    const int64_t nf = A.P.n;
    PairingCheckView views[2];
    int n_cand = 0;
    for (int q = 0; q < n_off && nf > 0; ++q) {
        const MatView &B = *offers[q]->view;
        if (B.P.n != nf || B.P.col != A.P.col) continue;
        views[n_cand] = PairingCheckView{&B, offers[q]->view_ready};
        cand[n_cand++] = offers[q];
    }
    if (n_cand == 0) return ORC_OK;
    int changed[2] = {0, 0};
    ORC_TRY(pairing_mismatches(choice, nf, views, n_cand, scratch, changed));
    for (int q = 0; q < n_cand; ++q) {
        const int slot = (int)(cand[q] - sibling.offer);
        if (cfg().amg_trace) fprintf(stderr, "[amg sibling n=%lld] offered system %d: rows that would change: %d\n", (long long)nf, slot, changed[q]);
        if (changed[q] != 0) continue;
        gs[(*n_sib)++] = GalerkinSibling{cand[q]->view, cand[q]->arena, cand[q]->rows_arena, cand[q]->level};
        took[slot] = true;
    }
    return ORC_OK;
}

// The set-up half of the Multigrid arm on its own: levels 1..3 of the hierarchy for `A_in` seen through the arm's
// preconditioner (linear_algebra.rs:159-166 then :80, :84 per level, recursion rule of :109).
int multigrid_prepare_dev(const MatView &A_in, int preconditioner, Arena &arena, AmgHierarchy &H, SiblingPairing *sibling, int sibling_role, Arena *scratch) {
    H = AmgHierarchy();
    const int64_t n = A_in.P.n;
    H.n_fine = n;
    // a follower (roles 2, 3) SPEAKS on every path — an offer or a withdrawal — because the leader waits for every follower it expects
    struct SpeakGuard {
        SiblingPairing *s;
        int slot;
        bool spoken = false;
        ~SpeakGuard() { if (s && !spoken) s->withdraw(slot); }
    } speak{(sibling && sibling_role >= 2) ? sibling : nullptr, sibling_role - 2};
    if (n == 0) return ORC_OK;
    if (scratch) {  // nothing of an earlier set-up's mirrors is alive
        scratch->companion().release(Arena::Mark{0, 0});
        ORC_TRY(scratch->companion().reset());
    }
    MatView views[4];
    views[0] = A_in;
    // Level 0 gets a row-contiguous mirror too (its pattern half is the mesh pattern's CSR form, built at mesh creation unless
    // ORC_AMG_L0_MIRROR=0; the values are exported here, one coalesced-read pass): the aggregation and the first Galerkin product walk single
    // rows, and in SELL every entry of a row is a cache line of its own (sell_from_csr_host).
    if (!views[0].rows.col && A_in.P.rows_col && A_in.P.rows_base && A_in.val && A_in.P.csr_row_ptr && A_in.P.nnz > 0 && cfg().amg_l0_mirror) {
        double *rv;
        ORC_TRY(arena.alloc((size_t)A_in.P.nnz, &rv));
        ORC_TRY(sell_rows_values_dev(A_in.P, A_in.val, rv));
        views[0].rows.slice_base = A_in.P.rows_base; views[0].rows.intra_off = A_in.P.rows_intra; views[0].rows.col = A_in.P.rows_col; views[0].rows.val = rv;
    }
    if (preconditioner == ORC_PRECOND_JACOBI) {
        double *dinv;
        ORC_TRY(arena.alloc((size_t)n, &dinv));
        ORC_TRY(diag_inverse_dev(A_in, dinv));
        if (!views[0].s1) views[0].s1 = dinv;
        else if (!views[0].s2) views[0].s2 = dinv;
        else return set_error(ORC_ERR_BAD_ARGUMENT, "more than two nested Jacobi scalings");
    }
    const uint64_t max_levels = 3;  // MULTIGRID_COARSENING_LEVELS, :10
    // One Galerkin pass for the momentum systems that share the fine pairing (SiblingPairing::make_offer ...; ORC_AMG_SHARED_GALERKIN=0:
    // every system multiplies for itself).  Read per call: the tests compare the two forms.
    const bool share_on = cfg().amg_shared_galerkin && scratch != nullptr;
    const bool follows = sibling && sibling_role >= 2, leads = sibling && sibling_role == 1;  // on level 1: there the systems share their pattern
    for (uint64_t level = 1; level <= max_levels; ++level) {
        const MatView &A = views[level - 1];
        const int64_t nf = A.P.n;
        AmgHierarchy::Level L;
        bool adopted = false;
        if (follows && level == 1) {
            const int slot = sibling_role - 2;
            speak.spoken = true;
            if (share_on && sibling->make_offer(slot, &views[0], &arena, scratch ? &scratch->companion() : nullptr, &L, ctx().stream) == ORC_OK)
                adopted = sibling->wait_answer(slot, ctx().stream);
            else
                sibling->withdraw(slot);
        }
        if (adopted) {  // the leader has built this level on ITS pattern with this system's values (L) and vouches for the pairing
            L.choice = const_cast<int *>(sibling->lead_choice);
            L.chooser = const_cast<int *>(sibling->lead_chooser);
            L.rounds = 1;
        } else {
            ORC_TRY(arena.alloc((size_t)std::max<int64_t>(nf, 1), &L.choice));
            ORC_TRY(arena.alloc((size_t)std::max<int64_t>(nf, 1), &L.chooser));
            const int *warm = nullptr;
            if (follows && level == 1) warm = sibling->wait((int)level, nf, ctx().stream);
            // the aggregation's work lists (48 bytes per row) are dead when it returns: they live in `scratch` when there is one
            Arena &agg_arena = scratch ? *scratch : arena;
            const Arena::Mark agg_mark = agg_arena.mark();
            const int agg_st = aggregate(A, agg_arena, L.choice, L.chooser, &L.rounds, warm);
            if (scratch) scratch->release(agg_mark);
            GalerkinSibling gs[2];
            int n_sib = 0;
            bool took[2] = {false, false};
            if (leads && level == 1 && agg_st == ORC_OK) {
                ORC_TRY(sibling->publish((int)level, L.choice, nf, ctx().stream));
                if (share_on) ORC_TRY(adopt_offers(*sibling, A, L.choice, *scratch, gs, took, &n_sib));
            }
            int gal_st = agg_st;
            if (gal_st == ORC_OK) gal_st = galerkin(A, arena, L, scratch, level == max_levels, gs, n_sib);
            if (leads && level == 1) {
                const bool none[2] = {false, false};
                const int ans_st = sibling->answer(gal_st == ORC_OK ? took : none, L.choice, L.chooser, ctx().stream);
                sibling->finish();
                if (gal_st == ORC_OK) gal_st = ans_st;
            }
            ORC_TRY(gal_st);
        }
        AmgHierarchy::Level &h = H.level[level - 1];
        h = L;
        if (h.rows_transient) {  // a mirror in the companion arena lives until the next level is built: the hierarchy does not carry it
            h.rows = RowsDev();
            h.rows_transient = false;
        }
        H.n_levels = (int)level;
        if (!(level < max_levels && L.n > 16)) break;  // :109
        views[level] = coarse_view(L, A.symmetric);
    }
    return ORC_OK;
}

int multigrid_coarse_part_dev(const MatView &A, const double *r, double *x, uint64_t iteration_count, double relaxation_factor,
                              double convergence_threshold, int preconditioner, Arena &arena, SolveStats *stats, int *dev_status) {
    if (A.P.n == 0) return ORC_OK;
    if (!stats || !stats->hierarchy || stats->hierarchy->n_levels < 1 || stats->hierarchy->n_fine != A.P.n)
        return set_error(ORC_ERR_BAD_ARGUMENT, "the coarse part of the Multigrid arm needs a hierarchy prepared for this matrix");
    MgParams mp{3 /* MULTIGRID_COARSENING_LEVELS, :10 */, iteration_count, ORC_SOLVER_BICGSTAB, preconditioner, relaxation_factor, convergence_threshold};
    return multigrid_solve_dev(A, r, 1, mp, convergence_threshold, arena, stats, dev_status, nullptr, x, nullptr);
}

// Multigrid arm of iterative_solve (:270-296); A and b are already the preconditioned system.
int multigrid_arm_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor,
                      double convergence_threshold, int preconditioner, Arena &arena, SolveStats *stats, int smoother) {
    const int64_t n = A.P.n;
    if (n == 0) return ORC_OK;
    hipStream_t st = ctx().stream;
    // two streams only where no host-synchronised smoother (colouring) is involved; on a partitioned operator the
    // level-0 work (halo exchanges, all-reduces) stays on the library stream — every RCCL call keeps its stream — and
    // only the rank-local coarse levels use the side stream
    SolveSide *side = (stats && stats->side && stats->side->stream && smoother == ORC_SOLVER_BICGSTAB && !stats->hierarchy) ? stats->side : nullptr;
    SolveSide *side0 = A.halo ? nullptr : side;
    Arena &varena = side0 ? *side0->arena : arena;
    SideScope scope(side, st, arena, varena, side0 != nullptr);  // runs on every return below
    ORC_TRY(side_wait_setup(side0, st));  // the preconditioned system (scaling vectors, b) was prepared on the set-up stream
    double *r;
    int *dev_status;
    {
        StreamSwitch sw(side0);
        // :273-282 — the smoother is called with the same preconditioner: the scaled system is scaled again (Q4)
        ORC_TRY(iterative_solve_dev(A, b, x, iteration_count, smoother, relaxation_factor, convergence_threshold, preconditioner, varena, stats));
        ORC_TRY(varena.alloc((size_t)n, &r));
        ORC_TRY(varena.alloc((size_t)1, &dev_status));
        ORC_HIP(hipMemsetAsync(dev_status, 0, sizeof(int), ctx().stream));
        ORC_TRY(residual_dev(A, b, x, r));  // :283
    }
    MgParams mp{3 /* MULTIGRID_COARSENING_LEVELS, :10 */, iteration_count, smoother, preconditioner, relaxation_factor, convergence_threshold};
    int stt = multigrid_solve_dev(A, r, 1, mp, convergence_threshold, arena, stats, dev_status, nullptr, x, side);  // :284-295
    if (stt == ORC_OK) {
        ORC_TRY(setup_wait_side(side, st));
        int h = 0;
        ORC_HIP(hipMemcpyAsync(&h, dev_status, sizeof(int), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        stt = h;
    }
    return stt;
}


// ------------------------------------------------------------------ the Multigrid arm for three systems on one pattern
// linear_algebra.rs:270-296 for the u, v and w momentum systems of one SIMPLE iteration at once (MatView3, linalg.hpp).
// Per system the operations and their order are those of multigrid_arm_dev / multigrid_solve_dev, so each system's result
// is bit-identical to its own solve; what changes is who shares a kernel:
//   * level 0 (the mesh pattern) — smoothing solve and residual for the three systems in lock-step (bicgstab3_dev);
//   * level 1 — whenever v's and w's fine-level pairings equal u's (the normal case: SiblingPairing), the three Galerkin
//     operators share their pattern as well and level 1 is solved in lock-step too;
//   * levels 2 and 3 — the level-1 pairings differ in a few rows, so these stay per system, queued on one stream each;
//   * the three hierarchies are built by one host thread each (their rounds synchronise their stream) beside the level-0 solve.
// Anything that does not fit (pairings differ, a level too small) falls back to the per-system coarse part.
int multigrid_arm3_dev(const MatView3 &A3, const double *const b[3], double *const x[3], uint64_t iteration_count, double relaxation_factor,
                       double convergence_threshold, int preconditioner, Arena &arena, TripleLane lanes[3], SiblingPairing *sibling, int status_out[3],
                       const std::function<void()> &on_hierarchies_built) {
    const int64_t n = A3.P.n;
    for (int k = 0; k < 3; ++k) status_out[k] = ORC_OK;
    if (n == 0) return ORC_OK;
    if (!triple_supported()) return set_error(ORC_ERR_BAD_ARGUMENT, "three-system solve: tree reductions only");
    Ctx &g = ctx();
    hipStream_t st = g.stream;
    ArenaScope scope(arena);
    const size_t n3 = (size_t)3 * (size_t)n;
    // [r04] partitioned mesh (A3.halo): level 0 exchanges the interleaved iterate's ghost entries and all-reduces its sums (every RCCL
    // call on the library stream, issued by this thread); the hierarchies and every coarse level are rank-local as in the
    // one-system path (ghost columns are never partners and are dropped from the Galerkin products).  x[k] hold ncols entries.
    const size_t ncols3 = (size_t)3 * (size_t)std::max<int64_t>(A3.P.ncols, n);
    const MgParams mp{3 /* MULTIGRID_COARSENING_LEVELS, :10 */, iteration_count, ORC_SOLVER_BICGSTAB, preconditioner, relaxation_factor, convergence_threshold};

    // ---- hierarchies: one thread per system, from now on (they need the matrices only)
    MatView plain[3];
    for (int k = 0; k < 3; ++k) {
        plain[k].P = A3.P;
        plain[k].val = A3.val[k];
        plain[k].symmetric = lanes[k].symmetric;
        plain[k].persistent_pattern = true;
        plain[k].halo = A3.halo;  // (nothing below exchanges through it: the set-up and the coarse parts are rank-local)
    }
    ORC_HIP(hipStreamSynchronize(st));  // the assembled matrices are complete before other streams read them
    Ctx local[3];
    std::thread th[3];
    int st_prep[3] = {ORC_OK, ORC_OK, ORC_OK};
    bool prepared[3] = {false, false, false};
    if (sibling) sibling->begin(true);
    auto prepare = [&](int k) {
        CtxScope cs(&local[k]);
        if (hipSetDevice(local[k].device) != hipSuccess) { st_prep[k] = set_error(ORC_ERR_HIP, "hipSetDevice failed in a set-up thread"); return; }
        lanes[k].hier_arena->release(Arena::Mark{0, 0});
        int stp = lanes[k].hier_arena->empty() ? lanes[k].hier_arena->reset() : ORC_OK;
        if (stp == ORC_OK && lanes[k].scratch_arena) {
            lanes[k].scratch_arena->release(Arena::Mark{0, 0});
            stp = lanes[k].scratch_arena->reset();  // nothing of the previous set-up is alive: a fragmented reservation becomes one chunk
        }
        // roles: 1 = leader (u), 2 / 3 = followers (slots 0 / 1 of the shared Galerkin pass)
        if (stp == ORC_OK) stp = multigrid_prepare_dev(plain[k], preconditioner, *lanes[k].hier_arena, lanes[k].hierarchy, sibling, k == 0 ? 1 : k + 1, lanes[k].scratch_arena);
        else if (k > 0 && sibling) sibling->withdraw(k - 1);  // the leader waits for every follower it was told to expect
        if (k == 0 && sibling) sibling->finish();  // whatever happened to u: v and w must not wait for a level that will not come
        if (hipStreamSynchronize(local[k].stream) != hipSuccess && stp == ORC_OK) stp = set_error(ORC_ERR_HIP, "stream synchronisation failed in a set-up thread");
        // test hook (tests/mp_worker.py, mode gpu_lane_error): ORC_DEBUG_INJECT_LANE_ERROR="rank:lane" fails that rank's set-up thread
        // locally — the level-0 collectives of every rank still complete and the caller's status agreement tells all of them
        if (!cfg().inject_lane_error.empty()) {
            int r_ = -1, k_ = -1;
            if (sscanf(cfg().inject_lane_error.c_str(), "%d:%d", &r_, &k_) == 2 && r_ == local[k].rank && k_ == k && stp == ORC_OK)
                stp = set_error(ORC_ERR_HIP, "injected lane error (rank %d, lane %d)", r_, k_);
        }
        st_prep[k] = stp;
        prepared[k] = true;
    };
    struct Joiner {  // no exit path may leave a thread running
        std::thread *t;
        ~Joiner() { for (int k = 0; k < 3; ++k) if (t[k].joinable()) t[k].join(); }
    } joiner{th};
    // followers first: the leader is told how many of them will speak (a follower without a thread runs after the join, when the leader
    // is through, and multiplies for itself)
    int n_follower_threads = 0;
    for (int k = 2; k >= 0; --k) {
        local[k] = g;
        local[k].stream = lanes[k].setup_stream;
        local[k].last_error.clear();
        if (k == 0 && sibling) sibling->set_expected(n_follower_threads);
        try { th[k] = std::thread(prepare, k); if (k > 0) ++n_follower_threads; } catch (...) { /* no thread to be had: prepared below, before the join */ }
    }

    auto join_hierarchies = [&] {
        for (int k = 0; k < 3; ++k) {
            if (th[k].joinable()) th[k].join();
            if (!prepared[k]) prepare(k);
        }
        if (on_hierarchies_built) on_hierarchies_built();
    };

    // ---- level 0 in lock-step
    double *b3, *x3, *r3;
    int *dev_status;
    ORC_TRY(arena.alloc(n3, &b3));
    ORC_TRY(arena.alloc(ncols3, &x3));
    ORC_TRY(arena.alloc(n3, &r3));
    ORC_TRY(arena.alloc((size_t)4, &dev_status));
    ORC_HIP(hipMemsetAsync(dev_status, 0, 4 * sizeof(int), st));
    ORC_TRY(interleave3_dev(b[0], b[1], b[2], b3, n));
    ORC_TRY(interleave3_dev(x[0], x[1], x[2], x3, n));
    MatView3 V = A3;
    const double *bp3 = b3;
    if (preconditioner == ORC_PRECOND_JACOBI) {  // iterative_solve's own scaling of the system the arm sees (:159-166)
        double *dinv3, *bt3;
        ORC_TRY(arena.alloc(n3, &dinv3));
        ORC_TRY(arena.alloc(n3, &bt3));
        ORC_TRY(diag_inverse3_dev(A3, dinv3));
        ORC_TRY(scale_vec_dev(dinv3, b3, bt3, (int64_t)n3));
        V.s1 = dinv3;
        bp3 = bt3;
    }
    ORC_TRACE("arm3: level-0 solve");
    ORC_TRY(bicgstab3_dev(V, bp3, x3, iteration_count, preconditioner, arena));  // :273-282 (scaled again inside: Q4)
    ORC_TRY(residual3_dev(V, bp3, x3, r3));                                       // :283
    ORC_TRACE("arm3: level-0 solve queued; joining the hierarchies");

    // ---- the hierarchies
    join_hierarchies();
    for (int k = 0; k < 3; ++k)
        if (st_prep[k] != ORC_OK) { g.last_error = local[k].last_error; return st_prep[k]; }
    const AmgHierarchy *H[3] = {&lanes[0].hierarchy, &lanes[1].hierarchy, &lanes[2].hierarchy};
    bool shared = H[0]->n_levels >= 1 && H[1]->n_levels == H[0]->n_levels && H[2]->n_levels == H[0]->n_levels;
    const int64_t nc = shared ? H[0]->level[0].n : 0;
    if (shared) {
        for (int k = 1; k < 3; ++k) shared = shared && H[k]->level[0].n == nc && H[k]->level[0].padded == H[0]->level[0].padded;
    }
    // [r05] A first coarse level with a packed mirror (ragged rows: config 5) is multiplied by spmv_xwin_k when a system is solved alone — one workgroup per
    // 256-row block, i.e. another thread -> row map and other partial sums than the SELL walk the lock-step kernels share with spmv_uniform_k: in
    // lock-step its dot products would round differently from the one-system solve's.  Such a level is solved per system (the lanes below).
    if (shared && H[0]->level[0].pk.ptr) shared = false;
    if (shared) {  // same pairing and same coarse row lengths => same coarse pattern (the symbolic part of the product depends on nothing else)
        int *diff;
        ORC_TRY(arena.alloc((size_t)1, &diff));
        ORC_HIP(hipMemsetAsync(diff, 0, sizeof(int), st));
        for (int k = 1; k < 3; ++k) {
            hipLaunchKernelGGL(count_diff_k, dim3(grid_for(n)), dim3(kBlock), 0, st, (const int *)H[0]->level[0].choice, (const int *)H[k]->level[0].choice, n, diff);
            hipLaunchKernelGGL(count_diff_k, dim3(grid_for(nc)), dim3(kBlock), 0, st, H[0]->level[0].P.row_len, H[k]->level[0].P.row_len, nc, diff);
        }
        int hd = 0;
        ORC_HIP(hipMemcpyAsync(&hd, diff, sizeof(int), hipMemcpyDeviceToHost, st));
        ORC_HIP(hipStreamSynchronize(st));
        shared = hd == 0;
    }
    const bool trace = cfg().amg_trace;
    if (trace) fprintf(stderr, "[amg triple n=%lld] level 1 %s\n", (long long)n, shared ? "in lock-step" : "per system");
    ORC_TRACE("arm3: hierarchies joined, level 1 %s", shared ? "in lock-step" : "per system");

    hipEvent_t ev_main = nullptr, ev_lane[3] = {nullptr, nullptr, nullptr};
    struct Events {
        hipEvent_t *m, *l;
        ~Events() { if (*m) (void)hipEventDestroy(*m); for (int k = 0; k < 3; ++k) if (l[k]) (void)hipEventDestroy(l[k]); }
    } events{&ev_main, ev_lane};
    ORC_HIP(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming));
    for (int k = 0; k < 3; ++k) ORC_HIP(hipEventCreateWithFlags(&ev_lane[k], hipEventDisableTiming));
    // every lane stream is drained before its arena is unwound, whatever happens below
    struct Drain {
        TripleLane *l;
        ~Drain() { for (int k = 0; k < 3; ++k) { (void)hipStreamSynchronize(l[k].solve_stream); l[k].vec_arena->release(Arena::Mark{0, 0}); } }
    } drain{lanes};
    for (int k = 0; k < 3; ++k) {
        lanes[k].vec_arena->release(Arena::Mark{0, 0});
        if (lanes[k].vec_arena->empty()) ORC_TRY(lanes[k].vec_arena->reset());
        lanes[k].stats = SolveStats();
        lanes[k].stats.hierarchy = &lanes[k].hierarchy;
    }
    // queues `fn` on lane k's solve stream (the calling thread keeps issuing; nothing below synchronises with the host)
    auto on_lane = [&](int k, auto &&fn) {
        hipStream_t saved = g.stream;
        g.stream = lanes[k].solve_stream;
        const int r = fn();
        g.stream = saved;
        return r;
    };

    if (!shared) {
        // per-system coarse parts (multigrid_coarse_part_dev) side by side: r and x per system, contiguous
        double *rk[3];
        for (int k = 0; k < 3; ++k) ORC_TRY(arena.alloc((size_t)n, &rk[k]));
        ORC_TRY(deinterleave3_dev(r3, rk[0], rk[1], rk[2], n));
        ORC_TRY(deinterleave3_dev(x3, x[0], x[1], x[2], n));
        ORC_HIP(hipEventRecord(ev_main, st));
        for (int k = 0; k < 3; ++k) {
            ORC_HIP(hipStreamWaitEvent(lanes[k].solve_stream, ev_main, 0));
            ORC_TRY(on_lane(k, [&] {
                return multigrid_coarse_part_dev(plain[k], rk[k], x[k], iteration_count, relaxation_factor, convergence_threshold, preconditioner,
                                                 *lanes[k].vec_arena, &lanes[k].stats, dev_status + k);
            }));
            ORC_HIP(hipEventRecord(ev_lane[k], lanes[k].solve_stream));
            ORC_HIP(hipStreamWaitEvent(st, ev_lane[k], 0));
        }
    } else {
        // ---- level 1 in lock-step (multigrid_solve_dev, level 1)
        const AmgHierarchy::Level &L0 = H[0]->level[0];
        MatView3 Ac3;
        Ac3.P = L0.P;
        for (int k = 0; k < 3; ++k) Ac3.val[k] = H[k]->level[0].val;
        const size_t nc3 = (size_t)3 * (size_t)nc;
        double *r1, *e1, *partials, *norm3;
        ORC_TRY(arena.alloc(nc3, &r1));
        ORC_TRY(arena.alloc(nc3, &e1));
        ORC_TRY(arena.alloc((size_t)3 * kMaxPartials, &partials));
        ORC_TRY(arena.alloc((size_t)4, &norm3));
        const int dbg_mask = cfg().debug_sync;  // debugging aid: drain the stream after chosen steps
        int step_no = 0;
        auto step = [&](const char *what) { if (dbg_mask & (1 << step_no)) { (void)hipStreamSynchronize(st); ORC_TRACE("arm3 level 1: %s done", what); } ++step_no; };
        const bool dbg_sync = (dbg_mask & 64) != 0;
        step("level 0");
        hipLaunchKernelGGL(restrict3_k, dim3(grid_for(nc)), dim3(kBlock), 0, st, (const int *)L0.choice, n, nc, (const double *)r3, r1);  // :82
        ORC_HIP(hipGetLastError());
        ORC_TRY(vec_fill(e1, 0., (int64_t)nc3));                                                                                      // :86
        step("restriction");
        const bool shared_scaling = cfg().amg_shared_scaling && preconditioner == ORC_PRECOND_JACOBI;  // as in multigrid_solve_dev
        ScaledOperator3 scaled3;
        if (shared_scaling) ORC_TRY(jacobi_scaling_prepare3_dev(Ac3, iteration_count, arena, scaled3));
        ORC_TRY(shared_scaling ? bicgstab3_scaled_dev(scaled3, r1, e1, arena) : bicgstab3_dev(Ac3, r1, e1, iteration_count, preconditioner, arena));  // :87-96
        step("pre-smoothing");
        ORC_TRY(residual_norm2_3_dev(Ac3, r1, e1, partials, norm3));                                                                  // :97-105
        step("residual norm");
        hipLaunchKernelGGL(nan_to_status3_k, dim3(1), dim3(64), 0, st, (const double *)norm3, dev_status, (int)ORC_ERR_MULTIGRID_DIVERGED);
        ORC_HIP(hipGetLastError());
        for (int k = 0; k < 3; ++k) {
            lanes[k].stats.amg_levels = 1;
            lanes[k].stats.amg_rows[1] = nc;
            lanes[k].stats.amg_nnz[1] = H[k]->level[0].padded;
            lanes[k].stats.amg_rounds[1] = H[k]->level[0].rounds;
        }
        if (1 < mp.max_levels && nc > 16) {  // :109
            // :110-121 — levels 2.. per system (their level-1 pairings differ), each on its own stream; the recursion receives r'
            double *rk[3], *ck[3];
            for (int k = 0; k < 3; ++k) {
                ORC_TRY(arena.alloc((size_t)nc, &rk[k]));
                ORC_TRY(arena.alloc((size_t)nc, &ck[k]));
            }
            ORC_TRY(deinterleave3_dev(r1, rk[0], rk[1], rk[2], nc));
            ORC_HIP(hipEventRecord(ev_main, st));
            for (int k = 0; k < 3; ++k) {
                const MatView Ak = coarse_view(H[k]->level[0], plain[k].symmetric);
                ORC_HIP(hipStreamWaitEvent(lanes[k].solve_stream, ev_main, 0));
                ORC_TRY(on_lane(k, [&] {
                    return multigrid_solve_dev(Ak, rk[k], 2, mp, convergence_threshold, *lanes[k].vec_arena, &lanes[k].stats, dev_status + k, ck[k], nullptr, nullptr);
                }));
                ORC_HIP(hipEventRecord(ev_lane[k], lanes[k].solve_stream));
                ORC_HIP(hipStreamWaitEvent(st, ev_lane[k], 0));
            }
            if (dbg_sync) for (int k = 0; k < 3; ++k) { (void)hipStreamSynchronize(lanes[k].solve_stream); ORC_TRACE("arm3 level 1: lane %d levels 2.. done", k); }
            hipLaunchKernelGGL(vec_add3_k, dim3(grid_for(nc)), dim3(kBlock), 0, st, e1, (const double *)ck[0], (const double *)ck[1], (const double *)ck[2], nc);  // e' += ...
            ORC_HIP(hipGetLastError());
            step("corrections added");
            ORC_TRY(shared_scaling ? bicgstab3_scaled_dev(scaled3, r1, e1, arena) : bicgstab3_dev(Ac3, r1, e1, iteration_count, preconditioner, arena));  // :123-132
            step("post-smoothing");
        }
        hipLaunchKernelGGL(prolong3_k, dim3(grid_for(n)), dim3(kBlock), 0, st, (const int *)L0.choice, (const int *)L0.chooser, n, (const double *)e1, x3);  // :140, :284
        ORC_HIP(hipGetLastError());
        ORC_TRY(deinterleave3_dev(x3, x[0], x[1], x[2], n));
    }
    int h[4] = {0, 0, 0, 0};
    ORC_TRACE("arm3: coarse parts queued; waiting for the status words");
    ORC_HIP(hipMemcpyAsync(h, dev_status, sizeof(h), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    ORC_TRACE("arm3: done (%d %d %d)", h[0], h[1], h[2]);
    for (int k = 0; k < 3; ++k) status_out[k] = h[k];
    return ORC_OK;
}

}  // namespace orc
