// simple_iteration.cpp — the host-side schedule of a SIMPLE iteration (solver.rs:60-222): which streams, lanes and host threads
// carry the momentum solves and the p' hierarchy set-up (the decision itself: schedule.hpp), and solver_iterate, which strings the
// assembly wrappers (assembly.hip) and the solves together.  Pure host code: every kernel is launched by what it calls.
#include <algorithm>
#include <cmath>

#include <condition_variable>
#include <mutex>
#include <thread>

#include "assembly.hpp"
#include "schedule.hpp"

namespace orc {

// Streams of the concurrent solves: set-up streams (dependent rounds of tiny kernels, each waited for by the host) and solve streams (the
// bandwidth-bound products) get different priority classes — stream_create (runtime.cpp) decides, and knows when it must not.
// [r04] measurement: ORC_SETUP_CU_MASK (a 32-bit hex pattern repeated over the device's CU mask words) confined the set-up streams to a share
// of the CUs: all settings within +-1 %; removed in r05 with the other measured-and-dropped switches.
static int create_stream(hipStream_t *out, int role, int lane) {
    return stream_create(out, role, lane, role == kSolveStream ? "solve" : "set-up");
}

// a lane's set-up stream; the second stream of a solve (SolveSide, linalg.hpp) with its two events, its temporaries in `arena`: created at first use
static int ensure_lane(SolverState &s, int k) {
    return s.lanes[k].stream ? ORC_OK : create_stream(&s.lanes[k].stream, kSetupStream, k);
}
static int ensure_side(SolveSide &side, int role, int lane, Arena *arena) {
    if (side.stream) return ORC_OK;
    ORC_TRY(create_stream(&side.stream, role, lane));
    ORC_HIP(hipEventCreateWithFlags(&side.ev_setup, hipEventDisableTiming));
    ORC_HIP(hipEventCreateWithFlags(&side.ev_solve, hipEventDisableTiming));
    side.arena = arena;
    return ORC_OK;
}

// the private context of a worker thread that drives `stream` (CtxScope): the caller's, with no error text yet
static Ctx lane_ctx(hipStream_t stream) {
    Ctx c = ctx();
    c.stream = stream;
    c.last_error.clear();
    return c;
}

// The Jacobi scaling ahead of a solve (linear_algebra.rs:159-166, as iterative_solve_dev does it): A gets 1 / diag as its row scaling,
// *b becomes the scaled right-hand side; both vectors live in `arena`.
static int jacobi_scale(Arena &arena, MatView &A, const double **b, int64_t n) {
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    double *dinv, *bt;
    ORC_TRY(arena.alloc(nn, &dinv));
    ORC_TRY(arena.alloc(nn, &bt));
    ORC_TRY(diag_inverse_dev(A, dinv));
    ORC_TRY(scale_vec_dev(dinv, *b, bt, n));
    A.s1 = dinv;
    *b = bt;
    return ORC_OK;
}

static int solve_field_on(SolverState &s, DevBuf<double> &a, DevBuf<double> &b, DevBuf<double> &x, int eq, Arena &arena, SolveStats &stats,
                          SolveSide *side, Arena *side_arena, const AmgHierarchy *prepared = nullptr, const OrcSettings *settings = nullptr) {
    const OrcSettings &t = settings ? *settings : s.settings;  // the scalar arm solves with its own solver fields
    if (arena.empty()) ORC_TRY(arena.reset());  // nothing of the previous solve is alive: a fragmented reservation is folded into one chunk
    if (side_arena && side_arena->empty()) ORC_TRY(side_arena->reset());
    CtxDefaultsScope restore_defaults(ctx());  // this solver's guard, reduction order and GMRES restart for the solve only
    ctx().breakdown_guard = t.breakdown_guard != 0;
    ctx().reduction_order = t.reduction_order;
    ctx().gmres_restart = t.gmres_restart;
    stats.side = nullptr;
    // the momentum systems share their pairing's starting state (the caller has opened the exchange: SiblingPairing::begin)
    stats.sibling = (s.sibling_pairing && eq < 3) ? &s.sibling : nullptr;
    stats.sibling_role = eq == 0 ? 1 : 2;
    stats.hierarchy = prepared ? prepared : ((eq == 3 && s.p_hierarchy.n_levels > 0) ? &s.p_hierarchy : nullptr);
    if (side && s.two_stream_multigrid && t.solver_type == ORC_SOLVER_MULTIGRID) {
        if (!side->stream) {
            // the side stream and the stream of this solve wait for each other's events level by level (side_wait_setup / setup_wait_side): they
            // share a class — "a stream only waits for its own class or a higher one" (runtime.cpp, stream_create)
            const int role = stream_role(ctx().stream) == kSetupStream ? kSetupStream : kSolveStream;
            ORC_TRY(ensure_side(*side, role, eq < 3 ? eq : 1, side_arena));
        }
        stats.side = side;
    }
    return iterative_solve_dev(mesh_view(s, a.p), b.p, x.p, t.iterations, t.solver_type, t.relaxation, t.relative_convergence_threshold,
                               t.preconditioner, arena, &stats);
}

static int solve_field(SolverState &s, DevBuf<double> &a, DevBuf<double> &b, DevBuf<double> &x, int eq) {
    return solve_field_on(s, a, b, x, eq, s.arena, s.stats, &s.side, &s.side_arena);
}

// Runs in a host thread of its own beside the momentum solves: the p' matrix from the fresh momentum diagonals (the
// RHS it also writes is recomputed after the solves), then the Multigrid hierarchy for it.  No rank-to-rank traffic.
static int prepare_p_hierarchy(SolverState &s) {
    hipStream_t st = ctx().stream;
    ORC_TRY(k_pressure_matrix(s));
    ORC_TRY(s.hier_arena.reset());
    // transient set-up storage: its own arena; when the momentum set-ups are through (lock-step schedule: this thread starts
    // after them) lane 0's is free and big enough
    Arena &scratch = s.p_scratch_shared ? s.lanes[0].scratch_arena : s.hier_scratch;
    scratch.release(Arena::Mark{0, 0});
    ORC_TRY(scratch.reset());
    // (a partitioned mesh: level 1 pairs owned rows only; nothing is exchanged)
    ORC_TRY(multigrid_prepare_dev(mesh_view(s, s.a_p.p), s.p_settings().preconditioner, s.hier_arena, s.p_hierarchy, nullptr, 0, &scratch));
    ORC_HIP(hipStreamSynchronize(st));
    s.p_hierarchy_setups += 1;
    return ORC_OK;
}

struct PrepareThread {
    std::thread th;
    Ctx local;
    int status = ORC_OK;
    bool running = false;
    void start(SolverState &s) {
        local = lane_ctx(s.prep_stream);
        auto work = [this, &s] {
            CtxScope scope(&local);
            if (hipSetDevice(local.device) != hipSuccess) { status = set_error(ORC_ERR_HIP, "hipSetDevice failed in the set-up thread"); return; }
            status = prepare_p_hierarchy(s);
        };
        try {
            th = std::thread(work);
            running = true;
        } catch (...) {  // no thread to be had: build the hierarchy right here
            work();
        }
    }
    int join() {
        if (running) {
            th.join();
            running = false;
        }
        if (status != ORC_OK) ctx().last_error = local.last_error;
        return status;
    }
    ~PrepareThread() { if (running) th.join(); }
};

// Partitioned runs (one rank of several): the same overlap with every RCCL call left where it was — on the library
// stream, issued by the calling thread, in an order that is the same on all ranks.  Per momentum system the Multigrid
// arm falls into (1) the Jacobi scaling, the level-0 smoothing solve and the residual, which exchange halos and
// all-reduce scalars, (2) the hierarchy set-up, which needs the matrix only, (3) the V-recursion from level 1 on, and
// (4) the status agreement.  (2) and (3) are rank-local: a lane (thread + streams) per system builds the hierarchy from
// the start and runs (3) as soon as the library stream has finished that system's (1); the calling thread does
// (1) for u, v, w in turn and (4) for u, v, w at the end.  Per system the operations and their order are those of the
// sequential path, so the fields are identical.
static int solve_momentum_partitioned(SolverState &s) {
    Ctx &g = ctx();
    const OrcSettings &t = s.settings;
    OrcMesh &m = *s.mesh;
    const int64_t n = m.n_own;
    DevBuf<double> *mats[3] = {&s.a_u, &s.a_v, &s.a_w}, *rhs[3] = {&s.b_u, &s.b_v, &s.b_w}, *sol[3] = {&s.u, &s.v, &s.w};
    ArenaScope arena_scope(s.arena);  // unwound on every exit (ORC_TRY / ORC_HIP return early)
    MatView plain[3], view[3];
    const double *b_used[3];
    double *r[3];
    int *dev_status;
    ORC_TRY(s.arena.alloc((size_t)4, &dev_status));
    ORC_HIP(hipMemsetAsync(dev_status, 0, 4 * sizeof(int), g.stream));
    for (int k = 0; k < 3; ++k) {
        plain[k] = view[k] = mesh_view(s, mats[k]->p);  // this path only runs on a partitioned mesh: the halo plan is in the view
        b_used[k] = rhs[k]->p;
        ORC_TRY(s.arena.alloc((size_t)std::max<int64_t>(n, 1), &r[k]));
        if (t.preconditioner == ORC_PRECOND_JACOBI) ORC_TRY(jacobi_scale(s.arena, view[k], &b_used[k], n));
        ORC_TRY(ensure_lane(s, k));
        ORC_TRY(ensure_side(s.lanes[k].side, kSolveStream, k, &s.lanes[k].side_arena));
        if (!s.lanes[k].level0_done) ORC_HIP(hipEventCreateWithFlags(&s.lanes[k].level0_done, hipEventDisableTiming));
    }
    ORC_HIP(hipStreamSynchronize(g.stream));  // the assembled systems and the scalings are complete
    g.breakdown_guard = t.breakdown_guard != 0;
    g.reduction_order = ORC_REDUCTION_TREE;  // partitioned operators always reduce as trees + all-reduce

    std::mutex mu;
    std::condition_variable cv;
    bool ready[3] = {false, false, false};
    bool abort_all = false;
    int st_lane[3] = {ORC_OK, ORC_OK, ORC_OK};
    Ctx local[3];
    std::thread th[3];
    for (int k = 0; k < 3; ++k) local[k] = lane_ctx(s.lanes[k].stream);
    auto lane_work = [&](int k) {
        SolverState::Lane &L = s.lanes[k];
        CtxScope scope(&local[k]);
        if (hipSetDevice(local[k].device) != hipSuccess) { st_lane[k] = set_error(ORC_ERR_HIP, "hipSetDevice failed in a solve thread"); return; }
        L.arena.release(Arena::Mark{0, 0});
        L.scratch_arena.release(Arena::Mark{0, 0});
        (void)L.scratch_arena.reset();
        int st = multigrid_prepare_dev(plain[k], t.preconditioner, L.arena, L.hierarchy, nullptr, 0, &L.scratch_arena);  // (2)
        if (st == ORC_OK && hipStreamSynchronize(local[k].stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "stream synchronisation failed in a solve thread");
        // test hook (tests/mp_worker.py, mode gpu_lane_error): ORC_DEBUG_INJECT_LANE_ERROR="rank:lane" makes that rank's lane fail
        // locally after its set-up — every rank must still leave the solve with the same verdict and nobody may hang
        if (!cfg().inject_lane_error.empty()) {
            int r_ = -1, k_ = -1;
            if (sscanf(cfg().inject_lane_error.c_str(), "%d:%d", &r_, &k_) == 2 && r_ == local[k].rank && k_ == k && st == ORC_OK)
                st = set_error(ORC_ERR_HIP, "injected lane error (rank %d, lane %d)", r_, k_);
        }
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return ready[k] || abort_all; });
            if (abort_all) { st_lane[k] = st; return; }
        }
        if (st == ORC_OK) {  // (3) on the lane's solve stream, behind the library stream's level-0 work for this system
            local[k].stream = L.side.stream;
            if (hipStreamWaitEvent(L.side.stream, L.level0_done, 0) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipStreamWaitEvent failed");
            L.stats = SolveStats();
            L.stats.hierarchy = &L.hierarchy;
            L.side_arena.release(Arena::Mark{0, 0});
            if (st == ORC_OK)
                st = multigrid_coarse_part_dev(view[k], r[k], sol[k]->p, t.iterations, t.relaxation, t.relative_convergence_threshold, t.preconditioner,
                                               L.side_arena, &L.stats, dev_status + k);
            if (hipStreamSynchronize(L.side.stream) != hipSuccess && st == ORC_OK) st = set_error(ORC_ERR_HIP, "stream synchronisation failed in a solve thread");
        }
        st_lane[k] = st;
    };
    for (int k = 0; k < 3; ++k) {
        try {
            th[k] = std::thread(lane_work, k);
        } catch (...) {
            // without a thread the lane's work is done further down, after the level-0 section of its system
        }
    }
    // (1) on the library stream, one system after the other
    int st_main = ORC_OK;
    for (int k = 0; k < 3 && st_main == ORC_OK; ++k) {
        s.stats.side = nullptr; s.stats.hierarchy = nullptr;
        st_main = iterative_solve_dev(view[k], b_used[k], sol[k]->p, t.iterations, ORC_SOLVER_BICGSTAB, t.relaxation, t.relative_convergence_threshold,
                                      t.preconditioner, s.arena, &s.stats);  // :273-282 (nested scaling, Q4)
        if (st_main == ORC_OK) st_main = residual_dev(view[k], b_used[k], sol[k]->p, r[k]);  // :283
        if (st_main == ORC_OK && hipEventRecord(s.lanes[k].level0_done, g.stream) != hipSuccess) st_main = set_error(ORC_ERR_HIP, "hipEventRecord failed");
        {
            std::lock_guard<std::mutex> lk(mu);
            if (st_main == ORC_OK) ready[k] = true;
            else abort_all = true;
        }
        cv.notify_all();
        if (st_main == ORC_OK && !th[k].joinable()) lane_work(k);  // no thread was to be had for this lane
    }
    if (st_main != ORC_OK) {
        { std::lock_guard<std::mutex> lk(mu); abort_all = true; }
        cv.notify_all();
    }
    for (int k = 0; k < 3; ++k)
        if (th[k].joinable()) th[k].join();
    // (4) the verdicts, agreed between the ranks in u, v, w order (a rank whose lane failed locally still takes part)
    // iterative_solve_dev has already agreed st_main between the ranks (its own status agreement), so either every rank
    // is here with st_main == ORC_OK or none is; a local HIP failure below still enters the three agreements.
    int result = st_main;
    if (st_main == ORC_OK) {
        int h[4] = {0, 0, 0, 0};
        int copy_st = ORC_OK;
        if (hipMemcpyAsync(h, dev_status, sizeof(h), hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess)
            copy_st = set_error(ORC_ERR_HIP, "fetching the Multigrid status words failed");
        for (int k = 0; k < 3; ++k) {
            int stk = st_lane[k] != ORC_OK ? st_lane[k] : (copy_st != ORC_OK ? copy_st : h[k]);
            if (st_lane[k] != ORC_OK) g.last_error = local[k].last_error;
            stk = comm_global_status(stk);
            if (result == ORC_OK && stk != ORC_OK) result = stk;
        }
    }
    s.stats = s.lanes[0].stats;
    return result;
}

// The three momentum solves of one iteration on three streams, one host thread each (the set-up phases synchronise
// their stream every few rounds).  Returns the first non-zero status in u, v, w order, like the sequential loop.
// setup_first (Multigrid arm): phase 1 builds the three hierarchies side by side (beside the p' hierarchy of `prep`) with
// no product running — the set-up rounds are chains of tiny dependent kernels, and behind other streams' 2048-workgroup
// products every one of them waits for a free wave slot (tail kernels: 0.48 s of kernel time per iteration alone, 1.5 s
// summed when stretched by that contention) — phase 2 runs the three solves on the prepared hierarchies.  Same kernels on
// the same data in the same order per system: same bits.
static int solve_momentum_concurrently(SolverState &s, bool setup_first, PrepareThread *prep) {
    Ctx &g = ctx();
    ORC_HIP(hipStreamSynchronize(g.stream));  // the assembled systems are complete
    DevBuf<double> *mats[3] = {&s.a_u, &s.a_v, &s.a_w}, *rhs[3] = {&s.b_u, &s.b_v, &s.b_w}, *sol[3] = {&s.u, &s.v, &s.w};
    int st[3] = {ORC_OK, ORC_OK, ORC_OK};
    Ctx local[3];
    for (int k = 0; k < 3; ++k) {
        ORC_TRY(ensure_lane(s, k));
        local[k] = lane_ctx(s.lanes[k].stream);
    }
    auto run_lanes = [&](auto &&work) {
        std::thread th[3];
        for (int k = 0; k < 3; ++k) {
            try {
                th[k] = std::thread(work, k);
            } catch (...) {  // no thread to be had: this lane runs here, after the ones already started (nothing crosses the C ABI)
                work(k);
            }
        }
        for (int k = 0; k < 3; ++k)
            if (th[k].joinable()) th[k].join();
    };
    if (setup_first) {
        auto prepare = [&](int k) {
            SolverState::Lane &L = s.lanes[k];
            CtxScope scope(&local[k]);
            if (hipSetDevice(local[k].device) != hipSuccess) { st[k] = set_error(ORC_ERR_HIP, "hipSetDevice failed in a set-up thread"); return; }
            L.arena.release(Arena::Mark{0, 0});
            L.scratch_arena.release(Arena::Mark{0, 0});
            (void)L.scratch_arena.reset();
            st[k] = multigrid_prepare_dev(mesh_view(s, mats[k]->p), s.settings.preconditioner, L.arena, L.hierarchy, nullptr, 0, &L.scratch_arena);
            if (hipStreamSynchronize(local[k].stream) != hipSuccess && st[k] == ORC_OK) st[k] = set_error(ORC_ERR_HIP, "stream synchronisation failed in a set-up thread");
        };
        run_lanes(prepare);
        const int pst = prep ? prep->join() : ORC_OK;  // the p' hierarchy was being built beside them
        for (int k = 0; k < 3; ++k)
            if (st[k] != ORC_OK) { g.last_error = local[k].last_error; return st[k]; }
        if (pst != ORC_OK) return pst;
    }
    auto work = [&](int k) {
        SolverState::Lane &L = s.lanes[k];
        CtxScope scope(&local[k]);
        if (hipSetDevice(local[k].device) != hipSuccess) { st[k] = set_error(ORC_ERR_HIP, "hipSetDevice failed in a solve thread"); return; }
        if (setup_first) {
            L.side_arena.release(Arena::Mark{0, 0});
            st[k] = solve_field_on(s, *mats[k], *rhs[k], *sol[k], k, L.side_arena, L.stats, nullptr, nullptr, &L.hierarchy);
        } else {
            st[k] = solve_field_on(s, *mats[k], *rhs[k], *sol[k], k, L.arena, L.stats, &L.side, &L.side_arena);
        }
        if (k == 0) s.sibling.finish();  // whatever happened to u: v and w must not wait for a level that will not come
        if (hipStreamSynchronize(local[k].stream) != hipSuccess && st[k] == ORC_OK) st[k] = set_error(ORC_ERR_HIP, "stream synchronisation failed in a solve thread");
    };
    s.sibling.begin(!setup_first);  // with the hierarchies prepared ahead nobody aggregates inside the solves
    run_lanes(work);
    s.stats = s.lanes[0].stats;
    for (int k = 0; k < 3; ++k)
        if (st[k] != ORC_OK) {
            g.last_error = local[k].last_error;
            return st[k];
        }
    return ORC_OK;
}

// The three momentum systems in lock-step (linalg.hpp MatView3 / multigrid_arm3_dev, bicgstab3_dev): single GPU, tree
// reductions, Multigrid or BiCGSTAB solver.  Returns the first non-zero status in u, v, w order, like the sequential loop.
static int solve_momentum_triple(SolverState &s, const std::function<void()> &on_hierarchies_built) {
    Ctx &g = ctx();
    const OrcSettings &t = s.settings;
    g.breakdown_guard = t.breakdown_guard != 0;
    g.reduction_order = t.reduction_order;
    MatView3 A3;
    A3.P = s.mesh->pat.dev();
    A3.val[0] = s.a_u.p; A3.val[1] = s.a_v.p; A3.val[2] = s.a_w.p;
    A3.mesh_pattern = true;
    if (s.mesh->halo.active()) {  // [r04] cell-partitioned mesh: one halo exchange and one all-reduce per step for the three systems
        A3.halo = &s.mesh->halo;
        g.reduction_order = ORC_REDUCTION_TREE;  // partitioned operators always reduce as trees + all-reduce
    }
    const double *b[3] = {s.b_u.p, s.b_v.p, s.b_w.p};
    double *x[3] = {s.u.p, s.v.p, s.w.p};
    if (s.arena.empty()) ORC_TRY(s.arena.reset());
    if (t.solver_type == ORC_SOLVER_BICGSTAB_GS_PRECOND) {  // [r04] BASELINE configs[2]: u, v, w per colour in ONE launch (gs_slot.hip, slot space)
        ArenaScope scope(s.arena);
        MatView V[3];
        const double *bb[3];
        for (int k = 0; k < 3; ++k) {
            V[k] = mesh_view(s, A3.val[k]);  // one GPU only (schedule.hpp): no halo plan in the view
            bb[k] = b[k];
            if (t.preconditioner == ORC_PRECOND_JACOBI) ORC_TRY(jacobi_scale(s.arena, V[k], &bb[k], s.n_own));
            else if (t.preconditioner != ORC_PRECOND_NONE) return set_error(ORC_ERR_BAD_ARGUMENT, "unknown preconditioner %d", t.preconditioner);
        }
        ORC_TRY(gs_bicgstab3_dev(V, bb, x, t.iterations, s.arena));
        ORC_HIP(hipStreamSynchronize(g.stream));
        return ORC_OK;
    }
    if (t.solver_type == ORC_SOLVER_BICGSTAB) {
        ArenaScope scope(s.arena);
        const size_t n3 = (size_t)3 * (size_t)s.n_own;
        double *b3, *x3;
        ORC_TRY(s.arena.alloc(n3, &b3));
        ORC_TRY(s.arena.alloc((size_t)3 * (size_t)s.n, &x3));  // with its ghost entries on a partitioned mesh
        ORC_TRY(interleave3_dev(b[0], b[1], b[2], b3, s.n_own));
        ORC_TRY(interleave3_dev(x[0], x[1], x[2], x3, s.n_own));
        ORC_TRY(bicgstab3_dev(A3, b3, x3, t.iterations, t.preconditioner, s.arena));
        ORC_TRY(deinterleave3_dev(x3, x[0], x[1], x[2], s.n_own));
        ORC_HIP(hipStreamSynchronize(g.stream));
        return ORC_OK;
    }
    for (int k = 0; k < 3; ++k) {
        SolverState::Lane &L = s.lanes[k];
        ORC_TRY(ensure_lane(s, k));
        ORC_TRY(ensure_side(L.side, kSolveStream, k, &L.side_arena));
        s.triple[k].setup_stream = L.stream;
        s.triple[k].solve_stream = L.side.stream;
        s.triple[k].hier_arena = &L.arena;
        s.triple[k].vec_arena = &L.side_arena;
        s.triple[k].scratch_arena = &L.scratch_arena;
        s.triple[k].symmetric = s.mesh->pat.symmetric;
    }
    int st3[3] = {ORC_OK, ORC_OK, ORC_OK};
    ORC_TRY(multigrid_arm3_dev(A3, b, x, t.iterations, t.relaxation, t.relative_convergence_threshold, t.preconditioner, s.arena, s.triple,
                               s.sibling_pairing ? &s.sibling : nullptr, st3, on_hierarchies_built));
    s.stats = s.triple[0].stats;
    for (int k = 0; k < 3; ++k)
        if (st3[k] != ORC_OK) return st3[k];
    return ORC_OK;
}

static void debug_field(SolverState &s, const char *name, const DevBuf<double> &f) {
    std::vector<double> h((size_t)s.n);
    (void)f.download(h.data(), (size_t)s.n);
    int nn = 0;
    double mx = 0.;
    for (double x : h) { if (std::isnan(x)) nn++; else mx = std::max(mx, std::fabs(x)); }
    fprintf(stderr, "[orc debug] it %llu %s: nan=%d max=%.17g\n", (unsigned long long)s.iterations_done, name, nn, mx);
}

// One pass of solver.rs:60-222 per iteration.  In a partitioned run (mesh.halo active) the ghost entries of every
// field a face kernel reads are refreshed first (C1); the solves exchange their own work vectors.
int solver_iterate(SolverState &s, uint64_t iterations, double *report) {
    // the solves below run with THIS solver's guard and reduction order; the process-wide defaults (orc_set_breakdown_guard,
    // orc_set_reduction_order: what orc_iterative_solve uses) are put back on every exit
    CtxDefaultsScope restore_defaults(ctx());
    const bool tvd = is_tvd(s.settings.momentum);
    const bool dbg = cfg().debug_nan;
    HaloPlan &H = s.mesh->halo;
    for (uint64_t it = 0; it < iterations; ++it) {
        double peclet[3] = {0., 0., 0.};
        if (s.arena.empty()) ORC_TRY(s.arena.reset());  // between iterations nothing in the solver's own arena is alive
        ORC_TRACE("iteration %llu: start", (unsigned long long)s.iterations_done);
        ORC_TRY(exchange_fields(s));
        if (s.vis.on) ORC_TRY(k_viscosity_update(s));            // variable viscosity: the law on the fresh fields, then a_di and b_*_di
        ORC_TRY(k_gradients(s, tvd));
        ORC_TRY(exchange_gradient(s, s.gp.p));
        ORC_TRY(k_face_flux(s, true));
        ORC_TRY(k_momentum(s, report ? peclet : nullptr));       // :61-82
        if (s.mon.on) ORC_TRY(k_momentum_residuals(s));          // the residuals before the solve: u, v, w are still the fields of the assembly
        if (H.active()) { double *d3[3] = {s.du.p, s.dv.p, s.dw.p}; ORC_TRY(H.exchange(d3, 3)); }
        if (dbg) { debug_field(s, "b_u", s.b_u); debug_field(s, "b_v", s.b_v); debug_field(s, "b_w", s.b_w); }
        const OrcSettings p_set = s.p_settings();   // the pressure correction's: the settings, or orc_solver_set_pressure_solver's override
        const int method_p = p_set.solver_type;
        const bool p_multigrid = method_p == ORC_SOLVER_MULTIGRID || method_p == ORC_SOLVER_MULTIGRID_GS;
        PrepareThread prep;
        s.p_hierarchy.n_levels = 0;
        // the schedule of this iteration — hence the SEQUENCE OF COLLECTIVES of a rank — from this solver's settings and the mesh alone
        // (schedule.hpp; the momentum systems' follows settings.solver_type, the p' hierarchy's p_settings())
        ScheduleInputs in;
        in.concurrent_momentum = s.concurrent_momentum; in.triple_momentum = s.triple_momentum; in.early_p_hierarchy = s.early_p_hierarchy;
        in.two_stream_multigrid = s.two_stream_multigrid; in.sibling_pairing = s.sibling_pairing;
        in.partitioned = H.active(); in.debug_nan = dbg; in.profiling = ctx().profile; in.gs_slot_space = gs_slot_space_enabled();
        in.momentum_solver = s.settings.solver_type; in.p_solver = method_p; in.reduction_order = s.settings.reduction_order;
        const Schedule plan = decide_schedule(in);
        if (plan.p_hierarchy != kPHierarchyInSolve && !s.prep_stream) ORC_TRY(create_stream(&s.prep_stream, kSetupStream, 2));
        s.p_scratch_shared = plan.p_hierarchy == kPHierarchyLate;
        if (plan.p_hierarchy == kPHierarchyEarly) {
            ORC_HIP(hipStreamSynchronize(ctx().stream));  // the diagonals (and their ghosts) are in place
            prep.start(s);
        }
        switch (plan.momentum) {
        case kMomentumLockStep: {
            // :99-136, the three systems in lock-step on their shared pattern (a partitioned mesh reduces as trees whatever the settings
            // say; solve_momentum_triple puts that into the context itself)
            ORC_TRACE("momentum: lock-step solve");
            int st3 = solve_momentum_triple(s, plan.p_hierarchy == kPHierarchyLate ? std::function<void()>([&] { prep.start(s); }) : std::function<void()>());
            ORC_TRACE("momentum: lock-step solve returned %d", st3);
            // partitioned: a rank whose set-up thread or coarse level failed locally has still taken part in every level-0 collective;
            // the verdict must be the same on every rank or they part ways at the next one
            if (H.active()) st3 = comm_global_status(st3);
            ORC_TRY(st3);
            break;
        }
        case kMomentumLanes:
            ORC_TRY(solve_momentum_concurrently(s, false, prep.running ? &prep : nullptr));  // :99-136, the three systems side by side
            break;
        case kMomentumLanesPartitioned:
            ORC_TRY(solve_momentum_partitioned(s));                     // the same with every RCCL call on the library stream
            break;
        case kMomentumSequential:
            s.sibling.begin(true);
            const int st_u = solve_field(s, s.a_u, s.b_u, s.u, 0);      // :99-110
            s.sibling.finish();
            ORC_TRY(st_u);
            if (dbg) debug_field(s, "u", s.u);
            ORC_TRY(solve_field(s, s.a_v, s.b_v, s.v, 1));              // :112-123
            if (dbg) debug_field(s, "v", s.v);
            ORC_TRY(solve_field(s, s.a_w, s.b_w, s.w, 2));              // :125-136
            if (dbg) debug_field(s, "w", s.w);
            break;
        }
        ORC_TRACE("momentum done; joining the p' set-up");
        ORC_TRY(prep.join());
        ORC_TRACE("p' set-up joined");
        if (H.active()) { double *f[3] = {s.u.p, s.v.p, s.w.p}; ORC_TRY(H.exchange(f, 3)); }
        ORC_TRY(k_pressure_correction(s));                       // :137-148 (the matrix comes out as in the early pass)
        if (s.mon.on) ORC_TRY(k_imbalance(s));                   // b_p: the mass imbalance of the fresh momentum solution
        ORC_TRY(vec_fill(s.p_prime.p, 0., s.n));                 // :167
        if (dbg) debug_field(s, "b_p", s.b_p);
        ORC_TRACE("p' solve");
        if (p_multigrid && s.p_hierarchy.n_levels == 0) s.p_hierarchy_setups += 1;  // no prepared hierarchy: the arm sets one up inside the solve
        ORC_TRY(solve_field_on(s, s.a_p, s.b_p, s.p_prime, 3, s.arena, s.stats, &s.side, &s.side_arena, nullptr,
                               s.p_solver_on ? &p_set : nullptr));  // :168-179
        ORC_TRACE("p' solve done");
        if (dbg) debug_field(s, "p_prime", s.p_prime);
        if (H.active()) ORC_TRY(H.exchange(s.p_prime.p));
        double sums[5];
        ORC_TRY(k_apply_correction(s, sums));                    // :193-208
        s.iterations_done++;
        const double ng = (double)s.mesh->n_global;
        const double u_avg = sums[2] / ng, v_avg = sums[3] / ng, w_avg = sums[4] / ng;
        if (report) {
            double *r = report + 8 * it;
            r[0] = u_avg; r[1] = v_avg; r[2] = w_avg; r[3] = peclet[0]; r[4] = peclet[1]; r[5] = peclet[2];
            r[6] = std::sqrt(sums[1]); r[7] = std::sqrt(sums[0]);
        }
        int st = 0;
        if (s.mon.on) ORC_TRY(monitor_fetch(s));  // behind every collective of the iteration; its copy is complete at the synchronisation below
        ORC_HIP(hipMemcpyAsync(&st, s.dev_status.p, sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
        ORC_HIP(hipStreamSynchronize(ctx().stream));
        if (s.mon.on) monitor_append(s);
        if (H.active()) st = comm_global_status(st);
        if (st) return st;
        if (std::isnan(u_avg) || std::isnan(v_avg) || std::isnan(w_avg)) return ORC_ERR_SOLUTION_DIVERGED;  // :217-221
    }
    return ORC_OK;
}

int solve_scalar_system(SolverState &s, const OrcSettings &t) {
    return solve_field_on(s, s.sc.a, s.sc.b, s.sc.phi, 4, s.arena, s.stats, &s.side, &s.side_arena, nullptr, &t);
}

}  // namespace orc
