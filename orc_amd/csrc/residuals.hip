// residuals.hip — residual monitors of the SIMPLE iteration (orc_solver_set_monitors; DESIGN.md §3 "Residual monitors"): the norms of
// the three momentum residuals "before the solve" in one fused pass over the assembled systems, the mass imbalance of the fresh
// momentum solution from the right-hand side of the pressure correction, their fold, and the host-side record.  No residual vector
// is stored and nothing the solver reads is written: the passes have partial sums of their own (SolverState::Monitor).
//
// Bandwidth-bound like every level-0 product (spmv.hip): the pass streams the three value arrays and the narrow column image once,
// gathers u, v, w where they lie and reads b_u, b_v, b_w — the three-system product's matrix bytes plus 24 bytes of b per row.
// Compiled with -ffp-contract=off: a row's sum is a separate multiply and add per entry in ascending stored order from 0.0, the
// one-system product's order, so tests/residual_restatement.py forms the same r_P and d_P bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "assembly.hpp"
#include "convergence.hpp"
#include "linalg_kernels.hpp"

namespace orc {

namespace {

struct Residual3Args {
    const double *val[3];  // a_u, a_v, a_w: SELL values on the mesh pattern
    const double *b[3];    // b_u, b_v, b_w
    const double *x[3];    // u, v, w as the systems were assembled from them (ghost entries refreshed at the top of the iteration)
};

// partials[(3 * kind + system) * gridDim.x + blockIdx.x], kind 0: sum |r_P|, 1: sum |d_P|, 2: sum r_P^2, 3: max |r_P|
enum { kResL1 = 0, kResScale = 1, kResSq = 2, kResMax = 3, kResKinds = 4 };

// One pass over the mesh pattern, thread per row, the slice walk and the chunking of spmv3_uniform_k.  d_P = a_PP phi_P is the term of
// the row's own column as the sum meets it (the mesh pattern stores a column once per row: the same product as through diag_pos, and
// 0 when no entry of the row has the row's column) — the diagonal's position is not read a second time.
template <bool kNarrow, bool kNT>
__global__ __launch_bounds__(kBlock) void momentum_residual3_k(SellDev P, Residual3Args A, double *__restrict__ partials) {
    __shared__ double lds[8];
    constexpr int kChunk = 4;
    const int lane = threadIdx.x & 63;
    double l1[3] = {0., 0., 0.}, sc[3] = {0., 0., 0.}, sq[3] = {0., 0., 0.}, mx[3] = {0., 0., 0.};
    SliceWalk w(P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int64_t base = P.slice_ptr[slice];
        const int width = (int)((P.slice_ptr[slice + 1] - base) >> 6);
        const bool live = row < P.n;
        const int len = live ? P.row_len[row] : 0;
        double acc0 = 0., acc1 = 0., acc2 = 0., d0 = 0., d1 = 0., d2 = 0.;
        const int32_t *__restrict__ cb = kNarrow ? P.colbase + (base >> 6) : nullptr;
        for (int k0 = 0; k0 < width; k0 += kChunk) {
            int c[kChunk];
            double v0[kChunk], v1[kChunk], v2[kChunk], x0[kChunk], x1[kChunk], x2[kChunk];
            const int64_t p0 = base + (int64_t)k0 * 64 + lane;
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {  // wave-uniform matrix loads at compile-time offsets from one chunk base (every slot of a slice is stored)
                const bool in = k0 + u < width;
                if (kNarrow) c[u] = in ? cb[k0 + u] + (int)ld_stream<kNT>(P.col16 + p0 + (int64_t)u * 64) : 0;
                else c[u] = in ? ld_stream<kNT>(P.col + p0 + (int64_t)u * 64) : 0;
                v0[u] = in ? ld_stream<kNT>(A.val[0] + p0 + (int64_t)u * 64) : 0.;
                v1[u] = in ? ld_stream<kNT>(A.val[1] + p0 + (int64_t)u * 64) : 0.;
                v2[u] = in ? ld_stream<kNT>(A.val[2] + p0 + (int64_t)u * 64) : 0.;
            }
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {  // padding slots and dead lanes gather nothing
                const bool in = k0 + u < len;
                x0[u] = in ? A.x[0][c[u]] : 0.;
                x1[u] = in ? A.x[1][c[u]] : 0.;
                x2[u] = in ? A.x[2][c[u]] : 0.;
            }
#pragma unroll
            for (int u = 0; u < kChunk; ++u) {
                if (k0 + u < len) {
                    const double t0 = v0[u] * x0[u], t1 = v1[u] * x1[u], t2 = v2[u] * x2[u];
                    acc0 += t0; acc1 += t1; acc2 += t2;
                    if ((int64_t)c[u] == row) { d0 = t0; d1 = t1; d2 = t2; }
                }
            }
        }
        if (live) {
            const double r0 = A.b[0][row] - acc0, r1 = A.b[1][row] - acc1, r2 = A.b[2][row] - acc2;
            const double a0 = fabs(r0), a1 = fabs(r1), a2 = fabs(r2);
            l1[0] += a0; l1[1] += a1; l1[2] += a2;
            sc[0] += fabs(d0); sc[1] += fabs(d1); sc[2] += fabs(d2);
            sq[0] += r0 * r0; sq[1] += r1 * r1; sq[2] += r2 * r2;
            mx[0] = max_nan(mx[0], a0); mx[1] = max_nan(mx[1], a1); mx[2] = max_nan(mx[2], a2);
        }
    }
    const size_t g = gridDim.x;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        double t = block_sum(l1[s], lds);
        if (threadIdx.x == 0) partials[(size_t)(3 * kResL1 + s) * g + blockIdx.x] = t;
        t = block_sum(sc[s], lds);
        if (threadIdx.x == 0) partials[(size_t)(3 * kResScale + s) * g + blockIdx.x] = t;
        t = block_sum(sq[s], lds);
        if (threadIdx.x == 0) partials[(size_t)(3 * kResSq + s) * g + blockIdx.x] = t;
        t = block_max(mx[s], lds);
        if (threadIdx.x == 0) partials[(size_t)(3 * kResMax + s) * g + blockIdx.x] = t;
    }
}

// sum |b|, sum b^2, max |b| over the owned rows: partials[q * gridDim.x + blockIdx.x], q = 0, 1, 2
__global__ __launch_bounds__(kBlock) void imbalance_k(const double *__restrict__ b, int64_t n_own, double *__restrict__ partials) {
    __shared__ double lds[8];
    double l1 = 0., sq = 0., mx = 0.;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_own; i += (int64_t)gridDim.x * kBlock) {
        const double v = b[i], a = fabs(v);
        l1 += a;
        sq += v * v;
        mx = max_nan(mx, a);
    }
    double t = block_sum(l1, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    t = block_sum(sq, lds);
    if (threadIdx.x == 0) partials[(size_t)gridDim.x + blockIdx.x] = t;
    t = block_max(mx, lds);
    if (threadIdx.x == 0) partials[(size_t)2 * gridDim.x + blockIdx.x] = t;
}

// the maxima's counterpart of reduce_partials_k: out[q] = max of partials[q * count .. (q + 1) * count), all of them >= 0 or NaN
__global__ __launch_bounds__(kBlock) void fold_max_k(const double *__restrict__ partials, int count, int nq, double *__restrict__ out) {
    __shared__ double lds[8];
    for (int q = 0; q < nq; ++q) {
        double v = 0.;
        for (int i = threadIdx.x; i < count; i += kBlock) v = max_nan(v, partials[(size_t)q * count + i]);
        const double t = block_max(v, lds);
        if (threadIdx.x == 0) out[q] = t;
    }
}

// where the folded slots sit in SolverState::Monitor::dev — sums first, maxima behind them: one all-reduce each on a partitioned mesh
enum { kDevMomentumSums = 0, kDevContinuitySums = 9, kDevMomentumMax = 11, kDevContinuityMax = 14 };
static_assert(kDevMomentumMax == SolverState::Monitor::kSums && kDevContinuityMax + 1 == SolverState::Monitor::kSums + SolverState::Monitor::kMaxima,
              "the collective layout of the monitor's folded slots");

}  // namespace

int monitors_enable(SolverState &s, bool on) {
    SolverState::Monitor &M = s.mon;
    if (on) {
        ORC_TRY(M.partials.ensure((size_t)(3 * kResKinds + 3) * kMaxPartials));
        ORC_TRY(M.dev.ensure((size_t)(SolverState::Monitor::kSums + SolverState::Monitor::kMaxima)));
        ORC_TRY(M.dev.zero());
        if (!M.raw.p) ORC_TRY(M.raw.alloc((size_t)(SolverState::Monitor::kSums + SolverState::Monitor::kMaxima)));
    } else {
        ORC_HIP(hipStreamSynchronize(ctx().stream));  // no pass of the monitor is in flight when its buffers go
        M.partials.release();
        M.dev.release();
        M.raw.release();
    }
    M.history.clear();
    M.seen = 0;
    M.scale = 0.;
    M.on = on;
    return ORC_OK;
}

int k_momentum_residuals(SolverState &s) {
    SolverState::Monitor &M = s.mon;
    const SellDev P = s.mesh->pat.dev();
    if (P.n == 0) return ORC_OK;
    const Residual3Args A{{s.a_u.p, s.a_v.p, s.a_w.p}, {s.b_u.p, s.b_v.p, s.b_w.p}, {s.u.p, s.v.p, s.w.p}};
    const int g = spmv_grid(P.n_slices);  // <= kMaxPartials
    // the matrix streams are read once: the non-temporal hint by the three-system product's rule (launch_spmv3)
    const bool nt = stream_nt_policy(P.padded * (P.col16 ? 26 : 28)) != 0;
    hipStream_t st = ctx().stream;
    if (P.col16) {
        if (nt) hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_residual3_k<true, true>), dim3(g), dim3(kBlock), 0, st, P, A, M.partials.p);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_residual3_k<true, false>), dim3(g), dim3(kBlock), 0, st, P, A, M.partials.p);
    } else {
        if (nt) hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_residual3_k<false, true>), dim3(g), dim3(kBlock), 0, st, P, A, M.partials.p);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_residual3_k<false, false>), dim3(g), dim3(kBlock), 0, st, P, A, M.partials.p);
    }
    ORC_HIP(hipGetLastError());
    ORC_TRY(reduce_partials(M.partials.p, g, 3 * kResMax, M.dev.p + kDevMomentumSums));  // this rank's sums; the ranks' are added in monitor_fetch
    hipLaunchKernelGGL(fold_max_k, dim3(1), dim3(kBlock), 0, st, M.partials.p + (size_t)3 * kResMax * g, g, 3, M.dev.p + kDevMomentumMax);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_imbalance(SolverState &s) {
    SolverState::Monitor &M = s.mon;
    double *part = M.partials.p + (size_t)3 * kResKinds * kMaxPartials;
    const int g = grid_for(s.n_own);
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(imbalance_k, dim3(g), dim3(kBlock), 0, st, s.b_p.p, s.n_own, part);
    ORC_HIP(hipGetLastError());
    ORC_TRY(reduce_partials(part, g, 2, M.dev.p + kDevContinuitySums));
    hipLaunchKernelGGL(fold_max_k, dim3(1), dim3(kBlock), 0, st, part + (size_t)2 * g, g, 1, M.dev.p + kDevContinuityMax);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int monitor_fetch(SolverState &s) {
    SolverState::Monitor &M = s.mon;
    constexpr int kS = SolverState::Monitor::kSums, kM = SolverState::Monitor::kMaxima;
    if (s.mesh->halo.active() && ctx().world > 1) {  // the owned rows of all ranks: one sum and one max, behind the iteration's own collectives
        ORC_TRY(comm_allreduce_sum(M.dev.p, kS));
        ORC_TRY(comm_allreduce_max(M.dev.p + kS, kM));
    }
    ORC_HIP(hipMemcpyAsync(M.raw.p, M.dev.p, sizeof(double) * (kS + kM), hipMemcpyDeviceToHost, ctx().stream));
    return ORC_OK;
}

void monitor_append(SolverState &s) {
    SolverState::Monitor &M = s.mon;
    double rec[ORC_RESIDUAL_N] = {0.};
    for (int k = 0; k < 9; ++k) rec[ORC_RESIDUAL_MOMENTUM_L1 + k] = M.raw.p[kDevMomentumSums + k];
    for (int k = 0; k < 3; ++k) rec[ORC_RESIDUAL_MOMENTUM_MAX + k] = M.raw.p[kDevMomentumMax + k];
    rec[ORC_RESIDUAL_CONTINUITY_L1] = M.raw.p[kDevContinuitySums];
    rec[ORC_RESIDUAL_CONTINUITY_SQ] = M.raw.p[kDevContinuitySums + 1];
    rec[ORC_RESIDUAL_CONTINUITY_MAX] = M.raw.p[kDevContinuityMax];
    residual_record_finish(rec, M.seen, &M.scale);
    M.seen += 1;
    M.history.insert(M.history.end(), rec, rec + ORC_RESIDUAL_N);
}

}  // namespace orc

using namespace orc;

extern "C" {

int orc_solver_set_monitors(OrcSolver *s, int32_t on) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "monitors: null solver");
    return monitors_enable(s->st, on != 0);
}

int64_t orc_solver_residual_count(OrcSolver *s) { return s ? (int64_t)(s->st.mon.history.size() / ORC_RESIDUAL_N) : 0; }

int orc_solver_residual_history(OrcSolver *s, uint64_t first, uint64_t count, double *out) {
    ORC_TRY(ensure_init());
    if (!s || (!out && count > 0)) return set_error(ORC_ERR_BAD_ARGUMENT, "residual history: null argument");
    const uint64_t have = s->st.mon.history.size() / ORC_RESIDUAL_N;
    if (first > have || count > have - first)
        return set_error(ORC_ERR_BAD_ARGUMENT, "residual history: records [%llu, %llu + %llu) of %llu", (unsigned long long)first, (unsigned long long)first,
                         (unsigned long long)count, (unsigned long long)have);
    if (count > 0) std::copy(s->st.mon.history.begin() + (std::ptrdiff_t)(first * ORC_RESIDUAL_N), s->st.mon.history.begin() + (std::ptrdiff_t)((first + count) * ORC_RESIDUAL_N), out);
    return ORC_OK;
}

int orc_convergence_check(const OrcConvergence *c, const double *record, int32_t *failing_mask) {
    if (!c || !record || !convergence_valid(*c)) {
        if (failing_mask) *failing_mask = 15;
        return -1;
    }
    return convergence_check(*c, record, failing_mask);
}

// measurement hook: momentum_residual3_k on the solver's assembled systems and current fields (launch, fold and all) `reps` times,
// HIP events on the library stream; average ms per pass.  Needs monitoring on (the pass writes the monitor's partial sums).
int orc_bench_momentum_residuals(OrcSolver *s, int reps, double *avg_ms) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    if (!s->st.mon.on) return set_error(ORC_ERR_BAD_ARGUMENT, "orc_bench_momentum_residuals without orc_solver_set_monitors");
    if (reps < 1) reps = 1;
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    int st = k_momentum_residuals(s->st);  // warm
    if (st == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    for (int i = 0; i < reps && st == ORC_OK; ++i) st = k_momentum_residuals(s->st);
    if (st == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    float ms = 0.f;
    if (st == ORC_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventElapsedTime failed");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / reps;
    return st;
}

int orc_solver_get_pressure_rhs(OrcSolver *s, double *b_p) {
    ORC_TRY(ensure_init());
    if (!s || !b_p) return set_error(ORC_ERR_BAD_ARGUMENT, "pressure right-hand side: null argument");
    return s->st.b_p.download(b_p, (size_t)s->st.n);
}

}  // extern "C"
