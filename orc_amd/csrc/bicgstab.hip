// bicgstab.hip — the BiCGSTAB arm of iterative_solve for one system and for three systems in lock-step: fused
// vector updates that fold the products' partial sums themselves, no host round-trip inside a solve.
// Reference: src/linear_algebra.rs:247-269, with the Jacobi scaling of :159-167.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "linalg_kernels.hpp"

namespace orc {

// scal[] layout (device doubles):
enum { S_RHO0 = 0, S_RHO1 = 1, S_SUM_NU = 2, S_TS = 3, S_TT = 4, S_FROZEN = 5, S_FROZEN2 = 6, S_COUNT = 8 };

// Breakdown guard (OrcSettings.breakdown_guard, new-build extension).  The reference iterates a fixed
// count with no test at all (:255-268); when rho, r_hat.nu, t.t or omega is exactly 0 (a cancelling
// tree sum, a zero right-hand side, a converged start) it divides 0/0 and the SIMPLE loop panics
// with "solution diverged".  With the guard the solve freezes instead: x keeps its last finite
// value and the remaining iterations are no-ops.  Nothing changes when no denominator is 0.
// S_FROZEN is written only by kernels whose reaction to a breakdown is "do nothing" (so a block
// that starts late and sees the flag behaves like one that evaluated the test itself); the x/r
// update kernel reacts with x = h, r = s and therefore publishes through S_FROZEN2, which it does
// not read.
__device__ __forceinline__ bool bicg_frozen(const double *__restrict__ scal, int guard) {
    return guard && (scal[S_FROZEN] != 0. || scal[S_FROZEN2] != 0.);
}
__device__ __forceinline__ bool finite_nonzero(double v) { return v != 0. && isfinite(v); }

// s = r - alpha*nu, alpha = rho / (r_hat_0 . nu)                     (:257, :259)
// fold (null: scal[S_SUM_NU] is there already): the product's partial sums of nu, folded by every workgroup here
__global__ __launch_bounds__(kBlock) void bicg_s_k(double *__restrict__ scal, int rho_idx, const double *__restrict__ r, const double *__restrict__ nu,
                                                   double *__restrict__ s, int64_t n, int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds16[16];
    if (bicg_frozen(scal, guard)) return;
    // 16-byte accesses: two consecutive elements per lane (arena vectors are 256-byte aligned).  The first pair of every
    // thread is requested BEFORE the fold, so that its round trip and the fold's overlap.
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    const double2 *r2 = reinterpret_cast<const double2 *>(r), *nu2 = reinterpret_cast<const double2 *>(nu);
    double2 *s2 = reinterpret_cast<double2 *>(s);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double2 a = make_double2(0., 0.), b = make_double2(0., 0.);
    if (i < n2) { a = r2[i]; b = nu2[i]; }
    double sum_nu;
    if (fold) {
        sum_nu = fold_partials_block(fold, fold_count, lds16);
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_SUM_NU] = sum_nu;  // the later kernels of the iteration read it
    } else {
        sum_nu = scal[S_SUM_NU];
    }
    const double alpha = scal[rho_idx] / sum_nu;
    if (guard && !(finite_nonzero(scal[rho_idx]) && finite_nonzero(sum_nu) && isfinite(alpha))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_FROZEN] = 1.;
        return;
    }
    while (i < n2) {
        const int64_t nx = i + stride;
        double2 an = make_double2(0., 0.), bn = make_double2(0., 0.);
        if (nx < n2) { an = r2[nx]; bn = nu2[nx]; }
        s2[i] = make_double2(a.x - alpha * b.x, a.y - alpha * b.y);
        a = an; b = bn; i = nx;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s[n - 1] = r[n - 1] - alpha * nu[n - 1];
}
// h = x + alpha p ; x = h + omega s ; r = s - omega t ; partial sum(r)   (:258, :261-263, :265)
__global__ __launch_bounds__(kBlock) void bicg_xr_k(double *__restrict__ scal, int rho_idx, double *__restrict__ x,
                                                    const double *__restrict__ p, const double *__restrict__ s,
                                                    const double *__restrict__ t, double *__restrict__ r, int64_t n,
                                                    double *__restrict__ partials, int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[8];
    __shared__ double lds16[32];
    if (guard && scal[S_FROZEN] != 0.) return;
    // the first pairs of every thread are requested before the folds (their round trips overlap)
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    double2 *x2 = reinterpret_cast<double2 *>(x), *r2 = reinterpret_cast<double2 *>(r);
    const double2 *p2 = reinterpret_cast<const double2 *>(p), *s2 = reinterpret_cast<const double2 *>(s), *t2 = reinterpret_cast<const double2 *>(t);
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double2 xv = make_double2(0., 0.), pv = xv, sv = xv, tv = xv;
    if (i0 < n2) { xv = x2[i0]; pv = p2[i0]; sv = s2[i0]; tv = t2[i0]; }
    double ts, tt;
    if (fold) {  // t.s and t.t from the product's two partial arrays (fold != partials: this kernel writes its own sums)
        double both[2];
        fold_partials_multi<2>(fold, fold_count, lds16, both);  // [r04] the two folds' loads in flight together, two barriers instead of four: the same bits
        ts = both[0]; tt = both[1];
        if (blockIdx.x == 0 && threadIdx.x == 0) { scal[S_TS] = ts; scal[S_TT] = tt; }
    } else {
        ts = scal[S_TS]; tt = scal[S_TT];
    }
    const double alpha = scal[rho_idx] / scal[S_SUM_NU];
    double omega = ts / tt;
    const bool bad = guard && !(finite_nonzero(tt) && isfinite(omega));
    double acc = 0.;
    if (bad) {
        // t = A s vanished (s is already the zero residual) or overflowed: take x = h, r = s and stop
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
            x[i] = x[i] + alpha * p[i];
            const double si = s[i];
            r[i] = si;
            acc += si;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_FROZEN2] = 1.;
    } else {
        int64_t i = i0;
        while (i < n2) {
            const int64_t nx = i + stride;
            double2 xn = make_double2(0., 0.), pn = xn, sn = xn, tn = xn;
            if (nx < n2) { xn = x2[nx]; pn = p2[nx]; sn = s2[nx]; tn = t2[nx]; }
            const double h0 = xv.x + alpha * pv.x, h1 = xv.y + alpha * pv.y;
            x2[i] = make_double2(h0 + omega * sv.x, h1 + omega * sv.y);
            const double q0 = sv.x - omega * tv.x, q1 = sv.y - omega * tv.y;
            r2[i] = make_double2(q0, q1);
            acc += q0;
            acc += q1;
            xv = xn; pv = pn; sv = sn; tv = tn; i = nx;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const int64_t i = n - 1;
            const double h = x[i] + alpha * p[i];
            const double si = s[i];
            x[i] = h + omega * si;
            const double ri = si - omega * t[i];
            r[i] = ri;
            acc += ri;
        }
    }
    const double tsum = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = tsum;
}
// beta = rho/rho_prev * alpha/omega ; p = r + beta (p - omega nu)       (:266-267)
__global__ __launch_bounds__(kBlock) void bicg_p_k(double *__restrict__ scal, int rho_prev_idx, int rho_idx, const double *__restrict__ r,
                                                   const double *__restrict__ nu, double *__restrict__ p, int64_t n, int guard,
                                                   const double *__restrict__ fold, int fold_count) {
    __shared__ double lds16[16];
    if (bicg_frozen(scal, guard)) {
        // bicg_xr_k took x = h, r = s and published through S_FROZEN2, which it does not read itself: promote it, or the next
        // iteration's bicg_xr_k would add alpha p once more (every workgroup of THIS launch returns here either way)
        if (guard && scal[S_FROZEN2] != 0. && blockIdx.x == 0 && threadIdx.x == 0) scal[S_FROZEN] = 1.;
        return;
    }
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    double2 *p2 = reinterpret_cast<double2 *>(p);
    const double2 *r2 = reinterpret_cast<const double2 *>(r), *nu2 = reinterpret_cast<const double2 *>(nu);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double2 rv = make_double2(0., 0.), pv = rv, nv = rv;
    if (i < n2) { rv = r2[i]; pv = p2[i]; nv = nu2[i]; }  // requested before the fold
    double rho;
    if (fold) {  // rho = sum(r) from bicg_xr_k's partial sums
        rho = fold_partials_block(fold, fold_count, lds16);
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[rho_idx] = rho;
    } else {
        rho = scal[rho_idx];
    }
    const double rho_prev = scal[rho_prev_idx];
    const double alpha = rho_prev / scal[S_SUM_NU];
    const double omega = scal[S_TS] / scal[S_TT];
    const double beta = rho / rho_prev * alpha / omega;
    if (guard && !(finite_nonzero(omega) && isfinite(beta))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_FROZEN] = 1.;
        return;
    }
    while (i < n2) {
        const int64_t nx = i + stride;
        double2 rn = make_double2(0., 0.), pn = rn, nn = rn;
        if (nx < n2) { rn = r2[nx]; pn = p2[nx]; nn = nu2[nx]; }
        p2[i] = make_double2(rv.x + beta * (pv.x - omega * nv.x), rv.y + beta * (pv.y - omega * nv.y));
        rv = rn; pv = pn; nv = nn; i = nx;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = r[n - 1] + beta * (p[n - 1] - omega * nu[n - 1]);
}

// one more solve in which the guard fired (orc_breakdown_guard_events): a drop-in caller must be able to tell that the
// reference would have produced NaN here
__global__ void guard_event_k(const double *__restrict__ scal, int *__restrict__ counter) {
    if (scal[S_FROZEN] != 0. || scal[S_FROZEN2] != 0.) atomicAdd(counter, 1);
}

struct BicgWork {
    double *r, *p, *nu, *s, *t, *partials, *partials2, *scal;  // partials2: bicg_xr_k's sums while it still folds the product's
};

static int bicg_alloc(Arena &arena, int64_t n, BicgWork &w) {  // n = vector length incl. ghost entries
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    ORC_TRY(arena.alloc(nn, &w.r));
    ORC_TRY(arena.alloc(nn, &w.p));
    ORC_TRY(arena.alloc(nn, &w.nu));
    ORC_TRY(arena.alloc(nn, &w.s));
    ORC_TRY(arena.alloc(nn, &w.t));
    ORC_TRY(arena.alloc((size_t)2 * kMaxPartials, &w.partials));
    ORC_TRY(arena.alloc((size_t)kMaxPartials, &w.partials2));
    ORC_TRY(arena.alloc((size_t)S_COUNT, &w.scal));
    ORC_HIP(hipMemsetAsync(w.scal, 0, S_COUNT * sizeof(double), ctx().stream));
    return ORC_OK;
}

static int bicg_iteration(const MatView &A, double *x, const BicgWork &w, uint64_t it, int guard) {
    const int64_t n = A.P.n;
    const int vg = grid_for((n + 1) / 2);  // two elements per lane
    const int cur = (int)(it & 1), nxt = cur ^ 1;
    const double *skip = guard ? w.scal + S_FROZEN : nullptr;  // frozen solves skip their SpMVs too
    int g = 0;
    const bool ref = reference_order(A);  // dot products in nalgebra's association (verification mode)
    // Single GPU, tree reductions: the three sums of the iteration are folded by the kernels that consume them (every
    // workgroup folds, workgroup 0 stores the scalar for the later kernels) instead of by one-workgroup launches in between.
    const bool fused = !ref && A.halo == nullptr;
    ORC_TRY(product_store_sum(A, w.p, w.nu, w.partials, &g, skip));            // nu = A p, sum(nu)
    if (ref) ORC_TRY(dot_reference(nullptr, w.nu, n, w.scal + S_SUM_NU, skip));            // r_hat_0 . nu  (:257)
    else if (!fused) ORC_TRY(reduce_partials(w.partials, g, 1, w.scal + S_SUM_NU, A.halo != nullptr));
    hipLaunchKernelGGL(bicg_s_k, dim3(vg), dim3(kBlock), 0, ctx().stream, w.scal, S_RHO0 + cur, w.r, w.nu, w.s, n, guard,
                       fused ? (const double *)w.partials : (const double *)nullptr, g);
    ORC_TRY(product_ts(A, w.s, w.t, w.partials, &g, skip));                    // t = A s, t.s, t.t
    if (ref) {
        ORC_TRY(dot_reference(w.t, w.s, n, w.scal + S_TS, skip));                          // t . s, t . t  (:261)
        ORC_TRY(dot_reference(w.t, w.t, n, w.scal + S_TT, skip));
    } else if (!fused) ORC_TRY(reduce_partials(w.partials, g, 2, w.scal + S_TS, A.halo != nullptr));
    double *xr_partials = fused ? w.partials2 : w.partials;
    hipLaunchKernelGGL(bicg_xr_k, dim3(vg), dim3(kBlock), 0, ctx().stream, w.scal, S_RHO0 + cur, x, w.p, w.s, w.t, w.r, n, xr_partials, guard,
                       fused ? (const double *)w.partials : (const double *)nullptr, g);
    if (ref) ORC_TRY(dot_reference(nullptr, w.r, n, w.scal + S_RHO0 + nxt, skip));  // rho = r_hat_0 . r  (:265)
    else if (!fused) ORC_TRY(reduce_partials(w.partials, vg, 1, w.scal + S_RHO0 + nxt, A.halo != nullptr));  // rho = r_hat_0 . r
    hipLaunchKernelGGL(bicg_p_k, dim3(vg), dim3(kBlock), 0, ctx().stream, w.scal, S_RHO0 + cur, S_RHO0 + nxt, w.r, w.nu, w.p, n, guard,
                       fused ? (const double *)w.partials2 : (const double *)nullptr, vg);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// linear_algebra.rs:247-269 on a view whose scalings are final (materialised or carried as s1 / s2)
static int bicgstab_run(const MatView &A, const double *b, double *x, uint64_t iteration_count, Arena &arena) {
    const int64_t n = A.P.n;
    if (n == 0) return ORC_OK;
    ArenaScope scope(arena);
    BicgWork w;
    ORC_TRY(bicg_alloc(arena, std::max(A.P.ncols, n), w));
    const int guard = ctx().breakdown_guard ? 1 : 0;
    int g = 0;
    ORC_TRY(product_residual(A, x, b, w.r, w.p, w.partials, &g, nullptr));     // r = b - A x ; p = r ; rho = sum(r)
    if (reference_order(A)) ORC_TRY(dot_reference(nullptr, w.r, n, w.scal + S_RHO0, nullptr));  // r . r_hat_0  (:253)
    else ORC_TRY(reduce_partials(w.partials, g, 1, w.scal + S_RHO0, A.halo != nullptr));
    for (uint64_t it = 0; it < iteration_count; ++it) ORC_TRY(bicg_iteration(A, x, w, it, guard));
    if (guard && ctx().guard_events) {
        hipLaunchKernelGGL(guard_event_k, dim3(1), dim3(1), 0, ctx().stream, w.scal, ctx().guard_events);
        ORC_HIP(hipGetLastError());
    }
    return ORC_OK;
}

int bicgstab_dev(const MatView &A_in, const double *b, double *x, uint64_t iteration_count, Arena &arena) {
    if (A_in.P.n == 0) return ORC_OK;
    ArenaScope scope(arena);
    MatView A = A_in;
    ORC_TRY(materialize_scaled_view(A, iteration_count, arena));
    return bicgstab_run(A, b, x, iteration_count, arena);
}

int jacobi_scaling_prepare_dev(const MatView &A_in, uint64_t iteration_count, Arena &arena, ScaledOperator &S) {
    ORC_TRY(ensure_init());
    const int64_t n = A_in.P.n;
    S = ScaledOperator();
    S.A = A_in;
    S.iterations = iteration_count;
    double *dinv;
    ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &dinv));
    ORC_TRY(diag_inverse_dev(A_in, dinv));
    if (!S.A.s1) S.A.s1 = dinv;
    else if (!S.A.s2) S.A.s2 = dinv;
    else return set_error(ORC_ERR_BAD_ARGUMENT, "more than two nested Jacobi scalings");
    S.dinv = dinv;
    return materialize_scaled_view(S.A, iteration_count, arena);
}

int bicgstab_scaled_dev(const ScaledOperator &S, const double *b, double *x, Arena &arena) {
    const int64_t n = S.A.P.n;
    if (n == 0) return ORC_OK;
    ArenaScope scope(arena);
    double *b_tmp;
    ORC_TRY(arena.alloc((size_t)n, &b_tmp));
    ORC_TRY(scale_vec_dev(S.dinv, b, b_tmp, n));  // :165
    return bicgstab_run(S.A, b_tmp, x, S.iterations, arena);
}

int bench_bicgstab_dev(const MatView &A, const double *b, double *x, int reps, Arena &arena, float *ms) {
    const int64_t n = A.P.n;
    Arena::Mark mk = arena.mark();
    BicgWork w;
    ORC_TRY(bicg_alloc(arena, std::max(A.P.ncols, n), w));
    int g = 0;
    ORC_TRY(product_residual(A, x, b, w.r, w.p, w.partials, &g, nullptr));
    ORC_TRY(reduce_partials(w.partials, g, 1, w.scal + S_RHO0, A.halo != nullptr));
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    ORC_TRY(bicg_iteration(A, x, w, 0, 0));  // warm; guard off so every timed launch does full work
    ORC_HIP(hipEventRecord(e0, ctx().stream));
    for (int it = 1; it <= reps; ++it) ORC_TRY(bicg_iteration(A, x, w, (uint64_t)it, 0));
    ORC_HIP(hipEventRecord(e1, ctx().stream));
    ORC_HIP(hipEventSynchronize(e1));
    ORC_HIP(hipEventElapsedTime(ms, e0, e1));
    *ms /= (float)reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    arena.release(mk);
    return ORC_OK;
}


// ------------------------------------------------------------------ three systems in lock-step (MatView3, linalg.hpp)
// The u, v and w momentum systems of an iteration: one pattern, three value arrays, interleaved vectors.  Every kernel
// below keeps, per system, the thread -> element map, the order of the additions and the fold of its one-system
// counterpart above, so a system solved here and the same system solved alone agree in every bit
// (tests/test_gpu_triple.py).  Scalars of system s: scal3[idx * 3 + s].
bool triple_supported() { return ctx().reduction_order != ORC_REDUCTION_REFERENCE; }

#define SC3(idx, s) ((idx) * 3 + (s))
__device__ __forceinline__ bool bicg_frozen3(const double *__restrict__ scal3, int s, int guard) {
    return guard && (scal3[SC3(S_FROZEN, s)] != 0. || scal3[SC3(S_FROZEN2, s)] != 0.);
}

// bicg_s_k for three systems: s = r - alpha nu, alpha = rho / sum(nu); fold: the product's partial sums, system s at fold + s * fold_count
__global__ __launch_bounds__(kBlock) void bicg_s3_k(double *__restrict__ scal3, int rho_idx, const double *__restrict__ r3, const double *__restrict__ nu3,
                                                    double *__restrict__ s3, int64_t n, int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds16[3 * 16];
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    const double2 *r2 = reinterpret_cast<const double2 *>(r3), *nu2 = reinterpret_cast<const double2 *>(nu3);
    double2 *s2 = reinterpret_cast<double2 *>(s3);
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double2 a0, a1, a2, b0, b1, b2;
    a0 = a1 = a2 = b0 = b1 = b2 = make_double2(0., 0.);
    if (i < n2) { a0 = r2[3 * i]; a1 = r2[3 * i + 1]; a2 = r2[3 * i + 2]; b0 = nu2[3 * i]; b1 = nu2[3 * i + 1]; b2 = nu2[3 * i + 2]; }
    double alpha[3];
    bool act[3];
    // fold_count == 0 (partitioned operator): fold holds the sums themselves — folded by reduce_partials_k, summed over the ranks
    double folded[3] = {0., 0., 0.};
    if (fold_count) fold_partials_multi<3>(fold, fold_count, lds16, folded);  // [r04] the three folds' loads in flight together, two barriers
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const bool frz = bicg_frozen3(scal3, s, guard);
        const double sum_nu = fold_count ? folded[s] : fold[s];
        const double rho = scal3[SC3(rho_idx, s)];
        alpha[s] = rho / sum_nu;
        const bool bad = guard && !(finite_nonzero(rho) && finite_nonzero(sum_nu) && isfinite(alpha[s]));
        act[s] = !frz && !bad;
        if (blockIdx.x == 0 && threadIdx.x == 0 && !frz) {
            scal3[SC3(S_SUM_NU, s)] = sum_nu;
            if (bad) scal3[SC3(S_FROZEN, s)] = 1.;
        }
    }
    if (act[0] && act[1] && act[2]) {
        // a pair of rows = six consecutive doubles: systems (0,1) (2,0) (1,2)
        while (i < n2) {
            const int64_t nx = i + stride;
            double2 an0, an1, an2, bn0, bn1, bn2;
            an0 = an1 = an2 = bn0 = bn1 = bn2 = make_double2(0., 0.);
            if (nx < n2) { an0 = r2[3 * nx]; an1 = r2[3 * nx + 1]; an2 = r2[3 * nx + 2]; bn0 = nu2[3 * nx]; bn1 = nu2[3 * nx + 1]; bn2 = nu2[3 * nx + 2]; }
            s2[3 * i] = make_double2(a0.x - alpha[0] * b0.x, a0.y - alpha[1] * b0.y);
            s2[3 * i + 1] = make_double2(a1.x - alpha[2] * b1.x, a1.y - alpha[0] * b1.y);
            s2[3 * i + 2] = make_double2(a2.x - alpha[1] * b2.x, a2.y - alpha[2] * b2.y);
            a0 = an0; a1 = an1; a2 = an2; b0 = bn0; b1 = bn1; b2 = bn2; i = nx;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int s = 0; s < 3; ++s) s3[3 * (n - 1) + s] = r3[3 * (n - 1) + s] - alpha[s] * nu3[3 * (n - 1) + s];
        }
    } else {  // a system broke down or is frozen: element by element, the others as usual
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (act[s]) s3[3 * e + s] = r3[3 * e + s] - alpha[s] * nu3[3 * e + s];
        }
    }
}

// bicg_xr_k for three systems.  partials: system s at partials + s * gridDim.x; fold: the product's sums, (t.s, t.t) of system s
// at fold + (2 s) * fold_count and fold + (2 s + 1) * fold_count
__global__ __launch_bounds__(kBlock) void bicg_xr3_k(double *__restrict__ scal3, int rho_idx, double *__restrict__ x3, const double *__restrict__ p3,
                                                     const double *__restrict__ s3, const double *__restrict__ t3, double *__restrict__ r3, int64_t n,
                                                     double *__restrict__ partials, int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[8];
    __shared__ double lds16[6 * 16];
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double2 *x2 = reinterpret_cast<double2 *>(x3), *r2 = reinterpret_cast<double2 *>(r3);
    const double2 *p2 = reinterpret_cast<const double2 *>(p3), *s2 = reinterpret_cast<const double2 *>(s3), *t2 = reinterpret_cast<const double2 *>(t3);
    double alpha[3], omega[3];
    int state[3];  // 0 = normal, 1 = t = A s vanished or overflowed (x = h, r = s, stop), 2 = frozen (no-op)
    double folded[6] = {0., 0., 0., 0., 0., 0.};
    if (fold_count) fold_partials_multi<6>(fold, fold_count, lds16, folded);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const bool frz = guard && scal3[SC3(S_FROZEN, s)] != 0.;
        const double ts = fold_count ? folded[2 * s] : fold[2 * s];
        const double tt = fold_count ? folded[2 * s + 1] : fold[2 * s + 1];
        alpha[s] = scal3[SC3(rho_idx, s)] / scal3[SC3(S_SUM_NU, s)];
        omega[s] = ts / tt;
        const bool bad = guard && !(finite_nonzero(tt) && isfinite(omega[s]));
        state[s] = frz ? 2 : (bad ? 1 : 0);
        if (blockIdx.x == 0 && threadIdx.x == 0 && !frz) { scal3[SC3(S_TS, s)] = ts; scal3[SC3(S_TT, s)] = tt; }
    }
    double acc[3] = {0., 0., 0.};
    if (state[0] == 0 && state[1] == 0 && state[2] == 0) {
        int64_t i = i0;
        while (i < n2) {
            const double2 xa = x2[3 * i], xb = x2[3 * i + 1], xc = x2[3 * i + 2];
            const double2 pa = p2[3 * i], pb = p2[3 * i + 1], pc = p2[3 * i + 2];
            const double2 sa = s2[3 * i], sb = s2[3 * i + 1], sc = s2[3 * i + 2];
            const double2 ta = t2[3 * i], tb = t2[3 * i + 1], tc = t2[3 * i + 2];
            // row 2i: (xa.x, xa.y, xb.x) = systems 0, 1, 2; row 2i + 1: (xb.y, xc.x, xc.y)
            const double h00 = xa.x + alpha[0] * pa.x, h01 = xa.y + alpha[1] * pa.y, h02 = xb.x + alpha[2] * pb.x;
            const double h10 = xb.y + alpha[0] * pb.y, h11 = xc.x + alpha[1] * pc.x, h12 = xc.y + alpha[2] * pc.y;
            x2[3 * i] = make_double2(h00 + omega[0] * sa.x, h01 + omega[1] * sa.y);
            x2[3 * i + 1] = make_double2(h02 + omega[2] * sb.x, h10 + omega[0] * sb.y);
            x2[3 * i + 2] = make_double2(h11 + omega[1] * sc.x, h12 + omega[2] * sc.y);
            const double q00 = sa.x - omega[0] * ta.x, q01 = sa.y - omega[1] * ta.y, q02 = sb.x - omega[2] * tb.x;
            const double q10 = sb.y - omega[0] * tb.y, q11 = sc.x - omega[1] * tc.x, q12 = sc.y - omega[2] * tc.y;
            r2[3 * i] = make_double2(q00, q01);
            r2[3 * i + 1] = make_double2(q02, q10);
            r2[3 * i + 2] = make_double2(q11, q12);
            acc[0] += q00; acc[0] += q10;
            acc[1] += q01; acc[1] += q11;
            acc[2] += q02; acc[2] += q12;
            i += stride;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int64_t e = 3 * (n - 1) + s;
                const double h = x3[e] + alpha[s] * p3[e];
                const double si = s3[e];
                x3[e] = h + omega[s] * si;
                const double ri = si - omega[s] * t3[e];
                r3[e] = ri;
                acc[s] += ri;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            if (state[s] == 1) {  // bicg_xr_k's breakdown branch: one element per step of the grid-stride loop
                for (int64_t e = i0; e < n; e += stride) {
                    x3[3 * e + s] = x3[3 * e + s] + alpha[s] * p3[3 * e + s];
                    const double si = s3[3 * e + s];
                    r3[3 * e + s] = si;
                    acc[s] += si;
                }
                if (blockIdx.x == 0 && threadIdx.x == 0) scal3[SC3(S_FROZEN2, s)] = 1.;
            } else if (state[s] == 0) {  // bicg_xr_k's pair loop, this system's entries only
                for (int64_t i = i0; i < n2; i += stride) {
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int64_t e = 3 * (2 * i + h2) + s;
                        const double h = x3[e] + alpha[s] * p3[e];
                        const double si = s3[e];
                        x3[e] = h + omega[s] * si;
                        const double q = si - omega[s] * t3[e];
                        r3[e] = q;
                        acc[s] += q;
                    }
                }
                if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
                    const int64_t e = 3 * (n - 1) + s;
                    const double h = x3[e] + alpha[s] * p3[e];
                    const double si = s3[e];
                    x3[e] = h + omega[s] * si;
                    const double ri = si - omega[s] * t3[e];
                    r3[e] = ri;
                    acc[s] += ri;
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const double tsum = block_sum(acc[s], lds);
        if (threadIdx.x == 0 && state[s] != 2) partials[(size_t)s * gridDim.x + blockIdx.x] = tsum;
    }
}

// bicg_p_k for three systems; fold: bicg_xr3_k's partial sums, system s at fold + s * fold_count
__global__ __launch_bounds__(kBlock) void bicg_p3_k(double *__restrict__ scal3, int rho_prev_idx, int rho_idx, const double *__restrict__ r3,
                                                    const double *__restrict__ nu3, double *__restrict__ p3, int64_t n, int guard,
                                                    const double *__restrict__ fold, int fold_count) {
    __shared__ double lds16[3 * 16];
    const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * blockDim.x;
    double2 *p2 = reinterpret_cast<double2 *>(p3);
    const double2 *r2 = reinterpret_cast<const double2 *>(r3), *nu2 = reinterpret_cast<const double2 *>(nu3);
    double beta[3], omega[3];
    bool act[3];
    double folded[3] = {0., 0., 0.};
    if (fold_count) fold_partials_multi<3>(fold, fold_count, lds16, folded);
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const bool frz = bicg_frozen3(scal3, s, guard);
        const double rho = fold_count ? folded[s] : fold[s];
        const double rho_prev = scal3[SC3(rho_prev_idx, s)];
        const double alpha = rho_prev / scal3[SC3(S_SUM_NU, s)];
        omega[s] = scal3[SC3(S_TS, s)] / scal3[SC3(S_TT, s)];
        beta[s] = rho / rho_prev * alpha / omega[s];
        const bool bad = guard && !(finite_nonzero(omega[s]) && isfinite(beta[s]));
        act[s] = !frz && !bad;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (!frz) {
                scal3[SC3(rho_idx, s)] = rho;
                if (bad) scal3[SC3(S_FROZEN, s)] = 1.;
            } else if (scal3[SC3(S_FROZEN2, s)] != 0.) {
                scal3[SC3(S_FROZEN, s)] = 1.;  // see bicg_p_k
            }
        }
    }
    if (act[0] && act[1] && act[2]) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
            const double2 ra = r2[3 * i], rb = r2[3 * i + 1], rc = r2[3 * i + 2];
            const double2 pa = p2[3 * i], pb = p2[3 * i + 1], pc = p2[3 * i + 2];
            const double2 na = nu2[3 * i], nb = nu2[3 * i + 1], nc = nu2[3 * i + 2];
            p2[3 * i] = make_double2(ra.x + beta[0] * (pa.x - omega[0] * na.x), ra.y + beta[1] * (pa.y - omega[1] * na.y));
            p2[3 * i + 1] = make_double2(rb.x + beta[2] * (pb.x - omega[2] * nb.x), rb.y + beta[0] * (pb.y - omega[0] * nb.y));
            p2[3 * i + 2] = make_double2(rc.x + beta[1] * (pc.x - omega[1] * nc.x), rc.y + beta[2] * (pc.y - omega[2] * nc.y));
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int64_t e = 3 * (n - 1) + s;
                p3[e] = r3[e] + beta[s] * (p3[e] - omega[s] * nu3[e]);
            }
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (act[s]) p3[3 * e + s] = r3[3 * e + s] + beta[s] * (p3[3 * e + s] - omega[s] * nu3[3 * e + s]);
        }
    }
}

__global__ void guard_event3_k(const double *__restrict__ scal3, int *__restrict__ counter) {
    int c = 0;
    for (int s = 0; s < 3; ++s)
        if (scal3[SC3(S_FROZEN, s)] != 0. || scal3[SC3(S_FROZEN2, s)] != 0.) ++c;
    if (c) atomicAdd(counter, c);
}

int jacobi_scaling_prepare3_dev(const MatView3 &A_in, uint64_t iteration_count, Arena &arena, ScaledOperator3 &S) {
    const int64_t n = A_in.P.n;
    S = ScaledOperator3();
    S.A = A_in;
    S.iterations = iteration_count;
    if (n == 0) return ORC_OK;
    double *dinv3;
    ORC_TRY(arena.alloc((size_t)3 * (size_t)n, &dinv3));
    ORC_TRY(diag_inverse3_dev(A_in, dinv3));
    if (!S.A.s1) S.A.s1 = dinv3;
    else if (!S.A.s2) S.A.s2 = dinv3;
    else return set_error(ORC_ERR_BAD_ARGUMENT, "more than two nested Jacobi scalings");
    S.dinv3 = dinv3;
    return materialize_scaled_view3(S.A, iteration_count, arena);
}

int bicgstab3_scaled_dev(const ScaledOperator3 &S, const double *b3, double *x3, Arena &arena) {
    const int64_t n = S.A.P.n;
    if (n == 0) return ORC_OK;
    ArenaScope scope(arena);
    double *bt3;
    ORC_TRY(arena.alloc((size_t)3 * (size_t)n, &bt3));
    ORC_TRY(scale_vec_dev(S.dinv3, b3, bt3, 3 * n));  // :165
    return bicgstab3_dev(S.A, bt3, x3, S.iterations, ORC_PRECOND_NONE, arena);
}

int bicgstab3_dev(const MatView3 &A_in, const double *b3_in, double *x3, uint64_t iteration_count, int preconditioner, Arena &arena) {
    const int64_t n = A_in.P.n;
    if (n == 0) return ORC_OK;
    if (!triple_supported()) return set_error(ORC_ERR_BAD_ARGUMENT, "three-system solve: tree reductions only");
    ArenaScope scope(arena);
    const size_t n3 = (size_t)3 * (size_t)n;
    // partitioned operator (A.halo): the vectors that ENTER a product (x3 — the caller's —, p3, s3) carry their ghost entries:
    // 3 * ncols doubles; the three sums of an iteration are folded by one-workgroup launches and summed over the ranks by one
    // all-reduce each (reduce_partials: 3, 6 and 3 scalars) instead of being folded by their consumers
    const bool part = A_in.halo != nullptr && ctx().world > 1;
    const size_t nc3 = (size_t)3 * (size_t)std::max<int64_t>(A_in.P.ncols, n);
    MatView3 A = A_in;
    const double *b3 = b3_in;
    if (preconditioner == ORC_PRECOND_JACOBI) {  // :159-167, as iterative_solve_body does it
        double *dinv3, *bt3;
        ORC_TRY(arena.alloc(n3, &dinv3));
        ORC_TRY(arena.alloc(n3, &bt3));
        ORC_TRY(diag_inverse3_dev(A_in, dinv3));
        ORC_TRY(scale_vec_dev(dinv3, b3_in, bt3, (int64_t)n3));
        if (!A.s1) A.s1 = dinv3;
        else if (!A.s2) A.s2 = dinv3;
        else return set_error(ORC_ERR_BAD_ARGUMENT, "more than two nested Jacobi scalings");
        b3 = bt3;
    } else if (preconditioner != ORC_PRECOND_NONE) {
        return set_error(ORC_ERR_BAD_ARGUMENT, "unknown preconditioner %d", preconditioner);
    }
    ORC_TRY(materialize_scaled_view3(A, iteration_count, arena));
    double *r3, *p3, *nu3, *s3, *t3, *partials, *partials2, *scal3;
    double *sums;  // partitioned: the folded and all-reduced sums of the launch before (6 doubles)
    ORC_TRY(arena.alloc(n3, &r3));
    ORC_TRY(arena.alloc(nc3, &p3));
    ORC_TRY(arena.alloc(n3, &nu3));
    ORC_TRY(arena.alloc(nc3, &s3));
    ORC_TRY(arena.alloc(n3, &t3));
    ORC_TRY(arena.alloc((size_t)6 * kMaxPartials, &partials));
    ORC_TRY(arena.alloc((size_t)3 * kMaxPartials, &partials2));
    ORC_TRY(arena.alloc((size_t)3 * S_COUNT, &scal3));
    ORC_TRY(arena.alloc((size_t)8, &sums));
    hipStream_t st = ctx().stream;
    ORC_HIP(hipMemsetAsync(scal3, 0, 3 * S_COUNT * sizeof(double), st));
    const int guard = ctx().breakdown_guard ? 1 : 0;
    const int vg = grid_for((n + 1) / 2);
    int g = 0;
    ORC_TRY(product_residual3(A, x3, b3, r3, p3, partials, &g));  // r = b - A x ; p = r ; rho = sum(r)   (:250-254)
    ORC_TRY(reduce_partials(partials, g, 3, scal3 + SC3(S_RHO0, 0), part));
    for (uint64_t it = 0; it < iteration_count; ++it) {
        const int cur = (int)(it & 1), nxt = cur ^ 1;
        ORC_TRY(product_store_sum3(A, p3, nu3, partials, &g));                                           // nu = A p, sum(nu)   (:256-257)
        if (part) ORC_TRY(reduce_partials(partials, g, 3, sums, true));                                  // C2: one all-reduce for the three systems
        hipLaunchKernelGGL(bicg_s3_k, dim3(vg), dim3(kBlock), 0, st, scal3, S_RHO0 + cur, (const double *)r3, (const double *)nu3, s3, n, guard,
                           part ? (const double *)sums : (const double *)partials, part ? 0 : g);        // s = r - alpha nu    (:259)
        ORC_TRY(product_ts3(A, s3, t3, partials, &g));                                                   // t = A s, t.s, t.t   (:260-261)
        if (part) ORC_TRY(reduce_partials(partials, g, 6, sums, true));
        hipLaunchKernelGGL(bicg_xr3_k, dim3(vg), dim3(kBlock), 0, st, scal3, S_RHO0 + cur, x3, (const double *)p3, (const double *)s3, (const double *)t3, r3,
                           n, partials2, guard, part ? (const double *)sums : (const double *)partials, part ? 0 : g);  // x, r, sum(r)  (:258, :262-265)
        if (part) ORC_TRY(reduce_partials(partials2, vg, 3, sums, true));
        hipLaunchKernelGGL(bicg_p3_k, dim3(vg), dim3(kBlock), 0, st, scal3, S_RHO0 + cur, S_RHO0 + nxt, (const double *)r3, (const double *)nu3, p3, n,
                           guard, part ? (const double *)sums : (const double *)partials2, part ? 0 : vg);  // p                   (:266-267)
    }
    ORC_HIP(hipGetLastError());
    if (guard && ctx().guard_events) {
        hipLaunchKernelGGL(guard_event3_k, dim3(1), dim3(1), 0, st, (const double *)scal3, ctx().guard_events);
        ORC_HIP(hipGetLastError());
    }
    return ORC_OK;
}
#undef SC3

}  // namespace orc
