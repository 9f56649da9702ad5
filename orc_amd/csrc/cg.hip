// cg.hip — preconditioned conjugate-gradient arm of iterative_solve (extension, no reference counterpart) for symmetric positive
// definite systems: the pressure correction (discretization.rs:401-438) and pure-conduction scalar systems.  Semantics:
// include/orc_amd.h at orc_last_cg_stats; numpy restatement: tests/cg_restatement.py.
//
// CG does NOT test the symmetry of the values.  On a non-symmetric or indefinite matrix it runs until p.q <= 0 (event 1) or until the
// iterations are spent.
//
// The other arms apply the Jacobi preconditioner as the reference's left scaling D^-1 A, D^-1 b (linear_algebra.rs:159-167), which
// destroys symmetry; this arm is dispatched ahead of that block and applies M = D inside the recurrence: z = dinv * r.
//
// One iteration (n rows, 8-byte values):
//   product     q = A p, partial sums of p.q                          product_store_dot (spmv.hip), halo as every arm
//   cg_update_k folds p.q; alpha = rho / p.q; x += alpha p; r -= alpha q; z = dinv r; partial sums of r.z and r.r
//               reads x, p, r, q, dinv, writes x, r: 56 n bytes (48 n without a preconditioner)
//   cg_direction_k folds r.z and r.r; stop test; beta = rho' / rho; p = z + beta p
//               reads r, dinv, p, writes p: 32 n bytes (24 n without a preconditioner)
// Every workgroup folds the partial sums it consumes (fold_partials_block: the association of reduce_partials_k, so every workgroup
// holds the same bits and takes the same decision); workgroup 0 publishes scalars and flags.  For a partitioned operator the sums
// are folded by reduce_partials and all-reduced over the ranks instead, and the kernels read the scalars: every rank decides alike.
// No float atomics, no host synchronisation inside the solve: the host queues the launches of iteration_count iterations and the
// device flag st[C_STOPPED] turns what follows a stop into no-ops (skip_flags convention of launch_spmv: two device doubles,
// non-zero = no-op).  A kernel that raises the flag reacts by doing nothing itself, so a workgroup that starts late and sees the
// flag behaves like one that evaluated the test.  That holds per workgroup only: the launch that raises the flag may still have
// workgroups starting (the grid of 2048 is not all resident above about 650 k rows), and waves of one workgroup reading the flag
// on their own could disagree, leaving the fold's barriers and LDS slots to a part of the workgroup.  So one thread reads the flag
// into LDS and the workgroup acts on it after a barrier (stopped_publish, stopped_agreed).  rho lives in two slots by iteration parity:
// cg_direction_k reads the one and writes the other.
#include <algorithm>
#include <cmath>

#include "linalg_kernels.hpp"

namespace orc {

// control block (device doubles)
enum {
    C_STOPPED = 0,  // a stop condition fired: every later launch is a no-op
    C_ZERO = 1,     // always 0 (second skip word)
    C_ITERS = 2, C_BETA0 = 3, C_RES = 4, C_EVENT = 5,
    C_RHO0 = 6, C_RHO1 = 7,  // r.z of the iteration in progress: slot C_RHO0 + (iteration & 1)
    C_PQ = 8,                // partitioned operators: the all-reduced p.q
    C_RZ = 9, C_RR = 10,     // ... r.z and r.r (adjacent: one reduce_partials of two quantities)
    C_COUNT = 16
};

// The stop flag as the whole workgroup sees it: thread 0's read, published through LDS.  Call stopped_publish first, issue whatever
// loads should overlap its round trip, then stopped_agreed (a barrier: every thread of the workgroup must reach it).
__device__ __forceinline__ void stopped_publish(const double *st, int *flag_lds) {
    if (threadIdx.x == 0) *flag_lds = st[C_STOPPED] != 0. ? 1 : 0;
}
__device__ __forceinline__ bool stopped_agreed(const int *flag_lds) {
    __syncthreads();
    return *flag_lds != 0;
}

// dinv = 1 / diag(A).  A missing, zero or non-finite diagonal entry: *status = ORC_ERR_STRUCTURAL_ZERO and the solve is stopped before
// it touches x.
__global__ __launch_bounds__(kBlock) void cg_diag_inverse_k(MatView A, double *__restrict__ dinv, double *__restrict__ st, int *__restrict__ status) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = A.P.diag_pos[r];
        const double v = d >= 0 ? A.val[d] : 0.;
        const bool ok = v != 0. && isfinite(v);
        dinv[r] = ok ? 1. / v : 0.;
        if (!ok) {
            atomicCAS(status, 0, (int)ORC_ERR_STRUCTURAL_ZERO);
            st[C_STOPPED] = 1.;
        }
    }
}

// start: p = z = dinv r (dinv null: z = r), partial sums of r.z
__global__ __launch_bounds__(kBlock) void cg_start_k(const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ p, int64_t n,
                                                     double *__restrict__ partials) {
    __shared__ double red[8];
    double rz = 0.;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; e < n; e += stride) {
        const double2 rv = load2(r, e, n);
        double2 z = rv;
        if (dinv) {
            const double2 d = load2(dinv, e, n);
            z.x = d.x * rv.x;
            z.y = d.y * rv.y;
        }
        store2(p, e, n, z);
        rz += rv.x * z.x + rv.y * z.y;
    }
    const double t = block_sum(rz, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// beta0 = sqrt(r.r); a zero beta0 stops the solve with x untouched, a non-finite one is event 2
__global__ void cg_begin_k(double *__restrict__ st, const double *__restrict__ rr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[C_STOPPED] != 0.) return;
    const double beta0 = sqrt(rr[0]);
    st[C_BETA0] = beta0;
    st[C_RES] = beta0;
    if (!isfinite(beta0)) { st[C_EVENT] = 2.; st[C_STOPPED] = 1.; }
    else if (beta0 == 0.) st[C_STOPPED] = 1.;
}

// alpha = rho / p.q ; x += alpha p ; r -= alpha q ; z = dinv r ; partial sums of r.z (partials[blockIdx.x]) and r.r
// (partials[gridDim.x + blockIdx.x]).  fold (null: st[C_PQ] holds the sum already): the product's partial sums of p.q.
__global__ __launch_bounds__(kBlock) void cg_update_k(double *__restrict__ st, int rho_idx, double *__restrict__ x, const double *__restrict__ p,
                                                      double *__restrict__ r, const double *__restrict__ q, const double *__restrict__ dinv, int64_t n,
                                                      double *__restrict__ partials, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds16[16];
    __shared__ double red[8];
    __shared__ int stopped;
    stopped_publish(st, &stopped);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    // the first pairs of every thread are requested before the flag is agreed and the sums folded (their round trips overlap)
    double2 xv = load2(x, e, n), pv = load2(p, e, n), rv = load2(r, e, n), qv = load2(q, e, n);
    double2 dv = dinv ? load2(dinv, e, n) : make_double2(1., 1.);
    if (stopped_agreed(&stopped)) return;
    const double pq = fold ? fold_partials_block(fold, fold_count, lds16) : st[C_PQ];
    const double rho = st[rho_idx];
    const double alpha = rho / pq;
    const bool nonfinite = !(isfinite(rho) && isfinite(pq)) || (pq > 0. && !isfinite(alpha));
    if (nonfinite || pq <= 0.) {  // x keeps the last completed iterate
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st[C_EVENT] = nonfinite ? 2. : 1.;
            st[C_STOPPED] = 1.;
        }
        return;
    }
    double rz = 0., rr = 0.;
    while (e < n) {
        const int64_t nx = e + stride;
        double2 xn = make_double2(0., 0.), pn = xn, rn = xn, qn = xn, dn = make_double2(1., 1.);
        if (nx < n) {
            xn = load2(x, nx, n); pn = load2(p, nx, n); rn = load2(r, nx, n); qn = load2(q, nx, n);
            if (dinv) dn = load2(dinv, nx, n);
        }
        store2(x, e, n, make_double2(xv.x + alpha * pv.x, xv.y + alpha * pv.y));
        const double2 rw = make_double2(rv.x - alpha * qv.x, rv.y - alpha * qv.y);  // (past n: 0 - alpha * 0)
        store2(r, e, n, rw);
        const double2 z = dinv ? make_double2(dv.x * rw.x, dv.y * rw.y) : rw;
        rz += rw.x * z.x + rw.y * z.y;
        rr += rw.x * rw.x + rw.y * rw.y;
        xv = xn; pv = pn; rv = rn; qv = qn; dv = dn; e = nx;
    }
    const double t0 = block_sum(rz, red);
    const double t1 = block_sum(rr, red + 4);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t0;
        partials[gridDim.x + blockIdx.x] = t1;
    }
}

// rho' = r.z, |r| = sqrt(r.r); the iteration counts; stop test; p = z + (rho' / rho) p.
// fold (null: st[C_RZ], st[C_RR] hold the sums already): cg_update_k's partial sums, two quantities of fold_count each.
__global__ __launch_bounds__(kBlock) void cg_direction_k(double *__restrict__ st, int rho_idx, int rho_next_idx, const double *__restrict__ r,
                                                         const double *__restrict__ dinv, double *__restrict__ p, int64_t n, double threshold, int last,
                                                         const double *__restrict__ fold, int fold_count) {
    __shared__ double lds32[32];
    __shared__ int stopped;
    stopped_publish(st, &stopped);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    double2 rv = load2(r, e, n), pv = load2(p, e, n);  // requested before the flag is agreed and the sums folded
    double2 dv = dinv ? load2(dinv, e, n) : make_double2(1., 1.);
    if (stopped_agreed(&stopped)) return;
    double rz, rr;
    if (fold) {
        double both[2];
        fold_partials_multi<2>(fold, fold_count, lds32, both);
        rz = both[0]; rr = both[1];
    } else {
        rz = st[C_RZ]; rr = st[C_RR];
    }
    const double res = sqrt(rr);
    const bool nonfinite = !(isfinite(rz) && isfinite(rr));
    const bool stop = nonfinite || (threshold > 0. && res <= threshold * st[C_BETA0]) || last != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[C_ITERS] += 1.;
        st[C_RES] = res;
        st[rho_next_idx] = rz;
        if (nonfinite) st[C_EVENT] = 2.;
        if (stop) st[C_STOPPED] = 1.;
    }
    if (stop) return;
    const double beta = rz / st[rho_idx];
    while (e < n) {
        const int64_t nx = e + stride;
        double2 rn = make_double2(0., 0.), pn = rn, dn = make_double2(1., 1.);
        if (nx < n) {
            rn = load2(r, nx, n); pn = load2(p, nx, n);
            if (dinv) dn = load2(dinv, nx, n);
        }
        const double2 z = dinv ? make_double2(dv.x * rv.x, dv.y * rv.y) : rv;
        store2(p, e, n, make_double2(z.x + beta * pv.x, z.y + beta * pv.y));
        rv = rn; pv = pn; dv = dn; e = nx;
    }
}

int cg_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double convergence_threshold, int preconditioner, Arena &arena,
           SolveStats *stats) {
    if (stats) { stats->cg_iterations = 0; stats->cg_beta0 = 0.; stats->cg_residual = 0.; stats->cg_event = 0; }
    if (preconditioner != ORC_PRECOND_NONE && preconditioner != ORC_PRECOND_JACOBI)
        return set_error(ORC_ERR_BAD_ARGUMENT, "unknown preconditioner %d", preconditioner);
    if (A.s1 || A.s2) return set_error(ORC_ERR_BAD_ARGUMENT, "CG on a row-scaled view: the scaled operator is not symmetric");
    const int64_t n = A.P.n;
    // iteration_count is the same on every rank.  n == 0 leaves ahead of every collective, as in launch_spmv (ahead of its halo
    // exchange) and bicgstab_dev: a partitioned operator owns rows on every rank, the library has no path for a rank without.
    if (n == 0 || iteration_count == 0) return ORC_OK;
    ArenaScope scope(arena);
    const size_t nn = (size_t)std::max(A.P.ncols, n);  // p is multiplied: ghost entries included
    const bool jacobi = preconditioner == ORC_PRECOND_JACOBI;
    const bool global = A.halo != nullptr;
    double *r, *p, *q, *dinv = nullptr, *pq_partials, *partials, *st;
    int *status;
    ORC_TRY(arena.alloc((size_t)n, &r));
    ORC_TRY(arena.alloc(nn, &p));
    ORC_TRY(arena.alloc((size_t)n, &q));
    if (jacobi) ORC_TRY(arena.alloc((size_t)n, &dinv));
    ORC_TRY(arena.alloc((size_t)kMaxPartials, &pq_partials));
    ORC_TRY(arena.alloc((size_t)2 * kMaxPartials, &partials));
    ORC_TRY(arena.alloc((size_t)C_COUNT, &st));
    ORC_TRY(arena.alloc((size_t)2, &status));
    hipStream_t s = ctx().stream;
    ORC_HIP(hipMemsetAsync(st, 0, C_COUNT * sizeof(double), s));
    ORC_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int), s));
    const double *skip = st + C_STOPPED;
    const int g_vec = grid_for((n + 1) / 2);  // two elements per lane
    if (jacobi) hipLaunchKernelGGL(cg_diag_inverse_k, dim3(grid_for(n)), dim3(kBlock), 0, s, A, dinv, st, status);
    int g = 0;
    ORC_TRY(product_residual_norm(A, x, b, r, partials, &g, skip));  // r = b - A x, partial |r|^2
    ORC_TRY(reduce_partials(partials, g, 1, st + C_RR, global));
    hipLaunchKernelGGL(cg_begin_k, dim3(1), dim3(1), 0, s, st, st + C_RR);
    hipLaunchKernelGGL(cg_start_k, dim3(g_vec), dim3(kBlock), 0, s, r, dinv, p, n, partials);
    ORC_TRY(reduce_partials(partials, g_vec, 1, st + C_RHO0, global));
    for (uint64_t it = 0; it < iteration_count; ++it) {
        const int cur = C_RHO0 + (int)(it & 1), nxt = C_RHO0 + (int)((it & 1) ^ 1);
        ORC_TRY(product_store_dot(A, p, q, pq_partials, &g, skip));
        if (global) ORC_TRY(reduce_partials(pq_partials, g, 1, st + C_PQ, true));
        hipLaunchKernelGGL(cg_update_k, dim3(g_vec), dim3(kBlock), 0, s, st, cur, x, p, r, q, dinv, n, partials,
                           global ? (const double *)nullptr : (const double *)pq_partials, g);
        if (global) ORC_TRY(reduce_partials(partials, g_vec, 2, st + C_RZ, true));
        hipLaunchKernelGGL(cg_direction_k, dim3(g_vec), dim3(kBlock), 0, s, st, cur, nxt, r, dinv, p, n, convergence_threshold,
                           it + 1 == iteration_count ? 1 : 0, global ? (const double *)nullptr : (const double *)partials, g_vec);
        ORC_HIP(hipGetLastError());
    }
    double h[C_COUNT];
    int hs = 0;
    ORC_HIP(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    ORC_HIP(hipMemcpyAsync(&hs, status, sizeof(int), hipMemcpyDeviceToHost, s));
    ORC_HIP(hipStreamSynchronize(s));
    if (hs != ORC_OK) return set_error(hs, "CG with the Jacobi preconditioner: a diagonal entry is missing, zero or non-finite");
    SolveStats &last = last_stats();
    last.cg_iterations = (int64_t)h[C_ITERS];
    last.cg_beta0 = h[C_BETA0];
    last.cg_residual = h[C_RES];
    last.cg_event = (int)h[C_EVENT];
    if (stats && stats != &last) {
        stats->cg_iterations = last.cg_iterations; stats->cg_beta0 = last.cg_beta0; stats->cg_residual = last.cg_residual;
        stats->cg_event = last.cg_event;
    }
    return ORC_OK;
}

}  // namespace orc
