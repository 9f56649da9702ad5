// gs_sweep.hip — the multicolour Gauss-Seidel sweep over the colour-sorted matrix, the GS-preconditioned BiCGSTAB in row space
// (partitioned operators, ORC_GS_SLOTSPACE=0) and the Gauss-Seidel arm of iterative_solve (gs.hpp).
#include <cmath>

#include "gs.hpp"

namespace orc {

// Row update of the reference's Gauss-Seidel arm (linear_algebra.rs:225-239) for the slices [slice_lo, slice_hi) of one colour,
// one lane per slot:
//   x_i = x_i (1 - w) + w (b_i - sum_{j != i} a_ij x_j) / a_ii ,  the j == i term contributing the literal 0.
// A row without a diagonal: get(i, i) panics (lib.rs:664); an EMPTY row (coarse AMG row whose fine rows found no partner) has
// nothing to relax.
__global__ __launch_bounds__(kBlock) void gs_color_sorted_k(const int64_t *__restrict__ sp, const int *__restrict__ row_len, const int *__restrict__ rowid,
                                                            const int *__restrict__ diag_off, const int *__restrict__ col, const double *__restrict__ val,
                                                            const double *__restrict__ b, double *__restrict__ x, int slice_lo, int slice_hi, double omega,
                                                            int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    for (int sidx = slice_lo + blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); sidx < slice_hi; sidx += gridDim.x * waves) {  // (scalar: see SliceWalk)
        const int64_t slot = (int64_t)sidx * 64 + lane;
        const int i = rowid[slot];
        const int len = i >= 0 ? row_len[slot] : 0;
        const int64_t base = sp[sidx] + lane;
        const int width = (int)((sp[sidx + 1] - sp[sidx]) >> 6);
        double sum = 0.;
        // chunks of 8 like the product: column and value loads first, then the x gathers, then the ordered additions
        for (int k0 = 0; k0 < width; k0 += 8) {
            int c[8];
            double v[8], xv[8];
            const int64_t p0 = base + (int64_t)k0 * 64;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = k0 + u < len;
                c[u] = in ? col[p0 + (int64_t)u * 64] : 0;
                v[u] = in ? val[p0 + (int64_t)u * 64] : 0.;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) xv[u] = (k0 + u < len) ? x[c[u]] : 0.;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < len) sum += (c[u] == i) ? 0. : v[u] * xv[u];
        }
        if (i < 0) continue;
        const int d = diag_off[slot];
        if (d < 0) {
            if (len > 0) atomicCAS(status, 0, (int)ORC_ERR_STRUCTURAL_ZERO);
            continue;
        }
        const double xi = x[i] * (1. - omega) + omega * (b[i] - sum) / val[d];
        x[i] = xi;
        if (xi != xi) atomicCAS(status, 0, (int)ORC_ERR_SOLUTION_DIVERGED);  // :240-242
    }
}

// one sweep: a launch per colour
static int gs_sweep(const Coloring &C, const double *val, const double *b, double *x, double omega, int *status) {
    const SortedLayout &L = C.layout;
    for (int c = 0; c < C.n_colors; ++c) {
        const int lo = C.color_slice[(size_t)c], hi = C.color_slice[(size_t)c + 1];
        if (hi <= lo) continue;
        const int g = std::min(kMaxGrid, (hi - lo + 3) / 4);
        hipLaunchKernelGGL(gs_color_sorted_k, dim3(g), dim3(kBlock), 0, ctx().stream, L.sp, L.row_len, L.rowid, L.diag_off, L.col, val, b, x, lo, hi, omega, status);
    }
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// Right-preconditioned recurrences with the same breakdown guard as the reference arm (bicgstab.hip): scal[5] / scal[6]
// are the frozen flags (5: set by kernels that react with a no-op, 6: by the x/r update).
__device__ __forceinline__ bool pre_frozen(const double *scal, int guard) { return guard && (scal[5] != 0. || scal[6] != 0.); }

// x = (x + alpha p^) + omega s^ ; r = s - omega t ; partial sum(r)
__global__ __launch_bounds__(kBlock) void bicg_xr_pre_k(double *__restrict__ scal, int rho_idx, int i_sum_nu, int i_ts, int i_tt, double *__restrict__ x,
                                                        const double *__restrict__ ph, const double *__restrict__ sh, const double *__restrict__ s,
                                                        const double *__restrict__ t, double *__restrict__ r, int64_t n, double *__restrict__ partials, int guard) {
    __shared__ double lds[8];
    if (guard && scal[5] != 0.) return;
    const double alpha = scal[rho_idx] / scal[i_sum_nu];
    double omega = scal[i_ts] / scal[i_tt];
    const bool bad = guard && !(fin_nz(scal[i_tt]) && isfinite(omega));
    if (bad) omega = 0.;
    double acc = 0.;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double h = x[i] + alpha * ph[i];
        x[i] = bad ? h : h + omega * sh[i];
        const double ri = bad ? s[i] : s[i] - omega * t[i];
        r[i] = ri;
        acc += ri;
    }
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) scal[6] = 1.;
    const double tsum = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = tsum;
}
__global__ void bicg_s_pre_k(double *__restrict__ scal, int rho_idx, int i_sum_nu, const double *__restrict__ r, const double *__restrict__ nu,
                             double *__restrict__ s, int64_t n, int guard) {
    if (pre_frozen(scal, guard)) return;
    const double alpha = scal[rho_idx] / scal[i_sum_nu];
    if (guard && !(fin_nz(scal[rho_idx]) && fin_nz(scal[i_sum_nu]) && isfinite(alpha))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[5] = 1.;
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s[i] = r[i] - alpha * nu[i];
}
__global__ void bicg_p_pre_k(double *__restrict__ scal, int rho_prev_idx, int rho_idx, int i_sum_nu, int i_ts, int i_tt, const double *__restrict__ r,
                             const double *__restrict__ nu, double *__restrict__ p, int64_t n, int guard) {
    if (pre_frozen(scal, guard)) return;
    const double rho_prev = scal[rho_prev_idx], rho = scal[rho_idx];
    const double alpha = rho_prev / scal[i_sum_nu];
    const double omega = scal[i_ts] / scal[i_tt];
    const double beta = rho / rho_prev * alpha / omega;
    if (guard && !(fin_nz(omega) && isfinite(beta))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) scal[5] = 1.;
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = r[i] + beta * (p[i] - omega * nu[i]);
}
struct EpiSum {  // y = A x ; partial sum(y)
    static constexpr int kReductions = 1;
    double *y;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const { y[row] = acc; r0 += acc; }
};
struct EpiTsPre {  // t = A s^ ; partials t.s, t.t  (s is the un-preconditioned residual)
    static constexpr int kReductions = 2;
    const double *s;
    double *t;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &r1) const { t[row] = acc; r0 += acc * s[row]; r1 += acc * acc; }
};
struct EpiRes {  // r = b - A x ; p = r ; partial sum(r)
    static constexpr int kReductions = 1;
    const double *b;
    double *r, *p;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const { const double v = b[row] - acc; r[row] = v; p[row] = v; r0 += v; }
};

// (not the named products of arms.hpp: they choose other kernels and grids by the view, and the partial sums would group differently)
template <class Epi>
static int spmv_launch(const MatView &A, const double *x, const Epi &epi, double *partials, int *grid_out, const double *skip = nullptr) {
    const int g = spmv_grid(A.P.n_slices);
    *grid_out = g;
    if (A.halo) ORC_TRY(A.halo->exchange(const_cast<double *>(x)));  // C1: refresh the ghost entries of x
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_k<Epi>), dim3((unsigned)g), dim3(kBlock), 0, ctx().stream, A, x, epi, partials, skip);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int gs_arm_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor, int method, Arena &arena) {
    const int64_t n = A.P.n;
    if (n == 0) return ORC_OK;
    // Partitioned operator: every rank colours and sweeps its own rows; the ghost entries of the swept vector are refreshed
    // once per sweep, so rows along a cut see their remote neighbours as of the previous sweep (processor-block
    // Gauss-Seidel: Gauss-Seidel inside a rank, Jacobi across the cuts).  Reductions are summed over the ranks.
    const bool global = A.halo != nullptr && ctx().world > 1;
    hipStream_t st = ctx().stream;
    std::unique_ptr<Coloring> owned;
    const Coloring *C = nullptr;
    const double *val = nullptr;  // the matrix in colour-sorted storage: the pattern's layout + this solve's values
    ArenaScope scope(arena);
    ORC_TRY(gs_prepare(A, arena, owned, &C, &val));
    int *status;
    ORC_TRY(arena.alloc((size_t)1, &status));
    ORC_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    if (method == ORC_SOLVER_MULTICOLOR_GS) {
        for (uint64_t it = 0; it < iteration_count; ++it) {
            if (A.halo) ORC_TRY(A.halo->exchange(x));
            ORC_TRY(gs_sweep(*C, val, b, x, relaxation_factor, status));
        }
    } else if (!global && gs_slot_space_enabled()) {  // the same recurrences in slot space (single GPU)
        ORC_TRY(gsx_bicgstab1(*C, val, b, x, iteration_count, arena, status));
    } else {  // ORC_SOLVER_BICGSTAB_GS_PRECOND: linear_algebra.rs:247-269 with p^ = M^-1 p, s^ = M^-1 s, M^-1 = one GS sweep from 0
        const size_t nn = (size_t)std::max(A.P.ncols, n);  // products gather ghost entries of p^ and s^
        double *r, *p, *nu, *s, *t, *ph, *sh, *partials, *scal;
        ORC_TRY(arena.alloc(nn, &r)); ORC_TRY(arena.alloc(nn, &p)); ORC_TRY(arena.alloc(nn, &nu)); ORC_TRY(arena.alloc(nn, &s));
        ORC_TRY(arena.alloc(nn, &t)); ORC_TRY(arena.alloc(nn, &ph)); ORC_TRY(arena.alloc(nn, &sh));
        ORC_TRY(arena.alloc((size_t)2 * kMaxPartials, &partials));
        ORC_TRY(arena.alloc((size_t)8, &scal));
        enum { RHO0 = 0, RHO1 = 1, SUM_NU = 2, TS = 3, TT = 4 };
        ORC_HIP(hipMemsetAsync(scal, 0, 8 * sizeof(double), st));
        const int guard = ctx().breakdown_guard ? 1 : 0;
        const double *skip = guard ? scal + 5 : nullptr;
        const int vg = grid_for(n);
        int g = 0;
        ORC_TRY(spmv_launch(A, x, EpiRes{b, r, p}, partials, &g));
        ORC_TRY(reduce_partials(partials, g, 1, scal + RHO0, global));
        for (uint64_t it = 0; it < iteration_count; ++it) {
            const int cur = (int)(it & 1), nxt = cur ^ 1;
            ORC_TRY(vec_fill(ph, 0., (int64_t)nn));  // ghost entries too: the preconditioner is rank-local
            ORC_TRY(gs_sweep(*C, val, p, ph, 1.0, status));
            ORC_TRY(spmv_launch(A, ph, EpiSum{nu}, partials, &g, skip));
            ORC_TRY(reduce_partials(partials, g, 1, scal + SUM_NU, global));
            hipLaunchKernelGGL(bicg_s_pre_k, dim3(vg), dim3(kBlock), 0, st, scal, RHO0 + cur, SUM_NU, r, nu, s, n, guard);
            ORC_TRY(vec_fill(sh, 0., (int64_t)nn));
            ORC_TRY(gs_sweep(*C, val, s, sh, 1.0, status));
            ORC_TRY(spmv_launch(A, sh, EpiTsPre{s, t}, partials, &g, skip));
            ORC_TRY(reduce_partials(partials, g, 2, scal + TS, global));
            hipLaunchKernelGGL(bicg_xr_pre_k, dim3(vg), dim3(kBlock), 0, st, scal, RHO0 + cur, SUM_NU, TS, TT, x, ph, sh, s, t, r, n, partials, guard);
            ORC_TRY(reduce_partials(partials, vg, 1, scal + RHO0 + nxt, global));
            hipLaunchKernelGGL(bicg_p_pre_k, dim3(vg), dim3(kBlock), 0, st, scal, RHO0 + cur, RHO0 + nxt, SUM_NU, TS, TT, r, nu, p, n, guard);
            ORC_HIP(hipGetLastError());
        }
    }
    int h = 0;
    ORC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    return method == ORC_SOLVER_MULTICOLOR_GS ? h : (h == ORC_ERR_STRUCTURAL_ZERO ? h : ORC_OK);
}

// bench.py (BASELINE configs[2]): one multicolour sweep = C->n_colors launches of gs_color_sorted_k over the colour-sorted matrix,
// `reps` sweeps between two HIP events on the library stream; x = M^-1 b from zero, as the preconditioner application does it.
int bench_gs_sweep_dev(const MatView &A, const double *b, double *x, int reps, Arena &arena, float *ms_per_sweep, int *n_colors) {
    const int64_t n = A.P.n;
    if (n == 0) return ORC_OK;
    std::unique_ptr<Coloring> owned;
    const Coloring *C = nullptr;
    const double *val = nullptr;
    ArenaScope scope(arena);
    ORC_TRY(gs_prepare(A, arena, owned, &C, &val));
    int *status;
    ORC_TRY(arena.alloc((size_t)1, &status));
    ORC_HIP(hipMemsetAsync(status, 0, sizeof(int), ctx().stream));
    if (n_colors) *n_colors = C->n_colors;
    ORC_TRY(vec_fill(x, 0., std::max(A.P.ncols, n)));
    return timed(reps, [&] { return gs_sweep(*C, val, b, x, 1.0, status); }, ms_per_sweep);
}

}  // namespace orc
