// jacobi.hip — the Jacobi arm of iterative_solve: sweep, residual and the reference's per-sweep bookkeeping on the
// device.  Reference: src/linear_algebra.rs:172-218.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "linalg_kernels.hpp"

namespace orc {

struct JacobiCtrl {
    int done;           // convergence break taken (:210-213)
    int status;         // sticky OrcStatus
    long long sweeps;   // sweeps executed
    double initial_residual;
    long long iter_num;
};

// x_new = omega * (b'_i - sum_j a'_ij x_j) + x_i (1 - omega), a' = offdiag(A)/diag(A), b' = b/diag(A);
// also flags NaN in the incoming x (:192-196)
__global__ __launch_bounds__(kBlock) void jacobi_sweep_k(MatView A, const double *__restrict__ b, const double *__restrict__ x,
                                                         double *__restrict__ x_new, double omega, JacobiCtrl *ctrl) {
    if (ctrl->done || ctrl->status) return;
    const int lane = threadIdx.x & 63;
    int saw_nan = 0;
    SliceWalk w(A.P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int64_t base = A.P.slice_ptr[slice];
        const int width = (int)((A.P.slice_ptr[slice + 1] - base) >> 6);
        const bool live = row < A.P.n;
        const int len = live ? A.P.row_len[row] : 0;
        double aii = 1.;
        if (live) {
            const int32_t d = A.P.diag_pos[row];
            if (d < 0) { atomicCAS(&ctrl->status, 0, (int)ORC_ERR_STRUCTURAL_ZERO); aii = 1.; }
            else aii = view_value(A, row, d);
        }
        double acc = 0.;
        for (int k = 0; k < width; ++k) {
            if (k < len) {
                const int64_t pos = base + (int64_t)k * 64 + lane;
                const int c = A.P.col[pos];
                const double v = (c == row) ? 0. : view_value(A, row, pos) / aii;  // :174-180
                acc += v * x[c];
            }
        }
        if (live) {
            const double xi = x[row];
            if (xi != xi) saw_nan = 1;
            const double bp = b[row] / aii;  // :181-187
            x_new[row] = omega * (bp - acc) + xi * (1. - omega);  // :199-200
        }
    }
    if (saw_nan) atomicCAS(&ctrl->status, 0, (int)ORC_ERR_JACOBI_NAN);
}

// partial sum((b - A x)^2) and max |x|  (:202-207)
__global__ __launch_bounds__(kBlock) void jacobi_residual_k(MatView A, const double *__restrict__ b, const double *__restrict__ x,
                                                            double *__restrict__ partials, JacobiCtrl *ctrl) {
    __shared__ double lds[8];
    if (ctrl->done || ctrl->status) return;
    const int lane = threadIdx.x & 63;
    double r2 = 0., mx = 0.;
    SliceWalk w(A.P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int64_t base = A.P.slice_ptr[slice];
        const int width = (int)((A.P.slice_ptr[slice + 1] - base) >> 6);
        const bool live = row < A.P.n;
        const int len = live ? A.P.row_len[row] : 0;
        double acc = 0.;
        for (int k = 0; k < width; ++k) {
            if (k < len) {
                const int64_t pos = base + (int64_t)k * 64 + lane;
                acc += view_value(A, row, pos) * x[A.P.col[pos]];
            }
        }
        if (live) {
            const double v = b[row] - acc;
            r2 += v * v;
            mx = max_nan(mx, fabs(x[row]));
        }
    }
    const double t = block_sum(r2, lds);
    const double m = block_max(mx, lds);
    if (threadIdx.x == 0) { partials[blockIdx.x] = t; partials[gridDim.x + blockIdx.x] = m; }
}

// fold the per-workgroup maxima (second partial array of jacobi_residual_k)
__global__ __launch_bounds__(1024) void reduce_max_k(const double *__restrict__ partials, int count, double *__restrict__ out) {
    __shared__ double lds[16];
    double v = 0.;
    for (int i = threadIdx.x; i < count; i += blockDim.x) v = max_nan(v, partials[i]);
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = lds[0];
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = max_nan(r, lds[i]);
        out[0] = r;
    }
}

// one thread: the reference's per-sweep bookkeeping (:208-216); red[0] = sum((b - A x)^2), red[1] = max |x| — NaN when x
// holds one: max_by(total_cmp) (:203-207) ranks NaN above everything, `NaN > 1e10` is false, and the next sweep's
// NaN check (:192-196) is what panics
__global__ void jacobi_control_k(const double *__restrict__ red, double threshold, JacobiCtrl *ctrl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ctrl->done || ctrl->status) return;
    const double r = sqrt(red[0]), mx = red[1];
    ctrl->sweeps += 1;
    const long long it = ctrl->iter_num;
    ctrl->iter_num = it + 1;
    if (it == 1) ctrl->initial_residual = r;
    else if (r / ctrl->initial_residual < threshold) { ctrl->done = 1; return; }
    if (mx > 1e10) ctrl->status = (int)ORC_ERR_JACOBI_TOO_LARGE;
}

int jacobi_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor,
                      double threshold, Arena &arena, SolveStats *stats, int *status_out) {
    const int64_t n = A.P.n;
    *status_out = ORC_OK;
    if (n == 0 || iteration_count == 0) return ORC_OK;
    ArenaScope scope(arena);
    double *x2, *partials, *red;
    JacobiCtrl *ctrl;
    const bool global = A.halo != nullptr;
    ORC_TRY(arena.alloc((size_t)std::max(A.P.ncols, n), &x2));
    ORC_TRY(arena.alloc((size_t)2 * kMaxPartials, &partials));
    ORC_TRY(arena.alloc((size_t)2, &red));
    ORC_TRY(arena.alloc((size_t)1, &ctrl));
    ORC_HIP(hipMemsetAsync(ctrl, 0, sizeof(JacobiCtrl), ctx().stream));
    const bool ref = reference_order(A);
    double *rvec = nullptr, *ref_partials = nullptr;
    if (ref) {
        ORC_TRY(arena.alloc((size_t)n, &rvec));
        ORC_TRY(arena.alloc((size_t)kMaxPartials, &ref_partials));
    }
    const int g = spmv_grid(A.P.n_slices);
    // Sweeps alternate x -> x2 -> x.  A sweep that is skipped (done/status set) leaves both
    // buffers untouched, so the newest iterate is in x2 iff the executed sweep count is odd.
    double *cur = x, *nxt = x2;
    for (uint64_t it = 0; it < iteration_count; ++it) {
        if (global) ORC_TRY(A.halo->exchange(cur));
        hipLaunchKernelGGL(jacobi_sweep_k, dim3(g), dim3(kBlock), 0, ctx().stream, A, b, cur, nxt, relaxation_factor, ctrl);
        if (global) ORC_TRY(A.halo->exchange(nxt));
        hipLaunchKernelGGL(jacobi_residual_k, dim3(g), dim3(kBlock), 0, ctx().stream, A, b, nxt, partials, ctrl);
        ORC_TRY(reduce_partials(partials, g, 1, red, global));
        if (ref) {  // |b - A x|^2 in nalgebra's association (:202); a sweep past the break recomputes a value nobody reads
            int g2 = 0;
            ORC_TRY(product_residual_norm(A, nxt, b, rvec, ref_partials, &g2, nullptr));
            ORC_TRY(dot_reference(rvec, rvec, n, red, nullptr));
        }
        hipLaunchKernelGGL(reduce_max_k, dim3(1), dim3(1024), 0, ctx().stream, partials + g, g, red + 1);
        if (global) ORC_TRY(comm_allreduce_max(red + 1, 1));
        hipLaunchKernelGGL(jacobi_control_k, dim3(1), dim3(1), 0, ctx().stream, red, threshold, ctrl);
        std::swap(cur, nxt);
    }
    ORC_HIP(hipGetLastError());
    JacobiCtrl h;
    ORC_HIP(hipMemcpyAsync(&h, ctrl, sizeof(h), hipMemcpyDeviceToHost, ctx().stream));
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    // the NaN check of the reference runs at the top of a sweep: a NaN seen by sweep k means
    // sweep k itself was still executed by the kernel above, but the reference panics before it.
    // Either way the call fails with "diverged"; the iterate is not observable after a panic.
    if (stats) stats->jacobi_sweeps = h.sweeps;
    // sweeps executed = h.sweeps, except that a sweep launched after a status was raised inside
    // jacobi_sweep_k (NaN / structural zero) has no matching control step.
    const bool newest_in_x2 = (h.sweeps & 1) != 0;
    if (newest_in_x2) ORC_TRY(vec_copy(x, x2, n));
    *status_out = h.status;
    return ORC_OK;
}

}  // namespace orc
