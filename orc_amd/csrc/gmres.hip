// gmres.hip — restarted GMRES(m) arm of iterative_solve (extension, no reference counterpart: ORC lists it as a TODO,
// lib.rs:170).  Semantics: include/orc_amd.h at orc_set_gmres_restart; numpy restatement: tests/gmres_restatement.py.
//
// One Arnoldi step j (w = v_{j+1} slot of the basis, nq = j + 1 basis vectors before it):
//   product     w = A v_j                                   product_store (spmv.hip), scalings / halo as every arm
//   dots        h1 = V^T w                                  gmres_dots_k          reads V (nq) + w         (j + 2) 8n bytes
//   update+dots w -= V h1 ; h2 = V^T w                      gmres_update_dots_k   reads V + w, writes w    (j + 3) 8n bytes
//   update+norm w -= V h2 ; |w|^2                           gmres_update_norm_k   reads V + w, writes w    (j + 3) 8n bytes
//   control     h = h1 + h2, Givens, stop test              gmres_ctrl_k          (one workgroup)
// The normalisation v_{j+1} = w / h_{j+1,j} is a scaling pass of its own (gmres_scale_k, 16n bytes): (3j + 10) 8n bytes per step
// besides the product.  gmres_update_dots_k stages the basis tile it subtracts in LDS and forms the second pass's dot products
// from there, so the basis comes from HBM once for both.  At the end of a cycle gmres_solve_y_k solves R y = g and
// gmres_update_norm_k (no norm) applies x += V y.
//
// Partial sums: one per workgroup and quantity, partials[q * grid + blockIdx.x], folded by reduce_partials in a fixed order
// (and all-reduced over the ranks of a partitioned operator): every rank computes the same Hessenberg and the same decisions.
// No float atomics, no host synchronisation inside the solve: the host queues every launch of iteration_count steps, and
// the device flags st[0] (stopped) / st[1] (finished: x is final) turn what follows a stop into no-ops (skip_flags
// convention of launch_spmv: two device doubles, non-zero = no-op).
#include <algorithm>
#include <cmath>

#include "linalg.hpp"

namespace orc {

constexpr int kGmresMaxRestart = 64;
constexpr int kGmresDefaultRestart = 30;
constexpr int kGmresQPerWave = kGmresMaxRestart / 4;  // basis vectors per wave in the dot-product kernels (4 waves per workgroup)
constexpr int kGmresTile = 128;                       // elements per workgroup tile of the dot-product kernels (64 lanes x double2)

// control block (device doubles)
enum {
    G_STOPPED = 0,   // a stop condition fired: the remaining steps and cycles are no-ops
    G_FINISHED = 1,  // x is final: the end-of-cycle update is a no-op too
    G_ZERO = 2,      // always 0 (second skip word of the end-of-cycle kernels)
    G_STEPS = 3, G_CYCLES = 4, G_BETA0 = 5, G_GEST = 6, G_EVENT = 7,
    G_INV = 8,       // 1 / beta or 1 / h_{j+1,j}: the scaling of the newest basis vector
    G_COLS = 9,      // columns of the cycle in progress
    G_COUNT = 16
};

static __device__ __forceinline__ bool gmres_skip(const double *f) { return f[0] != 0. || f[1] != 0.; }

// wave k of the workgroup owns the basis vectors q = k, k + 4, ...; its lane sums feed partials[q * gridDim.x + blockIdx.x]
static __device__ __forceinline__ void gmres_write_dots(const double (&acc)[kGmresQPerWave], int nq, double *__restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < kGmresQPerWave; ++t) {
        const int q = wave + 4 * t;
        if (q < nq) {
            const double s = wave_sum(acc[t]);
            if (lane == 0) partials[(size_t)q * gridDim.x + blockIdx.x] = s;
        }
    }
}

// partials of v_q . w, q < nq: tiles of 128 elements, lane l holds the pair (2l, 2l + 1) of the tile; w is read once per wave
__global__ __launch_bounds__(kBlock) void gmres_dots_k(const double *__restrict__ V, int64_t ld, int nq, const double *__restrict__ w,
                                                       int64_t n, double *__restrict__ partials, const double *__restrict__ skip) {
    if (gmres_skip(skip)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[kGmresQPerWave];
#pragma unroll
    for (int t = 0; t < kGmresQPerWave; ++t) acc[t] = 0.;
    for (int64_t base = (int64_t)blockIdx.x * kGmresTile; base < n; base += (int64_t)gridDim.x * kGmresTile) {
        const int64_t e = base + 2 * lane;
        const double2 wv = load2(w, e, n);
#pragma unroll
        for (int t = 0; t < kGmresQPerWave; ++t) {
            const int q = wave + 4 * t;
            if (q < nq) {
                const double2 v = load2(V + (size_t)q * ld, e, n);
                acc[t] += v.x * wv.x + v.y * wv.y;
            }
        }
    }
    gmres_write_dots(acc, nq, partials);
}

// w -= V c (c = the folded first-pass sums), then partials of v_q . w for the second pass.  The basis tile is staged in LDS
// while it is subtracted, so the dot products read it from there: one pass over the basis for both.  tile = 128 elements
// (64 when nq > 59: the LDS image stays under 64 KB); lds = nq * tile + 4 * tile + tile doubles.
__global__ __launch_bounds__(kBlock) void gmres_update_dots_k(const double *__restrict__ V, int64_t ld, int nq, double *__restrict__ w,
                                                              const double *__restrict__ c, int64_t n, int tile,
                                                              double *__restrict__ partials, const double *__restrict__ skip) {
    extern __shared__ __align__(16) double lds[];
    if (gmres_skip(skip)) return;
    double *lv = lds, *ls = lds + (size_t)nq * tile, *lw = ls + 4 * tile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pairs = tile / 2;
    const bool active = lane < pairs;
    double acc[kGmresQPerWave];
#pragma unroll
    for (int t = 0; t < kGmresQPerWave; ++t) acc[t] = 0.;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        const int64_t e = base + 2 * lane;
        // (a) each wave: its share of V c for the pair, the basis values into LDS
        double2 s = make_double2(0., 0.);
        if (active) {
#pragma unroll
            for (int t = 0; t < kGmresQPerWave; ++t) {
                const int q = wave + 4 * t;
                if (q < nq) {
                    const double2 v = load2(V + (size_t)q * ld, e, n);
                    const double cq = c[q];
                    s.x += cq * v.x;
                    s.y += cq * v.y;
                    *reinterpret_cast<double2 *>(lv + (size_t)q * tile + 2 * lane) = v;
                }
            }
            *reinterpret_cast<double2 *>(ls + wave * tile + 2 * lane) = s;
        }
        __syncthreads();
        // (b) wave 0: w' = w - (V c), four shares folded in a fixed order
        if (wave == 0 && active) {
            const double2 s0 = *reinterpret_cast<const double2 *>(ls + 2 * lane), s1 = *reinterpret_cast<const double2 *>(ls + tile + 2 * lane);
            const double2 s2 = *reinterpret_cast<const double2 *>(ls + 2 * tile + 2 * lane), s3 = *reinterpret_cast<const double2 *>(ls + 3 * tile + 2 * lane);
            double2 wv = load2(w, e, n);
            wv.x = wv.x - ((s0.x + s1.x) + (s2.x + s3.x));
            wv.y = wv.y - ((s0.y + s1.y) + (s2.y + s3.y));
            if (e >= n) wv.x = 0.;
            if (e + 1 >= n) wv.y = 0.;
            store2(w, e, n, wv);
            *reinterpret_cast<double2 *>(lw + 2 * lane) = wv;
        }
        __syncthreads();
        // (c) each wave: v_q . w' for its basis vectors, from LDS
        if (active) {
            const double2 wv = *reinterpret_cast<const double2 *>(lw + 2 * lane);
#pragma unroll
            for (int t = 0; t < kGmresQPerWave; ++t) {
                const int q = wave + 4 * t;
                if (q < nq) {
                    const double2 v = *reinterpret_cast<const double2 *>(lv + (size_t)q * tile + 2 * lane);
                    acc[t] += v.x * wv.x + v.y * wv.y;
                }
            }
        }
        __syncthreads();  // the tile's LDS is rewritten by the next one
    }
    gmres_write_dots(acc, nq, partials);
}

// w = w - sign * V c over the owned rows; with partials: the workgroup's partial sum of |w|^2.  sign = -1 with c = y is
// the end-of-cycle x += V y (st: the control block, whose column count bounds nq).  One double2 per lane, grid-stride.
__global__ __launch_bounds__(kBlock) void gmres_update_norm_k(const double *__restrict__ V, int64_t ld, int nq, double *__restrict__ w,
                                                              const double *__restrict__ c, double sign, int64_t n,
                                                              double *__restrict__ partials, const double *__restrict__ skip,
                                                              const double *__restrict__ st) {
    __shared__ double red[8];
    if (gmres_skip(skip)) return;
    if (st) nq = min(nq, (int)st[G_COLS]);  // x += V y: the columns the cycle computed (later slots were never written)
    double nrm = 0.;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; e < n; e += stride) {
        double sx = 0., sy = 0.;
        for (int q = 0; q < nq; ++q) {
            const double2 v = load2(V + (size_t)q * ld, e, n);
            const double cq = c[q];
            sx += cq * v.x;
            sy += cq * v.y;
        }
        double2 wv = load2(w, e, n);
        wv.x = wv.x - sign * sx;
        wv.y = wv.y - sign * sy;
        store2(w, e, n, wv);
        if (e + 1 >= n) wv.y = 0.;
        nrm += wv.x * wv.x + wv.y * wv.y;
    }
    if (partials) {
        const double t = block_sum(nrm, red);
        if (threadIdx.x == 0) partials[blockIdx.x] = t;
    }
}

// v *= st[G_INV] over the owned rows
__global__ __launch_bounds__(kBlock) void gmres_scale_k(double *__restrict__ v, const double *__restrict__ st, int64_t n,
                                                        const double *__restrict__ skip) {
    if (gmres_skip(skip)) return;
    const double s = st[G_INV];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 2;
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; e < n; e += stride) {
        double2 x = load2(v, e, n);
        x.x *= s;
        x.y *= s;
        store2(v, e, n, x);
    }
}

static __device__ __forceinline__ void gmres_stop(double *st, bool keep_x) {
    st[G_STOPPED] = 1.;
    if (keep_x) st[G_FINISHED] = 1.;
}

// start of a cycle: beta = sqrt(red[0]); g = (beta, 0, ...); 1 / beta for v_0
__global__ void gmres_cycle_k(double *__restrict__ st, const double *__restrict__ red, double *__restrict__ g, int m, int guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (gmres_skip(st)) return;
    const double beta = sqrt(red[0]);
    const bool first = st[G_CYCLES] == 0.;
    if (first) st[G_BETA0] = beta;
    st[G_GEST] = beta;
    st[G_COLS] = 0.;
    if (!isfinite(beta) && guard) {
        st[G_EVENT] = 1.;
        gmres_stop(st, true);  // x keeps the last completed cycle's value
        return;
    }
    // (no guard: a non-finite beta runs on into step 0, whose column is non-finite: the update applies it and NaN propagates)
    if (beta == 0.) { gmres_stop(st, true); return; }  // b - A x = 0: x stays as it is
    st[G_CYCLES] += 1.;
    for (int i = 0; i <= m; ++i) g[i] = 0.;
    g[0] = beta;
    st[G_INV] = 1. / beta;
}

// Arnoldi step j, after the three vector passes: column j of the Hessenberg (h = h1 + h2, h_{j+1,j} = |w|), the earlier
// rotations, the new one (hypot), g, and the stop tests.  H is column-major with m + 1 rows.
__global__ void gmres_ctrl_k(double *__restrict__ st, const double *__restrict__ h1, const double *__restrict__ h2, const double *__restrict__ nrm2,
                             double *__restrict__ Hm, double *__restrict__ cs, double *__restrict__ sn, double *__restrict__ g, int j, int m,
                             int last, double threshold, int guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (gmres_skip(st)) return;
    double *h = Hm + (size_t)j * (m + 1);
    double col2 = 0.;
    bool finite = true;
    for (int i = 0; i <= j; ++i) {
        const double v = h1[i] + h2[i];
        h[i] = v;
        col2 += v * v;
        finite = finite && isfinite(v);
    }
    const double hn = sqrt(nrm2[0]);
    h[j + 1] = hn;
    col2 += hn * hn;
    finite = finite && isfinite(hn);
    st[G_STEPS] += 1.;
    st[G_COLS] = j + 1;
    if (!finite) {
        if (guard) { st[G_EVENT] = 1.; gmres_stop(st, true); return; }  // x keeps the last completed cycle's value
        gmres_stop(st, false);  // no guard: the update runs with this column and NaN propagates
        st[G_GEST] = __builtin_nan("");
        return;
    }
    const bool happy = hn <= 1e-14 * sqrt(col2);
    for (int i = 0; i < j; ++i) {
        const double t = cs[i] * h[i] + sn[i] * h[i + 1];
        h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
        h[i] = t;
    }
    const double d = hypot(h[j], h[j + 1]);
    const double c = d == 0. ? 1. : h[j] / d, s = d == 0. ? 0. : h[j + 1] / d;
    cs[j] = c;
    sn[j] = s;
    h[j] = d;
    h[j + 1] = 0.;
    g[j + 1] = -s * g[j];
    g[j] = c * g[j];
    const double est = fabs(g[j + 1]);
    st[G_GEST] = est;
    st[G_INV] = 1. / hn;
    if (happy || (threshold > 0. && est <= threshold * st[G_BETA0]) || last) gmres_stop(st, false);
}

// end of a cycle: R y = g by back substitution over the cycle's columns; a stopped solve is finished after its update
__global__ void gmres_solve_y_k(double *__restrict__ st, const double *__restrict__ Hm, const double *__restrict__ g, double *__restrict__ y, int m) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[G_FINISHED] != 0.) return;
    const int k = (int)st[G_COLS];
    for (int i = k - 1; i >= 0; --i) {
        double s = g[i];
        for (int l = i + 1; l < k; ++l) s -= Hm[(size_t)l * (m + 1) + i] * y[l];
        y[i] = s / Hm[(size_t)i * (m + 1) + i];
    }
    for (int i = k; i < m; ++i) y[i] = 0.;
}

__global__ void gmres_finish_k(double *__restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[G_STOPPED] != 0.) st[G_FINISHED] = 1.;
}

__global__ void gmres_guard_event_k(const double *__restrict__ st, int *__restrict__ counter) {
    if (st[G_EVENT] != 0.) atomicAdd(counter, 1);
}

int gmres_dev(const MatView &A_in, const double *b, double *x, uint64_t iteration_count, double convergence_threshold, Arena &arena,
              SolveStats *stats) {
    const int restart = ctx().gmres_restart == 0 ? kGmresDefaultRestart : ctx().gmres_restart;
    if (restart < 1 || restart > kGmresMaxRestart)
        return set_error(ORC_ERR_BAD_ARGUMENT, "GMRES restart length %d outside 1..%d", ctx().gmres_restart, kGmresMaxRestart);
    const int64_t n = A_in.P.n;
    if (stats) { stats->gmres_steps = 0; stats->gmres_cycles = 0; stats->gmres_beta0 = 0.; stats->gmres_estimate = 0.; }
    if (n == 0 || iteration_count == 0) return ORC_OK;
    ArenaScope scope(arena);
    MatView A = A_in;
    ORC_TRY(materialize_scaled_view(A, iteration_count, arena));
    const int m = (int)std::min<uint64_t>((uint64_t)restart, iteration_count);
    const int64_t ld = (std::max(A.P.ncols, n) + 31) / 32 * 32;  // 256-byte aligned basis vectors, ghost entries included
    const bool global = A.halo != nullptr;
    const int guard = ctx().breakdown_guard ? 1 : 0;
    double *V, *partials, *red, *st, *Hm, *cs, *sn, *g, *y;
    ORC_TRY(arena.alloc((size_t)(m + 1) * ld, &V));
    ORC_TRY(arena.alloc((size_t)kGmresMaxRestart * kMaxPartials, &partials));
    ORC_TRY(arena.alloc((size_t)(2 * kGmresMaxRestart + 8), &red));
    ORC_TRY(arena.alloc((size_t)G_COUNT, &st));
    ORC_TRY(arena.alloc((size_t)(m + 1) * m, &Hm));
    ORC_TRY(arena.alloc((size_t)m, &cs));
    ORC_TRY(arena.alloc((size_t)m, &sn));
    ORC_TRY(arena.alloc((size_t)m + 1, &g));
    ORC_TRY(arena.alloc((size_t)m, &y));
    ORC_HIP(hipMemsetAsync(st, 0, G_COUNT * sizeof(double), ctx().stream));
    ORC_HIP(hipMemsetAsync(Hm, 0, (size_t)(m + 1) * m * sizeof(double), ctx().stream));
    double *h1 = red, *h2 = red + kGmresMaxRestart, *nrm2 = red + 2 * kGmresMaxRestart;
    const double *skip_step = st + G_STOPPED, *skip_end = st + G_FINISHED;
    hipStream_t s = ctx().stream;
    const int g_dots = grid_for(n, kGmresTile), g_vec = grid_for((n + 1) / 2);
    uint64_t left = iteration_count;
    while (left > 0) {
        const int k = (int)std::min<uint64_t>((uint64_t)m, left);
        left -= (uint64_t)k;
        int gr = 0;
        ORC_TRY(product_residual_norm(A, x, b, V, partials, &gr, skip_step));  // v_0 <- b - A x, partial |r|^2
        ORC_TRY(reduce_partials(partials, gr, 1, nrm2, global));
        hipLaunchKernelGGL(gmres_cycle_k, dim3(1), dim3(1), 0, s, st, nrm2, g, m, guard);
        hipLaunchKernelGGL(gmres_scale_k, dim3(g_vec), dim3(kBlock), 0, s, V, st, n, skip_step);
        for (int j = 0; j < k; ++j) {
            const int nq = j + 1;
            double *vj = V + (size_t)j * ld, *w = V + (size_t)(j + 1) * ld;
            ORC_TRY(product_store(A, vj, w, skip_step));
            hipLaunchKernelGGL(gmres_dots_k, dim3(g_dots), dim3(kBlock), 0, s, V, ld, nq, w, n, partials, skip_step);
            ORC_TRY(reduce_partials(partials, g_dots, nq, h1, global));
            const int tile = nq > 59 ? 64 : kGmresTile;
            const int g_ud = grid_for(n, tile);
            const size_t smem = sizeof(double) * (size_t)(nq * tile + 5 * tile);
            hipLaunchKernelGGL(gmres_update_dots_k, dim3(g_ud), dim3(kBlock), smem, s, V, ld, nq, w, h1, n, tile, partials, skip_step);
            ORC_TRY(reduce_partials(partials, g_ud, nq, h2, global));
            hipLaunchKernelGGL(gmres_update_norm_k, dim3(g_vec), dim3(kBlock), 0, s, V, ld, nq, w, h2, 1., n, partials, skip_step,
                               (const double *)nullptr);
            ORC_TRY(reduce_partials(partials, g_vec, 1, nrm2, global));
            hipLaunchKernelGGL(gmres_ctrl_k, dim3(1), dim3(1), 0, s, st, h1, h2, nrm2, Hm, cs, sn, g, j, m, (left == 0 && j == k - 1) ? 1 : 0,
                               convergence_threshold, guard);
            if (j + 1 < k) hipLaunchKernelGGL(gmres_scale_k, dim3(g_vec), dim3(kBlock), 0, s, w, st, n, skip_step);
        }
        hipLaunchKernelGGL(gmres_solve_y_k, dim3(1), dim3(1), 0, s, st, Hm, g, y, m);
        hipLaunchKernelGGL(gmres_update_norm_k, dim3(g_vec), dim3(kBlock), 0, s, V, ld, k, x, y, -1., n, (double *)nullptr, skip_end, st);
        hipLaunchKernelGGL(gmres_finish_k, dim3(1), dim3(1), 0, s, st);
        ORC_HIP(hipGetLastError());
    }
    if (guard && ctx().guard_events) {
        hipLaunchKernelGGL(gmres_guard_event_k, dim3(1), dim3(1), 0, s, st, ctx().guard_events);
        ORC_HIP(hipGetLastError());
    }
    double h[G_COUNT];
    ORC_HIP(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    ORC_HIP(hipStreamSynchronize(s));
    if (stats) {
        stats->gmres_steps = (int64_t)h[G_STEPS];
        stats->gmres_cycles = (int64_t)h[G_CYCLES];
        stats->gmres_beta0 = h[G_BETA0];
        stats->gmres_estimate = h[G_GEST];
    }
    return ORC_OK;
}

}  // namespace orc
