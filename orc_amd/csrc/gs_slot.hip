// gs_slot.hip — the GS-preconditioned BiCGSTAB in slot space, S systems in lock-step (gs.hpp)
#include <cmath>

#include "gs.hpp"

namespace orc {

// BASELINE configs[2] (1.03 M cells): r03's solve spent 54 % of its kernel time in 10-microsecond colour launches at 0.2 of peak,
// another 12 % in one-workgroup folds and zero fills, and ran u, v, w as three such chains.  Here the whole solve lives in the
// colour-sorted numbering ("slots"): the vectors are permuted once on the way in and out, products and sweeps gather through the
// slot of a column (SortedLayout::cslot) — still adding a row's entries in their original ascending-column order, so every row sum has
// its bits — and
//   * the preconditioner application x^ = M^-1 b (one sweep from zero, omega = 1) needs no zero fill: a colour's kernel knows that
//     every column of its own or a later colour still holds the zero of the start (a slot compare against the colour's first slot),
//     skips those gathers, and their products — exact zeros that leave the running sum unchanged — with them;
//   * the three sums of an iteration are folded by the kernels that consume them (fold_partials_block, as in the reference arm);
//   * S = 3: the momentum systems share the mesh pattern, so one launch serves u, v and w — interleaved vectors x[3 slot + s], three
//     value streams, one column stream: a third of the launches, three times the work per launch of these latency-bound kernels.
// Per system the arithmetic of S = 3 is that of S = 1 (same grids, same thread -> slot map, same folds): bit-identical (tests).
template <int S> struct SlotMat {
    const int64_t *sp;
    const int *row_len, *rowid, *diag_off, *cslot;
    const double *val[S];
    int n_slices;
    int64_t n_slots;
};
template <int S> struct CVecs { const double *p[S]; };
template <int S> struct MVecs { double *p[S]; };
enum { GX_RHO0 = 0, GX_RHO1 = 1, GX_SUM_NU = 2, GX_TS = 3, GX_TT = 4, GX_FROZEN = 5, GX_FROZEN2 = 6, GX_STRIDE = 8 };

template <int S>
__global__ void gsx_in_k(const int *__restrict__ rowid, int64_t n_slots, CVecs<S> src, double *__restrict__ dst) {
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < n_slots; slot += (int64_t)gridDim.x * blockDim.x) {
        const int i = rowid[slot];
#pragma unroll
        for (int s = 0; s < S; ++s) dst[S * slot + s] = i >= 0 ? src.p[s][i] : 0.;
    }
}
template <int S>
__global__ void gsx_out_k(const int *__restrict__ rowid, int64_t n_slots, const double *__restrict__ src, MVecs<S> dst) {
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < n_slots; slot += (int64_t)gridDim.x * blockDim.x) {
        const int i = rowid[slot];
        if (i < 0) continue;
#pragma unroll
        for (int s = 0; s < S; ++s) dst.p[s][i] = src[S * slot + s];
    }
}

// kMode 0: r = b - A x, p = r, sum(r)   1: y = A x, sum(y)   2: t = A x, t.aux, t.t      (linear_algebra.rs:250-261)
// partial sums: quantity q of system s at partials[(s * kRed + q) * gridDim.x + blockIdx.x]
// (r04, measured and dropped: skipping the value stream and the products of a system the guard has frozen — per-system predicates in these
// two kernels cost 10-25 % on the unfrozen path (config 3: 28.9 -> 31.3 ms per iteration) and no system of that run is ever frozen)
template <int S, int kMode>
__global__ __launch_bounds__(kBlock) void gsx_spmv_k(SlotMat<S> M, const double *__restrict__ x, const double *__restrict__ aux, double *__restrict__ y,
                                                     double *__restrict__ y2, double *__restrict__ partials) {
    __shared__ double lds[8];
    constexpr int kRed = kMode == 2 ? 2 : 1;
    const int lane = threadIdx.x & 63;
    double red[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) red[s][0] = red[s][1] = 0.;
    SliceWalk w(M.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t slot = slice * 64 + lane;
        const int i = M.rowid[slot];
        const int len = i >= 0 ? M.row_len[slot] : 0;
        const int64_t base = M.sp[slice] + lane;
        const int width = (int)((M.sp[slice + 1] - M.sp[slice]) >> 6);
        double acc[S];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s] = 0.;
        for (int k0 = 0; k0 < width; k0 += 8) {
            int c[8];
            double v[S][8];
            const int64_t p0 = base + (int64_t)k0 * 64;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = k0 + u < len;
                c[u] = in ? M.cslot[p0 + (int64_t)u * 64] : 0;
#pragma unroll
                for (int s = 0; s < S; ++s) v[s][u] = in ? M.val[s][p0 + (int64_t)u * 64] : 0.;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (k0 + u < len && c[u] >= 0) {  // (c < 0: a ghost column — never in a slot-space solve, which is single-GPU)
#pragma unroll
                    for (int s = 0; s < S; ++s) acc[s] += v[s][u] * x[(int64_t)S * c[u] + s];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int64_t e = S * slot + s;
            if (kMode == 0) {
                const double r = i >= 0 ? aux[e] - acc[s] : 0.;
                y[e] = r; y2[e] = r;
                red[s][0] += r;
            } else if (kMode == 1) {
                const double o = i >= 0 ? acc[s] : 0.;
                y[e] = o;
                red[s][0] += o;
            } else {
                const double o = i >= 0 ? acc[s] : 0.;
                y[e] = o;
                if (i >= 0) { red[s][0] += o * aux[e]; red[s][1] += o * o; }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int q = 0; q < kRed; ++q) {
            const double t = block_sum(red[s][q], lds);
            if (threadIdx.x == 0) partials[(size_t)(s * kRed + q) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// x^ = M^-1 b for the slots [slice_lo, slice_hi) of one colour: gs_color_sorted_k's row update (linear_algebra.rs:225-239, omega = 1)
// from a zero start — the entries whose column belongs to this or a later colour (cslot >= first slot of the colour) multiply the
// zero of the start: skipped with their gathers (an exact zero added to the running sum leaves it as it is)
template <int S>
__global__ __launch_bounds__(kBlock) void gsx_sweep0_k(SlotMat<S> M, const double *__restrict__ b, double *__restrict__ xh, int slice_lo, int slice_hi,
                                                       int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    const int first_slot = slice_lo * 64;
    for (int sidx = slice_lo + blockIdx.x * waves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); sidx < slice_hi; sidx += gridDim.x * waves) {  // (scalar: see SliceWalk)
        const int64_t slot = (int64_t)sidx * 64 + lane;
        const int i = M.rowid[slot];
        const int len = i >= 0 ? M.row_len[slot] : 0;
        const int64_t base = M.sp[sidx] + lane;
        const int width = (int)((M.sp[sidx + 1] - M.sp[sidx]) >> 6);
        double sum[S];
#pragma unroll
        for (int s = 0; s < S; ++s) sum[s] = 0.;
        for (int k0 = 0; k0 < width; k0 += 8) {
            int c[8];
            double v[S][8];
            const int64_t p0 = base + (int64_t)k0 * 64;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool in = k0 + u < len;
                c[u] = in ? M.cslot[p0 + (int64_t)u * 64] : first_slot;
                const bool prev = c[u] >= 0 && c[u] < first_slot;  // a column swept by an earlier colour: the only ones that are not zero yet
#pragma unroll
                for (int s = 0; s < S; ++s) v[s][u] = prev ? M.val[s][p0 + (int64_t)u * 64] : 0.;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (c[u] >= 0 && c[u] < first_slot) {
#pragma unroll
                    for (int s = 0; s < S; ++s) sum[s] += v[s][u] * xh[(int64_t)S * c[u] + s];
                }
            }
        }
        const int d = i >= 0 ? M.diag_off[slot] : -1;
        if (i >= 0 && d < 0 && len > 0) atomicCAS(status, 0, (int)ORC_ERR_STRUCTURAL_ZERO);  // get(i, i) panics (lib.rs:664)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            double xi = 0.;
            if (d >= 0) xi = 0. * (1. - 1.) + 1. * (b[S * slot + s] - sum[s]) / M.val[s][d];  // x_i (1 - w) + w (b_i - sum) / a_ii with x_i = 0, w = 1
            xh[S * slot + s] = xi;
        }
    }
}

__device__ __forceinline__ bool gx_frozen(const double *sc, int guard) { return guard && (sc[GX_FROZEN] != 0. || sc[GX_FROZEN2] != 0.); }

// rho_0 = sum(r) of every system from the residual product's partial sums (one workgroup)
template <int S>
__global__ __launch_bounds__(kBlock) void gsx_rho0_k(double *__restrict__ scal, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[S * 16];
    double rho[S];
    fold_partials_multi<S>(fold, fold_count, lds, rho);
    if (threadIdx.x == 0)
        for (int s = 0; s < S; ++s) scal[GX_STRIDE * s + GX_RHO0] = rho[s];
}
// The vector kernels work on the interleaved vectors as FLAT arrays (element e = S slot + s belongs to system e % S): fully coalesced
// 8-byte accesses — a thread that handled "its slot's S values" touched 24-byte strides, 12 cache lines per wave instruction instead
// of 4 (r04's first form: 1.9 TB/s).  Element-wise results do not depend on who computes them; the one reduction (sum(r) in gsx_xr_k)
// hands its r values back to the slot's own thread through LDS, so the partial sums keep the thread -> slot map of S = 1.
// s = r - alpha nu, alpha = rho / sum(nu)                                         (:257, :259)
template <int S>
__global__ __launch_bounds__(kBlock) void gsx_s_k(double *__restrict__ scal, int rho_idx, const double *__restrict__ r, const double *__restrict__ nu,
                                                  double *__restrict__ sv, int64_t n, int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[S * 16];
    double alpha[S], sum_nu[S];
    bool act[S];
    fold_partials_multi<S>(fold, fold_count, lds, sum_nu);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double *sc = scal + GX_STRIDE * s;
        const bool frz = gx_frozen(sc, guard);
        const double rho = sc[rho_idx];
        alpha[s] = rho / sum_nu[s];
        const bool bad = guard && !(fin_nz(rho) && fin_nz(sum_nu[s]) && isfinite(alpha[s]));
        act[s] = !frz && !bad;
        if (blockIdx.x == 0 && threadIdx.x == 0 && !frz) {
            sc[GX_SUM_NU] = sum_nu[s];
            if (bad) sc[GX_FROZEN] = 1.;
        }
    }
    const int64_t total = (int64_t)S * n, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int s = (int)(e % S);
        double a = alpha[0];
        bool on = act[0];
#pragma unroll
        for (int q = 1; q < S; ++q) { if (s == q) { a = alpha[q]; on = act[q]; } }
        if (on) sv[e] = r[e] - a * nu[e];
    }
}
// x = (x + alpha p^) + omega s^ ; r = s - omega t ; partial sum(r)                (:258, :261-265, right-preconditioned)
template <int S>
__global__ __launch_bounds__(kBlock) void gsx_xr_k(double *__restrict__ scal, int rho_idx, double *__restrict__ x, const double *__restrict__ ph,
                                                   const double *__restrict__ sh, const double *__restrict__ sv, const double *__restrict__ t,
                                                   double *__restrict__ r, const int *__restrict__ rowid, int64_t n, double *__restrict__ partials,
                                                   int guard, const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[8];
    __shared__ double lds_f[2 * S * 16];
    __shared__ double r_tile[S * kBlock];
    double alpha[S], omega[S], acc[S], tsq[2 * S];
    int state[S];  // 0 = normal, 1 = t vanished or overflowed (x = h, r = s, stop), 2 = frozen (no-op)
    fold_partials_multi<2 * S>(fold, fold_count, lds_f, tsq);  // (t.s, t.t) of system s at 2 s, 2 s + 1
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double *sc = scal + GX_STRIDE * s;
        const bool frz = guard && sc[GX_FROZEN] != 0.;
        const double ts = tsq[2 * s], tt = tsq[2 * s + 1];
        alpha[s] = sc[rho_idx] / sc[GX_SUM_NU];
        omega[s] = ts / tt;
        const bool bad = guard && !(fin_nz(tt) && isfinite(omega[s]));
        if (bad) omega[s] = 0.;
        state[s] = frz ? 2 : (bad ? 1 : 0);
        acc[s] = 0.;
        if (blockIdx.x == 0 && threadIdx.x == 0 && !frz) {
            sc[GX_TS] = ts; sc[GX_TT] = tt;
            if (bad) sc[GX_FROZEN2] = 1.;
        }
    }
    // a workgroup takes chunks of kBlock consecutive slots (= S kBlock consecutive doubles of every vector); thread tid owns slot
    // chunk * kBlock + tid for the sums — S = 1's map — and computes the flat elements chunk * S kBlock + tid + j kBlock, j < S
    const int64_t n_chunks = (n + kBlock - 1) / kBlock, total = (int64_t)S * n;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t base = chunk * (int64_t)S * kBlock;
        double xv[S], pv[S], hv[S], sv_[S], tv[S];
#pragma unroll
        for (int j = 0; j < S; ++j) {  // all loads of the chunk first: S x 5 requests in flight per lane
            const int64_t e = base + threadIdx.x + (int64_t)j * kBlock;
            const bool in = e < total;
            xv[j] = in ? x[e] : 0.; pv[j] = in ? ph[e] : 0.; hv[j] = in ? sh[e] : 0.; sv_[j] = in ? sv[e] : 0.; tv[j] = in ? t[e] : 0.;
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const int64_t e = base + threadIdx.x + (int64_t)j * kBlock;
            double ri = 0.;
            if (e < total) {
                const int s = (int)(e % S);
                double a = alpha[0], o = omega[0];
                int stt = state[0];
#pragma unroll
                for (int q = 1; q < S; ++q) { if (s == q) { a = alpha[q]; o = omega[q]; stt = state[q]; } }
                if (stt != 2) {
                    const double h = xv[j] + a * pv[j];
                    x[e] = stt == 1 ? h : h + o * hv[j];
                    ri = stt == 1 ? sv_[j] : sv_[j] - o * tv[j];
                    r[e] = ri;
                }
            }
            r_tile[threadIdx.x + j * kBlock] = ri;
        }
        __syncthreads();
        const int64_t slot = chunk * kBlock + threadIdx.x;
        if (slot < n && rowid[slot] >= 0) {
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] += r_tile[S * threadIdx.x + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double tsum = block_sum(acc[s], lds);
        if (threadIdx.x == 0 && state[s] != 2) partials[(size_t)s * gridDim.x + blockIdx.x] = tsum;
    }
}
// beta = rho / rho_prev * alpha / omega ; p = r + beta (p - omega nu)             (:266-267)
template <int S>
__global__ __launch_bounds__(kBlock) void gsx_p_k(double *__restrict__ scal, int rho_prev_idx, int rho_idx, const double *__restrict__ r,
                                                  const double *__restrict__ nu, double *__restrict__ p, int64_t n, int guard,
                                                  const double *__restrict__ fold, int fold_count) {
    __shared__ double lds[S * 16];
    double beta[S], omega[S], rho[S];
    bool act[S];
    fold_partials_multi<S>(fold, fold_count, lds, rho);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double *sc = scal + GX_STRIDE * s;
        const bool frz = gx_frozen(sc, guard);
        const double rho_prev = sc[rho_prev_idx];
        const double alpha = rho_prev / sc[GX_SUM_NU];
        omega[s] = sc[GX_TS] / sc[GX_TT];
        beta[s] = rho[s] / rho_prev * alpha / omega[s];
        const bool bad = guard && !(fin_nz(omega[s]) && isfinite(beta[s]));
        act[s] = !frz && !bad;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (!frz) {
                sc[rho_idx] = rho[s];
                if (bad) sc[GX_FROZEN] = 1.;
            } else if (sc[GX_FROZEN2] != 0.) {
                sc[GX_FROZEN] = 1.;  // the x / r update took x = h, r = s: promote, or the next one would add alpha p^ again (see bicg_p_k)
            }
        }
    }
    const int64_t total = (int64_t)S * n, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int s = (int)(e % S);
        double bt = beta[0], o = omega[0];
        bool on = act[0];
#pragma unroll
        for (int q = 1; q < S; ++q) { if (s == q) { bt = beta[q]; o = omega[q]; on = act[q]; } }
        if (on) p[e] = r[e] + bt * (p[e] - o * nu[e]);
    }
}
template <int S>
__global__ void gsx_guard_event_k(const double *__restrict__ scal, int *__restrict__ counter) {
    int c = 0;
    for (int s = 0; s < S; ++s)
        if (scal[GX_STRIDE * s + GX_FROZEN] != 0. || scal[GX_STRIDE * s + GX_FROZEN2] != 0.) ++c;
    if (c) atomicAdd(counter, c);
}

static inline int gsx_grid(int64_t work_groups) {  // <= 1024 workgroups: every consumer folds the partial sums of its producer
    int64_t g = std::min<int64_t>(work_groups, 1024);
    if (g >= 8) g = (g / 8) * 8;
    return clamp_partials_grid(g);
}

// x^ = M^-1 b from zero: a launch of gsx_sweep0_k per colour
template <int S>
static void gsx_sweep0(const SlotMat<S> &M, const std::vector<int> &color_slice, const double *b, double *xh, int *status) {
    for (size_t c = 0; c + 1 < color_slice.size(); ++c) {
        const int lo = color_slice[c], hi = color_slice[c + 1];
        if (hi <= lo) continue;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_sweep0_k<S>), dim3(std::min(kMaxGrid, (hi - lo + 3) / 4)), dim3(kBlock), 0, ctx().stream, M, b, xh, lo, hi, status);
    }
}

// linear_algebra.rs:247-269 right-preconditioned by one coloured Gauss-Seidel sweep (extension), S systems on one pattern.
// M: colour-sorted storage with this solve's values; b[s], x[s]: the systems' vectors in ROW order (x in / out).
template <int S>
static int gsx_bicgstab(const SlotMat<S> &M, const std::vector<int> &color_slice, const CVecs<S> &b, const MVecs<S> &x, uint64_t iteration_count, Arena &arena,
                        int *status) {
    hipStream_t st = ctx().stream;
    const int64_t ns = M.n_slots;
    const size_t len = (size_t)S * (size_t)std::max<int64_t>(ns, 1);
    double *bs, *xs, *r, *p, *nu, *sv, *t, *ph, *sh, *partials, *partials2, *scal;
    ORC_TRY(arena.alloc(len, &bs)); ORC_TRY(arena.alloc(len, &xs)); ORC_TRY(arena.alloc(len, &r)); ORC_TRY(arena.alloc(len, &p));
    ORC_TRY(arena.alloc(len, &nu)); ORC_TRY(arena.alloc(len, &sv)); ORC_TRY(arena.alloc(len, &t)); ORC_TRY(arena.alloc(len, &ph));
    ORC_TRY(arena.alloc(len, &sh));
    ORC_TRY(arena.alloc((size_t)2 * S * kMaxPartials, &partials));
    ORC_TRY(arena.alloc((size_t)S * kMaxPartials, &partials2));
    ORC_TRY(arena.alloc((size_t)S * GX_STRIDE, &scal));
    ORC_HIP(hipMemsetAsync(scal, 0, S * GX_STRIDE * sizeof(double), st));
    const int guard = ctx().breakdown_guard ? 1 : 0;
    const int vg = gsx_grid((ns + kBlock - 1) / kBlock), g = gsx_grid(((int64_t)M.n_slices + 3) / 4);
    CVecs<S> xc;
    for (int s = 0; s < S; ++s) xc.p[s] = x.p[s];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_in_k<S>), dim3(vg), dim3(kBlock), 0, st, M.rowid, ns, b, bs);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_in_k<S>), dim3(vg), dim3(kBlock), 0, st, M.rowid, ns, xc, xs);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_spmv_k<S, 0>), dim3(g), dim3(kBlock), 0, st, M, (const double *)xs, (const double *)bs, r, p, partials);  // r = b - A x ; p = r
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_rho0_k<S>), dim3(1), dim3(kBlock), 0, st, scal, (const double *)partials, g);
    for (uint64_t it = 0; it < iteration_count; ++it) {
        const int cur = (int)(it & 1), nxt = cur ^ 1;
        gsx_sweep0<S>(M, color_slice, p, ph, status);    // p^ = M^-1 p
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_spmv_k<S, 1>), dim3(g), dim3(kBlock), 0, st, M, (const double *)ph, (const double *)nullptr, nu, (double *)nullptr, partials);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_s_k<S>), dim3(vg), dim3(kBlock), 0, st, scal, GX_RHO0 + cur, (const double *)r, (const double *)nu, sv, ns, guard,
                           (const double *)partials, g);
        gsx_sweep0<S>(M, color_slice, sv, sh, status);  // s^ = M^-1 s
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_spmv_k<S, 2>), dim3(g), dim3(kBlock), 0, st, M, (const double *)sh, (const double *)sv, t, (double *)nullptr, partials);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_xr_k<S>), dim3(vg), dim3(kBlock), 0, st, scal, GX_RHO0 + cur, xs, (const double *)ph, (const double *)sh, (const double *)sv,
                           (const double *)t, r, M.rowid, ns, partials2, guard, (const double *)partials, g);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_p_k<S>), dim3(vg), dim3(kBlock), 0, st, scal, GX_RHO0 + cur, GX_RHO0 + nxt, (const double *)r, (const double *)nu, p, ns, guard,
                           (const double *)partials2, vg);
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_out_k<S>), dim3(vg), dim3(kBlock), 0, st, M.rowid, ns, (const double *)xs, x);
    ORC_HIP(hipGetLastError());
    if (guard && ctx().guard_events) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_guard_event_k<S>), dim3(1), dim3(1), 0, st, (const double *)scal, ctx().guard_events);
        ORC_HIP(hipGetLastError());
    }
    return ORC_OK;
}

// the kernels' argument block from the layout and the S value streams of a solve
template <int S>
static SlotMat<S> slot_mat(const SortedLayout &L, const double *const val[S]) {
    SlotMat<S> M;
    M.sp = L.sp; M.row_len = L.row_len; M.rowid = L.rowid; M.diag_off = L.diag_off; M.cslot = L.cslot;
    for (int s = 0; s < S; ++s) M.val[s] = val[s];
    M.n_slices = L.n_slices; M.n_slots = L.n_slots;
    return M;
}

int gsx_bicgstab1(const Coloring &C, const double *val, const double *b, double *x, uint64_t iteration_count, Arena &arena, int *status) {
    CVecs<1> bv;
    MVecs<1> xv;
    bv.p[0] = b; xv.p[0] = x;
    return gsx_bicgstab<1>(slot_mat<1>(C.layout, &val), C.color_slice, bv, xv, iteration_count, arena, status);
}

// the shared pattern's colouring and layout, and the values of every A[k] in it
static int prepare3(const MatView A[3], Arena &arena, std::unique_ptr<Coloring> &owned, const Coloring **C, const double *val[3]) {
    ORC_TRY(gs_prepare(A[0], arena, owned, C, &val[0]));
    for (int k = 1; k < 3; ++k) ORC_TRY(sorted_values(A[k], (*C)->layout, arena, &val[k]));
    return ORC_OK;
}
// The u, v, w momentum systems of a SIMPLE iteration (solver.rs:99-136) under ORC_SOLVER_BICGSTAB_GS_PRECOND, in lock-step: the views
// share the mesh pattern (persistent: its colouring and colour-sorted layout are cached); b[k], x[k] in row order.  Single GPU.
int gs_bicgstab3_dev(const MatView A[3], const double *const b[3], double *const x[3], uint64_t iteration_count, Arena &arena) {
    const int64_t n = A[0].P.n;
    if (n == 0) return ORC_OK;
    if (!A[0].persistent_pattern || A[0].halo) return set_error(ORC_ERR_BAD_ARGUMENT, "gs_bicgstab3_dev: mesh-pattern systems on one GPU only");
    hipStream_t st = ctx().stream;
    std::unique_ptr<Coloring> owned;
    const Coloring *C = nullptr;
    const double *val[3];
    ArenaScope scope(arena);
    ORC_TRY(prepare3(A, arena, owned, &C, val));
    int *status;
    ORC_TRY(arena.alloc((size_t)1, &status));
    ORC_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    CVecs<3> bv;
    MVecs<3> xv;
    for (int k = 0; k < 3; ++k) { bv.p[k] = b[k]; xv.p[k] = x[k]; }
    ORC_TRY(gsx_bicgstab<3>(slot_mat<3>(C->layout, val), C->color_slice, bv, xv, iteration_count, arena, status));
    int h = 0;
    ORC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
    ORC_HIP(hipStreamSynchronize(st));
    return h == ORC_ERR_STRUCTURAL_ZERO ? h : ORC_OK;
}
// is the slot-space solver used?  (ORC_GS_SLOTSPACE=0: the row-space recurrences of gs_sweep.hip; read per solve: the tests compare the two)
bool gs_slot_space_enabled() { return cfg().gs_slotspace; }

// the preconditioner application as the slot-space solver launches it: x^ = M^-1 b from zero (gsx_sweep0_k, n_colors launches, no
// zero fill), one system (ms[0]) and u, v, w per launch (ms[1]); A[k]: the three momentum views on the mesh pattern
int bench_gs_sweep0_dev(const MatView A[3], const double *const b[3], int reps, Arena &arena, float ms[2], int *n_colors) {
    const int64_t n = A[0].P.n;
    ms[0] = ms[1] = 0.f;
    if (n == 0) return ORC_OK;
    hipStream_t st = ctx().stream;
    std::unique_ptr<Coloring> owned;
    const Coloring *C = nullptr;
    const double *val[3];
    ArenaScope scope(arena);
    ORC_TRY(prepare3(A, arena, owned, &C, val));
    if (n_colors) *n_colors = C->n_colors;
    int *status;
    ORC_TRY(arena.alloc((size_t)1, &status));
    ORC_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    const SlotMat<3> M3 = slot_mat<3>(C->layout, val);
    const SlotMat<1> M1 = slot_mat<1>(C->layout, val);
    CVecs<3> bv;
    CVecs<1> b1;
    for (int k = 0; k < 3; ++k) bv.p[k] = b[k];
    b1.p[0] = b[0];
    const int64_t ns = M3.n_slots;
    double *bs3, *xh3, *bs1, *xh1;
    ORC_TRY(arena.alloc((size_t)3 * ns, &bs3)); ORC_TRY(arena.alloc((size_t)3 * ns, &xh3));
    ORC_TRY(arena.alloc((size_t)ns, &bs1)); ORC_TRY(arena.alloc((size_t)ns, &xh1));
    const int vg = gsx_grid((ns + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_in_k<3>), dim3(vg), dim3(kBlock), 0, st, M3.rowid, ns, bv, bs3);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(gsx_in_k<1>), dim3(vg), dim3(kBlock), 0, st, M1.rowid, ns, b1, bs1);
    ORC_HIP(hipGetLastError());
    ORC_TRY(timed(reps, [&] { gsx_sweep0<1>(M1, C->color_slice, bs1, xh1, status); return (int)ORC_OK; }, &ms[0]));
    ORC_TRY(timed(reps, [&] { gsx_sweep0<3>(M3, C->color_slice, bs3, xh3, status); return (int)ORC_OK; }, &ms[1]));
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace orc
