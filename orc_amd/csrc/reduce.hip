// reduce.hip — the fold of the kernels' partial sums, and the dot product and sum in the reference's own association for the
// verification mode.  Reference: nalgebra's dotx behind src/linear_algebra.rs:253-265, sum() behind src/solver.rs:206-208.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "linalg_kernels.hpp"

namespace orc {

// ------------------------------------------------------------------ reductions
__global__ __launch_bounds__(1024) void reduce_partials_k(const double *__restrict__ partials, int count, int nq, double *__restrict__ out) {
    __shared__ double lds[16];
    for (int q = 0; q < nq; ++q) {
        double v = 0.;
        for (int i = threadIdx.x; i < count; i += blockDim.x) v += partials[(size_t)q * count + i];
        v = wave_sum(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double r = 0.;
            for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += lds[i];
            out[q] = r;
        }
    }
}

int reduce_partials(const double *partials, int count, int nq, double *out, bool global) {
    hipLaunchKernelGGL(reduce_partials_k, dim3(1), dim3(1024), 0, ctx().stream, partials, count, nq, out);
    ORC_HIP(hipGetLastError());
    if (global && ctx().world > 1) ORC_TRY(comm_allreduce_sum(out, nq));
    return ORC_OK;
}

// ------------------------------------------------------------------ reference-order reductions (verification mode)
// OrcSettings.reduction_order = ORC_REDUCTION_REFERENCE: every dot product / norm of the solvers is evaluated in the
// association of nalgebra 0.32.4's `dotx` (base/blas.rs): eight running accumulators
// over blocks of 8, folded as res += (acc0+acc4); (acc1+acc5); (acc2+acc6); (acc3+acc7), then the tail left to right.
// Lane k of one wavefront owns accumulator k and walks its elements in order — n/8 dependent additions, so this is a
// slow path (milliseconds per ten million rows); it exists so that a device solve can be compared with the reference's
// arithmetic BIT FOR BIT at any iteration count, instead of through tolerances that the unguarded r_hat_0 = 1
// BiCGSTAB (linear_algebra.rs:252) amplifies.  a == nullptr stands for the all-ones r_hat_0 (1.0 * b[i] == b[i]).
// [r04] The n/8 dependent additions per accumulator are the floor (about 4 ms for 10.24 M elements); r02/r03's kernel paid a
// global-memory round trip per eight blocks on top of it (0.2 s per dot product at that size: ten minutes per SIMPLE iteration of
// the benchmark in this mode).  Now the products a[i] * b[i] are formed by fifteen loader wavefronts, coalesced, into a double-
// buffered LDS tile (the multiplication is element-wise: who performs it changes nothing), while lanes 0-7 of wavefront 0 walk the
// previous tile in order.  Same accumulators, same order of additions, same final fold: every bit as before.
constexpr int kDotTile = 4096;  // elements per LDS tile (2 x 32 KB)
__global__ __launch_bounds__(1024) void dot_reference_k(const double *__restrict__ a, const double *__restrict__ b, int64_t n,
                                                        double *__restrict__ out, const double *__restrict__ skip_flags) {
    __shared__ double tile[2][kDotTile];
    if (skip_flags && (skip_flags[0] != 0. || skip_flags[1] != 0.)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n8 = (n >> 3) << 3;  // elements in whole blocks of eight
    const int64_t n_tiles = (n8 + kDotTile - 1) / kDotTile;
    auto load = [&](int64_t t, int first, int stride) {  // products of tile t into tile[t & 1]
        double *dst = tile[t & 1];
        const int64_t base = t * kDotTile;
        for (int e = first; e < kDotTile; e += stride) {
            const int64_t i = base + e;
            if (i < n8) dst[e] = (a ? a[i] : 1.) * b[i];
        }
    };
    double acc = 0.;
    if (n_tiles > 0) load(0, tid, 1024);
    __syncthreads();
    for (int64_t t = 0; t < n_tiles; ++t) {
        if (wave == 0) {
            if (lane < 8) {
                const double *src = tile[t & 1] + lane;
                const int64_t left = n8 - t * kDotTile;
                const int cnt = (int)((left < kDotTile ? left : kDotTile) >> 3);  // blocks in this tile
                int j = 0;
                for (; j + 16 <= cnt; j += 16) {
                    double v[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) v[q] = src[(j + q) << 3];
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc += v[q];
                }
                for (; j < cnt; ++j) acc += src[j << 3];
            }
        } else if (t + 1 < n_tiles) {
            load(t + 1, tid - 64, 960);
        }
        __syncthreads();
    }
    if (wave != 0) return;
    // lane k < 4 forms acc_k + acc_{k+4}; lane 0 adds the four pairs and the tail in order
    const double hi = __shfl_down(acc, 4, 64);
    const double pair = acc + hi;
    const double p1 = __shfl(pair, 1, 64), p2 = __shfl(pair, 2, 64), p3 = __shfl(pair, 3, 64);
    if (lane == 0) {
        double res = 0.;
        res += pair;
        res += p1;
        res += p2;
        res += p3;
        for (int64_t k = n8; k < n; ++k) res += (a ? a[k] : 1.) * b[k];
        out[0] = res;
    }
}

int dot_reference(const double *a, const double *b, int64_t n, double *out, const double *skip_flags) {
    hipLaunchKernelGGL(dot_reference_k, dim3(1), dim3(1024), 0, ctx().stream, a, b, n, out, skip_flags);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// out[0] = ((0 + a[0]) + a[1]) + ...: the plain left-to-right fold behind nalgebra's `sum()` / `mean()` (solver.rs:206-208) and the
// running sums of the reference's cell loops (solver.rs:1224, discretization.rs:338) — ONE chain of n dependent additions (about
// 35 ms for 10.24 M elements): lane 0 of wavefront 0 walks LDS tiles the other fifteen wavefronts fill.  Verification mode only.
__global__ __launch_bounds__(1024) void sum_reference_k(const double *__restrict__ a, int64_t n, double *__restrict__ out) {
    __shared__ double tile[2][kDotTile];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int64_t n_tiles = (n + kDotTile - 1) / kDotTile;
    auto load = [&](int64_t t, int first, int stride) {
        double *dst = tile[t & 1];
        const int64_t base = t * kDotTile;
        for (int e = first; e < kDotTile; e += stride)
            if (base + e < n) dst[e] = a[base + e];
    };
    double acc = 0.;
    if (n_tiles > 0) load(0, tid, 1024);
    __syncthreads();
    for (int64_t t = 0; t < n_tiles; ++t) {
        if (wave == 0) {
            if (tid == 0) {
                const double *src = tile[t & 1];
                const int64_t left = n - t * kDotTile;
                const int cnt = (int)(left < kDotTile ? left : kDotTile);
                int j = 0;
                for (; j + 16 <= cnt; j += 16) {
                    double v[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) v[q] = src[j + q];
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc += v[q];
                }
                for (; j < cnt; ++j) acc += src[j];
            }
        } else if (t + 1 < n_tiles) {
            load(t + 1, tid - 64, 960);
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = acc;
}
int sum_reference(const double *a, int64_t n, double *out) {
    hipLaunchKernelGGL(sum_reference_k, dim3(1), dim3(1024), 0, ctx().stream, a, n, out);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace orc
