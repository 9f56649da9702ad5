// courant.hip — the Courant reduction of adaptive time stepping (new-build extension): the largest convective rate
// sum_f |U_f . n| A / (2 V) over the owned cells and the cell that attains it, formed where the fields live.  DESIGN.md §3
// "Adaptive time stepping" has the definitions; api_transient.cpp holds the controller that reads the result.
//
//   courant_k        one thread per owned cell, derived_cell_k's XCD-contiguous block walk: the face loop of gradient_cell.hpp with the
//                    gradient rows left out (grad_u_gg_cell<true, false>: the bits of ORC_DERIVED_CONVECTIVE_RATE under either
//                    reconstruction), then (rate, ORC id) pairs reduced by a wave __shfl_down tree, the four waves through LDS, one
//                    pair per workgroup.  kField: the per-cell rates are stored as well, from the same launch.
//   courant_fold_k   one workgroup folds the workgroup pairs by the same tree.
// The order on pairs: a NaN rate ranks above every number (fmax would drop it), then the larger rate, then the smaller ORC id — a
// total order, so the result does not depend on the association and a plain and a reordered mesh agree.  Read-only and opt-in: neither
// kernel is launched unless an entry of this file or a controlled step calls for it.  No atomics but the status word, no scratch.
#include <algorithm>
#include <cmath>
#include <limits>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"

namespace orc {

namespace {

constexpr long long kNoCell = std::numeric_limits<long long>::max();

// does (av, ai) rank before (bv, bi)?
__device__ __forceinline__ bool rate_before(double av, long long ai, double bv, long long bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}
__device__ __forceinline__ void rate_take(double &v, long long &id, double ov, long long oi) {
    if (rate_before(ov, oi, v, id)) { v = ov; id = oi; }
}
// the best pair of the workgroup (256 threads = 4 waves); valid in thread 0
__device__ __forceinline__ void block_rate(double &v, long long &id, double *lds_v, long long *lds_id) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const long long oi = __shfl_down(id, off, 64);
        rate_take(v, id, ov, oi);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { lds_v[w] = v; lds_id[w] = id; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < kBlock / kWave; ++i) rate_take(v, id, lds_v[i], lds_id[i]);
}

// One thread per owned cell; XCD g (workgroups g, g + 8, ...) takes a contiguous eighth of the cells (derived_cell_k, scalar_k; DESIGN
// §12).  Reads what grad_u_k reads but the volume ratio; writes one pair per workgroup and, with kField, one double per cell.
template <bool kField>
__global__ __launch_bounds__(kBlock) void courant_k(MeshDev M, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                                                    const int32_t *__restrict__ orc_id, double *__restrict__ rate_out,
                                                    double *__restrict__ part_v, long long *__restrict__ part_id, int *status) {
    __shared__ double lds_v[kBlock / kWave];
    __shared__ long long lds_id[kBlock / kWave];
    const int n_items = (int)M.n_own;  // cell ids are int32 (MeshDev.c0)
    const int n_blk = (n_items + kBlock - 1) / kBlock;
    int vb = blockIdx.x, vb_end = n_blk, vb_step = gridDim.x;
    if ((gridDim.x & 7) == 0 && gridDim.x >= 8) {
        const int per = (n_blk + 7) / 8;
        const int xcd = blockIdx.x & 7;
        vb = xcd * per + (int)(blockIdx.x >> 3);
        vb_end = (xcd + 1) * per < n_blk ? (xcd + 1) * per : n_blk;
        vb_step = gridDim.x >> 3;
    }
    double best = -INFINITY;
    long long best_id = kNoCell;
    for (; vb < vb_end; vb += vb_step) {
        const int c = vb * kBlock + (int)threadIdx.x;
        if (c >= n_items) break;
        V3 gx, gy, gz;
        double conv;
        grad_u_gg_cell<true, false>(M, u, v, w, c, status, gx, gy, gz, conv);
        const double rate = conv / (2. * M.vol[c]);
        if (kField) rate_out[c] = rate;
        rate_take(best, best_id, rate, orc_id ? (long long)orc_id[c] : (long long)c);
    }
    block_rate(best, best_id, lds_v, lds_id);
    if (threadIdx.x == 0) { part_v[blockIdx.x] = best; part_id[blockIdx.x] = best_id; }
}

// out[0] = rate_max, out[1] = its ORC id as a double; out[2] = rate_max with +inf in place of a NaN and out[3] = 1 for a NaN, else 0:
// the two slots a partitioned mesh all-reduces by maximum
__global__ __launch_bounds__(kBlock) void courant_fold_k(const double *__restrict__ part_v, const long long *__restrict__ part_id, int n_part,
                                                         double *__restrict__ out) {
    __shared__ double lds_v[kBlock / kWave];
    __shared__ long long lds_id[kBlock / kWave];
    double best = -INFINITY;
    long long best_id = kNoCell;
    for (int i = (int)threadIdx.x; i < n_part; i += kBlock) rate_take(best, best_id, part_v[i], part_id[i]);
    block_rate(best, best_id, lds_v, lds_id);
    if (threadIdx.x == 0) {
        const bool nan = best != best;
        out[0] = best;
        out[1] = (double)best_id;
        out[2] = nan ? INFINITY : best;
        out[3] = nan ? 1. : 0.;
    }
}

int prepare(SolverState &s) {
    SolverState::Courant &C = s.cr;
    if (C.ready) return ORC_OK;
    const OrcMesh &m = *s.mesh;
    ORC_TRY(C.part_v.alloc(kMaxPartials));
    ORC_TRY(C.part_id.alloc(kMaxPartials));
    ORC_TRY(C.out.alloc(4));
    ORC_TRY(C.status.alloc(1));
    ORC_TRY(C.status.zero());
    if (!m.halo.active() && !cell_order_ids(m).empty()) {
        std::vector<int32_t> g(cell_order_ids(m).begin(), cell_order_ids(m).end());
        ORC_TRY(C.orc_id.upload(g.data(), g.size()));
    }
    ORC_TRY(C.raw.alloc(2));
    C.ready = true;
    return ORC_OK;
}

// the two launches, asynchronous on ctx().stream; the fields' ghosts are current
int launch(SolverState &s, double *rate_dev) {
    SolverState::Courant &C = s.cr;
    OrcMesh &m = *s.mesh;
    const int grid = grid_for(m.n_own);
    long long *ids = reinterpret_cast<long long *>(C.part_id.p);
    if (rate_dev)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(courant_k<true>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), s.u.p, s.v.p, s.w.p, C.orc_id.p,
                           rate_dev, C.part_v.p, ids, C.status.p);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(courant_k<false>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), s.u.p, s.v.p, s.w.p, C.orc_id.p,
                           rate_dev, C.part_v.p, ids, C.status.p);
    hipLaunchKernelGGL(courant_fold_k, dim3(1), dim3(kBlock), 0, ctx().stream, C.part_v.p, ids, grid, C.out.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace

int courant_dev(SolverState &s, double *rate_max, int64_t *cell, double *rate_dev) {
    ORC_TRY(prepare(s));
    SolverState::Courant &C = s.cr;
    OrcMesh &m = *s.mesh;
    const bool partitioned = m.halo.active();
    if (partitioned) { double *f[3] = {s.u.p, s.v.p, s.w.p}; ORC_TRY(m.halo.exchange(f, 3)); }
    ORC_TRY(launch(s, rate_dev));
    if (partitioned) ORC_TRY(comm_allreduce_max(C.out.p + 2, 2));  // exact: every rank gets the same bits and chooses the same next step
    ORC_HIP(hipMemcpyAsync(C.raw.p, C.out.p + (partitioned ? 2 : 0), 2 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    if (partitioned) {
        if (rate_max) *rate_max = C.raw.p[1] != 0. ? std::numeric_limits<double>::quiet_NaN() : C.raw.p[0];
        if (cell) *cell = -1;  // no global tie rule is built
    } else {
        if (rate_max) *rate_max = C.raw.p[0];
        if (cell) *cell = m.n_own > 0 ? (int64_t)C.raw.p[1] : -1;
    }
    return ORC_OK;
}

}  // namespace orc

using namespace orc;

extern "C" {

int orc_solver_courant(OrcSolver *s, double *rate_max, int64_t *cell, double *rate) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "courant: null solver");
    SolverState &st = s->st;
    OrcMesh &m = *st.mesh;
    ORC_TRY(prepare(st));
    ORC_TRY(st.cr.status.zero());
    DevBuf<double> dev;
    if (rate) {
        ORC_TRY(dev.alloc((size_t)std::max<int64_t>(m.n_cells, 1)));
        ORC_TRY(dev.zero());  // the ghost cells' entries of a partitioned mesh stay zero
    }
    double r = 0.;
    int64_t c = -1;
    ORC_TRY(courant_dev(st, &r, &c, rate ? dev.p : nullptr));
    if (rate) ORC_TRY(download_cells(m, dev.p, rate));
    int h = 0;
    ORC_TRY(st.cr.status.download(&h, 1));
    if (m.halo.active()) h = comm_global_status(h);
    if (h != ORC_OK) return set_error(h, "courant: a boundary face lies in a zone whose type the assembly does not support");
    if (rate_max) *rate_max = r;
    if (cell) *cell = c;
    return ORC_OK;
}

int orc_bench_courant(OrcSolver *s, int reps, double *avg_ms) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench courant: null argument");
    SolverState &st = s->st;
    if (reps < 1) reps = 1;
    ORC_TRY(prepare(st));
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    int rc = launch(st, nullptr);  // warm-up
    if (rc == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) rc = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    for (int i = 0; i < reps && rc == ORC_OK; ++i) rc = launch(st, nullptr);
    float ms = 0.f;
    if (rc == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = set_error(ORC_ERR_HIP, "timing the courant launches failed");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ORC_TRY(rc);
    *avg_ms = (double)ms / reps;
    return ORC_OK;
}

}  // extern "C"
