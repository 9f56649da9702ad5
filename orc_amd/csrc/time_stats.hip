// time_stats.hip — running time statistics (new-build extension; ORC keeps no averages): weighted running means of the fields and the
// weighted co-moment sums of their fluctuations, accumulated where the fields live.  DESIGN.md §3 "Time statistics" has the
// definitions and the operator order; orc_types.h OrcStatGroup / OrcStatField name the groups and the fields.
//
//   time_stats_k   one fused grid-stride pass over the owned cells: the fields of the enabled groups and their K accumulators are read,
//                  West's update is applied in registers, the K accumulators are written back.  Each accumulator of a cell belongs to
//                  one thread: no atomics, no reductions, no status word.  The groups are template parameters: a group that is off
//                  costs no load.  The division r = w / W' is the host's.
//   stats_mean_k   the mean update alone over the 5 * nb boundary values boundary_map_k (derived.hip) has just written
// Read-only towards the flow and opt-in: neither kernel is launched unless the arm is on.
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"

namespace orc {

namespace {


constexpr uint32_t kMeanFields = 0xFu, kStressFields = 0x7F0u, kMuFields = 1u << ORC_STAT_MU, kPhiFields = 0x1F000u;
constexpr uint32_t kAllGroups = ORC_STAT_GROUP_MEAN | ORC_STAT_GROUP_STRESS | ORC_STAT_GROUP_VISCOSITY | ORC_STAT_GROUP_SCALAR | ORC_STAT_GROUP_BOUNDARY;
constexpr uint32_t kBoundaryMask = (1u << ORC_STAT_BOUNDARY_N) - 1;  // ORC_BOUNDARY_PRESSURE .. ORC_BOUNDARY_SHEAR_MAG
static_assert(ORC_STAT_N == 17 && ORC_STAT_PP == 10 && ORC_STAT_MU == 11 && ORC_STAT_PHI == 12 && ORC_STAT_WPHI == 16,
              "the field order is part of the ABI (orc_amd/solver.py STATISTIC_NAMES)");
static_assert(ORC_BOUNDARY_PRESSURE == 0 && ORC_BOUNDARY_SHEAR_MAG == ORC_STAT_BOUNDARY_N - 1, "the boundary means are the first five boundary maps");

uint32_t fields_of(uint32_t groups) {
    return kMeanFields | ((groups & ORC_STAT_GROUP_STRESS) ? kStressFields : 0u) | ((groups & ORC_STAT_GROUP_VISCOSITY) ? kMuFields : 0u) |
           ((groups & ORC_STAT_GROUP_SCALAR) ? kPhiFields : 0u);
}

struct StatsArgs {
    const double *u, *v, *w, *p, *mu, *phi;  // mu / phi: null while their group is off
    double *acc;                             // [K][stride]
    int64_t stride;
    double wt, r;                            // the sample's weight w and w / (W + w)
};

// West's update of one mean: dx = x - m, m' = m + r dx, ex = x - m'
__device__ __forceinline__ void mean_update(double &m, double x, double r, double &dx, double &ex) {
    dx = x - m;
    m = m + r * dx;
    ex = x - m;
}

// One sample on the K accumulators of one cell, a[] in OrcStatField order of the enabled groups.  C_xy' = C_xy + (w dx) ey.
template <bool kStress, bool kMu, bool kPhi>
__device__ __forceinline__ void stats_update(double *a, double u, double v, double w, double p, double mu, double phi, double wt, double r) {
    constexpr int oMu = 4 + (kStress ? 7 : 0), oPhi = oMu + (kMu ? 1 : 0);
    double du, eu, dv, ev, dw, ew, dp, ep;
    mean_update(a[0], u, r, du, eu);
    mean_update(a[1], v, r, dv, ev);
    mean_update(a[2], w, r, dw, ew);
    mean_update(a[3], p, r, dp, ep);
    if (kStress) {
        a[4] = a[4] + (wt * du) * eu;
        a[5] = a[5] + (wt * dv) * ev;
        a[6] = a[6] + (wt * dw) * ew;
        a[7] = a[7] + (wt * du) * ev;
        a[8] = a[8] + (wt * du) * ew;
        a[9] = a[9] + (wt * dv) * ew;
        a[10] = a[10] + (wt * dp) * ep;
    }
    if (kMu) {
        double dm, em;
        mean_update(a[oMu], mu, r, dm, em);
    }
    if (kPhi) {
        double df, ef;
        mean_update(a[oPhi], phi, r, df, ef);
        a[oPhi + 1] = a[oPhi + 1] + (wt * df) * ef;
        a[oPhi + 2] = a[oPhi + 2] + (wt * du) * ef;
        a[oPhi + 3] = a[oPhi + 3] + (wt * dv) * ef;
        a[oPhi + 4] = a[oPhi + 4] + (wt * dw) * ef;
    }
}

// One cell per thread: every load of a cell (up to 6 fields, K accumulators) is issued before the first use, so a wave keeps K + 6
// coalesced 512-byte requests in flight.  With MEAN + STRESS: 4 + 11 reads and 11 writes, 208 bytes per cell.  Two adjacent cells per
// thread with 16-byte accesses were measured against this at 10.24 M cells and came out within the run-to-run spread, so the
// form without a tail and without an alignment demand on the SoA stride stays.
template <bool kStress, bool kMu, bool kPhi>
__global__ __launch_bounds__(kBlock) void time_stats_k(int64_t n_own, StatsArgs A) {
    constexpr int K = 4 + (kStress ? 7 : 0) + (kMu ? 1 : 0) + (kPhi ? 5 : 0);
    GRID_STRIDE(c, n_own) {
        double a[K];
        double *acc = A.acc + c;
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = acc[(int64_t)k * A.stride];
        const double u = A.u[c], v = A.v[c], w = A.w[c], p = A.p[c];
        const double mu = kMu ? A.mu[c] : 0., phi = kPhi ? A.phi[c] : 0.;
        stats_update<kStress, kMu, kPhi>(a, u, v, w, p, mu, phi, A.wt, A.r);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[(int64_t)k * A.stride] = a[k];
    }
}

__global__ __launch_bounds__(kBlock) void stats_mean_k(int64_t n, const double *__restrict__ x, double *__restrict__ m, double r) {
    GRID_STRIDE(i, n) {
        const double m0 = m[i];
        const double dx = x[i] - m0;
        m[i] = m0 + r * dx;
    }
}

using StatsKernel = void (*)(int64_t, StatsArgs);
StatsKernel kernel_of(uint32_t groups) {
    static const StatsKernel table[8] = {time_stats_k<false, false, false>, time_stats_k<true, false, false>, time_stats_k<false, true, false>,
                                         time_stats_k<true, true, false>,   time_stats_k<false, false, true>, time_stats_k<true, false, true>,
                                         time_stats_k<false, true, true>,   time_stats_k<true, true, true>};
    return table[((groups & ORC_STAT_GROUP_STRESS) ? 1 : 0) | ((groups & ORC_STAT_GROUP_VISCOSITY) ? 2 : 0) | ((groups & ORC_STAT_GROUP_SCALAR) ? 4 : 0)];
}

// the cell pass of one sample (w, r) into `acc`
int k_time_stats(SolverState &s, double *acc, double w, double r) {
    const TimeStats &T = s.ts;
    if (s.n_own == 0) return ORC_OK;
    StatsArgs A{s.u.p, s.v.p, s.w.p, s.p.p, (T.c.groups & ORC_STAT_GROUP_VISCOSITY) ? s.vis.mu.p : nullptr,
                (T.c.groups & ORC_STAT_GROUP_SCALAR) ? s.sc.phi.p : nullptr, acc, s.n, w, r};
    hipLaunchKernelGGL(kernel_of(T.c.groups), dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, s.n_own, A);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// the boundary pass of one sample: the five maps of the current state into `now`, then the mean update of `mean`
int k_boundary_stats(SolverState &s, double *now, double *mean, double r) {
    TimeStats &T = s.ts;
    if (T.nb == 0) return ORC_OK;
    ORC_TRY(boundary_maps_dev(*s.mesh, s.u.p, s.v.p, s.w.p, s.p.p, s.rho, s.mu, s.cell_viscosity(), kBoundaryMask, now, T.bnd_status.p));
    const int64_t n = (int64_t)ORC_STAT_BOUNDARY_N * T.nb;
    hipLaunchKernelGGL(stats_mean_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, n, now, mean, r);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// one sample of weight w of the current state: W' = W + w, r = w / W' on the host, then the two passes
int sample(SolverState &s, double w) {
    TimeStats &T = s.ts;
    const double w_sum = T.W + w, r = w / w_sum;
    ORC_TRY(k_time_stats(s, T.acc.p, w, r));
    if (T.c.groups & ORC_STAT_GROUP_BOUNDARY) ORC_TRY(k_boundary_stats(s, T.bnd_now.p, T.bnd.p, r));
    T.W = w_sum;
    ++T.samples;
    return ORC_OK;
}

int boundary_status(SolverState &s, const char *what) {
    int h = 0;
    ORC_TRY(s.ts.bnd_status.download(&h, 1));
    if (h != ORC_OK) return set_error(h, "%s: a boundary face lies in a zone whose type the assembly does not support", what);
    return ORC_OK;
}

int validate(const SolverState &s, const OrcTimeStatistics &c) {
    if (!(c.groups & ORC_STAT_GROUP_MEAN)) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the MEAN group must be set");
    if (c.groups & ~kAllGroups) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: unknown group bits 0x%x", c.groups & ~kAllGroups);
    if (c.reserved0 != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: reserved0 must be 0");
    if (c.interval == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: interval must be at least 1");
    if ((c.groups & ORC_STAT_GROUP_VISCOSITY) && !s.vis.on)
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the VISCOSITY group needs the viscosity arm (orc_solver_set_viscosity)");
    if ((c.groups & ORC_STAT_GROUP_SCALAR) && !s.sc.on)
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the SCALAR group needs the scalar arm (orc_solver_set_scalar)");
    return ORC_OK;
}

}  // namespace

int stats_step_dev(SolverState &s) {
    TimeStats &T = s.ts;
    if (!T.on) return ORC_OK;
    ++T.step;
    if (T.step < T.c.start_step || (T.step - T.c.start_step) % T.c.interval != 0) return ORC_OK;
    return sample(s, s.dt);
}

}  // namespace orc

using namespace orc;

extern "C" {

static_assert(sizeof(OrcTimeStatistics) == 24 && offsetof(OrcTimeStatistics, groups) == 0 && offsetof(OrcTimeStatistics, reserved0) == 4 &&
                  offsetof(OrcTimeStatistics, start_step) == 8 && offsetof(OrcTimeStatistics, interval) == 16,
              "OrcTimeStatistics is part of the ABI (orc_amd/settings.py TimeStatistics mirrors it)");

void orc_time_statistics_default(OrcTimeStatistics *c) {
    if (!c) return;
    *c = OrcTimeStatistics{};
    c->groups = ORC_STAT_GROUP_MEAN | ORC_STAT_GROUP_STRESS;
    c->start_step = 1;
    c->interval = 1;
}

int orc_solver_set_time_statistics(OrcSolver *s, const OrcTimeStatistics *c) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!c) {  // off: advance launches nothing of the arm from here on
        ORC_HIP(hipStreamSynchronize(ctx().stream));
        st.ts = TimeStats();
        return ORC_OK;
    }
    ORC_TRY(validate(st, *c));
    TimeStats fresh;
    fresh.c = *c;
    fresh.field_mask = fields_of(c->groups);
    fresh.n_fields = popcount32(fresh.field_mask);
    ORC_TRY(fresh.acc.alloc((size_t)fresh.n_fields * (size_t)std::max<int64_t>(st.n, 1)));
    ORC_TRY(fresh.acc.zero());
    if (c->groups & ORC_STAT_GROUP_BOUNDARY) {
        ORC_TRY(surface_index(*st.mesh));
        fresh.nb = st.mesh->surface->n_bfaces;
        const size_t len = (size_t)ORC_STAT_BOUNDARY_N * (size_t)std::max<int64_t>(fresh.nb, 1);
        ORC_TRY(fresh.bnd.alloc(len));
        ORC_TRY(fresh.bnd.zero());
        ORC_TRY(fresh.bnd_now.alloc(len));
        ORC_TRY(fresh.bnd_status.alloc(1));
        ORC_TRY(fresh.bnd_status.zero());
        // the maps of the current state once, into the scratch: a zone type the assembly refuses is refused here
        int h = ORC_OK;
        ORC_TRY(boundary_maps_dev(*st.mesh, st.u.p, st.v.p, st.w.p, st.p.p, st.rho, st.mu, st.cell_viscosity(), kBoundaryMask, fresh.bnd_now.p,
                                  fresh.bnd_status.p));
        ORC_TRY(fresh.bnd_status.download(&h, 1));
        if (h != ORC_OK) return set_error(h, "time statistics: a boundary face lies in a zone whose type the assembly does not support");
    }
    fresh.on = true;
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    st.ts = std::move(fresh);
    return ORC_OK;
}

int orc_solver_sample_statistics(OrcSolver *s, double weight) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    if (!s->st.ts.on) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the arm is off (orc_solver_set_time_statistics)");
    if (!(weight > 0.) || !std::isfinite(weight)) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: a sample's weight must be positive and finite");
    return sample(s->st, weight);
}

int orc_solver_reset_statistics(OrcSolver *s) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    TimeStats &T = s->st.ts;
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the arm is off (orc_solver_set_time_statistics)");
    ORC_TRY(T.acc.zero());
    ORC_TRY(T.bnd.zero());
    T.W = 0.;
    T.samples = 0;
    return ORC_OK;
}

int orc_solver_statistics_info(OrcSolver *s, uint64_t *samples, double *weight_sum, int32_t *n_fields, int64_t *n_boundary_faces) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    const TimeStats &T = s->st.ts;
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the arm is off (orc_solver_set_time_statistics)");
    if (samples) *samples = T.samples;
    if (weight_sum) *weight_sum = T.W;
    if (n_fields) *n_fields = T.n_fields;
    if (n_boundary_faces) *n_boundary_faces = T.nb;
    return ORC_OK;
}

int orc_solver_get_statistics(OrcSolver *s, uint32_t field_mask, int32_t form, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: null argument");
    SolverState &st = s->st;
    const TimeStats &T = st.ts;
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the arm is off (orc_solver_set_time_statistics)");
    if (field_mask == 0 || (field_mask & ~T.field_mask))
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: mask 0x%x selects nothing, an unknown field or a field whose group is off", field_mask);
    if (form != ORC_STAT_RAW && form != ORC_STAT_NORMALISED) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: unknown form %d", form);
    if (form == ORC_STAT_NORMALISED && T.samples == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: NORMALISED needs at least one sample");
    const size_t n = (size_t)st.n;
    int slot = 0, q = 0;  // slot: row of the accumulator buffer; q: row of out
    for (int f = 0; f < ORC_STAT_N; ++f) {
        if (!(T.field_mask >> f & 1)) continue;
        const double *src = T.acc.p + (size_t)slot++ * n;
        if (!(field_mask >> f & 1)) continue;
        double *dst = out + (size_t)q++ * n;
        ORC_TRY(download_cells(*st.mesh, src, dst));
        const bool mean = f <= ORC_STAT_P || f == ORC_STAT_MU || f == ORC_STAT_PHI;
        if (form == ORC_STAT_NORMALISED && !mean)
            for (size_t c = 0; c < n; ++c) dst[c] = dst[c] / T.W;
    }
    return ORC_OK;
}

int orc_solver_set_statistics_state(OrcSolver *s, uint64_t samples, double weight_sum, uint32_t field_mask, const double *raw,
                                    const double *boundary_means) {
    ORC_TRY(ensure_init());
    if (!s || !raw) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: null argument");
    SolverState &st = s->st;
    TimeStats &T = st.ts;
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the arm is off (orc_solver_set_time_statistics)");
    if (field_mask != T.field_mask)
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: a state holds exactly the enabled fields (mask 0x%x, got 0x%x)", T.field_mask, field_mask);
    if (!(weight_sum >= 0.) || !std::isfinite(weight_sum)) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: weight_sum must be >= 0 and finite");
    if ((samples == 0) != (weight_sum == 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: 0 samples go with a weight sum of 0, and only they");
    const bool boundary = (T.c.groups & ORC_STAT_GROUP_BOUNDARY) != 0;
    if (boundary != (boundary_means != nullptr))
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: boundary means are given exactly when the BOUNDARY group is on");
    const size_t n = (size_t)st.n, n_own = (size_t)st.n_own;
    std::vector<double> own;  // ghost entries stay 0: a partitioned mesh (never a reordered one) uploads a copy with them zeroed
    if (n_own < n) own.assign(raw, raw + (size_t)T.n_fields * n);
    for (size_t k = 0; k < (size_t)T.n_fields && n_own < n; ++k) std::fill(own.begin() + (k * n + n_own), own.begin() + (k + 1) * n, 0.);
    ORC_TRY(upload_cells(*st.mesh, own.empty() ? raw : own.data(), T.acc, T.n_fields));
    if (boundary && T.nb > 0) ORC_TRY(T.bnd.upload(boundary_means, (size_t)ORC_STAT_BOUNDARY_N * (size_t)T.nb));
    T.W = weight_sum;
    T.samples = samples;
    return ORC_OK;
}

int orc_solver_get_boundary_statistics(OrcSolver *s, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: null argument");
    SolverState &st = s->st;
    const TimeStats &T = st.ts;
    if (!T.on || !(T.c.groups & ORC_STAT_GROUP_BOUNDARY))
        return set_error(ORC_ERR_BAD_ARGUMENT, "time statistics: the BOUNDARY group is off (orc_solver_set_time_statistics)");
    if (T.nb > 0) ORC_TRY(T.bnd.download(out, (size_t)ORC_STAT_BOUNDARY_N * (size_t)T.nb));
    return boundary_status(st, "time statistics");
}

int orc_bench_time_statistics(OrcSolver *s, int reps, double avg_ms[2]) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    SolverState &st = s->st;
    TimeStats &T = st.ts;
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "bench time statistics: the arm is off (orc_solver_set_time_statistics)");
    if (reps < 1) reps = 1;
    const bool boundary = (T.c.groups & ORC_STAT_GROUP_BOUNDARY) && T.nb > 0;
    DevBuf<double> acc, mean;  // the passes write here: the solver's statistics keep their bits
    ORC_TRY(acc.alloc((size_t)T.n_fields * (size_t)std::max<int64_t>(st.n, 1)));
    ORC_TRY(acc.zero());
    if (boundary) {
        ORC_TRY(mean.alloc((size_t)ORC_STAT_BOUNDARY_N * (size_t)T.nb));
        ORC_TRY(mean.zero());
    }
    int status = ORC_OK;
    for (int pass = 0; pass < 2 && status == ORC_OK; ++pass) {
        avg_ms[pass] = 0.;
        if (pass == 1 && !boundary) break;
        float ms = 0.f;
        status = timed(reps, [&] { return pass == 0 ? k_time_stats(st, acc.p, 1., 0.5) : k_boundary_stats(st, T.bnd_now.p, mean.p, 0.5); }, &ms,
                       "timing the statistics passes failed");
        avg_ms[pass] = (double)ms;
    }
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // the scratch is freed on return
    return status;
}

}  // extern "C"
