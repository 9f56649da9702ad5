// tracers.hip — tracer particles (new-build extension; ORC has none): massless particles moved through the cells in the solver's
// velocity.  DESIGN.md §3 "Tracer particles" has the definition; in short, one substep of an ACTIVE particle at (x, P)
//     U1 = velocity(x, P)             CELL (u_P, v_P, w_P);  LINEAR phi_P + ((G.x r.x + G.y r.y) + G.z r.z), r = x - x_P, G by the
//                                     assembly's per-cell bodies (gradient_cell.hpp) — the bits of probe_sample_k
//     h                               TIME direction step;  LENGTH (direction step) / s, s = sqrt((U1.x U1.x + U1.y U1.y) + U1.z U1.z),
//                                     STAGNANT unless s > min_speed
//     EULER  xn = x + h U1            RK2  xm = x + (0.5 h) U1, walk from P to Pm, U2 = velocity(xm, Pm), xn = x + h U2
//     walk to xn (point_walk.hpp)     INSIDE accepts: x = xn, P = Pn, age = age + h, steps = steps + 1;  OUTSIDE -> LEFT with the zone,
//                                     WALK_LIMIT -> WALK_LIMIT, both at the last accepted position
//
//   tracer_advect_k<kLsq, kLinear, kRk2>   one lane per particle, the seeds in the Morton order of the probes' locate so that a wave's
//                    particles are neighbours.  Position, cell, status, zone, age and steps are read once, stay in registers over all
//                    the substeps of a launch and are written once, with x - x_P for the sampler.  The mesh is read through MeshDev as
//                    the walk reads it, no table copy; the gradient of a visited cell is evaluated where it is needed and never stored
//                    (no memory, two evaluations per RK2 substep).  Bound by the latency of dependent gathers, not by bandwidth.
//                    Stopped lanes idle: no compaction.  No atomics but the status word of the gradient bodies: same input, same bits.
// A call advances the set from its state buffer into a second one and swaps them on success, so that a refused call leaves the set as
// it was.  Read-only towards mesh and solver, and opt-in: nothing here is launched unless a tracer entry is called or tracking is on.
#include <algorithm>
#include <cmath>
#include <memory>

#include "cell_order.hpp"
#include "gradient_cell.hpp"
#include "point_walk.hpp"
#include "probes.hpp"

static_assert(sizeof(OrcTracerSettings) == 32, "OrcTracerSettings is part of the ABI (orc_amd/settings.py TracerSettings)");
static_assert((int)ORC_TRACER_ACTIVE == (int)ORC_PROBE_STATUS_INSIDE && (int)ORC_TRACER_LEFT == (int)ORC_PROBE_STATUS_OUTSIDE &&
                  (int)ORC_TRACER_WALK_LIMIT == (int)ORC_PROBE_STATUS_WALK_LIMIT,
              "a seed's status is its locate's status");

namespace orc {
namespace {

struct TracerState {
    DevBuf<double> xyz, age, off;         // [3][n], [n], [3][n] x - x_cell
    DevBuf<int32_t> cell, status, zone;   // [n]: internal numbering, OrcTracerStatus, zone or -1
    DevBuf<int64_t> steps;                // [n]
    int alloc(int64_t n) {
        const size_t k = (size_t)n;
        ORC_TRY(xyz.alloc(3 * k)); ORC_TRY(age.alloc(k)); ORC_TRY(off.alloc(3 * k));
        ORC_TRY(cell.alloc(k)); ORC_TRY(status.alloc(k)); ORC_TRY(zone.alloc(k)); ORC_TRY(steps.alloc(k));
        return ORC_OK;
    }
};

struct TracerView {
    double *xyz, *age, *off;
    int32_t *cell, *status, *zone;
    int64_t *steps;
};
TracerView view(const TracerState &s) { return {s.xyz.p, s.age.p, s.off.p, s.cell.p, s.status.p, s.zone.p, s.steps.p}; }

}  // namespace
}  // namespace orc

// The particles of one mesh on the device, in the locate's (Morton) order: position k holds the caller's seed order[k].
struct OrcTracers {
    OrcMesh *mesh = nullptr;
    int64_t n = 0;
    std::vector<int64_t> order;
    orc::TracerState st[2];
    int cur = 0;  // st[cur] is the set; the other buffer is where the next call advances into
};

namespace orc {
namespace {

struct AdvectArgs {
    const double *u, *v, *w;
    TracerView in, out;    // out may be in: a lane reads its particle before it writes it
    int64_t n;
    double hs, min_speed;  // direction * step
    uint64_t n_sub;
    int length;            // step mode LENGTH
    double *record;        // [3][n] the positions after this launch, or null
    int32_t *accepted;     // [n] += the substeps accepted by this launch, or null
};

__device__ __forceinline__ double tracer_linear(double phi, V3 g, double rx, double ry, double rz) { return phi + ((g.x * rx + g.y * ry) + g.z * rz); }

template <bool kLsq, bool kLinear>
__device__ __forceinline__ V3 tracer_velocity(const MeshDev &M, const AdvectArgs &A, int P, double x, double y, double z, int *status) {
    V3 U = mk(A.u[P], A.v[P], A.w[P]);
    if (kLinear) {
        const double rx = x - M.ccx[P], ry = y - M.ccy[P], rz = z - M.ccz[P];
        V3 gx, gy, gz;
        double conv;
        if (kLsq) {
            double g[3][3];
            grad_u_lsq_cell<false>(M, A.u, A.v, A.w, P, status, g, conv);
            gx = mk(g[0][0], g[0][1], g[0][2]); gy = mk(g[1][0], g[1][1], g[1][2]); gz = mk(g[2][0], g[2][1], g[2][2]);
        } else {
            grad_u_gg_cell<false>(M, A.u, A.v, A.w, P, status, gx, gy, gz, conv);
        }
        U = mk(tracer_linear(U.x, gx, rx, ry, rz), tracer_linear(U.y, gy, rx, ry, rz), tracer_linear(U.z, gz, rx, ry, rz));
    }
    return U;
}

// One lane per particle.  Every cell a particle holds comes from the locate or from point_walk: below n_cells.
template <bool kLsq, bool kLinear, bool kRk2>
__global__ __launch_bounds__(kBlock) void tracer_advect_k(MeshDev M, AdvectArgs A, int *status) {
    GRID_STRIDE(i, A.n) {
        double x = A.in.xyz[i], y = A.in.xyz[A.n + i], z = A.in.xyz[2 * A.n + i], age = A.in.age[i];
        int P = A.in.cell[i], st = A.in.status[i], zn = A.in.zone[i];
        int64_t steps = A.in.steps[i];
        int32_t acc = 0;
        for (uint64_t k = 0; k < A.n_sub && st == ORC_TRACER_ACTIVE; ++k) {
            const V3 U1 = tracer_velocity<kLsq, kLinear>(M, A, P, x, y, z, status);
            double h = A.hs;
            if (A.length) {
                const double s = sqrt((U1.x * U1.x + U1.y * U1.y) + U1.z * U1.z);
                if (!(s > A.min_speed)) { st = ORC_TRACER_STAGNANT; break; }  // NaN too
                h = A.hs / s;
            }
            int Q = P;
            V3 U = U1;
            if (kRk2) {
                const double hh = 0.5 * h;
                const double xm = x + hh * U1.x, ym = y + hh * U1.y, zm = z + hh * U1.z;
                const WalkEnd e = point_walk(M, xm, ym, zm, Q);
                if (e.status != ORC_PROBE_STATUS_INSIDE) {
                    st = e.status;  // OUTSIDE = LEFT, WALK_LIMIT = WALK_LIMIT
                    if (e.status == ORC_PROBE_STATUS_OUTSIDE) zn = e.zone;
                    break;
                }
                U = tracer_velocity<kLsq, kLinear>(M, A, Q, xm, ym, zm, status);
            }
            const double xn = x + h * U.x, yn = y + h * U.y, znew = z + h * U.z;
            const WalkEnd e = point_walk(M, xn, yn, znew, Q);
            if (e.status != ORC_PROBE_STATUS_INSIDE) {
                st = e.status;
                if (e.status == ORC_PROBE_STATUS_OUTSIDE) zn = e.zone;
                break;
            }
            x = xn; y = yn; z = znew; P = Q;
            age = age + h;
            ++steps; ++acc;
        }
        A.out.xyz[i] = x; A.out.xyz[A.n + i] = y; A.out.xyz[2 * A.n + i] = z;
        A.out.age[i] = age;
        A.out.cell[i] = P; A.out.status[i] = st; A.out.zone[i] = zn;
        A.out.steps[i] = steps;
        A.out.off[i] = x - M.ccx[P]; A.out.off[A.n + i] = y - M.ccy[P]; A.out.off[2 * A.n + i] = z - M.ccz[P];
        if (A.record) { A.record[i] = x; A.record[A.n + i] = y; A.record[2 * A.n + i] = z; }
        if (A.accepted) A.accepted[i] += acc;
    }
}

// ====================================================================== host side
constexpr uint32_t kVelocityMask = (1u << ORC_PROBE_U) | (1u << ORC_PROBE_V) | (1u << ORC_PROBE_W);

int validate_settings(const SolverState &s, const OrcTracers *t, const OrcTracerSettings *c, bool tracking) {
    if (!t || !c) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: null argument");
    if (t->mesh != s.mesh) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: the set was seeded in another mesh");
    if (c->scheme != ORC_TRACER_EULER && c->scheme != ORC_TRACER_RK2) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: unknown scheme %d", c->scheme);
    if (c->interpolation != ORC_PROBE_CELL && c->interpolation != ORC_PROBE_LINEAR)
        return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: unknown interpolation %d", c->interpolation);
    if (c->step_mode != ORC_TRACER_STEP_TIME && c->step_mode != ORC_TRACER_STEP_LENGTH)
        return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: unknown step mode %d", c->step_mode);
    if (c->direction != 1 && c->direction != -1) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: direction must be +1 or -1, not %d", c->direction);
    if (!tracking && (!(c->step > 0.) || !std::isfinite(c->step))) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: step must be positive and finite");
    if (!(c->min_speed >= 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: min_speed must be >= 0");
    const int recon = s.settings.gradient_reconstruction;
    if (c->interpolation == ORC_PROBE_LINEAR && recon != ORC_GRAD_GREEN_GAUSS_CELL && recon != ORC_GRAD_LEAST_SQUARES)
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "tracers: unsupported gradient scheme");  // as the probes
    return ORC_OK;
}

// n_sub substeps of all particles from `in` to `out`, asynchronous on ctx().stream
int launch_advect(const SolverState &s, const OrcTracerSettings &c, double hs, const TracerView &in, const TracerView &out, int64_t n, uint64_t n_sub,
                  double *record, int32_t *accepted, int *status_dev) {
    AdvectArgs A{s.u.p, s.v.p, s.w.p, in, out, n, hs, c.min_speed, n_sub, c.step_mode == ORC_TRACER_STEP_LENGTH ? 1 : 0, record, accepted};
    const bool linear = c.interpolation == ORC_PROBE_LINEAR, rk2 = c.scheme == ORC_TRACER_RK2;
    const bool lsq = linear && s.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES;
    const dim3 grid(grid_for(n)), block(kBlock);
    const MeshDev M = s.mesh->dev();
#define ORC_TRACER_LAUNCH(L, I, R) hipLaunchKernelGGL(HIP_KERNEL_NAME(tracer_advect_k<L, I, R>), grid, block, 0, ctx().stream, M, A, status_dev)
    if (lsq) { if (rk2) ORC_TRACER_LAUNCH(true, true, true); else ORC_TRACER_LAUNCH(true, true, false); }
    else if (linear) { if (rk2) ORC_TRACER_LAUNCH(false, true, true); else ORC_TRACER_LAUNCH(false, true, false); }
    else { if (rk2) ORC_TRACER_LAUNCH(false, false, true); else ORC_TRACER_LAUNCH(false, false, false); }
#undef ORC_TRACER_LAUNCH
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// the status word of a tracking step on its way, if any
int tracking_flush(SolverState &s) {
    TracerTracking &T = s.tt;
    bool landed = false;
    ORC_TRY(T.raw.wait(&landed));
    const int h = landed ? *T.raw.host.p : ORC_OK;
    if (h != ORC_OK) {
        *T.raw.host.p = 0;
        ORC_TRY(T.status.zero());
        return sample_status(h);
    }
    return ORC_OK;
}

}  // namespace

int tracers_step_dev(SolverState &s) {
    TracerTracking &T = s.tt;
    if (!T.on) return ORC_OK;
    ORC_TRY(tracking_flush(s));  // the previous step's word: this step's iterations have synchronised the stream since
    OrcTracers &t = *T.set;
    ORC_TRY(launch_advect(s, T.c, s.dt / (double)T.substeps, view(t.st[t.cur]), view(t.st[1 - t.cur]), t.n, T.substeps, nullptr, nullptr, T.status.p));
    t.cur = 1 - t.cur;  // every reader of the set is ordered behind the launch on the stream
    ORC_TRY(T.raw.copy(0, T.status.p, sizeof(int)));
    return T.raw.mark();
}

}  // namespace orc

using namespace orc;

extern "C" {

void orc_tracer_settings_default(OrcTracerSettings *c) {
    if (!c) return;
    c->scheme = ORC_TRACER_RK2;
    c->interpolation = ORC_PROBE_LINEAR;
    c->step_mode = ORC_TRACER_STEP_LENGTH;
    c->direction = 1;
    c->step = 0.;
    c->min_speed = 0.;
}

OrcTracers *orc_tracers_create(OrcMesh *m, int64_t n, const double *xyz, int *status) {
    std::unique_ptr<OrcProbes> P(locate(m, n, xyz, true, 0, status));  // the device, the arguments and the mesh are looked at there
    if (!P) return nullptr;
    auto fail = [&](int st) { if (status) *status = st; (void)hipStreamSynchronize(ctx().stream); return (OrcTracers *)nullptr; };
    std::unique_ptr<OrcTracers> t(new OrcTracers());
    t->mesh = m;
    t->n = n;
    t->order = P->order;
    int st = ORC_OK;
    for (TracerState &s : t->st)
        if ((st = s.alloc(n)) != ORC_OK) return fail(st);
    TracerState &s = t->st[0];
    const size_t k = (size_t)n;
    const hipStream_t q = ctx().stream;
    const double *src[3] = {P->x.p, P->y.p, P->z.p};
    bool ok = true;
    for (int d = 0; d < 3; ++d) ok = ok && hipMemcpyAsync(s.xyz.p + d * k, src[d], k * sizeof(double), hipMemcpyDeviceToDevice, q) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.off.p, P->off.p, 3 * k * sizeof(double), hipMemcpyDeviceToDevice, q) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.cell.p, P->cell.p, k * sizeof(int32_t), hipMemcpyDeviceToDevice, q) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.status.p, P->status.p, k * sizeof(int32_t), hipMemcpyDeviceToDevice, q) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.zone.p, P->zone.p, k * sizeof(int32_t), hipMemcpyDeviceToDevice, q) == hipSuccess;
    ok = ok && s.age.zero() == ORC_OK && s.steps.zero() == ORC_OK;
    ok = ok && hipStreamSynchronize(q) == hipSuccess;  // the located set is freed on return
    if (!ok) return fail(set_error(ORC_ERR_HIP, "tracers: copying the located seeds failed"));
    return t.release();
}

void orc_tracers_destroy(OrcTracers *t) {
    if (t) (void)hipStreamSynchronize(ctx().stream);
    delete t;
}

int64_t orc_tracers_count(const OrcTracers *t) { return t ? t->n : 0; }

int orc_tracers_get(const OrcTracers *t, double *xyz, int64_t *cell, int32_t *status, int32_t *zone, double *age, int64_t *steps) {
    ORC_TRY(ensure_init());
    if (!t) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: null tracer set");
    const TracerState &s = t->st[t->cur];
    const size_t n = (size_t)t->n;
    if (xyz) {
        std::vector<double> h(3 * n);
        ORC_TRY(s.xyz.download(h.data(), 3 * n));
        for (size_t k = 0; k < n; ++k)
            for (int d = 0; d < 3; ++d) xyz[3 * t->order[k] + d] = h[d * n + k];
    }
    std::vector<int32_t> h(n);
    if (cell) {
        ORC_TRY(s.cell.download(h.data(), n));
        for (size_t k = 0; k < n; ++k) cell[t->order[k]] = orc_cell_id(*t->mesh, h[k]);
    }
    if (status) { ORC_TRY(s.status.download(h.data(), n)); unsort(t->order, h.data(), status); }
    if (zone) { ORC_TRY(s.zone.download(h.data(), n)); unsort(t->order, h.data(), zone); }
    if (age) {
        std::vector<double> a(n);
        ORC_TRY(s.age.download(a.data(), n));
        unsort(t->order, a.data(), age);
    }
    if (steps) {
        std::vector<int64_t> a(n);
        ORC_TRY(s.steps.download(a.data(), n));
        unsort(t->order, a.data(), steps);
    }
    return ORC_OK;
}

int orc_solver_advect_tracers(OrcSolver *s, OrcTracers *t, const OrcTracerSettings *c, uint64_t n_substeps, uint64_t record_stride, double *path,
                              int32_t *path_len) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: null solver");
    SolverState &st = s->st;
    ORC_TRY(validate_settings(st, t, c, false));
    if (record_stride > 0 && n_substeps % record_stride != 0)
        return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: n_substeps %llu is not a multiple of record_stride %llu", (unsigned long long)n_substeps,
                         (unsigned long long)record_stride);
    if (record_stride > 0 && !path) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: record_stride without a path array");
    const size_t n = (size_t)t->n;
    const uint64_t K = record_stride > 0 ? n_substeps / record_stride : 0;
    const TracerState &A = t->st[t->cur];
    TracerState &B = t->st[1 - t->cur];
    DevBuf<double> rec;
    DevBuf<int32_t> accepted;
    DevBuf<int> status;
    if (record_stride > 0) {
        ORC_TRY(rec.alloc((size_t)(K + 1) * 3 * n));
        ORC_TRY(accepted.alloc(n));
        ORC_TRY(accepted.zero());
        ORC_HIP(hipMemcpyAsync(rec.p, A.xyz.p, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, ctx().stream));  // record 0: at entry
    }
    int hs = 0;
    if (n_substeps > 0) {
        ORC_TRY(status.alloc(1));
        ORC_TRY(status.zero());
        const double step = (double)c->direction * c->step;
        const uint64_t launches = record_stride > 0 ? K : 1, per = record_stride > 0 ? record_stride : n_substeps;
        int launched = ORC_OK;
        for (uint64_t k = 0; k < launches && launched == ORC_OK; ++k)  // the first from the set into the second buffer, the others there in place
            launched = launch_advect(st, *c, step, view(k == 0 ? A : B), view(B), t->n, per, record_stride > 0 ? rec.p + (k + 1) * 3 * n : nullptr,
                                     accepted.p, status.p);
        if (launched != ORC_OK) {
            (void)hipStreamSynchronize(ctx().stream);
            return launched;
        }
        ORC_TRY(status.download(&hs, 1));  // the one synchronisation
        ORC_TRY(sample_status(hs));  // refused: the set is still its first buffer
        t->cur = 1 - t->cur;
    }
    if (record_stride > 0) {
        std::vector<double> h((size_t)(K + 1) * 3 * n);
        ORC_TRY(rec.download(h.data(), h.size()));
        for (size_t r = 0; r < (size_t)(K + 1) * 3; ++r) unsort(t->order, h.data() + r * n, path + r * n);
        if (path_len) {
            std::vector<int32_t> a(n);
            ORC_TRY(accepted.download(a.data(), n));
            for (size_t k = 0; k < n; ++k) {
                const uint64_t got = 1 + ((uint64_t)a[k] + record_stride - 1) / record_stride;
                path_len[t->order[k]] = (int32_t)std::min<uint64_t>(K + 1, got);
            }
        }
    }
    return ORC_OK;
}

int orc_solver_sample_tracers(OrcSolver *s, const OrcTracers *t, uint32_t field_mask, int32_t interpolation, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !t || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: null argument");
    SolverState &st = s->st;
    if (t->mesh != st.mesh) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: the set was seeded in another mesh");
    ORC_TRY(validate_fields(st, field_mask, interpolation));
    const TracerState &A = t->st[t->cur];
    return sample_to_host(st, A.cell.p, A.off.p, t->n, field_mask, interpolation, &t->order, out);
}

int orc_solver_set_tracer_tracking(OrcSolver *s, OrcTracers *t, const OrcTracerSettings *c, uint32_t substeps_per_step) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "tracers: null solver");
    SolverState &st = s->st;
    if (!t) {  // off: advance launches nothing of the tracking from here on
        const int last = tracking_flush(st);
        st.tt.clear();
        return last;
    }
    ORC_TRY(validate_settings(st, t, c, true));
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "tracer tracking: needs the transient arm (orc_solver_set_transient)");
    if (c->step_mode != ORC_TRACER_STEP_TIME) return set_error(ORC_ERR_BAD_ARGUMENT, "tracer tracking: the step mode must be TIME");
    if (c->direction != 1) return set_error(ORC_ERR_BAD_ARGUMENT, "tracer tracking: the direction must be +1");
    if (substeps_per_step == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "tracer tracking: substeps_per_step must be at least 1");
    TracerTracking T;
    if (c->interpolation == ORC_PROBE_LINEAR) {  // one evaluation at the particles first: what the gradient bodies refuse is refused here
        const TracerState &A = t->st[t->cur];
        ORC_TRY(sample_to_host(st, A.cell.p, A.off.p, t->n, kVelocityMask, ORC_PROBE_LINEAR, nullptr, nullptr, &T.status));
    } else {
        ORC_TRY(T.status.alloc(1));
        ORC_TRY(T.status.zero());
    }
    ORC_TRY(T.raw.create(1, "tracer tracking"));
    *T.raw.host.p = 0;
    T.set = t;
    T.c = *c;
    T.substeps = substeps_per_step;
    T.on = true;
    st.tt.clear();
    st.tt = std::move(T);
    return ORC_OK;
}

int orc_bench_tracers(OrcSolver *s, const OrcTracers *t, const OrcTracerSettings *c, uint64_t n_substeps, int reps, double *avg_ms) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench tracers: null argument");
    SolverState &st = s->st;
    ORC_TRY(validate_settings(st, t, c, false));
    if (reps < 1) reps = 1;
    TracerState scratch;  // the launches write here: the set keeps its bits
    DevBuf<int> status;
    ORC_TRY(scratch.alloc(t->n));
    ORC_TRY(status.alloc(1));
    ORC_TRY(status.zero());
    const double step = (double)c->direction * c->step;
    const TracerView in = view(t->st[t->cur]), out = view(scratch);
    float ms = 0.f;
    const int rc = timed(reps, [&] { return launch_advect(st, *c, step, in, out, t->n, n_substeps, nullptr, nullptr, status.p); }, &ms,
                         "timing the tracer launches failed");
    int hs = 0;
    ORC_TRY(status.download(&hs, 1));  // synchronises: the scratch is freed on return
    ORC_TRY(rc);
    ORC_TRY(sample_status(hs));
    *avg_ms = (double)ms;
    return ORC_OK;
}

}  // extern "C"
