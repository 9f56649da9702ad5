// viscosity.hip — variable viscosity (new-build extension; ORC knows one constant mu): a per-cell viscosity field, prescribed or a law
// of the strain-rate magnitude, and the diffusion matrix rebuilt from it.  DESIGN.md §3 "Variable viscosity" has the definitions and
// the operator order; orc_types.h OrcViscosity names the parameters.
//
//   viscosity_cell_k   one thread per owned cell, derived_cell_k's XCD-contiguous block walk: the velocity gradient of the settings'
//                      reconstruction by the assembly's own per-cell body (gradient_cell.hpp), g = strain_rate_mag(strain_ss(G)) — the
//                      bits of ORC_DERIVED_STRAIN_RATE_MAG — then the law, the clamp and the relaxation; writes mu and, for
//                      orc_solver_evaluate_viscosity, g.  Model and relaxation are wave-uniform arguments.  With wall damping of the
//                      Smagorinsky length (orc_solver_set_wall_damping) the "damped" instantiation also reads the cell's wall distance
//                      (wall_distance.hip) — DESIGN.md §3 "Wall distance and wall damping".
//   diffusion_var_k    one thread per owned row, the same walk: diffusion_k's loop (assembly.hip) with mu replaced by the face
//                      viscosity, i.e. one more gather (mu_N) per interior face; writes a_di, b_u_di, b_v_di, b_w_di
// momentum_k reads the diffusion coefficients from a_di and the wall terms from b_*_di and never sees mu: neither it, nor the Rhie-Chow
// path, nor any solve changes.  Opt-in: neither kernel is launched unless orc_solver_set_viscosity has switched the arm on.  Both are
// gather-bound like the kernels they are modelled on; no atomics but the status word, no LDS.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"
#include "var_diffusion.hpp"

namespace orc {

namespace {

struct ViscosityArgs {
    const double *u, *v, *w;
    const double *field;  // FIELD: the prescribed viscosity
    double *mu;           // [n_cells] out; with relax also the old field
    double *g;            // [n_cells] out, may be null
    int model, relax;     // the same in every lane
    double k, n, mu_zero, mu_inf, lambda, cs, mu_min, mu_max, relaxation;
    double rho, mu_lam;   // the solver's density and (laminar) viscosity: SMAGORINSKY
    // wall damping of the Smagorinsky length (OrcWallDamping): the mode (the same in every lane) and the wall distance per cell, null
    // unless the mode needs it
    int damping;
    const double *wall_d;
    double kappa, a_plus, u_tau;
};

// The law at strain-rate magnitude g in a cell of volume vol, then the clamp: THE operator order of DESIGN §3 "Variable viscosity".
// g = 0 with n < 1 makes pow return +inf, which the clamp turns into mu_max: intended.  d: the cell's wall distance (read by the
// damped Smagorinsky length only; DESIGN §3 "Wall distance and wall damping"): d = +inf gives l0 exactly in both modes.
// kDamped = false compiles today's undamped sequence alone: the kernel of a solver without damping is the one it was.
template <bool kDamped>
__device__ __forceinline__ double viscosity_law(const ViscosityArgs &A, double g, double vol, double d) {
    double m;
    if (A.model == ORC_VISCOSITY_POWER_LAW) {
        m = A.k * pow(g, A.n - 1.);
    } else if (A.model == ORC_VISCOSITY_CARREAU) {
        const double t = A.lambda * g;
        m = A.mu_inf + (A.mu_zero - A.mu_inf) * pow(1. + t * t, (A.n - 1.) / 2.);
    } else {  // SMAGORINSKY
        double l = A.cs * cbrt(vol);
        if (kDamped) {
            if (A.damping == ORC_WALL_DAMPING_MIN) {
                l = fmin(A.kappa * d, l);
            } else if (A.damping == ORC_WALL_DAMPING_VAN_DRIEST) {
                const double yp = ((A.rho * A.u_tau) * d) / A.mu_lam;
                l = l * (-expm1(-(yp / A.a_plus)));  // expm1: no cancellation at the wall
            }
        }
        m = A.mu_lam + (A.rho * (l * l)) * g;
    }
    return fmin(fmax(m, A.mu_min), A.mu_max);
}

// Reads what grad_u_k / grad_u_lsq_k read; writes one double per cell (two for orc_solver_evaluate_viscosity).
template <bool kLsq, bool kDamped>
__global__ __launch_bounds__(kBlock) void viscosity_cell_k(MeshDev M, ViscosityArgs A, int *status) {
    const int n_items = (int)M.n_own;  // cell ids are int32 (MeshDev.c0)
    for (BlockWalk W = block_walk(n_items); W.vb < W.vb_end; W.vb += W.vb_step) {
        const int c = W.vb * kBlock + (int)threadIdx.x;
        if (c >= n_items) break;
        V3 gx, gy, gz;
        double conv;
        if (kLsq) {
            double g[3][3];
            grad_u_lsq_cell<false>(M, A.u, A.v, A.w, c, status, g, conv);
            gx = mk(g[0][0], g[0][1], g[0][2]); gy = mk(g[1][0], g[1][1], g[1][2]); gz = mk(g[2][0], g[2][1], g[2][2]);
        } else {
            grad_u_gg_cell<false>(M, A.u, A.v, A.w, c, status, gx, gy, gz, conv);
        }
        const double g = strain_rate_mag(strain_ss(gx, gy, gz));
        if (A.g) A.g[c] = g;
        double mu;
        if (A.model == ORC_VISCOSITY_FIELD) {
            mu = A.field[c];
        } else {
            mu = viscosity_law<kDamped>(A, g, M.vol[c], kDamped ? A.wall_d[c] : INFINITY);
            if (A.relax) {
                const double old = A.mu[c];
                mu = old + A.relaxation * (mu - old);
            }
        }
        A.mu[c] = mu;
    }
}

// diffusion_k (assembly.hip; discretization.rs:39-131) with mu replaced by the face viscosity: the same branches per zone type, the
// same accumulation order of a_p and of the wall terms, d_i = mu_f * A / dist.  A boundary face takes its cell's viscosity.
__global__ __launch_bounds__(kBlock) void diffusion_var_k(MeshDev M, SellDev P, const double *__restrict__ mu, int harmonic,
                                                          double *__restrict__ a_di, double *__restrict__ b_u, double *__restrict__ b_v,
                                                          double *__restrict__ b_w, int *status) {
    const int n_items = (int)M.n_own;
    for (BlockWalk W = block_walk(n_items); W.vb < W.vb_end; W.vb += W.vb_step) {
        const int c = W.vb * kBlock + (int)threadIdx.x;
        if (c >= n_items) break;
        const V3 cc = cell_centroid(M, c);
        const double mu_p = mu[c];
        double a_p = 0., bu = 0., bv = 0., bw = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int z = M.fzone[f];
            const int zt = M.ztype[z];
            double d_i = 0.;
            if (zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET) {
                d_i = mu_p * M.area[f] / vnorm(vsub(face_centroid(M, f), cc));
                const V3 sc = vmuls(zone_vec(M, z), d_i);
                bu += sc.x; bv += sc.y; bw += sc.z;
            } else if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET || zt == ORC_BC_SYMMETRY) {
                d_i = 0.;
            } else if (zt == ORC_BC_INTERIOR) {
                const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
                d_i = face_viscosity(harmonic, mu_p, mu[nb]) * M.area[f] / vnorm(vsub(cell_centroid(M, nb), cc));
                a_di[M.cfpos[q]] = -d_i;
            } else {
                raise(status, ORC_ERR_UNSUPPORTED_BC);
            }
            a_p += d_i;
        }
        a_di[P.diag_pos[c]] = a_p;
        b_u[c] = bu; b_v[c] = bv; b_w[c] = bw;
    }
}

bool finite_all(std::initializer_list<double> xs) {
    for (double x : xs)
        if (!std::isfinite(x)) return false;
    return true;
}

int validate(const OrcViscosity &c) {
    if (c.model < ORC_VISCOSITY_FIELD || c.model > ORC_VISCOSITY_SMAGORINSKY) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: unknown model %d", c.model);
    if (c.face_interpolation != ORC_VISCOSITY_FACE_ARITHMETIC && c.face_interpolation != ORC_VISCOSITY_FACE_HARMONIC)
        return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: unknown face interpolation %d", c.face_interpolation);
    if (!finite_all({c.k, c.n, c.mu_zero, c.mu_inf, c.lambda, c.cs, c.mu_min, c.mu_max, c.relaxation}))
        return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: every parameter must be finite");
    if (!(c.cs >= 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: cs must be >= 0");
    if (!(c.mu_min > 0.) || !(c.mu_min <= c.mu_max)) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the clamp needs 0 < mu_min <= mu_max < inf");
    if (!(c.relaxation > 0.) || !(c.relaxation <= 1.)) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: relaxation must lie in (0, 1]");
    if (c.model == ORC_VISCOSITY_POWER_LAW && !(c.k > 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the power law needs k > 0");
    if (c.model == ORC_VISCOSITY_CARREAU && (!(c.mu_zero >= 0.) || !(c.mu_inf >= 0.) || !(c.lambda >= 0.)))
        return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: Carreau needs mu_zero, mu_inf and lambda >= 0");
    return ORC_OK;
}

int exchange_velocities(SolverState &s) {
    if (!s.mesh->halo.active()) return ORC_OK;
    double *f[3] = {s.u.p, s.v.p, s.w.p};
    return s.mesh->halo.exchange(f, 3);
}

// the viscosity's ghosts, then a_di and b_*_di from it
int exchange_and_rebuild(SolverState &s) {
    if (s.mesh->halo.active()) ORC_TRY(s.mesh->halo.exchange(s.vis.mu.p));
    return k_diffusion_var(s);
}

int status_of(SolverState &s, const char *what) {
    int h = fetch_status(s);
    if (s.mesh->halo.active()) h = comm_global_status(h);
    if (h == ORC_ERR_SINGULAR_MATRIX) return set_error(h, "%s: singular least-squares system", what);
    if (h != ORC_OK) return set_error(h, "%s: a boundary face lies in a zone whose type the assembly does not support", what);
    return ORC_OK;
}

}  // namespace

int k_viscosity(SolverState &s, double *mu_out, double *g_out, bool relax) {
    OrcMesh &m = *s.mesh;
    const OrcViscosity &c = s.vis.c;
    ViscosityArgs A{};
    A.u = s.u.p; A.v = s.v.p; A.w = s.w.p;
    A.field = s.vis.field.p;
    A.mu = mu_out; A.g = g_out;
    A.model = c.model;
    A.relax = relax ? 1 : 0;
    A.k = c.k; A.n = c.n; A.mu_zero = c.mu_zero; A.mu_inf = c.mu_inf; A.lambda = c.lambda; A.cs = c.cs;
    A.mu_min = c.mu_min; A.mu_max = c.mu_max; A.relaxation = c.relaxation;
    A.rho = s.rho; A.mu_lam = s.mu;
    const OrcWallDamping &wd = s.vis.wd;
    A.damping = ORC_WALL_DAMPING_NONE;
    A.wall_d = nullptr;
    A.kappa = wd.kappa; A.a_plus = wd.a_plus; A.u_tau = wd.u_tau;
    if (c.model == ORC_VISCOSITY_SMAGORINSKY && wd.mode != ORC_WALL_DAMPING_NONE) {
        A.damping = wd.mode;
        ORC_TRY(wall_distance_default(m, &A.wall_d));  // the mesh's cached field; searched here at first use
    }
    const int g = grid_for(s.n_own);
    const bool lsq = s.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES, damped = A.wall_d != nullptr;
    auto kernel = lsq ? (damped ? viscosity_cell_k<true, true> : viscosity_cell_k<true, false>)
                      : (damped ? viscosity_cell_k<false, true> : viscosity_cell_k<false, false>);
    hipLaunchKernelGGL(kernel, dim3(g), dim3(kBlock), 0, ctx().stream, m.dev(), A, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_diffusion_var(SolverState &s) {
    OrcMesh &m = *s.mesh;
    hipLaunchKernelGGL(diffusion_var_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), s.vis.mu.p,
                       s.vis.c.face_interpolation == ORC_VISCOSITY_FACE_HARMONIC ? 1 : 0, s.a_di.p, s.b_u_di.p, s.b_v_di.p, s.b_w_di.p,
                       s.dev_status.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_viscosity_update(SolverState &s) {
    SolverState::Viscosity &V = s.vis;
    if (V.c.model != ORC_VISCOSITY_FIELD) {
        ORC_TRY(k_viscosity(s, V.mu.p, nullptr, !V.first && V.c.relaxation < 1.));
        V.first = false;
    }
    return exchange_and_rebuild(s);
}

}  // namespace orc

using namespace orc;

extern "C" {

static_assert(sizeof(OrcViscosity) == 80 && offsetof(OrcViscosity, model) == 0 && offsetof(OrcViscosity, face_interpolation) == 4 &&
                  offsetof(OrcViscosity, k) == 8 && offsetof(OrcViscosity, n) == 16 && offsetof(OrcViscosity, mu_zero) == 24 &&
                  offsetof(OrcViscosity, mu_inf) == 32 && offsetof(OrcViscosity, lambda) == 40 && offsetof(OrcViscosity, cs) == 48 &&
                  offsetof(OrcViscosity, mu_min) == 56 && offsetof(OrcViscosity, mu_max) == 64 && offsetof(OrcViscosity, relaxation) == 72,
              "OrcViscosity is part of the ABI (orc_amd/settings.py Viscosity mirrors it)");

void orc_viscosity_default(OrcViscosity *c) {
    if (!c) return;
    *c = OrcViscosity{};
    c->model = ORC_VISCOSITY_POWER_LAW;  // with n = 1: Newtonian, mu = k
    c->face_interpolation = ORC_VISCOSITY_FACE_ARITHMETIC;
    c->k = 1e-3; c->n = 1.;
    c->mu_zero = 1e-3; c->mu_inf = 0.; c->lambda = 1.;
    c->cs = 0.17;
    c->mu_min = 1e-12; c->mu_max = 1e12;
    c->relaxation = 1.;
}

int orc_solver_set_viscosity(OrcSolver *s, const OrcViscosity *c) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    SolverState::Viscosity &V = st.vis;
    if (!c) {  // back to the constant mu: k_diffusion's a_di and wall terms, nothing of the arm is launched from here on
        if (st.ts.on && (st.ts.c.groups & ORC_STAT_GROUP_VISCOSITY))
            return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the time statistics' VISCOSITY group is on (orc_solver_set_time_statistics)");
        if (st.scalar_gamma_reads_viscosity())
            return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the scalar's EDDY diffusivity is on (orc_solver_set_scalar_diffusivity)");
        const bool was_on = V.on;
        ORC_HIP(hipStreamSynchronize(ctx().stream));
        const OrcWallDamping wd = V.wd;  // the damping setting is the solver's, not the arm's: it waits for the next SMAGORINSKY
        V = SolverState::Viscosity();
        V.wd = wd;
        if (was_on) ORC_TRY(k_diffusion(st));
        return ORC_OK;
    }
    ORC_TRY(validate(*c));
    if (st.scalar_gamma_reads_viscosity() && c->model != ORC_VISCOSITY_SMAGORINSKY && c->model != ORC_VISCOSITY_FIELD)
        return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the scalar's EDDY diffusivity needs model SMAGORINSKY or FIELD "
                                               "(orc_solver_set_scalar_diffusivity)");
    // the in-place diagonal mode is the reference's own, with the reference's constant mu (as the transient arm refuses it)
    if (st.settings.frozen_diagonals == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: not available with frozen_diagonals = 0");
    if (c->model == ORC_VISCOSITY_FIELD && !V.has_field)
        return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: the FIELD model needs orc_solver_set_viscosity_field first");
    const size_t n = (size_t)std::max<int64_t>(st.n, 1);
    if (V.mu.n < n) { ORC_TRY(V.mu.alloc(n)); ORC_TRY(V.mu.zero()); }
    V.c = *c;
    V.on = true;
    V.first = true;
    if (c->model == ORC_VISCOSITY_FIELD) {
        ORC_TRY(vec_copy(V.mu.p, V.field.p, st.n));
    } else {
        ORC_TRY(exchange_velocities(st));
        ORC_TRY(k_viscosity(st, V.mu.p, nullptr, false));
    }
    ORC_TRY(exchange_and_rebuild(st));
    return status_of(st, "viscosity");
}

int orc_solver_set_wall_damping(OrcSolver *s, const OrcWallDamping *w) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    SolverState::Viscosity &V = st.vis;
    OrcWallDamping next = V.wd;
    if (w) {
        ORC_TRY(wall_damping_validate(*w));
        next = *w;
    } else {
        next.mode = ORC_WALL_DAMPING_NONE;
    }
    V.wd = next;
    if (!V.on || V.c.model != ORC_VISCOSITY_SMAGORINSKY) return ORC_OK;  // takes effect when SMAGORINSKY is switched on
    V.first = true;
    ORC_TRY(exchange_velocities(st));
    ORC_TRY(k_viscosity(st, V.mu.p, nullptr, false));
    ORC_TRY(exchange_and_rebuild(st));
    return status_of(st, "wall damping");
}

int orc_solver_set_viscosity_field(OrcSolver *s, const double *mu) {
    ORC_TRY(ensure_init());
    if (!s || !mu) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity field: null argument");
    SolverState &st = s->st;
    SolverState::Viscosity &V = st.vis;
    const size_t n = (size_t)st.n;
    for (size_t i = 0; i < n; ++i)
        if (!(mu[i] > 0.) || !std::isfinite(mu[i]))
            return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity field: entry %lld is not positive and finite", (long long)i);
    ORC_TRY(upload_cells(*st.mesh, mu, V.field));
    V.has_field = true;
    if (V.on && V.c.model == ORC_VISCOSITY_FIELD) {
        ORC_TRY(vec_copy(V.mu.p, V.field.p, st.n));
        ORC_TRY(exchange_and_rebuild(st));
        return status_of(st, "viscosity field");
    }
    return ORC_OK;
}

int orc_solver_get_viscosity(OrcSolver *s, double *mu) {
    ORC_TRY(ensure_init());
    if (!s || !mu) return set_error(ORC_ERR_BAD_ARGUMENT, "viscosity: null argument");
    SolverState &st = s->st;
    if (!st.vis.on) {
        std::fill(mu, mu + st.n, st.mu);
        return ORC_OK;
    }
    return download_cells(*st.mesh, st.vis.mu.p, mu);
}

int orc_solver_evaluate_viscosity(OrcSolver *s, double *mu, double *strain_rate) {
    ORC_TRY(ensure_init());
    if (!s || !mu) return set_error(ORC_ERR_BAD_ARGUMENT, "evaluate viscosity: null argument");
    SolverState &st = s->st;
    if (!st.vis.on) return set_error(ORC_ERR_BAD_ARGUMENT, "evaluate viscosity: the arm is off (orc_solver_set_viscosity)");
    const size_t n = (size_t)std::max<int64_t>(st.n, 1);
    DevBuf<double> m_t, g_t;
    ORC_TRY(m_t.alloc(n)); ORC_TRY(m_t.zero());  // the ghost cells' entries of a partitioned mesh stay zero
    ORC_TRY(g_t.alloc(n)); ORC_TRY(g_t.zero());
    ORC_TRY(exchange_velocities(st));
    ORC_TRY(k_viscosity(st, m_t.p, g_t.p, false));
    ORC_TRY(download_cells(*st.mesh, m_t.p, mu));
    if (strain_rate) ORC_TRY(download_cells(*st.mesh, g_t.p, strain_rate));
    return status_of(st, "evaluate viscosity");
}

int orc_solver_get_diffusion(OrcSolver *s, double *a_di, double *b_u_di, double *b_v_di, double *b_w_di) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    OrcMesh &m = *st.mesh;
    if (a_di) {
        DevBuf<double> tmp;
        ORC_TRY(tmp.ensure((size_t)std::max<int64_t>(m.pat.nnz, 1)));
        ORC_TRY(sell_export_values(m.pat, st.a_di.p, tmp.p));
        ORC_TRY(tmp.download(a_di, (size_t)m.pat.nnz));
    }
    const size_t n = (size_t)st.n;
    if (b_u_di) ORC_TRY(st.b_u_di.download(b_u_di, n));
    if (b_v_di) ORC_TRY(st.b_v_di.download(b_v_di, n));
    if (b_w_di) ORC_TRY(st.b_w_di.download(b_w_di, n));
    return ORC_OK;
}

int orc_bench_viscosity(OrcSolver *s, int reps, double avg_ms[2]) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    SolverState &st = s->st;
    if (!st.vis.on) return set_error(ORC_ERR_BAD_ARGUMENT, "bench viscosity: the arm is off (orc_solver_set_viscosity)");
    if (reps < 1) reps = 1;
    DevBuf<double> scratch;  // the law pass writes here: the solver's field keeps its bits; the rebuild rewrites a_di with the same values
    ORC_TRY(scratch.alloc((size_t)std::max<int64_t>(st.n, 1)));
    ORC_TRY(scratch.zero());
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    int status = ORC_OK;
    for (int pass = 0; pass < 2 && status == ORC_OK; ++pass) {
        auto launch = [&] { return pass == 0 ? k_viscosity(st, scratch.p, nullptr, false) : k_diffusion_var(st); };
        status = launch();  // warm-up
        if (status == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) status = set_error(ORC_ERR_HIP, "hipEventRecord failed");
        for (int i = 0; i < reps && status == ORC_OK; ++i) status = launch();
        float ms = 0.f;
        if (status == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                                 hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
            status = set_error(ORC_ERR_HIP, "timing the viscosity passes failed");
        avg_ms[pass] = (double)ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // scratch is freed on return
    return status;
}

}  // extern "C"
