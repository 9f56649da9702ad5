// api_oneshot.cpp — C ABI of the calls that take host arrays, do one thing and hand host arrays back: solver::solve_steady and its
// converged and time-stepped siblings, discretization::*, calculate_gradients and solver::initialize_*.
#include <algorithm>
#include <chrono>
#include <memory>

#include "api_shared.hpp"
#include "cell_order.hpp"

using namespace orc;

namespace {

// ---------------------------------------------------------------- what the three orc_solve_* drivers share
// begin: a solver of the mesh with the caller's fields in it; the transient arm (`tr`, may be null) is set before the fields.
// The caller starts its GuardNote next, steps, and hands both to oneshot_end.
int oneshot_begin(OrcMesh *m, const double *u, const double *v, const double *w, const double *p, const OrcSettings *settings, double rho,
                  double mu, const OrcTransient *tr, std::unique_ptr<OrcSolver> &s) {
    int st = ORC_OK;
    s.reset(orc_solver_create(m, settings, rho, mu, &st));
    if (!s) return st;
    if (tr) ORC_TRY(orc_solver_set_transient(s.get(), tr));
    return orc_solver_set_fields(s.get(), u, v, w, p);
}

// end: the post-loop gradients (solver.rs:227-242) when the stepping went well, the fields back in any case (the reference mutates
// them in place up to a panic), the guard's note; the stepping's status goes before the download's
int oneshot_end(OrcSolver &s, const GuardNote &note, int st, double *u, double *v, double *w, double *p) {
    if (st == ORC_OK) st = post_loop_gradients_dev(s.st);
    const int st2 = orc_solver_get_fields(&s, u, v, w, p);
    note.leave(st != ORC_OK ? st : st2);
    return st != ORC_OK ? st : st2;
}

// the wall-clock report of solver.rs:209-216: due at every interval-th step, ms = time since the last report / interval
struct ReportClock {
    OrcReportFn cb;
    void *user;
    uint64_t interval;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    bool due(uint64_t it) const { return cb && interval > 0 && it % interval == 0; }
    void report(uint64_t it, const double *rep /*the 8 values of solver_iterate*/) {
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - last).count() / (double)interval;
        last = now;
        cb(it, rep, rep + 3, rep[6], rep[7], ms, user);
    }
};

// a_{u,v,w}.get(i, i) of the caller's CSR values into du/dv/dw: what Rhie-Chow reads
int upload_diagonals(SolverState &t, const OrcMesh &m, const double *a_u_values, const double *a_v_values, const double *a_w_values) {
    std::vector<double> d((size_t)t.n);
    const double *mats[3] = {a_u_values, a_v_values, a_w_values};
    DevBuf<double> *diags[3] = {&t.du, &t.dv, &t.dw};
    for (int k = 0; k < 3; ++k) {
        for (int64_t c = 0; c < t.n_own; ++c) {
            const int64_t *row = m.h_col.data() + m.h_row_ptr[(size_t)c];
            const int64_t len = m.h_row_ptr[(size_t)c + 1] - m.h_row_ptr[(size_t)c];
            d[(size_t)c] = mats[k][m.h_row_ptr[(size_t)c] + (std::lower_bound(row, row + len, c) - row)];
        }
        ORC_TRY(diags[k]->upload(d.data(), (size_t)t.n));
    }
    return ORC_OK;
}

// the scheme triple initialize_flow hard-codes (solver.rs:301-304); q1_compat / breakdown_guard follow the caller
OrcSettings initializer_settings(const OrcSettings *settings) {
    OrcSettings t;
    orc_settings_default(&t);
    if (settings) { t.q1_compat = settings->q1_compat; t.breakdown_guard = settings->breakdown_guard; t.reduction_order = settings->reduction_order; }
    t.momentum = ORC_MOMENTUM_UD;
    t.velocity_interpolation = ORC_VINTERP_LINEAR_WEIGHTED;
    t.pressure_interpolation = ORC_PINTERP_LINEAR_WEIGHTED;
    return t;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- solver::solve_steady (solver.rs:26-244)
int orc_solve_steady(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings, double rho, double mu,
                     uint64_t iteration_count, uint64_t reporting_interval, OrcReportFn report_cb, void *user) {
    if (!m || !settings || !u || !v || !w || !p) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    std::unique_ptr<OrcSolver> s;
    ORC_TRY(oneshot_begin(m, u, v, w, p, settings, rho, mu, nullptr, s));
    GuardNote note;
    ReportClock clock{report_cb, user, reporting_interval};
    int st = ORC_OK;
    for (uint64_t it = 1; it <= iteration_count && st == ORC_OK; ++it) {
        double rep[8];
        const bool want = clock.due(it);
        st = solver_iterate(s->st, 1, want ? rep : nullptr);
        if (want && st == ORC_OK) clock.report(it, rep);
    }
    return oneshot_end(*s, note, st, u, v, w, p);
}

int orc_solve_steady_converged(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings, double rho, double mu,
                               const OrcConvergence *c, uint64_t max_iterations, uint64_t reporting_interval, OrcReportFn report_cb, void *user,
                               uint64_t *iterations_done, int32_t *converged, double *last_record) {
    ORC_TRY(ensure_init());
    if (!m || !settings || !u || !v || !w || !p || !c) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    if (!convergence_valid(*c)) return set_error(ORC_ERR_BAD_ARGUMENT, "solve_steady_converged: tolerances must be >= 0 and reserved0 must be 0");
    std::unique_ptr<OrcSolver> s;
    ORC_TRY(oneshot_begin(m, u, v, w, p, settings, rho, mu, nullptr, s));
    ORC_TRY(monitors_enable(s->st, true));
    GuardNote note;
    ReportClock clock{report_cb, user, reporting_interval};
    double rep[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    const int st = iterate_until(s->st, max_iterations, *c, rep, iterations_done, converged, [&](uint64_t it) {
        if (clock.due(it)) clock.report(it, rep);
    });
    if (last_record) {
        const std::vector<double> &h = s->st.mon.history;
        if (h.empty()) std::fill(last_record, last_record + ORC_RESIDUAL_N, 0.);
        else std::copy(h.end() - ORC_RESIDUAL_N, h.end(), last_record);
    }
    return oneshot_end(*s, note, st, u, v, w, p);
}

int orc_solve_transient(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings, double rho, double mu,
                        const OrcTransient *t, uint64_t time_steps, uint64_t reporting_interval, OrcReportFn report_cb, void *user) {
    if (!m || !settings || !t || !u || !v || !w || !p) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    std::unique_ptr<OrcSolver> s;
    ORC_TRY(oneshot_begin(m, u, v, w, p, settings, rho, mu, t, s));
    GuardNote note;
    ReportClock clock{report_cb, user, reporting_interval};
    int st = ORC_OK;
    for (uint64_t k = 1; k <= time_steps && st == ORC_OK; ++k) {
        double row[10];
        st = advance_one(s->st, row);
        if (clock.due(k) && st == ORC_OK) clock.report(k, row);
    }
    return oneshot_end(*s, note, st, u, v, w, p);
}

// ---------------------------------------------------------------- discretization::* with host arrays
int orc_build_momentum_diffusion_matrix(const OrcMesh *m, int diffusion_scheme, double mu, double *a_values, double *b_u,
                                        double *b_v, double *b_w) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "null mesh");
    OrcSettings st;
    orc_settings_default(&st);
    st.diffusion = diffusion_scheme;
    auto s = std::make_unique<OrcSolver>();
    ORC_TRY(solver_init(s->st, const_cast<OrcMesh *>(m), &st, 1.0, mu));
    DevBuf<double> tmp;
    ORC_TRY(download_csr_values(*s->st.mesh, s->st.a_di, a_values, tmp));
    const size_t n = (size_t)m->n_cells;
    ORC_TRY(s->st.b_u_di.download(b_u, n));
    ORC_TRY(s->st.b_v_di.download(b_v, n));
    ORC_TRY(s->st.b_w_di.download(b_w, n));
    return ORC_OK;
}

int orc_initialize_momentum_matrix(const OrcMesh *m, double *a_values) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "null mesh");
    OrcSettings st;
    orc_settings_default(&st);
    auto s = std::make_unique<OrcSolver>();
    ORC_TRY(solver_init(s->st, const_cast<OrcMesh *>(m), &st, 1.0, 1.0));
    DevBuf<double> tmp;
    return download_csr_values(*s->st.mesh, s->st.a_u, a_values, tmp);
}

int orc_build_momentum_advection_matrices(const OrcMesh *m, double *a_u_values, double *a_v_values, double *a_w_values, double *b_u,
                                          double *b_v, double *b_w, const double *a_di_values, const double *u, const double *v,
                                          const double *w, const double *p, const OrcSettings *settings, double rho,
                                          double peclet[3]) {
    if (!m || !settings) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    auto s = std::make_unique<OrcSolver>();
    SolverState &t = s->st;
    ORC_TRY(solver_init(t, const_cast<OrcMesh *>(m), settings, rho, 1.0));
    DevBuf<double> tmp;
    // a_di, and the incoming a_u/a_v/a_w whose diagonals Rhie-Chow reads (solver.rs:1068-1081)
    ORC_TRY(upload_csr_values(*t.mesh, a_di_values, t.a_di, tmp));
    ORC_TRY(upload_csr_values(*t.mesh, a_u_values, t.a_u, tmp));
    ORC_TRY(upload_csr_values(*t.mesh, a_v_values, t.a_v, tmp));
    ORC_TRY(upload_csr_values(*t.mesh, a_w_values, t.a_w, tmp));
    ORC_TRY(upload_diagonals(t, *m, a_u_values, a_v_values, a_w_values));
    // the diffusion RHS is added by the caller in the reference (solver.rs:80-82): return b without it
    ORC_TRY(t.b_u_di.zero()); ORC_TRY(t.b_v_di.zero()); ORC_TRY(t.b_w_di.zero());
    ORC_TRY(orc_solver_set_fields(s.get(), u, v, w, p));
    return orc_solver_assemble_momentum(s.get(), a_u_values, a_v_values, a_w_values, b_u, b_v, b_w, peclet);
}

int orc_build_pressure_correction_matrices(const OrcMesh *m, const double *u, const double *v, const double *w, const double *p,
                                           const double *a_u_values, const double *a_v_values, const double *a_w_values,
                                           const OrcSettings *settings, double rho, double *a_values, double *b) {
    if (!m || !settings) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    auto s = std::make_unique<OrcSolver>();
    SolverState &t = s->st;
    ORC_TRY(solver_init(t, const_cast<OrcMesh *>(m), settings, rho, 1.0));
    ORC_TRY(upload_diagonals(t, *m, a_u_values, a_v_values, a_w_values));
    ORC_TRY(orc_solver_set_fields(s.get(), u, v, w, p));
    return orc_solver_assemble_pressure(s.get(), a_values, b);
}

int orc_calculate_gradients(const OrcMesh *m, const double *u, const double *v, const double *w, const double *p,
                            const OrcSettings *settings, double *grad_p, double *grad_u) {
    if (!m || !settings) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    auto s = std::make_unique<OrcSolver>();
    SolverState &t = s->st;
    ORC_TRY(solver_init(t, const_cast<OrcMesh *>(m), settings, 1.0, 1.0));
    ORC_TRY(orc_solver_set_fields(s.get(), u, v, w, p));
    ORC_TRY(k_gradients(t, grad_u != nullptr));
    const size_t n = (size_t)t.n;
    if (grad_p) {
        std::vector<double> g(3 * n);
        ORC_TRY(t.gp.download(g.data(), 3 * n));
        for (size_t c = 0; c < n; ++c)
            for (int k = 0; k < 3; ++k) grad_p[3 * c + k] = g[k * n + c];
    }
    if (grad_u) {
        std::vector<double> g(9 * n);
        ORC_TRY(t.gu.download(g.data(), 9 * n));
        for (size_t c = 0; c < n; ++c)
            for (int k = 0; k < 9; ++k) grad_u[9 * c + k] = g[k * n + c];
    }
    return fetch_status(t);
}

// ---------------------------------------------------------------- solver::initialize_* (solver.rs:246-509)
int orc_check_boundary_conditions(const OrcMesh *m, int *constraint_type) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "null mesh");
    const int kind = check_boundary_conditions(*m);
    if (kind < 0) return set_error(-kind, "You must set boundary conditions.");
    if (constraint_type) *constraint_type = kind;
    return ORC_OK;
}

int orc_initialize_pressure_field(const OrcMesh *m, double *p) {
    if (!m || !p) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    const OrcSettings t = initializer_settings(nullptr);
    auto s = std::make_unique<OrcSolver>();
    ORC_TRY(solver_init(s->st, const_cast<OrcMesh *>(m), &t, 1.0, 1.0));
    ORC_TRY(upload_cells(*m, p, s->st.p));  // the incoming p: the reference overwrites it
    int st = initialize_pressure_field_dev(s->st);
    ORC_TRY(download_cells(*m, s->st.p.p, p));
    return st;
}

int orc_initialize_flow(const OrcMesh *m, double mu, double rho, uint64_t iteration_count, const OrcSettings *settings, double *u, double *v,
                        double *w, double *p) {
    if (!m || !u || !v || !w || !p) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    const OrcSettings t = initializer_settings(settings);
    auto s = std::make_unique<OrcSolver>();
    ORC_TRY(solver_init(s->st, const_cast<OrcMesh *>(m), &t, rho, mu));  // fields start at zero (:273-277)
    int st = initialize_flow_dev(s->st, iteration_count);
    int st2 = orc_solver_get_fields(s.get(), u, v, w, p);
    return st != ORC_OK ? st : st2;
}

// initialize_velocity_field (solver.rs:511-696): u, v, w from the potential psi; psi (optional) is what the reference
// writes to ./examples/psi.csv — the files themselves are left to the caller (orc_write_data / orc_write_gradients).
int orc_initialize_velocity_field(const OrcMesh *m, const OrcSettings *settings, double *u, double *v, double *w, double *psi) {
    if (!m || !u || !v || !w) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    const OrcSettings t = initializer_settings(settings);
    auto s = std::make_unique<OrcSolver>();
    ORC_TRY(solver_init(s->st, const_cast<OrcMesh *>(m), &t, 1.0, 1.0));
    int st = initialize_velocity_field_dev(s->st);
    int st2 = download_cells(*m, s->st.u.p, u);
    if (st2 == ORC_OK) st2 = download_cells(*m, s->st.v.p, v);
    if (st2 == ORC_OK) st2 = download_cells(*m, s->st.w.p, w);
    if (st2 == ORC_OK && psi) st2 = download_cells(*m, s->st.p_prime.p, psi);
    return st != ORC_OK ? st : st2;
}

// initialize_flow_new (solver.rs:354-410): the match has overlapping arms, so Hybrid takes the first one — PressureOnly |
// Hybrid -> initialize_pressure_field (velocities stay zero), VelocityOnly -> initialize_velocity_field (pressure stays zero).
int orc_initialize_flow_new(const OrcMesh *m, double mu, double rho, uint64_t iteration_count, double *u, double *v, double *w, double *p) {
    (void)mu; (void)rho; (void)iteration_count;
    if (!m || !u || !v || !w || !p) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    int kind = 0;
    ORC_TRY(orc_check_boundary_conditions(m, &kind));
    const size_t n = (size_t)m->n_cells;
    std::fill(u, u + n, 0.); std::fill(v, v + n, 0.); std::fill(w, w + n, 0.); std::fill(p, p + n, 0.);
    if (kind == 1) return orc_initialize_velocity_field(m, nullptr, u, v, w, nullptr);
    return orc_initialize_pressure_field(m, p);
}

}  // extern "C"
