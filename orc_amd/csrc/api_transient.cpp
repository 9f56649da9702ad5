// api_transient.cpp — C ABI of implicit time stepping on the resident solver (OrcTransient): the arm, its time levels, the time step.
#include <algorithm>
#include <cmath>

#include "api_shared.hpp"
#include "cell_order.hpp"

using namespace orc;

namespace orc {

int advance_one(SolverState &st, double *row /*10*/) {
    if (st.time_levels >= 1)
        for (int k = 0; k < 3; ++k) ORC_TRY(vec_copy(st.lev[3 + k].p, st.lev[k].p, st.n));
    const double *cur[3] = {st.u.p, st.v.p, st.w.p};
    for (int k = 0; k < 3; ++k) ORC_TRY(vec_copy(st.lev[k].p, cur[k], st.n));
    st.time_levels = std::min(st.time_levels + 1, 2);
    st.time += st.tr.dt;
    const double tol = st.tr.inner_tolerance;
    double rep[8] = {0., 0., 0., 0., 0., 0., 0., 0.}, first_vc = 0., first_pc = 0.;
    uint64_t used = 0;
    for (uint64_t it = 0; it < st.tr.inner_iterations; ++it) {
        ORC_TRY(solver_iterate(st, 1, rep));
        ++used;
        if (it == 0) { first_vc = rep[6]; first_pc = rep[7]; }
        if (tol > 0. && (rep[6] < tol * first_vc || rep[6] == 0.) && (rep[7] < tol * first_pc || rep[7] == 0.)) break;
    }
    ORC_TRY(scalar_step_dev(st));  // scalar arm on: its levels shift and it is solved once on this step's flow
    ORC_TRY(stats_step_dev(st));   // statistics arm on: the step is counted and, when due, sampled with weight dt
    ORC_TRY(probes_step_dev(st));  // probe history on: the step is counted and, when due, recorded at the time reached
    ORC_TRY(tracers_step_dev(st)); // tracer tracking on: the set moves through the velocity just reached
    ORC_TRY(groups_step_dev(st));  // group history on: the step is counted and, when due, reduced over the groups at the time reached
    if (row) {
        std::copy(rep, rep + 8, row);
        row[8] = (double)used;
        row[9] = st.time;
    }
    return ORC_OK;
}

}  // namespace orc

extern "C" {

int orc_solver_set_transient(OrcSolver *s, const OrcTransient *t) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!t) {  // back to steady SIMPLE: k_momentum launches nothing new from here on
        st.transient = false;
        st.time_levels = 0;
        st.sc.levels = 0;
        return ORC_OK;
    }
    if (!(t->dt > 0.) || !std::isfinite(t->dt)) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: dt must be positive and finite");
    if (t->scheme != ORC_TIME_EULER && t->scheme != ORC_TIME_BDF2) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: unknown time scheme %d", t->scheme);
    if (t->reserved0 != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: reserved0 must be 0");
    if (t->inner_iterations == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: inner_iterations must be at least 1");
    if (!(t->inner_tolerance >= 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: inner_tolerance must be >= 0");
    // the in-place diagonal reads of frozen_diagonals = 0 would see this iteration's diagonals without the time term
    if (st.settings.frozen_diagonals == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "transient: not available with frozen_diagonals = 0");
    for (auto &b : st.lev) ORC_TRY(b.ensure((size_t)std::max<int64_t>(st.n, 1)));
    st.tr = *t;
    st.transient = true;
    st.time_levels = 0;
    st.sc.levels = 0;
    st.time = 0.;
    return ORC_OK;
}

int orc_solver_set_time_levels(OrcSolver *s, const double *u_n, const double *v_n, const double *w_n, const double *u_nm1,
                               const double *v_nm1, const double *w_nm1) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "time levels without orc_solver_set_transient");
    if (!u_n || !v_n || !w_n) return set_error(ORC_ERR_BAD_ARGUMENT, "level n must be given");
    const int given = (u_nm1 != nullptr) + (v_nm1 != nullptr) + (w_nm1 != nullptr);
    if (given != 0 && given != 3) return set_error(ORC_ERR_BAD_ARGUMENT, "level n-1: all of u, v, w or none");
    const double *src[6] = {u_n, v_n, w_n, u_nm1, v_nm1, w_nm1};
    for (int k = 0; k < (given ? 6 : 3); ++k) ORC_TRY(upload_cells(*st.mesh, src[k], st.lev[k]));
    st.time_levels = given ? 2 : 1;
    return ORC_OK;
}

int orc_solver_advance(OrcSolver *s, uint64_t time_steps, double *report) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    if (!s->st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "orc_solver_advance without orc_solver_set_transient");
    GuardNote note;
    int st = ORC_OK;
    for (uint64_t k = 0; k < time_steps && st == ORC_OK; ++k) st = advance_one(s->st, report ? report + 10 * k : nullptr);
    note.leave(st);
    return st;
}

}  // extern "C"
