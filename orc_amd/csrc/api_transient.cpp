// api_transient.cpp — C ABI of implicit time stepping on the resident solver (OrcTransient): the arm, its time levels, the time step.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>

#include "api_shared.hpp"
#include "cell_order.hpp"

using namespace orc;

namespace {

bool positive_finite(double x) { return x > 0. && std::isfinite(x); }

bool control_valid(const OrcTimeStepControl &c) {
    return positive_finite(c.target_courant) && positive_finite(c.dt_min) && positive_finite(c.dt_max) && c.dt_min <= c.dt_max &&
           c.max_growth >= 1. && c.max_growth <= 2. && c.max_shrink > 0. && c.max_shrink <= 1. && c.interval >= 1 && c.reserved0 == 0 &&
           c.reserved1 == 0;
}

// THE law (orc_types.h OrcTimeStepControl, DESIGN §3 "Adaptive time stepping"); c valid, dt positive, rate finite and >= 0
double step_law(const OrcTimeStepControl &c, double dt, double rate_max) {
    const double want = rate_max > 0. ? c.target_courant / rate_max : c.dt_max;
    double next = std::min(std::max(want, dt * c.max_shrink), dt * c.max_growth);
    next = std::min(std::max(next, c.dt_min), c.dt_max);
    return next;
}

// The end of a step: the step history moves on (dt_last <- the step just taken), and while control is on and the step is due the
// Courant reduction of the fields just reached chooses the next step — one synchronisation; nothing is launched with control off.
int step_control(SolverState &st) {
    SolverState::StepControl &K = st.ctl;
    const double used = st.dt;
    st.dt_before_last = st.dt_last;
    st.dt_last = used;
    double rate = std::numeric_limits<double>::quiet_NaN();
    int64_t cell = -1;
    int status = ORC_OK;
    if (K.on && ++K.step % K.c.interval == 0) {
        ORC_TRY(courant_dev(st, &rate, &cell, nullptr));
        if (!(rate >= 0.) || !std::isfinite(rate)) status = set_error(ORC_ERR_SOLUTION_DIVERGED, "time step control: the convective rate is %g", rate);
        else st.dt = step_law(K.c, used, rate);
    }
    if (K.on || K.manual) {
        const double row[4] = {st.time, used, rate, (double)cell};
        K.history.insert(K.history.end(), row, row + 4);
    }
    return status;
}

}  // namespace

namespace orc {

int advance_one(SolverState &st, double *row /*10*/) {
    if (st.time_levels >= 1)
        for (int k = 0; k < 3; ++k) ORC_TRY(vec_copy(st.lev[3 + k].p, st.lev[k].p, st.n));
    const double *cur[3] = {st.u.p, st.v.p, st.w.p};
    for (int k = 0; k < 3; ++k) ORC_TRY(vec_copy(st.lev[k].p, cur[k], st.n));
    st.time_levels = std::min(st.time_levels + 1, 2);
    st.time += st.dt;
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
    return step_control(st);  // last: the arms above saw the step taken and the step before it
}

}  // namespace orc

extern "C" {

int orc_solver_set_transient(OrcSolver *s, const OrcTransient *t) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!t) {  // back to steady SIMPLE: k_momentum launches nothing new from here on
        st.ctl.on = st.ctl.manual = false;
        st.ctl.history.clear();
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
    st.dt = st.dt_last = st.dt_before_last = t->dt;
    st.ctl.on = st.ctl.manual = false;
    st.ctl.step = 0;
    st.ctl.history.clear();
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
    st.dt_last = st.dt_before_last = st.dt;  // equal steps led here, unless orc_solver_set_time_state says otherwise
    return ORC_OK;
}

// ---------------------------------------------------------------- adaptive time stepping (OrcTimeStepControl)
static_assert(sizeof(OrcTimeStepControl) == 56 && offsetof(OrcTimeStepControl, target_courant) == 0 && offsetof(OrcTimeStepControl, dt_min) == 8 &&
                  offsetof(OrcTimeStepControl, dt_max) == 16 && offsetof(OrcTimeStepControl, max_growth) == 24 &&
                  offsetof(OrcTimeStepControl, max_shrink) == 32 && offsetof(OrcTimeStepControl, interval) == 40 &&
                  offsetof(OrcTimeStepControl, reserved0) == 48 && offsetof(OrcTimeStepControl, reserved1) == 52,
              "OrcTimeStepControl is part of the ABI (orc_amd/settings.py TimeStepControl mirrors it)");

void orc_time_step_control_default(OrcTimeStepControl *c) {
    if (!c) return;
    *c = OrcTimeStepControl{0.5, 1e-12, 1e12, 1.2, 0.5, 1, 0, 0};
}

int orc_time_step_next(const OrcTimeStepControl *c, double dt, double rate_max, double *dt_next) {
    if (!c || !dt_next) return set_error(ORC_ERR_BAD_ARGUMENT, "time step: null argument");
    if (!control_valid(*c)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step: a control field is outside its range");
    if (!positive_finite(dt)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step: dt must be positive and finite");
    if (!(rate_max >= 0.) || !std::isfinite(rate_max)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step: the rate must be finite and >= 0");
    *dt_next = step_law(*c, dt, rate_max);
    return ORC_OK;
}

int orc_solver_set_time_step(OrcSolver *s, double dt) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "time step without orc_solver_set_transient");
    if (!positive_finite(dt)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step: dt must be positive and finite");
    st.dt = dt;
    st.ctl.manual = true;
    return ORC_OK;
}

int orc_solver_set_time_step_control(OrcSolver *s, const OrcTimeStepControl *c) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "time step control without orc_solver_set_transient");
    if (!c) {  // off: advance launches nothing of the control from here on; the history stays until orc_solver_set_transient
        st.ctl.on = false;
        return ORC_OK;
    }
    if (!control_valid(*c)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step control: a field is outside its range");
    if (!(c->dt_min <= st.dt && st.dt <= c->dt_max))
        return set_error(ORC_ERR_BAD_ARGUMENT, "time step control: [dt_min, dt_max] does not contain the next step %g", st.dt);
    st.ctl.c = *c;
    st.ctl.on = true;
    st.ctl.step = 0;
    return ORC_OK;
}

int orc_solver_get_time_state(OrcSolver *s, double *time, double *dt_next, double *dt_last, double *dt_before_last) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    const SolverState &st = s->st;
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "time state without orc_solver_set_transient");
    if (time) *time = st.time;
    if (dt_next) *dt_next = st.dt;
    if (dt_last) *dt_last = st.dt_last;
    if (dt_before_last) *dt_before_last = st.dt_before_last;
    return ORC_OK;
}

int orc_solver_set_time_state(OrcSolver *s, double time, double dt_last, double dt_before_last) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "time state without orc_solver_set_transient");
    if (!(time >= 0.) || !std::isfinite(time) || !positive_finite(dt_last) || !positive_finite(dt_before_last))
        return set_error(ORC_ERR_BAD_ARGUMENT, "time state: time must be >= 0, the steps positive, all finite");
    st.time = time;
    st.dt_last = dt_last;
    st.dt_before_last = dt_before_last;
    return ORC_OK;
}

int64_t orc_solver_time_step_count(OrcSolver *s) { return s ? (int64_t)(s->st.ctl.history.size() / 4) : 0; }

int orc_solver_time_step_history(OrcSolver *s, uint64_t first, uint64_t count, double *out) {
    if (!s || (!out && count)) return set_error(ORC_ERR_BAD_ARGUMENT, "time step history: null argument");
    const std::vector<double> &h = s->st.ctl.history;
    const uint64_t have = h.size() / 4;
    if (first > have || count > have - first) return set_error(ORC_ERR_BAD_ARGUMENT, "time step history: the range is past the %llu rows", (unsigned long long)have);
    std::copy(h.begin() + 4 * first, h.begin() + 4 * (first + count), out);
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
