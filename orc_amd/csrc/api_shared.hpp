// api_shared.hpp — what the host-boundary files (api_solver.cpp, api_transient.cpp, api_oneshot.cpp) share.
#pragma once
#include "assembly.hpp"
#include "convergence.hpp"

namespace orc {

// CSR values of the mesh pattern (host, ORC's element order) <-> a SELL value array on the device; tmp is scratch the caller owns
inline int upload_csr_values(OrcMesh &m, const double *host_vals, DevBuf<double> &sell, DevBuf<double> &tmp) {
    ORC_TRY(tmp.upload(host_vals, (size_t)m.pat.nnz));
    return sell_import_values(m.pat, tmp.p, sell.p);
}
inline int download_csr_values(OrcMesh &m, const DevBuf<double> &sell, double *host_vals, DevBuf<double> &tmp) {
    ORC_TRY(tmp.ensure((size_t)m.pat.nnz));
    ORC_TRY(sell_export_values(m.pat, sell.p, tmp.p));
    return tmp.download(host_vals, (size_t)m.pat.nnz);
}

// A drop-in for solver::solve_steady must not hide that the breakdown guard (default on) kept a solve alive where the
// reference divides 0/0 and panics "solution diverged" (solver.rs:217-221): an ORC_OK return then carries a note.
struct GuardNote {
    int64_t before;
    GuardNote() : before(orc_breakdown_guard_events(0)) {}
    void leave(int status) const {
        if (status != ORC_OK) return;
        const int64_t fired = orc_breakdown_guard_events(0) - before;
        if (fired > 0) set_error(ORC_OK, "breakdown guard fired in %lld solve(s): the reference would have returned NaN (linear_algebra.rs:255-268)", (long long)fired);
        else ctx().last_error.clear();
    }
};

// SIMPLE iterations until the last record passes the check (not before c.min_iterations) or max_iterations are through; rep (8
// doubles, may be null) keeps the last iteration's report, each(it) is called after iteration `it` (counted from 1)
template <class Each>
int iterate_until(SolverState &st, uint64_t max_iterations, const OrcConvergence &c, double *rep, uint64_t *done, int32_t *converged, Each &&each) {
    uint64_t it = 0;
    int32_t ok = 0;
    int status = ORC_OK;
    while (it < max_iterations && !ok && status == ORC_OK) {
        status = solver_iterate(st, 1, rep);
        if (status != ORC_OK) break;
        ++it;
        each(it);
        if (it >= c.min_iterations) ok = convergence_check(c, st.mon.history.data() + st.mon.history.size() - ORC_RESIDUAL_N, nullptr);
    }
    if (done) *done = it;
    if (converged) *converged = ok;
    return status;
}

// api_transient.cpp: one time step — shift the levels (n-1 <- n, n <- current fields), then up to inner_iterations SIMPLE iterations
// and the arms that follow a step; row (10 doubles, may be null): the last iteration's report, the iterations used, the time reached
int advance_one(SolverState &st, double *row);

}  // namespace orc
