// postproc_state.hpp — the state of the post-processing arms a SolverState holds by value (ts, ph, gh, tt) and what orc_solver_advance
// runs for each.  Every arm is off unless enabled, reads the fields and never writes them; snapshot / restore leave it alone.
#pragma once
#include <vector>

#include "deferred.hpp"

struct OrcProbes;
struct OrcCellGroups;
struct OrcTracers;

namespace orc {

struct SolverState;

// Running time statistics (orc_solver_set_time_statistics, time_stats.hip): every buffer allocated by the set call.
struct TimeStats {
    bool on = false;
    OrcTimeStatistics c{};
    uint32_t field_mask = 0;  // OrcStatField bits of the enabled groups
    int n_fields = 0;         // K = popcount(field_mask)
    DevBuf<double> acc;       // [K][n] SoA, enabled fields in enum order, internal cell order; ghost entries stay 0
    int64_t nb = 0;           // boundary faces (BOUNDARY group), else 0
    DevBuf<double> bnd, bnd_now;  // [5][nb]: the means, and the maps of the state being sampled
    DevBuf<int> bnd_status;   // boundary_map_k's status word
    double W = 0.;            // sum of the weights
    uint64_t samples = 0, step = 0;  // samples taken; orc_solver_advance steps since the arm was enabled
};

// What the probe and the group history share: every `interval`-th step of orc_solver_advance since the arm was enabled is recorded.  A
// record is made on the device, sent to the arm's pinned buffer behind it (Deferred) and joins the history at the next step, at a history
// call or when the arm goes off.
struct StepHistory {
    bool on = false;
    uint64_t interval = 1, step = 0;
    double pending_time = 0.;           // the time slot of the record on its way
    std::vector<double> times, values;  // k records: the time slots, and the records one after the other
    bool due() { return ++step % interval == 0; }  // counts the step
};

// the records [first, first + count) of `have`, or a refusal
inline int history_range(const char *what, uint64_t first, uint64_t count, uint64_t have) {
    if (first > have || count > have - first)
        return set_error(ORC_ERR_BAD_ARGUMENT, "%s: records [%llu, %llu) asked for, %llu kept", what, (unsigned long long)first,
                         (unsigned long long)(first + count), (unsigned long long)have);
    return ORC_OK;
}

// Probe history (orc_solver_set_probe_history, probes.hip): a record is sampled into `rec`; values holds the records in the caller's
// point order.
struct ProbeHistory : StepHistory {
    const OrcProbes *probes = nullptr;
    uint32_t mask = 0;
    int32_t interpolation = 0;
    int n_fields = 0;
    DevBuf<double> rec;    // [n_fields][n_points], the points in the probe set's device order
    DevBuf<int> status;    // probe_sample_k's status word
    Deferred<double> raw;  // [n_fields * n_points + 1]: the record, then the status word as a double
    void clear() { raw.release(); *this = ProbeHistory(); }  // the copy on its way lands first
};

// Group history (orc_solver_set_group_history, groups.hip): a record [G][1 + 6 F] is reduced into `rec`; values holds the records as the
// device wrote them.
struct GroupHistory : StepHistory {
    OrcCellGroups *groups = nullptr;
    uint32_t mask = 0;
    int32_t weighting = 0;
    int n_fields = 0;
    DevBuf<double> rec;        // one record as group_fold_k writes it
    Deferred<double> raw;      // the same
    std::vector<double> w_of;  // [G] the weight sums W: the group set's and the weighting's, the same in every record
    void clear() { raw.release(); *this = GroupHistory(); }
};

// Tracer tracking (orc_solver_set_tracer_tracking, tracers.hip): every step of orc_solver_advance moves the set by `substeps` substeps of
// dt / substeps (the step just taken) in the new velocity; the kernel's status word is sent to `raw` behind it and looked at by the next step.
struct TracerTracking {
    bool on = false;
    OrcTracers *set = nullptr;
    OrcTracerSettings c{};
    uint32_t substeps = 0;
    DevBuf<int> status;
    Deferred<int> raw;  // [1]
    void clear() { raw.release(); *this = TracerTracking(); }
};

// time statistics (time_stats.hip): what orc_solver_advance runs after scalar_step_dev — counts the step and, when the arm is on and the
// step is due, takes one sample of weight dt; asynchronous on ctx().stream, nothing while the arm is off
int stats_step_dev(SolverState &s);
// probe history (probes.hip): what orc_solver_advance runs after stats_step_dev — counts the step and, when the history is on and the
// step is due, samples one record on the device and starts its copy to the host; asynchronous on ctx().stream, nothing while it is off
int probes_step_dev(SolverState &s);
// tracer tracking (tracers.hip): what orc_solver_advance runs after probes_step_dev — while tracking is on, one launch that moves the
// set through the step's velocity; asynchronous on ctx().stream, nothing while it is off
int tracers_step_dev(SolverState &s);
// group history (groups.hip): what orc_solver_advance runs last — counts the step and, when the history is on and the step is due,
// reduces one record on the device and starts its copy to the host; asynchronous on ctx().stream, nothing while it is off
int groups_step_dev(SolverState &s);

}  // namespace orc
