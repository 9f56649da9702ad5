// schedule.hpp — which momentum schedule a SIMPLE iteration runs and when the p' hierarchy is built: one pure decision.
// Every schedule computes the same bits, so no test of results can see this decision change; it would show as lost speed, or on a
// partitioned mesh as ranks that issue different collectives.  Hence the rule this header enforces by including nothing of the
// runtime: the decision reads the solver's settings and switches and the mesh alone — never the thread context (its reduction
// order is whatever the last solve left there: ADVICE r04), never the environment.  tests/test_abi_cpu.py pins the whole table
// through orc_debug_schedule.
#pragma once
#include "../../include/orc_types.h"

namespace orc {

enum MomentumSchedule {
    kMomentumSequential = 0,        // u, v, w one after the other on the library stream (solver.rs:99-136 as written)
    kMomentumLanes = 1,             // the three systems side by side: a stream, an arena and a host thread each
    kMomentumLanesPartitioned = 2,  // the same with every collective left on the library stream (Multigrid on a partitioned mesh)
    kMomentumLockStep = 3           // the three systems in lock-step on their shared pattern (MatView3)
};
enum PHierarchySchedule {
    kPHierarchyInSolve = 0,  // nothing ahead of the p' solve: a Multigrid arm builds its hierarchy itself
    kPHierarchyEarly = 1,    // on its own stream and host thread from the moment the momentum diagonals exist
    kPHierarchyLate = 2      // started by the lock-step solve once the momentum set-ups are through (it borrows lane 0's scratch arena)
};

struct ScheduleInputs {
    // the solver's five switches (config.hpp, fixed at the solver's creation); the decision reads the first three
    bool concurrent_momentum = true, triple_momentum = true, early_p_hierarchy = true, two_stream_multigrid = true, sibling_pairing = true;
    bool partitioned = false;     // the mesh has a halo plan (one rank of several)
    bool debug_nan = false;       // ORC_DEBUG_NAN: fields are downloaded between the solves
    bool profiling = false;       // orc_profile_enable: everything stays on the library stream
    bool gs_slot_space = false;   // gs_slot_space_enabled(): the one-launch-per-colour u, v, w sweep exists
    int momentum_solver = 0;      // OrcSolverType of the settings
    int p_solver = 0;             // OrcSolverType of the p' solve (the settings', or orc_solver_set_pressure_solver's)
    int reduction_order = 0;      // OrcReductionOrder of the settings
};

struct Schedule {
    MomentumSchedule momentum;
    PHierarchySchedule p_hierarchy;
};

inline Schedule decide_schedule(const ScheduleInputs &in) {
    const int m = in.momentum_solver, mp = in.p_solver;
    const bool quiet = !in.debug_nan && !in.profiling;
    const bool concurrent = in.concurrent_momentum && quiet;
    const bool lanes = concurrent && !in.partitioned &&
                       (m == ORC_SOLVER_MULTIGRID || m == ORC_SOLVER_BICGSTAB || m == ORC_SOLVER_JACOBI || m == ORC_SOLVER_MULTIGRID_GS ||
                        m == ORC_SOLVER_BICGSTAB_GS_PRECOND || m == ORC_SOLVER_MULTICOLOR_GS);
    // Lock-step on one GPU: tree reductions only.  On a partitioned mesh (tree reductions there by construction, whatever the
    // settings say): N > 1 runs the schedule of the N = 1 headline, with a third of the momentum phase's halo exchanges and all-reduces.
    const bool lock_step = concurrent && in.triple_momentum &&
                           (in.partitioned ? (m == ORC_SOLVER_MULTIGRID || m == ORC_SOLVER_BICGSTAB)
                                           : (in.reduction_order != ORC_REDUCTION_REFERENCE &&
                                              (m == ORC_SOLVER_MULTIGRID || m == ORC_SOLVER_BICGSTAB ||
                                               (m == ORC_SOLVER_BICGSTAB_GS_PRECOND && in.gs_slot_space))));
    Schedule out;
    out.momentum = lock_step                                                     ? kMomentumLockStep
                   : lanes                                                       ? kMomentumLanes
                   : (concurrent && in.partitioned && m == ORC_SOLVER_MULTIGRID) ? kMomentumLanesPartitioned
                                                                                 : kMomentumSequential;
    // The p' hierarchy is needed after the momentum solves.  Beside the per-system lanes it is built from the start; in the
    // lock-step schedule the momentum set-ups are the critical path of the first phase (nothing bandwidth-bound but the
    // level-0 solve runs beside them), so it starts when they are through and runs beside the bandwidth-bound coarse levels.
    const bool ahead = in.early_p_hierarchy && quiet && (mp == ORC_SOLVER_MULTIGRID || mp == ORC_SOLVER_MULTIGRID_GS);
    out.p_hierarchy = !ahead                                                                               ? kPHierarchyInSolve
                      : (lock_step && m == ORC_SOLVER_MULTIGRID && mp == ORC_SOLVER_MULTIGRID) ? kPHierarchyLate
                                                                                                           : kPHierarchyEarly;
    return out;
}

}  // namespace orc
