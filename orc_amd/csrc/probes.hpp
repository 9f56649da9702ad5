// probes.hpp — the sampler's interface (probes.hip): the located point set, the locate, the solver's field table and the sampler itself.
#pragma once
#include <vector>

#include "assembly.hpp"

// The located points of one mesh, on the device in the search's (Morton) order: position k holds the caller's point order[k].
struct OrcProbes {
    OrcMesh *mesh = nullptr;
    int64_t n = 0;
    std::vector<int64_t> order;
    orc::DevBuf<double> x, y, z;                    // [n]
    orc::DevBuf<int32_t> cell, status, steps, zone;  // [n]: the final cell (internal numbering), OrcProbeStatus, moves, zone or -1
    orc::DevBuf<double> excess, off;                // [n] the last largest g; [3][n] x - x_cell
};

namespace orc {

// orc_probes_create's locate (Morton order, search, fold, walk); NULL + *status on failure.  cull / forced_slabs: the debug entry's switches
OrcProbes *locate(OrcMesh *m, int64_t n, const double *xyz, bool cull, int forced_slabs, int *status);
// THE field table of a solver: the OrcProbeField-ordered sources — PHI null while the scalar arm is off, MU null while the viscosity arm
// is off, and then the constant `mu` stands for it.  The sampler, the group reports and the cuts all read this one.
struct SolverFields {
    const double *src[ORC_PROBE_N];
    double mu;
};
inline SolverFields solver_field_table(const SolverState &s) {
    return {{s.u.p, s.v.p, s.w.p, s.p.p, s.sc.on ? s.sc.phi.p : nullptr, s.cell_viscosity()}, s.mu};
}
// probe_sample_k on n points given by cell (internal numbering) and offset [3][n]: the fields of `mask` into out_dev [popcount][n],
// asynchronous on ctx().stream
int launch_sample(const SolverState &s, const int32_t *cell, const double *off, int64_t n, uint32_t mask, int32_t interpolation, double *out_dev,
                  int *status_dev);
// mask, interpolation and gradient scheme as orc_solver_sample_probes refuses them
int validate_fields(const SolverState &s, uint32_t mask, int32_t interpolation);
// the sampler's status word as a status with its message
int sample_status(int h);
// launch_sample into buffers of its own and the result on the host: a zeroed status word, the launch, the download into out
// [popcount][n] (null = none: the call only checks), the status word as a status, the caller's order (null = the device order).
// keep_status (may be null): the status word's buffer, left zeroed on success for a caller that goes on sampling
int sample_to_host(const SolverState &s, const int32_t *cell, const double *off, int64_t n, uint32_t mask, int32_t interpolation,
                   const std::vector<int64_t> *order, double *out, DevBuf<int> *keep_status = nullptr);

}  // namespace orc
