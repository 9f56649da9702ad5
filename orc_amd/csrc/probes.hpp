// probes.hpp — what tracers.hip takes from probes.hip: the located point set, the locate itself and the sampler's launch.
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

// orc_probes_create's locate (culled search, fold, walk); NULL + *status on failure
OrcProbes *probes_locate(OrcMesh *m, int64_t n, const double *xyz, int *status);
// probe_sample_k on n points given by cell (internal numbering) and offset [3][n]: the fields of `mask` into out_dev [popcount][n],
// asynchronous on ctx().stream
int probes_launch_sample(const SolverState &s, const int32_t *cell, const double *off, int64_t n, uint32_t mask, int32_t interpolation,
                         double *out_dev, int *status_dev);
// mask, interpolation and gradient scheme as orc_solver_sample_probes refuses them
int probes_validate_fields(const SolverState &s, uint32_t mask, int32_t interpolation);
// the sampler's status word as a status with its message
int probes_sample_status(int h);

}  // namespace orc
