// point_walk.hpp — the containment walk of DESIGN.md §3 "Point probes", shared by probe_walk_k (probes.hip: from the nearest centroid)
// and tracer_advect_k (tracers.hip: from the cell a particle was in).  Device code only; one body, the same bits for both callers.
#pragma once
#include "assembly.hpp"

#ifdef __HIPCC__
namespace orc {

struct WalkEnd {
    int status;   // OrcProbeStatus
    int moves;    // moves made
    int zone;     // the zone of the boundary face an OUTSIDE walk ended at, else -1
    double g;     // the last largest g
};

// From cell P (updated to the cell reached): at every cell the face f of its list with the largest g_f = (r.x n.x + r.y n.y) + r.z n.z,
// r = x - x_f, negated when P is not c0[f] (the first face among ties) — g <= 0 INSIDE, a boundary face OUTSIDE, else on to the
// neighbour, ORC_PROBE_WALK_LIMIT moves at most.  Every cell reached is c0 or c1 >= 0 of a face of an owned cell of an unpartitioned
// mesh: below n_cells.
__device__ __forceinline__ WalkEnd point_walk(const MeshDev &M, double x, double y, double z, int &P) {
    WalkEnd e{ORC_PROBE_STATUS_INSIDE, 0, -1, 0.};
    for (;;) {
        int fbest = -1;
        e.g = -INFINITY;
        for (int q = M.cfp[P]; q < M.cfp[P + 1]; ++q) {
            const int f = M.cf[q];
            const double rx = x - M.fcx[f], ry = y - M.fcy[f], rz = z - M.fcz[f];
            double g = (rx * M.nx[f] + ry * M.ny[f]) + rz * M.nz[f];
            if (M.c0[f] != P) g = -g;
            if (fbest < 0 || g > e.g) { e.g = g; fbest = f; }
        }
        if (fbest < 0 || e.g <= 0.) { e.status = ORC_PROBE_STATUS_INSIDE; break; }
        if (M.c1[fbest] < 0) { e.status = ORC_PROBE_STATUS_OUTSIDE; e.zone = M.fzone[fbest]; break; }
        if (e.moves == ORC_PROBE_WALK_LIMIT) { e.status = ORC_PROBE_STATUS_WALK_LIMIT; break; }
        P = M.c0[fbest] == P ? M.c1[fbest] : M.c0[fbest];
        ++e.moves;
    }
    return e;
}

}  // namespace orc
#endif
