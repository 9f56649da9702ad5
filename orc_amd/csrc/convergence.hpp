// convergence.hpp — the stopping rule of a convergence-controlled run and the host half of a residual record: pure functions of
// recorded doubles.  Like schedule.hpp this header includes nothing of the runtime, so the rule can be checked where no device is
// (tests/test_residuals_cpu.py through orc_convergence_check).
#pragma once
#include "../../include/orc_types.h"

namespace orc {

inline bool convergence_valid(const OrcConvergence &c) {
    for (int k = 0; k < 3; ++k)
        if (!(c.momentum_tolerance[k] >= 0.)) return false;  // negative or NaN
    return c.continuity_tolerance >= 0. && c.reserved0 == 0;
}

// 1 when every scaled residual of the record is <= its tolerance and that tolerance is > 0; bit k of *failing_mask (may be null)
// names an equation that fails (u, v, w, continuity).  `r <= t` is false for a NaN r and for +inf: non-finite residuals never converge.
inline int convergence_check(const OrcConvergence &c, const double *record, int32_t *failing_mask) {
    int32_t mask = 0;
    for (int k = 0; k < 4; ++k) {
        const double tol = k < 3 ? c.momentum_tolerance[k] : c.continuity_tolerance;
        const double r = record[ORC_RESIDUAL_MOMENTUM_SCALED + k];
        if (!(tol > 0. && r <= tol)) mask |= 1 << k;
    }
    if (failing_mask) *failing_mask = mask;
    return mask == 0 ? 1 : 0;
}

// Slots 15..19 of a record from its raw slots 0..14: `seen` = monitored iterations before this one since monitoring was switched
// on, *scale = the continuity scale so far (updated while seen < 5).
inline void residual_record_finish(double *record, uint64_t seen, double *scale) {
    const double l1 = record[ORC_RESIDUAL_CONTINUITY_L1];
    if (seen < 5 && (seen == 0 || l1 > *scale)) *scale = l1;
    record[ORC_RESIDUAL_CONTINUITY_SCALE] = *scale;
    for (int k = 0; k < 3; ++k) {
        const double s = record[ORC_RESIDUAL_MOMENTUM_SCALE + k], r = record[ORC_RESIDUAL_MOMENTUM_L1 + k];
        record[ORC_RESIDUAL_MOMENTUM_SCALED + k] = s == 0. ? r : r / s;
    }
    record[ORC_RESIDUAL_CONTINUITY_SCALED] = *scale == 0. ? 0. : l1 / *scale;
}

}  // namespace orc
