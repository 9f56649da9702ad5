// linalg.hip — the iterative_solve driver: the Jacobi preconditioner's scaling and the switch over the arms (arms.hpp).
// Reference: src/linear_algebra.rs:144-299.
#include <algorithm>

#include "linalg.hpp"

namespace orc {

static int iterative_solve_body(const MatView &A_in, const double *b_in, double *x, uint64_t iteration_count, int method,
                                double relaxation_factor, double convergence_threshold, int preconditioner, Arena &arena,
                                SolveStats *stats) {
    const int64_t n = A_in.P.n;
    // extension: CG keeps the operator symmetric — no left scaling, M = D inside the recurrence; relaxation_factor and reduction_order
    // play no part (tree sums always)
    if (method == ORC_SOLVER_CG) return cg_dev(A_in, b_in, x, iteration_count, convergence_threshold, preconditioner, arena, stats);
    ArenaScope scope(arena);
    MatView A = A_in;
    const double *b = b_in;
    if (preconditioner == ORC_PRECOND_JACOBI) {  // :159-167
        double *dinv, *b_tmp;
        ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &dinv));
        ORC_TRY(arena.alloc((size_t)std::max<int64_t>(n, 1), &b_tmp));
        ORC_TRY(diag_inverse_dev(A_in, dinv));
        ORC_TRY(scale_vec_dev(dinv, b_in, b_tmp, n));
        if (!A.s1) A.s1 = dinv;
        else if (!A.s2) A.s2 = dinv;
        else return set_error(ORC_ERR_BAD_ARGUMENT, "more than two nested Jacobi scalings");
        b = b_tmp;
    } else if (preconditioner != ORC_PRECOND_NONE) {
        return set_error(ORC_ERR_BAD_ARGUMENT, "unknown preconditioner %d", preconditioner);
    }
    int st = ORC_OK;
    switch (method) {
    case ORC_SOLVER_JACOBI: {
        int jst = ORC_OK;
        st = jacobi_dev(A, b, x, iteration_count, relaxation_factor, convergence_threshold, arena, stats, &jst);
        if (st == ORC_OK) st = jst;
        break;
    }
    case ORC_SOLVER_BICGSTAB:
        st = bicgstab_dev(A, b, x, iteration_count, arena);
        break;
    case ORC_SOLVER_MULTIGRID:
        st = multigrid_arm_dev(A, b, x, iteration_count, relaxation_factor, convergence_threshold, preconditioner, arena, stats, ORC_SOLVER_BICGSTAB);
        break;
    case ORC_SOLVER_MULTIGRID_GS:
        st = multigrid_arm_dev(A, b, x, iteration_count, relaxation_factor, convergence_threshold, preconditioner, arena, stats, ORC_SOLVER_MULTICOLOR_GS);
        break;
    case ORC_SOLVER_MULTICOLOR_GS:
    case ORC_SOLVER_BICGSTAB_GS_PRECOND:
        st = gs_arm_dev(A, b, x, iteration_count, relaxation_factor, method, arena);
        break;
    case ORC_SOLVER_GMRES:  // extension: relaxation_factor and reduction_order play no part (tree sums always)
        st = gmres_dev(A, b, x, iteration_count, convergence_threshold, arena, stats);
        break;
    case ORC_SOLVER_GAUSS_SEIDEL:
        // The reference's arm scans every (i, j) through get(), which panics on the first
        // structural zero of a sparse matrix, and otherwise ends in
        // panic!("Gauss-Seidel out for maintenance :)") (linear_algebra.rs:219-246).
        st = ORC_ERR_GS_MAINTENANCE;
        break;
    default:
        st = ORC_ERR_UNSUPPORTED_SOLVER;  // :297
    }
    return st;
}

int iterative_solve_dev(const MatView &A_in, const double *b_in, double *x, uint64_t iteration_count, int method,
                        double relaxation_factor, double convergence_threshold, int preconditioner, Arena &arena,
                        SolveStats *stats) {
    int st = ensure_init();
    if (st == ORC_OK)
        st = iterative_solve_body(A_in, b_in, x, iteration_count, method, relaxation_factor, convergence_threshold, preconditioner, arena, stats);
    // partitioned operator: whatever happened locally (an early error return included), every rank takes part in the
    // status agreement and leaves with the same verdict — a rank that skipped it would strand its peers in RCCL
    if (A_in.halo) st = comm_global_status(st);
    return st;
}

}  // namespace orc
