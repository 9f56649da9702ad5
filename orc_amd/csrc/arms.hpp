// arms.hpp — every function that one translation unit of the solvers calls in another: the named products of spmv.hip, the arms of
// iterative_solve (linear_algebra.rs:144-299) and the test / bench hooks.  Included at the end of linalg.hpp; a declaration here is
// the only one outside the file that defines the function.
#pragma once
#include <vector>

namespace orc {

// verification mode: every dot product / norm of a solve in nalgebra's association (reduce.hip); rank-local operators only
inline bool reference_order(const MatView &A) { return ctx().reduction_order == ORC_REDUCTION_REFERENCE && A.halo == nullptr; }

// ---- reduce.hip
// Folds nq partial arrays of `count` entries each (fixed order => reproducible) into out[q].  One workgroup; launched after every
// kernel that produces partials.  global: followed by an RCCL all-reduce of out[0..nq) when the run has more than one rank.
int reduce_partials(const double *partials, int count, int nq, double *out, bool global = false);

// ---- spmv.hip: the products of the arms, named by their epilogue.  Arguments: (A, x, further inputs, outputs, partials, grid_out,
// skip_flags).  partials: kMaxPartials doubles per reduction; *grid_out: how many of them were written per reduction (what
// reduce_partials or a folding consumer is given as `count`); skip_flags (optional): two device doubles, non-zero = the launch is a no-op.
int spmv_grid(int32_t n_slices);  // the grid of a product over n_slices slices (also the Jacobi arm's sweeps and the scaling passes)
// y = A x
int product_store(const MatView &A, const double *x, double *y, const double *skip_flags);
// y = A x ; partial sum(y)                                   (nu = A p, r_hat_0 . nu : linear_algebra.rs:256-257)
int product_store_sum(const MatView &A, const double *x, double *y, double *partials, int *grid_out, const double *skip_flags);
// r = b - A x ; p = r (p optional) ; partial sum(r)           (linear_algebra.rs:250-254)
int product_residual(const MatView &A, const double *x, const double *b, double *r, double *p, double *partials, int *grid_out, const double *skip_flags);
// partial sum((b - A x)^2) ; r = b - A x (r optional)          (linear_algebra.rs:97, :202)
int product_residual_norm(const MatView &A, const double *x, const double *b, double *r, double *partials, int *grid_out, const double *skip_flags);
// t = A s ; partials t.s, t.t                                 (linear_algebra.rs:260-261)
int product_ts(const MatView &A, const double *s, double *t, double *partials, int *grid_out, const double *skip_flags);
// q = A p ; partial sum(p . q)                                (the CG arm)
int product_store_dot(const MatView &A, const double *p, double *q, double *partials, int *grid_out, const double *skip_flags);
// the same for three systems in lock-step (MatView3: interleaved vectors, 3 x the partial sums, system s at partials + s * grid)
int product_store_sum3(const MatView3 &A, const double *x3, double *y3, double *partials, int *grid_out);
int product_residual3(const MatView3 &A, const double *x3, const double *b3, double *r3, double *p3, double *partials, int *grid_out);
int product_ts3(const MatView3 &A, const double *s3, double *t3, double *partials, int *grid_out);

// ---- the arms of iterative_solve_dev (linalg.hip).  A carries the Jacobi preconditioner's scaling already (:159-167), except for CG.
// the Jacobi arm (jacobi.hip, :172-218); *status_out: the sticky OrcStatus of the sweeps
int jacobi_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor, double threshold, Arena &arena,
               SolveStats *stats, int *status_out);
// the BiCGSTAB arm (bicgstab.hip, :247-269)
int bicgstab_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, Arena &arena);
// the Multigrid arm (amg_cycle.hip, :270-296); smoother: ORC_SOLVER_BICGSTAB (the reference's) or ORC_SOLVER_MULTICOLOR_GS
int multigrid_arm_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor,
                      double convergence_threshold, int preconditioner, Arena &arena, SolveStats *stats, int smoother);
// extension: multicolour Gauss-Seidel and GS-preconditioned BiCGSTAB (gs_sweep.hip)
int gs_arm_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double relaxation_factor, int method, Arena &arena);
// extension: restarted GMRES (gmres.hip)
int gmres_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double convergence_threshold, Arena &arena,
              SolveStats *stats);
// extension: preconditioned CG (cg.hip)
int cg_dev(const MatView &A, const double *b, double *x, uint64_t iteration_count, double convergence_threshold, int preconditioner, Arena &arena,
           SolveStats *stats);
// the statistics of the newest orc_iterative_solve (api_linalg.cpp)
SolveStats &last_stats();

// ---- test and bench hooks behind the orc_debug_* / orc_bench_* entries of include/orc_amd.h
// product launches per kernel family (spmv.hip)
int debug_product_launches(long long *out, int n_out, bool reset);
// counters and single set-up steps of the hierarchy (amg_pairing.hip, amg_galerkin.hip, amg_mirror.hip, amg_hooks.hip)
void debug_amg_certification(long long out[2], bool reset);
void debug_amg_setup_stats(long long out[16], bool reset);
long long debug_shared_galerkin(bool reset);
int debug_xwin_counters(long long out[3], bool reset);
int amg_debug_coarsen(const MatView &A, Arena &arena, std::vector<int> &choice_h, std::vector<int64_t> &row_ptr_h,
                      std::vector<int64_t> &col_h, std::vector<double> &val_h, int *rounds, const double *x_h = nullptr, double *y_h = nullptr,
                      int scaled = 0, int *mirror_out = nullptr);
int amg_debug_packed(const MatView &A, Arena &arena, int64_t sizes[5], int32_t *row_len_h, int64_t *pk_ptr_h, int32_t *pk_col_h, double *pk_val_h,
                     int64_t *lptr_h, uint16_t *lidx_h, int32_t *wcol_h, int32_t *wsize_h);
int amg_debug_xwin_raw(const MatView &A, Arena &arena, int64_t info[10], int64_t *lptr_h, unsigned char *pos_raw_h, int32_t *wcol_raw_h, int32_t *wsize_h,
                       int32_t *wfmt_h);
// the colouring cache, the sweeps alone and the colouring of a pattern (gs_coloring.hip, gs_sweep.hip, gs_slot.hip)
void gs_forget_pattern(const void *col_ptr);
int bench_gs_sweep_dev(const MatView &A, const double *b, double *x, int reps, Arena &arena, float *ms_per_sweep, int *n_colors);
int bench_gs_sweep0_dev(const MatView A[3], const double *const b[3], int reps, Arena &arena, float ms[2], int *n_colors);
int gs_debug_coloring(const SellDev &P, std::vector<int> &colors, int *n_colors);

}  // namespace orc
