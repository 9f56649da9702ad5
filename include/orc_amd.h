/* orc_amd.h — C ABI of liborc_amd.so: ORC's per-SIMPLE-iteration hot path on MI355X (gfx950).
 *
 * ORC (reidprichard/ORC v0.3.0) has no plugin/FFI layer; the drop-in boundary is its ordinary
 * `pub fn` surface.  Each entry point below replaces one of those functions and
 * cites it (file:line into the reference).  A Rust `extern "C"` shim that keeps ORC's own
 * signatures on top of this header is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; every array is caller-owned host memory unless the name
 *    says `_dev`; the library copies in/out and keeps its own device allocations.
 *  - fields and matrices are in ORC cell order; indices are 0-based int64 (`usize`).
 *  - return value: OrcStatus (include/orc_types.h). ORC panics where we return non-zero; the
 *    shim turns non-zero into panic!(orc_status_string(code)).
 *  - there is NO CPU fallback: without a HIP device every compute entry returns ORC_ERR_NO_DEVICE.
 *  - CSR matrices use ORC's pattern: per cell the diagonal plus one entry per interior face,
 *    columns ascending (what CsrMatrix::from(&CooMatrix) yields at discretization.rs:130,445,471).
 */
#ifndef ORC_AMD_H
#define ORC_AMD_H

#include <stdint.h>
#include "orc_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OrcMesh OrcMesh;     /* device-resident SoA image of mesh::Mesh (mesh.rs:181-187) */
typedef struct OrcSolver OrcSolver; /* device-resident state of one solve_steady call (solver.rs:39-49) */

/* ---------- runtime ---------- */
int orc_init(int device_ordinal);              /* hipSetDevice + stream; idempotent */
int orc_device_count(void);                    /* 0 when no HIP device is visible */
int orc_synchronize(void);                     /* hipStreamSynchronize on the library stream */
const char *orc_status_string(int status);     /* the reference's panic text for the code */
const char *orc_last_error(void);              /* detail of the last ORC_ERR_HIP / BAD_ARGUMENT */
/* The library reads its environment switches (ORC_*: INTEGRATION.md lists them; none changes a result) ONCE, in the first orc_init; a caller
 * that changes one afterwards — the tests do — says so here.  Never called by the library itself. */
int orc_reload_environment(void);
int orc_device_memory(int64_t *free_bytes, int64_t *total_bytes); /* hipMemGetInfo of the library's device */
/* "<device name> | pci <domain:bus:device.function> | ordinal <n> | <CUs> CUs" of the library's device: a multi-GPU run reports it per rank,
 * so that "did N ranks run on N different cards" is answered by the result itself.  Returns ORC_ERR_BAD_ARGUMENT when cap is too small. */
int orc_device_info(char *buf, int cap);
void orc_settings_default(OrcSettings *s);     /* NumericalSettings::default() + MatrixSolverSettings::default(), lib.rs:58-86 */

/* ---------- mesh::Mesh (mesh.rs:140-187) ---------- */
/* face_c0/face_c1: Face.cell_indices[0], [1] (-1 when the face has one cell, io.rs:332-337);
 * face_normal: unit normal outward from face_c0 (mesh.rs:216-222); face_zone: index into the
 * zone arrays; zone_type: OrcFaceConditionType per zone (FaceZone.zone_type, mesh.rs:12-17);
 * cell_faces: Cell.face_indices, ascending face id (io.rs:404-410). */
OrcMesh *orc_mesh_create(int64_t n_cells, int64_t n_faces, int32_t n_zones,
                         const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone,
                         const double *face_area, const double *face_normal /*[3F]*/, const double *face_centroid /*[3F]*/,
                         const double *cell_centroid /*[3n]*/, const double *cell_volume,
                         const int64_t *cell_face_ptr /*[n+1]*/, const int64_t *cell_faces,
                         const int32_t *zone_type, const double *zone_scalar, const double *zone_vector /*[3Z]*/,
                         int *status);
/* The same mesh with its cells renumbered internally by `ordering` (OrcCellOrdering; ORC_ORDER_RCM = the north star's
 * "rows sorted by RCM"): for meshes whose generator numbered the cells arbitrarily.  Callers keep speaking ORC order:
 *   ORC order       every per-cell array of orc_solver_set_fields / get_fields, orc_solve_steady / _steady_converged / _transient,
 *                   orc_solver_set_time_levels, orc_initialize_*, the scalar arm's field, source, levels and
 *                   diffusivity (field and orc_solver_get_scalar_diffusivity), the viscosity arm's field, orc_solver_get_viscosity / evaluate_viscosity, orc_mesh_wall_distance, orc_derived_fields /
 *                   orc_solver_derived_fields, the fields into orc_surface_integrals / orc_boundary_fields, the time statistics
 *                   (get and set_statistics_state), the cell ids of orc_probes_get / orc_tracers_get, and everything per cell of
 *                   the volume reports (the labels and cell ids of a cell group set, the fields into orc_group_integrals, `where`)
 *   internal order  matrices, patterns and the per-cell arrays of the assembly entry points (orc_mesh_matrix_pattern,
 *                   orc_solver_assemble_momentum / _pressure / _scalar, orc_solver_get_diffusion, orc_solver_get_pressure_rhs,
 *                   orc_build_momentum_diffusion_matrix, orc_initialize_momentum_matrix)
 *   mixed           fields in in ORC order, results out in internal order: orc_calculate_gradients,
 *                   orc_build_momentum_advection_matrices, orc_build_pressure_correction_matrices
 * orc_mesh_cell_order reports the internal order (global_ids[c] = ORC index of internal cell c).  A renumbered run is the reference's algorithm on a renumbered mesh: its
 * iterates differ from the ORC-order run wherever the reference depends on the numbering (pairwise aggregation by row
 * index), its converged fields do not. */
OrcMesh *orc_mesh_create_reordered(int64_t n_cells, int64_t n_faces, int32_t n_zones,
                                   const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone,
                                   const double *face_area, const double *face_normal, const double *face_centroid,
                                   const double *cell_centroid, const double *cell_volume,
                                   const int64_t *cell_face_ptr, const int64_t *cell_faces,
                                   const int32_t *zone_type, const double *zone_scalar, const double *zone_vector,
                                   int32_t ordering, int *status);
int orc_mesh_cell_order(const OrcMesh *m, int64_t *global_ids /*[n]*/);
/* One rank's part of a cell-partitioned mesh: local cells are numbered owned first [0, n_owned), then one
 * contiguous block of ghost cells per peer (recv_ptr, in peer order); cell_face_ptr gives ghost cells empty face lists;
 * faces are those touching an owned cell, in ascending global id with the global c0/c1 orientation.
 * send_idx[send_ptr[q] .. send_ptr[q+1]) are the owned cells whose values peer q needs, in the order of q's ghost block.
 * Requires orc_comm_init (RCCL) or orc_comm_set_host_transport first when n_peers > 0. */
OrcMesh *orc_mesh_create_partitioned(int64_t n_owned, int64_t n_cells, int64_t n_cells_global, int64_t n_faces, int32_t n_zones,
                                     const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone, const double *face_area,
                                     const double *face_normal, const double *face_centroid, const double *cell_centroid,
                                     const double *cell_volume, const int64_t *cell_face_ptr, const int64_t *cell_faces,
                                     const int32_t *zone_type, const double *zone_scalar, const double *zone_vector, int32_t n_peers,
                                     const int32_t *peers, const int64_t *send_ptr, const int64_t *send_idx, const int64_t *recv_ptr,
                                     int *status);
int64_t orc_mesh_n_owned(const OrcMesh *m);
/* Cell partitioning of any mesh (host only, no device needed): the cells are put in `ordering` (OrcCellOrdering) and cut
 * into n_ranks contiguous blocks; the result holds rank `rank`'s arrays exactly as orc_mesh_create_partitioned takes them
 * (owned cells in block order, ghost blocks per peer sorted by position in the order, faces touching an owned cell in
 * ascending global id).  Every rank calls it on the same global arrays (those of orc_mesh_create / orc_mesh_data_arrays);
 * my send list to a peer and that peer's ghost block of my cells coincide by construction.  global_ids[n_local] maps a
 * local cell to its ORC index: fields are scattered / gathered through it, so the permutation stays internal.
 * n_ranks = 1 gives the whole mesh renumbered (e.g. RCM row ordering on one GPU). */
typedef struct OrcPartition OrcPartition;
OrcPartition *orc_mesh_partition(int64_t n_cells, int64_t n_faces, const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone,
                                 const double *face_area, const double *face_normal, const double *face_centroid,
                                 const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr,
                                 const int64_t *cell_faces, int32_t n_ranks, int32_t rank, int32_t ordering, int *status);
/* [r04] The same for a mesh a rank generated or read FOR ITSELF (its share of the cells plus ghost layers): the caller names the
 * owner of every cell (cell_owner[n_cells]: a rank, or -1 = nobody's — e.g. the outer of two generated ghost layers; such a cell
 * may not touch a cell of `rank`), the cells keep their order, n_global is the cell count of the whole mesh (< 0: n_cells).
 * No process ever holds the whole mesh: BASELINE configs[4] (40 M mixed cells on 8 GPUs) generates 1/8 + two block layers per
 * side on every rank.  The two ranks of a cut must number the cells they share in the same relative order (generators that
 * number layer by layer do; tests/test_partition_cpu.py exchanges global ids over gloo to check it).  global_ids are indices
 * into the caller's own arrays. */
OrcPartition *orc_mesh_partition_owner(int64_t n_cells, int64_t n_faces, const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone,
                                       const double *face_area, const double *face_normal, const double *face_centroid,
                                       const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr,
                                       const int64_t *cell_faces, const int32_t *cell_owner, int32_t n_ranks, int32_t rank, int64_t n_global,
                                       int *status);
void orc_partition_destroy(OrcPartition *p);
int orc_partition_sizes(const OrcPartition *p, int64_t *n_owned, int64_t *n_local, int64_t *n_global, int64_t *n_faces, int64_t *n_cell_faces,
                        int32_t *n_peers, int64_t *n_send);
/* any pointer may be NULL; sizes from orc_partition_sizes (send_ptr / recv_ptr: n_peers + 1) */
int orc_partition_arrays(const OrcPartition *p, int64_t *face_c0, int64_t *face_c1, int32_t *face_zone, double *face_area, double *face_normal,
                         double *face_centroid, double *cell_centroid, double *cell_volume, int64_t *cell_face_ptr, int64_t *cell_faces,
                         int64_t *global_ids, int64_t *global_face_ids, int32_t *peers, int64_t *send_ptr, int64_t *send_idx, int64_t *recv_ptr);
/* = orc_mesh_create_partitioned on the partition's arrays and the (global) zone tables */
OrcMesh *orc_partition_upload(const OrcPartition *p, int32_t n_zones, const int32_t *zone_type, const double *zone_scalar,
                              const double *zone_vector, int *status);
/* mesh.get_face_zone(name).zone_type / scalar_value / vector_value = ... (tests.rs:60-76) */
int orc_mesh_update_zones(OrcMesh *m, const int32_t *zone_type, const double *zone_scalar, const double *zone_vector);
void orc_mesh_destroy(OrcMesh *m);
int64_t orc_mesh_n_cells(const OrcMesh *m);
int64_t orc_mesh_nnz(const OrcMesh *m);
/* CSR pattern shared by a_di, a_u, a_v, a_w and the pressure-correction matrix */
int orc_mesh_matrix_pattern(const OrcMesh *m, int64_t *row_ptr /*[n+1]*/, int64_t *col_idx /*[nnz]*/);

/* ---------- io::read_mesh (io.rs:32-515) and Mesh::get_face_zone (mesh.rs:189-195): host only, no device needed ----------
 * TGRID / Fluent ASCII .msh -> flat host image of mesh::Mesh with the reference's numbering and geometry rules
 * (normal (n2-n1)x(n1-n0) normalised, flipped when cell 0 is absent; face centroid = node mean; area = triangle fan
 * about the centroid; cell centroid = mean of face centroids; volume = sum A |(fc-cc).n| / dim; Cell.face_indices in
 * ascending face id).  Reader quirks are kept: section items are read as hexadecimal (io.rs:47-54), zone-0 declaration
 * sections are skipped (io.rs:24-30), a zone takes the last word of the preceding "(0 ...)" comment as its name
 * (io.rs:83-90), the node count of a face line is "tokens - 2" also for mixed/polygonal zones (io.rs:232).
 * Every expect()/panic! of the reference is ORC_ERR_MESH_FORMAT (ORC_ERR_IO when the file cannot be opened). */
typedef struct OrcMeshData OrcMeshData;
OrcMeshData *orc_read_mesh(const char *mesh_path, int *status);
void orc_mesh_data_destroy(OrcMeshData *d);
int orc_mesh_data_sizes(const OrcMeshData *d, int32_t *dimensions, int64_t *n_vertices, int64_t *n_cells, int64_t *n_faces,
                        int64_t *n_cell_faces, int64_t *n_face_nodes, int32_t *n_zones);
/* the argument arrays of orc_mesh_create; any pointer may be NULL */
int orc_mesh_data_arrays(const OrcMeshData *d, int64_t *face_c0, int64_t *face_c1, int32_t *face_zone, double *face_area,
                         double *face_normal, double *face_centroid, double *cell_centroid, double *cell_volume,
                         int64_t *cell_face_ptr, int64_t *cell_faces);
/* Mesh.vertices and Face.node_indices (0-based) */
int orc_mesh_data_nodes(const OrcMeshData *d, double *vertices /*[3V]*/, int64_t *face_node_ptr /*[F+1]*/, int64_t *face_nodes);
/* FaceZone k (order of first appearance in the file): TGRID zone id, type, values, name */
int orc_mesh_data_zone(const OrcMeshData *d, int32_t k, uint64_t *zone_id, int32_t *zone_type, double *scalar_value,
                       double *vector_value /*[3]*/, char *name, int64_t name_len);
int orc_mesh_data_zone_index(const OrcMeshData *d, const char *name); /* -1 when absent */
/* `let z = mesh.get_face_zone(name); z.zone_type = ..; z.scalar_value = ..; z.vector_value = ..` (tests.rs:60-76);
 * ORC_ERR_ZONE_NOT_FOUND where the reference panics */
int orc_mesh_data_set_zone(OrcMeshData *d, const char *name, int32_t zone_type, double scalar_value, const double *vector_value /*[3] or NULL*/);
OrcMesh *orc_mesh_upload(const OrcMeshData *d, int *status);    /* = orc_mesh_create on the arrays above */
int orc_mesh_sync_zones(OrcMesh *m, const OrcMeshData *d);      /* = orc_mesh_update_zones from d's zone table */

/* ---------- io::read_data / write_data / write_data_with_precision / write_gradients (io.rs:519-662) ----------
 * One line per cell: "{centroid}\t({u}, {v}, {w})\t{p}", centroid as Vector's Display "({:.2e}, {:.2e}, {:.2e})"
 * (lib.rs:551-555), values in Rust LowerExp form (no '+', no exponent padding): shortest round-trip digits when
 * decimal_precision < 0 (write_data's "{:.e}"), else that many fraction digits (write_data_with_precision). */
int orc_write_data(const char *output_file_name, int64_t n_cells, const double *cell_centroid /*[3n]*/, const double *u,
                   const double *v, const double *w, const double *p, int decimal_precision);
/* Fills at most `capacity` rows, returns the row count of the file in n_read (capacity 0: count only).
 * ORC_ERR_IO = the reference's Err("could not read data file"). */
int orc_read_data(const char *data_file_path, int64_t capacity, double *u, double *v, double *w, double *p, int64_t *n_read);
/* "{centroid}\t({9 velocity-gradient entries, row-major, each followed by ', '})\t({3 pressure-gradient entries, same})":
 * the trailing ", " inside the parentheses is the reference's (its strip_suffix result is dropped, io.rs:644,654).
 * Gradients come from the device Green-Gauss kernels (orc_calculate_gradients). */
int orc_write_gradients(const OrcMesh *m, const double *cell_centroid, const double *u, const double *v, const double *w,
                        const double *p, const char *output_file_name, int decimal_precision, const OrcSettings *settings);

/* ---------- linear_algebra::iterative_solve (linear_algebra.rs:144-153) ---------- */
int orc_iterative_solve(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values,
                        const double *b, double *solution_vector /*in/out*/, uint64_t iteration_count,
                        int method /*OrcSolutionMethod*/, double relaxation_factor, double convergence_threshold,
                        int preconditioner /*OrcPreconditionMethod*/);
/* The same for THREE systems that share one sparsity pattern — what solver::solve_steady's three momentum solves are
 * (solver.rs:99-136: a_u, a_v, a_w come from one initialize_momentum_matrix pattern, discretization.rs:450-472).  One
 * column stream and one 24-byte gather per entry serve the three value streams; the fixed iteration count of the BiCGSTAB
 * arm (linear_algebra.rs:255) keeps the systems in lock-step.  method: ORC_SOLVER_BICGSTAB or ORC_SOLVER_MULTIGRID (tree
 * reductions, single GPU).  Each system's result is bit-identical to orc_iterative_solve on that system alone;
 * status_out[k] is system k's verdict (e.g. ORC_ERR_MULTIGRID_DIVERGED), the return value the call's own. */
int orc_iterative_solve3(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *const values[3],
                         const double *const b[3], double *const solution_vectors[3] /*in/out*/, uint64_t iteration_count,
                         int method, double relaxation_factor, double convergence_threshold, int preconditioner,
                         int status_out[3]);
/* Process-wide default of OrcSettings.breakdown_guard for orc_iterative_solve (whose signature has no
 * settings argument, like the reference's).  1 (default) = guard on; 0 = NaN like the reference. */
int orc_set_breakdown_guard(int on);
/* Number of BiCGSTAB solves (process-wide, since the last call with reset != 0) in which the breakdown guard fired, i.e.
 * in which the reference (linear_algebra.rs:255-268, no test at all) would have divided 0/0 and returned NaN — a caller
 * that replaces solver::solve_steady (solver.rs:217-221 "solution diverged") can tell that the guard kept it alive.
 * orc_solve_steady / orc_solver_iterate also leave "breakdown guard fired in N solve(s)" in orc_last_error() when they
 * return ORC_OK after such an iteration. */
int64_t orc_breakdown_guard_events(int reset);
/* Process-wide default of OrcSettings.reduction_order for orc_iterative_solve (OrcReductionOrder). */
int orc_set_reduction_order(int order);
/* sweeps the Jacobi arm executed in the last orc_iterative_solve (linear_algebra.rs:188-217) */
int64_t orc_last_jacobi_sweeps(void);
/* ORC_SOLVER_GMRES (extension, no reference counterpart; ORC's own TODO at lib.rs:170): restarted GMRES(m).
 *  - preconditioner: ORC_PRECOND_JACOBI is the left scaling p_inv * a, p_inv * b of every arm (linear_algebra.rs:159-167);
 *    every residual below is one of that system.  relaxation_factor is ignored, and so is reduction_order: there is no
 *    reference arithmetic to match, the sums are always per-workgroup trees folded in a fixed order.
 *  - iteration_count = Arnoldi steps (products with A) over all restarts; m = min(restart, iteration_count);
 *    iteration_count == 0 or n == 0 leaves x unchanged.
 *  - a cycle: r = b - A x, beta = |r| (beta0: of the first cycle), v0 = r / beta, g = (beta, 0, ...); step j: w = A v_j,
 *    classical Gram-Schmidt twice (h1 = V^T w; w -= V h1; h2 = V^T w; w -= V h2; h = h1 + h2), h_{j+1,j} = |w|,
 *    v_{j+1} = w / h_{j+1,j}; the earlier Givens rotations on column j, the new one from hypot, g updated; at the end of
 *    the cycle R y = g by back substitution and x += V y.
 *  - the cycle and the solve end early when |g_{j+1}| <= convergence_threshold * beta0 (never with a threshold <= 0), on a
 *    happy breakdown h_{j+1,j} <= 1e-14 * |h_{:,j}| (x takes the update with that column), or when the steps are spent.
 *    A new cycle whose beta is 0 stops without touching x.
 *  - a non-finite beta0 or Hessenberg entry: with breakdown_guard on, x keeps the value of the last completed cycle, the
 *    solve stops and orc_breakdown_guard_events counts one event; with it off the update is applied and NaN propagates.
 *  - bit-reproducible from run to run on one device (no float atomics); no host synchronisation inside the solve.
 * Process-wide default of OrcSettings.gmres_restart for orc_iterative_solve: 0 = 30, 1..64; anything else makes the GMRES
 * arm return ORC_ERR_BAD_ARGUMENT. */
int orc_set_gmres_restart(int m);
/* the last orc_iterative_solve's GMRES arm: Arnoldi steps, cycles, beta0 and the final residual estimate |g| */
int orc_last_gmres_stats(int64_t *steps, int64_t *cycles, double *initial_residual, double *final_estimate);
/* ORC_SOLVER_CG (extension, no reference counterpart): preconditioned conjugate gradients for a symmetric positive definite
 * system — what build_pressure_correction_matrices (discretization.rs:359-448) and a pure-conduction scalar system are.
 *  - CG does NOT test the symmetry of the values: on a non-symmetric or indefinite matrix it runs until p.q <= 0 (event 1)
 *    or until the iterations are spent, and what it returns is then no Krylov minimiser of anything.
 *  - preconditioner: the other arms apply ORC_PRECOND_JACOBI as the left scaling p_inv * a, which destroys symmetry.  This
 *    arm keeps the operator unscaled and applies M = D inside the recurrence: z = D^-1 r (JACOBI) or z = r (NONE).  A view
 *    that arrives already scaled (CG nested inside another arm) is ORC_ERR_BAD_ARGUMENT; a diagonal entry that is missing,
 *    zero or non-finite under JACOBI is ORC_ERR_STRUCTURAL_ZERO.  relaxation_factor and reduction_order play no part: the
 *    sums are per-workgroup trees folded in a fixed order, as for GMRES.
 *  - start: r = b - A x, z = M^-1 r, p = z, rho = r.z, beta0 = |r|.  Iteration k: q = A p; alpha = rho / p.q; x += alpha p;
 *    r -= alpha q; z = M^-1 r; rho' = r.z; p = z + (rho' / rho) p.
 *  - stops, all decided on the device: beta0 == 0 (no iteration, x untouched); after the update of an iteration, which
 *    counts, |r| <= convergence_threshold * beta0 (never with a threshold <= 0); iteration_count reached; and the events.
 *    Event 1: p.q <= 0.  Event 2: rho or p.q is non-finite, or alpha overflows.  Both are tested before the update, so x keeps the last
 *    completed iterate and that iteration does not count.  Event 2 is also raised right after an update whose r.z or r.r
 *    came out non-finite (that iteration counts).  An event is recorded in orc_last_cg_stats and the status stays ORC_OK.
 *  - iteration_count == 0 or n == 0 leaves x unchanged.  At most three launches per iteration (product with the p.q partial
 *    sums, cg_update_k, cg_direction_k), no float atomics (two solves of one system give identical bits), one host
 *    synchronisation at the end of the solve.
 * orc_last_cg_stats: completed iterations, beta0, the final recurrence residual |r| and the event of the last CG solve of
 * this process (orc_iterative_solve, or a solver's system solved with ORC_SOLVER_CG).  Any pointer may be NULL. */
int orc_last_cg_stats(int64_t *iterations, double *initial_residual, double *final_residual, int32_t *event);
/* y = A x: the `&CsrMatrix * &DVector` product the reference takes from nalgebra-sparse
 * (linear_algebra.rs:256,260); row sums accumulate in ascending-column order from 0.0, so y is
 * bit-identical to the CPU product.  `reps` > 1 repeats the launch (timing); avg_ms may be NULL. */
int orc_csr_spmv(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values, const double *x,
                 double *y, int reps, double *avg_ms);

/* Test hooks for the two private functions under the Multigrid arm (linear_algebra.rs:12-63, :80-84):
 * partner[i] = strongest_unmerged_neighbor of row i (-1 = none) of build_restriction_matrix(Strongest), and
 * a' = (R a) R^T as CSR.  Call with out_col == NULL to get the sizes (out_n_coarse, out_nnz). */
int orc_amg_coarsen(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values, int64_t *partner /*[n]*/,
                    int64_t *out_n_coarse, int64_t *out_nnz, int64_t *out_row_ptr, int64_t *out_col, double *out_val,
                    int *rounds);

/* Test hook for the multicolour Gauss-Seidel extension: the distance-1 colouring (Jones-Plassmann, first fit) the device
 * uses for a pattern; rows of one colour share no entry. */
int orc_debug_coloring(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, int32_t *colors /*[n]*/, int32_t *n_colors);

/* ---------- discretization::* ---------- */
/* build_momentum_diffusion_matrix (discretization.rs:39-48): values in pattern order + 3 RHS */
int orc_build_momentum_diffusion_matrix(const OrcMesh *m, int diffusion_scheme, double mu,
                                        double *a_values /*[nnz]*/, double *b_u, double *b_v, double *b_w);
/* initialize_momentum_matrix (discretization.rs:450) */
int orc_initialize_momentum_matrix(const OrcMesh *m, double *a_values /*[nnz]*/);
/* build_momentum_advection_matrices (discretization.rs:134-152).  a_u/a_v/a_w values are in/out:
 * their diagonals on entry are what Rhie-Chow reads (frozen-diagonal semantics).
 * peclet: (avg, min, max) as returned by the reference (:355). */
int orc_build_momentum_advection_matrices(const OrcMesh *m, double *a_u_values, double *a_v_values, double *a_w_values,
                                          double *b_u, double *b_v, double *b_w, const double *a_di_values,
                                          const double *u, const double *v, const double *w, const double *p,
                                          const OrcSettings *settings, double rho, double peclet[3]);
/* build_pressure_correction_matrices (discretization.rs:359-370) -> LinearSystem{a,b} */
int orc_build_pressure_correction_matrices(const OrcMesh *m, const double *u, const double *v, const double *w,
                                           const double *p, const double *a_u_values, const double *a_v_values,
                                           const double *a_w_values, const OrcSettings *settings, double rho,
                                           double *a_values /*[nnz]*/, double *b /*[n]*/);

/* ---------- solver::* ---------- */
/* calculate_pressure_gradient / calculate_velocity_gradient (solver.rs:774-950) evaluated for every cell with
 * settings->gradient_reconstruction — GreenGauss(CellBased) or LeastSquares: grad_p[3n], grad_u[9n] (row = velocity
 * component).  ORC_ERR_SINGULAR_MATRIX where the reference's try_inverse().unwrap() panics. */
int orc_calculate_gradients(const OrcMesh *m, const double *u, const double *v, const double *w, const double *p,
                            const OrcSettings *settings, double *grad_p, double *grad_u);
/* check_boundary_conditions (solver.rs:710-772): constraint_type 0 PressureOnly, 1 VelocityOnly, 2 Hybrid;
 * ORC_ERR_NO_BOUNDARY_CONDITIONS for its "You must set boundary conditions." panic */
int orc_check_boundary_conditions(const OrcMesh *m, int *constraint_type);
/* initialize_pressure_field (solver.rs:414-509): Laplace system on the mesh pattern, 10 Jacobi sweeps; p in/out */
int orc_initialize_pressure_field(const OrcMesh *m, double *p /*[n]*/);
/* initialize_flow (solver.rs:246-352): pressure initialisation, UD / LinearWeighted momentum assembly at zero velocity,
 * then the six-step diffusion -> advection ramp of Jacobi-preconditioned BiCGSTAB solves (iteration_count each).
 * settings may be NULL; only q1_compat and breakdown_guard are read from it.  Outputs u, v, w, p [n]. */
int orc_initialize_flow(const OrcMesh *m, double mu, double rho, uint64_t iteration_count, const OrcSettings *settings,
                        double *u, double *v, double *w, double *p);
/* initialize_velocity_field (solver.rs:511-696): potential-flow system for psi (velocity inlets as sources, a pressure
 * outlet as psi = 0), ten Jacobi-preconditioned BiCGSTAB iterations, then u, v, w = least-squares gradient of psi over
 * the interior neighbours with all-zero columns dropped.  settings may be NULL (q1_compat, breakdown_guard and
 * reduction_order are read).  psi [n] is optional: the field the reference writes to ./examples/psi.csv. */
int orc_initialize_velocity_field(const OrcMesh *m, const OrcSettings *settings, double *u, double *v, double *w, double *psi);
/* initialize_flow_new (solver.rs:354-410): PressureOnly | Hybrid -> initialize_pressure_field, VelocityOnly ->
 * initialize_velocity_field */
int orc_initialize_flow_new(const OrcMesh *m, double mu, double rho, uint64_t iteration_count,
                            double *u, double *v, double *w, double *p);
/* solve_steady (solver.rs:26-37). report_cb is called every reporting_interval iterations with
 * what the reference prints (solver.rs:209-216): iteration, mean u/v/w, Peclet avg/min/max,
 * velocity- and pressure-correction norms, ms/iter.  May be NULL. */
typedef void (*OrcReportFn)(uint64_t iteration, const double mean_velocity[3], const double peclet[3],
                            double velocity_correction, double pressure_correction, double ms_per_iter, void *user);
int orc_solve_steady(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings,
                     double rho, double mu, uint64_t iteration_count, uint64_t reporting_interval,
                     OrcReportFn report_cb, void *user);

/* ---------- device-resident solver (what orc_solve_steady is made of) ---------- */
OrcSolver *orc_solver_create(OrcMesh *m, const OrcSettings *settings, double rho, double mu, int *status); /* solver.rs:39-49 */
void orc_solver_destroy(OrcSolver *s);
int orc_solver_set_fields(OrcSolver *s, const double *u, const double *v, const double *w, const double *p);
int orc_solver_get_fields(OrcSolver *s, double *u, double *v, double *w, double *p);
/* runs `iterations` SIMPLE iterations (solver.rs:60-222); report, if not NULL, receives 8 doubles per
 * iteration: u_avg, v_avg, w_avg, peclet_avg, peclet_min, peclet_max, vel_corr, p_corr */
int orc_solver_iterate(OrcSolver *s, uint64_t iterations, double *report);
/* Device-side copy of the state a SIMPLE iteration starts from (u, v, w, p and the momentum diagonals that Rhie-Chow
 * reads, solver.rs:1068-1081) and its restoration (asynchronous device-to-device copies on the library stream):
 * bench.py times the same iteration repeatedly, so that every step does identical work. */
int orc_solver_snapshot(OrcSolver *s);
int orc_solver_restore(OrcSolver *s);
/* A linear solver of its own for the pressure correction (new-build extension, orc_types.h OrcLinearSolver).  The p' matrix is
 * symmetric positive definite (discretization.rs:401-438: a_PN is symmetric in P and N), the momentum matrices are not, and
 * the reference solves all four with one MatrixSolverSettings (solver.rs:99-179).
 *  - orc_solver_set_pressure_solver(s, c): c == NULL removes the override.  Otherwise c is validated (a solver type of
 *    OrcSolutionMethod that iterative_solve knows, a known preconditioner, iterations >= 1, threshold >= 0 and not NaN, a
 *    finite relaxation: ORC_ERR_BAD_ARGUMENT otherwise, solver unchanged) and from then on every p' solve
 *    (orc_solver_iterate, orc_solver_advance) runs with these five fields in
 *    place of the settings'.  The momentum solves and their schedule keep following OrcSettings.solver_type.
 *  - the p' Multigrid hierarchy is set up ahead of the solve only when the method that will solve p' is a Multigrid arm.
 *  - a solver that never sets the override launches exactly what it launched before; an override equal to the settings'
 *    own fields changes no bit.  On a partitioned mesh every rank must set the same override.
 *  - orc_solver_snapshot / orc_solver_restore do not touch it.
 * orc_solver_get_pressure_solver: *enabled = 1 and the override, or 0 and the five fields of the settings.
 * orc_solver_debug_pressure_hierarchies (test hook): p' Multigrid hierarchies this solver has set up so far, ahead of a solve or
 * inside one. */
int orc_solver_set_pressure_solver(OrcSolver *s, const OrcLinearSolver *c);
int orc_solver_get_pressure_solver(OrcSolver *s, OrcLinearSolver *c, int32_t *enabled);
long long orc_solver_debug_pressure_hierarchies(OrcSolver *s);
/* individual phases, for the parity tests: matrices come back in pattern order */
int orc_solver_assemble_momentum(OrcSolver *s, double *a_u, double *a_v, double *a_w, double *b_u, double *b_v, double *b_w, double peclet[3]);
int orc_solver_assemble_pressure(OrcSolver *s, double *a_p, double *b_p);

/* ---------- implicit time stepping (new-build extension, orc_types.h OrcTransient) ----------
 * Off by default: a solver that never calls orc_solver_set_transient runs exactly the steady code paths.
 *  - orc_solver_set_transient(s, t): t == NULL switches back to steady SIMPLE; otherwise validates t and turns the arm on
 *    with 0 known time levels.  Invalid (dt <= 0 or non-finite, unknown scheme, inner_iterations == 0, negative or NaN
 *    inner_tolerance, reserved0 != 0, or a solver with frozen_diagonals = 0) is ORC_ERR_BAD_ARGUMENT, solver unchanged.
 *  - while the arm is on and at least one level is known, every momentum assembly (orc_solver_iterate,
 *    orc_solver_assemble_momentum and the pressure system through the diagonals) carries the time term; BDF2 runs as Euler
 *    while only one level is known.  orc_solver_iterate does not shift the levels.
 *  - orc_solver_set_time_levels: levels n (and n-1, or NULL for one known level) in ORC cell order; needs the arm on.
 *  - orc_solver_advance: per time step, n-1 <- n, n <- current fields (known levels min(k + 1, 2)), then up to
 *    inner_iterations SIMPLE iterations, fewer once both correction norms (report slots 6, 7) are below inner_tolerance times
 *    their values at the first inner iteration.  report (may be NULL): 10 doubles per step, the 8 of orc_solver_iterate for
 *    the last inner iteration, the inner iterations used, and the time reached since the arm was enabled.
 *  - orc_solver_snapshot / orc_solver_restore include the time levels, their count and the time while the arm is on.
 *  - the step is OrcTransient.dt throughout unless an entry of "adaptive time stepping" below changes it. */
int orc_solver_set_transient(OrcSolver *s, const OrcTransient *t);
int orc_solver_set_time_levels(OrcSolver *s, const double *u_n, const double *v_n, const double *w_n, const double *u_nm1,
                               const double *v_nm1, const double *w_nm1);
int orc_solver_advance(OrcSolver *s, uint64_t time_steps, double *report);
/* solve_steady's counterpart: time_steps steps of t from u, v, w, p (updated in place); report_cb every reporting_interval
 * steps with the last inner iteration's report (iteration = time step, ms_per_iter = ms per time step) */
int orc_solve_transient(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings, double rho, double mu,
                        const OrcTransient *t, uint64_t time_steps, uint64_t reporting_interval, OrcReportFn report_cb, void *user);

/* ---------- adaptive time stepping (new-build extension, orc_types.h OrcTimeStepControl) ----------
 * Off by default: a solver that calls none of these entries launches what it launched before and produces the same bits.
 * The time state of the arm: `time` reached, dt_next (the step orc_solver_advance takes next; OrcTransient.dt at first), dt_last (the
 * step that led from level n-1 to level n) and dt_before_last.  The time terms of the momentum systems and of the scalar read
 * w = dt_next / dt_last (OrcTimeStepControl above); the statistics weight, the tracer substep, the scalar time term, the time reached
 * and the history tags follow the step actually taken.
 *  - orc_solver_courant: rate_max = the largest ORC_DERIVED_CONVECTIVE_RATE of the solver's current u, v, w over the owned cells (its
 *    bits), *cell = the smallest ORC id among the cells that attain it, rate (may be NULL) = the per-cell values in ORC order, from the
 *    same launch.  A NaN rate anywhere makes rate_max NaN.  On a partitioned mesh rate_max is the maximum over all ranks (the same
 *    bits on every rank) and *cell is -1.  Reads the fields, writes none; two calls on one state give the same bits.
 *  - orc_time_step_next: the law of OrcTimeStepControl on the host, no device needed.  An invalid control, a dt that is not positive
 *    and finite, or a NaN, negative or infinite rate_max is ORC_ERR_BAD_ARGUMENT with *dt_next untouched.
 *  - orc_solver_set_time_step: dt_next; levels, time and history are kept.  From now on every step appends a history row.
 *  - orc_solver_set_time_step_control: c == NULL turns control off.  Otherwise, after every interval-th step from now on,
 *    orc_solver_advance reduces the rate on the fields just reached (one more synchronisation), and sets dt_next by the law; a NaN or
 *    infinite rate there is ORC_ERR_SOLUTION_DIVERGED.  Refused: a control whose [dt_min, dt_max] does not contain dt_next.
 *    The choice lags one step: no step is rejected and repeated.
 *  - orc_solver_get_time_state (any output may be NULL) / orc_solver_set_time_state: with orc_solver_set_time_levels and
 *    orc_solver_set_time_step a run continues bit for bit.  orc_solver_set_time_levels alone assumes dt_last = dt_before_last = dt_next.
 *  - orc_solver_time_step_count / _history: one row per step while control is on or a manual step has been set — time reached, dt
 *    used, rate_max at its end (NaN where it was not measured), cell (-1 likewise and on a partitioned mesh).  A range past the
 *    history is ORC_ERR_BAD_ARGUMENT.
 *  - orc_solver_set_transient resets the time state, turns control off and clears the history; orc_solver_snapshot / _restore carry
 *    the time state (time, dt_next, dt_last, dt_before_last and the controller's step count), not the history.
 *  - orc_bench_courant: HIP-event average ms over `reps` of the reduction (courant_k and its fold) on the solver's current fields;
 *    orc_bench_derived_rate: the same for derived_cell_k selecting ORC_DERIVED_CONVECTIVE_RATE alone.
 * Refused with ORC_ERR_BAD_ARGUMENT, nothing changed: a null solver, the three set entries without the transient arm, a value that
 * is not positive and finite (time >= 0), a control outside the ranges of OrcTimeStepControl. */
void orc_time_step_control_default(OrcTimeStepControl *c);
int orc_time_step_next(const OrcTimeStepControl *c, double dt, double rate_max, double *dt_next);
int orc_solver_courant(OrcSolver *s, double *rate_max, int64_t *cell, double *rate);
int orc_solver_set_time_step(OrcSolver *s, double dt);
int orc_solver_set_time_step_control(OrcSolver *s, const OrcTimeStepControl *c);
int orc_solver_get_time_state(OrcSolver *s, double *time, double *dt_next, double *dt_last, double *dt_before_last);
int orc_solver_set_time_state(OrcSolver *s, double time, double dt_last, double dt_before_last);
int64_t orc_solver_time_step_count(OrcSolver *s);
int orc_solver_time_step_history(OrcSolver *s, uint64_t first, uint64_t count, double *out);
int orc_bench_courant(OrcSolver *s, int reps, double *avg_ms);
int orc_bench_derived_rate(OrcSolver *s, int reps, double *avg_ms);

/* ---------- passive scalar transport (new-build extension, orc_types.h OrcScalarSettings) ----------
 * Off by default: a solver that never calls orc_solver_set_scalar runs exactly the code it ran before.  The scalar is carried
 * by the flux face_k forms from the current u, v, w, p (Rhie-Chow included) and changes no bit of the flow state.
 *  - orc_scalar_settings_default: UD, BiCGSTAB + Jacobi, 500 iterations, relative threshold 1e-10, relaxation 0.5,
 *    30 outer rounds / 1e-8, Gamma = 1e-3.
 *  - orc_solver_set_scalar(s, c): c == NULL turns the arm off and frees its buffers; otherwise validates c (Gamma <= 0 or
 *    non-finite, unknown solver or preconditioner, reserved0 != 0, iterations or outer_iterations 0, negative tolerances:
 *    ORC_ERR_BAD_ARGUMENT; CD2 or an unknown scheme: ORC_ERR_UNSUPPORTED_SCHEME) and turns the arm on with phi = 0, no
 *    source, no time levels and every zone DEFAULT.  A refusal leaves the solver unchanged.
 *  - orc_solver_set_scalar_bc: zone = the index orc_mesh_update_zones uses; kind an OrcScalarBc; interior zones refused.
 *  - fields, sources and levels in ORC cell order.  orc_solver_set_scalar_levels needs both arms on (phi_nm1 may be NULL).
 *  - orc_solver_solve_scalar: one solve (UD, CD1: one linear solve; TVD: up to outer_iterations rounds of gradient, face
 *    correction, assembly and linear solve).  With Rhie-Chow it needs momentum diagonals (an orc_solver_iterate or an
 *    assembly first): ORC_ERR_BAD_ARGUMENT otherwise.  report (may be NULL): rounds used, last relative change, min phi,
 *    max phi over the owned cells.  orc_solver_iterate never touches the scalar.
 *  - orc_solver_advance with both arms on: after each step's SIMPLE iterations the scalar levels shift (n-1 <- n, n <- phi)
 *    and the scalar is solved once with its time term; orc_solver_last_scalar_report returns that solve's report.
 *  - orc_solver_assemble_scalar: the system of the current state (TVD: its correction from the current phi); a in pattern
 *    order like orc_solver_assemble_momentum, b in the mesh's internal cell order; either may be NULL.
 *  - orc_solver_scalar_boundary_flux: per zone (n_zones doubles) the convective plus diffusive flux of phi INTO the domain
 *    under the current phi and flow; interior zones 0.
 *  - orc_solver_snapshot / orc_solver_restore include phi, its levels and their count while the arm is on. */
void orc_scalar_settings_default(OrcScalarSettings *c);
int orc_solver_set_scalar(OrcSolver *s, const OrcScalarSettings *c);
int orc_solver_set_scalar_bc(OrcSolver *s, int32_t zone, int32_t kind, double value);
int orc_solver_set_scalar_field(OrcSolver *s, const double *phi);
int orc_solver_get_scalar_field(OrcSolver *s, double *phi);
int orc_solver_set_scalar_source(OrcSolver *s, const double *source /* per unit volume, NULL = none */);
int orc_solver_set_scalar_levels(OrcSolver *s, const double *phi_n, const double *phi_nm1 /* may be NULL */);
int orc_solver_solve_scalar(OrcSolver *s, double report[4]);
int orc_solver_last_scalar_report(OrcSolver *s, double report[4]);
int orc_solver_assemble_scalar(OrcSolver *s, double *a, double *b);
int orc_solver_scalar_boundary_flux(OrcSolver *s, double *per_zone);

/* ---------- variable scalar diffusivity (new-build extension, orc_types.h OrcScalarDiffusivity) ----------
 * Off by default: a solver that never calls these launches exactly what it launched before and allocates nothing new.  While a model
 * is on, the Gamma part of the scalar system (scalar_diffusion_var_k) and the boundary term of orc_solver_scalar_boundary_flux take a
 * per-cell Gamma evaluated on the fly; the row kernel, the solves and the flow never see it.
 *  - orc_scalar_diffusivity_default: CONSTANT, ARITHMETIC faces, schmidt_t 0.7, beta 0, phi_ref 0, clamp 1e-12 .. 1e12.
 *  - orc_solver_set_scalar_diffusivity(s, c): c == NULL or model CONSTANT switches the model off (the constant Gamma part comes back
 *    bit for bit).  Refused with ORC_ERR_BAD_ARGUMENT, the solver unchanged: scalar arm off, unknown model or face mode, a non-finite
 *    parameter, schmidt_t <= 0, a clamp that is not 0 < gamma_min <= gamma_max < inf, reserved0 != 0, FIELD without a field, EDDY unless
 *    the viscosity arm is on with model SMAGORINSKY or FIELD.  While EDDY is on, orc_solver_set_viscosity refuses to switch that arm
 *    off or to select a power-law or Carreau model.  orc_solver_set_scalar (NULL or new settings) switches the model off and frees
 *    the field.
 *  - orc_solver_set_scalar_diffusivity_field: the FIELD model's data, n_cells doubles in ORC cell order (on a partitioned mesh the
 *    rank's array, ghost entries included), every entry positive and finite; it may be set before or while FIELD is on.
 *  - The Gamma part is rebuilt when the model, the field, the arm's settings or a scalar condition changed; with EDDY also once at the
 *    start of every orc_solver_solve_scalar and orc_solver_assemble_scalar (so once per time step of orc_solver_advance); with LINEAR
 *    before every assembly from the current phi, and UD and CD1 solves then run the outer (Picard) loop as TVD solves do.
 *  - orc_solver_get_scalar_diffusivity: Gamma per cell under the current state (the constant while the model is off), cell order as
 *    orc_solver_get_scalar_field.
 *  - orc_bench_scalar_diffusivity: HIP-event ms per launch of [0] scalar_diffusion_k (the constant Gamma part), [1]
 *    scalar_diffusion_var_k of the model that is on, [2] the boundary-term pass scalar_face_var_k; all three write scratch buffers. */
void orc_scalar_diffusivity_default(OrcScalarDiffusivity *c);
int orc_solver_set_scalar_diffusivity(OrcSolver *s, const OrcScalarDiffusivity *c);
int orc_solver_set_scalar_diffusivity_field(OrcSolver *s, const double *gamma /*[n_cells]*/);
int orc_solver_get_scalar_diffusivity(OrcSolver *s, double *gamma /*[n_cells]*/);
int orc_bench_scalar_diffusivity(OrcSolver *s, int reps, double avg_ms[3]);

/* ---------- surface reports (new-build extension) ----------
 * Force, moment, mass and momentum flow, area and area-weighted pressure of every boundary zone (orc_types.h OrcSurfaceQuantity;
 * DESIGN.md §3 "Surface reports" has the definitions and the operator order).  Opt-in and read-only: two kernels over the boundary
 * faces only, through an index the mesh builds on the device at its first report and keeps; zone types and values are read from the
 * mesh's current zone table at report time.  Fixed association, no float atomics: the same state gives the same bits.  Interior
 * zones and zones without owned faces give zeros; a boundary face in a zone whose type the assembly refuses (anything but Wall,
 * VelocityInlet, PressureInlet, PressureOutlet, Symmetry) makes the call return ORC_ERR_UNSUPPORTED_BC.  All three entries look for a
 * device first (ORC_ERR_NO_DEVICE without one, whatever the arguments); then a non-finite origin, a null solver / mesh / field /
 * output, and for orc_surface_integrals a non-finite or non-positive rho or mu, are ORC_ERR_BAD_ARGUMENT. */
/* per zone ORC_SURFACE_N doubles (orc_types.h OrcSurfaceQuantity), zone index as orc_mesh_update_zones uses it.
 * origin: reference point of MOMENT, NULL = (0,0,0).  Uses the solver's current u, v, w, p, rho, mu (with variable viscosity on: the
 * viscosity of the face's cell, see "variable viscosity" below) and the mesh's current zone table; changes no bit of the solver.  On a partitioned mesh every rank calls it and receives the global sums. */
int orc_solver_surface_report(OrcSolver *s, const double origin[3], double *per_zone /*[n_zones * ORC_SURFACE_N]*/);
/* the same on host fields in ORC cell order (post-processing a read_data file): uploads, reports, frees */
int orc_surface_integrals(OrcMesh *m, const double *u, const double *v, const double *w, const double *p,
                          double rho, double mu, const double origin[3], double *per_zone);
/* the boundary index (builds it if need be): zone_ptr[n_zones + 1]; faces (may be NULL) receives zone_ptr[n_zones] face ids
 * in the mesh's internal face numbering; *n_builds = how often this mesh has built it (stays 1); *chunk = faces per workgroup */
int orc_mesh_boundary_index(OrcMesh *m, int64_t *zone_ptr, int32_t *faces, int64_t *n_builds, int32_t *chunk);

/* ---------- residual monitors and convergence-controlled runs (new-build extension) ----------
 * Equation residuals and the mass imbalance of every SIMPLE iteration, a host-side history of them and a stopping rule
 * (orc_types.h OrcResidual, OrcConvergence; DESIGN.md §3 "Residual monitors" has the definitions and the operator order).
 * Off by default: a solver that never switches monitoring on launches exactly what it launched before.  Read-only: with monitoring on,
 * u, v, w, p, the eight report doubles and every later iteration keep their bits.  Fixed association, no float atomics: the same
 * state gives the same record.
 *  - orc_solver_set_monitors(s, on): on != 0 allocates the monitor's buffers, clears the history and resets the continuity scale;
 *    0 frees the buffers and the history.  From then on every iteration of orc_solver_iterate and every inner iteration of
 *    orc_solver_advance (whose own stopping rule is unchanged) appends one record: one fused pass over the three assembled momentum
 *    systems with the fields they were assembled from (the residual before the solve), one pass over the right-hand side of the
 *    pressure correction before its solve, folded on the device and copied with the iteration's last synchronisation.
 *    On a partitioned mesh the sums and maxima cover the owned rows of all ranks (two collectives per iteration, after the
 *    iteration's own) and every rank must switch monitoring the same way, before the same iteration.
 *  - orc_solver_residual_count: records so far.  orc_solver_residual_history: records [first, first + count) into out
 *    (count * ORC_RESIDUAL_N doubles); a range past the history is ORC_ERR_BAD_ARGUMENT.
 *  - orc_solver_snapshot / orc_solver_restore do not touch the history or the continuity scale.
 *  - orc_convergence_check: pure host arithmetic, no device needed.  Returns 1 when every scaled residual (record[16..19]) is <= its
 *    tolerance and that tolerance is > 0, else 0 (a NaN or infinite residual never converges); *failing_mask (may be NULL) gets bit
 *    k for equation k (u, v, w, continuity) that fails.  A null or invalid OrcConvergence (negative or NaN tolerance,
 *    reserved0 != 0) or a null record returns -1 with every bit set.
 *  - orc_solver_iterate_until: iterations until the check passes, but at least c->min_iterations, and at most max_iterations.
 *    Needs monitoring on.  report (may be NULL): 8 doubles of the LAST iteration run, laid out as orc_solver_iterate's.
 *    *iterations_done, *converged: may be NULL.
 *  - orc_solve_steady_converged: orc_solve_steady with that rule: at most max_iterations iterations; last_record (may be NULL)
 *    receives the last record.
 *  - orc_solver_get_pressure_rhs: the right-hand side of the pressure correction as the last iteration (or assembly) left it, in the
 *    mesh's internal cell order, n_cells doubles; assembles nothing.
 * All entries but orc_convergence_check look for a device first (ORC_ERR_NO_DEVICE without one, whatever the arguments); then a null
 * pointer or an invalid struct is ORC_ERR_BAD_ARGUMENT with the solver unchanged. */
int orc_solver_set_monitors(OrcSolver *s, int32_t on);
int64_t orc_solver_residual_count(OrcSolver *s);
int orc_solver_residual_history(OrcSolver *s, uint64_t first, uint64_t count, double *out /*[count * ORC_RESIDUAL_N]*/);
int orc_convergence_check(const OrcConvergence *c, const double record[ORC_RESIDUAL_N], int32_t *failing_mask);
int orc_solver_iterate_until(OrcSolver *s, uint64_t max_iterations, const OrcConvergence *c, double *report /*[8]*/,
                             uint64_t *iterations_done, int32_t *converged);
int orc_solve_steady_converged(OrcMesh *m, double *u, double *v, double *w, double *p, const OrcSettings *settings, double rho, double mu,
                               const OrcConvergence *c, uint64_t max_iterations, uint64_t reporting_interval, OrcReportFn report_cb,
                               void *user, uint64_t *iterations_done, int32_t *converged, double last_record[ORC_RESIDUAL_N]);
int orc_solver_get_pressure_rhs(OrcSolver *s, double *b_p /*[n_cells]*/);

/* ---------- derived fields, boundary-face maps and VTU export (new-build extension) ----------
 * Opt-in and read-only post-processing of a velocity field where it lives (DESIGN.md §3 "Derived fields and boundary maps").  The
 * compute entries look for a device first (ORC_ERR_NO_DEVICE without one, whatever the arguments); then a null pointer, mask == 0 or
 * a mask bit at or above ORC_DERIVED_N / ORC_BOUNDARY_N is ORC_ERR_BAD_ARGUMENT.  No atomics but a status word: the same state gives
 * the same bits. */
/* Cell fields (orc_types.h OrcDerivedField) selected by `mask`, from the velocity gradient of the solver's settings
 * (gradient_reconstruction: Green-Gauss or least squares, exactly orc_calculate_gradients' grad_u), never stored.  out: the
 * selected fields in ascending enum order, field k of the selection at out[k * n + c]; n, the cell order and the ownership are
 * orc_solver_get_fields' (ORC order also on a reordered mesh; on a partitioned mesh the rank's array length with the owned cells
 * filled and zeros behind them, ghost velocities exchanged first).  A boundary face in a zone the assembly refuses:
 * ORC_ERR_UNSUPPORTED_BC; a singular least-squares system: ORC_ERR_SINGULAR_MATRIX.  Changes no bit of the solver. */
int orc_solver_derived_fields(OrcSolver *s, uint32_t mask, double *out /*[popcount(mask) * n]*/);
/* the same on host fields in ORC cell order: uploads, computes, frees */
int orc_derived_fields(OrcMesh *m, const double *u, const double *v, const double *w, const OrcSettings *settings, uint32_t mask,
                       double *out);
/* Boundary-face maps (orc_types.h OrcBoundaryField): one value per face of orc_mesh_boundary_index, in its order; field k of the
 * selection at out[k * nb + i], nb = zone_ptr[n_zones].  Terms, argument checks and refused zone types are the surface report's. */
int orc_solver_boundary_fields(OrcSolver *s, uint32_t mask, double *out /*[popcount(mask) * nb]*/);
int orc_boundary_fields(OrcMesh *m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                        uint32_t mask, double *out);
/* VTK XML UnstructuredGrid (.vtu, version 1.0, header_type UInt64, little endian); host only, no device needed.  Cells with four
 * triangles are VTK_TETRA, with six quadrilaterals over eight nodes VTK_HEXAHEDRON, every other cell VTK_POLYHEDRON; only the
 * points the file uses are written, renumbered ascending.  data[a]: components[a] * n_cells doubles, structure-of-arrays by
 * component.  encoding 0: ASCII (%.17g, round-trips exactly); 1: appended raw.  ORC_ERR_IO when the file cannot be written,
 * ORC_ERR_BAD_ARGUMENT for null or inconsistent arrays or an index out of range. */
int orc_write_vtu(const char *path, int64_t n_points, const double *points /*[3V]*/, int64_t n_cells, const int64_t *cell_face_ptr,
                  const int64_t *cell_faces, const int64_t *face_node_ptr, const int64_t *face_nodes, int32_t n_arrays,
                  const char *const *names, const int32_t *components, const double *const *data, int32_t encoding);
/* the faces face_ids[n_faces] as VTK_POLYGON cells (a boundary map); data[a]: components[a] * n_faces doubles */
int orc_write_vtu_faces(const char *path, int64_t n_points, const double *points, int64_t n_faces, const int64_t *face_ids,
                        const int64_t *face_node_ptr, const int64_t *face_nodes, int32_t n_arrays, const char *const *names,
                        const int32_t *components, const double *const *data, int32_t encoding);

/* ---------- variable viscosity (new-build extension, orc_types.h OrcViscosity) ----------
 * A per-cell viscosity in the momentum diffusion: a prescribed field, or a power-law, Carreau or Smagorinsky law of the strain-rate
 * magnitude (DESIGN.md §3 "Variable viscosity" has the definitions and the operator order).  Off by default: a solver that never calls
 * orc_solver_set_viscosity* launches exactly what it launched before and allocates nothing new.  The momentum assembly, Rhie-Chow and
 * the solves are untouched: two passes ahead of them evaluate the law per cell and rebuild the diffusion matrix a_di and its wall
 * terms b_u_di, b_v_di, b_w_di with a face viscosity.  The momentum equation keeps its Laplacian form div(mu grad U); the transpose
 * part div(mu (grad U)^T) is not added.
 *  - orc_solver_set_viscosity(s, c): checks c, then evaluates the law on the current fields (no relaxation) and rebuilds a_di at
 *    once.  From then on every SIMPLE iteration and every orc_solver_assemble_momentum re-evaluates the law on its fresh fields (not
 *    for FIELD), exchanges the ghost viscosities of a partitioned mesh and rebuilds a_di before the momentum assembly.  The first of
 *    these evaluations takes the law's value itself; later ones are relaxed with c->relaxation.  c == NULL turns the arm off, frees
 *    its buffers and puts the constant-mu a_di, b_*_di back, bit for bit.
 *  - orc_solver_set_viscosity_field: the FIELD model's data, n_cells doubles in ORC cell order (on a partitioned mesh the rank's
 *    array, ghost entries included), every entry > 0 and finite.  May be called before the model is selected; with FIELD on, a_di is
 *    rebuilt at once.
 *  - orc_solver_get_viscosity: the field the last assembly used (the constant mu while the arm is off), cell order as
 *    orc_solver_get_fields.
 *  - orc_solver_evaluate_viscosity: the law on the current fields without relaxation into mu, the strain-rate magnitude it was
 *    evaluated at into strain_rate (may be NULL); changes no bit of the solver.  Needs the arm on.
 *  - orc_solver_get_diffusion: a_di in the CSR order of orc_mesh_matrix_pattern and the three wall terms (each may be NULL).
 *  - orc_solver_surface_report and orc_solver_boundary_fields use the cell's viscosity in d = (mu A) / dist and in y+ while the arm
 *    is on; orc_surface_integrals and orc_boundary_fields keep the constant they are given.
 *  - orc_solver_snapshot / orc_solver_restore include the viscosity field and the first-evaluation flag while the arm is on.
 *  - On a partitioned mesh every rank makes the same calls in the same order: the set calls, orc_solver_evaluate_viscosity and
 *    orc_solver_assemble_momentum exchange ghost values (the velocities', then the viscosity's) while the arm is on.
 * Refused with ORC_ERR_BAD_ARGUMENT and the solver unchanged: a parameter outside its range or not finite, an unknown model or face
 * interpolation, FIELD without a field, a field entry that is not positive and finite, and a solver with frozen_diagonals = 0. */
void orc_viscosity_default(OrcViscosity *c);
int orc_solver_set_viscosity(OrcSolver *s, const OrcViscosity *c);
int orc_solver_set_viscosity_field(OrcSolver *s, const double *mu /*[n_cells]*/);
int orc_solver_get_viscosity(OrcSolver *s, double *mu /*[n_cells]*/);
int orc_solver_evaluate_viscosity(OrcSolver *s, double *mu /*[n_cells]*/, double *strain_rate /*[n_cells], may be NULL*/);
int orc_solver_get_diffusion(OrcSolver *s, double *a_di /*[nnz]*/, double *b_u_di, double *b_v_di, double *b_w_di /*[n_cells] each*/);
/* the two passes of the arm on the solver's current state, HIP-event average ms per launch over `reps`: avg_ms[0] the law pass
 * (viscosity_cell_k, into scratch), avg_ms[1] the rebuild (diffusion_var_k); needs the arm on, changes no bit of the solver */
int orc_bench_viscosity(OrcSolver *s, int reps, double avg_ms[2]);

/* ---------- wall distance and wall damping (new-build extension, orc_types.h OrcWallDamping) ----------
 * The wall faces of a mesh are the boundary faces of owned cells whose zone is a wall: zone_is_wall[n_zones] != 0, or with
 * zone_is_wall == NULL the zones of type ORC_BC_WALL.  The wall distance of a cell is the distance to the plane of the wall face whose
 * centroid is nearest to the cell's centroid; among faces that tie exactly in that squared centroid distance the smallest plane
 * distance wins (DESIGN.md §3 "Wall distance and wall damping": operator order, the approximation next to convex wall edges).  The
 * value depends on the set of wall faces only: not on their order, the cell numbering or a partition.  A mesh without a wall face
 * gives +inf.
 *  - orc_mesh_wall_distance: d in the cell order of orc_solver_get_fields (ORC order on a reordered mesh); the ghost entries of a
 *    partitioned mesh are 0.  The field is searched at first use and kept on the mesh, keyed by the resolved wall mask;
 *    orc_mesh_update_zones / orc_mesh_sync_zones drop it when the wall-ness of a zone changes.  On a partitioned mesh every rank calls
 *    it (the ranks' wall tables are gathered with two all-reduces).
 *  - orc_solver_set_wall_damping: checks w and stores it on the solver; it takes effect whenever the viscosity model is SMAGORINSKY
 *    (the wall distance of the default mask is then read by the law pass).  With SMAGORINSKY on, the field is re-evaluated at once
 *    without relaxation, as orc_solver_set_viscosity does.  w == NULL or mode NONE: the undamped law, bit for bit.  Refused with
 *    ORC_ERR_BAD_ARGUMENT and the solver unchanged: a value that is not finite, kappa (MIN), a_plus or u_tau (VAN_DRIEST) <= 0, an
 *    unknown mode, reserved0 != 0.
 *  - orc_solver_get_wall_damping: the stored setting; *enabled = 1 when its mode is not NONE.
 *  - orc_debug_wall_distance: the search without the cache; cull = 0 walks every table entry for every cell.
 *  - orc_debug_wall_search: out = {wall faces over all ranks, tile length T, tiles, tile visits summed over waves, waves}: the table
 *    of the last search and the visits and waves of all searches since the last reset (reset != 0 clears them after the read).
 *  - orc_bench_wall_distance: HIP-event average ms of `reps` launches of the search kernel alone on the default mask's table. */
int orc_mesh_wall_distance(OrcMesh *m, const int32_t *zone_is_wall /*[n_zones], NULL = type WALL*/, double *d /*[n_cells]*/);
void orc_wall_damping_default(OrcWallDamping *w);
int orc_solver_set_wall_damping(OrcSolver *s, const OrcWallDamping *w /*NULL = off*/);
int orc_solver_get_wall_damping(OrcSolver *s, OrcWallDamping *w, int32_t *enabled);
int orc_debug_wall_distance(OrcMesh *m, const int32_t *zone_is_wall, int cull, double *d /*[n_cells]*/);
int orc_debug_wall_search(long long out[5], int reset);
int orc_bench_wall_distance(OrcMesh *m, int cull, int reps, double *avg_ms);

/* ---------- running time statistics (new-build extension, orc_types.h OrcTimeStatistics) ----------
 * Time-averaged fields and the second moments of their fluctuations, accumulated where the fields live (DESIGN.md §3 "Time
 * statistics" has the definitions and the operator order).  Off by default: a solver that never calls
 * orc_solver_set_time_statistics launches exactly what it launched before and allocates nothing new.  Read-only towards the flow:
 * with the arm on, u, v, w, p, the scalar, the viscosity and every report keep their bits.  One fused streaming pass per sample
 * (time_stats_k) over K * n_cells accumulators, K = the fields of the enabled groups in OrcStatField order; no atomics, no
 * reductions: the same samples give the same bits.
 *  - orc_time_statistics_default: MEAN | STRESS, start_step 1, interval 1.
 *  - orc_solver_set_time_statistics(s, c): c == NULL turns the arm off and frees its buffers; otherwise validates c and turns the arm
 *    on with zeroed accumulators, weight sum W = 0, 0 samples and step counter 0.  It does not need the transient arm.
 *  - orc_solver_advance with the arm on: after each step's SIMPLE iterations (and the scalar solve) the step counter advances, and the
 *    step is sampled with weight dt when counter >= start_step and (counter - start_step) % interval == 0.
 *  - orc_solver_sample_statistics: one sample of the current state with the caller's weight (> 0, finite): for steady runs that
 *    oscillate, or a schedule of the caller's own.  It does not move the step counter.
 *  - orc_solver_reset_statistics: accumulators, W and the sample count go to zero; settings and step counter are kept.
 *  - orc_solver_statistics_info: samples, W, K and the number of boundary faces (0 unless BOUNDARY is on); each pointer may be NULL.
 *  - orc_solver_get_statistics: the fields of field_mask (OrcStatField bits, ascending) in the cell order of orc_solver_get_fields,
 *    field k of the selection at out[k * n_cells + c]; the ghost entries of a partitioned mesh are 0.  form RAW: means and weighted
 *    co-moment sums C; NORMALISED: means and C / W (divided on the host).  RAW with 0 samples returns zeros.
 *  - orc_solver_set_statistics_state: the restart path.  raw holds exactly the enabled cell fields (field_mask must equal the enabled
 *    mask) as orc_solver_get_statistics(RAW) returned them; boundary_means holds the 5 * nb doubles of
 *    orc_solver_get_boundary_statistics when BOUNDARY is on and must be NULL otherwise.  samples == 0 exactly when weight_sum == 0.
 *    Sampling continues as if the earlier samples had been taken on this solver, bit for bit.
 *  - orc_solver_get_boundary_statistics: the means of ORC_BOUNDARY_PRESSURE, TRACTION_X, _Y, _Z and SHEAR_MAG of every face of
 *    orc_mesh_boundary_index, in its order, field k at out[k * nb + i]; needs the BOUNDARY group.  A boundary face in a zone whose type
 *    the assembly refuses makes this call and orc_solver_set_time_statistics return ORC_ERR_UNSUPPORTED_BC.
 *  - orc_solver_snapshot / orc_solver_restore do not touch the statistics (as they do not touch the pressure-solver override).
 *  - On a partitioned mesh every rank enables the same groups and samples at the same steps; nothing is communicated.
 *  - orc_bench_time_statistics: HIP-event average ms per launch over `reps`: avg_ms[0] the cell pass (time_stats_k of the enabled
 *    groups, on scratch accumulators), avg_ms[1] the boundary pass (boundary_map_k and stats_mean_k; 0 without BOUNDARY); needs the
 *    arm on, changes no bit of the solver or its statistics.
 * All entries but orc_time_statistics_default look for a device first (ORC_ERR_NO_DEVICE without one).  Refused with
 * ORC_ERR_BAD_ARGUMENT and the solver unchanged: a null solver or output; groups without MEAN or with unknown bits, reserved0 != 0,
 * interval 0, VISCOSITY without the viscosity arm, SCALAR without the scalar arm; a weight <= 0 or not finite; any entry but the set
 * call while the arm is off; a field_mask of 0, with unknown bits or with a field whose group is off; an unknown form; NORMALISED
 * with 0 samples; a state whose mask is not the enabled one, whose weight_sum is negative or not finite, or whose boundary pointer
 * does not match the BOUNDARY group.  orc_solver_set_scalar(s, NULL) and orc_solver_set_viscosity(s, NULL) are refused the same way
 * while the SCALAR or VISCOSITY group is on. */
void orc_time_statistics_default(OrcTimeStatistics *c);
int orc_solver_set_time_statistics(OrcSolver *s, const OrcTimeStatistics *c /*NULL = off*/);
int orc_solver_sample_statistics(OrcSolver *s, double weight);
int orc_solver_reset_statistics(OrcSolver *s);
int orc_solver_statistics_info(OrcSolver *s, uint64_t *samples, double *weight_sum, int32_t *n_fields, int64_t *n_boundary_faces);
int orc_solver_get_statistics(OrcSolver *s, uint32_t field_mask, int32_t form, double *out /*[popcount(field_mask) * n_cells]*/);
int orc_solver_set_statistics_state(OrcSolver *s, uint64_t samples, double weight_sum, uint32_t field_mask,
                                    const double *raw /*[K * n_cells]*/, const double *boundary_means /*[5 * nb] or NULL*/);
int orc_solver_get_boundary_statistics(OrcSolver *s, double *out /*[5 * nb]*/);
int orc_bench_time_statistics(OrcSolver *s, int reps, double avg_ms[2]);

/* ---------- point probes (new-build extension, orc_types.h OrcProbeStatus / OrcProbeField / OrcProbeInterpolation) ----------
 * A probe set is a list of points located in the cells of one mesh: per point the owned cell with the nearest centroid, then a walk
 * across faces to a cell that contains the point (orc_types.h, DESIGN.md §3 "Point probes": operator order and tie rules).  The set
 * lives on the device; a solver of the same mesh samples its fields there, at any time or step by step into a history.  Opt-in and
 * read-only: no entry changes a bit of a mesh or a solver, and a solver without a probe history launches what it launched before.
 *  - orc_probes_create: locates all n_points points xyz (point-major) at once; NULL + *status on failure.  A partitioned mesh is
 *    refused (a rank-confined walk leaves points unclaimed).  Destroy a probe set before its mesh.
 *  - orc_probes_get: per point the cell (ORC order, as orc_mesh_cell_order), the OrcProbeStatus, the moves of the walk, the zone of the
 *    boundary face an OUTSIDE point left through (-1 otherwise) and the excess, the largest g of the final cell (<= 0 exactly when
 *    INSIDE).  Each output may be NULL.
 *  - orc_solver_sample_probes: the fields of field_mask (OrcProbeField bits, ascending) at the points, field k at out[k * n_points + i].
 *    OUTSIDE and WALK_LIMIT points are sampled at their final cell.  LINEAR evaluates the cell's gradient for the hit cells only, by the
 *    assembly's per-cell bodies; a zone type the assembly refuses returns ORC_ERR_UNSUPPORTED_BC, a singular least-squares system
 *    ORC_ERR_SINGULAR_MATRIX, as orc_solver_derived_fields.
 *  - orc_solver_set_probe_history: p == NULL turns the history off and drops it; otherwise from now on orc_solver_advance appends one
 *    record after every step whose counter (steps since enabling, first = 1) is a multiple of `interval`: the time reached (slot 9 of
 *    the step's report) and popcount(field_mask) * n_points values laid out as by orc_solver_sample_probes.  The record is sampled on
 *    the device after the step's statistics and copied asynchronously: no synchronisation is added to a step.
 *  - orc_solver_record_probes: appends one record of the current state with `tag` in the time slot (steady runs).
 *  - orc_solver_probe_history_count / orc_solver_probe_history: the records [first, first + count); times[count],
 *    out[count][popcount][n_points]; each may be NULL.  orc_solver_snapshot / orc_solver_restore leave the history alone.
 *  - orc_debug_probes_locate: orc_probes_create with cull = 0 (every cell for every point) or a forced number of cell slabs (0 = the
 *    library's choice); the result does not depend on either.
 *  - orc_debug_probe_search: out = {cell tile length T, cell tiles of the last search, tile visits summed over waves, waves, slabs of
 *    the last search, walk moves summed over points}, the sums since the last reset.
 *  - orc_bench_probe_locate: HIP-event average ms over `reps` of avg_ms[0] the search and its fold, avg_ms[1] the walk, of the points
 *    of `p` on scratch buffers.
 * Every entry looks for a device first (ORC_ERR_NO_DEVICE without one).  Refused with ORC_ERR_BAD_ARGUMENT, solver and mesh unchanged:
 * a null mesh, solver, probe set or coordinate array; n_points < 1; a coordinate that is not finite; a partitioned mesh; a field_mask
 * of 0 or with unknown bits; ORC_PROBE_PHI without the scalar arm; an unknown interpolation; interval 0; a probe set of another mesh;
 * orc_solver_record_probes and orc_solver_probe_history while the history is off; a range past the history. */
typedef struct OrcProbes OrcProbes;
OrcProbes *orc_probes_create(OrcMesh *m, int64_t n_points, const double *xyz /*[3 * n_points] point-major*/, int *status);
void orc_probes_destroy(OrcProbes *p);
int64_t orc_probes_count(const OrcProbes *p);
int orc_probes_get(const OrcProbes *p, int64_t *cell, int32_t *status, int32_t *steps, int32_t *zone, double *excess /*[n_points] each, or NULL*/);
int orc_solver_sample_probes(OrcSolver *s, const OrcProbes *p, uint32_t field_mask, int32_t interpolation,
                             double *out /*[popcount(field_mask) * n_points]*/);
int orc_solver_set_probe_history(OrcSolver *s, const OrcProbes *p /*NULL = off*/, uint32_t field_mask, int32_t interpolation, uint64_t interval);
int orc_solver_record_probes(OrcSolver *s, double tag);
int64_t orc_solver_probe_history_count(OrcSolver *s);
int orc_solver_probe_history(OrcSolver *s, uint64_t first, uint64_t count, double *times /*[count]*/, double *out /*[count * popcount * n_points]*/);
OrcProbes *orc_debug_probes_locate(OrcMesh *m, int64_t n_points, const double *xyz, int cull, int slabs /*0 = automatic*/, int *status);
int orc_debug_probe_search(long long out[6], int reset);
int orc_bench_probe_locate(OrcMesh *m, const OrcProbes *p, int cull, int reps, double avg_ms[2]);

/* ---------- volume reports (new-build extension, orc_types.h OrcGroupQuantity / OrcGroupWeighting) ----------
 * A cell group set is a labelling of the cells of one mesh: group_of_cell[c] in [0, n_groups) for ORC cell c, or -1 for "in no group".
 * A report reduces cell fields over every group on the device (orc_types.h, DESIGN.md §3 "Volume reports": definitions, operator order,
 * association): sums[G][F][ORC_GROUP_N], weight[G][2] = (W, number of cells) and where[G][F][2] = the ORC ids of the cells of MIN and
 * MAX; each output may be NULL.  Sums are deterministic (no float atomics) and depend on the group set only, not on the mesh's internal
 * numbering.  Opt-in and read-only: no entry changes a bit of a mesh or a solver, and a solver without a group history launches what it
 * launched before.
 *  - orc_cell_groups_create: built once on the host and uploaded; NULL + *status on failure.  Destroy a set before its mesh, and after
 *    any solver whose group history reads it.  A partitioned mesh is refused.
 *  - orc_cell_groups_get: group_ptr[G + 1] into cells, cells[group_ptr[G]] the ORC ids ascending inside a group, *chunk the list entries
 *    one workgroup of a report takes; each may be NULL.  orc_group_limits: the fields of one launch (more run in batches), that chunk,
 *    the entries of one lane, the largest n_groups.
 *  - orc_solver_group_report: the solver's current fields of field_mask (OrcProbeField bits, ascending; PHI needs the scalar arm, MU is
 *    the constant while the viscosity arm is off).
 *  - orc_group_integrals: n_fields caller fields, field k at fields[k * n_cells + c], ORC order.
 *  - orc_solver_group_statistics: the running statistics of stat_field_mask (OrcStatField bits) in `form` (OrcStatForm), reduced where
 *    they lie: per cell exactly the value orc_solver_get_statistics returns.
 *  - orc_solver_set_group_history: g == NULL turns the history off and drops it; otherwise from now on orc_solver_advance appends one
 *    report of field_mask after every step whose counter (steps since enabling, first = 1) is a multiple of `interval`, with the time
 *    reached.  Reduced on the device after the step's other arms and copied asynchronously: no synchronisation is added to a step.
 *  - orc_solver_record_groups: appends one record of the current state with `tag` in the time slot (steady runs).
 *  - orc_solver_group_history_count / orc_solver_group_history: the records [first, first + count): times[count],
 *    sums[count][G][F][ORC_GROUP_N], weight[G][2], where[count][G][F][2]; each may be NULL.
 *  - orc_bench_group_report: HIP-event average ms over `reps` of avg_ms[0] group_chunk_k and avg_ms[1] group_fold_k on the solver's
 *    fields of field_mask (at most one launch's fields).
 * Every entry but orc_cell_groups_get / _count / orc_group_limits looks for a device first.  Refused with ORC_ERR_BAD_ARGUMENT, nothing
 * changed: a null mesh, solver, label or field array; n_groups outside [1, ORC_GROUP_MAX_GROUPS]; a label outside [-1, n_groups); a
 * partitioned mesh; a group set of another mesh; a field_mask of 0 or with unknown bits; ORC_PROBE_PHI without the scalar arm; n_fields
 * outside [1, ORC_GROUP_MAX_FIELDS]; an unknown weighting; what orc_solver_get_statistics refuses; interval 0; orc_solver_record_groups
 * and the history read-outs while the history is off; a range past the history. */
typedef struct OrcCellGroups OrcCellGroups;
OrcCellGroups *orc_cell_groups_create(OrcMesh *m, int32_t n_groups, const int32_t *group_of_cell /*[n_cells] ORC order*/, int *status);
void orc_cell_groups_destroy(OrcCellGroups *g);
int32_t orc_cell_groups_count(const OrcCellGroups *g);
int orc_cell_groups_get(const OrcCellGroups *g, int64_t *group_ptr /*[G + 1]*/, int64_t *cells /*[group_ptr[G]] ORC ids*/, int32_t *chunk);
int orc_group_limits(int32_t *fields_per_launch, int32_t *chunk, int32_t *lane_slots, int32_t *max_groups);
int orc_solver_group_report(OrcSolver *s, OrcCellGroups *g, uint32_t field_mask, int32_t weighting, double *sums, double *weight, int64_t *where);
int orc_group_integrals(OrcMesh *m, OrcCellGroups *g, int32_t n_fields, const double *fields /*[n_fields][n_cells] ORC order*/, int32_t weighting,
                        double *sums, double *weight, int64_t *where);
int orc_solver_group_statistics(OrcSolver *s, OrcCellGroups *g, uint32_t stat_field_mask, int32_t form, int32_t weighting, double *sums,
                                double *weight, int64_t *where);
int orc_solver_set_group_history(OrcSolver *s, OrcCellGroups *g /*NULL = off*/, uint32_t field_mask, int32_t weighting, uint64_t interval);
int orc_solver_record_groups(OrcSolver *s, double tag);
int64_t orc_solver_group_history_count(OrcSolver *s);
int orc_solver_group_history(OrcSolver *s, uint64_t first, uint64_t count, double *times, double *sums, double *weight, int64_t *where);
int orc_bench_group_report(OrcSolver *s, OrcCellGroups *g, uint32_t field_mask, int32_t weighting, int reps, double avg_ms[2]);

/* ---------- tracer particles (new-build extension, orc_types.h OrcTracerStatus / OrcTracerSettings) ----------
 * A tracer set is a list of massless particles in the cells of one mesh, kept on the device: per particle the position, the cell, the
 * OrcTracerStatus, the zone it left through (-1 otherwise), the age (the signed sum of the accepted h) and the accepted substeps.  A
 * solver of the same mesh moves the set through its current u, v, w (orc_types.h, DESIGN.md §3 "Tracer particles": the substep and its
 * operator order).  Opt-in and read-only towards mesh and solver: a solver that calls no tracer entry launches what it launched before.
 *  - orc_tracers_create: the seeds xyz (point-major) located exactly as orc_probes_create locates points; INSIDE seeds start ACTIVE,
 *    OUTSIDE seeds LEFT with the walk's zone, WALK_LIMIT seeds WALK_LIMIT, and the latter two never move.  NULL + *status on failure.  A
 *    partitioned mesh is refused.  Destroy a set before its mesh, and after any solver that tracks it.
 *  - orc_tracers_get: each output [n] (xyz [3 n] point-major, cell in ORC order) or NULL.
 *  - orc_solver_advect_tracers: up to n_substeps substeps of every particle in the solver's current velocity.  record_stride > 0 (which
 *    n_substeps must be a multiple of, K = n_substeps / record_stride) also returns the path: record k of path[K + 1][3][n] holds the
 *    positions after k record_stride substeps of this call, record 0 those at entry, a stopped particle repeating its last position;
 *    path_len[i] = min(K + 1, 1 + ceil(a_i / record_stride)) with a_i the substeps particle i accepted in this call (may be NULL).  One
 *    launch per record, no synchronisation between them.  With LINEAR a zone type the assembly refuses returns ORC_ERR_UNSUPPORTED_BC
 *    and a singular least-squares system ORC_ERR_SINGULAR_MATRIX, as orc_solver_sample_probes; the set is then as it was before the call.
 *  - orc_solver_sample_tracers: orc_solver_sample_probes at the particles' present positions and cells.
 *  - orc_solver_set_tracer_tracking: t == NULL turns it off; otherwise from now on every step of orc_solver_advance moves the set by
 *    substeps_per_step substeps of h = dt / substeps_per_step in the velocity of the new time level (first order in time),
 *    after the probe history and without a synchronisation.  Needs orc_solver_set_transient, step_mode TIME and direction +1; `step` is
 *    ignored.  A gradient failure of a step is returned by the next step or the next call of this entry.  orc_solver_snapshot /
 *    orc_solver_restore leave the set alone.
 *  - orc_write_vtu_lines: host only; one VTK_POLY_LINE cell per line (VTK_VERTEX for a line of one point) over points
 *    [line_ptr[i], line_ptr[i + 1]) with point data arrays (component-major per array), in the conventions of orc_write_vtu_faces.
 *  - orc_bench_tracers: HIP-event average ms over `reps` of one launch of n_substeps substeps from the set's state into scratch buffers.
 * Every compute entry looks for a device first (ORC_ERR_NO_DEVICE without one).  Refused with ORC_ERR_BAD_ARGUMENT, solver, mesh and set
 * unchanged: null arguments; n < 1; a coordinate that is not finite; a partitioned mesh; a set of another mesh; an unknown scheme,
 * interpolation, step mode or direction; a step that is not positive and finite (except under tracking); a min_speed that is not >= 0;
 * record_stride > 0 with n_substeps not a multiple of it or with a null path; tracking without the transient arm, with LENGTH, with
 * direction -1 or with substeps_per_step = 0.  LINEAR with an unsupported gradient scheme: ORC_ERR_UNSUPPORTED_SCHEME. */
typedef struct OrcTracers OrcTracers;
void orc_tracer_settings_default(OrcTracerSettings *c); /* RK2, LINEAR, LENGTH, +1, step 0 (must be set), min_speed 0 */
OrcTracers *orc_tracers_create(OrcMesh *m, int64_t n, const double *xyz /*[3 * n] point-major*/, int *status);
void orc_tracers_destroy(OrcTracers *t);
int64_t orc_tracers_count(const OrcTracers *t);
int orc_tracers_get(const OrcTracers *t, double *xyz, int64_t *cell, int32_t *status, int32_t *zone, double *age, int64_t *steps);
int orc_solver_advect_tracers(OrcSolver *s, OrcTracers *t, const OrcTracerSettings *c, uint64_t n_substeps, uint64_t record_stride /*0 = no path*/,
                              double *path /*[K + 1][3][n]*/, int32_t *path_len /*[n]*/);
int orc_solver_sample_tracers(OrcSolver *s, const OrcTracers *t, uint32_t field_mask, int32_t interpolation,
                              double *out /*[popcount(field_mask) * n]*/);
int orc_solver_set_tracer_tracking(OrcSolver *s, OrcTracers *t /*NULL = off*/, const OrcTracerSettings *c, uint32_t substeps_per_step);
int orc_write_vtu_lines(const char *path, int64_t n_lines, const int64_t *line_ptr /*[n_lines + 1]*/, const double *points /*[3 * line_ptr[n_lines]]*/,
                        int32_t n_arrays, const char *const *names, const int32_t *components, const double *const *data /*per point*/, int32_t encoding);
int orc_bench_tracers(OrcSolver *s, const OrcTracers *t, const OrcTracerSettings *c, uint64_t n_substeps, int reps, double *avg_ms);

/* ---------- measurement hooks (bench.py): HIP-event timed launches of single kernels ---------- */
/* y = A x with the momentum matrix a_u of the solver, `reps` launches; returns average ms per launch */
int orc_bench_spmv(OrcSolver *s, int reps, double *avg_ms, double *checksum);
/* one BiCGSTAB iteration body (linear_algebra.rs:255-268) repeated `reps` times on a_u */
int orc_bench_bicgstab_iteration(OrcSolver *s, int reps, double *avg_ms);
/* The Multigrid hierarchy of the momentum system a_u as the solver builds it (Jacobi-scaled operator, levels 0..3):
 * per level rows, stored non-zeros, padded SELL-64 entries and the HIP-event average of `reps` products y = A x.
 * Arrays hold up to 4 entries; *n_levels receives the count (level 0 = the mesh-pattern matrix). */
/* bench.py's headline roofline: the level-0 products of a_u as the solver's BiCGSTAB iterations launch them inside the
 * Multigrid arm (two Jacobi scalings, reduction epilogues), timed with HIP events on the library stream.  avg_ms[0], [1]: one
 * system per launch (nu = A p with sum(nu); t = A s with t.s, t.t); avg_ms[2], [3]: u, v, w in one launch (0 when unsupported). */
int orc_bench_inloop_products(OrcSolver *s, int reps, double avg_ms[4]);
/* the fused residual pass of the monitors (momentum_residual3_k with its folds) on the solver's assembled momentum systems and
 * current fields: average ms per pass over `reps`; needs orc_solver_set_monitors */
int orc_bench_momentum_residuals(OrcSolver *s, int reps, double *avg_ms);
/* "<narrow>, <scaled>": the last two template arguments of the kernels orc_bench_inloop_products has just launched
 * (spmv_uniform_k<Epi, false, true, narrow, scaled>), so that bench.py names the kernel as a kernel trace does */
const char *orc_bench_inloop_variant(void);
/* one multicolour Gauss-Seidel sweep over a_u (extension; BASELINE configs[2]): n_colors launches of the colour-sorted
 * kernel per sweep, average ms per sweep over `reps` sweeps */
int orc_bench_gs_sweep(OrcSolver *s, int reps, double *avg_ms, int *n_colors);
/* [r04] the preconditioner application x^ = M^-1 b as the slot-space GS-BiCGSTAB launches it (one sweep from zero without a zero fill,
 * n_colors launches): avg_ms[0] one system (the p' solve), avg_ms[1] the u, v, w momentum systems per launch */
int orc_bench_gs_sweep0(OrcSolver *s, int reps, double avg_ms[2], int *n_colors);
int orc_bench_amg_levels(OrcSolver *s, int reps, int64_t *rows, int64_t *nnz, int64_t *padded, double *avg_ms, int *n_levels);
/* Test hook: how many level-0 products of partitioned operators this thread has run in the overlapped form (interior rows
 * on a second stream beside the halo exchange, rows along the cuts after it) since orc_init. */
long long orc_debug_halo_overlaps(void);
/* Which of the library's streams still hold work — hipStreamQuery, never blocks; meant for a watchdog thread while the calling thread of a
 * solve waits: one line per stream, "<name>[<lane>] priority <p> busy|idle".  Returns the number of busy streams (-1: buffer too short). */
int orc_debug_stream_report(char *buf, int cap);
/* [r04] test hooks.  orc_debug_clamp_partials_grid: the ONE function through which every launcher sizes a grid whose workgroups
 * write per-workgroup partial sums (<= orc_debug_max_partials(), whatever the CU count or a measurement switch asks for); host only.
 * orc_debug_amg_certification: out[0] = aggregations whose asynchronous cascades were followed by the certifying lock-step
 * rounds, out[1] = the rounds those took in total; equal means no certification changed a pairing.  orc_debug_xwin_counters:
 * out[0] = 256-row blocks of coarse operators given an LDS x window description since the last reset, out[1] = of those
 * without a window because it would exceed the cap (ORC_XWIN_CAP <= 5000 entries), out[2] = because the block's column span
 * exceeds the bitmap (ORC_XWIN_BITWORDS <= 8192 words of 32 columns): the products of such blocks gather from global memory. */
/* orc_debug_amg_coarse_product: one level of the Multigrid set-up on (A) — pairing, (R a) R^T, and where the coarse rows are
 * long enough (ORC_SPMV_XWIN_MIN_NNZ, 24 entries per row) the packed mirror with its LDS x windows — then y = Ac x launched as
 * the solves launch it (linear_algebra.rs:82-97: `a_prime * e_prime`); x, y hold ceil(n / 2) doubles.  scaled != 0: the Jacobi
 * scaling 1 / diag materialised into the streamed values, as inside a smoothing solve (:159-166).  Ac itself comes from
 * orc_amg_coarsen (same kernels), so a test can evaluate the same product on the oracle. */
int orc_debug_amg_coarse_product(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values, int scaled, const double *x,
                                 double *y, int *has_window_mirror);
/* orc_debug_amg_packed_mirror: the same set-up, and the coarse level's packed mirror and LDS x windows as the products read them:
 * sizes = {coarse rows, slices, value slots, window-position slots, 256-row blocks} (0 slots: no mirror); the arrays (row_len [rows],
 * pk_ptr [slices + 1], pk_col / pk_val [value slots], lptr [slices + 1], lidx [position slots], wcol [blocks * 5000], wsize [blocks])
 * are written only if none of them is null, so a caller asks for the sizes first. */
int orc_debug_amg_packed_mirror(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values, int64_t sizes[5], int32_t *row_len,
                                int64_t *pk_ptr, int32_t *pk_col, double *pk_val, int64_t *lptr, uint16_t *lidx, int32_t *wcol, int32_t *wsize);
/* [r08] orc_debug_amg_xwin_raw: the same set-up, and the level's window streams byte for byte as the products read them (ORC_XWIN_COMPACT; the hook
 * above keeps returning the wide image, expanded on the host where the level is stored compactly).  info = {coarse rows, slices, 256-row blocks
 * (0: no mirror), window-position slots, bits per position (12 where the level's LDS share is at most 4096 entries, else 16), bytes of the position
 * stream, the level's LDS share in entries, blocks with 16-bit window columns, blocks with a window and 32-bit columns, bytes of window columns a
 * product reads}.  A granule of eight 12-bit positions is 12 bytes, position u in bits [12 u, 12 u + 12) of its 96, slice s at byte 1.5 lptr[s].
 * A block owns 5000 words of wcol_raw: with wfmt[b] = 0 its wsize[b] columns, with wfmt[b] = 1 ceil(wsize[b] / 64) bases (the column of list entry
 * 64 s) followed by wsize[b] 16-bit offsets from the base of the entry's segment.  The arrays (lptr [slices + 1], pos_raw [bytes of the position
 * stream], wcol_raw [blocks * 5000], wsize / wfmt [blocks]) are written only if none of them is null, so a caller asks for info first. */
int orc_debug_amg_xwin_raw(int64_t n, const int64_t *row_ptr, const int64_t *col_idx, const double *values, int64_t info[10], int64_t *lptr,
                           unsigned char *pos_raw, int32_t *wcol_raw, int32_t *wsize, int32_t *wfmt);
/* collectives this process has issued since the last reset — halo exchanges (one grouped ncclSend/ncclRecv launch each) and
 * all-reduces, status agreements included: the latency-bound messages of a partitioned SIMPLE iteration */
long long orc_debug_collectives(int reset);
int orc_debug_clamp_partials_grid(long long requested);
int orc_debug_max_partials(void);
/* Test hook, host only (no device, no orc_init): the schedule a SIMPLE iteration would run for these inputs — the one decision of
 * orc_amd/csrc/schedule.hpp, which no test of results can see because every schedule computes the same bits.  switches: bit 0
 * ORC_CONCURRENT_MOMENTUM, 1 ORC_TRIPLE_MOMENTUM, 2 ORC_EARLY_P_HIERARCHY, 3 ORC_TWO_STREAM_MULTIGRID, 4 ORC_AMG_SIBLING (the solver's five
 * switches), 5 partitioned mesh, 6 ORC_DEBUG_NAN, 7 profiling enabled, 8 the slot-space Gauss-Seidel sweep enabled; the solver types are
 * OrcSolverType of the momentum systems and of the pressure correction.  Returns momentum + 256 * p_hierarchy with momentum 0 sequential,
 * 1 lanes, 2 lanes on a partitioned mesh, 3 lock-step and p_hierarchy 0 inside the solve (or none), 1 early, 2 late. */
int orc_debug_schedule(unsigned switches, int momentum_solver, int p_solver, int reduction_order);
int orc_debug_amg_certification(long long out[2], int reset);
/* Test hook: what the calling process's most recent pairing (build_restriction_matrix, linear_algebra.rs:30-60) and the Galerkin product
 * behind it did; not cumulative.  out[0..4] = the deferred-acceptance chains: rows left to them, their proposals, proposals found by a scan of
 * the row (its four-entry preference list having run out), proposals of the longest chain, chains cut by the step budget (ORC_AMG_DA_STEPS);
 * out[5] = rows the certifying pass would have paired differently; out[6] = sweeps of the slice-sequential fallback (0: it did not run, the
 * chains' pairing was certified as it stood); out[7] = lanes per chain (0: ORC_AMG_DA=0, or a sibling's pairing was taken over);
 * out[8..14] = coarse rows per LDS tier of the merge (tier t holds rows of at most 32 << t candidate entries; longer rows, which the set-up
 * refuses, count in the last); out[15] = the largest candidate count.  Host-side copies of counters the set-up reads anyway: no device
 * access, no synchronisation. */
int orc_debug_amg_setup_stats(long long out[16], int reset);
int orc_debug_xwin_counters(long long out[3], int reset);
/* [r04] coarse operators of SIBLING systems built by a shared Galerkin pass since the last reset (the u, v, w momentum matrices of a
 * SIMPLE iteration share their pattern; when v's and w's fine pairings verify as u's, ONE symbolic pass carries the three value sets:
 * linear_algebra.rs:80-84 per system, bit-identical).  ORC_AMG_SHARED_GALERKIN=0 switches the shared pass off. */
long long orc_debug_shared_galerkin(int reset);
/* Test hook: product launches per kernel family since the last reset.  launch_spmv (orc_amd/csrc/spmv.hip) picks one of about a
 * dozen instantiations by the matrix (raggedness class, narrow column image, mirrors) and by the call (scalings carried or materialised,
 * non-temporal policy); the counters are incremented on the host where each launch is made, so a test that compares a product bit for
 * bit can tell which kernel produced the bits.  out[f] for f < min(n_out, ORC_PRODUCT_FAMILIES) (further entries are zeroed); out may
 * be null (reset only).  Returns ORC_PRODUCT_FAMILIES.  No device code; neither kernel arguments nor the dispatch depend on it. */
enum {
    ORC_PRODUCT_RAGGED = 0,         /* spmv_k<Epi, kSpmvRagged>: long ragged rows (class 1) without a mirror */
    ORC_PRODUCT_PACKED = 1,         /* spmv_k<Epi, kSpmvPacked>: packed mirror without windows */
    ORC_PRODUCT_WINDOW = 2,         /* spmv_xwin_k: packed mirror with LDS x windows */
    ORC_PRODUCT_GENERIC_SCALED = 3, /* spmv_uniform_k<Epi, false>: scalings applied on the fly (32-bit columns) */
    ORC_PRODUCT_WIDE = 4,           /* spmv_uniform_k<Epi, false, false, false, false>: unscaled, 32-bit columns */
    ORC_PRODUCT_NARROW = 5,         /* spmv_uniform_k<Epi, false, false, true, false>: unscaled, narrow column image */
    ORC_PRODUCT_NARROW_NT = 6,      /* the same with non-temporal matrix loads */
    ORC_PRODUCT_MESH = 7,           /* every persistent-pattern (level-0 mesh) variant */
    ORC_PRODUCT_FAMILIES = 8
};
int orc_debug_product_launches(long long *out, int n_out, int reset);
/* kernel-level timers accumulated inside orc_solver_iterate when enabled: name/ms pairs */
int orc_profile_enable(int on);
int orc_profile_report(char *buf, int64_t buf_len);

/* ---------- synthetic meshes: host-side generator, ORC numbering rules ---------- */
/* Structured hex channel nx*ny*nz cells on [0,lx]x[0,ly]x[0,lz]: interior faces first, then zones
 * INLET(x-min) OUTLET(x-max) PERIODIC_-Z PERIODIC_+Z TOP_WALL BOTTOM_WALL — the zone order of
 * couette_flow_128x64x1.msh; all boundary zones type 3 (wall) like the reference's fixtures.
 * Call with NULL arrays to get sizes. */
int orc_hex_channel_sizes(int64_t nx, int64_t ny, int64_t nz, int64_t *n_cells, int64_t *n_faces, int64_t *n_cell_faces);
int orc_hex_channel_generate(int64_t nx, int64_t ny, int64_t nz, double lx, double ly, double lz,
                             int64_t *face_c0, int64_t *face_c1, int32_t *face_zone, double *face_area,
                             double *face_normal, double *face_centroid, double *cell_centroid, double *cell_volume,
                             int64_t *cell_face_ptr, int64_t *cell_faces);
/* writes the same mesh as an ASCII TGRID .msh that ORC's read_mesh (io.rs:32) accepts */
int orc_hex_channel_write_msh(const char *path, int64_t nx, int64_t ny, int64_t nz, double lx, double ly, double lz);

/* BASELINE config 5 workload: a box of nx x ny x nz blocks (nx >= 20) cut along x into regions of hexahedra, columns of
 * triangular prisms, Kuhn tetrahedra (six per block) and one-block transition layers of pyramids, conforming
 * throughout; about 3 cells per block, matrix rows of 5 / 6 / 7 entries.  Written as a TGRID .msh with triangular and
 * quadrilateral faces in separate zones (the reference's reader cannot parse mixed sections, io.rs:232); zones FLUID,
 * INLET, OUTLET, WALL, PERIODIC_-Z, PERIODIC_+Z and their "_TRI" twins, boundary zones of type 3 (wall). */
int orc_mixed_channel_write_msh(const char *path, int64_t nx, int64_t ny, int64_t nz, double lx, double ly, double lz,
                                int64_t *n_cells, int64_t *n_faces);
/* The same with a region of POLYHEDRAL cells between x = lx/20 and lx/4 (BASELINE config 5: "tet/hex/poly"): blocks
 * alternate between a hexahedron and six pyramids about the block centre, and every pyramid is agglomerated into the
 * hexahedron behind its base — rhombic dodecahedra of 12 planar quadrilateral faces (13 matrix entries per row), with
 * partial cells and left-over pyramids along the region's sides.  Polyhedral CELLS written through triangular and
 * quadrilateral face sections: the subset of TGRID the reference's reader parses correctly (io.rs:232-233 misreads the
 * per-line node count of face_type 0 / 5 sections), no two cells sharing more than one face (discretization.rs:312-322). */
int orc_poly_channel_write_msh(const char *path, int64_t nx, int64_t ny, int64_t nz, double lx, double ly, double lz,
                               int64_t *n_cells, int64_t *n_faces);
/* [r05] The same mesh (polyhedra = 0: orc_mixed_channel_write_msh's, != 0: orc_poly_channel_write_msh's) built IN MEMORY: a handle as from
 * orc_read_mesh whose every array equals, bit for bit, what reading the written file gives (same numbering, zones, geometry code) — without
 * the 580 MB temporary file per rank that BASELINE configs[4] cost in r04.  NULL + *status on failure. */
OrcMeshData *orc_mixed_channel_generate(int64_t nx, int64_t ny, int64_t nz, double lx, double ly, double lz, int polyhedra, int *status);

/* ---------- cut surfaces (new-build extension, orc_types.h ORC_CUT_MAX_POINTS / OrcCutSkip) ----------
 * Plane slices and iso-surfaces as polygons, built on the device from the mesh's node geometry (DESIGN.md §3 "Cut surfaces": every rule
 * of the surface, bit for bit).  Opt-in and read-only: no entry changes a bit of a mesh's cell geometry or of a solver, and a solver that
 * never asks for a cut launches what it launched before.
 *  - orc_mesh_set_nodes: the arrays of orc_mesh_data_nodes.  Checked on the host (n_faces equal to the mesh's, every node id in
 *    [0, n_vertices), at least 3 nodes per face, n_vertices < 2^31), uploaded once with 32-bit ids together with a node -> cell table
 *    (per node the cells with a face through it, ascending ORC id) and kept by the mesh.  A later call is checked in the same way and
 *    changes nothing; one that brings other sizes is refused.  The cells must be closed (every edge of a cell in exactly two of its
 *    faces): otherwise a cell may emit fewer points than it was counted for, and the points it leaves are zero with key (0, 0) and join
 *    the polygon before them — within bounds, uncounted.  A partitioned mesh is refused.
 *  - orc_mesh_node_average: phi_v = (sum_c w_c phi_c) / (sum_c w_c), w_c = 1 / |x_c - x_v| over the node's cells in ascending ORC id;
 *    cell values only, also at boundary nodes.
 *  - orc_cut_plane: d_v = ((x - o.x) n.x + (y - o.y) n.y) + (z - o.z) n.z; the normal finite and not zero, any length.
 *    orc_cut_node_level: d_v = node_values[v] - level.  orc_cut_cell_field: orc_mesh_node_average of cell_values (ORC order), then the
 *    level.  orc_solver_cut_field: the same on the solver's own field (field_bit = 1u << one OrcProbeField) without leaving the device.
 *    All four return NULL + *status on failure.  Destroy a cut before its mesh.
 *  - orc_cut_sizes / orc_cut_get: polygons P, points NP, the cells skipped per OrcCutSkip; poly_ptr [P + 1] into the points, the owner
 *    cell (ORC id) per polygon, points [3 NP] point-major, the key (lo, hi node id of the cut edge) per point, the area vector [3 P]
 *    polygon-major.  Every output may be NULL; P = 0 is legal.  Polygons ascend in ORC cell id whatever the mesh's internal numbering.
 *  - orc_solver_sample_cut: the fields of field_mask as orc_solver_sample_probes; ORC_PROBE_CELL: one value per polygon (the owner's),
 *    field k at out[k * P + p]; ORC_PROBE_LINEAR: one per polygon vertex through the owner's gradient, field k at out[k * NP + i] - the
 *    bits orc_solver_sample_probes gives for that cell and point.  Refusals and error codes are those of orc_solver_sample_probes.
 *  - orc_cut_sample_cells: the CELL gather for n_fields host arrays of n_cells values each in ORC order, field k at out[k * P + p].
 *  - orc_cut_limits: ORC_CUT_MAX_POINTS and the entries one workgroup of the scan takes.  Needs no device.
 *  - orc_bench_cut: HIP-event average ms over `reps` of avg_ms[0] the node average of a cell field, [1] the classify pass with its
 *    face pass, [2] the scan, [3] the emit (points, polygon table, area vectors) of the plane (origin, normal).
 *  - orc_write_vtu_polygons: host only; VTK_POLYGON cells over poly_nodes [poly_ptr[n_polys]] (ids into points) with cell data (per
 *    polygon) and point data (per point; every point must be used), in the conventions of orc_write_vtu_faces.
 * Every compute entry looks for a device first (ORC_ERR_NO_DEVICE without one).  Refused with ORC_ERR_BAD_ARGUMENT, mesh and solver
 * unchanged: a null handle or array; a zero or non-finite normal, a non-finite origin or level; a cut before orc_mesh_set_nodes; a cut of
 * another mesh handed to a solver; a field_mask of 0 or with unknown bits, a field_bit that is not exactly one known bit; ORC_PROBE_PHI
 * without the scalar arm; a partitioned mesh. */
typedef struct OrcCut OrcCut;
int orc_mesh_set_nodes(OrcMesh *m, int64_t n_vertices, const double *vertices /*[3V]*/, int64_t n_faces, const int64_t *face_node_ptr /*[F+1]*/,
                       const int64_t *face_nodes);
int orc_mesh_node_average(OrcMesh *m, const double *cell_values /*[n_cells] ORC order*/, double *node_values /*[V]*/);
OrcCut *orc_cut_plane(OrcMesh *m, const double origin[3], const double normal[3], int *status);
OrcCut *orc_cut_node_level(OrcMesh *m, const double *node_values /*[V]*/, double level, int *status);
OrcCut *orc_cut_cell_field(OrcMesh *m, const double *cell_values /*[n_cells] ORC order*/, double level, int *status);
OrcCut *orc_solver_cut_field(OrcSolver *s, uint32_t field_bit, double level, int *status);
void orc_cut_destroy(OrcCut *cut);
int orc_cut_sizes(const OrcCut *cut, int64_t *n_polygons, int64_t *n_points, int64_t *n_skipped_nonfinite, int64_t *n_skipped_overflow);
int orc_cut_get(const OrcCut *cut, int64_t *poly_ptr /*[P+1]*/, int64_t *cell /*[P]*/, double *points /*[3 NP]*/, int64_t *key_lo /*[NP]*/,
                int64_t *key_hi /*[NP]*/, double *area_vector /*[3P]*/);
int orc_cut_limits(int32_t *max_points, int32_t *scan_chunk);
int orc_solver_sample_cut(OrcSolver *s, const OrcCut *cut, uint32_t field_mask, int32_t interpolation, double *out);
int orc_cut_sample_cells(const OrcCut *cut, int32_t n_fields, const double *fields /*[n_fields][n_cells] ORC order*/, double *out /*[n_fields][P]*/);
int orc_bench_cut(OrcMesh *m, const double *cell_values /*[n_cells] ORC order*/, const double origin[3], const double normal[3], int reps,
                  double avg_ms[4]);
int orc_write_vtu_polygons(const char *path, int64_t n_points, const double *points /*[3 n_points]*/, int64_t n_polys, const int64_t *poly_ptr /*[n_polys + 1]*/,
                           const int64_t *poly_nodes, int32_t n_cell_arrays, const char *const *cell_names, const int32_t *cell_components,
                           const double *const *cell_data, int32_t n_point_arrays, const char *const *point_names, const int32_t *point_components,
                           const double *const *point_data, int32_t encoding);

/* ---------- multi-GPU (one process per GPU, RCCL over xGMI) ---------- */
#define ORC_COMM_ID_BYTES 128
int orc_comm_get_unique_id(unsigned char id[ORC_COMM_ID_BYTES]);          /* rank 0, then broadcast by the host launcher */
int orc_comm_init(const unsigned char id[ORC_COMM_ID_BYTES], int rank, int world_size);
int orc_comm_finalize(void);
/* One-GPU self-check of the RCCL data path (single-rank communicator, rank 0 as its own neighbour): halo exchange of
 * two fields, sum/max all-reduce, status agreement.  Needs an uninitialised communicator. */
int orc_comm_selftest(void);
/* Debug/test: a persistent single-rank RCCL communicator posing as a two-rank world whose only peer is this rank.  A
 * partitioned mesh whose halo plan names peer 0 everywhere then runs the whole partitioned path (RCCL halos, all-reduces,
 * status agreement, the products that overlap their halo exchange) on ONE GPU; the run is self-coupled (ghost values are
 * the rank's own cells), so it is compared with itself under other switches.  Ended by orc_comm_finalize. */
int orc_comm_init_self_loop(void);
/* Debug transport for tests where ranks share one GPU (RCCL refuses duplicate devices): halo exchange and all-reduce
 * are staged through host memory and carried by the caller's callbacks (e.g. torch.distributed/gloo).
 * exchange_fn: void(int n_peers, const int* peers, const double* send, const int64_t* send_off, const int64_t* send_cnt,
 *                   double* recv, const int64_t* recv_off, const int64_t* recv_cnt, void* user)
 * allreduce_fn: void(double* values, int n, int op (0 sum, 1 max), void* user).  Call orc_comm_init(NULL, rank, world) first. */
int orc_comm_set_host_transport(void *exchange_fn, void *allreduce_fn, void *user);

#ifdef __cplusplus
}
#endif
#endif /* ORC_AMD_H */
