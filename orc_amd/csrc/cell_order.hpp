// cell_order.hpp — the boundary between the caller's ORC cell order and the mesh's internal one (host only).
//
// orc_mesh_create_reordered renumbers the cells inside the library: internal cell c holds ORC cell g[c], g = OrcMesh::h_global_ids
// (empty = identity: every other mesh).  This unit is the one place that reads g; every entry that takes or returns a per-cell array
// goes through it.  The order each entry of the C ABI speaks:
//   ORC       orc_solver_set_fields / get_fields, orc_solve_steady / _converged / _transient, orc_solver_set_time_levels,
//             orc_initialize_pressure_field / _flow / _velocity_field / _flow_new, orc_solver_set_scalar_field / get_scalar_field /
//             set_scalar_source / set_scalar_levels, orc_solver_set_viscosity_field / get_viscosity / evaluate_viscosity,
//             orc_mesh_wall_distance, orc_debug_wall_distance, orc_derived_fields, orc_solver_derived_fields, the fields into
//             orc_surface_integrals and orc_boundary_fields, orc_solver_get_statistics / set_statistics_state, and the cell ids of
//             orc_probes_get and orc_tracers_get, the labels into orc_cell_groups_create, the cell ids of orc_cell_groups_get, the
//             fields into orc_group_integrals and the `where` cells of every group report (orc_solver_group_report / _statistics /
//             _history, orc_group_integrals), the cell and the per-cell rates of orc_solver_courant, the cell values into orc_mesh_node_average / orc_cut_cell_field /
//             orc_cut_sample_cells and the owner cells of orc_cut_get
//   internalorc_mesh_matrix_pattern, the matrix values and right-hand sides of orc_solver_assemble_momentum / _pressure / _scalar,
//             orc_solver_get_diffusion, orc_solver_get_pressure_rhs, orc_build_momentum_diffusion_matrix, orc_initialize_momentum_matrix
//             (orc_mesh_cell_order reports g)
//   mixed     fields in in ORC order, per-cell results out in internal order: orc_calculate_gradients,
//             orc_build_momentum_advection_matrices, orc_build_pressure_correction_matrices
#pragma once
#include "assembly.hpp"

namespace orc {

// g itself (empty = identity): orc_mesh_cell_order copies it out, probes.hip uploads it for its tie-break
const std::vector<int64_t> &cell_order_ids(const OrcMesh &m);
// the ORC id of internal cell `internal`
int64_t orc_cell_id(const OrcMesh &m, int32_t internal);
// the inverse of g: the internal cell of every ORC id (empty = identity): groups.hip stores its ORC-ordered lists through it
std::vector<int32_t> internal_cell_ids(const OrcMesh &m);
// `fields` arrays of n = m.n_cells doubles, one after the other.  upload: dst[q n + c] = src_orc[q n + g[c]] (dst grows if need be);
// download: dst_orc[q n + g[c]] = dev[q n + c].  Both copy on ctx().stream and return with it synchronised, as DevBuf::upload /
// download do; the identity is a straight copy without a temporary.
int upload_cells(const OrcMesh &m, const double *src_orc, DevBuf<double> &dst, int fields = 1);
int download_cells(const OrcMesh &m, const double *dev, double *dst_orc, int fields = 1);

}  // namespace orc
