"""Loader for liborc_amd.so (hand-written HIP for gfx950 behind the C ABI of include/orc_amd.h).

There is no CPU fallback anywhere in this package: if the shared library is missing, or no HIP
device is visible when a compute entry is called, the call fails loudly.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liborc_amd.so")


class OrcError(RuntimeError):
    def __init__(self, status, text, detail=""):
        super().__init__("%s (status %d)%s" % (text, status, (": " + detail) if detail else ""))
        self.status = status


def build(force=False):
    """hipcc --offload-arch=gfx950 build of every HIP translation unit (csrc/Makefile)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OrcError(12, "liborc_amd.so is not built", "run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.orc_status_string.restype = C.c_char_p
        L.orc_last_error.restype = C.c_char_p
        for name in ("orc_mesh_create", "orc_solver_create"):
            if hasattr(L, name):
                getattr(L, name).restype = C.c_void_p
        for name in ("orc_mesh_n_cells", "orc_mesh_nnz", "orc_last_jacobi_sweeps"):
            if hasattr(L, name):
                getattr(L, name).restype = C.c_int64
        # entries added with the CG arm and the p' solver override: full signatures
        if hasattr(L, "orc_last_cg_stats"):
            L.orc_last_cg_stats.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
            L.orc_last_cg_stats.restype = C.c_int
        if hasattr(L, "orc_solver_set_pressure_solver"):
            L.orc_solver_set_pressure_solver.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_pressure_solver.restype = C.c_int
            L.orc_solver_get_pressure_solver.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
            L.orc_solver_get_pressure_solver.restype = C.c_int
            L.orc_solver_debug_pressure_hierarchies.argtypes = [C.c_void_p]
            L.orc_solver_debug_pressure_hierarchies.restype = C.c_longlong
        # surface reports (orc_amd.h "surface reports"): full signatures
        if hasattr(L, "orc_solver_surface_report"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_solver_surface_report.argtypes = [C.c_void_p, _f64, _f64]
            L.orc_solver_surface_report.restype = C.c_int
            L.orc_surface_integrals.argtypes = [C.c_void_p, _f64, _f64, _f64, _f64, C.c_double, C.c_double, _f64, _f64]
            L.orc_surface_integrals.restype = C.c_int
            L.orc_mesh_boundary_index.argtypes = [C.c_void_p, _i64, _i32, _i64, _i32]
            L.orc_mesh_boundary_index.restype = C.c_int
        # derived fields, boundary-face maps and the VTU writers (orc_amd.h "derived fields, boundary-face maps and VTU export")
        if hasattr(L, "orc_solver_derived_fields"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_solver_derived_fields.argtypes = [C.c_void_p, C.c_uint32, _f64]
            L.orc_solver_derived_fields.restype = C.c_int
            L.orc_derived_fields.argtypes = [C.c_void_p, _f64, _f64, _f64, C.c_void_p, C.c_uint32, _f64]
            L.orc_derived_fields.restype = C.c_int
            L.orc_solver_boundary_fields.argtypes = [C.c_void_p, C.c_uint32, _f64]
            L.orc_solver_boundary_fields.restype = C.c_int
            L.orc_boundary_fields.argtypes = [C.c_void_p, _f64, _f64, _f64, _f64, C.c_double, C.c_double, C.c_uint32, _f64]
            L.orc_boundary_fields.restype = C.c_int
            _tables = [C.c_int32, C.POINTER(C.c_char_p), _i32, C.POINTER(_f64), C.c_int32]
            L.orc_write_vtu.argtypes = [C.c_char_p, C.c_int64, _f64, C.c_int64, _i64, _i64, _i64, _i64] + _tables
            L.orc_write_vtu.restype = C.c_int
            L.orc_write_vtu_faces.argtypes = [C.c_char_p, C.c_int64, _f64, C.c_int64, _i64, _i64, _i64] + _tables
            L.orc_write_vtu_faces.restype = C.c_int
        # residual monitors and convergence-controlled runs (orc_amd.h "residual monitors"): full signatures
        if hasattr(L, "orc_solver_set_monitors"):
            _f64, _u64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
            L.orc_solver_set_monitors.argtypes = [C.c_void_p, C.c_int32]
            L.orc_solver_set_monitors.restype = C.c_int
            L.orc_solver_residual_count.argtypes = [C.c_void_p]
            L.orc_solver_residual_count.restype = C.c_int64
            L.orc_solver_residual_history.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, _f64]
            L.orc_solver_residual_history.restype = C.c_int
            L.orc_convergence_check.argtypes = [C.c_void_p, _f64, _i32]
            L.orc_convergence_check.restype = C.c_int
            L.orc_solver_iterate_until.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, _f64, _u64, _i32]
            L.orc_solver_iterate_until.restype = C.c_int
            L.orc_solve_steady_converged.argtypes = [C.c_void_p, _f64, _f64, _f64, _f64, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                                     C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, _u64, _i32, _f64]
            L.orc_solve_steady_converged.restype = C.c_int
            L.orc_solver_get_pressure_rhs.argtypes = [C.c_void_p, _f64]
            L.orc_solver_get_pressure_rhs.restype = C.c_int
        # variable viscosity (orc_amd.h "variable viscosity"): full signatures
        if hasattr(L, "orc_solver_set_viscosity"):
            _f64 = C.POINTER(C.c_double)
            L.orc_viscosity_default.argtypes = [C.c_void_p]
            L.orc_viscosity_default.restype = None
            L.orc_solver_set_viscosity.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_viscosity.restype = C.c_int
            L.orc_solver_set_viscosity_field.argtypes = [C.c_void_p, _f64]
            L.orc_solver_set_viscosity_field.restype = C.c_int
            L.orc_solver_get_viscosity.argtypes = [C.c_void_p, _f64]
            L.orc_solver_get_viscosity.restype = C.c_int
            L.orc_solver_evaluate_viscosity.argtypes = [C.c_void_p, _f64, _f64]
            L.orc_solver_evaluate_viscosity.restype = C.c_int
            L.orc_solver_get_diffusion.argtypes = [C.c_void_p, _f64, _f64, _f64, _f64]
            L.orc_solver_get_diffusion.restype = C.c_int
            L.orc_bench_viscosity.argtypes = [C.c_void_p, C.c_int, _f64]
            L.orc_bench_viscosity.restype = C.c_int
        # variable scalar diffusivity (orc_amd.h "variable scalar diffusivity"): full signatures
        if hasattr(L, "orc_solver_set_scalar_diffusivity"):
            _f64 = C.POINTER(C.c_double)
            L.orc_scalar_diffusivity_default.argtypes = [C.c_void_p]
            L.orc_scalar_diffusivity_default.restype = None
            L.orc_solver_set_scalar_diffusivity.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_scalar_diffusivity.restype = C.c_int
            L.orc_solver_set_scalar_diffusivity_field.argtypes = [C.c_void_p, _f64]
            L.orc_solver_set_scalar_diffusivity_field.restype = C.c_int
            L.orc_solver_get_scalar_diffusivity.argtypes = [C.c_void_p, _f64]
            L.orc_solver_get_scalar_diffusivity.restype = C.c_int
            L.orc_bench_scalar_diffusivity.argtypes = [C.c_void_p, C.c_int, _f64]
            L.orc_bench_scalar_diffusivity.restype = C.c_int
        # wall distance and wall damping (orc_amd.h "wall distance and wall damping"): full signatures
        if hasattr(L, "orc_mesh_wall_distance"):
            _f64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
            L.orc_mesh_wall_distance.argtypes = [C.c_void_p, _i32, _f64]
            L.orc_mesh_wall_distance.restype = C.c_int
            L.orc_debug_wall_distance.argtypes = [C.c_void_p, _i32, C.c_int, _f64]
            L.orc_debug_wall_distance.restype = C.c_int
            L.orc_debug_wall_search.argtypes = [C.POINTER(C.c_longlong), C.c_int]
            L.orc_debug_wall_search.restype = C.c_int
            L.orc_bench_wall_distance.argtypes = [C.c_void_p, C.c_int, C.c_int, _f64]
            L.orc_bench_wall_distance.restype = C.c_int
            L.orc_wall_damping_default.argtypes = [C.c_void_p]
            L.orc_wall_damping_default.restype = None
            L.orc_solver_set_wall_damping.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_wall_damping.restype = C.c_int
            L.orc_solver_get_wall_damping.argtypes = [C.c_void_p, C.c_void_p, _i32]
            L.orc_solver_get_wall_damping.restype = C.c_int
        # running time statistics (orc_amd.h "running time statistics"): full signatures
        if hasattr(L, "orc_solver_set_time_statistics"):
            _f64, _u64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_time_statistics_default.argtypes = [C.c_void_p]
            L.orc_time_statistics_default.restype = None
            L.orc_solver_set_time_statistics.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_time_statistics.restype = C.c_int
            L.orc_solver_sample_statistics.argtypes = [C.c_void_p, C.c_double]
            L.orc_solver_sample_statistics.restype = C.c_int
            L.orc_solver_reset_statistics.argtypes = [C.c_void_p]
            L.orc_solver_reset_statistics.restype = C.c_int
            L.orc_solver_statistics_info.argtypes = [C.c_void_p, _u64, _f64, _i32, _i64]
            L.orc_solver_statistics_info.restype = C.c_int
            L.orc_solver_get_statistics.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, _f64]
            L.orc_solver_get_statistics.restype = C.c_int
            L.orc_solver_set_statistics_state.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_uint32, _f64, _f64]
            L.orc_solver_set_statistics_state.restype = C.c_int
            L.orc_solver_get_boundary_statistics.argtypes = [C.c_void_p, _f64]
            L.orc_solver_get_boundary_statistics.restype = C.c_int
            L.orc_bench_time_statistics.argtypes = [C.c_void_p, C.c_int, _f64]
            L.orc_bench_time_statistics.restype = C.c_int
        # point probes (orc_amd.h "point probes"): full signatures
        if hasattr(L, "orc_probes_create"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_probes_create.argtypes = [C.c_void_p, C.c_int64, _f64, C.POINTER(C.c_int)]
            L.orc_probes_create.restype = C.c_void_p
            L.orc_debug_probes_locate.argtypes = [C.c_void_p, C.c_int64, _f64, C.c_int, C.c_int, C.POINTER(C.c_int)]
            L.orc_debug_probes_locate.restype = C.c_void_p
            L.orc_probes_destroy.argtypes = [C.c_void_p]
            L.orc_probes_destroy.restype = None
            L.orc_probes_count.argtypes = [C.c_void_p]
            L.orc_probes_count.restype = C.c_int64
            L.orc_probes_get.argtypes = [C.c_void_p, _i64, _i32, _i32, _i32, _f64]
            L.orc_probes_get.restype = C.c_int
            L.orc_solver_sample_probes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, _f64]
            L.orc_solver_sample_probes.restype = C.c_int
            L.orc_solver_set_probe_history.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64]
            L.orc_solver_set_probe_history.restype = C.c_int
            L.orc_solver_record_probes.argtypes = [C.c_void_p, C.c_double]
            L.orc_solver_record_probes.restype = C.c_int
            L.orc_solver_probe_history_count.argtypes = [C.c_void_p]
            L.orc_solver_probe_history_count.restype = C.c_int64
            L.orc_solver_probe_history.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, _f64, _f64]
            L.orc_solver_probe_history.restype = C.c_int
            L.orc_debug_probe_search.argtypes = [C.POINTER(C.c_longlong), C.c_int]
            L.orc_debug_probe_search.restype = C.c_int
            L.orc_bench_probe_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _f64]
            L.orc_bench_probe_locate.restype = C.c_int
        # tracer particles (orc_amd.h "tracer particles"): full signatures
        if hasattr(L, "orc_tracers_create"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_tracer_settings_default.argtypes = [C.c_void_p]
            L.orc_tracer_settings_default.restype = None
            L.orc_tracers_create.argtypes = [C.c_void_p, C.c_int64, _f64, C.POINTER(C.c_int)]
            L.orc_tracers_create.restype = C.c_void_p
            L.orc_tracers_destroy.argtypes = [C.c_void_p]
            L.orc_tracers_destroy.restype = None
            L.orc_tracers_count.argtypes = [C.c_void_p]
            L.orc_tracers_count.restype = C.c_int64
            L.orc_tracers_get.argtypes = [C.c_void_p, _f64, _i64, _i32, _i32, _f64, _i64]
            L.orc_tracers_get.restype = C.c_int
            L.orc_solver_advect_tracers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, _f64, _i32]
            L.orc_solver_advect_tracers.restype = C.c_int
            L.orc_solver_sample_tracers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, _f64]
            L.orc_solver_sample_tracers.restype = C.c_int
            L.orc_solver_set_tracer_tracking.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.orc_solver_set_tracer_tracking.restype = C.c_int
            L.orc_write_vtu_lines.argtypes = [C.c_char_p, C.c_int64, _i64, _f64, C.c_int32, C.POINTER(C.c_char_p), _i32, C.POINTER(_f64), C.c_int32]
            L.orc_write_vtu_lines.restype = C.c_int
            L.orc_bench_tracers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, _f64]
            L.orc_bench_tracers.restype = C.c_int
        # volume reports (orc_amd.h "volume reports"): full signatures
        if hasattr(L, "orc_cell_groups_create"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_cell_groups_create.argtypes = [C.c_void_p, C.c_int32, _i32, C.POINTER(C.c_int)]
            L.orc_cell_groups_create.restype = C.c_void_p
            L.orc_cell_groups_destroy.argtypes = [C.c_void_p]
            L.orc_cell_groups_destroy.restype = None
            L.orc_cell_groups_count.argtypes = [C.c_void_p]
            L.orc_cell_groups_count.restype = C.c_int32
            L.orc_cell_groups_get.argtypes = [C.c_void_p, _i64, _i64, _i32]
            L.orc_cell_groups_get.restype = C.c_int
            L.orc_group_limits.argtypes = [_i32, _i32, _i32, _i32]
            L.orc_group_limits.restype = C.c_int
            L.orc_solver_group_report.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, _f64, _f64, _i64]
            L.orc_solver_group_report.restype = C.c_int
            L.orc_group_integrals.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, _f64, C.c_int32, _f64, _f64, _i64]
            L.orc_group_integrals.restype = C.c_int
            L.orc_solver_group_statistics.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, _f64, _f64, _i64]
            L.orc_solver_group_statistics.restype = C.c_int
            L.orc_solver_set_group_history.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64]
            L.orc_solver_set_group_history.restype = C.c_int
            L.orc_solver_record_groups.argtypes = [C.c_void_p, C.c_double]
            L.orc_solver_record_groups.restype = C.c_int
            L.orc_solver_group_history_count.argtypes = [C.c_void_p]
            L.orc_solver_group_history_count.restype = C.c_int64
            L.orc_solver_group_history.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, _f64, _f64, _f64, _i64]
            L.orc_solver_group_history.restype = C.c_int
            L.orc_bench_group_report.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int, _f64]
            L.orc_bench_group_report.restype = C.c_int
        # adaptive time stepping (orc_amd.h "adaptive time stepping"): full signatures
        if hasattr(L, "orc_solver_courant"):
            _f64, _i64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
            L.orc_time_step_control_default.argtypes = [C.c_void_p]
            L.orc_time_step_control_default.restype = None
            L.orc_time_step_next.argtypes = [C.c_void_p, C.c_double, C.c_double, _f64]
            L.orc_time_step_next.restype = C.c_int
            L.orc_solver_courant.argtypes = [C.c_void_p, _f64, _i64, _f64]
            L.orc_solver_courant.restype = C.c_int
            L.orc_solver_set_time_step.argtypes = [C.c_void_p, C.c_double]
            L.orc_solver_set_time_step.restype = C.c_int
            L.orc_solver_set_time_step_control.argtypes = [C.c_void_p, C.c_void_p]
            L.orc_solver_set_time_step_control.restype = C.c_int
            L.orc_solver_get_time_state.argtypes = [C.c_void_p, _f64, _f64, _f64, _f64]
            L.orc_solver_get_time_state.restype = C.c_int
            L.orc_solver_set_time_state.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
            L.orc_solver_set_time_state.restype = C.c_int
            L.orc_solver_time_step_count.argtypes = [C.c_void_p]
            L.orc_solver_time_step_count.restype = C.c_int64
            L.orc_solver_time_step_history.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, _f64]
            L.orc_solver_time_step_history.restype = C.c_int
            L.orc_bench_courant.argtypes = [C.c_void_p, C.c_int, _f64]
            L.orc_bench_courant.restype = C.c_int
            L.orc_bench_derived_rate.argtypes = [C.c_void_p, C.c_int, _f64]
            L.orc_bench_derived_rate.restype = C.c_int
        # cut surfaces (orc_amd.h "cut surfaces"): full signatures
        if hasattr(L, "orc_cut_plane"):
            _f64, _i64, _i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            L.orc_mesh_set_nodes.argtypes = [C.c_void_p, C.c_int64, _f64, C.c_int64, _i64, _i64]
            L.orc_mesh_set_nodes.restype = C.c_int
            L.orc_mesh_node_average.argtypes = [C.c_void_p, _f64, _f64]
            L.orc_mesh_node_average.restype = C.c_int
            L.orc_cut_plane.argtypes = [C.c_void_p, _f64, _f64, C.POINTER(C.c_int)]
            L.orc_cut_plane.restype = C.c_void_p
            L.orc_cut_node_level.argtypes = [C.c_void_p, _f64, C.c_double, C.POINTER(C.c_int)]
            L.orc_cut_node_level.restype = C.c_void_p
            L.orc_cut_cell_field.argtypes = [C.c_void_p, _f64, C.c_double, C.POINTER(C.c_int)]
            L.orc_cut_cell_field.restype = C.c_void_p
            L.orc_solver_cut_field.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.POINTER(C.c_int)]
            L.orc_solver_cut_field.restype = C.c_void_p
            L.orc_cut_destroy.argtypes = [C.c_void_p]
            L.orc_cut_destroy.restype = None
            L.orc_cut_sizes.argtypes = [C.c_void_p, _i64, _i64, _i64, _i64]
            L.orc_cut_sizes.restype = C.c_int
            L.orc_cut_get.argtypes = [C.c_void_p, _i64, _i64, _f64, _i64, _i64, _f64]
            L.orc_cut_get.restype = C.c_int
            L.orc_cut_limits.argtypes = [_i32, _i32]
            L.orc_cut_limits.restype = C.c_int
            L.orc_solver_sample_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, _f64]
            L.orc_solver_sample_cut.restype = C.c_int
            L.orc_cut_sample_cells.argtypes = [C.c_void_p, C.c_int32, _f64, _f64]
            L.orc_cut_sample_cells.restype = C.c_int
            L.orc_bench_cut.argtypes = [C.c_void_p, _f64, _f64, _f64, C.c_int, _f64]
            L.orc_bench_cut.restype = C.c_int
            _tables = [C.c_int32, C.POINTER(C.c_char_p), _i32, C.POINTER(_f64)]
            L.orc_write_vtu_polygons.argtypes = [C.c_char_p, C.c_int64, _f64, C.c_int64, _i64, _i64] + _tables + _tables + [C.c_int32]
            L.orc_write_vtu_polygons.restype = C.c_int
        # the set-up's statistics (orc_amd.h "orc_debug_amg_setup_stats")
        if hasattr(L, "orc_debug_amg_setup_stats"):
            L.orc_debug_amg_setup_stats.argtypes = [C.POINTER(C.c_longlong), C.c_int]
            L.orc_debug_amg_setup_stats.restype = C.c_int
        _lib = L
    return _lib


def last_error():
    """orc_last_error(): the library's text for the last failure (or note) of this thread's context"""
    return lib().orc_last_error().decode()


def check(status):
    if status != 0:
        L = lib()
        raise OrcError(status, L.orc_status_string(C.c_int(status)).decode(), L.orc_last_error().decode())


def device_count():
    return lib().orc_device_count()


def init(device=-1):
    check(lib().orc_init(C.c_int(device)))
