// assembly.hpp — device mesh (SoA image of mesh::Mesh) and the SIMPLE-iteration state.
#pragma once
#include <memory>

#include "linalg.hpp"
#include "postproc_state.hpp"

namespace orc {

// Device pointers of the mesh, passed to kernels by value.  AoS `Vec<Face>` / `Vec<Cell>` with heap
// adjacency (mesh.rs:140-187) becomes structure-of-arrays so face- and cell-parallel kernels read
// coalesced; the zone HashMap lookup (solver.rs:1113) becomes a per-face zone index into three
// tiny tables.
struct MeshDev {
    int64_t n_cells = 0, n_faces = 0;  // n_cells = owned + ghost cells (array length / SoA stride)
    int64_t n_own = 0;                 // cells this rank assembles and solves: [0, n_own)
    int32_t n_zones = 0;
    const int32_t *c0 = nullptr, *c1 = nullptr, *fzone = nullptr;
    const double *area = nullptr, *nx = nullptr, *ny = nullptr, *nz = nullptr;
    const double *fcx = nullptr, *fcy = nullptr, *fcz = nullptr;
    const double *ccx = nullptr, *ccy = nullptr, *ccz = nullptr, *vol = nullptr;
    const int32_t *cfp = nullptr;    // [n+1] cell -> face list (Cell.face_indices, ascending face id)
    const int32_t *cf = nullptr;     // face ids
    const int32_t *cfpos = nullptr;  // SELL element offset of A(cell, neighbour) for that face, -1 on boundary faces
    const int32_t *ztype = nullptr;  // OrcFaceConditionType per zone
    const double *zscal = nullptr;   // FaceZone.scalar_value
    const double *zvec = nullptr;    // FaceZone.vector_value [3Z]
};

// The boundary faces of owned cells grouped by zone (surface.hip): built on the device at a mesh's first surface report and
// never again — the face -> zone map of a mesh is immutable; zone types and values are read from ztype / zscal / zvec at
// report time.  The report's partial sums, output and status word live here too, so that a report allocates nothing.
struct SurfaceIndex {
    int64_t n_bfaces = 0, n_chunks = 0, builds = 0;
    std::vector<int64_t> h_zone_ptr;       // [Z + 1] into bface
    DevBuf<int32_t> bface;                 // face ids, ascending inside a zone
    DevBuf<int32_t> chunk;                 // [n_chunks][4] = {zone, begin, end, 0}: <= kSurfaceChunk faces of ONE zone each
    DevBuf<int32_t> zone_chunk_ptr;        // [Z + 1] into the chunk table
    DevBuf<double> partials, out;          // [n_chunks][16], [Z][16]
    DevBuf<int> status;
};

// The wall table of one wall mask and the distance field searched from it (wall_distance.hip): built at a mesh's first use, kept
// until the wall-ness of a zone changes (orc_mesh_update_zones).  The table holds the wall faces of ALL ranks, SoA, this rank's
// ascending in face id; tile t covers the entries [t * kWallTile, (t + 1) * kWallTile) and carries a bounding sphere of their centroids.
struct WallDistance {
    std::vector<int32_t> mask;   // [Z] the resolved mask the table was built for
    bool from_types = false;     // the mask is the default one (type WALL): a change of zone types can invalidate it
    int64_t n_wall = 0, n_tiles = 0;
    DevBuf<double> table;        // [6][n_wall]: centroid x, y, z, normal x, y, z
    DevBuf<double> tiles;        // [4][n_tiles]: sphere centre x, y, z and (widened) radius
    DevBuf<double> d;            // [n_cells] internal cell order, ghost entries 0
    bool searched = false;       // d holds the field
};

// What the point search of probes.hip keeps per mesh, built at the first orc_probes_create: tile t covers the owned cells
// [t * kProbeTile, (t + 1) * kProbeTile) of the internal numbering and carries a bounding sphere of their centroids; the cell geometry
// of a mesh never changes, so the spheres live as long as the mesh.
struct ProbeTiles {
    int64_t n_tiles = 0;
    DevBuf<double> tiles;     // [4][n_tiles]: sphere centre x, y, z and (widened) radius
    DevBuf<int32_t> orc_id;   // [n_cells] ORC id of every internal cell; empty when the numbering is ORC's own
};

// The node geometry of a mesh (cut.hip, orc_mesh_set_nodes): the device mesh itself holds no vertex, so a cut needs the vertices, the
// faces' node cycles and, for the node average of a cell field, the cells around every node.  Uploaded once, kept as long as the mesh.
struct CutNodes {
    int64_t n_vertices = 0, n_face_nodes = 0, n_node_cells = 0;
    DevBuf<double> vx, vy, vz;          // [V]
    DevBuf<int32_t> fnp, fn;            // [F + 1] into fn; the node cycle of every face
    DevBuf<int32_t> ncp, nc;            // [V + 1] into nc; per node the cells (internal numbering) with a face through it, ascending ORC id
    DevBuf<int32_t> orc2int, int2orc;   // [n_cells] each; both empty when the numbering is ORC's own
};

#ifdef __HIPCC__
// the TVD limiters of settings::MomentumDiscretization (lib.rs:107-118): momentum_k and the scalar arm's scalar_face_k
__device__ __forceinline__ double psi_eval(int momentum, double r) {
    switch (momentum) {
    case ORC_MOMENTUM_TVD_UD: return 0.;
    case ORC_MOMENTUM_TVD_CD1: return 1.;
    case ORC_MOMENTUM_TVD_LUD: return r;
    case ORC_MOMENTUM_TVD_QUICK: return (3. + r) / 4.;
    default: {  // UMIST; f64::min / max ignore NaN like fmin / fmax
        double acc = INFINITY;
        acc = fmin(acc, 2. * r);
        acc = fmin(acc, (1. + 3. * r) / 4.);
        acc = fmin(acc, (3. + r) / 4.);
        acc = fmin(acc, 2.);
        return fmax(0., acc);
    }
    }
}
#endif

}  // namespace orc

struct OrcMesh {
    int64_t n_cells = 0, n_faces = 0, n_cell_faces = 0;
    int64_t n_own = 0;         // == n_cells on a single GPU
    int64_t n_global = 0;      // cells of the whole mesh (report averages, solver.rs:206-208)
    orc::HaloPlan halo;        // empty on a single GPU
    int32_t n_zones = 0;
    orc::DevBuf<int32_t> c0, c1, fzone, cfp, cf, cfpos, ztype;
    orc::DevBuf<double> area, nx, ny, nz, fcx, fcy, fcz, ccx, ccy, ccz, vol, zscal, zvec;
    orc::SellMatrix pat;  // shared sparsity of a_di, a_u, a_v, a_w, A_p
    std::vector<int64_t> h_row_ptr, h_col;  // the same pattern in CSR (ORC order) for the C ABI
    std::vector<int64_t> h_global_ids;      // orc_mesh_create_reordered: ORC index of every internal cell (empty = identity);
                                            // read by cell_order.hpp alone, which every per-cell array of the C ABI goes through
    std::unique_ptr<orc::SurfaceIndex> surface;  // null until the first surface report (surface.hip)
    std::unique_ptr<orc::WallDistance> wall;     // null until the first wall distance (wall_distance.hip)
    std::unique_ptr<orc::ProbeTiles> probe_tiles;  // null until the first probe set (probes.hip)
    std::unique_ptr<orc::CutNodes> nodes;          // null until orc_mesh_set_nodes (cut.hip)
    orc::MeshDev dev() const;
};

namespace orc {

struct Fields {
    double *u, *v, *w, *p;
};

// Everything solve_steady allocates before its loop (solver.rs:39-49) plus per-iteration scratch.
struct SolverState {
    OrcMesh *mesh = nullptr;
    OrcSettings settings;
    double rho = 0., mu = 0.;
    int64_t n = 0;      // local array length (owned + ghost)
    int64_t n_own = 0;  // rows
    DevBuf<double> u, v, w, p, p_prime;
    DevBuf<double> a_di, a_u, a_v, a_w, a_p;            // SELL value arrays (mesh pattern)
    DevBuf<double> b_u_di, b_v_di, b_w_di, b_u, b_v, b_w, b_p;
    DevBuf<double> du, dv, dw;                           // a_{u,v,w}.get(i,i): what Rhie-Chow reads
    // frozen_diagonals = 0 (the reference's in-place reads): last iteration's diagonals, per-cell Peclet terms and
    // the level schedule of the cell order (level_cells[level_ptr[l] .. level_ptr[l+1]) = cells of level l, ascending)
    DevBuf<double> du_old, dv_old, dw_old, pe;
    DevBuf<int32_t> level_cells;
    std::vector<int64_t> level_ptr;
    DevBuf<double> gp;                                   // grad p  [3][n]
    DevBuf<double> gu;                                   // grad U  [9][n]  (TVD only)
    DevBuf<double> flux, pf, coef;                       // per face: outward (from c0) flux, face pressure, p' coefficient
    DevBuf<double> partials, scal;
    DevBuf<int> dev_status;
    Arena arena;
    SolveStats stats;
    SiblingPairing sibling;  // u's pairing of this iteration as the starting state of v's and w's (linalg.hpp)
    // The u, v and w systems of an iteration are independent (solver.rs:99-136 solves them one after the other, none
    // reads another's result): each gets its own stream, arena and host thread, so the latency-bound set-up rounds of
    // one hierarchy overlap the bandwidth-bound products of another.  Same kernels, same order per system: same bits.
    struct Lane {
        hipStream_t stream = nullptr;
        Arena arena;
        SolveStats stats;
        SolveSide side;   // second stream of the lane's Multigrid solves (set-up beside smoothing, linalg.hpp)
        Arena side_arena;
        Arena scratch_arena;  // transient storage of a hierarchy set-up ahead of its solve (multigrid_prepare_dev's `scratch`)
        AmgHierarchy hierarchy;        // partitioned runs: built by the lane while the library stream does the level-0 work
        hipEvent_t level0_done = nullptr;
    } lanes[3];
    // The three momentum systems solved in lock-step on their shared pattern (MatView3, linalg.hpp): one column stream and one
    // 24-byte gather per entry for three value streams on level 0 and, when the pairings coincide, on level 1.  Uses the
    // lanes' streams and arenas for the hierarchy set-ups and the per-system coarse levels.  ORC_TRIPLE_MOMENTUM=0: off.
    TripleLane triple[3];
    bool triple_momentum = true;
    // The pressure-correction matrix depends on the momentum diagonals and the geometry only (discretization.rs:401-438;
    // the new velocities enter its RHS), so its Multigrid hierarchy is built on a stream of its own while the momentum
    // systems are being solved, and the p' solve finds it ready.
    AmgHierarchy p_hierarchy;
    Arena hier_arena, hier_scratch;
    hipStream_t prep_stream = nullptr;
    bool early_p_hierarchy = true;
    bool p_scratch_shared = false;  // this iteration's p' set-up borrows lane 0's scratch arena (it starts when the momentum set-ups are through)
    bool sibling_pairing = true;  // v and w take u's fine-level pairing when it verifies as theirs (ORC_AMG_SIBLING=0: off)
    SolveSide side;       // the same for the solves on the library stream (p', or all four when the lanes are off)
    Arena side_arena;
    bool two_stream_multigrid = true;
    // A linear solver of its own for the pressure correction (orc_solver_set_pressure_solver): off unless set.  The momentum schedule
    // keeps following settings.solver_type; the p' solve and the decision about its early hierarchy follow p_settings().
    bool p_solver_on = false;
    OrcLinearSolver p_solver{};
    OrcSettings p_settings() const {  // the settings the p' solve runs with
        OrcSettings t = settings;
        if (p_solver_on) {
            t.solver_type = p_solver.solver_type; t.preconditioner = p_solver.preconditioner; t.iterations = p_solver.iterations;
            t.relative_convergence_threshold = p_solver.relative_convergence_threshold; t.relaxation = p_solver.relaxation;
        }
        return t;
    }
    // Test hook (orc_solver_debug_pressure_hierarchies): p' hierarchies set up so far.  A set-up ahead of the solve is counted where it
    // ran (prepare of the p' hierarchy); one inside the solve is INFERRED, not observed: the iteration loop counts a p' solve by a
    // Multigrid arm that finds no prepared hierarchy, because that arm then builds its own.
    long long p_hierarchy_setups = 0;
    bool concurrent_momentum = true;
    ~SolverState();
    uint64_t iterations_done = 0;
    // orc_solver_snapshot / orc_solver_restore: the state one SIMPLE iteration starts from (u, v, w, p and the momentum
    // diagonals Rhie-Chow reads), kept device-side so that a benchmark can time the SAME iteration repeatedly
    DevBuf<double> snap[7];
    uint64_t snap_iterations = 0;
    bool has_snapshot = false;
    // Implicit time stepping (orc_solver_set_transient): off unless enabled.  lev[0..2] = u, v, w at level n, lev[3..5] at n-1,
    // allocated on first enabling; time_term_k adds the time term at the end of k_momentum while transient && time_levels > 0.
    bool transient = false;
    OrcTransient tr{};
    int time_levels = 0;  // known previous levels, 0..2
    double time = 0.;     // time reached since the arm was enabled
    DevBuf<double> lev[6];
    DevBuf<double> snap_lev[6];
    int snap_time_levels = 0;
    double snap_time = 0.;
    bool snap_transient = false;
    // Adaptive time stepping (orc_solver_set_time_step / _control, api_transient.cpp): dt is the step the next orc_solver_advance step
    // takes (OrcTransient.dt until someone changes it), dt_last the one that led from level n-1 to n.  Every arm reads dt, never the
    // OrcTransient; with nothing changed dt_last == dt and time_coef() is 1.5 / 2 / 0.5 exactly.
    double dt = 0., dt_last = 0., dt_before_last = 0.;
    double snap_dt = 0., snap_dt_last = 0., snap_dt_before_last = 0.;
    struct TimeCoef { double a0, a1, a2; };
    TimeCoef time_coef() const {  // variable-step BDF2 on the host, once per launch: w = dt / dt_last
        const double w = dt / dt_last;
        return {(1. + 2. * w) / (1. + w), 1. + w, (w * w) / (1. + w)};
    }
    struct StepControl {
        bool on = false;           // orc_solver_set_time_step_control
        bool manual = false;       // orc_solver_set_time_step was called: rows are recorded without control too
        OrcTimeStepControl c{};
        uint64_t step = 0, snap_step = 0;  // steps since control was set
        std::vector<double> history;       // 4 doubles per recorded step
    } ctl;
    // The Courant reduction (courant.hip): off until orc_solver_courant or a controlled step asks; every buffer its own.
    struct Courant {
        DevBuf<double> part_v, out;   // [kMaxPartials] workgroup maxima; [4] rate_max, id, (rate_max or +inf, NaN flag) for the all-reduce
        DevBuf<int64_t> part_id;      // [kMaxPartials] their ORC ids
        DevBuf<int32_t> orc_id;       // ORC id of every internal cell; empty when the numbering is ORC's own
        DevBuf<int> status;
        PinnedBuf<double> raw;        // [2] where the pair lands
        bool ready = false;
    } cr;
    bool diagonals_assembled = false;  // k_momentum has written du/dv/dw at least once (Rhie-Chow face fluxes need them)
    // Residual monitors (orc_solver_set_monitors, residuals.hip): off unless enabled.  The partial sums and the folded raw slots are
    // the monitor's own — s.partials / s.scal belong to the Peclet statistics and the correction.  dev: the folded slots in
    // COLLECTIVE order (kSums sums, then kMaxima maxima: one all-reduce each); raw: pinned host memory where the iteration's copy of
    // them lands (complete at the iteration's last synchronisation).
    struct Monitor {
        static constexpr int kSums = 11, kMaxima = 4;  // sum|r|, sum|d|, sum r^2 x 3, sum|b_p|, sum b_p^2; max|r| x 3, max|b_p|
        bool on = false;
        DevBuf<double> partials;   // [12 * kMaxPartials] momentum pass, then [3 * kMaxPartials] imbalance pass
        DevBuf<double> dev;        // [kSums + kMaxima]
        PinnedBuf<double> raw;     // [kSums + kMaxima]
        std::vector<double> history;  // ORC_RESIDUAL_N doubles per monitored iteration
        uint64_t seen = 0;         // monitored iterations since monitoring was switched on
        double scale = 0.;         // the continuity scale (record slot 15)
    } mon;
    // Passive scalar transport (orc_solver_set_scalar, scalar.hip): off unless enabled; every buffer is the arm's own, so
    // that nothing the flow reads is written.
    struct Scalar {
        bool on = false;
        OrcScalarSettings c{};
        DevBuf<double> phi, phi_old, lev[2], src;      // [n]
        DevBuf<double> a, a_g;                          // SELL values: the system, its Gamma part (built once per configuration)
        DevBuf<double> b, b_g;                          // [n]: the right-hand side, its Gamma part
        DevBuf<double> grad;                            // [3][n] Green-Gauss grad phi (TVD)
        DevBuf<double> gp, flux, pf, corr, bterm;       // the arm's grad p [3][n]; per face: flux, face pressure, c_f, boundary term
        DevBuf<int32_t> zkind;                          // resolved OrcScalarBc per zone (VALUE, FLUX, ZERO_GRADIENT)
        DevBuf<double> zval, partials, scal;
        std::vector<int32_t> kind;                      // as set per zone (DEFAULT included)
        std::vector<double> value;
        std::vector<int32_t> resolved_kind;             // what a_g / b_g were built for
        std::vector<double> resolved_value;
        bool has_source = false;
        int levels = 0;                                 // known previous levels, 0..2
        double report[4] = {0., 0., 0., 0.};
        DevBuf<double> snap_phi, snap_lev[2];
        int snap_levels = 0;
        bool snap_on = false;
        // Variable diffusivity (orc_solver_set_scalar_diffusivity): off unless enabled; Gamma is a function of state that is already
        // covered (the field as set, the viscosity arm's mu, phi), evaluated on the fly — no per-cell Gamma is kept.
        struct Diffusivity {
            bool on = false;
            OrcScalarDiffusivity c{};
            DevBuf<double> field;  // [n] the FIELD model's data as set
            bool has_field = false;
            bool stale = false;    // a_g / b_g were built for another model or field
        } gd;
    } sc;
    // the scalar's EDDY diffusivity reads vis.mu: orc_solver_set_viscosity keeps the arm on with a model that has an eddy part
    bool scalar_gamma_reads_viscosity() const { return sc.on && sc.gd.on && sc.gd.c.model == ORC_SCALAR_GAMMA_EDDY; }
    // Variable viscosity (orc_solver_set_viscosity, viscosity.hip): off unless enabled, every buffer allocated by a set call.  While it
    // is on, a_di and b_*_di are rebuilt from `mu` ahead of every momentum assembly; off again, they are k_diffusion's.
    struct Viscosity {
        bool on = false;
        OrcViscosity c{};
        DevBuf<double> mu;      // [n] the field the last assembly used (ghost entries exchanged before the rebuild)
        DevBuf<double> field;   // [n] the FIELD model's data as set
        bool has_field = false;
        bool first = true;      // the next evaluation of an assembly takes the law's value itself (no relaxation)
        DevBuf<double> snap_mu;
        bool snap_on = false, snap_first = true;
        OrcWallDamping wd{ORC_WALL_DAMPING_NONE, 0, 0.41, 26., 0.};  // wall damping of the Smagorinsky length (orc_solver_set_wall_damping); mode NONE = off
    } vis;
    const double *cell_viscosity() const { return vis.on ? vis.mu.p : nullptr; }  // what the surface reports and boundary maps take
    // the post-processing arms (postproc_state.hpp): time statistics, probe history, group history, tracer tracking
    TimeStats ts;
    ProbeHistory ph;
    GroupHistory gh;
    TracerTracking tt;
};

int mesh_upload(OrcMesh &m, int64_t n_own, int64_t n_cells, int64_t n_faces, int32_t n_zones, const int64_t *face_c0, const int64_t *face_c1,
                const int32_t *face_zone, const double *face_area, const double *face_normal, const double *face_centroid,
                const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr, const int64_t *cell_faces,
                const int32_t *zone_type, const double *zone_scalar, const double *zone_vector);

// solver_state.cpp
int solver_init(SolverState &s, OrcMesh *m, const OrcSettings *settings, double rho, double mu);
int fetch_status(SolverState &s);

inline bool is_tvd(int momentum) { return momentum >= ORC_MOMENTUM_TVD_LUD && momentum <= ORC_MOMENTUM_TVD_CD1; }

// a matrix on the mesh pattern (a_u, a_v, a_w, a_p, a_di, the scalar arm's) as the solves see it
inline MatView mesh_view(const SolverState &s, const double *values) {
    MatView A;
    A.P = s.mesh->pat.dev();
    A.val = values;
    A.symmetric = s.mesh->pat.symmetric;
    A.halo = s.mesh->halo.active() ? &s.mesh->halo : nullptr;
    A.persistent_pattern = true;
    return A;
}

// partitioned mesh: the ghost entries of u, v, w, p, and of a gradient [3][n], before a face kernel reads them (C1)
inline int exchange_fields(SolverState &s) {
    if (!s.mesh->halo.active()) return ORC_OK;
    double *f[4] = {s.u.p, s.v.p, s.w.p, s.p.p};
    return s.mesh->halo.exchange(f, 4);
}
inline int exchange_gradient(SolverState &s, double *gp) {
    if (!s.mesh->halo.active()) return ORC_OK;
    double *g3[3] = {gp, gp + s.n, gp + 2 * s.n};
    return s.mesh->halo.exchange(g3, 3);
}

// assembly.hip: the kernels' launch wrappers (all asynchronous on the calling thread's stream, ctx().stream)
int k_diffusion(SolverState &s);                 // K14  discretization.rs:39-131
int k_init_momentum(SolverState &s);             // discretization.rs:450-472
int k_gradients(SolverState &s, bool need_gu);   // K9   solver.rs:774-802, 874-902
int k_face_flux(SolverState &s, bool with_pf);   // K10  solver.rs:1007-1150
int k_momentum(SolverState &s, double *peclet_host /*3, may be null*/);  // K11  discretization.rs:134-356
int k_time_term(SolverState &s);                 // implicit time term on the momentum systems (transient arm, k_momentum)
int k_pressure_correction(SolverState &s);       // K12  discretization.rs:359-448
int k_pressure_matrix(SolverState &s);           // the p' matrix alone from the fresh momentum diagonals: face_coef_k, then pressure_k
int k_apply_correction(SolverState &s, double *sums_host /*5: p'^2, |dU|^2, sum u, sum v, sum w*/);  // K13 solver.rs:1170-1227
// simple_iteration.cpp
int solver_iterate(SolverState &s, uint64_t iterations, double *report);
// initialize.hip
int check_boundary_conditions(const OrcMesh &m);       // solver.rs:710-772: 0 PressureOnly, 1 VelocityOnly, 2 Hybrid, < 0 = -status
int initialize_pressure_field_dev(SolverState &s);     // solver.rs:414-509
int initialize_flow_dev(SolverState &s, uint64_t iteration_count);  // solver.rs:246-352
int initialize_velocity_field_dev(SolverState &s);     // solver.rs:511-696 (psi in s.p_prime, velocities in s.u/v/w)
int post_loop_gradients_dev(SolverState &s);           // solver.rs:227-242
// scalar arm (scalar.hip): face_k<0>'s flux of the current fields into the arm's own gp / flux / pf (ghosts exchanged first)
int k_scalar_face_flux(SolverState &s);
// the linear solve of the scalar system (equation index 4: no sibling pairing, no p' hierarchy) with the settings `t`
int solve_scalar_system(SolverState &s, const OrcSettings &t);
// one scalar solve of orc_solver_advance (levels shifted first), the report kept in s.sc.report
int scalar_step_dev(SolverState &s);
// surface reports (surface.hip): per zone ORC_SURFACE_N sums of the device fields u, v, w, p (the mesh's internal cell order) to the host
// mu_cell (may be null): a per-cell viscosity of the same order that replaces mu in the viscous terms
int surface_report_dev(OrcMesh &m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                       const double *mu_cell, const double origin[3], double *per_zone);
// the boundary index of the mesh (m.surface), built at first use: what the reports and the boundary maps of derived.hip walk
int surface_index(OrcMesh &m);
// residual monitors (residuals.hip), all asynchronous on ctx().stream: the fused pass over a_u/a_v/a_w, b_u/b_v/b_w and the fields they
// were assembled from (after k_momentum, before the solves); the pass over b_p (after k_pressure_correction, before the p' solve);
// the all-reduces of a partitioned mesh and the copy of the fifteen raw slots into s.mon.raw (complete at the iteration's last
// synchronisation); the record of the iteration from s.mon.raw, appended to the history.
int monitors_enable(SolverState &s, bool on);
int k_momentum_residuals(SolverState &s);
int k_imbalance(SolverState &s);
int monitor_fetch(SolverState &s);
void monitor_append(SolverState &s);
// variable viscosity (viscosity.hip), asynchronous on ctx().stream.  k_viscosity: viscosity_cell_k, the law on the current fields into
// mu_out (relaxed against mu_out's old content when `relax`), the strain-rate magnitude into g_out (may be null).  k_diffusion_var:
// diffusion_var_k, a_di and b_*_di from s.vis.mu.  k_viscosity_update: what an assembly runs ahead of k_face_flux while the arm is on
// (the fields' ghosts are current): the law (not FIELD), one exchange of the viscosity's ghosts, the rebuild.
int k_viscosity(SolverState &s, double *mu_out, double *g_out, bool relax);
int k_diffusion_var(SolverState &s);
int k_viscosity_update(SolverState &s);
// wall distance (wall_distance.hip): the cached field of the default mask (zones of type WALL) in the mesh's internal cell order, searched
// at first use; synchronises and, on a partitioned mesh, runs two all-reduces when it has to build.  wall_zones_changed: what
// orc_mesh_update_zones calls with the new zone types before it uploads them.
int wall_distance_default(OrcMesh &m, const double **d_dev);
void wall_zones_changed(OrcMesh &m, const int32_t *zone_type);
int wall_damping_validate(const OrcWallDamping &w);  // ORC_ERR_BAD_ARGUMENT with a message, or ORC_OK
// boundary maps (derived.hip): the fields of `mask` (OrcBoundaryField bits) of device fields in the mesh's internal order into the DEVICE
// buffer out_dev [popcount(mask)][nb], asynchronous on ctx().stream; a face in a refused zone raises *status_dev.  Builds the boundary
// index if need be.
int boundary_maps_dev(OrcMesh &m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                      const double *mu_cell, uint32_t mask, double *out_dev, int *status_dev);
// the Courant reduction (courant.hip): the largest convective rate of the current u, v, w over the owned cells (all ranks' on a
// partitioned mesh) and the smallest ORC id that attains it (-1 on a partitioned mesh) to the host; rate_dev (may be null): the per-cell
// values, internal order, n long, from the same launch.  Exchanges the fields' ghosts first; returns with the stream synchronised.
int courant_dev(SolverState &s, double *rate_max, int64_t *cell, double *rate_dev);

}  // namespace orc

struct OrcSolver {
    orc::SolverState st;
};
