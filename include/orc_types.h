/* orc_types.h — plain-C value types shared by the C-ABI (include/orc_amd.h) and the
 * test oracle (oracle/).  Values only, no code.
 *
 * Every enum mirrors one Rust enum of the reference (ORC v0.3.0); the numeric values are
 * ours (Rust enums without #[repr] have no ABI), the names and meaning are the reference's.
 * Citations are file:line into /root/reference.
 */
#ifndef ORC_TYPES_H
#define ORC_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* settings::MomentumDiscretization (src/lib.rs:95-118).  The reference's `TVD(fn(f64)->f64)`
 * carries a bare function pointer; across the C ABI it becomes a limiter tag. */
enum OrcMomentumDiscretization {
    ORC_MOMENTUM_UD = 0,        /* lib.rs:98  */
    ORC_MOMENTUM_CD1 = 1,       /* lib.rs:100 */
    ORC_MOMENTUM_CD2 = 2,       /* lib.rs:102 — reference panics "unsupported momentum scheme" (discretization.rs:287) */
    ORC_MOMENTUM_TVD_LUD = 3,   /* lib.rs:109  psi(r) = r */
    ORC_MOMENTUM_TVD_QUICK = 4, /* lib.rs:110  psi(r) = (3 + r) / 4 */
    ORC_MOMENTUM_TVD_UMIST = 5, /* lib.rs:111-118 */
    ORC_MOMENTUM_TVD_UD = 6,    /* lib.rs:107  psi = 0 (private const in the reference) */
    ORC_MOMENTUM_TVD_CD1 = 7    /* lib.rs:108  psi = 1 (private const in the reference) */
};

/* settings::DiffusionScheme (lib.rs:120-123) */
enum OrcDiffusionScheme { ORC_DIFFUSION_CD = 0 };

/* settings::PressureInterpolation (lib.rs:125-133) */
enum OrcPressureInterpolation {
    ORC_PINTERP_LINEAR = 0,
    ORC_PINTERP_LINEAR_WEIGHTED = 1,
    ORC_PINTERP_STANDARD = 2, /* reference panics (solver.rs:1136) */
    ORC_PINTERP_SECOND_ORDER = 3,
    ORC_PINTERP_NONE = 4
};

/* settings::VelocityInterpolation (lib.rs:135-146) */
enum OrcVelocityInterpolation {
    ORC_VINTERP_LINEAR = 0,
    ORC_VINTERP_LINEAR_WEIGHTED = 1,
    ORC_VINTERP_RHIE_CHOW = 2,
    ORC_VINTERP_NONE = 3
};

/* settings::GradientReconstructionMethods (lib.rs:154-162) */
enum OrcGradientReconstruction {
    ORC_GRAD_GREEN_GAUSS_CELL = 0,
    ORC_GRAD_GREEN_GAUSS_NODE = 1, /* reference panics (solver.rs:901) */
    ORC_GRAD_LEAST_SQUARES = 2,    /* solver.rs:803-869, 903-947: normal equations per cell, 3x3 inverse */
    ORC_GRAD_NONE = 3
};

/* settings::SolutionMethod (lib.rs:171-179) */
enum OrcSolutionMethod {
    ORC_SOLVER_GAUSS_SEIDEL = 0, /* reference: dense row scan then panic!("Gauss-Seidel out for maintenance") (linear_algebra.rs:219-246) */
    ORC_SOLVER_JACOBI = 1,
    ORC_SOLVER_MULTIGRID = 2,
    ORC_SOLVER_BICGSTAB = 3,
    /* --- new-build extensions, no reference counterpart --- */
    ORC_SOLVER_MULTICOLOR_GS = 16,         /* multicolour Gauss-Seidel sweeps */
    ORC_SOLVER_BICGSTAB_GS_PRECOND = 17,   /* right-preconditioned BiCGSTAB, M = one multicolour GS sweep */
    ORC_SOLVER_MULTIGRID_GS = 18,          /* Multigrid arm with multicolour GS as the smoother */
    ORC_SOLVER_GMRES = 19,                 /* restarted GMRES(m), CGS2 Arnoldi, relative stopping test (orc_amd.h: orc_set_gmres_restart) */
    ORC_SOLVER_CG = 20                     /* preconditioned conjugate gradients for symmetric positive definite systems (orc_amd.h: orc_last_cg_stats) */
};

/* settings::PreconditionMethod (lib.rs:181-185) */
enum OrcPreconditionMethod { ORC_PRECOND_NONE = 0, ORC_PRECOND_JACOBI = 1 };

/* mesh::FaceConditionTypes (mesh.rs:25-42); values are the TGRID codes of mesh.rs:51-65 */
enum OrcFaceConditionType {
    ORC_BC_INTERIOR = 2,
    ORC_BC_WALL = 3,
    ORC_BC_PRESSURE_INLET = 4,
    ORC_BC_PRESSURE_OUTLET = 5,
    ORC_BC_SYMMETRY = 7,
    ORC_BC_PERIODIC_SHADOW = 8,
    ORC_BC_PRESSURE_FAR_FIELD = 9,
    ORC_BC_VELOCITY_INLET = 10,
    ORC_BC_PERIODIC = 12,
    ORC_BC_POROUS_JUMP = 14,
    ORC_BC_MASS_FLOW_INLET = 20,
    ORC_BC_INTERFACE = 24,
    ORC_BC_PARENT = 31,
    ORC_BC_OUTFLOW = 36,
    ORC_BC_AXIS = 37
};

/* Status codes: one per panic! site on the path (SURVEY §5 "Failure detection").
 * A Rust shim turns non-zero back into panic!(orc_status_string(code)). */
enum OrcStatus {
    ORC_OK = 0,
    ORC_ERR_SOLUTION_DIVERGED = 1,     /* solver.rs:217-221 "solution diverged" */
    ORC_ERR_MULTIGRID_DIVERGED = 2,    /* linear_algebra.rs:103-105 */
    ORC_ERR_JACOBI_NAN = 3,            /* linear_algebra.rs:192-196 "diverged" */
    ORC_ERR_JACOBI_TOO_LARGE = 4,      /* linear_algebra.rs:214-216 */
    ORC_ERR_GS_MAINTENANCE = 5,        /* linear_algebra.rs:245 */
    ORC_ERR_STRUCTURAL_ZERO = 6,       /* lib.rs:664-666 */
    ORC_ERR_UNSUPPORTED_BC = 7,        /* discretization.rs:114-117, solver.rs:1001,1100,1148,1209-1212 */
    ORC_ERR_UNSUPPORTED_SCHEME = 8,    /* discretization.rs:50,287; solver.rs:224,870,901,948,994,1097,1136,1145 */
    ORC_ERR_UNSUPPORTED_SOLVER = 9,    /* linear_algebra.rs:297 */
    ORC_ERR_BAD_ARGUMENT = 10,
    ORC_ERR_NO_DEVICE = 11,            /* HIP runtime/device missing: the product never falls back to a CPU path */
    ORC_ERR_HIP = 12,
    ORC_ERR_IO = 13,
    ORC_ERR_COMM = 14,
    ORC_ERR_MESH_FORMAT = 15,          /* io.rs:32-515: any of read_mesh's expect()/panic! sites; orc_last_error() names file:line and the reference's message */
    ORC_ERR_ZONE_NOT_FOUND = 16,       /* mesh.rs:189-195 "face zone '{zone_name}' should exist in mesh" */
    ORC_ERR_NO_BOUNDARY_CONDITIONS = 17, /* solver.rs:770 "You must set boundary conditions." */
    ORC_ERR_SINGULAR_MATRIX = 18       /* solver.rs:850,943: `a.try_inverse().unwrap()` on a singular least-squares normal matrix */
};

/* Association of the solvers' dot products and norms (linear_algebra.rs:97,202,253,257,261,265).
 * TREE: per-workgroup wave-shuffle trees folded in a fixed order — deterministic, fast, the product default.
 * REFERENCE: nalgebra 0.32.4's `dotx` order (eight running accumulators over blocks of 8, then the tail), evaluated by
 * one wavefront — slow, but every iterate of BiCGSTAB / Jacobi / the Multigrid arm is then bit-identical to the
 * reference's arithmetic at any iteration count (verification mode; single GPU only). */
enum OrcReductionOrder { ORC_REDUCTION_TREE = 0, ORC_REDUCTION_REFERENCE = 1 };

/* Cell orders for orc_mesh_partition: ORC's own numbering (io.rs:404-438), reverse Cuthill-McKee over the face-neighbour
 * graph, or sorted along the longest extent of the domain. */
enum OrcCellOrdering { ORC_ORDER_ORC = 0, ORC_ORDER_RCM = 1, ORC_ORDER_GEOMETRIC = 2 };

/* settings::NumericalSettings + settings::MatrixSolverSettings (lib.rs:14-56), flattened.
 * orc_settings_default() fills in lib.rs:58-86. */
typedef struct OrcSettings {
    int32_t momentum;                /* OrcMomentumDiscretization; default CD1   (lib.rs:62) */
    int32_t diffusion;               /* OrcDiffusionScheme;        default CD    (lib.rs:63) */
    int32_t pressure_interpolation;  /* default SecondOrder (lib.rs:64) */
    int32_t velocity_interpolation;  /* default RhieChow    (lib.rs:65) */
    int32_t gradient_reconstruction; /* default GreenGauss(CellBased) (lib.rs:66-68) */
    int32_t solver_type;             /* default Multigrid   (lib.rs:79) */
    int32_t preconditioner;          /* default Jacobi      (lib.rs:83) */
    int32_t q1_compat;               /* 1 = reproduce `f64 * Vector` z:=y bug (lib.rs:540-548); default 1 */
    uint64_t iterations;             /* default 50   (lib.rs:80) */
    double momentum_relaxation;      /* default 0.5  (lib.rs:70) */
    double pressure_relaxation;      /* default 0.01 (lib.rs:69) */
    double relaxation;               /* default 0.5  (lib.rs:81) */
    double relative_convergence_threshold; /* default 1e-3 (lib.rs:82) */
    int32_t frozen_diagonals;        /* 0 = reference's in-place (order dependent) diagonal reads — oracle only;
                                        1 = all Rhie-Chow reads see last iteration's diagonals (what the device computes) */
    int32_t breakdown_guard;         /* new-build extension, default 1: BiCGSTAB stops updating x when a denominator of its
                                        recurrences (rho, r_hat.nu, t.t, omega) is exactly 0 or non-finite — the only cases
                                        in which the reference (no guard, linear_algebra.rs:255-268) yields NaN and panics
                                        "solution diverged".  0 = reference behaviour (NaN propagates).  Every solve in
                                        which the guard fired is counted: orc_breakdown_guard_events(). */
    int32_t reduction_order;         /* OrcReductionOrder; default TREE */
    int32_t gmres_restart;           /* new-build extension: restart length m of ORC_SOLVER_GMRES; 0 (default) = 30, 1..64 accepted,
                                        anything else is ORC_ERR_BAD_ARGUMENT when the GMRES arm runs */
} OrcSettings;

/* Implicit time stepping (new-build extension; ORC's roadmap lists "Iterate transient" as not done).  With c = rho V_P / dt
 * the three momentum systems get  Euler: diag += c, b += c u_n;  BDF2: diag += 1.5 c, b += c (2 u_n - 0.5 u_nm1)
 * (the fixed-step values of the coefficients under OrcTimeStepControl below).
 * orc_amd.h: orc_solver_set_transient, orc_solver_advance, orc_solve_transient. */
enum OrcTimeScheme { ORC_TIME_EULER = 0, ORC_TIME_BDF2 = 1 };

typedef struct OrcTransient {
    double dt;                 /* > 0, finite */
    int32_t scheme;            /* OrcTimeScheme */
    int32_t reserved0;         /* 0 */
    uint64_t inner_iterations; /* >= 1: SIMPLE iterations per time step at most */
    double inner_tolerance;    /* >= 0; 0 = always inner_iterations */
} OrcTransient;

/* Adaptive time stepping (new-build extension): the rule by which orc_solver_advance chooses the next step from the largest
 * convective rate max_c sum_f |U_f . n| A / (2 V_c) of the fields just reached (orc_solver_courant).  The law, in this operator order:
 *     want = rate_max > 0 ? target_courant / rate_max : dt_max
 *     next = min(max(want, dt * max_shrink), dt * max_growth)
 *     next = min(max(next, dt_min), dt_max)
 * With a changing step, w = dt / dt_last, BDF2 reads  diag += a0 c, b += c (a1 u_n - a2 u_nm1),  a0 = (1 + 2 w) / (1 + w),
 * a1 = 1 + w, a2 = (w w) / (1 + w); w = 1 gives 1.5, 2 and 0.5 exactly.
 * orc_amd.h: orc_solver_set_time_step_control, orc_time_step_next and their companions. */
typedef struct OrcTimeStepControl {
    double target_courant;        /* > 0, finite */
    double dt_min, dt_max;        /* 0 < dt_min <= dt_max, finite */
    double max_growth;            /* in [1, 2]: dt_next <= max_growth * dt (BDF2's zero-stability needs a ratio below 1 + sqrt 2) */
    double max_shrink;            /* in (0, 1]: dt_next >= max_shrink * dt */
    uint64_t interval;            /* >= 1: dt is chosen anew after every interval-th step */
    int32_t reserved0, reserved1; /* 0 */
} OrcTimeStepControl;

/* Passive scalar transport (new-build extension; ORC has no scalar equation):
 *     rho dphi/dt + div(rho U phi) = div(Gamma grad phi) + S
 * carried by the solver's current flow, which it never changes.  orc_amd.h: orc_solver_set_scalar and its companions;
 * DESIGN.md "Passive scalar transport" defines the discretisation.  A zone's scalar condition: */
enum OrcScalarBc {
    ORC_SCALAR_BC_DEFAULT = 0,       /* from the flow's zone type: Wall, Symmetry -> FLUX 0; VelocityInlet, PressureInlet -> VALUE 0;
                                        PressureOutlet -> ZERO_GRADIENT */
    ORC_SCALAR_BC_VALUE = 1,         /* phi_b = value */
    ORC_SCALAR_BC_FLUX = 2,          /* value = diffusive flux INTO the domain per unit area */
    ORC_SCALAR_BC_ZERO_GRADIENT = 3  /* FLUX 0 */
};

typedef struct OrcScalarSettings {
    double diffusivity;                    /* Gamma > 0, finite, in the units of mu; default 1e-3 */
    int32_t scheme;                        /* OrcMomentumDiscretization except CD2; default UD.  TVD_* = implicit UD + deferred
                                              correction with the momentum scheme's limiter, iterated by the outer (Picard) loop */
    int32_t solver_type;                   /* OrcSolutionMethod; default BiCGSTAB */
    int32_t preconditioner;                /* OrcPreconditionMethod; default Jacobi */
    int32_t reserved0;                     /* 0 */
    uint64_t iterations;                   /* >= 1: linear solver iterations; default 500 */
    double relative_convergence_threshold; /* >= 0; default 1e-10 */
    double relaxation;                     /* the linear solver's relaxation factor (as OrcSettings.relaxation); default 0.5 */
    uint64_t outer_iterations;             /* >= 1: Picard rounds of a TVD solve at most; default 30 */
    double outer_tolerance;                /* >= 0: stop once |phi_new - phi_old|_2 <= outer_tolerance |phi_new|_2; default 1e-8 */
} OrcScalarSettings;

/* A linear solver of its own for ONE system of the SIMPLE iteration (new-build extension; the reference's solve_steady has one
 * MatrixSolverSettings for all four systems, solver.rs:99-179).  orc_amd.h: orc_solver_set_pressure_solver — the pressure
 * correction is symmetric positive definite, the momentum systems are not, so ORC_SOLVER_CG can serve the one and not the others. */
typedef struct OrcLinearSolver {
    int32_t solver_type;    /* OrcSolutionMethod */
    int32_t preconditioner; /* OrcPreconditionMethod */
    uint64_t iterations;    /* >= 1 */
    double relative_convergence_threshold; /* >= 0 */
    double relaxation;
} OrcLinearSolver;

/* Per-zone surface reports (new-build extension; orc_amd.h: orc_solver_surface_report): every zone gets ORC_SURFACE_N doubles, each
 * the sum over the zone's boundary faces of owned cells of the term named below.  n = unit normal out of the face's cell, A = area,
 * U_f / p_f / phi_f = the boundary value of get_face_velocity (VelocityInterpolation::None) / get_face_pressure / get_face_flux,
 * d_f = mu A / |x_f - x_P| on Wall and VelocityInlet faces and 0 elsewhere (the coefficient of build_momentum_diffusion_matrix).
 * DESIGN.md §3 "Surface reports" fixes the operator order of every term. */
enum OrcSurfaceQuantity {
    ORC_SURFACE_AREA = 0,            /* A */
    ORC_SURFACE_MASS_FLOW = 1,       /* rho phi_f A; positive = leaving the domain */
    ORC_SURFACE_PRESSURE_FORCE = 2,  /* [2..4] p_f A n: the force the fluid exerts ON the boundary */
    ORC_SURFACE_VISCOUS_FORCE = 5,   /* [5..7] d_f (U_P - U_f): likewise, the momentum the discrete equations hand to the boundary */
    ORC_SURFACE_MOMENTUM_FLOW = 8,   /* [8..10] rho phi_f A U_f */
    ORC_SURFACE_MOMENT = 11,         /* [11..13] (x_f - x_0) x (p_f A n + d_f (U_P - U_f)) about the caller's origin x_0 */
    ORC_SURFACE_PRESSURE_AREA = 14,  /* p_f A; mean pressure = [14] / [0] */
    ORC_SURFACE_FACES = 15,          /* 1.0 */
    ORC_SURFACE_N = 16
};

/* Derived cell fields (new-build extension; orc_amd.h: orc_solver_derived_fields).  G = the velocity gradient of the settings'
 * gradient_reconstruction, G[i][j] = d u_i / d x_j (row = velocity component, the layout of orc_calculate_gradients' grad_u);
 * S_ij = (G_ij + G_ji) / 2, W_ij = (G_ij - G_ji) / 2.  A field is selected by bit (1 << value) of a mask.  DESIGN.md §3
 * "Derived fields and boundary maps" fixes the operator order. */
enum OrcDerivedField {
    ORC_DERIVED_VORTICITY_X = 0,     /* G[2][1] - G[1][2] */
    ORC_DERIVED_VORTICITY_Y = 1,     /* G[0][2] - G[2][0] */
    ORC_DERIVED_VORTICITY_Z = 2,     /* G[1][0] - G[0][1] */
    ORC_DERIVED_VORTICITY_MAG = 3,   /* sqrt((wx^2 + wy^2) + wz^2) */
    ORC_DERIVED_STRAIN_RATE_MAG = 4, /* sqrt(2 SS), SS = ((G00^2 + G11^2) + G22^2) + 2 ((S01^2 + S02^2) + S12^2) */
    ORC_DERIVED_Q_CRITERION = 5,     /* (OO - SS) / 2, OO = 2 ((W01^2 + W02^2) + W12^2) */
    ORC_DERIVED_DIVERGENCE = 6,      /* (G00 + G11) + G22 */
    ORC_DERIVED_CONVECTIVE_RATE = 7, /* (sum_f |U_f . n| A) / (2 V) in 1/s, U_f = the linear face value; times dt = the Courant number */
    ORC_DERIVED_N = 8
};

/* Boundary-face maps (new-build extension; orc_amd.h: orc_solver_boundary_fields): one value per boundary face of an owned cell in
 * the order of orc_mesh_boundary_index.  Every term is the surface report's (OrcSurfaceQuantity above), same operator order. */
enum OrcBoundaryField {
    ORC_BOUNDARY_PRESSURE = 0,   /* p_f */
    ORC_BOUNDARY_TRACTION_X = 1, /* [1..3] d_f (U_P - U_f) / A: the report's viscous term per unit area; 0 where d_f is 0 */
    ORC_BOUNDARY_TRACTION_Y = 2,
    ORC_BOUNDARY_TRACTION_Z = 3,
    ORC_BOUNDARY_SHEAR_MAG = 4,  /* |t - (t . n) n| */
    ORC_BOUNDARY_Y_PLUS = 5,     /* rho sqrt(SHEAR_MAG / rho) |x_f - x_P| / mu */
    ORC_BOUNDARY_MASS_FLUX = 6,  /* rho phi_f; positive = leaving the domain */
    ORC_BOUNDARY_AREA = 7,       /* A */
    ORC_BOUNDARY_N = 8
};

/* Residual monitors (new-build extension; orc_amd.h: orc_solver_set_monitors): one record of ORC_RESIDUAL_N doubles per monitored
 * SIMPLE iteration.  For a momentum system k in {u, v, w} and an owned row P, with the fields the system was assembled from:
 * y_P = sum_j a_Pj phi_j (ascending stored order from 0.0, separate multiply and add), r_P = b_P - y_P, d_P = a_PP phi_P (0 without a
 * stored diagonal).  b_p is the right-hand side of the pressure correction: the cell mass imbalance of the fresh momentum solution.
 * DESIGN.md §3 "Residual monitors" fixes the operator order and the association of the sums. */
enum OrcResidual {
    ORC_RESIDUAL_MOMENTUM_L1 = 0,        /* [0..2] sum |r_P| for u, v, w */
    ORC_RESIDUAL_MOMENTUM_SCALE = 3,     /* [3..5] sum |d_P| */
    ORC_RESIDUAL_MOMENTUM_SQ = 6,        /* [6..8] sum r_P^2 */
    ORC_RESIDUAL_MOMENTUM_MAX = 9,       /* [9..11] max |r_P| */
    ORC_RESIDUAL_CONTINUITY_L1 = 12,     /* sum |b_p| */
    ORC_RESIDUAL_CONTINUITY_SQ = 13,     /* sum b_p^2 */
    ORC_RESIDUAL_CONTINUITY_MAX = 14,    /* max |b_p| */
    ORC_RESIDUAL_CONTINUITY_SCALE = 15,  /* the largest [12] of the first min(k, 5) monitored iterations since monitoring was switched on */
    ORC_RESIDUAL_MOMENTUM_SCALED = 16,   /* [16..18] [k] / [3 + k], or [k] itself where the scale is 0 */
    ORC_RESIDUAL_CONTINUITY_SCALED = 19, /* [12] / [15], or 0 where the scale is 0 */
    ORC_RESIDUAL_N = 20
};

/* The stopping rule of orc_solver_iterate_until / orc_solve_steady_converged: converged when each of the four scaled residuals
 * ([16..19] of a record) is <= its tolerance.  A tolerance of 0 is never met, not even by a residual of exactly 0: that equation
 * alone keeps the run from stopping early. */
typedef struct OrcConvergence {
    double momentum_tolerance[3]; /* >= 0, not NaN: u, v, w */
    double continuity_tolerance;  /* >= 0, not NaN */
    uint64_t min_iterations;      /* the check is not made before this many iterations of the call */
    int32_t reserved0;            /* 0 */
} OrcConvergence;

/* Variable viscosity (new-build extension; orc_amd.h: orc_solver_set_viscosity): a per-cell viscosity in the momentum diffusion, either
 * prescribed (FIELD) or a law of the strain-rate magnitude g = ORC_DERIVED_STRAIN_RATE_MAG of the settings' gradient scheme, bit for bit.
 * DESIGN.md §3 "Variable viscosity" fixes the operator order. */
enum OrcViscosityModel {
    ORC_VISCOSITY_FIELD = 1,       /* the data of orc_solver_set_viscosity_field, neither clamped nor relaxed */
    ORC_VISCOSITY_POWER_LAW = 2,   /* m = k * pow(g, n - 1) */
    ORC_VISCOSITY_CARREAU = 3,     /* t = lambda * g; m = mu_inf + (mu_zero - mu_inf) * pow(1 + t * t, (n - 1) / 2) */
    ORC_VISCOSITY_SMAGORINSKY = 4  /* l = cs * cbrt(V_P); m = mu + (rho * (l * l)) * g, mu and rho the solver's */
};
/* the viscosity of an interior face from its two cells, lo = fmin(mu_P, mu_N), hi = fmax(mu_P, mu_N); a boundary face takes mu_P */
enum OrcViscosityFace {
    ORC_VISCOSITY_FACE_ARITHMETIC = 0, /* (lo + hi) * 0.5 */
    ORC_VISCOSITY_FACE_HARMONIC = 1    /* lo * (hi / ((lo + hi) * 0.5)) */
};
typedef struct OrcViscosity {
    int32_t model;              /* OrcViscosityModel */
    int32_t face_interpolation; /* OrcViscosityFace */
    double k, n;                /* POWER_LAW: k > 0, n finite; CARREAU also uses n */
    double mu_zero, mu_inf;     /* CARREAU: >= 0 */
    double lambda;              /* CARREAU: >= 0 */
    double cs;                  /* SMAGORINSKY: >= 0 */
    double mu_min, mu_max;      /* every law (not FIELD): mu = fmin(fmax(m, mu_min), mu_max); 0 < mu_min <= mu_max < inf */
    double relaxation;          /* (0, 1]: the stored field becomes mu_old + w (mu - mu_old); 1 = none, no arithmetic */
} OrcViscosity;

/* Variable scalar diffusivity (new-build extension; orc_amd.h: orc_solver_set_scalar_diffusivity): a per-cell Gamma in the diffusion of
 * the passive scalar.  With gamma0 = OrcScalarSettings.diffusivity, mu_c the viscosity field of the last momentum assembly
 * (orc_solver_get_viscosity), mu_lam the solver's mu and phi_c the cell's scalar, each law is evaluated in the order written
 * (DESIGN.md §3 "Variable scalar diffusivity"); an interior face takes OrcViscosityFace's formula on (Gamma_P, Gamma_N), a boundary
 * VALUE face its cell's Gamma_P. */
enum OrcScalarDiffusivityModel {
    ORC_SCALAR_GAMMA_CONSTANT = 0, /* gamma0: the arm as it is without the model */
    ORC_SCALAR_GAMMA_FIELD = 1,    /* the data of orc_solver_set_scalar_diffusivity_field, not clamped */
    ORC_SCALAR_GAMMA_EDDY = 2,     /* g = gamma0 + fmax(mu_c - mu_lam, 0.) / schmidt_t, then the clamp */
    ORC_SCALAR_GAMMA_LINEAR = 3    /* g = gamma0 * (1. + beta * (phi_c - phi_ref)), then the clamp */
};
typedef struct OrcScalarDiffusivity {
    int32_t model;              /* OrcScalarDiffusivityModel */
    int32_t face_interpolation; /* OrcViscosityFace: the same two formulas */
    double schmidt_t;           /* EDDY: turbulent Schmidt / Prandtl number, > 0; default 0.7 */
    double beta, phi_ref;       /* LINEAR */
    double gamma_min, gamma_max; /* EDDY and LINEAR: Gamma = fmin(fmax(g, gamma_min), gamma_max); 0 < gamma_min <= gamma_max < inf */
    double reserved0;           /* 0 */
} OrcScalarDiffusivity;

/* Wall damping of the Smagorinsky length (new-build extension; orc_amd.h: orc_solver_set_wall_damping): with d the wall distance of the
 * cell (orc_mesh_wall_distance, zones of type WALL) and l0 = cs * cbrt(V_P), the law's length l becomes
 *   MIN:        l = fmin(kappa * d, l0)
 *   VAN_DRIEST: yp = ((rho * u_tau) * d) / mu;  l = l0 * (-expm1(-(yp / a_plus)))
 * DESIGN.md §3 "Wall distance and wall damping" fixes the operator order. */
enum OrcWallDampingMode { ORC_WALL_DAMPING_NONE = 0, ORC_WALL_DAMPING_MIN = 1, ORC_WALL_DAMPING_VAN_DRIEST = 2 };
typedef struct OrcWallDamping {
    int32_t mode, reserved0; /* OrcWallDampingMode; reserved0 = 0 */
    double kappa;            /* MIN: > 0, default 0.41 */
    double a_plus;           /* VAN_DRIEST: > 0, default 26 */
    double u_tau;            /* VAN_DRIEST: > 0, the caller's friction velocity (channel: sqrt(h |dp/dx| / rho)); default 0 */
} OrcWallDamping;            /* 32 bytes */

/* Running time statistics (new-build extension; orc_amd.h: orc_solver_set_time_statistics): weighted running means of the fields and
 * the weighted co-moment sums C_xy = sum_k w_k (x_k - <x>)(y_k - <y>) of their fluctuations, updated sample by sample with West's
 * recurrence.  One sample of weight w on the state x:  W' = W + w, r = w / W' (host);  per mean  dx = x - m, m' = m + r * dx,
 * ex = x - m';  per co-moment of the ordered pair (x, y)  C' = C + (w * dx) * ey.  C / W is the (co)variance.
 * DESIGN.md §3 "Time statistics" fixes the operator order. */
enum OrcStatGroup {               /* bits of OrcTimeStatistics::groups */
    ORC_STAT_GROUP_MEAN = 1,      /* <u> <v> <w> <p>: always required */
    ORC_STAT_GROUP_STRESS = 2,    /* C_uu C_vv C_ww C_uv C_uw C_vw C_pp */
    ORC_STAT_GROUP_VISCOSITY = 4, /* <mu>: the cell viscosity the momentum assembly used; needs the viscosity arm */
    ORC_STAT_GROUP_SCALAR = 8,    /* <phi> C_phiphi C_uphi C_vphi C_wphi; needs the scalar arm */
    ORC_STAT_GROUP_BOUNDARY = 16  /* per boundary face: <p_f> <t_x> <t_y> <t_z> <shear_mag> (OrcBoundaryField 0..4) */
};
/* the cell fields, selected by bit (1 << value) of a mask; a pair XY is ordered: x = the first letter's field, y = the second's */
enum OrcStatField { ORC_STAT_U = 0, ORC_STAT_V, ORC_STAT_W, ORC_STAT_P,
                    ORC_STAT_UU, ORC_STAT_VV, ORC_STAT_WW, ORC_STAT_UV, ORC_STAT_UW, ORC_STAT_VW, ORC_STAT_PP,
                    ORC_STAT_MU, ORC_STAT_PHI, ORC_STAT_PHIPHI, ORC_STAT_UPHI, ORC_STAT_VPHI, ORC_STAT_WPHI,
                    ORC_STAT_N /* 17 */ };
enum OrcStatForm { ORC_STAT_RAW = 0 /* means and weighted co-moment sums C */, ORC_STAT_NORMALISED = 1 /* means and C / W */ };
#define ORC_STAT_BOUNDARY_N 5 /* boundary means per face: ORC_BOUNDARY_PRESSURE .. ORC_BOUNDARY_SHEAR_MAG */
typedef struct OrcTimeStatistics {
    uint32_t groups;      /* OrcStatGroup bits; MEAN must be set */
    int32_t reserved0;    /* 0 */
    uint64_t start_step;  /* orc_solver_advance samples from this step on (steps counted since the arm was enabled, first = 1) */
    uint64_t interval;    /* >= 1: every interval-th step from start_step */
} OrcTimeStatistics;      /* 24 bytes */

/* Point probes (new-build extension; orc_amd.h: orc_probes_create, orc_solver_sample_probes): a point is located by the owned cell with
 * the nearest centroid (smallest s = (r.x r.x + r.y r.y) + r.z r.z, r = x - x_P; the smallest ORC cell id among exact ties) followed by
 * a walk: at cell P the face f of its face list with the largest g_f = (r.x n.x + r.y n.y) + r.z n.z, r = x - x_f, the sign turned
 * where P is not the face's first cell (the first face among exact ties), decides — g <= 0: INSIDE P; a boundary face: OUTSIDE, left
 * through that face's zone; else on to the cell across, at most ORC_PROBE_WALK_LIMIT times.  DESIGN.md §3 "Point probes" fixes the
 * operator order. */
enum OrcProbeStatus {
    ORC_PROBE_STATUS_INSIDE = 0,     /* every face of the cell has g <= 0 */
    ORC_PROBE_STATUS_OUTSIDE = 1,    /* the walk left the mesh through a boundary face of the cell */
    ORC_PROBE_STATUS_WALK_LIMIT = 2  /* ORC_PROBE_WALK_LIMIT moves made and the cell reached still has an interior face with g > 0 */
};
#define ORC_PROBE_WALK_LIMIT 64 /* moves of a walk */
/* the sampled fields, selected by bit (1 << value) of a mask */
enum OrcProbeField { ORC_PROBE_U = 0, ORC_PROBE_V, ORC_PROBE_W, ORC_PROBE_P,
                     ORC_PROBE_PHI, /* the scalar arm's field; needs the arm */
                     ORC_PROBE_MU,  /* the viscosity the last assembly used (the constant while the viscosity arm is off) */
                     ORC_PROBE_N /* 6 */ };
enum OrcProbeInterpolation {
    ORC_PROBE_CELL = 0,  /* the value of the cell */
    ORC_PROBE_LINEAR = 1 /* u, v, w, p: phi_P + ((G.x r.x + G.y r.y) + G.z r.z), G the cell's gradient of the solver's
                            gradient_reconstruction (a row of orc_calculate_gradients, bit for bit), r = x - x_P; PHI and MU: the cell's */
};

/* Volume reports (new-build extension; orc_amd.h: orc_cell_groups_create, orc_solver_group_report): per group g of a cell group set and
 * per field x, with the weight w of a cell, t1 = w * x and t2 = t1 * x (separate multiplies): SUM = sum t1, SUM_SQ = sum t2, MIN, MAX
 * and the cells where the extrema occur; per group W = sum w and the number of cells.  A NaN never wins a comparison; among equal
 * values the smallest ORC cell id wins; a group without a cell, or with NaN only, gives +inf, -inf and the cell -1.  DESIGN.md §3
 * "Volume reports" fixes the association of the sums. */
enum OrcGroupQuantity { ORC_GROUP_SUM = 0, ORC_GROUP_SUM_SQ = 1, ORC_GROUP_MIN = 2, ORC_GROUP_MAX = 3, ORC_GROUP_N /* 4 */ };
enum OrcGroupWeighting {
    ORC_GROUP_WEIGHT_VOLUME = 0, /* w = the mesh's stored cell volume */
    ORC_GROUP_WEIGHT_UNIT = 1    /* w = 1.0 */
};
#define ORC_GROUP_MAX_GROUPS (1 << 20) /* groups of one set */
#define ORC_GROUP_MAX_FIELDS 64        /* fields of one orc_group_integrals call */

/* Tracer particles (new-build extension; orc_amd.h: orc_tracers_create, orc_solver_advect_tracers): massless particles moved through
 * the cells in the solver's velocity.  A substep of an ACTIVE particle at (x, P): U1 = velocity(x, P); h = direction step (TIME) or
 * (direction step) / |U1| (LENGTH; STAGNANT unless |U1| > min_speed); EULER xn = x + h U1, RK2 xm = x + (0.5 h) U1, U2 at xm in the
 * cell the probes' walk reaches from P, xn = x + h U2; the walk from there to xn accepts the substep (INSIDE) or stops the particle at
 * its last accepted position (LEFT through a boundary face's zone, or WALK_LIMIT).  DESIGN.md §3 "Tracer particles" fixes the operator
 * order. */
enum OrcTracerStatus {
    ORC_TRACER_ACTIVE = 0,     /* moves */
    ORC_TRACER_LEFT = 1,       /* a stage walk ended at a boundary face: zone tells which; position and cell are the last accepted ones */
    ORC_TRACER_WALK_LIMIT = 2, /* a stage walk made ORC_PROBE_WALK_LIMIT moves without finding the cell */
    ORC_TRACER_STAGNANT = 3    /* LENGTH mode: the speed at the particle is not above min_speed (or is NaN) */
};
enum OrcTracerScheme { ORC_TRACER_EULER = 0, ORC_TRACER_RK2 = 1 /* midpoint */ };
enum OrcTracerStepMode { ORC_TRACER_STEP_TIME = 0 /* h = direction step */, ORC_TRACER_STEP_LENGTH = 1 /* |xn - x| about step */ };
typedef struct OrcTracerSettings {
    int32_t scheme;        /* OrcTracerScheme */
    int32_t interpolation; /* OrcProbeInterpolation */
    int32_t step_mode;     /* OrcTracerStepMode */
    int32_t direction;     /* +1 with the flow, -1 against it */
    double step;           /* > 0: a time (TIME) or a length (LENGTH) */
    double min_speed;      /* >= 0, LENGTH only */
} OrcTracerSettings;       /* 32 bytes */

/* Cut surfaces (new-build extension; orc_amd.h: orc_cut_plane, orc_cut_node_level, orc_cut_cell_field, orc_solver_cut_field): the
 * polygons in which a level set of a node function d cuts the cells.  DESIGN.md §3 "Cut surfaces" fixes every rule. */
#define ORC_CUT_MAX_POINTS 32 /* cut points one cell may carry; a cell with more is skipped and counted (OVERFLOW) */
enum OrcCutSkip {
    ORC_CUT_SKIP_NONFINITE = 0, /* a node of the cell has a d that is not finite */
    ORC_CUT_SKIP_OVERFLOW = 1   /* more than ORC_CUT_MAX_POINTS cut points */
};

#ifdef __cplusplus
}
#endif
#endif /* ORC_TYPES_H */
