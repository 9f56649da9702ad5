"""settings::* of the reference (src/lib.rs:8-202) as plain values for the C ABI."""
import ctypes as C

from ._lib import lib


class NumericalSettings(C.Structure):
    """NumericalSettings + MatrixSolverSettings (lib.rs:14-56) flattened = OrcSettings."""
    _fields_ = [
        ("momentum", C.c_int32), ("diffusion", C.c_int32), ("pressure_interpolation", C.c_int32),
        ("velocity_interpolation", C.c_int32), ("gradient_reconstruction", C.c_int32),
        ("solver_type", C.c_int32), ("preconditioner", C.c_int32), ("q1_compat", C.c_int32),
        ("iterations", C.c_uint64), ("momentum_relaxation", C.c_double), ("pressure_relaxation", C.c_double),
        ("relaxation", C.c_double), ("relative_convergence_threshold", C.c_double),
        ("frozen_diagonals", C.c_int32), ("breakdown_guard", C.c_int32),
        ("reduction_order", C.c_int32), ("gmres_restart", C.c_int32),
    ]

    @classmethod
    def default(cls, **overrides):
        """NumericalSettings::default() (lib.rs:58-86), struct-update style overrides."""
        s = cls()
        lib().orc_settings_default(C.byref(s))
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class MomentumDiscretization:  # lib.rs:95-118
    UD, CD1, CD2, TVD_LUD, TVD_QUICK, TVD_UMIST, TVD_UD, TVD_CD1 = range(8)


class PressureInterpolation:  # lib.rs:125-133
    Linear, LinearWeighted, Standard, SecondOrder, NoInterpolation = range(5)


class VelocityInterpolation:  # lib.rs:135-146
    Linear, LinearWeighted, RhieChow, NoInterpolation = range(4)


class SolutionMethod:  # lib.rs:171-179 (+ new-build extensions)
    GaussSeidel, Jacobi, Multigrid, BiCGSTAB = range(4)
    MulticolorGS, BiCGSTAB_GS, Multigrid_GS = 16, 17, 18
    GMRES = 19
    CG = 20  # preconditioned conjugate gradients: symmetric positive definite systems (the pressure correction)


class ReductionOrder:  # include/orc_types.h OrcReductionOrder
    Tree, Reference = 0, 1


class PreconditionMethod:  # lib.rs:181-185
    NoPreconditioner, Jacobi = 0, 1


class FaceConditionTypes:  # mesh.rs:25-65
    Interior, Wall, PressureInlet, PressureOutlet, Symmetry, VelocityInlet = 2, 3, 4, 5, 7, 10


class LinearSolver(C.Structure):
    """OrcLinearSolver: a linear solver of its own for one system (Solver.set_pressure_solver)."""
    _fields_ = [
        ("solver_type", C.c_int32), ("preconditioner", C.c_int32), ("iterations", C.c_uint64),
        ("relative_convergence_threshold", C.c_double), ("relaxation", C.c_double),
    ]


class Convergence(C.Structure):
    """OrcConvergence: the stopping rule of Solver.iterate_until / solve_steady_converged — converged when each scaled residual
    (record slots 16..19: u, v, w, continuity) is <= its tolerance; a tolerance of 0 is never met."""
    _fields_ = [
        ("momentum_tolerance", C.c_double * 3), ("continuity_tolerance", C.c_double), ("min_iterations", C.c_uint64),
        ("reserved0", C.c_int32),
    ]

    @classmethod
    def make(cls, momentum=1e-4, continuity=1e-4, min_iterations=0):
        """momentum: one tolerance for u, v, w or three of them"""
        m = [float(momentum)] * 3 if not hasattr(momentum, "__len__") else [float(x) for x in momentum]
        return cls(momentum_tolerance=(C.c_double * 3)(*m), continuity_tolerance=float(continuity), min_iterations=int(min_iterations),
                   reserved0=0)


class TimeScheme:  # include/orc_types.h OrcTimeScheme
    Euler, BDF2 = 0, 1


class Transient(C.Structure):
    """OrcTransient: implicit time stepping (Solver.set_transient, solve_transient); dt is the step, the first one under a TimeStepControl."""
    _fields_ = [
        ("dt", C.c_double), ("scheme", C.c_int32), ("reserved0", C.c_int32),
        ("inner_iterations", C.c_uint64), ("inner_tolerance", C.c_double),
    ]

    @classmethod
    def make(cls, dt, scheme=TimeScheme.Euler, inner_iterations=20, inner_tolerance=0.0):
        return cls(dt=dt, scheme=scheme, reserved0=0, inner_iterations=inner_iterations, inner_tolerance=inner_tolerance)


class TimeStepControl(C.Structure):
    """OrcTimeStepControl: the rule by which Solver.advance chooses the next step from the largest convective rate
    (Solver.set_time_step_control, solver.time_step_next): want = target_courant / rate_max, held inside
    [dt * max_shrink, dt * max_growth] and then inside [dt_min, dt_max], chosen anew after every interval-th step."""
    _fields_ = [
        ("target_courant", C.c_double), ("dt_min", C.c_double), ("dt_max", C.c_double), ("max_growth", C.c_double),
        ("max_shrink", C.c_double), ("interval", C.c_uint64), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
    ]

    @classmethod
    def make(cls, target_courant=None, dt_min=None, dt_max=None, **overrides):
        """orc_time_step_control_default with the given fields replaced"""
        from ._lib import lib
        c = cls()
        lib().orc_time_step_control_default(C.byref(c))
        given = dict(overrides, target_courant=target_courant, dt_min=dt_min, dt_max=dt_max)
        for k, v in given.items():
            if v is None:
                continue
            if k not in dict(cls._fields_):
                raise TypeError("TimeStepControl has no field %r" % k)
            setattr(c, k, v)
        return c


class ScalarBc:  # include/orc_types.h OrcScalarBc
    DEFAULT, VALUE, FLUX, ZERO_GRADIENT = 0, 1, 2, 3


class ScalarSettings(C.Structure):
    """OrcScalarSettings: passive scalar transport on the solver's flow (Solver.set_scalar)."""
    _fields_ = [
        ("diffusivity", C.c_double), ("scheme", C.c_int32), ("solver_type", C.c_int32), ("preconditioner", C.c_int32),
        ("reserved0", C.c_int32), ("iterations", C.c_uint64), ("relative_convergence_threshold", C.c_double),
        ("relaxation", C.c_double), ("outer_iterations", C.c_uint64), ("outer_tolerance", C.c_double),
    ]

    @classmethod
    def default(cls, **overrides):
        """orc_scalar_settings_default (UD, BiCGSTAB + Jacobi, 500 iterations, 1e-10, outer 30 / 1e-8, Gamma 1e-3) with overrides"""
        s = cls()
        lib().orc_scalar_settings_default(C.byref(s))
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class ViscosityModel:  # include/orc_types.h OrcViscosityModel
    FIELD, POWER_LAW, CARREAU, SMAGORINSKY = 1, 2, 3, 4


class ViscosityFace:  # include/orc_types.h OrcViscosityFace
    ARITHMETIC, HARMONIC = 0, 1


class Viscosity(C.Structure):
    """OrcViscosity: a per-cell viscosity in the momentum diffusion (Solver.set_viscosity) — a prescribed field or a law of the
    strain-rate magnitude g: POWER_LAW k g^(n-1), CARREAU mu_inf + (mu_zero - mu_inf) (1 + (lambda g)^2)^((n-1)/2), SMAGORINSKY
    mu + rho (cs V^(1/3))^2 g; every law clamped to [mu_min, mu_max] and under-relaxed with `relaxation`."""
    _fields_ = [
        ("model", C.c_int32), ("face_interpolation", C.c_int32), ("k", C.c_double), ("n", C.c_double),
        ("mu_zero", C.c_double), ("mu_inf", C.c_double), ("lambda_", C.c_double), ("cs", C.c_double),
        ("mu_min", C.c_double), ("mu_max", C.c_double), ("relaxation", C.c_double),
    ]

    @classmethod
    def make(cls, model, face_interpolation=ViscosityFace.ARITHMETIC, **overrides):
        """orc_viscosity_default (power law with n = 1, clamp 1e-12 .. 1e12, no relaxation) with the model, the face interpolation and
        any other field overridden; `lambda_` is the struct's lambda"""
        s = cls()
        lib().orc_viscosity_default(C.byref(s))
        s.model, s.face_interpolation = int(model), int(face_interpolation)
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class ScalarDiffusivityModel:  # include/orc_types.h OrcScalarDiffusivityModel
    CONSTANT, FIELD, EDDY, LINEAR = 0, 1, 2, 3


class ScalarDiffusivity(C.Structure):
    """OrcScalarDiffusivity: a per-cell Gamma in the scalar's diffusion (Solver.set_scalar_diffusivity) — FIELD the data of
    Solver.set_scalar_diffusivity_field; EDDY gamma0 + max(mu_c - mu, 0) / schmidt_t on the viscosity arm's field; LINEAR
    gamma0 (1 + beta (phi - phi_ref)); EDDY and LINEAR clamped to [gamma_min, gamma_max].  gamma0 is ScalarSettings.diffusivity."""
    _fields_ = [
        ("model", C.c_int32), ("face_interpolation", C.c_int32), ("schmidt_t", C.c_double), ("beta", C.c_double),
        ("phi_ref", C.c_double), ("gamma_min", C.c_double), ("gamma_max", C.c_double), ("reserved0", C.c_double),
    ]

    @classmethod
    def make(cls, model, face_interpolation=ViscosityFace.ARITHMETIC, **overrides):
        """orc_scalar_diffusivity_default (schmidt_t 0.7, beta 0, phi_ref 0, clamp 1e-12 .. 1e12) with the model, the face
        interpolation (a ViscosityFace) and any other field overridden"""
        s = cls()
        lib().orc_scalar_diffusivity_default(C.byref(s))
        s.model, s.face_interpolation = int(model), int(face_interpolation)
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class WallDampingMode:  # include/orc_types.h OrcWallDampingMode
    NONE, MIN, VAN_DRIEST = 0, 1, 2


class WallDamping(C.Structure):
    """OrcWallDamping: wall damping of the Smagorinsky length l0 = cs V^(1/3) with the wall distance d (Solver.set_wall_damping) —
    MIN l = min(kappa d, l0); VAN_DRIEST l = l0 (1 - exp(-y+ / a_plus)), y+ = rho u_tau d / mu with the caller's friction velocity."""
    _fields_ = [("mode", C.c_int32), ("reserved0", C.c_int32), ("kappa", C.c_double), ("a_plus", C.c_double), ("u_tau", C.c_double)]

    @classmethod
    def make(cls, mode, **overrides):
        """orc_wall_damping_default (kappa 0.41, a_plus 26, u_tau 0) with the mode and any other field overridden"""
        s = cls()
        lib().orc_wall_damping_default(C.byref(s))
        s.mode = int(mode)
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


class StatGroup:  # include/orc_types.h OrcStatGroup (bits)
    MEAN, STRESS, VISCOSITY, SCALAR, BOUNDARY = 1, 2, 4, 8, 16
    ALL = 31


class StatForm:  # include/orc_types.h OrcStatForm
    RAW, NORMALISED = 0, 1


class TimeStatistics(C.Structure):
    """OrcTimeStatistics: running time means and co-moments of the fields (Solver.set_time_statistics) — `groups` is a sum of StatGroup
    bits (MEAN always); Solver.advance samples every `interval`-th step from `start_step` on (steps counted from 1 since the arm was
    enabled) with weight dt."""
    _fields_ = [("groups", C.c_uint32), ("reserved0", C.c_int32), ("start_step", C.c_uint64), ("interval", C.c_uint64)]

    @classmethod
    def make(cls, groups=None, start_step=1, interval=1):
        """orc_time_statistics_default (MEAN | STRESS, every step from the first) with the groups, start_step and interval overridden"""
        s = cls()
        lib().orc_time_statistics_default(C.byref(s))
        if groups is not None:
            s.groups = int(groups)
        s.start_step, s.interval = int(start_step), int(interval)
        return s


class ProbeStatus:  # include/orc_types.h OrcProbeStatus
    INSIDE, OUTSIDE, WALK_LIMIT = 0, 1, 2


class ProbeField:  # include/orc_types.h OrcProbeField (bit = 1 << value)
    U, V, W, P, PHI, MU = 0, 1, 2, 3, 4, 5
    N = 6


class ProbeInterpolation:  # include/orc_types.h OrcProbeInterpolation
    CELL, LINEAR = 0, 1


PROBE_WALK_LIMIT = 64  # include/orc_types.h ORC_PROBE_WALK_LIMIT: moves of a walk


class TracerStatus:  # include/orc_types.h OrcTracerStatus
    ACTIVE, LEFT, WALK_LIMIT, STAGNANT = 0, 1, 2, 3


class TracerScheme:  # include/orc_types.h OrcTracerScheme
    EULER, RK2 = 0, 1


class TracerStepMode:  # include/orc_types.h OrcTracerStepMode
    TIME, LENGTH = 0, 1


class TracerSettings(C.Structure):
    """OrcTracerSettings: how Solver.advect moves a Mesh.seed() set — scheme (TracerScheme), interpolation (ProbeInterpolation),
    step_mode (TracerStepMode: `step` is a time, or the length of a substep), direction (+1 with the flow, -1 against it), min_speed
    (LENGTH: a particle slower than this becomes STAGNANT)."""
    _fields_ = [("scheme", C.c_int32), ("interpolation", C.c_int32), ("step_mode", C.c_int32), ("direction", C.c_int32),
                ("step", C.c_double), ("min_speed", C.c_double)]

    @classmethod
    def make(cls, step=0.0, **overrides):
        """orc_tracer_settings_default (RK2, LINEAR, LENGTH, +1, min_speed 0) with the step and any other field overridden"""
        s = cls()
        lib().orc_tracer_settings_default(C.byref(s))
        s.step = float(step)
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s
