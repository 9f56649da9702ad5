"""solver::* of the reference (src/solver.rs) on MI355X."""
import ctypes as C

import numpy as np

from ._lib import OrcError, check, lib

_F64 = C.POINTER(C.c_double)
_REPORT_FN = C.CFUNCTYPE(None, C.c_uint64, _F64, _F64, C.c_double, C.c_double, C.c_double, C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_F64)


def solve_steady(mesh, u, v, w, p, numerical_settings, rho, mu, iteration_count, reporting_interval=0, report=None,
                 raise_on_error=True):
    """solver::solve_steady (solver.rs:26-37): u, v, w, p are updated in place.
    report(iteration, mean_velocity[3], peclet[3], velocity_correction, pressure_correction, ms_per_iter)."""
    for a in (u, v, w, p):
        assert a.dtype == np.float64 and a.flags.c_contiguous and len(a) == mesh.n_cells
    cb = None
    if report is not None:
        def _cb(it, mv, pe, vc, pc, ms, _user):
            report(it, (mv[0], mv[1], mv[2]), (pe[0], pe[1], pe[2]), vc, pc, ms)
        cb = _REPORT_FN(_cb)
    st = lib().orc_solve_steady(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.byref(numerical_settings), C.c_double(rho),
                                C.c_double(mu), C.c_uint64(iteration_count), C.c_uint64(reporting_interval),
                                cb if cb is not None else C.cast(None, _REPORT_FN), None)
    if raise_on_error:
        check(st)
    return st


# orc_types.h OrcResidual: the twenty doubles of a residual record (Solver.residual_history), by slot
RESIDUAL_NAMES = ("l1_u", "l1_v", "l1_w", "scale_u", "scale_v", "scale_w", "sq_u", "sq_v", "sq_w", "max_u", "max_v", "max_w",
                  "continuity_l1", "continuity_sq", "continuity_max", "continuity_scale", "scaled_u", "scaled_v", "scaled_w",
                  "scaled_continuity")
_RESIDUAL_N = len(RESIDUAL_NAMES)  # ORC_RESIDUAL_N


def convergence_check(convergence, record):
    """orc_convergence_check (host arithmetic, no device): (converged, failing_mask) of one residual record under a
    settings.Convergence; bit k of the mask = equation k (u, v, w, continuity) fails.  converged is -1 for an invalid rule."""
    rec = _f64(record).reshape(_RESIDUAL_N)
    mask = C.c_int32(0)
    ok = lib().orc_convergence_check(C.byref(convergence) if convergence is not None else None, _p(rec), C.byref(mask))
    return ok, mask.value


def solve_steady_converged(mesh, u, v, w, p, numerical_settings, rho, mu, convergence, max_iterations, reporting_interval=0,
                           report=None, raise_on_error=True):
    """orc_solve_steady_converged: solve_steady that stops once `convergence` (settings.Convergence) is met, after at most
    max_iterations; u, v, w, p are updated in place -> (status, iterations used, converged, last residual record)."""
    for a in (u, v, w, p):
        assert a.dtype == np.float64 and a.flags.c_contiguous and len(a) == mesh.n_cells
    cb = None
    if report is not None:
        def _cb(it, mv, pe, vc, pc, ms, _user):
            report(it, (mv[0], mv[1], mv[2]), (pe[0], pe[1], pe[2]), vc, pc, ms)
        cb = _REPORT_FN(_cb)
    done, conv, rec = C.c_uint64(0), C.c_int32(0), np.zeros(_RESIDUAL_N)
    st = lib().orc_solve_steady_converged(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.byref(numerical_settings), C.c_double(rho),
                                          C.c_double(mu), C.byref(convergence), C.c_uint64(max_iterations),
                                          C.c_uint64(reporting_interval), cb, None, C.byref(done), C.byref(conv), _p(rec))
    if raise_on_error:
        check(st)
    return st, int(done.value), bool(conv.value), rec


def time_step_next(control, dt, rate_max, raise_on_error=True):
    """orc_time_step_next (host arithmetic, no device): the step that follows `dt` under a settings.TimeStepControl when the largest
    convective rate is rate_max (with raise_on_error=False: (status, dt_next), dt_next None when refused)"""
    out = C.c_double(0.0)
    st = lib().orc_time_step_next(C.byref(control) if control is not None else None, C.c_double(dt), C.c_double(rate_max), C.byref(out))
    if raise_on_error:
        check(st)
        return out.value
    return st, (out.value if st == 0 else None)


def solve_transient(mesh, u, v, w, p, settings, rho, mu, transient, time_steps, reporting_interval=0, report=None,
                    raise_on_error=True, control=None):
    """Implicit time stepping (orc_solve_transient): time_steps steps of `transient` (settings.Transient) from u, v, w, p,
    updated in place.  report(step, mean_velocity[3], peclet[3], velocity_correction, pressure_correction, ms_per_step)
    with the last inner iteration's values.  control (settings.TimeStepControl): the steps after the first are chosen by it
    (Solver.set_time_step_control); the run then goes through a Solver, ms_per_step is 0 and the step history is returned
    next to the status."""
    for a in (u, v, w, p):
        assert a.dtype == np.float64 and a.flags.c_contiguous and len(a) == mesh.n_cells
    if control is not None:
        s = Solver(mesh, settings, rho, mu)
        s.set_fields(u, v, w, p)
        st = s.set_transient(transient, raise_on_error=raise_on_error)
        st = st or s.set_time_step_control(control, raise_on_error=raise_on_error)
        for k in range(1, time_steps + 1):
            if st != 0:
                break
            st, row = s.advance(1, report=True, raise_on_error=False)
            if raise_on_error:
                check(st)
            if st == 0 and report is not None and reporting_interval and k % reporting_interval == 0:
                report(k, tuple(row[0, 0:3]), tuple(row[0, 3:6]), row[0, 6], row[0, 7], 0.0)
        for dst, src in zip((u, v, w, p), s.get_fields()):
            dst[:] = src
        return st, s.time_step_history()
    cb = None
    if report is not None:
        def _cb(it, mv, pe, vc, pc, ms, _user):
            report(it, (mv[0], mv[1], mv[2]), (pe[0], pe[1], pe[2]), vc, pc, ms)
        cb = _REPORT_FN(_cb)
    st = lib().orc_solve_transient(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.byref(settings), C.c_double(rho), C.c_double(mu),
                                   C.byref(transient), C.c_uint64(time_steps), C.c_uint64(reporting_interval),
                                   cb if cb is not None else C.cast(None, _REPORT_FN), None)
    if raise_on_error:
        check(st)
    return st


def calculate_gradients(mesh, u, v, w, p, settings, velocity=True):
    """Green-Gauss arms of calculate_pressure_gradient / calculate_velocity_gradient for every cell."""
    n = mesh.n_cells
    gp = np.empty((n, 3))
    gu = np.empty((n, 3, 3)) if velocity else None
    u, v, w, p = map(_f64, (u, v, w, p))
    check(lib().orc_calculate_gradients(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.byref(settings), _p(gp),
                                        _p(gu) if velocity else None))
    return gp, gu


_SURFACE_N = 16  # orc_types.h ORC_SURFACE_N


class SurfaceReport:
    """Per-zone surface sums (orc_solver_surface_report / orc_surface_integrals): `raw` is the (Z, 16) array in the order of
    OrcSurfaceQuantity; the properties are views of it.  Forces and the moment are what the fluid exerts ON the boundary; a
    positive mass flow leaves the domain."""

    def __init__(self, raw, zone_names=None):
        self.raw = np.asarray(raw, dtype=np.float64).reshape(-1, _SURFACE_N)
        self.zone_names = list(zone_names) if zone_names is not None else None

    area = property(lambda self: self.raw[:, 0])
    mass_flow = property(lambda self: self.raw[:, 1])
    pressure_force = property(lambda self: self.raw[:, 2:5])
    viscous_force = property(lambda self: self.raw[:, 5:8])
    momentum_flow = property(lambda self: self.raw[:, 8:11])
    moment = property(lambda self: self.raw[:, 11:14])
    faces = property(lambda self: self.raw[:, 15])

    @property
    def force(self):
        """pressure plus viscous force, (Z, 3)"""
        return self.raw[:, 2:5] + self.raw[:, 5:8]

    @property
    def mean_pressure(self):
        """area-weighted mean of the face pressure; NaN where the zone has no area"""
        a = self.raw[:, 0]
        out = np.full(len(a), np.nan)
        np.divide(self.raw[:, 14], a, out=out, where=a != 0.0)
        return out

    def zone(self, name):
        """the 16 sums of the zone called `name` (needs a mesh whose arrays carry zone_names)"""
        if self.zone_names is None:
            raise KeyError("the mesh arrays carry no zone_names")
        return self.raw[self.zone_names.index(name)]


def _origin(origin):
    if origin is None:
        return None, None
    o = _f64(origin).reshape(3)
    return o, _p(o)


def surface_integrals(mesh, u, v, w, p, rho, mu, origin=None, raise_on_error=True):
    """orc_surface_integrals: the surface report of host fields in ORC cell order (with raise_on_error=False: (status, report))"""
    u, v, w, p = map(_f64, (u, v, w, p))
    for a in (u, v, w, p):
        assert len(a) == mesh.n_cells
    out = np.zeros((len(mesh.arrays["zone_type"]), _SURFACE_N))
    keep, o = _origin(origin)
    st = lib().orc_surface_integrals(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.c_double(rho), C.c_double(mu), o, _p(out))
    rep = SurfaceReport(out, mesh.arrays.get("zone_names"))
    if raise_on_error:
        check(st)
        return rep
    return st, rep


# ------------------------------------------------------------------ derived fields and boundary-face maps (orc_types.h)
DERIVED_NAMES = ("vorticity_x", "vorticity_y", "vorticity_z", "vorticity_mag", "strain_rate_mag", "q_criterion", "divergence",
                 "convective_rate")  # OrcDerivedField, by value
BOUNDARY_NAMES = ("pressure", "traction_x", "traction_y", "traction_z", "shear_mag", "y_plus", "mass_flux", "area")  # OrcBoundaryField


def _mask_of(names_or_mask, table, groups=()):
    """(mask, the names asked for) of a bit mask, one name or a list of names; `groups` maps a name to several fields"""
    if isinstance(names_or_mask, (int, np.integer)):
        mask = int(names_or_mask)
        return mask, [n for k, n in enumerate(table) if mask >> k & 1]
    names = [names_or_mask] if isinstance(names_or_mask, str) else list(names_or_mask)
    mask = 0
    for name in names:
        for part in dict(groups).get(name, (name,)):
            if part not in table:
                raise KeyError("unknown field '%s'; known: %s" % (name, ", ".join(table + tuple(dict(groups)))))
            mask |= 1 << table.index(part)
    return mask, names


_VORTICITY = (("vorticity", ("vorticity_x", "vorticity_y", "vorticity_z")),)


def _derived_dict(out, mask, names, n):
    """the SoA block of the selected fields -> {name: ndarray[n]}, 'vorticity' -> (n, 3)"""
    rows = {DERIVED_NAMES[k]: out[i] for i, k in enumerate(k for k in range(len(DERIVED_NAMES)) if mask >> k & 1)}
    res = {}
    for name in names:
        res[name] = np.stack([rows[c] for c in _VORTICITY[0][1]], axis=1) if name == "vorticity" else rows[name]
    return res


def derived_fields(mesh, u, v, w, settings, names, raise_on_error=True):
    """orc_derived_fields: derived cell fields (DERIVED_NAMES, 'vorticity' = (n, 3), or a bit mask) of host fields in ORC cell
    order, from the velocity gradient of settings.gradient_reconstruction -> {name: ndarray} (raise_on_error=False: (status, dict))"""
    u, v, w = map(_f64, (u, v, w))
    for a in (u, v, w):
        assert len(a) == mesh.n_cells
    mask, names = _mask_of(names, DERIVED_NAMES, _VORTICITY)
    out = np.zeros((max(bin(mask).count("1"), 1), mesh.n_cells))
    st = lib().orc_derived_fields(mesh.ptr, _p(u), _p(v), _p(w), C.byref(settings), C.c_uint32(mask & 0xFFFFFFFF), _p(out))
    if raise_on_error:
        check(st)
        return _derived_dict(out, mask, names, mesh.n_cells)
    return st, (_derived_dict(out, mask, names, mesh.n_cells) if st == 0 else {})


class BoundaryFields:
    """Boundary-face maps (orc_solver_boundary_fields / orc_boundary_fields): one value per boundary face of an owned cell in the
    order of Mesh.boundary_index() — `zone_ptr` [Z + 1], `faces` (internal face numbering), `arrays` {name: ndarray[nb]}."""

    def __init__(self, zone_ptr, faces, arrays, zone_names=None):
        self.zone_ptr, self.faces, self.arrays = zone_ptr, faces, arrays
        self.zone_names = list(zone_names) if zone_names is not None else None

    def __getitem__(self, name):
        return self.arrays[name]

    def zone(self, name):
        """{field: the slice of the zone called `name` (or with index `name`)}"""
        if isinstance(name, str):
            if self.zone_names is None:
                raise KeyError("the mesh arrays carry no zone_names")
            name = self.zone_names.index(name)
        lo, hi = int(self.zone_ptr[name]), int(self.zone_ptr[name + 1])
        return {k: a[lo:hi] for k, a in self.arrays.items()}


def _boundary_result(mesh, out, mask, names):
    zp, faces, _, _ = mesh.boundary_index()
    rows = {BOUNDARY_NAMES[k]: out[i] for i, k in enumerate(k for k in range(len(BOUNDARY_NAMES)) if mask >> k & 1)}
    return BoundaryFields(zp, faces, {name: rows[name] for name in names}, mesh.arrays.get("zone_names"))


def boundary_fields(mesh, u, v, w, p, rho, mu, names=BOUNDARY_NAMES, raise_on_error=True):
    """orc_boundary_fields: the boundary-face maps (BOUNDARY_NAMES or a bit mask) of host fields in ORC cell order ->
    BoundaryFields (raise_on_error=False: (status, BoundaryFields or None))"""
    u, v, w, p = map(_f64, (u, v, w, p))
    for a in (u, v, w, p):
        assert len(a) == mesh.n_cells
    mask, names = _mask_of(names, BOUNDARY_NAMES)
    nb = int(mesh.boundary_index()[0][-1])
    out = np.zeros((max(bin(mask).count("1"), 1), nb))
    st = lib().orc_boundary_fields(mesh.ptr, _p(u), _p(v), _p(w), _p(p), C.c_double(rho), C.c_double(mu), C.c_uint32(mask & 0xFFFFFFFF),
                                   _p(out))
    if raise_on_error:
        check(st)
        return _boundary_result(mesh, out, mask, names)
    return st, (_boundary_result(mesh, out, mask, names) if st == 0 else None)


# orc_types.h OrcStatField, by value: running means of the fields and co-moments of their fluctuations (Solver.statistics)
STATISTIC_NAMES = ("u", "v", "w", "p", "uu", "vv", "ww", "uv", "uw", "vw", "pp", "mu", "phi", "phiphi", "uphi", "vphi", "wphi")
STAT_BOUNDARY_NAMES = BOUNDARY_NAMES[:5]  # the boundary maps whose running means the BOUNDARY group keeps
_STAT_MEAN, _STAT_STRESS, _STAT_SCALAR = STATISTIC_NAMES[:4], STATISTIC_NAMES[4:11], STATISTIC_NAMES[12:]


# orc_types.h OrcProbeField, by value: what Solver.sample and the probe history read at a point
PROBE_NAMES = ("u", "v", "w", "p", "phi", "mu")


def _interpolation(x):
    """'cell' / 'linear' or a settings.ProbeInterpolation value -> the value"""
    return {"cell": 0, "linear": 1}[x.lower()] if isinstance(x, str) else int(x)


def _probe_rows(out, mask, names):
    order = [i for i in range(len(PROBE_NAMES)) if mask >> i & 1]
    rows = {PROBE_NAMES[f]: out[q] for q, f in enumerate(order)}
    return {name: rows[name] for name in names}


_I64 = C.POINTER(C.c_int64)
_GROUP_N = 4  # orc_types.h ORC_GROUP_N: SUM, SUM_SQ, MIN, MAX
GROUP_WEIGHTINGS = ("volume", "unit")  # orc_types.h OrcGroupWeighting, by value


def _weighting(x):
    """'volume' / 'unit' or an OrcGroupWeighting value -> the value"""
    if isinstance(x, str):
        if x.lower() not in GROUP_WEIGHTINGS:
            raise KeyError("unknown weighting '%s'; known: %s" % (x, ", ".join(GROUP_WEIGHTINGS)))
        return GROUP_WEIGHTINGS.index(x.lower())
    return int(x)


def _group_out(G, F):
    return np.zeros((max(G, 1), max(F, 1), _GROUP_N)), np.zeros((max(G, 1), 2)), np.zeros((max(G, 1), max(F, 1), 2), np.int64)


class GroupReport:
    """A volume report (orc_solver_group_report and its relatives): per group g and field f (`names`, the columns)
        weight [G] = W = sum w, count [G]; sum [G, F] = sum (w x), sum_sq = sum ((w x) x), min, max, argmin, argmax (ORC cell ids, -1
        where the group holds no cell or NaN only)
    and derived on the host: mean = sum / W, variance = sum_sq / W - mean^2, rms = sqrt(sum_sq / W); NaN where W is 0."""

    def __init__(self, names, sums, weight, where):
        self.names = list(names)
        G, F = np.asarray(weight).reshape(-1, 2).shape[0], len(self.names)
        self.raw = np.asarray(sums, dtype=np.float64).reshape(G, -1, _GROUP_N)[:, :F]
        self.where = np.asarray(where, dtype=np.int64).reshape(G, -1, 2)[:, :F]
        w = np.asarray(weight, dtype=np.float64).reshape(G, 2)
        self.weight, self.count = w[:, 0].copy(), w[:, 1].astype(np.int64)

    sum = property(lambda self: self.raw[:, :, 0])
    sum_sq = property(lambda self: self.raw[:, :, 1])
    min = property(lambda self: self.raw[:, :, 2])
    max = property(lambda self: self.raw[:, :, 3])
    argmin = property(lambda self: self.where[:, :, 0])
    argmax = property(lambda self: self.where[:, :, 1])

    def _per_weight(self, a):
        out = np.full(a.shape, np.nan)
        w = np.broadcast_to(self.weight[:, None], a.shape)
        np.divide(a, w, out=out, where=w != 0.0)
        return out

    @property
    def mean(self):
        return self._per_weight(self.sum)

    @property
    def variance(self):
        m = self.mean
        return self._per_weight(self.sum_sq) - m * m

    @property
    def rms(self):
        q = self._per_weight(self.sum_sq)
        with np.errstate(invalid="ignore"):
            return np.sqrt(q)

    def column(self, name):
        """the column index of the field called `name`"""
        return self.names.index(name)


def group_integrals(mesh, groups, fields, weighting="volume", raise_on_error=True):
    """orc_group_integrals: the volume report of caller fields {name: ndarray[n_cells]} in ORC cell order (a file's data, derived
    fields, a product of two fields) -> GroupReport, columns in the dict's order (raise_on_error=False: (status, report or None))"""
    names = list(fields.keys())
    block = np.ascontiguousarray(np.stack([_f64(fields[k]).reshape(-1) for k in names]) if names else np.zeros((0, mesh.n_cells)))
    if block.shape[1] != mesh.n_cells:
        raise ValueError("group integrals: a field holds %d values, the mesh %d cells" % (block.shape[1], mesh.n_cells))
    G = len(groups) if groups is not None else 0
    sums, weight, where = _group_out(G, len(names))
    st = lib().orc_group_integrals(mesh.ptr, groups.ptr if groups is not None else None, C.c_int32(len(names)), _p(block),
                                   C.c_int32(_weighting(weighting)), _p(sums), _p(weight), where.ctypes.data_as(_I64))
    if raise_on_error:
        check(st)
        return GroupReport(names, sums, weight, where)
    return st, (GroupReport(names, sums, weight, where) if st == 0 else None)


class Solver:
    """Device-resident state of one solve_steady call (OrcSolver*): what bench.py drives."""

    def __init__(self, mesh, settings, rho, mu):
        st = C.c_int(0)
        self.mesh = mesh
        self.ptr = lib().orc_solver_create(mesh.ptr, C.byref(settings), C.c_double(rho), C.c_double(mu), C.byref(st))
        check(st.value)
        self.ptr = C.c_void_p(self.ptr)
        self.n = mesh.n_cells
        self.rho, self.mu = float(rho), float(mu)
        self._stat_groups = 0

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_solver_destroy(self.ptr)
            self.ptr = None

    def set_fields(self, u, v, w, p):
        u, v, w, p = map(_f64, (u, v, w, p))
        check(lib().orc_solver_set_fields(self.ptr, _p(u), _p(v), _p(w), _p(p)))

    def get_fields(self):
        u, v, w, p = (np.empty(self.n) for _ in range(4))
        check(lib().orc_solver_get_fields(self.ptr, _p(u), _p(v), _p(w), _p(p)))
        return u, v, w, p

    def iterate(self, iterations=1, report=False, raise_on_error=True):
        rep = np.zeros((iterations, 8)) if report else None
        st = lib().orc_solver_iterate(self.ptr, C.c_uint64(iterations), _p(rep) if report else None)
        if raise_on_error:
            check(st)
        return (st, rep) if report else st

    # ---------------------------------------------------------------- residual monitors (orc_solver_set_monitors)
    def set_monitors(self, on=True, raise_on_error=True):
        """orc_solver_set_monitors: from now on every iterate() and every inner iteration of advance() appends one residual record;
        switching on clears the history and resets the continuity scale, switching off frees the monitor.  Reads only: fields and
        reports keep their bits.  On a partitioned mesh every rank switches the same way."""
        st = lib().orc_solver_set_monitors(self.ptr, C.c_int32(1 if on else 0))
        if raise_on_error:
            check(st)
        return st

    def residual_history(self, first=0, count=None):
        """the residual records [first, first + count) -> an array (k, 20), columns as RESIDUAL_NAMES (count=None: all from first)"""
        have = int(lib().orc_solver_residual_count(self.ptr))
        if count is None:
            count = max(have - first, 0)
        out = np.zeros((count, _RESIDUAL_N))
        check(lib().orc_solver_residual_history(self.ptr, C.c_uint64(first), C.c_uint64(count), _p(out)))
        return out

    def iterate_until(self, max_iterations, convergence, report=False, raise_on_error=True):
        """orc_solver_iterate_until: SIMPLE iterations until `convergence` (settings.Convergence) is met, not before its
        min_iterations and at most max_iterations; needs set_monitors() -> (status, iterations done, converged), with report=True
        also the 8 report values of the last iteration"""
        rep = np.zeros(8) if report else None
        done, conv = C.c_uint64(0), C.c_int32(0)
        st = lib().orc_solver_iterate_until(self.ptr, C.c_uint64(max_iterations), C.byref(convergence) if convergence is not None else None,
                                            _p(rep) if report else None, C.byref(done), C.byref(conv))
        if raise_on_error:
            check(st)
        res = (st, int(done.value), bool(conv.value))
        return res + (rep,) if report else res

    def pressure_rhs(self):
        """orc_solver_get_pressure_rhs: the right-hand side of the pressure correction as the last iteration left it (the cell mass
        imbalance of its momentum solution), the mesh's internal cell order; assembles nothing"""
        b = np.zeros(self.n)
        check(lib().orc_solver_get_pressure_rhs(self.ptr, _p(b)))
        return b

    def set_transient(self, transient=None, raise_on_error=True):
        """orc_solver_set_transient: a settings.Transient turns implicit time stepping on (0 known levels), None turns it off"""
        st = lib().orc_solver_set_transient(self.ptr, C.byref(transient) if transient is not None else None)
        if raise_on_error:
            check(st)
        return st

    def set_time_levels(self, u_n, v_n, w_n, u_nm1=None, v_nm1=None, w_nm1=None, raise_on_error=True):
        """orc_solver_set_time_levels: the previous time levels of the step in progress, ORC cell order (n-1 optional)"""
        lv = [_f64(a) for a in (u_n, v_n, w_n)]
        old = [None if a is None else _f64(a) for a in (u_nm1, v_nm1, w_nm1)]
        st = lib().orc_solver_set_time_levels(self.ptr, *[_p(a) for a in lv], *[None if a is None else _p(a) for a in old])
        if raise_on_error:
            check(st)
        return st

    def advance(self, steps=1, report=False, raise_on_error=True):
        """orc_solver_advance: `steps` time steps.  report=True returns an array (steps, 10): the 8 values of iterate() for the
        last inner iteration, the inner iterations used, and the time reached (with raise_on_error=False: (status, array))."""
        rep = np.zeros((steps, 10)) if report else None
        st = lib().orc_solver_advance(self.ptr, C.c_uint64(steps), _p(rep) if report else None)
        if raise_on_error:
            check(st)
            return rep if report else st
        return (st, rep) if report else st

    # ---------------------------------------------------------------- adaptive time stepping (orc_amd.h "adaptive time stepping")
    def courant(self, field=False, raise_on_error=True):
        """orc_solver_courant: (rate_max, cell[, rate]) — the largest convective rate sum_f |U_f . n| A / (2 V) of the current fields
        (times dt: the Courant number), the smallest ORC id that attains it (-1 on a partitioned mesh) and, with field=True, the
        per-cell rates in ORC order from the same launch (with raise_on_error=False the status comes first)"""
        r, c = C.c_double(0.0), C.c_int64(-1)
        rate = np.zeros(self.n) if field else None
        st = lib().orc_solver_courant(self.ptr, C.byref(r), C.byref(c), _p(rate) if field else None)
        out = (r.value, int(c.value), rate) if field else (r.value, int(c.value))
        if raise_on_error:
            check(st)
            return out
        return (st,) + out

    def set_time_step(self, dt, raise_on_error=True):
        """orc_solver_set_time_step: the step the next advance() takes; levels, time and history are kept"""
        st = lib().orc_solver_set_time_step(self.ptr, C.c_double(dt))
        if raise_on_error:
            check(st)
        return st

    def set_time_step_control(self, control=None, raise_on_error=True):
        """orc_solver_set_time_step_control: a settings.TimeStepControl lets advance() choose its steps, None turns that off"""
        st = lib().orc_solver_set_time_step_control(self.ptr, C.byref(control) if control is not None else None)
        if raise_on_error:
            check(st)
        return st

    def time_state(self):
        """orc_solver_get_time_state: dict(time, dt_next, dt_last, dt_before_last)"""
        v = [C.c_double(0.0) for _ in range(4)]
        check(lib().orc_solver_get_time_state(self.ptr, *[C.byref(x) for x in v]))
        return dict(zip(("time", "dt_next", "dt_last", "dt_before_last"), (x.value for x in v)))

    def set_time_state(self, time, dt_last=None, dt_before_last=None, raise_on_error=True):
        """orc_solver_set_time_state: the clock and the steps that led to the levels of set_time_levels (a restart); a dict from
        time_state() is taken as well, its dt_next going to set_time_step"""
        if isinstance(time, dict):
            d = time
            st = lib().orc_solver_set_time_state(self.ptr, C.c_double(d["time"]), C.c_double(d["dt_last"]), C.c_double(d["dt_before_last"]))
            st = st or lib().orc_solver_set_time_step(self.ptr, C.c_double(d["dt_next"]))
        else:
            st = lib().orc_solver_set_time_state(self.ptr, C.c_double(time), C.c_double(dt_last),
                                                 C.c_double(dt_last if dt_before_last is None else dt_before_last))
        if raise_on_error:
            check(st)
        return st

    def time_step_history(self, first=0, count=None):
        """orc_solver_time_step_history: (k, 4) — time reached, dt used, rate_max at the step's end (NaN where it was not measured),
        cell — one row per step while control is on or a manual step has been set"""
        have = int(lib().orc_solver_time_step_count(self.ptr))
        count = have - first if count is None else count
        out = np.zeros((max(count, 0), 4))
        check(lib().orc_solver_time_step_history(self.ptr, C.c_uint64(first), C.c_uint64(count), _p(out)))
        return out

    def bench_courant(self, reps=50):
        """(ms of the Courant reduction, ms of derived_cell_k selecting the convective rate alone): HIP-event averages"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        check(lib().orc_bench_courant(self.ptr, C.c_int(reps), C.byref(a)))
        check(lib().orc_bench_derived_rate(self.ptr, C.c_int(reps), C.byref(b)))
        return a.value, b.value

    # ---------------------------------------------------------------- a linear solver of its own for p' (orc_solver_set_pressure_solver)
    def set_pressure_solver(self, solver_type=None, preconditioner=1, iterations=50, threshold=0.0, relaxation=0.5, raise_on_error=True):
        """the p' solves run with these five fields instead of the settings' (settings.SolutionMethod.CG: the pressure correction
        is symmetric positive definite); solver_type=None removes the override"""
        if solver_type is None:
            st = lib().orc_solver_set_pressure_solver(self.ptr, None)
        else:
            from .settings import LinearSolver
            c = LinearSolver(solver_type=int(solver_type), preconditioner=int(preconditioner), iterations=int(iterations),
                             relative_convergence_threshold=float(threshold), relaxation=float(relaxation))
            st = lib().orc_solver_set_pressure_solver(self.ptr, C.byref(c))
        if raise_on_error:
            check(st)
        return st

    def pressure_solver(self):
        """(enabled, dict of the five fields the p' solve runs with: the override's, or the settings' when none is set)"""
        from .settings import LinearSolver
        c, on = LinearSolver(), C.c_int32(0)
        check(lib().orc_solver_get_pressure_solver(self.ptr, C.byref(c), C.byref(on)))
        return bool(on.value), dict(solver_type=c.solver_type, preconditioner=c.preconditioner, iterations=c.iterations,
                                    threshold=c.relative_convergence_threshold, relaxation=c.relaxation)

    def debug_pressure_hierarchies(self):
        """test hook: p' Multigrid hierarchies this solver has set up so far (ahead of a solve or inside one)"""
        return int(lib().orc_solver_debug_pressure_hierarchies(self.ptr))

    # ---------------------------------------------------------------- passive scalar (orc_solver_set_scalar)
    def set_scalar(self, settings=None, raise_on_error=True):
        """a settings.ScalarSettings turns the scalar arm on (phi = 0, no source, no levels, every zone DEFAULT); None turns it off"""
        st = lib().orc_solver_set_scalar(self.ptr, C.byref(settings) if settings is not None else None)
        if raise_on_error:
            check(st)
        return st

    def set_scalar_bc(self, zone, kind, value=0.0, raise_on_error=True):
        """zone: index (orc_mesh_update_zones order) or name in the mesh's zone_names; kind: settings.ScalarBc"""
        if isinstance(zone, str):
            zone = list(self.mesh.arrays["zone_names"]).index(zone)
        st = lib().orc_solver_set_scalar_bc(self.ptr, C.c_int32(zone), C.c_int32(kind), C.c_double(value))
        if raise_on_error:
            check(st)
        return st

    def set_scalar_field(self, phi):
        phi = _f64(phi)
        check(lib().orc_solver_set_scalar_field(self.ptr, _p(phi)))

    def get_scalar_field(self):
        phi = np.empty(self.n)
        check(lib().orc_solver_get_scalar_field(self.ptr, _p(phi)))
        return phi

    def set_scalar_source(self, source=None):
        """source per unit volume in ORC cell order; None = no source"""
        src = None if source is None else _f64(source)
        check(lib().orc_solver_set_scalar_source(self.ptr, None if src is None else _p(src)))

    def set_scalar_levels(self, phi_n, phi_nm1=None, raise_on_error=True):
        """previous scalar levels (ORC cell order) of the step in progress; needs the transient and the scalar arm on"""
        a, b = _f64(phi_n), None if phi_nm1 is None else _f64(phi_nm1)
        st = lib().orc_solver_set_scalar_levels(self.ptr, _p(a), None if b is None else _p(b))
        if raise_on_error:
            check(st)
        return st

    def solve_scalar(self, raise_on_error=True):
        """one scalar solve -> [outer rounds used, last relative change, min phi, max phi] (with raise_on_error=False: (status, report))"""
        rep = np.zeros(4)
        st = lib().orc_solver_solve_scalar(self.ptr, _p(rep))
        if raise_on_error:
            check(st)
            return rep
        return st, rep

    def last_scalar_report(self):
        rep = np.zeros(4)
        check(lib().orc_solver_last_scalar_report(self.ptr, _p(rep)))
        return rep

    def assemble_scalar(self, raise_on_error=True):
        """(a in pattern order, b in the mesh's internal cell order) of the scalar system of the current state"""
        a, b = np.empty(self.mesh.nnz), np.zeros(self.n)
        st = lib().orc_solver_assemble_scalar(self.ptr, _p(a), _p(b))
        if raise_on_error:
            check(st)
            return a, b
        return st

    def scalar_boundary_flux(self):
        """per zone: the convective plus diffusive flux of phi into the domain"""
        out = np.zeros(len(self.mesh.arrays["zone_type"]))
        check(lib().orc_solver_scalar_boundary_flux(self.ptr, _p(out)))
        return out

    # ---------------------------------------------------------------- variable scalar diffusivity (orc_solver_set_scalar_diffusivity)
    def set_scalar_diffusivity(self, cfg=None, raise_on_error=True):
        """a settings.ScalarDiffusivity puts a per-cell Gamma into the scalar's diffusion (FIELD, EDDY on the viscosity arm's field,
        LINEAR in phi); None or model CONSTANT switches it off and puts the constant Gamma part back.  Needs set_scalar()."""
        st = lib().orc_solver_set_scalar_diffusivity(self.ptr, C.byref(cfg) if cfg is not None else None)
        if raise_on_error:
            check(st)
        return st

    def set_scalar_diffusivity_field(self, gamma, raise_on_error=True):
        """the FIELD model's data: one Gamma per cell (> 0, finite), cell order as set_scalar_field()"""
        gamma = _f64(gamma)
        st = lib().orc_solver_set_scalar_diffusivity_field(self.ptr, _p(gamma))
        if raise_on_error:
            check(st)
        return st

    def scalar_diffusivity(self):
        """Gamma per cell under the current state (the constant while no model is on), cell order as get_scalar_field()"""
        g = np.empty(self.n)
        check(lib().orc_solver_get_scalar_diffusivity(self.ptr, _p(g)))
        return g

    def bench_scalar_diffusivity(self, reps=50):
        """orc_bench_scalar_diffusivity: ms per launch of (scalar_diffusion_k, scalar_diffusion_var_k of the model that is on, the
        boundary-term pass scalar_face_var_k); needs set_scalar_diffusivity()"""
        ms = np.zeros(3)
        check(lib().orc_bench_scalar_diffusivity(self.ptr, C.c_int(reps), _p(ms)))
        return float(ms[0]), float(ms[1]), float(ms[2])

    # ---------------------------------------------------------------- variable viscosity (orc_solver_set_viscosity)
    def set_viscosity(self, v=None, raise_on_error=True):
        """a settings.Viscosity turns the per-cell viscosity on (evaluated on the current fields and a_di rebuilt at once, then ahead
        of every momentum assembly); None turns it off and puts the constant-mu diffusion matrix back"""
        st = lib().orc_solver_set_viscosity(self.ptr, C.byref(v) if v is not None else None)
        if raise_on_error:
            check(st)
        return st

    def set_wall_damping(self, w=None, raise_on_error=True):
        """a settings.WallDamping damps the Smagorinsky length with the wall distance of the zones of type Wall (in effect whenever the
        viscosity model is SMAGORINSKY; the field is re-evaluated at once if it is); None turns the damping off"""
        st = lib().orc_solver_set_wall_damping(self.ptr, C.byref(w) if w is not None else None)
        if raise_on_error:
            check(st)
        return st

    def wall_damping(self):
        """orc_solver_get_wall_damping -> (settings.WallDamping as stored, enabled)"""
        from .settings import WallDamping
        w, on = WallDamping(), C.c_int32(0)
        check(lib().orc_solver_get_wall_damping(self.ptr, C.byref(w), C.byref(on)))
        return w, bool(on.value)

    def set_viscosity_field(self, mu, raise_on_error=True):
        """the FIELD model's data: one viscosity per cell (> 0, finite), cell order as set_fields()"""
        mu = _f64(mu)
        st = lib().orc_solver_set_viscosity_field(self.ptr, _p(mu))
        if raise_on_error:
            check(st)
        return st

    def viscosity(self):
        """the viscosity field the last assembly used (the constant mu while the arm is off), cell order as get_fields()"""
        mu = np.empty(self.n)
        check(lib().orc_solver_get_viscosity(self.ptr, _p(mu)))
        return mu

    def evaluate_viscosity(self, raise_on_error=True):
        """the law on the current fields, no relaxation, no state change -> (mu, strain-rate magnitude)
        (raise_on_error=False: (status, mu, strain_rate))"""
        mu, g = np.zeros(self.n), np.zeros(self.n)
        st = lib().orc_solver_evaluate_viscosity(self.ptr, _p(mu), _p(g))
        if raise_on_error:
            check(st)
            return mu, g
        return st, mu, g

    def diffusion(self):
        """(a_di in the CSR order of the mesh pattern, b_u_di, b_v_di, b_w_di in the mesh's internal cell order): the diffusion
        matrix and wall terms the next momentum assembly reads"""
        a = np.empty(self.mesh.nnz)
        bu, bv, bw = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        check(lib().orc_solver_get_diffusion(self.ptr, _p(a), _p(bu), _p(bv), _p(bw)))
        return a, bu, bv, bw

    def bench_viscosity(self, reps=50):
        """orc_bench_viscosity: (ms per law pass viscosity_cell_k, ms per rebuild diffusion_var_k); needs set_viscosity()"""
        ms = np.zeros(2)
        check(lib().orc_bench_viscosity(self.ptr, C.c_int(reps), _p(ms)))
        return float(ms[0]), float(ms[1])

    # ---------------------------------------------------------------- running time statistics (orc_solver_set_time_statistics)
    def set_time_statistics(self, c=None, raise_on_error=True):
        """a settings.TimeStatistics turns the statistics arm on (zeroed accumulators, no samples, step counter 0): from then on
        advance() samples the steps that are due with weight dt; None turns it off and frees its buffers.  Reads only: fields and
        reports keep their bits.  On a partitioned mesh every rank enables the same groups."""
        st = lib().orc_solver_set_time_statistics(self.ptr, C.byref(c) if c is not None else None)
        if st == 0:
            self._stat_groups = int(c.groups) if c is not None else 0  # OrcStatGroup bits in force
        if raise_on_error:
            check(st)
        return st

    def sample_statistics(self, weight=1.0, raise_on_error=True):
        """one sample of the current state with `weight` (> 0): for steady runs that oscillate, or a schedule of the caller's own"""
        st = lib().orc_solver_sample_statistics(self.ptr, C.c_double(weight))
        if raise_on_error:
            check(st)
        return st

    def reset_statistics(self, raise_on_error=True):
        """accumulators, weight sum and sample count back to zero; the settings and the step counter are kept"""
        st = lib().orc_solver_reset_statistics(self.ptr)
        if raise_on_error:
            check(st)
        return st

    def statistics_info(self, raise_on_error=True):
        """dict(samples, weight_sum, n_fields, n_boundary_faces) (raise_on_error=False: (status, dict))"""
        ns, w, k, nb = C.c_uint64(0), C.c_double(0.0), C.c_int32(0), C.c_int64(0)
        st = lib().orc_solver_statistics_info(self.ptr, C.byref(ns), C.byref(w), C.byref(k), C.byref(nb))
        info = dict(samples=int(ns.value), weight_sum=w.value, n_fields=k.value, n_boundary_faces=int(nb.value))
        if raise_on_error:
            check(st)
            return info
        return st, info

    def statistics_fields(self):
        """the names (STATISTIC_NAMES) of the enabled cell fields, in the order of the accumulator buffer"""
        g = self._stat_groups
        return [n for n in STATISTIC_NAMES if n in _STAT_MEAN or (n in _STAT_STRESS and g & 2) or (n == "mu" and g & 4) or (n in _STAT_SCALAR and g & 8)]

    def statistics(self, names=None, normalised=True, raise_on_error=True):
        """orc_solver_get_statistics: {name: ndarray[n]} of the statistics `names` (STATISTIC_NAMES or a bit mask; None = every enabled
        field), cell order as get_fields() — the means, and the co-moments divided by the weight sum (normalised=False: the weighted
        co-moment sums themselves).  The dict serves as cell data of io.write_vtu.  (raise_on_error=False: (status, dict))"""
        if names is None:
            names = self.statistics_fields()
        mask, names = _mask_of(names, STATISTIC_NAMES)
        out = np.zeros((max(bin(mask).count("1"), 1), self.n))
        st = lib().orc_solver_get_statistics(self.ptr, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(1 if normalised else 0), _p(out))
        rows = {STATISTIC_NAMES[k]: out[i] for i, k in enumerate(k for k in range(len(STATISTIC_NAMES)) if mask >> k & 1)}
        if raise_on_error:
            check(st)
            return {name: rows[name] for name in names}
        return st, ({name: rows[name] for name in names} if st == 0 else {})

    def boundary_statistics(self, raise_on_error=True):
        """orc_solver_get_boundary_statistics: the running means of the boundary maps STAT_BOUNDARY_NAMES -> BoundaryFields (its
        zone_ptr and faces are Mesh.boundary_index()'s); needs the BOUNDARY group (raise_on_error=False: (status, BoundaryFields or None))"""
        nb = int(self.mesh.boundary_index()[0][-1])
        out = np.zeros((len(STAT_BOUNDARY_NAMES), max(nb, 1)))[:, :nb]
        out = np.ascontiguousarray(out)
        st = lib().orc_solver_get_boundary_statistics(self.ptr, _p(out))
        if raise_on_error:
            check(st)
        res = _boundary_result(self.mesh, out, (1 << len(STAT_BOUNDARY_NAMES)) - 1, list(STAT_BOUNDARY_NAMES)) if st == 0 else None
        return res if raise_on_error else (st, res)

    def statistics_state(self):
        """what a restart needs: dict(samples, weight_sum, names, raw (K, n): every enabled field, RAW form, boundary (5, nb) or None)"""
        info = self.statistics_info()
        names = self.statistics_fields()
        raw = self.statistics(names, normalised=False)
        state = dict(samples=info["samples"], weight_sum=info["weight_sum"], names=names, raw=np.stack([raw[n] for n in names]), boundary=None)
        if info["n_boundary_faces"] > 0:
            b = self.boundary_statistics()
            state["boundary"] = np.stack([b[n] for n in STAT_BOUNDARY_NAMES])
        return state

    def set_statistics_state(self, state, raise_on_error=True):
        """orc_solver_set_statistics_state: continue from a statistics_state() (of this or another solver with the same groups enabled)"""
        mask, _ = _mask_of(list(state["names"]), STATISTIC_NAMES)
        raw = _f64(state["raw"])
        assert raw.size == len(state["names"]) * self.n
        b = None if state.get("boundary") is None else _f64(state["boundary"])
        st = lib().orc_solver_set_statistics_state(self.ptr, C.c_uint64(state["samples"]), C.c_double(state["weight_sum"]),
                                                   C.c_uint32(mask), _p(raw), None if b is None else _p(b))
        if raise_on_error:
            check(st)
        return st

    def mean_friction_velocity(self, zone_name):
        """sqrt((sum_f A <shear_mag> / sum_f A) / rho) over the boundary faces of the zone `zone_name` (a name or an index): the friction
        velocity of the time-mean wall shear, the number settings.WallDamping.u_tau asks for.  Host arithmetic on boundary_statistics()."""
        b = self.boundary_statistics()
        if isinstance(zone_name, str):
            zone_name = list(self.mesh.arrays["zone_names"]).index(zone_name)
        lo, hi = int(b.zone_ptr[zone_name]), int(b.zone_ptr[zone_name + 1])
        area = np.asarray(self.mesh.arrays["face_area"])[np.asarray(b.faces[lo:hi])]
        return float(np.sqrt((np.sum(area * b["shear_mag"][lo:hi]) / np.sum(area)) / self.rho))

    def bench_time_statistics(self, reps=50):
        """orc_bench_time_statistics: (ms per cell pass time_stats_k, ms per boundary pass); needs set_time_statistics()"""
        ms = np.zeros(2)
        check(lib().orc_bench_time_statistics(self.ptr, C.c_int(reps), _p(ms)))
        return float(ms[0]), float(ms[1])

    # ---------------------------------------------------------------- point probes (orc_solver_sample_probes, orc_solver_set_probe_history)
    def sample(self, probes, fields=("u", "v", "w", "p"), interpolation="linear", raise_on_error=True):
        """orc_solver_sample_probes: {name: ndarray[len(probes)]} of the fields (PROBE_NAMES or a bit mask) at the points of a
        Mesh.locate() result; interpolation 'cell' or 'linear' (or a settings.ProbeInterpolation value).  Points outside the mesh are
        sampled at their final cell: probes.status tells.  Reads only.  (raise_on_error=False: (status, dict))"""
        mask, names = _mask_of(fields, PROBE_NAMES)
        n = len(probes)
        out = np.zeros((max(bin(mask).count("1"), 1), n))
        st = lib().orc_solver_sample_probes(self.ptr, probes.ptr if probes is not None else None, C.c_uint32(mask & 0xFFFFFFFF),
                                            C.c_int32(_interpolation(interpolation)), _p(out))
        res = _probe_rows(out, mask, names) if st == 0 else {}
        if raise_on_error:
            check(st)
            return res
        return st, res

    def sample_line(self, a, b, n, **kw):
        """n points from a to b (both included), located and sampled -> (points [n, 3], Probes, {name: ndarray[n]}); kw as sample()"""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        t = np.linspace(0.0, 1.0, n)[:, None] if n > 1 else np.zeros((1, 1))
        points = a[None, :] + t * (b - a)[None, :]
        probes = self.mesh.locate(points)
        return points, probes, self.sample(probes, **kw)

    def set_probe_history(self, probes=None, fields=("u", "v", "w", "p"), interpolation="linear", interval=1, raise_on_error=True):
        """orc_solver_set_probe_history: from now on advance() appends one record of the fields at the probes after every `interval`-th
        step (steps counted from 1 since enabling); probes=None turns the history off and drops it.  Reads only: fields and reports
        keep their bits, and a step gains no synchronisation."""
        if probes is None:
            st = lib().orc_solver_set_probe_history(self.ptr, None, C.c_uint32(0), C.c_int32(0), C.c_uint64(1))
            mask, names = 0, []
        else:
            mask, names = _mask_of(fields, PROBE_NAMES)
            st = lib().orc_solver_set_probe_history(self.ptr, probes.ptr, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(_interpolation(interpolation)),
                                                    C.c_uint64(interval))
        if st == 0:
            self._probe_history = (probes, mask, names)  # keeps the probe set alive while the history reads it
        if raise_on_error:
            check(st)
        return st

    def record_probes(self, tag=0.0, raise_on_error=True):
        """orc_solver_record_probes: one record of the current state with `tag` in the time slot (steady runs)"""
        st = lib().orc_solver_record_probes(self.ptr, C.c_double(tag))
        if raise_on_error:
            check(st)
        return st

    def probe_history_count(self):
        """records kept (-1 while the history is off)"""
        return int(lib().orc_solver_probe_history_count(self.ptr))

    def probe_history(self, first=0, count=None):
        """the records [first, first + count) -> (times [k], {name: ndarray (k, n_points)}) (count=None: all from first)"""
        probes, mask, names = getattr(self, "_probe_history", None) or (None, 0, [])
        have = self.probe_history_count()
        if count is None:
            count = max(have - first, 0)
        k, n = max(bin(mask).count("1"), 1), len(probes) if probes is not None else 0
        times, out = np.zeros(count), np.zeros((count, k, max(n, 1)))
        check(lib().orc_solver_probe_history(self.ptr, C.c_uint64(first), C.c_uint64(count), _p(times), _p(out)))
        order = [i for i in range(len(PROBE_NAMES)) if mask >> i & 1]
        rows = {PROBE_NAMES[f]: np.ascontiguousarray(out[:, q, :n]) for q, f in enumerate(order)}
        return times, {name: rows[name] for name in names}

    # ---------------------------------------------------------------- volume reports (orc_solver_group_report, ...)
    def group_report(self, groups, fields=("u", "v", "w", "p"), weighting="volume", raise_on_error=True):
        """orc_solver_group_report: the current fields (PROBE_NAMES or a bit mask; columns in PROBE_NAMES order) reduced over every group
        of a Mesh.cell_groups() / bin_cells() / box_cells() set on the device -> GroupReport.  Reads only.  (raise_on_error=False:
        (status, report or None))"""
        mask, _ = _mask_of(fields, PROBE_NAMES)
        names = [n for k, n in enumerate(PROBE_NAMES) if mask >> k & 1]
        G = len(groups) if groups is not None else 0
        sums, weight, where = _group_out(G, len(names))
        st = lib().orc_solver_group_report(self.ptr, groups.ptr if groups is not None else None, C.c_uint32(mask & 0xFFFFFFFF),
                                           C.c_int32(_weighting(weighting)), _p(sums), _p(weight), where.ctypes.data_as(_I64))
        if raise_on_error:
            check(st)
            return GroupReport(names, sums, weight, where)
        return st, (GroupReport(names, sums, weight, where) if st == 0 else None)

    def group_statistics(self, groups, names=None, form="normalised", weighting="volume", raise_on_error=True):
        """orc_solver_group_statistics: the running statistics `names` (STATISTIC_NAMES or a bit mask; None = every enabled field;
        columns in STATISTIC_NAMES order) reduced over the groups where they lie, per cell exactly the values statistics() returns in
        that form ('normalised' or 'raw') -> GroupReport.  (raise_on_error=False: (status, report or None))"""
        if names is None:
            names = self.statistics_fields()
        mask, _ = _mask_of(names, STATISTIC_NAMES)
        cols = [n for k, n in enumerate(STATISTIC_NAMES) if mask >> k & 1]
        G = len(groups) if groups is not None else 0
        sums, weight, where = _group_out(G, len(cols))
        f = {"raw": 0, "normalised": 1}[form.lower()] if isinstance(form, str) else int(form)
        st = lib().orc_solver_group_statistics(self.ptr, groups.ptr if groups is not None else None, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(f),
                                               C.c_int32(_weighting(weighting)), _p(sums), _p(weight), where.ctypes.data_as(_I64))
        if raise_on_error:
            check(st)
            return GroupReport(cols, sums, weight, where)
        return st, (GroupReport(cols, sums, weight, where) if st == 0 else None)

    def set_group_history(self, groups=None, fields=("u", "v", "w", "p"), interval=1, weighting="volume", raise_on_error=True):
        """orc_solver_set_group_history: from now on advance() appends one group report of the fields after every `interval`-th step
        (steps counted from 1 since enabling); groups=None turns the history off and drops it.  Reads only, and adds no
        synchronisation to a step."""
        if groups is None:
            st = lib().orc_solver_set_group_history(self.ptr, None, C.c_uint32(0), C.c_int32(0), C.c_uint64(1))
            names = []
        else:
            mask, _ = _mask_of(fields, PROBE_NAMES)
            names = [n for k, n in enumerate(PROBE_NAMES) if mask >> k & 1]
            st = lib().orc_solver_set_group_history(self.ptr, groups.ptr, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(_weighting(weighting)),
                                                    C.c_uint64(interval))
        if st == 0:
            self._group_history = (groups, names) if groups is not None else None  # keeps the group set alive while the history reads it
        if raise_on_error:
            check(st)
        return st

    def record_groups(self, tag=0.0, raise_on_error=True):
        """orc_solver_record_groups: one record of the current state with `tag` in the time slot (steady runs)"""
        st = lib().orc_solver_record_groups(self.ptr, C.c_double(tag))
        if raise_on_error:
            check(st)
        return st

    def group_history_count(self):
        """records kept (-1 while the history is off)"""
        return int(lib().orc_solver_group_history_count(self.ptr))

    def group_history(self, first=0, count=None, full=False):
        """the records [first, first + count) -> (times [k], values [k, G, F, 4] in the order SUM, SUM_SQ, MIN, MAX, weight [G] = W)
        (count=None: all from first); full=True: (times, [GroupReport per record]) with the cells of the extrema as well"""
        groups, names = getattr(self, "_group_history", None) or (None, [])
        have = self.group_history_count()
        if count is None:
            count = max(have - first, 0)
        G, F = (len(groups) if groups is not None else 0), len(names)
        times = np.zeros(count)
        sums, where = np.zeros((count, max(G, 1), max(F, 1), _GROUP_N)), np.zeros((count, max(G, 1), max(F, 1), 2), np.int64)
        weight = np.zeros((max(G, 1), 2))
        check(lib().orc_solver_group_history(self.ptr, C.c_uint64(first), C.c_uint64(count), _p(times), _p(sums), _p(weight),
                                             where.ctypes.data_as(_I64)))
        if full:
            return times, [GroupReport(names, sums[k], weight, where[k]) for k in range(count)]
        return times, sums[:, :G, :F], weight[:G, 0].copy()

    def bench_group_report(self, groups, fields=("u", "v", "w", "p"), weighting="volume", reps=20):
        """orc_bench_group_report: HIP-event (ms per group_chunk_k, ms per group_fold_k) of one launch's fields"""
        mask, _ = _mask_of(fields, PROBE_NAMES)
        ms = np.zeros(2)
        check(lib().orc_bench_group_report(self.ptr, groups.ptr, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(_weighting(weighting)), C.c_int(reps), _p(ms)))
        return float(ms[0]), float(ms[1])

    # ---------------------------------------------------------------- tracer particles (orc_solver_advect_tracers, ...)
    def advect(self, tracers, settings, n_substeps, record_stride=0, raise_on_error=True):
        """orc_solver_advect_tracers: up to n_substeps substeps of a Mesh.seed() set in the current u, v, w (settings.TracerSettings).
        record_stride > 0 (a divisor of n_substeps) -> (path [K + 1, n, 3], path_len [n]): the positions after every record_stride
        substeps, record 0 those at entry; the polyline of particle i is path[:path_len[i], i].  Otherwise None.  Reads the solver
        only.  (raise_on_error=False: (status, result))"""
        n = len(tracers) if tracers is not None else 0
        path = plen = None
        if record_stride > 0:
            K = n_substeps // record_stride
            path, plen = np.zeros((K + 1, 3, max(n, 1))), np.zeros(max(n, 1), np.int32)
        st = lib().orc_solver_advect_tracers(self.ptr, tracers.ptr if tracers is not None else None, C.byref(settings) if settings is not None else None,
                                             C.c_uint64(n_substeps), C.c_uint64(record_stride), None if path is None else _p(path),
                                             None if plen is None else plen.ctypes.data_as(C.POINTER(C.c_int32)))
        res = None
        if st == 0 and path is not None:
            res = (np.ascontiguousarray(path[:, :, :n].transpose(0, 2, 1)), plen[:n])
        if raise_on_error:
            check(st)
            return res
        return st, res

    def streamlines(self, points, step, n_substeps, both_directions=False, **kw):
        """Streamlines of the current velocity from the points [n, 3]: seeds, advects with LENGTH steps of `step` and a recorded path
        -> a list of [m_i, 3] arrays.  both_directions joins the backward half (reversed) to the forward half at the seed.  kw:
        further fields of settings.TracerSettings (scheme, interpolation, min_speed)."""
        from .settings import TracerSettings, TracerStepMode
        halves = []
        for direction in ((-1, 1) if both_directions else (1,)):
            c = TracerSettings.make(step, step_mode=TracerStepMode.LENGTH, direction=direction, **kw)
            path, plen = self.advect(self.mesh.seed(points), c, n_substeps, record_stride=1)
            halves.append([path[:plen[i], i] for i in range(path.shape[1])])
        if not both_directions:
            return halves[0]
        return [np.concatenate([b[:0:-1], f]) for b, f in zip(*halves)]

    def isosurface(self, field, level):
        """orc_solver_cut_field: the surface field = level of one of the solver's own fields (a PROBE_NAMES name) without leaving the
        device: the node average of Mesh.node_average, then the level -> mesh.Cut.  Needs Mesh.set_nodes().  Reads only."""
        from .mesh import Cut
        bit = 1 << PROBE_NAMES.index(field) if isinstance(field, str) else int(field)
        st = C.c_int(0)
        ptr = lib().orc_solver_cut_field(self.ptr, C.c_uint32(bit & 0xFFFFFFFF), C.c_double(level), C.byref(st))
        return Cut(self.mesh, ptr, st.value)

    def sample_cut(self, cut, fields=("u", "v", "w", "p"), interpolation="cell", raise_on_error=True):
        """orc_solver_sample_cut: {name: ndarray} of the fields on a mesh.Cut; 'cell': one value per polygon (the owner cell's),
        'linear': one per polygon vertex through the owner's gradient, the bits sample() gives for that cell and point.  Reads only.
        (raise_on_error=False: (status, dict))"""
        mask, names = _mask_of(fields, PROBE_NAMES)
        n = 0 if cut is None else (cut.n_points if _interpolation(interpolation) == 1 else cut.n_polygons)
        out = np.zeros((max(bin(mask).count("1"), 1), n))
        st = lib().orc_solver_sample_cut(self.ptr, cut.ptr if cut is not None else None, C.c_uint32(mask & 0xFFFFFFFF),
                                         C.c_int32(_interpolation(interpolation)), _p(out))
        res = _probe_rows(out, mask, names) if st == 0 else {}
        if raise_on_error:
            check(st)
            return res
        return st, res

    def sample_tracers(self, tracers, fields=("u", "v", "w", "p"), interpolation="linear", raise_on_error=True):
        """orc_solver_sample_tracers: sample() at the particles' present positions and cells -> {name: ndarray[len(tracers)]}"""
        mask, names = _mask_of(fields, PROBE_NAMES)
        out = np.zeros((max(bin(mask).count("1"), 1), len(tracers)))
        st = lib().orc_solver_sample_tracers(self.ptr, tracers.ptr, C.c_uint32(mask & 0xFFFFFFFF), C.c_int32(_interpolation(interpolation)), _p(out))
        res = _probe_rows(out, mask, names) if st == 0 else {}
        if raise_on_error:
            check(st)
            return res
        return st, res

    def set_tracer_tracking(self, tracers=None, settings=None, substeps=1, raise_on_error=True):
        """orc_solver_set_tracer_tracking: from now on every step of advance() moves the set by `substeps` substeps of dt / substeps in
        the velocity just reached (TIME mode, direction +1; the settings' step is ignored); tracers=None turns it off.  Reads only:
        fields and reports keep their bits, and a step gains no synchronisation."""
        st = lib().orc_solver_set_tracer_tracking(self.ptr, tracers.ptr if tracers is not None else None,
                                                  C.byref(settings) if settings is not None else None, C.c_uint32(substeps))
        if st == 0:
            self._tracked = tracers  # keeps the set alive while advance() moves it
        if raise_on_error:
            check(st)
        return st

    def bench_tracers(self, tracers, settings, n_substeps, reps=5):
        """orc_bench_tracers: HIP-event ms per launch of n_substeps substeps from the set's state into scratch buffers"""
        ms = C.c_double(0.0)
        check(lib().orc_bench_tracers(self.ptr, tracers.ptr, C.byref(settings), C.c_uint64(n_substeps), C.c_int(reps), C.byref(ms)))
        return ms.value

    def surface_report(self, origin=None, raise_on_error=True):
        """orc_solver_surface_report: per-zone force, moment, mass and momentum flow, area and mean pressure of the current
        state -> SurfaceReport (with raise_on_error=False: (status, report)); reads only"""
        out = np.zeros((len(self.mesh.arrays["zone_type"]), _SURFACE_N))
        keep, o = _origin(origin)
        st = lib().orc_solver_surface_report(self.ptr, o, _p(out))
        rep = SurfaceReport(out, self.mesh.arrays.get("zone_names"))
        if raise_on_error:
            check(st)
            return rep
        return st, rep

    def derived_fields(self, names_or_mask, raise_on_error=True):
        """orc_solver_derived_fields: derived cell fields of the current u, v, w (DERIVED_NAMES, 'vorticity' = (n, 3), or a bit
        mask), cell order as get_fields() -> {name: ndarray} (raise_on_error=False: (status, dict)); reads only"""
        mask, names = _mask_of(names_or_mask, DERIVED_NAMES, _VORTICITY)
        out = np.zeros((max(bin(mask).count("1"), 1), self.n))
        st = lib().orc_solver_derived_fields(self.ptr, C.c_uint32(mask & 0xFFFFFFFF), _p(out))
        if raise_on_error:
            check(st)
            return _derived_dict(out, mask, names, self.n)
        return st, (_derived_dict(out, mask, names, self.n) if st == 0 else {})

    def boundary_fields(self, names=BOUNDARY_NAMES, raise_on_error=True):
        """orc_solver_boundary_fields: the boundary-face maps of the current state -> BoundaryFields (raise_on_error=False:
        (status, BoundaryFields or None)); reads only"""
        mask, names = _mask_of(names, BOUNDARY_NAMES)
        nb = int(self.mesh.boundary_index()[0][-1])
        out = np.zeros((max(bin(mask).count("1"), 1), nb))
        st = lib().orc_solver_boundary_fields(self.ptr, C.c_uint32(mask & 0xFFFFFFFF), _p(out))
        if raise_on_error:
            check(st)
            return _boundary_result(self.mesh, out, mask, names)
        return st, (_boundary_result(self.mesh, out, mask, names) if st == 0 else None)

    def assemble_momentum(self):
        nnz, n = self.mesh.nnz, self.n
        au, av, aw = np.empty(nnz), np.empty(nnz), np.empty(nnz)
        bu, bv, bw = np.empty(n), np.empty(n), np.empty(n)
        pe = np.zeros(3)
        check(lib().orc_solver_assemble_momentum(self.ptr, _p(au), _p(av), _p(aw), _p(bu), _p(bv), _p(bw), _p(pe)))
        return au, av, aw, bu, bv, bw, tuple(pe)

    def assemble_pressure(self):
        a, b = np.empty(self.mesh.nnz), np.empty(self.n)
        check(lib().orc_solver_assemble_pressure(self.ptr, _p(a), _p(b)))
        return a, b

    def assemble_momentum_only(self):
        """the momentum assembly of the current state, matrices left on the device (bench.py's product measurements)"""
        check(lib().orc_solver_assemble_momentum(self.ptr, None, None, None, None, None, None, None))

    def snapshot(self):
        """device-side copy of the state the next SIMPLE iteration starts from"""
        check(lib().orc_solver_snapshot(self.ptr))

    def restore(self):
        check(lib().orc_solver_restore(self.ptr))

    def bench_amg_levels(self, reps=20):
        """per level of a_u's Multigrid hierarchy: (rows, nnz, padded SELL entries, ms per product)"""
        rows, nnz, padded = (np.zeros(4, dtype=np.int64) for _ in range(3))
        ms = np.zeros(4)
        nl = C.c_int(0)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        check(lib().orc_bench_amg_levels(self.ptr, C.c_int(reps), i64(rows), i64(nnz), i64(padded), _p(ms), C.byref(nl)))
        return [(int(rows[k]), int(nnz[k]), int(padded[k]), float(ms[k])) for k in range(nl.value)]

    def bench_spmv(self, reps=50):
        ms, cs = C.c_double(0.0), C.c_double(0.0)
        check(lib().orc_bench_spmv(self.ptr, C.c_int(reps), C.byref(ms), C.byref(cs)))
        return ms.value, cs.value

    def bench_inloop_products(self, reps=50):
        """orc_bench_inloop_products: ms per launch of the level-0 products as the BiCGSTAB loop launches them —
        (one system: EpiStoreSum, EpiTs; three systems in one launch: EpiStoreSum3, EpiTs3)."""
        ms = (C.c_double * 4)()
        check(lib().orc_bench_inloop_products(self.ptr, C.c_int(reps), ms))
        lib().orc_bench_inloop_variant.restype = C.c_char_p
        self.inloop_variant = lib().orc_bench_inloop_variant().decode()  # "<narrow>, <scaled>, <non-temporal>" template arguments of those launches
        return [ms[k] for k in range(4)]

    def bench_momentum_residuals(self, reps=50):
        """orc_bench_momentum_residuals: ms per fused residual pass over the assembled momentum systems (needs set_monitors())"""
        ms = C.c_double(0.0)
        check(lib().orc_bench_momentum_residuals(self.ptr, C.c_int(reps), C.byref(ms)))
        return ms.value

    def bench_gs_sweep0(self, reps=50):
        """orc_bench_gs_sweep0: (ms per sweep-from-zero of one system, ms per sweep of u, v, w in one launch per colour, colours)"""
        ms = (C.c_double * 2)()
        nc = C.c_int(0)
        check(lib().orc_bench_gs_sweep0(self.ptr, C.c_int(reps), ms, C.byref(nc)))
        return ms[0], ms[1], nc.value

    def bench_gs_sweep(self, reps=50):
        """orc_bench_gs_sweep: (ms per multicolour Gauss-Seidel sweep over a_u, number of colours = launches per sweep)"""
        ms, nc = C.c_double(0.0), C.c_int(0)
        check(lib().orc_bench_gs_sweep(self.ptr, C.c_int(reps), C.byref(ms), C.byref(nc)))
        return ms.value, nc.value

    def bench_bicgstab_iteration(self, reps=20):
        ms = C.c_double(0.0)
        check(lib().orc_bench_bicgstab_iteration(self.ptr, C.c_int(reps), C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------ solver::initialize_* (solver.rs:246-509)
PRESSURE_ONLY, VELOCITY_ONLY, HYBRID = 0, 1, 2


def check_boundary_conditions(mesh):
    """solver::check_boundary_conditions (solver.rs:710-772) -> PRESSURE_ONLY | VELOCITY_ONLY | HYBRID;
    OrcError(ORC_ERR_NO_BOUNDARY_CONDITIONS) for "You must set boundary conditions."."""
    kind = C.c_int(0)
    check(lib().orc_check_boundary_conditions(mesh.ptr, C.byref(kind)))
    return kind.value


def initialize_pressure_field(mesh, p=None):
    """solver::initialize_pressure_field (solver.rs:414-509); p defaults to zeros like the reference's callers."""
    p = np.zeros(mesh.n_cells) if p is None else _f64(p).copy()
    check(lib().orc_initialize_pressure_field(mesh.ptr, _p(p)))
    return p


def initialize_flow(mesh, mu, rho, iteration_count, settings=None):
    """solver::initialize_flow (solver.rs:246-352) -> (u, v, w, p)."""
    u, v, w, p = (np.zeros(mesh.n_cells) for _ in range(4))
    check(lib().orc_initialize_flow(mesh.ptr, C.c_double(mu), C.c_double(rho), C.c_uint64(iteration_count),
                                    C.byref(settings) if settings is not None else None, _p(u), _p(v), _p(w), _p(p)))
    return u, v, w, p


def initialize_velocity_field(mesh, settings=None):
    """solver::initialize_velocity_field (solver.rs:511-696) -> (u, v, w, psi)."""
    u, v, w, psi = (np.zeros(mesh.n_cells) for _ in range(4))
    check(lib().orc_initialize_velocity_field(mesh.ptr, C.byref(settings) if settings is not None else None, _p(u), _p(v), _p(w), _p(psi)))
    return u, v, w, psi


def initialize_flow_new(mesh, mu, rho, iteration_count):
    """solver::initialize_flow_new (solver.rs:354-410) -> (u, v, w, p)."""
    u, v, w, p = (np.zeros(mesh.n_cells) for _ in range(4))
    check(lib().orc_initialize_flow_new(mesh.ptr, C.c_double(mu), C.c_double(rho), C.c_uint64(iteration_count),
                                        _p(u), _p(v), _p(w), _p(p)))
    return u, v, w, p
