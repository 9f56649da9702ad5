"""numpy restatement of the surface reports (DESIGN.md §3 "Surface reports", orc_types.h OrcSurfaceQuantity) from MeshArrays.

Every term is formed in float64 in THE documented operator order, one IEEE operation per numpy operation (numpy never fuses a
multiply with an add), so a term here and the device's term of the same face are the same bits; only the summation differs.  The
sums are math.fsum (exactly rounded), and next to every sum comes sum |term|: the scale of the device's rounding.

Per boundary face f of cell P (c1 < 0), n = the stored face normal (it points out of c0 = P), A = area:
    U_f  = zone vector (Wall, VelocityInlet)           else U_P            get_face_velocity, VelocityInterpolation::None
    p_f  = zone scalar (PressureInlet, PressureOutlet)  else p_P            get_face_pressure
    phi  = 0 (Wall, Symmetry)  else (n.x U_f.x + n.y U_f.y) + n.z U_f.z      get_face_flux
    d    = (mu A) / sqrt((dx dx + dy dy) + dz dz), dx = x_f - x_P (Wall, VelocityInlet)  else 0
    m = (rho phi) A     pa = p_f A     Fp = pa n     Fv = d (U_P - U_f)     r = x_f - x_0     F = Fp + Fv
    M = (r.y F.z - r.z F.y,  r.z F.x - r.x F.z,  r.x F.y - r.y F.x)
"""
import math

import numpy as np

INTERIOR, WALL, PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY, VELOCITY_INLET, OUTFLOW = 2, 3, 4, 5, 7, 10, 36
SUPPORTED = (WALL, PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY, VELOCITY_INLET)
N = 16
AREA, MASS_FLOW, PRESSURE_FORCE, VISCOUS_FORCE, MOMENTUM_FLOW, MOMENT, PRESSURE_AREA, FACES = 0, 1, 2, 5, 8, 11, 14, 15
EPS = 2.0 ** -53  # unit roundoff of float64: the relative error of one rounded operation

# Rounded operations that form ONE term of each quantity, counted from the order above:
#   AREA, FACES       0   (stored values)
#   MASS_FLOW         7   phi: 3 products + 2 sums; rho phi; times A
#   PRESSURE_FORCE    2   p_f A; times n.k
#   VISCOUS_FORCE    13   d: 3 differences, 3 squares, 2 sums, sqrt, mu A, the quotient = 11; U_P - U_f; times d
#   MOMENTUM_FLOW     8   m (7); times U_f.k
#   MOMENT           16   F.k = Fp.k + Fv.k: max(2, 13) + 1 = 14; r.k: 1; a product r F: 15; the difference of two: 16
#   PRESSURE_AREA     1   p_f A
C_OPS = np.array([0, 7, 2, 2, 2, 13, 13, 13, 8, 8, 8, 16, 16, 16, 1, 0])


def boundary_faces(a, n_own=None):
    """per zone: the boundary faces of owned cells, ascending — what Mesh.boundary_index() must return"""
    c0, c1, fz = np.asarray(a["face_c0"]), np.asarray(a["face_c1"]), np.asarray(a["face_zone"])
    own = np.ones(len(c0), bool) if n_own is None else c0 < n_own
    Z = len(a["zone_type"])
    return [np.flatnonzero((c1 < 0) & own & (fz == z)) for z in range(Z)]


def face_values(a, u, v, w, p, faces):
    """(U_f [k,3], p_f [k], phi_f [k]) of the boundary faces `faces`: the oracle's get_face_velocity (None), get_face_pressure,
    get_face_flux.  A zone type outside SUPPORTED raises ValueError (ORC_ERR_UNSUPPORTED_BC on the device)."""
    faces = np.asarray(faces, dtype=np.int64)
    zt = np.asarray(a["zone_type"])[np.asarray(a["face_zone"])[faces]]
    if not np.all(np.isin(zt, SUPPORTED)):
        raise ValueError("unsupported boundary condition")
    z = np.asarray(a["face_zone"])[faces]
    P = np.asarray(a["face_c0"])[faces]
    n = np.asarray(a["face_normal"], dtype=np.float64).reshape(-1, 3)[faces]
    UP = np.stack([np.asarray(u)[P], np.asarray(v)[P], np.asarray(w)[P]], axis=1)
    vec_bc = (zt == WALL) | (zt == VELOCITY_INLET)
    p_bc = (zt == PRESSURE_INLET) | (zt == PRESSURE_OUTLET)
    no_flux = (zt == WALL) | (zt == SYMMETRY)
    Uf = np.where(vec_bc[:, None], np.asarray(a["zone_vector"], dtype=np.float64).reshape(-1, 3)[z], UP)
    pf = np.where(p_bc, np.asarray(a["zone_scalar"], dtype=np.float64)[z], np.asarray(p)[P])
    phi = (n[:, 0] * Uf[:, 0] + n[:, 1] * Uf[:, 1]) + n[:, 2] * Uf[:, 2]
    phi = np.where(no_flux, 0.0, phi)
    return Uf, pf, phi


def terms(a, u, v, w, p, rho, mu, origin, faces):
    """T[k, 16]: the sixteen terms of every face of `faces`, in the documented operator order"""
    faces = np.asarray(faces, dtype=np.int64)
    T = np.zeros((len(faces), N))
    if len(faces) == 0:
        return T
    x0 = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    zt = np.asarray(a["zone_type"])[np.asarray(a["face_zone"])[faces]]
    vec_bc = (zt == WALL) | (zt == VELOCITY_INLET)
    no_flux = (zt == WALL) | (zt == SYMMETRY)
    P = np.asarray(a["face_c0"])[faces]
    A = np.asarray(a["face_area"], dtype=np.float64)[faces]
    n = np.asarray(a["face_normal"], dtype=np.float64).reshape(-1, 3)[faces]
    xf = np.asarray(a["face_centroid"], dtype=np.float64).reshape(-1, 3)[faces]
    xP = np.asarray(a["cell_centroid"], dtype=np.float64).reshape(-1, 3)[P]
    UP = np.stack([np.asarray(u)[P], np.asarray(v)[P], np.asarray(w)[P]], axis=1)
    Uf, pf, phi = face_values(a, u, v, w, p, faces)
    m = np.where(no_flux, 0.0, (rho * phi) * A)
    pa = pf * A
    Fp = pa[:, None] * n
    dx = xf - xP
    dist = np.sqrt((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])
    d = (mu * A) / dist
    Fv = np.where(vec_bc[:, None], d[:, None] * (UP - Uf), 0.0)
    r = xf - x0
    F = Fp + Fv
    T[:, AREA] = A
    T[:, MASS_FLOW] = m
    T[:, 2:5] = Fp
    T[:, 5:8] = Fv
    T[:, 8:11] = np.where(no_flux[:, None], 0.0, m[:, None] * Uf)
    T[:, 11] = r[:, 1] * F[:, 2] - r[:, 2] * F[:, 1]
    T[:, 12] = r[:, 2] * F[:, 0] - r[:, 0] * F[:, 2]
    T[:, 13] = r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]
    T[:, PRESSURE_AREA] = pa
    T[:, FACES] = 1.0
    return T


def report(a, u, v, w, p, rho, mu, origin=None, n_own=None):
    """(S [Z,16] exactly rounded sums, Sabs [Z,16] sums of |term|, faces per zone [Z])"""
    zones = boundary_faces(a, n_own)
    Z = len(zones)
    S, Sabs = np.zeros((Z, N)), np.zeros((Z, N))
    for z, faces in enumerate(zones):
        T = terms(a, u, v, w, p, rho, mu, origin, faces)
        for q in range(N):
            S[z, q] = math.fsum(T[:, q].tolist())
            Sabs[z, q] = math.fsum(np.abs(T[:, q]).tolist())
    return S, Sabs, np.array([len(f) for f in zones])


def bound(Sabs, n_faces, chunk):
    """The derived bound on |device - restatement| per zone and quantity:
        (c_ops + ceil(log2(faces)) + ceil(log2(chunks)) + 2) EPS sum|term|
    c_ops bounds the rounding of one term (here in fact zero: both sides form a term with the same operations); the device sums a
    chunk over a tree of depth <= ceil(log2(faces)) + 1 (a lane's eight slots pairwise, the wave tree, then the four waves in
    sequence: one addition more than a tree over four) and a zone's chunks over a tree of depth ceil(log2(chunks)); the last unit
    is the rounding of this restatement's own exactly rounded sum.
    A partitioned run adds the ranks' sums of a zone (one addition for two ranks).  The bound stays the single-rank one, with the
    faces and chunks of the WHOLE zone, wherever no rank holds more than half of a shared zone rounded up to a power of two,
    ceil(log2(faces on a rank)) + 1 <= ceil(log2(faces)): each rank's tree is then a level shallower than the whole zone's, and
    the addition across the ranks takes that level.  tests/surface_mp_worker.py asserts this of its cut before it uses the bound."""
    n_faces = np.asarray(n_faces)
    chunks = np.maximum((n_faces + chunk - 1) // chunk, 1)
    depth = np.ceil(np.log2(np.maximum(n_faces, 1))) + np.ceil(np.log2(chunks))
    return (C_OPS[None, :] + depth[:, None] + 2.0) * EPS * Sabs


EXACT_ZERO_TYPES = {MASS_FLOW: (WALL, SYMMETRY), MOMENTUM_FLOW: (WALL, SYMMETRY),
                    VISCOUS_FORCE: (PRESSURE_INLET, PRESSURE_OUTLET, SYMMETRY)}


def check(got, a, u, v, w, p, rho, mu, origin, chunk, n_own=None):
    """assert the device's (Z,16) array against the restatement: FACES exactly, defined zeros == 0.0, the rest within bound();
    returns the largest error / bound ratio seen (for printing)"""
    got = np.asarray(got).reshape(-1, N)
    S, Sabs, nf = report(a, u, v, w, p, rho, mu, origin, n_own)
    B = bound(Sabs, nf, chunk)
    zt = np.asarray(a["zone_type"])
    assert got.shape == S.shape, (got.shape, S.shape)
    assert np.array_equal(got[:, FACES], nf.astype(np.float64)), (got[:, FACES], nf)
    worst = 0.0
    for z in range(len(nf)):
        if nf[z] == 0:
            assert np.all(got[z] == 0.0), (z, got[z])
            continue
        for q0, types in EXACT_ZERO_TYPES.items():
            width = 1 if q0 == MASS_FLOW else 3
            if zt[z] in types:
                assert np.all(got[z, q0:q0 + width] == 0.0), (z, q0, got[z])
        err = np.abs(got[z] - S[z])
        assert np.all(err <= B[z]), (z, int(nf[z]), err, B[z], got[z], S[z])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(B[z] > 0, err / B[z], 0.0)
        worst = max(worst, float(ratio.max()))
    return worst
