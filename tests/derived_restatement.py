"""numpy restatement of the derived cell fields and the boundary-face maps (DESIGN.md §3 "Derived fields and boundary maps",
orc_types.h OrcDerivedField / OrcBoundaryField) from MeshArrays.

Every value is formed in float64 in THE documented operator order, one IEEE operation per numpy operation (numpy never fuses a
multiply with an add), so a value here and the device's value of the same cell or face are the same bits.

The Green-Gauss gradient is grad_u_k's (orc_amd/csrc/gradient_cell.hpp): per cell, its faces in cell_faces order,
    U_f = zone vector (Wall, VelocityInlet);  (U_c0 + U_c1) / 2 (Interior);  U_c0 otherwise        face_velocity_linear
    n_out = n, or -n when the cell is the face's c1;   nn = n_out * (A / V)
    G[i][j] <- G[i][j] + U_f.i * nn.j                                                         from 0.0, face after face
    conv    <- conv + |(n_out.x U_f.x + n_out.y U_f.y) + n_out.z U_f.z| * A
The table formulas (fields(), one operation per line of the table):
    w = (G21 - G12, G02 - G20, G10 - G01)       |w| = sqrt((wx wx + wy wy) + wz wz)
    S_ij = (G_ij + G_ji) / 2, W_ij = (G_ij - G_ji) / 2
    SS = ((G00 G00 + G11 G11) + G22 G22) + 2 ((S01 S01 + S02 S02) + S12 S12)      OO = 2 ((W01 W01 + W02 W02) + W12 W12)
    strain = sqrt(2 SS)     Q = (OO - SS) / 2     div = (G00 + G11) + G22     rate = conv / (2 V)
The boundary maps reuse tests/surface_restatement.py (face values and the sixteen terms) and add, per face,
    t = Fv / A     tn = (t.x n.x + t.y n.y) + t.z n.z     s = t - tn n     shear = sqrt((s.x s.x + s.y s.y) + s.z s.z)
    y+ = ((rho sqrt(shear / rho)) dist) / mu, dist = sqrt((dx dx + dy dy) + dz dz), dx = x_f - x_P     flux = rho phi

Error bounds (gradient_bound, field_bounds) are DERIVED, for the analytic checks of tests/test_derived_cpu.py:
  a gradient entry is a sequential sum of F = faces terms, each a product of three rounded factors (A / V, n * that, U_f * that) of
  a face value that is itself one rounded sum: |computed - exact| <= (F + 3) EPS sum_f |U_f.i nn.j| to first order (F - 1 additions
  bounded by F EPS times the sum of magnitudes, 3 EPS for the factors of a term).  field_bounds() carries that through the table:
  differences and sums add the entries' bounds; sqrt(2 SS) = sqrt(2) |S|_F and sqrt(w.w) are 1-Lipschitz in the Frobenius / Euclidean
  norm of their arguments; Q = (|W|_F^2 - |S|_F^2) / 2 moves by at most |W| |dW| + |S| |dS| + (|dW|^2 + |dS|^2) / 2; every formula
  adds its own roundings, counted per formula below, times EPS times the magnitude it rounds.
"""
import numpy as np

import surface_restatement as R

EPS = R.EPS
N = 8
VORTICITY_X, VORTICITY_Y, VORTICITY_Z, VORTICITY_MAG, STRAIN_RATE_MAG, Q_CRITERION, DIVERGENCE, CONVECTIVE_RATE = range(8)
NAMES = ("vorticity_x", "vorticity_y", "vorticity_z", "vorticity_mag", "strain_rate_mag", "q_criterion", "divergence", "convective_rate")
B_N = 8
B_PRESSURE, B_TRACTION_X, B_TRACTION_Y, B_TRACTION_Z, B_SHEAR_MAG, B_Y_PLUS, B_MASS_FLUX, B_AREA = range(8)
B_NAMES = ("pressure", "traction_x", "traction_y", "traction_z", "shear_mag", "y_plus", "mass_flux", "area")
ASSEMBLY_TYPES = (R.INTERIOR,) + tuple(R.SUPPORTED)


def _walk(a, u, v, w, n_own=None):
    """yields, for the k-th face slot of every cell that has one: (cells, U_f [m,3], n_out [m,3], A [m], V [m])"""
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    fz, zt = np.asarray(a["face_zone"]), np.asarray(a["zone_type"])
    zvec = np.asarray(a["zone_vector"], dtype=np.float64).reshape(-1, 3)
    area = np.asarray(a["face_area"], dtype=np.float64)
    nrm = np.asarray(a["face_normal"], dtype=np.float64).reshape(-1, 3)
    vol = np.asarray(a["cell_volume"], dtype=np.float64)
    cfp, cf = np.asarray(a["cell_face_ptr"]), np.asarray(a["cell_faces"])
    U = np.stack([np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)], axis=1)
    n = len(vol) if n_own is None else n_own
    counts = np.diff(cfp)[:n]
    for k in range(int(counts.max()) if n else 0):
        cells = np.flatnonzero(counts > k)
        f = cf[cfp[cells] + k]
        t = zt[fz[f]]
        if not np.all(np.isin(t, ASSEMBLY_TYPES)):
            raise ValueError("unsupported boundary condition")
        a0, b0 = c0[f], np.maximum(c1[f], 0)
        interior = t == R.INTERIOR
        vec_bc = (t == R.WALL) | (t == R.VELOCITY_INLET)
        Uf = np.where(interior[:, None], (U[a0] + U[b0]) / 2.0, U[a0])
        Uf = np.where(vec_bc[:, None], zvec[fz[f]], Uf)
        n_out = np.where((c0[f] != cells)[:, None], -nrm[f], nrm[f])
        yield cells, Uf, n_out, area[f], vol[cells]


def gg_gradient(a, u, v, w, n_own=None):
    """(G [n,3,3], conv [n], Gabs [n,3,3] = sum_f |U_f.i nn.j|, convabs [n] = sum_f (|n.x U.x| + |n.y U.y| + |n.z U.z|) A, faces [n])
    of the owned cells; G[c, i, j] = d u_i / d x_j"""
    n = len(a["cell_volume"]) if n_own is None else n_own
    G, Gabs = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    conv, convabs = np.zeros(n), np.zeros(n)
    for cells, Uf, n_out, A, V in _walk(a, u, v, w, n_own):
        nn = n_out * (A / V)[:, None]
        term = Uf[:, :, None] * nn[:, None, :]
        G[cells] = G[cells] + term
        Gabs[cells] = Gabs[cells] + np.abs(term)
        phi = (n_out[:, 0] * Uf[:, 0] + n_out[:, 1] * Uf[:, 1]) + n_out[:, 2] * Uf[:, 2]
        conv[cells] = conv[cells] + np.abs(phi) * A
        convabs[cells] = convabs[cells] + np.abs(n_out * Uf).sum(axis=1) * A
    faces = np.diff(np.asarray(a["cell_face_ptr"]))[:n]
    return G, conv, Gabs, convabs, faces


def fields(G, conv, vol):
    """[8, n]: the table formulas applied to a gradient G [n,3,3] (any reconstruction), conv [n] and the cell volumes"""
    G = np.asarray(G, dtype=np.float64).reshape(-1, 3, 3)
    g = lambda i, j: G[:, i, j]
    out = np.zeros((N, len(G)))
    wx, wy, wz = g(2, 1) - g(1, 2), g(0, 2) - g(2, 0), g(1, 0) - g(0, 1)
    out[VORTICITY_X], out[VORTICITY_Y], out[VORTICITY_Z] = wx, wy, wz
    out[VORTICITY_MAG] = np.sqrt((wx * wx + wy * wy) + wz * wz)
    s01, s02, s12 = (g(0, 1) + g(1, 0)) / 2.0, (g(0, 2) + g(2, 0)) / 2.0, (g(1, 2) + g(2, 1)) / 2.0
    ss = ((g(0, 0) * g(0, 0) + g(1, 1) * g(1, 1)) + g(2, 2) * g(2, 2)) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12)
    out[STRAIN_RATE_MAG] = np.sqrt(2.0 * ss)
    w01, w02, w12 = (g(0, 1) - g(1, 0)) / 2.0, (g(0, 2) - g(2, 0)) / 2.0, (g(1, 2) - g(2, 1)) / 2.0
    oo = 2.0 * ((w01 * w01 + w02 * w02) + w12 * w12)
    out[Q_CRITERION] = (oo - ss) / 2.0
    out[DIVERGENCE] = (g(0, 0) + g(1, 1)) + g(2, 2)
    out[CONVECTIVE_RATE] = np.asarray(conv) / (2.0 * np.asarray(vol, dtype=np.float64)[:len(G)])
    return out


def cell_fields(a, u, v, w, n_own=None):
    """[8, n] of the Green-Gauss arm"""
    G, conv, _, _, _ = gg_gradient(a, u, v, w, n_own)
    return fields(G, conv, np.asarray(a["cell_volume"])[:len(G)])


def convective_sum(a, u, v, w, n_own=None):
    """conv [n] alone (the least-squares arm uses the same face values and the same sum)"""
    return gg_gradient(a, u, v, w, n_own)[1]


def select(all_fields, mask):
    """the rows a mask selects, ascending: what the device packs"""
    return np.stack([all_fields[k] for k in range(all_fields.shape[0]) if mask >> k & 1])


# ------------------------------------------------------------------ derived bounds
def gradient_bound(Gabs, faces):
    """E [n,3,3]: (faces + 3) EPS sum_f |U_f.i nn.j| per gradient entry"""
    return (np.asarray(faces, dtype=np.float64)[:, None, None] + 3.0) * EPS * Gabs


def field_bounds(G, E, conv, convabs, faces, vol):
    """[8, n]: E carried through the table formulas (module docstring), each with the roundings of its own formula"""
    F = fields(G, conv, vol)
    e = lambda i, j: E[:, i, j]
    B = np.zeros_like(F)
    dw = np.stack([e(2, 1) + e(1, 2), e(0, 2) + e(2, 0), e(1, 0) + e(0, 1)])
    for k in range(3):  # one subtraction
        B[k] = dw[k] + EPS * np.abs(F[k])
    wnorm = np.sqrt((dw ** 2).sum(axis=0))
    B[VORTICITY_MAG] = (wnorm + np.abs(B[:3] - dw).sum(axis=0)) * (1 + 8 * EPS) + 4 * EPS * F[VORTICITY_MAG]  # 3 squares, 2 sums, sqrt: <= 4 EPS relative
    dS = np.sqrt(sum(((e(i, j) + e(j, i)) / 2.0) ** 2 for i in range(3) for j in range(3)))  # |dS|_F
    dW = np.sqrt(sum(((e(i, j) + e(j, i)) / 2.0) ** 2 for i in range(3) for j in range(3) if i != j))  # |dW|_F
    Sn = F[STRAIN_RATE_MAG] / np.sqrt(2.0) + dS  # |S|_F, |W|_F of the exact gradient, from the computed ones
    W = (G - np.transpose(G, (0, 2, 1))) / 2.0
    Wn = np.sqrt((W ** 2).sum(axis=(1, 2))) + dW
    # sqrt(2) |S|_F: 1-Lipschitz in S; 3 sums S_ij (relative EPS each, already inside |S|), 6 squares, 5 sums, 2 scalings, sqrt: <= 8 EPS relative
    B[STRAIN_RATE_MAG] = np.sqrt(2.0) * dS * (1 + 8 * EPS) + 8 * EPS * (F[STRAIN_RATE_MAG] + np.sqrt(2.0) * dS)
    # Q: the two squared norms (each <= 8 EPS relative as above), one difference, one halving
    B[Q_CRITERION] = (Wn * dW + Sn * dS + (dW ** 2 + dS ** 2) / 2.0) * (1 + 16 * EPS) + 9 * EPS * (Wn ** 2 + Sn ** 2)
    B[DIVERGENCE] = e(0, 0) + e(1, 1) + e(2, 2) + 2 * EPS * (np.abs(G[:, 0, 0]) + np.abs(G[:, 1, 1]) + np.abs(G[:, 2, 2]))
    # rate: F terms |phi| A, phi = 3 products and 2 sums (5 EPS of |n.x U.x| + |n.y U.y| + |n.z U.z|), times A, the sequential sum,
    # 2 V and the quotient: (faces + 3) EPS sum |phi| A + 6 EPS convabs, over 2 V
    V2 = 2.0 * np.asarray(vol, dtype=np.float64)[:len(G)]
    B[CONVECTIVE_RATE] = ((np.asarray(faces, dtype=np.float64) + 3.0) * EPS * np.asarray(conv) + 6 * EPS * np.asarray(convabs)) / V2
    return B


# ------------------------------------------------------------------ boundary maps
def boundary_fields(a, u, v, w, p, rho, mu, n_own=None):
    """(zone_ptr [Z+1], faces [nb], values [8, nb]) in the order of Mesh.boundary_index(): grouped by zone, ascending inside a zone"""
    zones = R.boundary_faces(a, n_own)
    zone_ptr = np.concatenate([[0], np.cumsum([len(f) for f in zones])]).astype(np.int64)
    faces = np.concatenate(zones).astype(np.int64) if zones else np.zeros(0, np.int64)
    out = np.zeros((B_N, len(faces)))
    if len(faces) == 0:
        return zone_ptr, faces, out
    zt = np.asarray(a["zone_type"])[np.asarray(a["face_zone"])[faces]]
    vec_bc = (zt == R.WALL) | (zt == R.VELOCITY_INLET)
    no_flux = (zt == R.WALL) | (zt == R.SYMMETRY)
    T = R.terms(a, u, v, w, p, rho, mu, None, faces)
    Uf, pf, phi = R.face_values(a, u, v, w, p, faces)
    A = np.asarray(a["face_area"], dtype=np.float64)[faces]
    n = np.asarray(a["face_normal"], dtype=np.float64).reshape(-1, 3)[faces]
    P = np.asarray(a["face_c0"])[faces]
    dx = np.asarray(a["face_centroid"], dtype=np.float64).reshape(-1, 3)[faces] - np.asarray(a["cell_centroid"], dtype=np.float64).reshape(-1, 3)[P]
    dist = np.sqrt((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])
    t = np.where(vec_bc[:, None], T[:, R.VISCOUS_FORCE:R.VISCOUS_FORCE + 3] / A[:, None], 0.0)
    tn = (t[:, 0] * n[:, 0] + t[:, 1] * n[:, 1]) + t[:, 2] * n[:, 2]
    s = t - tn[:, None] * n
    shear = np.where(vec_bc, np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]), 0.0)
    out[B_PRESSURE] = pf
    out[B_TRACTION_X], out[B_TRACTION_Y], out[B_TRACTION_Z] = t[:, 0], t[:, 1], t[:, 2]
    out[B_SHEAR_MAG] = shear
    out[B_Y_PLUS] = np.where(vec_bc, ((rho * np.sqrt(shear / rho)) * dist) / mu, 0.0)
    out[B_MASS_FLUX] = np.where(no_flux, 0.0, rho * phi)
    out[B_AREA] = A
    return zone_ptr, faces, out
