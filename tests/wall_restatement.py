"""numpy restatement of the wall distance (orc_amd/csrc/wall_distance.hip) and of the wall-damped Smagorinsky law (viscosity.hip), in
the operator order of DESIGN.md section 3 "Wall distance and wall damping".  numpy never fuses a multiply with an add, as the library
(-ffp-contract=off):

    wall faces   boundary faces (c1 < 0) of owned cells whose zone is in the wall mask (default: the zones of type Wall)
    r   = x_P - x_f                              s_f = (r.x*r.x + r.y*r.y) + r.z*r.z
    d_f = fabs((r.x*n.x + r.y*n.y) + r.z*n.z)     d_P = min{ d_f : s_f == min_g s_g }            (+inf without a wall face)

    l0 = cs * cbrt(V)
    MIN:        l = fmin(kappa * d, l0)
    VAN_DRIEST: yp = ((rho * u_tau) * d) / mu;  l = l0 * (-expm1(-(yp / a_plus)))
    m = mu + (rho * (l * l)) * g;  mu_t = fmin(fmax(m, mu_min), mu_max)
"""
import numpy as np

WALL = 3  # settings.FaceConditionTypes.Wall
NONE, MIN, VAN_DRIEST = 0, 1, 2
EPS = 2.0 ** -52
PAIRS_PER_CHUNK = 1 << 21  # cells x wall faces held at once by the brute-force search


def wall_mask(a, zones=None):
    """zones: None (type Wall) or names / indices -> bool per zone"""
    zt = np.asarray(a["zone_type"])
    if zones is None:
        return zt == WALL
    mask = np.zeros(len(zt), bool)
    for z in zones:
        mask[list(a["zone_names"]).index(z) if isinstance(z, str) else int(z)] = True
    return mask


def wall_faces(a, zones=None, n_owned=None):
    """ids of the wall faces, ascending"""
    c0, c1, fz = np.asarray(a["face_c0"]), np.asarray(a["face_c1"]), np.asarray(a["face_zone"])
    n_owned = len(a["cell_volume"]) if n_owned is None else n_owned
    return np.flatnonzero((c1 < 0) & (c0 < n_owned) & wall_mask(a, zones)[fz])


def wall_table(a, zones=None, n_owned=None):
    f = wall_faces(a, zones, n_owned)
    return np.asarray(a["face_centroid"], dtype=np.float64)[f], np.asarray(a["face_normal"], dtype=np.float64)[f]


def wall_distance(cell_centroid, table):
    """brute force over all (cell, wall face) pairs, in chunks of cells; table = (centroids [W, 3], normals [W, 3]) in any order"""
    cc = np.asarray(cell_centroid, dtype=np.float64)
    fc, fn = table
    n, W = len(cc), len(fc)
    out = np.full(n, np.inf)
    if W == 0 or n == 0:
        return out
    step = max(1, PAIRS_PER_CHUNK // W)
    for i0 in range(0, n, step):
        x = cc[i0:i0 + step]
        rx, ry, rz = (x[:, None, k] - fc[None, :, k] for k in range(3))
        s = (rx * rx + ry * ry) + rz * rz
        d = np.abs((rx * fn[None, :, 0] + ry * fn[None, :, 1]) + rz * fn[None, :, 2])
        out[i0:i0 + step] = np.where(s == s.min(axis=1)[:, None], d, np.inf).min(axis=1)
    return out


def mesh_wall_distance(a, zones=None, n_owned=None, table=None):
    """the wall distance of the owned cells of the mesh arrays `a` (ghost entries 0); table: all ranks' wall faces of a partition"""
    n = len(a["cell_volume"])
    n_owned = n if n_owned is None else n_owned
    out = np.zeros(n)
    out[:n_owned] = wall_distance(np.asarray(a["cell_centroid"])[:n_owned], table if table is not None else wall_table(a, zones, n_owned))
    return out


def damped_law(mode, g, vol, d, rho, mu, cs=0.17, kappa=0.41, a_plus=26.0, u_tau=0.0, mu_min=1e-12, mu_max=1e12, dtype=np.float64):
    """the clamped Smagorinsky viscosity with the damped length; mode NONE repeats viscosity_restatement.law"""
    T = dtype
    g, vol, d = (np.asarray(x, dtype=T) for x in (g, vol, d))
    with np.errstate(over="ignore", invalid="ignore"):
        l = T(cs) * np.cbrt(vol)
        if mode == MIN:
            l = np.fmin(T(kappa) * d, l)
        elif mode == VAN_DRIEST:
            yp = ((T(rho) * T(u_tau)) * d) / T(mu)
            l = l * (-np.expm1(-(yp / T(a_plus))))
        m = T(mu) + (T(rho) * (l * l)) * g
    return np.fmin(np.fmax(m, T(mu_min)), T(mu_max))
