"""Case table of the assembly tests (tests/test_assembly_cases_cpu.py, tests/test_gpu_assembly_cases.py): meshes, fields, arms, plain restatements.

The face-loop assembly (orc_amd/csrc/assembly.hip, gradient_cell.hpp: grad_*_k, face_k, momentum_k, pressure_k, correction_k) branches on
quantities the hexahedral and prismatic fixtures of tests/test_gpu_assembly.py never move:
  * the faces of a cell (4 on a tetrahedron, 12 / 13 on a polyhedron): rows of the least-squares system, terms of every Green-Gauss sum;
  * the distances of the two centroids to the face centroid (LinearWeighted), equal on a uniform hexahedral mesh;
  * the limiter's ratio r and the sign of the face flux (which cell is downstream, which branch of psi);
  * the launch grid: momentum_k<false> walks the cell blocks XCD by XCD when its grid is a multiple of 8 (grid = ceil(n / 256) up to 2 048,
    per = ceil(n_blk / 8) blocks per XCD), and every grid-stride kernel takes a second round above 2 048 * 256 cells (faces: rows);
  * the cell numbering: momentum_k<true> reads a neighbour's NEW diagonal where `other < c`.  The generators number so that c0 < c1 on every
    interior face: seen from c0 the other cell is always above, seen from c1 always below.  A shuffled numbering has c0 > c1 on half of the
    faces (both combinations of side and age) and a SHALLOWER schedule (12 levels against 27 on `poly`: a random order has short
    ascending chains), so more cells per launch.
The meshes here sit on those.  What each is listed for (`why`) is re-derived from its arrays by the CPU test.

Every mesh comes from a generator of the repository (orc_amd.mesh.write_mixed_channel_msh / hex_channel, tests/meshgen.py), read back by
the oracle's reader where it is a file, and goes to the device and to the oracle from the same arrays.  Nothing is committed; the builders
are deterministic and cached per process — callers must not modify what they return.  No GPU."""
import functools
import hashlib
import os
import tempfile
from collections import namedtuple

import numpy as np

import helpers as H
import meshgen

RHO, MU = 1000.0, 1e-3
UD, CD1, CD2, TVD_LUD, TVD_QUICK, TVD_UMIST, TVD_UD, TVD_CD1 = range(8)
MOMENTUM = (UD, CD1, TVD_LUD, TVD_QUICK, TVD_UMIST, TVD_UD, TVD_CD1)  # CD2 is refused by device and oracle alike
MOMENTUM_NAMES = {UD: "UD", CD1: "CD1", TVD_LUD: "LUD", TVD_QUICK: "QUICK", TVD_UMIST: "UMIST", TVD_UD: "TVD_UD", TVD_CD1: "TVD_CD1"}
V_LINEAR, V_WEIGHTED, V_RHIE_CHOW = 0, 1, 2
P_LINEAR, P_WEIGHTED, P_SECOND_ORDER = 0, 1, 3
V_NAMES = {V_LINEAR: "vLinear", V_WEIGHTED: "vWeighted", V_RHIE_CHOW: "RhieChow"}
P_NAMES = {P_LINEAR: "pLinear", P_WEIGHTED: "pWeighted", P_SECOND_ORDER: "SecondOrder"}
GREEN_GAUSS, LEAST_SQUARES = 0, 2
JACOBI, REFERENCE_ORDER, TREE_ORDER = 1, 1, 0
BLOCK, MAX_GRID = 256, 2048  # kBlock and the cap of grid_for (orc_amd/csrc/common.hpp)

Arm = namedtuple("Arm", "momentum vinterp pinterp gradient q1")


def arm_name(arm):
    return "%s/%s/%s/%s/q1=%d" % (MOMENTUM_NAMES[arm.momentum], V_NAMES[arm.vinterp], P_NAMES[arm.pinterp],
                                  "LSQ" if arm.gradient == LEAST_SQUARES else "GG", arm.q1)


def arm_settings(arm, **more):
    return dict(momentum=arm.momentum, velocity_interpolation=arm.vinterp, pressure_interpolation=arm.pinterp,
                gradient_reconstruction=arm.gradient, q1_compat=arm.q1, **more)


# (a) 7 x 3 x 3 with Green-Gauss and q1_compat = 1; (b) Rhie-Chow + SecondOrder on least squares, q1_compat 1 and 0; (c) on Green-Gauss, 0
ARMS_A = [Arm(m, vi, pi, GREEN_GAUSS, 1) for m in MOMENTUM for vi in (V_LINEAR, V_WEIGHTED, V_RHIE_CHOW) for pi in (P_LINEAR, P_WEIGHTED, P_SECOND_ORDER)]
ARMS_B = [Arm(m, V_RHIE_CHOW, P_SECOND_ORDER, LEAST_SQUARES, q1) for m in MOMENTUM for q1 in (1, 0)]
ARMS_C = [Arm(m, V_RHIE_CHOW, P_SECOND_ORDER, GREEN_GAUSS, 0) for m in MOMENTUM]
ARMS = ARMS_A + ARMS_B + ARMS_C
assert (len(ARMS_A), len(ARMS_B), len(ARMS_C)) == (63, 14, 7) and len(set(ARMS)) == 84

# whole SIMPLE iterations: the 7 schemes on Rhie-Chow + SecondOrder, UMIST on LinearWeighted twice, UMIST and QUICK on least squares
ITERATION_ARMS = [Arm(m, V_RHIE_CHOW, P_SECOND_ORDER, GREEN_GAUSS, 1) for m in MOMENTUM] + [
    Arm(TVD_UMIST, V_WEIGHTED, P_WEIGHTED, GREEN_GAUSS, 1),
    Arm(TVD_UMIST, V_RHIE_CHOW, P_SECOND_ORDER, LEAST_SQUARES, 1), Arm(TVD_QUICK, V_RHIE_CHOW, P_SECOND_ORDER, LEAST_SQUARES, 1)]
ROUND2_ARM = Arm(TVD_UMIST, V_RHIE_CHOW, P_SECOND_ORDER, GREEN_GAUSS, 1)

# Arms whose outputs cannot differ, by the text of discretization.rs, with the reason; the CPU test finds exactly these.
# None: every scheme changes a_nb on some face (UD against TVD_UD: min(f, 0) against f * 0 / 2 on an inflow face; CD1 against TVD_CD1:
# f / 2 against min(f, 0) on a pressure boundary), every interpolation changes a flux or a face pressure, and both gradient settings enter
# Rhie-Chow's third term.
IDENTICAL_ARMS = {}

MESHES = ("tets", "poly", "poly_shuffled", "skew", "poly_x8", "hex_x16", "hex_round2", "hex_round2_cut")
SMALL_MESHES = MESHES[:6]             # every arm of the table
ITERATION_MESHES = MESHES[:4]         # whole SIMPLE iterations
LARGE_MESHES = MESHES[6:]             # one arm
# hex_round2: 2 080 = 8 * 260 blocks, so ceil(n_blk / 8) = n_blk / 8 and no XCD's range is cut.  hex_round2_cut: 528 125 cells = 2 063
# blocks, per = 258, 8 * 258 = 2 064: the last XCD's range ends at n_blk, a `per` rounded down loses seven blocks, and the last block
# has 253 live threads.
LARGE_DIMS = {"hex_round2": (130, 64, 64), "hex_round2_cut": (125, 65, 65)}
WHY = {
    "tets": dict(faces={4, 5, 6}, tri_zone_types={H.BC_WALL, H.BC_SYMMETRY}),
    "poly": dict(faces={4, 5, 6, 12, 13}, n=1496),
    "poly_shuffled": dict(faces={4, 5, 6, 12, 13}, n=1496, reversed_faces=0.4),
    "skew": dict(faces={5, 6}, non_orthogonal=True),
    "poly_x8": dict(faces={4, 5, 6, 12, 13}, grid=8, tri_zone_types={H.BC_VINLET, H.BC_PINLET, H.BC_POUTLET}),
    "hex_x16": dict(faces={6}, n=4080, grid=16, last_block=240),
    "hex_round2": dict(faces={6}, n=532480, n_blk=2080, cut=False),
    "hex_round2_cut": dict(faces={6}, n=528125, n_blk=2063, cut=True, last_block=253),
}
# the share of interior faces whose LinearWeighted weight dx0 / (dx0 + dx1) is further than 1e-3 from 1/2: at least this much.  The meshes
# give 0.73 (tets), 0.78 (poly, poly_x8), 0.67 (skew); a uniform hexahedral mesh gives 0.
WEIGHTED_SHARE = {"tets": 0.5, "poly": 0.5, "poly_shuffled": 0.5, "skew": 0.5, "poly_x8": 0.5}

_TMP = None


def _tmp(name):
    global _TMP
    if _TMP is None:
        _TMP = tempfile.mkdtemp(prefix="orc_assembly_")
    return os.path.join(_TMP, name + ".msh")


def all_types_bcs(set_zone, zone_names):
    """The velocity-inlet variant on the zones of the mixed channel (every location has a quadrilateral zone and, except INLET / OUTLET,
    a "_TRI" twin): velocity inlet on the whole -z side, pressure inlet on the triangles of the +z side (symmetry on its quadrilaterals),
    pressure outlet on the wall's triangles (moving wall on its quadrilaterals).  With the other meshes' channel set-up (wall and
    symmetry on triangles) every supported zone type sits on triangular as well as on quadrilateral faces."""
    for name in zone_names:
        if name.startswith("FLUID"):
            continue
        if name in ("PERIODIC_-Z", "PERIODIC_-Z_TRI"):
            set_zone(name, H.BC_VINLET, 0.0, (2e-5, -1e-5, 3e-4))
        elif name == "PERIODIC_+Z":
            set_zone(name, H.BC_SYMMETRY, 0.0, (0.0, 0.0, 0.0))
        elif name == "PERIODIC_+Z_TRI":
            set_zone(name, H.BC_PINLET, 0.004, (0.0, 0.0, 0.0))
        elif name == "WALL":
            set_zone(name, H.BC_WALL, 0.0, (5e-4, 0.0, 0.0))
        elif name == "WALL_TRI":
            set_zone(name, H.BC_POUTLET, 0.001, (0.0, 0.0, 0.0))
        elif name == "INLET":
            set_zone(name, H.BC_PINLET, 0.01, (0.0, 0.0, 0.0))
        elif name == "OUTLET":
            set_zone(name, H.BC_POUTLET, 0.0, (0.0, 0.0, 0.0))
        else:
            raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """-> (oracle mesh, MeshArrays)"""
    from oracle import pyoracle as oracle
    from orc_amd.mesh import MeshArrays, hex_channel, set_channel_bcs, write_mixed_channel_msh
    if name in ("tets", "poly", "poly_x8"):
        dims = {"tets": (20, 4, 3), "poly": (24, 5, 4), "poly_x8": (32, 5, 4)}[name]
        path = _tmp(name)
        write_mixed_channel_msh(path, *dims, lz=1e-4 * dims[2] * 1.3, polyhedra=(name != "tets"))
        om = oracle.Mesh.read(path)
        if name == "poly_x8":
            all_types_bcs(om.set_zone, om.zone_names())
        else:
            meshgen.mixed_channel_bcs(om.set_zone, om.zone_names(), top_wall_velocity=5e-4)
        a = MeshArrays(om.arrays())
    elif name == "skew":
        path = _tmp(name)
        info = meshgen.write_mixed_channel_msh(path, 10, 6, 4, skew=0.3, split="checker")
        om = oracle.Mesh.read(path)
        meshgen.mixed_channel_bcs(om.set_zone, info["zone_names"], top_wall_velocity=5e-4)
        a = MeshArrays(om.arrays())
    elif name == "poly_shuffled":
        a = meshgen.shuffle_cells(_mesh("poly")[1])
        om = oracle.Mesh.from_arrays(a)
    elif name == "hex_x16" or name in LARGE_DIMS:
        a = set_channel_bcs(hex_channel(*((17, 16, 15) if name == "hex_x16" else LARGE_DIMS[name])), top_wall_velocity=5e-4)
        om = oracle.Mesh.from_arrays(a)
    else:
        raise KeyError(name)
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return om, a


def mesh(name):
    """(oracle mesh, MeshArrays) of a case, built once per process"""
    return _mesh(name)


# ---------------------------------------------------------------- fields
def _interior_pair(a, n_faces_of_cell, want, avoid=()):
    """(cell, neighbour): the first cell with `want` faces and the first cell behind one of its interior faces, neither of them in `avoid`"""
    cfp, cf, c0, c1 = (np.asarray(a[k]) for k in ("cell_face_ptr", "cell_faces", "face_c0", "face_c1"))
    for c in np.flatnonzero(n_faces_of_cell == want):
        if int(c) in avoid:
            continue
        for f in cf[cfp[c]:cfp[c + 1]]:
            nb = int(c1[f] if c0[f] == c else c0[f])
            if c1[f] >= 0 and nb not in avoid:
                return int(c), nb
    raise LookupError("no cell with %d faces has a free interior face" % want)


def _with_neighbours(a, cells):
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    m = (c1 >= 0) & (np.isin(c0, list(cells)) | np.isin(c1, list(cells)))
    return set(cells) | set(c0[m].tolist()) | set(c1[m].tolist())


def planted_cells(a):
    """The cells the planted fields touch: `few` = (cell, neighbour) on the cell shape with the fewest faces (a tetrahedron where the mesh
    has one), `many` = on the shape with the most (a 13-face polyhedron where it has one), `component` = a pair elsewhere; no cell of one
    pair is a cell or a neighbour of another pair."""
    nf = np.diff(np.asarray(a["cell_face_ptr"]))
    few = _interior_pair(a, nf, int(nf.min()))
    taken = _with_neighbours(a, few)
    many = _interior_pair(a, nf, int(nf.max()), avoid=taken)
    taken = _with_neighbours(a, set(few) | set(many))
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    for f in np.flatnonzero(c1 >= 0)[::-1]:
        if int(c0[f]) not in taken and int(c1[f]) not in taken:
            return dict(few=few, many=many, component=(int(c0[f]), int(c1[f])))
    raise LookupError("no free interior face")


def fields(kind, a):
    """seeded: H.seeded_fields; rough: H.rough_fields; planted: rough, then the neighbour of `few` and of `many` gets its cell's velocity
    vector (a downstream neighbour with vnorm(dv) == 0) and the second cell of `component` gets the first one's u alone (dv.x == 0 with
    dv != 0: the reference divides by it)."""
    if kind == "seeded":
        return H.seeded_fields(a, seed=3)
    u, v, w, p = H.rough_fields(np.asarray(a["cell_centroid"]))
    if kind == "rough":
        return u, v, w, p
    assert kind == "planted"
    pl = planted_cells(a)
    for c, nb in (pl["few"], pl["many"]):
        u[nb], v[nb], w[nb] = u[c], v[c], w[c]
    c, nb = pl["component"]
    u[nb] = u[c]
    return u, v, w, p


FIELD_KINDS = ("seeded", "rough", "planted")


# ---------------------------------------------------------------- properties of a mesh, from its arrays
def interior_faces(a):
    return np.flatnonzero(np.asarray(a["face_c1"]) >= 0)


def weighted_weights(a):
    """dx0 / (dx0 + dx1) of every interior face: the weight LinearWeighted gives the second cell"""
    f = interior_faces(a)
    cc, fc = np.asarray(a["cell_centroid"]), np.asarray(a["face_centroid"])[f]
    dx0 = np.linalg.norm(cc[np.asarray(a["face_c0"])[f]] - fc, axis=1)
    dx1 = np.linalg.norm(cc[np.asarray(a["face_c1"])[f]] - fc, axis=1)
    return dx0 / (dx0 + dx1)


def level_depth(a):
    """levels of the in-place schedule (solver_state.cpp): level(c) = 1 + max level(j) over the neighbours j < c, 0 without one"""
    f = interior_faces(a)
    lo = np.minimum(np.asarray(a["face_c0"])[f], np.asarray(a["face_c1"])[f])
    hi = np.maximum(np.asarray(a["face_c0"])[f], np.asarray(a["face_c1"])[f])
    order = np.argsort(hi, kind="stable")
    level = [0] * len(a["cell_volume"])
    for l, h in zip(lo[order].tolist(), hi[order].tolist()):  # ascending hi: level[l] is final, since l < h
        if level[l] + 1 > level[h]:
            level[h] = level[l] + 1
    return max(level) + 1


def triangular_zone_types(a, path_nodes=None):
    """zone types that sit on at least one triangular boundary face: the generators put triangles in the zones named *_TRI"""
    zt = np.asarray(a["zone_type"])
    used = set(np.unique(np.asarray(a["face_zone"])).tolist())
    return {int(zt[i]) for i, nm in enumerate(a["zone_names"]) if nm.endswith("_TRI") and not nm.startswith("FLUID") and i in used}


def quadrilateral_zone_types(a):
    zt = np.asarray(a["zone_type"])
    used = set(np.unique(np.asarray(a["face_zone"])).tolist())
    return {int(zt[i]) for i, nm in enumerate(a["zone_names"]) if not nm.endswith("_TRI") and not nm.startswith("FLUID") and i in used}


# ---------------------------------------------------------------- the oracle side of one arm
@functools.lru_cache(maxsize=None)
def diffusion(name):
    """the oracle's diffusion matrix of a mesh (Csr, kept) and its value array"""
    from oracle import pyoracle as oracle
    a_di, *_ = oracle.build_momentum_diffusion_matrix(mesh(name)[0], MU)
    return a_di


@functools.lru_cache(maxsize=None)
def incoming_values(name):
    """Three momentum matrices with non-trivial diagonals (iteration >= 2 of the SIMPLE loop), as test_momentum_and_pressure_assembly_bit_exact
    builds them: initialize_momentum_matrix with diagonal (1 + |sin(c + k)| / 2) * 1e-6 -> (template Csr, [3 value arrays])"""
    from oracle import pyoracle as oracle
    om = mesh(name)[0]
    n = om.n_cells
    template = oracle.initialize_momentum_matrix(om)
    rp, ci, val = template.arrays()
    on = np.repeat(np.arange(n), np.diff(rp)) == ci
    out = []
    for k in range(3):
        v = val.copy()
        v[on] = (1.0 + 0.5 * np.abs(np.sin(np.arange(n) + k))) * 1e-6
        v.setflags(write=False)
        out.append(v)
    return template, out


def diagonal_mask(name):
    template = incoming_values(name)[0]
    rp, ci, _ = template.arrays()
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp)) == ci


Assembled = namedtuple("Assembled", "a b pe ap bp")  # 3 matrices, 3 right-hand sides, (mean, min, max), p' matrix, p' right-hand side


def oracle_assembly(name, f, arm):
    """build_momentum_advection_matrices on the incoming matrices, then build_pressure_correction_matrices on the result, frozen diagonals;
    any status but 0 (a singular least-squares matrix among them) raises"""
    from oracle import pyoracle as oracle
    om = mesh(name)[0]
    template, vals = incoming_values(name)
    mats = []
    for v in vals:
        m = template.clone()
        m.arrays()[2][:] = v
        mats.append(m)
    s = oracle.default_settings(**arm_settings(arm, frozen_diagonals=1))
    bu, bv, bw, pe = oracle.build_momentum_advection_matrices(mats[0], mats[1], mats[2], diffusion(name), om, *f, s, RHO)
    a_p, b_p = oracle.build_pressure_correction_matrices(om, *f, mats[0], mats[1], mats[2], s, RHO)
    return Assembled([m.arrays()[2].copy() for m in mats], [bu, bv, bw], pe, a_p.arrays()[2].copy(), b_p)


def digest(r):
    h = hashlib.sha256()
    for x in list(r.a) + list(r.b) + [np.asarray(r.pe), r.ap, r.bp]:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def same_bits(x, y):
    """equal doubles bit for bit, NaNs equal where both hold one (a NaN's payload and sign are not compared: the ISA's default NaN and
    the host's differ)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint64), y[~ny].view(np.uint64))


def oracle_gradients(name, f, cells=None):
    """per-cell calls of the oracle for `cells` (None: all): dict(gg_p1, gg_p0 [m, 3]: Green-Gauss grad p with q1_compat 1 / 0; gg_u [m, 3, 3];
    lsq_p [m, 3]; lsq_u [m, 3, 3]); a status but 0 (a singular normal matrix) fails"""
    import ctypes as C
    from oracle import pyoracle as oracle
    om = mesh(name)[0]
    cells = np.arange(om.n_cells) if cells is None else np.asarray(cells)
    u, v, w, p = (np.ascontiguousarray(x, dtype=np.float64) for x in f)
    L = oracle.lib()
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    vec, ten = oracle._Vec3(), (oracle._Vec3 * 3)()
    m = len(cells)
    out = dict(gg_p1=np.zeros((m, 3)), gg_p0=np.zeros((m, 3)), gg_u=np.zeros((m, 3, 3)), lsq_p=np.zeros((m, 3)), lsq_u=np.zeros((m, 3, 3)))
    pu, pv, pw, pp = dp(u), dp(v), dp(w), dp(p)
    for i, c in enumerate(cells.tolist()):
        cc = C.c_int64(c)
        for key, scheme, q1 in (("gg_p1", GREEN_GAUSS, 1), ("gg_p0", GREEN_GAUSS, 0), ("lsq_p", LEAST_SQUARES, 1)):
            st = L.or_calculate_pressure_gradient(om.ptr, pp, cc, C.c_int(scheme), C.c_int(q1), C.byref(vec))
            assert st == 0, (name, key, c, st)
            out[key][i] = (vec.x, vec.y, vec.z)
        for key, scheme in (("gg_u", GREEN_GAUSS), ("lsq_u", LEAST_SQUARES)):
            st = L.or_calculate_velocity_gradient(om.ptr, pu, pv, pw, cc, C.c_int(scheme), ten)
            assert st == 0, (name, key, c, st)
            out[key][i] = [(r.x, r.y, r.z) for r in ten]
    return out


# ---------------------------------------------------------------- the limiter's ratio, restated
UMIST_OUTCOMES = ("0", "2r", "(1+3r)/4", "(3+r)/4", "2")


def limiter_census(name, f, cells=None, q1=1):
    """Every (cell, interior face) visit of the TVD arm of discretization.rs:233-286 for `cells` (None: all), restated in numpy from the
    oracle's Green-Gauss velocity gradients, with the face flux of velocity interpolation Linear (n . (U_c + U_nb) / 2).
    -> dict of arrays over the visits: cell, nb, flux (outward from the cell), equal (down is the NEIGHBOUR and down's velocity equals the
    cell's: the vnorm(dv) == 0 branch with a real difference behind it), dv [m, 3] (zero rows where the cell is its own downstream),
    r [m, 3] (NaN where not evaluated), outcome [m, 3] (index into UMIST_OUTCOMES, -1 where r is not evaluated or NaN)."""
    om, a = mesh(name)
    cells = np.arange(om.n_cells) if cells is None else np.asarray(cells)
    u, v, w, _ = f
    vel = np.stack([u, v, w], axis=1)
    cfp, cf, c0, c1 = (np.asarray(a[k]) for k in ("cell_face_ptr", "cell_faces", "face_c0", "face_c1"))
    cnt = cfp[cells + 1] - cfp[cells]
    vc = np.repeat(cells, cnt)
    vf = cf[np.concatenate([np.arange(cfp[c], cfp[c + 1]) for c in cells.tolist()])]
    keep = c1[vf] >= 0
    vc, vf = vc[keep], vf[keep]
    side0 = c0[vf] == vc
    nb = np.where(side0, c1[vf], c0[vf])
    nrm = np.asarray(a["face_normal"])[vf] * np.where(side0, 1.0, -1.0)[:, None]
    flux = np.einsum("ij,ij->i", nrm, (vel[vc] + vel[nb]) / 2.0)
    down = np.where(flux > 0.0, nb, vc)
    dv = vel[down] - vel[vc]
    zero = np.sqrt((dv * dv).sum(axis=1)) == 0.0
    g = oracle_gradients(name, f, cells)["gg_u"]
    row = np.searchsorted(cells, vc)
    r_pa = np.asarray(a["cell_centroid"])[nb] - np.asarray(a["cell_centroid"])[vc]
    inner = np.einsum("ijk,ik->ij", g[row], r_pa)
    if q1:
        inner = inner[:, [0, 1, 1]]  # Float * Vector puts y into z
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 2.0 * inner / dv - 1.0
    r[zero] = np.nan
    cand = np.stack([2.0 * r, (1.0 + 3.0 * r) / 4.0, (3.0 + r) / 4.0, np.full_like(r, 2.0)], axis=2)
    with np.errstate(invalid="ignore"):
        low = np.fmin.reduce(cand, axis=2)
        which = np.argmin(np.where(np.isnan(cand), np.inf, cand), axis=2) + 1
        outcome = np.where(low <= 0.0, 0, which)
    outcome[np.isnan(r)] = -1
    return dict(cell=vc, nb=nb, face=vf, flux=flux, equal=zero & (down == nb), dv=dv, r=r, outcome=outcome)
