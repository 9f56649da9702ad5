"""mesh::Mesh of the reference (src/mesh.rs) as flat arrays + the device-resident OrcMesh handle."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .settings import FaceConditionTypes

_F64 = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_I32 = C.POINTER(C.c_int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class MeshArrays(dict):
    """Plain-array image of mesh::Mesh: the argument list of orc_mesh_create.

    keys: face_c0, face_c1 (-1 = boundary), face_zone, face_area, face_normal[F,3], face_centroid[F,3],
    cell_centroid[n,3], cell_volume, cell_face_ptr, cell_faces, zone_type, zone_scalar, zone_vector[Z,3],
    zone_names.
    """

    @property
    def n_cells(self):
        return len(self["cell_volume"])

    @property
    def n_faces(self):
        return len(self["face_area"])

    def get_face_zone(self, name):
        """mesh.get_face_zone(name) (mesh.rs:189-195): index of the zone; KeyError like the reference's panic."""
        try:
            return self["zone_names"].index(name)
        except ValueError:
            raise KeyError("face zone '%s' should exist in mesh" % name)

    def set_zone(self, name, zone_type, scalar=0.0, vector=(0.0, 0.0, 0.0)):
        k = self.get_face_zone(name)
        self["zone_type"][k] = zone_type
        self["zone_scalar"][k] = scalar
        self["zone_vector"][k] = vector


def splitmix64_uniform(n, seed=0x4F5243, ids=None):
    """uniform[-1,1) f64 from splitmix64, seed "ORC" (SURVEY §8d synthetic inputs); vectorised, stateless.
    ids: the stream positions (0-based) to evaluate instead of 0 .. n-1 — a rank's cells by their GLOBAL ids get the whole mesh's numbers."""
    idx = np.arange(1, n + 1, dtype=np.uint64) if ids is None else np.asarray(ids, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / (1 << 53)) - 1.0


ZONE_NAMES = ["FLUID", "INLET", "OUTLET", "PERIODIC_-Z", "PERIODIC_+Z", "TOP_WALL", "BOTTOM_WALL"]


def hex_channel(nx, ny, nz, lx=0.002, ly=0.001, lz=None):
    """Synthetic structured hex channel in ORC's conventions; lz defaults to 0.1 mm per cell."""
    if lz is None:
        lz = 1e-4 * nz
    L = lib()
    nc, nf, ncf = C.c_int64(), C.c_int64(), C.c_int64()
    check(L.orc_hex_channel_sizes(C.c_int64(nx), C.c_int64(ny), C.c_int64(nz), C.byref(nc), C.byref(nf), C.byref(ncf)))
    n, F, ncf = nc.value, nf.value, ncf.value
    a = MeshArrays(
        face_c0=np.empty(F, np.int64), face_c1=np.empty(F, np.int64), face_zone=np.empty(F, np.int32),
        face_area=np.empty(F), face_normal=np.empty((F, 3)), face_centroid=np.empty((F, 3)),
        cell_centroid=np.empty((n, 3)), cell_volume=np.empty(n), cell_face_ptr=np.empty(n + 1, np.int64),
        cell_faces=np.empty(ncf, np.int64),
        zone_type=np.array([FaceConditionTypes.Interior] + [FaceConditionTypes.Wall] * 6, dtype=np.int32),
        zone_scalar=np.zeros(7), zone_vector=np.zeros((7, 3)), zone_names=list(ZONE_NAMES))
    check(L.orc_hex_channel_generate(
        C.c_int64(nx), C.c_int64(ny), C.c_int64(nz), C.c_double(lx), C.c_double(ly), C.c_double(lz),
        a["face_c0"].ctypes.data_as(_I64), a["face_c1"].ctypes.data_as(_I64), a["face_zone"].ctypes.data_as(_I32),
        a["face_area"].ctypes.data_as(_F64), a["face_normal"].ctypes.data_as(_F64), a["face_centroid"].ctypes.data_as(_F64),
        a["cell_centroid"].ctypes.data_as(_F64), a["cell_volume"].ctypes.data_as(_F64),
        a["cell_face_ptr"].ctypes.data_as(_I64), a["cell_faces"].ctypes.data_as(_I64)))
    return a


def hex_channel_nodes(a, nx, ny, nz, lx=0.002, ly=0.001, lz=None):
    """Node geometry for the arrays of hex_channel(nx, ny, nz, ...), which carry none: (vertices [V, 3], face_node_ptr, face_nodes) as
    MeshData.nodes() returns them, rebuilt from the lattice — a face's four nodes are its centroid plus and minus half a cell in its two
    tangential directions, node (i, j, k) has id (k (ny + 1) + j)(nx + 1) + i.  The winding of a cycle is not the file's; the cuts derive
    the orientation from the geometry, so either serves (Mesh.set_nodes)."""
    if lz is None:
        lz = 1e-4 * nz
    h = np.array([lx / nx, ly / ny, lz / nz])
    n1 = np.array([nx + 1, ny + 1, nz + 1])
    k, j, i = np.meshgrid(np.arange(n1[2]), np.arange(n1[1]), np.arange(n1[0]), indexing="ij")
    vert = np.stack([i.ravel() * h[0], j.ravel() * h[1], k.ravel() * h[2]], axis=1)
    fc, fn = np.asarray(a["face_centroid"]), np.asarray(a["face_normal"])
    axis = np.argmax(np.abs(fn), axis=1)
    F = len(fc)
    nodes = np.zeros((F, 4), np.int64)
    for ax in range(3):
        sel = np.where(axis == ax)[0]
        t1, t2 = [q for q in range(3) if q != ax]
        base = np.rint(fc[sel] / h[None, :] * 2).astype(np.int64)  # twice the lattice coordinate: even along the axis, odd across
        for q, (s1, s2) in enumerate([(-1, -1), (1, -1), (1, 1), (-1, 1)]):
            ijk = base.copy()
            ijk[:, t1] += s1
            ijk[:, t2] += s2
            ijk //= 2
            nodes[sel, q] = (ijk[:, 2] * n1[1] + ijk[:, 1]) * n1[0] + ijk[:, 0]
    return vert, np.arange(F + 1, dtype=np.int64) * 4, nodes.reshape(-1)


def write_hex_channel_msh(path, nx, ny, nz, lx=0.002, ly=0.001, lz=None):
    if lz is None:
        lz = 1e-4 * nz
    check(lib().orc_hex_channel_write_msh(path.encode(), C.c_int64(nx), C.c_int64(ny), C.c_int64(nz), C.c_double(lx),
                                          C.c_double(ly), C.c_double(lz)))


def write_mixed_channel_msh(path, nx, ny, nz, lx=0.002, ly=0.001, lz=None, polyhedra=False):
    """BASELINE config 5 workload (orc_mixed_channel_write_msh): tet / pyramid / prism / hex channel as a TGRID file;
    polyhedra=True (orc_poly_channel_write_msh) adds a region of agglomerated polyhedral cells (12-face rhombic dodecahedra).
    Returns (n_cells, n_faces)."""
    if lz is None:
        lz = 1e-4 * nz
    nc, nf = C.c_int64(), C.c_int64()
    fn = lib().orc_poly_channel_write_msh if polyhedra else lib().orc_mixed_channel_write_msh
    check(fn(path.encode(), C.c_int64(nx), C.c_int64(ny), C.c_int64(nz), C.c_double(lx), C.c_double(ly),
             C.c_double(lz), C.byref(nc), C.byref(nf)))
    return nc.value, nf.value


def renumber_cells(a, new_of_old):
    """The same mesh with cell `c` renamed new_of_old[c] (faces keep their ids, orientation and per-cell ascending order):
    what a mesh generator with another cell numbering would have written.  Used to measure how much the products depend
    on the numbering (config 5) and to undo it with the RCM ordering of orc_mesh_partition."""
    new_of_old = np.asarray(new_of_old, dtype=np.int64)
    n = len(new_of_old)
    old_of_new = np.empty(n, np.int64)
    old_of_new[new_of_old] = np.arange(n)
    c0, c1 = np.asarray(a["face_c0"]), np.asarray(a["face_c1"])
    cfp, cf = np.asarray(a["cell_face_ptr"]), np.asarray(a["cell_faces"])
    counts = np.diff(cfp)[old_of_new]
    new_cfp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    # face-list positions of the new cells, one after the other: old start of each cell + offset inside it
    idx = (np.repeat(cfp[:-1][old_of_new], counts) + (np.arange(int(new_cfp[-1]), dtype=np.int64) - np.repeat(new_cfp[:-1], counts))) if n else np.zeros(0, np.int64)
    out = MeshArrays(a)
    out.update(face_c0=new_of_old[c0], face_c1=np.where(c1 >= 0, new_of_old[np.maximum(c1, 0)], -1),
               cell_centroid=np.asarray(a["cell_centroid"])[old_of_new].copy(), cell_volume=np.asarray(a["cell_volume"])[old_of_new].copy(),
               cell_face_ptr=new_cfp, cell_faces=cf[idx].copy())
    return out


def set_channel_bcs(a, top_wall_velocity=0.0, dp_dx=5.0, dx=0.002):
    """Boundary conditions of tests::channel_flow::solve_channel_flow (tests.rs:60-76)."""
    T = FaceConditionTypes
    if "TOP_WALL" in a["zone_names"]:
        a.set_zone("TOP_WALL", T.Wall, 0.0, (top_wall_velocity, 0.0, 0.0))
        a.set_zone("BOTTOM_WALL", T.Wall)
    else:
        a.set_zone("WALL", T.Wall)
    a.set_zone("INLET", T.PressureInlet, -dp_dx * dx)
    a.set_zone("OUTLET", T.PressureOutlet, 0.0)
    a.set_zone("PERIODIC_-Z", T.Symmetry)
    a.set_zone("PERIODIC_+Z", T.Symmetry)
    return a


def set_mixed_channel_bcs(a, top_wall_velocity=0.0, dp_dx=5.0, dx=0.002):
    """tests.rs:60-76 on the zones of orc_mixed_channel_write_msh (every location has a quadrilateral zone and a "_TRI" twin)."""
    T = FaceConditionTypes
    for name in list(a["zone_names"]):
        base = name[:-4] if name.endswith("_TRI") else name
        if base == "WALL":
            a.set_zone(name, T.Wall, 0.0, (top_wall_velocity, 0.0, 0.0))
        elif base == "INLET":
            a.set_zone(name, T.PressureInlet, -dp_dx * dx)
        elif base == "OUTLET":
            a.set_zone(name, T.PressureOutlet, 0.0)
        elif base.startswith("PERIODIC"):
            a.set_zone(name, T.Symmetry)
    return a


def wall_search_stats(reset=False):
    """orc_debug_wall_search -> dict(wall_faces, tile, tiles, tile_visits, waves): the table of the last wall-distance search and the
    tile visits and waves of all searches since the last reset"""
    out = (C.c_longlong * 5)()
    check(lib().orc_debug_wall_search(out, C.c_int(1 if reset else 0)))
    return dict(zip(("wall_faces", "tile", "tiles", "tile_visits", "waves"), (int(x) for x in out)))


def probe_search_stats(reset=False):
    """orc_debug_probe_search -> dict(tile, tiles, tile_visits, waves, slabs, walk_moves): the cell tiles and slabs of the last point
    search, and the tile visits, waves and walk moves of all searches since the last reset"""
    out = (C.c_longlong * 6)()
    check(lib().orc_debug_probe_search(out, C.c_int(1 if reset else 0)))
    return dict(zip(("tile", "tiles", "tile_visits", "waves", "slabs", "walk_moves"), (int(x) for x in out)))


class Probes:
    """Points located in the cells of a mesh (OrcProbes*), kept on the device: what Solver.sample and the probe history read.
    cell (ORC order, as Solver.get_fields()), status (settings.ProbeStatus), steps (moves of the walk), zone (of the boundary face an
    OUTSIDE point left through, else -1), excess (the largest g of the final cell: <= 0 exactly when inside)."""

    def __init__(self, mesh, points, cull=None, slabs=0):
        self.mesh = mesh  # keeps the mesh alive: a probe set goes before its mesh
        self.points = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        n = len(self.points)
        st = C.c_int(0)
        if cull is None and not slabs:
            ptr = lib().orc_probes_create(mesh.ptr, C.c_int64(n), self.points.ctypes.data_as(_F64), C.byref(st))
        else:
            ptr = lib().orc_debug_probes_locate(mesh.ptr, C.c_int64(n), self.points.ctypes.data_as(_F64), C.c_int(0 if cull is False else 1),
                                                C.c_int(int(slabs)), C.byref(st))
        check(st.value)
        self.ptr = C.c_void_p(ptr)
        self.cell, self.status = np.zeros(n, np.int64), np.zeros(n, np.int32)
        self.steps, self.zone, self.excess = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
        check(lib().orc_probes_get(self.ptr, self.cell.ctypes.data_as(_I64), self.status.ctypes.data_as(_I32), self.steps.ctypes.data_as(_I32),
                                   self.zone.ctypes.data_as(_I32), self.excess.ctypes.data_as(_F64)))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_probes_destroy(self.ptr)
            self.ptr = None

    def __len__(self):
        return int(lib().orc_probes_count(self.ptr))

    @property
    def inside(self):
        return self.status == 0

    def bench_locate(self, cull=True, reps=5):
        """orc_bench_probe_locate: HIP-event (ms per search and fold, ms per walk) of these points on scratch buffers"""
        ms = np.zeros(2)
        check(lib().orc_bench_probe_locate(self.mesh.ptr, self.ptr, C.c_int(1 if cull else 0), C.c_int(reps), ms.ctypes.data_as(_F64)))
        return float(ms[0]), float(ms[1])


def group_limits():
    """orc_group_limits -> dict(fields, chunk, slots, max_groups): the fields one launch of a volume report takes (more run in
    batches), the list entries of one workgroup and of one lane, the largest n_groups.  Needs no device."""
    v = [C.c_int32(0) for _ in range(4)]
    check(lib().orc_group_limits(*[C.byref(x) for x in v]))
    return dict(zip(("fields", "chunk", "slots", "max_groups"), (int(x.value) for x in v)))


def bin_ids(cell_centroid, direction, edges):
    """The labels of Mesh.bin_cells: s = (c.x d.x + c.y d.y) + c.z d.z with d = direction / |direction|, in float64 numpy; bin k holds the
    cells with edges[k] <= s < edges[k + 1] (the lower edge belongs to the bin, the upper one to the next); a cell below edges[0], at or
    above edges[-1], or with s NaN gets -1.  edges must ascend strictly.  -> (ids int32 [n], number of bins)"""
    c = np.asarray(cell_centroid, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    norm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if not np.isfinite(norm) or norm == 0.0:
        raise ValueError("bin_cells: the direction must be finite and not zero")
    if len(e) < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("bin_cells: at least two finite, strictly ascending edges")
    d = d / norm
    s = (c[:, 0] * d[0] + c[:, 1] * d[1]) + c[:, 2] * d[2]
    k = np.searchsorted(e, s, side="right") - 1
    k[(k >= len(e) - 1) | np.isnan(s)] = -1
    return k.astype(np.int32), len(e) - 1


def box_ids(cell_centroid, lo, hi):
    """The labels of Mesh.box_cells: 0 where lo[k] <= centroid[k] < hi[k] in every coordinate k, else -1 -> ids int32 [n]"""
    c = np.asarray(cell_centroid, dtype=np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    inside = np.all((c >= lo[None, :]) & (c < hi[None, :]), axis=1)
    return np.where(inside, 0, -1).astype(np.int32)


def check_group_ids(ids, n_cells, n_groups=None):
    """ids as orc_cell_groups_create takes them (int32 [n_cells], -1 = in no group) and n_groups (None: the largest id + 1, at least 1);
    raises ValueError for what the library would refuse"""
    a = np.asarray(ids)
    if a.ndim != 1 or len(a) != n_cells:
        raise ValueError("cell groups: one id per cell (%d), got shape %s" % (n_cells, a.shape))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("cell groups: the ids must be integers")
    if n_groups is None:
        n_groups = max(int(a.max()) + 1, 1) if len(a) else 1
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError("cell groups: n_groups must be at least 1")
    if len(a) and (int(a.min()) < -1 or int(a.max()) >= n_groups):
        raise ValueError("cell groups: an id lies outside [-1, %d)" % n_groups)
    return np.ascontiguousarray(a, dtype=np.int32), n_groups


class CellGroups:
    """A labelling of the cells of a mesh (OrcCellGroups*), kept on the device as lists: what the volume reports reduce over.
    len() = the groups; group_ptr [G + 1] into cells; cells = the ORC ids, ascending inside a group; chunk = the list entries one
    workgroup of a report takes."""

    def __init__(self, mesh, ids, n_groups=None):
        self.mesh = mesh  # keeps the mesh alive: a group set goes before its mesh
        self.ids, n_groups = check_group_ids(ids, mesh.n_cells, n_groups)
        st = C.c_int(0)
        ptr = lib().orc_cell_groups_create(mesh.ptr, C.c_int32(n_groups), self.ids.ctypes.data_as(_I32), C.byref(st))
        check(st.value)
        self.ptr = C.c_void_p(ptr)
        self.group_ptr = np.zeros(n_groups + 1, np.int64)
        chunk = C.c_int32(0)
        check(lib().orc_cell_groups_get(self.ptr, self.group_ptr.ctypes.data_as(_I64), None, C.byref(chunk)))
        self.cells = np.zeros(max(int(self.group_ptr[-1]), 1), np.int64)
        check(lib().orc_cell_groups_get(self.ptr, None, self.cells.ctypes.data_as(_I64), None))
        self.cells = self.cells[:int(self.group_ptr[-1])]
        self.chunk = int(chunk.value)

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_cell_groups_destroy(self.ptr)
            self.ptr = None

    def __len__(self):
        return int(lib().orc_cell_groups_count(self.ptr))

    @property
    def count(self):
        """cells per group"""
        return np.diff(self.group_ptr)


class Tracers:
    """Tracer particles in the cells of a mesh (OrcTracers*), kept on the device: what Solver.advect moves and Solver.sample_tracers
    reads.  positions [n, 3], cell (ORC order), status (settings.TracerStatus), zone (of the boundary face a LEFT particle went
    through, else -1), age (the signed sum of the accepted h), steps (accepted substeps): each read from the device when asked for."""

    def __init__(self, mesh, points):
        self.mesh = mesh  # keeps the mesh alive: a tracer set goes before its mesh
        self.seeds = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        st = C.c_int(0)
        ptr = lib().orc_tracers_create(mesh.ptr, C.c_int64(len(self.seeds)), self.seeds.ctypes.data_as(_F64), C.byref(st))
        check(st.value)
        self.ptr = C.c_void_p(ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_tracers_destroy(self.ptr)
            self.ptr = None

    def __len__(self):
        return int(lib().orc_tracers_count(self.ptr))

    def get(self):
        """orc_tracers_get: dict(positions, cell, status, zone, age, steps) in one call"""
        n = len(self)
        out = dict(positions=np.zeros((n, 3)), cell=np.zeros(n, np.int64), status=np.zeros(n, np.int32), zone=np.zeros(n, np.int32),
                   age=np.zeros(n), steps=np.zeros(n, np.int64))
        check(lib().orc_tracers_get(self.ptr, out["positions"].ctypes.data_as(_F64), out["cell"].ctypes.data_as(_I64),
                                    out["status"].ctypes.data_as(_I32), out["zone"].ctypes.data_as(_I32), out["age"].ctypes.data_as(_F64),
                                    out["steps"].ctypes.data_as(_I64)))
        return out

    def _one(self, slot, shape, dtype, ctype):
        a = np.zeros(shape, dtype)
        args = [None] * 6
        args[slot] = a.ctypes.data_as(ctype)
        check(lib().orc_tracers_get(self.ptr, *args))
        return a

    positions = property(lambda self: self._one(0, (len(self), 3), np.float64, _F64))
    cell = property(lambda self: self._one(1, len(self), np.int64, _I64))
    status = property(lambda self: self._one(2, len(self), np.int32, _I32))
    zone = property(lambda self: self._one(3, len(self), np.int32, _I32))
    age = property(lambda self: self._one(4, len(self), np.float64, _F64))
    steps = property(lambda self: self._one(5, len(self), np.int64, _I64))

    @property
    def active(self):
        return self.status == 0


def cut_limits():
    """orc_cut_limits -> dict(max_points, scan_chunk): the cut points one cell may carry (ORC_CUT_MAX_POINTS) and the entries one
    workgroup of the scan takes.  Needs no device."""
    a, b = C.c_int32(0), C.c_int32(0)
    check(lib().orc_cut_limits(C.byref(a), C.byref(b)))
    return dict(max_points=int(a.value), scan_chunk=int(b.value))


class Cut:
    """A cut surface (OrcCut*), kept on the device: the polygons of Mesh.slice / cut_nodes / isosurface and Solver.isosurface, in
    ascending ORC cell id.  poly_ptr [P + 1] into the points; cell [P] the owner (ORC id); points [NP, 3]; keys [NP, 2] the (lo, hi)
    node ids of every point's cut edge; area_vector [P, 3]; area [P] its length; skipped = dict(nonfinite, overflow), the cells left
    out and why.  Each array is read from the device when first asked for."""

    def __init__(self, mesh, ptr, status):
        check(status)
        self.mesh = mesh  # keeps the mesh alive: a cut goes before its mesh
        self.ptr = C.c_void_p(ptr)
        v = [C.c_int64(0) for _ in range(4)]
        check(lib().orc_cut_sizes(self.ptr, *[C.byref(x) for x in v]))
        self.n_polygons, self.n_points = int(v[0].value), int(v[1].value)
        self.skipped = dict(nonfinite=int(v[2].value), overflow=int(v[3].value))
        self._got = None

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_cut_destroy(self.ptr)
            self.ptr = None

    def __len__(self):
        return self.n_polygons

    def _get(self):
        if self._got is None:
            P, NP = self.n_polygons, self.n_points
            g = dict(poly_ptr=np.zeros(P + 1, np.int64), cell=np.zeros(P, np.int64), points=np.zeros((NP, 3)), lo=np.zeros(NP, np.int64),
                     hi=np.zeros(NP, np.int64), area_vector=np.zeros((P, 3)))
            check(lib().orc_cut_get(self.ptr, g["poly_ptr"].ctypes.data_as(_I64), g["cell"].ctypes.data_as(_I64), g["points"].ctypes.data_as(_F64),
                                    g["lo"].ctypes.data_as(_I64), g["hi"].ctypes.data_as(_I64), g["area_vector"].ctypes.data_as(_F64)))
            g["keys"] = np.stack([g.pop("lo"), g.pop("hi")], axis=1)
            self._got = g
        return self._got

    poly_ptr = property(lambda self: self._get()["poly_ptr"])
    cell = property(lambda self: self._get()["cell"])
    points = property(lambda self: self._get()["points"])
    keys = property(lambda self: self._get()["keys"])
    area_vector = property(lambda self: self._get()["area_vector"])

    @property
    def area(self):
        a = self.area_vector
        return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])

    def welded(self):
        """-> (points [M, 3], nodes [NP], first [M]): the unique points by key in ascending (lo, hi), the polygon connectivity
        (poly_ptr indexes it) and, per unique point, its first occurrence among the polygon vertices.  A key gives the same bits in every
        cell that shares its edge, so any occurrence serves."""
        k = self.keys
        if len(k) == 0:
            return np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64)
        _, first, nodes = np.unique(k, axis=0, return_index=True, return_inverse=True)
        return self.points[first], np.asarray(nodes, np.int64).reshape(-1), np.asarray(first, np.int64)

    def integrate(self, per_polygon_vectors):
        """sum over the polygons of v . A on the host, polygon by polygon in order: ((v.x A.x + v.y A.y) + v.z A.z) accumulated left to
        right.  per_polygon_vectors [P, 3], e.g. rho (u, v, w) from Solver.sample_cut(cut, "uvw", "cell") for the mass flow."""
        v = np.asarray(per_polygon_vectors, dtype=np.float64).reshape(-1, 3)
        a = self.area_vector
        if len(v) != len(a):
            raise ValueError("integrate: one vector per polygon (%d), got %d" % (len(a), len(v)))
        total = 0.0
        for t in ((v[:, 0] * a[:, 0] + v[:, 1] * a[:, 1]) + v[:, 2] * a[:, 2]).tolist():
            total = total + t
        return total

    def sample_cells(self, fields):
        """orc_cut_sample_cells: {name: ndarray[n_cells] in ORC order} -> {name: ndarray[P]}, every polygon its owner cell's value"""
        names = list(fields)
        n = self.mesh.n_cells
        src = np.ascontiguousarray(np.stack([np.asarray(fields[k], dtype=np.float64).reshape(n) for k in names]))
        out = np.zeros((len(names), self.n_polygons))
        check(lib().orc_cut_sample_cells(self.ptr, C.c_int32(len(names)), src.ctypes.data_as(_F64), out.ctypes.data_as(_F64)))
        return {k: out[q] for q, k in enumerate(names)}


class Mesh:
    """Device-resident mesh (OrcMesh*)."""

    def __init__(self, arrays, ordering=None, nodes=None):
        """ordering: None = ORC's numbering; 1 = RCM, 2 = geometric (orc_mesh_create_reordered: internal renumbering,
        fields still in ORC order).  nodes: a MeshData (or its nodes() tuple) for set_nodes()."""
        a = arrays
        self.arrays = a
        self._keep = [_i64(a["face_c0"]), _i64(a["face_c1"]), _i32(a["face_zone"]), _f64(a["face_area"]),
                      _f64(a["face_normal"]), _f64(a["face_centroid"]), _f64(a["cell_centroid"]), _f64(a["cell_volume"]),
                      _i64(a["cell_face_ptr"]), _i64(a["cell_faces"]), _i32(a["zone_type"]), _f64(a["zone_scalar"]),
                      _f64(a["zone_vector"])]
        k = self._keep
        st = C.c_int(0)
        args = [C.c_int64(len(k[7])), C.c_int64(len(k[3])), C.c_int32(len(k[10])), k[0].ctypes.data_as(_I64),
                k[1].ctypes.data_as(_I64), k[2].ctypes.data_as(_I32), k[3].ctypes.data_as(_F64), k[4].ctypes.data_as(_F64),
                k[5].ctypes.data_as(_F64), k[6].ctypes.data_as(_F64), k[7].ctypes.data_as(_F64), k[8].ctypes.data_as(_I64),
                k[9].ctypes.data_as(_I64), k[10].ctypes.data_as(_I32), k[11].ctypes.data_as(_F64), k[12].ctypes.data_as(_F64)]
        if ordering:
            lib().orc_mesh_create_reordered.restype = C.c_void_p
            self.ptr = lib().orc_mesh_create_reordered(*args, C.c_int32(int(ordering)), C.byref(st))
        else:
            self.ptr = lib().orc_mesh_create(*args, C.byref(st))
        check(st.value)
        self.ptr = C.c_void_p(self.ptr)
        self._keep = None
        self.n_cells = lib().orc_mesh_n_cells(self.ptr)
        self.nnz = lib().orc_mesh_nnz(self.ptr)
        self.n_vertices = 0
        if nodes is not None:
            self.set_nodes(nodes)

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_mesh_destroy(self.ptr)
            self.ptr = None

    def cell_order(self):
        """global_ids[c] = ORC index of internal cell c (identity unless the mesh was created reordered)"""
        g = np.empty(self.n_cells, np.int64)
        check(lib().orc_mesh_cell_order(self.ptr, g.ctypes.data_as(_I64)))
        return g

    def update_zones(self):
        a = self.arrays
        zt, zs, zv = _i32(a["zone_type"]), _f64(a["zone_scalar"]), _f64(a["zone_vector"])
        check(lib().orc_mesh_update_zones(self.ptr, zt.ctypes.data_as(_I32), zs.ctypes.data_as(_F64), zv.ctypes.data_as(_F64)))

    def boundary_index(self):
        """orc_mesh_boundary_index: the boundary faces of owned cells grouped by zone, as the surface reports walk them (built on
        the device at first use, then kept) -> (zone_ptr[Z + 1], faces[zone_ptr[Z]] ascending inside a zone and in the mesh's
        internal face numbering, n_builds, chunk = faces per workgroup of a report)"""
        zp = np.zeros(len(self.arrays["zone_type"]) + 1, np.int64)
        nb, chunk = C.c_int64(0), C.c_int32(0)
        check(lib().orc_mesh_boundary_index(self.ptr, zp.ctypes.data_as(_I64), None, C.byref(nb), C.byref(chunk)))
        faces = np.zeros(max(int(zp[-1]), 1), np.int32)
        check(lib().orc_mesh_boundary_index(self.ptr, zp.ctypes.data_as(_I64), faces.ctypes.data_as(_I32), C.byref(nb), C.byref(chunk)))
        return zp, faces[:int(zp[-1])], int(nb.value), int(chunk.value)

    def _wall_mask(self, zones):
        """zones: None (the zones of type Wall) or a list of zone names or indices -> int32 mask per zone, or None"""
        if zones is None:
            return None
        mask = np.zeros(len(self.arrays["zone_type"]), np.int32)
        for z in zones:
            mask[list(self.arrays["zone_names"]).index(z) if isinstance(z, str) else int(z)] = 1
        return mask

    def wall_distance(self, zones=None):
        """orc_mesh_wall_distance: per cell the distance to the plane of the wall face with the nearest centroid (+inf without a wall
        face; the ghost entries of a partitioned mesh are 0), cell order as Solver.get_fields().  zones: the wall zones by name or
        index, None = the zones of type Wall.  Searched on the device at first use and kept until update_zones() changes a wall."""
        mask = self._wall_mask(zones)
        d = np.zeros(self.n_cells)
        check(lib().orc_mesh_wall_distance(self.ptr, None if mask is None else mask.ctypes.data_as(_I32), d.ctypes.data_as(_F64)))
        return d

    def debug_wall_distance(self, zones=None, cull=True):
        """orc_debug_wall_distance: the same search past the cache; cull=False walks the whole wall table for every cell"""
        mask = self._wall_mask(zones)
        d = np.zeros(self.n_cells)
        check(lib().orc_debug_wall_distance(self.ptr, None if mask is None else mask.ctypes.data_as(_I32), C.c_int(1 if cull else 0),
                                            d.ctypes.data_as(_F64)))
        return d

    def bench_wall_distance(self, cull=True, reps=5):
        """orc_bench_wall_distance: HIP-event ms per launch of the search kernel on the default mask's table"""
        ms = C.c_double(0.0)
        check(lib().orc_bench_wall_distance(self.ptr, C.c_int(1 if cull else 0), C.c_int(reps), C.byref(ms)))
        return ms.value

    def locate(self, points, cull=None, slabs=0):
        """orc_probes_create: the points [n, 3] located in the cells of this mesh, all at once on the device -> Probes.  cull=False
        (every cell for every point) and slabs (a forced number of cell slabs) go through orc_debug_probes_locate: same result."""
        return Probes(self, points, cull, slabs)

    def probe_search_stats(self, reset=False):
        """the counters of the point search (module function probe_search_stats)"""
        return probe_search_stats(reset)

    def cell_groups(self, ids, n_groups=None):
        """orc_cell_groups_create: ids[c] = the group of ORC cell c in [0, n_groups), -1 = in no group (n_groups=None: the largest
        id + 1) -> CellGroups, what Solver.group_report and its relatives reduce over.  A partitioned mesh is refused."""
        return CellGroups(self, ids, n_groups)

    def bin_cells(self, direction, edges):
        """Bins along a direction -> CellGroups with len(edges) - 1 groups.  The rule (bin_ids): s = centroid . direction / |direction|
        in numpy; bin k holds edges[k] <= s < edges[k + 1]; a cell outside [edges[0], edges[-1]) is in no group."""
        ids, n = bin_ids(self.arrays["cell_centroid"], direction, edges)
        return CellGroups(self, ids, n)

    def box_cells(self, lo, hi):
        """The cells whose centroid lies in the box lo <= x < hi (per coordinate, box_ids) -> a CellGroups of one group"""
        return CellGroups(self, box_ids(self.arrays["cell_centroid"], lo, hi), 1)

    def set_nodes(self, mesh_data):
        """orc_mesh_set_nodes: the node geometry (a MeshData, or the tuple its nodes() returns) onto the device, once per mesh: what
        every cut and node_average() need.  A partitioned mesh is refused."""
        vert, fnp, fn = mesh_data.nodes() if hasattr(mesh_data, "nodes") else mesh_data
        vert, fnp, fn = _f64(np.asarray(vert).reshape(-1, 3)), _i64(fnp), _i64(fn)
        check(lib().orc_mesh_set_nodes(self.ptr, C.c_int64(len(vert)), vert.ctypes.data_as(_F64), C.c_int64(len(fnp) - 1), fnp.ctypes.data_as(_I64),
                                       fn.ctypes.data_as(_I64)))
        self.n_vertices = len(vert)

    def node_average(self, x):
        """orc_mesh_node_average: the cell field x (ORC order) at the nodes, inverse-distance weighted over the cells around each node
        (cell values only, also at boundary nodes) -> ndarray[V]"""
        x = _f64(np.asarray(x, dtype=np.float64).reshape(self.n_cells))
        out = np.zeros(self.n_vertices)
        check(lib().orc_mesh_node_average(self.ptr, x.ctypes.data_as(_F64), out.ctypes.data_as(_F64)))
        return out

    def slice(self, origin, normal):
        """orc_cut_plane: the polygons in which the plane through `origin` with `normal` (any length) cuts the cells -> Cut"""
        o, n = _f64(np.asarray(origin, dtype=np.float64).reshape(3)), _f64(np.asarray(normal, dtype=np.float64).reshape(3))
        st = C.c_int(0)
        ptr = lib().orc_cut_plane(self.ptr, o.ctypes.data_as(_F64), n.ctypes.data_as(_F64), C.byref(st))
        return Cut(self, ptr, st.value)

    def cut_nodes(self, values, level=0.0):
        """orc_cut_node_level: the surface values = level of any function given at the nodes [V] -> Cut"""
        v = _f64(np.asarray(values, dtype=np.float64).reshape(-1))
        if len(v) != self.n_vertices:
            raise ValueError("cut_nodes: one value per node (%d), got %d" % (self.n_vertices, len(v)))
        st = C.c_int(0)
        ptr = lib().orc_cut_node_level(self.ptr, v.ctypes.data_as(_F64), C.c_double(level), C.byref(st))
        return Cut(self, ptr, st.value)

    def isosurface(self, cell_values, level):
        """orc_cut_cell_field: node_average() of a cell field (ORC order), then its level -> Cut"""
        x = _f64(np.asarray(cell_values, dtype=np.float64).reshape(-1))
        if len(x) != self.n_cells:
            raise ValueError("isosurface: one value per cell (%d), got %d" % (self.n_cells, len(x)))
        st = C.c_int(0)
        ptr = lib().orc_cut_cell_field(self.ptr, x.ctypes.data_as(_F64), C.c_double(level), C.byref(st))
        return Cut(self, ptr, st.value)

    def bench_cut(self, cell_values, origin, normal, reps=5):
        """orc_bench_cut: HIP-event ms of (node average, classify, scan, emit) for the plane (origin, normal)"""
        x = _f64(np.asarray(cell_values, dtype=np.float64).reshape(self.n_cells))
        o, n = _f64(np.asarray(origin, dtype=np.float64).reshape(3)), _f64(np.asarray(normal, dtype=np.float64).reshape(3))
        ms = np.zeros(4)
        check(lib().orc_bench_cut(self.ptr, x.ctypes.data_as(_F64), o.ctypes.data_as(_F64), n.ctypes.data_as(_F64), C.c_int(reps),
                                  ms.ctypes.data_as(_F64)))
        return tuple(float(t) for t in ms)

    def seed(self, points):
        """orc_tracers_create: tracer particles at the points [n, 3], located as locate() locates them -> Tracers.  Seeds outside the
        mesh are LEFT from the start and never move."""
        return Tracers(self, points)

    def matrix_pattern(self):
        rp = np.empty(self.n_cells + 1, np.int64)
        ci = np.empty(self.nnz, np.int64)
        check(lib().orc_mesh_matrix_pattern(self.ptr, rp.ctypes.data_as(_I64), ci.ctypes.data_as(_I64)))
        return rp, ci

    def csr(self, values):
        import scipy.sparse as sp
        rp, ci = self.matrix_pattern()
        return sp.csr_matrix((values, ci, rp), shape=(self.n_cells, self.n_cells))
