"""io.rs of the reference: read_mesh (io.rs:32-515), read_data / write_data / write_data_with_precision /
write_gradients (io.rs:519-662), carried by liborc_amd.so's host-side C++ (orc_amd/csrc/mesh_io.cpp)."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .mesh import Mesh, MeshArrays

_F64 = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_I32 = C.POINTER(C.c_int32)


def _p(a, t=_F64):
    return a.ctypes.data_as(t)


class MeshData:
    """Host image of mesh::Mesh as read_mesh builds it (OrcMeshData*)."""

    def __init__(self, mesh_path, _handle=None):
        L = lib()
        if _handle is None:
            L.orc_read_mesh.restype = C.c_void_p
            st = C.c_int(0)
            _handle = L.orc_read_mesh(str(mesh_path).encode(), C.byref(st))
            check(st.value)
        self.ptr = C.c_void_p(_handle)
        dims, nv, nc, nf, ncf, nfn, nz = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        check(L.orc_mesh_data_sizes(self.ptr, C.byref(dims), C.byref(nv), C.byref(nc), C.byref(nf), C.byref(ncf), C.byref(nfn), C.byref(nz)))
        self.dimensions, self.n_vertices, self.n_cells, self.n_faces = dims.value, nv.value, nc.value, nf.value
        self.n_cell_faces, self.n_face_nodes, self.n_zones = ncf.value, nfn.value, nz.value

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().orc_mesh_data_destroy(self.ptr)
            self.ptr = None

    @classmethod
    def mixed_channel(cls, nx, ny, nz, lx=0.002, ly=0.001, lz=None, polyhedra=False):
        """orc_mixed_channel_generate: the mesh of mesh.write_mixed_channel_msh(...) built in memory — bit for bit what reading that file gives."""
        L = lib()
        L.orc_mixed_channel_generate.restype = C.c_void_p
        st = C.c_int(0)
        h = L.orc_mixed_channel_generate(C.c_int64(nx), C.c_int64(ny), C.c_int64(nz), C.c_double(lx), C.c_double(ly),
                                         C.c_double(1e-4 * nz if lz is None else lz), C.c_int(1 if polyhedra else 0), C.byref(st))
        check(st.value)
        return cls(None, _handle=h)

    def zones(self):
        """[(zone id, FaceConditionTypes code, scalar_value, vector_value, name)] in file order."""
        out = []
        for k in range(self.n_zones):
            zid, zt, sc = C.c_uint64(), C.c_int32(), C.c_double()
            vec = (C.c_double * 3)()
            name = C.create_string_buffer(256)
            check(lib().orc_mesh_data_zone(self.ptr, C.c_int32(k), C.byref(zid), C.byref(zt), C.byref(sc), vec, name, C.c_int64(256)))
            out.append((zid.value, zt.value, sc.value, tuple(vec), name.value.decode()))
        return out

    def get_face_zone(self, zone_name):
        """Index of the zone called zone_name; the reference panics when there is none (mesh.rs:189-195)."""
        k = lib().orc_mesh_data_zone_index(self.ptr, zone_name.encode())
        if k < 0:
            raise KeyError("face zone '%s' should exist in mesh" % zone_name)
        return k

    def set_zone(self, zone_name, zone_type, scalar_value=0.0, vector_value=(0.0, 0.0, 0.0)):
        vec = (C.c_double * 3)(*vector_value)
        check(lib().orc_mesh_data_set_zone(self.ptr, zone_name.encode(), C.c_int32(int(zone_type)), C.c_double(scalar_value), vec))

    def arrays(self):
        """The argument arrays of orc_mesh_create as a MeshArrays (zone tables included)."""
        F, n = self.n_faces, self.n_cells
        a = MeshArrays(
            face_c0=np.empty(F, np.int64), face_c1=np.empty(F, np.int64), face_zone=np.empty(F, np.int32), face_area=np.empty(F),
            face_normal=np.empty((F, 3)), face_centroid=np.empty((F, 3)), cell_centroid=np.empty((n, 3)), cell_volume=np.empty(n),
            cell_face_ptr=np.empty(n + 1, np.int64), cell_faces=np.empty(self.n_cell_faces, np.int64))
        check(lib().orc_mesh_data_arrays(
            self.ptr, _p(a["face_c0"], _I64), _p(a["face_c1"], _I64), _p(a["face_zone"], _I32), _p(a["face_area"]), _p(a["face_normal"]),
            _p(a["face_centroid"]), _p(a["cell_centroid"]), _p(a["cell_volume"]), _p(a["cell_face_ptr"], _I64), _p(a["cell_faces"], _I64)))
        z = self.zones()
        a["zone_id"] = np.array([t[0] for t in z], np.uint64)
        a["zone_type"] = np.array([t[1] for t in z], np.int32)
        a["zone_scalar"] = np.array([t[2] for t in z], np.float64)
        a["zone_vector"] = np.array([t[3] for t in z], np.float64).reshape(-1, 3)
        a["zone_names"] = [t[4] for t in z]
        return a

    def nodes(self):
        """(vertices[V,3], face_node_ptr[F+1], face_nodes) — Mesh.vertices and Face.node_indices."""
        vert = np.empty((self.n_vertices, 3))
        ptr = np.empty(self.n_faces + 1, np.int64)
        idx = np.empty(self.n_face_nodes, np.int64)
        check(lib().orc_mesh_data_nodes(self.ptr, _p(vert), _p(ptr, _I64), _p(idx, _I64)))
        return vert, ptr, idx

    def upload(self):
        """Device mesh with the current zone table (orc_mesh_upload)."""
        return Mesh(self.arrays())


def read_mesh(mesh_path):
    """io::read_mesh (io.rs:32)."""
    return MeshData(mesh_path)


def write_data(cell_centroid, u, v, w, p, output_file_name, decimal_precision=None):
    """io::write_data (decimal_precision None: "{:.e}") / write_data_with_precision (io.rs:573-620)."""
    cc = np.ascontiguousarray(cell_centroid, np.float64)
    u, v, w, p = (np.ascontiguousarray(x, np.float64) for x in (u, v, w, p))
    check(lib().orc_write_data(str(output_file_name).encode(), C.c_int64(len(u)), _p(cc), _p(u), _p(v), _p(w), _p(p),
                               C.c_int(-1 if decimal_precision is None else int(decimal_precision))))


def read_data(data_file_path):
    """io::read_data (io.rs:519-571) -> (u, v, w, p); OrcError(ORC_ERR_IO) is the reference's Err."""
    n = C.c_int64(0)
    path = str(data_file_path).encode()
    check(lib().orc_read_data(path, C.c_int64(0), None, None, None, None, C.byref(n)))
    u, v, w, p = (np.empty(n.value) for _ in range(4))
    check(lib().orc_read_data(path, C.c_int64(n.value), _p(u), _p(v), _p(w), _p(p), C.byref(n)))
    return u, v, w, p


def write_gradients(mesh, cell_centroid, u, v, w, p, output_file_name, decimal_precision, settings):
    """io::write_gradients (io.rs:623-662); the gradients are computed on the device."""
    cc = np.ascontiguousarray(cell_centroid, np.float64)
    u, v, w, p = (np.ascontiguousarray(x, np.float64) for x in (u, v, w, p))
    check(lib().orc_write_gradients(mesh.ptr, _p(cc), _p(u), _p(v), _p(w), _p(p), str(output_file_name).encode(),
                                    C.c_int(int(decimal_precision)), C.byref(settings)))


# ------------------------------------------------------------------ VTK XML export (orc_write_vtu, orc_write_vtu_faces)
def _vtu_tables(arrays, n_items):
    """{name: ndarray[n] or [n, k]} -> (keep-alive list, n_arrays, names, components, data) of the C tables (SoA by component)"""
    names, comps, cols = [], [], []
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[0] != n_items:
            raise ValueError("array '%s' has shape %s, expected (%d,) or (%d, k)" % (name, a.shape, n_items, n_items))
        names.append(str(name).encode())
        comps.append(a.shape[1])
        cols.append(np.ascontiguousarray(a.T))  # component-major
    k = len(names)
    c_names = (C.c_char_p * max(k, 1))(*names)
    c_comps = np.array(comps if comps else [0], np.int32)
    c_data = (_F64 * max(k, 1))(*[_p(c) for c in cols])
    return (cols, c_comps), k, c_names, _p(c_comps, _I32), c_data


_ENCODINGS = {"ascii": 0, "raw": 1}


def write_vtu(path, mesh_data, cell_arrays, encoding="raw"):
    """orc_write_vtu: the cells of `mesh_data` (a MeshData: nodes and connectivity) with `cell_arrays` {name: ndarray[n] or [n, k]}
    in ORC cell order as a VTK XML UnstructuredGrid; encoding "raw" (appended binary) or "ascii" (both round-trip exactly)."""
    vert, fnp, fn = mesh_data.nodes()
    a = mesh_data.arrays()
    cfp, cf = np.ascontiguousarray(a["cell_face_ptr"], np.int64), np.ascontiguousarray(a["cell_faces"], np.int64)
    keep, k, names, comps, data = _vtu_tables(cell_arrays, mesh_data.n_cells)
    check(lib().orc_write_vtu(str(path).encode(), C.c_int64(len(vert)), _p(vert), C.c_int64(mesh_data.n_cells), _p(cfp, _I64), _p(cf, _I64),
                              _p(fnp, _I64), _p(fn, _I64), C.c_int32(k), names, comps, data, C.c_int32(_ENCODINGS[encoding])))


def write_vtu_boundary(path, mesh_data, boundary_fields, extra_arrays=None, encoding="raw"):
    """orc_write_vtu_faces: the faces of a solver.BoundaryFields as VTK_POLYGON cells carrying its arrays, a per-face "zone" index
    and `extra_arrays` {name: ndarray[nb] or [nb, k]}.  The traction components are also written as one 3-vector "traction"."""
    vert, fnp, fn = mesh_data.nodes()
    faces = np.ascontiguousarray(boundary_fields.faces, np.int64)
    arrays = dict(boundary_fields.arrays)
    if all(("traction_" + c) in arrays for c in "xyz"):
        arrays["traction"] = np.stack([arrays["traction_" + c] for c in "xyz"], axis=1)
    arrays["zone"] = np.repeat(np.arange(len(boundary_fields.zone_ptr) - 1), np.diff(boundary_fields.zone_ptr)).astype(np.float64)
    arrays.update(extra_arrays or {})
    keep, k, names, comps, data = _vtu_tables(arrays, len(faces))
    check(lib().orc_write_vtu_faces(str(path).encode(), C.c_int64(len(vert)), _p(vert), C.c_int64(len(faces)), _p(faces, _I64), _p(fnp, _I64),
                                    _p(fn, _I64), C.c_int32(k), names, comps, data, C.c_int32(_ENCODINGS[encoding])))


def write_vtu_lines(path, lines, point_data=None, encoding="raw"):
    """orc_write_vtu_lines: `lines`, a list of [m_i, 3] arrays (Solver.streamlines), as VTK_POLY_LINE cells (VTK_VERTEX for a single
    point) of a VTK XML UnstructuredGrid; point_data {name: ndarray[sum m_i] or [sum m_i, k]} in the order of the concatenated lines."""
    lines = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in lines]
    ptr = np.concatenate([[0], np.cumsum([len(a) for a in lines])]).astype(np.int64)
    pts = np.ascontiguousarray(np.concatenate(lines)) if lines else np.zeros((0, 3))
    keep, k, names, comps, data = _vtu_tables(point_data or {}, int(ptr[-1]))
    check(lib().orc_write_vtu_lines(str(path).encode(), C.c_int64(len(lines)), _p(ptr, _I64), _p(pts), C.c_int32(k), names, comps, data,
                                    C.c_int32(_ENCODINGS[encoding])))


def write_vtu_cut(path, cut, cell_data=None, point_data=None, encoding="raw", per="vertex"):
    """orc_write_vtu_polygons: the welded surface of a mesh.Cut as VTK_POLYGON cells.  cell_data {name: ndarray[P] or [P, k]} per polygon.
    point_data with per="vertex" (the default): {name: ndarray[NP] or [NP, k]} per polygon vertex (Solver.sample_cut(..., "linear")); a
    point takes the value of its first occurrence, i.e. the first polygon in order wins — LINEAR values of one point are bit-identical
    only within one cell.  per="point": {name: ndarray[M] or [M, k]} per welded point, in the order of cut.welded()."""
    if per not in ("vertex", "point"):
        raise ValueError("write_vtu_cut: per must be 'vertex' or 'point'")
    pts, nodes, first = cut.welded()
    ptr = np.ascontiguousarray(cut.poly_ptr, np.int64)
    pd = {}
    for name, a in (point_data or {}).items():
        a = np.asarray(a, dtype=np.float64)
        if per == "vertex":
            if len(a) != cut.n_points:
                raise ValueError("array '%s': per='vertex' needs one value per polygon vertex (%d), got %d" % (name, cut.n_points, len(a)))
            a = a[first]
        pd[name] = a
    keep_c, kc, names_c, comps_c, data_c = _vtu_tables(cell_data or {}, cut.n_polygons)
    keep_p, kp, names_p, comps_p, data_p = _vtu_tables(pd, len(pts))
    pts = np.ascontiguousarray(pts)
    check(lib().orc_write_vtu_polygons(str(path).encode(), C.c_int64(len(pts)), _p(pts), C.c_int64(cut.n_polygons), _p(ptr, _I64), _p(nodes, _I64),
                                       C.c_int32(kc), names_c, comps_c, data_c, C.c_int32(kp), names_p, comps_p, data_p, C.c_int32(_ENCODINGS[encoding])))
