// vtk_io.cpp — VTK XML UnstructuredGrid (.vtu) export of cell arrays and boundary-face arrays (new-build extension; the reference
// writes its own text format only, io.rs:573-662).  Host code, no device work.  Version 1.0, header_type UInt64, little endian;
// ASCII (%.17g: a double round-trips exactly) or appended raw data ('_', then per array a UInt64 byte count and the bytes).
// A cell of four triangles is a VTK_TETRA, one of six quadrilaterals over eight nodes a VTK_HEXAHEDRON, both in VTK's node order
// with positive orientation; every other cell is a VTK_POLYHEDRON with its face stream.  Only the points a file uses are written.
// The arrays carry no face count, so a face id can only be checked against 0: cell_faces / face_ids must index face_node_ptr.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "orc_amd.h"

namespace {

using orc::set_error;

constexpr uint8_t kVtkVertex = 1, kVtkPolyLine = 4, kVtkPolygon = 7, kVtkTetra = 10, kVtkHexahedron = 12, kVtkPolyhedron = 42;

struct P3 {
    double x, y, z;
};
inline P3 sub(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline P3 cross(P3 a, P3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// what the two writers share: the arrays of one <Piece>, in the caller's point numbering until finish() renumbers them
struct Piece {
    std::vector<int64_t> connectivity, offsets, faces, faceoffsets;
    std::vector<uint8_t> types;
    bool any_polyhedron = false;
};

struct Arrays {
    int32_t n = 0;
    const char *const *names = nullptr;
    const int32_t *components = nullptr;
    const double *const *data = nullptr;
};

int check_arrays(const Arrays &A, int32_t encoding) {
    if (encoding != 0 && encoding != 1) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: encoding must be 0 (ascii) or 1 (appended raw)");
    if (A.n < 0) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: negative array count");
    if (A.n > 0 && (!A.names || !A.components || !A.data)) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: null array table");
    for (int32_t a = 0; a < A.n; ++a) {
        if (!A.names[a] || !A.names[a][0] || !A.data[a]) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: array %d has no name or no data", a);
        if (strpbrk(A.names[a], "\"<>&")) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: array name %d holds a character XML reserves", a);
        if (A.components[a] < 1) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: array %d has %d components", a, A.components[a]);
    }
    return ORC_OK;
}

// nodes of face f, checked: [begin, end) into face_nodes, every id in [0, n_points)
int face_span(int64_t f, int64_t n_points, const int64_t *fnp, const int64_t *fn, int64_t &b, int64_t &e) {
    if (f < 0) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: negative face id");
    b = fnp[f]; e = fnp[f + 1];
    if (b < 0 || e < b || e - b < 3) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: face %lld has an inconsistent node range", (long long)f);
    for (int64_t i = b; i < e; ++i)
        if (fn[i] < 0 || fn[i] >= n_points) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: face %lld names node %lld of %lld", (long long)f, (long long)fn[i], (long long)n_points);
    return ORC_OK;
}

inline P3 point(const double *pts, int64_t i) { return {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}; }

// four triangles over four nodes -> VTK's order: the first face, wound so that its right-hand normal points to the apex
bool as_tetra(const double *pts, const int64_t *fn, const int64_t *b /*[4] face begins*/, int64_t out[4]) {
    int64_t a0 = fn[b[0]], a1 = fn[b[0] + 1], a2 = fn[b[0] + 2], apex = -1;
    if (a0 == a1 || a0 == a2 || a1 == a2) return false;
    for (int k = 1; k < 4; ++k)
        for (int i = 0; i < 3; ++i) {
            const int64_t v = fn[b[k] + i];
            if (v == a0 || v == a1 || v == a2) continue;
            if (apex >= 0 && v != apex) return false;
            apex = v;
        }
    if (apex < 0) return false;
    const double vol6 = dot(cross(sub(point(pts, a1), point(pts, a0)), sub(point(pts, a2), point(pts, a0))), sub(point(pts, apex), point(pts, a0)));
    if (vol6 < 0.) std::swap(a1, a2);
    out[0] = a0; out[1] = a1; out[2] = a2; out[3] = apex;
    return true;
}

// six quadrilaterals over eight nodes -> VTK's order: the first face as nodes 0-3, above each of them the node its side edge
// leads to as 4-7, the bottom wound so that its right-hand normal points to the top
bool as_hexahedron(const double *pts, const int64_t *fn, const int64_t *b /*[6]*/, int64_t out[8]) {
    int64_t q[4], t[4] = {-1, -1, -1, -1};
    for (int i = 0; i < 4; ++i) q[i] = fn[b[0] + i];
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (q[i] == q[j]) return false;
    auto bottom = [&](int64_t v) { for (int i = 0; i < 4; ++i) if (q[i] == v) return i; return -1; };
    int opposite = 0;
    for (int k = 1; k < 6; ++k) {
        int on_bottom = 0;
        for (int i = 0; i < 4; ++i) {
            const int64_t x = fn[b[k] + i], y = fn[b[k] + (i + 1) % 4];
            const int ix = bottom(x), iy = bottom(y);
            if (ix >= 0) ++on_bottom;
            if (ix >= 0 && iy < 0) { if (t[ix] >= 0 && t[ix] != y) return false; t[ix] = y; }
            if (iy >= 0 && ix < 0) { if (t[iy] >= 0 && t[iy] != x) return false; t[iy] = x; }
        }
        if (on_bottom == 0) ++opposite;
        else if (on_bottom != 2) return false;
    }
    if (opposite != 1) return false;
    for (int i = 0; i < 4; ++i) {
        if (t[i] < 0) return false;
        for (int j = 0; j < i; ++j)
            if (t[i] == t[j]) return false;
    }
    P3 nrm = {0., 0., 0.}, up = {0., 0., 0.};  // Newell normal of the bottom, mean of the four side edges
    for (int i = 0; i < 4; ++i) {
        const P3 c = cross(point(pts, q[i]), point(pts, q[(i + 1) % 4]));
        nrm = {nrm.x + c.x, nrm.y + c.y, nrm.z + c.z};
        const P3 e = sub(point(pts, t[i]), point(pts, q[i]));
        up = {up.x + e.x, up.y + e.y, up.z + e.z};
    }
    const bool flip = dot(nrm, up) < 0.;
    for (int i = 0; i < 4; ++i) {
        const int s = flip ? (4 - i) % 4 : i;
        out[i] = q[s]; out[4 + i] = t[s];
    }
    return true;
}

struct Writer {
    FILE *f = nullptr;
    bool raw = false;
    uint64_t offset = 0;                       // of the next appended block
    std::vector<std::vector<char>> appended;   // raw mode: the blocks in header order
    ~Writer() { if (f) fclose(f); }
    template <class T>
    void array(const char *type, const char *name, int comps, const std::vector<T> &v, const char *fmt) {
        fprintf(f, "        <DataArray type=\"%s\" Name=\"%s\"", type, name);
        if (comps > 0) fprintf(f, " NumberOfComponents=\"%d\"", comps);
        if (raw) {
            fprintf(f, " format=\"appended\" offset=\"%llu\"/>\n", (unsigned long long)offset);
            std::vector<char> blk(v.size() * sizeof(T));
            if (!blk.empty()) memcpy(blk.data(), v.data(), blk.size());
            offset += sizeof(uint64_t) + blk.size();
            appended.push_back(std::move(blk));
            return;
        }
        fprintf(f, " format=\"ascii\">\n");
        const size_t per = comps > 0 ? (size_t)comps : 8;
        for (size_t i = 0; i < v.size(); ++i) {
            if (sizeof(T) == 1) fprintf(f, "%u", (unsigned)v[i]);
            else fprintf(f, fmt, v[i]);
            fputc((i + 1) % per == 0 || i + 1 == v.size() ? '\n' : ' ', f);
        }
        fprintf(f, "        </DataArray>\n");
    }
};

// one <CellData> or <PointData> section: structure-of-arrays by component -> VTK's tuples
void data_section(Writer &W, const char *tag, const Arrays &A, int64_t n_items) {
    fprintf(W.f, "      <%s>\n", tag);
    std::vector<double> tuples;
    for (int32_t a = 0; a < A.n; ++a) {
        const int32_t k = A.components[a];
        tuples.resize((size_t)k * (size_t)n_items);
        for (int32_t q = 0; q < k; ++q)
            for (int64_t c = 0; c < n_items; ++c) tuples[(size_t)c * k + q] = A.data[a][(size_t)q * n_items + c];
        W.array("Float64", A.names[a], k, tuples, "%.17g");
    }
    fprintf(W.f, "      </%s>\n", tag);
}

// renumber the used points ascending, then write the file; C: cell data of the n_items cells (null: no section), Pt: point data of the
// n_points points, every one of which the piece must use (null: no section)
int finish(const char *path, int64_t n_points, const double *points, Piece &P, const Arrays *C, const Arrays *Pt, int64_t n_items, int32_t encoding) {
    std::vector<int64_t> new_id((size_t)n_points, -1);
    for (int64_t v : P.connectivity) new_id[(size_t)v] = 0;
    if (P.any_polyhedron)
        for (size_t i = 0; i < P.faces.size();) {  // the stream: faces, then per face its node count and nodes
            const int64_t nf = P.faces[i++];
            for (int64_t k = 0; k < nf; ++k) {
                const int64_t np = P.faces[i++];
                for (int64_t j = 0; j < np; ++j) new_id[(size_t)P.faces[i++]] = 0;
            }
        }
    std::vector<double> xyz;
    int64_t used = 0;
    for (int64_t v = 0; v < n_points; ++v)
        if (new_id[(size_t)v] == 0) {
            new_id[(size_t)v] = used++;
            xyz.push_back(points[3 * v]); xyz.push_back(points[3 * v + 1]); xyz.push_back(points[3 * v + 2]);
        }
    for (int64_t &v : P.connectivity) v = new_id[(size_t)v];
    if (P.any_polyhedron)
        for (size_t i = 0; i < P.faces.size();) {
            const int64_t nf = P.faces[i++];
            for (int64_t k = 0; k < nf; ++k) {
                const int64_t np = P.faces[i++];
                for (int64_t j = 0; j < np; ++j, ++i) P.faces[i] = new_id[(size_t)P.faces[i]];
            }
        }

    Writer W;
    W.raw = encoding == 1;
    W.f = fopen(path, "wb");
    if (!W.f) return set_error(ORC_ERR_IO, "write_vtu: cannot open '%s' for writing", path);
    FILE *f = W.f;
    fprintf(f, "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" header_type=\"UInt64\">\n");
    fprintf(f, "  <UnstructuredGrid>\n    <Piece NumberOfPoints=\"%lld\" NumberOfCells=\"%lld\">\n", (long long)used, (long long)n_items);  // n_items: still the cells
    fprintf(f, "      <Points>\n");
    W.array("Float64", "Points", 3, xyz, "%.17g");
    fprintf(f, "      </Points>\n      <Cells>\n");
    W.array("Int64", "connectivity", 0, P.connectivity, "%lld");
    W.array("Int64", "offsets", 0, P.offsets, "%lld");
    W.array("UInt8", "types", 0, P.types, "%u");
    if (P.any_polyhedron) {
        W.array("Int64", "faces", 0, P.faces, "%lld");
        W.array("Int64", "faceoffsets", 0, P.faceoffsets, "%lld");
    }
    fprintf(f, "      </Cells>\n");
    if (Pt) data_section(W, "PointData", *Pt, used);
    if (C) data_section(W, "CellData", *C, n_items);
    fprintf(f, "    </Piece>\n  </UnstructuredGrid>\n");
    if (W.raw) {
        fprintf(f, "  <AppendedData encoding=\"raw\">\n_");
        for (const std::vector<char> &blk : W.appended) {
            const uint64_t bytes = blk.size();
            fwrite(&bytes, sizeof bytes, 1, f);
            if (bytes) fwrite(blk.data(), 1, blk.size(), f);
        }
        fprintf(f, "\n  </AppendedData>\n");
    }
    fprintf(f, "</VTKFile>\n");
    const bool bad = ferror(f) != 0;
    const bool close_bad = fclose(f) != 0;
    W.f = nullptr;
    if (bad || close_bad) return set_error(ORC_ERR_IO, "write_vtu: writing '%s' failed", path);
    return ORC_OK;
}

}  // namespace

extern "C" {

int orc_write_vtu(const char *path, int64_t n_points, const double *points, int64_t n_cells, const int64_t *cell_face_ptr,
                  const int64_t *cell_faces, const int64_t *face_node_ptr, const int64_t *face_nodes, int32_t n_arrays,
                  const char *const *names, const int32_t *components, const double *const *data, int32_t encoding) {
    if (!path || n_points < 0 || n_cells < 0 || !cell_face_ptr || (n_points > 0 && !points))
        return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: null or negative argument");
    if (n_cells > 0 && (!cell_faces || !face_node_ptr || !face_nodes)) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: null connectivity");
    Arrays A{n_arrays, names, components, data};
    ORC_TRY(check_arrays(A, encoding));
    if (cell_face_ptr[0] < 0) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: cell_face_ptr starts below 0");
    Piece P;
    std::vector<int64_t> begin, nodes;
    for (int64_t c = 0; c < n_cells; ++c) {
        const int64_t lo = cell_face_ptr[c], hi = cell_face_ptr[c + 1];
        if (hi < lo) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: cell_face_ptr decreases at cell %lld", (long long)c);
        if (hi - lo < 4) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu: cell %lld has fewer than four faces", (long long)c);
        begin.clear(); nodes.clear();
        bool all3 = true, all4 = true;
        for (int64_t q = lo; q < hi; ++q) {
            int64_t b, e;
            ORC_TRY(face_span(cell_faces[q], n_points, face_node_ptr, face_nodes, b, e));
            begin.push_back(b);
            all3 = all3 && e - b == 3; all4 = all4 && e - b == 4;
            nodes.insert(nodes.end(), face_nodes + b, face_nodes + e);
        }
        std::sort(nodes.begin(), nodes.end());
        nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
        int64_t fixed[8];
        if (hi - lo == 4 && all3 && nodes.size() == 4 && as_tetra(points, face_nodes, begin.data(), fixed)) {
            P.connectivity.insert(P.connectivity.end(), fixed, fixed + 4);
            P.types.push_back(kVtkTetra);
            P.faceoffsets.push_back(-1);
        } else if (hi - lo == 6 && all4 && nodes.size() == 8 && as_hexahedron(points, face_nodes, begin.data(), fixed)) {
            P.connectivity.insert(P.connectivity.end(), fixed, fixed + 8);
            P.types.push_back(kVtkHexahedron);
            P.faceoffsets.push_back(-1);
        } else {
            P.connectivity.insert(P.connectivity.end(), nodes.begin(), nodes.end());
            P.types.push_back(kVtkPolyhedron);
            P.any_polyhedron = true;
            P.faces.push_back(hi - lo);
            for (int64_t q = lo; q < hi; ++q) {
                const int64_t f = cell_faces[q], b = face_node_ptr[f], e = face_node_ptr[f + 1];
                P.faces.push_back(e - b);
                P.faces.insert(P.faces.end(), face_nodes + b, face_nodes + e);
            }
            P.faceoffsets.push_back((int64_t)P.faces.size());
        }
        P.offsets.push_back((int64_t)P.connectivity.size());
    }
    return finish(path, n_points, points, P, &A, nullptr, n_cells, encoding);
}

int orc_write_vtu_faces(const char *path, int64_t n_points, const double *points, int64_t n_faces, const int64_t *face_ids,
                        const int64_t *face_node_ptr, const int64_t *face_nodes, int32_t n_arrays, const char *const *names,
                        const int32_t *components, const double *const *data, int32_t encoding) {
    if (!path || n_points < 0 || n_faces < 0 || (n_points > 0 && !points)) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_faces: null or negative argument");
    if (n_faces > 0 && (!face_ids || !face_node_ptr || !face_nodes)) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_faces: null connectivity");
    Arrays A{n_arrays, names, components, data};
    ORC_TRY(check_arrays(A, encoding));
    Piece P;
    for (int64_t i = 0; i < n_faces; ++i) {
        int64_t b, e;
        ORC_TRY(face_span(face_ids[i], n_points, face_node_ptr, face_nodes, b, e));
        P.connectivity.insert(P.connectivity.end(), face_nodes + b, face_nodes + e);
        P.offsets.push_back((int64_t)P.connectivity.size());
        P.types.push_back(kVtkPolygon);
    }
    return finish(path, n_points, points, P, &A, nullptr, n_faces, encoding);
}

int orc_write_vtu_lines(const char *path, int64_t n_lines, const int64_t *line_ptr, const double *points, int32_t n_arrays, const char *const *names,
                        const int32_t *components, const double *const *data, int32_t encoding) {
    if (!path || n_lines < 0 || !line_ptr) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_lines: null or negative argument");
    Arrays A{n_arrays, names, components, data};
    ORC_TRY(check_arrays(A, encoding));
    if (line_ptr[0] != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_lines: line_ptr must start at 0");
    for (int64_t i = 0; i < n_lines; ++i)
        if (line_ptr[i + 1] <= line_ptr[i]) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_lines: line %lld has no point (line_ptr must increase)", (long long)i);
    const int64_t n_points = line_ptr[n_lines];
    if (n_points > 0 && !points) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_lines: null points");
    Piece P;
    for (int64_t i = 0; i < n_lines; ++i) {
        for (int64_t v = line_ptr[i]; v < line_ptr[i + 1]; ++v) P.connectivity.push_back(v);
        P.offsets.push_back(line_ptr[i + 1]);
        P.types.push_back(line_ptr[i + 1] - line_ptr[i] == 1 ? kVtkVertex : kVtkPolyLine);
    }
    return finish(path, n_points, points, P, nullptr, &A, n_lines, encoding);
}

int orc_write_vtu_polygons(const char *path, int64_t n_points, const double *points, int64_t n_polys, const int64_t *poly_ptr, const int64_t *poly_nodes,
                           int32_t n_cell_arrays, const char *const *cell_names, const int32_t *cell_components, const double *const *cell_data,
                           int32_t n_point_arrays, const char *const *point_names, const int32_t *point_components, const double *const *point_data,
                           int32_t encoding) {
    if (!path || n_points < 0 || n_polys < 0 || !poly_ptr || (n_points > 0 && !points)) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: null or negative argument");
    Arrays C{n_cell_arrays, cell_names, cell_components, cell_data}, Pt{n_point_arrays, point_names, point_components, point_data};
    ORC_TRY(check_arrays(C, encoding));
    ORC_TRY(check_arrays(Pt, encoding));
    if (poly_ptr[0] != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: poly_ptr must start at 0");
    for (int64_t i = 0; i < n_polys; ++i)
        if (poly_ptr[i + 1] - poly_ptr[i] < 3) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: polygon %lld has fewer than 3 nodes", (long long)i);
    if (n_polys > 0 && !poly_nodes) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: null connectivity");
    std::vector<char> used((size_t)n_points, 0);
    Piece P;
    for (int64_t i = 0; i < n_polys; ++i) {
        for (int64_t q = poly_ptr[i]; q < poly_ptr[i + 1]; ++q) {
            const int64_t v = poly_nodes[q];
            if (v < 0 || v >= n_points) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: polygon %lld names point %lld of %lld", (long long)i, (long long)v, (long long)n_points);
            used[(size_t)v] = 1;
            P.connectivity.push_back(v);
        }
        P.offsets.push_back(poly_ptr[i + 1]);
        P.types.push_back(kVtkPolygon);
    }
    for (int64_t v = 0; v < n_points; ++v)  // point data is written per point of the file: none may drop out
        if (!used[(size_t)v]) return set_error(ORC_ERR_BAD_ARGUMENT, "write_vtu_polygons: point %lld belongs to no polygon", (long long)v);
    return finish(path, n_points, points, P, &C, &Pt, n_polys, encoding);
}

}  // extern "C"
