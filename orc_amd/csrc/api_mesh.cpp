// api_mesh.cpp — C ABI for mesh::Mesh: the device mesh of one GPU, of one rank of a partitioned run, and the internally reordered one.
#include <algorithm>

#include "cell_order.hpp"

using namespace orc;

namespace {

// the send / receive blocks of one rank (orc_mesh_create_partitioned's arguments) into the mesh's halo plan
int build_halo_plan(HaloPlan &H, int64_t n_owned, int64_t n_cells, int32_t n_peers, const int32_t *peers, const int64_t *send_ptr,
                    const int64_t *send_idx, const int64_t *recv_ptr) {
    int st = ORC_OK;
    H.n_own = n_owned;
    H.n_ghost = n_cells - n_owned;
    H.n_send = send_ptr[n_peers];
    if (recv_ptr[n_peers] != H.n_ghost) st = set_error(ORC_ERR_BAD_ARGUMENT, "ghost blocks (%lld) do not cover the ghost cells (%lld)",
                                                        (long long)recv_ptr[n_peers], (long long)H.n_ghost);
    std::vector<int32_t> idx((size_t)H.n_send);
    for (int64_t i = 0; i < H.n_send && st == ORC_OK; ++i) {
        if (send_idx[i] < 0 || send_idx[i] >= n_owned) st = set_error(ORC_ERR_BAD_ARGUMENT, "send index out of the owned range");
        idx[(size_t)i] = (int32_t)send_idx[i];
    }
    for (int q = 0; q < n_peers; ++q) {
        H.peers.push_back(peers[q]);
        H.send_off.push_back(send_ptr[q]); H.send_cnt.push_back(send_ptr[q + 1] - send_ptr[q]);
        H.recv_off.push_back(recv_ptr[q]); H.recv_cnt.push_back(recv_ptr[q + 1] - recv_ptr[q]);
    }
    if (st == ORC_OK) st = H.send_idx.upload(idx.data(), idx.size());
    return st;
}

// H.interior_lo / _hi: the longest run of 64-row slices whose rows have no ghost neighbour
void find_interior_slices(HaloPlan &H, int64_t n_owned, int64_t n_faces, const int64_t *face_c0, const int64_t *face_c1) {
    const int64_t n_slices = (n_owned + 63) / 64;
    std::vector<unsigned char> touches((size_t)n_slices, 0);
    for (int64_t f = 0; f < n_faces; ++f) {
        const int64_t a = face_c0[f], b = face_c1[f];
        if (b < 0) continue;
        if (a < n_owned && b >= n_owned) touches[(size_t)(a >> 6)] = 1;
        if (b < n_owned && a >= n_owned) touches[(size_t)(b >> 6)] = 1;
    }
    int64_t best_lo = 0, best_len = 0, run_lo = 0;
    for (int64_t sl = 0; sl <= n_slices; ++sl) {
        if (sl == n_slices || touches[(size_t)sl]) {
            if (sl - run_lo > best_len) { best_len = sl - run_lo; best_lo = run_lo; }
            run_lo = sl + 1;
        }
    }
    H.interior_lo = (int32_t)best_lo;
    H.interior_hi = (int32_t)(best_lo + best_len);
}

}  // namespace

extern "C" {

OrcMesh *orc_mesh_create(int64_t n_cells, int64_t n_faces, int32_t n_zones, const int64_t *face_c0, const int64_t *face_c1,
                         const int32_t *face_zone, const double *face_area, const double *face_normal, const double *face_centroid,
                         const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr,
                         const int64_t *cell_faces, const int32_t *zone_type, const double *zone_scalar, const double *zone_vector,
                         int *status) {
    int st = ensure_init();
    OrcMesh *m = nullptr;
    if (st == ORC_OK) {
        m = new OrcMesh();
        st = mesh_upload(*m, n_cells, n_cells, n_faces, n_zones, face_c0, face_c1, face_zone, face_area, face_normal, face_centroid,
                         cell_centroid, cell_volume, cell_face_ptr, cell_faces, zone_type, zone_scalar, zone_vector);
        if (st != ORC_OK) { delete m; m = nullptr; }
    }
    if (status) *status = st;
    return m;
}

OrcMesh *orc_mesh_create_partitioned(int64_t n_owned, int64_t n_cells, int64_t n_cells_global, int64_t n_faces, int32_t n_zones,
                                     const int64_t *face_c0, const int64_t *face_c1, const int32_t *face_zone, const double *face_area,
                                     const double *face_normal, const double *face_centroid, const double *cell_centroid,
                                     const double *cell_volume, const int64_t *cell_face_ptr, const int64_t *cell_faces,
                                     const int32_t *zone_type, const double *zone_scalar, const double *zone_vector, int32_t n_peers,
                                     const int32_t *peers, const int64_t *send_ptr, const int64_t *send_idx, const int64_t *recv_ptr,
                                     int *status) {
    int st = ensure_init();
    OrcMesh *m = nullptr;
    if (st == ORC_OK) {
        m = new OrcMesh();
        m->n_global = n_cells_global;
        st = mesh_upload(*m, n_owned, n_cells, n_faces, n_zones, face_c0, face_c1, face_zone, face_area, face_normal, face_centroid,
                         cell_centroid, cell_volume, cell_face_ptr, cell_faces, zone_type, zone_scalar, zone_vector);
        if (st == ORC_OK && n_peers > 0) {
            st = build_halo_plan(m->halo, n_owned, n_cells, n_peers, peers, send_ptr, send_idx, recv_ptr);
            if (st == ORC_OK) find_interior_slices(m->halo, n_owned, n_faces, face_c0, face_c1);
        }
        if (st != ORC_OK) { delete m; m = nullptr; }
    }
    if (status) *status = st;
    return m;
}

// The whole mesh renumbered by `ordering` (orc_mesh_partition with one rank): rows sorted by RCM for coalesced reads when
// the generator's numbering is arbitrary.  Fields still go in and out in ORC order (cell_order.hpp).
OrcMesh *orc_mesh_create_reordered(int64_t n_cells, int64_t n_faces, int32_t n_zones, const int64_t *face_c0, const int64_t *face_c1,
                                   const int32_t *face_zone, const double *face_area, const double *face_normal, const double *face_centroid,
                                   const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr,
                                   const int64_t *cell_faces, const int32_t *zone_type, const double *zone_scalar, const double *zone_vector,
                                   int32_t ordering, int *status) {
    int st = ORC_OK;
    OrcPartition *P = orc_mesh_partition(n_cells, n_faces, face_c0, face_c1, face_zone, face_area, face_normal, face_centroid, cell_centroid,
                                         cell_volume, cell_face_ptr, cell_faces, 1, 0, ordering, &st);
    OrcMesh *m = nullptr;
    if (P) {
        m = orc_partition_upload(P, n_zones, zone_type, zone_scalar, zone_vector, &st);
        if (m) {
            m->h_global_ids.resize((size_t)n_cells);
            st = orc_partition_arrays(P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, m->h_global_ids.data(),
                                      nullptr, nullptr, nullptr, nullptr, nullptr);
            bool identity = true;
            for (int64_t c = 0; c < n_cells && identity; ++c) identity = m->h_global_ids[(size_t)c] == c;
            if (identity) m->h_global_ids.clear();
        }
        orc_partition_destroy(P);
    }
    if (status) *status = st;
    return m;
}

int orc_mesh_cell_order(const OrcMesh *m, int64_t *global_ids) {
    if (!m || !global_ids) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    const std::vector<int64_t> &g = cell_order_ids(*m);
    for (int64_t c = 0; c < m->n_cells; ++c) global_ids[c] = g.empty() ? c : g[(size_t)c];
    return ORC_OK;
}

int orc_mesh_update_zones(OrcMesh *m, const int32_t *zone_type, const double *zone_scalar, const double *zone_vector) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "null mesh");
    if (zone_type) wall_zones_changed(*m, zone_type);  // the cached wall distance goes when the wall-ness of a zone changes
    ORC_TRY(m->ztype.upload(zone_type, (size_t)m->n_zones));
    ORC_TRY(m->zscal.upload(zone_scalar, (size_t)m->n_zones));
    ORC_TRY(m->zvec.upload(zone_vector, (size_t)3 * m->n_zones));
    return ORC_OK;
}

void orc_mesh_destroy(OrcMesh *m) {
    if (m) orc::gs_forget_pattern((const void *)m->pat.col.p);
    delete m;
}
int64_t orc_mesh_n_cells(const OrcMesh *m) { return m ? m->n_cells : 0; }
int64_t orc_mesh_n_owned(const OrcMesh *m) { return m ? m->n_own : 0; }
int64_t orc_mesh_nnz(const OrcMesh *m) { return m ? m->pat.nnz : 0; }

int orc_mesh_matrix_pattern(const OrcMesh *m, int64_t *row_ptr, int64_t *col_idx) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "null mesh");
    std::copy(m->h_row_ptr.begin(), m->h_row_ptr.end(), row_ptr);
    std::copy(m->h_col.begin(), m->h_col.end(), col_idx);
    return ORC_OK;
}

}  // extern "C"
