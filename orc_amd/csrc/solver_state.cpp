// solver_state.cpp — the device image of a mesh (mesh_upload, OrcMesh::dev) and the life of a SolverState: settings check,
// allocation and the two once-only assemblies (solver_init, solver.rs:39-49), the status word, the streams' destruction.
#include <algorithm>

#include "assembly.hpp"

orc::MeshDev OrcMesh::dev() const {
    orc::MeshDev d;
    d.n_cells = n_cells; d.n_own = n_own; d.n_faces = n_faces; d.n_zones = n_zones;
    d.c0 = c0.p; d.c1 = c1.p; d.fzone = fzone.p; d.area = area.p; d.nx = nx.p; d.ny = ny.p; d.nz = nz.p;
    d.fcx = fcx.p; d.fcy = fcy.p; d.fcz = fcz.p; d.ccx = ccx.p; d.ccy = ccy.p; d.ccz = ccz.p; d.vol = vol.p;
    d.cfp = cfp.p; d.cf = cf.p; d.cfpos = cfpos.p; d.ztype = ztype.p; d.zscal = zscal.p; d.zvec = zvec.p;
    return d;
}

namespace orc {

template <class T, class S>
static int upload_as(DevBuf<T> &dst, const S *src, size_t n, size_t stride = 1, size_t off = 0) {
    std::vector<T> tmp(std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; ++i) tmp[i] = (T)src[i * stride + off];
    return dst.upload(tmp.data(), n);
}

int mesh_upload(OrcMesh &m, int64_t n_own, int64_t n_cells, int64_t n_faces, int32_t n_zones, const int64_t *face_c0, const int64_t *face_c1,
                const int32_t *face_zone, const double *face_area, const double *face_normal, const double *face_centroid,
                const double *cell_centroid, const double *cell_volume, const int64_t *cell_face_ptr, const int64_t *cell_faces,
                const int32_t *zone_type, const double *zone_scalar, const double *zone_vector) {
    if (n_cells < 1 || n_faces < 1 || n_zones < 1 || n_own < 1 || n_own > n_cells) return set_error(ORC_ERR_BAD_ARGUMENT, "empty mesh");
    if (n_faces >= ((int64_t)1 << 31) || n_cells >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "mesh too large for 32-bit device indices");
    const int64_t ncf = cell_face_ptr[n_cells];
    if (ncf >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "mesh too large for 32-bit device indices");
    for (int64_t f = 0; f < n_faces; ++f) {
        if (face_c0[f] < 0 || face_c0[f] >= n_cells || face_c1[f] >= n_cells || face_zone[f] < 0 || face_zone[f] >= n_zones)
            return set_error(ORC_ERR_BAD_ARGUMENT, "face %lld: index out of range", (long long)f);
    }
    m.n_cells = n_cells; m.n_own = n_own; m.n_faces = n_faces; m.n_zones = n_zones; m.n_cell_faces = ncf;
    if (m.n_global == 0) m.n_global = n_own;
    // matrix pattern: diagonal + one entry per interior face, ascending columns
    // (CsrMatrix::from(&CooMatrix) at discretization.rs:130,445,471)
    m.h_row_ptr.assign((size_t)n_own + 1, 0);
    std::vector<int64_t> nbr((size_t)ncf);
    for (int64_t c = 0; c < n_own; ++c) {
        int64_t cnt = 1;
        for (int64_t q = cell_face_ptr[c]; q < cell_face_ptr[c + 1]; ++q) {
            const int64_t f = cell_faces[q];
            if (f < 0 || f >= n_faces) return set_error(ORC_ERR_BAD_ARGUMENT, "cell %lld: face index out of range", (long long)c);
            int64_t nb = -1;
            if (face_c1[f] >= 0) nb = face_c0[f] == c ? face_c1[f] : face_c0[f];
            nbr[(size_t)q] = nb;
            if (nb >= 0) cnt++;
        }
        m.h_row_ptr[(size_t)c + 1] = m.h_row_ptr[(size_t)c] + cnt;
    }
    m.h_col.assign((size_t)m.h_row_ptr[(size_t)n_own], 0);
    for (int64_t c = 0; c < n_own; ++c) {
        int64_t *row = m.h_col.data() + m.h_row_ptr[(size_t)c];
        int64_t k = 0;
        row[k++] = c;
        for (int64_t q = cell_face_ptr[c]; q < cell_face_ptr[c + 1]; ++q)
            if (nbr[(size_t)q] >= 0) row[k++] = nbr[(size_t)q];
        std::sort(row, row + k);
        // two cells sharing two faces would give duplicate columns (summed by the reference's
        // COO->CSR); not supported by the fixed-pattern assembly
        for (int64_t t = 1; t < k; ++t)
            if (row[t] == row[t - 1]) return set_error(ORC_ERR_BAD_ARGUMENT, "cells %lld and %lld share more than one face", (long long)c, (long long)row[t]);
    }
    ORC_TRY(sell_from_csr_host(n_own, n_cells, m.h_row_ptr.data(), m.h_col.data(), m.pat));
    // SELL offsets of the neighbour entries
    std::vector<int32_t> cfpos((size_t)ncf, -1);
    {
        std::vector<int64_t> slice_ptr((size_t)m.pat.n_slices + 1);
        ORC_TRY(m.pat.slice_ptr.download(slice_ptr.data(), slice_ptr.size()));
        for (int64_t c = 0; c < n_own; ++c) {
            const int64_t *row = m.h_col.data() + m.h_row_ptr[(size_t)c];
            const int64_t len = m.h_row_ptr[(size_t)c + 1] - m.h_row_ptr[(size_t)c];
            const int64_t base = slice_ptr[(size_t)(c >> 6)] + (c & 63);
            for (int64_t q = cell_face_ptr[c]; q < cell_face_ptr[c + 1]; ++q) {
                if (nbr[(size_t)q] < 0) continue;
                const int64_t k = std::lower_bound(row, row + len, nbr[(size_t)q]) - row;
                cfpos[(size_t)q] = (int32_t)(base + k * 64);
            }
        }
    }
    ORC_TRY(upload_as(m.c0, face_c0, (size_t)n_faces));
    ORC_TRY(upload_as(m.c1, face_c1, (size_t)n_faces));
    ORC_TRY(m.fzone.upload(face_zone, (size_t)n_faces));
    ORC_TRY(m.area.upload(face_area, (size_t)n_faces));
    ORC_TRY(upload_as(m.nx, face_normal, (size_t)n_faces, 3, 0));
    ORC_TRY(upload_as(m.ny, face_normal, (size_t)n_faces, 3, 1));
    ORC_TRY(upload_as(m.nz, face_normal, (size_t)n_faces, 3, 2));
    ORC_TRY(upload_as(m.fcx, face_centroid, (size_t)n_faces, 3, 0));
    ORC_TRY(upload_as(m.fcy, face_centroid, (size_t)n_faces, 3, 1));
    ORC_TRY(upload_as(m.fcz, face_centroid, (size_t)n_faces, 3, 2));
    ORC_TRY(upload_as(m.ccx, cell_centroid, (size_t)n_cells, 3, 0));
    ORC_TRY(upload_as(m.ccy, cell_centroid, (size_t)n_cells, 3, 1));
    ORC_TRY(upload_as(m.ccz, cell_centroid, (size_t)n_cells, 3, 2));
    ORC_TRY(m.vol.upload(cell_volume, (size_t)n_cells));
    ORC_TRY(upload_as(m.cfp, cell_face_ptr, (size_t)n_cells + 1));
    ORC_TRY(upload_as(m.cf, cell_faces, (size_t)ncf));
    ORC_TRY(m.cfpos.upload(cfpos.data(), (size_t)ncf));
    ORC_TRY(m.ztype.upload(zone_type, (size_t)n_zones));
    ORC_TRY(m.zscal.upload(zone_scalar, (size_t)n_zones));
    ORC_TRY(m.zvec.upload(zone_vector, (size_t)3 * n_zones));
    return ORC_OK;
}

static int validate_settings(const OrcSettings &s) {
    if (!(s.momentum == ORC_MOMENTUM_UD || s.momentum == ORC_MOMENTUM_CD1 || is_tvd(s.momentum)))
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "unsupported momentum scheme");  // discretization.rs:287
    if (s.diffusion != ORC_DIFFUSION_CD) return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "unsupported diffusion scheme");  // :50
    if (s.gradient_reconstruction != ORC_GRAD_GREEN_GAUSS_CELL && s.gradient_reconstruction != ORC_GRAD_LEAST_SQUARES)
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "unsupported gradient scheme");  // solver.rs:870,901,948
    if (!(s.pressure_interpolation == ORC_PINTERP_LINEAR || s.pressure_interpolation == ORC_PINTERP_LINEAR_WEIGHTED ||
          s.pressure_interpolation == ORC_PINTERP_SECOND_ORDER))
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "unsupported pressure interpolation");  // solver.rs:1136,1145
    if (!(s.velocity_interpolation == ORC_VINTERP_LINEAR || s.velocity_interpolation == ORC_VINTERP_LINEAR_WEIGHTED ||
          s.velocity_interpolation == ORC_VINTERP_RHIE_CHOW))
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "unsupported velocity interpolation");  // solver.rs:994,1097
    if (s.frozen_diagonals != 0 && s.frozen_diagonals != 1) return set_error(ORC_ERR_BAD_ARGUMENT, "frozen_diagonals must be 0 or 1");
    if (s.reduction_order != ORC_REDUCTION_TREE && s.reduction_order != ORC_REDUCTION_REFERENCE)
        return set_error(ORC_ERR_BAD_ARGUMENT, "unknown reduction order %d", s.reduction_order);
    return ORC_OK;
}

int fetch_status(SolverState &s) {
    int h = 0;
    ORC_HIP(hipMemcpyAsync(&h, s.dev_status.p, sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    return h;
}

int solver_init(SolverState &s, OrcMesh *m, const OrcSettings *settings, double rho, double mu) {
    ORC_TRY(ensure_init());
    s.mesh = m;
    s.settings = *settings;
    s.rho = rho; s.mu = mu; s.n = m->n_cells; s.n_own = m->n_own;
    // the schedule of THIS solver: fixed at its creation (config.hpp; a solver never changes schedule between iterations)
    s.concurrent_momentum = cfg().concurrent_momentum;
    s.two_stream_multigrid = cfg().two_stream_multigrid;
    s.triple_momentum = cfg().triple_momentum;
    s.early_p_hierarchy = cfg().early_p_hierarchy;
    s.sibling_pairing = cfg().amg_sibling;
    ORC_TRY(validate_settings(s.settings));
    const size_t n = (size_t)s.n, pad = (size_t)std::max<int64_t>(m->pat.padded, 1), F = (size_t)m->n_faces;
    DevBuf<double> *nvec[] = {&s.u, &s.v, &s.w, &s.p, &s.p_prime, &s.b_u_di, &s.b_v_di, &s.b_w_di, &s.b_u, &s.b_v, &s.b_w, &s.b_p, &s.du, &s.dv, &s.dw};
    for (auto *b : nvec) { ORC_TRY(b->alloc(n)); ORC_TRY(b->zero()); }
    DevBuf<double> *mats[] = {&s.a_di, &s.a_u, &s.a_v, &s.a_w, &s.a_p};
    for (auto *b : mats) { ORC_TRY(b->alloc(pad)); ORC_TRY(b->zero()); }
    ORC_TRY(s.gp.alloc(3 * n));
    ORC_TRY(s.gu.alloc(9 * n));
    ORC_TRY(s.flux.alloc(F));
    ORC_TRY(s.pf.alloc(F));
    ORC_TRY(s.coef.alloc(F));
    if (s.settings.frozen_diagonals == 0) {
        // the order dependence is defined on ONE process's cell order; a partitioned mesh has no such order across ranks
        if (m->halo.active()) return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "frozen_diagonals = 0 (in-place diagonals) is not available on a partitioned mesh");
        ORC_TRY(s.du_old.alloc(n));
        ORC_TRY(s.dv_old.alloc(n));
        ORC_TRY(s.dw_old.alloc(n));
        ORC_TRY(s.pe.alloc(3 * n));
        // level(c) = 1 + max level(j), j < c a neighbour of c (the matrix pattern is the face-neighbour graph + the diagonal)
        std::vector<int32_t> level((size_t)s.n_own, 0);
        int32_t n_levels = 0;
        for (int64_t c = 0; c < s.n_own; ++c) {
            int32_t lv = 0;
            for (int64_t q = m->h_row_ptr[(size_t)c]; q < m->h_row_ptr[(size_t)c + 1]; ++q) {
                const int64_t j = m->h_col[(size_t)q];
                if (j < c) lv = std::max(lv, level[(size_t)j] + 1);
            }
            level[(size_t)c] = lv;
            n_levels = std::max(n_levels, lv + 1);
        }
        s.level_ptr.assign((size_t)n_levels + 1, 0);
        for (int64_t c = 0; c < s.n_own; ++c) ++s.level_ptr[(size_t)level[(size_t)c] + 1];
        for (int32_t l = 0; l < n_levels; ++l) s.level_ptr[(size_t)l + 1] += s.level_ptr[(size_t)l];
        std::vector<int32_t> cells((size_t)std::max<int64_t>(s.n_own, 1));
        std::vector<int64_t> cur(s.level_ptr.begin(), s.level_ptr.end() - 1);
        for (int64_t c = 0; c < s.n_own; ++c) cells[(size_t)cur[(size_t)level[(size_t)c]]++] = (int32_t)c;
        ORC_TRY(s.level_cells.upload(cells.data(), cells.size()));
    } else if (s.settings.reduction_order == ORC_REDUCTION_REFERENCE && !m->halo.active()) {
        ORC_TRY(s.pe.alloc(n));  // [r05] per-cell terms of the report's sums in the reference's association (k_momentum, k_apply_correction)
    }
    ORC_TRY(s.partials.alloc((size_t)8 * kMaxPartials));
    ORC_TRY(s.scal.alloc(16));
    ORC_TRY(s.dev_status.alloc(1));
    ORC_TRY(s.dev_status.zero());
    ORC_TRY(k_diffusion(s));       // solver.rs:41-42
    ORC_TRY(k_init_momentum(s));   // solver.rs:43-45
    int st = fetch_status(s);
    if (st) return set_error(st, "unsupported boundary condition in mesh zones");
    return ORC_OK;
}

static void destroy_side(SolveSide &d) {
    if (d.stream) stream_destroy(d.stream);
    if (d.ev_setup) (void)hipEventDestroy(d.ev_setup);
    if (d.ev_solve) (void)hipEventDestroy(d.ev_solve);
    d = SolveSide();
}

SolverState::~SolverState() {
    for (auto &l : lanes) {
        if (l.stream) stream_destroy(l.stream);
        if (l.level0_done) (void)hipEventDestroy(l.level0_done);
        destroy_side(l.side);
    }
    destroy_side(side);
    if (prep_stream) stream_destroy(prep_stream);
}

}  // namespace orc
