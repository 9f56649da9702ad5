// derived.hip — derived flow fields and boundary-face maps (new-build extension; ORC writes u, v, w, p and nothing else): what a
// viewer needs next to the solution, formed where the fields live.  DESIGN.md §3 "Derived fields and boundary maps" has the
// definitions and the operator order; orc_types.h OrcDerivedField / OrcBoundaryField name the fields.
//
//   derived_cell_k   one thread per owned cell, scalar_k's XCD-contiguous block walk: the velocity gradient of the settings'
//                    reconstruction by the assembly's own per-cell body (gradient_cell.hpp: the bits of grad_u_k / grad_u_lsq_k), kept
//                    in registers, and |U_f . n| A summed in the same face loop; then the selected fields, structure-of-arrays
//   boundary_map_k   grid-stride over the boundary index of surface.hip, one thread per face, the zone type decided per face:
//                    the surface report's terms per face instead of per zone, no reduction
// Read-only and opt-in: neither kernel is launched unless an entry of this file is called.  No atomics but the status word.
#include <cmath>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"


namespace orc {

namespace {

struct DerivedArgs {
    const double *u, *v, *w;
    double *out;      // [popcount(mask)][n_cells]
    uint32_t mask;    // bit k = OrcDerivedField k; the same in every lane
};

// The selected fields of cell c from its gradient rows gx, gy, gz (G[i][j] = row i, component j) in THE operator order:
//   w = (G21 - G12, G02 - G20, G10 - G01)        |w| = sqrt((wx wx + wy wy) + wz wz)
//   S01 = (G01 + G10) / 2, S02 = (G02 + G20) / 2, S12 = (G12 + G21) / 2        W01 = (G01 - G10) / 2, W02, W12 likewise
//   SS = ((G00 G00 + G11 G11) + G22 G22) + 2 ((S01 S01 + S02 S02) + S12 S12)    OO = 2 ((W01 W01 + W02 W02) + W12 W12)
//   strain = sqrt(2 SS)    Q = (OO - SS) / 2    div = (G00 + G11) + G22    rate = conv / (2 V)
// Every branch tests the wave-uniform mask; the face loop is behind us.
__device__ __forceinline__ void derived_store(const DerivedArgs &A, int64_t n, int64_t c, V3 gx, V3 gy, V3 gz, double conv, double vol) {
    const uint32_t mask = A.mask;
    double *o = A.out + c;
    const double wx = gz.y - gy.z, wy = gx.z - gz.x, wz = gy.x - gx.y;
    if (mask & (1u << ORC_DERIVED_VORTICITY_X)) { *o = wx; o += n; }
    if (mask & (1u << ORC_DERIVED_VORTICITY_Y)) { *o = wy; o += n; }
    if (mask & (1u << ORC_DERIVED_VORTICITY_Z)) { *o = wz; o += n; }
    if (mask & (1u << ORC_DERIVED_VORTICITY_MAG)) { *o = sqrt((wx * wx + wy * wy) + wz * wz); o += n; }
    if (mask & ((1u << ORC_DERIVED_STRAIN_RATE_MAG) | (1u << ORC_DERIVED_Q_CRITERION))) {
        const double ss = strain_ss(gx, gy, gz);  // gradient_cell.hpp: shared with the viscosity laws
        if (mask & (1u << ORC_DERIVED_STRAIN_RATE_MAG)) { *o = strain_rate_mag(ss); o += n; }
        if (mask & (1u << ORC_DERIVED_Q_CRITERION)) {
            const double w01 = (gx.y - gy.x) / 2., w02 = (gx.z - gz.x) / 2., w12 = (gy.z - gz.y) / 2.;
            const double oo = 2. * ((w01 * w01 + w02 * w02) + w12 * w12);
            *o = (oo - ss) / 2.; o += n;
        }
    }
    if (mask & (1u << ORC_DERIVED_DIVERGENCE)) { *o = (gx.x + gy.y) + gz.z; o += n; }
    if (mask & (1u << ORC_DERIVED_CONVECTIVE_RATE)) *o = conv / (2. * vol);
}

// One thread per owned cell; XCD g (workgroups g, g + 8, ...) takes a contiguous eighth of the cells, so that the two cells of a
// face mostly share one L2 (scalar_k, momentum_k).  Reads what grad_u_k reads, writes popcount(mask) doubles per cell.
template <bool kLsq>
__global__ __launch_bounds__(kBlock) void derived_cell_k(MeshDev M, DerivedArgs A, int *status) {
    const int n_items = (int)M.n_own;  // cell ids are int32 (MeshDev.c0): the walk's counters fit with room to spare
    const int64_t n = M.n_cells;
    const int n_blk = (n_items + kBlock - 1) / kBlock;
    int vb = blockIdx.x, vb_end = n_blk, vb_step = gridDim.x;
    if ((gridDim.x & 7) == 0 && gridDim.x >= 8) {
        const int per = (n_blk + 7) / 8;
        const int xcd = blockIdx.x & 7;
        vb = xcd * per + (int)(blockIdx.x >> 3);
        vb_end = (xcd + 1) * per < n_blk ? (xcd + 1) * per : n_blk;
        vb_step = gridDim.x >> 3;
    }
    for (; vb < vb_end; vb += vb_step) {
        const int c = vb * kBlock + (int)threadIdx.x;
        if (c >= n_items) break;
        V3 gx, gy, gz;
        double conv;
        if (kLsq) {
            double g[3][3];
            grad_u_lsq_cell<true>(M, A.u, A.v, A.w, c, status, g, conv);
            gx = mk(g[0][0], g[0][1], g[0][2]); gy = mk(g[1][0], g[1][1], g[1][2]); gz = mk(g[2][0], g[2][1], g[2][2]);
        } else {
            grad_u_gg_cell<true>(M, A.u, A.v, A.w, c, status, gx, gy, gz, conv);
        }
        derived_store(A, n, c, gx, gy, gz, conv, M.vol[c]);
    }
}

struct BoundaryArgs {
    const int32_t *bface;
    int64_t nb;
    const double *u, *v, *w, *p;
    double rho, mu;
    const double *mu_cell;  // null, or the per-cell viscosity that replaces mu (variable viscosity on: the face's cell)
    double *out;  // [popcount(mask)][nb]
    uint32_t mask;
};

// The surface report's terms of one face (surface.hip surface_terms, same operator order), per unit area where the table says so:
//   p_f        t = Fv / A, Fv = d (U_P - U_f), d = (mu A) / dist, dist = sqrt((dx dx + dy dy) + dz dz), dx = x_f - x_P
//   tn = (t.x n.x + t.y n.y) + t.z n.z    s = t - tn n    shear = sqrt((s.x s.x + s.y s.y) + s.z s.z)
//   y+ = ((rho sqrt(shear / rho)) dist) / mu        mass flux = rho phi, phi = (n.x U.x + n.y U.y) + n.z U.z
// Traction, shear and y+ are exactly 0 where d_f is 0 (every zone but Wall and VelocityInlet), the flux where phi_f is.
__global__ __launch_bounds__(kBlock) void boundary_map_k(MeshDev M, BoundaryArgs A, int *status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.nb; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = A.bface[i];
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        const bool supported = zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET || zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET ||
                               zt == ORC_BC_SYMMETRY;
        double pf = 0., tx = 0., ty = 0., tz = 0., shear = 0., yplus = 0., flux = 0., a = 0.;
        if (!supported) {
            raise(status, ORC_ERR_UNSUPPORTED_BC);
        } else {
            const bool vec_bc = zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET;
            const bool p_bc = zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET;
            const bool no_flux = zt == ORC_BC_WALL || zt == ORC_BC_SYMMETRY;
            const int P = M.c0[f];
            a = M.area[f];
            const double nx = M.nx[f], ny = M.ny[f], nz = M.nz[f];
            const double upx = A.u[P], upy = A.v[P], upz = A.w[P];
            const double ufx = vec_bc ? M.zvec[3 * z] : upx, ufy = vec_bc ? M.zvec[3 * z + 1] : upy, ufz = vec_bc ? M.zvec[3 * z + 2] : upz;
            pf = p_bc ? M.zscal[z] : A.p[P];
            flux = no_flux ? 0. : A.rho * ((nx * ufx + ny * ufy) + nz * ufz);
            if (vec_bc) {
                const double dx = M.fcx[f] - M.ccx[P], dy = M.fcy[f] - M.ccy[P], dz = M.fcz[f] - M.ccz[P];
                const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                const double mu = A.mu_cell ? A.mu_cell[P] : A.mu;
                const double d = (mu * a) / dist;
                tx = (d * (upx - ufx)) / a; ty = (d * (upy - ufy)) / a; tz = (d * (upz - ufz)) / a;
                const double tn = (tx * nx + ty * ny) + tz * nz;
                const double sx = tx - tn * nx, sy = ty - tn * ny, sz = tz - tn * nz;
                shear = sqrt((sx * sx + sy * sy) + sz * sz);
                yplus = ((A.rho * sqrt(shear / A.rho)) * dist) / mu;
            }
        }
        const double val[ORC_BOUNDARY_N] = {pf, tx, ty, tz, shear, yplus, flux, a};
        double *o = A.out + i;
#pragma unroll
        for (int k = 0; k < ORC_BOUNDARY_N; ++k)
            if (A.mask & (1u << k)) { *o = val[k]; o += A.nb; }
    }
}

int fetch(DevBuf<int> &status, bool partitioned, const char *what) {
    int h = 0;
    ORC_TRY(status.download(&h, 1));
    if (partitioned) h = comm_global_status(h);
    if (h == ORC_ERR_SINGULAR_MATRIX) return set_error(h, "%s: singular least-squares system", what);
    if (h != ORC_OK) return set_error(h, "%s: a boundary face lies in a zone whose type the assembly does not support", what);
    return ORC_OK;
}

// u, v, w: device fields of the mesh's internal order, n_cells long (ghost entries are refreshed here on a partitioned mesh)
int derived_fields_dev(OrcMesh &m, double *u, double *v, double *w, const OrcSettings &settings, uint32_t mask, double *out) {
    const int recon = settings.gradient_reconstruction;
    if (recon != ORC_GRAD_GREEN_GAUSS_CELL && recon != ORC_GRAD_LEAST_SQUARES)
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "derived fields: unsupported gradient scheme");  // solver.rs:870
    if (m.halo.active()) { double *f[3] = {u, v, w}; ORC_TRY(m.halo.exchange(f, 3)); }
    const int k = popcount32(mask);
    DevBuf<double> dev;
    DevBuf<int> status;
    ORC_TRY(dev.alloc((size_t)k * (size_t)m.n_cells));
    ORC_TRY(dev.zero());  // the ghost cells' entries of a partitioned mesh stay zero
    ORC_TRY(status.alloc(1));
    ORC_TRY(status.zero());
    DerivedArgs A{u, v, w, dev.p, mask};
    const int grid = grid_for(m.n_own);
    if (recon == ORC_GRAD_LEAST_SQUARES)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(derived_cell_k<true>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), A, status.p);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(derived_cell_k<false>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), A, status.p);
    ORC_HIP(hipGetLastError());
    ORC_TRY(download_cells(m, dev.p, out, k));  // entries past n_own were zeroed on the device
    return fetch(status, m.halo.active(), "derived fields");
}

int boundary_fields_dev(OrcMesh &m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                        const double *mu_cell, uint32_t mask, double *out) {
    ORC_TRY(surface_index(m));
    const SurfaceIndex &X = *m.surface;
    const int k = popcount32(mask);
    const int64_t nb = X.n_bfaces;
    DevBuf<int> status;
    ORC_TRY(status.alloc(1));
    ORC_TRY(status.zero());
    if (nb > 0) {
        DevBuf<double> dev;
        ORC_TRY(dev.alloc((size_t)k * (size_t)nb));
        ORC_TRY(boundary_maps_dev(m, u, v, w, p, rho, mu, mu_cell, mask, dev.p, status.p));
        ORC_TRY(dev.download(out, (size_t)k * (size_t)nb));
    }
    return fetch(status, m.halo.active(), "boundary fields");
}

}  // namespace

int boundary_maps_dev(OrcMesh &m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                      const double *mu_cell, uint32_t mask, double *out_dev, int *status_dev) {
    ORC_TRY(surface_index(m));
    const SurfaceIndex &X = *m.surface;
    const int64_t nb = X.n_bfaces;
    if (nb == 0) return ORC_OK;
    BoundaryArgs A{X.bface.p, nb, u, v, w, p, rho, mu, mu_cell, out_dev, mask};
    hipLaunchKernelGGL(boundary_map_k, dim3(grid_for(nb)), dim3(kBlock), 0, ctx().stream, m.dev(), A, status_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace orc

using namespace orc;

extern "C" {

int orc_solver_derived_fields(OrcSolver *s, uint32_t mask, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "derived fields: null argument");
    if (mask == 0 || (mask >> ORC_DERIVED_N) != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "derived fields: mask 0x%x selects nothing or an unknown field", mask);
    SolverState &st = s->st;
    return derived_fields_dev(*st.mesh, st.u.p, st.v.p, st.w.p, st.settings, mask, out);
}

int orc_derived_fields(OrcMesh *m, const double *u, const double *v, const double *w, const OrcSettings *settings, uint32_t mask, double *out) {
    ORC_TRY(ensure_init());
    if (!m || !u || !v || !w || !settings || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "derived fields: null argument");
    if (mask == 0 || (mask >> ORC_DERIVED_N) != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "derived fields: mask 0x%x selects nothing or an unknown field", mask);
    const double *src[3] = {u, v, w};
    DevBuf<double> dev[3];
    for (int k = 0; k < 3; ++k) ORC_TRY(upload_cells(*m, src[k], dev[k]));
    return derived_fields_dev(*m, dev[0].p, dev[1].p, dev[2].p, *settings, mask, out);
}

// the comparison partner of orc_bench_courant: derived_cell_k selecting the convective rate alone (it forms the gradient as well and
// stores n doubles), HIP-event average ms over `reps` on the solver's current fields
int orc_bench_derived_rate(OrcSolver *s, int reps, double *avg_ms) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench derived rate: null argument");
    SolverState &st = s->st;
    OrcMesh &m = *st.mesh;
    if (reps < 1) reps = 1;
    DevBuf<double> dev;
    DevBuf<int> status;
    ORC_TRY(dev.alloc((size_t)std::max<int64_t>(m.n_cells, 1)));
    ORC_TRY(status.alloc(1));
    ORC_TRY(status.zero());
    DerivedArgs A{st.u.p, st.v.p, st.w.p, dev.p, 1u << ORC_DERIVED_CONVECTIVE_RATE};
    const int grid = grid_for(m.n_own);
    const bool lsq = st.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES;
    auto launch = [&] {
        if (lsq) hipLaunchKernelGGL(HIP_KERNEL_NAME(derived_cell_k<true>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), A, status.p);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(derived_cell_k<false>), dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), A, status.p);
        return (int)ORC_OK;
    };
    float ms = 0.f;
    const bool ok = timed(reps, launch, &ms) == ORC_OK;
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // dev is freed on return
    if (!ok || hipGetLastError() != hipSuccess) return set_error(ORC_ERR_HIP, "timing derived_cell_k failed");
    *avg_ms = (double)ms;
    return ORC_OK;
}

int orc_solver_boundary_fields(OrcSolver *s, uint32_t mask, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "boundary fields: null argument");
    if (mask == 0 || (mask >> ORC_BOUNDARY_N) != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "boundary fields: mask 0x%x selects nothing or an unknown field", mask);
    SolverState &st = s->st;
    return boundary_fields_dev(*st.mesh, st.u.p, st.v.p, st.w.p, st.p.p, st.rho, st.mu, st.cell_viscosity(), mask, out);
}

int orc_boundary_fields(OrcMesh *m, const double *u, const double *v, const double *w, const double *p, double rho, double mu, uint32_t mask,
                        double *out) {
    ORC_TRY(ensure_init());
    if (!m || !u || !v || !w || !p || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "boundary fields: null argument");
    if (mask == 0 || (mask >> ORC_BOUNDARY_N) != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "boundary fields: mask 0x%x selects nothing or an unknown field", mask);
    if (!(rho > 0.) || !std::isfinite(rho) || !(mu > 0.) || !std::isfinite(mu))
        return set_error(ORC_ERR_BAD_ARGUMENT, "boundary fields: rho and mu must be positive and finite");
    const double *src[4] = {u, v, w, p};
    DevBuf<double> dev[4];
    for (int k = 0; k < 4; ++k) ORC_TRY(upload_cells(*m, src[k], dev[k]));
    return boundary_fields_dev(*m, dev[0].p, dev[1].p, dev[2].p, dev[3].p, rho, mu, nullptr, mask, out);
}

}  // extern "C"
