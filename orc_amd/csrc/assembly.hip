// assembly.hip — face-loop assembly of the SIMPLE iteration on the device.
// Reference: src/discretization.rs (all), src/solver.rs:774-802, 874-902, 952-1227.
//
// The reference walks cells, and inside each (cell, face) visit recomputes two or four
// Green-Gauss pressure gradients (solver.rs:1082-1084, 1139-1140).  p, u, v, w are immutable
// during an assembly, so here every gradient is evaluated once per cell (K9), every face flux and
// face pressure once per face (K10 — the two sides of a face see exactly opposite fluxes once the
// Rhie-Chow diagonals are frozen), and the cell kernel (K11/K12) only gathers.
// The cell kernels visit a cell's faces in ascending face id and use the reference's operator
// order, so with -ffp-contract=off every assembled coefficient is bit-identical to the CPU
// oracle in frozen-diagonal mode.  All kernels are HBM-bound gathers; no atomics are needed
// because each thread owns its matrix row.
// This file: the kernels and their launch wrappers (k_*), nothing else.  The solver's state is set up in solver_state.cpp, the
// iteration that calls the wrappers is simple_iteration.cpp, the initialisers and their kernels are initialize.hip.
#include <cmath>

#include "assembly.hpp"
#include "gradient_cell.hpp"
#include "linalg_kernels.hpp"

namespace orc {

// ------------------------------------------------------------------ K14: diffusion matrix (once)
// discretization.rs:39-131
__global__ void diffusion_k(MeshDev M, SellDev P, double mu, double *__restrict__ a_di, double *__restrict__ b_u,
                            double *__restrict__ b_v, double *__restrict__ b_w, int *status) {
    GRID_STRIDE(c, M.n_own) {
        const V3 cc = cell_centroid(M, (int)c);
        double a_p = 0., bu = 0., bv = 0., bw = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int z = M.fzone[f];
            const int zt = M.ztype[z];
            double d_i = 0.;
            if (zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET) {  // :70-79
                d_i = mu * M.area[f] / vnorm(vsub(face_centroid(M, f), cc));
                const V3 sc = vmuls(zone_vec(M, z), d_i);
                bu += sc.x; bv += sc.y; bw += sc.z;
            } else if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET || zt == ORC_BC_SYMMETRY) {  // :80-88
                d_i = 0.;
            } else if (zt == ORC_BC_INTERIOR) {  // :89-113
                const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
                d_i = mu * M.area[f] / vnorm(vsub(cell_centroid(M, nb), cc));
                a_di[M.cfpos[q]] = -d_i;  // :125
            } else {
                raise(status, ORC_ERR_UNSUPPORTED_BC);  // :114-117
            }
            a_p += d_i;
        }
        a_di[P.diag_pos[c]] = a_p;  // :128
        b_u[c] = bu; b_v[c] = bv; b_w[c] = bw;
    }
}

// discretization.rs:450-472
__global__ void init_momentum_k(MeshDev M, SellDev P, double *__restrict__ a) {
    GRID_STRIDE(c, M.n_own) {
        a[P.diag_pos[c]] = 1.;
        const double nf = (double)(M.cfp[c + 1] - M.cfp[c]);
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q)
            if (M.cfpos[q] >= 0) a[M.cfpos[q]] = -1. / nf;
    }
}

__global__ void extract_diag_k(SellDev P, const double *__restrict__ a, double *__restrict__ d) {
    GRID_STRIDE(c, P.n) d[c] = a[P.diag_pos[c]];
}

// ------------------------------------------------------------------ K9: Green-Gauss gradients
// face_pressure_linear — get_face_pressure with PressureInterpolation::Linear — lives in gradient_cell.hpp beside the gradient bodies.

// calculate_pressure_gradient, GreenGauss(CellBased) (solver.rs:883-900); returns (gx, gy, gy) under Q1; the per-cell body is
// grad_p_gg_cell (gradient_cell.hpp), shared with probe_sample_k
__global__ void grad_p_k(MeshDev M, const double *__restrict__ p, double *__restrict__ gp, int q1, int *status) {
    const int64_t n = M.n_cells;
    GRID_STRIDE(c, M.n_own) {
        const V3 acc = grad_p_gg_cell(M, p, c, q1, status);
        gp[c] = acc.x; gp[n + c] = acc.y; gp[2 * n + c] = acc.z;
    }
}


// calculate_velocity_gradient, GreenGauss arm (solver.rs:784-801): row = velocity component; the per-cell body is
// grad_u_gg_cell (gradient_cell.hpp), shared with derived_cell_k
__global__ void grad_u_k(MeshDev M, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                         double *__restrict__ gu, int *status) {
    const int64_t n = M.n_cells;
    GRID_STRIDE(c, M.n_own) {
        V3 tx, ty, tz;
        double conv;
        grad_u_gg_cell<false>(M, u, v, w, c, status, tx, ty, tz, conv);
        gu[0 * n + c] = tx.x; gu[1 * n + c] = tx.y; gu[2 * n + c] = tx.z;
        gu[3 * n + c] = ty.x; gu[4 * n + c] = ty.y; gu[5 * n + c] = ty.z;
        gu[6 * n + c] = tz.x; gu[7 * n + c] = tz.y; gu[8 * n + c] = tz.z;
    }
}


__global__ void grad_p_lsq_k(MeshDev M, const double *__restrict__ p, double *__restrict__ gp, int *status) {
    const int64_t n = M.n_cells;
    GRID_STRIDE(c, M.n_own) {
        double g[3];
        grad_p_lsq_cell(M, p, c, status, g);  // gradient_cell.hpp, shared with probe_sample_k
        gp[c] = g[0]; gp[n + c] = g[1]; gp[2 * n + c] = g[2];
    }
}

__global__ void grad_u_lsq_k(MeshDev M, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                             double *__restrict__ gu, int *status) {
    const int64_t n = M.n_cells;
    GRID_STRIDE(c, M.n_own) {
        double g[3][3], conv;
        grad_u_lsq_cell<false>(M, u, v, w, c, status, g, conv);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) gu[(3 * r + k) * n + c] = g[r][k];
    }
}

// ------------------------------------------------------------------ K10: face flux / face pressure
struct FaceArgs {
    const double *u, *v, *w, *p, *gp, *du, *dv, *dw;
    int vinterp, pinterp, q1;
    double rho;
};

// get_face_flux seen from cell_indices[0] (solver.rs:1007-1102); the other side is the exact negative GIVEN the same two
// momentum diagonals.  d_i / d_j: a_{u,v,w}.get(i,i) / get(j,j) as the visiting cell sees them (both from the previous
// iteration with frozen diagonals; the reference's in-place mix otherwise, momentum_k<true>).
__device__ __forceinline__ double face_flux_c0(const MeshDev &M, const FaceArgs &A, int f, int zt, int z, int *status, V3 d_i, V3 d_j) {
    const int i = M.c0[f];
    const V3 n = face_normal(M, f);
    if (zt == ORC_BC_WALL || zt == ORC_BC_SYMMETRY) return 0.;  // :1026
    if (zt == ORC_BC_VELOCITY_INLET) return vdot(n, zone_vec(M, z));  // :1027-1039
    if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET) return vdot(n, mk(A.u[i], A.v[i], A.w[i]));
    if (zt != ORC_BC_INTERIOR) { raise(status, ORC_ERR_UNSUPPORTED_BC); return 0.; }  // :1100
    const int j = M.c1[f];
    const V3 vel_i = mk(A.u[i], A.v[i], A.w[i]), vel_j = mk(A.u[j], A.v[j], A.w[j]);
    if (A.vinterp == ORC_VINTERP_LINEAR) return vdot(n, vdivs(vadd(vel_i, vel_j), 2.));  // :987
    if (A.vinterp == ORC_VINTERP_LINEAR_WEIGHTED) {  // :988-992
        const V3 fc = face_centroid(M, f);
        const double dx0 = vnorm(vsub(cell_centroid(M, i), fc)), dx1 = vnorm(vsub(cell_centroid(M, j), fc));
        return vdot(n, vadd(vel_i, vdivs(vmuls(vsub(vel_j, vel_i), dx0), dx0 + dx1)));
    }
    // Rhie-Chow (:1051-1095)
    const int64_t nc = M.n_cells;
    const V3 ccv = vsub(cell_centroid(M, j), cell_centroid(M, i));
    const double a_i = vnorm(mk(d_i.x * n.x, d_i.y * n.y, d_i.z * n.z));  // discretization.rs:14-23
    const double a_j = vnorm(mk(d_j.x * n.x, d_j.y * n.y, d_j.z * n.z));
    const V3 g_i = mk(A.gp[i], A.gp[nc + i], A.gp[2 * nc + i]), g_j = mk(A.gp[j], A.gp[nc + j], A.gp[2 * nc + j]);
    const double vol_i = M.vol[i], vol_j = M.vol[j];
    const double len = vnorm(ccv);
    const double term_1 = vdot(vadd(vel_i, vel_j), n);
    const double term_2 = (vol_i / a_i + vol_j / a_j) * (A.p[i] - A.p[j]) / len;
    const V3 unit = mk(ccv.x / len, ccv.y / len, ccv.z / len);
    const double term_3 = vdot(vadd(smulv(vol_i / a_i, g_i, A.q1), smulv(vol_j / a_j, g_j, A.q1)), unit);
    return 0.5 * (term_1 + term_2 - term_3);
}

// get_face_pressure (solver.rs:1104-1150)
__device__ __forceinline__ double face_pressure(const MeshDev &M, const FaceArgs &A, int f, int zt, int z) {
    if (zt != ORC_BC_INTERIOR) return face_pressure_linear(M, A.p, f, zt, z);
    const int c0 = M.c0[f], c1 = M.c1[f];
    const double p0 = A.p[c0], p1 = A.p[c1];
    if (A.pinterp == ORC_PINTERP_LINEAR) return (p0 + p1) * 0.5;
    const V3 fc = face_centroid(M, f);
    if (A.pinterp == ORC_PINTERP_LINEAR_WEIGHTED) {  // :1129-1133
        const double x0 = vnorm(vsub(cell_centroid(M, c0), fc)), x1 = vnorm(vsub(cell_centroid(M, c1), fc));
        return p0 + (p1 - p0) * x0 / (x0 + x1);
    }
    // SecondOrder (:1138-1144)
    const int64_t nc = M.n_cells;
    const V3 g0 = mk(A.gp[c0], A.gp[nc + c0], A.gp[2 * nc + c0]), g1 = mk(A.gp[c1], A.gp[nc + c1], A.gp[2 * nc + c1]);
    const V3 r0 = vsub(fc, cell_centroid(M, c0)), r1 = vsub(fc, cell_centroid(M, c1));
    return 0.5 * ((p0 + p1) + (vdot(g0, r0) + vdot(g1, r1)));
}

// MODE 0: momentum phase (flux + face pressure); MODE 1: pressure-correction phase (flux + coefficient)
template <int MODE>
__global__ void face_k(MeshDev M, FaceArgs A, double *__restrict__ flux, double *__restrict__ pf, double *__restrict__ coef, int *status) {
    GRID_STRIDE(f, M.n_faces) {
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        {
            const int i0 = M.c0[f], j0 = M.c1[f] >= 0 ? M.c1[f] : M.c0[f];
            flux[f] = face_flux_c0(M, A, (int)f, zt, z, status, mk(A.du[i0], A.dv[i0], A.dw[i0]), mk(A.du[j0], A.dv[j0], A.dw[j0]));
        }
        if (MODE == 0) {
            pf[f] = bc_supported(zt) ? face_pressure(M, A, (int)f, zt, z) : 0.;
        } else {
            // discretization.rs:401-436: rho * A^2 / a~ ; a~ from the (sign-insensitive) inward normal
            const V3 n = face_normal(M, (int)f);
            const int i = M.c0[f], j = M.c1[f];
            const double ar = M.area[f];
            if (j >= 0) {
                const double a_int = 0.5 * vnorm(mk((A.du[i] + A.du[j]) * -n.x, (A.dv[i] + A.dv[j]) * -n.y, (A.dw[i] + A.dw[j]) * -n.z));
                coef[f] = A.rho * (ar * ar) / a_int;
            } else {
                const double a_ii = vnorm(mk(A.du[i] * -n.x, A.dv[i] * -n.y, A.dw[i] * -n.z));
                coef[f] = A.rho * (ar * ar) / a_ii;
            }
        }
    }
}

// the coefficient half of face_k<1> alone: what the p' MATRIX needs (no velocity is read)
__global__ void face_coef_k(MeshDev M, const double *__restrict__ du, const double *__restrict__ dv, const double *__restrict__ dw, double rho,
                            double *__restrict__ coef) {
    GRID_STRIDE(f, M.n_faces) {
        const V3 n = face_normal(M, (int)f);
        const int i = M.c0[f], j = M.c1[f];
        const double ar = M.area[f];
        if (j >= 0) {
            const double a_int = 0.5 * vnorm(mk((du[i] + du[j]) * -n.x, (dv[i] + dv[j]) * -n.y, (dw[i] + dw[j]) * -n.z));
            coef[f] = rho * (ar * ar) / a_int;
        } else {
            const double a_ii = vnorm(mk(du[i] * -n.x, dv[i] * -n.y, dw[i] * -n.z));
            coef[f] = rho * (ar * ar) / a_ii;
        }
    }
}

// ------------------------------------------------------------------ K11: momentum matrices
// psi_eval (lib.rs:107-118): assembly.hpp, shared with the scalar arm's face correction

struct MomentumArgs {
    const double *u, *v, *w, *gu, *flux, *pf, *a_di, *b_u_di, *b_v_di, *b_w_di;
    double *a_u, *a_v, *a_w, *b_u, *b_v, *b_w, *du, *dv, *dw;
    int momentum, q1;
    double rho;
};

// The reference's in-place diagonal reads (discretization.rs:182-197, 340-351; frozen_diagonals = 0): while cell
// c is assembled, Rhie-Chow sees THIS iteration's diagonal of a neighbour j < c (its row is already rewritten) and LAST
// iteration's of c itself and of every j > c.  New diagonals thus form a triangular recurrence over the cell order; it
// is evaluated level by level (level(c) = 1 + max level of the neighbours below c): the cells of one level only read new
// diagonals of lower levels, so a level is one parallel launch over its cell list.
struct InplaceArgs {
    const int32_t *cells;  // cells of this level (ascending)
    int64_t count;
    const double *du_old, *dv_old, *dw_old;  // diagonals of the previous iteration
    double *pe;                              // [3][n] per-cell Peclet terms, folded after the last level
    FaceArgs F;                              // what get_face_flux reads
    int *status;
};

// discretization.rs:134-356, one thread per cell (= per matrix row)
template <bool kInplace>
__global__ __launch_bounds__(kBlock) void momentum_k(MeshDev M, SellDev P, MomentumArgs A, double *__restrict__ partials, InplaceArgs I) {
    __shared__ double lds[8];
    const int64_t n = M.n_cells;
    double pe_sum = 0., pe_min = INFINITY, pe_max = -INFINITY;
    const bool tvd = A.momentum >= ORC_MOMENTUM_TVD_LUD;
    // [r04] Cells in blocks of one workgroup; XCD g (workgroups g, g + 8, ...) walks a contiguous eighth of the blocks.  With the plain grid
    // stride neighbouring blocks — the two cells of every y- and z-face — sit on different XCDs, each XCD's L2 fetches the face's geometry, flux
    // and the neighbour's fields for itself, and the kernel moved 3.2x its algorithmic bytes (18.3 GB against 5.8 GB).
    const int64_t n_items = kInplace ? I.count : M.n_own;
    const int64_t n_blk = (n_items + blockDim.x - 1) / blockDim.x;
    int64_t vb = blockIdx.x, vb_end = n_blk, vb_step = gridDim.x;
    if (!kInplace && (gridDim.x & 7) == 0 && gridDim.x >= 8) {
        const int64_t per = (n_blk + 7) / 8;
        const int xcd = blockIdx.x & 7;
        vb = (int64_t)xcd * per + (blockIdx.x >> 3);
        vb_end = (int64_t)(xcd + 1) * per < n_blk ? (int64_t)(xcd + 1) * per : n_blk;
        vb_step = gridDim.x >> 3;
    }
    for (; vb < vb_end; vb += vb_step) {
        const int64_t idx = vb * blockDim.x + threadIdx.x;
        if (idx >= n_items) break;
        const int64_t c = kInplace ? (int64_t)I.cells[idx] : idx;
        V3 s_u = mk(0., 0., 0.);  // get_momentum_source_term (solver.rs:698-701)
        const int dpos = P.diag_pos[c];
        const double a_ii_di = A.a_di[dpos];  // :176
        V3 a_p = mk(0., 0., 0.);
        const V3 vel = mk(A.u[c], A.v[c], A.w[c]);
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const bool side0 = M.c0[f] == c;
            V3 n_out = face_normal(M, f);
            if (!side0) n_out = vneg(n_out);
            double face_flux = side0 ? A.flux[f] : -A.flux[f];
            if (kInplace && M.c1[f] >= 0 && I.F.vinterp == ORC_VINTERP_RHIE_CHOW) {
                // the visiting cell's own mix of old and new diagonals (get() on the matrices being rewritten)
                const int i0 = M.c0[f], j0 = M.c1[f];
                const int other = side0 ? j0 : i0;
                const V3 d_self = mk(I.du_old[c], I.dv_old[c], I.dw_old[c]);
                const V3 d_other = other < c ? mk(A.du[other], A.dv[other], A.dw[other]) : mk(I.du_old[other], I.dv_old[other], I.dw_old[other]);
                const double fl = face_flux_c0(M, I.F, f, ORC_BC_INTERIOR, M.fzone[f], I.status, side0 ? d_self : d_other, side0 ? d_other : d_self);
                face_flux = side0 ? fl : -fl;
            }
            const double ar = M.area[f];
            const double f_i = face_flux * ar * A.rho;  // :202
            const double face_pressure = A.pf[f];
            const int c1 = M.c1[f];
            const int nb = c1 < 0 ? -1 : (side0 ? c1 : M.c0[f]);
            V3 a_nb;
            if (A.momentum == ORC_MOMENTUM_UD || (tvd && nb < 0)) {
                a_nb = smulv(fmin(f_i, 0.), mk(1., 1., 1.), A.q1);  // :226, :238
            } else if (A.momentum == ORC_MOMENTUM_CD1) {
                a_nb = vdivs(smulv(f_i, mk(1., 1., 1.), A.q1), 2.);  // :231
            } else {
                const int down = f_i > 0. ? nb : (int)c;  // :244-248
                const V3 dvel = mk(A.u[down], A.v[down], A.w[down]);
                const V3 dv = vsub(dvel, vel);
                if (vnorm(dv) == 0.) {
                    a_nb = vdivs(smulv(f_i, mk(1., 1., 1.), A.q1), 2.);  // :264
                } else {
                    const V3 r_pa = vsub(cell_centroid(M, nb), cell_centroid(M, (int)c));
                    const V3 gx = mk(A.gu[c], A.gu[n + c], A.gu[2 * n + c]);
                    const V3 gy = mk(A.gu[3 * n + c], A.gu[4 * n + c], A.gu[5 * n + c]);
                    const V3 gz = mk(A.gu[6 * n + c], A.gu[7 * n + c], A.gu[8 * n + c]);
                    const V3 inner = mk(vdot(gx, r_pa), vdot(gy, r_pa), vdot(gz, r_pa));  // lib.rs:584-590
                    const V3 two = smulv(2., inner, A.q1);                                   // :276
                    const V3 r = vadds(mk(two.x / dv.x, two.y / dv.y, two.z / dv.z), -1.);  // :277-278
                    const V3 ps = mk(psi_eval(A.momentum, r.x), psi_eval(A.momentum, r.y), psi_eval(A.momentum, r.z));
                    a_nb = vdivs(smulv(f_i, ps, A.q1), 2.);  // :279-283
                }
            }
            a_p = vadd(a_p, vadds(vneg(a_nb), f_i));                           // :290
            s_u = vadd(s_u, vmuls(vmuls(vneg(n_out), face_pressure), ar));     // :291
            if (nb < 0) {  // :294-307
                const int z = M.fzone[f];
                const int zt = M.ztype[z];
                if (zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET) {
                    const V3 vv = zone_vec(M, z);
                    s_u = vadd(s_u, mk((a_nb.x - f_i) * vv.x, (a_nb.y - f_i) * vv.y, (a_nb.z - f_i) * vv.z));
                } else {
                    s_u = vadd(s_u, mk(0., 0., 0.));
                }
            } else {  // :308-324
                const int pos = M.cfpos[q];
                const double a_ij_di = A.a_di[pos];
                A.a_u[pos] = a_nb.x + a_ij_di;
                A.a_v[pos] = a_nb.y + a_ij_di;
                A.a_w[pos] = a_nb.z + a_ij_di;
            }
        }
        const V3 total = vadd(vadd(s_u, mk(0., 0., 0.)), mk(0., 0., 0.));  // :326
        A.b_u[c] = total.x + A.b_u_di[c];                                   // :327-329 then solver.rs:80-82
        A.b_v[c] = total.y + A.b_v_di[c];
        A.b_w[c] = total.z + A.b_w_di[c];
        const double px = a_p.x / a_ii_di, py = a_p.y / a_ii_di, pz = a_p.z / a_ii_di;  // :331-333
        if (kInplace) { I.pe[c] = px; I.pe[n + c] = py; I.pe[2 * n + c] = pz; }
        else if (I.pe) I.pe[c] = (((0. + px) + py) + pz) / 3.;  // [r05] reference reduction order with frozen diagonals: the cell's term of :338
        pe_max = fmax(pe_max, fmax(px, fmax(py, pz)));
        pe_min = fmin(pe_min, fmin(px, fmin(py, pz)));
        pe_sum += (((0. + px) + py) + pz) / 3.;  // :338
        const double d_u = a_p.x + a_ii_di, d_v = a_p.y + a_ii_di, d_w = a_p.z + a_ii_di;  // :340-351
        A.a_u[dpos] = d_u; A.a_v[dpos] = d_v; A.a_w[dpos] = d_w;
        A.du[c] = d_u; A.dv[c] = d_v; A.dw[c] = d_w;
    }
    if (kInplace) return;  // the statistics are folded by peclet_stats_k once every level is done
    const double t = block_sum(pe_sum, lds);
    const double mn = -block_max(-pe_min, lds);
    const double mx = block_max(pe_max, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t;
        partials[gridDim.x + blockIdx.x] = mn;
        partials[2 * gridDim.x + blockIdx.x] = mx;
    }
}

// pe[c] <- (((0 + pe_x) + pe_y) + pe_z) / 3: the term cell c adds to the reference's running mean (discretization.rs:338)
__global__ void peclet_cell_term_k(double *__restrict__ pe, int64_t n) {
    GRID_STRIDE(c, n) pe[c] = (((0. + pe[c]) + pe[n + c]) + pe[2 * n + c]) / 3.;
}

// the Peclet statistics of momentum_k from the stored per-cell terms (same per-workgroup partial layout)
__global__ __launch_bounds__(kBlock) void peclet_stats_k(const double *__restrict__ pe, int64_t n_own, int64_t n, double *__restrict__ partials) {
    __shared__ double lds[8];
    double pe_sum = 0., pe_min = INFINITY, pe_max = -INFINITY;
    GRID_STRIDE(c, n_own) {
        const double px = pe[c], py = pe[n + c], pz = pe[2 * n + c];
        pe_max = fmax(pe_max, fmax(px, fmax(py, pz)));
        pe_min = fmin(pe_min, fmin(px, fmin(py, pz)));
        pe_sum += (((0. + px) + py) + pz) / 3.;
    }
    const double t = block_sum(pe_sum, lds);
    const double mn = -block_max(-pe_min, lds);
    const double mx = block_max(pe_max, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = t;
        partials[gridDim.x + blockIdx.x] = mn;
        partials[2 * gridDim.x + blockIdx.x] = mx;
    }
}

// ------------------------------------------------------------------ implicit time term (transient arm)
// After momentum_k, per owned cell with c = rho V_P / dt:  Euler  diag += c,     b += c u_n;
//                                                          BDF2   diag += a0 c,  b += c (a1 u_n - a2 u_nm1),
// a0, a1, a2 the variable-step coefficients of w = dt / dt_last, formed once on the host (SolverState::time_coef): 1.5, 2, 0.5 exactly
// for a fixed step, and a product with 2 or 0.5 is exact, so a fixed-step run keeps the bits the literals gave.
// The new diagonal also goes to du/dv/dw (written, never read), so Rhie-Chow and the p' coefficients see the time term.
// One pass over the three systems; the diagonal slots sit at depth k of their 64-row slice (SellDev::diag_pos), so a wave's
// read-modify-writes fall into as many 512-byte segments as its rows have distinct diagonal depths.
struct TimeTermArgs {
    const double *un, *vn, *wn, *unm1, *vnm1, *wnm1;
    double *a_u, *a_v, *a_w, *b_u, *b_v, *b_w, *du, *dv, *dw;
    double rho, dt, a0, a1, a2;
};

template <bool kBdf2>
__global__ __launch_bounds__(kBlock) void time_term_k(int64_t n_own, const double *__restrict__ vol, const int32_t *__restrict__ diag_pos,
                                                      TimeTermArgs T) {
    GRID_STRIDE(c, n_own) {
        const double coef = (T.rho * vol[c]) / T.dt;
        const int dpos = diag_pos[c];
        double add, su, sv, sw;
        if (kBdf2) {
            add = T.a0 * coef;
            su = coef * (T.a1 * T.un[c] - T.a2 * T.unm1[c]);
            sv = coef * (T.a1 * T.vn[c] - T.a2 * T.vnm1[c]);
            sw = coef * (T.a1 * T.wn[c] - T.a2 * T.wnm1[c]);
        } else {
            add = coef;
            su = coef * T.un[c];
            sv = coef * T.vn[c];
            sw = coef * T.wn[c];
        }
        const double d_u = T.a_u[dpos] + add, d_v = T.a_v[dpos] + add, d_w = T.a_w[dpos] + add;
        T.a_u[dpos] = d_u; T.a_v[dpos] = d_v; T.a_w[dpos] = d_w;
        T.du[c] = d_u; T.dv[c] = d_v; T.dw[c] = d_w;
        T.b_u[c] += su; T.b_v[c] += sv; T.b_w[c] += sw;
    }
}

// ------------------------------------------------------------------ K12: pressure-correction system
// discretization.rs:359-448 with the fixed pattern (no COO build / sort per iteration)
__global__ void pressure_k(MeshDev M, SellDev P, const double *__restrict__ flux, const double *__restrict__ coef, double rho,
                           double *__restrict__ a_p_mat, double *__restrict__ b_p) {
    GRID_STRIDE(c, M.n_own) {
        double a_p = 0., b = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const double out_flux = (M.c0[f] == c) ? flux[f] : -flux[f];
            b += rho * (-out_flux) * M.area[f];  // :399
            const double a_nb = coef[f];
            const int pos = M.cfpos[q];
            if (pos >= 0) {
                a_p_mat[pos] = -a_nb;  // :423
                a_p += a_nb;
            } else {
                a_p += a_nb / 2.;  // :435
            }
        }
        a_p_mat[P.diag_pos[c]] = a_p;  // :438
        b_p[c] = b;
    }
}

// ------------------------------------------------------------------ K13: velocity / pressure correction
// solver.rs:1170-1227 fused with the report sums of solver.rs:206-208
__global__ __launch_bounds__(kBlock) void correction_k(MeshDev M, const double *__restrict__ du, const double *__restrict__ dv,
                                                       const double *__restrict__ dw, const double *__restrict__ pp,
                                                       double *__restrict__ u, double *__restrict__ v, double *__restrict__ w,
                                                       double *__restrict__ p, double alpha_p, double alpha_u,
                                                       double *__restrict__ partials, int *status, double *__restrict__ corr_cell) {
    __shared__ double lds[8];
    double s_pp = 0., s_corr = 0., s_u = 0., s_v = 0., s_w = 0.;
    GRID_STRIDE(c, M.n_own) {
        const double ppc = pp[c];
        p[c] += alpha_p * ppc;  // :1186
        V3 acc = mk(0., 0., 0.);
        const double iu = du[c], iv = dv[c], iw = dw[c];
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int zt = M.ztype[M.fzone[f]];
            V3 n = face_normal(M, f);
            const bool side0 = M.c0[f] == c;
            if (!side0) n = vneg(n);
            double pp_nb;
            if (zt == ORC_BC_INTERIOR) pp_nb = pp[side0 ? M.c1[f] : M.c0[f]];
            else if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET) pp_nb = 0.;
            else if (zt == ORC_BC_WALL || zt == ORC_BC_SYMMETRY || zt == ORC_BC_VELOCITY_INLET) pp_nb = ppc;
            else { raise(status, ORC_ERR_UNSUPPORTED_BC); pp_nb = ppc; }  // :1209-1212
            const V3 scaled = mk(n.x / iu, n.y / iv, n.z / iw);
            acc = vadd(acc, vmuls(vmuls(scaled, ppc - pp_nb), M.area[f]));  // :1219
        }
        const double un = u[c] + acc.x * alpha_u, vn = v[c] + acc.y * alpha_u, wn = w[c] + acc.z * alpha_u;  // :1221-1223
        u[c] = un; v[c] = vn; w[c] = wn;
        const double nn = vnorm(acc);
        s_corr += nn * nn;  // :1224
        if (corr_cell) corr_cell[c] = nn * nn;  // reference reduction order: summed cell by cell afterwards (k_apply_correction)
        s_pp += ppc * ppc;
        s_u += un; s_v += vn; s_w += wn;
    }
    const double t0 = block_sum(s_pp, lds), t1 = block_sum(s_corr, lds), t2 = block_sum(s_u, lds), t3 = block_sum(s_v, lds),
                 t4 = block_sum(s_w, lds);
    if (threadIdx.x == 0) {
        const int g = gridDim.x;
        partials[blockIdx.x] = t0; partials[g + blockIdx.x] = t1; partials[2 * g + blockIdx.x] = t2;
        partials[3 * g + blockIdx.x] = t3; partials[4 * g + blockIdx.x] = t4;
    }
}

__global__ void negate_k(double *x) { if (threadIdx.x == 0 && blockIdx.x == 0) *x = -*x; }

__global__ void reduce_minmax_k(const double *__restrict__ partials, int count, double *__restrict__ out) {
    // out[0] = sum(partials[0..count)), out[1] = min(partials[count..2count)), out[2] = max(partials[2count..3count))
    if (threadIdx.x != 0) return;
    double s = 0., mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < count; ++i) { s += partials[i]; mn = fmin(mn, partials[count + i]); mx = fmax(mx, partials[2 * count + i]); }
    out[0] = s; out[1] = mn; out[2] = mx;
}

// ====================================================================== launch wrappers
int k_diffusion(SolverState &s) {
    OrcMesh &m = *s.mesh;
    ORC_TRY(s.a_di.zero());
    hipLaunchKernelGGL(diffusion_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), s.mu, s.a_di.p,
                       s.b_u_di.p, s.b_v_di.p, s.b_w_di.p, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_init_momentum(SolverState &s) {
    OrcMesh &m = *s.mesh;
    DevBuf<double> *mats[3] = {&s.a_u, &s.a_v, &s.a_w};
    for (auto *a : mats) {
        ORC_TRY(a->zero());
        hipLaunchKernelGGL(init_momentum_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), a->p);
    }
    ORC_HIP(hipGetLastError());
    ORC_TRY(vec_fill(s.du.p, 1., s.n));  // diag = 1.0: what Rhie-Chow reads in iteration 1
    ORC_TRY(vec_fill(s.dv.p, 1., s.n));
    ORC_TRY(vec_fill(s.dw.p, 1., s.n));
    return ORC_OK;
}

// grad p of the current pressure into `gp` [3][n] by the settings' gradient scheme (the caller checks the launch)
static void launch_grad_p(SolverState &s, double *gp) {
    OrcMesh &m = *s.mesh;
    if (s.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES)
        hipLaunchKernelGGL(grad_p_lsq_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), s.p.p, gp, s.dev_status.p);
    else
        hipLaunchKernelGGL(grad_p_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), s.p.p, gp, s.settings.q1_compat, s.dev_status.p);
}

int k_gradients(SolverState &s, bool need_gu) {
    OrcMesh &m = *s.mesh;
    launch_grad_p(s, s.gp.p);
    if (need_gu) {
        if (s.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES)
            hipLaunchKernelGGL(grad_u_lsq_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), s.u.p, s.v.p, s.w.p, s.gu.p, s.dev_status.p);
        else
            hipLaunchKernelGGL(grad_u_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), s.u.p, s.v.p, s.w.p, s.gu.p, s.dev_status.p);
    }
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// what get_face_flux / get_face_pressure read: the current fields and momentum diagonals, with grad p taken from `gp`
static FaceArgs face_args(SolverState &s, const double *gp) {
    return FaceArgs{s.u.p, s.v.p, s.w.p, s.p.p, gp, s.du.p, s.dv.p, s.dw.p, s.settings.velocity_interpolation,
                    s.settings.pressure_interpolation, s.settings.q1_compat, s.rho};
}

int k_face_flux(SolverState &s, bool momentum_phase) {
    OrcMesh &m = *s.mesh;
    const FaceArgs A = face_args(s, s.gp.p);
    const int g = grid_for(m.n_faces);
    if (momentum_phase)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(face_k<0>), dim3(g), dim3(kBlock), 0, ctx().stream, m.dev(), A, s.flux.p, s.pf.p, s.coef.p, s.dev_status.p);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(face_k<1>), dim3(g), dim3(kBlock), 0, ctx().stream, m.dev(), A, s.flux.p, s.pf.p, s.coef.p, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_momentum(SolverState &s, double *peclet_host) {
    OrcMesh &m = *s.mesh;
    MomentumArgs A{s.u.p, s.v.p, s.w.p, s.gu.p, s.flux.p, s.pf.p, s.a_di.p, s.b_u_di.p, s.b_v_di.p, s.b_w_di.p,
                   s.a_u.p, s.a_v.p, s.a_w.p, s.b_u.p, s.b_v.p, s.b_w.p, s.du.p, s.dv.p, s.dw.p, s.settings.momentum,
                   s.settings.q1_compat, s.rho};
    const int g = grid_for(s.n);
    bool ref_pe = false;  // the mean Peclet number as the reference's running sum (discretization.rs:338), reference reduction order only
    if (s.settings.frozen_diagonals == 0) {
        // in-place diagonals (the reference's own mode): level by level over the cell order
        ORC_TRY(vec_copy(s.du_old.p, s.du.p, s.n));
        ORC_TRY(vec_copy(s.dv_old.p, s.dv.p, s.n));
        ORC_TRY(vec_copy(s.dw_old.p, s.dw.p, s.n));
        InplaceArgs I;
        I.du_old = s.du_old.p; I.dv_old = s.dv_old.p; I.dw_old = s.dw_old.p;
        I.pe = s.pe.p;
        I.F = face_args(s, s.gp.p);
        I.status = s.dev_status.p;
        for (size_t l = 0; l + 1 < s.level_ptr.size(); ++l) {
            I.cells = s.level_cells.p + s.level_ptr[l];
            I.count = s.level_ptr[l + 1] - s.level_ptr[l];
            if (I.count == 0) continue;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_k<true>), dim3(grid_for(I.count)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), A, s.partials.p, I);
        }
        hipLaunchKernelGGL(peclet_stats_k, dim3(g), dim3(kBlock), 0, ctx().stream, s.pe.p, s.n_own, s.n, s.partials.p);
        ref_pe = s.settings.reduction_order == ORC_REDUCTION_REFERENCE && !s.mesh->halo.active() && peclet_host != nullptr;
        if (ref_pe) hipLaunchKernelGGL(peclet_cell_term_k, dim3(g), dim3(kBlock), 0, ctx().stream, s.pe.p, s.n);  // pe[c] = its term of :338
    } else {
        // [r05] frozen diagonals in the reference's reduction order (a verification mode too: the frozen oracle bit for bit, report included)
        InplaceArgs I{};
        ref_pe = s.settings.reduction_order == ORC_REDUCTION_REFERENCE && !s.mesh->halo.active() && peclet_host != nullptr && s.pe.p != nullptr;
        I.pe = ref_pe ? s.pe.p : nullptr;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(momentum_k<false>), dim3(g), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), A, s.partials.p, I);
    }
    hipLaunchKernelGGL(reduce_minmax_k, dim3(1), dim3(64), 0, ctx().stream, s.partials.p, g, s.scal.p + 8);
    ORC_HIP(hipGetLastError());
    if (ref_pe) ORC_TRY(sum_reference(s.pe.p, s.n, s.scal.p + 8));
    s.diagonals_assembled = true;
    if (s.transient && s.time_levels > 0) ORC_TRY(k_time_term(s));  // after the Peclet statistics, which exclude the time term
    if (peclet_host) {
        if (s.mesh->halo.active()) {  // statistics over the whole mesh: sum; max of (-min, max)
            hipLaunchKernelGGL(negate_k, dim3(1), dim3(1), 0, ctx().stream, s.scal.p + 9);
            ORC_TRY(comm_allreduce_sum(s.scal.p + 8, 1));
            ORC_TRY(comm_allreduce_max(s.scal.p + 9, 2));
            hipLaunchKernelGGL(negate_k, dim3(1), dim3(1), 0, ctx().stream, s.scal.p + 9);
        }
        ORC_HIP(hipMemcpyAsync(peclet_host, s.scal.p + 8, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        ORC_HIP(hipStreamSynchronize(ctx().stream));
        peclet_host[0] /= (double)s.mesh->n_global;  // discretization.rs:355
    }
    return ORC_OK;
}

int k_time_term(SolverState &s) {
    OrcMesh &m = *s.mesh;
    const bool bdf2 = s.tr.scheme == ORC_TIME_BDF2 && s.time_levels >= 2;  // BDF2 starts as Euler while one level is known
    const SolverState::TimeCoef k = s.time_coef();
    TimeTermArgs T{s.lev[0].p, s.lev[1].p, s.lev[2].p, s.lev[3].p, s.lev[4].p, s.lev[5].p, s.a_u.p, s.a_v.p, s.a_w.p,
                   s.b_u.p, s.b_v.p, s.b_w.p, s.du.p, s.dv.p, s.dw.p, s.rho, s.dt, k.a0, k.a1, k.a2};
    const int g = grid_for(s.n_own);
    if (bdf2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(time_term_k<true>), dim3(g), dim3(kBlock), 0, ctx().stream, s.n_own, m.vol.p, m.pat.diag_pos.p, T);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(time_term_k<false>), dim3(g), dim3(kBlock), 0, ctx().stream, s.n_own, m.vol.p, m.pat.diag_pos.p, T);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_pressure_correction(SolverState &s) {
    OrcMesh &m = *s.mesh;
    ORC_TRY(k_face_flux(s, false));
    hipLaunchKernelGGL(pressure_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), s.flux.p, s.coef.p, s.rho,
                       s.a_p.p, s.b_p.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_pressure_matrix(SolverState &s) {
    OrcMesh &m = *s.mesh;
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(face_coef_k, dim3(grid_for(m.n_faces)), dim3(kBlock), 0, st, m.dev(), s.du.p, s.dv.p, s.dw.p, s.rho, s.coef.p);
    hipLaunchKernelGGL(pressure_k, dim3(grid_for(s.n)), dim3(kBlock), 0, st, m.dev(), m.pat.dev(), s.flux.p, s.coef.p, s.rho, s.a_p.p, s.b_p.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int k_apply_correction(SolverState &s, double *sums_host) {
    OrcMesh &m = *s.mesh;
    const int g = grid_for(s.n);
    // [r04] The reference's own mode (in-place diagonals + nalgebra's reduction order, one GPU): the REPORT's sums are taken in the
    // reference's association too — p'.norm() through dotx (solver.rs:1226), the velocity-correction sum cell by cell (:1224), the
    // means as left-to-right folds (:206-208) — so that not only the fields but the six report doubles of an iteration are the
    // oracle's bit for bit (scripts/reference_mode_fullsize.py compares exactly those at 10.24 M cells).  s.pe is free by now.
    const bool ref_report = s.settings.reduction_order == ORC_REDUCTION_REFERENCE && !s.mesh->halo.active() && s.pe.p;
    hipLaunchKernelGGL(correction_k, dim3(g), dim3(kBlock), 0, ctx().stream, m.dev(), s.du.p, s.dv.p, s.dw.p, s.p_prime.p, s.u.p, s.v.p,
                       s.w.p, s.p.p, s.settings.pressure_relaxation, s.settings.momentum_relaxation, s.partials.p, s.dev_status.p,
                       ref_report ? s.pe.p : (double *)nullptr);
    ORC_HIP(hipGetLastError());
    if (ref_report) {
        ORC_TRY(dot_reference(s.p_prime.p, s.p_prime.p, s.n, s.scal.p + 0, nullptr));
        ORC_TRY(sum_reference(s.pe.p, s.n, s.scal.p + 1));
        ORC_TRY(sum_reference(s.u.p, s.n, s.scal.p + 2));
        ORC_TRY(sum_reference(s.v.p, s.n, s.scal.p + 3));
        ORC_TRY(sum_reference(s.w.p, s.n, s.scal.p + 4));
    } else {
        ORC_TRY(reduce_partials(s.partials.p, g, 5, s.scal.p, s.mesh->halo.active()));
    }
    if (sums_host) {
        ORC_HIP(hipMemcpyAsync(sums_host, s.scal.p, 5 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
        ORC_HIP(hipStreamSynchronize(ctx().stream));
    }
    return ORC_OK;
}

// ------------------------------------------------------------------ scalar arm (scalar.hip)
// The flux the momentum assembly would see for the current fields — grad p, then face_k<0> — written to the arm's own
// buffers: the flow's gp, flux, pf, partials and scal keep their values.
int k_scalar_face_flux(SolverState &s) {
    OrcMesh &m = *s.mesh;
    SolverState::Scalar &c = s.sc;
    ORC_TRY(exchange_fields(s));
    launch_grad_p(s, c.gp.p);
    ORC_HIP(hipGetLastError());
    ORC_TRY(exchange_gradient(s, c.gp.p));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(face_k<0>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(), face_args(s, c.gp.p), c.flux.p,
                       c.pf.p, (double *)nullptr, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace orc
