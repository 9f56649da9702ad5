// gradient_cell.hpp — the per-cell gradient arithmetic of the assembly (K9), shared by grad_u_k / grad_u_lsq_k / grad_p_k / grad_p_lsq_k
// (assembly.hip), derived_cell_k (derived.hip), courant_k (courant.hip), viscosity_cell_k (viscosity.hip) and probe_sample_k (probes.hip): the small vector type,
// the boundary-value rules, the two per-cell bodies of the velocity gradient and the two of the pressure gradient, the strain-rate
// magnitude; the grid-stride loop of the assembly kernels (assembly.hip, initialize.hip).
// Device code only.  Every operation and its order are the reference's; a kernel that calls a body gets the same bits as any other.
#pragma once
#include "assembly.hpp"

#ifdef __HIPCC__
#define GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

namespace orc {

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 mk(double x, double y, double z) { return {x, y, z}; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 vneg(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 vmuls(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }   // Vector * Float (lib.rs:479-492)
__device__ __forceinline__ V3 vdivs(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ V3 vadds(V3 a, double s) { return {a.x + s, a.y + s, a.z + s}; }
__device__ __forceinline__ double vdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double vnorm(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
// Float * Vector (lib.rs:540-548): z := rhs.y * self when q1
__device__ __forceinline__ V3 smulv(double s, V3 a, int q1) { return {a.x * s, a.y * s, (q1 ? a.y : a.z) * s}; }

__device__ __forceinline__ V3 face_normal(const MeshDev &M, int f) { return mk(M.nx[f], M.ny[f], M.nz[f]); }
__device__ __forceinline__ V3 cell_centroid(const MeshDev &M, int c) { return mk(M.ccx[c], M.ccy[c], M.ccz[c]); }
__device__ __forceinline__ V3 face_centroid(const MeshDev &M, int f) { return mk(M.fcx[f], M.fcy[f], M.fcz[f]); }
__device__ __forceinline__ V3 zone_vec(const MeshDev &M, int z) { return mk(M.zvec[3 * z], M.zvec[3 * z + 1], M.zvec[3 * z + 2]); }

__device__ __forceinline__ void raise(int *status, int code) { atomicCAS(status, 0, code); }

__device__ __forceinline__ bool bc_supported(int zt) {
    return zt == ORC_BC_INTERIOR || zt == ORC_BC_WALL || zt == ORC_BC_SYMMETRY || zt == ORC_BC_VELOCITY_INLET ||
           zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET;
}

// get_face_velocity(…, Linear) (solver.rs:952-987)
__device__ __forceinline__ V3 face_velocity_linear(const MeshDev &M, const double *__restrict__ u, const double *__restrict__ v,
                                                   const double *__restrict__ w, int f, int zt, int z) {
    const int a = M.c0[f];
    if (zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET) return zone_vec(M, z);
    if (zt == ORC_BC_INTERIOR) {
        const int b = M.c1[f];
        return vdivs(vadd(mk(u[a], v[a], w[a]), mk(u[b], v[b], w[b])), 2.);
    }
    return mk(u[a], v[a], w[a]);
}

// ------------------------------------------------------------------ least-squares gradients (solver.rs:803-869, 903-947)
// One thread per cell: the rows of the n x 3 system are the cell's faces in Cell.face_indices order — neighbour centroid
// minus cell centroid with the value DIFFERENCE on interior faces, face centroid minus cell centroid with the face VALUE
// itself on boundary faces (the reference's own formulation, solver.rs:830-838, 925-934) — and the normal equations are
// accumulated face by face in nalgebra's small-matrix product order (one gemv per output column: left-to-right sums,
// the first term assigned, (1 * a) * b per term), inverted with its closed 3 x 3 form (linalg/inverse.rs) and applied
// by one more gemv.  A zero determinant is the reference's `try_inverse().unwrap()` panic.
struct Lsq3 {
    double ata[3][3], atb[3][3];
    bool first = true;
    __device__ __forceinline__ void add_row(const double x[3], const double *b, int nb) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double t = (1. * x[i]) * x[j];
                ata[i][j] = first ? t : t + 1. * ata[i][j];
            }
            for (int q = 0; q < nb; ++q) {
                const double t = (1. * x[i]) * b[q];
                atb[q][i] = first ? t : t + 1. * atb[q][i];
            }
        }
        first = false;
    }
};
// nalgebra try_inverse, dimension 3, in place; false = singular
__device__ __forceinline__ bool inverse3(double a[3][3]) {
    const double m11 = a[0][0], m12 = a[0][1], m13 = a[0][2], m21 = a[1][0], m22 = a[1][1], m23 = a[1][2], m31 = a[2][0], m32 = a[2][1], m33 = a[2][2];
    const double minor_m12_m23 = m22 * m33 - m32 * m23;
    const double minor_m11_m23 = m21 * m33 - m31 * m23;
    const double minor_m11_m22 = m21 * m32 - m31 * m22;
    const double determinant = m11 * minor_m12_m23 - m12 * minor_m11_m23 + m13 * minor_m11_m22;
    if (determinant == 0.) return false;
    a[0][0] = minor_m12_m23 / determinant;
    a[0][1] = (m13 * m32 - m33 * m12) / determinant;
    a[0][2] = (m12 * m23 - m22 * m13) / determinant;
    a[1][0] = -minor_m11_m23 / determinant;
    a[1][1] = (m11 * m33 - m31 * m13) / determinant;
    a[1][2] = (m13 * m21 - m23 * m11) / determinant;
    a[2][0] = minor_m11_m22 / determinant;
    a[2][1] = (m12 * m31 - m32 * m11) / determinant;
    a[2][2] = (m11 * m22 - m21 * m12) / determinant;
    return true;
}
__device__ __forceinline__ void inv_times3(const double ainv[3][3], const double b[3], double out[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double y = (1. * ainv[i][0]) * b[0];
        y = (1. * ainv[i][1]) * b[1] + 1. * y;
        y = (1. * ainv[i][2]) * b[2] + 1. * y;
        out[i] = y;
    }
}

// |U_f . n| A of one face, U_f . n = (n.x U.x + n.y U.y) + n.z U.z: the term of the convective rate.  The same bits for n and -n, and
// for the U_f of face_velocity_linear however its two cells are ordered, so every face loop below adds the same number.
__device__ __forceinline__ double conv_face_term(V3 nrm, V3 fv, double area) { return fabs((nrm.x * fv.x + nrm.y * fv.y) + nrm.z * fv.z) * area; }

// The Green-Gauss velocity gradient of cell c (solver.rs:784-801): rows tx, ty, tz = grad u, grad v, grad w, the cell's faces in
// Cell.face_indices order.  kConv: also conv = sum over the same faces of |U_f . n| A (the convective rate of derived.hip; a face in a
// refused zone takes no part in either).  kGrad = false: the face loop with the gradient rows left out (they come back 0) — what
// courant_k (courant.hip) runs; conv has the bits of either reconstruction's, since both add conv_face_term of the same faces in order.
template <bool kConv, bool kGrad = true>
__device__ __forceinline__ void grad_u_gg_cell(const MeshDev &M, const double *__restrict__ u, const double *__restrict__ v,
                                               const double *__restrict__ w, int64_t c, int *status, V3 &tx, V3 &ty, V3 &tz, double &conv) {
    const double vol = M.vol[c];
    tx = mk(0., 0., 0.); ty = tx; tz = tx;
    conv = 0.;
    for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
        const int f = M.cf[q];
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        if (!bc_supported(zt)) { raise(status, ORC_ERR_UNSUPPORTED_BC); continue; }  // solver.rs:1001
        const V3 fv = face_velocity_linear(M, u, v, w, f, zt, z);
        V3 nrm = face_normal(M, f);
        if (M.c0[f] != c) nrm = vneg(nrm);
        if (kGrad) {
            const V3 nn = vmuls(nrm, M.area[f] / vol);  // :799
            tx = vadd(tx, mk(fv.x * nn.x, fv.x * nn.y, fv.x * nn.z));  // outer (lib.rs:275-293)
            ty = vadd(ty, mk(fv.y * nn.x, fv.y * nn.y, fv.y * nn.z));
            tz = vadd(tz, mk(fv.z * nn.x, fv.z * nn.y, fv.z * nn.z));
        }
        if (kConv) conv = conv + conv_face_term(nrm, fv, M.area[f]);
    }
}

// The least-squares velocity gradient of cell c (solver.rs:803-869): g[r] = grad of velocity component r, zeros and
// ORC_ERR_SINGULAR_MATRIX when the normal matrix has no inverse.  kConv as above, with face_velocity_linear's U_f formed from the
// values the row already holds.
template <bool kConv>
__device__ __forceinline__ void grad_u_lsq_cell(const MeshDev &M, const double *__restrict__ u, const double *__restrict__ v,
                                                const double *__restrict__ w, int64_t c, int *status, double g[3][3], double &conv) {
    const V3 cc = cell_centroid(M, (int)c);
    Lsq3 L;
    conv = 0.;
    for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
        const int f = M.cf[q];
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        if (!bc_supported(zt)) { raise(status, ORC_ERR_UNSUPPORTED_BC); continue; }
        V3 d, lin = mk(0., 0., 0.);
        double b[3];
        if (zt == ORC_BC_INTERIOR) {
            const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
            d = vsub(cell_centroid(M, nb), cc);
            b[0] = u[nb] - u[c]; b[1] = v[nb] - v[c]; b[2] = w[nb] - w[c];
            if (kConv) lin = vdivs(vadd(mk(u[c], v[c], w[c]), mk(u[nb], v[nb], w[nb])), 2.);  // face_velocity_linear: a + b = b + a
        } else {  // get_face_velocity(…, None): zone vector on walls / velocity inlets, cell-0 velocity elsewhere
            d = vsub(face_centroid(M, f), cc);
            const int a0 = M.c0[f];
            const V3 fv = (zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET) ? zone_vec(M, z) : mk(u[a0], v[a0], w[a0]);
            b[0] = fv.x; b[1] = fv.y; b[2] = fv.z;
            if (kConv) lin = fv;  // the boundary value of face_velocity_linear is this one
        }
        const double x[3] = {d.x, d.y, d.z};
        L.add_row(x, b, 3);
        if (kConv) {
            conv = conv + conv_face_term(face_normal(M, f), lin, M.area[f]);  // |U_f . n| is the same for n and -n
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) g[r][k] = 0.;
    if (L.first || !inverse3(L.ata)) raise(status, ORC_ERR_SINGULAR_MATRIX);
    else {
        inv_times3(L.ata, L.atb[0], g[0]);
        inv_times3(L.ata, L.atb[1], g[1]);
        inv_times3(L.ata, L.atb[2], g[2]);
    }
}

// get_face_pressure with PressureInterpolation::Linear (solver.rs:1114-1128)
__device__ __forceinline__ double face_pressure_linear(const MeshDev &M, const double *__restrict__ p, int f, int zt, int z) {
    if (zt == ORC_BC_INTERIOR) return (p[M.c0[f]] + p[M.c1[f]]) * 0.5;
    if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET) return M.zscal[z];
    return p[M.c0[f]];  // Symmetry | Wall | VelocityInlet
}

// The Green-Gauss pressure gradient of cell c (calculate_pressure_gradient, GreenGauss(CellBased), solver.rs:883-900): the body of
// grad_p_k (assembly.hip), shared with probe_sample_k (probes.hip); returns (gx, gy, gy) under Q1
__device__ __forceinline__ V3 grad_p_gg_cell(const MeshDev &M, const double *__restrict__ p, int64_t c, int q1, int *status) {
    const double vol = M.vol[c];
    V3 acc = mk(0., 0., 0.);
    for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
        const int f = M.cf[q];
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        if (!bc_supported(zt)) { raise(status, ORC_ERR_UNSUPPORTED_BC); continue; }  // solver.rs:1148
        const double fv = face_pressure_linear(M, p, f, zt, z);
        V3 nrm = face_normal(M, f);
        if (M.c0[f] != c) nrm = vneg(nrm);
        acc = vadd(acc, smulv(fv * (M.area[f] / vol), nrm, q1));  // :896-898
    }
    return acc;
}

// The least-squares pressure gradient of cell c: the body of grad_p_lsq_k (assembly.hip), rows as in grad_u_lsq_cell; zeros and
// ORC_ERR_SINGULAR_MATRIX when the normal matrix has no inverse
__device__ __forceinline__ void grad_p_lsq_cell(const MeshDev &M, const double *__restrict__ p, int64_t c, int *status, double g[3]) {
    const V3 cc = cell_centroid(M, (int)c);
    Lsq3 L;
    for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
        const int f = M.cf[q];
        const int z = M.fzone[f];
        const int zt = M.ztype[z];
        if (!bc_supported(zt)) { raise(status, ORC_ERR_UNSUPPORTED_BC); continue; }
        V3 d;
        double val;
        if (zt == ORC_BC_INTERIOR) {
            const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
            d = vsub(cell_centroid(M, nb), cc);
            val = p[nb] - p[c];
        } else {  // get_face_pressure(…, None, None): zone scalar on pressure zones, cell-0 value elsewhere
            d = vsub(face_centroid(M, f), cc);
            val = (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET) ? M.zscal[z] : p[M.c0[f]];
        }
        const double x[3] = {d.x, d.y, d.z};
        L.add_row(x, &val, 1);
    }
    g[0] = 0.; g[1] = 0.; g[2] = 0.;
    if (L.first || !inverse3(L.ata)) raise(status, ORC_ERR_SINGULAR_MATRIX);  // a cell without faces: 0 x 0 ... the reference cannot get there either
    else inv_times3(L.ata, L.atb[0], g);
}

// SS = S : S of the gradient rows gx, gy, gz (G[i][j] = row i, component j) and the strain-rate magnitude sqrt(2 SS), in THE operator
// order of DESIGN §3 "Derived fields and boundary maps": what derived_store (derived.hip) writes as ORC_DERIVED_STRAIN_RATE_MAG and
// what viscosity_cell_k (viscosity.hip) evaluates its law at — one expression, the same bits.
__device__ __forceinline__ double strain_ss(V3 gx, V3 gy, V3 gz) {
    const double s01 = (gx.y + gy.x) / 2., s02 = (gx.z + gz.x) / 2., s12 = (gy.z + gz.y) / 2.;
    return ((gx.x * gx.x + gy.y * gy.y) + gz.z * gz.z) + 2. * ((s01 * s01 + s02 * s02) + s12 * s12);
}
__device__ __forceinline__ double strain_rate_mag(double ss) { return sqrt(2. * ss); }

}  // namespace orc
#endif
