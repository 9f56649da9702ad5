// initialize.hip — solver::initialize_* and check_boundary_conditions on the device (solver.rs:246-772), with the kernels only they
// launch: the Laplace system of the pressure initialisation, the potential-flow system and its velocities, the matrix blend of
// initialize_flow.  Everything else they run is the SIMPLE iteration's own (the k_* wrappers of assembly.hip, iterative_solve_dev).
#include <algorithm>
#include <cmath>

#include "assembly.hpp"
#include "gradient_cell.hpp"

namespace orc {

// ------------------------------------------------------------------ initialize_pressure_field's Laplace system
// solver.rs:436-492 on the mesh pattern: interior faces couple the two cells with
// a_nb = (cc - c_nb).reciprocal() . n_out * (A / V); pressure boundaries add a_nb to the diagonal and a_nb * P_bc to b;
// every other zone type contributes nothing.  Sums run in Cell.face_indices order from 0.0 like the reference's.
__device__ __forceinline__ V3 vreciprocal(V3 a) {  // lib.rs:246-252
    return mk(a.x != 0. ? 1. / a.x : 0., a.y != 0. ? 1. / a.y : 0., a.z != 0. ? 1. / a.z : 0.);
}

__global__ void laplace_p_k(MeshDev M, SellDev P, double *__restrict__ a, double *__restrict__ b, int *status) {
    GRID_STRIDE(c, M.n_own) {
        const V3 cc = cell_centroid(M, (int)c);
        const double vol = M.vol[c];
        double a_p = 0., src = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int z = M.fzone[f];
            const int zt = M.ztype[z];
            V3 nrm = mk(M.nx[f], M.ny[f], M.nz[f]);
            if (M.c0[f] != c) nrm = vneg(nrm);  // get_outward_face_normal (mesh.rs:216-222)
            double a_nb = 0., source = 0.;
            if (zt == ORC_BC_INTERIOR) {  // :451-466
                if (M.cfpos[q] < 0) { raise(status, ORC_ERR_BAD_ARGUMENT); continue; }  // cell_indices[1] out of bounds in the reference
                const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
                a_nb = vdot(vreciprocal(vsub(cc, cell_centroid(M, nb))), nrm) * (M.area[f] / vol);
                a[M.cfpos[q]] = -a_nb;  // :486
            } else if (zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET) {  // :467-474
                a_nb = vdot(vreciprocal(vsub(cc, face_centroid(M, f))), nrm) * (M.area[f] / vol);
                source = a_nb * M.zscal[z];
            }
            src += source;  // :488
            a_p += a_nb;    // :489
        }
        a[P.diag_pos[c]] = a_p;  // :491
        b[c] = src;
    }
}

// &a * (1. - f) + &a_di * f (solver.rs:319, 329, 339): CSR scale, CSR scale, CSR add — entry-wise on the shared pattern
__global__ void blend_k(int64_t len, const double *__restrict__ a, const double *__restrict__ a_di, double one_minus_f, double f,
                        double *__restrict__ out) {
    GRID_STRIDE(i, len) out[i] = a[i] * one_minus_f + a_di[i] * f;
}

// ------------------------------------------------------------------ initialize_velocity_field (solver.rs:511-696)
// Potential-flow system for psi on the mesh pattern: interior coupling (cc - cc_nb).reciprocal() . n * A / V, velocity inlets
// put -U . n on the right-hand side, a pressure outlet adds (cc - fc).reciprocal() . n to the diagonal (no A / V: :565-575).
__global__ void psi_system_k(MeshDev M, SellDev P, double *__restrict__ a, double *__restrict__ b, int *status) {
    GRID_STRIDE(c, M.n_own) {
        const V3 cc = cell_centroid(M, (int)c);
        const double vol = M.vol[c];
        double a_p = 0., src = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int z = M.fzone[f];
            const int zt = M.ztype[z];
            V3 nrm = mk(M.nx[f], M.ny[f], M.nz[f]);
            if (M.c0[f] != c) nrm = vneg(nrm);
            double a_nb = 0., source = 0.;
            if (zt == ORC_BC_INTERIOR) {
                if (M.cfpos[q] < 0) { raise(status, ORC_ERR_BAD_ARGUMENT); continue; }
                const int nb = (M.c0[f] == c) ? M.c1[f] : M.c0[f];
                a_nb = vdot(vreciprocal(vsub(cc, cell_centroid(M, nb))), nrm) * (M.area[f] / vol);
                a[M.cfpos[q]] = -a_nb;
            } else if (zt == ORC_BC_VELOCITY_INLET) {
                source = -vdot(zone_vec(M, z), nrm);
            } else if (zt == ORC_BC_PRESSURE_OUTLET) {
                a_nb = vdot(vreciprocal(vsub(cc, face_centroid(M, f))), nrm);
            }
            src += source;
            a_p += a_nb;
        }
        a[P.diag_pos[c]] = a_p;
        b[c] = src;
    }
}

// velocity = least-squares gradient of psi over the interior neighbours, all-zero columns dropped (:622-692)
__global__ void psi_velocity_k(MeshDev M, const double *__restrict__ psi, double *__restrict__ u, double *__restrict__ v, double *__restrict__ w) {
    GRID_STRIDE(c, M.n_own) {
        const V3 cc = cell_centroid(M, (int)c);
        // pass 1: which columns have a non-zero minimum or maximum
        double mn[3] = {0., 0., 0.}, mx[3] = {0., 0., 0.};
        int rows = 0;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            if (M.c1[f] < 0) continue;
            const int nb = (M.c0[f] != c) ? M.c0[f] : M.c1[f];
            const V3 d = vsub(cell_centroid(M, nb), cc);
            const double x[3] = {d.x, d.y, d.z};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (rows == 0 || x[j] < mn[j]) mn[j] = x[j];
                if (rows == 0 || x[j] > mx[j]) mx[j] = x[j];
            }
            ++rows;
        }
        int cols[3], dim = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (mn[j] != 0. || mx[j] != 0.) cols[dim++] = j;
        // pass 2: normal equations of the selected columns, face by face
        double ata[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}}, atb[3] = {0., 0., 0.};
        bool first = true;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            if (M.c1[f] < 0) continue;
            const int nb = (M.c0[f] != c) ? M.c0[f] : M.c1[f];
            const V3 d = vsub(cell_centroid(M, nb), cc);
            const double x[3] = {d.x, d.y, d.z};
            const double dpsi = psi[nb] - psi[c];
            for (int i = 0; i < dim; ++i) {
                for (int j = 0; j < dim; ++j) {
                    const double t = (1. * x[cols[i]]) * x[cols[j]];
                    ata[i][j] = first ? t : t + 1. * ata[i][j];
                }
                const double t = (1. * x[cols[i]]) * dpsi;
                atb[i] = first ? t : t + 1. * atb[i];
            }
            first = false;
        }
        double cv[3] = {0., 0., 0.};
        bool ok = true;
        if (dim == 1) {
            if (ata[0][0] == 0.) ok = false;
            else cv[0] = (1. * (1. / ata[0][0])) * atb[0];
        } else if (dim == 2) {
            const double m11 = ata[0][0], m12 = ata[0][1], m21 = ata[1][0], m22 = ata[1][1];
            const double determinant = m11 * m22 - m21 * m12;
            if (determinant == 0.) ok = false;
            else {
                const double i00 = m22 / determinant, i01 = -m12 / determinant, i10 = -m21 / determinant, i11 = m11 / determinant;
                cv[0] = (1. * i01) * atb[1] + 1. * ((1. * i00) * atb[0]);
                cv[1] = (1. * i11) * atb[1] + 1. * ((1. * i10) * atb[0]);
            }
        } else if (dim == 3) {
            if (!inverse3(ata)) ok = false;
            else inv_times3(ata, atb, cv);
        }
        double comp[3] = {0., 0., 0.};
        if (ok)
            for (int j = 0; j < dim; ++j) comp[cols[j]] = cv[j];
        u[c] = comp[0] != comp[0] ? 0. : comp[0];
        v[c] = comp[1] != comp[1] ? 0. : comp[1];
        w[c] = comp[2] != comp[2] ? 0. : comp[2];
    }
}

// check_boundary_conditions (solver.rs:710-772).  Its angle tolerance is 5*180/pi radians (:713), which no angle
// exceeds, so the two "tangent" panics cannot fire; what remains is the count of velocity- and pressure-type zones.
// A moving wall adds one count per mesh face (:722-723, a u16 that a release build wraps; not reproduced).
// Returns 0 PressureOnly, 1 VelocityOnly, 2 Hybrid, or ORC_ERR_NO_BOUNDARY_CONDITIONS as a negative number.
int check_boundary_conditions(const OrcMesh &m) {
    std::vector<int32_t> zt((size_t)m.n_zones);
    std::vector<double> zv((size_t)3 * m.n_zones);
    if (m.ztype.download(zt.data(), zt.size()) != ORC_OK || m.zvec.download(zv.data(), zv.size()) != ORC_OK) return -ORC_ERR_HIP;
    uint64_t pressure = 0, velocity = 0;
    for (int z = 0; z < m.n_zones; ++z) {
        const double *v = &zv[(size_t)3 * z];
        if (zt[z] == ORC_BC_WALL) {
            if (std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > 0.) velocity += (uint64_t)m.n_faces;
        } else if (zt[z] == ORC_BC_VELOCITY_INLET) {
            velocity += 1;
        } else if (zt[z] == ORC_BC_PRESSURE_INLET || zt[z] == ORC_BC_PRESSURE_OUTLET) {
            pressure += 1;
        }
    }
    if (velocity > 0) return pressure > 1 ? 2 : 1;
    if (pressure > 0) return 0;
    return -ORC_ERR_NO_BOUNDARY_CONDITIONS;  // "You must set boundary conditions."
}

// initialize_pressure_field (solver.rs:414-509): Laplace system in s.a_p / s.b_p, 10 Jacobi sweeps (omega 0.1,
// Jacobi-preconditioned) on s.p.
int initialize_pressure_field_dev(SolverState &s) {
    OrcMesh &m = *s.mesh;
    ORC_TRY(s.a_p.zero());
    hipLaunchKernelGGL(laplace_p_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), s.a_p.p, s.b_p.p, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    ORC_TRY(iterative_solve_dev(mesh_view(s, s.a_p.p), s.b_p.p, s.p.p, 10, ORC_SOLVER_JACOBI, 0.1, 1e-6, ORC_PRECOND_JACOBI, s.arena, &s.stats));
    return fetch_status(s);
}

// initialize_velocity_field (solver.rs:511-696): potential psi from ten Jacobi-preconditioned BiCGSTAB iterations on the
// psi system (assembled in s.a_p / s.b_p, solved into s.p_prime), then u, v, w = least-squares gradient of psi.
int initialize_velocity_field_dev(SolverState &s) {
    OrcMesh &m = *s.mesh;
    ORC_TRY(s.a_p.zero());
    hipLaunchKernelGGL(psi_system_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), s.a_p.p, s.b_p.p, s.dev_status.p);
    ORC_HIP(hipGetLastError());
    ORC_TRY(vec_fill(s.p_prime.p, 0., s.n));
    CtxDefaultsScope restore_defaults(ctx());
    ctx().breakdown_guard = s.settings.breakdown_guard != 0;
    ctx().reduction_order = s.settings.reduction_order;
    ORC_TRY(iterative_solve_dev(mesh_view(s, s.a_p.p), s.b_p.p, s.p_prime.p, 10, ORC_SOLVER_BICGSTAB, 0.1, 1e-6, ORC_PRECOND_JACOBI, s.arena, &s.stats));  // :595-604
    if (m.halo.active()) ORC_TRY(m.halo.exchange(s.p_prime.p));
    hipLaunchKernelGGL(psi_velocity_k, dim3(grid_for(s.n)), dim3(kBlock), 0, ctx().stream, m.dev(), s.p_prime.p, s.u.p, s.v.p, s.w.p);
    ORC_HIP(hipGetLastError());
    return fetch_status(s);
}

// the gradient pass solve_steady runs after its loop (solver.rs:227-242): the accumulated values are never used, but an
// unsupported scheme or a singular least-squares matrix still panics there
int post_loop_gradients_dev(SolverState &s) {
    ORC_TRY(exchange_fields(s));
    ORC_TRY(k_gradients(s, true));
    int st = fetch_status(s);
    if (s.mesh->halo.active()) st = comm_global_status(st);
    return st;
}

// initialize_flow (solver.rs:246-352).  `s` must have been set up with UD / LinearWeighted / LinearWeighted
// (:301-303) and zero fields; the blended matrix lives in s.a_p, which the pressure initialisation no longer needs.
int initialize_flow_dev(SolverState &s, uint64_t iteration_count) {
    const int kind = check_boundary_conditions(*s.mesh);  // :272 (result unused there, panics kept)
    if (kind < 0) return set_error(-kind, "You must set boundary conditions.");
    ORC_TRY(initialize_pressure_field_dev(s));  // :287
    ORC_TRY(exchange_fields(s));
    ORC_TRY(k_gradients(s, false));
    ORC_TRY(exchange_gradient(s, s.gp.p));
    ORC_TRY(k_face_flux(s, true));
    ORC_TRY(k_momentum(s, nullptr));  // :288-309 (b += b_di inside)
    CtxDefaultsScope restore_defaults(ctx());
    ctx().breakdown_guard = s.settings.breakdown_guard != 0;
    ctx().reduction_order = s.settings.reduction_order;
    const int64_t len = std::max<int64_t>(s.mesh->pat.padded, 1);
    double diffusion_fraction = 1.;
    while (diffusion_fraction >= 0.) {  // :316-349
        DevBuf<double> *mats[3] = {&s.a_u, &s.a_v, &s.a_w}, *rhs[3] = {&s.b_u, &s.b_v, &s.b_w}, *x[3] = {&s.u, &s.v, &s.w};
        for (int k = 0; k < 3; ++k) {
            hipLaunchKernelGGL(blend_k, dim3(grid_for(len)), dim3(kBlock), 0, ctx().stream, len, mats[k]->p, s.a_di.p, 1. - diffusion_fraction,
                               diffusion_fraction, s.a_p.p);
            ORC_HIP(hipGetLastError());
            ORC_TRY(iterative_solve_dev(mesh_view(s, s.a_p.p), rhs[k]->p, x[k]->p, iteration_count, ORC_SOLVER_BICGSTAB, 0.5, 1e-6,
                                        ORC_PRECOND_JACOBI, s.arena, &s.stats));
        }
        diffusion_fraction -= 0.2;
    }
    return fetch_status(s);
}

}  // namespace orc
