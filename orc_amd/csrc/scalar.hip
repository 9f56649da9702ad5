// scalar.hip — passive scalar transport on the solver's flow (new-build extension; ORC has no scalar equation).
//
//     rho dphi/dt + div(rho U phi) = div(Gamma grad phi) + S
//
// Finite volumes on the mesh pattern, mass flux F = rho A flux[f] with flux[f] the face_k<0> flux of the current u, v, w, p
// (k_scalar_face_flux, assembly.hip), written to the arm's own buffers.  Four passes on the library stream, fp64, no atomics:
//   scalar_diffusion_k  the Gamma matrix and the boundary D_b, D_b phi_b, q A terms (once per configuration)
//   scalar_grad_k       Green-Gauss grad phi, one thread per cell (TVD only)
//   scalar_face_k       per face: the deferred TVD correction c_f (one value per face: both cells see it, conservative to
//                       rounding) and the per-face boundary term of the boundary-flux report
//   scalar_k            one thread per row: Gamma part + UD / CD1 convection + both sides' c_f + source + time term
// DESIGN.md "Passive scalar transport" has the discretisation and the bytes of every pass.
// The system is symmetric only without convection (a flow at rest: the Gamma part alone, plus the time term on the diagonal):
// OrcScalarSettings.solver_type = ORC_SOLVER_CG is accepted for every configuration, and CG does not test symmetry (cg.hip).
#include <algorithm>
#include <cmath>

#include "assembly.hpp"
#include "cell_order.hpp"

namespace orc {
namespace {

struct P3 {
    double x, y, z;
};
__device__ __forceinline__ P3 p3(double x, double y, double z) { return {x, y, z}; }
__device__ __forceinline__ P3 psub(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double pdot(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double pnorm(P3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ P3 cc_of(const MeshDev &M, int c) { return p3(M.ccx[c], M.ccy[c], M.ccz[c]); }
__device__ __forceinline__ P3 fc_of(const MeshDev &M, int f) { return p3(M.fcx[f], M.fcy[f], M.fcz[f]); }

#define SC_GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

bool scheme_is_tvd(int scheme) { return scheme >= ORC_MOMENTUM_TVD_LUD && scheme <= ORC_MOMENTUM_TVD_CD1; }

}  // namespace

// ------------------------------------------------------------------ 1. the Gamma part (once per configuration)
// interior: D = Gamma A / |x_N - x_P| on the diagonal, -D off it; VALUE: D_b = Gamma A / |x_f - x_P| on the diagonal and
// D_b phi_b in b; FLUX: q A in b.  Sums over the cell's faces in ascending face id from 0.
__global__ void scalar_diffusion_k(MeshDev M, SellDev P, double gamma, const int32_t *__restrict__ zkind, const double *__restrict__ zval,
                                   double *__restrict__ a_g, double *__restrict__ b_g) {
    SC_GRID_STRIDE(c, M.n_own) {
        const P3 cc = cc_of(M, (int)c);
        double a_pp = 0., b = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int c1 = M.c1[f];
            if (c1 >= 0) {
                const int nb = M.c0[f] == c ? c1 : M.c0[f];
                const double d = gamma * M.area[f] / pnorm(psub(cc_of(M, nb), cc));
                a_g[M.cfpos[q]] = -d;
                a_pp += d;
            } else {
                const int z = M.fzone[f];
                const int k = zkind[z];
                if (k == ORC_SCALAR_BC_VALUE) {
                    const double d = gamma * M.area[f] / pnorm(psub(fc_of(M, f), cc));
                    a_pp += d;
                    b += d * zval[z];
                } else if (k == ORC_SCALAR_BC_FLUX) {
                    b += zval[z] * M.area[f];
                }
            }
        }
        a_g[P.diag_pos[c]] = a_pp;
        b_g[c] = b;
    }
}

// ------------------------------------------------------------------ 2. Green-Gauss grad phi (TVD)
// grad_P = (sum_f n_out (phi_f A)) / V; phi_f = (phi_P + phi_N) / 2 inside, phi_b on VALUE faces, phi_P elsewhere
__global__ void scalar_grad_k(MeshDev M, const double *__restrict__ phi, const int32_t *__restrict__ zkind, const double *__restrict__ zval,
                              double *__restrict__ grad) {
    const int64_t n = M.n_cells;
    SC_GRID_STRIDE(c, M.n_own) {
        const double pc = phi[c];
        double gx = 0., gy = 0., gz = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const bool side0 = M.c0[f] == c;
            const int c1 = M.c1[f];
            double pf;
            if (c1 >= 0) pf = (pc + phi[side0 ? c1 : M.c0[f]]) * 0.5;
            else {
                const int z = M.fzone[f];
                pf = zkind[z] == ORC_SCALAR_BC_VALUE ? zval[z] : pc;
            }
            const double s = pf * M.area[f];
            const double sx = M.nx[f] * s, sy = M.ny[f] * s, sz = M.nz[f] * s;
            if (side0) { gx += sx; gy += sy; gz += sz; }
            else { gx -= sx; gy -= sy; gz -= sz; }
        }
        const double vol = M.vol[c];
        grad[c] = gx / vol; grad[n + c] = gy / vol; grad[2 * n + c] = gz / vol;
    }
}

// ------------------------------------------------------------------ 3. per-face correction and boundary terms
// F = (flux A) rho seen from c0.  Interior (kTvd): upwind U = c0 if F > 0 else c1, d = x_D - x_U,
// r = 2 (grad_U . d) / (phi_D - phi_U) - 1, phi_f = phi_U + psi(r)/2 (phi_D - phi_U), c_f = F (phi_f - phi_U) (0 when
// phi_D == phi_U).  Boundary: the flux of phi INTO the domain through the face (VALUE: -F phi_b + D_b (phi_b - phi_P);
// FLUX: q A - F phi_P; ZERO_GRADIENT: -F phi_P); 0 on interior faces.
template <bool kTvd>
__global__ __launch_bounds__(kBlock) void scalar_face_k(MeshDev M, const double *__restrict__ flux, const double *__restrict__ phi,
                                                        const double *__restrict__ grad, const int32_t *__restrict__ zkind,
                                                        const double *__restrict__ zval, double gamma, double rho, int scheme,
                                                        double *__restrict__ corr, double *__restrict__ bterm) {
    const int64_t n = M.n_cells;
    SC_GRID_STRIDE(f, M.n_faces) {
        const int i = M.c0[f], j = M.c1[f];
        const double F = flux[f] * M.area[f] * rho;
        if (j >= 0) {
            bterm[f] = 0.;
            if (kTvd) {
                const int up = F > 0. ? i : j, dn = F > 0. ? j : i;
                const double pu = phi[up], dphi = phi[dn] - pu;
                double c = 0.;
                if (dphi != 0.) {
                    const P3 d = psub(cc_of(M, dn), cc_of(M, up));
                    const P3 g = p3(grad[up], grad[n + up], grad[2 * n + up]);
                    const double r = 2. * pdot(g, d) / dphi - 1.;
                    const double phi_f = pu + psi_eval(scheme, r) / 2. * dphi;
                    c = F * (phi_f - pu);
                }
                corr[f] = c;
            }
        } else {
            const int z = M.fzone[f];
            const int k = zkind[z];
            const double pc = phi[i];
            double t;
            if (k == ORC_SCALAR_BC_VALUE) {
                const double pb = zval[z];
                const double d = gamma * M.area[f] / pnorm(psub(fc_of(M, (int)f), cc_of(M, i)));
                t = -F * pb + d * (pb - pc);
            } else if (k == ORC_SCALAR_BC_FLUX) {
                t = zval[z] * M.area[f] - F * pc;
            } else {
                t = -F * pc;
            }
            bterm[f] = t;
        }
    }
}

// ------------------------------------------------------------------ 4. the rows
struct ScalarArgs {
    const double *flux, *corr, *a_g, *b_g, *src, *phi_n, *phi_nm1;
    const int32_t *zkind;
    const double *zval;
    double *a, *b;
    double rho, dt;
    int cd1, tvd, time;  // time: 0 none, 1 Euler, 2 BDF2
};

// One thread per row, the cell's faces in ascending face id, momentum_k's XCD-contiguous block walk: XCD g (workgroups g,
// g + 8, ...) assembles a contiguous eighth of the rows, so the two cells of a face mostly share one L2.
// a_PP = Gamma part + per face UD max(F, 0) or CD1 F/2 (boundary FLUX / ZERO_GRADIENT faces: F) + time term;
// a_PN = Gamma part + UD min(F, 0) or CD1 F/2; b = Gamma part, then per face -F phi_b (VALUE) and -/+ c_f, then S V, then
// the time term's level part.
__global__ __launch_bounds__(kBlock) void scalar_k(MeshDev M, SellDev P, ScalarArgs A) {
    const int64_t n_items = M.n_own;
    const int64_t n_blk = (n_items + blockDim.x - 1) / blockDim.x;
    int64_t vb = blockIdx.x, vb_end = n_blk, vb_step = gridDim.x;
    if ((gridDim.x & 7) == 0 && gridDim.x >= 8) {
        const int64_t per = (n_blk + 7) / 8;
        const int xcd = blockIdx.x & 7;
        vb = (int64_t)xcd * per + (blockIdx.x >> 3);
        vb_end = (int64_t)(xcd + 1) * per < n_blk ? (int64_t)(xcd + 1) * per : n_blk;
        vb_step = gridDim.x >> 3;
    }
    for (; vb < vb_end; vb += vb_step) {
        const int64_t c = vb * blockDim.x + threadIdx.x;
        if (c >= n_items) break;
        const int dpos = P.diag_pos[c];
        double a_pp = A.a_g[dpos], b = A.b_g[c];
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const bool side0 = M.c0[f] == c;
            const double F = (side0 ? A.flux[f] : -A.flux[f]) * M.area[f] * A.rho;
            if (M.c1[f] >= 0) {
                const int pos = M.cfpos[q];
                double ap, an;
                if (A.cd1) { ap = F / 2.; an = F / 2.; }
                else { ap = fmax(F, 0.); an = fmin(F, 0.); }
                a_pp += ap;
                A.a[pos] = A.a_g[pos] + an;
                if (A.tvd) b = side0 ? b - A.corr[f] : b + A.corr[f];
            } else {
                const int z = M.fzone[f];
                if (A.zkind[z] == ORC_SCALAR_BC_VALUE) b += -F * A.zval[z];
                else a_pp += F;
            }
        }
        if (A.src) b += A.src[c] * M.vol[c];
        if (A.time) {
            const double coef = (A.rho * M.vol[c]) / A.dt;
            if (A.time == 2) {
                a_pp += 1.5 * coef;
                b += coef * (2.0 * A.phi_n[c] - 0.5 * A.phi_nm1[c]);
            } else {
                a_pp += coef;
                b += coef * A.phi_n[c];
            }
        }
        A.a[dpos] = a_pp;
        A.b[c] = b;
    }
}

// ------------------------------------------------------------------ reductions of the report (fixed association, no atomics)
// partials: [0] sum (phi - phi_old)^2, [1] sum phi^2, [2] min phi, [3] max phi per workgroup over the owned cells
__global__ __launch_bounds__(kBlock) void scalar_stats_k(int64_t n_own, const double *__restrict__ phi, const double *__restrict__ old,
                                                         double *__restrict__ partials) {
    __shared__ double lds[8];
    double d2 = 0., p2 = 0., mn = INFINITY, mx = -INFINITY;
    SC_GRID_STRIDE(c, n_own) {
        const double x = phi[c], d = x - old[c];
        d2 += d * d;
        p2 += x * x;
        mn = fmin(mn, x);
        mx = fmax(mx, x);
    }
    const double t0 = block_sum(d2, lds), t1 = block_sum(p2, lds);
    const double t2 = -block_max(-mn, lds), t3 = block_max(mx, lds);
    if (threadIdx.x == 0) {
        const int g = gridDim.x;
        partials[blockIdx.x] = t0; partials[g + blockIdx.x] = t1; partials[2 * g + blockIdx.x] = t2; partials[3 * g + blockIdx.x] = t3;
    }
}

// out[0], out[1] = sums, out[2] = -min, out[3] = max (negated min: one all-reduce max covers both on a partitioned mesh)
__global__ void scalar_stats_fold_k(const double *__restrict__ partials, int count, double *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s0 = 0., s1 = 0., mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < count; ++i) {
        s0 += partials[i]; s1 += partials[count + i];
        mn = fmin(mn, partials[2 * count + i]); mx = fmax(mx, partials[3 * count + i]);
    }
    out[0] = s0; out[1] = s1; out[2] = -mn; out[3] = mx;
}

// per zone (one workgroup each): the sum of the boundary terms of the faces of owned cells in that zone
__global__ __launch_bounds__(kBlock) void scalar_zone_sum_k(MeshDev M, const double *__restrict__ bterm, double *__restrict__ out) {
    __shared__ double lds[8];
    const int z = blockIdx.x;
    double s = 0.;
    for (int64_t f = threadIdx.x; f < M.n_faces; f += blockDim.x)
        if (M.c1[f] < 0 && M.fzone[f] == z && M.c0[f] < M.n_own) s += bterm[f];
    const double t = block_sum(s, lds);
    if (threadIdx.x == 0) out[z] = t;
}

// ====================================================================== host side
namespace {

using Scalar = SolverState::Scalar;

int resolve_bcs(SolverState &s, std::vector<int32_t> &kind, std::vector<double> &value) {
    const OrcMesh &m = *s.mesh;
    std::vector<int32_t> zt((size_t)m.n_zones);
    if (m.n_zones) ORC_TRY(m.ztype.download(zt.data(), zt.size()));
    kind = s.sc.kind;
    value = s.sc.value;
    for (size_t z = 0; z < zt.size(); ++z) {
        if (kind[z] != ORC_SCALAR_BC_DEFAULT) continue;
        value[z] = 0.;
        switch (zt[z]) {
        case ORC_BC_WALL:
        case ORC_BC_SYMMETRY: kind[z] = ORC_SCALAR_BC_FLUX; break;
        case ORC_BC_VELOCITY_INLET:
        case ORC_BC_PRESSURE_INLET: kind[z] = ORC_SCALAR_BC_VALUE; break;
        default: kind[z] = ORC_SCALAR_BC_ZERO_GRADIENT; break;  // PressureOutlet (interior zones carry no boundary face)
        }
    }
    return ORC_OK;
}

// the zone table and the Gamma part, rebuilt when the arm or a boundary condition (or a DEFAULT's zone type) changed
int ensure_configured(SolverState &s) {
    Scalar &c = s.sc;
    std::vector<int32_t> kind;
    std::vector<double> value;
    ORC_TRY(resolve_bcs(s, kind, value));
    if (kind == c.resolved_kind && value == c.resolved_value) return ORC_OK;
    OrcMesh &m = *s.mesh;
    ORC_TRY(c.zkind.upload(kind.data(), kind.size()));
    ORC_TRY(c.zval.upload(value.data(), value.size()));
    ORC_TRY(c.a_g.zero());
    hipLaunchKernelGGL(scalar_diffusion_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), c.c.diffusivity,
                       c.zkind.p, c.zval.p, c.a_g.p, c.b_g.p);
    ORC_HIP(hipGetLastError());
    c.resolved_kind = kind;
    c.resolved_value = value;
    return ORC_OK;
}

int ready(SolverState &s) {
    if (!s.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    if (s.settings.velocity_interpolation == ORC_VINTERP_RHIE_CHOW && !s.diagonals_assembled)
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: Rhie-Chow face fluxes need the momentum diagonals, which have never been assembled "
                                               "(run orc_solver_iterate or orc_solver_assemble_momentum first)");
    return ORC_OK;
}

// the face pass (TVD: gradient and correction; always: the boundary terms) on the current phi and the arm's flux
int face_pass(SolverState &s, bool tvd) {
    Scalar &c = s.sc;
    OrcMesh &m = *s.mesh;
    HaloPlan &H = m.halo;
    const int64_t n = s.n;
    if (H.active()) ORC_TRY(H.exchange(c.phi.p));
    if (tvd) {
        hipLaunchKernelGGL(scalar_grad_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), c.phi.p, c.zkind.p, c.zval.p, c.grad.p);
        ORC_HIP(hipGetLastError());
        if (H.active()) { double *g3[3] = {c.grad.p, c.grad.p + n, c.grad.p + 2 * n}; ORC_TRY(H.exchange(g3, 3)); }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_k<true>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(), c.flux.p,
                           c.phi.p, c.grad.p, c.zkind.p, c.zval.p, c.c.diffusivity, s.rho, c.c.scheme, c.corr.p, c.bterm.p);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_k<false>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(), c.flux.p,
                           c.phi.p, c.grad.p, c.zkind.p, c.zval.p, c.c.diffusivity, s.rho, c.c.scheme, c.corr.p, c.bterm.p);
    }
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int assemble(SolverState &s) {
    Scalar &c = s.sc;
    OrcMesh &m = *s.mesh;
    const bool tvd = scheme_is_tvd(c.c.scheme);
    if (tvd) ORC_TRY(face_pass(s, true));
    ScalarArgs A{};
    A.flux = c.flux.p; A.corr = c.corr.p; A.a_g = c.a_g.p; A.b_g = c.b_g.p;
    A.src = c.has_source ? c.src.p : nullptr;
    A.phi_n = c.lev[0].p; A.phi_nm1 = c.lev[1].p;
    A.zkind = c.zkind.p; A.zval = c.zval.p;
    A.a = c.a.p; A.b = c.b.p;
    A.rho = s.rho; A.dt = s.tr.dt;
    A.cd1 = c.c.scheme == ORC_MOMENTUM_CD1;
    A.tvd = tvd;
    A.time = (s.transient && c.levels > 0) ? ((s.tr.scheme == ORC_TIME_BDF2 && c.levels >= 2) ? 2 : 1) : 0;
    hipLaunchKernelGGL(scalar_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), A);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// (|phi - phi_old|^2, |phi|^2, min, max) over the whole mesh, to the host
int stats(SolverState &s, double out[4]) {
    Scalar &c = s.sc;
    const int g = grid_for(s.n_own);
    hipLaunchKernelGGL(scalar_stats_k, dim3(g), dim3(kBlock), 0, ctx().stream, s.n_own, c.phi.p, c.phi_old.p, c.partials.p);
    hipLaunchKernelGGL(scalar_stats_fold_k, dim3(1), dim3(64), 0, ctx().stream, c.partials.p, g, c.scal.p);
    ORC_HIP(hipGetLastError());
    if (s.mesh->halo.active()) {
        ORC_TRY(comm_allreduce_sum(c.scal.p, 2));
        ORC_TRY(comm_allreduce_max(c.scal.p + 2, 2));
    }
    ORC_HIP(hipMemcpyAsync(out, c.scal.p, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    out[2] = -out[2];
    return ORC_OK;
}

int solve(SolverState &s, double report[4]) {
    ORC_TRY(ready(s));
    Scalar &c = s.sc;
    ORC_TRY(ensure_configured(s));
    ORC_TRY(k_scalar_face_flux(s));
    OrcSettings t = s.settings;  // the flow's guard, reduction order and GMRES restart with the scalar's solver fields
    t.solver_type = c.c.solver_type;
    t.preconditioner = c.c.preconditioner;
    t.iterations = c.c.iterations;
    t.relative_convergence_threshold = c.c.relative_convergence_threshold;
    t.relaxation = c.c.relaxation;
    const bool tvd = scheme_is_tvd(c.c.scheme);
    const uint64_t rounds = tvd ? c.c.outer_iterations : 1;
    double rep[4] = {0., 0., 0., 0.};
    int st = ORC_OK;
    for (uint64_t k = 0; k < rounds; ++k) {
        ORC_TRY(assemble(s));
        ORC_TRY(vec_copy(c.phi_old.p, c.phi.p, s.n));
        st = solve_scalar_system(s, t);  // a partitioned solve leaves with the same verdict on every rank
        if (st != ORC_OK) break;
        double r[4];
        ORC_TRY(stats(s, r));
        const double dn = std::sqrt(r[0]), pn = std::sqrt(r[1]);
        rep[0] = (double)(k + 1);
        rep[1] = pn > 0. ? dn / pn : (dn > 0. ? INFINITY : 0.);
        rep[2] = r[2];
        rep[3] = r[3];
        if (std::isnan(r[0]) || std::isnan(r[1])) { st = set_error(ORC_ERR_SOLUTION_DIVERGED, "scalar: solution diverged"); break; }
        if (dn <= c.c.outer_tolerance * pn) break;
    }
    int h = fetch_status(s);
    if (s.mesh->halo.active()) h = comm_global_status(h);
    if (st == ORC_OK) st = h;
    std::copy(rep, rep + 4, c.report);
    if (report) std::copy(rep, rep + 4, report);
    return st;
}

int validate(const OrcScalarSettings &c) {
    if (!(c.diffusivity > 0.) || !std::isfinite(c.diffusivity)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: diffusivity must be positive and finite");
    if (!(c.scheme == ORC_MOMENTUM_UD || c.scheme == ORC_MOMENTUM_CD1 || scheme_is_tvd(c.scheme)))
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "scalar: unsupported scheme %d", c.scheme);
    const int m = c.solver_type;
    if (!(m == ORC_SOLVER_JACOBI || m == ORC_SOLVER_MULTIGRID || m == ORC_SOLVER_BICGSTAB || m == ORC_SOLVER_MULTICOLOR_GS ||
          m == ORC_SOLVER_BICGSTAB_GS_PRECOND || m == ORC_SOLVER_MULTIGRID_GS || m == ORC_SOLVER_GMRES || m == ORC_SOLVER_CG))
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: unknown solver type %d", m);
    if (c.preconditioner != ORC_PRECOND_NONE && c.preconditioner != ORC_PRECOND_JACOBI)
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: unknown preconditioner %d", c.preconditioner);
    if (c.reserved0 != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: reserved0 must be 0");
    if (c.iterations == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: iterations must be at least 1");
    if (!(c.relative_convergence_threshold >= 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: relative_convergence_threshold must be >= 0");
    if (!std::isfinite(c.relaxation)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: relaxation must be finite");
    if (c.outer_iterations == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: outer_iterations must be at least 1");
    if (!(c.outer_tolerance >= 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: outer_tolerance must be >= 0");
    return ORC_OK;
}

}  // namespace

int scalar_step_dev(SolverState &s) {
    Scalar &c = s.sc;
    if (!c.on) return ORC_OK;
    if (c.levels >= 1) ORC_TRY(vec_copy(c.lev[1].p, c.lev[0].p, s.n));
    ORC_TRY(vec_copy(c.lev[0].p, c.phi.p, s.n));
    c.levels = std::min(c.levels + 1, 2);
    return solve(s, nullptr);
}

}  // namespace orc

using namespace orc;

extern "C" {

void orc_scalar_settings_default(OrcScalarSettings *c) {
    if (!c) return;
    *c = OrcScalarSettings{};
    c->diffusivity = 1e-3;
    c->scheme = ORC_MOMENTUM_UD;
    c->solver_type = ORC_SOLVER_BICGSTAB;
    c->preconditioner = ORC_PRECOND_JACOBI;
    c->reserved0 = 0;
    c->iterations = 500;
    c->relative_convergence_threshold = 1e-10;
    c->relaxation = 0.5;
    c->outer_iterations = 30;
    c->outer_tolerance = 1e-8;
}

int orc_solver_set_scalar(OrcSolver *s, const OrcScalarSettings *cfg_in) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!cfg_in) {
        if (st.ts.on && (st.ts.c.groups & ORC_STAT_GROUP_SCALAR))
            return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the time statistics' SCALAR group is on (orc_solver_set_time_statistics)");
        st.sc = SolverState::Scalar();
        return ORC_OK;
    }
    ORC_TRY(validate(*cfg_in));
    Scalar fresh;
    const size_t n = (size_t)std::max<int64_t>(st.n, 1), F = (size_t)std::max<int64_t>(st.mesh->n_faces, 1);
    const size_t pad = (size_t)std::max<int64_t>(st.mesh->pat.padded, 1), Z = (size_t)std::max<int32_t>(st.mesh->n_zones, 1);
    DevBuf<double> *nvec[] = {&fresh.phi, &fresh.phi_old, &fresh.lev[0], &fresh.lev[1], &fresh.src, &fresh.b, &fresh.b_g};
    for (auto *b : nvec) { ORC_TRY(b->alloc(n)); ORC_TRY(b->zero()); }
    ORC_TRY(fresh.a.alloc(pad)); ORC_TRY(fresh.a.zero());
    ORC_TRY(fresh.a_g.alloc(pad)); ORC_TRY(fresh.a_g.zero());
    ORC_TRY(fresh.grad.alloc(3 * n)); ORC_TRY(fresh.grad.zero());
    ORC_TRY(fresh.gp.alloc(3 * n));
    DevBuf<double> *fvec[] = {&fresh.flux, &fresh.pf, &fresh.corr, &fresh.bterm};
    for (auto *b : fvec) { ORC_TRY(b->alloc(F)); ORC_TRY(b->zero()); }
    ORC_TRY(fresh.zkind.alloc(Z));
    ORC_TRY(fresh.zval.alloc(Z));
    ORC_TRY(fresh.partials.alloc((size_t)4 * kMaxPartials));
    ORC_TRY(fresh.scal.alloc(8));
    fresh.c = *cfg_in;
    fresh.kind.assign((size_t)st.mesh->n_zones, ORC_SCALAR_BC_DEFAULT);
    fresh.value.assign((size_t)st.mesh->n_zones, 0.);
    fresh.on = true;
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    st.sc = std::move(fresh);
    return ORC_OK;
}

int orc_solver_set_scalar_bc(OrcSolver *s, int32_t zone, int32_t kind, double value) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    if (zone < 0 || zone >= st.mesh->n_zones) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: zone %d out of range", zone);
    if (kind < ORC_SCALAR_BC_DEFAULT || kind > ORC_SCALAR_BC_ZERO_GRADIENT) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: unknown condition %d", kind);
    if (!std::isfinite(value)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: condition value must be finite");
    std::vector<int32_t> zt((size_t)st.mesh->n_zones);
    ORC_TRY(st.mesh->ztype.download(zt.data(), zt.size()));
    if (zt[(size_t)zone] == ORC_BC_INTERIOR) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: zone %d is an interior zone", zone);
    st.sc.kind[(size_t)zone] = kind;
    st.sc.value[(size_t)zone] = kind == ORC_SCALAR_BC_ZERO_GRADIENT || kind == ORC_SCALAR_BC_DEFAULT ? 0. : value;
    return ORC_OK;
}

int orc_solver_set_scalar_field(OrcSolver *s, const double *phi) {
    if (!s || !phi) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    if (!s->st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    return upload_cells(*s->st.mesh, phi, s->st.sc.phi);
}

int orc_solver_get_scalar_field(OrcSolver *s, double *phi) {
    if (!s || !phi) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    return download_cells(*st.mesh, st.sc.phi.p, phi);
}

int orc_solver_set_scalar_source(OrcSolver *s, const double *source) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    if (!source) { st.sc.has_source = false; return ORC_OK; }
    ORC_TRY(upload_cells(*st.mesh, source, st.sc.src));
    st.sc.has_source = true;
    return ORC_OK;
}

int orc_solver_set_scalar_levels(OrcSolver *s, const double *phi_n, const double *phi_nm1) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    if (!st.transient) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar levels without orc_solver_set_transient");
    if (!phi_n) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: level n must be given");
    ORC_TRY(upload_cells(*st.mesh, phi_n, st.sc.lev[0]));
    if (phi_nm1) ORC_TRY(upload_cells(*st.mesh, phi_nm1, st.sc.lev[1]));
    st.sc.levels = phi_nm1 ? 2 : 1;
    return ORC_OK;
}

int orc_solver_solve_scalar(OrcSolver *s, double report[4]) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    return solve(s->st, report);
}

int orc_solver_last_scalar_report(OrcSolver *s, double report[4]) {
    if (!s || !report) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    if (!s->st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    std::copy(s->st.sc.report, s->st.sc.report + 4, report);
    return ORC_OK;
}

int orc_solver_assemble_scalar(OrcSolver *s, double *a, double *b) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(ready(st));
    ORC_TRY(ensure_configured(st));
    ORC_TRY(k_scalar_face_flux(st));
    ORC_TRY(assemble(st));
    OrcMesh &m = *st.mesh;
    if (a) {
        DevBuf<double> tmp;
        ORC_TRY(tmp.ensure((size_t)std::max<int64_t>(m.pat.nnz, 1)));
        ORC_TRY(sell_export_values(m.pat, st.sc.a.p, tmp.p));
        ORC_TRY(tmp.download(a, (size_t)m.pat.nnz));
    }
    if (b) ORC_TRY(st.sc.b.download(b, (size_t)st.n_own));
    int h = fetch_status(st);
    if (m.halo.active()) h = comm_global_status(h);
    return h;
}

int orc_solver_scalar_boundary_flux(OrcSolver *s, double *per_zone) {
    if (!s || !per_zone) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    SolverState &st = s->st;
    ORC_TRY(ready(st));
    ORC_TRY(ensure_configured(st));
    ORC_TRY(k_scalar_face_flux(st));
    ORC_TRY(face_pass(st, false));
    OrcMesh &m = *st.mesh;
    const int Z = m.n_zones;
    if (Z > 0) {
        DevBuf<double> out;
        ORC_TRY(out.alloc((size_t)Z));
        hipLaunchKernelGGL(scalar_zone_sum_k, dim3(Z), dim3(kBlock), 0, ctx().stream, m.dev(), st.sc.bterm.p, out.p);
        ORC_HIP(hipGetLastError());
        if (m.halo.active()) ORC_TRY(comm_allreduce_sum(out.p, Z));
        ORC_TRY(out.download(per_zone, (size_t)Z));
    }
    int h = fetch_status(st);
    if (m.halo.active()) h = comm_global_status(h);
    return h;
}

}  // extern "C"
