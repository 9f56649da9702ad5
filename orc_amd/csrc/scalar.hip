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
// Variable diffusivity (orc_solver_set_scalar_diffusivity; DESIGN.md §3 "Variable scalar diffusivity"), opt-in: while a model is on,
//   scalar_diffusion_var_k  replaces scalar_diffusion_k: the same loop with Gamma evaluated on the fly for the cell and for the
//                           neighbour of every interior face (one more gather per interior face), the face value by face_viscosity
//   scalar_face_var_k       scalar_face_k's body with the cell's Gamma in the boundary term
//   scalar_gamma_k          Gamma per cell, for orc_solver_get_scalar_diffusivity only
// scalar_k reads the Gamma part from a_g, b_g and never sees Gamma.
// The system is symmetric only without convection (a flow at rest: the Gamma part alone, plus the time term on the diagonal):
// OrcScalarSettings.solver_type = ORC_SOLVER_CG is accepted for every configuration, and CG does not test symmetry (cg.hip).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "var_diffusion.hpp"

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

// the constant Gamma of the arm without a diffusivity model
struct GammaConst {
    double gamma;
    __device__ __forceinline__ double operator()(int) const { return gamma; }
};

// Gamma of cell c under a diffusivity model, THE operator order of DESIGN §3 "Variable scalar diffusivity".  x: what the law reads per
// cell (FIELD: the field as set; EDDY: the viscosity field of the last momentum assembly; LINEAR: phi), ghost entries current.  The
// model is the same in every lane.
struct GammaLaw {
    const double *x;
    int model, harmonic;
    double gamma0, mu_lam, schmidt_t, beta, phi_ref, gamma_min, gamma_max;
    __device__ __forceinline__ double operator()(int c) const {
        const double v = x[c];
        if (model == ORC_SCALAR_GAMMA_FIELD) return v;
        double g;
        if (model == ORC_SCALAR_GAMMA_EDDY) g = gamma0 + fmax(v - mu_lam, 0.) / schmidt_t;
        else g = gamma0 * (1. + beta * (v - phi_ref));  // LINEAR
        return fmin(fmax(g, gamma_min), gamma_max);
    }
};

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

// scalar_diffusion_k's loop — the same branches, the same accumulation order of a_pp and b — with Gamma replaced by the face value of
// (Gamma_P, Gamma_N) on interior faces and by Gamma_P on VALUE faces.  One thread per owned row, diffusion_var_k's block walk.
__global__ __launch_bounds__(kBlock) void scalar_diffusion_var_k(MeshDev M, SellDev P, GammaLaw G, const int32_t *__restrict__ zkind,
                                                                 const double *__restrict__ zval, double *__restrict__ a_g,
                                                                 double *__restrict__ b_g) {
    const int n_items = (int)M.n_own;  // cell ids are int32 (MeshDev.c0)
    for (BlockWalk W = block_walk(n_items); W.vb < W.vb_end; W.vb += W.vb_step) {
        const int c = W.vb * kBlock + (int)threadIdx.x;
        if (c >= n_items) break;
        const P3 cc = cc_of(M, c);
        const double g_p = G(c);
        double a_pp = 0., b = 0.;
        for (int q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
            const int f = M.cf[q];
            const int c1 = M.c1[f];
            if (c1 >= 0) {
                const int nb = M.c0[f] == c ? c1 : M.c0[f];
                const double d = face_viscosity(G.harmonic, g_p, G(nb)) * M.area[f] / pnorm(psub(cc_of(M, nb), cc));
                a_g[M.cfpos[q]] = -d;
                a_pp += d;
            } else {
                const int z = M.fzone[f];
                const int k = zkind[z];
                if (k == ORC_SCALAR_BC_VALUE) {
                    const double d = g_p * M.area[f] / pnorm(psub(fc_of(M, f), cc));
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

// Gamma per cell (ghost cells included), for orc_solver_get_scalar_diffusivity only: nothing on the solve path reads it
__global__ void scalar_gamma_k(int64_t n_cells, GammaLaw G, double *__restrict__ gamma) {
    SC_GRID_STRIDE(c, n_cells) gamma[c] = G((int)c);
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
// gamma_of(cell): the diffusivity a boundary VALUE face takes from its cell (GammaConst or GammaLaw).
template <bool kTvd, class GammaOf>
__device__ __forceinline__ void scalar_face_body(const MeshDev &M, const double *__restrict__ flux, const double *__restrict__ phi,
                                                 const double *__restrict__ grad, const int32_t *__restrict__ zkind,
                                                 const double *__restrict__ zval, const GammaOf &gamma_of, double rho, int scheme,
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
                const double d = gamma_of(i) * M.area[f] / pnorm(psub(fc_of(M, (int)f), cc_of(M, i)));
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

template <bool kTvd>
__global__ __launch_bounds__(kBlock) void scalar_face_k(MeshDev M, const double *__restrict__ flux, const double *__restrict__ phi,
                                                        const double *__restrict__ grad, const int32_t *__restrict__ zkind,
                                                        const double *__restrict__ zval, double gamma, double rho, int scheme,
                                                        double *__restrict__ corr, double *__restrict__ bterm) {
    scalar_face_body<kTvd>(M, flux, phi, grad, zkind, zval, GammaConst{gamma}, rho, scheme, corr, bterm);
}

// the further instantiation of a diffusivity model: the boundary term with the cell's Gamma, so that the boundary-flux report and the
// conservation identity hold with variable Gamma
template <bool kTvd>
__global__ __launch_bounds__(kBlock) void scalar_face_var_k(MeshDev M, const double *__restrict__ flux, const double *__restrict__ phi,
                                                            const double *__restrict__ grad, const int32_t *__restrict__ zkind,
                                                            const double *__restrict__ zval, GammaLaw G, double rho, int scheme,
                                                            double *__restrict__ corr, double *__restrict__ bterm) {
    scalar_face_body<kTvd>(M, flux, phi, grad, zkind, zval, G, rho, scheme, corr, bterm);
}

// ------------------------------------------------------------------ 4. the rows
struct ScalarArgs {
    const double *flux, *corr, *a_g, *b_g, *src, *phi_n, *phi_nm1;
    const int32_t *zkind;
    const double *zval;
    double *a, *b;
    double rho, dt, a0, a1, a2;
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
                a_pp += A.a0 * coef;  // the variable-step coefficients of time_term_k: 1.5, 2, 0.5 exactly for a fixed step
                b += coef * (A.a1 * A.phi_n[c] - A.a2 * A.phi_nm1[c]);
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

int gamma_model(const SolverState &s) { return s.sc.gd.on ? s.sc.gd.c.model : ORC_SCALAR_GAMMA_CONSTANT; }

// the law of the model that is on, reading the solver's current state
GammaLaw gamma_law(SolverState &s) {
    const Scalar &c = s.sc;
    const OrcScalarDiffusivity &d = c.gd.c;
    GammaLaw G{};
    G.model = d.model;
    G.x = d.model == ORC_SCALAR_GAMMA_FIELD ? c.gd.field.p : d.model == ORC_SCALAR_GAMMA_EDDY ? s.vis.mu.p : c.phi.p;
    G.harmonic = d.face_interpolation == ORC_VISCOSITY_FACE_HARMONIC ? 1 : 0;
    G.gamma0 = c.c.diffusivity; G.mu_lam = s.mu; G.schmidt_t = d.schmidt_t; G.beta = d.beta; G.phi_ref = d.phi_ref;
    G.gamma_min = d.gamma_min; G.gamma_max = d.gamma_max;
    return G;
}

// a_g and b_g of the resolved zone table: scalar_diffusion_k, or scalar_diffusion_var_k while a diffusivity model is on (LINEAR reads phi,
// whose ghosts the caller has exchanged)
int build_gamma_part(SolverState &s, double *a_g, double *b_g) {
    Scalar &c = s.sc;
    OrcMesh &m = *s.mesh;
    if (gamma_model(s) == ORC_SCALAR_GAMMA_CONSTANT)
        hipLaunchKernelGGL(scalar_diffusion_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), c.c.diffusivity,
                           c.zkind.p, c.zval.p, a_g, b_g);
    else
        hipLaunchKernelGGL(scalar_diffusion_var_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), gamma_law(s),
                           c.zkind.p, c.zval.p, a_g, b_g);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// The zone table and the Gamma part, rebuilt when the arm or a boundary condition (or a DEFAULT's zone type) changed, or the diffusivity
// model or its field.  for_system (a solve or an assembly begins): EDDY rebuilds every time, from the viscosity field of the last
// momentum assembly; LINEAR leaves the Gamma part to assemble(), which rebuilds it from the current phi every time.
int ensure_configured(SolverState &s, bool for_system) {
    Scalar &c = s.sc;
    std::vector<int32_t> kind;
    std::vector<double> value;
    ORC_TRY(resolve_bcs(s, kind, value));
    const bool same_table = kind == c.resolved_kind && value == c.resolved_value;
    const int model = gamma_model(s);
    if (same_table && !c.gd.stale && !(for_system && model == ORC_SCALAR_GAMMA_EDDY)) return ORC_OK;
    if (!same_table) {
        ORC_TRY(c.zkind.upload(kind.data(), kind.size()));
        ORC_TRY(c.zval.upload(value.data(), value.size()));
    }
    if (model != ORC_SCALAR_GAMMA_LINEAR) {
        ORC_TRY(c.a_g.zero());
        ORC_TRY(build_gamma_part(s, c.a_g.p, c.b_g.p));
        c.gd.stale = false;
    }
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
// bterm: where the boundary terms go (the arm's buffer, or the bench hook's scratch)
int face_pass(SolverState &s, bool tvd, double *bterm) {
    Scalar &c = s.sc;
    OrcMesh &m = *s.mesh;
    HaloPlan &H = m.halo;
    const int64_t n = s.n;
    const bool var = gamma_model(s) != ORC_SCALAR_GAMMA_CONSTANT;
    if (H.active()) ORC_TRY(H.exchange(c.phi.p));
    if (tvd) {
        hipLaunchKernelGGL(scalar_grad_k, dim3(grid_for(s.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), c.phi.p, c.zkind.p, c.zval.p, c.grad.p);
        ORC_HIP(hipGetLastError());
        if (H.active()) { double *g3[3] = {c.grad.p, c.grad.p + n, c.grad.p + 2 * n}; ORC_TRY(H.exchange(g3, 3)); }
        if (var)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_var_k<true>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(),
                               c.flux.p, c.phi.p, c.grad.p, c.zkind.p, c.zval.p, gamma_law(s), s.rho, c.c.scheme, c.corr.p, bterm);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_k<true>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(), c.flux.p,
                               c.phi.p, c.grad.p, c.zkind.p, c.zval.p, c.c.diffusivity, s.rho, c.c.scheme, c.corr.p, bterm);
    } else if (var) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_var_k<false>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(),
                           c.flux.p, c.phi.p, c.grad.p, c.zkind.p, c.zval.p, gamma_law(s), s.rho, c.c.scheme, c.corr.p, bterm);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_k<false>), dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, m.dev(), c.flux.p,
                           c.phi.p, c.grad.p, c.zkind.p, c.zval.p, c.c.diffusivity, s.rho, c.c.scheme, c.corr.p, bterm);
    }
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int assemble(SolverState &s) {
    Scalar &c = s.sc;
    OrcMesh &m = *s.mesh;
    const bool tvd = scheme_is_tvd(c.c.scheme);
    if (gamma_model(s) == ORC_SCALAR_GAMMA_LINEAR) {  // Gamma(phi): the Gamma part of this round's phi
        if (m.halo.active()) ORC_TRY(m.halo.exchange(c.phi.p));
        ORC_TRY(c.a_g.zero());
        ORC_TRY(build_gamma_part(s, c.a_g.p, c.b_g.p));
    }
    if (tvd) ORC_TRY(face_pass(s, true, c.bterm.p));
    ScalarArgs A{};
    A.flux = c.flux.p; A.corr = c.corr.p; A.a_g = c.a_g.p; A.b_g = c.b_g.p;
    A.src = c.has_source ? c.src.p : nullptr;
    A.phi_n = c.lev[0].p; A.phi_nm1 = c.lev[1].p;
    A.zkind = c.zkind.p; A.zval = c.zval.p;
    A.a = c.a.p; A.b = c.b.p;
    A.rho = s.rho; A.dt = s.dt;
    { const SolverState::TimeCoef k = s.time_coef(); A.a0 = k.a0; A.a1 = k.a1; A.a2 = k.a2; }
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
    ORC_TRY(ensure_configured(s, true));
    ORC_TRY(k_scalar_face_flux(s));
    OrcSettings t = s.settings;  // the flow's guard, reduction order and GMRES restart with the scalar's solver fields
    t.solver_type = c.c.solver_type;
    t.preconditioner = c.c.preconditioner;
    t.iterations = c.c.iterations;
    t.relative_convergence_threshold = c.c.relative_convergence_threshold;
    t.relaxation = c.c.relaxation;
    const bool tvd = scheme_is_tvd(c.c.scheme);
    // the outer (Picard) loop: the TVD correction and a Gamma that depends on phi share its rounds
    const uint64_t rounds = tvd || gamma_model(s) == ORC_SCALAR_GAMMA_LINEAR ? c.c.outer_iterations : 1;
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

int validate(const OrcScalarDiffusivity &c) {
    if (c.model < ORC_SCALAR_GAMMA_CONSTANT || c.model > ORC_SCALAR_GAMMA_LINEAR)
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: unknown model %d", c.model);
    if (c.face_interpolation != ORC_VISCOSITY_FACE_ARITHMETIC && c.face_interpolation != ORC_VISCOSITY_FACE_HARMONIC)
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: unknown face interpolation %d", c.face_interpolation);
    for (double x : {c.schmidt_t, c.beta, c.phi_ref, c.gamma_min, c.gamma_max, c.reserved0})
        if (!std::isfinite(x)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: every parameter must be finite");
    if (!(c.schmidt_t > 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: schmidt_t must be > 0");
    if (!(c.gamma_min > 0.) || !(c.gamma_min <= c.gamma_max))
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: the clamp needs 0 < gamma_min <= gamma_max < inf");
    if (c.reserved0 != 0.) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: reserved0 must be 0");
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
    ORC_TRY(ensure_configured(st, true));
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
    ORC_TRY(ensure_configured(st, false));
    ORC_TRY(k_scalar_face_flux(st));
    ORC_TRY(face_pass(st, false, st.sc.bterm.p));
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

// ------------------------------------------------------------------ variable diffusivity
static_assert(sizeof(OrcScalarDiffusivity) == 56 && offsetof(OrcScalarDiffusivity, model) == 0 &&
                  offsetof(OrcScalarDiffusivity, face_interpolation) == 4 && offsetof(OrcScalarDiffusivity, schmidt_t) == 8 &&
                  offsetof(OrcScalarDiffusivity, beta) == 16 && offsetof(OrcScalarDiffusivity, phi_ref) == 24 &&
                  offsetof(OrcScalarDiffusivity, gamma_min) == 32 && offsetof(OrcScalarDiffusivity, gamma_max) == 40 &&
                  offsetof(OrcScalarDiffusivity, reserved0) == 48,
              "OrcScalarDiffusivity is part of the ABI (orc_amd/settings.py ScalarDiffusivity mirrors it)");

void orc_scalar_diffusivity_default(OrcScalarDiffusivity *c) {
    if (!c) return;
    *c = OrcScalarDiffusivity{};
    c->model = ORC_SCALAR_GAMMA_CONSTANT;
    c->face_interpolation = ORC_VISCOSITY_FACE_ARITHMETIC;
    c->schmidt_t = 0.7;
    c->beta = 0.; c->phi_ref = 0.;
    c->gamma_min = 1e-12; c->gamma_max = 1e12;
    c->reserved0 = 0.;
}

int orc_solver_set_scalar_diffusivity(OrcSolver *s, const OrcScalarDiffusivity *c) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    Scalar::Diffusivity &D = st.sc.gd;
    if (c) ORC_TRY(validate(*c));
    if (!c || c->model == ORC_SCALAR_GAMMA_CONSTANT) {  // back to the constant: scalar_diffusion_k's Gamma part at the next use
        if (D.on) D.stale = true;
        D.on = false;
        return ORC_OK;
    }
    if (c->model == ORC_SCALAR_GAMMA_FIELD && !D.has_field)
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: the FIELD model needs orc_solver_set_scalar_diffusivity_field first");
    if (c->model == ORC_SCALAR_GAMMA_EDDY &&
        !(st.vis.on && (st.vis.c.model == ORC_VISCOSITY_SMAGORINSKY || st.vis.c.model == ORC_VISCOSITY_FIELD)))
        return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: EDDY needs the viscosity arm on with model SMAGORINSKY or FIELD "
                                               "(orc_solver_set_viscosity)");
    D.c = *c;
    D.on = true;
    D.stale = true;
    return ORC_OK;
}

int orc_solver_set_scalar_diffusivity_field(OrcSolver *s, const double *gamma) {
    if (!s || !gamma) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity field: null argument");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    Scalar::Diffusivity &D = st.sc.gd;
    const size_t n = (size_t)st.n;
    for (size_t i = 0; i < n; ++i)
        if (!(gamma[i] > 0.) || !std::isfinite(gamma[i]))
            return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity field: entry %lld is not positive and finite", (long long)i);
    ORC_TRY(upload_cells(*st.mesh, gamma, D.field));
    D.has_field = true;
    if (D.on && D.c.model == ORC_SCALAR_GAMMA_FIELD) D.stale = true;
    return ORC_OK;
}

int orc_solver_get_scalar_diffusivity(OrcSolver *s, double *gamma) {
    if (!s || !gamma) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar diffusivity: null argument");
    SolverState &st = s->st;
    if (!st.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "scalar: the arm is off (orc_solver_set_scalar)");
    if (gamma_model(st) == ORC_SCALAR_GAMMA_CONSTANT) {
        std::fill(gamma, gamma + st.n, st.sc.c.diffusivity);
        return ORC_OK;
    }
    OrcMesh &m = *st.mesh;
    if (gamma_model(st) == ORC_SCALAR_GAMMA_LINEAR && m.halo.active()) ORC_TRY(m.halo.exchange(st.sc.phi.p));
    DevBuf<double> out;
    ORC_TRY(out.alloc((size_t)std::max<int64_t>(st.n, 1)));
    hipLaunchKernelGGL(scalar_gamma_k, dim3(grid_for(st.n)), dim3(kBlock), 0, ctx().stream, st.n, gamma_law(st), out.p);
    ORC_HIP(hipGetLastError());
    return download_cells(m, out.p, gamma);
}

int orc_bench_scalar_diffusivity(OrcSolver *s, int reps, double avg_ms[3]) {
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "null argument");
    SolverState &st = s->st;
    ORC_TRY(ready(st));
    if (!st.sc.gd.on) return set_error(ORC_ERR_BAD_ARGUMENT, "bench scalar diffusivity: no model is on (orc_solver_set_scalar_diffusivity)");
    if (reps < 1) reps = 1;
    ORC_TRY(ensure_configured(st, false));
    ORC_TRY(k_scalar_face_flux(st));
    OrcMesh &m = *st.mesh;
    Scalar &c = st.sc;
    if (m.halo.active()) ORC_TRY(m.halo.exchange(c.phi.p));
    DevBuf<double> a_t, b_t, bt_t;  // every pass writes here: the arm's Gamma part and boundary terms keep their bits
    ORC_TRY(a_t.alloc((size_t)std::max<int64_t>(m.pat.padded, 1))); ORC_TRY(a_t.zero());
    ORC_TRY(b_t.alloc((size_t)std::max<int64_t>(st.n, 1))); ORC_TRY(b_t.zero());
    ORC_TRY(bt_t.alloc((size_t)std::max<int64_t>(m.n_faces, 1))); ORC_TRY(bt_t.zero());
    const GammaLaw G = gamma_law(st);
    const int g_rows = grid_for(st.n_own), g_faces = grid_for(m.n_faces);
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    int status = ORC_OK;
    for (int pass = 0; pass < 3 && status == ORC_OK; ++pass) {
        auto launch = [&] {
            if (pass == 0)
                hipLaunchKernelGGL(scalar_diffusion_k, dim3(g_rows), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), c.c.diffusivity,
                                   c.zkind.p, c.zval.p, a_t.p, b_t.p);
            else if (pass == 1)
                hipLaunchKernelGGL(scalar_diffusion_var_k, dim3(g_rows), dim3(kBlock), 0, ctx().stream, m.dev(), m.pat.dev(), G, c.zkind.p,
                                   c.zval.p, a_t.p, b_t.p);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(scalar_face_var_k<false>), dim3(g_faces), dim3(kBlock), 0, ctx().stream, m.dev(), c.flux.p,
                                   c.phi.p, c.grad.p, c.zkind.p, c.zval.p, G, st.rho, c.c.scheme, c.corr.p, bt_t.p);
            return hipGetLastError() == hipSuccess ? (int)ORC_OK : set_error(ORC_ERR_HIP, "bench scalar diffusivity: launch failed");
        };
        status = launch();  // warm-up
        if (status == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) status = set_error(ORC_ERR_HIP, "hipEventRecord failed");
        for (int i = 0; i < reps && status == ORC_OK; ++i) status = launch();
        float ms = 0.f;
        if (status == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                                 hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
            status = set_error(ORC_ERR_HIP, "timing the scalar diffusivity passes failed");
        avg_ms[pass] = (double)ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // the scratch buffers are freed on return
    return status;
}

}  // extern "C"
