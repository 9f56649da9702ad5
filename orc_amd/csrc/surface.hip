// surface.hip — per-zone surface reports (new-build extension; ORC reports no surface quantity): force, moment, mass and
// momentum flow, area and area-weighted pressure of every boundary zone, summed over the zone's boundary faces of owned cells.
// DESIGN.md §3 "Surface reports" has the definitions; orc_types.h OrcSurfaceQuantity names the sixteen sums.
//
//   the boundary index (once per mesh, on the device, deterministic by construction: no atomic append)
//     surface_count_k   one thread per segment of kSurfaceSegment consecutive faces: boundary faces of owned cells per zone
//     surface_scan_k    one workgroup: exclusive scan of the [zone][segment] count table, zone-major = the order of bface
//     surface_place_k   the same walk as the count: face f of zone z goes to the next free slot of (z, segment)
//   a report (two launches on the library stream, fp64, no float atomics)
//     surface_zone_k    one workgroup per chunk of <= kSurfaceChunk faces of ONE zone: sixteen terms per face, a tree per lane,
//                       wave __shfl_down, LDS across the four waves -> partials[chunk][16]
//     surface_fold_k    one workgroup per zone: the zone's chunks in chunk order, pairwise -> out[zone][16]
// The association depends on the mesh only (chunk table) and never on a grid size: two reports of one state give the same bits.
#include <algorithm>
#include <cmath>

#include "assembly.hpp"
#include "cell_order.hpp"

namespace orc {

constexpr int kSurfaceSlots = 8;                       // faces a lane of surface_zone_k takes at most
constexpr int kSurfaceChunk = kBlock * kSurfaceSlots;  // faces per workgroup
constexpr int kSurfaceSegment = 256;                   // consecutive faces one thread of the index build walks
constexpr int kSurfaceFoldDepth = 32;                  // pairwise fold: one stack level per bit of the (int32) chunk count

namespace {

__device__ __forceinline__ bool surface_face(const MeshDev &M, int64_t f) { return M.c1[f] < 0 && M.c0[f] < M.n_own; }

// ------------------------------------------------------------------ the boundary index
// cnt[z * S + t]: boundary faces of owned cells of zone z among the faces [t * kSurfaceSegment, (t + 1) * kSurfaceSegment)
// Lane t walks 256 consecutive faces, so neighbouring lanes read 1 KB apart: uncoalesced on purpose (the order of the walk is the
// order of bface); a cost paid once per mesh, as in surface_place_k.  The table costs 4 Z S bytes and surface_scan_k's single
// workgroup Z S additions: both grow linearly with the zone count (DESIGN §3 "Surface reports").
__global__ __launch_bounds__(kBlock) void surface_count_k(MeshDev M, int64_t S, int32_t *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return;
    const int64_t f0 = t * kSurfaceSegment, f1 = f0 + kSurfaceSegment < M.n_faces ? f0 + kSurfaceSegment : M.n_faces;
    for (int64_t f = f0; f < f1; ++f)
        if (surface_face(M, f)) cnt[(int64_t)M.fzone[f] * S + t] += 1;
}

// In place: cnt[i] <- sum of cnt[0 .. i) (zone-major, so the faces of a zone are contiguous and ascending in face id);
// zone_ptr[z] = the offset of zone z's first segment, zone_ptr[Z] = the total.  One workgroup, each thread a contiguous piece.
__global__ __launch_bounds__(kBlock) void surface_scan_k(int32_t *__restrict__ cnt, int64_t N, int64_t S, int Z, int64_t *__restrict__ zone_ptr) {
    __shared__ int64_t base[kBlock + 1];
    const int64_t per = (N + kBlock - 1) / kBlock;
    const int64_t lo = (int64_t)threadIdx.x * per < N ? (int64_t)threadIdx.x * per : N;
    const int64_t hi = lo + per < N ? lo + per : N;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += cnt[i];
    base[threadIdx.x + 1] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        base[0] = 0;
        for (int i = 1; i <= kBlock; ++i) base[i] += base[i - 1];
        zone_ptr[Z] = base[kBlock];
    }
    __syncthreads();
    int64_t run = base[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        if (i % S == 0) zone_ptr[i / S] = run;
        const int32_t c = cnt[i];
        cnt[i] = (int32_t)run;
        run += c;
    }
}

// off[z * S + t]: the next free slot of (zone, segment); a thread owns its slots, so the placement is stable without atomics.
// The walk and its predicate are surface_count_k's, so every slot lies in [0, nb); one that does not is not written and raises
// *bad, which fails the build (build_index) instead of leaving a face out silently.
__global__ __launch_bounds__(kBlock) void surface_place_k(MeshDev M, int64_t S, int32_t *__restrict__ off, int64_t nb, int32_t *__restrict__ bface,
                                                          int *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return;
    const int64_t f0 = t * kSurfaceSegment, f1 = f0 + kSurfaceSegment < M.n_faces ? f0 + kSurfaceSegment : M.n_faces;
    for (int64_t f = f0; f < f1; ++f) {
        if (!surface_face(M, f)) continue;
        const int64_t slot = (int64_t)M.fzone[f] * S + t;
        const int32_t pos = off[slot];
        if (pos >= 0 && pos < nb) bface[pos] = (int32_t)f;
        else atomicCAS(bad, 0, 1);
        off[slot] = pos + 1;
    }
}

// ------------------------------------------------------------------ a report
struct SurfaceArgs {
    const int32_t *bface;
    const int4 *chunk;  // {zone, begin, end, 0}
    const double *u, *v, *w, *p;
    double rho, mu, x0, y0, z0;
    const double *mu_cell;  // null, or the per-cell viscosity that replaces mu (variable viscosity on: the face's cell)
};

// what a zone type means for a boundary face (get_face_velocity solver.rs:952-1003, get_face_pressure :1104-1150, get_face_flux
// :1007-1102 and build_momentum_diffusion_matrix discretization.rs:70-88): uniform per workgroup, decided once, outside the face loop
struct ZoneRule {
    bool vec_bc;   // U_f = the zone vector (Wall, VelocityInlet), else the cell velocity
    bool p_bc;     // p_f = the zone scalar (PressureInlet, PressureOutlet), else the cell pressure
    bool no_flux;  // phi_f = 0 exactly (Wall, Symmetry)
    double zs, zx, zy, zz;
};

// The sixteen terms of one face in THE operator order (DESIGN §3 "Surface reports"; tests/surface_restatement.py repeats it):
//   phi = (n.x U.x + n.y U.y) + n.z U.z        d = (mu A) / sqrt((dx dx + dy dy) + dz dz), dx = x_f - x_P
//   m = (rho phi) A        pa = p_f A        Fp = pa n        Fv = d (U_P - U_f)        r = x_f - x_0        F = Fp + Fv
//   M = (r.y F.z - r.z F.y, r.z F.x - r.x F.z, r.x F.y - r.y F.x)
__device__ __forceinline__ void surface_terms(const MeshDev &M, const SurfaceArgs &A, const ZoneRule &R, int f, double t[ORC_SURFACE_N]) {
    const int P = M.c0[f];
    const double a = M.area[f], nx = M.nx[f], ny = M.ny[f], nz = M.nz[f];  // n points out of c0, the only cell of a boundary face
    const double fx = M.fcx[f], fy = M.fcy[f], fz = M.fcz[f];
    const double upx = A.u[P], upy = A.v[P], upz = A.w[P];
    const double ufx = R.vec_bc ? R.zx : upx, ufy = R.vec_bc ? R.zy : upy, ufz = R.vec_bc ? R.zz : upz;
    const double pf = R.p_bc ? R.zs : A.p[P];
    const double m = R.no_flux ? 0. : (A.rho * ((nx * ufx + ny * ufy) + nz * ufz)) * a;
    const double pa = pf * a;
    const double fpx = pa * nx, fpy = pa * ny, fpz = pa * nz;
    double fvx = 0., fvy = 0., fvz = 0.;
    if (R.vec_bc) {
        const double dx = fx - M.ccx[P], dy = fy - M.ccy[P], dz = fz - M.ccz[P];
        const double d = ((A.mu_cell ? A.mu_cell[P] : A.mu) * a) / sqrt((dx * dx + dy * dy) + dz * dz);
        fvx = d * (upx - ufx); fvy = d * (upy - ufy); fvz = d * (upz - ufz);
    }
    const double rx = fx - A.x0, ry = fy - A.y0, rz = fz - A.z0;
    const double Fx = fpx + fvx, Fy = fpy + fvy, Fz = fpz + fvz;
    t[ORC_SURFACE_AREA] = a;
    t[ORC_SURFACE_MASS_FLOW] = m;
    t[ORC_SURFACE_PRESSURE_FORCE] = fpx; t[ORC_SURFACE_PRESSURE_FORCE + 1] = fpy; t[ORC_SURFACE_PRESSURE_FORCE + 2] = fpz;
    t[ORC_SURFACE_VISCOUS_FORCE] = fvx; t[ORC_SURFACE_VISCOUS_FORCE + 1] = fvy; t[ORC_SURFACE_VISCOUS_FORCE + 2] = fvz;
    t[ORC_SURFACE_MOMENTUM_FLOW] = R.no_flux ? 0. : m * ufx;
    t[ORC_SURFACE_MOMENTUM_FLOW + 1] = R.no_flux ? 0. : m * ufy;
    t[ORC_SURFACE_MOMENTUM_FLOW + 2] = R.no_flux ? 0. : m * ufz;
    t[ORC_SURFACE_MOMENT] = ry * Fz - rz * Fy;
    t[ORC_SURFACE_MOMENT + 1] = rz * Fx - rx * Fz;
    t[ORC_SURFACE_MOMENT + 2] = rx * Fy - ry * Fx;
    t[ORC_SURFACE_PRESSURE_AREA] = pa;
    t[ORC_SURFACE_FACES] = 1.;
}

// One workgroup per chunk.  Lane `tid` takes the faces begin + tid + k kBlock, k = 0 .. 7 (a missing face is sixteen zeros) and
// sums its eight slots as ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)); then block_sum's association per quantity: the wave
// tree of __shfl_down (offsets 32 .. 1), then ((w0 + w1) + w2) + w3 over the four waves through LDS — all sixteen quantities
// behind one barrier.  Depth of the tree over a full chunk: 3 + 6 + 3 rounded additions.
__global__ __launch_bounds__(kBlock) void surface_zone_k(MeshDev M, SurfaceArgs A, double *__restrict__ partials, int *status) {
    __shared__ double lds[kBlock / kWave][ORC_SURFACE_N];
    const int4 c = A.chunk[blockIdx.x];
    const int z = c.x, begin = c.y, end = c.z;
    const int zt = M.ztype[z];
    const bool supported = zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET || zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET ||
                           zt == ORC_BC_SYMMETRY;
    if (!supported) {  // what diffusion_k and face_k refuse (discretization.rs:114-117, solver.rs:1001, 1148)
        if (threadIdx.x == 0) atomicCAS(status, 0, (int)ORC_ERR_UNSUPPORTED_BC);
        if (threadIdx.x < ORC_SURFACE_N) partials[(int64_t)blockIdx.x * ORC_SURFACE_N + threadIdx.x] = 0.;
        return;
    }
    ZoneRule R;
    R.vec_bc = zt == ORC_BC_WALL || zt == ORC_BC_VELOCITY_INLET;
    R.p_bc = zt == ORC_BC_PRESSURE_INLET || zt == ORC_BC_PRESSURE_OUTLET;
    R.no_flux = zt == ORC_BC_WALL || zt == ORC_BC_SYMMETRY;
    R.zs = M.zscal[z]; R.zx = M.zvec[3 * z]; R.zy = M.zvec[3 * z + 1]; R.zz = M.zvec[3 * z + 2];

    double acc[ORC_SURFACE_N], pair[ORC_SURFACE_N], quad[ORC_SURFACE_N], half[ORC_SURFACE_N];
#pragma unroll
    for (int q = 0; q < ORC_SURFACE_N; ++q) acc[q] = pair[q] = quad[q] = half[q] = 0.;
#pragma unroll
    for (int k = 0; k < kSurfaceSlots; ++k) {
        double t[ORC_SURFACE_N];
#pragma unroll
        for (int q = 0; q < ORC_SURFACE_N; ++q) t[q] = 0.;
        const int i = begin + k * kBlock + (int)threadIdx.x;
        if (i < end) surface_terms(M, A, R, A.bface[i], t);
#pragma unroll
        for (int q = 0; q < ORC_SURFACE_N; ++q) {
            if ((k & 1) == 0) { pair[q] = t[q]; continue; }
            pair[q] = pair[q] + t[q];
            if ((k & 2) == 0) { quad[q] = pair[q]; continue; }
            quad[q] = quad[q] + pair[q];
            if ((k & 4) == 0) half[q] = quad[q];
            else acc[q] = half[q] + quad[q];
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < ORC_SURFACE_N; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) lds[wv][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < ORC_SURFACE_N) {
        const int q = threadIdx.x;
        partials[(int64_t)blockIdx.x * ORC_SURFACE_N + q] = ((lds[0][q] + lds[1][q]) + lds[2][q]) + lds[3][q];
    }
}

// One workgroup per zone; thread q < 16 folds quantity q of the zone's chunks in chunk order, pairwise: chunk i is pushed on a
// stack and merged with the entry below it once for every trailing one bit of i (earlier + later), the left-overs are merged from
// the top down.  Depth ceil(log2(chunks)); a zone without a chunk gives zeros.  After chunk i the stack holds one entry per one bit
// of i + 1, and chunk indices are int32: never more than 31 entries, so kSurfaceFoldDepth = 32 levels cannot overflow.  Also publishes the status word behind the sums, so
// that one download carries both.
__global__ __launch_bounds__(kWave) void surface_fold_k(const int32_t *__restrict__ zone_chunk_ptr, const double *__restrict__ partials,
                                                        const int *__restrict__ status, int Z, double *__restrict__ out) {
    __shared__ double stack[kSurfaceFoldDepth][ORC_SURFACE_N];
    const int z = blockIdx.x, q = threadIdx.x;
    if (z == 0 && q == 0) out[(int64_t)Z * ORC_SURFACE_N] = (double)*status;
    if (q >= ORC_SURFACE_N) return;
    const int lo = zone_chunk_ptr[z], hi = zone_chunk_ptr[z + 1];
    int sp = 0;
    for (int i = lo; i < hi; ++i) {
        double v = partials[(int64_t)i * ORC_SURFACE_N + q];
        for (unsigned k = (unsigned)(i - lo); (k & 1u) && sp > 0; k >>= 1) v = stack[--sp][q] + v;
        stack[sp++][q] = v;
    }
    double r = 0.;
    if (sp > 0) {
        r = stack[--sp][q];
        while (sp > 0) r = stack[--sp][q] + r;
    }
    out[(int64_t)z * ORC_SURFACE_N + q] = r;
}

// ====================================================================== host side
int build_index(OrcMesh &m) {
    std::unique_ptr<SurfaceIndex> X(new SurfaceIndex());
    const int Z = m.n_zones;
    const int64_t S = (m.n_faces + kSurfaceSegment - 1) / kSurfaceSegment, N = (int64_t)Z * S;
    if (S / kBlock + 1 >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "surface index: mesh too large");
    const int grid = (int)((S + kBlock - 1) / kBlock);
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> zone_ptr;
    ORC_TRY(cnt.alloc((size_t)N));
    ORC_TRY(cnt.zero());
    ORC_TRY(zone_ptr.alloc((size_t)Z + 1));
    hipLaunchKernelGGL(surface_count_k, dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), S, cnt.p);
    hipLaunchKernelGGL(surface_scan_k, dim3(1), dim3(kBlock), 0, ctx().stream, cnt.p, N, S, Z, zone_ptr.p);
    ORC_HIP(hipGetLastError());
    X->h_zone_ptr.assign((size_t)Z + 1, 0);
    ORC_TRY(zone_ptr.download(X->h_zone_ptr.data(), (size_t)Z + 1));
    const int64_t nb = X->h_zone_ptr[(size_t)Z];
    if (nb < 0 || nb > m.n_faces) return set_error(ORC_ERR_HIP, "surface index: inconsistent boundary-face count %lld", (long long)nb);
    X->n_bfaces = nb;
    ORC_TRY(X->bface.alloc((size_t)std::max<int64_t>(nb, 1)));
    DevBuf<int> bad;
    ORC_TRY(bad.alloc(1));
    ORC_TRY(bad.zero());
    hipLaunchKernelGGL(surface_place_k, dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), S, cnt.p, nb, X->bface.p, bad.p);
    ORC_HIP(hipGetLastError());
    int h_bad = 0;
    ORC_TRY(bad.download(&h_bad, 1));
    if (h_bad) return set_error(ORC_ERR_HIP, "surface index: placement disagrees with the count");
    // the chunk table: every zone's segment cut into pieces of at most kSurfaceChunk faces, none across two zones
    std::vector<int32_t> chunk, zcp((size_t)Z + 1, 0);
    for (int z = 0; z < Z; ++z) {
        for (int64_t b = X->h_zone_ptr[(size_t)z]; b < X->h_zone_ptr[(size_t)z + 1]; b += kSurfaceChunk) {
            const int64_t e = std::min<int64_t>(b + kSurfaceChunk, X->h_zone_ptr[(size_t)z + 1]);
            chunk.push_back(z); chunk.push_back((int32_t)b); chunk.push_back((int32_t)e); chunk.push_back(0);
        }
        zcp[(size_t)z + 1] = (int32_t)(chunk.size() / 4);
    }
    X->n_chunks = (int64_t)(chunk.size() / 4);
    if (chunk.empty()) chunk.assign(4, 0);
    ORC_TRY(X->chunk.upload(chunk.data(), chunk.size()));
    ORC_TRY(X->zone_chunk_ptr.upload(zcp.data(), zcp.size()));
    ORC_TRY(X->partials.alloc((size_t)std::max<int64_t>(X->n_chunks, 1) * ORC_SURFACE_N));
    ORC_TRY(X->out.alloc((size_t)Z * ORC_SURFACE_N + 1));
    ORC_TRY(X->status.alloc(1));
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // cnt and zone_ptr are freed on return
    X->builds = 1;
    m.surface = std::move(X);
    return ORC_OK;
}

int ensure_index(OrcMesh &m) { return m.surface ? ORC_OK : build_index(m); }

bool finite3(const double *x) { return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]); }

}  // namespace

int surface_index(OrcMesh &m) { return ensure_index(m); }

int surface_report_dev(OrcMesh &m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                       const double *mu_cell, const double origin[3], double *per_zone) {
    ORC_TRY(ensure_index(m));
    SurfaceIndex &X = *m.surface;
    const int Z = m.n_zones;
    SurfaceArgs A{};
    A.bface = X.bface.p; A.chunk = reinterpret_cast<const int4 *>(X.chunk.p);
    A.u = u; A.v = v; A.w = w; A.p = p;
    A.rho = rho; A.mu = mu; A.mu_cell = mu_cell;
    A.x0 = origin ? origin[0] : 0.; A.y0 = origin ? origin[1] : 0.; A.z0 = origin ? origin[2] : 0.;
    ORC_TRY(X.status.zero());
    if (X.n_chunks > 0) hipLaunchKernelGGL(surface_zone_k, dim3((unsigned)X.n_chunks), dim3(kBlock), 0, ctx().stream, m.dev(), A, X.partials.p, X.status.p);
    hipLaunchKernelGGL(surface_fold_k, dim3(Z), dim3(kWave), 0, ctx().stream, X.zone_chunk_ptr.p, X.partials.p, X.status.p, Z, X.out.p);
    ORC_HIP(hipGetLastError());
    const size_t n_out = (size_t)Z * ORC_SURFACE_N;
    if (m.halo.active()) ORC_TRY(comm_allreduce_sum(X.out.p, (int)n_out));
    std::vector<double> host(n_out + 1);
    ORC_TRY(X.out.download(host.data(), n_out + 1));  // the only synchronisation of a report
    int h = (int)host[n_out];
    if (m.halo.active()) h = comm_global_status(h);
    std::copy(host.begin(), host.begin() + (std::ptrdiff_t)n_out, per_zone);
    if (h != ORC_OK) return set_error(h, "surface report: a boundary face lies in a zone whose type the assembly does not support");
    return ORC_OK;
}

}  // namespace orc

using namespace orc;

extern "C" {

int orc_solver_surface_report(OrcSolver *s, const double origin[3], double *per_zone) {
    ORC_TRY(ensure_init());
    if (!s || !per_zone) return set_error(ORC_ERR_BAD_ARGUMENT, "surface report: null argument");
    if (origin && !finite3(origin)) return set_error(ORC_ERR_BAD_ARGUMENT, "surface report: the origin must be finite");
    SolverState &st = s->st;
    return surface_report_dev(*st.mesh, st.u.p, st.v.p, st.w.p, st.p.p, st.rho, st.mu, st.cell_viscosity(), origin, per_zone);
}

int orc_surface_integrals(OrcMesh *m, const double *u, const double *v, const double *w, const double *p, double rho, double mu,
                          const double origin[3], double *per_zone) {
    ORC_TRY(ensure_init());
    if (!m || !u || !v || !w || !p || !per_zone) return set_error(ORC_ERR_BAD_ARGUMENT, "surface integrals: null argument");
    if (origin && !finite3(origin)) return set_error(ORC_ERR_BAD_ARGUMENT, "surface integrals: the origin must be finite");
    if (!(rho > 0.) || !std::isfinite(rho) || !(mu > 0.) || !std::isfinite(mu))
        return set_error(ORC_ERR_BAD_ARGUMENT, "surface integrals: rho and mu must be positive and finite");
    const double *src[4] = {u, v, w, p};
    DevBuf<double> dev[4];
    for (int k = 0; k < 4; ++k) ORC_TRY(upload_cells(*m, src[k], dev[k]));
    return surface_report_dev(*m, dev[0].p, dev[1].p, dev[2].p, dev[3].p, rho, mu, nullptr, origin, per_zone);
}

int orc_mesh_boundary_index(OrcMesh *m, int64_t *zone_ptr, int32_t *faces, int64_t *n_builds, int32_t *chunk) {
    ORC_TRY(ensure_init());
    if (!m || !zone_ptr) return set_error(ORC_ERR_BAD_ARGUMENT, "boundary index: null argument");
    ORC_TRY(ensure_index(*m));
    const SurfaceIndex &X = *m->surface;
    std::copy(X.h_zone_ptr.begin(), X.h_zone_ptr.end(), zone_ptr);
    if (faces && X.n_bfaces > 0) ORC_TRY(X.bface.download(faces, (size_t)X.n_bfaces));
    if (n_builds) *n_builds = X.builds;
    if (chunk) *chunk = kSurfaceChunk;
    return ORC_OK;
}

}  // extern "C"
