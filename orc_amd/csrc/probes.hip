// probes.hip — point probes (new-build extension; ORC has no entry that takes a coordinate): points located in cells, fields sampled at
// them, a per-step history.  DESIGN.md §3 "Point probes" has the definition; in short, for a point x
//     start cell   the owned cell P with the smallest s_P = (r.x r.x + r.y r.y) + r.z r.z, r = x - x_P; the smallest ORC id among ties
//     walk         at P the face f of P's list with the largest g_f = (r.x n.x + r.y n.y) + r.z n.z, r = x - x_f, negated when P is not
//                  c0[f] (the first face among ties): g <= 0 INSIDE, a boundary face OUTSIDE, else on to the neighbour, 64 moves at most
//     sample       CELL phi_P;  LINEAR phi_P + ((G.x r.x + G.y r.y) + G.z r.z), r = x - x_P, G by the assembly's per-cell bodies
//
//   sphere_tiles_k   (sphere_cull.hpp) once per mesh: a sphere around every tile of kProbeTile consecutive cell centroids
//   probe_search_k   M points x N cells, fp64, compute-bound: one lane per point, the cell index wave-uniform — the three centroid values
//                    come from the mesh's own ccx / ccy / ccz through scalar loads, no table copy, no LDS.  M / 64 waves cannot fill the
//                    chip, so the tiles are cut into slabs over gridDim.y; every (slab, point) writes one partial (s, cell).  Culled
//                    (the default) as wall_search_k: the slab's tile nearest to the wave's first point seeds the best value, then a tile
//                    is entered only if some lane's lower bound over its sphere does not exceed that lane's best.  The host sorts the
//                    points along a Morton curve first so that the points of a wave are neighbours, and un-sorts every output.
//   probe_fold_k     one lane per point: the minimum of its slab partials under the tie rule.  No float atomics anywhere: the same
//                    input gives the same bits, whatever the point order, the slab count or the cull.
//   probe_walk_k     one lane per point: the walk.
//   probe_sample_k   one lane per point: the cell's gradient through gradient_cell.hpp (the bits of orc_calculate_gradients) and the
//                    selected fields in one pass; the history calls it into a device record.
// Read-only towards mesh and solver, and opt-in: nothing here is launched unless a probe entry is called or the history is on.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <numeric>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"
#include "point_walk.hpp"
#include "probes.hpp"
#include "sphere_cull.hpp"

namespace orc {

constexpr int kProbeTile = 64;           // cells per tile: one bounding sphere, one skip decision per wave
constexpr int kProbeTargetWaves = 8192;  // 256 CUs x 4 SIMDs x 8 waves: what the slabs aim at
constexpr int kProbeMaxSlabs = 4096;     // gridDim.y stays far below 65535; the partials hold slabs x points entries

namespace {

struct ProbeStats {
    long long n_tiles = 0, visits = 0, waves = 0, slabs = 0, moves = 0;
};
ProbeStats g_stats;

constexpr uint32_t kAllFields = (1u << ORC_PROBE_N) - 1;
constexpr uint32_t kVelocity = (1u << ORC_PROBE_U) | (1u << ORC_PROBE_V) | (1u << ORC_PROBE_W);
static_assert(ORC_PROBE_N == 6 && ORC_PROBE_P == 3 && ORC_PROBE_PHI == 4 && ORC_PROBE_MU == 5,
              "the field order is part of the ABI (orc_amd/settings.py ProbeField)");

// ------------------------------------------------------------------ the search
struct ProbeBest {
    double s;    // the smallest s so far
    int32_t id;  // the ORC id of the cell that reached it, the smallest one among exact ties
    int32_t j;   // that cell in the internal numbering, -1 = none yet
};

// one cell against one point: THE operator order of the definition.  j is wave-uniform: three scalar loads (four with a map), no LDS.
template <bool kMap>
__device__ __forceinline__ void probe_entry(const int32_t *__restrict__ orc, int64_t j, double cx, double cy, double cz, double x, double y, double z,
                                            ProbeBest &b) {
    const double rx = x - cx, ry = y - cy, rz = z - cz;
    const double s = (rx * rx + ry * ry) + rz * rz;
    if (s <= b.s) {
        const int32_t id = kMap ? orc[j] : (int32_t)j;
        if (s < b.s || id < b.id) { b.s = s; b.id = id; b.j = (int32_t)j; }
    }
}

// A full tile goes in groups of kProbeGroup cells whose 3 kProbeGroup centroid values are loaded before the first is used: the rarely
// taken branch of an entry would otherwise stand between one entry's scalar loads and the next's, and every entry would wait for its own.
constexpr int kProbeGroup = 8;
template <bool kMap>
__device__ __forceinline__ void probe_tile(const MeshDev &M, const int32_t *__restrict__ orc, int64_t t, double x, double y, double z, ProbeBest &b) {
    const int64_t j0 = t * kProbeTile;
    if (j0 + kProbeTile <= M.n_own) {
        for (int k0 = 0; k0 < kProbeTile; k0 += kProbeGroup) {
            double cx[kProbeGroup], cy[kProbeGroup], cz[kProbeGroup];
#pragma unroll
            for (int k = 0; k < kProbeGroup; ++k) { cx[k] = M.ccx[j0 + k0 + k]; cy[k] = M.ccy[j0 + k0 + k]; cz[k] = M.ccz[j0 + k0 + k]; }
#pragma unroll
            for (int k = 0; k < kProbeGroup; ++k) probe_entry<kMap>(orc, j0 + k0 + k, cx[k], cy[k], cz[k], x, y, z, b);
        }
    } else {
        for (int64_t j = j0; j < M.n_own; ++j) probe_entry<kMap>(orc, j, M.ccx[j], M.ccy[j], M.ccz[j], x, y, z, b);
    }
}

struct SearchArgs {
    const int32_t *orc;      // internal -> ORC id (kMap)
    const double *tiles;     // [4][n_tiles]
    int64_t n_tiles;
    int slabs;               // == gridDim.y
    const double *x, *y, *z; // [n_pts]
    int64_t n_pts;
    double *part_s;          // [slabs][n_pts]
    int32_t *part_j;         // [slabs][n_pts], -1 where the slab holds no cell
    unsigned long long *visits;
};

// Lane i of a wave owns point 64 wave + i; the idle lanes of the last wave repeat the last point and write nothing, so that every vote
// of the wave is a vote of points.  Slab y covers the tiles [y n_tiles / slabs, (y + 1) n_tiles / slabs) — possibly none.  Any order of
// the walk gives the same bits (a minimum with a tie rule), so the culled search may start where it likes and leave out what cannot
// matter (sphere_skip, sphere_cull.hpp).  Every index is below n_own (tiles) or n_pts (points) by construction of t0, t1 and ii.
template <bool kCull, bool kMap>
__global__ __launch_bounds__(kBlock) void probe_search_k(MeshDev M, SearchArgs A) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    if (i - lane >= A.n_pts) return;  // the whole wave lies past the points
    const int64_t ii = i < A.n_pts ? i : A.n_pts - 1;
    const double x = A.x[ii], y = A.y[ii], z = A.z[ii];
    const int64_t slab = blockIdx.y;
    const int64_t t0 = slab * A.n_tiles / A.slabs, t1 = (slab + 1) * A.n_tiles / A.slabs;
    ProbeBest b{INFINITY, INT_MAX, -1};
    unsigned long long entered = 0;
    if (!kCull) {
        for (int64_t t = t0; t < t1; ++t) probe_tile<kMap>(M, A.orc, t, x, y, z, b);
        entered = (unsigned long long)(t1 - t0);
    } else if (t1 > t0) {
        const int64_t nt = A.n_tiles;
        const double *tx = A.tiles, *ty = A.tiles + nt, *tz = A.tiles + 2 * nt, *tr = A.tiles + 3 * nt;
        // the seed: the slab's tile whose centre is nearest to the wave's first point (the points of a wave are neighbours)
        int64_t near = t0;
        double near_q = INFINITY;
        for (int64_t t = t0; t < t1; ++t) {
            const double q = sphere_q(x, y, z, tx[t], ty[t], tz[t]);
            if (q < near_q) { near_q = q; near = t; }
        }
        const int64_t seed = __builtin_amdgcn_readfirstlane((int)near);
        probe_tile<kMap>(M, A.orc, seed, x, y, z, b);
        entered = 1;
        double sb = sphere_reach(b.s);
        for (int64_t t = t0; t < t1; ++t) {
            if (t == seed) continue;
            const bool skip = sphere_skip(sphere_q(x, y, z, tx[t], ty[t], tz[t]), sb, tr[t]);
            if (!__any(!skip)) continue;
            probe_tile<kMap>(M, A.orc, t, x, y, z, b);
            sb = sphere_reach(b.s);
            ++entered;
        }
    }
    if (i < A.n_pts) {
        A.part_s[slab * A.n_pts + i] = b.s;
        A.part_j[slab * A.n_pts + i] = b.j;
    }
    if (lane == 0) atomicAdd(A.visits, entered);
}

// the minimum over the slabs of one point under the tie rule; a point no slab found a cell for (impossible with n_own >= 1) starts at 0
template <bool kMap>
__global__ __launch_bounds__(kBlock) void probe_fold_k(const int32_t *__restrict__ orc, int slabs, int64_t n_pts, const double *__restrict__ part_s,
                                                       const int32_t *__restrict__ part_j, int32_t *__restrict__ start) {
    GRID_STRIDE(i, n_pts) {
        double bs = INFINITY;
        int32_t bj = -1, bid = INT_MAX;
        for (int k = 0; k < slabs; ++k) {
            const double s = part_s[(int64_t)k * n_pts + i];
            const int32_t j = part_j[(int64_t)k * n_pts + i];
            if (j < 0) continue;
            const int32_t id = kMap ? orc[j] : j;
            if (bj < 0 || s < bs || (s == bs && id < bid)) { bs = s; bj = j; bid = id; }
        }
        start[i] = bj < 0 ? 0 : bj;
    }
}

// ------------------------------------------------------------------ the walk
struct WalkArgs {
    const double *x, *y, *z;
    int64_t n_pts;
    const int32_t *start;
    int32_t *cell, *status, *steps, *zone;
    double *excess, *off;  // [n_pts], [3][n_pts]
    unsigned long long *moves;
};

// One lane per point: the walk of point_walk.hpp from the search's start cell.
__global__ __launch_bounds__(kBlock) void probe_walk_k(MeshDev M, WalkArgs A) {
    int total = 0;
    GRID_STRIDE(i, A.n_pts) {
        const double x = A.x[i], y = A.y[i], z = A.z[i];
        int P = A.start[i];
        const WalkEnd e = point_walk(M, x, y, z, P);
        A.cell[i] = P; A.status[i] = e.status; A.steps[i] = e.moves; A.zone[i] = e.zone;
        A.excess[i] = e.g;
        A.off[i] = x - M.ccx[P]; A.off[A.n_pts + i] = y - M.ccy[P]; A.off[2 * A.n_pts + i] = z - M.ccz[P];
        total += e.moves;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o, 64);
    if ((threadIdx.x & (kWave - 1)) == 0 && total > 0) atomicAdd(A.moves, (unsigned long long)total);
}

// ------------------------------------------------------------------ the sampler
struct SampleArgs {
    const double *u, *v, *w, *p, *phi, *mu_cell;  // phi: null unless selected; mu_cell: null = the constant mu
    double mu;
    const int32_t *cell;
    const double *off;
    int64_t n_pts;
    double *out;  // [popcount(mask)][n_pts]
    uint32_t mask;
    int linear, q1;
};

__device__ __forceinline__ double linear_at(double phi, V3 g, double rx, double ry, double rz) { return phi + ((g.x * rx + g.y * ry) + g.z * rz); }

// One lane per point: the gradients of the hit cell only, never stored.  kLsq: the solver's gradient_reconstruction.
template <bool kLsq>
__global__ __launch_bounds__(kBlock) void probe_sample_k(MeshDev M, SampleArgs A, int *status) {
    GRID_STRIDE(i, A.n_pts) {
        const int c = A.cell[i];
        const double rx = A.off[i], ry = A.off[A.n_pts + i], rz = A.off[2 * A.n_pts + i];
        double val[ORC_PROBE_N] = {0., 0., 0., 0., 0., 0.};
        if (A.mask & kVelocity) {
            val[ORC_PROBE_U] = A.u[c]; val[ORC_PROBE_V] = A.v[c]; val[ORC_PROBE_W] = A.w[c];
            if (A.linear) {
                V3 gx, gy, gz;
                double conv;
                if (kLsq) {
                    double g[3][3];
                    grad_u_lsq_cell<false>(M, A.u, A.v, A.w, c, status, g, conv);
                    gx = mk(g[0][0], g[0][1], g[0][2]); gy = mk(g[1][0], g[1][1], g[1][2]); gz = mk(g[2][0], g[2][1], g[2][2]);
                } else {
                    grad_u_gg_cell<false>(M, A.u, A.v, A.w, c, status, gx, gy, gz, conv);
                }
                val[ORC_PROBE_U] = linear_at(val[ORC_PROBE_U], gx, rx, ry, rz);
                val[ORC_PROBE_V] = linear_at(val[ORC_PROBE_V], gy, rx, ry, rz);
                val[ORC_PROBE_W] = linear_at(val[ORC_PROBE_W], gz, rx, ry, rz);
            }
        }
        if (A.mask & (1u << ORC_PROBE_P)) {
            val[ORC_PROBE_P] = A.p[c];
            if (A.linear) {
                V3 g;
                if (kLsq) {
                    double t[3];
                    grad_p_lsq_cell(M, A.p, c, status, t);
                    g = mk(t[0], t[1], t[2]);
                } else {
                    g = grad_p_gg_cell(M, A.p, c, A.q1, status);
                }
                val[ORC_PROBE_P] = linear_at(val[ORC_PROBE_P], g, rx, ry, rz);
            }
        }
        if (A.mask & (1u << ORC_PROBE_PHI)) val[ORC_PROBE_PHI] = A.phi[c];
        if (A.mask & (1u << ORC_PROBE_MU)) val[ORC_PROBE_MU] = A.mu_cell ? A.mu_cell[c] : A.mu;
        double *o = A.out + i;
#pragma unroll
        for (int k = 0; k < ORC_PROBE_N; ++k)
            if (A.mask & (1u << k)) { *o = val[k]; o += A.n_pts; }
    }
}

// ====================================================================== host side
// the mesh's spheres and its internal -> ORC map, built once
int ensure_tiles(OrcMesh &m) {
    if (m.probe_tiles) return ORC_OK;
    if (m.n_cells >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: mesh too large");
    std::unique_ptr<ProbeTiles> T(new ProbeTiles());
    T->n_tiles = (m.n_own + kProbeTile - 1) / kProbeTile;
    ORC_TRY(T->tiles.alloc((size_t)std::max<int64_t>(4 * T->n_tiles, 1)));
    if (T->n_tiles > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(sphere_tiles_k<kProbeTile>), dim3((unsigned)((T->n_tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx().stream,
                           m.ccx.p, m.ccy.p, m.ccz.p, m.n_own, T->n_tiles, T->tiles.p);
        ORC_HIP(hipGetLastError());
    }
    if (!cell_order_ids(m).empty()) {
        std::vector<int32_t> g(cell_order_ids(m).begin(), cell_order_ids(m).end());
        ORC_TRY(T->orc_id.upload(g.data(), g.size()));
    }
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    m.probe_tiles = std::move(T);
    return ORC_OK;
}

int choose_slabs(const OrcMesh &m, int64_t n_pts, int forced) {
    if (forced > 0) return std::min(forced, kProbeMaxSlabs);
    const int64_t waves = (n_pts + kWave - 1) / kWave;
    const int64_t want = (kProbeTargetWaves + waves - 1) / waves;
    // no more slabs than tiles, and partials of at most 2^24 entries
    const int64_t cap = std::max<int64_t>(((int64_t)1 << 24) / std::max<int64_t>(n_pts, 1), 1);
    return (int)std::max<int64_t>(1, std::min<int64_t>({want, m.probe_tiles->n_tiles, (int64_t)kProbeMaxSlabs, cap}));
}

struct Scratch {
    DevBuf<double> part_s;
    DevBuf<int32_t> part_j, start;
    DevBuf<unsigned long long> counters;  // [0] tile visits, [1] walk moves
};

int launch_search(OrcMesh &m, const OrcProbes &P, bool cull, int slabs, Scratch &S) {
    const ProbeTiles &T = *m.probe_tiles;
    const int64_t blocks = (P.n + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: too many points");
    SearchArgs A{T.orc_id.p, T.tiles.p, T.n_tiles, slabs, P.x.p, P.y.p, P.z.p, P.n, S.part_s.p, S.part_j.p, S.counters.p};
    const dim3 grid((unsigned)blocks, (unsigned)slabs);
    const bool map = T.orc_id.p != nullptr;
    if (cull && map) hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_search_k<true, true>), grid, dim3(kBlock), 0, ctx().stream, m.dev(), A);
    else if (cull) hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_search_k<true, false>), grid, dim3(kBlock), 0, ctx().stream, m.dev(), A);
    else if (map) hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_search_k<false, true>), grid, dim3(kBlock), 0, ctx().stream, m.dev(), A);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_search_k<false, false>), grid, dim3(kBlock), 0, ctx().stream, m.dev(), A);
    ORC_HIP(hipGetLastError());
    if (map) hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_fold_k<true>), dim3(grid_for(P.n)), dim3(kBlock), 0, ctx().stream, T.orc_id.p, slabs, P.n, S.part_s.p, S.part_j.p, S.start.p);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_fold_k<false>), dim3(grid_for(P.n)), dim3(kBlock), 0, ctx().stream, T.orc_id.p, slabs, P.n, S.part_s.p, S.part_j.p, S.start.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// the walk from S.start into the buffers of `out` (the probe set itself, or a scratch set of the bench)
int launch_walk(OrcMesh &m, const OrcProbes &P, OrcProbes &out, Scratch &S) {
    WalkArgs A{P.x.p, P.y.p, P.z.p, P.n, S.start.p, out.cell.p, out.status.p, out.steps.p, out.zone.p, out.excess.p, out.off.p, S.counters.p + 1};
    hipLaunchKernelGGL(probe_walk_k, dim3(grid_for(P.n)), dim3(kBlock), 0, ctx().stream, m.dev(), A);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int alloc_scratch(int64_t n, int slabs, Scratch &S) {
    ORC_TRY(S.part_s.alloc((size_t)slabs * (size_t)n));
    ORC_TRY(S.part_j.alloc((size_t)slabs * (size_t)n));
    ORC_TRY(S.start.alloc((size_t)n));
    ORC_TRY(S.counters.alloc(2));
    ORC_TRY(S.counters.zero());
    return ORC_OK;
}

int alloc_results(int64_t n, OrcProbes &P) {
    const size_t k = (size_t)n;
    ORC_TRY(P.cell.alloc(k)); ORC_TRY(P.status.alloc(k)); ORC_TRY(P.steps.alloc(k)); ORC_TRY(P.zone.alloc(k));
    ORC_TRY(P.excess.alloc(k)); ORC_TRY(P.off.alloc(3 * k));
    return ORC_OK;
}

// position k of the search order holds point order[k]: ascending 30-bit Morton code of the points in their own bounding box (ties by
// index), so that the 64 points of a wave are neighbours and the cull of a wave skips what all of them can skip
void morton_order(int64_t n, const double *xyz, std::vector<int64_t> &order) {
    double lo[3], hi[3];
    for (int q = 0; q < 3; ++q) lo[q] = hi[q] = xyz[q];
    for (int64_t i = 1; i < n; ++i)
        for (int q = 0; q < 3; ++q) { lo[q] = std::min(lo[q], xyz[3 * i + q]); hi[q] = std::max(hi[q], xyz[3 * i + q]); }
    std::vector<uint32_t> key((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        uint32_t code = 0;
        for (int q = 0; q < 3; ++q) {
            const double span = hi[q] - lo[q];
            const double t = span > 0. && std::isfinite(span) ? (xyz[3 * i + q] - lo[q]) / span : 0.;
            uint32_t v = (uint32_t)std::min(1023., std::max(0., t * 1024.));
            v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u;
            code |= v << q;
        }
        key[(size_t)i] = code;
    }
    order.resize((size_t)n);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key[(size_t)a] < key[(size_t)b]; });
}

}  // namespace

OrcProbes *locate(OrcMesh *m, int64_t n, const double *xyz, bool cull, int forced_slabs, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcProbes *)nullptr; };
    if (status) *status = ORC_OK;
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if (!m || !xyz) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: null argument"));
    if (n < 1) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: n_points must be at least 1"));
    if (n >= ((int64_t)1 << 31)) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: too many points"));
    if (forced_slabs < 0) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: slabs must be >= 0"));
    if (m->halo.active())
        return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: a partitioned mesh is refused: a walk confined to one rank's cells leaves points that no "
                                                    "rank claims, and there is no hand-over between ranks yet"));
    if (m->n_own < 1) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: the mesh has no cells"));
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(xyz[i])) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "probes: coordinate %lld of point %lld is not finite", (long long)(i % 3), (long long)(i / 3)));
    if ((st = ensure_tiles(*m)) != ORC_OK) return fail(st);
    std::unique_ptr<OrcProbes> P(new OrcProbes());
    P->mesh = m;
    P->n = n;
    morton_order(n, xyz, P->order);
    std::vector<double> h((size_t)n);
    DevBuf<double> *dst[3] = {&P->x, &P->y, &P->z};
    for (int q = 0; q < 3; ++q) {
        for (int64_t k = 0; k < n; ++k) h[(size_t)k] = xyz[3 * P->order[(size_t)k] + q];
        if ((st = dst[q]->upload(h.data(), (size_t)n)) != ORC_OK) return fail(st);
    }
    const int slabs = choose_slabs(*m, n, forced_slabs);
    Scratch S;
    if ((st = alloc_scratch(n, slabs, S)) != ORC_OK || (st = alloc_results(n, *P)) != ORC_OK) return fail(st);
    if ((st = launch_search(*m, *P, cull, slabs, S)) != ORC_OK || (st = launch_walk(*m, *P, *P, S)) != ORC_OK) {
        (void)hipStreamSynchronize(ctx().stream);
        return fail(st);
    }
    unsigned long long c[2] = {0, 0};
    if ((st = S.counters.download(c, 2)) != ORC_OK) return fail(st);  // synchronises: the scratch is freed on return
    g_stats.n_tiles = m->probe_tiles->n_tiles;
    g_stats.slabs = slabs;
    g_stats.visits += (long long)c[0];
    g_stats.waves += (long long)slabs * ((n + kWave - 1) / kWave);
    g_stats.moves += (long long)c[1];
    return P.release();
}

// ------------------------------------------------------------------ sampling
int validate_fields(const SolverState &s, uint32_t mask, int32_t interpolation) {
    if (mask == 0 || (mask & ~kAllFields)) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: mask 0x%x selects nothing or an unknown field", mask);
    if ((mask & (1u << ORC_PROBE_PHI)) && !s.sc.on) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: PHI needs the scalar arm (orc_solver_set_scalar)");
    if (interpolation != ORC_PROBE_CELL && interpolation != ORC_PROBE_LINEAR) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: unknown interpolation %d", interpolation);
    const int recon = s.settings.gradient_reconstruction;
    if (interpolation == ORC_PROBE_LINEAR && recon != ORC_GRAD_GREEN_GAUSS_CELL && recon != ORC_GRAD_LEAST_SQUARES)
        return set_error(ORC_ERR_UNSUPPORTED_SCHEME, "probes: unsupported gradient scheme");  // as the derived fields
    return ORC_OK;
}

int launch_sample(const SolverState &s, const int32_t *cell, const double *off, int64_t n, uint32_t mask, int32_t interpolation, double *out_dev,
                  int *status_dev) {
    const SolverFields F = solver_field_table(s);
    SampleArgs A{F.src[ORC_PROBE_U], F.src[ORC_PROBE_V], F.src[ORC_PROBE_W], F.src[ORC_PROBE_P], (mask & (1u << ORC_PROBE_PHI)) ? F.src[ORC_PROBE_PHI] : nullptr,
                 F.src[ORC_PROBE_MU], F.mu, cell, off, n, out_dev, mask, interpolation == ORC_PROBE_LINEAR ? 1 : 0, s.settings.q1_compat};
    if (s.settings.gradient_reconstruction == ORC_GRAD_LEAST_SQUARES)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_sample_k<true>), dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, s.mesh->dev(), A, status_dev);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(probe_sample_k<false>), dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, s.mesh->dev(), A, status_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int sample_status(int h) {
    if (h == ORC_ERR_SINGULAR_MATRIX) return set_error(h, "probes: singular least-squares system");
    if (h != ORC_OK) return set_error(h, "probes: a face of a probed cell lies in a zone whose type the assembly does not support");
    return ORC_OK;
}

int sample_to_host(const SolverState &s, const int32_t *cell, const double *off, int64_t n, uint32_t mask, int32_t interpolation,
                   const std::vector<int64_t> *order, double *out, DevBuf<int> *keep_status) {
    const size_t len = (size_t)popcount32(mask) * (size_t)n;
    DevBuf<double> dev;
    DevBuf<int> own, &status = keep_status ? *keep_status : own;
    ORC_TRY(dev.alloc(len));
    ORC_TRY(status.alloc(1));
    ORC_TRY(status.zero());
    ORC_TRY(launch_sample(s, cell, off, n, mask, interpolation, dev.p, status.p));
    std::vector<double> h(out && order ? len : 0);
    if (out) ORC_TRY(dev.download(order ? h.data() : out, len));
    int hs = 0;
    ORC_TRY(status.download(&hs, 1));
    ORC_TRY(sample_status(hs));
    for (size_t q = 0; out && order && q < len; q += (size_t)n) unsort(*order, h.data() + q, out + q);
    return ORC_OK;
}

namespace {

int validate_sample(const SolverState &s, const OrcProbes *p, uint32_t mask, int32_t interpolation) {
    if (!p) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: null probe set");
    if (p->mesh != s.mesh) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: the probe set was located in another mesh");
    return validate_fields(s, mask, interpolation);
}

int history_on(const SolverState &s) {
    if (!s.ph.on) return set_error(ORC_ERR_BAD_ARGUMENT, "probe history: the history is off (orc_solver_set_probe_history)");
    return ORC_OK;
}

// the record on its way, if any, joins the history in the caller's point order; its copy was started a step ago, so the wait is over
// before it begins
int history_flush(SolverState &s) {
    ProbeHistory &H = s.ph;
    bool landed = false;
    ORC_TRY(H.raw.wait(&landed));
    if (!landed) return ORC_OK;
    const size_t n = (size_t)H.probes->n, len = (size_t)H.n_fields * n, base = H.values.size();
    int h = 0;
    std::memcpy(&h, H.raw.host.p + len, sizeof(int));
    ORC_TRY(sample_status(h));
    H.values.resize(base + len);
    for (size_t q = 0; q < len; q += n) unsort(H.probes->order, H.raw.host.p + q, H.values.data() + base + q);
    H.times.push_back(H.pending_time);
    return ORC_OK;
}

// one record of the current state, sampled and sent on its way: the record and the status word are two copies
int history_enqueue(SolverState &s, double time) {
    ProbeHistory &H = s.ph;
    const size_t len = (size_t)H.n_fields * (size_t)H.probes->n;
    ORC_TRY(launch_sample(s, H.probes->cell.p, H.probes->off.p, H.probes->n, H.mask, H.interpolation, H.rec.p, H.status.p));
    ORC_TRY(H.raw.copy(0, H.rec.p, len * sizeof(double)));
    ORC_TRY(H.raw.copy(len, H.status.p, sizeof(int)));
    ORC_TRY(H.raw.mark());
    H.pending_time = time;
    return ORC_OK;
}

}  // namespace

int probes_step_dev(SolverState &s) {
    if (!s.ph.on) return ORC_OK;
    ORC_TRY(history_flush(s));  // the previous record: this step's iterations have synchronised the stream since
    return s.ph.due() ? history_enqueue(s, s.time) : ORC_OK;
}

}  // namespace orc

using namespace orc;

extern "C" {

OrcProbes *orc_probes_create(OrcMesh *m, int64_t n_points, const double *xyz, int *status) { return locate(m, n_points, xyz, true, 0, status); }

OrcProbes *orc_debug_probes_locate(OrcMesh *m, int64_t n_points, const double *xyz, int cull, int slabs, int *status) {
    return locate(m, n_points, xyz, cull != 0, slabs, status);
}

void orc_probes_destroy(OrcProbes *p) {
    if (p) (void)hipStreamSynchronize(ctx().stream);
    delete p;
}

int64_t orc_probes_count(const OrcProbes *p) { return p ? p->n : 0; }

int orc_probes_get(const OrcProbes *p, int64_t *cell, int32_t *status, int32_t *steps, int32_t *zone, double *excess) {
    ORC_TRY(ensure_init());
    if (!p) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: null probe set");
    const size_t n = (size_t)p->n;
    std::vector<int32_t> h(n);
    if (cell) {
        ORC_TRY(p->cell.download(h.data(), n));
        for (size_t k = 0; k < n; ++k) cell[p->order[k]] = orc_cell_id(*p->mesh, h[k]);
    }
    const DevBuf<int32_t> *src[3] = {&p->status, &p->steps, &p->zone};
    int32_t *dst[3] = {status, steps, zone};
    for (int q = 0; q < 3; ++q) {
        if (!dst[q]) continue;
        ORC_TRY(src[q]->download(h.data(), n));
        unsort(p->order, h.data(), dst[q]);
    }
    if (excess) {
        std::vector<double> e(n);
        ORC_TRY(p->excess.download(e.data(), n));
        unsort(p->order, e.data(), excess);
    }
    return ORC_OK;
}

int orc_solver_sample_probes(OrcSolver *s, const OrcProbes *p, uint32_t field_mask, int32_t interpolation, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "probes: null argument");
    SolverState &st = s->st;
    ORC_TRY(validate_sample(st, p, field_mask, interpolation));
    return sample_to_host(st, p->cell.p, p->off.p, p->n, field_mask, interpolation, &p->order, out);
}

int orc_solver_set_probe_history(OrcSolver *s, const OrcProbes *p, uint32_t field_mask, int32_t interpolation, uint64_t interval) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!p) {  // off: advance launches nothing of the history from here on
        st.ph.clear();
        return ORC_OK;
    }
    ORC_TRY(validate_sample(st, p, field_mask, interpolation));
    if (interval == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "probe history: interval must be at least 1");
    // one record of the current state first: a zone type the assembly refuses or a singular system is refused here, nothing changed
    ProbeHistory H;
    ORC_TRY(sample_to_host(st, p->cell.p, p->off.p, p->n, field_mask, interpolation, nullptr, nullptr, &H.status));
    H.n_fields = popcount32(field_mask);
    const size_t len = (size_t)H.n_fields * (size_t)p->n;
    ORC_TRY(H.rec.alloc(len));
    ORC_TRY(H.raw.create(len + 1, "probe history"));
    H.probes = p;
    H.mask = field_mask;
    H.interpolation = interpolation;
    H.interval = interval;
    H.on = true;
    st.ph.clear();
    st.ph = std::move(H);
    return ORC_OK;
}

int orc_solver_record_probes(OrcSolver *s, double tag) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(history_on(st));
    ORC_TRY(history_flush(st));
    ORC_TRY(history_enqueue(st, tag));
    return history_flush(st);
}

int64_t orc_solver_probe_history_count(OrcSolver *s) {
    if (ensure_init() != ORC_OK) return -1;
    if (!s) { (void)set_error(ORC_ERR_BAD_ARGUMENT, "null solver"); return -1; }
    if (history_on(s->st) != ORC_OK || history_flush(s->st) != ORC_OK) return -1;
    return (int64_t)s->st.ph.times.size();
}

int orc_solver_probe_history(OrcSolver *s, uint64_t first, uint64_t count, double *times, double *out) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(history_on(st));
    ORC_TRY(history_flush(st));
    const ProbeHistory &H = st.ph;
    ORC_TRY(history_range("probe history", first, count, H.times.size()));
    const size_t len = (size_t)H.n_fields * (size_t)H.probes->n;
    if (times) std::copy(H.times.begin() + (ptrdiff_t)first, H.times.begin() + (ptrdiff_t)(first + count), times);
    if (out) std::copy(H.values.begin() + (ptrdiff_t)(first * len), H.values.begin() + (ptrdiff_t)((first + count) * len), out);
    return ORC_OK;
}

int orc_debug_probe_search(long long out[6], int reset) {
    if (!out) return set_error(ORC_ERR_BAD_ARGUMENT, "probe search: null argument");
    out[0] = kProbeTile; out[1] = g_stats.n_tiles; out[2] = g_stats.visits; out[3] = g_stats.waves; out[4] = g_stats.slabs; out[5] = g_stats.moves;
    if (reset) g_stats = ProbeStats();
    return ORC_OK;
}

int orc_bench_probe_locate(OrcMesh *m, const OrcProbes *p, int cull, int reps, double avg_ms[2]) {
    ORC_TRY(ensure_init());
    if (!m || !p || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench probe locate: null argument");
    if (p->mesh != m) return set_error(ORC_ERR_BAD_ARGUMENT, "bench probe locate: the probe set was located in another mesh");
    if (reps < 1) reps = 1;
    ORC_TRY(ensure_tiles(*m));
    const int slabs = choose_slabs(*m, p->n, 0);
    Scratch S;          // the passes write here: the probe set keeps its bits
    OrcProbes scratch;
    ORC_TRY(alloc_scratch(p->n, slabs, S));
    ORC_TRY(alloc_results(p->n, scratch));
    int status = ORC_OK;
    for (int pass = 0; pass < 2 && status == ORC_OK; ++pass) {  // the warm call of the walk starts from the search's cells
        float ms = 0.f;
        status = timed(reps, [&] { return pass == 0 ? launch_search(*m, *p, cull != 0, slabs, S) : launch_walk(*m, *p, scratch, S); }, &ms,
                       "timing the probe passes failed");
        avg_ms[pass] = (double)ms;
    }
    unsigned long long c[2] = {0, 0};
    ORC_TRY(S.counters.download(c, 2));  // synchronises: the scratch is freed on return
    ORC_TRY(status);
    g_stats.n_tiles = m->probe_tiles->n_tiles;
    g_stats.slabs = slabs;
    g_stats.visits += (long long)c[0];
    g_stats.waves += (long long)(reps + 1) * slabs * ((p->n + kWave - 1) / kWave);
    g_stats.moves += (long long)c[1];
    return ORC_OK;
}

}  // extern "C"
