// wall_distance.hip — the distance of every cell to the nearest wall (new-build extension; ORC has no such field).  DESIGN.md §3 "Wall
// distance and wall damping" has the definition: the wall faces are the boundary faces of owned cells in the zones of the wall mask;
// for cell P and wall face f
//     r = x_P - x_f      s_f = (r.x r.x + r.y r.y) + r.z r.z      d_f = fabs((r.x n.x + r.y n.y) + r.z n.z)
//     d_P = min{ d_f : s_f == min_g s_g }
// i.e. the plane distance to the face with the nearest centroid, the smallest one among exact ties: a function of the SET of wall faces,
// so that neither the order of the table, nor the cell numbering, nor a partition changes a bit.
//
//   the wall table (once per mesh and mask, on the device, deterministic by construction: no atomic append)
//     wall_count_k    one thread per segment of kWallSegment consecutive faces: its wall faces
//     (host)          exclusive scan of the segment counts
//     wall_place_k    the same walk: the wall faces, ascending in face id, into the SoA table [6][W] at this rank's offset
//     (partitioned)   the per-rank counts, then the zero-filled table with every rank's slice, summed over the ranks: x + 0 is exact
//     sphere_tiles_k  (sphere_cull.hpp) one thread per tile of kWallTile consecutive entries: a sphere around the tile's centroids
//   the search (one launch, fp64, compute-bound: N W pairs un-culled)
//     wall_search_k   one lane per owned cell; the wave walks the table, whose entry is wave-uniform and arrives through scalar loads.
//                     Culled (the default): the tile whose centre is nearest to the wave's first cell seeds the best value, then a
//                     tile is entered only if some lane's lower bound of s over the tile's sphere does not exceed its best value.
//                     No float atomics; one integer atomicAdd per wave counts the tiles it entered (orc_debug_wall_search).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "sphere_cull.hpp"

namespace orc {

constexpr int kWallTile = 64;      // table entries per tile: one bounding sphere, one skip decision per wave
constexpr int kWallSegment = 256;   // consecutive faces one thread of the table build walks

namespace {

struct WallStats {
    long long n_wall = 0, n_tiles = 0, visits = 0, waves = 0;
};
WallStats g_stats;

__device__ __forceinline__ bool wall_face(const MeshDev &M, const int32_t *__restrict__ mask, int64_t f) {
    return M.c1[f] < 0 && M.c0[f] < M.n_own && mask[M.fzone[f]] != 0;
}

// ------------------------------------------------------------------ the wall table
__global__ __launch_bounds__(kBlock) void wall_count_k(MeshDev M, const int32_t *__restrict__ mask, int64_t S, int32_t *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return;
    const int64_t f0 = t * kWallSegment, f1 = f0 + kWallSegment < M.n_faces ? f0 + kWallSegment : M.n_faces;
    int32_t n = 0;
    for (int64_t f = f0; f < f1; ++f) n += wall_face(M, mask, f) ? 1 : 0;
    cnt[t] = n;
}

// off[t]: the first slot of segment t among this rank's wall faces; the rank's slice starts at `base` of the W entries per component.
// The walk and its predicate are wall_count_k's, so every slot lies in [off[t], off[t + 1]) and below n_local; one that does not is
// not written and raises *bad, which fails the build.
__global__ __launch_bounds__(kBlock) void wall_place_k(MeshDev M, const int32_t *__restrict__ mask, int64_t S, const int64_t *__restrict__ off,
                                                       int64_t n_local, int64_t base, int64_t W, double *__restrict__ tab, int *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return;
    const int64_t f0 = t * kWallSegment, f1 = f0 + kWallSegment < M.n_faces ? f0 + kWallSegment : M.n_faces;
    int64_t pos = off[t];
    for (int64_t f = f0; f < f1; ++f) {
        if (!wall_face(M, mask, f)) continue;
        if (pos >= 0 && pos < n_local) {
            const int64_t j = base + pos;
            tab[j] = M.fcx[f]; tab[W + j] = M.fcy[f]; tab[2 * W + j] = M.fcz[f];
            tab[3 * W + j] = M.nx[f]; tab[4 * W + j] = M.ny[f]; tab[5 * W + j] = M.nz[f];
        } else {
            atomicCAS(bad, 0, 1);
        }
        ++pos;
    }
}

// ------------------------------------------------------------------ the search
struct WallBest {
    double s, d;  // the smallest s so far and the smallest d_f among the faces that reach it
};

// one table entry against one cell: THE operator order of the definition.  j is wave-uniform: six scalar loads, no LDS.
__device__ __forceinline__ void wall_entry(const double *__restrict__ tab, int64_t W, int64_t j, double x, double y, double z, WallBest &b) {
    const double rx = x - tab[j], ry = y - tab[W + j], rz = z - tab[2 * W + j];
    const double s = (rx * rx + ry * ry) + rz * rz;
    if (s <= b.s) {
        const double d = fabs((rx * tab[3 * W + j] + ry * tab[4 * W + j]) + rz * tab[5 * W + j]);
        b.d = s < b.s ? d : fmin(b.d, d);
        b.s = s;
    }
}

__device__ __forceinline__ void wall_tile(const double *__restrict__ tab, int64_t W, int64_t t, double x, double y, double z, WallBest &b) {
    const int64_t j0 = t * kWallTile;
    if (j0 + kWallTile <= W) {
#pragma unroll 8
        for (int k = 0; k < kWallTile; ++k) wall_entry(tab, W, j0 + k, x, y, z, b);
    } else {
        for (int64_t j = j0; j < W; ++j) wall_entry(tab, W, j, x, y, z, b);
    }
}

// Lane i of a wave owns cell 64 wave + i; the idle lanes of the last wave repeat the last owned cell and write nothing, so that every
// vote of the wave is a vote of cells.  Any order of the walk gives the same bits (a minimum with a tie rule), so the culled search may
// start where it likes and leave out what cannot matter.
// The skip of a tile is sphere_skip (sphere_cull.hpp, with its reasoning): a skipped tile holds no entry with computed s <= b.
template <bool kCull>
__global__ __launch_bounds__(kBlock) void wall_search_k(MeshDev M, const double *__restrict__ tab, int64_t W, const double *__restrict__ tiles,
                                                        int64_t n_tiles, double *__restrict__ d, unsigned long long *__restrict__ visits) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    if (c - lane >= M.n_own) return;  // the whole wave lies past the owned cells
    const int64_t cc = c < M.n_own ? c : M.n_own - 1;
    const double x = M.ccx[cc], y = M.ccy[cc], z = M.ccz[cc];
    WallBest b{INFINITY, INFINITY};
    unsigned long long entered = 0;
    if (!kCull) {
        for (int64_t t = 0; t < n_tiles; ++t) wall_tile(tab, W, t, x, y, z, b);
        entered = (unsigned long long)n_tiles;
    } else if (n_tiles > 0) {
        const double *tx = tiles, *ty = tiles + n_tiles, *tz = tiles + 2 * n_tiles, *tr = tiles + 3 * n_tiles;
        // the seed: the tile whose centre is nearest to the wave's first cell (the cells of a wave are neighbours)
        int near = 0;
        double near_q = INFINITY;
        for (int64_t t = 0; t < n_tiles; ++t) {
            const double dx = x - tx[t], dy = y - ty[t], dz = z - tz[t];
            const double q = (dx * dx + dy * dy) + dz * dz;
            if (q < near_q) { near_q = q; near = (int)t; }
        }
        const int64_t seed = __builtin_amdgcn_readfirstlane(near);
        wall_tile(tab, W, seed, x, y, z, b);
        entered = 1;
        double sb = sphere_reach(b.s);
        for (int64_t t = 0; t < n_tiles; ++t) {
            if (t == seed) continue;
            const bool skip = sphere_skip(sphere_q(x, y, z, tx[t], ty[t], tz[t]), sb, tr[t]);
            if (!__any(!skip)) continue;
            wall_tile(tab, W, t, x, y, z, b);
            sb = sphere_reach(b.s);
            ++entered;
        }
    }
    if (c < M.n_own) d[c] = b.d;
    if (lane == 0) atomicAdd(visits, entered);
}

// ====================================================================== host side
int resolve_mask(OrcMesh &m, const int32_t *zone_is_wall, std::vector<int32_t> &mask) {
    const size_t Z = (size_t)m.n_zones;
    mask.assign(Z, 0);
    if (zone_is_wall) {
        for (size_t z = 0; z < Z; ++z) mask[z] = zone_is_wall[z] != 0 ? 1 : 0;
        return ORC_OK;
    }
    std::vector<int32_t> zt(Z);
    if (Z) ORC_TRY(m.ztype.download(zt.data(), Z));
    for (size_t z = 0; z < Z; ++z) mask[z] = zt[z] == ORC_BC_WALL ? 1 : 0;
    return ORC_OK;
}

// the table of `mask` and its tiles into X (X.d is left alone)
int build_table(OrcMesh &m, const std::vector<int32_t> &mask, WallDistance &X) {
    const int64_t S = (m.n_faces + kWallSegment - 1) / kWallSegment;
    if (S / kBlock + 1 >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "wall distance: mesh too large");
    const int grid = (int)std::max<int64_t>((S + kBlock - 1) / kBlock, 1);
    DevBuf<int32_t> d_mask, cnt;
    DevBuf<int64_t> off;
    if (mask.empty()) ORC_TRY(d_mask.alloc(1));
    else ORC_TRY(d_mask.upload(mask.data(), mask.size()));
    ORC_TRY(cnt.alloc((size_t)std::max<int64_t>(S, 1)));
    hipLaunchKernelGGL(wall_count_k, dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), d_mask.p, S, cnt.p);
    ORC_HIP(hipGetLastError());
    std::vector<int32_t> h_cnt((size_t)S);
    ORC_TRY(cnt.download(h_cnt.data(), (size_t)S));
    std::vector<int64_t> h_off((size_t)S + 1, 0);
    for (int64_t t = 0; t < S; ++t) h_off[(size_t)t + 1] = h_off[(size_t)t] + h_cnt[(size_t)t];
    const int64_t n_local = h_off[(size_t)S];
    if (n_local < 0 || n_local > m.n_faces) return set_error(ORC_ERR_HIP, "wall distance: inconsistent wall-face count %lld", (long long)n_local);
    // every rank needs all ranks' wall faces: the counts first, then the slices
    const bool gather = m.halo.active() && ctx().world > 1;
    int64_t base = 0, W = n_local;
    if (gather) {
        const int world = ctx().world, rank = ctx().rank;
        std::vector<double> h((size_t)world, 0.);
        h[(size_t)rank] = (double)n_local;
        DevBuf<double> counts;
        ORC_TRY(counts.upload(h.data(), (size_t)world));
        ORC_TRY(comm_allreduce_sum(counts.p, world));
        ORC_TRY(counts.download(h.data(), (size_t)world));
        W = 0;
        for (int r = 0; r < world; ++r) {
            if (r == rank) base = W;
            W += (int64_t)h[(size_t)r];
        }
    }
    if (6 * W >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "wall distance: %lld wall faces are too many", (long long)W);
    X.mask = mask;
    X.n_wall = W;
    X.n_tiles = (W + kWallTile - 1) / kWallTile;
    ORC_TRY(X.table.alloc((size_t)std::max<int64_t>(6 * W, 1)));
    ORC_TRY(X.table.zero());
    ORC_TRY(X.tiles.alloc((size_t)std::max<int64_t>(4 * X.n_tiles, 1)));
    if (n_local > 0) {
        DevBuf<int> bad;
        ORC_TRY(bad.alloc(1));
        ORC_TRY(bad.zero());
        ORC_TRY(off.upload(h_off.data(), (size_t)S));
        hipLaunchKernelGGL(wall_place_k, dim3(grid), dim3(kBlock), 0, ctx().stream, m.dev(), d_mask.p, S, off.p, n_local, base, W, X.table.p, bad.p);
        ORC_HIP(hipGetLastError());
        int h_bad = 0;
        ORC_TRY(bad.download(&h_bad, 1));
        if (h_bad) return set_error(ORC_ERR_HIP, "wall distance: placement disagrees with the count");
    }
    if (gather && W > 0) ORC_TRY(comm_allreduce_sum(X.table.p, (int)(6 * W)));
    if (X.n_tiles > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(sphere_tiles_k<kWallTile>), dim3((unsigned)((X.n_tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx().stream,
                           X.table.p, X.table.p + W, X.table.p + 2 * W, W, X.n_tiles, X.tiles.p);
        ORC_HIP(hipGetLastError());
    }
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // d_mask, cnt and off are freed on return
    return ORC_OK;
}

int launch_search(OrcMesh &m, const WallDistance &X, bool cull, double *d_dev, unsigned long long *visits) {
    if (m.n_own <= 0) return ORC_OK;
    const int64_t blocks = (m.n_own + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "wall distance: mesh too large");
    if (cull)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(wall_search_k<true>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx().stream, m.dev(), X.table.p, X.n_wall,
                           X.tiles.p, X.n_tiles, d_dev, visits);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(wall_search_k<false>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx().stream, m.dev(), X.table.p, X.n_wall,
                           X.tiles.p, X.n_tiles, d_dev, visits);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// `launches` searches of X into d_dev ([n_cells], ghost entries zeroed first), the counters of orc_debug_wall_search updated
int search(OrcMesh &m, const WallDistance &X, bool cull, double *d_dev, int launches, double *avg_ms) {
    DevBuf<unsigned long long> visits;
    ORC_TRY(visits.alloc(1));
    ORC_TRY(visits.zero());
    if (m.n_cells > 0) ORC_HIP(hipMemsetAsync(d_dev, 0, (size_t)m.n_cells * sizeof(double), ctx().stream));
    int status = ORC_OK;
    if (avg_ms) {
        hipEvent_t e0, e1;
        ORC_HIP(hipEventCreate(&e0));
        ORC_HIP(hipEventCreate(&e1));
        status = launch_search(m, X, cull, d_dev, visits.p);  // warm-up
        if (status == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) status = set_error(ORC_ERR_HIP, "hipEventRecord failed");
        for (int i = 0; i < launches && status == ORC_OK; ++i) status = launch_search(m, X, cull, d_dev, visits.p);
        float ms = 0.f;
        if (status == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                                 hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
            status = set_error(ORC_ERR_HIP, "timing the wall search failed");
        *avg_ms = (double)ms / launches;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        ++launches;
    } else {
        for (int i = 0; i < launches && status == ORC_OK; ++i) status = launch_search(m, X, cull, d_dev, visits.p);
    }
    unsigned long long h = 0;
    ORC_TRY(visits.download(&h, 1));  // synchronises: visits is freed on return
    ORC_TRY(status);
    g_stats.n_wall = X.n_wall;
    g_stats.n_tiles = X.n_tiles;
    g_stats.visits += (long long)h;
    g_stats.waves += (long long)launches * ((m.n_own + kWave - 1) / kWave);
    return ORC_OK;
}

// the mesh's cached field of `mask`, built and searched when the cache holds another mask or nothing
int ensure_field(OrcMesh &m, const std::vector<int32_t> &mask, bool from_types) {
    if (m.wall && m.wall->searched && m.wall->mask == mask) {
        m.wall->from_types = m.wall->from_types || from_types;
        return ORC_OK;
    }
    m.wall.reset();
    std::unique_ptr<WallDistance> X(new WallDistance());
    ORC_TRY(build_table(m, mask, *X));
    ORC_TRY(X->d.alloc((size_t)std::max<int64_t>(m.n_cells, 1)));
    ORC_TRY(search(m, *X, true, X->d.p, 1, nullptr));
    X->searched = true;
    X->from_types = from_types;
    m.wall = std::move(X);
    return ORC_OK;
}

bool finite_all(std::initializer_list<double> xs) {
    for (double x : xs)
        if (!std::isfinite(x)) return false;
    return true;
}

}  // namespace

int wall_damping_validate(const OrcWallDamping &w) {
    if (w.mode < ORC_WALL_DAMPING_NONE || w.mode > ORC_WALL_DAMPING_VAN_DRIEST) return set_error(ORC_ERR_BAD_ARGUMENT, "wall damping: unknown mode %d", w.mode);
    if (w.reserved0 != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "wall damping: reserved0 must be 0");
    if (!finite_all({w.kappa, w.a_plus, w.u_tau})) return set_error(ORC_ERR_BAD_ARGUMENT, "wall damping: every parameter must be finite");
    if (w.mode == ORC_WALL_DAMPING_MIN && !(w.kappa > 0.)) return set_error(ORC_ERR_BAD_ARGUMENT, "wall damping: MIN needs kappa > 0");
    if (w.mode == ORC_WALL_DAMPING_VAN_DRIEST && (!(w.a_plus > 0.) || !(w.u_tau > 0.)))
        return set_error(ORC_ERR_BAD_ARGUMENT, "wall damping: VAN_DRIEST needs a_plus > 0 and u_tau > 0");
    return ORC_OK;
}

int wall_distance_default(OrcMesh &m, const double **d_dev) {
    if (!(m.wall && m.wall->searched && m.wall->from_types)) {
        std::vector<int32_t> mask;
        ORC_TRY(resolve_mask(m, nullptr, mask));
        ORC_TRY(ensure_field(m, mask, true));
    }
    *d_dev = m.wall->d.p;
    return ORC_OK;
}

void wall_zones_changed(OrcMesh &m, const int32_t *zone_type) {
    if (!m.wall || !m.wall->from_types) return;  // a field of an explicit mask does not depend on the zone types
    for (size_t z = 0; z < m.wall->mask.size(); ++z)
        if ((zone_type[z] == ORC_BC_WALL ? 1 : 0) != m.wall->mask[z]) {
            (void)hipStreamSynchronize(ctx().stream);
            m.wall.reset();
            return;
        }
}

}  // namespace orc

using namespace orc;

extern "C" {

static_assert(sizeof(OrcWallDamping) == 32 && offsetof(OrcWallDamping, mode) == 0 && offsetof(OrcWallDamping, reserved0) == 4 &&
                  offsetof(OrcWallDamping, kappa) == 8 && offsetof(OrcWallDamping, a_plus) == 16 && offsetof(OrcWallDamping, u_tau) == 24,
              "OrcWallDamping is part of the ABI (orc_amd/settings.py WallDamping mirrors it)");

int orc_mesh_wall_distance(OrcMesh *m, const int32_t *zone_is_wall, double *d) {
    ORC_TRY(ensure_init());
    if (!m || !d) return set_error(ORC_ERR_BAD_ARGUMENT, "wall distance: null argument");
    std::vector<int32_t> mask;
    ORC_TRY(resolve_mask(*m, zone_is_wall, mask));
    ORC_TRY(ensure_field(*m, mask, zone_is_wall == nullptr));
    return download_cells(*m, m->wall->d.p, d);
}

int orc_debug_wall_distance(OrcMesh *m, const int32_t *zone_is_wall, int cull, double *d) {
    ORC_TRY(ensure_init());
    if (!m || !d) return set_error(ORC_ERR_BAD_ARGUMENT, "wall distance: null argument");
    std::vector<int32_t> mask;
    ORC_TRY(resolve_mask(*m, zone_is_wall, mask));
    WallDistance X;
    ORC_TRY(build_table(*m, mask, X));
    ORC_TRY(X.d.alloc((size_t)std::max<int64_t>(m->n_cells, 1)));
    ORC_TRY(search(*m, X, cull != 0, X.d.p, 1, nullptr));
    return download_cells(*m, X.d.p, d);
}

int orc_debug_wall_search(long long out[5], int reset) {
    if (!out) return set_error(ORC_ERR_BAD_ARGUMENT, "wall search: null argument");
    out[0] = g_stats.n_wall; out[1] = kWallTile; out[2] = g_stats.n_tiles; out[3] = g_stats.visits; out[4] = g_stats.waves;
    if (reset) g_stats = WallStats();
    return ORC_OK;
}

int orc_bench_wall_distance(OrcMesh *m, int cull, int reps, double *avg_ms) {
    ORC_TRY(ensure_init());
    if (!m || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench wall distance: null argument");
    if (reps < 1) reps = 1;
    const double *unused = nullptr;
    ORC_TRY(wall_distance_default(*m, &unused));  // the table of the default mask, built if need be
    DevBuf<double> scratch;                       // the searches write here: the cached field keeps its bits
    ORC_TRY(scratch.alloc((size_t)std::max<int64_t>(m->n_cells, 1)));
    return search(*m, *m->wall, cull != 0, scratch.p, reps, avg_ms);
}

void orc_wall_damping_default(OrcWallDamping *w) {
    if (!w) return;
    *w = OrcWallDamping{};
    w->mode = ORC_WALL_DAMPING_NONE;
    w->kappa = 0.41;
    w->a_plus = 26.;
    w->u_tau = 0.;
}

int orc_solver_get_wall_damping(OrcSolver *s, OrcWallDamping *w, int32_t *enabled) {
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    if (w) *w = s->st.vis.wd;
    if (enabled) *enabled = s->st.vis.wd.mode != ORC_WALL_DAMPING_NONE ? 1 : 0;
    return ORC_OK;
}

}  // extern "C"
