// sphere_cull.hpp — the bounding spheres and the skip test of the two fp64 nearest-centroid searches: wall_search_k (wall_distance.hip,
// cells against wall faces) and probe_search_k (probes.hip, points against cells).  Both walk a table of centroids in tiles of
// consecutive entries, carry per lane the smallest squared distance s found so far, and leave a tile out when no lane of the wave can
// improve or tie inside it.  Device code only; one expression each, so both searches round alike.
#pragma once
#include "common.hpp"

#ifdef __HIPCC__
namespace orc {

// the safety factors of the skip: every rounding of the bound is below 2^-50 relative, the factors move it by 2^-40
constexpr double kWiden = 1. + 0x1p-40, kShrink = 1. - 0x1p-40;

// tile t = the entries [t kTile, min((t + 1) kTile, W)) of the SoA centroids x, y, z: centre = the middle of the centroids' bounding
// box, radius = the largest computed centre-to-centroid distance times kWiden (each distance is within 2^-51 relative of the true one:
// never too small).  tiles: [4][n_tiles] = centre x, y, z and the widened radius.
template <int kTile>
__global__ __launch_bounds__(kBlock) void sphere_tiles_k(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                         int64_t W, int64_t n_tiles, double *__restrict__ tiles) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t j0 = t * kTile, j1 = j0 + kTile < W ? j0 + kTile : W;
    const double *tab[3] = {x, y, z};
    double lo[3], hi[3];
    for (int q = 0; q < 3; ++q) lo[q] = hi[q] = tab[q][j0];
    for (int64_t j = j0 + 1; j < j1; ++j)
        for (int q = 0; q < 3; ++q) {
            const double v = tab[q][j];
            lo[q] = fmin(lo[q], v); hi[q] = fmax(hi[q], v);
        }
    double c[3];
    for (int q = 0; q < 3; ++q) c[q] = lo[q] + (hi[q] - lo[q]) * 0.5;
    double r = 0.;
    for (int64_t j = j0; j < j1; ++j) {
        const double dx = x[j] - c[0], dy = y[j] - c[1], dz = z[j] - c[2];
        r = fmax(r, sqrt((dx * dx + dy * dy) + dz * dz));
    }
    tiles[t] = c[0]; tiles[n_tiles + t] = c[1]; tiles[2 * n_tiles + t] = c[2];
    tiles[3 * n_tiles + t] = r * kWiden;
}

// The skip of a tile with centre c, radius R for a lane at x with best value b: every entry of the tile lies within R of c, so its s is
// at least (|x - c| - R)^2; the tile cannot improve or tie when |x - c| > sqrt(b) + R, tested as q kShrink > (sb + R)^2 with
// q = |x - c|^2 as computed, sb = sqrt(b) kWiden and R widened by sphere_tiles_k.  Roundings: q, the computed s of an entry and the
// square are each within 2^-50 relative; the three factors of 2^-40 dominate them, so a skipped tile holds no entry with computed
// s <= b.  A NaN anywhere makes the comparison false: the tile is entered.
__device__ __forceinline__ double sphere_reach(double best_s) { return sqrt(best_s) * kWiden; }
__device__ __forceinline__ double sphere_q(double x, double y, double z, double cx, double cy, double cz) {
    const double dx = x - cx, dy = y - cy, dz = z - cz;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ bool sphere_skip(double q, double sb, double R) {
    const double reach = sb + R;
    return q * kShrink > reach * reach;
}

}  // namespace orc
#endif
