// wall_pair_rate.hip — the chip's own rate for the instruction mix of wall_search_k's inner loop (orc_amd/csrc/wall_distance.hip), with
// no memory in it: every lane keeps a point (x, y, z) and its best pair (s, d) in registers, the eight table entries are kernel arguments
// (wave-uniform, in scalar registers), and the loop is wall_entry's — three subtractions, three multiplies, two additions, one compare,
// and under the branch the plane distance.  The point moves a little away from all entries after every round of eight, so that nothing is
// loop-invariant and, as in the search once a wave has seen its nearest tile, the branch is not taken after the first round.
// What the un-culled search achieves in pairs per second is reported as a fraction of this figure (scripts/wall_distance_measure.py).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off wall_pair_rate.hip -o wall_pair_rate
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

struct Entries {
    double c[8][3], n[8][3];
};

__global__ __launch_bounds__(256) void pairs_k(Entries E, int rounds, double step, double *sink) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double x = 1. + 1e-3 * (i & 1023), y = 0.5 + 1e-3 * ((i >> 10) & 1023), z = 1. + 1e-3 * (i >> 20);
    double bs = INFINITY, bd = INFINITY;
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double rx = x - E.c[k][0], ry = y - E.c[k][1], rz = z - E.c[k][2];
            const double s = (rx * rx + ry * ry) + rz * rz;
            if (s <= bs) {
                const double d = fabs((rx * E.n[k][0] + ry * E.n[k][1]) + rz * E.n[k][2]);
                bd = s < bs ? d : fmin(bd, d);
                bs = s;
            }
        }
        x += step; y += step; z += step;
    }
    if (bs == -1.) sink[0] = bd;  // never true: keeps the loop alive
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 20000;
    Entries E;
    for (int k = 0; k < 8; ++k) {
        E.c[k][0] = 1e-3 * k; E.c[k][1] = 0.; E.c[k][2] = 5e-4 * k;
        E.n[k][0] = 0.; E.n[k][1] = 1.; E.n[k][2] = 0.;
    }
    double *sink;
    CK(hipMalloc(&sink, sizeof(double)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int wgs_per_cu : {2, 4, 8}) {
        const int grid = 256 * wgs_per_cu;
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {  // the first launch is the warm-up
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(pairs_k, dim3(grid), dim3(256), 0, 0, E, rounds, 1e-9, sink);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms = 0.f;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        const double pairs = (double)grid * 256 * rounds * 8;
        printf("{\"microbench\": \"wall_pair_rate\", \"workgroups\": %d, \"rounds\": %d, \"ms\": %.3f, \"pairs_per_s\": %.4e}\n", grid, rounds, best,
               pairs / (best * 1e-3));
    }
    return 0;
}
