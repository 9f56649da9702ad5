// var_diffusion.hpp — what the two variable-coefficient diffusion rebuilds share: diffusion_var_k (viscosity.hip, the momentum side) and
// scalar_diffusion_var_k (scalar.hip, the scalar side) walk the owned rows the same way and form a face's coefficient from its two
// cells by the same formula (orc_types.h OrcViscosityFace).  Device code only.
#pragma once

#include "common.hpp"

namespace orc {

// Blocks of kBlock cells; XCD g (workgroups g, g + 8, ...) walks a contiguous eighth of the blocks, so that the two cells of a face
// mostly share one L2 (momentum_k, scalar_k, derived_cell_k).  A grid that is no multiple of 8 strides plainly.
struct BlockWalk {
    int vb, vb_end, vb_step;
};
__device__ __forceinline__ BlockWalk block_walk(int n_items) {
    const int n_blk = (n_items + kBlock - 1) / kBlock;
    BlockWalk w{(int)blockIdx.x, n_blk, (int)gridDim.x};
    if ((gridDim.x & 7) == 0 && gridDim.x >= 8) {
        const int per = (n_blk + 7) / 8;
        const int xcd = blockIdx.x & 7;
        w.vb = xcd * per + (int)(blockIdx.x >> 3);
        w.vb_end = (xcd + 1) * per < n_blk ? (xcd + 1) * per : n_blk;
        w.vb_step = gridDim.x >> 3;
    }
    return w;
}

// symmetric in its two cells, and exactly mu where both hold mu: (mu + mu) * 0.5 = mu, mu / mu = 1, mu * 1 = mu
__device__ __forceinline__ double face_viscosity(int harmonic, double mu_p, double mu_n) {
    const double lo = fmin(mu_p, mu_n), hi = fmax(mu_p, mu_n);
    const double mean = (lo + hi) * 0.5;
    return harmonic ? lo * (hi / mean) : mean;
}

}  // namespace orc
