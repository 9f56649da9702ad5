// sell.hip — the SELL-64 image of a CSR pattern, value import / export, and the plain vector kernels of the solvers (fill, copy, inverse
// diagonal, row scaling, interleaving of three systems).  Reference: src/linear_algebra.rs:159-166 (p_inv and p_inv * b).
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "linalg_kernels.hpp"

namespace orc {

// ------------------------------------------------------------------ SELL build / import / export
int sell_from_csr_host(int64_t n, int64_t ncols, const int64_t *row_ptr, const int64_t *col, SellMatrix &out) {
    if (ncols < n) ncols = n;
    if (n < 0) return set_error(ORC_ERR_BAD_ARGUMENT, "negative row count");
    const int64_t nnz = n > 0 ? row_ptr[n] : 0;
    const int32_t n_slices = (int32_t)((n + 63) / 64);
    std::vector<int64_t> slice_ptr((size_t)n_slices + 1, 0);
    std::vector<int32_t> row_len((size_t)std::max<int64_t>(n, 1));
    for (int32_t s = 0; s < n_slices; ++s) {
        int64_t w = 0;
        for (int64_t r = (int64_t)s * 64; r < std::min<int64_t>(n, (int64_t)s * 64 + 64); ++r) w = std::max(w, row_ptr[r + 1] - row_ptr[r]);
        slice_ptr[s + 1] = slice_ptr[s] + w * 64;
    }
    const int64_t padded = slice_ptr[n_slices];
    if (padded >= (int64_t)1 << 31) return set_error(ORC_ERR_BAD_ARGUMENT, "matrix too large for 32-bit element offsets (%lld)", (long long)padded);
    std::vector<int32_t> scol((size_t)std::max<int64_t>(padded, 1), 0), diag((size_t)std::max<int64_t>(n, 1), -1);
    bool symmetric = true;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t b = row_ptr[r], e = row_ptr[r + 1];
        row_len[r] = (int32_t)(e - b);
        const int64_t base = slice_ptr[r >> 6] + (r & 63);
        for (int64_t k = 0; k < e - b; ++k) {
            const int64_t c = col[b + k];
            if (c < 0 || c >= ncols) return set_error(ORC_ERR_BAD_ARGUMENT, "column index out of range");
            if (k > 0 && col[b + k - 1] >= c) return set_error(ORC_ERR_BAD_ARGUMENT, "CSR columns must be strictly ascending per row");
            scol[base + k * 64] = (int32_t)c;
            if (c == r) diag[r] = (int32_t)(base + k * 64);
            if (symmetric && c != r && c < n) {
                const int64_t *lo = col + row_ptr[c], *hi = col + row_ptr[c + 1];
                const int64_t *it = std::lower_bound(lo, hi, r);
                if (it == hi || *it != r) symmetric = false;
            }
        }
        // padding slots point at the row itself (never dereferenced: guarded by row_len)
        const int64_t width = (slice_ptr[(r >> 6) + 1] - slice_ptr[r >> 6]) >> 6;
        for (int64_t k = e - b; k < width; ++k) scol[base + k * 64] = (int32_t)r;
    }
    out.n = n; out.ncols = ncols; out.nnz = nnz; out.padded = padded; out.n_slices = n_slices; out.symmetric = symmetric;
    out.ragged = (double)padded > 1.08 * (double)std::max<int64_t>(nnz, 1) ? (padded < 24 * std::max<int64_t>(n, 1) ? 2 : 1) : 0;
    ORC_TRY(out.slice_ptr.upload(slice_ptr.data(), slice_ptr.size()));
    ORC_TRY(out.row_len.upload(row_len.data(), (size_t)n));
    ORC_TRY(out.col.upload(scol.data(), (size_t)padded));
    // narrow column image (SellDev): per slice and depth the smallest column among the rows that reach that depth + 16-bit offsets
    const bool narrow_on = cfg().spmv_narrow_cols;
    if (narrow_on && padded > 0) {
        std::vector<uint16_t> c16((size_t)padded, 0);
        std::vector<int32_t> cbase((size_t)(padded / 64), 0);
        bool all_fit = true;
        int64_t wide_slices = 0;
        const bool count_wide = cfg().trace;
        for (int32_t s_ = 0; s_ < n_slices && (all_fit || count_wide); ++s_) {
            const int64_t sb = slice_ptr[s_], w = (slice_ptr[s_ + 1] - sb) / 64;
            const int64_t r0 = (int64_t)s_ * 64, r1 = std::min<int64_t>(n, r0 + 64);
            bool fits = true;
            for (int64_t k = 0; k < w && fits; ++k) {
                int64_t lo = INT64_MAX, hi = -1;
                for (int64_t r = r0; r < r1; ++r)
                    if (k < row_len[r]) { const int64_t c = scol[sb + k * 64 + (r - r0)]; lo = std::min(lo, c); hi = std::max(hi, c); }
                if (hi < 0) { cbase[(size_t)(sb / 64 + k)] = 0; continue; }
                if (hi - lo > 65535) { fits = false; break; }
                cbase[(size_t)(sb / 64 + k)] = (int32_t)lo;
                for (int64_t r = r0; r < r1; ++r)
                    if (k < row_len[r]) c16[(size_t)(sb + k * 64 + (r - r0))] = (uint16_t)(scol[sb + k * 64 + (r - r0)] - lo);
            }
            all_fit = all_fit && fits;
            if (!fits) ++wide_slices;
        }
        if (count_wide && wide_slices) fprintf(stderr, "[orc sell] narrow column image: %lld of %d slices have a depth that spans more than 65 535 columns\n", (long long)wide_slices, n_slices);
        if (all_fit) {  // all or nothing: the product kernels have no per-slice branch (scalar registers, see spmv_uniform_k)
            ORC_TRY(out.col16.upload(c16.data(), c16.size()));
            ORC_TRY(out.colbase.upload(cbase.data(), cbase.size()));
        }
    }
    ORC_TRY(out.diag_pos.upload(diag.data(), (size_t)n));
    ORC_TRY(out.csr_row_ptr.upload(row_ptr, (size_t)n + 1));
    // the pattern half of the row-contiguous mirror: CSR itself, addressed per slice (SellDev::rows_*)
    // (r04, measured twice at 10.24 M cells.  First half of the round: not a millisecond in any set-up phase on one stream — the walks are
    // latency-bound either way — and 2.8 GB more: off.  End of the round, with the set-up's counters and launches out of the way, in the CONCURRENT
    // iteration: 788.3 / 780.9 -> 774.0 / 771.4 ms on one box — a row is 2 cache lines instead of 15, and the fine level's sweeps and cascades
    // stop taking ~150 GB per iteration from the products beside them.  ON by default; ORC_AMG_L0_MIRROR=0 leaves it out.)
    const bool l0_mirror = cfg().amg_l0_mirror;
    if (l0_mirror && n > 0 && nnz > 0 && nnz < ((int64_t)1 << 31)) {
        std::vector<long long> rb((size_t)n_slices);
        std::vector<int32_t> ri((size_t)n), rc((size_t)nnz);
        for (int32_t s_ = 0; s_ < n_slices; ++s_) rb[(size_t)s_] = (long long)row_ptr[(int64_t)s_ * 64];
        for (int64_t r = 0; r < n; ++r) ri[(size_t)r] = (int32_t)(row_ptr[r] - row_ptr[(r >> 6) << 6]);
        for (int64_t q = 0; q < nnz; ++q) rc[(size_t)q] = (int32_t)col[q];
        ORC_TRY(out.rows_base.upload(rb.data(), rb.size()));
        ORC_TRY(out.rows_intra.upload(ri.data(), ri.size()));
        ORC_TRY(out.rows_col.upload(rc.data(), rc.size()));
    }
    return ORC_OK;
}

__global__ void sell_import_k(SellDev P, const int64_t *__restrict__ row_ptr, const double *__restrict__ csr, double *__restrict__ sell) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = P.slice_ptr[r >> 6] + (r & 63), b = row_ptr[r];
        const int len = P.row_len[r];
        const int width = (int)((P.slice_ptr[(r >> 6) + 1] - P.slice_ptr[r >> 6]) >> 6);
        for (int k = 0; k < width; ++k) sell[base + (int64_t)k * 64] = k < len ? csr[b + k] : 0.;
    }
}
__global__ void sell_export_k(SellDev P, const int64_t *__restrict__ row_ptr, const double *__restrict__ sell, double *__restrict__ csr) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t base = P.slice_ptr[r >> 6] + (r & 63), b = row_ptr[r];
        const int len = P.row_len[r];
        for (int k = 0; k < len; ++k) csr[b + k] = sell[base + (int64_t)k * 64];
    }
}

int sell_import_values(const SellMatrix &m, const double *csr_vals_dev, double *sell_vals_dev) {
    if (m.n == 0) return ORC_OK;
    hipLaunchKernelGGL(sell_import_k, dim3(grid_for(m.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.csr_row_ptr.p, csr_vals_dev, sell_vals_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
// values of a view's padded image -> row-contiguous (CSR) order: the VALUE half of the level-0 row mirror (SellDev::rows_*)
int sell_rows_values_dev(const SellDev &P, const double *sell_vals_dev, double *rows_vals_dev) {
    if (P.n == 0 || !P.csr_row_ptr) return ORC_OK;
    hipLaunchKernelGGL(sell_export_k, dim3(grid_for(P.n)), dim3(kBlock), 0, ctx().stream, P, P.csr_row_ptr, sell_vals_dev, rows_vals_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
int sell_export_values(const SellMatrix &m, const double *sell_vals_dev, double *csr_vals_dev) {
    if (m.n == 0) return ORC_OK;
    hipLaunchKernelGGL(sell_export_k, dim3(grid_for(m.n)), dim3(kBlock), 0, ctx().stream, m.dev(), m.csr_row_ptr.p, sell_vals_dev, csr_vals_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// ------------------------------------------------------------------ vector kernels
__global__ void fill_k(double *x, double v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = v;
}
int vec_fill(double *x, double v, int64_t n) {
    if (n == 0) return ORC_OK;
    hipLaunchKernelGGL(fill_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, x, v, n);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
int vec_copy(double *dst, const double *src, int64_t n) {
    if (n) ORC_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx().stream));
    return ORC_OK;
}

// dinv[i] = 1 / A(i,i) through the view; 0 where the diagonal is not stored (the reference's
// p_inv row is then empty: linear_algebra.rs:160-165)
__global__ void diag_inverse_k(MatView A, double *__restrict__ dinv) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = A.P.diag_pos[r];
        dinv[r] = d >= 0 ? 1. / view_value(A, r, d) : 0.;
    }
}
int diag_inverse_dev(const MatView &A, double *dinv) {
    if (A.P.n == 0) return ORC_OK;
    hipLaunchKernelGGL(diag_inverse_k, dim3(grid_for(A.P.n)), dim3(kBlock), 0, ctx().stream, A, dinv);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
// out = 0 + s * b   (p_inv * b as a one-entry-per-row SpMV, linear_algebra.rs:165)
__global__ void scale_vec_k(const double *__restrict__ s, const double *__restrict__ b, double *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = 0. + s[i] * b[i];
}

int scale_vec_dev(const double *sv, const double *b, double *out, int64_t n) {
    if (n == 0) return ORC_OK;
    hipLaunchKernelGGL(scale_vec_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, sv, b, out, n);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// ------------------------------------------------------------------ three systems in lock-step: interleaved vectors (MatView3, linalg.hpp)
__global__ void interleave3_k(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ c, double *__restrict__ out3, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<Vec3d *>(out3)[i] = Vec3d{a[i], b[i], c[i]};
}
__global__ void deinterleave3_k(const double *__restrict__ in3, double *__restrict__ a, double *__restrict__ b, double *__restrict__ c, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const Vec3d v = reinterpret_cast<const Vec3d *>(in3)[i];
        if (a) a[i] = v.a;
        if (b) b[i] = v.b;
        if (c) c[i] = v.c;
    }
}
int interleave3_dev(const double *a, const double *b, const double *c, double *out3, int64_t n) {
    if (n == 0) return ORC_OK;
    hipLaunchKernelGGL(interleave3_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, a, b, c, out3, n);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
int deinterleave3_dev(const double *in3, double *a, double *b, double *c, int64_t n) {
    if (n == 0) return ORC_OK;
    hipLaunchKernelGGL(deinterleave3_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, in3, a, b, c, n);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

__global__ void diag_inverse3_k(MatView3 A, double *__restrict__ dinv3) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < A.P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = A.P.diag_pos[r];
        double o[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            double v = 0.;
            if (d >= 0) {  // view_value per system
                v = A.val[s][d];
                if (A.s1) v = A.s1[3 * r + s] * v;
                if (A.s2) v = A.s2[3 * r + s] * v;
                v = 1. / v;
            }
            o[s] = v;
        }
        reinterpret_cast<Vec3d *>(dinv3)[r] = Vec3d{o[0], o[1], o[2]};
    }
}
int diag_inverse3_dev(const MatView3 &A, double *dinv3) {
    if (A.P.n == 0) return ORC_OK;
    hipLaunchKernelGGL(diag_inverse3_k, dim3(grid_for(A.P.n)), dim3(kBlock), 0, ctx().stream, A, dinv3);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

}  // namespace orc
