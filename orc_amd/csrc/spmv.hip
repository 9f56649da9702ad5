// spmv.hip — y = A x on SELL-64 and its mirrors: the epilogues the solvers fuse into a product, the choice of the
// kernel, the overlap of a product with its halo exchange, and the materialisation of scaled values.  The one translation unit that
// instantiates a product kernel (linalg_kernels.hpp).  Reference: src/linear_algebra.rs:159-166 (p_inv * a), :250-261 (the products).
//
// Everything is HBM-bound fp64 (AI ~ 0.13 flop/B): no MFMA, the levers are coalescing (SELL-64), XCD-local x-vector reuse, fused
// epilogues and no host round-trips inside a solve.  Compiled with -ffp-contract=off: rustc never fuses a*b+c, and bit-parity of
// y = A x with the CPU oracle depends on that.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>

#include "linalg_kernels.hpp"

namespace orc {

// Non-temporal matrix loads pay where the matrix streams through the caches (10.24 M cells: ~1 GB per product; in-loop level-0
// product 198 -> 178 us) and cost where it lives in the 256 MB Infinity Cache (1.03 M cells, 62 MB: 0.65 -> 0.60 of peak).
// ORC_SPMV_NT=0 / 1 forces the policy.
static inline int stream_nt(int64_t stream_bytes) {
    const int forced = cfg().spmv_nt;
    if (forced >= 0) return forced != 0;
    return stream_bytes > ((int64_t)128 << 20);
}

int stream_nt_policy(int64_t stream_bytes) { return stream_nt(stream_bytes); }
int matview_stream_nt(const MatView &A) { return stream_nt(A.pk.ptr && A.xw.lidx ? A.pk.total * 10 : A.P.padded * (A.P.col16 ? 10 : 12)); }

int spmv_grid(int32_t n_slices) {
    int64_t g = ((int64_t)n_slices + 3) / 4;  // 4 waves (slices) per workgroup
    const int cap = cfg().spmv_grid > 0 ? std::max(8, cfg().spmv_grid) : kMaxGrid;  // (ORC_SPMV_GRID: a test hook of the partial-sum bound)
    if (g > cap) g = cap;
    if (g >= 8) g = (g / 8) * 8;  // multiple of 8 for the XCD-aware walk
    return clamp_partials_grid(g);
}

// ------------------------------------------------------------------ SpMV epilogues
struct EpiStore {  // y = A x
    static constexpr int kReductions = 0;
    double *y;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &, double &) const { y[row] = acc; }
};
struct EpiStoreSum {  // y = A x ; partial sum(y)          (nu = A p, r_hat_0 . nu : linear_algebra.rs:256-257)
    static constexpr int kReductions = 1;
    double *y;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const { y[row] = acc; r0 += acc; }
};
struct EpiResidual {  // r = b - A x ; p = r ; partial sum(r)  (linear_algebra.rs:250-254)
    static constexpr int kReductions = 1;
    const double *b;
    double *r, *p;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const {
        const double v = b[row] - acc;
        r[row] = v;
        if (p) p[row] = v;
        r0 += v;
    }
};
struct EpiResidualNorm {  // partial sum((b - A x)^2)       (linear_algebra.rs:97, :202)
    static constexpr int kReductions = 1;
    const double *b;
    double *r;  // optional
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const {
        const double v = b[row] - acc;
        if (r) r[row] = v;
        r0 += v * v;
    }
};
struct EpiTs {  // t = A s ; partials t.s, t.t            (linear_algebra.rs:260-261)
    static constexpr int kReductions = 2;
    const double *s;
    double *t;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &r1) const {
        t[row] = acc;
        r0 += acc * s[row];
        r1 += acc * acc;
    }
};
struct EpiStoreDot {  // y = A x ; partial sum(y * s)             (q = A p, p . q : the CG arm, cg.hip)
    static constexpr int kReductions = 1;
    const double *s;
    double *y;
    __device__ __forceinline__ void apply(int64_t row, double acc, double &r0, double &) const {
        y[row] = acc;
        r0 += acc * s[row];
    }
};

// Host-side launch counters of launch_spmv, one per kernel family (orc_debug_product_launches, include/orc_amd.h: ORC_PRODUCT_*): a test
// that compares a product bit for bit has to know WHICH kernel produced the bits.  Counted where the launch is made; no device code.
enum { kFamRagged = 0, kFamPacked, kFamWindow, kFamGenericScaled, kFamWide, kFamNarrow, kFamNarrowNT, kFamMesh, kFamCount };
static std::atomic<long long> g_product_launches[kFamCount];
static inline void count_launch(int family) { g_product_launches[family].fetch_add(1, std::memory_order_relaxed); }
int debug_product_launches(long long *out, int n_out, bool reset) {
    for (int f = 0; f < kFamCount; ++f) {
        const long long v = reset ? g_product_launches[f].exchange(0, std::memory_order_relaxed) : g_product_launches[f].load(std::memory_order_relaxed);
        if (out && f < n_out) out[f] = v;
    }
    for (int f = kFamCount; out && f < n_out; ++f) out[f] = 0;
    return kFamCount;
}

// The grid of a window product (spmv_xwin_k) of the view A — the launch's own copy: fold_scratch is cleared on it when the workgroups
// write one partial sum each.  reductions: Epi::kReductions.
// One workgroup per 256-row block.  The blocks differ in cost (row lengths; blocks without a window gather from global
// memory), and a workgroup's share is fixed, so MORE workgroups than are resident balance better: r02's 5 per CU left the
// chip at 10 of 20 waves per CU on average (profiles/r03_pmc_products.csv: SQ_WAVE_CYCLES / GRBM_GUI_ACTIVE; 4 are resident
// with 32.7 KB of LDS and 92-96 VGPRs each); 8 per CU = the 2048 partial sums a product may write (kMaxPartials) measured
// level 2: 251 -> 245 us, level 3: 289 -> 270 us.
static int xwin_grid(MatView &A, int reductions) {
    const int per_cu = cfg().xwin_wgs_per_cu;  // (8; a test hook sweeps it far past the partial-sum bound)
    static const int n_cu = [] {
        hipDeviceProp_t prop;
        int dev = 0;
        return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }();
    int64_t gb = ((int64_t)A.P.n_slices + 3) / 4;
    // [r05] ONE workgroup per block, dispatched by the hardware as wave slots free up: with 2 048 persistent workgroups of 4-5 (level 2) or 2-3 blocks
    // (level 3) each, a third of a CU's wave slots stood empty on average (SQ_WAVE_CYCLES / GRBM_GUI_ACTIVE: 13 of 20) — the plain product 230-235 ->
    // 215-217 us on level 2, 250 -> 243 us on level 3 (scripts/archive/gpu_r05_z.sh).  Products with reductions fold their sums inside the launch
    // (spmv_xwin_k, XWinDev::fold_scratch): the consumers see one sum per quantity.
    // Blocks of short rows (config 5's level 1: 4 350 entries per block) are over before the ticket of the fold has paid for itself (its iteration
    // +5 ... +10 ms with one block per workgroup): such a level's workgroups take up to four blocks.  (Per-XCD block queues and other shares per
    // workgroup were measured and lost: HISTORY.md, appendix of round 5.)
    const bool one_per_block = cfg().xwin_wg_per_block && (reductions == 0 || A.xw.fold_scratch != nullptr) && A.pk.total > 0;
    if (one_per_block) {
        // about 12 000 entries per workgroup: one block on the channel's levels 2-3 (8 450 / 18 000 entries per block), three on config 5's level 1 (4 350)
        const int64_t per_block = std::max<int64_t>(1, A.pk.total / std::max<int64_t>(gb, 1));
        const int64_t blocks_per_wg = std::min<int64_t>(4, std::max<int64_t>(1, (12000 + per_block / 2) / per_block));
        gb = (gb + blocks_per_wg - 1) / blocks_per_wg;
        gb = (gb + 7) / 8 * 8;
    } else {
        A.xw.fold_scratch = nullptr;  // the kernel writes one partial sum per workgroup
        if (gb > (int64_t)n_cu * per_cu) gb = (int64_t)n_cu * per_cu;
        gb = clamp_partials_grid(gb);  // whatever the CU count (304 on gfx942) and the switch: the epilogue writes partials[blockIdx.x]
    }
    if (gb >= 8) gb = (gb / 8) * 8;
    return (int)std::max<int64_t>(gb, 1);
}

// Partitioned level-0 operator (View = MatView or MatView3): the rows without a ghost column (a contiguous run of slices,
// HaloPlan::interior_*) are multiplied on a second stream while the exchange travels; the rows along the cuts follow it on the library
// stream.  The three pieces write their partial sums side by side (View::part_base / part_stride), so one reduce_partials folds them;
// for three systems: the same slice ranges, grids and layout of the partial sums as the one-system form, per system the same bits.
// g: the grid of the undivided product; exchange(): refreshes the ghost entries of x; launch(V, grid, stream): one piece.
template <class View, class Exchange, class Launch>
static int launch_overlapped(const View &A, int g, int *grid_out, Exchange &&exchange, Launch &&launch) {
    HaloPlan *H = A.halo;
    const int g_b = std::max(8, (g / 8 / 8) * 8), g_i = std::max(8, ((g - 2 * g_b) / 8) * 8);
    const int total = g_i + 2 * g_b;
    if (grid_out) *grid_out = total;
    if (!H->aux_stream) {
        hipStream_t st2;
        hipEvent_t e1, e2;
        ORC_TRY(stream_create(&st2, kSolveStream, 0, "halo-overlap"));
        ORC_HIP(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
        ORC_HIP(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
        H->aux_stream = st2; H->ev_ready = e1; H->ev_done = e2;
    }
    hipStream_t lib = ctx().stream, aux = (hipStream_t)H->aux_stream;
    ORC_HIP(hipEventRecord((hipEvent_t)H->ev_ready, lib));  // x and whatever the epilogue reads are complete
    ORC_HIP(hipStreamWaitEvent(aux, (hipEvent_t)H->ev_ready, 0));
    View V = A;
    V.part_stride = total;
    V.slice_lo = H->interior_lo; V.slice_hi = H->interior_hi; V.part_base = 0;
    // RCCL: the exchange is queued first, so that its kernels are resident before the interior product fills the CUs.
    // The debug transport blocks this thread inside exchange(): there the interior product is launched first.
    const bool exchange_first = !comm_host_transport_active();
    if (exchange_first) ORC_TRY(exchange());  // C1 on the library stream (every RCCL call stays there)
    launch(V, g_i, aux);
    ORC_HIP(hipEventRecord((hipEvent_t)H->ev_done, aux));
    if (!exchange_first) {
        const int ex = exchange();
        if (ex != ORC_OK) {  // the interior product is in flight: the library stream must not run ahead of it
            (void)hipStreamWaitEvent(lib, (hipEvent_t)H->ev_done, 0);
            return ex;
        }
    }
    V.slice_lo = 0; V.slice_hi = H->interior_lo; V.part_base = g_i;
    launch(V, g_b, lib);
    V.slice_lo = H->interior_hi; V.slice_hi = A.P.n_slices; V.part_base = g_i + g_b;
    launch(V, g_b, lib);
    ORC_HIP(hipStreamWaitEvent(lib, (hipEvent_t)H->ev_done, 0));
    ORC_HIP(hipGetLastError());
    ctx().halo_overlaps += 1;
    return ORC_OK;
}
// the condition both forms share: a multi-rank run, a grid worth dividing, and an interior of at least half the slices
static inline bool overlap_pays(const HaloPlan *H, int32_t n_slices, int g) {
    return H && cfg().halo_overlap && ctx().world > 1 && g >= 64 && (int64_t)(H->interior_hi - H->interior_lo) * 2 >= (int64_t)n_slices;
}

// One launch of the wave-uniform product by the names of its template arguments (linalg_kernels.hpp: spmv_uniform_k).  No instantiation
// pairs kScaled with kNT: a view that still carries its scalings is launched without the hint, whatever MatView::nt says.
template <class Epi, bool kMesh, bool kNarrow, bool kScaled, bool kNT>
static void launch_uniform_as(const MatView &A, int g, hipStream_t stream, const double *x, const Epi &epi, double *partials, const double *skip_flags) {
    static_assert(!(kScaled && kNT), "a scaled view is never streamed with the non-temporal hint");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_uniform_k<Epi, false, kMesh, kNarrow, kScaled, kNT>), dim3(g), dim3(kBlock), 0, stream, A, x, epi, partials, skip_flags);
}
// ... with the run-time state of the view — row scalings, cache policy (MatView::nt) — turned into kScaled and kNT
template <class Epi, bool kMesh, bool kNarrow>
static void launch_uniform(const MatView &A, int g, const double *x, const Epi &epi, double *partials, const double *skip_flags) {
    if (A.s1 || A.s2) launch_uniform_as<Epi, kMesh, kNarrow, true, false>(A, g, ctx().stream, x, epi, partials, skip_flags);
    else if (A.nt) launch_uniform_as<Epi, kMesh, kNarrow, false, true>(A, g, ctx().stream, x, epi, partials, skip_flags);
    else launch_uniform_as<Epi, kMesh, kNarrow, false, false>(A, g, ctx().stream, x, epi, partials, skip_flags);
}

// One launch of the window product by its template arguments: scaled view or materialised values, cache policy (MatView::nt), and the level's
// position format (XWinDev::pos12)
template <class Epi, bool kP12>
static void launch_xwin(const MatView &A, int g, size_t smem, bool scaled, const double *x, const Epi &epi, double *partials, const double *skip_flags) {
    if (!scaled && A.nt) hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_xwin_k<Epi, false, true, kP12>), dim3(g), dim3(kBlock), smem, ctx().stream, A, x, epi, partials, skip_flags);
    else if (!scaled) hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_xwin_k<Epi, false, false, kP12>), dim3(g), dim3(kBlock), smem, ctx().stream, A, x, epi, partials, skip_flags);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_xwin_k<Epi, true, false, kP12>), dim3(g), dim3(kBlock), smem, ctx().stream, A, x, epi, partials, skip_flags);
}

// Every product of one system: sizes the grid, refreshes the ghost entries of x (or overlaps that with the interior rows) and picks the
// kernel by the view.  *grid_out: the partial sums written per reduction.
template <class Epi>
static int launch_spmv(const MatView &A_in, const double *x, const Epi &epi, double *partials, int *grid_out, const double *skip_flags = nullptr) {
    MatView A = A_in;
    A.nt = matview_stream_nt(A);
    const bool xwin = A.xw.lidx != nullptr && A.pk.ptr != nullptr;
    const int g = xwin ? xwin_grid(A, Epi::kReductions) : spmv_grid(A.P.n_slices);
    const bool scaled = A.s1 || A.s2;
    const bool uniform_kernel = !A.pk.ptr && A.P.ragged != 1;
    if (uniform_kernel && A.slice_hi < 0 && overlap_pays(A.halo, A.P.n_slices, g))
        return launch_overlapped(A, g, grid_out, [&] { return A.halo->exchange(const_cast<double *>(x)); },
                                 [&](const MatView &V, int grid, hipStream_t stream) {
                                     launch_uniform_as<Epi, false, false, true, false>(V, grid, stream, x, epi, partials, skip_flags);
                                     count_launch(kFamGenericScaled);
                                 });
    if (grid_out) *grid_out = (xwin && Epi::kReductions > 0 && A.xw.fold_scratch) ? 1 : g;  // (folded inside the launch: one sum per quantity)
    if (A.P.n == 0) return ORC_OK;
    if (A.halo) ORC_TRY(A.halo->exchange(const_cast<double *>(x)));  // C1: refresh the ghost entries of x
    if (xwin) {
        const size_t xwin_smem = sizeof(double) * (size_t)std::max(1, std::min(A.xw.cap, kXWinCap));
        if (A.xw.pos12) launch_xwin<Epi, true>(A, g, xwin_smem, scaled, x, epi, partials, skip_flags);
        else launch_xwin<Epi, false>(A, g, xwin_smem, scaled, x, epi, partials, skip_flags);
        count_launch(kFamWindow);
    } else if (A.pk.ptr) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_k<Epi, kSpmvPacked>), dim3(g), dim3(kBlock), 0, ctx().stream, A, x, epi, partials, skip_flags);
        count_launch(kFamPacked);
    } else if (A.P.ragged == 1) {  // long ragged rows without a mirror: every slot clamped, nothing skipped
        hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_k<Epi, kSpmvRagged>), dim3(g), dim3(kBlock), 0, ctx().stream, A, x, epi, partials, skip_flags);
        count_launch(kFamRagged);
    } else if (A.persistent_pattern) {  // mesh-pattern matrices (level 0): wave-uniform loads, predicated gathers
        if (A.P.col16) launch_uniform<Epi, true, true>(A, g, x, epi, partials, skip_flags);
        else launch_uniform<Epi, true, false>(A, g, x, epi, partials, skip_flags);
        count_launch(kFamMesh);
    } else if (!scaled && A.P.col16) {  // first coarse level, scaled values materialised, narrow column image
        if (A.nt) launch_uniform_as<Epi, false, true, false, true>(A, g, ctx().stream, x, epi, partials, skip_flags);
        else launch_uniform_as<Epi, false, true, false, false>(A, g, ctx().stream, x, epi, partials, skip_flags);
        count_launch(A.nt ? kFamNarrowNT : kFamNarrow);
    } else if (!scaled) {  // short ragged rows (first coarse level): the same kernel under its own name; scaled values materialised
        launch_uniform_as<Epi, false, false, false, false>(A, g, ctx().stream, x, epi, partials, skip_flags);
        count_launch(kFamWide);
    } else {
        launch_uniform_as<Epi, false, false, true, false>(A, g, ctx().stream, x, epi, partials, skip_flags);
        count_launch(kFamGenericScaled);
    }
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// ------------------------------------------------------------------ named products (arms.hpp)
int spmv_dev(const MatView &A, const double *x, double *y) { return launch_spmv(A, x, EpiStore{y}, nullptr, nullptr); }
int product_store(const MatView &A, const double *x, double *y, const double *skip_flags) {
    return launch_spmv(A, x, EpiStore{y}, nullptr, nullptr, skip_flags);
}
int product_store_sum(const MatView &A, const double *x, double *y, double *partials, int *grid_out, const double *skip_flags) {
    return launch_spmv(A, x, EpiStoreSum{y}, partials, grid_out, skip_flags);
}
int product_residual(const MatView &A, const double *x, const double *b, double *r, double *p, double *partials, int *grid_out, const double *skip_flags) {
    return launch_spmv(A, x, EpiResidual{b, r, p}, partials, grid_out, skip_flags);
}
int product_residual_norm(const MatView &A, const double *x, const double *b, double *r, double *partials, int *grid_out, const double *skip_flags) {
    return launch_spmv(A, x, EpiResidualNorm{b, r}, partials, grid_out, skip_flags);
}
int product_ts(const MatView &A, const double *s, double *t, double *partials, int *grid_out, const double *skip_flags) {
    return launch_spmv(A, s, EpiTs{s, t}, partials, grid_out, skip_flags);
}
int product_store_dot(const MatView &A, const double *p, double *q, double *partials, int *grid_out, const double *skip_flags) {
    return launch_spmv(A, p, EpiStoreDot{p, q}, partials, grid_out, skip_flags);
}

// partial sums nobody reads (residual_dev, residual3_dev: 3 * kMaxPartials doubles); one thread-safe allocation per process (concurrent solves)
static double *unread_partials() {
    static double *const p = [] {
        double *q = nullptr;
        return hipMalloc((void **)&q, sizeof(double) * 3 * kMaxPartials) == hipSuccess ? q : nullptr;
    }();
    return p;
}
int residual_dev(const MatView &A, const double *b, const double *x, double *r) {
    int g = 0;
    double *dummy = unread_partials();
    if (!dummy) return set_error(ORC_ERR_HIP, "hipMalloc of the residual scratch failed");
    return launch_spmv(A, x, EpiResidual{b, r, nullptr}, dummy, &g);
}

int residual_norm2_dev(const MatView &A, const double *b, const double *x, double *partials, double *out, double *r_scratch) {
    int g = 0;
    const bool ref = reference_order(A) && r_scratch != nullptr;
    ORC_TRY(launch_spmv(A, x, EpiResidualNorm{b, ref ? r_scratch : nullptr}, partials, &g));
    if (ref) return dot_reference(r_scratch, r_scratch, A.P.n, out, nullptr);
    return reduce_partials(partials, g, 1, out, A.halo != nullptr);
}

// Jacobi-scaled values, materialised: out[p] = s2[row] * (s1[row] * val[p]) — the product kernels' own expression, evaluated once per
// solve instead of once per product.  The reference materialises `p_inv * a` too (linear_algebra.rs:159-166); on the device the
// point is bytes: a level-0 product is bandwidth-bound at 5.6 TB/s of real traffic (profiles/r03_pmc_products.csv) and the two
// scaling vectors are 16 of its ~125 bytes per row — read 101 times per smoothing solve, against one extra pass over the values.
__global__ __launch_bounds__(kBlock) void scale_values_k(MatView A, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    SliceWalk w(A.P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int64_t base = A.P.slice_ptr[slice];
        const int width = (int)((A.P.slice_ptr[slice + 1] - base) >> 6);
        const bool live = row < A.P.n;
        const double s1 = (A.s1 && live) ? A.s1[row] : 1.;
        const double s2 = (A.s2 && live) ? A.s2[row] : 1.;
        for (int k = 0; k < width; ++k) {
            const int64_t p = base + (int64_t)k * 64 + lane;
            double t = A.val[p];
            if (A.s1) t = s1 * t;
            if (A.s2) t = s2 * t;
            out[p] = t;
        }
    }
}
// from how many iterations on a solve materialises its scaled values (ORC_MATERIALIZE_SCALING=0: never)
static inline bool materialize_scaling(uint64_t iteration_count) {
    const int min_its = cfg().materialize_scaling;
    return min_its > 0 && iteration_count >= (uint64_t)min_its;
}

// the same over a packed mirror (PackedDev): per pair of depths, the pairs of the lanes whose rows reach it sit back to back in lane order
// (a row's padding slot is scaled too: it stays finite and the product drops it)
__global__ __launch_bounds__(kBlock) void scale_packed_k(MatView A, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    SliceWalk w(A.P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int width = (int)((A.P.slice_ptr[slice + 1] - A.P.slice_ptr[slice]) >> 6);
        const bool live = row < A.P.n;
        const int len = live ? A.P.row_len[row] : 0;
        const double s1 = (A.s1 && live) ? A.s1[row] : 1.;
        const double s2 = (A.s2 && live) ? A.s2[row] : 1.;
        const f64x2_t *src = reinterpret_cast<const f64x2_t *>(A.pk.val + A.pk.ptr[slice]);
        f64x2_t *dst = reinterpret_cast<f64x2_t *>(out + A.pk.ptr[slice]);
        int off = 0;
        for (int k = 0; k < width; k += 2) {
            const bool in = k < len;
            const unsigned long long m = __ballot(in);
            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (in) {
                f64x2_t t = src[off + rank];
                if (A.s1) { t.x = s1 * t.x; t.y = s1 * t.y; }
                if (A.s2) { t.x = s2 * t.x; t.y = s2 * t.y; }
                dst[off + rank] = t;
            }
            off += __popcll(m);
        }
    }
}

int materialize_scaled_view(MatView &A, uint64_t iteration_count, Arena &arena) {
    if (!((A.s1 || A.s2) && A.P.n > 0 && materialize_scaling(iteration_count))) return ORC_OK;
    if (A.pk.ptr) {
        // levels with a packed mirror + LDS windows: their products stream pk.val only (launch_spmv: production variant)
        if (!(A.xw.lidx && A.pk.total > 0)) return ORC_OK;
        double *scaled;
        ORC_TRY(arena.alloc((size_t)A.pk.slots, &scaled));
        hipLaunchKernelGGL(scale_packed_k, dim3(spmv_grid(A.P.n_slices)), dim3(kBlock), 0, ctx().stream, A, scaled);
        ORC_HIP(hipGetLastError());
        A.pk.val = scaled;
        A.val = nullptr;  // the padded image keeps the unscaled values: nothing may read it through this view
        A.s1 = A.s2 = nullptr;
        return ORC_OK;
    }
    if (A.P.padded <= 0) return ORC_OK;
    double *scaled;
    ORC_TRY(arena.alloc((size_t)A.P.padded, &scaled));
    hipLaunchKernelGGL(scale_values_k, dim3(spmv_grid(A.P.n_slices)), dim3(kBlock), 0, ctx().stream, A, scaled);
    ORC_HIP(hipGetLastError());
    A.val = scaled;
    A.s1 = A.s2 = nullptr;
    return ORC_OK;
}

template <class Fn>
static int time_launches(int reps, float *ms, Fn &&launch) {
    hipEvent_t e0, e1;
    ORC_HIP(hipEventCreate(&e0));
    ORC_HIP(hipEventCreate(&e1));
    int st = launch();  // warm
    if (st == ORC_OK && hipEventRecord(e0, ctx().stream) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    for (int i = 0; i < reps && st == ORC_OK; ++i) st = launch();
    if (st == ORC_OK && (hipEventRecord(e1, ctx().stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) st = set_error(ORC_ERR_HIP, "hipEventRecord failed");
    if (st == ORC_OK && hipEventElapsedTime(ms, e0, e1) != hipSuccess) st = set_error(ORC_ERR_HIP, "hipEventElapsedTime failed");
    if (st == ORC_OK) *ms /= (float)std::max(reps, 1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return st;
}
int bench_inloop_products_dev(const MatView &A, const double *x, double *y, double *partials, int reps, float ms[2]) {
    int g = 0;
    ORC_TRY(time_launches(reps, &ms[0], [&] { return launch_spmv(A, x, EpiStoreSum{y}, partials, &g, nullptr); }));
    ORC_TRY(time_launches(reps, &ms[1], [&] { return launch_spmv(A, x, EpiTs{x, y}, partials, &g, nullptr); }));
    return ORC_OK;
}

// ------------------------------------------------------------------ three systems in lock-step (MatView3, linalg.hpp)
// The u, v and w momentum systems of an iteration: one pattern, three value arrays, interleaved vectors.  Every product below keeps,
// per system, the thread -> element map, the order of the additions and the fold of its one-system counterpart above, so a system
// multiplied here and the same system multiplied alone agree in every bit (tests/test_gpu_triple.py).
struct EpiStore3 {
    static constexpr int kReductions = 0;
    double *y3;
    __device__ __forceinline__ void apply(int64_t row, const double (&acc)[3], double (&)[3][2]) const {
        reinterpret_cast<Vec3d *>(y3)[row] = Vec3d{acc[0], acc[1], acc[2]};
    }
};
struct EpiStoreSum3 {
    static constexpr int kReductions = 1;
    double *y3;
    __device__ __forceinline__ void apply(int64_t row, const double (&acc)[3], double (&red)[3][2]) const {
        reinterpret_cast<Vec3d *>(y3)[row] = Vec3d{acc[0], acc[1], acc[2]};
        red[0][0] += acc[0]; red[1][0] += acc[1]; red[2][0] += acc[2];
    }
};
struct EpiResidual3 {
    static constexpr int kReductions = 1;
    const double *b3;
    double *r3, *p3;
    __device__ __forceinline__ void apply(int64_t row, const double (&acc)[3], double (&red)[3][2]) const {
        const Vec3d b = reinterpret_cast<const Vec3d *>(b3)[row];
        const Vec3d v = {b.a - acc[0], b.b - acc[1], b.c - acc[2]};
        reinterpret_cast<Vec3d *>(r3)[row] = v;
        if (p3) reinterpret_cast<Vec3d *>(p3)[row] = v;
        red[0][0] += v.a; red[1][0] += v.b; red[2][0] += v.c;
    }
};
struct EpiResidualNorm3 {
    static constexpr int kReductions = 1;
    const double *b3;
    __device__ __forceinline__ void apply(int64_t row, const double (&acc)[3], double (&red)[3][2]) const {
        const Vec3d b = reinterpret_cast<const Vec3d *>(b3)[row];
        const double v0 = b.a - acc[0], v1 = b.b - acc[1], v2 = b.c - acc[2];
        red[0][0] += v0 * v0; red[1][0] += v1 * v1; red[2][0] += v2 * v2;
    }
};
struct EpiTs3 {
    static constexpr int kReductions = 2;
    const double *s3;
    double *t3;
    __device__ __forceinline__ void apply(int64_t row, const double (&acc)[3], double (&red)[3][2]) const {
        const Vec3d sv = reinterpret_cast<const Vec3d *>(s3)[row];
        reinterpret_cast<Vec3d *>(t3)[row] = Vec3d{acc[0], acc[1], acc[2]};
        red[0][0] += acc[0] * sv.a; red[0][1] += acc[0] * acc[0];
        red[1][0] += acc[1] * sv.b; red[1][1] += acc[1] * acc[1];
        red[2][0] += acc[2] * sv.c; red[2][1] += acc[2] * acc[2];
    }
};

// One launch of the three-system wave-uniform product by the names of its template arguments (linalg_kernels.hpp: spmv3_uniform_k)
template <class Epi3, bool kMesh, bool kNarrow, bool kScaled, bool kNT>
static void launch_uniform3_as(const MatView3 &A, int g, hipStream_t stream, const double *x3, const Epi3 &epi, double *partials) {
    static_assert(!(kScaled && kNT), "a scaled view is never streamed with the non-temporal hint");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv3_uniform_k<Epi3, 4, kMesh, kNarrow, kScaled, kNT>), dim3(g), dim3(kBlock), 0, stream, A, x3, epi, partials);
}
// ... with the run-time state of the view turned into kScaled and kNT (as launch_uniform)
template <class Epi3, bool kMesh, bool kNarrow>
static void launch_uniform3(const MatView3 &A, int g, hipStream_t stream, const double *x3, const Epi3 &epi, double *partials) {
    if (A.s1 || A.s2) launch_uniform3_as<Epi3, kMesh, kNarrow, true, false>(A, g, stream, x3, epi, partials);
    else if (A.nt) launch_uniform3_as<Epi3, kMesh, kNarrow, false, true>(A, g, stream, x3, epi, partials);
    else launch_uniform3_as<Epi3, kMesh, kNarrow, false, false>(A, g, stream, x3, epi, partials);
}

template <class Epi3>
static int launch_spmv3(const MatView3 &A_in, const double *x3, const Epi3 &epi, double *partials, int *grid_out) {
    MatView3 A = A_in;
    A.nt = stream_nt(A.P.padded * (A.P.col16 ? 26 : 28));
    const int g = spmv_grid(A.P.n_slices);  // the one-system grid: same walk, same partial sums
    if (grid_out) *grid_out = g;
    if (A.P.n == 0) return ORC_OK;
    const bool scaled = A.s1 || A.s2;
    // [r04] a partitioned level-0 operator overlaps the exchange of the interleaved iterate as launch_spmv does for one system
    const bool plain_kernel = A.mesh_pattern && A.P.col16 != nullptr && !scaled;  // the variant the solves launch (materialised, narrow columns)
    if (plain_kernel && overlap_pays(A.halo, A.P.n_slices, g))
        return launch_overlapped(A, g, grid_out, [&] { return A.halo->exchange_interleaved(const_cast<double *>(x3), 3); },
                                 [&](const MatView3 &V, int grid, hipStream_t stream) { launch_uniform3<Epi3, true, true>(V, grid, stream, x3, epi, partials); });
    if (A.halo) ORC_TRY(A.halo->exchange_interleaved(const_cast<double *>(x3), 3));  // C1: the ghost entries of the three systems in one message per peer
    hipStream_t stream = ctx().stream;
    if (A.mesh_pattern) {
        if (A.P.col16) launch_uniform3<Epi3, true, true>(A, g, stream, x3, epi, partials);
        else launch_uniform3<Epi3, true, false>(A, g, stream, x3, epi, partials);
    } else if (!scaled && A.P.col16 && A.nt) launch_uniform3_as<Epi3, false, true, false, true>(A, g, stream, x3, epi, partials);
    else if (!scaled && A.P.col16) launch_uniform3_as<Epi3, false, true, false, false>(A, g, stream, x3, epi, partials);
    else if (!scaled) launch_uniform3_as<Epi3, false, false, false, false>(A, g, stream, x3, epi, partials);
    else launch_uniform3_as<Epi3, false, false, true, false>(A, g, stream, x3, epi, partials);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int spmv3_dev(const MatView3 &A, const double *x3, double *y3) { return launch_spmv3(A, x3, EpiStore3{y3}, nullptr, nullptr); }
int product_store_sum3(const MatView3 &A, const double *x3, double *y3, double *partials, int *grid_out) {
    return launch_spmv3(A, x3, EpiStoreSum3{y3}, partials, grid_out);
}
int product_residual3(const MatView3 &A, const double *x3, const double *b3, double *r3, double *p3, double *partials, int *grid_out) {
    return launch_spmv3(A, x3, EpiResidual3{b3, r3, p3}, partials, grid_out);
}
int product_ts3(const MatView3 &A, const double *s3, double *t3, double *partials, int *grid_out) {
    return launch_spmv3(A, s3, EpiTs3{s3, t3}, partials, grid_out);
}

int residual3_dev(const MatView3 &A, const double *b3, double *x3, double *r3) {
    double *dummy = unread_partials();
    if (!dummy) return set_error(ORC_ERR_HIP, "hipMalloc of the residual scratch failed");
    return launch_spmv3(A, x3, EpiResidual3{b3, r3, nullptr}, dummy, nullptr);
}
int residual_norm2_3_dev(const MatView3 &A, const double *b3, double *x3, double *partials, double *out3) {
    int g = 0;
    ORC_TRY(launch_spmv3(A, x3, EpiResidualNorm3{b3}, partials, &g));
    return reduce_partials(partials, g, 3, out3, A.halo != nullptr);
}

// scale_values_k for system `sys` of a MatView3 (scalings interleaved)
__global__ __launch_bounds__(kBlock) void scale_values3_k(MatView3 A, int sys, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const double *__restrict__ val = A.val[sys];
    SliceWalk w(A.P.n_slices);
    for (int64_t slice = w.begin; slice < w.end; slice += w.step) {
        const int64_t row = slice * 64 + lane;
        const int64_t base = A.P.slice_ptr[slice];
        const int width = (int)((A.P.slice_ptr[slice + 1] - base) >> 6);
        const bool live = row < A.P.n;
        const double s1 = (A.s1 && live) ? A.s1[3 * row + sys] : 1.;
        const double s2 = (A.s2 && live) ? A.s2[3 * row + sys] : 1.;
        for (int k = 0; k < width; ++k) {
            const int64_t p = base + (int64_t)k * 64 + lane;
            double t = val[p];
            if (A.s1) t = s1 * t;
            if (A.s2) t = s2 * t;
            out[p] = t;
        }
    }
}

int materialize_scaled_view3(MatView3 &A, uint64_t iteration_count, Arena &arena) {
    if (!((A.s1 || A.s2) && A.P.padded > 0 && A.P.n > 0 && materialize_scaling(iteration_count))) return ORC_OK;
    for (int s = 0; s < 3; ++s) {
        double *scaled;
        ORC_TRY(arena.alloc((size_t)A.P.padded, &scaled));
        hipLaunchKernelGGL(scale_values3_k, dim3(spmv_grid(A.P.n_slices)), dim3(kBlock), 0, ctx().stream, A, s, scaled);
        A.val[s] = scaled;  // the kernel reads A.val[sys] only; the scalings are dropped once all three are through
    }
    ORC_HIP(hipGetLastError());
    A.s1 = A.s2 = nullptr;
    return ORC_OK;
}

int bench_inloop_products3_dev(const MatView3 &A, const double *x3, double *y3, double *partials, int reps, float ms[2]) {
    int g = 0;
    ORC_TRY(time_launches(reps, &ms[0], [&] { return launch_spmv3(A, x3, EpiStoreSum3{y3}, partials, &g); }));
    ORC_TRY(time_launches(reps, &ms[1], [&] { return launch_spmv3(A, x3, EpiTs3{x3, y3}, partials, &g); }));
    return ORC_OK;
}

}  // namespace orc
