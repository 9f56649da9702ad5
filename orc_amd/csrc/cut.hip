// cut.hip — cut surfaces (new-build extension; ORC has no entry that draws anything): plane slices and iso-surfaces as polygons with
// sampled fields.  DESIGN.md §3 "Cut surfaces" has the definition; in short, for a node function d
//     above        a node is above iff d >= 0; an edge of a face's node cycle is cut iff its ends differ
//     cut point    on the edge from the lower node id to the higher: t = d_lo / (d_lo - d_hi), x = x_lo + t (x_hi - x_lo); key (lo, hi)
//     segments     every maximal run of above nodes of a face's cycle is cut off by one segment, directed so that the region d >= 0
//                  lies on its left seen from outside the cell
//     loops        the segments of a cell's faces join at equal keys; every loop is a polygon, started at its smallest key, the loops
//                  of a cell in the order of their starts, the cells in ascending ORC id
//     node value   phi_v = (sum_c w_c phi_c) / (sum_c w_c), w_c = 1 / sqrt((dx dx + dy dy) + dz dz), d. = x_c - x_v, c ascending in ORC id
//
//   node_average_k   one lane per node: the gather through the node -> cell table
//   node_plane_k / node_level_k   d per node
//   face_count_k     one lane per face: the cut edges of its cycle (7 bits, saturating) and a non-finite flag in ONE byte — the cell
//                    pass then reads a byte per face in place of every node id and every d twice (measured at 10.24 M cells: 374 us
//                    for both passes against 633 us for a cell pass that reads the node lists itself)
//   cut_classify_k   one lane per cell in ORC order, the hot pass: cut points = half the cut edges of its faces, 0 for a skipped cell;
//                    skipped cells are counted per reason with integer atomics
//   scan_sums_k / scan_top_k / scan_place_k   the chunked exclusive scan in ORC-id order: per-chunk sums, one workgroup over the sums,
//                    then every chunk places its non-zero entries into a compact list with their offsets.  Used twice: cells -> (cut
//                    cell, first point), and points' loop-start flags -> poly_ptr
//   cut_emit_k       one lane per cut cell: the segments into a link table (LDS, one column per lane), the loops out in order
//   cut_polygons_k   one lane per polygon: the owner cell and the area vector A = 1/2 sum (p_i - p_0) x (p_i+1 - p_0)
// No float atomics anywhere: two cuts of one state give the same bits.  The host reads counts twice to size the outputs — (cut cells,
// NP, skipped cells) after the first scan, P after the second — and allocates in between; the owners' ORC ids come to the host when
// orc_cut_get or orc_cut_sample_cells first asks for them.
// A mesh whose cells are not closed (an edge of a cell in one face only, or in three) is outside the definition: such a cell may emit
// fewer points than it was counted for; the points it leaves stay zero-filled with key (0, 0) and join the polygon before them.  Nothing
// is read or written out of bounds, and nothing counts such cells.
#include <algorithm>
#include <cmath>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "gradient_cell.hpp"
#include "probes.hpp"

struct OrcCut {
    OrcMesh *mesh = nullptr;
    int64_t P = 0, NP = 0, n_nonfinite = 0, n_overflow = 0;
    orc::DevBuf<int32_t> poly_ptr, cell, owner, klo, khi;  // [P + 1] (the P starts), [P] internal id, [NP] internal id, [NP], [NP]
    orc::DevBuf<double> points, area;                      // [3 NP] point-major, [3 P] polygon-major
    orc::DevBuf<uint8_t> lstart;                           // [NP] 1 at the first point of every loop
    mutable std::vector<int64_t> h_cell;                   // [P] ORC ids, fetched at first use (owners_on_host)
    mutable bool h_cell_valid = false;
};

namespace orc {

constexpr int kCutMaxPoints = ORC_CUT_MAX_POINTS;
constexpr int kScanPerThread = 4;
constexpr int kScanChunk = kBlock * kScanPerThread;  // entries of one workgroup of the scan
constexpr int kEmitBlock = kWave;                    // one wave per workgroup: 64 columns of the link table
static_assert(kCutMaxPoints >= 32 && kCutMaxPoints <= 62, "the visited mask is one 64-bit word and the face byte saturates at 127 cut edges");

namespace {

struct CutDev {
    int64_t V, F;
    const double *vx, *vy, *vz;
    const int32_t *fnp, *fn, *ncp, *nc, *orc2int, *int2orc;
};
CutDev cut_dev(const OrcMesh &m) {
    const CutNodes &N = *m.nodes;
    return {N.n_vertices, m.n_faces, N.vx.p, N.vy.p, N.vz.p, N.fnp.p, N.fn.p, N.ncp.p, N.nc.p, N.orc2int.p, N.int2orc.p};
}

// ------------------------------------------------------------------ node values
__global__ __launch_bounds__(kBlock) void node_average_k(MeshDev M, CutDev N, const double *__restrict__ phi, double *__restrict__ out) {
    GRID_STRIDE(v, N.V) {
        const double x = N.vx[v], y = N.vy[v], z = N.vz[v];
        double sw = 0., swp = 0.;
        for (int32_t q = N.ncp[v]; q < N.ncp[v + 1]; ++q) {
            const int32_t c = N.nc[q];
            const double dx = M.ccx[c] - x, dy = M.ccy[c] - y, dz = M.ccz[c] - z;
            const double w = 1. / sqrt((dx * dx + dy * dy) + dz * dz);
            swp = swp + w * phi[c];
            sw = sw + w;
        }
        out[v] = swp / sw;
    }
}

__global__ __launch_bounds__(kBlock) void node_plane_k(CutDev N, double ox, double oy, double oz, double nx, double ny, double nz, double *__restrict__ d) {
    GRID_STRIDE(v, N.V) d[v] = ((N.vx[v] - ox) * nx + (N.vy[v] - oy) * ny) + (N.vz[v] - oz) * nz;
}

__global__ __launch_bounds__(kBlock) void node_level_k(int64_t V, const double *__restrict__ val, double level, double *__restrict__ d) {
    GRID_STRIDE(v, V) d[v] = val[v] - level;
}

__global__ __launch_bounds__(kBlock) void fill_k(int64_t n, double value, double *__restrict__ out) {
    GRID_STRIDE(i, n) out[i] = value;
}

// ------------------------------------------------------------------ classify
__device__ __forceinline__ bool finite_d(double d) { return fabs(d) <= 1.7976931348623157e308; }  // false for NaN and the infinities

// the cut edges of face f's cycle (saturating at 127) with bit 7 set when a node's d is not finite
__device__ __forceinline__ uint32_t face_cut_byte(const CutDev &N, const double *__restrict__ d, int32_t f) {
    const int32_t b = N.fnp[f], e = N.fnp[f + 1];
    double dp = d[N.fn[e - 1]];
    uint32_t cuts = 0, bad = finite_d(dp) ? 0u : 1u;
    bool prev = dp >= 0.;
    for (int32_t i = b; i < e; ++i) {
        const double dv = d[N.fn[i]];
        const bool cur = dv >= 0.;
        cuts += cur != prev ? 1u : 0u;
        bad |= finite_d(dv) ? 0u : 1u;
        prev = cur;
    }
    return (cuts > 127u ? 127u : cuts) | (bad << 7);
}

__global__ __launch_bounds__(kBlock) void face_count_k(CutDev N, const double *__restrict__ d, uint8_t *__restrict__ fcut) {
    GRID_STRIDE(f, N.F) fcut[f] = (uint8_t)face_cut_byte(N, d, (int32_t)f);
}

// one lane per ORC cell id g: count[g] = its cut points, 0 when it is not cut or skipped; skipped[0 / 1] += the NONFINITE / OVERFLOW cells
__global__ __launch_bounds__(kBlock) void cut_classify_k(MeshDev M, const int32_t *__restrict__ orc2int, const uint8_t *__restrict__ fcut,
                                                         int32_t *__restrict__ count, unsigned long long *__restrict__ skipped) {
    const int64_t n = M.n_own;
    const int64_t span = ((n + kBlock - 1) / kBlock) * kBlock;  // whole workgroups reach the votes below
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < span; g += (int64_t)gridDim.x * blockDim.x) {
        uint32_t edges = 0, bad = 0;
        if (g < n) {
            const int32_t c = orc2int ? orc2int[g] : (int32_t)g;
            for (int32_t q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
                const uint32_t b = fcut[M.cf[q]];
                edges += b & 127u;
                bad |= b >> 7;
            }
        }
        const uint32_t pts = edges >> 1;  // every cut edge of a closed cell lies in two of its faces
        const bool nonfinite = bad != 0, overflow = !nonfinite && pts > (uint32_t)kCutMaxPoints;
        if (g < n) count[g] = (nonfinite || overflow) ? 0 : (int32_t)pts;
        const unsigned long long v0 = __ballot(nonfinite), v1 = __ballot(overflow);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            if (v0) atomicAdd(skipped, (unsigned long long)__popcll(v0));
            if (v1) atomicAdd(skipped + 1, (unsigned long long)__popcll(v1));
        }
    }
}

// ------------------------------------------------------------------ the scan
// (x, y) = (entries that are not zero, their sum) before a position
__device__ __forceinline__ int2 add2(int2 a, int2 b) { return make_int2(a.x + b.x, a.y + b.y); }

// inclusive sum over the workgroup's kBlock threads; s holds kBlock entries
__device__ __forceinline__ int2 block_scan_inclusive(int2 v, int2 *s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int2 add = t >= o ? s[t - o] : make_int2(0, 0);
        __syncthreads();
        s[t] = add2(s[t], add);
        __syncthreads();
    }
    return s[t];
}

template <class T>
__device__ __forceinline__ int2 thread_entries(const T *__restrict__ in, int64_t n, int64_t first, int v[kScanPerThread]) {
    int2 sum = make_int2(0, 0);
#pragma unroll
    for (int k = 0; k < kScanPerThread; ++k) {
        v[k] = first + k < n ? (int)in[first + k] : 0;
        sum.x += v[k] != 0 ? 1 : 0;
        sum.y += v[k];
    }
    return sum;
}

// workgroup b sums chunk b = the entries [b kScanChunk, (b + 1) kScanChunk)
template <class T>
__global__ __launch_bounds__(kBlock) void scan_sums_k(const T *__restrict__ in, int64_t n, int2 *__restrict__ sums) {
    __shared__ int2 s[kBlock];
    int v[kScanPerThread];
    const int2 mine = thread_entries(in, n, (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPerThread, v);
    const int2 incl = block_scan_inclusive(mine, s);
    if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = incl;
}

// ONE workgroup: the chunk sums become what lies before each chunk; total = everything
__global__ __launch_bounds__(kBlock) void scan_top_k(int2 *__restrict__ sums, int64_t n_chunks, int2 *__restrict__ total) {
    __shared__ int2 s[kBlock];
    int2 carry = make_int2(0, 0);
    for (int64_t base = 0; base < n_chunks; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const int2 v = i < n_chunks ? sums[i] : make_int2(0, 0);
        const int2 incl = block_scan_inclusive(v, s);
        if (i < n_chunks) sums[i] = make_int2(carry.x + incl.x - v.x, carry.y + incl.y - v.y);
        carry = add2(carry, s[kBlock - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// every entry that is not zero goes to list[k], k = the non-zero entries before it, with list_off[k] = the sum before it
template <class T>
__global__ __launch_bounds__(kBlock) void scan_place_k(const T *__restrict__ in, int64_t n, const int2 *__restrict__ before, int32_t *__restrict__ list,
                                                       int32_t *__restrict__ list_off) {
    __shared__ int2 s[kBlock];
    int v[kScanPerThread];
    const int64_t first = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPerThread;
    const int2 mine = thread_entries(in, n, first, v);
    const int2 incl = block_scan_inclusive(mine, s);
    const int2 b = before[blockIdx.x];
    int k = b.x + incl.x - mine.x, off = b.y + incl.y - mine.y;
#pragma unroll
    for (int q = 0; q < kScanPerThread; ++q)
        if (v[q] != 0) {  // first + q < n: entries past the end read as 0
            list[k] = (int32_t)(first + q);
            if (list_off) list_off[k] = off;
            ++k;
            off += v[q];
        }
}

// ------------------------------------------------------------------ emit
struct EmitArgs {
    const double *d;
    const int32_t *count;      // [n] by ORC id
    const int32_t *cut_cells;  // [n_cut] ORC ids, ascending
    const int32_t *cut_first;  // [n_cut] the cell's first point
    int64_t n_cut;
    double *points;            // [3 NP]
    int32_t *klo, *khi, *owner;
    uint8_t *lstart;
};

// The loops of the emit kernel are short and lane-divergent: they are kept rolled, and their selections are conditional moves.
constexpr unsigned long long kNoKey = ~0ull;
__device__ __forceinline__ unsigned long long pack_key(int32_t a, int32_t b) {
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return ((unsigned long long)(uint32_t)lo << 32) | (unsigned long long)(uint32_t)hi;  // ordered as (lo, then hi)
}

// the slot of a key in this lane's column, entered if new; -1 when the column is full (a cell that is not closed)
__device__ __forceinline__ int key_slot(unsigned long long (*s_key)[kEmitBlock], uint8_t (*s_next)[kEmitBlock], int lane, int &n_slots, unsigned long long key) {
    int found = -1;
#pragma unroll 1
    for (int s = 0; s < n_slots; ++s) found = (found < 0 && s_key[s][lane] == key) ? s : found;
    const bool enter = found < 0 && n_slots < kCutMaxPoints;
    if (enter) {
        s_key[n_slots][lane] = key;
        s_next[n_slots][lane] = 0xFF;
        found = n_slots;
        n_slots = n_slots + 1;
    }
    return found;
}

// One lane per cut cell.  The link table lives in LDS, slot-major, so that the 64 lanes of the wave read 64 consecutive words: no
// private array, no scratch.  A lane touches its own column only: no barrier.
__global__ __launch_bounds__(kEmitBlock) void cut_emit_k(MeshDev M, CutDev N, EmitArgs A) {
    __shared__ unsigned long long s_key[kCutMaxPoints][kEmitBlock];
    __shared__ uint8_t s_next[kCutMaxPoints][kEmitBlock];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kEmitBlock + lane;
    if (i >= A.n_cut) return;
    const int32_t g = A.cut_cells[i];
    const int32_t c = N.orc2int ? N.orc2int[g] : g;
    const int32_t first = A.cut_first[i], np = A.count[g];
    int n_slots = 0;
#pragma unroll 1
    for (int32_t q = M.cfp[c]; q < M.cfp[c + 1]; ++q) {
        const int32_t f = M.cf[q];
        const int32_t b = N.fnp[f], m = N.fnp[f + 1] - b;
        // outside: the cycle's right-hand normal r = (x1 - x0) x (x2 - x1) against the stored normal, which leaves cell c0
        const int32_t n0 = N.fn[b], n1 = N.fn[b + 1], n2 = N.fn[b + 2];
        const double ax = N.vx[n1] - N.vx[n0], ay = N.vy[n1] - N.vy[n0], az = N.vz[n1] - N.vz[n0];
        const double bx = N.vx[n2] - N.vx[n1], by = N.vy[n2] - N.vy[n1], bz = N.vz[n2] - N.vz[n1];
        const double rx = ay * bz - az * by, ry = az * bx - ax * bz, rz = ax * by - ay * bx;
        const double along = (rx * M.nx[f] + ry * M.ny[f]) + rz * M.nz[f];
        const bool ccw_outside = (M.c0[f] == c) ? along > 0. : along < 0.;  // the cycle runs counter-clockwise seen from outside c
        // the first position that enters a run of above nodes; none: the face is not cut
        int j0 = -1;
        bool prev = A.d[N.fn[b + m - 1]] >= 0.;
#pragma unroll 1
        for (int j = 0; j < m; ++j) {
            const bool cur = A.d[N.fn[b + j]] >= 0.;
            j0 = (j0 < 0 && cur && !prev) ? j : j0;
            prev = cur;
        }
        if (j0 >= 0) {
            // once around from there: entry, exit, entry, exit ...; a run's segment joins its exit edge and its entry edge
            int32_t enter_a = N.fn[b + (j0 + m - 1) % m], enter_b = N.fn[b + j0];
            int32_t pn = enter_b;
            prev = true;
#pragma unroll 1
            for (int t = 1; t <= m; ++t) {
                const int32_t cn = N.fn[b + (j0 + t) % m];
                const bool cur = A.d[cn] >= 0.;
                const bool enters = cur && !prev, leaves = !cur && prev;
                enter_a = enters ? pn : enter_a;
                enter_b = enters ? cn : enter_b;
                if (leaves) {
                    const int se = key_slot(s_key, s_next, lane, n_slots, pack_key(enter_a, enter_b));
                    const int sx = key_slot(s_key, s_next, lane, n_slots, pack_key(pn, cn));
                    if (se >= 0 && sx >= 0) {
                        // region on the left: seen from outside a counter-clockwise cycle, from the exit back to the entry
                        const int from = ccw_outside ? sx : se, to = ccw_outside ? se : sx;
                        s_next[from][lane] = (uint8_t)to;
                    }
                }
                prev = cur;
                pn = cn;
            }
        }
    }
    // the loops: the unvisited slot with the smallest key starts the next one
    unsigned long long visited = 0;
    int emitted = 0;
#pragma unroll 1
    while (emitted < np) {
        unsigned long long best = kNoKey;
        int start = -1;
#pragma unroll 1
        for (int s = 0; s < n_slots; ++s) {
            const unsigned long long k = (visited >> s & 1ull) ? kNoKey : s_key[s][lane];
            const bool take = k < best;
            best = take ? k : best;
            start = take ? s : start;
        }
        if (start < 0) {
            emitted = np;  // a cell that is not closed: nothing left to start from
        } else {
            int cur = start;
            bool head = true, more = true;
#pragma unroll 1
            while (more) {
                const unsigned long long key = s_key[cur][lane];
                const int32_t lo = (int32_t)(key >> 32), hi = (int32_t)(key & 0xFFFFFFFFull);
                const double dlo = A.d[lo], dhi = A.d[hi];
                const double t = dlo / (dlo - dhi);
                const int64_t o = (int64_t)first + emitted;
                A.points[3 * o] = N.vx[lo] + t * (N.vx[hi] - N.vx[lo]);
                A.points[3 * o + 1] = N.vy[lo] + t * (N.vy[hi] - N.vy[lo]);
                A.points[3 * o + 2] = N.vz[lo] + t * (N.vz[hi] - N.vz[lo]);
                A.klo[o] = lo; A.khi[o] = hi; A.owner[o] = c;
                A.lstart[o] = head ? 1 : 0;
                head = false;
                visited |= 1ull << cur;
                emitted = emitted + 1;
                const int nxt = s_next[cur][lane];
                const bool linked = nxt < n_slots;
                const int shift = linked ? nxt : 0;
                // on while the cell has points left and the link leads to an unvisited slot (back at the start: closed)
                more = emitted < np && linked && !(visited >> shift & 1ull);
                cur = more ? nxt : cur;
            }
        }
    }
}

// one lane per polygon: owner and area vector, the fan about its first point with the components accumulated left to right
__global__ __launch_bounds__(kBlock) void cut_polygons_k(int64_t P, int64_t NP, const int32_t *__restrict__ poly_ptr, const int32_t *__restrict__ owner,
                                                         const double *__restrict__ pts, int32_t *__restrict__ cell, double *__restrict__ area) {
    GRID_STRIDE(p, P) {
        const int32_t b = poly_ptr[p], e = p + 1 < P ? poly_ptr[p + 1] : (int32_t)NP;  // the device table holds the P starts
        cell[p] = owner[b];
        const double x0 = pts[3 * (int64_t)b], y0 = pts[3 * (int64_t)b + 1], z0 = pts[3 * (int64_t)b + 2];
        double sx = 0., sy = 0., sz = 0.;
        for (int64_t i = b + 1; i + 1 < e; ++i) {
            const double ax = pts[3 * i] - x0, ay = pts[3 * i + 1] - y0, az = pts[3 * i + 2] - z0;
            const double bx = pts[3 * i + 3] - x0, by = pts[3 * i + 4] - y0, bz = pts[3 * i + 5] - z0;
            sx = sx + (ay * bz - az * by);
            sy = sy + (az * bx - ax * bz);
            sz = sz + (ax * by - ay * bx);
        }
        area[3 * p] = 0.5 * sx; area[3 * p + 1] = 0.5 * sy; area[3 * p + 2] = 0.5 * sz;
    }
}

// the sampler's sites: per polygon (the owner, no offset) or per polygon vertex (the owner, x - x_owner as probe_walk_k forms it)
__global__ __launch_bounds__(kBlock) void cut_sites_k(MeshDev M, int64_t n, const int32_t *__restrict__ owner, const double *__restrict__ pts,
                                                      double *__restrict__ off) {
    GRID_STRIDE(i, n) {
        const int32_t c = owner[i];
        off[i] = pts ? pts[3 * i] - M.ccx[c] : 0.;
        off[n + i] = pts ? pts[3 * i + 1] - M.ccy[c] : 0.;
        off[2 * n + i] = pts ? pts[3 * i + 2] - M.ccz[c] : 0.;
    }
}

// ====================================================================== host side
// what one cut needs between its passes; the bench keeps one across its repetitions
struct Work {
    DevBuf<uint8_t> fcut;             // [F]
    DevBuf<int32_t> count;            // [n] by ORC id
    DevBuf<int2> sums, total;         // [chunks], [1]
    DevBuf<unsigned long long> skipped;  // [2]
    DevBuf<int32_t> cut_cells, cut_first;
};

int64_t chunks_of(int64_t n) { return std::max<int64_t>((n + kScanChunk - 1) / kScanChunk, 1); }

int launch_classify(const OrcMesh &m, const double *d, Work &W) {
    const CutDev N = cut_dev(m);
    hipLaunchKernelGGL(face_count_k, dim3(grid_for(m.n_faces)), dim3(kBlock), 0, ctx().stream, N, d, W.fcut.p);
    hipLaunchKernelGGL(cut_classify_k, dim3(grid_for(m.n_own)), dim3(kBlock), 0, ctx().stream, m.dev(), N.orc2int, W.fcut.p, W.count.p, W.skipped.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// sums and the scan of the sums; the totals stay on the device in W.total
template <class T>
int launch_scan(const T *in, int64_t n, Work &W) {
    const int64_t chunks = chunks_of(n);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(scan_sums_k<T>), dim3((unsigned)chunks), dim3(kBlock), 0, ctx().stream, in, n, W.sums.p);
    hipLaunchKernelGGL(scan_top_k, dim3(1), dim3(kBlock), 0, ctx().stream, W.sums.p, chunks, W.total.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}
template <class T>
int launch_place(const T *in, int64_t n, Work &W, int32_t *list, int32_t *list_off) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(scan_place_k<T>), dim3((unsigned)chunks_of(n)), dim3(kBlock), 0, ctx().stream, in, n, W.sums.p, list, list_off);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int alloc_work(const OrcMesh &m, Work &W) {
    ORC_TRY(W.fcut.alloc((size_t)std::max<int64_t>(m.n_faces, 1)));
    ORC_TRY(W.count.alloc((size_t)std::max<int64_t>(m.n_own, 1)));
    ORC_TRY(W.sums.alloc((size_t)chunks_of(m.n_own)));
    ORC_TRY(W.total.alloc(1));
    ORC_TRY(W.skipped.alloc(2));
    return W.skipped.zero();
}

int alloc_points(OrcCut &C, int64_t NP) {
    const size_t k = (size_t)std::max<int64_t>(NP, 1);
    ORC_TRY(C.points.alloc(3 * k)); ORC_TRY(C.klo.alloc(k)); ORC_TRY(C.khi.alloc(k)); ORC_TRY(C.owner.alloc(k)); ORC_TRY(C.lstart.alloc(k));
    // a cell that is not closed may emit fewer points than it was counted for: what it leaves stays zero, never undefined
    ORC_TRY(C.points.zero()); ORC_TRY(C.klo.zero()); ORC_TRY(C.khi.zero()); ORC_TRY(C.owner.zero());
    return C.lstart.zero();
}

int launch_emit(const OrcMesh &m, const double *d, const Work &W, int64_t n_cut, OrcCut &C) {
    if (n_cut < 1) return ORC_OK;
    EmitArgs A{d, W.count.p, W.cut_cells.p, W.cut_first.p, n_cut, C.points.p, C.klo.p, C.khi.p, C.owner.p, C.lstart.p};
    hipLaunchKernelGGL(cut_emit_k, dim3((unsigned)((n_cut + kEmitBlock - 1) / kEmitBlock)), dim3(kEmitBlock), 0, ctx().stream, m.dev(), cut_dev(m), A);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// poly_ptr from the loop-start flags, then owners and area vectors; P must be known (the flags' total)
int launch_polygons(Work &W, OrcCut &C) {
    if (C.P < 1) return ORC_OK;
    ORC_TRY(launch_place(C.lstart.p, C.NP, W, C.poly_ptr.p, (int32_t *)nullptr));
    hipLaunchKernelGGL(cut_polygons_k, dim3(grid_for(C.P)), dim3(kBlock), 0, ctx().stream, C.P, C.NP, C.poly_ptr.p, C.owner.p, C.points.p, C.cell.p, C.area.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// the surface d = 0 of the node function d [V] (device) through mesh m
int cut_build(OrcMesh &m, const double *d, OrcCut &C) {
    Work W;
    ORC_TRY(alloc_work(m, W));
    ORC_TRY(launch_classify(m, d, W));
    ORC_TRY(launch_scan(W.count.p, m.n_own, W));
    int2 total = make_int2(0, 0);
    ORC_TRY(W.total.download(&total, 1));  // the first wait: cut cells and NP (the skip counters lie ready behind it)
    unsigned long long skipped[2] = {0, 0};
    ORC_TRY(W.skipped.download(skipped, 2));
    C.n_nonfinite = (int64_t)skipped[0];
    C.n_overflow = (int64_t)skipped[1];
    const int64_t n_cut = total.x;
    C.NP = total.y;
    ORC_TRY(alloc_points(C, C.NP));
    ORC_TRY(W.cut_cells.alloc((size_t)std::max<int64_t>(n_cut, 1)));
    ORC_TRY(W.cut_first.alloc((size_t)std::max<int64_t>(n_cut, 1)));
    if (n_cut > 0) {
        ORC_TRY(launch_place(W.count.p, m.n_own, W, W.cut_cells.p, W.cut_first.p));
        ORC_TRY(launch_emit(m, d, W, n_cut, C));
        ORC_TRY(W.sums.ensure((size_t)chunks_of(C.NP)));
        ORC_TRY(launch_scan(C.lstart.p, C.NP, W));
        ORC_TRY(W.total.download(&total, 1));  // the second wait: P
        C.P = total.x;
    }
    ORC_TRY(C.poly_ptr.alloc((size_t)C.P + 1));
    ORC_TRY(C.poly_ptr.zero());
    ORC_TRY(C.cell.alloc((size_t)std::max<int64_t>(C.P, 1)));
    ORC_TRY(C.area.alloc((size_t)std::max<int64_t>(3 * C.P, 1)));
    ORC_TRY(launch_polygons(W, C));
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // the work buffers are freed on return
    return ORC_OK;
}

// the owners' ORC ids on the host, fetched once
int owners_on_host(const OrcCut &C) {
    if (C.h_cell_valid) return ORC_OK;
    std::vector<int32_t> h((size_t)C.P);
    ORC_TRY(C.cell.download(h.data(), (size_t)C.P));
    C.h_cell.resize((size_t)C.P);
    for (int64_t p = 0; p < C.P; ++p) C.h_cell[(size_t)p] = orc_cell_id(*C.mesh, h[(size_t)p]);
    C.h_cell_valid = true;
    return ORC_OK;
}

int require_nodes(const OrcMesh *m, const char *what) {
    if (!m) return set_error(ORC_ERR_BAD_ARGUMENT, "%s: null mesh", what);
    if (!m->nodes) return set_error(ORC_ERR_BAD_ARGUMENT, "%s: the mesh has no node geometry (orc_mesh_set_nodes)", what);
    return ORC_OK;
}

int launch_node_average(const OrcMesh &m, const double *phi_dev, double *out_dev) {
    hipLaunchKernelGGL(node_average_k, dim3(grid_for(m.nodes->n_vertices)), dim3(kBlock), 0, ctx().stream, m.dev(), cut_dev(m), phi_dev, out_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// d = value - level on the device, then the cut
OrcCut *cut_of_level(OrcMesh *m, const double *node_values_dev, double level, DevBuf<double> &d, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    const int64_t V = m->nodes->n_vertices;
    int st = d.alloc((size_t)V);
    if (st != ORC_OK) return fail(st);
    hipLaunchKernelGGL(node_level_k, dim3(grid_for(V)), dim3(kBlock), 0, ctx().stream, V, node_values_dev, level, d.p);
    std::unique_ptr<OrcCut> C(new OrcCut());
    C->mesh = m;
    if ((st = cut_build(*m, d.p, *C)) != ORC_OK) {
        (void)hipStreamSynchronize(ctx().stream);
        return fail(st);
    }
    if (status) *status = ORC_OK;
    return C.release();
}

OrcCut *cut_of_cell_field(OrcMesh *m, const double *phi_dev, double level, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    DevBuf<double> val, d;
    int st = val.alloc((size_t)m->nodes->n_vertices);
    if (st != ORC_OK || (st = launch_node_average(*m, phi_dev, val.p)) != ORC_OK) return fail(st);
    return cut_of_level(m, val.p, level, d, status);  // waits for the stream before val and d go
}

}  // namespace
}  // namespace orc

using namespace orc;

extern "C" {

int orc_cut_limits(int32_t *max_points, int32_t *scan_chunk) {
    if (max_points) *max_points = kCutMaxPoints;
    if (scan_chunk) *scan_chunk = kScanChunk;
    return ORC_OK;
}

int orc_mesh_set_nodes(OrcMesh *m, int64_t n_vertices, const double *vertices, int64_t n_faces, const int64_t *face_node_ptr, const int64_t *face_nodes) {
    ORC_TRY(ensure_init());
    if (!m || !vertices || !face_node_ptr || !face_nodes) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: null argument");
    if (m->halo.active())
        return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: a partitioned mesh is refused: a rank's polygons would end at its ghost layer, a node on the "
                                               "rank boundary would average over the cells of one rank only, and there is no gather of the pieces yet");
    const int64_t F = m->n_faces, n = m->n_cells;
    if (n_faces != F) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: %lld faces given, the mesh has %lld", (long long)n_faces, (long long)F);
    if (n_vertices < 1 || n_vertices >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: n_vertices must lie in [1, 2^31)");
    if (n > ((int64_t)1 << 31) / (2 * kCutMaxPoints)) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: mesh too large for 32-bit point offsets");
    if (face_node_ptr[0] != 0) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: face_node_ptr must start at 0");
    for (int64_t f = 0; f < F; ++f)
        if (face_node_ptr[f + 1] - face_node_ptr[f] < 3)
            return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: face %lld has %lld nodes, at least 3 are needed", (long long)f, (long long)(face_node_ptr[f + 1] - face_node_ptr[f]));
    const int64_t nfn = face_node_ptr[F];
    if (nfn >= ((int64_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: too many face nodes");
    for (int64_t i = 0; i < nfn; ++i)
        if (face_nodes[i] < 0 || face_nodes[i] >= n_vertices)
            return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: face node %lld names vertex %lld of %lld", (long long)i, (long long)face_nodes[i], (long long)n_vertices);
    for (int64_t i = 0; i < 3 * n_vertices; ++i)
        if (!std::isfinite(vertices[i])) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: coordinate %lld of vertex %lld is not finite", (long long)(i % 3), (long long)(i / 3));

    if (m->nodes) {  // built once per mesh: a later call is checked as the first was and must bring the same sizes
        if (m->nodes->n_vertices != n_vertices || m->nodes->n_face_nodes != nfn)
            return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: the mesh already holds other node geometry (%lld vertices, %lld face nodes)",
                             (long long)m->nodes->n_vertices, (long long)m->nodes->n_face_nodes);
        return ORC_OK;
    }
    std::unique_ptr<CutNodes> N(new CutNodes());
    N->n_vertices = n_vertices;
    N->n_face_nodes = nfn;
    std::vector<double> h((size_t)n_vertices);
    DevBuf<double> *dst[3] = {&N->vx, &N->vy, &N->vz};
    for (int q = 0; q < 3; ++q) {
        for (int64_t v = 0; v < n_vertices; ++v) h[(size_t)v] = vertices[3 * v + q];
        ORC_TRY(dst[q]->upload(h.data(), (size_t)n_vertices));
    }
    std::vector<int32_t> fnp(face_node_ptr, face_node_ptr + F + 1), fn(face_nodes, face_nodes + nfn);
    ORC_TRY(N->fnp.upload(fnp.data(), fnp.size()));
    ORC_TRY(N->fn.upload(fn.data(), std::max<size_t>(fn.size(), 1)));
    // node -> cells: the (node, ORC cell) pairs of every face, sorted and made unique; the device holds the internal ids
    std::vector<int32_t> c0((size_t)F), c1((size_t)F);
    ORC_TRY(m->c0.download(c0.data(), (size_t)F));
    ORC_TRY(m->c1.download(c1.data(), (size_t)F));
    const std::vector<int64_t> &g = cell_order_ids(*m);  // internal -> ORC, empty = identity
    auto orc_of = [&](int32_t c) { return g.empty() ? (int64_t)c : g[(size_t)c]; };
    std::vector<std::pair<int64_t, int32_t>> around;  // of one node: (ORC id, internal id)
    // two passes over the faces by node would need the inverse lists; instead gather per node through a face list of the nodes
    std::vector<int64_t> nfp((size_t)n_vertices + 1, 0);
    for (int64_t i = 0; i < nfn; ++i) ++nfp[(size_t)face_nodes[i] + 1];
    for (int64_t v = 0; v < n_vertices; ++v) nfp[(size_t)v + 1] += nfp[(size_t)v];
    std::vector<int32_t> nf((size_t)nfn);
    {
        std::vector<int64_t> cur(nfp.begin(), nfp.end() - 1);
        for (int64_t f = 0; f < F; ++f)
            for (int64_t i = face_node_ptr[f]; i < face_node_ptr[f + 1]; ++i) nf[(size_t)cur[(size_t)face_nodes[i]]++] = (int32_t)f;
    }
    std::vector<int32_t> ncp((size_t)n_vertices + 1, 0), nc;
    nc.reserve((size_t)nfn);
    for (int64_t v = 0; v < n_vertices; ++v) {
        around.clear();
        for (int64_t q = nfp[(size_t)v]; q < nfp[(size_t)v + 1]; ++q) {
            const int32_t f = nf[(size_t)q];
            for (int32_t c : {c0[(size_t)f], c1[(size_t)f]})
                if (c >= 0 && c < m->n_own) around.emplace_back(orc_of(c), c);
        }
        std::sort(around.begin(), around.end());
        around.erase(std::unique(around.begin(), around.end()), around.end());
        for (const auto &a : around) nc.push_back(a.second);
        if (nc.size() >= ((size_t)1 << 31)) return set_error(ORC_ERR_BAD_ARGUMENT, "set nodes: node -> cell table too large");
        ncp[(size_t)v + 1] = (int32_t)nc.size();
    }
    N->n_node_cells = (int64_t)nc.size();
    ORC_TRY(N->ncp.upload(ncp.data(), ncp.size()));
    ORC_TRY(N->nc.upload(nc.data(), std::max<size_t>(nc.size(), 1)));
    if (!g.empty()) {
        std::vector<int32_t> i2o(g.begin(), g.end()), o2i = internal_cell_ids(*m);
        ORC_TRY(N->int2orc.upload(i2o.data(), i2o.size()));
        ORC_TRY(N->orc2int.upload(o2i.data(), o2i.size()));
    }
    m->nodes = std::move(N);
    return ORC_OK;
}

int orc_mesh_node_average(OrcMesh *m, const double *cell_values, double *node_values) {
    ORC_TRY(ensure_init());
    ORC_TRY(require_nodes(m, "node average"));
    if (!cell_values || !node_values) return set_error(ORC_ERR_BAD_ARGUMENT, "node average: null argument");
    DevBuf<double> phi, out;
    ORC_TRY(upload_cells(*m, cell_values, phi));
    ORC_TRY(out.alloc((size_t)m->nodes->n_vertices));
    ORC_TRY(launch_node_average(*m, phi.p, out.p));
    return out.download(node_values, (size_t)m->nodes->n_vertices);
}

OrcCut *orc_cut_plane(OrcMesh *m, const double origin[3], const double normal[3], int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if ((st = require_nodes(m, "cut plane")) != ORC_OK) return fail(st);
    if (!origin || !normal) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut plane: null argument"));
    for (int q = 0; q < 3; ++q)
        if (!std::isfinite(origin[q]) || !std::isfinite(normal[q])) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut plane: origin and normal must be finite"));
    if (normal[0] == 0. && normal[1] == 0. && normal[2] == 0.) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut plane: the normal is zero"));
    DevBuf<double> d;
    const int64_t V = m->nodes->n_vertices;
    if ((st = d.alloc((size_t)V)) != ORC_OK) return fail(st);
    hipLaunchKernelGGL(node_plane_k, dim3(grid_for(V)), dim3(kBlock), 0, ctx().stream, cut_dev(*m), origin[0], origin[1], origin[2], normal[0], normal[1], normal[2], d.p);
    std::unique_ptr<OrcCut> C(new OrcCut());
    C->mesh = m;
    if ((st = cut_build(*m, d.p, *C)) != ORC_OK) {
        (void)hipStreamSynchronize(ctx().stream);
        return fail(st);
    }
    if (status) *status = ORC_OK;
    return C.release();
}

OrcCut *orc_cut_node_level(OrcMesh *m, const double *node_values, double level, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if ((st = require_nodes(m, "cut node level")) != ORC_OK) return fail(st);
    if (!node_values) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut node level: null argument"));
    if (!std::isfinite(level)) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut node level: the level is not finite"));
    DevBuf<double> val, d;
    if ((st = val.upload(node_values, (size_t)m->nodes->n_vertices)) != ORC_OK) return fail(st);
    return cut_of_level(m, val.p, level, d, status);
}

OrcCut *orc_cut_cell_field(OrcMesh *m, const double *cell_values, double level, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if ((st = require_nodes(m, "cut cell field")) != ORC_OK) return fail(st);
    if (!cell_values) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut cell field: null argument"));
    if (!std::isfinite(level)) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cut cell field: the level is not finite"));
    DevBuf<double> phi;
    if ((st = upload_cells(*m, cell_values, phi)) != ORC_OK) return fail(st);
    return cut_of_cell_field(m, phi.p, level, status);
}

OrcCut *orc_solver_cut_field(OrcSolver *s, uint32_t field_bit, double level, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCut *)nullptr; };
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if (!s) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "solver cut field: null solver"));
    SolverState &S = s->st;
    if ((st = require_nodes(S.mesh, "solver cut field")) != ORC_OK) return fail(st);
    if (field_bit == 0 || (field_bit & (field_bit - 1)) != 0 || (field_bit >> ORC_PROBE_N) != 0)
        return fail(set_error(ORC_ERR_BAD_ARGUMENT, "solver cut field: 0x%x is not exactly one OrcProbeField bit", field_bit));
    if (field_bit == (1u << ORC_PROBE_PHI) && !S.sc.on) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "solver cut field: PHI needs the scalar arm (orc_solver_set_scalar)"));
    if (!std::isfinite(level)) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "solver cut field: the level is not finite"));
    const SolverFields F = solver_field_table(S);
    const double *phi = F.src[__builtin_ctz(field_bit)];
    DevBuf<double> constant;
    if (!phi) {  // MU while the viscosity arm is off: the constant, as the probes sample it
        if ((st = constant.alloc((size_t)S.mesh->n_cells)) != ORC_OK) return fail(st);
        hipLaunchKernelGGL(fill_k, dim3(grid_for(S.mesh->n_cells)), dim3(kBlock), 0, ctx().stream, S.mesh->n_cells, F.mu, constant.p);
        phi = constant.p;
    }
    return cut_of_cell_field(S.mesh, phi, level, status);
}

void orc_cut_destroy(OrcCut *cut) {
    if (cut) (void)hipStreamSynchronize(ctx().stream);
    delete cut;
}

int orc_cut_sizes(const OrcCut *cut, int64_t *n_polygons, int64_t *n_points, int64_t *n_skipped_nonfinite, int64_t *n_skipped_overflow) {
    ORC_TRY(ensure_init());
    if (!cut) return set_error(ORC_ERR_BAD_ARGUMENT, "cut: null cut");
    if (n_polygons) *n_polygons = cut->P;
    if (n_points) *n_points = cut->NP;
    if (n_skipped_nonfinite) *n_skipped_nonfinite = cut->n_nonfinite;
    if (n_skipped_overflow) *n_skipped_overflow = cut->n_overflow;
    return ORC_OK;
}

int orc_cut_get(const OrcCut *cut, int64_t *poly_ptr, int64_t *cell, double *points, int64_t *key_lo, int64_t *key_hi, double *area_vector) {
    ORC_TRY(ensure_init());
    if (!cut) return set_error(ORC_ERR_BAD_ARGUMENT, "cut: null cut");
    const size_t P = (size_t)cut->P, NP = (size_t)cut->NP;
    std::vector<int32_t> h;
    if (poly_ptr) {
        h.resize(P + 1);
        ORC_TRY(cut->poly_ptr.download(h.data(), P + 1));
        std::copy(h.begin(), h.end(), poly_ptr);
        poly_ptr[P] = cut->NP;
    }
    if (cell) {
        ORC_TRY(owners_on_host(*cut));
        std::copy(cut->h_cell.begin(), cut->h_cell.end(), cell);
    }
    if (points && NP) ORC_TRY(cut->points.download(points, 3 * NP));
    const DevBuf<int32_t> *src[2] = {&cut->klo, &cut->khi};
    int64_t *dst[2] = {key_lo, key_hi};
    for (int q = 0; q < 2; ++q) {
        if (!dst[q] || !NP) continue;
        h.resize(NP);
        ORC_TRY(src[q]->download(h.data(), NP));
        std::copy(h.begin(), h.end(), dst[q]);
    }
    if (area_vector && P) ORC_TRY(cut->area.download(area_vector, 3 * P));
    return ORC_OK;
}

int orc_solver_sample_cut(OrcSolver *s, const OrcCut *cut, uint32_t field_mask, int32_t interpolation, double *out) {
    ORC_TRY(ensure_init());
    if (!s || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "sample cut: null argument");
    if (!cut) return set_error(ORC_ERR_BAD_ARGUMENT, "sample cut: null cut");
    SolverState &st = s->st;
    if (cut->mesh != st.mesh) return set_error(ORC_ERR_BAD_ARGUMENT, "sample cut: the cut was made in another mesh");
    ORC_TRY(validate_fields(st, field_mask, interpolation));
    const bool linear = interpolation == ORC_PROBE_LINEAR;
    const int64_t n = linear ? cut->NP : cut->P;
    if (n < 1) return ORC_OK;
    DevBuf<double> off;
    ORC_TRY(off.alloc(3 * (size_t)n));
    const int32_t *site = linear ? cut->owner.p : cut->cell.p;
    hipLaunchKernelGGL(cut_sites_k, dim3(grid_for(n)), dim3(kBlock), 0, ctx().stream, st.mesh->dev(), n, site, linear ? cut->points.p : (const double *)nullptr, off.p);
    ORC_HIP(hipGetLastError());
    return sample_to_host(st, site, off.p, n, field_mask, interpolation, nullptr, out);  // synchronises: off is freed on return
}

int orc_cut_sample_cells(const OrcCut *cut, int32_t n_fields, const double *fields, double *out) {
    ORC_TRY(ensure_init());
    if (!cut || !fields || !out) return set_error(ORC_ERR_BAD_ARGUMENT, "cut sample cells: null argument");
    if (n_fields < 1) return set_error(ORC_ERR_BAD_ARGUMENT, "cut sample cells: n_fields must be at least 1");
    const int64_t n = cut->mesh->n_cells;
    ORC_TRY(owners_on_host(*cut));
    for (int32_t k = 0; k < n_fields; ++k)
        for (int64_t p = 0; p < cut->P; ++p) out[(size_t)k * (size_t)cut->P + (size_t)p] = fields[(size_t)k * (size_t)n + (size_t)cut->h_cell[(size_t)p]];
    return ORC_OK;
}

int orc_bench_cut(OrcMesh *m, const double *cell_values, const double origin[3], const double normal[3], int reps, double avg_ms[4]) {
    ORC_TRY(ensure_init());
    ORC_TRY(require_nodes(m, "bench cut"));
    if (!cell_values || !origin || !normal || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench cut: null argument");
    if (reps < 1) reps = 1;
    const int64_t V = m->nodes->n_vertices;
    DevBuf<double> phi, val, d;
    ORC_TRY(upload_cells(*m, cell_values, phi));
    ORC_TRY(val.alloc((size_t)V));
    ORC_TRY(d.alloc((size_t)V));
    hipLaunchKernelGGL(node_plane_k, dim3(grid_for(V)), dim3(kBlock), 0, ctx().stream, cut_dev(*m), origin[0], origin[1], origin[2], normal[0], normal[1], normal[2], d.p);
    // one cut first: the sizes every pass works on
    Work W;
    OrcCut C;
    C.mesh = m;
    ORC_TRY(alloc_work(*m, W));
    ORC_TRY(launch_classify(*m, d.p, W));
    ORC_TRY(launch_scan(W.count.p, m->n_own, W));
    int2 total = make_int2(0, 0);
    ORC_TRY(W.total.download(&total, 1));
    const int64_t n_cut = total.x;
    C.NP = total.y;
    ORC_TRY(alloc_points(C, C.NP));
    ORC_TRY(W.cut_cells.alloc((size_t)std::max<int64_t>(n_cut, 1)));
    ORC_TRY(W.cut_first.alloc((size_t)std::max<int64_t>(n_cut, 1)));
    DevBuf<int2> sums2;  // the flags' scan has its own sums: the cells' stay valid for the placing pass
    ORC_TRY(sums2.alloc((size_t)chunks_of(C.NP)));
    if (n_cut > 0) {
        ORC_TRY(launch_place(W.count.p, m->n_own, W, W.cut_cells.p, W.cut_first.p));
        ORC_TRY(launch_emit(*m, d.p, W, n_cut, C));
        std::swap(W.sums, sums2);
        ORC_TRY(launch_scan(C.lstart.p, C.NP, W));
        ORC_TRY(W.total.download(&total, 1));
        C.P = total.x;
        std::swap(W.sums, sums2);
    }
    ORC_TRY(C.poly_ptr.alloc((size_t)C.P + 1));
    ORC_TRY(C.cell.alloc((size_t)std::max<int64_t>(C.P, 1)));
    ORC_TRY(C.area.alloc((size_t)std::max<int64_t>(3 * C.P, 1)));
    int status = ORC_OK;
    for (int pass = 0; pass < 4 && status == ORC_OK; ++pass) {
        auto launch = [&]() -> int {
            switch (pass) {
            case 0: return launch_node_average(*m, phi.p, val.p);
            case 1: return launch_classify(*m, d.p, W);
            case 2:
                ORC_TRY(launch_scan(W.count.p, m->n_own, W));
                return n_cut > 0 ? launch_place(W.count.p, m->n_own, W, W.cut_cells.p, W.cut_first.p) : ORC_OK;
            default: {
                ORC_TRY(launch_emit(*m, d.p, W, n_cut, C));
                if (C.P < 1) return ORC_OK;
                std::swap(W.sums, sums2);
                int st = launch_scan(C.lstart.p, C.NP, W);
                if (st == ORC_OK) st = launch_polygons(W, C);
                std::swap(W.sums, sums2);
                return st;
            }
            }
        };
        float ms = 0.f;
        status = timed(reps, launch, &ms, "timing the cut passes failed");
        avg_ms[pass] = (double)ms;
    }
    ORC_HIP(hipStreamSynchronize(ctx().stream));  // every buffer is freed on return
    return status;
}

}  // extern "C"
