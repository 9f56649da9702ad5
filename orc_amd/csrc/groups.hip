// groups.hip — volume reports (new-build extension; ORC reports no volume quantity): weighted sums, sums of squares, extrema and the
// cells of the extrema of cell fields over every group of a cell group set.  DESIGN.md §3 "Volume reports" has the definitions and the
// operator order; orc_types.h OrcGroupQuantity / OrcGroupWeighting name the outputs and the weights.
//
//   the group set (once, on the host: one stable counting sort of the labels in ORC order, then three uploads)
//     list              the cells of group 0, then of group 1, ...: ascending in ORC id inside a group, stored in the internal numbering
//     chunk table       every group's list cut from its start into pieces of at most kGroupChunk entries, none across two groups
//   a report (three launches per batch of <= kGroupFields fields on the library stream, fp64, no float atomics)
//     group_chunk_k     one workgroup per chunk: lane `tid` takes the entries begin + tid + 256 k in ascending k, a wave __shfl_down
//                       tree, the four waves through LDS in fixed order, everything behind one barrier -> partials[chunk][25]
//     group_fold_k      the group's chunks in chunk order, pairwise, level by level in place: one workgroup per 256 chunks, then one per
//                       group over the blocks' results -> rec[group][1 + 6 F]
// The association depends on the group set only (list order = ORC order, chunk table), never on a grid size or on the mesh's internal
// numbering: two reports of one state give the same bits, and so do a plain and a reordered mesh.
// Read-only towards mesh and solver, and opt-in: nothing here is launched unless a group entry is called or the history is on.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "assembly.hpp"
#include "cell_order.hpp"
#include "groups.hpp"
#include "probes.hpp"

namespace orc {

constexpr int kGroupFields = 4;                          // fields of one launch; more run in batches
constexpr int kGroupSlots = 8;                           // entries a lane of group_chunk_k takes at most
constexpr int kGroupRound = 4;                           // slots whose loads are in flight together
constexpr int kGroupChunk = kBlock * kGroupSlots;        // entries per workgroup
static_assert(kGroupSlots % kGroupRound == 0, "a lane's slots go in whole rounds");
constexpr int kGroupSums = 1 + 2 * kGroupFields;         // W, then SUM and SUM_SQ per field
constexpr int kGroupExtrema = 2 * kGroupFields;          // MIN and MAX per field
constexpr int kGroupPartial = kGroupSums + 2 * kGroupExtrema;  // doubles per chunk: the sums, then (value, list position) pairs
constexpr int kGroupFoldBlock = 256;                     // chunks one workgroup of the fold's first pass takes
constexpr int kGroupRecord = 6;                          // doubles per (group, field) of a record: SUM, SUM_SQ, MIN, MAX, two positions
static_assert(ORC_GROUP_N == 4 && ORC_GROUP_SUM == 0 && ORC_GROUP_SUM_SQ == 1 && ORC_GROUP_MIN == 2 && ORC_GROUP_MAX == 3,
              "the quantity order is part of the ABI (orc_amd/solver.py GroupReport)");
static_assert(kGroupSums + kGroupExtrema <= kBlock, "group_fold_k writes one quantity of the record per thread");

namespace {

struct GroupArgs {
    const int32_t *list;
    const int4 *chunk;  // {group, begin, count, 0}
    const double *vol;
    const double *x[kGroupFields];
    double cval;                    // kGroupConstLast: the value of the launch's last field in every cell (nothing is loaded for it)
    double div[kGroupFields];       // kGroupDivide: x is the stored value divided by this (1.0 leaves every bit as it is)
};

// What a launch does beside loading its fields.  A template parameter, not a per-field test in the kernel: a runtime "load or constant"
// choice per entry makes the compiler branch around every load and wait for each on its own.
enum GroupMode { kGroupPlain = 0, kGroupConstLast = 1, kGroupDivide = 2 };

// (x, i) replaces (m, p) as the minimum / maximum: a NaN never does (both comparisons are false), among equal values the smaller list
// position does, and "none yet" (p = -1) is the largest position of all.  Bitwise, not short-circuit: selects, no branches.
__device__ __forceinline__ bool beats_min(double x, int i, double m, int p) { return (x < m) | ((x == m) & ((unsigned)i < (unsigned)p)); }
__device__ __forceinline__ bool beats_max(double x, int i, double m, int p) { return (x > m) | ((x == m) & ((unsigned)i < (unsigned)p)); }

// One workgroup per chunk.  The lane's slots go in rounds of kGroupRound: the round's list entries are loaded, then its volumes and field
// values (every load of a round is issued before the first use), then the entries are accumulated in ascending k.  A slot past the
// chunk's end loads the chunk's last entry (always in bounds) and is not accumulated: selects, so that no branch stands between a
// round's loads.  Per entry: w, then per field t1 = w x, t2 = t1 x (separate multiplies), S = S + t1, Q = Q + t2; then per sum the wave
// tree of __shfl_down (offsets 32 .. 1) and ((w0 + w1) + w2) + w3 over the four waves through LDS.  Depth over a full chunk:
// kGroupSlots + 6 + 3 rounded additions.
template <int NF, bool kVol, int kMode>
__global__ __launch_bounds__(kBlock) void group_chunk_k(GroupArgs A, double *__restrict__ partials) {
    constexpr int NS = 1 + 2 * NF, NE = 2 * NF;
    constexpr int NL = kMode == kGroupConstLast ? NF - 1 : NF;  // fields that are loaded
    __shared__ double lds_s[kBlock / kWave][kGroupSums];
    __shared__ double lds_e[kBlock / kWave][kGroupExtrema];
    __shared__ int lds_p[kBlock / kWave][kGroupExtrema];
    const int4 c = A.chunk[blockIdx.x];
    const int begin = c.y, end = c.y + c.z;  // count >= 1: a group without a cell has no chunk
    double s[NS], e[NE];
    int p[NE];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.;
#pragma unroll
    for (int f = 0; f < NF; ++f) { e[2 * f] = INFINITY; e[2 * f + 1] = -INFINITY; p[2 * f] = p[2 * f + 1] = -1; }
#pragma unroll
    for (int k0 = 0; k0 < kGroupSlots; k0 += kGroupRound) {
        int cell[kGroupRound];
        double w[kGroupRound], x[kGroupRound][NF];
#pragma unroll
        for (int k = 0; k < kGroupRound; ++k) {
            const int i = begin + (k0 + k) * kBlock + (int)threadIdx.x;
            cell[k] = A.list[i < end ? i : end - 1];
        }
#pragma unroll
        for (int k = 0; k < kGroupRound; ++k) {
            w[k] = kVol ? A.vol[cell[k]] : 1.;
#pragma unroll
            for (int f = 0; f < NL; ++f) x[k][f] = A.x[f][cell[k]];
            if (kMode == kGroupConstLast) x[k][NF - 1] = A.cval;
        }
#pragma unroll
        for (int k = 0; k < kGroupRound; ++k) {
            const int i = begin + (k0 + k) * kBlock + (int)threadIdx.x;
            const bool valid = i < end;
            s[0] = valid ? s[0] + w[k] : s[0];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const double v = kMode == kGroupDivide ? x[k][f] / A.div[f] : x[k][f];
                const double t1 = w[k] * v;
                const double t2 = t1 * v;
                s[1 + 2 * f] = valid ? s[1 + 2 * f] + t1 : s[1 + 2 * f];
                s[2 + 2 * f] = valid ? s[2 + 2 * f] + t2 : s[2 + 2 * f];
                const bool lo = valid & beats_min(v, i, e[2 * f], p[2 * f]), hi = valid & beats_max(v, i, e[2 * f + 1], p[2 * f + 1]);
                e[2 * f] = lo ? v : e[2 * f]; p[2 * f] = lo ? i : p[2 * f];
                e[2 * f + 1] = hi ? v : e[2 * f + 1]; p[2 * f + 1] = hi ? i : p[2 * f + 1];
            }
        }
    }
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double t = wave_sum(s[q]);
        if (lane == 0) lds_s[wv][q] = t;
    }
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        double m = e[q];
        int pm = p[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double om = __shfl_down(m, o, 64);
            const int op = __shfl_down(pm, o, 64);
            if ((q & 1) ? beats_max(om, op, m, pm) : beats_min(om, op, m, pm)) { m = om; pm = op; }
        }
        if (lane == 0) { lds_e[wv][q] = m; lds_p[wv][q] = pm; }
    }
    __syncthreads();
    double *out = partials + (int64_t)blockIdx.x * kGroupPartial;
    if (threadIdx.x < NS) {
        const int q = threadIdx.x;
        out[q] = ((lds_s[0][q] + lds_s[1][q]) + lds_s[2][q]) + lds_s[3][q];
    } else if (threadIdx.x >= kWave && threadIdx.x < kWave + NE) {
        const int q = threadIdx.x - kWave;
        double m = lds_e[0][q];
        int pm = lds_p[0][q];
#pragma unroll
        for (int k = 1; k < kBlock / kWave; ++k)
            if ((q & 1) ? beats_max(lds_e[k][q], lds_p[k][q], m, pm) : beats_min(lds_e[k][q], lds_p[k][q], m, pm)) { m = lds_e[k][q]; pm = lds_p[k][q]; }
        out[kGroupSums + 2 * q] = m;
        out[kGroupSums + 2 * q + 1] = (double)pm;
    }
}

// The fold of a group's chunks c_0 .. c_{m-1} is ONE tree, the pairwise tree surface_fold_k walks with its stack: level by level at the
// strides s = 1, 2, 4, ..., c_i <- c_i + c_{i+s} (earlier + later) for every i that is a multiple of 2 s with i + s < m; a chunk
// without a partner moves up as it is; the result is c_0, depth ceil(log2 m).  The extrema take the same tree under the tie rule (any
// tree gives the same pair).  group_fold_k runs the levels of one task in place in `partials`, over the elements begin + j stride,
// j < n, one (pair, quantity) per thread and a barrier per level:
//   pass 1   one task per block of kGroupFoldBlock consecutive chunks of a group, counted from the group's first: stride 1, levels 1 .. 128
//   pass 2   one task per group over the first chunks of its blocks: stride kGroupFoldBlock, levels 256 and up; then the record of the
//            group: rec[g][0] = W, per field f0 + f: SUM, SUM_SQ, MIN, MAX, the list positions of MIN and MAX as doubles.  A group
//            without a chunk gives zeros, +inf, -inf and -1.
// One wave walking a group's chunks with the stack took 1.59 ms for the 5 000 chunks of one group of 10.24 M cells.
template <bool kFinal>
__global__ __launch_bounds__(kBlock) void group_fold_k(const int4 *__restrict__ tasks, int stride, double *partials, int nf, int f0, int n_fields,
                                                       double *__restrict__ rec) {
    const int4 t = tasks[blockIdx.x];
    const int begin = t.x, n = t.y;
    const int ns = 1 + 2 * nf, slots = ns + 2 * nf;
    for (int s = 1; s < n; s <<= 1) {
        const int pairs = (n - s + 2 * s - 1) / (2 * s);
        for (int item = threadIdx.x; item < pairs * slots; item += kBlock) {
            const int k = item / slots, q = item - k * slots;
            double *a = partials + ((int64_t)begin + (int64_t)(2 * s) * k * stride) * kGroupPartial;
            const double *b = a + (int64_t)s * stride * kGroupPartial;
            if (q < ns) {
                a[q] = a[q] + b[q];
            } else {
                const int x = q - ns, at = kGroupSums + 2 * x;  // x = 2 f + (0 = MIN, 1 = MAX)
                const double m = a[at], v = b[at];
                const int pm = (int)a[at + 1], pv = (int)b[at + 1];
                if ((x & 1) ? beats_max(v, pv, m, pm) : beats_min(v, pv, m, pm)) { a[at] = v; a[at + 1] = b[at + 1]; }
            }
        }
        __syncthreads();  // uniform: n is the task's
    }
    if (!kFinal) return;
    const int q = threadIdx.x;
    if (q >= slots) return;
    const double *a = partials + (int64_t)begin * kGroupPartial;  // not read when the group has no chunk
    double *out = rec + (int64_t)blockIdx.x * (1 + kGroupRecord * n_fields);
    if (q < ns) {
        const double r = n > 0 ? a[q] : 0.;
        if (q == 0) out[0] = r;
        else out[1 + kGroupRecord * (f0 + (q - 1) / 2) + ((q - 1) & 1)] = r;
    } else {
        const int x = q - ns;
        double *o = out + 1 + kGroupRecord * (f0 + x / 2);
        o[2 + (x & 1)] = n > 0 ? a[kGroupSums + 2 * x] : ((x & 1) ? -INFINITY : INFINITY);
        o[4 + (x & 1)] = n > 0 ? a[kGroupSums + 2 * x + 1] : -1.;
    }
}

// ====================================================================== host side
struct GroupField {
    const double *x = nullptr;  // device, the mesh's internal cell order; null: the constant cval in every cell
    double cval = 0.;
    double div = 0.;            // != 0: x is the stored value divided by it (a normalised co-moment of the statistics)
};

using ChunkKernel = void (*)(GroupArgs, double *);
template <bool kVol, int kMode>
ChunkKernel chunk_kernel_of(int nf) {
    static const ChunkKernel table[kGroupFields] = {group_chunk_k<1, kVol, kMode>, group_chunk_k<2, kVol, kMode>, group_chunk_k<3, kVol, kMode>,
                                                    group_chunk_k<4, kVol, kMode>};
    return table[nf - 1];
}
ChunkKernel chunk_kernel(int nf, bool vol, int mode) {
    if (mode == kGroupConstLast) return vol ? chunk_kernel_of<true, kGroupConstLast>(nf) : chunk_kernel_of<false, kGroupConstLast>(nf);
    if (mode == kGroupDivide) return vol ? chunk_kernel_of<true, kGroupDivide>(nf) : chunk_kernel_of<false, kGroupDivide>(nf);
    return vol ? chunk_kernel_of<true, kGroupPlain>(nf) : chunk_kernel_of<false, kGroupPlain>(nf);
}

size_t record_len(const OrcCellGroups &g, int n_fields) { return (size_t)g.n_groups * (size_t)(1 + kGroupRecord * n_fields); }

int launch_chunks(OrcCellGroups &g, const GroupField *f, int nf, int32_t weighting) {
    if (g.n_chunks == 0) return ORC_OK;
    GroupArgs A{};
    A.list = g.list.p; A.chunk = reinterpret_cast<const int4 *>(g.chunk.p); A.vol = g.mesh->vol.p;
    // a constant field (null pointer) is the last of its launch: the only one is MU, the last bit of a solver mask
    int mode = f[nf - 1].x ? kGroupPlain : kGroupConstLast;
    for (int k = 0; k < nf; ++k) {
        if (!f[k].x && k != nf - 1) return set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: a constant field must be the last of its launch");
        if (f[k].div != 0.) mode = kGroupDivide;
    }
    for (int k = 0; k < nf; ++k) { A.x[k] = f[k].x; A.div[k] = f[k].div != 0. ? f[k].div : 1.; }
    A.cval = f[nf - 1].cval;
    hipLaunchKernelGGL(chunk_kernel(nf, weighting == ORC_GROUP_WEIGHT_VOLUME, mode), dim3((unsigned)g.n_chunks), dim3(kBlock), 0, ctx().stream, A, g.partials.p);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

int launch_fold(OrcCellGroups &g, int nf, int f0, int n_fields, double *rec_dev) {
    if (g.n_fold_blocks > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(group_fold_k<false>), dim3((unsigned)g.n_fold_blocks), dim3(kBlock), 0, ctx().stream,
                           reinterpret_cast<const int4 *>(g.fold_blocks.p), 1, g.partials.p, nf, f0, n_fields, rec_dev);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(group_fold_k<true>), dim3((unsigned)g.n_groups), dim3(kBlock), 0, ctx().stream,
                       reinterpret_cast<const int4 *>(g.fold_groups.p), kGroupFoldBlock, g.partials.p, nf, f0, n_fields, rec_dev);
    ORC_HIP(hipGetLastError());
    return ORC_OK;
}

// the record [G][1 + 6 n_fields] of n_fields fields into rec_dev, in batches of kGroupFields; asynchronous on ctx().stream (the batches
// share the set's partials: the stream orders them)
int launch_report(OrcCellGroups &g, const GroupField *f, int n_fields, int32_t weighting, double *rec_dev) {
    for (int f0 = 0; f0 < n_fields; f0 += kGroupFields) {
        const int nf = std::min(kGroupFields, n_fields - f0);
        ORC_TRY(launch_chunks(g, f + f0, nf, weighting));
        ORC_TRY(launch_fold(g, nf, f0, n_fields, rec_dev));
    }
    return ORC_OK;
}

// a record on the host into the entries' outputs (each may be null): list positions become ORC ids, the count is the list's
void unpack(const OrcCellGroups &g, const double *rec, int n_fields, double *sums, double *weight, int64_t *where) {
    const size_t stride = (size_t)(1 + kGroupRecord * n_fields);
    for (size_t k = 0; k < (size_t)g.n_groups; ++k) {
        const double *r = rec + k * stride;
        if (weight) { weight[2 * k] = r[0]; weight[2 * k + 1] = (double)(g.h_group_ptr[k + 1] - g.h_group_ptr[k]); }
        for (size_t f = 0; f < (size_t)n_fields; ++f) {
            const double *q = r + 1 + kGroupRecord * f;
            if (sums) std::copy(q, q + ORC_GROUP_N, sums + (k * (size_t)n_fields + f) * ORC_GROUP_N);
            if (where)
                for (int e = 0; e < 2; ++e) where[(k * (size_t)n_fields + f) * 2 + (size_t)e] = q[4 + e] < 0. ? -1 : g.h_cells[(size_t)q[4 + e]];
        }
    }
}

// launch, download (the only synchronisation of a report), unpack
int report_host(OrcCellGroups &g, const GroupField *f, int n_fields, int32_t weighting, double *sums, double *weight, int64_t *where) {
    const size_t len = record_len(g, n_fields);
    ORC_TRY(g.rec.ensure(len));
    ORC_TRY(launch_report(g, f, n_fields, weighting, g.rec.p));
    std::vector<double> host(len);
    ORC_TRY(g.rec.download(host.data(), len));
    unpack(g, host.data(), n_fields, sums, weight, where);
    return ORC_OK;
}

int validate_weighting(int32_t weighting) {
    if (weighting != ORC_GROUP_WEIGHT_VOLUME && weighting != ORC_GROUP_WEIGHT_UNIT) return set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: unknown weighting %d", weighting);
    return ORC_OK;
}

int validate_groups(const OrcCellGroups *g, const OrcMesh *m) {
    if (!g) return set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: null group set");
    if (g->mesh != m) return set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: the group set was built for another mesh");
    return ORC_OK;
}

// the solver's fields of `mask` (OrcProbeField bits, ascending) as the kernels take them
int solver_fields(const SolverState &s, uint32_t mask, GroupField *f) {
    const SolverFields F = solver_field_table(s);
    int k = 0;
    for (int b = 0; b < ORC_PROBE_N; ++b) {
        if (!(mask >> b & 1)) continue;
        f[k].x = F.src[b];
        f[k].cval = b == ORC_PROBE_MU ? F.mu : 0.;
        ++k;
    }
    return k;
}

int validate_solver_report(const SolverState &s, const OrcCellGroups *g, uint32_t mask, int32_t weighting) {
    ORC_TRY(validate_groups(g, s.mesh));
    ORC_TRY(validate_fields(s, mask, ORC_PROBE_CELL));
    return validate_weighting(weighting);
}

// the record on its way, if any, joins the history as it is; its copy was started a step ago, so the wait is over before it begins
int history_flush(SolverState &s) {
    GroupHistory &H = s.gh;
    bool landed = false;
    ORC_TRY(H.raw.wait(&landed));
    if (!landed) return ORC_OK;
    H.values.insert(H.values.end(), H.raw.host.p, H.raw.host.p + record_len(*H.groups, H.n_fields));
    H.times.push_back(H.pending_time);
    return ORC_OK;
}

// one record of the current state, reduced and sent on its way
int history_enqueue(SolverState &s, double time) {
    GroupHistory &H = s.gh;
    GroupField f[ORC_PROBE_N];
    const int k = solver_fields(s, H.mask, f);
    ORC_TRY(launch_report(*H.groups, f, k, H.weighting, H.rec.p));
    ORC_TRY(H.raw.copy(0, H.rec.p, record_len(*H.groups, k) * sizeof(double)));
    ORC_TRY(H.raw.mark());
    H.pending_time = time;
    return ORC_OK;
}

int history_on(const SolverState &s) {
    if (!s.gh.on) return set_error(ORC_ERR_BAD_ARGUMENT, "group history: the history is off (orc_solver_set_group_history)");
    return ORC_OK;
}

}  // namespace

int groups_step_dev(SolverState &s) {
    if (!s.gh.on) return ORC_OK;
    ORC_TRY(history_flush(s));  // the previous record: this step's iterations have synchronised the stream since
    return s.gh.due() ? history_enqueue(s, s.time) : ORC_OK;
}

}  // namespace orc

using namespace orc;

extern "C" {

OrcCellGroups *orc_cell_groups_create(OrcMesh *m, int32_t n_groups, const int32_t *group_of_cell, int *status) {
    auto fail = [&](int st) { if (status) *status = st; return (OrcCellGroups *)nullptr; };
    if (status) *status = ORC_OK;
    int st = ensure_init();
    if (st != ORC_OK) return fail(st);
    if (!m || !group_of_cell) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: null argument"));
    if (n_groups < 1 || n_groups > ORC_GROUP_MAX_GROUPS)
        return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: n_groups must lie in [1, %d]", (int)ORC_GROUP_MAX_GROUPS));
    if (m->halo.active())
        return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: a partitioned mesh is refused: the association of a report is defined on one process's "
                                                    "list, and there is no combination across ranks yet"));
    if (m->n_cells >= ((int64_t)1 << 31)) return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: mesh too large"));
    const size_t n = (size_t)m->n_cells, G = (size_t)n_groups;
    for (size_t c = 0; c < n; ++c)
        if (group_of_cell[c] < -1 || group_of_cell[c] >= n_groups)
            return fail(set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: cell %lld has group %d outside [-1, %d)", (long long)c, group_of_cell[c], n_groups));
    std::unique_ptr<OrcCellGroups> X(new OrcCellGroups());
    X->mesh = m;
    X->n_groups = n_groups;
    // one stable counting sort over the cells in ORC order: a group's list ascends in ORC id
    X->h_group_ptr.assign(G + 1, 0);
    for (size_t c = 0; c < n; ++c)
        if (group_of_cell[c] >= 0) ++X->h_group_ptr[(size_t)group_of_cell[c] + 1];
    for (size_t k = 0; k < G; ++k) X->h_group_ptr[k + 1] += X->h_group_ptr[k];
    X->n_listed = X->h_group_ptr[G];
    X->h_cells.assign((size_t)X->n_listed, 0);
    std::vector<int32_t> list((size_t)std::max<int64_t>(X->n_listed, 1), 0);
    const std::vector<int32_t> internal = internal_cell_ids(*m);  // empty = identity
    {
        std::vector<int64_t> next(X->h_group_ptr.begin(), X->h_group_ptr.end() - 1);
        for (size_t c = 0; c < n; ++c) {
            if (group_of_cell[c] < 0) continue;
            const size_t pos = (size_t)next[(size_t)group_of_cell[c]]++;
            X->h_cells[pos] = (int64_t)c;
            list[pos] = internal.empty() ? (int32_t)c : internal[c];
        }
    }
    std::vector<int32_t> chunk, blocks, tasks;
    for (size_t k = 0; k < G; ++k) {
        const int32_t lo = (int32_t)(chunk.size() / 4);
        for (int64_t b = X->h_group_ptr[k]; b < X->h_group_ptr[k + 1]; b += kGroupChunk) {
            const int64_t e = std::min<int64_t>(b + kGroupChunk, X->h_group_ptr[k + 1]);
            chunk.push_back((int32_t)k); chunk.push_back((int32_t)b); chunk.push_back((int32_t)(e - b)); chunk.push_back(0);
        }
        const int32_t m = (int32_t)(chunk.size() / 4) - lo;
        for (int32_t b = 0; b < m; b += kGroupFoldBlock) {  // the fold's first pass: blocks of chunks counted from the group's first
            blocks.push_back(lo + b); blocks.push_back(std::min<int32_t>(kGroupFoldBlock, m - b)); blocks.push_back(0); blocks.push_back(0);
        }
        tasks.push_back(lo); tasks.push_back((m + kGroupFoldBlock - 1) / kGroupFoldBlock); tasks.push_back(0); tasks.push_back(0);
    }
    X->n_chunks = (int64_t)(chunk.size() / 4);
    X->n_fold_blocks = (int64_t)(blocks.size() / 4);
    if (chunk.empty()) chunk.assign(4, 0);
    if (blocks.empty()) blocks.assign(4, 0);
    if ((st = X->list.upload(list.data(), list.size())) != ORC_OK || (st = X->chunk.upload(chunk.data(), chunk.size())) != ORC_OK ||
        (st = X->fold_blocks.upload(blocks.data(), blocks.size())) != ORC_OK || (st = X->fold_groups.upload(tasks.data(), tasks.size())) != ORC_OK ||
        (st = X->partials.alloc((size_t)std::max<int64_t>(X->n_chunks, 1) * kGroupPartial)) != ORC_OK)
        return fail(st);
    return X.release();
}

void orc_cell_groups_destroy(OrcCellGroups *g) {
    if (g) (void)hipStreamSynchronize(ctx().stream);
    delete g;
}

int32_t orc_cell_groups_count(const OrcCellGroups *g) { return g ? g->n_groups : 0; }

int orc_cell_groups_get(const OrcCellGroups *g, int64_t *group_ptr, int64_t *cells, int32_t *chunk) {
    if (!g) return set_error(ORC_ERR_BAD_ARGUMENT, "cell groups: null group set");
    if (group_ptr) std::copy(g->h_group_ptr.begin(), g->h_group_ptr.end(), group_ptr);
    if (cells) std::copy(g->h_cells.begin(), g->h_cells.end(), cells);
    if (chunk) *chunk = kGroupChunk;
    return ORC_OK;
}

int orc_group_limits(int32_t *fields_per_launch, int32_t *chunk, int32_t *slots, int32_t *max_groups) {
    if (fields_per_launch) *fields_per_launch = kGroupFields;
    if (chunk) *chunk = kGroupChunk;
    if (slots) *slots = kGroupSlots;
    if (max_groups) *max_groups = ORC_GROUP_MAX_GROUPS;
    return ORC_OK;
}

int orc_solver_group_report(OrcSolver *s, OrcCellGroups *g, uint32_t field_mask, int32_t weighting, double *sums, double *weight, int64_t *where) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(validate_solver_report(st, g, field_mask, weighting));
    GroupField f[ORC_PROBE_N];
    const int k = solver_fields(st, field_mask, f);
    return report_host(*g, f, k, weighting, sums, weight, where);
}

int orc_group_integrals(OrcMesh *m, OrcCellGroups *g, int32_t n_fields, const double *fields, int32_t weighting, double *sums, double *weight,
                        int64_t *where) {
    ORC_TRY(ensure_init());
    if (!m || !fields) return set_error(ORC_ERR_BAD_ARGUMENT, "group integrals: null argument");
    ORC_TRY(validate_groups(g, m));
    if (n_fields < 1 || n_fields > ORC_GROUP_MAX_FIELDS)
        return set_error(ORC_ERR_BAD_ARGUMENT, "group integrals: n_fields must lie in [1, %d]", (int)ORC_GROUP_MAX_FIELDS);
    ORC_TRY(validate_weighting(weighting));
    DevBuf<double> dev;
    ORC_TRY(upload_cells(*m, fields, dev, n_fields));
    std::vector<GroupField> f((size_t)n_fields);
    for (int k = 0; k < n_fields; ++k) f[(size_t)k].x = dev.p + (size_t)k * (size_t)m->n_cells;
    return report_host(*g, f.data(), n_fields, weighting, sums, weight, where);  // synchronises: dev is freed on return
}

int orc_solver_group_statistics(OrcSolver *s, OrcCellGroups *g, uint32_t stat_field_mask, int32_t form, int32_t weighting, double *sums,
                                double *weight, int64_t *where) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    const TimeStats &T = st.ts;
    ORC_TRY(validate_groups(g, st.mesh));
    if (!T.on) return set_error(ORC_ERR_BAD_ARGUMENT, "group statistics: the arm is off (orc_solver_set_time_statistics)");
    if (stat_field_mask == 0 || (stat_field_mask & ~T.field_mask))
        return set_error(ORC_ERR_BAD_ARGUMENT, "group statistics: mask 0x%x selects nothing, an unknown field or a field whose group is off", stat_field_mask);
    if (form != ORC_STAT_RAW && form != ORC_STAT_NORMALISED) return set_error(ORC_ERR_BAD_ARGUMENT, "group statistics: unknown form %d", form);
    if (form == ORC_STAT_NORMALISED && T.samples == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "group statistics: NORMALISED needs at least one sample");
    ORC_TRY(validate_weighting(weighting));
    GroupField f[ORC_STAT_N];
    int slot = 0, k = 0;  // slot: row of the accumulator buffer; k: field of the report
    for (int b = 0; b < ORC_STAT_N; ++b) {
        if (!(T.field_mask >> b & 1)) continue;
        const double *src = T.acc.p + (size_t)slot++ * (size_t)st.n;
        if (!(stat_field_mask >> b & 1)) continue;
        const bool mean = b <= ORC_STAT_P || b == ORC_STAT_MU || b == ORC_STAT_PHI;
        f[k].x = src;
        f[k].div = form == ORC_STAT_NORMALISED && !mean ? T.W : 0.;  // what orc_solver_get_statistics divides by, on the host
        ++k;
    }
    return report_host(*g, f, k, weighting, sums, weight, where);
}

int orc_solver_set_group_history(OrcSolver *s, OrcCellGroups *g, uint32_t field_mask, int32_t weighting, uint64_t interval) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    if (!g) {  // off: advance launches nothing of the history from here on
        st.gh.clear();
        return ORC_OK;
    }
    ORC_TRY(validate_solver_report(st, g, field_mask, weighting));
    if (interval == 0) return set_error(ORC_ERR_BAD_ARGUMENT, "group history: interval must be at least 1");
    GroupHistory H;
    const int k = H.n_fields = popcount32(field_mask);
    const size_t len = record_len(*g, k);
    ORC_TRY(H.rec.alloc(len));
    // one record of the current state first: its W (a property of the group set and the weighting) is what the read-out returns
    GroupField f[ORC_PROBE_N];
    (void)solver_fields(st, field_mask, f);
    std::vector<double> first(len);
    ORC_TRY(launch_report(*g, f, k, weighting, H.rec.p));
    ORC_TRY(H.rec.download(first.data(), len));
    H.w_of.resize((size_t)g->n_groups);
    for (size_t q = 0; q < H.w_of.size(); ++q) H.w_of[q] = first[q * (size_t)(1 + kGroupRecord * k)];
    ORC_TRY(H.raw.create(len, "group history"));
    H.groups = g;
    H.mask = field_mask;
    H.weighting = weighting;
    H.interval = interval;
    H.on = true;
    st.gh.clear();
    st.gh = std::move(H);
    return ORC_OK;
}

int orc_solver_record_groups(OrcSolver *s, double tag) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(history_on(st));
    ORC_TRY(history_flush(st));
    ORC_TRY(history_enqueue(st, tag));
    return history_flush(st);
}

int64_t orc_solver_group_history_count(OrcSolver *s) {
    if (ensure_init() != ORC_OK) return -1;
    if (!s) { (void)set_error(ORC_ERR_BAD_ARGUMENT, "null solver"); return -1; }
    if (history_on(s->st) != ORC_OK || history_flush(s->st) != ORC_OK) return -1;
    return (int64_t)s->st.gh.times.size();
}

int orc_solver_group_history(OrcSolver *s, uint64_t first, uint64_t count, double *times, double *sums, double *weight, int64_t *where) {
    ORC_TRY(ensure_init());
    if (!s) return set_error(ORC_ERR_BAD_ARGUMENT, "null solver");
    SolverState &st = s->st;
    ORC_TRY(history_on(st));
    ORC_TRY(history_flush(st));
    const GroupHistory &H = st.gh;
    ORC_TRY(history_range("group history", first, count, H.times.size()));
    const OrcCellGroups &g = *H.groups;
    const size_t len = record_len(g, H.n_fields), per = (size_t)g.n_groups * (size_t)H.n_fields;
    if (times) std::copy(H.times.begin() + (ptrdiff_t)first, H.times.begin() + (ptrdiff_t)(first + count), times);
    for (uint64_t r = 0; r < count; ++r)
        unpack(g, H.values.data() + (size_t)(first + r) * len, H.n_fields, sums ? sums + (size_t)r * per * ORC_GROUP_N : nullptr, nullptr,
               where ? where + (size_t)r * per * 2 : nullptr);
    for (size_t k = 0; weight && k < (size_t)g.n_groups; ++k) {
        weight[2 * k] = H.w_of[k];
        weight[2 * k + 1] = (double)(g.h_group_ptr[k + 1] - g.h_group_ptr[k]);
    }
    return ORC_OK;
}

int orc_bench_group_report(OrcSolver *s, OrcCellGroups *g, uint32_t field_mask, int32_t weighting, int reps, double avg_ms[2]) {
    ORC_TRY(ensure_init());
    if (!s || !avg_ms) return set_error(ORC_ERR_BAD_ARGUMENT, "bench group report: null argument");
    SolverState &st = s->st;
    ORC_TRY(validate_solver_report(st, g, field_mask, weighting));
    GroupField f[ORC_PROBE_N];
    const int k = solver_fields(st, field_mask, f);
    if (k > kGroupFields) return set_error(ORC_ERR_BAD_ARGUMENT, "bench group report: at most %d fields (one batch)", kGroupFields);
    if (reps < 1) reps = 1;
    ORC_TRY(g->rec.ensure(record_len(*g, k)));
    int status = ORC_OK;
    for (int pass = 0; pass < 2 && status == ORC_OK; ++pass) {  // the warm call of the fold reads the chunk pass's partials
        float ms = 0.f;
        status = timed(reps, [&] { return pass == 0 ? launch_chunks(*g, f, k, weighting) : launch_fold(*g, k, 0, k, g->rec.p); }, &ms,
                       "timing the group passes failed");
        avg_ms[pass] = (double)ms;
    }
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    return status;
}

}  // extern "C"
