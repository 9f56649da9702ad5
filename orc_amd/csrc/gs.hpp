// gs.hpp — what the Gauss-Seidel sources share (gs_coloring.hip, gs_layout.hip, gs_sweep.hip, gs_slot.hip); nothing else
// includes it: arms.hpp and linalg.hpp declare what the rest of the library calls.
//
// Multicolour Gauss-Seidel: NEW-BUILD EXTENSION, no reference counterpart.
// ORC's Gauss-Seidel arm scans every (i, j) through get() — which panics on the first structural zero of a sparse
// matrix — and ends in panic!("Gauss-Seidel out for maintenance :)") (linear_algebra.rs:219-246); its
// PreconditionMethod knows only None | Jacobi (lib.rs:181-185).  BASELINE configs 3/4 nevertheless ask for
// "multicolour GS-preconditioned BiCGSTAB" and an "AMG V-cycle (GS smoother)", so these files provide
//   ORC_SOLVER_MULTICOLOR_GS        iteration_count sweeps of the reference's row update (:225-239) in colour order,
//   ORC_SOLVER_BICGSTAB_GS_PRECOND  the reference's BiCGSTAB recurrences, right-preconditioned by one GS sweep,
//   ORC_SOLVER_MULTIGRID_GS         the Multigrid arm with GS sweeps as its smoother (amg_cycle.hip).
// The colouring is proper on the pattern of A united with its transpose: no stored a_ij or a_ji joins two rows of one
// colour, whether or not the pattern is structurally symmetric.  So a colour is one fully parallel kernel and the sweep
// is a true Gauss-Seidel in colour order; the row sum runs in ascending-column order like everything else.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "linalg_kernels.hpp"

namespace orc {

// Colour-sorted copy of a pattern: the rows of a colour are contiguous ("slots": rows by colour, ascending inside a colour),
// every colour starts on a slice boundary, columns keep their original numbering.  A sweep over one colour is then a
// product-like pass over a contiguous slice range with fully coalesced matrix reads; with the rows left in mesh order every
// colour's kernel touches every cache line of the matrix (n_colors times the traffic).  Pointers and sizes only:
// build_sorted_layout (gs_layout.hip) is the one place that fills it.
struct SortedLayout {
    const int64_t *sp = nullptr;                                  // [n_slices + 1]
    const int *row_len = nullptr, *rowid = nullptr, *diag_off = nullptr;  // per slot: entries, original row (-1: padding slot), element offset of the diagonal (-1: none)
    const int *col = nullptr;                                     // [padded] original column indices
    const int *cslot = nullptr;                                   // [padded] the slot of that column's row (-1: ghost column): what the slot-space solver gathers through
    const int *slot_of_row = nullptr;                             // [n] what sorted_values permutes a solve's values through
    int n_slices = 0;
    int64_t n_slots = 0, padded = 0;
};

// Colouring and colour-sorted layout of one pattern.  The arrays of a persistent pattern (the mesh pattern of a solver)
// are owned here and cached; those of a pattern that lives for one solve (coarse AMG levels) sit in the solve's arena.
struct Coloring {
    int n_colors = 0;
    const int *color = nullptr;    // [n]
    std::vector<int> start;        // [n_colors + 1] rows before every colour
    SortedLayout layout;
    std::vector<int> color_slice;  // [n_colors + 1] first slice of every colour
    struct Owned {
        DevBuf<int> color, row_len, rowid, diag_off, col, cslot, slot_of_row;
        DevBuf<int64_t> sp;
    } own;
};

// gs_coloring.hip
// arena == nullptr: C.own keeps the colours; otherwise they live in the arena
int build_coloring(const SellDev &P, Coloring &C, Arena *arena);
// The colouring, the layout and this solve's values in that layout (*val, in the arena) for A.  A persistent pattern's
// colouring and layout come from the cache; every other pattern gets them built now, in the arena, and `owned` holds them.
int gs_prepare(const MatView &A, Arena &arena, std::unique_ptr<Coloring> &owned, const Coloring **out, const double **val);

// gs_layout.hip
// C.layout and C.color_slice from C's colours.  cached: the arrays go to C.own and only the pattern is laid out (val == nullptr);
// otherwise everything is allocated in the arena and *val receives A's values in the layout.
int build_sorted_layout(const MatView &A, Coloring &C, Arena &arena, bool cached, const double **val);
// A's values (the view's scalings applied) in the layout L of A's pattern, in the arena
int sorted_values(const MatView &A, const SortedLayout &L, Arena &arena, const double **val);

// gs_slot.hip
// the GS-preconditioned BiCGSTAB of one system in slot space; b, x in row order (x in / out)
int gsx_bicgstab1(const Coloring &C, const double *val, const double *b, double *x, uint64_t iteration_count, Arena &arena, int *status);

__device__ __forceinline__ bool fin_nz(double v) { return v != 0. && isfinite(v); }

}  // namespace orc
