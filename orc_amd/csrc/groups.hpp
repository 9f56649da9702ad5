// groups.hpp — the cell group set of groups.hip as the solver state sees it.
#pragma once
#include <vector>

#include "assembly.hpp"

// A labelling of the cells of one mesh, as lists: group g owns list positions [h_group_ptr[g], h_group_ptr[g + 1]), its cells ascending
// in ORC id.  The lists live on the device in the mesh's internal numbering, cut into chunks of at most kGroupChunk entries of ONE group;
// a report's partial sums and its folded record live here too, so that a report allocates nothing.
struct OrcCellGroups {
    OrcMesh *mesh = nullptr;
    int32_t n_groups = 0;
    int64_t n_listed = 0, n_chunks = 0;
    std::vector<int64_t> h_group_ptr;     // [G + 1] into the list
    std::vector<int64_t> h_cells;         // [n_listed] ORC ids, ascending inside a group
    orc::DevBuf<int32_t> list;            // [n_listed] the same cells in the mesh's internal numbering
    orc::DevBuf<int32_t> chunk;           // [n_chunks][4] = {group, begin, count, 0}
    int64_t n_fold_blocks = 0;
    orc::DevBuf<int32_t> fold_blocks;     // [n_fold_blocks][4] = {first chunk, chunks, 0, 0}: <= 256 consecutive chunks of ONE group
    orc::DevBuf<int32_t> fold_groups;     // [G][4] = {the group's first chunk, its blocks, 0, 0}
    orc::DevBuf<double> partials;         // [n_chunks][kGroupPartial]
    orc::DevBuf<double> rec;              // a record of the entries that download at once: [G][1 + 6 F]
};
