// cell_order.cpp — see cell_order.hpp.
#include "cell_order.hpp"

namespace orc {

const std::vector<int64_t> &cell_order_ids(const OrcMesh &m) { return m.h_global_ids; }

int64_t orc_cell_id(const OrcMesh &m, int32_t internal) {
    return m.h_global_ids.empty() ? (int64_t)internal : m.h_global_ids[(size_t)internal];
}

std::vector<int32_t> internal_cell_ids(const OrcMesh &m) {
    const std::vector<int64_t> &g = m.h_global_ids;
    std::vector<int32_t> inv(g.size());
    for (size_t c = 0; c < g.size(); ++c) inv[(size_t)g[c]] = (int32_t)c;
    return inv;
}

int upload_cells(const OrcMesh &m, const double *src_orc, DevBuf<double> &dst, int fields) {
    const size_t n = (size_t)m.n_cells, total = (size_t)fields * n;
    const std::vector<int64_t> &g = m.h_global_ids;
    if (g.empty()) return dst.upload(src_orc, total);
    std::vector<double> tmp(total);
    for (int q = 0; q < fields; ++q)
        for (size_t c = 0; c < n; ++c) tmp[(size_t)q * n + c] = src_orc[(size_t)q * n + (size_t)g[c]];
    return dst.upload(tmp.data(), total);
}

int download_cells(const OrcMesh &m, const double *dev, double *dst_orc, int fields) {
    const size_t n = (size_t)m.n_cells, total = (size_t)fields * n;
    const std::vector<int64_t> &g = m.h_global_ids;
    std::vector<double> tmp(g.empty() ? 0 : total);
    if (total) ORC_HIP(hipMemcpyAsync(g.empty() ? dst_orc : tmp.data(), dev, total * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    ORC_HIP(hipStreamSynchronize(ctx().stream));
    for (int q = 0; q < fields && !g.empty(); ++q)
        for (size_t c = 0; c < n; ++c) dst_orc[(size_t)q * n + (size_t)g[c]] = tmp[(size_t)q * n + c];
    return ORC_OK;
}

}  // namespace orc
