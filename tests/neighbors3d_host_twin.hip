// The query bodies of csrc/sqgr_neighbors3d.hip are host-callable: this wrapper runs the cell-list builder and every query on
// the CPU, so that the shell walk, its stop rule and the cell sizing can be checked without a device
// (tests/test_neighbors3d_cpu.py builds it into a scratch directory and calls it through ctypes).
#include "sqgr_neighbors3d.hip"

using namespace sqgr;

// grid_out: h, gx, gy, gz, occupied cells, most points in one cell
extern "C" int twin_knn3(const double* xyz, int64_t n, int k, int32_t* idx, double* d2, double* grid_out) {
    HostGrid3 hg;
    const int rc = build_grid3(xyz, n, 2.0, 0.0, hg);
    if (rc) return rc;
    double occupied = 0, most = 0;
    for (size_t c = 0; c + 1 < hg.cell_start.size(); ++c) {
        const int m = hg.cell_start[c + 1] - hg.cell_start[c];
        occupied += m > 0;
        most = std::max(most, (double)m);
    }
    const double g[6] = {hg.g.h, (double)hg.g.gx, (double)hg.g.gy, (double)hg.g.gz, occupied, most};
    for (int i = 0; i < 6; ++i) grid_out[i] = g[i];
    const Point3* pts = hg.pts.data();
    const int32_t *lay = hg.layer_of.data(), *nxt = hg.next_layer.data(), *cs = hg.cell_start.data();
    for (int64_t t = 0; t < n; ++t) {
        if (k <= 4) knn_query3<4>(hg.g, pts, lay, nxt, cs, t, k, idx, d2);
        else if (k <= 8) knn_query3<8>(hg.g, pts, lay, nxt, cs, t, k, idx, d2);
        else if (k <= 16) knn_query3<16>(hg.g, pts, lay, nxt, cs, t, k, idx, d2);
        else if (k <= 32) knn_query3<32>(hg.g, pts, lay, nxt, cs, t, k, idx, d2);
        else knn_query3<64>(hg.g, pts, lay, nxt, cs, t, k, idx, d2);
    }
    return 0;
}

// the count pass (idx == NULL) or both passes; returns the number of neighbours, -1 on error
extern "C" int64_t twin_radius3(const double* xyz, int64_t n, double r, int64_t* indptr, int32_t* idx, double* d2) {
    HostGrid3 hg;
    if (build_grid3(xyz, n, 2.0, r / 4.0, hg)) return -1;
    const Point3* pts = hg.pts.data();
    const int32_t *lay = hg.layer_of.data(), *nxt = hg.next_layer.data(), *cs = hg.cell_start.data();
    std::vector<int64_t> cnt((size_t)n);
    for (int64_t t = 0; t < n; ++t) radius_query3<true>(hg.g, pts, lay, nxt, cs, t, r, r * r, cnt.data(), nullptr, nullptr, nullptr);
    indptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) indptr[i + 1] = indptr[i] + cnt[i];
    if (idx)
        for (int64_t t = 0; t < n; ++t) radius_query3<false>(hg.g, pts, lay, nxt, cs, t, r, r * r, nullptr, indptr, idx, d2);
    return indptr[n];
}
