// The query body of csrc/sqgr_anchor.hip is host-callable: this wrapper lays the grids out with the library's own planner, fills
// the cell lists with plain loops (count, exclusive scan, scatter — the kernels' steps) and runs every (query, set) search on the
// CPU, so that the ring walk, its pruning and its stop rule can be checked without a device
// (tests/test_var_by_distance_cpu.py builds it into a scratch directory and calls it through ctypes).
#include "sqgr_anchor.hip"

using namespace sqgr;

namespace {

template <int DIM, int METRIC>
void run(const std::vector<AnchorGrid>& grids, int64_t cells, const double* q, int64_t nq, const double* r, const int32_t* r_set, int64_t nr,
         double* out, int64_t* walks) {
    std::vector<int32_t> start((size_t)cells + 1, 0), cell_of((size_t)nr);
    for (int64_t j = 0; j < nr; ++j) {
        cell_of[j] = anchor_cell_of<DIM>(grids[r_set[j]], r + j * DIM);
        ++start[(size_t)cell_of[j] + 1];
    }
    for (int64_t c = 0; c < cells; ++c) start[c + 1] += start[c];
    std::vector<int32_t> cursor(start.begin(), start.end() - 1);
    std::vector<APoint<DIM>> pts((size_t)std::max<int64_t>(nr, 1));
    for (int64_t j = nr - 1; j >= 0; --j) {  // (any order inside a cell)
        APoint<DIM> t = {};
        for (int k = 0; k < DIM; ++k) t.c[k] = r[j * DIM + k];
        pts[(size_t)cursor[cell_of[j]]++] = t;
    }
    for (size_t s = 0; s < grids.size(); ++s)
        for (int64_t i = 0; i < nq; ++i) {
            AnchorWalk w = {0, 0, 0};
            double d = __builtin_nan("");
            if (grids[s].count > 0) {
                d = anchor_query<DIM, METRIC, true>(grids[s], pts.data(), start.data(), q + i * DIM, &w);
                if (METRIC == 0) d = std::sqrt(d);
            }
            out[s * nq + i] = d;
            walks[3 * (s * nq + i)] = w.rings;
            walks[3 * (s * nq + i) + 1] = w.reached;
            walks[3 * (s * nq + i) + 2] = w.read;
        }
}

}  // namespace

// out: [n_sets][nq]; walks: [n_sets][nq][3] = rings entered, cells of the runs the loops reached (pruned or not), cells read;
// grid_out: [n_sets][8] = cells per axis (x, y, z), the points of the set, the cell side, the box's lower corner (x, y, z)
extern "C" int twin_anchor(int dim, int metric, const double* q, int64_t nq, const double* r, const int32_t* r_set, int64_t nr, int32_t n_sets,
                           int64_t brute_below, double target, double* out, int64_t* walks, double* grid_out) {
    std::vector<AnchorGrid> grids;
    int64_t cells = 0;
    const int rc = anchor_plan(dim, r, r_set, nr, n_sets, brute_below, target, grids, &cells);
    if (rc) return rc;
    for (int32_t s = 0; s < n_sets; ++s) {
        for (int a = 0; a < 3; ++a) grid_out[8 * s + a] = grids[s].g[a];
        grid_out[8 * s + 3] = grids[s].count;
        grid_out[8 * s + 4] = grids[s].h;
        for (int a = 0; a < 3; ++a) grid_out[8 * s + 5 + a] = grids[s].o[a];
    }
#define TWIN(D, M) run<D, M>(grids, cells, q, nq, r, r_set, nr, out, walks)
    if (dim == 2) {
        if (metric == 0) TWIN(2, 0); else if (metric == 1) TWIN(2, 1); else TWIN(2, 2);
    } else {
        if (metric == 0) TWIN(3, 0); else if (metric == 1) TWIN(3, 1); else TWIN(3, 2);
    }
#undef TWIN
    return 0;
}
