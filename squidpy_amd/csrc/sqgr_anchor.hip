// libsqgr: distance from every observation to the nearest member of each anchor set — the search of `var_by_distance`
// (tl/_var_by_distance.py:129-134: one sklearn KDTree per (anchor, slide), queried with every observation of the slide).
//
// Reference arithmetic (sklearn's KD-tree, checked bit for bit): the differences are accumulated in coordinate order without
// FMA — euclidean sqrt(min((dx*dx + dy*dy) + dz*dz)), manhattan min((|dx| + |dy|) + |dz|), chebyshev min(max |d|).
//
// MI355X design: every reference set (the members of one anchor in one slide, or a one-point custom anchor) gets its own uniform
// grid of square / cubic cells over its bounding box; all grids live in one concatenated cell table with one descriptor per set.
// The cell lists are built on the device (count per cell, exclusive scan, scatter); the order inside a cell is arbitrary and a
// minimum does not depend on it.  A set below ANCHOR_BRUTE_BELOW points gets one cell: the same kernel then sweeps it whole.
// One thread per (query, anchor column) walks the rings of cells around the query's clamped cell, keeping one best value:
//   - a run of cells is read only if its box can hold a closer point (gap of the query to the run, in the metric);
//   - the walk ends when no cell outside the visited block can hold a closer point.  What lies outside the block lies behind one
//     of its faces AND inside the set's bounding box, so the bound of a face combines the distance to that face with the query's
//     gaps to the box along the other axes; a face at the grid's edge has nothing behind it.  A query far outside the box — the
//     usual case: an anchor structure sits in one corner of the tissue — therefore stops after the few cells facing it.
// Both tests are exact: gaps are lower bounds of |coordinate differences| (with a slack for cell rounding), and the metrics are
// monotone in every |difference| under IEEE rounding, so a bound computed in the distance's own operation order never exceeds
// the computed distance of a point it covers.  DESIGN 3.13.
#include "sqgr_common.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

namespace sqgr {

constexpr int ANCHOR_T = 128;              // threads of a block (as the other one-walk-per-thread searches)
constexpr int64_t ANCHOR_BRUTE_BELOW = 32;  // sets with fewer points: one cell (the sweep of tools/var_by_distance_time.py: a tie at 16, the grid ahead from 32 on)
constexpr int64_t ANCHOR_PER_CELL = 2;      // target points per cell (the hook takes a fraction)
constexpr int ANCHOR_MAX_COLUMNS = 65535;  // anchor columns of one call (a grid dimension)

struct AnchorGrid {
    double o[3];    // lower corner of the bounding box
    double ext[3];  // its extent: every point has 0 <= v - o <= ext
    double h, inv_h;
    int32_t g[3];   // cells per axis
    int32_t cell0;  // first entry of the set in the cell table
    int32_t count;  // points of the set
    int32_t pad;
};

template <int DIM>
struct APoint;
template <>
struct alignas(16) APoint<2> {
    double c[2];
};
template <>
struct alignas(32) APoint<3> {
    double c[3];
    double pad;
};

__host__ __device__ __forceinline__ int anchor_cell(double u, double inv_h, int g) {
    const double c = floor(u * inv_h);  // clamped as a double: a far-away query never reaches the int conversion
    return (int)fmin(fmax(c, 0.0), (double)(g - 1));
}

template <int DIM>
__host__ __device__ __forceinline__ int anchor_cell_of(const AnchorGrid& g, const double* __restrict__ v) {
    int cell = 0;
#pragma unroll
    for (int a = DIM - 1; a >= 0; --a) cell = cell * g.g[a] + anchor_cell(v[a] - g.o[a], g.inv_h, g.g[a]);  // x fastest
    return g.cell0 + cell;
}

__host__ __device__ __forceinline__ double anchor_mul(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dmul_rn(a, b);  // never fused
#else
    return a * b;  // the build sets -ffp-contract=off
#endif
}
__host__ __device__ __forceinline__ double anchor_add(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}

// the metric of three coordinate differences (the third is 0 in 2-D) in its reduced form: squared for euclidean.  Monotone in
// every |d|: also the lower bound of a box from the gaps to it.
template <int DIM, int METRIC>
__host__ __device__ __forceinline__ double anchor_metric(double dx, double dy, double dz) {
    if (METRIC == 0) {
        const double s = anchor_add(anchor_mul(dx, dx), anchor_mul(dy, dy));
        return DIM == 3 ? anchor_add(s, anchor_mul(dz, dz)) : s;
    }
    if (METRIC == 1) {
        const double s = anchor_add(fabs(dx), fabs(dy));
        return DIM == 3 ? anchor_add(s, fabs(dz)) : s;
    }
    const double s = fmax(fabs(dx), fabs(dy));
    return DIM == 3 ? fmax(s, fabs(dz)) : s;
}

// lower bound of |u - v| over the points of cells lo .. hi of one axis (v: offset from the box's corner).  An edge cell ends at
// the box, where the clamping put everything beyond the last cell boundary.
__host__ __device__ __forceinline__ double anchor_gap(double u, int lo, int hi, int g, double h, double ext, double slack) {
    const double a = (lo == 0 ? 0.0 : (double)lo * h) - slack;
    const double b = (hi == g - 1 ? ext : (double)(hi + 1) * h) + slack;
    return fmax(fmax(a - u, u - b), 0.0);
}

// what one walk did (the host twin's counters): rings entered, cells of the runs the loops reached (pruned or not), cells read
struct AnchorWalk {
    int64_t rings, reached, read;
};

// The search of one query against one set: the reduced distance (squared for euclidean) to the nearest point, +inf for an empty
// set.  pts: the points of all sets in cell order; cell_start[c] .. cell_start[c + 1]: members of cell c of the concatenated
// table.  COUNT: *walk is filled.  Host-callable, so that the walk and its stop rule can be run on a CPU.
template <int DIM, int METRIC, bool COUNT>
__host__ __device__ __forceinline__ double anchor_query(const AnchorGrid& g, const APoint<DIM>* __restrict__ pts, const int32_t* __restrict__ cell_start,
                                                        const double* __restrict__ q, AnchorWalk* walk) {
    using std::max;
    using std::min;
    const double inf = __builtin_inf();
    double u[3] = {0.0, 0.0, 0.0}, qq[3] = {0.0, 0.0, 0.0}, sl[3] = {0.0, 0.0, 0.0}, box[3] = {0.0, 0.0, 0.0};
    int c[3] = {0, 0, 0};
    int rmax = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        qq[a] = q[a];
        u[a] = qq[a] - g.o[a];  // offsets from the grid's corner, as the cell of a point is computed from them
        c[a] = anchor_cell(u[a], g.inv_h, g.g[a]);
        rmax = max(rmax, max(c[a], g.g[a] - 1 - c[a]));
        // cell rounding (at most 2^19 cells per axis: below 5e-10 h) and the rounding of u against q - p for a query far away
        sl[a] = 1e-9 * g.h + 4.5e-16 * fabs(u[a]);
        box[a] = fmax(fmax(-sl[a] - u[a], u[a] - (g.ext[a] + sl[a])), 0.0);  // gap to the whole bounding box
    }
    const int g0 = g.g[0], g1 = g.g[1], g2 = DIM == 3 ? g.g[2] : 1;
    double best = inf;
    for (int r = 0; r <= rmax; ++r) {
        if (COUNT) ++walk->rings;
        // Only the cells within reach of the best value so far, two cells of margin, are walked at all: along every axis a point
        // closer than `best` lies within `reach` of the query (every metric here is at least each |difference|).  For a query far
        // outside the box the ring is then a few cells of the side facing it, not a ring.
        const double reach = METRIC == 0 ? sqrt(best) : best;
        int rlo[3] = {0, 0, 0}, rhi[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            rlo[a] = max(anchor_cell(u[a] - reach, g.inv_h, g.g[a]) - 2, 0);
            rhi[a] = min(anchor_cell(u[a] + reach, g.inv_h, g.g[a]) + 2, g.g[a] - 1);
        }
        // surface of the block [c - r, c + r]^DIM: the two z faces whole; of the planes between them the two y rows whole and
        // of the remaining rows the two end cells
        for (int zz = max(c[2] - r, rlo[2]); zz <= min(c[2] + r, DIM == 3 ? rhi[2] : 0); ++zz) {
            const bool zface = DIM == 3 && ((zz == c[2] - r) || (zz == c[2] + r));
            const double bz = DIM == 3 ? anchor_gap(u[2], zz, zz, g2, g.h, g.ext[2], sl[2]) : 0.0;
            for (int yy = max(c[1] - r, rlo[1]); yy <= min(c[1] + r, rhi[1]); ++yy) {
                const bool whole = zface || (yy == c[1] - r) || (yy == c[1] + r);
                const double by = anchor_gap(u[1], yy, yy, g1, g.h, g.ext[1], sl[1]);
                const int row = g.cell0 + (zz * g1 + yy) * g0;
                for (int seg = 0; seg < (whole ? 1 : 2); ++seg) {
                    int lo, hi;
                    if (whole) {  // cells along x are adjacent in memory: the run is one range of points
                        lo = max(c[0] - r, rlo[0]);
                        hi = min(c[0] + r, rhi[0]);
                        if (lo > hi) continue;
                    } else {
                        lo = hi = seg ? c[0] + r : c[0] - r;
                        if (lo < rlo[0] || lo > rhi[0]) continue;
                    }
                    if (COUNT) walk->reached += hi - lo + 1;
                    const double bx = anchor_gap(u[0], lo, hi, g0, g.h, g.ext[0], sl[0]);
                    if (anchor_metric<DIM, METRIC>(bx, by, bz) >= best) continue;  // nothing in this run is closer
                    if (COUNT) walk->read += hi - lo + 1;
                    const int pe = cell_start[row + hi + 1];
                    for (int p = cell_start[row + lo]; p < pe; ++p) {
                        const APoint<DIM> t = pts[p];
                        best = fmin(best, anchor_metric<DIM, METRIC>(qq[0] - t.c[0], qq[1] - t.c[1], DIM == 3 ? qq[2] - t.c[DIM - 1] : 0.0));
                    }
                }
            }
        }
        // everything not yet visited lies behind a face of the block that the grid reaches beyond, and inside the bounding box
        double m = inf;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            double d[3] = {box[0], box[1], box[2]};
            if (c[a] - r > 0) {
                d[a] = fmax(u[a] - ((double)(c[a] - r) * g.h + sl[a]), 0.0);
                m = fmin(m, anchor_metric<DIM, METRIC>(d[0], d[1], d[2]));
            }
            if (c[a] + r < g.g[a] - 1) {
                d[a] = fmax(((double)(c[a] + r + 1) * g.h - sl[a]) - u[a], 0.0);
                m = fmin(m, anchor_metric<DIM, METRIC>(d[0], d[1], d[2]));
            }
        }
        if (best <= m) break;  // (m == inf: the block covers the grid)
    }
    return best;
}

// out[a][i] for anchor column a = blockIdx.y: consecutive lanes take consecutive queries of one column, so a wave writes one
// contiguous run and — with the observations in a spatial order — walks the same few cells.
template <int DIM, int METRIC>
__global__ __launch_bounds__(ANCHOR_T) void k_anchor_query(const double* __restrict__ q, const int32_t* __restrict__ q_slide, int64_t nq,
                                                            const AnchorGrid* __restrict__ grids, const int32_t* __restrict__ set_of, int n_slides,
                                                            const APoint<DIM>* __restrict__ pts, const int32_t* __restrict__ cell_start,
                                                            double* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)ANCHOR_T + threadIdx.x;
    if (i >= nq) return;
    const int a = blockIdx.y;
    double res = __builtin_nan("");
    const int slide = q_slide[i];
    if (slide >= 0) {
        const int s = set_of[(int64_t)a * n_slides + slide];
        if (s >= 0 && grids[s].count > 0) {
            const AnchorGrid g = grids[s];
            double qv[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) qv[k] = q[i * DIM + k];
            res = anchor_query<DIM, METRIC, false>(g, pts, cell_start, qv, nullptr);
            if (METRIC == 0) res = __dsqrt_rn(res);
        }
    }
    out[(int64_t)a * nq + i] = res;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_anchor_count(const double* __restrict__ r, const int32_t* __restrict__ r_set, int64_t nr,
                                                       const AnchorGrid* __restrict__ grids, int32_t* __restrict__ cell_of, int32_t* __restrict__ counts) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= nr) return;
    double v[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) v[k] = r[j * DIM + k];
    const int cell = anchor_cell_of<DIM>(grids[r_set[j]], v);
    cell_of[j] = cell;
    atomicAdd(&counts[cell], 1);
}

// counts[c] still holds the members of cell c: it is the cursor, counted down (the order inside a cell is irrelevant to a minimum)
template <int DIM>
__global__ __launch_bounds__(256) void k_anchor_scatter(const double* __restrict__ r, int64_t nr, const int32_t* __restrict__ cell_of,
                                                         const int32_t* __restrict__ cell_start, int32_t* __restrict__ counts, APoint<DIM>* __restrict__ pts) {
    const int64_t j = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (j >= nr) return;
    const int cell = cell_of[j];
    const int pos = cell_start[cell] + atomicSub(&counts[cell], 1) - 1;
    APoint<DIM> t = {};
#pragma unroll
    for (int k = 0; k < DIM; ++k) t.c[k] = r[j * DIM + k];
    pts[pos] = t;
}

// cell side for ~target points per cell of a set that fills its bounding box evenly.  Only the axes wider than a cell count: a
// flat axis holds a single layer of cells, so a plane in 3-D gets square cells sized in 2-D and a single site one cell.
inline double anchor_side(const double ext[3], int64_t n, double target) {
    bool active[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
    for (;;) {
        int dims = 0;
        double logv = 0.0;
        for (int a = 0; a < 3; ++a)
            if (active[a]) {
                ++dims;
                logv += std::log(ext[a]);
            }
        if (dims == 0) return 1.0;
        const double h = std::exp((logv + std::log(target / (double)n)) / dims);
        int thin = -1;
        for (int a = 0; a < 3; ++a)
            if (active[a] && ext[a] < h && (thin < 0 || ext[a] < ext[thin])) thin = a;
        if (thin < 0) return h;
        active[thin] = false;
    }
}

// Checks the reference points and lays out one grid per set: bounding boxes in one pass on the host (the pass that refuses
// non-finite coordinates), cells of side >= widest / 2^19 (the walk's rounding slack), at most 4 n + 64 cells per set.
inline int anchor_plan(int dim, const double* r, const int32_t* r_set, int64_t nr, int32_t n_sets, int64_t brute_below, double target,
                       std::vector<AnchorGrid>& grids, int64_t* total_cells) {
    grids.assign((size_t)n_sets, AnchorGrid{});
    std::vector<double> hi((size_t)n_sets * 3, 0.0);
    for (int64_t j = 0; j < nr; ++j) {
        const int32_t s = r_set[j];
        SQGR_REQUIRE(s >= 0 && s < n_sets, "reference point %lld: set %d is not in [0, %d)", (long long)j, s, n_sets);
        AnchorGrid& g = grids[s];
        for (int a = 0; a < dim; ++a) {
            const double v = r[j * dim + a];
            SQGR_REQUIRE(std::isfinite(v), "reference point %lld: a coordinate is not finite", (long long)j);
            if (g.count == 0) g.o[a] = hi[3 * s + a] = v;
            g.o[a] = std::min(g.o[a], v);
            hi[3 * s + a] = std::max(hi[3 * s + a], v);
        }
        ++g.count;
    }
    int64_t cells = 0;
    for (int32_t s = 0; s < n_sets; ++s) {
        AnchorGrid& g = grids[s];
        double widest = 0.0;
        for (int a = 0; a < 3; ++a) {
            g.ext[a] = a < dim ? hi[3 * s + a] - g.o[a] : 0.0;
            widest = std::max(widest, g.ext[a]);
            g.g[a] = 1;
        }
        SQGR_REQUIRE(std::isfinite(widest), "set %d: the coordinate range is not finite", s);
        double h = widest > 0.0 ? widest : 1.0;  // one cell: the whole set is swept
        if (g.count >= brute_below && g.count > 1 && widest > 0.0) {
            h = std::max(anchor_side(g.ext, g.count, target), widest / 524288.0);  // a set of identical points keeps one cell
            if (!(h > 0.0) || !std::isfinite(h)) h = widest;
            const double cap = (double)std::min<int64_t>(4 * (int64_t)g.count + 64, (int64_t)1 << 30);
            for (;; h *= 1.25) {
                double vol = 1.0;
                for (int a = 0; a < dim; ++a) vol *= std::floor(g.ext[a] / h) + 1.0;
                if (vol <= cap) break;
            }
            for (int a = 0; a < dim; ++a) g.g[a] = (int)std::floor(g.ext[a] / h) + 1;
        }
        g.h = h;
        g.inv_h = 1.0 / h;
        SQGR_REQUIRE(std::isfinite(g.inv_h), "set %d: the coordinate range is too small for a cell grid", s);
        g.cell0 = (int32_t)cells;
        cells += (int64_t)g.g[0] * g.g[1] * g.g[2];
        SQGR_REQUIRE(cells < (int64_t)0x7fffffff, "more than 2^31 cells");
    }
    *total_cells = cells;
    return SQGR_OK;
}

namespace {

template <int DIM>
int anchor_search(sqgr_ctx* ctx, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set, int64_t nr,
                  const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, const std::vector<AnchorGrid>& grids, int64_t cells,
                  double* out, int64_t* query_launches) {
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n_pairs = (size_t)n_anchors * n_slides;
    DevBuf<double> d_q, d_r, d_out;
    DevBuf<int32_t> d_slide, d_rset, d_setof, d_cell_of, d_counts, d_start;
    DevBuf<AnchorGrid> d_grids;
    DevBuf<APoint<DIM>> d_pts;
    SQGR_TRY(d_q.alloc_pooled((size_t)nq * DIM));
    SQGR_TRY(d_slide.alloc_pooled((size_t)nq));
    SQGR_TRY(d_r.alloc_pooled((size_t)nr * DIM));
    SQGR_TRY(d_rset.alloc_pooled((size_t)nr));
    SQGR_TRY(d_setof.alloc_pooled(n_pairs));
    SQGR_TRY(d_grids.alloc_pooled(grids.size()));
    SQGR_TRY(d_cell_of.alloc_pooled((size_t)nr));
    SQGR_TRY(d_counts.alloc_pooled((size_t)cells + 1));
    SQGR_TRY(d_start.alloc_pooled((size_t)cells + 1));
    SQGR_TRY(d_pts.alloc_pooled((size_t)nr));
    SQGR_TRY(d_out.alloc_pooled((size_t)n_anchors * nq));
    SQGR_HIP(hipMemcpyAsync(d_q.p, q, (size_t)nq * DIM * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(d_slide.p, q_slide, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(d_setof.p, set_of, n_pairs * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(d_grids.p, grids.data(), grids.size() * sizeof(AnchorGrid), hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemsetAsync(d_counts.p, 0, ((size_t)cells + 1) * 4, st));
    if (nr) {
        SQGR_HIP(hipMemcpyAsync(d_r.p, r, (size_t)nr * DIM * 8, hipMemcpyHostToDevice, st));
        SQGR_HIP(hipMemcpyAsync(d_rset.p, r_set, (size_t)nr * 4, hipMemcpyHostToDevice, st));
        LaunchTimer t(ctx, "anchor_count");
        k_anchor_count<DIM><<<(unsigned)ceil_div(nr, 256), 256, 0, st>>>(d_r.p, d_rset.p, nr, d_grids.p, d_cell_of.p, d_counts.p);
        SQGR_HIP(hipGetLastError());
    }
    {
        size_t tmp_bytes = 0;
        SQGR_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_counts.p, d_start.p, (int)(cells + 1), st));
        void* tmp = nullptr;  // the context's reusable scratch: no allocator call per search
        SQGR_TRY(ctx->scratch_get(7, tmp_bytes, &tmp));
        LaunchTimer t(ctx, "anchor_scan");
        SQGR_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d_counts.p, d_start.p, (int)(cells + 1), st));
    }
    if (nr) {
        LaunchTimer t(ctx, "anchor_scatter");
        k_anchor_scatter<DIM><<<(unsigned)ceil_div(nr, 256), 256, 0, st>>>(d_r.p, nr, d_cell_of.p, d_start.p, d_counts.p, d_pts.p);
        SQGR_HIP(hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "anchor_query");
        const dim3 grid((unsigned)ceil_div(nq, ANCHOR_T), (unsigned)n_anchors);
#define SQGR_ANCHOR(M) k_anchor_query<DIM, M><<<grid, ANCHOR_T, 0, st>>>(d_q.p, d_slide.p, nq, d_grids.p, d_setof.p, n_slides, d_pts.p, d_start.p, d_out.p)
        if (metric == 0) SQGR_ANCHOR(0); else if (metric == 1) SQGR_ANCHOR(1); else SQGR_ANCHOR(2);
#undef SQGR_ANCHOR
        SQGR_HIP(hipGetLastError());
        ++*query_launches;
    }
    SQGR_HIP(hipMemcpyAsync(out, d_out.p, (size_t)n_anchors * nq * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int anchor_dist(sqgr_ctx* ctx, int32_t dim, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set, int64_t nr,
                const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, double* out, int64_t* out_stats, int64_t brute_below,
                double target) {
    SQGR_REQUIRE(ctx && q && q_slide && set_of && out && out_stats, "null argument");
    SQGR_REQUIRE(dim == 2 || dim == 3, "Expected coordinates of width 2 or 3, found %d", dim);
    SQGR_REQUIRE(nq >= 1 && nq < (int64_t)0x7fffffff, "nq=%lld out of range", (long long)nq);
    SQGR_REQUIRE(nr >= 0 && nr < (int64_t)0x7fffffff, "nr=%lld out of range", (long long)nr);
    SQGR_REQUIRE(nr == 0 || (r && r_set), "null argument");
    SQGR_REQUIRE(n_anchors >= 1 && n_anchors <= ANCHOR_MAX_COLUMNS, "n_anchors=%d is not in [1, %d]", n_anchors, ANCHOR_MAX_COLUMNS);
    SQGR_REQUIRE(n_slides >= 1 && (int64_t)n_anchors * n_slides < (int64_t)0x7fffffff, "n_slides=%d out of range", n_slides);
    SQGR_REQUIRE(metric >= 0 && metric <= 2, "metric %d is not one of 0 euclidean, 1 manhattan, 2 chebyshev", metric);
    SQGR_REQUIRE(brute_below >= 0 && target >= 0.0 && std::isfinite(target), "brute_below=%lld, target_per_cell=%g", (long long)brute_below, target);
    int32_t n_sets = 0;
    for (int64_t p = 0; p < (int64_t)n_anchors * n_slides; ++p) {
        SQGR_REQUIRE(set_of[p] >= -1, "set_of[%lld]=%d", (long long)p, set_of[p]);
        SQGR_REQUIRE(set_of[p] < (int64_t)n_anchors * n_slides, "set_of[%lld]=%d: set ids stay below the number of (anchor, slide) pairs", (long long)p, set_of[p]);
        n_sets = std::max(n_sets, set_of[p] + 1);
    }
    for (int64_t i = 0; i < nq; ++i) {
        SQGR_REQUIRE(q_slide[i] >= -1 && q_slide[i] < n_slides, "query %lld: slide %d is not in [-1, %d)", (long long)i, q_slide[i], n_slides);
        for (int a = 0; a < dim; ++a) SQGR_REQUIRE(std::isfinite(q[i * dim + a]), "query %lld: a coordinate is not finite", (long long)i);
    }
    std::vector<AnchorGrid> grids;
    int64_t cells = 0;
    SQGR_TRY(anchor_plan(dim, r, r_set, nr, std::max(n_sets, 1), brute_below ? brute_below : ANCHOR_BRUTE_BELOW, target > 0.0 ? target : (double)ANCHOR_PER_CELL,
                         grids, &cells));
    int64_t query_launches = 0;
    if (dim == 2) SQGR_TRY(anchor_search<2>(ctx, q, q_slide, nq, r, r_set, nr, set_of, n_anchors, n_slides, metric, grids, cells, out, &query_launches));
    else SQGR_TRY(anchor_search<3>(ctx, q, q_slide, nq, r, r_set, nr, set_of, n_anchors, n_slides, metric, grids, cells, out, &query_launches));
    int64_t gridded = 0;
    for (const AnchorGrid& g : grids) gridded += (int64_t)g.g[0] * g.g[1] * g.g[2] > 1;
    out_stats[0] = cells;
    out_stats[1] = gridded;
    out_stats[2] = query_launches;
    out_stats[3] = nr;
    return SQGR_OK;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_anchor_dist_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = ANCHOR_BRUTE_BELOW;
    out_info[1] = ANCHOR_PER_CELL;
    out_info[2] = 3;
    out_info[3] = ANCHOR_MAX_COLUMNS;
    out_info[4] = ANCHOR_T;
    return SQGR_OK;
}

int sqgr_anchor_dist(sqgr_ctx* ctx, int32_t dim, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set, int64_t nr,
                     const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, double* out, int64_t* out_stats) {
    return anchor_dist(ctx, dim, q, q_slide, nq, r, r_set, nr, set_of, n_anchors, n_slides, metric, out, out_stats, 0, 0.0);
}

int sqgr_anchor_dist_hook(sqgr_ctx* ctx, int32_t dim, const double* q, const int32_t* q_slide, int64_t nq, const double* r, const int32_t* r_set,
                          int64_t nr, const int32_t* set_of, int32_t n_anchors, int32_t n_slides, int32_t metric, double* out, int64_t* out_stats,
                          int64_t brute_below, double target_per_cell) {
    return anchor_dist(ctx, dim, q, q_slide, nq, r, r_set, nr, set_of, n_anchors, n_slides, metric, out, out_stats, brute_below, target_per_cell);
}
