// libsqgr: spatial graph construction in 3-D — exact k-nearest-neighbour and fixed-radius neighbour search on
// (n, 3) coordinates (stacked serial sections, volumetric MERFISH / STARmap, z-resolved Stereo-seq).
//
// Reference semantics: the same sklearn calls as the 2-D search (sqgr_neighbors.hip), which take coordinates of
// any width — gr/neighbors.py:196-199, 402-405 (kneighbors) and :252-255 (radius_neighbors).  sklearn's KD-tree
// accumulates the squared distance coordinate by coordinate without FMA, so d2 = (dx*dx + dy*dy) + dz*dz, and tests the
// radius on squared distances (d2 <= r*r).
//
// MI355X design: a uniform grid of cubic cells over the bounding box, built by a counting sort on the host; points
// lie in cell order (x fastest, then y, then z), so a run of cells along x is one contiguous range of points.  Layers
// of cells (one z index) that hold no point are not stored: sections stacked far apart cost one table entry per empty
// layer between them, not a plane of empty cells.  One thread per query walks cubic shells of cells around its own cell and keeps the k best (d2, index) pairs in
// registers.  Exact and deterministic: ties are broken by the smaller sample index.  The 2-D kernels and the 2-D
// cell list (sqgr_grid.h) are separate code and are not touched by anything here.
#include "sqgr_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sqgr {

struct CellGrid3 {
    double x0, y0, z0, inv_h, h;
    int gx, gy, gz;
};

// one point of the cell-ordered list: a query reads a candidate with one 32-byte access instead of four gathers
struct alignas(32) Point3 {
    double x, y, z;
    int32_t id;
    int32_t pad;
};

__host__ __device__ __forceinline__ int cell_coord(double v, double v0, double inv_h, int g) {
    const double c = floor((v - v0) * inv_h);  // clamped as a double: a far-away v never reaches the int conversion
    return (int)fmin(fmax(c, 0.0), (double)(g - 1));
}

__host__ __device__ __forceinline__ double sqdist3(const Point3& a, const Point3& b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
#ifdef __HIP_DEVICE_COMPILE__
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));  // never fused, coordinate order
#else
    return (dx * dx + dy * dy) + dz * dz;  // the build sets -ffp-contract=off
#endif
}

// lexicographic (d2, index) order
__host__ __device__ __forceinline__ bool closer3(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// The search of one query, pts[t].  pts: points sorted by cell; layer_of[cz]: rank of layer cz among the layers that
// hold points, -1 for an empty one; next_layer[cz]: the first layer >= cz that holds points (gz: none; gz + 1 entries), so
// that a walk along z steps over empty layers; cell_start[c] .. cell_start[c+1]: members of cell
// c = (layer_of[cz]*gy + cy)*gx + cx.
// Host-callable as well, so that the walk and its stop rule can be run on a CPU.
template <int KMAX>
__host__ __device__ __forceinline__ void knn_query3(const CellGrid3& g, const Point3* __restrict__ pts, const int32_t* __restrict__ layer_of,
                                                    const int32_t* __restrict__ next_layer, const int32_t* __restrict__ cell_start, int64_t t, int k, int32_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    using std::max;
    using std::min;
    const Point3 q = pts[t];
    const int cx = cell_coord(q.x, g.x0, g.inv_h, g.gx), cy = cell_coord(q.y, g.y0, g.inv_h, g.gy),
              cz = cell_coord(q.z, g.z0, g.inv_h, g.gz);
    double bd[KMAX];  // only ever indexed by unrolled loop counters: stays in registers
    int bi[KMAX];
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        bd[s] = __builtin_inf();
        bi[s] = 0x7fffffff;
    }
    const int rmax = max(max(max(cx, g.gx - 1 - cx), max(cy, g.gy - 1 - cy)), max(cz, g.gz - 1 - cz));
    const double inf = __builtin_inf();
    // offsets from the grid's corner, as the cell of a point is computed from them: face distances taken from these are
    // off by rounding of the extent, not of the absolute coordinates
    const double ux = q.x - g.x0, uy = q.y - g.y0, uz = q.z - g.z0;
    for (int r = 0; r <= rmax; ++r) {
        // surface of the cube [c-r, c+r]^3: the two z faces whole; of the planes between them the two y rows whole
        // and of the remaining rows the two end cells
        for (int zz = next_layer[max(cz - r, 0)]; zz <= min(cz + r, g.gz - 1); zz = next_layer[zz + 1]) {
            const int layer = layer_of[zz];
            const bool zface = (zz == cz - r) || (zz == cz + r);
            for (int yy = max(cy - r, 0); yy <= min(cy + r, g.gy - 1); ++yy) {
                const bool whole = zface || (yy == cy - r) || (yy == cy + r);
                const int row = (layer * g.gy + yy) * g.gx;
                for (int seg = 0; seg < (whole ? 1 : 2); ++seg) {
                    int lo, hi;
                    if (whole) {  // cells along x are adjacent in memory: the whole row is one range of points
                        lo = max(cx - r, 0);
                        hi = min(cx + r, g.gx - 1);
                    } else {
                        lo = hi = seg ? cx + r : cx - r;
                        if (lo < 0 || lo >= g.gx) continue;
                    }
                    const int pe = cell_start[row + hi + 1];
                    for (int p = cell_start[row + lo]; p < pe; ++p) {
                        const Point3 c = pts[p];
                        if (c.id == q.id) continue;  // by index: a coincident other point is a neighbour at distance 0
                        double d = sqdist3(q, c);
                        int di = c.id;
                        if (closer3(d, di, bd[KMAX - 1], bi[KMAX - 1])) {
#pragma unroll
                            for (int s = 0; s < KMAX; ++s) {  // sorted insertion: compare-exchange down the register list
                                const bool sw = closer3(d, di, bd[s], bi[s]);
                                const double td = sw ? bd[s] : d;
                                const int ti = sw ? bi[s] : di;
                                bd[s] = sw ? d : bd[s];
                                bi[s] = sw ? di : bi[s];
                                d = td;
                                di = ti;
                            }
                        }
                    }
                }
            }
        }
        // everything not yet visited lies outside the block of cells [c-r, c+r]^3; a face the grid does not reach
        // beyond has nothing behind it
        const double fxl = cx - r > 0 ? ux - (double)(cx - r) * g.h : inf;
        const double fxh = cx + r < g.gx - 1 ? (double)(cx + r + 1) * g.h - ux : inf;
        const double fyl = cy - r > 0 ? uy - (double)(cy - r) * g.h : inf;
        const double fyh = cy + r < g.gy - 1 ? (double)(cy + r + 1) * g.h - uy : inf;
        const double fzl = cz - r > 0 ? uz - (double)(cz - r) * g.h : inf;
        const double fzh = cz + r < g.gz - 1 ? (double)(cz + r + 1) * g.h - uz : inf;
        const double m = fmin(fmin(fmin(fxl, fxh), fmin(fyl, fyh)), fmin(fzl, fzh)) - 1e-9 * g.h;  // slack for cell rounding
        double kth = inf;  // k-th best so far (select chain: a dynamic register index would spill)
#pragma unroll
        for (int s = 0; s < KMAX; ++s) kth = (s == k - 1) ? bd[s] : kth;
        if (m > 0.0 && kth < m * m) break;  // strict: an unexplored point at exactly the k-th distance could win a tie
    }
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
        if (s < k) {
            out_idx[(size_t)q.id * k + s] = bi[s];
            out_d2[(size_t)q.id * k + s] = bd[s];
        }
}

template <int KMAX>
__global__ __launch_bounds__(128) void k_knn_grid3(CellGrid3 g, const Point3* __restrict__ pts, const int32_t* __restrict__ layer_of,
                                                   const int32_t* __restrict__ next_layer, const int32_t* __restrict__ cell_start, int64_t n, int k, int32_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;  // queries in cell order: neighbouring threads
    if (t < n) knn_query3<KMAX>(g, pts, layer_of, next_layer, cell_start, t, k, out_idx, out_d2);  // walk neighbouring cells (cache locality)
}

// distance from v to the interval [lo, hi], 0 inside
__host__ __device__ __forceinline__ double gap(double v, double lo, double hi) { return fmax(fmax(lo - v, v - hi), 0.0); }

// fixed radius: COUNT == true  -> counts[id] = #neighbours;  COUNT == false -> fill rows at offsets indptr[id].
// The query visits the cells its ball's bounding box touches, row by row along x (one range of points per row), and
// leaves out the rows that lie wholly outside the ball.
template <bool COUNT>
__host__ __device__ __forceinline__ void radius_query3(const CellGrid3& g, const Point3* __restrict__ pts, const int32_t* __restrict__ layer_of,
                                                       const int32_t* __restrict__ next_layer, const int32_t* __restrict__ cell_start, int64_t t, double radius, double r2, int64_t* __restrict__ counts,
                                                       const int64_t* __restrict__ indptr, int32_t* __restrict__ out_idx,
                                                       double* __restrict__ out_d2) {
    const Point3 q = pts[t];
    const double slack = 1e-9 * g.h;  // cell rounding
    const double reach = radius + slack;
    const int xlo = cell_coord(q.x - reach, g.x0, g.inv_h, g.gx), xhi = cell_coord(q.x + reach, g.x0, g.inv_h, g.gx);
    const int ylo = cell_coord(q.y - reach, g.y0, g.inv_h, g.gy), yhi = cell_coord(q.y + reach, g.y0, g.inv_h, g.gy);
    const int zlo = cell_coord(q.z - reach, g.z0, g.inv_h, g.gz), zhi = cell_coord(q.z + reach, g.z0, g.inv_h, g.gz);
    const double uy = q.y - g.y0, uz = q.z - g.z0;  // offsets from the grid's corner, as cells are computed from them
    int64_t cnt = 0;
    const int64_t base = COUNT ? 0 : indptr[q.id];
    for (int zz = next_layer[zlo]; zz <= zhi; zz = next_layer[zz + 1]) {
        const int layer = layer_of[zz];
        const double far_z = gap(uz, (double)zz * g.h - slack, (double)(zz + 1) * g.h + slack);
        for (int yy = ylo; yy <= yhi; ++yy) {
            const double far_y = gap(uy, (double)yy * g.h - slack, (double)(yy + 1) * g.h + slack);
            if (far_z * far_z + far_y * far_y > r2) continue;  // no point of this row is within the radius
            const int row = (layer * g.gy + yy) * g.gx;
            const int pe = cell_start[row + xhi + 1];
            for (int p = cell_start[row + xlo]; p < pe; ++p) {
                const Point3 c = pts[p];
                if (c.id == q.id) continue;
                const double d = sqdist3(q, c);
                if (d <= r2) {
                    if (!COUNT) {
                        out_idx[base + cnt] = c.id;
                        out_d2[base + cnt] = d;
                    }
                    ++cnt;
                }
            }
        }
    }
    if (COUNT) counts[q.id] = cnt;
}

template <bool COUNT>
__global__ __launch_bounds__(128) void k_radius_grid3(CellGrid3 g, const Point3* __restrict__ pts, const int32_t* __restrict__ layer_of,
                                                      const int32_t* __restrict__ next_layer, const int32_t* __restrict__ cell_start, int64_t n, double radius, double r2, int64_t* __restrict__ counts,
                                                      const int64_t* __restrict__ indptr, int32_t* __restrict__ out_idx,
                                                      double* __restrict__ out_d2) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < n) radius_query3<COUNT>(g, pts, layer_of, next_layer, cell_start, t, radius, r2, counts, indptr, out_idx, out_d2);
}

struct HostGrid3 {
    CellGrid3 g;
    std::vector<Point3> pts;
    std::vector<int32_t> layer_of, next_layer, cell_start;
};

namespace {

// cell side for ~target points per cell of a point set that fills its bounding box evenly.  Only the axes that are
// wider than a cell count: a flat axis (or one thinner than the cells the others ask for) holds a single layer of cells
// and is left out of the volume, so a plane gets square cells sized in 2-D, a line intervals, a single site one cell.
double side_from_extents(const double ext[3], int64_t n, double target, int& dims) {
    bool active[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
    for (;;) {
        dims = 0;
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

}  // namespace

// counting sort of the points into cubic cells of side >= min_h with ~target_per_cell points per OCCUPIED cell
int build_grid3(const double* xyz, int64_t n, double target_per_cell, double min_h, HostGrid3& out) {
    double lo[3] = {xyz[0], xyz[1], xyz[2]}, hi[3] = {xyz[0], xyz[1], xyz[2]};
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double v = xyz[3 * i + a];
            if (!std::isfinite(v)) {
                set_error("coordinate %lld is not finite", (long long)i);
                return SQGR_ERR_INVALID;
            }
            lo[a] = std::min(lo[a], v);
            hi[a] = std::max(hi[a], v);
        }
    const double ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double widest = std::max(ext[0], std::max(ext[1], ext[2]));
    SQGR_REQUIRE(std::isfinite(widest), "the coordinate range is not finite");
    // the number of stored cells is capped as a whole, at a small multiple of n (a long thin volume may have most of its
    // cells along one axis); cell indices stay below 2^30
    const double cap = (double)std::min<int64_t>(4 * n + 64, (int64_t)1 << 30);
    auto admissible = [&](double h) {
        h = std::max(h, min_h);
        if (!(h > 0.0) || !std::isfinite(h)) h = 1.0;
        return std::max(h, widest / 1048576.0);  // the kernels' rounding slack of 1e-9 cells holds up to 2^20 cells per axis
    };
    CellGrid3 g;
    int layers = 0;
    auto dims_at = [&](double h) {
        g.x0 = lo[0]; g.y0 = lo[1]; g.z0 = lo[2]; g.h = h; g.inv_h = 1.0 / h;
        g.gx = (int)std::floor(ext[0] / h) + 1;
        g.gy = (int)std::floor(ext[1] / h) + 1;
        g.gz = (int)std::floor(ext[2] / h) + 1;
    };
    auto fits = [&](double h) {  // the occupied layers of cells of side h, and whether their cells stay under the cap
        dims_at(h);
        out.layer_of.assign((size_t)g.gz, -1);
        for (int64_t i = 0; i < n; ++i) out.layer_of[cell_coord(xyz[3 * i + 2], g.z0, g.inv_h, g.gz)] = 0;
        layers = 0;
        for (int32_t& l : out.layer_of)
            if (l == 0) l = layers++;
        return (double)g.gx * (double)g.gy * (double)layers <= cap;
    };
    std::vector<int32_t> cell((size_t)n);
    size_t ncell = 0;
    auto assign = [&]() -> int64_t {  // after fits(): cell of every point, members per cell, number of occupied cells
        ncell = (size_t)g.gx * g.gy * layers;
        out.cell_start.assign(ncell + 1, 0);
        int64_t occupied = 0;
        for (int64_t i = 0; i < n; ++i) {
            const int cx = cell_coord(xyz[3 * i], g.x0, g.inv_h, g.gx), cy = cell_coord(xyz[3 * i + 1], g.y0, g.inv_h, g.gy),
                      cz = cell_coord(xyz[3 * i + 2], g.z0, g.inv_h, g.gz);
            cell[i] = (out.layer_of[cz] * g.gy + cy) * g.gx + cx;
            occupied += out.cell_start[cell[i] + 1]++ == 0;
        }
        return occupied;
    };
    int dims = 0;
    double h = admissible(side_from_extents(ext, n, target_per_cell, dims));
    while (!fits(h)) h *= 1.25;  // (the volume estimate stays under the cap; this is for the floors of `admissible`)
    double fill = (double)n / (double)assign();  // points per occupied cell
    // The bounding box says nothing about how the points fill it.  Sections stacked far apart leave most layers of cells
    // empty and crowd the occupied ones; the cells then shrink until the occupied ones hold about the target.  `fill`
    // grows like h^d with d the dimension the points fill locally: d is the number of wide axes at first and is
    // measured from the last two sides after that.  (Too few points per cell cannot happen: the volume estimate never
    // makes more than n / target cells.)
    double d = std::max(dims, 1);
    bool current = true;  // `g`, `layer_of` and `cell` belong to h
    for (int round = 0; round < 6 && fill > 2.0 * target_per_cell; ++round) {
        double h_new = admissible(h * std::pow(target_per_cell / fill, 1.0 / d));
        if (!(h_new < 0.95 * h)) break;  // at the floor
        current = false;
        if (!fits(h_new)) {  // over the cap: halfway, once
            h_new = std::sqrt(h * h_new);
            if (!(h_new < 0.95 * h) || !fits(h_new)) break;
        }
        const double fill_new = (double)n / (double)assign();
        current = true;
        if (!(fill_new < 0.9 * fill)) {  // coincident points: smaller cells do not separate them
            current = false;
            break;
        }
        d = std::min(3.0, std::max(1.0, std::log(fill / fill_new) / std::log(h / h_new)));
        h = h_new;
        fill = fill_new;
    }
    if (!current) {  // the last side tried was over the cap or no better: back to the one in use
        fits(h);
        assign();
    }
    out.g = g;
    out.next_layer.assign((size_t)g.gz + 1, g.gz);
    for (int z = g.gz - 1; z >= 0; --z) out.next_layer[z] = out.layer_of[z] >= 0 ? z : out.next_layer[z + 1];
    for (size_t c = 0; c < ncell; ++c) out.cell_start[c + 1] += out.cell_start[c];
    out.pts.resize((size_t)n);
    std::vector<int32_t> fillp(out.cell_start.begin(), out.cell_start.end() - 1);
    for (int64_t i = 0; i < n; ++i) {  // stable: members of a cell stay in index order
        Point3& p = out.pts[(size_t)fillp[cell[i]]++];
        p.x = xyz[3 * i];
        p.y = xyz[3 * i + 1];
        p.z = xyz[3 * i + 2];
        p.id = (int32_t)i;
        p.pad = 0;
    }
    return SQGR_OK;
}

struct DevGrid3 {
    DevBuf<Point3> pts;
    DevBuf<int32_t> layer_of, next_layer, cell_start;
    int upload(const HostGrid3& h, hipStream_t st) {
        SQGR_TRY(pts.alloc(h.pts.size()));
        SQGR_TRY(layer_of.alloc(h.layer_of.size()));
        SQGR_TRY(next_layer.alloc(h.next_layer.size()));
        SQGR_HIP(hipMemcpyAsync(layer_of.p, h.layer_of.data(), h.layer_of.size() * 4, hipMemcpyHostToDevice, st));
        SQGR_HIP(hipMemcpyAsync(next_layer.p, h.next_layer.data(), h.next_layer.size() * 4, hipMemcpyHostToDevice, st));
        SQGR_TRY(cell_start.alloc(h.cell_start.size()));
        SQGR_HIP(hipMemcpyAsync(pts.p, h.pts.data(), h.pts.size() * sizeof(Point3), hipMemcpyHostToDevice, st));
        SQGR_HIP(hipMemcpyAsync(cell_start.p, h.cell_start.data(), h.cell_start.size() * 4, hipMemcpyHostToDevice, st));
        return SQGR_OK;
    }
};

}  // namespace sqgr

using namespace sqgr;

extern "C" {

int sqgr_knn_self3(sqgr_ctx* ctx, const double* xyz, int64_t n, int32_t k, int32_t* out_idx, double* out_d2) {
    SQGR_REQUIRE(ctx && xyz && out_idx && out_d2, "null argument");
    SQGR_REQUIRE(n >= 1 && n < (int64_t)0x7fffffff, "n=%lld out of range", (long long)n);
    SQGR_REQUIRE(k >= 1 && k < n, "Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %lld, n_samples = %lld",
                 k + 1, (long long)n, (long long)n);  // sklearn queries k+1 and drops the sample itself
    if (k > 64) {
        set_error("n_neighbors=%d > 64 is not supported by the register-resident kNN search", k);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    HostGrid3 hg;
    SQGR_TRY(build_grid3(xyz, n, 2.0, 0.0, hg));
    DevGrid3 dg;
    hipStream_t st = ctx->stream;
    SQGR_TRY(dg.upload(hg, st));
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_d2;
    SQGR_TRY(d_idx.alloc((size_t)n * k));
    SQGR_TRY(d_d2.alloc((size_t)n * k));
    {
        LaunchTimer t(ctx, "neighbors3d_knn_grid");
        const unsigned grid = (unsigned)ceil_div(n, 128);
#define SQGR_KNN3(KM) k_knn_grid3<KM><<<grid, 128, 0, st>>>(hg.g, dg.pts.p, dg.layer_of.p, dg.next_layer.p, dg.cell_start.p, n, k, d_idx.p, d_d2.p)
        if (k <= 4) SQGR_KNN3(4); else if (k <= 8) SQGR_KNN3(8); else if (k <= 16) SQGR_KNN3(16); else if (k <= 32) SQGR_KNN3(32); else SQGR_KNN3(64);
#undef SQGR_KNN3
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_idx, d_idx.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_d2, d_d2.p, (size_t)n * k * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_radius_self3(sqgr_ctx* ctx, const double* xyz, int64_t n, double radius, int64_t* out_indptr, int32_t* out_idx,
                      double* out_d2, int64_t capacity) {
    SQGR_REQUIRE(ctx && xyz && out_indptr, "null argument");
    SQGR_REQUIRE(n >= 1 && n < (int64_t)0x7fffffff, "n=%lld out of range", (long long)n);
    SQGR_REQUIRE(radius >= 0.0 && std::isfinite(radius), "radius must be finite and >= 0");
    SQGR_HIP(hipSetDevice(ctx->device));
    HostGrid3 hg;
    // Cell floor radius / 4: the ball's bounding box then spans at most 10 cells per axis, which a query walks as at
    // most 10 x 10 rows along x — each row one contiguous range of points — of which the corner rows are skipped.  (The
    // 2-D floor radius / 8 would allow 18 x 18 rows of 18 cells.)  The floor only binds where the ball holds hundreds
    // of points, so the box's surplus over the ball, below 4x in candidates, is set against an output of that size.
    SQGR_TRY(build_grid3(xyz, n, 2.0, radius / 4.0, hg));
    DevGrid3 dg;
    hipStream_t st = ctx->stream;
    SQGR_TRY(dg.upload(hg, st));
    const double r2 = radius * radius;  // sklearn: EuclideanDistance._dist_to_rdist
    DevBuf<int64_t> d_cnt, d_ptr;
    SQGR_TRY(d_cnt.alloc((size_t)n));
    const unsigned grid = (unsigned)ceil_div(n, 128);
    {
        LaunchTimer t(ctx, "neighbors3d_radius_count");
        k_radius_grid3<true><<<grid, 128, 0, st>>>(hg.g, dg.pts.p, dg.layer_of.p, dg.next_layer.p, dg.cell_start.p, n, radius, r2, d_cnt.p, nullptr, nullptr, nullptr);
        SQGR_HIP(hipGetLastError());
    }
    std::vector<int64_t> cnt((size_t)n);
    SQGR_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    out_indptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) out_indptr[i + 1] = out_indptr[i] + cnt[i];
    if (!out_idx || !out_d2) return SQGR_OK;  // counting pass only
    const int64_t nnz = out_indptr[n];
    SQGR_REQUIRE(capacity >= nnz, "capacity %lld < %lld neighbours", (long long)capacity, (long long)nnz);
    if (nnz == 0) return SQGR_OK;
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_d2;
    SQGR_TRY(d_ptr.alloc((size_t)n + 1));
    SQGR_TRY(d_idx.alloc((size_t)nnz));
    SQGR_TRY(d_d2.alloc((size_t)nnz));
    SQGR_HIP(hipMemcpyAsync(d_ptr.p, out_indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(ctx, "neighbors3d_radius_fill");
        k_radius_grid3<false><<<grid, 128, 0, st>>>(hg.g, dg.pts.p, dg.layer_of.p, dg.next_layer.p, dg.cell_start.p, n, radius, r2, nullptr, d_ptr.p, d_idx.p, d_d2.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_idx, d_idx.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_d2, d_d2.p, (size_t)nnz * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

}  // extern "C"
