// libsqgr: mask_graph — `LineString([a, b]).within(polygon_mask)` for every edge of a spatial graph (gr/_mask.py).
//
// The numpy code of gr/_mask.py (`_classify`, `segments_within`) is the contract; the kernels restate it operation for operation: the
// same float64 subtractions, products, differences of products, divisions and comparisons in the same order, every one rounded on its
// own (no FMA: the library is built with -ffp-contract=off and the pragma below says it again), IEEE division.  Every decision is a
// comparison of such values, so the device returns the host's booleans bit for bit.
//
// The polygon goes up once per call as a flat table of ring edges (px, py, qx, qy) in ring order plus one flag word per edge: bit 0 the
// last edge of its ring, bit 1 the ring is a shell (the first ring of its polygon), bit 2 the last edge of its polygon.
//
// k_poly_classify one lane per point, a loop over ALL ring edges in order.  Crossing parity is kept per ring and closed at the ring's
//                 last edge: the shell's parity is `inside_shell`, a hole's parity is OR-ed into `in_hole` (two overlapping holes: a
//                 point in both is in a hole, the total parity would say otherwise).  The class — 0 outside, 1 on a boundary, 2 inside —
//                 is closed at the polygon's last edge and the maximum over polygons kept (`best` of `_classify`).  The edge index is
//                 the loop counter, the same in every lane: the four coordinates and the flag word arrive through scalar loads.
//                 Serves a, b, the midpoints 0.5 (a + b) and the piece midpoints of the cut segments: one function, one place to be wrong.
// k_seg_mid       0.5 * (a + b) behind a and b in the point list.
// k_seg_touch     one lane per segment over all ring edges: `hit` and `col` of segments_within, the number of cut parameters the
//                 segment would produce (0, 1, one per hit, two candidates per collinear ring edge) and its state: untouched ->
//                 mid == 2; touched with an end outside -> 0; otherwise "cut" (3), or overflow (2) when the parameters pass MASK_CAP.
// k_seg_cut       one wave per cut segment (compacted by a host prefix sum over the states).  Lanes take ring edges 64 at a time and
//                 recompute hit / col with the expressions of k_seg_touch; parameters are appended to an LDS list by ballot and
//                 popcount, sorted there (bitonic) and exact duplicates dropped (np.unique on finite doubles; -0.0 == 0.0 as there).
//                 The piece midpoints a + tm (b - a), tm = 0.5 (ts[i] + ts[i + 1]), go to a global list that k_poly_classify classifies.
//                 A segment owns (parameters - 1) slots of that list; slots that duplicates left over repeat the first midpoint,
//                 which changes neither all() nor any().
// k_seg_combine   one lane per cut segment: all(cls > 0) and any(cls == 2) over its slots.
//
// A zero-length segment (d2 = dx dx + dy dy is not > 0) is "collinear" with every ring edge whose line holds the point, but each such
// edge projects to tt = 0.0 (`... if d2 > 0 else 0.0`), a duplicate of the parameter 0: it contributes no parameter here.
//
// Every launch of the three kernels that walk the ring edges covers at most `pairs per launch` (point or segment, ring edge) pairs:
// brute force over a huge polygon is cut into many short kernels, never one long one.
#include "sqgr_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace sqgr {
namespace {

constexpr int MASK_T = 256;
constexpr int MASK_CAP = 256;                         // cut parameters of one segment held in LDS (0 and 1 included)
constexpr int64_t MASK_PAIRS = (int64_t)1 << 32;      // (point or segment, ring edge) pairs of one launch
constexpr int EDGE_RING_END = 1, EDGE_SHELL = 2, EDGE_POLY_END = 4;

struct RingEdge {
    double px, py, qx, qy;
};

__device__ __forceinline__ int classify_point(double x, double y, const RingEdge* __restrict__ edges, const int32_t* __restrict__ flags,
                                              int R) {
    int best = 0;
    bool on_edge = false, in_hole = false, inside_shell = false, odd = false;
    for (int j = 0; j < R; ++j) {  // j is uniform: scalar loads
        const RingEdge e = edges[j];
        const int f = flags[j];
        const double ex = e.qx - e.px, ey = e.qy - e.py, rx = x - e.px, ry = y - e.py;
        const double cr = ex * ry - ey * rx;
        if (cr == 0.0 && x >= fmin(e.px, e.qx) && x <= fmax(e.px, e.qx) && y >= fmin(e.py, e.qy) && y <= fmax(e.py, e.qy)) on_edge = true;
        if ((e.py > y) != (e.qy > y)) {  // half-open rule on y; ey != 0 here
            const double xi = e.px + (ry * ex) / ey;
            odd ^= (x < xi);
        }
        if (f & EDGE_RING_END) {
            if (f & EDGE_SHELL) inside_shell = odd;
            else in_hole |= odd;
            odd = false;
        }
        if (f & EDGE_POLY_END) {
            const int cls = on_edge ? 1 : ((inside_shell && !in_hole) ? 2 : 0);
            best = max(best, cls);
            on_edge = in_hole = inside_shell = false;
        }
    }
    return best;
}

__global__ __launch_bounds__(MASK_T) void k_poly_classify(const double2* __restrict__ pts, int64_t i0, int64_t count,
                                                          const RingEdge* __restrict__ edges, const int32_t* __restrict__ flags, int R,
                                                          uint8_t* __restrict__ out_cls) {
    const int64_t k = blockIdx.x * (int64_t)MASK_T + threadIdx.x;
    if (k >= count) return;
    const double2 p = pts[i0 + k];
    out_cls[i0 + k] = (uint8_t)classify_point(p.x, p.y, edges, flags, R);
}

// pts = [a (E) | b (E) | mid (E)]
__global__ __launch_bounds__(MASK_T) void k_seg_mid(double2* __restrict__ pts, int64_t E) {
    const int64_t s = blockIdx.x * (int64_t)MASK_T + threadIdx.x;
    if (s >= E) return;
    const double2 a = pts[s], b = pts[E + s];
    pts[2 * E + s] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y + b.y));
}

// hit / col of one (segment, ring edge) pair: lines 120-130 of gr/_mask.py.  c2 is the numerator of u and the collinearity test.
struct PairTest {
    bool hit, col;
    double t;
};
__device__ __forceinline__ PairTest pair_test(double ax, double ay, double dx, double dy, const RingEdge& e) {
    const double ex = e.qx - e.px, ey = e.qy - e.py, wx = e.px - ax, wy = e.py - ay;
    const double den = dx * ey - dy * ex;
    const double c2 = wx * dy - wy * dx;
    PairTest r{false, false, 0.0};
    if (den != 0.0) {
        const double c1 = wx * ey - wy * ex;
        const double t = c1 / den, u = c2 / den;
        r.hit = t >= 0.0 && t <= 1.0 && u >= 0.0 && u <= 1.0;
        r.t = t;
    } else {
        r.col = c2 == 0.0;
    }
    return r;
}

// state[s] = code | touched << 2; code: 0 / 1 the answer, 2 overflow, 3 cut (answer pending)
__global__ __launch_bounds__(MASK_T) void k_seg_touch(const double2* __restrict__ pts, const uint8_t* __restrict__ cls, int64_t E, int64_t s0,
                                                      int64_t count, const RingEdge* __restrict__ edges, int R, uint8_t* __restrict__ state,
                                                      int32_t* __restrict__ ncand) {
    const int64_t k = blockIdx.x * (int64_t)MASK_T + threadIdx.x;
    if (k >= count) return;
    const int64_t s = s0 + k;
    const double2 a = pts[s], b = pts[E + s];
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double d2 = dx * dx + dy * dy;
    int64_t nh = 0, nc = 0;
    for (int j = 0; j < R; ++j) {
        const RingEdge e = edges[j];
        const PairTest r = pair_test(a.x, a.y, dx, dy, e);
        nh += r.hit;
        nc += r.col;
    }
    const bool touched = nh > 0 || nc > 0;
    const int64_t cand = 2 + nh + (d2 > 0.0 ? 2 * nc : 0);
    int code;
    if (!touched) code = cls[2 * E + s] == 2;
    else if (cls[s] == 0 || cls[E + s] == 0) code = 0;
    else code = cand > MASK_CAP ? 2 : 3;
    state[s] = (uint8_t)(code | (touched ? 4 : 0));
    ncand[s] = (int32_t)(cand < INT32_MAX ? cand : INT32_MAX);
}

// one wave (= one block) per cut segment w: mids[slot_off[w] .. slot_off[w + 1])
__global__ __launch_bounds__(64) void k_seg_cut(const int32_t* __restrict__ cut_ids, const int64_t* __restrict__ slot_off, int64_t w0,
                                                const double2* __restrict__ pts, int64_t E, const RingEdge* __restrict__ edges, int R,
                                                double2* __restrict__ mids) {
    __shared__ double ts[MASK_CAP];
    __shared__ double us[MASK_CAP];
    const int lane = threadIdx.x;
    const int64_t w = w0 + blockIdx.x;
    const int64_t s = cut_ids[w];
    const double2 a = pts[s], b = pts[E + s];
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double d2 = dx * dx + dy * dy;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    if (lane == 0) {
        ts[0] = 0.0;
        ts[1] = 1.0;
    }
    int n = 2;  // uniform
    // the host sends a segment here only when its candidates fit; the bound checks keep a mistake there from writing past the list
    for (int j0 = 0; j0 < R; j0 += 64) {
        const int j = j0 + lane;
        PairTest r{false, false, 0.0};
        RingEdge e{0.0, 0.0, 0.0, 0.0};
        if (j < R) {
            e = edges[j];
            r = pair_test(a.x, a.y, dx, dy, e);
        }
        unsigned long long m = __ballot(r.hit);
        if (m) {
            const int pos = n + __popcll(m & below);
            if (r.hit && pos < MASK_CAP) ts[pos] = r.t;
            n = min(n + __popcll(m), MASK_CAP);
        }
        if (d2 > 0.0 && __ballot(r.col)) {
#pragma unroll
            for (int end = 0; end < 2; ++end) {
                const double ptx = end ? e.qx : e.px, pty = end ? e.qy : e.py;
                const double tt = ((ptx - a.x) * dx + (pty - a.y) * dy) / d2;
                const bool in = r.col && tt >= 0.0 && tt <= 1.0;
                m = __ballot(in);
                const int pos = n + __popcll(m & below);
                if (in && pos < MASK_CAP) ts[pos] = tt;
                n = min(n + __popcll(m), MASK_CAP);
            }
        }
    }
    int P = 2;  // sort the first P >= n entries, a power of two <= MASK_CAP
    while (P < n) P <<= 1;
    for (int i = n + lane; i < P; i += 64) ts[i] = INFINITY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int l = i ^ jj;
                if (l > i) {
                    const double x = ts[i], y = ts[l];
                    if ((x > y) == ((i & k) == 0)) {
                        ts[i] = y;
                        ts[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    int u = 0;  // distinct parameters, uniform
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < n && (i == 0 || ts[i] != ts[i - 1]);
        const unsigned long long m = __ballot(keep);
        if (keep) us[u + __popcll(m & below)] = ts[i];
        u += __popcll(m);
    }
    __syncthreads();
    const int pieces = u - 1;  // >= 1: 0 and 1 are always there
    const int64_t o = slot_off[w];
    const int slots = (int)(slot_off[w + 1] - o);
    for (int i = lane; i < slots; i += 64) {
        const int p = i < pieces ? i : 0;
        const double tm = 0.5 * (us[p] + us[p + 1]);
        mids[o + i] = make_double2(a.x + tm * dx, a.y + tm * dy);
    }
}

__global__ __launch_bounds__(MASK_T) void k_seg_combine(const int32_t* __restrict__ cut_ids, const int64_t* __restrict__ slot_off, int64_t n_cut,
                                                        const uint8_t* __restrict__ mid_cls, uint8_t* __restrict__ state) {
    const int64_t w = blockIdx.x * (int64_t)MASK_T + threadIdx.x;
    if (w >= n_cut) return;
    bool all_in = true, any_inside = false;
    for (int64_t i = slot_off[w]; i < slot_off[w + 1]; ++i) {
        const uint8_t c = mid_cls[i];
        all_in &= c > 0;
        any_inside |= c == 2;
    }
    state[cut_ids[w]] = (uint8_t)(4 | ((all_in && any_inside) ? 1 : 0));
}

int classify_range(sqgr_ctx* ctx, const double2* pts, int64_t n, const RingEdge* edges, const int32_t* flags, int R, uint8_t* cls, int64_t per,
                   int64_t* launches) {
    for (int64_t i0 = 0; i0 < n; i0 += per) {
        const int64_t count = std::min(per, n - i0);
        LaunchTimer t(ctx, "mask_classify");
        k_poly_classify<<<(unsigned)ceil_div(count, MASK_T), MASK_T, 0, ctx->stream>>>(pts, i0, count, edges, flags, R, cls);
        SQGR_HIP(hipGetLastError());
        ++*launches;
    }
    return SQGR_OK;
}

int segments_within(sqgr_ctx* ctx, const double* a_xy, const double* b_xy, int64_t E, const double* ring_xy, const int64_t* ring_offsets,
                    const int32_t* ring_polygon, int64_t n_rings, uint8_t* out_within, int64_t* out_stats, int64_t pairs_per_launch,
                    uint8_t* out_classes) {
    SQGR_REQUIRE(ctx && ring_xy && ring_offsets && ring_polygon && out_stats, "null argument");
    SQGR_REQUIRE(E >= 0 && E < ((int64_t)1 << 31), "E=%lld", (long long)E);
    SQGR_REQUIRE(E == 0 || (a_xy && b_xy && out_within), "null argument");
    SQGR_REQUIRE(n_rings >= 1 && n_rings < ((int64_t)1 << 31), "n_rings=%lld", (long long)n_rings);
    SQGR_REQUIRE(pairs_per_launch >= 0, "pairs_per_launch=%lld", (long long)pairs_per_launch);
    SQGR_REQUIRE(ring_offsets[0] == 0, "ring_offsets[0]=%lld", (long long)ring_offsets[0]);
    int64_t R64 = 0;
    for (int64_t r = 0; r < n_rings; ++r) {
        const int64_t o = ring_offsets[r], len = ring_offsets[r + 1] - o;
        SQGR_REQUIRE(len >= 4, "ring %lld has %lld stored points (a closed ring has at least 4)", (long long)r, (long long)len);
        SQGR_REQUIRE(r == 0 ? ring_polygon[0] == 0 : (ring_polygon[r] == ring_polygon[r - 1] || ring_polygon[r] == ring_polygon[r - 1] + 1),
                     "ring_polygon[%lld]=%d: polygon ids count up from 0, a polygon's rings are contiguous", (long long)r, ring_polygon[r]);
        R64 += len - 1;
        SQGR_REQUIRE(R64 < ((int64_t)1 << 31), "more than 2^31 ring edges");
        for (int64_t i = o; i < o + len; ++i)
            SQGR_REQUIRE(std::isfinite(ring_xy[2 * i]) && std::isfinite(ring_xy[2 * i + 1]), "ring %lld: a coordinate is not finite", (long long)r);
        SQGR_REQUIRE(ring_xy[2 * o] == ring_xy[2 * (o + len - 1)] && ring_xy[2 * o + 1] == ring_xy[2 * (o + len - 1) + 1],
                     "ring %lld is not closed (its first and last stored points differ)", (long long)r);
    }
    for (int64_t i = 0; i < 2 * E; ++i)
        SQGR_REQUIRE(std::isfinite(a_xy[i]) && std::isfinite(b_xy[i]), "segment %lld: a coordinate is not finite", (long long)(i / 2));
    for (int k = 0; k < 4; ++k) out_stats[k] = 0;
    if (E == 0) return SQGR_OK;
    const int R = (int)R64;
    const int64_t limit = pairs_per_launch ? pairs_per_launch : MASK_PAIRS;
    const int64_t per = std::max<int64_t>(1, limit / R);  // points, segments or waves of one launch

    std::vector<RingEdge> h_edges((size_t)R);
    std::vector<int32_t> h_flags((size_t)R);
    for (int64_t r = 0, j = 0; r < n_rings; ++r) {
        const bool shell = r == 0 || ring_polygon[r] != ring_polygon[r - 1];
        const bool last_of_poly = r + 1 == n_rings || ring_polygon[r + 1] != ring_polygon[r];
        for (int64_t i = ring_offsets[r]; i + 1 < ring_offsets[r + 1]; ++i, ++j) {
            h_edges[j] = RingEdge{ring_xy[2 * i], ring_xy[2 * i + 1], ring_xy[2 * i + 2], ring_xy[2 * i + 3]};
            const bool ring_end = i + 2 == ring_offsets[r + 1];
            h_flags[j] = (ring_end ? EDGE_RING_END : 0) | (shell ? EDGE_SHELL : 0) | (ring_end && last_of_poly ? EDGE_POLY_END : 0);
        }
    }

    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<RingEdge> edges;
    DevBuf<int32_t> flags, ncand;
    DevBuf<double2> pts;
    DevBuf<uint8_t> cls, state;
    SQGR_TRY(edges.alloc((size_t)R));
    SQGR_TRY(flags.alloc((size_t)R));
    SQGR_TRY(pts.alloc_pooled((size_t)E * 3));
    SQGR_TRY(cls.alloc((size_t)E * 3));
    SQGR_TRY(state.alloc((size_t)E));
    SQGR_TRY(ncand.alloc((size_t)E));
    SQGR_HIP(hipMemcpyAsync(edges.p, h_edges.data(), (size_t)R * sizeof(RingEdge), hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(flags.p, h_flags.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(pts.p, a_xy, (size_t)E * 16, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(pts.p + E, b_xy, (size_t)E * 16, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(ctx, "mask_mid");
        k_seg_mid<<<(unsigned)ceil_div(E, MASK_T), MASK_T, 0, st>>>(pts.p, E);
        SQGR_HIP(hipGetLastError());
    }
    int64_t launches = 0;
    SQGR_TRY(classify_range(ctx, pts.p, 3 * E, edges.p, flags.p, R, cls.p, per, &launches));
    for (int64_t s0 = 0; s0 < E; s0 += per) {
        const int64_t count = std::min(per, E - s0);
        LaunchTimer t(ctx, "mask_touch");
        k_seg_touch<<<(unsigned)ceil_div(count, MASK_T), MASK_T, 0, st>>>(pts.p, cls.p, E, s0, count, edges.p, R, state.p, ncand.p);
        SQGR_HIP(hipGetLastError());
        ++launches;
    }
    std::vector<uint8_t> h_state((size_t)E);
    std::vector<int32_t> h_ncand((size_t)E);
    SQGR_HIP(hipMemcpyAsync(h_state.data(), state.p, (size_t)E, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(h_ncand.data(), ncand.p, (size_t)E * 4, hipMemcpyDeviceToHost, st));
    if (out_classes) SQGR_HIP(hipMemcpyAsync(out_classes, cls.p, (size_t)E * 3, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));

    // the cut segments, compacted in segment order; segment w of them owns (parameters - 1) slots of the midpoint list
    std::vector<int32_t> cut_ids;
    std::vector<int64_t> slot_off(1, 0);
    int64_t touched = 0, overflow = 0;
    for (int64_t s = 0; s < E; ++s) {
        const int code = h_state[s] & 3;
        touched += (h_state[s] >> 2) & 1;
        overflow += code == 2;
        if (code == 3) {
            SQGR_REQUIRE(h_ncand[s] >= 2 && h_ncand[s] <= MASK_CAP, "internal: segment %lld has %d cut parameters", (long long)s, h_ncand[s]);
            cut_ids.push_back((int32_t)s);
            slot_off.push_back(slot_off.back() + h_ncand[s] - 1);
        }
    }
    const int64_t n_cut = (int64_t)cut_ids.size(), n_slots = slot_off.back();
    if (n_cut) {
        DevBuf<int32_t> d_cut;
        DevBuf<int64_t> d_off;
        DevBuf<double2> mids;
        DevBuf<uint8_t> mid_cls;
        SQGR_TRY(d_cut.alloc((size_t)n_cut));
        SQGR_TRY(d_off.alloc((size_t)n_cut + 1));
        SQGR_TRY(mids.alloc((size_t)n_slots));
        SQGR_TRY(mid_cls.alloc((size_t)n_slots));
        SQGR_HIP(hipMemcpyAsync(d_cut.p, cut_ids.data(), (size_t)n_cut * 4, hipMemcpyHostToDevice, st));
        SQGR_HIP(hipMemcpyAsync(d_off.p, slot_off.data(), ((size_t)n_cut + 1) * 8, hipMemcpyHostToDevice, st));
        const int64_t per_cut = std::min<int64_t>(per, (int64_t)1 << 30);  // one block per segment
        for (int64_t w0 = 0; w0 < n_cut; w0 += per_cut) {
            const int64_t count = std::min(per_cut, n_cut - w0);
            LaunchTimer t(ctx, "mask_cut");
            k_seg_cut<<<(unsigned)count, 64, 0, st>>>(d_cut.p, d_off.p, w0, pts.p, E, edges.p, R, mids.p);
            SQGR_HIP(hipGetLastError());
            ++launches;
        }
        SQGR_TRY(classify_range(ctx, mids.p, n_slots, edges.p, flags.p, R, mid_cls.p, per, &launches));
        {
            LaunchTimer t(ctx, "mask_combine");
            k_seg_combine<<<(unsigned)ceil_div(n_cut, MASK_T), MASK_T, 0, st>>>(d_cut.p, d_off.p, n_cut, mid_cls.p, state.p);
            SQGR_HIP(hipGetLastError());
        }
        SQGR_HIP(hipMemcpyAsync(h_state.data(), state.p, (size_t)E, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
    }
    for (int64_t s = 0; s < E; ++s) out_within[s] = h_state[s] & 3;
    out_stats[0] = touched;
    out_stats[1] = n_cut + overflow;
    out_stats[2] = overflow;
    out_stats[3] = launches;
    return SQGR_OK;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_mask_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = MASK_CAP;
    out_info[1] = MASK_PAIRS;
    return SQGR_OK;
}

int sqgr_segments_within(sqgr_ctx* ctx, const double* a_xy, const double* b_xy, int64_t E, const double* ring_xy, const int64_t* ring_offsets,
                         const int32_t* ring_polygon, int64_t n_rings, uint8_t* out_within, int64_t* out_stats) {
    return segments_within(ctx, a_xy, b_xy, E, ring_xy, ring_offsets, ring_polygon, n_rings, out_within, out_stats, 0, nullptr);
}

int sqgr_segments_within_hook(sqgr_ctx* ctx, const double* a_xy, const double* b_xy, int64_t E, const double* ring_xy,
                              const int64_t* ring_offsets, const int32_t* ring_polygon, int64_t n_rings, uint8_t* out_within, int64_t* out_stats,
                              int64_t pairs_per_launch, uint8_t* out_classes) {
    return segments_within(ctx, a_xy, b_xy, E, ring_xy, ring_offsets, ring_polygon, n_rings, out_within, out_stats, pairs_per_launch, out_classes);
}
