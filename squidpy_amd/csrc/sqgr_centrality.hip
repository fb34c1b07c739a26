// libsqgr: centrality_scores — the integer side of group closeness, group degree and local clustering (gr/_nhood.py).
//
// Reference semantics (squidpy, src/squidpy/gr/_nhood.py):
//   :432-454  _build_graph: A = csr(conn); A + A^T; diagonal and stored zeros removed; rows sorted — the HOST does this (scipy) and
//             uploads the result, so both entry points see an undirected, unweighted graph without self loops, rows sorted
//   :457-491  _local_clustering: two_tri[v] = sum over u in N(v) of |N(v) n N(u)| (sorted-list merge), cc = two_tri / (k (k - 1))
//   :309-312  rx.group_closeness_centrality / rx.group_degree_centrality per cluster: one multi-source BFS per cluster
//
// Everything computed here is an integer, so no result depends on launch geometry or atomic arrival order; the host forms the floats.
//
// k_tri       one thread per stored edge (v, u) with v < u: |N(v) n N(u)| goes to two_tri[v] AND two_tri[u] (the mirror entry (u, v)
//             would count the same set).  Work per edge, not per row: a hub of thousands of neighbours is thousands of threads.  Lists
//             of very different length are intersected by binary search of the short one's entries in the long one.
// k_bfs_level one level of up to 64 multi-source BFS at once: bit g of a node's 64-bit word <=> group g has reached the node.  A pull
//             sweep from mask_in to mask_out (an in-place sweep would carry a bit several hops in one level):
//                 new = (OR of the neighbours' words) & ~own;   adjacent[g] = #new bits of g at level 1;
//                 dist_sum[g] += level * #new bits of g;        reached[g] += #new bits of g
//             counted per group in LDS and flushed once per block.  Rows longer than BFS_LONG_ROW are gathered by the whole wave.
//             The level loop runs on the host in batches of plain launches; after a batch one word tells whether it added a bit.
#include "sqgr_common.h"

#include <algorithm>
#include <vector>

namespace sqgr {
namespace {

constexpr int CENT_T = 256;
constexpr int BFS_LONG_ROW = 128;  // stored entries from which a row is gathered by its wave, 64 entries per step
constexpr int TRI_SKEW = 16;       // length ratio from which the short list is looked up in the long one instead of merged
constexpr int BFS_BATCH0 = 8;      // levels of the first batch of a pass; doubles up to BFS_BATCH_MAX while bits keep arriving
constexpr int BFS_BATCH_MAX = 128;

// flags[0]: an entry without its mirror; flags[1]: a row that is not strictly increasing; flags[2]: a self loop
__global__ __launch_bounds__(CENT_T) void k_cent_check(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                       const int32_t* __restrict__ erow, int64_t nnz, int* __restrict__ flags) {
    const int64_t e = blockIdx.x * (int64_t)CENT_T + threadIdx.x;
    if (e >= nnz) return;
    const int32_t r = erow[e], c = indices[e];
    if (e > indptr[r] && indices[e - 1] >= c) flags[1] = 1;
    if (r == c) {
        flags[2] = 1;
        return;
    }
    int64_t lo = indptr[c], hi = indptr[c + 1];  // first position in row c with index >= r
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indices[mid] < r) lo = mid + 1; else hi = mid;
    }
    if (lo >= end || indices[lo] != r) flags[0] = 1;
}

__global__ __launch_bounds__(CENT_T) void k_tri(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                const int32_t* __restrict__ erow, int64_t nnz, unsigned long long* __restrict__ two_tri) {
    const int64_t e = blockIdx.x * (int64_t)CENT_T + threadIdx.x;
    if (e >= nnz) return;
    const int32_t v = erow[e], u = indices[e];
    if (v >= u) return;  // the mirror entry's thread serves the pair
    const int64_t v0 = indptr[v], v1 = indptr[v + 1], u0 = indptr[u], u1 = indptr[u + 1];
    const bool v_short = v1 - v0 <= u1 - u0;
    const int32_t* a = indices + (v_short ? v0 : u0);  // the shorter list
    const int32_t* b = indices + (v_short ? u0 : v0);
    const int64_t la = v_short ? v1 - v0 : u1 - u0, lb = v_short ? u1 - u0 : v1 - v0;
    uint32_t c = 0;  // <= la < 2^31
    if (lb > (int64_t)TRI_SKEW * la) {
        int64_t from = 0;  // both lists ascend: the search window only shrinks
        for (int64_t i = 0; i < la && from < lb; ++i) {
            const int32_t x = a[i];
            int64_t lo = from, hi = lb;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (b[mid] < x) lo = mid + 1; else hi = mid;
            }
            if (lo < lb && b[lo] == x) {
                ++c;
                ++lo;
            }
            from = lo;
        }
    } else {
        int64_t i = 0, j = 0;
        while (i < la && j < lb) {
            const int32_t x = a[i], y = b[j];
            c += x == y;
            i += x <= y;
            j += y <= x;
        }
    }
    if (c) {
        atomicAdd(&two_tri[v], (unsigned long long)c);
        atomicAdd(&two_tri[u], (unsigned long long)c);
    }
}

// word of node i for the pass over groups [base, base + 64)
__global__ __launch_bounds__(CENT_T) void k_bfs_init(const int32_t* __restrict__ labels, int64_t n, int32_t base, uint64_t* __restrict__ mask) {
    const int64_t i = blockIdx.x * (int64_t)CENT_T + threadIdx.x;
    if (i >= n) return;
    const int32_t g = labels[i] - base;
    mask[i] = (g >= 0 && g < 64) ? (uint64_t)1 << g : 0;
}

// One level.  adjacent / dist_sum / reached point at the pass's first group; state[0] += bits added (zeroed by the host per batch),
// state[1] = max(state[1], level) when this level added a bit.  `full` has the pass's groups set: a node that holds it gathers nothing.
__global__ __launch_bounds__(CENT_T) void k_bfs_level(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const uint64_t* __restrict__ mask_in, uint64_t* __restrict__ mask_out, int64_t n,
                                                      uint64_t full, uint32_t level, unsigned long long* __restrict__ adjacent,
                                                      unsigned long long* __restrict__ dist_sum, unsigned long long* __restrict__ reached,
                                                      unsigned long long* __restrict__ state) {
    __shared__ uint32_t cnt[64];  // new bits per group in this block (a block sees fewer than 2^31 nodes)
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t base = blockIdx.x * (int64_t)CENT_T; base < n; base += (int64_t)gridDim.x * CENT_T) {  // uniform per block
        const int64_t v = base + threadIdx.x;
        uint64_t own = full, acc = 0;
        int64_t a = 0, b = 0;
        if (v < n) {
            own = mask_in[v];
            a = indptr[v];
            b = indptr[v + 1];
        }
        const bool want = v < n && own != full;
        const bool is_long = want && b - a > BFS_LONG_ROW;
        if (want && !is_long)
            for (int64_t e = a; e < b; ++e) acc |= mask_in[indices[e]];
        unsigned long long longs = __ballot(is_long);
        while (longs) {  // every lane of the wave gathers 1/64 of the row of lane `src`
            const int src = __ffsll(longs) - 1;
            longs &= longs - 1;
            const int64_t ra = __shfl((long long)a, src, 64), rb = __shfl((long long)b, src, 64);
            unsigned long long part = 0;
            for (int64_t e = ra + lane; e < rb; e += 64) part |= mask_in[indices[e]];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) part |= __shfl_xor(part, o, 64);
            if (lane == src) acc = part;
        }
        if (v < n) {
            uint64_t nw = acc & ~own;  // words hold bits of `full` only
            mask_out[v] = own | nw;
            while (nw) {
                atomicAdd(&cnt[__ffsll((unsigned long long)nw) - 1], 1u);
                nw &= nw - 1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // wave 0: one flush per block
        const uint32_t c = cnt[threadIdx.x];
        if (c) {
            atomicAdd(&reached[threadIdx.x], (unsigned long long)c);
            atomicAdd(&dist_sum[threadIdx.x], (unsigned long long)c * level);
            if (level == 1) atomicAdd(&adjacent[threadIdx.x], (unsigned long long)c);
        }
        unsigned long long tot = c;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) tot += __shfl_xor(tot, o, 64);
        if (threadIdx.x == 0 && tot) {
            atomicAdd(&state[0], tot);
            atomicMax(&state[1], (unsigned long long)level);
        }
    }
}

// both entry points need an undirected simple graph in canonical CSR form (what _build_graph hands its kernels).  sqgr_graph::ensure_half
// asks the same of a graph but also builds the half edge list of the permutation test, which nothing here reads.
int require_simple_graph(sqgr_ctx* ctx, const sqgr_graph* g, const char* who) {
    if (g->nnz == 0) return SQGR_OK;
    SQGR_REQUIRE(g->nnz < ((int64_t)1 << 39), "%s: nnz=%lld", who, (long long)g->nnz);  // blocks of the per-edge grids
    hipStream_t st = ctx->stream;
    DevBuf<int> flags;
    SQGR_TRY(flags.alloc(3));
    SQGR_HIP(hipMemsetAsync(flags.p, 0, 3 * sizeof(int), st));
    {
        LaunchTimer t(ctx, "centrality_check");
        k_cent_check<<<(unsigned)ceil_div(g->nnz, CENT_T), CENT_T, 0, st>>>(g->indptr.p, g->indices.p, g->erow.p, g->nnz, flags.p);
        SQGR_HIP(hipGetLastError());
    }
    int h[3] = {1, 1, 1};
    SQGR_HIP(hipMemcpyAsync(h, flags.p, sizeof(h), hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    SQGR_REQUIRE(!h[1], "%s: a row of the graph is not sorted or repeats an entry (sort_indices / sum_duplicates)", who);
    SQGR_REQUIRE(!h[2], "%s: the graph has a self loop (setdiag(0) and eliminate_zeros)", who);
    SQGR_REQUIRE(!h[0], "%s: the graph is not structurally symmetric (A + A.T)", who);
    return SQGR_OK;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_graph_triangles(sqgr_ctx* ctx, const sqgr_graph* g, int64_t* out_two_tri) {
    SQGR_REQUIRE(ctx && g && out_two_tri, "null argument");
    SQGR_REQUIRE(g->ctx == ctx, "graph belongs to a different context");
    SQGR_HIP(hipSetDevice(ctx->device));
    SQGR_TRY(require_simple_graph(ctx, g, "sqgr_graph_triangles"));
    hipStream_t st = ctx->stream;
    DevBuf<unsigned long long> tt;
    SQGR_TRY(tt.alloc((size_t)g->n));
    SQGR_HIP(hipMemsetAsync(tt.p, 0, (size_t)g->n * 8, st));
    if (g->nnz) {
        LaunchTimer t(ctx, "centrality_tri");
        k_tri<<<(unsigned)ceil_div(g->nnz, CENT_T), CENT_T, 0, st>>>(g->indptr.p, g->indices.p, g->erow.p, g->nnz, tt.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_two_tri, tt.p, (size_t)g->n * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_group_bfs(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int64_t* out_adjacent, int64_t* out_dist_sum,
                   int64_t* out_reached, int64_t* out_levels) {
    return sqgr_group_bfs_hook(ctx, g, labels, K, out_adjacent, out_dist_sum, out_reached, out_levels, 0);
}

int sqgr_group_bfs_hook(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int64_t* out_adjacent, int64_t* out_dist_sum,
                        int64_t* out_reached, int64_t* out_levels, int32_t grid_blocks) {
    SQGR_REQUIRE(ctx && g && labels && out_adjacent && out_dist_sum && out_reached && out_levels, "null argument");
    SQGR_REQUIRE(grid_blocks >= 0, "grid_blocks=%d", grid_blocks);
    SQGR_REQUIRE(g->ctx == ctx, "graph belongs to a different context");
    SQGR_REQUIRE(K >= 1, "K=%d", K);
    const int64_t n = g->n;
    for (int64_t i = 0; i < n; ++i)
        SQGR_REQUIRE(labels[i] >= -1 && labels[i] < K, "labels[%lld]=%d outside [-1,%d)", (long long)i, labels[i], K);
    SQGR_HIP(hipSetDevice(ctx->device));
    SQGR_TRY(require_simple_graph(ctx, g, "sqgr_group_bfs"));
    hipStream_t st = ctx->stream;
    DevBuf<int32_t> d_lab;
    DevBuf<uint64_t> mask;              // [2][n]
    DevBuf<unsigned long long> counts;  // adjacent[K] | dist_sum[K] | reached[K] | state[2]
    SQGR_TRY(d_lab.alloc((size_t)n));
    SQGR_TRY(mask.alloc_pooled((size_t)n * 2));
    SQGR_TRY(counts.alloc((size_t)K * 3 + 2));
    SQGR_HIP(hipMemcpyAsync(d_lab.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemsetAsync(counts.p, 0, ((size_t)K * 3 + 2) * 8, st));
    unsigned long long* state = counts.p + (size_t)K * 3;
    const unsigned node_blocks = (unsigned)ceil_div(n, CENT_T);
    const unsigned grid = std::min<unsigned>(node_blocks, grid_blocks ? (unsigned)grid_blocks : 8u * (unsigned)std::max(ctx->cu_count, 1));
    for (int32_t base = 0; base < K; base += 64) {
        const int kp = std::min(64, K - base);
        const uint64_t full = kp == 64 ? ~(uint64_t)0 : (((uint64_t)1 << kp) - 1);
        {
            LaunchTimer t(ctx, "centrality_bfs_init");
            k_bfs_init<<<node_blocks, CENT_T, 0, st>>>(d_lab.p, n, base, mask.p);
            SQGR_HIP(hipGetLastError());
        }
        int64_t level = 0;  // levels done: the words of level `level` are in half (level & 1) of `mask`
        int batch = BFS_BATCH0;
        while (level < n - 1) {  // no shortest path has more than n - 1 edges
            SQGR_HIP(hipMemsetAsync(state, 0, 8, st));
            const int64_t stop = std::min<int64_t>(n - 1, level + batch);
            for (; level < stop; ++level) {
                const uint64_t* in = mask.p + (size_t)(level & 1) * n;
                uint64_t* out = mask.p + (size_t)((level + 1) & 1) * n;
                LaunchTimer t(ctx, "centrality_bfs_level");
                k_bfs_level<<<grid, CENT_T, 0, st>>>(g->indptr.p, g->indices.p, in, out, n, full, (uint32_t)(level + 1), counts.p + base,
                                                     counts.p + K + base, counts.p + 2 * (size_t)K + base, state);
                SQGR_HIP(hipGetLastError());
            }
            unsigned long long added = 0;
            SQGR_HIP(hipMemcpyAsync(&added, state, 8, hipMemcpyDeviceToHost, st));
            SQGR_HIP(hipStreamSynchronize(st));
            if (!added) break;  // a level that adds nothing is the fixed point; the levels behind it added 0
            batch = std::min(2 * batch, BFS_BATCH_MAX);
        }
    }
    std::vector<unsigned long long> h((size_t)K * 3 + 2);
    SQGR_HIP(hipMemcpyAsync(h.data(), counts.p, h.size() * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    for (int32_t k = 0; k < K; ++k) {
        out_adjacent[k] = (int64_t)h[k];
        out_dist_sum[k] = (int64_t)h[(size_t)K + k];
        out_reached[k] = (int64_t)h[2 * (size_t)K + k];
    }
    *out_levels = (int64_t)h[3 * (size_t)K + 1];
    return SQGR_OK;
}
