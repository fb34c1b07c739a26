// libsqgr: exact k-nearest-neighbour search in feature space (1 to 256 dimensions) and UMAP's fuzzy kNN weights — the two parts of
// `sc.pp.neighbors(adata_embedding, n_neighbors, use_rep="X")` that grow with n, the call the reference's `neighborhood` and `utag`
// niche flavours make in front of `sc.tl.leiden` (gr/_niche.py:1417).  The symmetrisation stays on the host (gr/_niche_graph.py).
//
//   d2(i, c) = sum_j (x[i][j] - x[c][j])^2      j ascending; every difference, product and sum rounded on its own
//
// (__dsub_rn / __dmul_rn / __dadd_rn: no FMA whatever the compiler's contraction setting) — sklearn's KD-tree `rdist`, bit for bit.
// The k nearest OTHER rows of every row, ascending by (d2, index): a strict total order, so the answer is unique and independent of
// the launch geometry.  The cell lists of sqgr_neighbors.hip prune nothing at 30 to 64 dimensions, so this is all pairs:
//
// k_knn_nd   a block of 256 threads owns KN_Q = 64 query rows and streams every candidate row past them in tiles of KN_C = 64, in
//            ascending index order.  Strips of KN_JW = 32 columns of both tiles are staged transposed in LDS ([column][row], pitch
//            65: the staging stores are conflict-free), the next strip already on its way in registers; a thread owns a 4 x 4
//            register tile of d2 — per column 8 LDS values for 16 differences, 16 products and 16 sums — and carries it through the
//            strips of a candidate tile, j ascending.  Every query keeps its k best (d2, index) pairs sorted in LDS ([rank][query]);
//            its last entry is the threshold.  After the last strip a thread compares its 16 values with the thresholds of its four
//            queries; the few that pass are written to a 64 x 64 tile of d2 (it takes the strips' place) and flagged in a 64-bit
//            mask per query (an LDS integer OR), and lane q of the block's first wave inserts query q's flagged candidates in
//            ascending index order, comparing (d2, index) lexicographically.  Past the first tiles a candidate at index i passes with
//            probability about k / i, so the insert may be slow.  LDS: 33 792 + 768 k bytes (44.5 KB at k = 14: three blocks per CU).
// k_fuzzy_knn  UMAP's smooth_knn_dist and compute_membership_strengths for local_connectivity = 1: one lane per row.
#include "sqgr_common.h"

#include <cmath>

namespace sqgr {
namespace {

constexpr int KN_T = 256;
constexpr int KN_Q = 64;      // query rows of a block
constexpr int KN_C = 64;      // candidate rows of a tile
constexpr int KN_JW = 32;     // columns of a strip
constexpr int KN_PITCH = 65;  // doubles between two columns of a staged strip, and between two queries of the d2 tile
constexpr int KN_PER = KN_Q * KN_JW / KN_T;  // values of each strip a thread stages
constexpr int KN_MAX_D = 256;
constexpr int KN_MAX_K = 64;
constexpr int KN_STRIPS = 2 * KN_JW * KN_PITCH;  // doubles of the two strips = of the d2 tile
static_assert(KN_Q * KN_PITCH <= KN_STRIPS, "the d2 tile takes the strips' place");
static_assert(KN_Q == 64 && KN_C == 64, "one lane of a wave per query, one mask bit per candidate");

size_t knn_lds_bytes(int k) { return (size_t)(KN_STRIPS + KN_Q) * 8 + (size_t)k * KN_Q * 12; }

// lexicographic (d2, index) order
__device__ __forceinline__ bool before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__global__ __launch_bounds__(KN_T) void k_knn_widen(const float* __restrict__ in, int64_t count, double* __restrict__ out) {
    const int64_t t = blockIdx.x * (int64_t)KN_T + threadIdx.x;
    if (t < count) out[t] = (double)in[t];
}

__global__ __launch_bounds__(KN_T) void k_knn_nd(const double* __restrict__ X, int64_t n, int D, int k, int32_t* __restrict__ out_idx,
                                                 double* __restrict__ out_d2) {
    extern __shared__ double smem[];
    double* Qs = smem;                                    // [KN_JW][KN_PITCH]
    double* Cs = smem + KN_JW * KN_PITCH;                 // [KN_JW][KN_PITCH]
    double* tile = smem;                                  // [KN_Q][KN_PITCH]: in the strips' place between two candidate tiles
    unsigned* mask = (unsigned*)(smem + KN_STRIPS);       // [KN_Q][2]
    double* ld2 = smem + KN_STRIPS + KN_Q;                // [k][KN_Q]
    int* lidx = (int*)(ld2 + (size_t)k * KN_Q);           // [k][KN_Q]
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t row0 = blockIdx.x * (int64_t)KN_Q;
    const int nstrips = (D + KN_JW - 1) / KN_JW;
    const int64_t ntiles = (n + KN_C - 1) / KN_C;
    for (int e = t; e < k * KN_Q; e += KN_T) {
        ld2[e] = INFINITY;
        lidx[e] = INT32_MAX;
    }
    if (t < 2 * KN_Q) mask[t] = 0u;
    double nq[KN_PER], nc[KN_PER];
    auto fetch = [&](int64_t ct, int s) {
#pragma unroll
        for (int u = 0; u < KN_PER; ++u) {
            const int e = t + KN_T * u, jj = e & (KN_JW - 1), r = e / KN_JW;
            const int col = s * KN_JW + jj;
            const int64_t qrow = row0 + r, crow = ct * KN_C + r;
            nq[u] = (col < D && qrow < n) ? X[(size_t)qrow * (size_t)D + col] : 0.0;
            nc[u] = (col < D && crow < n) ? X[(size_t)crow * (size_t)D + col] : 0.0;
        }
    };
    fetch(0, 0);
    double acc[16];
    for (int64_t ct = 0; ct < ntiles; ++ct) {
        for (int s = 0; s < nstrips; ++s) {
            __syncthreads();  // the previous strip's readers, or the previous tile's inserts, are done
#pragma unroll
            for (int u = 0; u < KN_PER; ++u) {
                const int e = t + KN_T * u, jj = e & (KN_JW - 1), r = e / KN_JW;
                Qs[jj * KN_PITCH + r] = nq[u];
                Cs[jj * KN_PITCH + r] = nc[u];
            }
            __syncthreads();
            if (s + 1 < nstrips) fetch(ct, s + 1);  // the next strip travels while this one is used
            else if (ct + 1 < ntiles) fetch(ct + 1, 0);
            if (s == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.0;
            }
            const int jw = min(KN_JW, D - s * KN_JW);
#pragma unroll 2
            for (int jj = 0; jj < jw; ++jj) {
                double a[4], b[4], prod[16];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    a[p] = Qs[jj * KN_PITCH + 4 * ty + p];
                    b[p] = Cs[jj * KN_PITCH + 4 * tx + p];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double diff = __dsub_rn(a[p], b[q]);
                        prod[p * 4 + q] = __dmul_rn(diff, diff);
                    }
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = __dadd_rn(acc[e], prod[e]);
            }
        }
        __syncthreads();  // the last strip's readers are done: the d2 tile may take its place
        const int64_t c0 = ct * KN_C;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int q = 4 * ty + p;
            const int64_t qrow = row0 + q;
            const double thr_d = ld2[(k - 1) * KN_Q + q];
            const int thr_i = lidx[(k - 1) * KN_Q + q];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int cl = 4 * tx + c;
                const int64_t cand = c0 + cl;
                if (qrow < n && cand < n && cand != qrow && before(acc[p * 4 + c], (int)cand, thr_d, thr_i)) {
                    tile[q * KN_PITCH + cl] = acc[p * 4 + c];
                    atomicOr(&mask[2 * q + (cl >> 5)], 1u << (cl & 31));
                }
            }
        }
        __syncthreads();
        if (t < KN_Q) {  // lane q inserts query q's flagged candidates, ascending
            const int q = t;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                unsigned m = mask[2 * q + half];
                if (m) mask[2 * q + half] = 0u;
                while (m) {
                    const int cl = half * 32 + __ffs((int)m) - 1;
                    m &= m - 1;
                    const double d = tile[q * KN_PITCH + cl];
                    const int ci = (int)(c0 + cl);
                    if (!before(d, ci, ld2[(k - 1) * KN_Q + q], lidx[(k - 1) * KN_Q + q])) continue;
                    int p = k - 1;
                    while (p > 0) {
                        const double pd = ld2[(p - 1) * KN_Q + q];
                        const int pi = lidx[(p - 1) * KN_Q + q];
                        if (before(pd, pi, d, ci)) break;
                        ld2[p * KN_Q + q] = pd;
                        lidx[p * KN_Q + q] = pi;
                        --p;
                    }
                    ld2[p * KN_Q + q] = d;
                    lidx[p * KN_Q + q] = ci;
                }
            }
        }
    }
    __syncthreads();
    for (int e = t; e < k * KN_Q; e += KN_T) {
        const int q = e / k, r = e - q * k;
        const int64_t row = row0 + q;
        if (row < n) {
            out_idx[(size_t)row * (size_t)k + r] = lidx[r * KN_Q + q];
            out_d2[(size_t)row * (size_t)k + r] = ld2[r * KN_Q + q];
        }
    }
}

// dist[n][k] ascending true distances; one lane per row
__global__ __launch_bounds__(KN_T) void k_fuzzy_knn(const double* __restrict__ dist, int64_t n, int k, double mean_all, double* __restrict__ out_rho,
                                                    double* __restrict__ out_sigma, int32_t* __restrict__ out_iters, double* __restrict__ out_vals) {
    const int64_t i = blockIdx.x * (int64_t)KN_T + threadIdx.x;
    if (i >= n) return;
    const double* __restrict__ d = dist + (size_t)i * (size_t)k;
    const double m = (double)(k + 1);
    const double target = log2(m);
    double rho = 0.0, total = 0.0;
    bool found = false;
    for (int j = 0; j < k; ++j) {
        const double v = d[j];
        if (!found && v > 0.0) {
            rho = v;
            found = true;
        }
        total = __dadd_rn(total, v);
    }
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    int last = 0;
    for (int it = 0; it < 64; ++it) {
        last = it;
        double psum = 0.0;
        for (int j = 0; j < k; ++j) {
            const double e = __dsub_rn(d[j], rho);
            psum = __dadd_rn(psum, e > 0.0 ? exp(-__ddiv_rn(e, mid)) : 1.0);
        }
        if (fabs(__dsub_rn(psum, target)) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = __ddiv_rn(__dadd_rn(lo, hi), 2.0);
        } else {
            lo = mid;
            mid = hi == INFINITY ? __dmul_rn(mid, 2.0) : __ddiv_rn(__dadd_rn(lo, hi), 2.0);
        }
    }
    double sigma = mid;
    const double floor_ = rho > 0.0 ? __dmul_rn(1e-3, __ddiv_rn(total, m)) : __dmul_rn(1e-3, mean_all);
    if (sigma < floor_) sigma = floor_;
    out_rho[i] = rho;
    out_sigma[i] = sigma;
    out_iters[i] = last;
    double* __restrict__ o = out_vals + (size_t)i * (size_t)k;
    for (int j = 0; j < k; ++j) {
        const double e = __dsub_rn(d[j], rho);
        o[j] = (e <= 0.0 || sigma == 0.0) ? 1.0 : exp(-__ddiv_rn(e, sigma));
    }
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_knn_nd_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = KN_Q;
    out_info[1] = KN_C;
    out_info[2] = KN_MAX_D;
    out_info[3] = KN_MAX_K;
    return SQGR_OK;
}

int sqgr_knn_nd(sqgr_ctx* ctx, const void* x, int32_t value_bytes, int64_t n, int32_t D, int64_t ld, int32_t k, int32_t* out_idx,
                double* out_d2) {
    SQGR_REQUIRE(ctx && x && out_idx && out_d2, "null argument");
    SQGR_REQUIRE(value_bytes == 4 || value_bytes == 8, "value_bytes=%d", value_bytes);
    if (D < 1 || D > KN_MAX_D || k < 1 || k > KN_MAX_K || n < 2 || (int64_t)k > n - 1 || n >= ((int64_t)1 << 31)) {
        set_error("sqgr_knn_nd: supported are 1 <= D <= %d columns, 1 <= k <= min(%d, n - 1) neighbours and n < 2^31 rows; found D=%d k=%d n=%lld",
                  KN_MAX_D, KN_MAX_K, D, k, (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_REQUIRE(ld >= D, "ld=%lld < D=%d", (long long)ld, D);
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t count = (size_t)n * (size_t)D;
    DevBuf<double> X, d2;
    DevBuf<int32_t> idx;
    DevBuf<float> stage;
    SQGR_TRY(X.alloc_pooled(count));
    SQGR_TRY(idx.alloc_pooled((size_t)n * (size_t)k));
    SQGR_TRY(d2.alloc_pooled((size_t)n * (size_t)k));
    if (value_bytes == 8) {
        if (ld == D) SQGR_HIP(hipMemcpyAsync(X.p, x, count * 8, hipMemcpyHostToDevice, st));
        else SQGR_HIP(hipMemcpy2DAsync(X.p, (size_t)D * 8, x, (size_t)ld * 8, (size_t)D * 8, (size_t)n, hipMemcpyHostToDevice, st));
    } else {
        SQGR_TRY(stage.alloc_pooled(count));
        if (ld == D) SQGR_HIP(hipMemcpyAsync(stage.p, x, count * 4, hipMemcpyHostToDevice, st));
        else SQGR_HIP(hipMemcpy2DAsync(stage.p, (size_t)D * 4, x, (size_t)ld * 4, (size_t)D * 4, (size_t)n, hipMemcpyHostToDevice, st));
        LaunchTimer t(ctx, "knn_nd_widen");
        k_knn_widen<<<(unsigned)ceil_div((int64_t)count, KN_T), KN_T, 0, st>>>(stage.p, (int64_t)count, X.p);
        SQGR_HIP(hipGetLastError());
    }
    const size_t lds = knn_lds_bytes(k);
    SQGR_TRY(allow_lds(k_knn_nd, lds));
    {
        LaunchTimer t(ctx, "knn_nd");
        k_knn_nd<<<(unsigned)ceil_div(n, KN_Q), KN_T, lds, st>>>(X.p, n, D, k, idx.p, d2.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_idx, idx.p, (size_t)n * (size_t)k * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_d2, d2.p, (size_t)n * (size_t)k * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_fuzzy_knn(sqgr_ctx* ctx, const double* dist, int64_t n, int32_t k, double mean_all, double* out_rho, double* out_sigma,
                   int32_t* out_iters, double* out_vals) {
    SQGR_REQUIRE(ctx && dist && out_rho && out_sigma && out_iters && out_vals, "null argument");
    SQGR_REQUIRE(n >= 1, "n=%lld", (long long)n);
    if (k < 1 || k > KN_MAX_K || n >= ((int64_t)1 << 31)) {
        set_error("sqgr_fuzzy_knn: supported are 1 <= k <= %d neighbours and n < 2^31 rows; found k=%d n=%lld", KN_MAX_K, k, (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nk = (size_t)n * (size_t)k;
    DevBuf<double> dd, rho, sigma, vals;
    DevBuf<int32_t> iters;
    SQGR_TRY(dd.alloc_pooled(nk));
    SQGR_TRY(vals.alloc_pooled(nk));
    SQGR_TRY(rho.alloc_pooled((size_t)n));
    SQGR_TRY(sigma.alloc_pooled((size_t)n));
    SQGR_TRY(iters.alloc_pooled((size_t)n));
    SQGR_HIP(hipMemcpyAsync(dd.p, dist, nk * 8, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(ctx, "fuzzy_knn");
        k_fuzzy_knn<<<(unsigned)ceil_div(n, KN_T), KN_T, 0, st>>>(dd.p, n, k, mean_all, rho.p, sigma.p, iters.p, vals.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_rho, rho.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_sigma, sigma.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_iters, iters.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_vals, vals.p, nk * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}
