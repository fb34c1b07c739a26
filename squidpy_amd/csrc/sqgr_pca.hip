// libsqgr: PCA of a dense float64 matrix resident on the device — the O(n D^2) and O(n D c) parts of scanpy's default `sc.tl.pca`
// (sklearn's PCA(svd_solver="arpack")): column means, the centred scatter matrix and the projection on given components.  The
// D x D eigenproblem between the two stays on the host (squidpy_amd/gr/_niche.py: niche_pca).
//
//   mean_j  = (sum_i F[i][j]) / n
//   S[a][b] = sum_i (F[i][a] - mean_a) * (F[i][b] - mean_b)          the mean is subtracted BEFORE the product; not divided
//   out[i][r] = sum_j (F[i][j] - mean_j) * components[r][j]           j ascending
//
// Float64 throughout, no float atomics, every difference, product and sum rounded on its own (__dsub_rn / __dmul_rn / __dadd_rn: no
// FMA whatever the compiler's contraction setting).  Every order of summation is a function of (n, D) alone:
//
// k_pca_colsum   grid (column tiles of 64, row chunks): thread (column, q) adds the rows begin + q, begin + q + 4, ... of its chunk in
//                ascending order, the four q are added in q order.  Chunks of PCA_CHUNK * ceil(ceil(n / PCA_CHUNK) / PCA_MAX_CHUNKS) rows.
// k_pca_mean     one thread per column: the chunk sums in chunk order, then one division by n.
// k_pca_scatter  the hot path: a symmetric rank-n update over the upper-triangular 64 x 64 tile pairs (ti <= tj) only.  Grid (tile
//                pairs, row chunks); a block stages 32 rows of both tiles' centred columns in LDS (the next 32 are already on their way
//                in registers) and each of its 256 threads owns a 4 x 4 register tile: per row 8 LDS values for 16 products and 16
//                sums, the 16 products formed before the 16 sums.  A thread adds its chunk's rows in ascending order.  Plain VALU
//                tiles, as k_gmm_cov; columns past D are staged as zeros.
// k_pca_scatter_finish  one thread per element of the upper triangle: the chunk partials in chunk order; S[a][b] and S[b][a] are
//                written from the same sum, so the matrix is exactly symmetric.
// k_pca_project  rows across lanes, 64 rows per block.  A strip of 32 centred columns is staged transposed in LDS; the components lie
//                transposed ([D][c padded to 16]) so that the 16 coefficients of a column are one wave-uniform (scalar) read, as
//                k_gmm_estep reads P; every lane keeps its row's c sums in registers.
#include "sqgr_pca.h"

#include <algorithm>
#include <vector>

namespace sqgr {
namespace {

constexpr int PCA_T = 256;
constexpr int PCA_TILE = 64;            // columns of a scatter tile
constexpr int PCA_RT = 32;              // rows staged at a time
constexpr int PCA_CHUNK = 512;          // rows of a chunk: a multiple of this
constexpr int PCA_MAX_CHUNKS = 1024;    // chunks of the column sums at most
constexpr int PCA_TARGET_BLOCKS = 2048; // tile pairs x chunks of the scatter grid, about
constexpr int PCA_MAX_D = 4096;
constexpr int PCA_MAX_C = 64;
constexpr int PCA_P_T = 64;             // rows of a projection tile = threads of its block
constexpr int PCA_P_JW = 32;            // columns of a projection strip (16.6 KB of LDS per block: two waves per SIMD)
constexpr int PCA_P_PITCH = PCA_P_T + 1;

struct PcaGeometry {
    int nt = 0, npairs = 0;
    int64_t mean_rows = 0, scat_rows = 0;  // rows per chunk
    int mean_chunks = 0, scat_chunks = 0;
};

// a function of (n, D) alone: the order of every sum follows from it
PcaGeometry pca_geometry(int64_t n, int D) {
    PcaGeometry q;
    q.nt = (D + PCA_TILE - 1) / PCA_TILE;
    q.npairs = q.nt * (q.nt + 1) / 2;
    const int64_t base = ceil_div(n, PCA_CHUNK);
    q.mean_rows = PCA_CHUNK * ceil_div(base, PCA_MAX_CHUNKS);
    q.mean_chunks = (int)ceil_div(n, q.mean_rows);
    const int64_t max_chunks = std::min<int64_t>(PCA_MAX_CHUNKS, std::max<int64_t>(1, PCA_TARGET_BLOCKS / q.npairs));
    q.scat_rows = PCA_CHUNK * ceil_div(base, max_chunks);
    q.scat_chunks = (int)ceil_div(n, q.scat_rows);
    return q;
}

__global__ __launch_bounds__(PCA_T) void k_pca_widen(const float* __restrict__ in, int64_t n, int c, int64_t ld, double* __restrict__ out) {
    const int64_t t = blockIdx.x * (int64_t)PCA_T + threadIdx.x;
    if (t >= n * c) return;
    const int64_t i = t / c;
    const int j = (int)(t - i * c);
    out[(size_t)i * (size_t)ld + j] = (double)in[t];
}

__global__ __launch_bounds__(PCA_T) void k_pca_colsum(const double* __restrict__ F, int64_t n, int D, int64_t rows_per_chunk,
                                                      double* __restrict__ part) {
    __shared__ double red[4][PCA_TILE];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int col = blockIdx.x * PCA_TILE + c;
    const int64_t begin = blockIdx.y * rows_per_chunk, end = min(n, begin + rows_per_chunk);
    double s = 0.0;
    if (col < D)
        for (int64_t r = begin + q; r < end; r += 4) s = __dadd_rn(s, F[(size_t)r * (size_t)D + col]);
    red[q][c] = s;
    __syncthreads();
    if (q == 0 && col < D) {
        double v = red[0][c];
        for (int g = 1; g < 4; ++g) v = __dadd_rn(v, red[g][c]);
        part[(size_t)blockIdx.y * D + col] = v;
    }
}

__global__ __launch_bounds__(PCA_T) void k_pca_mean(const double* __restrict__ part, int nchunks, int D, int64_t n, double* __restrict__ mean) {
    const int col = blockIdx.x * PCA_T + threadIdx.x;
    if (col >= D) return;
    double s = 0.0;
    for (int b = 0; b < nchunks; ++b) s = __dadd_rn(s, part[(size_t)b * D + col]);
    mean[col] = __ddiv_rn(s, (double)n);
}

// tile pair p of the upper triangle in row order: (0,0) (0,1) ... (0,nt-1) (1,1) ...
__device__ __forceinline__ void pair_tiles(int p, int nt, int* ti, int* tj) {
    int a = 0;
    while (p >= nt - a) {
        p -= nt - a;
        ++a;
    }
    *ti = a;
    *tj = a + p;
}

// part[chunk][pair][64][64] = sum over the chunk's rows, ascending, of (x_a - mean_a) * (x_b - mean_b), a in tile ti, b in tile tj
__global__ __launch_bounds__(PCA_T) void k_pca_scatter(const double* __restrict__ F, int64_t n, int D, const double* __restrict__ mean,
                                                       int64_t rows_per_chunk, int nt, double* __restrict__ part) {
    __shared__ double A[PCA_RT][PCA_TILE];
    __shared__ double B[PCA_RT][PCA_TILE];
    int ti, tj;
    pair_tiles((int)blockIdx.x, nt, &ti, &tj);
    const bool diag = ti == tj;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int sc = t & 63, sr = t >> 6;  // staging: one column, rows sr, sr + 4, ...
    const int ca = ti * PCA_TILE + sc, cb = tj * PCA_TILE + sc;
    const bool has_a = ca < D, has_b = cb < D && !diag;
    const double ma = has_a ? mean[ca] : 0.0, mb = has_b ? mean[cb] : 0.0;
    const int64_t begin = blockIdx.y * rows_per_chunk, end = min(n, begin + rows_per_chunk);
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    double na[PCA_RT / 4], nb[PCA_RT / 4];
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int k = 0; k < PCA_RT / 4; ++k) {
            const int64_t row = r0 + sr + 4 * k;
            const bool ok = row < end;
            na[k] = (ok && has_a) ? __dsub_rn(F[(size_t)row * (size_t)D + ca], ma) : 0.0;
            nb[k] = (ok && has_b) ? __dsub_rn(F[(size_t)row * (size_t)D + cb], mb) : 0.0;
        }
    };
    if (begin < end) fetch(begin);
    const double (*Bp)[PCA_TILE] = diag ? A : B;
    for (int64_t r0 = begin; r0 < end; r0 += PCA_RT) {
        const int rows = (int)min((int64_t)PCA_RT, end - r0);
        __syncthreads();  // the previous sub-tile's readers are done
#pragma unroll
        for (int k = 0; k < PCA_RT / 4; ++k) {
            A[sr + 4 * k][sc] = na[k];
            if (!diag) B[sr + 4 * k][sc] = nb[k];
        }
        __syncthreads();
        if (r0 + PCA_RT < end) fetch(r0 + PCA_RT);  // the next sub-tile travels while this one is used
        for (int r = 0; r < rows; ++r) {
            double a[4], b[4], prod[16];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                a[p] = A[r][4 * ty + p];
                b[p] = Bp[r][4 * tx + p];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) prod[p * 4 + q] = __dmul_rn(a[p], b[q]);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = __dadd_rn(acc[e], prod[e]);
        }
    }
    double* __restrict__ o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(PCA_TILE * PCA_TILE);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) o[(4 * ty + p) * PCA_TILE + 4 * tx + q] = acc[p * 4 + q];
}

// grid (pairs, 16): S[a][b] = S[b][a] = the chunk partials in chunk order, for a <= b < D
__global__ __launch_bounds__(PCA_T) void k_pca_scatter_finish(const double* __restrict__ part, int nchunks, int npairs, int nt, int D,
                                                              double* __restrict__ S) {
    int ti, tj;
    pair_tiles((int)blockIdx.x, nt, &ti, &tj);
    const int e = blockIdx.y * PCA_T + threadIdx.x;
    const int i = e >> 6, j = e & 63;
    const int a = ti * PCA_TILE + i, b = tj * PCA_TILE + j;
    if (a >= D || b >= D || a > b) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s = __dadd_rn(s, part[((size_t)c * npairs + blockIdx.x) * (size_t)(PCA_TILE * PCA_TILE) + e]);
    S[(size_t)a * D + b] = s;
    S[(size_t)b * D + a] = s;
}

// out[row][r] = sum over j ascending of (F[row][j] - mean[j]) * Ct[j][r];  Ct: [D][cp], cp = 16 NC, columns past c are zeros
template <int NC>
__global__ __launch_bounds__(PCA_P_T) void k_pca_project(const double* __restrict__ F, int64_t n, int D, const double* __restrict__ mean,
                                                         const double* __restrict__ Ct, int c, double* __restrict__ out) {
    __shared__ double xs[PCA_P_JW * PCA_P_PITCH];
    constexpr int cp = 16 * NC;
    const int t = threadIdx.x;
    const int64_t row0 = blockIdx.x * (int64_t)PCA_P_T;
    const int rows = (int)min((int64_t)PCA_P_T, n - row0);
    double acc[cp];
#pragma unroll
    for (int r = 0; r < cp; ++r) acc[r] = 0.0;
    for (int j0 = 0; j0 < D; j0 += PCA_P_JW) {
        const int jw = min(PCA_P_JW, D - j0);
        __syncthreads();  // the previous strip's readers are done
        for (int idx = t; idx < PCA_P_T * jw; idx += PCA_P_T) {
            const int r = idx / jw, jj = idx - r * jw;
            xs[jj * PCA_P_PITCH + r] = r < rows ? __dsub_rn(F[(size_t)(row0 + r) * (size_t)D + j0 + jj], mean[j0 + jj]) : 0.0;
        }
        __syncthreads();
        for (int jj = 0; jj < jw; ++jj) {
            const double diff = xs[jj * PCA_P_PITCH + t];
            const double* __restrict__ cj = Ct + (size_t)(j0 + jj) * cp;  // the same for every lane
            double prod[cp];
#pragma unroll
            for (int r = 0; r < cp; ++r) prod[r] = __dmul_rn(diff, cj[r]);
#pragma unroll
            for (int r = 0; r < cp; ++r) acc[r] = __dadd_rn(acc[r], prod[r]);
        }
    }
    if (t < rows) {
        double* __restrict__ o = out + (size_t)(row0 + t) * (size_t)c;
#pragma unroll
        for (int r = 0; r < cp; ++r)
            if (r < c) o[r] = acc[r];
    }
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_pca_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = PCA_CHUNK;
    out_info[1] = PCA_MAX_D;
    out_info[2] = PCA_MAX_C;
    out_info[3] = PCA_TILE;
    return SQGR_OK;
}

int sqgr_pca_geometry(int64_t n, int32_t D, int64_t* out) {
    SQGR_REQUIRE(out, "null argument");
    SQGR_REQUIRE(n >= 2 && n < ((int64_t)1 << 31) && D >= 2 && D <= PCA_MAX_D, "sqgr_pca_geometry: n=%lld D=%d", (long long)n, D);
    const PcaGeometry q = pca_geometry(n, D);
    const int64_t v[10] = {q.nt, q.npairs, q.mean_rows, q.scat_rows, q.mean_chunks, q.scat_chunks, PCA_CHUNK, PCA_MAX_CHUNKS, PCA_TARGET_BLOCKS,
                           PCA_TILE};
    std::copy(v, v + 10, out);
    return SQGR_OK;
}

int sqgr_pca_create(sqgr_ctx* ctx, int64_t n, int32_t D, sqgr_pca** out) {
    SQGR_REQUIRE(ctx && out, "null argument");
    if (n < 2 || n >= ((int64_t)1 << 31) || D < 2 || D > PCA_MAX_D) {
        set_error("sqgr_pca_create: supported are 2 <= n < 2^31 rows and 2 <= D <= %d columns; found n=%lld D=%d", PCA_MAX_D, (long long)n, D);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    sqgr_pca* h = new sqgr_pca();
    h->ctx = ctx;
    h->n = n;
    h->D = D;
    int rc = h->F.alloc_pooled((size_t)n * (size_t)D);
    if (rc == SQGR_OK) rc = h->mean.alloc((size_t)D);
    if (rc == SQGR_OK && hipMemsetAsync(h->F.p, 0, (size_t)n * (size_t)D * 8, ctx->stream) != hipSuccess) {
        set_error("sqgr_pca_create: hipMemsetAsync failed");
        rc = SQGR_ERR_HIP;
    }
    if (rc != SQGR_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return SQGR_OK;
}

int sqgr_pca_destroy(sqgr_pca* h) {
    if (!h) return SQGR_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return SQGR_OK;
}

int sqgr_pca_upload(sqgr_pca* h, const void* x, int32_t value_bytes, int64_t ld, int32_t col0, int32_t n_cols) {
    SQGR_REQUIRE(h && x, "null argument");
    SQGR_REQUIRE(value_bytes == 4 || value_bytes == 8, "value_bytes=%d", value_bytes);
    SQGR_REQUIRE(col0 >= 0 && n_cols >= 1 && (int64_t)col0 + n_cols <= h->D, "columns [%d, %d + %d) outside [0, %d)", col0, col0, n_cols, h->D);
    SQGR_REQUIRE(ld >= n_cols, "ld=%lld < n_cols=%d", (long long)ld, n_cols);
    SQGR_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int64_t n = h->n;
    h->have_mean = false;
    double* dst = h->F.p + col0;
    if (value_bytes == 8) {
        if (ld == n_cols && n_cols == h->D)
            SQGR_HIP(hipMemcpyAsync(dst, x, (size_t)n * (size_t)n_cols * 8, hipMemcpyHostToDevice, st));
        else
            SQGR_HIP(hipMemcpy2DAsync(dst, (size_t)h->D * 8, x, (size_t)ld * 8, (size_t)n_cols * 8, (size_t)n, hipMemcpyHostToDevice, st));
        SQGR_HIP(hipStreamSynchronize(st));
        return SQGR_OK;
    }
    DevBuf<float> stage;  // [n][n_cols]
    SQGR_TRY(stage.alloc_pooled((size_t)n * (size_t)n_cols));
    if (ld == n_cols)
        SQGR_HIP(hipMemcpyAsync(stage.p, x, (size_t)n * (size_t)n_cols * 4, hipMemcpyHostToDevice, st));
    else
        SQGR_HIP(hipMemcpy2DAsync(stage.p, (size_t)n_cols * 4, x, (size_t)ld * 4, (size_t)n_cols * 4, (size_t)n, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(h->ctx, "pca_widen");
        k_pca_widen<<<(unsigned)ceil_div(n * n_cols, PCA_T), PCA_T, 0, st>>>(stage.p, n, n_cols, h->D, dst);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_pca_moments(sqgr_pca* h, double* out_mean, double* out_scatter) {
    SQGR_REQUIRE(h && out_mean && out_scatter, "null argument");
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = h->n;
    const int D = h->D;
    const PcaGeometry q = pca_geometry(n, D);
    DevBuf<double> mean_part, scat_part, S;
    SQGR_TRY(mean_part.alloc_pooled((size_t)q.mean_chunks * D));
    SQGR_TRY(scat_part.alloc_pooled((size_t)q.scat_chunks * q.npairs * PCA_TILE * PCA_TILE));
    SQGR_TRY(S.alloc_pooled((size_t)D * D));
    {
        LaunchTimer t(ctx, "pca_mean");
        k_pca_colsum<<<dim3(q.nt, q.mean_chunks), PCA_T, 0, st>>>(h->F.p, n, D, q.mean_rows, mean_part.p);
        SQGR_HIP(hipGetLastError());
        k_pca_mean<<<(unsigned)ceil_div(D, PCA_T), PCA_T, 0, st>>>(mean_part.p, q.mean_chunks, D, n, h->mean.p);
        SQGR_HIP(hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "pca_scatter");
        k_pca_scatter<<<dim3(q.npairs, q.scat_chunks), PCA_T, 0, st>>>(h->F.p, n, D, h->mean.p, q.scat_rows, q.nt, scat_part.p);
        SQGR_HIP(hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "pca_scatter_finish");
        k_pca_scatter_finish<<<dim3(q.npairs, PCA_TILE * PCA_TILE / PCA_T), PCA_T, 0, st>>>(scat_part.p, q.scat_chunks, q.npairs, q.nt, D, S.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_mean, h->mean.p, (size_t)D * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_scatter, S.p, (size_t)D * D * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    h->have_mean = true;
    return SQGR_OK;
}

int sqgr_pca_project(sqgr_pca* h, const double* components, int32_t c, double* out) {
    SQGR_REQUIRE(h && components && out, "null argument");
    const int64_t n = h->n;
    const int D = h->D;
    SQGR_REQUIRE(c >= 1, "sqgr_pca_project: c=%d", c);
    if (c > PCA_MAX_C || c >= std::min<int64_t>(n, D)) {
        set_error("sqgr_pca_project: supported are 1 <= c <= %d components with c < min(n, D); found c=%d n=%lld D=%d", PCA_MAX_C, c, (long long)n, D);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_REQUIRE(h->have_mean, "sqgr_pca_project: sqgr_pca_moments has not run since the matrix was last written");
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nc = (c + 15) / 16, cp = 16 * nc;
    std::vector<double> ct((size_t)D * cp, 0.0);
    for (int r = 0; r < c; ++r)
        for (int j = 0; j < D; ++j) ct[(size_t)j * cp + r] = components[(size_t)r * D + j];
    DevBuf<double> Ct, Y;
    SQGR_TRY(Ct.alloc(ct.size()));
    SQGR_TRY(Y.alloc_pooled((size_t)n * (size_t)c));
    SQGR_HIP(hipMemcpyAsync(Ct.p, ct.data(), ct.size() * 8, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(ctx, "pca_project");
        const unsigned grid = (unsigned)ceil_div(n, PCA_P_T);
        if (nc == 1) k_pca_project<1><<<grid, PCA_P_T, 0, st>>>(h->F.p, n, D, h->mean.p, Ct.p, c, Y.p);
        else if (nc == 2) k_pca_project<2><<<grid, PCA_P_T, 0, st>>>(h->F.p, n, D, h->mean.p, Ct.p, c, Y.p);
        else if (nc == 3) k_pca_project<3><<<grid, PCA_P_T, 0, st>>>(h->F.p, n, D, h->mean.p, Ct.p, c, Y.p);
        else k_pca_project<4><<<grid, PCA_P_T, 0, st>>>(h->F.p, n, D, h->mean.p, Ct.p, c, Y.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out, Y.p, (size_t)n * (size_t)c * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}
