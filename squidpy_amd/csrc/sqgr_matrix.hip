// libsqgr: the expression matrix resident on the device — upload and validation (dense, CSR, CSC; float32 or float64), the by-column
// twin of a CSR matrix, and the expansion of columns into the gene-major float64 blocks X[g][i] that the statistics work on.
#include "sqgr_matrix.h"

namespace sqgr {

constexpr int GT = MATRIX_TILE;

// ---- cell-major input D[i][G_all] (what AnnData's X is) -> the staged gene-major block X[gl][i] of genes g0..g0+gc
__global__ __launch_bounds__(256) void k_cells_to_genes(const double* __restrict__ D, int64_t ld, int64_t n, int64_t g0, int gc,
                                                        double* __restrict__ X) {
    __shared__ double tile[GT][GT + 1];
    const int64_t i0 = (int64_t)blockIdx.x * GT;
    const int gb = blockIdx.y * GT;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < GT; r += 4) {  // r: spot inside tile, tx: gene
        const int64_t i = i0 + r;
        tile[r][tx] = (i < n && gb + tx < gc) ? D[(size_t)i * ld + g0 + gb + tx] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < GT; r += 4) {  // r: gene inside tile, tx: spot
        const int64_t i = i0 + tx;
        if (gb + r < gc && i < n) X[(size_t)(gb + r) * n + i] = tile[tx][r];
    }
}

// The same from a float32 matrix (AnnData's usual `X` dtype): widened to float64 on the way — exactly what
// `.astype(float64)` does on the host, so everything downstream is bit-identical to the float64 upload.
__global__ __launch_bounds__(256) void k_cells_to_genes_f32(const float* __restrict__ D, int64_t ld, int64_t n, int64_t g0, int gc,
                                                            double* __restrict__ X) {
    __shared__ double tile[GT][GT + 1];
    const int64_t i0 = (int64_t)blockIdx.x * GT;
    const int gb = blockIdx.y * GT;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < GT; r += 4) {
        const int64_t i = i0 + r;
        tile[r][tx] = (i < n && gb + tx < gc) ? (double)D[(size_t)i * ld + g0 + gb + tx] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < GT; r += 4) {
        const int64_t i = i0 + tx;
        if (gb + r < gc && i < n) X[(size_t)(gb + r) * n + i] = tile[tx][r];
    }
}

// Sparse expression (scipy CSR / CSC of the cells x genes matrix, float32 or float64 values) -> the staged gene-major block
// X[gl][i] of genes g0..g0+gc, which the caller has zeroed: the dense block `toarray()` would give, formed on the device.
// Stored entries of one cell (CSR) / one gene (CSC) land in distinct cells of X unless the matrix holds duplicates, which
// scipy sums — so does the atomic add (0 + v is exact: canonical matrices reproduce `toarray()` bit for bit).
// CSR: one thread per cell, binary search of the first stored gene >= g0 in its (sorted) row.
template <typename V>
__global__ __launch_bounds__(256) void k_csr_to_genes(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const V* __restrict__ values, int64_t n, int64_t g0, int gc, double* __restrict__ X) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t lo = indptr[i], hi = indptr[i + 1];
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indices[mid] < g0) lo = mid + 1; else hi = mid;
    }
    for (int64_t e = lo; e < end; ++e) {
        const int64_t c = indices[e] - g0;
        if (c >= gc) break;
        atomicAdd(&X[(size_t)c * n + i], (double)values[e]);
    }
}

// CSC: block (x, gene): the gene's stored cells, strided over the block's threads and the blocks of grid.x
template <typename V>
__global__ __launch_bounds__(256) void k_csc_to_genes(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const V* __restrict__ values, int64_t n, int64_t g0, double* __restrict__ X) {
    const int64_t g = blockIdx.y;
    const int64_t e0 = indptr[g0 + g], e1 = indptr[g0 + g + 1];
    for (int64_t e = e0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < e1; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&X[(size_t)g * n + indices[e]], (double)values[e]);
}

// one wave per major slice: flags[0] an index outside [0, minor), flags[1] a slice that is not ascending, flags[2] a repeated index
__global__ __launch_bounds__(256) void k_check_sparse(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t nslices,
                                                      int64_t minor, int* __restrict__ flags) {
    const int64_t j = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
    if (j >= nslices) return;
    const int64_t a = indptr[j], b = indptr[j + 1];
    int bad_range = 0, bad_order = 0, dup = 0;
    for (int64_t e = a + (threadIdx.x & 63); e < b; e += 64) {
        const int32_t c = indices[e];
        bad_range |= (c < 0 || c >= minor);
        if (e > a) {
            bad_order |= indices[e - 1] > c;
            dup |= indices[e - 1] == c;
        }
    }
    if (bad_range) flags[0] = 1;
    if (bad_order) flags[1] = 1;
    if (dup) flags[2] = 1;
}

// Feature blocks given as a LIST of columns (the reference's HVG default and explicit `genes` subsets, gr/_ppatterns.py:156-166:
// `adata[:, genes].X` — a copy of the selected columns on the host; here the selection happens on the device).
// Dense rows: the 64 x 64 LDS transpose with gathered columns.
template <typename T>
__global__ __launch_bounds__(256) void k_cells_to_genes_idx(const T* __restrict__ D, int64_t ld, int64_t n, const int32_t* __restrict__ cols, int gc,
                                                            double* __restrict__ X) {
    __shared__ double tile[GT][GT + 1];
    const int64_t i0 = (int64_t)blockIdx.x * GT;
    const int gb = blockIdx.y * GT;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c = (gb + tx < gc) ? cols[gb + tx] : -1;
    for (int r = ty; r < GT; r += 4) {
        const int64_t i = i0 + r;
        tile[r][tx] = (i < n && c >= 0) ? (double)D[(size_t)i * ld + c] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < GT; r += 4) {
        const int64_t i = i0 + tx;
        if (gb + r < gc && i < n) X[(size_t)(gb + r) * n + i] = tile[tx][r];
    }
}

// CSC: block (x, g) expands column cols[g]
template <typename V>
__global__ __launch_bounds__(256) void k_csc_to_genes_idx(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                          const V* __restrict__ values, int64_t n, const int32_t* __restrict__ cols,
                                                          double* __restrict__ X) {
    const int64_t g = blockIdx.y, c = cols[g];
    const int64_t e0 = indptr[c], e1 = indptr[c + 1];
    for (int64_t e = e0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < e1; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&X[(size_t)g * n + indices[e]], (double)values[e]);
}

// CSR -> CSC on the device (once per matrix, when a column LIST is asked for): column histogram, exclusive scan (host: n_cols + 1
// numbers), scatter through per-column cursors.  The order inside a column is whatever the atomics give — the expansion adds
// every stored entry into its own cell of a zeroed block, so it does not matter (a canonical matrix has one entry per cell).
__global__ void k_count_columns(const int32_t* __restrict__ indices, int64_t nnz, unsigned long long* __restrict__ cnt) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < nnz) atomicAdd(&cnt[indices[e]], 1ull);
}
template <typename V>
__global__ __launch_bounds__(256) void k_scatter_to_columns(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const V* __restrict__ values, int64_t n_rows, unsigned long long* __restrict__ cursor,
                                                            int32_t* __restrict__ out_rows, V* __restrict__ out_vals) {
    const int64_t i = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);  // one wave per row
    if (i >= n_rows) return;
    for (int64_t e = indptr[i] + (threadIdx.x & 63); e < indptr[i + 1]; e += 64) {
        const unsigned long long pos = atomicAdd(&cursor[indices[e]], 1ull);
        out_rows[pos] = (int32_t)i;
        out_vals[pos] = values[e];
    }
}

// int64 index arrays of a scipy matrix with more than 2^31 stored entries -> the library's layout
__global__ void k_narrow_indices(const int64_t* __restrict__ src, int64_t count, int32_t* __restrict__ dst) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // an index that does not fit int32 must not wrap into the valid range: it becomes -1, which the range check that follows
    // (k_check_sparse: 0 <= index < minor) rejects like any other out-of-range index
    if (t < count) {
        const int64_t v = src[t];
        dst[t] = (v < 0 || v > (int64_t)0x7fffffff) ? -1 : (int32_t)v;
    }
}
__global__ void k_widen_indptr(const int32_t* __restrict__ src, int64_t count, int64_t* __restrict__ dst) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < count) dst[t] = src[t];
}

}  // namespace sqgr

using namespace sqgr;

int sqgr_matrix::ensure_by_column() const {
    if (kind != 1 || by_col_ready) return SQGR_OK;
    hipStream_t st = ctx->stream;
    DevBuf<unsigned long long> cnt;
    SQGR_TRY(cnt.alloc((size_t)n_cols + 1));
    SQGR_HIP(hipMemsetAsync(cnt.p, 0, ((size_t)n_cols + 1) * 8, st));
    const size_t count = (size_t)std::max<int64_t>(nnz, 1);
    SQGR_TRY(c_indptr.alloc((size_t)n_cols + 1));
    SQGR_TRY(c_rows.alloc_pooled(count));  // (every entry is written by the scatter)
    SQGR_TRY(f32 ? c_data32.alloc_pooled(count) : c_data.alloc_pooled(count));
    LaunchTimer t(ctx, "autocorr_csr_to_csc");
    if (nnz > 0) k_count_columns<<<(unsigned)ceil_div(nnz, 256), 256, 0, st>>>(indices.p, nnz, cnt.p);
    std::vector<unsigned long long> h((size_t)n_cols + 1);
    SQGR_HIP(hipMemcpyAsync(h.data(), cnt.p, ((size_t)n_cols + 1) * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> ptr((size_t)n_cols + 1);
    unsigned long long run = 0;
    for (int64_t c = 0; c <= n_cols; ++c) {  // exclusive scan; the cursors start at the column starts
        const unsigned long long v = c < n_cols ? h[c] : 0;
        ptr[c] = (int64_t)run;
        h[c] = run;
        run += v;
    }
    SQGR_HIP(hipMemcpyAsync(c_indptr.p, ptr.data(), ((size_t)n_cols + 1) * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(cnt.p, h.data(), ((size_t)n_cols + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz > 0) {
        if (f32) k_scatter_to_columns<float><<<(unsigned)ceil_div(n_rows, 4), 256, 0, st>>>(indptr.p, indices.p, data32.p, n_rows, cnt.p, c_rows.p, c_data32.p);
        else k_scatter_to_columns<double><<<(unsigned)ceil_div(n_rows, 4), 256, 0, st>>>(indptr.p, indices.p, data.p, n_rows, cnt.p, c_rows.p, c_data.p);
    }
    SQGR_HIP(hipGetLastError());
    SQGR_HIP(hipStreamSynchronize(st));  // `cnt`, `h`, `ptr` are released on return
    by_col_ready = true;
    return SQGR_OK;
}

namespace sqgr {
hipError_t expand_column_list(const sqgr_matrix* dm, const int32_t* dev_cols, int gc, double* X, hipStream_t st) {
    const int64_t n = dm->n_rows;
    if (dm->kind == 0) {
        const dim3 tgrid((unsigned)ceil_div(n, GT), (unsigned)ceil_div(gc, GT));
        if (dm->f32) k_cells_to_genes_idx<float><<<tgrid, 256, 0, st>>>(dm->data32.p, dm->ld, n, dev_cols, gc, X);
        else k_cells_to_genes_idx<double><<<tgrid, 256, 0, st>>>(dm->data.p, dm->ld, n, dev_cols, gc, X);
    } else {
        const hipError_t e = hipMemsetAsync(X, 0, (size_t)gc * n * 8, st);
        if (e != hipSuccess) return e;
        const bool twin = dm->kind == 1;  // CSR: its by-column twin (ensure_by_column, called by the owner of the column list)
        const int64_t* cp = twin ? dm->c_indptr.p : dm->indptr.p;
        const int32_t* cr = twin ? dm->c_rows.p : dm->indices.p;
        const dim3 cgrid(8, (unsigned)gc);
        if (dm->f32) k_csc_to_genes_idx<float><<<cgrid, 256, 0, st>>>(cp, cr, twin ? dm->c_data32.p : dm->data32.p, n, dev_cols, X);
        else k_csc_to_genes_idx<double><<<cgrid, 256, 0, st>>>(cp, cr, twin ? dm->c_data.p : dm->data.p, n, dev_cols, X);
    }
    return hipGetLastError();
}

hipError_t expand_dense_f64(const double* D, int64_t ld, int64_t n, int64_t g0, int gc, double* X, hipStream_t st) {
    k_cells_to_genes<<<dim3((unsigned)ceil_div(n, GT), (unsigned)ceil_div(gc, GT)), 256, 0, st>>>(D, ld, n, g0, gc, X);
    return hipGetLastError();
}

hipError_t expand_column_range(const sqgr_matrix* dm, int64_t col0, int64_t g0, int gc, double* X, hipStream_t st) {
    const int64_t n = dm->n_rows;
    if (dm->kind == 0 && !dm->f32) return expand_dense_f64(dm->data.p + col0, dm->ld, n, g0, gc, X, st);
    if (dm->kind == 0) {
        const dim3 tgrid((unsigned)ceil_div(n, GT), (unsigned)ceil_div(gc, GT));
        k_cells_to_genes_f32<<<tgrid, 256, 0, st>>>(dm->data32.p + col0, dm->ld, n, g0, gc, X);
    } else {
        const hipError_t e = hipMemsetAsync(X, 0, (size_t)gc * n * 8, st);
        if (e != hipSuccess) return e;
        if (dm->kind == 1) {
            if (dm->f32) k_csr_to_genes<float><<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(dm->indptr.p, dm->indices.p, dm->data32.p, n, col0 + g0, gc, X);
            else k_csr_to_genes<double><<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(dm->indptr.p, dm->indices.p, dm->data.p, n, col0 + g0, gc, X);
        } else {
            const dim3 cgrid(8, (unsigned)gc);
            if (dm->f32) k_csc_to_genes<float><<<cgrid, 256, 0, st>>>(dm->indptr.p, dm->indices.p, dm->data32.p, n, col0 + g0, X);
            else k_csc_to_genes<double><<<cgrid, 256, 0, st>>>(dm->indptr.p, dm->indices.p, dm->data.p, n, col0 + g0, X);
        }
    }
    return hipGetLastError();
}
}  // namespace sqgr

extern "C" {

int sqgr_matrix_create_dense(sqgr_ctx* ctx, const void* x, int32_t value_bytes, int64_t n_rows, int64_t n_cols, int64_t ld,
                             sqgr_matrix** out) {
    SQGR_REQUIRE(ctx && x && out && n_rows > 0 && n_cols > 0, "null argument or empty matrix");
    SQGR_REQUIRE(value_bytes == 4 || value_bytes == 8, "value_bytes must be 4 (float32) or 8 (float64), found %d", value_bytes);
    SQGR_REQUIRE(ld >= n_cols, "row pitch %lld < %lld columns", (long long)ld, (long long)n_cols);
    *out = nullptr;
    SQGR_HIP(hipSetDevice(ctx->device));
    sqgr_matrix* m = new sqgr_matrix();
    m->ctx = ctx;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->ld = n_cols;  // stored densely whatever the pitch of the source
    m->f32 = value_bytes == 4;
    const size_t count = (size_t)n_rows * n_cols;
    int rc = m->f32 ? m->data32.alloc_pooled(count) : m->data.alloc_pooled(count);  // (overwritten whole by the upload)
    if (rc != SQGR_OK) {
        delete m;
        return rc;
    }
    void* dst = m->f32 ? (void*)m->data32.p : (void*)m->data.p;
    hipError_t e = (ld == n_cols) ? hipMemcpyAsync(dst, x, count * value_bytes, hipMemcpyHostToDevice, ctx->stream)
                                  : hipMemcpy2DAsync(dst, (size_t)n_cols * value_bytes, x, (size_t)ld * value_bytes, (size_t)n_cols * value_bytes,
                                                     (size_t)n_rows, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        set_error("matrix upload failed: %s", hipGetErrorString(e));
        delete m;
        return SQGR_ERR_HIP;
    }
    *out = m;
    return SQGR_OK;
}

// The same matrix filled column block by column block WHILE the first blocks are being worked on: sqgr_matrix_alloc_dense reserves
// the device array, sqgr_matrix_upload_columns copies a column range of the host matrix into it on the context's copy stream and
// waits for that stream only — it may be called from another host thread than the one that runs the statistics (the pool and the
// error state are thread-safe; nothing else of the context is touched).  16 GB of dense float64 cross PCIe in 0.29 s; uploaded
// whole before the first feature block, config 3 took 0.29 + 0.58 s.
int sqgr_matrix_alloc_dense(sqgr_ctx* ctx, int32_t value_bytes, int64_t n_rows, int64_t n_cols, sqgr_matrix** out) {
    SQGR_REQUIRE(ctx && out && n_rows > 0 && n_cols > 0, "null argument or empty matrix");
    SQGR_REQUIRE(value_bytes == 4 || value_bytes == 8, "value_bytes must be 4 (float32) or 8 (float64), found %d", value_bytes);
    *out = nullptr;
    SQGR_HIP(hipSetDevice(ctx->device));
    sqgr_matrix* m = new sqgr_matrix();
    m->ctx = ctx;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->ld = n_cols;
    m->f32 = value_bytes == 4;
    const size_t count = (size_t)n_rows * n_cols;
    const int rc = m->f32 ? m->data32.alloc_pooled(count) : m->data.alloc_pooled(count);  // (every column is uploaded before it is read)
    if (rc != SQGR_OK) {
        delete m;
        return rc;
    }
    m->cols_pending = n_cols;
    streaming_upload_begin();  // closed by the upload of the last column (or by sqgr_matrix_destroy)
    *out = m;
    return SQGR_OK;
}

int sqgr_matrix_upload_columns(sqgr_matrix* m, const void* x, int64_t ld, int64_t col0, int64_t n_cols) {
    SQGR_REQUIRE(m && x && m->kind == 0, "null argument or not a dense matrix");
    SQGR_REQUIRE(col0 >= 0 && n_cols > 0 && col0 + n_cols <= m->n_cols && ld >= n_cols, "columns [%lld, %lld) of %lld, row pitch %lld", (long long)col0,
                 (long long)(col0 + n_cols), (long long)m->n_cols, (long long)ld);
    sqgr_ctx* ctx = m->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    const size_t vb = m->f32 ? 4 : 8;
    char* dst = (m->f32 ? reinterpret_cast<char*>(m->data32.p) : reinterpret_cast<char*>(m->data.p)) + (size_t)col0 * vb;
    hipError_t e = hipMemcpy2DAsync(dst, (size_t)m->n_cols * vb, x, (size_t)ld * vb, (size_t)n_cols * vb, (size_t)m->n_rows, hipMemcpyHostToDevice,
                                    ctx->copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
    if (e != hipSuccess) {
        set_error("matrix upload failed: %s", hipGetErrorString(e));
        return SQGR_ERR_HIP;
    }
    if (m->cols_pending > 0) {
        m->cols_pending -= std::min<int64_t>(n_cols, m->cols_pending);
        if (m->cols_pending == 0) streaming_upload_end();
    }
    return SQGR_OK;
}

int sqgr_matrix_create(sqgr_ctx* ctx, const double* x, int64_t n_rows, int64_t n_cols, sqgr_matrix** out) {
    return sqgr_matrix_create_dense(ctx, x, 8, n_rows, n_cols, n_cols, out);
}

// kind 1: CSR (indptr has n_rows + 1 entries, indices are columns), kind 2: CSC (n_cols + 1, rows)
static int matrix_create_sparse(sqgr_ctx* ctx, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, const void* indices,
                                int32_t index_bytes, const void* values, int32_t value_bytes, sqgr_matrix** out) {
    SQGR_REQUIRE(ctx && indptr && out && n_rows > 0 && n_cols > 0 && nnz >= 0, "null argument or empty matrix");
    SQGR_REQUIRE((indices && values) || nnz == 0, "indices/values is NULL");
    SQGR_REQUIRE(index_bytes == 4 || index_bytes == 8, "index_bytes must be 4 or 8, found %d", index_bytes);
    SQGR_REQUIRE(value_bytes == 4 || value_bytes == 8, "value_bytes must be 4 (float32) or 8 (float64), found %d", value_bytes);
    SQGR_REQUIRE(n_rows < (int64_t)0x7fffffff && n_cols < (int64_t)0x7fffffff, "more than 2^31 rows or columns");
    *out = nullptr;
    const int64_t nptr = (kind == 1 ? n_rows : n_cols) + 1, minor = kind == 1 ? n_cols : n_rows;
    // host-side validation (the arrays are caller memory): monotone pointers ending at nnz, indices inside the minor axis,
    // ascending inside every major slice (the CSR expansion bisects its rows)
    auto at = [&](const void* a, int64_t i) -> int64_t {
        return index_bytes == 4 ? (int64_t) static_cast<const int32_t*>(a)[i] : static_cast<const int64_t*>(a)[i];
    };
    SQGR_REQUIRE(at(indptr, 0) == 0 && at(indptr, nptr - 1) == nnz, "indptr must run from 0 to nnz=%lld", (long long)nnz);
    for (int64_t j = 0; j + 1 < nptr; ++j)
        SQGR_REQUIRE(at(indptr, j) <= at(indptr, j + 1) && at(indptr, j + 1) <= nnz, "indptr is not monotone at %lld", (long long)j);
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    sqgr_matrix* m = new sqgr_matrix();
    m->ctx = ctx;
    m->n_rows = n_rows;
    m->n_cols = n_cols;
    m->ld = n_cols;
    m->kind = kind;
    m->f32 = value_bytes == 4;
    m->nnz = nnz;
    auto fail = [&](int code) {
        delete m;
        return code;
    };
    int rc = SQGR_OK;
    const size_t cnt = (size_t)std::max<int64_t>(nnz, 1);
    if ((rc = m->indptr.alloc((size_t)nptr)) || (rc = m->indices.alloc_pooled(cnt)) || (rc = m->f32 ? m->data32.alloc_pooled(cnt) : m->data.alloc_pooled(cnt))) return fail(rc);
    hipError_t e = hipSuccess;
    if (index_bytes == 8) {
        DevBuf<int64_t> wide;
        if ((rc = wide.alloc(cnt))) return fail(rc);
        e = hipMemcpyAsync(m->indptr.p, indptr, (size_t)nptr * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(wide.p, indices, (size_t)nnz * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && nnz > 0) k_narrow_indices<<<(unsigned)ceil_div(nnz, 256), 256, 0, st>>>(wide.p, nnz, m->indices.p);
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // `wide` is released on return
    } else {
        DevBuf<int32_t> narrow;
        if ((rc = narrow.alloc((size_t)nptr))) return fail(rc);
        e = hipMemcpyAsync(narrow.p, indptr, (size_t)nptr * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) k_widen_indptr<<<(unsigned)ceil_div(nptr, 256), 256, 0, st>>>(narrow.p, nptr, m->indptr.p);
        if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(m->indices.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(m->f32 ? (void*)m->data32.p : (void*)m->data.p, values, (size_t)nnz * value_bytes, hipMemcpyHostToDevice, st);
    // the indices are checked where they now are: inside the minor axis, ascending inside every slice
    DevBuf<int> flags;
    int hflags[3] = {0, 0, 0};
    if (e == hipSuccess && (rc = flags.alloc(3))) return fail(rc);
    if (e == hipSuccess) e = hipMemsetAsync(flags.p, 0, 12, st);
    if (e == hipSuccess && nnz > 0) k_check_sparse<<<(unsigned)ceil_div(nptr - 1, 4), 256, 0, st>>>(m->indptr.p, m->indices.p, nptr - 1, minor, flags.p);
    if (e == hipSuccess) e = hipMemcpyAsync(hflags, flags.p, 12, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("sparse matrix upload failed: %s", hipGetErrorString(e));
        return fail(SQGR_ERR_HIP);
    }
    if (hflags[0] || hflags[1] || hflags[2]) {
        // (repeated indices: scipy's `toarray()` sums them in the matrix dtype, which a float64 accumulation would not reproduce
        //  for float32 values — the caller sums them first)
        set_error(hflags[0] ? "sparse matrix: an index lies outside [0,%lld)"
                            : (hflags[1] ? "sparse matrix: indices are not sorted inside a row/column (call .sort_indices())"
                                         : "sparse matrix: duplicate entries (call .sum_duplicates())"),
                  (long long)minor);
        return fail(SQGR_ERR_INVALID);
    }
    *out = m;
    return SQGR_OK;
}

int sqgr_matrix_create_csr(sqgr_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, const void* indices,
                           int32_t index_bytes, const void* values, int32_t value_bytes, sqgr_matrix** out) {
    return matrix_create_sparse(ctx, 1, n_rows, n_cols, nnz, indptr, indices, index_bytes, values, value_bytes, out);
}

int sqgr_matrix_create_csc(sqgr_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr, const void* indices,
                           int32_t index_bytes, const void* values, int32_t value_bytes, sqgr_matrix** out) {
    return matrix_create_sparse(ctx, 2, n_rows, n_cols, nnz, indptr, indices, index_bytes, values, value_bytes, out);
}

int sqgr_matrix_destroy(sqgr_matrix* m) {
    if (!m) return SQGR_OK;
    (void)hipSetDevice(m->ctx->device);
    if (m->cols_pending > 0) streaming_upload_end();  // a streaming session that was never completed
    delete m;
    return SQGR_OK;
}

}  // extern "C"
