#pragma once
// The expression matrix resident on the device (sqgr_matrix_create*, sqgr_matrix.hip) and the expansions of its columns into a
// gene-major float64 block that its consumers share (spatial_autocorr's feature blocks, sepal's gene batches, niche, PCA).
#include "sqgr_common.h"

// The expression matrix resident on the device (uploaded once per call): dense row-major float64 / float32, or scipy's
// CSR / CSC arrays as they are (int64 indptr, int32 indices; values float32 or float64).
struct sqgr_matrix {
    sqgr_ctx* ctx = nullptr;
    int64_t n_rows = 0, n_cols = 0, ld = 0;
    int kind = 0;        // 0 dense, 1 CSR (rows = cells), 2 CSC (columns = features)
    bool f32 = false;    // values are float32
    sqgr::DevBuf<double> data;
    sqgr::DevBuf<float> data32;
    sqgr::DevBuf<int64_t> indptr;
    sqgr::DevBuf<int32_t> indices;
    int64_t nnz = 0;
    // CSR matrices: the same entries by column, built on the device the first time a column LIST is asked for (ensure_by_column)
    int64_t cols_pending = -1;  // sqgr_matrix_alloc_dense: columns still to be uploaded (a streaming session is open while > 0)
    mutable bool by_col_ready = false;
    mutable sqgr::DevBuf<int64_t> c_indptr;
    mutable sqgr::DevBuf<int32_t> c_rows;
    mutable sqgr::DevBuf<double> c_data;
    mutable sqgr::DevBuf<float> c_data32;
    int ensure_by_column() const;
};

namespace sqgr {
constexpr int MATRIX_TILE = 64;  // the dense expansions transpose tiles of 64 cells x 64 columns through LDS
// X[g * n_rows + i] = (double) m[i, dev_cols[g]] for g < gc: dev_cols is a device array; a CSR matrix needs its by-column twin
// (m->ensure_by_column()) first.  Enqueued on `st`.
hipError_t expand_column_list(const sqgr_matrix* m, const int32_t* dev_cols, int gc, double* X, hipStream_t st);
// The same for the contiguous columns [col0 + g0, col0 + g0 + gc) of any kind of matrix (no twin needed).
hipError_t expand_column_range(const sqgr_matrix* m, int64_t col0, int64_t g0, int gc, double* X, hipStream_t st);
// ... and of a dense float64 cell-major device array D[n][ld] that is not a sqgr_matrix: X[g * n + i] = D[i * ld + g0 + g].
hipError_t expand_dense_f64(const double* D, int64_t ld, int64_t n, int64_t g0, int gc, double* X, hipStream_t st);
}  // namespace sqgr
