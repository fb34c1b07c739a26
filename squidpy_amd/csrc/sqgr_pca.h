#pragma once
// The feature matrix of a PCA resident on the device (sqgr_pca_create, sqgr_pca.hip).  sqgr_niche.hip writes aggregated blocks into
// it (sqgr_pca_fill_aggregate): the two translation units share this layout and nothing else.
#include "sqgr_common.h"

struct sqgr_pca {
    sqgr_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t D = 0;
    sqgr::DevBuf<double> F;     // [n][D] row-major
    sqgr::DevBuf<double> mean;  // [D], valid while have_mean
    bool have_mean = false;     // sqgr_pca_moments has run since the last write into F
};
