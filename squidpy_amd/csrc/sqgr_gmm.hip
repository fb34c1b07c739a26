// libsqgr: calculate_niche_cellcharter — a full-covariance Gaussian mixture fitted by EM in float64 (gr/_niche.py).
//
// Reference semantics (squidpy, src/squidpy/gr/_niche.py):
//   :1474-1480  GaussianMixture(n_components, random_state, init_params="random_from_data").fit(embedding).predict(embedding)
// and behind it scikit-learn 1.7's sklearn/mixture/_base.py (fit_predict's loop) and _gaussian_mixture.py, step for step:
//   init    resp[init_rows[c]][c] = 1, everything else 0 (the HOST draws init_rows); parameters from these responsibilities
//   M-step  nk = sum r + 10 eps;  mean = sum r x / nk;  cov = sum r (x - mean)(x - mean)^T / nk + reg_covar I   (centred, two passes)
//           weights = nk / n at the initialisation, nk / sum nk afterwards;  P = L^-T of cov = L L^T  (upper triangular)
//   E-step  y = (x - mean) P;  wlp_c = -(d log 2pi + sum y^2) / 2 + sum log diag P + log w_c;  lpn = logsumexp_c wlp (maximum subtracted)
//           resp = exp(wlp - lpn);  lower bound = mean of lpn
//   loop    at most max_iter steps of E then M; converged when |lb - lb_prev| < tol, the parameters of that step are kept
//   labels  argmax_c wlp_c under the final parameters, the first maximum wins
//
// Every sum over rows has ONE order, a function of (n, d, k) alone: no float atomics, no dependence on the device's CU count, so two
// calls return the same bytes.  The project compiles with -ffp-contract=off: each product and each sum below is rounded on its own.
//
// k_gmm_estep   rows across lanes.  A block stages 64 rows of X transposed in LDS; mean and P of the component are the same for
//               every lane (scalar loads), y is formed in strips of 16 columns of P that live in registers, rows of P below the strip
//               are skipped (P is upper triangular).  Each lane writes its row's wlp to resp, reads them back for the logsumexp and
//               overwrites them with the responsibilities; lpn is summed per lane over the block's tiles in row order, then by a
//               fixed tree over the block; k_gmm_lb adds the block partials in block order.
// k_gmm_sums    out[c][i] = sum_rows resp[row][c] x[row][i] and nk: a weighted A^T B with 4 x 4 output tiles in registers.  A block
//               takes a chunk of rows, stages sub-tiles of resp and X in LDS, and splits the rows of a sub-tile over thread groups
//               (group g takes rows g, g + G, ...); groups are added in group order through LDS, chunks in chunk order by the
//               finishing kernel.
// k_gmm_cov     the same shape for one component per block: A = r (x - mean), B = x - mean, upper-triangular tiles only.
// k_gmm_cov_finish  one workgroup per component: adds the chunk partials, divides, adds reg_covar, factorises in LDS (right-looking
//               Cholesky), inverts the factor by forward substitution (one thread per column) and writes P and its log determinant.
//               A pivot that is not positive raises the status flag the host reads with the lower bound: one 16-byte copy per step.
#include "sqgr_common.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <vector>

namespace sqgr {
namespace {

constexpr int GMM_MAX = 64;          // d and k
constexpr int E_T = 64;              // rows of an E-step tile = threads of its block
constexpr int E_JT = 16;             // columns of P per strip (accumulators per lane)
constexpr int E_MAX_BLOCKS = 4096;   // partial sums of the lower bound
constexpr int M_T = 256;
constexpr int M_MAX_BLOCKS = 2048;   // chunks x components of the M-step grids
constexpr int M_MIN_ROWS = 512;      // rows of a chunk at least
constexpr int M_SUMS_BLOCKS = 512;   // chunks of k_gmm_sums, which takes every component in one block
constexpr int M_RED = 20;            // values a thread hands to the group reduction: 16 tile entries + 4 row sums of A
constexpr size_t M_STAGE_BYTES = 48 * 1024;

__global__ __launch_bounds__(GMM_MAX) void k_gmm_init_resp(const int64_t* __restrict__ init_rows, int k, int64_t n, double* __restrict__ resp) {
    const int c = threadIdx.x;
    if (c < k) resp[(int64_t)c * n + init_rows[c]] = 1.0;
}

template <bool PREDICT>
__global__ __launch_bounds__(E_T) void k_gmm_estep(const double* __restrict__ X, int64_t n, int d, int k, int dp, const double* __restrict__ mu,
                                                   const double* __restrict__ P, const double* __restrict__ logdet,
                                                   const double* __restrict__ logw, double dlog2pi, int64_t tiles_per_block,
                                                   double* __restrict__ resp, double* __restrict__ lpn_part, int32_t* __restrict__ labels) {
    extern __shared__ double gmm_lds[];  // xs[d][E_T]
    __shared__ double red[E_T];
    double* xs = gmm_lds;
    const int t = threadIdx.x;
    const int64_t ntiles = (n + E_T - 1) / E_T;
    const int64_t tile0 = blockIdx.x * tiles_per_block, tile1 = min(ntiles, tile0 + tiles_per_block);
    double lsum = 0.0;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t row0 = tile * E_T;
        const int rows = (int)min((int64_t)E_T, n - row0);
        __syncthreads();  // the previous tile's readers are done
        for (int idx = t; idx < rows * d; idx += E_T) {
            const int r = idx / d, i = idx - r * d;
            xs[i * E_T + r] = X[row0 * d + idx];
        }
        if (t >= rows)
            for (int i = 0; i < d; ++i) xs[i * E_T + t] = 0.0;  // lanes without a row compute on zeros and store nothing
        __syncthreads();
        const bool valid = t < rows;
        const int64_t row = row0 + t;
        double best = -INFINITY;
        int bestc = 0;
        for (int c = 0; c < k; ++c) {
            const double* __restrict__ Pc = P + (size_t)c * d * dp;
            const double* __restrict__ muc = mu + (size_t)c * d;
            double s = 0.0;
            for (int jt = 0; jt < d; jt += E_JT) {
                double y[E_JT];
#pragma unroll
                for (int jj = 0; jj < E_JT; ++jj) y[jj] = 0.0;
                const int iend = min(d, jt + E_JT);  // P[i][j] = 0 for i > j
                // the strip's row of P for the NEXT i is fetched (scalar loads) while this one is used, and the 16 products are formed
                // before the 16 sums: one or two waves per SIMD have nothing else to cover a load or a dependent pair with
                double pn[E_JT], mn = muc[0];
#pragma unroll
                for (int jj = 0; jj < E_JT; ++jj) pn[jj] = Pc[jt + jj];  // columns past d are stored zeros
                for (int i = 0; i < iend; ++i) {
                    double pr[E_JT], prod[E_JT];
#pragma unroll
                    for (int jj = 0; jj < E_JT; ++jj) pr[jj] = pn[jj];
                    const double diff = xs[i * E_T + t] - mn;
                    const int inext = min(i + 1, iend - 1);
                    mn = muc[inext];
#pragma unroll
                    for (int jj = 0; jj < E_JT; ++jj) pn[jj] = Pc[(size_t)inext * dp + jt + jj];
#pragma unroll
                    for (int jj = 0; jj < E_JT; ++jj) prod[jj] = diff * pr[jj];
#pragma unroll
                    for (int jj = 0; jj < E_JT; ++jj) y[jj] += prod[jj];
                }
#pragma unroll
                for (int jj = 0; jj < E_JT; ++jj) s += y[jj] * y[jj];
            }
            const double w = ((-0.5 * (dlog2pi + s)) + logdet[c]) + logw[c];
            if (PREDICT) {
                if (w > best) {  // the first maximum wins
                    best = w;
                    bestc = c;
                }
            } else {
                if (valid) resp[(int64_t)c * n + row] = w;
                best = fmax(best, w);
            }
        }
        if (PREDICT) {
            if (valid) labels[row] = bestc;
        } else if (valid) {
            double sum = 0.0;
            for (int c = 0; c < k; ++c) sum += exp(resp[(int64_t)c * n + row] - best);
            const double lpn = log(sum) + best;
            for (int c = 0; c < k; ++c) {
                const int64_t at = (int64_t)c * n + row;
                resp[at] = exp(resp[at] - lpn);
            }
            lsum += lpn;
        }
    }
    if (!PREDICT) {
        red[t] = lsum;
        __syncthreads();
        for (int s = E_T / 2; s >= 1; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        if (t == 0) lpn_part[blockIdx.x] = red[0];
    }
}

// status[0] = (sum of the block partials in block order) / n
__global__ __launch_bounds__(E_T) void k_gmm_lb(const double* __restrict__ part, int nblocks, int64_t n, double* __restrict__ status) {
    __shared__ double red[E_T];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int b = t; b < nblocks; b += E_T) s += part[b];
    red[t] = s;
    __syncthreads();
    for (int o = E_T / 2; o >= 1; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) status[0] = red[0] / (double)n;
}

// The rows of one staged sub-tile that belong to this thread's group, into its 4 x 4 tile: acc[p][q] += A[r][a0 + p] * B[r][b0 + q].
__device__ __forceinline__ void gmm_tile_rows(const double* __restrict__ A, int pa, int a0, const double* __restrict__ B, int pb, int b0,
                                              int g, int G, int rows, bool row_sums, double (&acc)[16], double (&accn)[4]) {
    for (int r = g; r < rows; r += G) {
        double a[4], b[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            a[p] = A[r * pa + a0 + p];
            b[p] = B[r * pb + b0 + p];
        }
        double prod[16];  // the 16 products before the 16 sums: no dependent pair back to back
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) prod[p * 4 + q] = a[p] * b[q];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] += prod[e];
        if (row_sums) {
#pragma unroll
            for (int p = 0; p < 4; ++p) accn[p] += a[p];
        }
    }
}

// Groups in group order: red[(g * ntile + tile) * M_RED + e]; afterwards value e of tile `tile` is the return of gmm_group_sum.
__device__ __forceinline__ void gmm_hand_over(double* red, int g, int tile, int ntile, bool active, const double (&acc)[16], const double (&accn)[4]) {
    __syncthreads();  // the staging area is reused
    if (active) {
        double* o = red + ((size_t)g * ntile + tile) * M_RED;
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = acc[e];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[16 + e] = accn[e];
    }
    __syncthreads();
}

__device__ __forceinline__ double gmm_group_sum(const double* red, int tile, int e, int ntile, int G) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += red[((size_t)g * ntile + tile) * M_RED + e];
    return s;
}

// out[chunk][c][i] = sum over the chunk's rows of resp[c][row] * X[row][i] (i < d);  out[chunk][c][d] = sum of resp[c][row]
__global__ __launch_bounds__(M_T) void k_gmm_sums(const double* __restrict__ X, int64_t n, int d, int k, const double* __restrict__ resp,
                                                  int64_t rows_per_chunk, int RT, double* __restrict__ out) {
    extern __shared__ double gmm_lds[];
    const int t = threadIdx.x;
    const int ka = (k + 3) & ~3, db = (d + 3) & ~3;
    double* A = gmm_lds;             // [RT][ka]
    double* B = gmm_lds + RT * ka;   // [RT][db]
    const int nbt = db / 4, ntile = (ka / 4) * nbt, G = M_T / ntile;
    const int tile = t % ntile, g = t / ntile;
    const bool active = g < G;
    const int at = tile / nbt, bt = tile - at * nbt;
    double acc[16], accn[4];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) accn[e] = 0.0;
    const int64_t row_begin = blockIdx.x * rows_per_chunk, row_end = min(n, row_begin + rows_per_chunk);
    for (int64_t r0 = row_begin; r0 < row_end; r0 += RT) {
        const int rows = (int)min((int64_t)RT, row_end - r0);
        __syncthreads();
        for (int idx = t; idx < RT * ka; idx += M_T) {
            const int c = idx / RT, r = idx - c * RT;
            A[r * ka + c] = (c < k && r < rows) ? resp[(int64_t)c * n + r0 + r] : 0.0;
        }
        for (int idx = t; idx < RT * db; idx += M_T) {
            const int r = idx / db, i = idx - r * db;
            B[idx] = (i < d && r < rows) ? X[(r0 + r) * d + i] : 0.0;
        }
        __syncthreads();
        if (active) gmm_tile_rows(A, ka, 4 * at, B, db, 4 * bt, g, G, rows, bt == 0, acc, accn);
    }
    gmm_hand_over(gmm_lds, g, tile, ntile, active, acc, accn);
    double* o = out + (size_t)blockIdx.x * k * (d + 1);
    for (int idx = t; idx < ntile * M_RED; idx += M_T) {
        const int tl = idx / M_RED, e = idx - tl * M_RED;
        const int a_t = tl / nbt, b_t = tl - a_t * nbt;
        if (e < 16) {
            const int c = 4 * a_t + e / 4, i = 4 * b_t + (e & 3);
            if (c < k && i < d) o[(size_t)c * (d + 1) + i] = gmm_group_sum(gmm_lds, tl, e, ntile, G);
        } else if (b_t == 0) {
            const int c = 4 * a_t + (e - 16);
            if (c < k) o[(size_t)c * (d + 1) + d] = gmm_group_sum(gmm_lds, tl, e, ntile, G);
        }
    }
}

// one block per component: chunks in chunk order; nk = sum + 10 eps; mean = sum / nk
__global__ __launch_bounds__(GMM_MAX + 64) void k_gmm_means(const double* __restrict__ part, int nchunks, int d, int k, double* __restrict__ means,
                                                            double* __restrict__ nk) {
    __shared__ double val[GMM_MAX + 1];
    const int c = blockIdx.x, i = threadIdx.x;
    if (i <= d) {
        double s = 0.0;
        for (int b = 0; b < nchunks; ++b) s += part[((size_t)b * k + c) * (d + 1) + i];
        val[i] = s;
    }
    __syncthreads();
    const double nkc = val[d] + 10.0 * DBL_EPSILON;
    if (i < d) means[(size_t)c * d + i] = val[i] / nkc;
    if (i == 0) nk[c] = nkc;
}

// weights = nk / total (total = n at the initialisation, the sum of nk in component order afterwards) and their logarithms
__global__ __launch_bounds__(GMM_MAX) void k_gmm_weights(const double* __restrict__ nk, int k, double n_or_zero, double* __restrict__ weights,
                                                         double* __restrict__ logw) {
    __shared__ double total;
    if (threadIdx.x == 0) {
        double s = n_or_zero;
        if (s == 0.0)
            for (int c = 0; c < k; ++c) s += nk[c];
        total = s;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < k) {
        const double w = nk[c] / total;
        weights[c] = w;
        logw[c] = log(w);
    }
}

// grid (chunks, components): out[chunk][c][i][j] = sum over the chunk's rows of (r (x_i - mu_i)) * (x_j - mu_j), tiles with i-tile <= j-tile
__global__ __launch_bounds__(M_T) void k_gmm_cov(const double* __restrict__ X, int64_t n, int d, int k, const double* __restrict__ resp,
                                                 const double* __restrict__ means, int64_t rows_per_chunk, int RT, double* __restrict__ out) {
    extern __shared__ double gmm_lds[];
    const int t = threadIdx.x, c = blockIdx.y;
    const int db = (d + 3) & ~3;
    double* A = gmm_lds;            // [RT][db]  r * diff
    double* B = gmm_lds + RT * db;  // [RT][db]  diff
    const int nbt = db / 4, ntile = nbt * (nbt + 1) / 2, G = M_T / ntile;
    const int tile = t % ntile, g = t / ntile;
    const bool active = g < G;
    int at = 0, rem = tile;
    while (rem >= nbt - at) {
        rem -= nbt - at;
        ++at;
    }
    const int bt = at + rem;
    const double* __restrict__ muc = means + (size_t)c * d;
    const double* __restrict__ rc = resp + (int64_t)c * n;
    double acc[16], accn[4];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) accn[e] = 0.0;
    const int64_t row_begin = blockIdx.x * rows_per_chunk, row_end = min(n, row_begin + rows_per_chunk);
    for (int64_t r0 = row_begin; r0 < row_end; r0 += RT) {
        const int rows = (int)min((int64_t)RT, row_end - r0);
        __syncthreads();
        for (int idx = t; idx < RT * db; idx += M_T) {
            const int r = idx / db, i = idx - r * db;
            double diff = 0.0, wd = 0.0;
            if (i < d && r < rows) {
                diff = X[(r0 + r) * d + i] - muc[i];
                wd = rc[r0 + r] * diff;
            }
            A[idx] = wd;
            B[idx] = diff;
        }
        __syncthreads();
        if (active) gmm_tile_rows(A, db, 4 * at, B, db, 4 * bt, g, G, rows, false, acc, accn);
    }
    gmm_hand_over(gmm_lds, g, tile, ntile, active, acc, accn);
    double* o = out + ((size_t)blockIdx.x * k + c) * d * d;
    for (int idx = t; idx < ntile * 16; idx += M_T) {
        const int tl = idx >> 4, e = idx & 15;
        int a_t = 0, rm = tl;
        while (rm >= nbt - a_t) {
            rm -= nbt - a_t;
            ++a_t;
        }
        const int i = 4 * a_t + (e >> 2), j = 4 * (a_t + rm) + (e & 3);
        if (i < d && j < d) o[(size_t)i * d + j] = gmm_group_sum(gmm_lds, tl, e, ntile, G);
    }
}

// one workgroup per component: covariance from the chunk partials, its Cholesky factor, P = L^-T and log det P.  status[1] = 1 when a
// pivot is not positive (the component's P is then left as it was).
__global__ __launch_bounds__(M_T) void k_gmm_cov_finish(const double* __restrict__ part, int nchunks, int d, int k, int dp, const double* __restrict__ nk,
                                                        double reg_covar, double* __restrict__ cov, double* __restrict__ P,
                                                        double* __restrict__ logdet, double* __restrict__ status) {
    __shared__ double As[GMM_MAX][GMM_MAX + 1];
    __shared__ double zd[GMM_MAX];
    const int t = threadIdx.x, c = blockIdx.x;
    const double nkc = nk[c];
    for (int idx = t; idx < d * d; idx += M_T) {
        const int i = idx / d, j = idx - i * d;
        if (i > j) continue;
        double s = 0.0;
        for (int b = 0; b < nchunks; ++b) s += part[(((size_t)b * k + c) * d + i) * d + j];
        s = s / nkc;
        if (i == j) s += reg_covar;
        As[i][j] = s;
        As[j][i] = s;
        cov[((size_t)c * d + i) * d + j] = s;
        cov[((size_t)c * d + j) * d + i] = s;
    }
    // right-looking Cholesky on the lower triangle
    bool bad = false;
    for (int j = 0; j < d; ++j) {
        __syncthreads();
        const double piv = As[j][j];
        if (!(piv > 0.0)) {  // the same value in every thread
            bad = true;
            break;
        }
        const double ljj = sqrt(piv);
        __syncthreads();
        if (t == 0) As[j][j] = ljj;
        for (int i = j + 1 + t; i < d; i += M_T) As[i][j] = As[i][j] / ljj;
        __syncthreads();
        const int cnt = d - j - 1;
        for (int e = t; e < cnt * cnt; e += M_T) {
            const int i = j + 1 + e / cnt, m = j + 1 + e % cnt;
            if (m <= i) As[i][m] -= As[i][j] * As[m][j];
        }
    }
    if (bad) {
        if (t == 0) status[1] = 1.0;
        return;
    }
    __syncthreads();
    // Z = L^-1 by forward substitution, thread m owns column m: z_i = ((i == m) - sum_{q = m}^{i - 1} L[i][q] z_q) / L[i][i].
    // P[m][i] = Z[i][m]: kept in the row m of the (now free) upper triangle, the diagonal in zd.
    if (t < d) {
        const int m = t;
        const double zm = 1.0 / As[m][m];
        for (int i = m + 1; i < d; ++i) {
            double s = As[i][m] * zm;
            for (int q = m + 1; q < i; ++q) s += As[i][q] * As[m][q];
            As[m][i] = (0.0 - s) / As[i][i];
        }
        zd[m] = zm;
    }
    __syncthreads();
    double* Pc = P + (size_t)c * d * dp;
    for (int idx = t; idx < d * dp; idx += M_T) {
        const int a = idx / dp, b = idx - a * dp;
        Pc[idx] = (b < a || b >= d) ? 0.0 : (b == a ? zd[a] : As[a][b]);
    }
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s += log(zd[i]);
        logdet[c] = s;
    }
}

struct GmmGeometry {
    int dp = 0;
    int64_t e_tiles_per_block = 0;
    int e_blocks = 0;
    int64_t rows_per_chunk = 0, sums_rows_per_chunk = 0;  // of k_gmm_cov (grid chunks x components) and of k_gmm_sums
    int nchunks = 0, sums_nchunks = 0, rt_sums = 0, rt_cov = 0;
    size_t lds_e = 0, lds_sums = 0, lds_cov = 0;
};

int rows_per_stage(int pitch_doubles) {
    int rt = (int)(M_STAGE_BYTES / ((size_t)pitch_doubles * 8));
    rt = std::min(256, rt / 32 * 32);
    return std::max(rt, 32);
}

// a function of (n, d, k) alone: the order of every sum follows from it
GmmGeometry gmm_geometry(int64_t n, int d, int k) {
    GmmGeometry q;
    q.dp = (d + E_JT - 1) / E_JT * E_JT;
    const int64_t ntiles = ceil_div(n, E_T);
    q.e_tiles_per_block = ceil_div(ntiles, E_MAX_BLOCKS);
    q.e_blocks = (int)ceil_div(ntiles, q.e_tiles_per_block);
    const int64_t max_chunks = std::max(1, M_MAX_BLOCKS / k);
    const int64_t chunks = std::min<int64_t>(std::max<int64_t>(1, n / M_MIN_ROWS), max_chunks);
    q.rows_per_chunk = ceil_div(n, chunks);
    q.nchunks = (int)ceil_div(n, q.rows_per_chunk);
    const int64_t sums_chunks = std::min<int64_t>(std::max<int64_t>(1, n / M_MIN_ROWS), M_SUMS_BLOCKS);
    q.sums_rows_per_chunk = ceil_div(n, sums_chunks);
    q.sums_nchunks = (int)ceil_div(n, q.sums_rows_per_chunk);
    const int ka = (k + 3) & ~3, db = (d + 3) & ~3;
    q.rt_sums = rows_per_stage(ka + db);
    q.rt_cov = rows_per_stage(2 * db);
    const size_t red = (size_t)M_T * M_RED * 8;
    q.lds_e = (size_t)d * E_T * 8;
    q.lds_sums = std::max((size_t)q.rt_sums * (ka + db) * 8, red);
    q.lds_cov = std::max((size_t)q.rt_cov * 2 * db * 8, red);
    return q;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_gmm_geometry(int64_t n, int32_t d, int32_t k, int64_t* out) {
    SQGR_REQUIRE(out, "null argument");
    SQGR_REQUIRE(n >= 1 && d >= 1 && d <= GMM_MAX && k >= 1 && k <= GMM_MAX && n <= (int64_t)INT32_MAX, "sqgr_gmm_geometry: n=%lld d=%d k=%d",
                 (long long)n, d, k);
    const GmmGeometry q = gmm_geometry(n, d, k);
    const int64_t v[20] = {q.dp, q.e_tiles_per_block, q.e_blocks, q.rows_per_chunk, q.sums_rows_per_chunk, q.nchunks, q.sums_nchunks, q.rt_sums,
                           q.rt_cov, (int64_t)q.lds_e, (int64_t)q.lds_sums, (int64_t)q.lds_cov, E_T, E_MAX_BLOCKS, M_MAX_BLOCKS, M_MIN_ROWS,
                           M_SUMS_BLOCKS, E_JT, (int64_t)M_STAGE_BYTES, (int64_t)M_T * M_RED * 8};
    std::copy(v, v + 20, out);
    return SQGR_OK;
}

int sqgr_gmm_fit(sqgr_ctx* ctx, const double* X, int64_t n, int32_t d, int32_t k, const int64_t* init_rows, double reg_covar, double tol,
                 int32_t max_iter, double* out_weights, double* out_means, double* out_covariances, double* out_lower_bounds,
                 int32_t* out_n_iter, int32_t* out_converged, int32_t* out_labels) {
    SQGR_REQUIRE(ctx && X && init_rows && out_weights && out_means && out_covariances && out_lower_bounds && out_n_iter && out_converged && out_labels,
                 "null argument");
    SQGR_REQUIRE(n >= 1 && d >= 1 && k >= 1, "sqgr_gmm_fit: n=%lld d=%d k=%d", (long long)n, d, k);
    if (d > GMM_MAX || k > GMM_MAX || n > (int64_t)INT32_MAX) {
        set_error("sqgr_gmm_fit: supported are at most %d features, %d components and %d rows; found d=%d k=%d n=%lld", GMM_MAX, GMM_MAX, INT32_MAX,
                  d, k, (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_REQUIRE(k <= n, "sqgr_gmm_fit: k=%d components need at least as many rows, found n=%lld", k, (long long)n);
    SQGR_REQUIRE(max_iter >= 1, "sqgr_gmm_fit: max_iter=%d", max_iter);
    SQGR_REQUIRE(reg_covar >= 0.0 && tol >= 0.0, "sqgr_gmm_fit: reg_covar=%g tol=%g", reg_covar, tol);
    for (int32_t c = 0; c < k; ++c)
        SQGR_REQUIRE(init_rows[c] >= 0 && init_rows[c] < n, "sqgr_gmm_fit: init_rows[%d]=%lld outside [0,%lld)", c, (long long)init_rows[c], (long long)n);
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const GmmGeometry q = gmm_geometry(n, d, k);

    // every buffer of the call, before the first step
    DevBuf<double> dX, resp, lpn_part, sums_part, cov_part, small;
    DevBuf<int64_t> d_init;
    DevBuf<int32_t> d_labels;
    const size_t kd = (size_t)k * d, kdd = kd * d, kddp = kd * q.dp;
    SQGR_TRY(dX.alloc_pooled((size_t)n * d));
    SQGR_TRY(resp.alloc_pooled((size_t)n * k));
    SQGR_TRY(lpn_part.alloc((size_t)q.e_blocks));
    SQGR_TRY(sums_part.alloc_pooled((size_t)q.sums_nchunks * k * (d + 1)));
    SQGR_TRY(cov_part.alloc_pooled((size_t)q.nchunks * kdd));
    // means[k d] | cov[k d d] | P[k d dp] | nk[k] | weights[k] | logw[k] | logdet[k] | status[2]
    SQGR_TRY(small.alloc(kd + kdd + kddp + 4 * (size_t)k + 2));
    SQGR_TRY(d_init.alloc((size_t)k));
    SQGR_TRY(d_labels.alloc((size_t)n));
    double* means = small.p;
    double* cov = means + kd;
    double* P = cov + kdd;
    double* nk = P + kddp;
    double* weights = nk + k;
    double* logw = weights + k;
    double* logdet = logw + k;
    double* status = logdet + k;
    SQGR_TRY(allow_lds(k_gmm_sums, q.lds_sums));
    SQGR_TRY(allow_lds(k_gmm_cov, q.lds_cov));

    SQGR_HIP(hipMemcpyAsync(dX.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(d_init.p, init_rows, (size_t)k * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemsetAsync(resp.p, 0, (size_t)n * k * 8, st));
    SQGR_HIP(hipMemsetAsync(small.p, 0, small.bytes(), st));
    {
        LaunchTimer t(ctx, "gmm_init");
        k_gmm_init_resp<<<1, GMM_MAX, 0, st>>>(d_init.p, k, n, resp.p);
        SQGR_HIP(hipGetLastError());
    }

    auto m_step = [&](bool init) -> int {
        {
            LaunchTimer t(ctx, "gmm_sums");
            k_gmm_sums<<<q.sums_nchunks, M_T, q.lds_sums, st>>>(dX.p, n, d, k, resp.p, q.sums_rows_per_chunk, q.rt_sums, sums_part.p);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "gmm_means");
            k_gmm_means<<<k, GMM_MAX + 64, 0, st>>>(sums_part.p, q.sums_nchunks, d, k, means, nk);
            SQGR_HIP(hipGetLastError());
            k_gmm_weights<<<1, GMM_MAX, 0, st>>>(nk, k, init ? (double)n : 0.0, weights, logw);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "gmm_cov");
            k_gmm_cov<<<dim3(q.nchunks, k), M_T, q.lds_cov, st>>>(dX.p, n, d, k, resp.p, means, q.rows_per_chunk, q.rt_cov, cov_part.p);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "gmm_cholesky");
            k_gmm_cov_finish<<<k, M_T, 0, st>>>(cov_part.p, q.nchunks, d, k, q.dp, nk, reg_covar, cov, P, logdet, status);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    };
    const char* ill = "sqgr_gmm_fit: ill-defined empirical covariance (a Cholesky pivot is not positive)";
    const double dlog2pi = (double)d * std::log(2.0 * M_PI);

    SQGR_TRY(m_step(true));
    double lb = -std::numeric_limits<double>::infinity();
    int32_t n_iter = 0, converged = 0;
    for (int32_t it = 1; it <= max_iter; ++it) {
        const double prev = lb;
        {
            LaunchTimer t(ctx, "gmm_estep");
            k_gmm_estep<false><<<q.e_blocks, E_T, q.lds_e, st>>>(dX.p, n, d, k, q.dp, means, P, logdet, logw, dlog2pi, q.e_tiles_per_block,
                                                               resp.p, lpn_part.p, nullptr);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "gmm_lower_bound");
            k_gmm_lb<<<1, E_T, 0, st>>>(lpn_part.p, q.e_blocks, n, status);
            SQGR_HIP(hipGetLastError());
        }
        SQGR_TRY(m_step(false));
        double h[2] = {0.0, 1.0};  // the step's one read-back: the lower bound and the pivot flag (of this step's and the initial factorisations)
        SQGR_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        SQGR_REQUIRE(h[1] == 0.0, "%s", ill);
        lb = h[0];
        out_lower_bounds[it - 1] = lb;
        n_iter = it;
        if (std::fabs(lb - prev) < tol) {
            converged = 1;
            break;
        }
    }
    {
        LaunchTimer t(ctx, "gmm_predict");
        k_gmm_estep<true><<<q.e_blocks, E_T, q.lds_e, st>>>(dX.p, n, d, k, q.dp, means, P, logdet, logw, dlog2pi, q.e_tiles_per_block, nullptr,
                                                          nullptr, d_labels.p);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out_weights, weights, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_means, means, kd * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_covariances, cov, kdd * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(out_labels, d_labels.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    *out_n_iter = n_iter;
    *out_converged = converged;
    return SQGR_OK;
}
