// libsqgr: niche feature matrices — stage 1 of the reference's three niche flavours (gr/_niche.py), everything in front of scanpy.
//
// Reference semantics (squidpy, src/squidpy/gr/_niche.py):
//   :1002-1038  _setdiag / _hop / _normalize: the CellCharter hop shells.  With vis_1 = A with its diagonal set to 1 and hop_1 = A
//               without its diagonal (every stored value of A is 1):
//                   P_k   = hop_{k-1} @ A       path sums; a stored entry of hop_{k-1} counts 1, self loops of A take part
//                   hop_k = P_k > vis_{k-1}     elementwise, an absent entry is 0
//                   vis_k = vis_{k-1} + hop_k
//               This is NOT a BFS: a node visited before re-enters shell k whenever more paths reach it than it has been visited.
//   :1041-1054  _aggregate: block k = D_k^-1 hop_k X ("mean"), D_k^-1 hop_k X^2 - (D_k^-1 hop_k X)^2 ("variance"); 1/0 -> 0
//   :1259-1260  UTAG: normalize(A, "l1", axis=1) @ X
//   :1117-1221  neighbourhood profile: hop h = A^h onehot(labels), formed here as A (A^(h-1) onehot) — A^h is never built
//
// Arithmetic: float64 throughout, every sum over a row's stored entries in ascending column order, products and sums rounded
// separately (__dmul_rn / __dadd_rn: no FMA whatever the compiler's contraction setting), variance = m2 - m1 * m1 unfused.  Shell
// structure and path counts are 32-bit integers.  No result depends on launch geometry or on the arrival order of an atomic.
//
// k_shell_row    one wave per row: the row of hop_{k-1} is expanded through A's rows into an LDS hash table (SHELL_SLOTS slots of
//                column / path count, LDS atomics), the row's visit counts are looked up in it, and hop_k / vis_k come out as sorted
//                CSR (rank sort of the few qualifying columns).  Run twice per shell: once to size the rows, once to fill them.
// k_shell_spill  rows whose expansion (sum of the lengths of the A rows they walk) exceeds SHELL_CAPACITY: one block per row on a
//                dense count array of n words in global memory, swept in column order between the smallest and the largest column
//                touched and zeroed again by a second walk.
// k_aggregate    one thread per (row, four columns of the block): Y = diag(s) S X[:, c0:c0+c] on the block that expand_column_list
//                densifies (dense / CSR / CSC, float32 / float64), transposed on the device to row-major: a row's index is read once
//                for four sums, an entry's four values are one 32-byte read, and the result is copied out as it lies.
// k_label_hop    one thread per (row, category): P_h = A P_{h-1} on an n x K panel, P_0 = onehot(labels).
#include "sqgr_matrix.h"
#include "sqgr_pca.h"

#include <algorithm>
#include <vector>

namespace sqgr {
namespace {

constexpr int NICHE_T = 256;
constexpr int SHELL_SLOTS = 1024;    // hash slots of one row's table (a power of two)
constexpr int SHELL_CAPACITY = 512;  // largest expansion a row may have on chip: the table is never more than half full
constexpr int SHELL_WAVE = 64;
constexpr int SPILL_T = 256;
constexpr int SPILL_BLOCKS = 16;     // dense count arrays (n words each) of the global-memory path
constexpr uint32_t COUNT_LIMIT = 1u << 24;  // the reference's float32 path sums stop being exact here
constexpr int AGG_MAX_COLS = 64;     // columns of X per block
constexpr int MAX_DISTANCE = 64;

__device__ __forceinline__ uint32_t slot_of(int32_t key) { return ((uint32_t)key * 2654435761u) >> 22; }  // top 10 bits: SHELL_SLOTS

// flags[0]: a row that is not strictly increasing
__global__ __launch_bounds__(NICHE_T) void k_check_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n,
                                                        int* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= n) return;
    for (int64_t e = indptr[i] + 1; e < indptr[i + 1]; ++e)
        if (indices[e - 1] >= indices[e]) flags[0] = 1;
}

// hop_1 = A without its diagonal, vis_1 = A with its diagonal: row lengths (fill == 0) or entries
template <bool FILL>
__global__ __launch_bounds__(NICHE_T) void k_shell_first(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n,
                                                         int64_t* __restrict__ hop_ptr, int64_t* __restrict__ vis_ptr,
                                                         int32_t* __restrict__ hop_idx, int32_t* __restrict__ vis_idx,
                                                         int32_t* __restrict__ vis_cnt) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= n) return;
    const int64_t a = indptr[i], b = indptr[i + 1];
    if (!FILL) {
        int diag = 0;
        for (int64_t e = a; e < b; ++e) diag |= indices[e] == (int32_t)i;
        hop_ptr[i] = (b - a) - diag;
        vis_ptr[i] = (b - a) + 1 - diag;
        return;
    }
    int64_t h = hop_ptr[i], v = vis_ptr[i];
    bool placed = false;
    for (int64_t e = a; e < b; ++e) {
        const int32_t c = indices[e];
        if (!placed && c >= (int32_t)i) {
            vis_idx[v] = (int32_t)i;
            vis_cnt[v++] = 1;
            placed = true;
        }
        if (c != (int32_t)i) {
            hop_idx[h++] = c;
            vis_idx[v] = c;
            vis_cnt[v++] = 1;
        }
    }
    if (!placed) {
        vis_idx[v] = (int32_t)i;
        vis_cnt[v] = 1;
    }
}

// expansion[i] = sum over j in hop_{k-1}[i] of len(A[j])
__global__ __launch_bounds__(NICHE_T) void k_shell_expansion(const int64_t* __restrict__ a_ptr, const int64_t* __restrict__ h_ptr,
                                                             const int32_t* __restrict__ h_idx, int64_t n, int64_t* __restrict__ expansion) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= n) return;
    int64_t s = 0;
    for (int64_t e = h_ptr[i]; e < h_ptr[i + 1]; ++e) {
        const int32_t j = h_idx[e];
        s += a_ptr[j + 1] - a_ptr[j];
    }
    expansion[i] = s;
}

// position of `key` in the ascending list idx[lo, hi): the first entry >= key
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ idx, int64_t lo, int64_t hi, int32_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One wave per row.  FILL == false: new_hop_len[i] / new_vis_len[i]; FILL == true: the entries behind new_hop_ptr[i] / new_vis_ptr[i].
// flags[1]: a path count reached `limit`.
template <bool FILL>
__global__ __launch_bounds__(SHELL_WAVE) void k_shell_row(const int64_t* __restrict__ a_ptr, const int32_t* __restrict__ a_idx,
                                                          const int64_t* __restrict__ h_ptr, const int32_t* __restrict__ h_idx,
                                                          const int64_t* __restrict__ v_ptr, const int32_t* __restrict__ v_idx,
                                                          const int32_t* __restrict__ v_cnt, const int64_t* __restrict__ expansion,
                                                          uint32_t limit, int64_t* __restrict__ new_hop_ptr, int64_t* __restrict__ new_vis_ptr,
                                                          int32_t* __restrict__ new_hop_idx, int32_t* __restrict__ new_vis_idx,
                                                          int32_t* __restrict__ new_vis_cnt, int* __restrict__ flags) {
    __shared__ int32_t key[SHELL_SLOTS];
    __shared__ uint32_t cnt[SHELL_SLOTS];   // path count of the slot's column
    __shared__ int32_t seen[SHELL_SLOTS];   // its visit count in vis_{k-1}, 0: not visited
    __shared__ int32_t hop_list[SHELL_CAPACITY], new_list[SHELL_CAPACITY];
    __shared__ int n_hop, n_new;
    const int64_t i = blockIdx.x;
    if (expansion[i] > SHELL_CAPACITY) return;  // k_shell_spill's row (uniform: the whole block leaves)
    const int lane = threadIdx.x;
    for (int s = lane; s < SHELL_SLOTS; s += SHELL_WAVE) {
        key[s] = -1;
        cnt[s] = 0;
        seen[s] = 0;
    }
    if (lane == 0) n_hop = n_new = 0;
    __syncthreads();
    const int64_t h0 = h_ptr[i], h1 = h_ptr[i + 1];
    for (int64_t e = h0 + lane; e < h1; e += SHELL_WAVE) {  // one lane per walked row of A
        const int32_t j = h_idx[e];
        for (int64_t f = a_ptr[j]; f < a_ptr[j + 1]; ++f) {
            const int32_t c = a_idx[f];
            uint32_t s = slot_of(c);
            for (;;) {  // at most SHELL_CAPACITY distinct columns in SHELL_SLOTS slots: a free slot exists
                const int32_t was = atomicCAS(&key[s], -1, c);
                if (was == -1 || was == c) break;
                s = (s + 1) & (SHELL_SLOTS - 1);
            }
            atomicAdd(&cnt[s], 1u);
        }
    }
    __syncthreads();
    const int64_t v0 = v_ptr[i], v1 = v_ptr[i + 1];
    for (int64_t e = v0 + lane; e < v1; e += SHELL_WAVE) {  // the visited columns that the expansion reached
        const int32_t c = v_idx[e];
        uint32_t s = slot_of(c);
        while (key[s] != -1 && key[s] != c) s = (s + 1) & (SHELL_SLOTS - 1);
        if (key[s] == c) seen[s] = v_cnt[e];
    }
    __syncthreads();
    for (int s = lane; s < SHELL_SLOTS; s += SHELL_WAVE) {
        if (key[s] == -1) continue;
        if (cnt[s] >= limit) flags[1] = 1;
        if (cnt[s] > (uint32_t)seen[s]) hop_list[atomicAdd(&n_hop, 1)] = key[s];  // (arrival order: ranked below)
        if (seen[s] == 0) new_list[atomicAdd(&n_new, 1)] = key[s];
    }
    __syncthreads();
    const int nh = n_hop, nn = n_new;
    if (!FILL) {
        if (lane == 0) {
            new_hop_ptr[i] = nh;
            new_vis_ptr[i] = (v1 - v0) + nn;
        }
        return;
    }
    const int64_t oh = new_hop_ptr[i], ov = new_vis_ptr[i];
    for (int t = lane; t < nh; t += SHELL_WAVE) {  // hop_k: its columns by rank
        const int32_t c = hop_list[t];
        int r = 0;
        for (int u = 0; u < nh; ++u) r += hop_list[u] < c;
        new_hop_idx[oh + r] = c;
    }
    for (int t = lane; t < nn; t += SHELL_WAVE) {  // vis_k: the new columns between the old ones
        const int32_t c = new_list[t];
        int r = 0;
        for (int u = 0; u < nn; ++u) r += new_list[u] < c;
        const int64_t p = ov + r + (lower_bound(v_idx, v0, v1, c) - v0);
        new_vis_idx[p] = c;
        new_vis_cnt[p] = 1;
    }
    for (int64_t e = v0 + lane; e < v1; e += SHELL_WAVE) {  // ... and the old ones, one visit more where hop_k has them
        const int32_t c = v_idx[e];
        int r = 0;
        for (int u = 0; u < nn; ++u) r += new_list[u] < c;
        uint32_t s = slot_of(c);
        while (key[s] != -1 && key[s] != c) s = (s + 1) & (SHELL_SLOTS - 1);
        const bool again = key[s] == c && cnt[s] > (uint32_t)seen[s];
        const int64_t p = ov + (e - v0) + r;
        new_vis_idx[p] = c;
        new_vis_cnt[p] = v_cnt[e] + (again ? 1 : 0);
    }
}

// exclusive prefix sum of one flag per thread over the block; *total <- the block's sum.  `part` holds SPILL_T / 64 + 1 words.
__device__ __forceinline__ int block_exclusive(int flag, int* part, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ball = __ballot(flag);
    const int before = __popcll(ball & (((unsigned long long)1 << lane) - 1));
    __syncthreads();  // `part` of the previous call has been read
    if (lane == 0) part[wave] = __popcll(ball);
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < SPILL_T / 64; ++w) {
        if (w < wave) base += part[w];
        sum += part[w];
    }
    *total = sum;
    return base + before;
}

// The rows of `rows[0, n_rows)` (expansion above SHELL_CAPACITY), one block per row at a time on its own dense count array
// dense + blockIdx.x * n, all zero on entry and on exit.
template <bool FILL>
__global__ __launch_bounds__(SPILL_T) void k_shell_spill(const int64_t* __restrict__ a_ptr, const int32_t* __restrict__ a_idx,
                                                         const int64_t* __restrict__ h_ptr, const int32_t* __restrict__ h_idx,
                                                         const int64_t* __restrict__ v_ptr, const int32_t* __restrict__ v_idx,
                                                         const int32_t* __restrict__ v_cnt, const int32_t* __restrict__ rows, int64_t n_rows,
                                                         int64_t n, uint32_t limit, uint32_t* __restrict__ dense,
                                                         int64_t* __restrict__ new_hop_ptr, int64_t* __restrict__ new_vis_ptr,
                                                         int32_t* __restrict__ new_hop_idx, int32_t* __restrict__ new_vis_idx,
                                                         int32_t* __restrict__ new_vis_cnt, int* __restrict__ flags) {
    __shared__ int lo_col, hi_col;
    __shared__ int part[SPILL_T / 64 + 1];
    uint32_t* __restrict__ mine = dense + (size_t)blockIdx.x * (size_t)n;
    for (int64_t q = blockIdx.x; q < n_rows; q += gridDim.x) {  // uniform per block
        const int64_t i = rows[q];
        const int64_t h0 = h_ptr[i], h1 = h_ptr[i + 1], v0 = v_ptr[i], v1 = v_ptr[i + 1];
        if (threadIdx.x == 0) {  // the sweep covers the visited columns too (vis_1 has the diagonal: v1 > v0)
            lo_col = v_idx[v0];
            hi_col = v_idx[v1 - 1];
        }
        __syncthreads();
        for (int64_t e = h0; e < h1; ++e) {  // the block walks one row of A at a time
            const int32_t j = h_idx[e];
            const int64_t f0 = a_ptr[j], f1 = a_ptr[j + 1];
            for (int64_t f = f0 + threadIdx.x; f < f1; f += SPILL_T) atomicAdd(&mine[a_idx[f]], 1u);
            if (threadIdx.x == 0 && f1 > f0) {  // rows of A ascend
                atomicMin(&lo_col, a_idx[f0]);
                atomicMax(&hi_col, a_idx[f1 - 1]);
            }
        }
        __threadfence();
        __syncthreads();
        const int32_t lo = lo_col, hi = hi_col;
        int64_t oh = FILL ? new_hop_ptr[i] : 0, ov = FILL ? new_vis_ptr[i] : 0;
        int64_t nh = 0, nv = 0;
        for (int64_t c0 = lo; c0 <= hi; c0 += SPILL_T) {  // in column order
            const int64_t c = c0 + threadIdx.x;
            uint32_t paths = 0;
            int32_t visits = 0;
            if (c <= hi) {
                paths = __hip_atomic_load(&mine[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the counts were formed by atomics, past L1
                const int64_t p = lower_bound(v_idx, v0, v1, (int32_t)c);
                if (p < v1 && v_idx[p] == (int32_t)c) visits = v_cnt[p];
                if (paths >= limit) flags[1] = 1;
            }
            const int is_hop = paths > (uint32_t)visits, is_vis = visits > 0 || paths > 0;
            int th, tv;
            const int ph = block_exclusive(is_hop, part, &th);
            const int pv = block_exclusive(is_vis, part, &tv);
            if (FILL) {
                if (is_hop) new_hop_idx[oh + nh + ph] = (int32_t)c;
                if (is_vis) {
                    new_vis_idx[ov + nv + pv] = (int32_t)c;
                    new_vis_cnt[ov + nv + pv] = visits + is_hop;
                }
            }
            nh += th;
            nv += tv;
        }
        if (!FILL && threadIdx.x == 0) {
            new_hop_ptr[i] = nh;
            new_vis_ptr[i] = nv;
        }
        __syncthreads();  // every thread has read its counts
        for (int64_t e = h0; e < h1; ++e) {
            const int32_t j = h_idx[e];
            for (int64_t f = a_ptr[j] + threadIdx.x; f < a_ptr[j + 1]; f += SPILL_T) mine[a_idx[f]] = 0;
        }
        __threadfence();
        __syncthreads();
    }
}

// scale[i] of a shell: 1 / (stored entries of row i), 1 / 0 -> 0 (_normalize)
__global__ __launch_bounds__(NICHE_T) void k_scale_shell(const int64_t* __restrict__ ptr, int64_t n, double* __restrict__ scale) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= n) return;
    const int64_t len = ptr[i + 1] - ptr[i];
    scale[i] = len ? __ddiv_rn(1.0, (double)len) : 0.0;
}

// scale[i] of a graph: the L1 norm of row i in ascending column order (sklearn's normalize(A, "l1")); w == nullptr: every entry 1
__global__ __launch_bounds__(NICHE_T) void k_scale_l1(const int64_t* __restrict__ ptr, const double* __restrict__ w, int64_t n,
                                                      double* __restrict__ scale) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) s = __dadd_rn(s, w ? fabs(w[e]) : 1.0);
    scale[i] = s;
}

// Y[i * cp + j] for the columns j of the block X (row-major, n rows of cp doubles, cp a multiple of 4): one thread per row and group
// of four columns, so that a row's index is read once for four sums and the four gathers of an entry are one 32-byte read; every
// element's sum still runs over the row's entries in ascending column order.  MODE 1: shell — the coefficient of every entry is
// scale[i]; 2: L1-normalised graph — the coefficient is w / scale[i] (w itself where the norm is 0).
template <int MODE, bool VARIANCE>
__global__ __launch_bounds__(NICHE_T) void k_aggregate(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                       const double* __restrict__ w, const double* __restrict__ scale,
                                                       const double* __restrict__ X, int64_t n, int cp, double* __restrict__ Y) {
    const int groups = cp >> 2;
    const int64_t t = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (t >= n * groups) return;
    const int64_t i = t / groups;
    const int q = (int)(t - i * groups);
    const double* __restrict__ x = X + 4 * q;
    const double s = scale[i];
    double m1[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
        double coef = s;
        if (MODE == 2) {
            const double a = w ? w[e] : 1.0;
            coef = s != 0.0 ? __ddiv_rn(a, s) : a;
        }
        const double2* __restrict__ v = reinterpret_cast<const double2*>(x + (size_t)idx[e] * (size_t)cp);  // 32-byte aligned
        const double2 lo = v[0], hi = v[1];
        const double val[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m1[u] = __dadd_rn(m1[u], __dmul_rn(coef, val[u]));
            if (VARIANCE) m2[u] = __dadd_rn(m2[u], __dmul_rn(coef, __dmul_rn(val[u], val[u])));
        }
    }
    double* __restrict__ y = Y + (size_t)i * (size_t)cp + 4 * q;
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = VARIANCE ? __dsub_rn(m2[u], __dmul_rn(m1[u], m1[u])) : m1[u];
}

// out[i * ld + j] = in[j * n + i] for j < c
__global__ __launch_bounds__(NICHE_T) void k_transpose(const double* __restrict__ in, int64_t n, int c, int ld, double* __restrict__ out) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t i0 = blockIdx.x * (int64_t)32;
    const int j0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        if (j0 + r < c && i0 + tx < n) tile[r][tx] = in[(size_t)(j0 + r) * (size_t)n + (size_t)(i0 + tx)];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (i0 + r < n && j0 + tx < c) out[(size_t)(i0 + r) * (size_t)ld + (size_t)(j0 + tx)] = tile[tx][r];
}

// cols[t] = c0 + t
__global__ void k_iota(int32_t* __restrict__ cols, int32_t c0, int c) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < c) cols[t] = c0 + t;
}

// out[i * K + c] = sum over the stored entries (i, j) in ascending j of w_ij * prev[j * K + c]; prev == nullptr: the onehot of
// `labels` (a label outside [0, K) belongs to no category).  w == nullptr: every entry 1.
__global__ __launch_bounds__(NICHE_T) void k_label_hop(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                       const double* __restrict__ w, const int32_t* __restrict__ labels,
                                                       const double* __restrict__ prev, int64_t n, int K, double* __restrict__ out) {
    const int64_t t = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (t >= n * K) return;
    const int64_t i = t / K;
    const int c = (int)(t - i * K);
    double acc = 0.0;
    for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
        const int32_t j = idx[e];
        const double p = prev ? prev[(size_t)j * K + c] : (labels[j] == c ? 1.0 : 0.0);
        acc = __dadd_rn(acc, __dmul_rn(w ? w[e] : 1.0, p));
    }
    out[t] = acc;
}

// every row divided by its sum over the K categories (ascending), 0 / 0 -> 0 (`profile_df.div(total).fillna(0.0)`)
__global__ __launch_bounds__(NICHE_T) void k_label_normalise(double* __restrict__ P, int64_t rows, int K) {
    const int64_t i = blockIdx.x * (int64_t)NICHE_T + threadIdx.x;
    if (i >= rows) return;
    double* __restrict__ p = P + (size_t)i * K;
    double s = 0.0;
    for (int c = 0; c < K; ++c) s = __dadd_rn(s, p[c]);
    for (int c = 0; c < K; ++c) {
        const double q = __ddiv_rn(p[c], s);
        p[c] = q != q ? 0.0 : q;
    }
}

struct Shell {  // hop_k and vis_k as sorted CSR
    DevBuf<int64_t> hop_ptr, vis_ptr;
    DevBuf<int32_t> hop_idx, vis_idx, vis_cnt;
    int64_t hop_nnz = 0, vis_nnz = 0, spilled = 0, at_capacity = 0;
};

// lens[0, n) -> exclusive prefix sums in ptr[0, n]; returns the total
int scan_to_ptr(hipStream_t st, int64_t n, DevBuf<int64_t>& ptr, std::vector<int64_t>& host, int64_t* total) {
    SQGR_HIP(hipMemcpyAsync(host.data(), ptr.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    int64_t run = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v = host[i];
        host[i] = run;
        run += v;
    }
    host[n] = run;
    SQGR_HIP(hipMemcpyAsync(ptr.p, host.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipStreamSynchronize(st));  // `host` is reused
    *total = run;
    return SQGR_OK;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

struct sqgr_shells {
    sqgr_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t distance = 0;
    std::vector<Shell*> shell;  // [distance]: shell[k - 1] is hop_k / vis_k
    ~sqgr_shells() {
        for (Shell* s : shell) delete s;
    }
};

int sqgr_niche_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = SHELL_CAPACITY;
    out_info[1] = COUNT_LIMIT;
    out_info[2] = AGG_MAX_COLS;
    out_info[3] = MAX_DISTANCE;
    return SQGR_OK;
}

static int build_shells(sqgr_shells* h, const sqgr_graph* g, uint32_t limit) {
    sqgr_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int64_t n = g->n;
    const unsigned row_blocks = (unsigned)ceil_div(n, NICHE_T);
    DevBuf<int> flags;
    SQGR_TRY(flags.alloc(2));
    SQGR_HIP(hipMemsetAsync(flags.p, 0, 2 * sizeof(int), st));
    {
        LaunchTimer t(ctx, "niche_check_rows");
        k_check_rows<<<row_blocks, NICHE_T, 0, st>>>(g->indptr.p, g->indices.p, n, flags.p);
        SQGR_HIP(hipGetLastError());
    }
    int hf[2] = {1, 1};
    SQGR_HIP(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    SQGR_REQUIRE(!hf[0], "sqgr_shells_create: a row of the graph is not sorted or repeats an entry (sort_indices / sum_duplicates)");

    std::vector<int64_t> host((size_t)n + 1);
    DevBuf<int64_t> expansion;
    DevBuf<int32_t> spill_rows;
    DevBuf<uint32_t> dense;
    SQGR_TRY(expansion.alloc((size_t)n));
    for (int32_t k = 1; k <= h->distance; ++k) {
        Shell* s = new Shell();
        h->shell.push_back(s);
        SQGR_TRY(s->hop_ptr.alloc((size_t)n + 1));
        SQGR_TRY(s->vis_ptr.alloc((size_t)n + 1));
        if (k == 1) {
            {
                LaunchTimer t(ctx, "niche_shell_first");
                k_shell_first<false><<<row_blocks, NICHE_T, 0, st>>>(g->indptr.p, g->indices.p, n, s->hop_ptr.p, s->vis_ptr.p, nullptr, nullptr,
                                                                     nullptr);
                SQGR_HIP(hipGetLastError());
            }
            SQGR_TRY(scan_to_ptr(st, n, s->hop_ptr, host, &s->hop_nnz));
            SQGR_TRY(scan_to_ptr(st, n, s->vis_ptr, host, &s->vis_nnz));
            SQGR_TRY(s->hop_idx.alloc((size_t)s->hop_nnz));
            SQGR_TRY(s->vis_idx.alloc((size_t)s->vis_nnz));
            SQGR_TRY(s->vis_cnt.alloc((size_t)s->vis_nnz));
            LaunchTimer t(ctx, "niche_shell_first");
            k_shell_first<true><<<row_blocks, NICHE_T, 0, st>>>(g->indptr.p, g->indices.p, n, s->hop_ptr.p, s->vis_ptr.p, s->hop_idx.p,
                                                                s->vis_idx.p, s->vis_cnt.p);
            SQGR_HIP(hipGetLastError());
            continue;
        }
        const Shell* p = h->shell[(size_t)k - 2];
        {
            LaunchTimer t(ctx, "niche_shell_expansion");
            k_shell_expansion<<<row_blocks, NICHE_T, 0, st>>>(g->indptr.p, p->hop_ptr.p, p->hop_idx.p, n, expansion.p);
            SQGR_HIP(hipGetLastError());
        }
        SQGR_HIP(hipMemcpyAsync(host.data(), expansion.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        std::vector<int32_t> rows;
        for (int64_t i = 0; i < n; ++i) {
            if (host[i] > SHELL_CAPACITY) rows.push_back((int32_t)i);
            s->at_capacity += host[i] == SHELL_CAPACITY;
        }
        s->spilled = (int64_t)rows.size();
        const unsigned spill_grid = (unsigned)std::min<int64_t>(SPILL_BLOCKS, s->spilled);
        if (s->spilled) {
            SQGR_TRY(spill_rows.alloc(rows.size()));
            SQGR_HIP(hipMemcpyAsync(spill_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
            if (!dense.p) {  // zeroed once: every row leaves its array zeroed
                SQGR_TRY(dense.alloc_pooled((size_t)SPILL_BLOCKS * (size_t)n));
                SQGR_HIP(hipMemsetAsync(dense.p, 0, (size_t)SPILL_BLOCKS * (size_t)n * 4, st));
            }
        }
        for (int pass = 0; pass < 2; ++pass) {
            if (pass == 1) {
                SQGR_TRY(scan_to_ptr(st, n, s->hop_ptr, host, &s->hop_nnz));
                SQGR_TRY(scan_to_ptr(st, n, s->vis_ptr, host, &s->vis_nnz));
                SQGR_TRY(s->hop_idx.alloc((size_t)s->hop_nnz));
                SQGR_TRY(s->vis_idx.alloc((size_t)s->vis_nnz));
                SQGR_TRY(s->vis_cnt.alloc((size_t)s->vis_nnz));
            }
            if (n > 0) {
                LaunchTimer t(ctx, "niche_shell_row");
                if (pass == 0)
                    k_shell_row<false><<<(unsigned)n, SHELL_WAVE, 0, st>>>(g->indptr.p, g->indices.p, p->hop_ptr.p, p->hop_idx.p, p->vis_ptr.p,
                                                                           p->vis_idx.p, p->vis_cnt.p, expansion.p, limit, s->hop_ptr.p,
                                                                           s->vis_ptr.p, nullptr, nullptr, nullptr, flags.p);
                else
                    k_shell_row<true><<<(unsigned)n, SHELL_WAVE, 0, st>>>(g->indptr.p, g->indices.p, p->hop_ptr.p, p->hop_idx.p, p->vis_ptr.p,
                                                                          p->vis_idx.p, p->vis_cnt.p, expansion.p, limit, s->hop_ptr.p,
                                                                          s->vis_ptr.p, s->hop_idx.p, s->vis_idx.p, s->vis_cnt.p, flags.p);
                SQGR_HIP(hipGetLastError());
            }
            if (s->spilled) {
                LaunchTimer t(ctx, "niche_shell_spill");
                if (pass == 0)
                    k_shell_spill<false><<<spill_grid, SPILL_T, 0, st>>>(g->indptr.p, g->indices.p, p->hop_ptr.p, p->hop_idx.p, p->vis_ptr.p,
                                                                         p->vis_idx.p, p->vis_cnt.p, spill_rows.p, s->spilled, n, limit, dense.p,
                                                                         s->hop_ptr.p, s->vis_ptr.p, nullptr, nullptr, nullptr, flags.p);
                else
                    k_shell_spill<true><<<spill_grid, SPILL_T, 0, st>>>(g->indptr.p, g->indices.p, p->hop_ptr.p, p->hop_idx.p, p->vis_ptr.p,
                                                                        p->vis_idx.p, p->vis_cnt.p, spill_rows.p, s->spilled, n, limit, dense.p,
                                                                        s->hop_ptr.p, s->vis_ptr.p, s->hop_idx.p, s->vis_idx.p, s->vis_cnt.p,
                                                                        flags.p);
                SQGR_HIP(hipGetLastError());
            }
            if (pass == 0) {
                SQGR_HIP(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
                SQGR_HIP(hipStreamSynchronize(st));
                if (hf[1]) {
                    set_error("sqgr_shells_create: a path count of shell %d reaches %u; the reference's float32 path sums stop being exact at 2^24",
                              (int)k, limit);
                    return SQGR_ERR_UNSUPPORTED;
                }
            }
        }
    }
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_shells_create(sqgr_ctx* ctx, const sqgr_graph* g, int32_t distance, int32_t count_limit, sqgr_shells** out) {
    SQGR_REQUIRE(ctx && g && out, "null argument");
    SQGR_REQUIRE(g->ctx == ctx, "graph belongs to a different context");
    SQGR_REQUIRE(distance >= 1 && distance <= MAX_DISTANCE, "distance=%d outside [1, %d]", distance, MAX_DISTANCE);
    SQGR_REQUIRE(count_limit >= 0 && (uint32_t)count_limit <= COUNT_LIMIT, "count_limit=%d outside [0, 2^24]", count_limit);
    if (g->n >= ((int64_t)1 << 31) - 1) {
        set_error("sqgr_shells_create: n=%lld; one block per row needs n < 2^31 - 1", (long long)g->n);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    sqgr_shells* h = new sqgr_shells();
    h->ctx = ctx;
    h->n = g->n;
    h->distance = distance;
    const int rc = build_shells(h, g, count_limit ? (uint32_t)count_limit : COUNT_LIMIT);
    if (rc != SQGR_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        delete h;
        return rc;
    }
    *out = h;
    return SQGR_OK;
}

int sqgr_shells_info(const sqgr_shells* h, int32_t k, int64_t* out_info) {
    SQGR_REQUIRE(h && out_info, "null argument");
    SQGR_REQUIRE(k >= 1 && k <= h->distance, "k=%d outside [1, %d]", k, h->distance);
    const Shell* s = h->shell[(size_t)k - 1];
    out_info[0] = h->n;
    out_info[1] = s->hop_nnz;
    out_info[2] = s->vis_nnz;
    out_info[3] = s->spilled;
    out_info[4] = s->at_capacity;
    return SQGR_OK;
}

int sqgr_shells_read(const sqgr_shells* h, int32_t k, int64_t* hop_indptr, int32_t* hop_indices, int64_t* vis_indptr, int32_t* vis_indices,
                     int32_t* vis_counts) {
    SQGR_REQUIRE(h && hop_indptr && hop_indices && vis_indptr && vis_indices && vis_counts, "null argument");
    SQGR_REQUIRE(k >= 1 && k <= h->distance, "k=%d outside [1, %d]", k, h->distance);
    SQGR_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const Shell* s = h->shell[(size_t)k - 1];
    SQGR_HIP(hipMemcpyAsync(hop_indptr, s->hop_ptr.p, ((size_t)h->n + 1) * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipMemcpyAsync(vis_indptr, s->vis_ptr.p, ((size_t)h->n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (s->hop_nnz) SQGR_HIP(hipMemcpyAsync(hop_indices, s->hop_idx.p, (size_t)s->hop_nnz * 4, hipMemcpyDeviceToHost, st));
    if (s->vis_nnz) {
        SQGR_HIP(hipMemcpyAsync(vis_indices, s->vis_idx.p, (size_t)s->vis_nnz * 4, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipMemcpyAsync(vis_counts, s->vis_cnt.p, (size_t)s->vis_nnz * 4, hipMemcpyDeviceToHost, st));
    }
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_shells_destroy(sqgr_shells* h) {
    if (!h) return SQGR_OK;
    (void)hipSetDevice(h->ctx->device);
    delete h;
    return SQGR_OK;
}

// The body of sqgr_niche_aggregate and sqgr_pca_fill_aggregate: the same kernels and the same arithmetic; every block of columns ends
// in one pitched copy, to the host array `out` (kind hipMemcpyDeviceToHost) or to a device matrix (hipMemcpyDeviceToDevice).
static int aggregate_blocks(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_shells* shells, int32_t k, const sqgr_matrix* m, int32_t variance,
                            double* out, int64_t ld_out, hipMemcpyKind kind) {
    SQGR_REQUIRE(ctx && m && out && (g != nullptr) != (shells != nullptr), "null argument, or both / neither of graph and shells");
    SQGR_REQUIRE(m->ctx == ctx && (!g || g->ctx == ctx) && (!shells || shells->ctx == ctx), "handle belongs to a different context");
    SQGR_REQUIRE(m->cols_pending <= 0, "the matrix is still being uploaded");
    const int64_t n = m->n_rows, nv = m->n_cols;
    SQGR_REQUIRE(n == (g ? g->n : shells->n), "the matrix has %lld rows, the graph %lld", (long long)n, (long long)(g ? g->n : shells->n));
    SQGR_REQUIRE(ld_out >= nv, "ld_out=%lld < n_cols=%lld", (long long)ld_out, (long long)nv);
    SQGR_REQUIRE(!shells || (k >= 0 && k <= shells->distance), "k=%d outside [0, %d]", k, shells ? shells->distance : 0);
    SQGR_REQUIRE(variance == 0 || variance == 1, "variance=%d", variance);
    SQGR_REQUIRE(!g || !variance, "variance applies to shells only");
    if (n == 0 || nv == 0) return SQGR_OK;
    if (nv >= ((int64_t)1 << 31)) {
        set_error("sqgr_niche_aggregate: n_cols=%lld", (long long)nv);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SQGR_TRY(m->ensure_by_column());
    const unsigned row_blocks = (unsigned)ceil_div(n, NICHE_T);
    const int mode = shells ? (k == 0 ? 0 : 1) : 2;
    const int64_t* ptr = nullptr;
    const int32_t* idx = nullptr;
    const double* w = nullptr;
    DevBuf<double> scale;
    if (mode == 1) {
        const Shell* s = shells->shell[(size_t)k - 1];
        ptr = s->hop_ptr.p;
        idx = s->hop_idx.p;
        SQGR_TRY(scale.alloc((size_t)n));
        LaunchTimer t(ctx, "niche_scale");
        k_scale_shell<<<row_blocks, NICHE_T, 0, st>>>(ptr, n, scale.p);
        SQGR_HIP(hipGetLastError());
    } else if (mode == 2) {
        ptr = g->indptr.p;
        idx = g->indices.p;
        w = g->has_data ? g->data.p : nullptr;
        SQGR_TRY(scale.alloc((size_t)n));
        LaunchTimer t(ctx, "niche_scale");
        k_scale_l1<<<row_blocks, NICHE_T, 0, st>>>(ptr, w, n, scale.p);
        SQGR_HIP(hipGetLastError());
    }
    // one block of columns resident at a time: X column-major as the densification writes it, X and Y row-major (rows padded to a
    // multiple of four columns; the padding is zeroed once and never copied out), at most 256 MB each
    const int cb = (int)std::min<int64_t>({nv, (int64_t)AGG_MAX_COLS, std::max<int64_t>(1, ((int64_t)256 << 20) / (n * 8))});
    const int cp = (cb + 3) & ~3;
    DevBuf<int32_t> cols;
    DevBuf<double> X, Xr, Y;
    SQGR_TRY(cols.alloc((size_t)cb));
    SQGR_TRY(X.alloc_pooled((size_t)cb * n));
    SQGR_TRY(Xr.alloc_pooled((size_t)cp * n));
    SQGR_HIP(hipMemsetAsync(Xr.p, 0, (size_t)cp * n * 8, st));
    if (mode != 0) SQGR_TRY(Y.alloc_pooled((size_t)cp * n));
    for (int64_t c0 = 0; c0 < nv; c0 += cb) {
        const int c = (int)std::min<int64_t>(cb, nv - c0);
        k_iota<<<1, AGG_MAX_COLS, 0, st>>>(cols.p, (int32_t)c0, c);
        SQGR_HIP(hipGetLastError());
        {
            LaunchTimer t(ctx, "niche_expand");
            SQGR_HIP(expand_column_list(m, cols.p, c, X.p, st));
        }
        {
            LaunchTimer t(ctx, "niche_transpose");
            const dim3 grid((unsigned)ceil_div(n, 32), (unsigned)ceil_div(c, 32));
            k_transpose<<<grid, NICHE_T, 0, st>>>(X.p, n, c, cp, Xr.p);
            SQGR_HIP(hipGetLastError());
        }
        if (mode != 0) {
            LaunchTimer t(ctx, "niche_aggregate");
            const unsigned grid = (unsigned)ceil_div(n * (cp >> 2), NICHE_T);
            if (mode == 1 && !variance) k_aggregate<1, false><<<grid, NICHE_T, 0, st>>>(ptr, idx, w, scale.p, Xr.p, n, cp, Y.p);
            else if (mode == 1) k_aggregate<1, true><<<grid, NICHE_T, 0, st>>>(ptr, idx, w, scale.p, Xr.p, n, cp, Y.p);
            else k_aggregate<2, false><<<grid, NICHE_T, 0, st>>>(ptr, idx, w, scale.p, Xr.p, n, cp, Y.p);
            SQGR_HIP(hipGetLastError());
        }
        SQGR_HIP(hipMemcpy2DAsync(out + c0, (size_t)ld_out * 8, mode != 0 ? Y.p : Xr.p, (size_t)cp * 8, (size_t)c * 8, (size_t)n, kind, st));
        SQGR_HIP(hipStreamSynchronize(st));  // the buffers are reused by the next block
    }
    return SQGR_OK;
}

int sqgr_niche_aggregate(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_shells* shells, int32_t k, const sqgr_matrix* m, int32_t variance,
                         double* out, int64_t ld_out) {
    return aggregate_blocks(ctx, g, shells, k, m, variance, out, ld_out, hipMemcpyDeviceToHost);
}

int sqgr_pca_fill_aggregate(sqgr_pca* h, int32_t col0, const sqgr_graph* g, const sqgr_shells* shells, int32_t k, const sqgr_matrix* m,
                            int32_t variance) {
    SQGR_REQUIRE(h && m, "null argument");
    SQGR_REQUIRE(m->n_rows == h->n, "the matrix has %lld rows, the PCA %lld", (long long)m->n_rows, (long long)h->n);
    SQGR_REQUIRE(col0 >= 0 && (int64_t)col0 + m->n_cols <= h->D, "columns [%d, %d + %lld) outside [0, %d)", col0, col0, (long long)m->n_cols, h->D);
    h->have_mean = false;
    return aggregate_blocks(h->ctx, g, shells, k, m, variance, h->F.p + col0, h->D, hipMemcpyDeviceToDevice);
}

int sqgr_niche_label_hops(sqgr_ctx* ctx, const sqgr_graph* g, const int32_t* labels, int32_t K, int32_t distance, int32_t weighted,
                          int32_t normalise, double* out) {
    SQGR_REQUIRE(ctx && g && labels && out, "null argument");
    SQGR_REQUIRE(g->ctx == ctx, "graph belongs to a different context");
    SQGR_REQUIRE(K >= 1 && distance >= 1 && distance <= MAX_DISTANCE, "K=%d, distance=%d", K, distance);
    SQGR_REQUIRE(!weighted || g->has_data, "weighted=1 but the graph was created without weights");
    const int64_t n = g->n;
    if (n == 0) return SQGR_OK;
    const int64_t panel = n * (int64_t)K;
    if (panel >= ((int64_t)1 << 38)) {
        set_error("sqgr_niche_label_hops: n * K = %lld", (long long)panel);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<int32_t> d_lab;
    DevBuf<double> P;  // [distance][n][K]
    SQGR_TRY(d_lab.alloc((size_t)n));
    SQGR_TRY(P.alloc_pooled((size_t)panel * distance));
    SQGR_HIP(hipMemcpyAsync(d_lab.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const double* w = weighted ? g->data.p : nullptr;
    for (int32_t hop = 0; hop < distance; ++hop) {
        LaunchTimer t(ctx, "niche_label_hop");
        k_label_hop<<<(unsigned)ceil_div(panel, NICHE_T), NICHE_T, 0, st>>>(g->indptr.p, g->indices.p, w, d_lab.p,
                                                                            hop ? P.p + (size_t)(hop - 1) * panel : nullptr, n, K,
                                                                            P.p + (size_t)hop * panel);
        SQGR_HIP(hipGetLastError());
    }
    if (normalise) {  // after the last hop: hop h reads the sums of hop h - 1, not its proportions
        LaunchTimer t(ctx, "niche_label_normalise");
        k_label_normalise<<<(unsigned)ceil_div(n * distance, NICHE_T), NICHE_T, 0, st>>>(P.p, n * distance, K);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(out, P.p, (size_t)panel * distance * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}
