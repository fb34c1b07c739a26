// libsqgr: sepal — diffusion-time scores of spatially variable genes (gr/_sepal.py).
//
// Reference semantics (squidpy, src/squidpy/gr/_sepal.py):
//   :229-242  one sweep, Jacobi-style, float64:  nbrs_j = sum of c over the stored neighbours of saturated spot j (left to right);
//             hex d2 = (2 nbrs - 12 c) / 3, rect d2 = nbrs - 4 c;  c_sat += d2 dt;  c_unsat += d2[nearest saturated] dt
//             (d2 from the concentrations BEFORE the sweep);  c = 0 where c < 0
//   :244-251  ent_i = H(c[sat]) / n_sat (_entropy :290-305);  stop at the first i with |ent_i - ent_{i-1}| <= thresh (ent_{-1} = 1)
//
// The host hands over one table row per spot j: the spot t whose d2 moves j (t = j for a saturated spot, its nearest saturated spot
// otherwise) and t's neighbours in their stored order.  An unsaturated spot recomputes the d2 of its t from the same old values with
// the same operations, so the whole sweep is one pass with one barrier.  Every product and sum is rounded on its own (the library is
// built with -ffp-contract=off) and the hex division is IEEE: the concentrations follow numpy's bit for bit.  The entropy is a
// fixed-order block reduction (a gene's score depends on that gene alone); its float64 sums and log are not numpy's.
//
// Routes, chosen from n:
//   LDS     n <= SEPAL_LDS_MAX_SPOTS: one workgroup per gene, the gene's vector in LDS.  A persistent grid takes genes from a device
//           counter (sweeps per gene differ by ~40x).  New values wait in registers across the barrier, so no second copy is needed,
//           and the stop test of sweep i is read after the first barrier of sweep i + 1 (2 barriers per sweep).
//   global  larger grids (Visium HD bins): the vector ping-pongs between two global buffers, one workgroup per gene.
// Both routes run in chunks of sweeps (run_batch): a gene still running at the end of a launch leaves its vector and last entropy in
// global memory for the next one, so that no launch runs for long whatever n_iter is.
#include "sqgr_common.h"
#include "sqgr_matrix.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sqgr {
namespace {

constexpr double SEPAL_EPS = 2.220446049250313e-16;  // np.finfo(np.float64).eps
constexpr int SEPAL_T = 1024;                         // workgroup size of both routes (16 waves)
constexpr int SEPAL_MAXW = SEPAL_T / 64;
constexpr int SEPAL_LDS_BYTES = 160 * 1024;
constexpr int64_t SEPAL_LDS_MAX_SPOTS = (SEPAL_LDS_BYTES - 1024) / 8;  // 20352: the rest holds the reduction slots
// spot-sweeps one launch may schedule (genes x n x sweeps of the chunk): 0.34 s (LDS) and 0.60 s (global) measured with every gene
// running; both routes cut n_iter into chunks of sweeps, so this holds for any n_iter
constexpr double SEPAL_LAUNCH_BUDGET = 6.0e10;
constexpr double SEPAL_GLOBAL_BUDGET = 2.0e10;

__device__ inline double wave_sum(double v) {  // xor butterfly: every lane ends with the same, fixed-order sum
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one table row: ix[0] = t, ix[1 .. K] = t's neighbours in stored order
struct Tab16 {  // n <= 65536: eight uint16 in one uint4
    const uint4* p;
    __device__ inline void get(int64_t j, int (&ix)[7]) const { unpack(p[j], ix); }
    __device__ static inline void unpack(const uint4 u, int (&ix)[7]) {
        ix[0] = (int)(u.x & 0xffffu), ix[1] = (int)(u.x >> 16), ix[2] = (int)(u.y & 0xffffu), ix[3] = (int)(u.y >> 16);
        ix[4] = (int)(u.z & 0xffffu), ix[5] = (int)(u.z >> 16), ix[6] = (int)(u.w & 0xffffu);
    }
};
struct Tab32 {  // eight int32 in two int4
    const int4* p;
    __device__ inline void get(int64_t j, int (&ix)[7]) const {
        const int4 a = p[2 * j], b = p[2 * j + 1];
        ix[0] = a.x, ix[1] = a.y, ix[2] = a.z, ix[3] = a.w, ix[4] = b.x, ix[5] = b.y, ix[6] = b.z;
    }
};

// the new concentration of spot j from the old vector c (gr/_sepal.py:229-242)
template <int K>
__device__ inline double sepal_new(const double* c, int64_t j, const int (&ix)[7], double dt) {
    double s = c[ix[1]];
#pragma unroll
    for (int k = 2; k <= K; ++k) s = s + c[ix[k]];  // np.sum of < 8 elements: left to right
    const double ct = c[ix[0]];
    double d2;
    if (K == 6) d2 = (2.0 * s - 12.0 * ct) / 3.0;  // _laplacian_hex
    else d2 = s - 4.0 * ct;                         // _laplacian_rect
    const double own = (ix[0] == j) ? ct : c[j];
    const double v = own + d2 * dt;
    return v < 0.0 ? 0.0 : v;  // conc[conc < 0] = 0: a compare and select, NaN stays
}

// one term of _entropy (:290-305) for a saturated spot's value v > 0, S = sum of the positive values
__device__ inline double entropy_term(double v, double S) {
    const double x = v / S;
    return -log(x < SEPAL_EPS ? SEPAL_EPS : x) * x;
}

// one gene's sweeps [it0, it1) on the LDS route (k_sepal_lds)
template <int K, int SPT, bool REG>
__device__ __forceinline__ void sepal_gene(double* __restrict__ c, double* red_s, double (*red_h)[SEPAL_MAXW], double* __restrict__ xg,
                                           int n, int g, const uint4* __restrict__ tab, const uint4 (&tb)[REG ? SPT : 1], uint32_t satmask,
                                           double rn_sat, int it0, int it1, double dt, double thresh, double* __restrict__ prev_ent,
                                           int32_t* __restrict__ out_iter, int trace, double* __restrict__ trace_ent) {
    const int T = blockDim.x, W = T >> 6, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < n; j += T) c[j] = xg[j];
    __syncthreads();
    double prev = it0 == 0 ? 1.0 : prev_ent[g];
    int stop = -1;
    double nv[SPT];
    for (int it = it0;; ++it) {
        if (it < it1) {
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                const int j = threadIdx.x + k * T;
                if (j < n) {
                    int ix[7];
                    Tab16::unpack(REG ? tb[REG ? k : 0] : tab[j], ix);
                    nv[k] = sepal_new<K>(c, j, ix, dt);
                }
                __builtin_amdgcn_sched_barrier(0);  // one item at a time: hoisting the loads of all SPT items spills registers
            }
        }
        __syncthreads();  // every read of the old vector is done; the entropy partials of sweep it - 1 are visible
        if (it > it0) {
            double H = 0.0;
            for (int q = 0; q < W; ++q) H += red_h[(it - 1) & 1][q];
            const double ent = H / rn_sat;
            const double d = fabs(ent - prev);
            prev = ent;
            if (trace) {
                if (threadIdx.x == 0) trace_ent[it - 1] = ent;
            } else if (d <= thresh) {  // a NaN difference never qualifies
                stop = it - 1;
                break;
            }
        }
        if (it == it1) break;
        double ps = 0.0;
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int j = threadIdx.x + k * T;
            if (j < n) {
                c[j] = nv[k];
                if (((satmask >> k) & 1u) && nv[k] > 0.0) ps += nv[k];
            }
        }
        ps = wave_sum(ps);
        if (lane == 0) red_s[w] = ps;
        __syncthreads();  // the new vector and the S partials are visible
        double S = 0.0;
        for (int q = 0; q < W; ++q) S += red_s[q];
        double ph = 0.0;
        if (!(S < SEPAL_EPS)) {
#pragma unroll
            for (int k = 0; k < SPT; ++k) {
                if (((satmask >> k) & 1u) && nv[k] > 0.0) ph += entropy_term(nv[k], S);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        ph = wave_sum(ph);
        if (lane == 0) red_h[it & 1][w] = ph;
    }
    if (stop >= 0) {
        if (threadIdx.x == 0) out_iter[g] = stop;
    } else {  // still running: the next chunk resumes from here (the last barrier passed after the final write to c)
        for (int j = threadIdx.x; j < n; j += T) xg[j] = c[j];
        if (threadIdx.x == 0) prev_ent[g] = prev;
    }
}

// ---- LDS route: sweeps [it0, it1) of a chunked run.  X: the batch's genes, gene-major [gb][n]; a gene that is still running at
// it1 leaves its vector in X and its last entropy in prev_ent[g] for the next launch; out_iter[g] >= 0 marks a gene that has
// stopped (-1: running, or no stop within n_iter after the last chunk).
// trace != 0: no stop test; ent of every sweep to trace_ent[it].
template <int K, int SPT>
__global__ __launch_bounds__(SEPAL_T) void k_sepal_lds(double* __restrict__ X, int n, int gb, const uint4* __restrict__ tab, int n_sat,
                                                      int it0, int it1, double dt, double thresh, unsigned* __restrict__ next_gene,
                                                      double* __restrict__ prev_ent, int32_t* __restrict__ out_iter, int trace,
                                                      double* __restrict__ trace_ent) {
    extern __shared__ double c[];  // [n]
    __shared__ double red_s[SEPAL_MAXW], red_h[2][SEPAL_MAXW];
    __shared__ int s_gene;
    constexpr bool REG = SPT <= 8;  // table rows held in registers for the whole kernel; larger grids re-read them (L2) every sweep
    const int T = blockDim.x;
    uint4 tb[REG ? SPT : 1];
    if (REG) {
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            const int j = threadIdx.x + k * T;
            tb[REG ? k : 0] = j < n ? tab[j] : make_uint4(0, 0, 0, 0);
        }
    }
    uint32_t satmask = 0;  // bit k: item k is a saturated spot
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int j = threadIdx.x + k * T;
        if (j < n && (int)((REG ? tb[REG ? k : 0] : tab[j]).x & 0xffffu) == j) satmask |= 1u << k;
    }
    const double rn_sat = (double)n_sat;
    for (;;) {
        if (threadIdx.x == 0) s_gene = (int)atomicAdd(next_gene, 1u);
        __syncthreads();
        const int g = s_gene;
        if (g >= gb) break;
        if (out_iter[g] < 0) sepal_gene<K, SPT, REG>(c, red_s, red_h, X + (size_t)g * n, n, g, tab, tb, satmask, rn_sat, it0, it1, dt, thresh,
                                                 prev_ent, out_iter, trace, trace_ent);  // else: stopped in an earlier chunk
        __syncthreads();  // `c` and `s_gene` are reused by the next gene
    }
}

// ---- global route: one workgroup per gene, sweeps [it0, it1) of a chunked run.  The vector ping-pongs between A = X (sweep
// parity 0 reads it) and B; prev_ent[g] carries the last entropy across launches, out_iter[g] >= 0 marks a gene that has stopped.
template <int K, typename TAB>
__global__ __launch_bounds__(SEPAL_T) void k_sepal_global(double* __restrict__ A, double* __restrict__ B, int64_t n, TAB tab, int n_sat,
                                                         int it0, int it1, double dt, double thresh, double* __restrict__ prev_ent,
                                                         int32_t* __restrict__ out_iter, int trace, double* __restrict__ trace_ent) {
    __shared__ double red_s[SEPAL_MAXW], red_h[SEPAL_MAXW];
    const int g = blockIdx.x;
    if (out_iter[g] >= 0) return;
    const int T = blockDim.x, W = T >> 6, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double* a = A + (size_t)g * n;
    double* b = B + (size_t)g * n;
    double prev = it0 == 0 ? 1.0 : prev_ent[g];
    const double rn_sat = (double)n_sat;
    for (int it = it0; it < it1; ++it) {
        const double* co = (it & 1) ? b : a;
        double* cn = (it & 1) ? a : b;
        double ps = 0.0;
        for (int64_t j = threadIdx.x; j < n; j += T) {
            int ix[7];
            tab.get(j, ix);
            const double v = sepal_new<K>(co, j, ix, dt);
            cn[j] = v;
            if (ix[0] == j && v > 0.0) ps += v;
        }
        ps = wave_sum(ps);
        if (lane == 0) red_s[w] = ps;
        __syncthreads();  // the new vector (this workgroup's own global writes) and the S partials are visible
        double S = 0.0;
        for (int q = 0; q < W; ++q) S += red_s[q];
        double ph = 0.0;
        if (!(S < SEPAL_EPS)) {
            for (int64_t j = threadIdx.x; j < n; j += T) {
                int ix[7];
                tab.get(j, ix);
                const double v = cn[j];
                if (ix[0] == j && v > 0.0) ph += entropy_term(v, S);
            }
        }
        ph = wave_sum(ph);
        if (lane == 0) red_h[w] = ph;
        __syncthreads();
        double H = 0.0;
        for (int q = 0; q < W; ++q) H += red_h[q];
        const double ent = H / rn_sat;
        const double d = fabs(ent - prev);
        prev = ent;
        if (trace) {
            if (threadIdx.x == 0) trace_ent[it] = ent;
        } else if (d <= thresh) {
            if (threadIdx.x == 0) out_iter[g] = it;
            return;
        }
    }
    if (threadIdx.x == 0) prev_ent[g] = prev;
}

}  // namespace
}  // namespace sqgr

using namespace sqgr;

struct sqgr_sepal {
    sqgr_ctx* ctx = nullptr;
    int64_t n = 0, n_sat = 0;
    int K = 0;
    bool lds = false, wide = false;
    int spt = 0;  // LDS route: items per thread (template instance)
    DevBuf<uint4> tab16;
    DevBuf<int4> tab32;
    DevBuf<unsigned> counter;
};

namespace {

// the LDS-route kernel instance of this lattice, its LDS size set; `slots` = workgroups resident on the GPU at once
int lds_kernel(sqgr_sepal* h, const void** out_fn, int* slots) {
    const size_t lds = (size_t)h->n * 8;
    const void* fn = nullptr;
#define SEPAL_PICK(KK, SS) \
    if (h->K == KK && h->spt == SS) fn = reinterpret_cast<const void*>(k_sepal_lds<KK, SS>);
    SEPAL_PICK(6, 8) SEPAL_PICK(6, 16) SEPAL_PICK(6, 24) SEPAL_PICK(4, 8) SEPAL_PICK(4, 16) SEPAL_PICK(4, 24)
#undef SEPAL_PICK
    SQGR_REQUIRE(fn, "no LDS kernel for K=%d, %d items per thread", h->K, h->spt);
    SQGR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int occ = 0;
    SQGR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, SEPAL_T, lds));
    *out_fn = fn;
    *slots = std::max(occ, 1) * std::max(h->ctx->cu_count, 1);
    return SQGR_OK;
}

// n_iter sweeps (fewer for genes that stop) of the gb genes whose vectors are in X, in launches of `chunk` sweeps: a launch
// schedules at most max(budget, gb x n) spot-sweeps whatever n_iter is.  out_iter filled on return; after a trace X[0] holds the
// vector after n_iter sweeps.
int run_batch(sqgr_sepal* h, double* X, int gb, int n_iter, double dt, double thresh, int32_t* out_iter, int trace, double* trace_ent) {
    sqgr_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    DevBuf<double> B, prev;
    if (!h->lds) SQGR_TRY(B.alloc_pooled((size_t)gb * h->n));
    SQGR_TRY(prev.alloc((size_t)gb));
    SQGR_HIP(hipMemsetAsync(out_iter, 0xff, (size_t)gb * 4, st));  // -1: running
    const void* fn = nullptr;
    int slots = 0;
    if (h->lds) SQGR_TRY(lds_kernel(h, &fn, &slots));
    const double budget = h->lds ? SEPAL_LAUNCH_BUDGET : SEPAL_GLOBAL_BUDGET;
    const int chunk = (int)std::max<double>(1.0, std::min<double>(n_iter, budget / ((double)gb * (double)h->n)));
    std::vector<int32_t> host((size_t)gb);
    const int n = (int)h->n, n_sat = (int)h->n_sat;
    for (int it0 = 0; it0 < n_iter; it0 += chunk) {
        int it1 = (int)std::min<int64_t>(n_iter, (int64_t)it0 + chunk);
        if (h->lds) {
            SQGR_HIP(hipMemsetAsync(h->counter.p, 0, sizeof(unsigned), st));
            const uint4* tab = h->tab16.p;
            unsigned* next = h->counter.p;
            double* pe = prev.p;
            void* args[] = {(void*)&X, (void*)&n, (void*)&gb, (void*)&tab, (void*)&n_sat, (void*)&it0, (void*)&it1, (void*)&dt,
                            (void*)&thresh, (void*)&next, (void*)&pe, (void*)&out_iter, (void*)&trace, (void*)&trace_ent};
            LaunchTimer t(ctx, "sepal_lds");
            SQGR_HIP(hipLaunchKernel(fn, dim3((unsigned)std::min(gb, slots)), dim3(SEPAL_T), args, (size_t)n * 8, st));
        } else {
            LaunchTimer t(ctx, "sepal_global");
            if (h->wide) {
                const Tab32 tab{h->tab32.p};
                if (h->K == 6) k_sepal_global<6, Tab32><<<gb, SEPAL_T, 0, st>>>(X, B.p, h->n, tab, n_sat, it0, it1, dt, thresh, prev.p, out_iter, trace, trace_ent);
                else k_sepal_global<4, Tab32><<<gb, SEPAL_T, 0, st>>>(X, B.p, h->n, tab, n_sat, it0, it1, dt, thresh, prev.p, out_iter, trace, trace_ent);
            } else {
                const Tab16 tab{h->tab16.p};
                if (h->K == 6) k_sepal_global<6, Tab16><<<gb, SEPAL_T, 0, st>>>(X, B.p, h->n, tab, n_sat, it0, it1, dt, thresh, prev.p, out_iter, trace, trace_ent);
                else k_sepal_global<4, Tab16><<<gb, SEPAL_T, 0, st>>>(X, B.p, h->n, tab, n_sat, it0, it1, dt, thresh, prev.p, out_iter, trace, trace_ent);
            }
        }
        SQGR_HIP(hipGetLastError());
        if (it1 < n_iter && !trace) {  // every gene stopped: the remaining chunks would return at once
            SQGR_HIP(hipMemcpyAsync(host.data(), out_iter, (size_t)gb * 4, hipMemcpyDeviceToHost, st));
            SQGR_HIP(hipStreamSynchronize(st));
            if (std::all_of(host.begin(), host.end(), [](int32_t v) { return v >= 0; })) break;
        }
    }
    if (trace && !h->lds && (n_iter & 1))  // global route: after an odd number of sweeps the vector is in B
        SQGR_HIP(hipMemcpyAsync(X, B.p, (size_t)h->n * 8, hipMemcpyDeviceToDevice, st));
    SQGR_HIP(hipStreamSynchronize(st));  // B and prev are released on return
    return SQGR_OK;
}

int check_columns(const sqgr_sepal* h, const sqgr_matrix* m, const int32_t* cols, int64_t G) {
    SQGR_REQUIRE(m->ctx == h->ctx, "matrix belongs to a different context");
    SQGR_REQUIRE(m->n_rows == h->n, "matrix has %lld rows, the lattice %lld spots", (long long)m->n_rows, (long long)h->n);
    SQGR_REQUIRE(m->cols_pending <= 0, "matrix columns are still being uploaded");
    for (int64_t k = 0; k < G; ++k)
        SQGR_REQUIRE(cols[k] >= 0 && cols[k] < m->n_cols, "cols[%lld]=%d outside the matrix (%lld columns)", (long long)k, cols[k],
                     (long long)m->n_cols);
    return SQGR_OK;
}

}  // namespace

int sqgr_sepal_create(sqgr_ctx* ctx, int64_t n, int32_t max_neighs, const int32_t* sat, int64_t n_sat, const int32_t* nbr,
                      const int32_t* unsat, const int32_t* src, int64_t n_unsat, sqgr_sepal** out) {
    SQGR_REQUIRE(ctx && sat && nbr && out && (n_unsat == 0 || (unsat && src)), "null argument");
    *out = nullptr;
    SQGR_REQUIRE(max_neighs == 4 || max_neighs == 6, "max_neighs=%d (4 or 6)", max_neighs);
    SQGR_REQUIRE(n >= 1 && n <= INT32_MAX, "n=%lld", (long long)n);
    SQGR_REQUIRE(n_sat >= 1 && n_unsat >= 0 && n_sat + n_unsat == n, "n_sat=%lld + n_unsat=%lld != n=%lld", (long long)n_sat,
                 (long long)n_unsat, (long long)n);
    const int K = max_neighs;
    std::vector<int32_t> rows((size_t)n * 8, 0);
    std::vector<uint8_t> seen((size_t)n, 0);
    auto put = [&](int64_t spot, int64_t p) {  // spot moves with the d2 of saturated position p
        int32_t* r = &rows[(size_t)spot * 8];
        r[0] = sat[p];
        for (int k = 0; k < K; ++k) r[1 + k] = nbr[p * K + k];
    };
    for (int64_t p = 0; p < n_sat; ++p) {
        SQGR_REQUIRE(sat[p] >= 0 && sat[p] < n && !seen[sat[p]], "sat[%lld]=%d out of range or repeated", (long long)p, sat[p]);
        seen[sat[p]] = 1;
        for (int k = 0; k < K; ++k)
            SQGR_REQUIRE(nbr[p * K + k] >= 0 && nbr[p * K + k] < n, "nbr[%lld][%d]=%d out of range", (long long)p, k, nbr[p * K + k]);
        put(sat[p], p);
    }
    for (int64_t q = 0; q < n_unsat; ++q) {
        SQGR_REQUIRE(unsat[q] >= 0 && unsat[q] < n && !seen[unsat[q]], "unsat[%lld]=%d out of range or repeated", (long long)q, unsat[q]);
        SQGR_REQUIRE(src[q] >= 0 && src[q] < n_sat, "src[%lld]=%d is no position in sat", (long long)q, src[q]);
        seen[unsat[q]] = 1;
        put(unsat[q], src[q]);
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    sqgr_sepal* h = new sqgr_sepal();
    h->ctx = ctx;
    h->n = n;
    h->n_sat = n_sat;
    h->K = K;
    h->lds = n <= SEPAL_LDS_MAX_SPOTS;
    h->wide = n > 65536;
    if (h->lds) {
        const int64_t per = ceil_div(n, SEPAL_T);
        h->spt = per <= 8 ? 8 : per <= 16 ? 16 : 24;
    }
    int rc = SQGR_OK;
    hipStream_t st = ctx->stream;
    if (h->wide) {
        if ((rc = h->tab32.alloc((size_t)n * 2))) {
            delete h;
            return rc;
        }
        const hipError_t e = hipMemcpyAsync(h->tab32.p, rows.data(), (size_t)n * 32, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) rc = hipStreamSynchronize(st) == hipSuccess ? SQGR_OK : SQGR_ERR_HIP;
        else rc = SQGR_ERR_HIP;
    } else {
        std::vector<uint16_t> r16((size_t)n * 8);
        for (size_t i = 0; i < r16.size(); ++i) r16[i] = (uint16_t)rows[i];
        if ((rc = h->tab16.alloc((size_t)n))) {
            delete h;
            return rc;
        }
        const hipError_t e = hipMemcpyAsync(h->tab16.p, r16.data(), (size_t)n * 16, hipMemcpyHostToDevice, st);
        rc = (e == hipSuccess && hipStreamSynchronize(st) == hipSuccess) ? SQGR_OK : SQGR_ERR_HIP;
    }
    if (rc == SQGR_OK) rc = h->counter.alloc(1);
    if (rc != SQGR_OK) {
        if (rc == SQGR_ERR_HIP) set_error("sqgr_sepal_create: uploading the lattice failed");
        delete h;
        return rc;
    }
    *out = h;
    return SQGR_OK;
}

int sqgr_sepal_run(sqgr_sepal* h, const sqgr_matrix* m, const int32_t* cols, int64_t G, int32_t n_iter, double dt, double thresh,
                   int32_t* out_iter) {
    SQGR_REQUIRE(h && m && out_iter && (G == 0 || cols), "null argument");
    SQGR_REQUIRE(G >= 0 && n_iter >= 0, "G=%lld, n_iter=%d", (long long)G, n_iter);
    SQGR_TRY(check_columns(h, m, cols, G));
    if (G == 0) return SQGR_OK;
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SQGR_TRY(m->ensure_by_column());
    DevBuf<int32_t> d_cols, d_iter;
    SQGR_TRY(d_cols.alloc((size_t)G));
    SQGR_TRY(d_iter.alloc((size_t)G));
    SQGR_HIP(hipMemcpyAsync(d_cols.p, cols, (size_t)G * 4, hipMemcpyHostToDevice, st));
    // genes per batch: as many as 512 MB of expanded columns hold; run_batch cuts the sweeps into launches
    const int64_t gb = std::min<int64_t>({G, std::max<int64_t>(1, ((int64_t)512 << 20) / (h->n * 8)), 65535});
    DevBuf<double> X;
    SQGR_TRY(X.alloc_pooled((size_t)gb * h->n));
    for (int64_t g0 = 0; g0 < G; g0 += gb) {
        const int gc = (int)std::min<int64_t>(gb, G - g0);
        {
            LaunchTimer t(ctx, "sepal_expand");
            SQGR_HIP(expand_column_list(m, d_cols.p + g0, gc, X.p, st));
        }
        SQGR_TRY(run_batch(h, X.p, gc, n_iter, dt, thresh, d_iter.p + g0, 0, nullptr));  // synchronous: X is reused by the next batch
    }
    SQGR_HIP(hipMemcpyAsync(out_iter, d_iter.p, (size_t)G * 4, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_sepal_trace(sqgr_sepal* h, const sqgr_matrix* m, int32_t col, int32_t n_steps, double dt, double* out_conc, double* out_ent) {
    SQGR_REQUIRE(h && m, "null argument");
    SQGR_REQUIRE(n_steps >= 0, "n_steps=%d", n_steps);
    SQGR_TRY(check_columns(h, m, &col, 1));
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SQGR_TRY(m->ensure_by_column());
    DevBuf<int32_t> d_col, d_iter;
    DevBuf<double> X, ent;
    SQGR_TRY(d_col.alloc(1));
    SQGR_TRY(d_iter.alloc(1));
    SQGR_TRY(X.alloc((size_t)h->n));
    SQGR_TRY(ent.alloc((size_t)std::max(n_steps, 1)));
    SQGR_HIP(hipMemcpyAsync(d_col.p, &col, 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(expand_column_list(m, d_col.p, 1, X.p, st));
    SQGR_TRY(run_batch(h, X.p, 1, n_steps, dt, 0.0, d_iter.p, 1, ent.p));
    if (out_conc) SQGR_HIP(hipMemcpyAsync(out_conc, X.p, (size_t)h->n * 8, hipMemcpyDeviceToHost, st));
    if (out_ent && n_steps > 0) SQGR_HIP(hipMemcpyAsync(out_ent, ent.p, (size_t)n_steps * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    return SQGR_OK;
}

int sqgr_sepal_destroy(sqgr_sepal* h) {
    if (!h) return SQGR_OK;
    (void)hipSetDevice(h->ctx->device);
    delete h;
    return SQGR_OK;
}
