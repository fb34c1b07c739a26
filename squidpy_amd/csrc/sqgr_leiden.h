// libsqgr: what sqgr_leiden.hip (one graph) and sqgr_leiden_multiplex.hip (two layers over the same vertices) share: the constants of
// the contract, the hash and the priority of the independent set, the candidate order, the table insert, and the kernels that see one
// CSR at a time (row sums, the input check, tot, the split sums of Q, renumbering and the coarse CSR).  Every kernel here is one
// layer's; the host driver that both run (sqgr_leiden_driver.h) launches them once per layer.
#ifndef SQGR_LEIDEN_H
#define SQGR_LEIDEN_H

#include "sqgr_common.h"

#include <algorithm>
#include <vector>

namespace sqgr {
namespace {

constexpr int LD_T = 256;
constexpr int LD_WAVES = LD_T / 64;
constexpr int LD_CAP = 128;         // stored entries of a row up to which its table is on chip
constexpr int LD_SLOTS = 256;       // slots of a wave's LDS table: a row of LD_CAP entries fills at most (LD_CAP + 1) / LD_SLOTS of it
constexpr int LD_WEIGHT_BITS = 24;  // the caller's quantisation: q = max(1, rint(w / w_max * 2^24))
constexpr int LD_SWEEP_CAP = 1024;  // sweeps of one local moving or refinement phase
constexpr int LD_ITER_CAP = 16;     // iterations when n_iterations < 0

__host__ __device__ inline uint32_t ld_hash(uint32_t v, uint32_t s) {
    uint32_t x = v * 0x9E3779B1u + s * 0x85EBCA77u;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__device__ inline bool ld_beats(int32_t v, int32_t u, uint32_t s) {
    const uint32_t hv = ld_hash((uint32_t)v, s), hu = ld_hash((uint32_t)u, s);
    return hv < hu || (hv == hu && v < u);
}

__device__ inline unsigned long long ld_priority(int32_t v, uint32_t s) {  // smaller wins
    return ((unsigned long long)ld_hash((uint32_t)v, s) << 32) | (uint32_t)v;
}

__device__ inline double ld_penalty(double gamma, int64_t a, int64_t b, double two_m) { return gamma * (double)a * (double)b / two_m; }

struct Cand {
    double g;
    int32_t c;  // -1: none
    long long k;
};

__device__ inline bool cand_better(const Cand& a, const Cand& b) {  // a before b
    if (b.c < 0) return a.c >= 0;
    if (a.c < 0) return false;
    return a.g > b.g || (a.g == b.g && a.c < b.c);
}

__device__ inline Cand cand_wave_best(Cand x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        Cand y;
        y.g = __shfl_xor(x.g, o, 64);
        y.c = __shfl_xor(x.c, o, 64);
        y.k = __shfl_xor(x.k, o, 64);
        if (cand_better(y, x)) x = y;
    }
    return x;
}

__device__ inline void tbl_insert(int32_t* keys, unsigned long long* vals, uint32_t nslots, int32_t key, long long w) {
    uint32_t s = ld_hash((uint32_t)key, 0x5bd1e995u) % nslots;
    for (;;) {  // ends: the table has more slots than the row has distinct keys
        const int32_t prev = atomicCAS(&keys[s], -1, key);
        if (prev == -1 || prev == key) {
            atomicAdd(&vals[s], (unsigned long long)w);
            return;
        }
        s = s + 1 == nslots ? 0 : s + 1;
    }
}

struct LevelView {
    int64_t n;
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* w;
    const int64_t* k;  // row sums, self loop included
};

struct Acc {  // zeroed by the host where noted
    unsigned long long moves;     // per sweep
    long long sum_in;             // running sum of in_c
    unsigned long long sq[3];     // per sweep: sum of tot_c^2 as sum(lo & 0xffffffff), sum(lo >> 32), sum(hi)
    unsigned long long two_m[2];  // sum(k & 0xffffffff), sum(k >> 32)
    unsigned long long n_long;    // rows of more than LD_CAP entries
    unsigned long long count;     // k_count_flags
};

__device__ inline unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// a wave per row: k[v], erow, the list of long rows (where long_rows is not null), and the split sum of all k
__global__ __launch_bounds__(LD_T) void k_rows(int64_t n, const int64_t* __restrict__ indptr, const int64_t* __restrict__ w,
                                               int64_t* __restrict__ k, int32_t* __restrict__ erow, int32_t* __restrict__ long_rows,
                                               Acc* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)LD_T + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * LD_WAVES;
    for (int64_t v = wave0; v < n; v += n_waves) {
        const int64_t a = indptr[v], b = indptr[v + 1];
        unsigned long long s = 0;
        for (int64_t e = a + lane; e < b; e += 64) {
            s += (unsigned long long)w[e];
            erow[e] = (int32_t)v;
        }
        s = wave_sum(s);
        if (lane == 0) {
            k[v] = (int64_t)s;
            atomicAdd(&acc->two_m[0], s & 0xffffffffull);
            atomicAdd(&acc->two_m[1], s >> 32);
            if (long_rows && b - a > LD_CAP) long_rows[atomicAdd(&acc->n_long, 1ull)] = (int32_t)v;  // the list's order decides nothing
        }
    }
}

__global__ __launch_bounds__(LD_T) void k_widen(const int32_t* __restrict__ w32, int64_t nnz, int64_t* __restrict__ w) {
    for (int64_t e = blockIdx.x * (int64_t)LD_T + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * LD_T) w[e] = w32[e];
}

// flags: [0] no mirror entry of equal weight, [1] row not strictly increasing, [2] self loop, [3] weight < 1, [4] index outside [0, n)
__global__ __launch_bounds__(LD_T) void k_check(int64_t n, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                const int32_t* __restrict__ w32, const int32_t* __restrict__ erow, int64_t nnz,
                                                int* __restrict__ flags) {
    for (int64_t e = blockIdx.x * (int64_t)LD_T + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * LD_T) {
        const int32_t r = erow[e], c = indices[e];
        if (c < 0 || c >= n) {
            flags[4] = 1;
            continue;
        }
        if (w32[e] < 1) flags[3] = 1;
        if (e > indptr[r] && indices[e - 1] >= c) flags[1] = 1;
        if (r == c) {
            flags[2] = 1;
            continue;
        }
        int64_t lo = indptr[c], hi = indptr[c + 1];
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (indices[mid] < r) lo = mid + 1; else hi = mid;
        }
        if (lo >= end || indices[lo] != r || w32[lo] != w32[e]) flags[0] = 1;
    }
}

__global__ __launch_bounds__(LD_T) void k_iota(int64_t n, int32_t* __restrict__ x) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) x[i] = (int32_t)i;
}

__global__ __launch_bounds__(LD_T) void k_tot(int64_t n, const int32_t* __restrict__ comm, const int64_t* __restrict__ k,
                                              int64_t* __restrict__ tot) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T)
        if (k[i]) atomicAdd((unsigned long long*)&tot[comm[i]], (unsigned long long)k[i]);
}

__global__ __launch_bounds__(LD_T) void k_sumsq(int64_t n, const int64_t* __restrict__ tot, Acc* __restrict__ acc) {
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) {
        const unsigned long long t = (unsigned long long)tot[i], lo = t * t, hi = __umul64hi(t, t);
        a0 += lo & 0xffffffffull;
        a1 += lo >> 32;
        a2 += hi;
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if ((threadIdx.x & 63) == 0) {
        if (a0) atomicAdd(&acc->sq[0], a0);
        if (a1) atomicAdd(&acc->sq[1], a1);
        if (a2) atomicAdd(&acc->sq[2], a2);
    }
}

// sum of the weights of the entries whose ends share a community (self loops included): sum_c in_c
__global__ __launch_bounds__(LD_T) void k_sum_in(int64_t nnz, const int32_t* __restrict__ erow, const int32_t* __restrict__ indices,
                                                 const int64_t* __restrict__ w, const int32_t* __restrict__ comm, Acc* __restrict__ acc) {
    unsigned long long s = 0;
    for (int64_t e = blockIdx.x * (int64_t)LD_T + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * LD_T)
        if (comm[erow[e]] == comm[indices[e]]) s += (unsigned long long)w[e];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)&acc->sum_in, s);
}

// a wave per row: the refinement's start, every vertex alone
__global__ __launch_bounds__(LD_T) void k_refine_init(LevelView L, const int32_t* __restrict__ comm, int32_t* __restrict__ rcomm,
                                                      int64_t* __restrict__ rtot, int64_t* __restrict__ rext, int32_t* __restrict__ rsize,
                                                      int64_t* __restrict__ vext) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)LD_T + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * LD_WAVES;
    for (int64_t v = wave0; v < L.n; v += n_waves) {
        const int32_t C = comm[v];
        unsigned long long s = 0;
        for (int64_t e = L.indptr[v] + lane; e < L.indptr[v + 1]; e += 64) {
            const int32_t u = L.indices[e];
            if (u != v && comm[u] == C) s += (unsigned long long)L.w[e];
        }
        s = wave_sum(s);
        if (lane == 0) {
            rcomm[v] = (int32_t)v;
            rtot[v] = L.k[v];
            rext[v] = (int64_t)s;
            vext[v] = (int64_t)s;
            rsize[v] = 1;
        }
    }
}

__global__ __launch_bounds__(LD_T) void k_flag(int64_t n, const int32_t* __restrict__ ids, int32_t* __restrict__ flags) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) flags[ids[i]] = 1;
}

__global__ __launch_bounds__(LD_T) void k_count_flags(int64_t n, const int32_t* __restrict__ flags, Acc* __restrict__ acc) {
    unsigned long long s = 0;
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) s += flags[i] != 0;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc->count, s);
}

// nr[v] = new id of v's refined community; pmin[C] = smallest new id inside community C
__global__ __launch_bounds__(LD_T) void k_relabel(int64_t n, const int32_t* __restrict__ rcomm, const int32_t* __restrict__ newid,
                                                  const int32_t* __restrict__ comm, int32_t* __restrict__ nr, int32_t* __restrict__ pmin) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) {
        const int32_t r = newid[rcomm[i]];
        nr[i] = r;
        atomicMin(&pmin[comm[i]], r);
    }
}

__global__ __launch_bounds__(LD_T) void k_coarse_comm(int64_t n, const int32_t* __restrict__ nr, const int32_t* __restrict__ comm,
                                                      const int32_t* __restrict__ pmin, int32_t* __restrict__ ccomm) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) ccomm[nr[i]] = pmin[comm[i]];
}

__global__ __launch_bounds__(LD_T) void k_edge_keys(int64_t nnz, const int32_t* __restrict__ erow, const int32_t* __restrict__ indices,
                                                    const int32_t* __restrict__ nr, uint64_t* __restrict__ keys) {
    for (int64_t e = blockIdx.x * (int64_t)LD_T + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * LD_T)
        keys[e] = ((uint64_t)(uint32_t)nr[erow[e]] << 32) | (uint32_t)nr[indices[e]];
}

__global__ __launch_bounds__(LD_T) void k_coarse_cols(int64_t m, const uint64_t* __restrict__ ukeys, int32_t* __restrict__ indices) {
    for (int64_t j = blockIdx.x * (int64_t)LD_T + threadIdx.x; j < m; j += (int64_t)gridDim.x * LD_T)
        indices[j] = (int32_t)(ukeys[j] & 0xffffffffull);
}

// indptr[r] = first position whose key is at least (r, 0), r = 0 .. n_rows
__global__ __launch_bounds__(LD_T) void k_coarse_indptr(int64_t n_rows, int64_t m, const uint64_t* __restrict__ ukeys,
                                                        int64_t* __restrict__ indptr) {
    for (int64_t r = blockIdx.x * (int64_t)LD_T + threadIdx.x; r <= n_rows; r += (int64_t)gridDim.x * LD_T) {
        const uint64_t key = (uint64_t)r << 32;
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ukeys[mid] < key) lo = mid + 1; else hi = mid;
        }
        indptr[r] = lo;
    }
}

__global__ __launch_bounds__(LD_T) void k_compose(int64_t n, const int32_t* __restrict__ nr, int32_t* __restrict__ node_of) {
    for (int64_t i = blockIdx.x * (int64_t)LD_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * LD_T) node_of[i] = nr[node_of[i]];
}

struct LevelBuf {
    DevBuf<int64_t> indptr, w, k;
    DevBuf<int32_t> indices, erow;
    int64_t n = 0, nnz = 0;
    int alloc(int64_t n_cap, int64_t nnz_cap) {
        SQGR_TRY(indptr.alloc((size_t)n_cap + 1));
        SQGR_TRY(k.alloc((size_t)n_cap));
        SQGR_TRY(w.alloc((size_t)nnz_cap));
        SQGR_TRY(indices.alloc((size_t)nnz_cap));
        SQGR_TRY(erow.alloc((size_t)nnz_cap));
        return SQGR_OK;
    }
    LevelView view() const { return LevelView{n, indptr.p, indices.p, w.p, k.p}; }
};

inline double ld_quality(int64_t sum_in, unsigned __int128 sumsq, double gamma, int64_t two_m) {
    const double m2 = (double)two_m;
    return (double)sum_in / m2 - gamma * ((double)sumsq / (m2 * m2));
}

inline unsigned __int128 ld_join_sq(const Acc& h) {
    return (unsigned __int128)h.sq[0] + ((unsigned __int128)h.sq[1] << 32) + ((unsigned __int128)h.sq[2] << 64);
}

// communities numbered by size descending, ties by smallest member; returns K
inline int64_t canonical_labels(const std::vector<int32_t>& ids, int64_t id_range, int32_t* out) {
    const int64_t n = (int64_t)ids.size();
    std::vector<int64_t> size((size_t)id_range, 0), first((size_t)id_range, -1);
    for (int64_t i = 0; i < n; ++i) {
        if (first[ids[i]] < 0) first[ids[i]] = i;
        ++size[ids[i]];
    }
    std::vector<int32_t> order;
    for (int64_t c = 0; c < id_range; ++c)
        if (size[c]) order.push_back((int32_t)c);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return size[a] != size[b] ? size[a] > size[b] : first[a] < first[b]; });
    std::vector<int32_t> rank((size_t)id_range, -1);
    for (size_t r = 0; r < order.size(); ++r) rank[order[r]] = (int32_t)r;
    for (int64_t i = 0; i < n; ++i) out[i] = rank[ids[i]];
    return (int64_t)order.size();
}

}  // namespace
}  // namespace sqgr

#endif  // SQGR_LEIDEN_H
