// libsqgr: sqgr_leiden_multiplex — Leiden on two layers over the same vertices (a latent and a spatial graph): what the reference's
// `calculate_niche_spatialleiden` gets from spatialleiden / leidenalg's optimise_partition_multiplex (gr/_niche.py:466-620), as the
// deterministic synchronous variant of sqgr_leiden.hip.  One partition, one RBConfiguration quality per layer, unnormalised:
//     Q = sum_l a_l sum_c (in^l_c - gamma_l (tot^l_c)^2 / 2m_l),   a_0 = 1, a_1 = layer_ratio.
// It is sqgr_leiden.hip with these changes and nothing else:
//   integers      every k^l_v, k^l_{v,c}, tot^l_c, in^l_c, 2m_l and W^l_c is an exact int64 per layer, on every level.
//   gain          g_l(v, c) = (double)k^l_vc - gamma_l * (double)k^l_v * (double)(tot^l_c - [c == comm(v)] k^l_v) / (double)two_m_l, left
//                 to right, exactly +0.0 for a layer with 2m_l = 0;  gain = g_0 + layer_ratio * g_1: the product rounded, then the sum
//                 (no FMA).  Every other floating-point test (well connected, crowded gain, Q at the cap) mixes its two per-layer
//                 terms the same way.
//   candidates    the communities of v's neighbours in either layer, plus its own: ONE table keyed by community with two 64-bit sums
//                 per slot (20 bytes), so a community reachable through both layers is one candidate.
//   independent   a mover yields to a wanting neighbour in either layer: k_apply walks both rows.
//   overshoot     `claimed` is kept per layer; the crowded gain uses tot^l_c + W^l_c - k^l_v in each layer.
//   refinement    v is well connected when (x_0 - p_0) + layer_ratio * (x_1 - p_1) >= 0, x_l = (double)k^l_{v, C - v}, p_l = gamma_l *
//                 (double)k^l_v * (double)(tot^l_C - k^l_v) / two_m_l; the same for a target S; S must be adjacent in a layer.
//   aggregation   one coarse CSR per layer over the same refined-community numbering; a self loop carries in^l_c.
// A row takes the on-chip path when its stored entries in layer 0 plus those in layer 1 are <= LD_CAP, else the global-memory path
// with a table of twice that sum at 2 * (indptr0[v] + indptr1[v]).  Both paths form the same integers and pick by the same order.
#include "sqgr_leiden.h"

#include <rocprim/rocprim.hpp>

#include <cmath>
#include <numeric>

namespace sqgr {
namespace {

constexpr int MX_LAYERS = 2;
constexpr int MX_STATS = 10;

struct MxParams {
    double gamma[MX_LAYERS];
    double two_m[MX_LAYERS];  // 0.0: the layer has no weight, its terms are +0.0
    double ratio;
};

// (double)x - gamma_l * (double)a * (double)b / two_m_l
__host__ __device__ inline double mx_term(const MxParams& P, int l, long long x, int64_t a, int64_t b) {
    return P.two_m[l] == 0.0 ? 0.0 : (double)x - P.gamma[l] * (double)a * (double)b / P.two_m[l];
}

__host__ __device__ inline double mx_mix(const MxParams& P, double t0, double t1) {
    const double scaled = P.ratio * t1;  // rounded on its own
    return t0 + scaled;
}

struct MxLevel {
    LevelView L[MX_LAYERS];  // the same n
};

struct MxRefine {  // refinement state; all null in local moving
    const int32_t* rcomm;
    const int32_t* rsize;
    const int64_t* rtot[MX_LAYERS];
    const int64_t* rext[MX_LAYERS];  // weight between a refined community and the rest of its community
    const int64_t* vext[MX_LAYERS];  // weight between a vertex and the rest of its community
};

struct MxMove {  // local moving only
    int64_t* k_best[MX_LAYERS];
    double* g_own;
    int64_t* tot_target[MX_LAYERS];
    unsigned long long* claimed[MX_LAYERS];  // per community and layer: sum of k^l_v over the vertices that want into it
    unsigned long long* first;               // per community: the smallest priority among them
};

struct Cand2 {
    double g;
    int32_t c;  // -1: none
    long long k[MX_LAYERS];
};

__device__ inline bool cand2_better(const Cand2& a, const Cand2& b) {  // a before b: the order of cand_better
    if (b.c < 0) return a.c >= 0;
    if (a.c < 0) return false;
    return a.g > b.g || (a.g == b.g && a.c < b.c);
}

__device__ inline Cand2 cand2_wave_best(Cand2 x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        Cand2 y;
        y.g = __shfl_xor(x.g, o, 64);
        y.c = __shfl_xor(x.c, o, 64);
        y.k[0] = __shfl_xor(x.k[0], o, 64);
        y.k[1] = __shfl_xor(x.k[1], o, 64);
        if (cand2_better(y, x)) x = y;
    }
    return x;
}

// want[v] = the community v wants to move to, or -1;  dk_l[v] = k^l_{v,want} - k^l_{v,own} (local moving), k^l_{v,want} (refinement).
// LONG: one block per row of `rows`, tables of 2 * len slots at 2 * (indptr0[v] + indptr1[v]) in gkeys / gvals0 / gvals1, len the
// row's entries in both layers.  !LONG: one wave per row, rows of len > LD_CAP are skipped.
template <bool LONG, bool REFINE>
__global__ __launch_bounds__(LD_T) void k_best2(MxLevel G, const int32_t* __restrict__ comm, const int64_t* __restrict__ tot0,
                                                const int64_t* __restrict__ tot1, MxRefine R, MxParams P, const int32_t* __restrict__ rows,
                                                int64_t n_rows, int32_t* __restrict__ gkeys, unsigned long long* __restrict__ gvals0,
                                                unsigned long long* __restrict__ gvals1, int32_t* __restrict__ want, int64_t* __restrict__ dk0,
                                                int64_t* __restrict__ dk1, MxMove M, uint32_t sweep) {
    __shared__ int32_t s_keys[LONG ? 1 : LD_WAVES * LD_SLOTS];
    __shared__ unsigned long long s_vals0[LONG ? 1 : LD_WAVES * LD_SLOTS];
    __shared__ unsigned long long s_vals1[LONG ? 1 : LD_WAVES * LD_SLOTS];
    __shared__ double s_g[LD_WAVES], s_gown[LD_WAVES];
    __shared__ int32_t s_c[LD_WAVES];
    __shared__ long long s_k[MX_LAYERS][LD_WAVES], s_kown[MX_LAYERS][LD_WAVES];
    const int64_t* const tot[MX_LAYERS] = {tot0, tot1};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = LONG ? (int)threadIdx.x : lane, gsize = LONG ? LD_T : 64;
    const int64_t n_items = LONG ? n_rows : G.L[0].n;
    const int64_t per_block = LONG ? 1 : LD_WAVES;
    for (int64_t base = blockIdx.x * per_block; base < n_items; base += (int64_t)gridDim.x * per_block) {  // uniform per block
        const int64_t item = LONG ? base : base + wave;
        int64_t v = -1, a[MX_LAYERS] = {0, 0}, b[MX_LAYERS] = {0, 0};
        if (item < n_items) {
            v = LONG ? (int64_t)rows[item] : item;
            for (int l = 0; l < MX_LAYERS; ++l) {
                a[l] = G.L[l].indptr[v];
                b[l] = G.L[l].indptr[v + 1];
            }
            if (!LONG && (b[0] - a[0]) + (b[1] - a[1]) > LD_CAP) v = -1;  // the long kernel's row
        }
        const int64_t len = (b[0] - a[0]) + (b[1] - a[1]), at = 2 * (a[0] + a[1]);
        int32_t* keys = LONG ? gkeys + at : s_keys + wave * LD_SLOTS;
        unsigned long long* vals[MX_LAYERS] = {LONG ? gvals0 + at : s_vals0 + wave * LD_SLOTS, LONG ? gvals1 + at : s_vals1 + wave * LD_SLOTS};
        const uint32_t nslots = LONG ? (uint32_t)(2 * len) : (uint32_t)LD_SLOTS;
        int32_t own = -1, C = -1;
        int64_t kv[MX_LAYERS] = {0, 0}, totC[MX_LAYERS] = {0, 0};
        bool act = v >= 0;
        if (act) {
            C = comm[v];
            own = REFINE ? R.rcomm[v] : C;
            for (int l = 0; l < MX_LAYERS; ++l) kv[l] = G.L[l].k[v];
            if (REFINE) {
                for (int l = 0; l < MX_LAYERS; ++l) totC[l] = tot[l][C];
                act = R.rsize[own] == 1 &&
                      mx_mix(P, mx_term(P, 0, R.vext[0][v], kv[0], totC[0] - kv[0]), mx_term(P, 1, R.vext[1][v], kv[1], totC[1] - kv[1])) >= 0.0;
            }
        }
        if (act)
            for (uint32_t s = gtid; s < nslots; s += gsize) {
                keys[s] = -1;
                vals[0][s] = 0;
                vals[1][s] = 0;
            }
        __syncthreads();
        if (act) {
            if (gtid == 0) tbl_insert(keys, vals[0], nslots, own, 0);
            for (int l = 0; l < MX_LAYERS; ++l)
                for (int64_t e = a[l] + gtid; e < b[l]; e += gsize) {
                    const int32_t u = G.L[l].indices[e];
                    if (u == v) continue;
                    if (REFINE) {
                        if (comm[u] != C) continue;
                        tbl_insert(keys, vals[l], nslots, R.rcomm[u], G.L[l].w[e]);
                    } else {
                        tbl_insert(keys, vals[l], nslots, comm[u], G.L[l].w[e]);
                    }
                }
        }
        __syncthreads();
        Cand2 best{0.0, -1, {0, 0}};
        double g_own = -INFINITY;
        long long k_own[MX_LAYERS] = {0, 0};
        if (act)
            for (uint32_t s = gtid; s < nslots; s += gsize) {
                const int32_t c = keys[s];
                if (c < 0) continue;
                Cand2 x;
                x.c = c;
                x.k[0] = (long long)vals[0][s];
                x.k[1] = (long long)vals[1][s];
                if (c == own) {
                    const int64_t t0 = (REFINE ? R.rtot[0][c] : tot[0][c]) - kv[0], t1 = (REFINE ? R.rtot[1][c] : tot[1][c]) - kv[1];
                    x.g = mx_mix(P, mx_term(P, 0, x.k[0], kv[0], t0), mx_term(P, 1, x.k[1], kv[1], t1));
                    g_own = x.g;
                    k_own[0] = x.k[0];
                    k_own[1] = x.k[1];
                } else if (REFINE) {
                    const int64_t ts0 = R.rtot[0][c], ts1 = R.rtot[1][c];
                    if (!(mx_mix(P, mx_term(P, 0, R.rext[0][c], ts0, totC[0] - ts0), mx_term(P, 1, R.rext[1][c], ts1, totC[1] - ts1)) >= 0.0))
                        continue;  // the target is not well connected
                    x.g = mx_mix(P, mx_term(P, 0, x.k[0], kv[0], ts0), mx_term(P, 1, x.k[1], kv[1], ts1));
                } else {
                    x.g = mx_mix(P, mx_term(P, 0, x.k[0], kv[0], tot[0][c]), mx_term(P, 1, x.k[1], kv[1], tot[1][c]));
                }
                if (cand2_better(x, best)) best = x;
            }
        best = cand2_wave_best(best);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            g_own = fmax(g_own, __shfl_xor(g_own, o, 64));
            k_own[0] += __shfl_xor(k_own[0], o, 64);
            k_own[1] += __shfl_xor(k_own[1], o, 64);
        }
        if (LONG) {
            if (lane == 0) {
                s_g[wave] = best.g;
                s_c[wave] = best.c;
                s_gown[wave] = g_own;
                for (int l = 0; l < MX_LAYERS; ++l) {
                    s_k[l][wave] = best.k[l];
                    s_kown[l][wave] = k_own[l];
                }
            }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 1; i < LD_WAVES; ++i) {
                    const Cand2 y{s_g[i], s_c[i], {s_k[0][i], s_k[1][i]}};
                    if (cand2_better(y, best)) best = y;
                    g_own = fmax(g_own, s_gown[i]);
                    k_own[0] += s_kown[0][i];
                    k_own[1] += s_kown[1][i];
                }
        }
        if (v >= 0 && gtid == 0) {
            const bool move = act && best.c >= 0 && best.c != own && best.g > g_own;
            want[v] = move ? best.c : -1;
            dk0[v] = move ? (REFINE ? best.k[0] : best.k[0] - k_own[0]) : 0;
            dk1[v] = move ? (REFINE ? best.k[1] : best.k[1] - k_own[1]) : 0;
            if (!REFINE && move) {  // what k_apply2's overshoot rule needs: the claims on the target and the sweep's own numbers
                M.g_own[v] = g_own;
                for (int l = 0; l < MX_LAYERS; ++l) {
                    M.k_best[l][v] = best.k[l];
                    M.tot_target[l][v] = tot[l][best.c];
                    if (kv[l]) atomicAdd(&M.claimed[l][best.c], (unsigned long long)kv[l]);
                }
                atomicMin(&M.first[best.c], ld_priority((int32_t)v, sweep));
            }
        }
        __syncthreads();  // the tables and s_* are reused by the next row
    }
}

// a wave per row: the vertex moves unless a neighbour in either layer that wants to move has the better priority
template <bool REFINE>
__global__ __launch_bounds__(LD_T) void k_apply2(MxLevel G, const int32_t* __restrict__ want, const int64_t* __restrict__ dk0,
                                                 const int64_t* __restrict__ dk1, uint32_t sweep, int32_t* __restrict__ comm,
                                                 int64_t* __restrict__ tot0, int64_t* __restrict__ tot1, int32_t* __restrict__ rsize,
                                                 int64_t* __restrict__ rext0, int64_t* __restrict__ rext1, const int64_t* __restrict__ vext0,
                                                 const int64_t* __restrict__ vext1, Acc* __restrict__ acc, MxMove M, MxParams P) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)LD_T + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * LD_WAVES;
    for (int64_t v = wave0; v < G.L[0].n; v += n_waves) {
        const int32_t t = want[v];
        if (t < 0) continue;  // uniform per wave
        const int64_t kv0 = G.L[0].k[v], kv1 = G.L[1].k[v];
        if (!REFINE && M.first[t] != ld_priority((int32_t)v, sweep)) {
            // not the first of those that want into t: moves only if its gain still beats staying after ALL of them have joined
            const int64_t crowded0 = M.tot_target[0][v] + (int64_t)M.claimed[0][t] - kv0;
            const int64_t crowded1 = M.tot_target[1][v] + (int64_t)M.claimed[1][t] - kv1;
            if (!(mx_mix(P, mx_term(P, 0, M.k_best[0][v], kv0, crowded0), mx_term(P, 1, M.k_best[1][v], kv1, crowded1)) > M.g_own[v])) continue;
        }
        bool lose = false;
        for (int l = 0; l < MX_LAYERS; ++l)
            for (int64_t e = G.L[l].indptr[v] + lane; e < G.L[l].indptr[v + 1]; e += 64) {
                const int32_t u = G.L[l].indices[e];
                if (u != v && want[u] >= 0 && !ld_beats((int32_t)v, u, sweep)) lose = true;
            }
        if (__any(lose)) continue;
        if (lane == 0) {
            const int32_t old = comm[v];
            comm[v] = t;
            atomicAdd((unsigned long long*)&tot0[t], (unsigned long long)kv0);
            atomicAdd((unsigned long long*)&tot0[old], (unsigned long long)(-kv0));
            atomicAdd((unsigned long long*)&tot1[t], (unsigned long long)kv1);
            atomicAdd((unsigned long long*)&tot1[old], (unsigned long long)(-kv1));
            if (REFINE) {
                atomicAdd(&rsize[t], 1);
                atomicSub(&rsize[old], 1);
                atomicAdd((unsigned long long*)&rext0[t], (unsigned long long)(vext0[v] - 2 * dk0[v]));
                atomicAdd((unsigned long long*)&rext1[t], (unsigned long long)(vext1[v] - 2 * dk1[v]));
            } else {
                atomicAdd((unsigned long long*)&acc[0].sum_in, (unsigned long long)(2 * dk0[v]));
                atomicAdd((unsigned long long*)&acc[1].sum_in, (unsigned long long)(2 * dk1[v]));
            }
            atomicAdd(&acc[0].moves, 1ull);
        }
    }
}

// the rows whose entries in both layers together exceed LD_CAP; the list's order decides nothing
__global__ __launch_bounds__(LD_T) void k_long_rows2(int64_t n, const int64_t* __restrict__ indptr0, const int64_t* __restrict__ indptr1,
                                                     int32_t* __restrict__ long_rows, Acc* __restrict__ acc) {
    for (int64_t v = blockIdx.x * (int64_t)LD_T + threadIdx.x; v < n; v += (int64_t)gridDim.x * LD_T)
        if ((indptr0[v + 1] - indptr0[v]) + (indptr1[v + 1] - indptr1[v]) > LD_CAP) long_rows[atomicAdd(&acc->n_long, 1ull)] = (int32_t)v;
}

struct MxLevelBuf {
    LevelBuf l[MX_LAYERS];
    int64_t n = 0;
    MxLevel view() const { return MxLevel{{l[0].view(), l[1].view()}}; }
};

struct Multiplex {
    sqgr_ctx* ctx;
    hipStream_t st;
    unsigned grid;  // blocks of the grid-stride kernels
    MxParams P;
    int64_t two_m[MX_LAYERS];
    int64_t n0, ecap[MX_LAYERS];
    MxLevelBuf g0, ga, gb;
    DevBuf<int32_t> comm, best_comm, want, rcomm, rsize, flags, newid, nr, pmin, ccomm, node_of, long_rows, tkeys;
    DevBuf<int64_t> tot[MX_LAYERS], dk[MX_LAYERS], rtot[MX_LAYERS], rext[MX_LAYERS], vext[MX_LAYERS], mk_best[MX_LAYERS], mtot_target[MX_LAYERS];
    DevBuf<int64_t> sw_out;
    DevBuf<double> mg_own;
    DevBuf<unsigned long long> mclaimed[MX_LAYERS], mfirst, tvals[MX_LAYERS];
    DevBuf<uint64_t> keys_in, keys_out, ukeys;
    DevBuf<char> temp;
    DevBuf<Acc> acc;  // one per layer; moves, n_long and count live in acc[0]
    DevBuf<int64_t> n_unique;
    int64_t n_long = 0;
    int64_t stat_levels = 0, stat_sweeps = 0, stat_cap_hits = 0;

    unsigned blocks(int64_t items) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, LD_T), grid)); }
    unsigned wave_blocks(int64_t rows) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, LD_WAVES), grid)); }

    int read_acc(Acc* h) {  // Acc[MX_LAYERS]
        SQGR_HIP(hipMemcpyAsync(h, acc.p, MX_LAYERS * sizeof(Acc), hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        return SQGR_OK;
    }

    // k, erow and 2m per layer, and the long rows, of a level whose CSRs are in place
    int prepare(MxLevelBuf& g, Acc* h) {
        for (int l = 0; l < MX_LAYERS; ++l) {
            SQGR_HIP(hipMemsetAsync(&acc.p[l].two_m, 0, 3 * sizeof(unsigned long long), st));  // two_m[2] and n_long
            LaunchTimer t(ctx, "mleiden_rows");
            k_rows<<<wave_blocks(g.n), LD_T, 0, st>>>(g.n, g.l[l].indptr.p, g.l[l].w.p, g.l[l].k.p, g.l[l].erow.p, nullptr, &acc.p[l]);
            SQGR_HIP(hipGetLastError());
        }
        k_long_rows2<<<blocks(g.n), LD_T, 0, st>>>(g.n, g.l[0].indptr.p, g.l[1].indptr.p, long_rows.p, acc.p);
        SQGR_HIP(hipGetLastError());
        SQGR_TRY(read_acc(h));
        n_long = (int64_t)h[0].n_long;
        if (n_long && !tkeys.p) {  // the global tables: two slots per stored entry of both layers of the largest level
            const size_t slots = 2 * (size_t)(ecap[0] + ecap[1]);
            SQGR_TRY(tkeys.alloc_pooled(slots));
            SQGR_TRY(tvals[0].alloc_pooled(slots));
            SQGR_TRY(tvals[1].alloc_pooled(slots));
        }
        return SQGR_OK;
    }

    int rebuild_tot(const MxLevelBuf& g) {
        for (int l = 0; l < MX_LAYERS; ++l) {
            SQGR_HIP(hipMemsetAsync(tot[l].p, 0, (size_t)g.n * 8, st));
            LaunchTimer t(ctx, "mleiden_tot");
            k_tot<<<blocks(g.n), LD_T, 0, st>>>(g.n, comm.p, g.l[l].k.p, tot[l].p);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    template <bool REFINE>
    int sweep(const MxLevelBuf& g, uint32_t s) {
        const MxLevel G = g.view();
        const MxMove M{{mk_best[0].p, mk_best[1].p}, mg_own.p, {mtot_target[0].p, mtot_target[1].p}, {mclaimed[0].p, mclaimed[1].p}, mfirst.p};
        if (!REFINE) {
            SQGR_HIP(hipMemsetAsync(mclaimed[0].p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(mclaimed[1].p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(mfirst.p, 0xff, (size_t)g.n * 8, st));
        }
        const MxRefine R = REFINE ? MxRefine{rcomm.p, rsize.p, {rtot[0].p, rtot[1].p}, {rext[0].p, rext[1].p}, {vext[0].p, vext[1].p}}
                                  : MxRefine{nullptr, nullptr, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
        {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_best" : "mleiden_move_best");
            k_best2<false, REFINE><<<wave_blocks(g.n), LD_T, 0, st>>>(G, comm.p, tot[0].p, tot[1].p, R, P, nullptr, 0, nullptr, nullptr, nullptr, want.p,
                                                                      dk[0].p, dk[1].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        if (n_long) {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_best_long" : "mleiden_move_best_long");
            k_best2<true, REFINE><<<(unsigned)std::min<int64_t>(n_long, grid), LD_T, 0, st>>>(G, comm.p, tot[0].p, tot[1].p, R, P, long_rows.p, n_long,
                                                                                             tkeys.p, tvals[0].p, tvals[1].p, want.p, dk[0].p, dk[1].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_apply" : "mleiden_move_apply");
            if (REFINE)
                k_apply2<true><<<wave_blocks(g.n), LD_T, 0, st>>>(G, want.p, dk[0].p, dk[1].p, s, rcomm.p, rtot[0].p, rtot[1].p, rsize.p, rext[0].p,
                                                                  rext[1].p, vext[0].p, vext[1].p, acc.p, M, P);
            else
                k_apply2<false><<<wave_blocks(g.n), LD_T, 0, st>>>(G, want.p, dk[0].p, dk[1].p, s, comm.p, tot[0].p, tot[1].p, nullptr, nullptr, nullptr,
                                                                   nullptr, nullptr, acc.p, M, P);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    int sumsq(const MxLevelBuf& g) {
        for (int l = 0; l < MX_LAYERS; ++l) {
            LaunchTimer t(ctx, "mleiden_sumsq");
            k_sumsq<<<blocks(g.n), LD_T, 0, st>>>(g.n, tot[l].p, &acc.p[l]);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    // Q = (double)two_m_0 * q_0 + layer_ratio * ((double)two_m_1 * q_1), q_l the single-layer expression, 0 for a layer without weight
    double quality(const Acc* h) const {
        double part[MX_LAYERS];
        for (int l = 0; l < MX_LAYERS; ++l)
            part[l] = two_m[l] ? (double)two_m[l] * ld_quality(h[l].sum_in, ld_join_sq(h[l]), P.gamma[l], two_m[l]) : 0.0;
        return mx_mix(P, part[0], part[1]);
    }

    int local_moving(const MxLevelBuf& g) {
        Acc h[MX_LAYERS];
        for (int l = 0; l < MX_LAYERS; ++l) {
            SQGR_HIP(hipMemsetAsync(&acc.p[l], 0, offsetof(Acc, two_m), st));  // moves, sum_in, sq
            if (g.l[l].nnz) {
                LaunchTimer t(ctx, "mleiden_sum_in");
                k_sum_in<<<blocks(g.l[l].nnz), LD_T, 0, st>>>(g.l[l].nnz, g.l[l].erow.p, g.l[l].indices.p, g.l[l].w.p, comm.p, &acc.p[l]);
                SQGR_HIP(hipGetLastError());
            }
        }
        SQGR_TRY(sumsq(g));
        SQGR_TRY(read_acc(h));
        double best_q = quality(h);
        SQGR_HIP(hipMemcpyAsync(best_comm.p, comm.p, (size_t)g.n * 4, hipMemcpyDeviceToDevice, st));
        bool converged = false;
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p[0].moves, 0, 8, st));
            for (int l = 0; l < MX_LAYERS; ++l) SQGR_HIP(hipMemsetAsync(&acc.p[l].sq, 0, 24, st));
            SQGR_TRY(sweep<false>(g, (uint32_t)s));
            SQGR_TRY(sumsq(g));
            SQGR_TRY(read_acc(h));
            ++stat_sweeps;
            if (!h[0].moves) {
                converged = true;
                break;
            }
            const double q = quality(h);
            if (q > best_q) {
                best_q = q;
                SQGR_HIP(hipMemcpyAsync(best_comm.p, comm.p, (size_t)g.n * 4, hipMemcpyDeviceToDevice, st));
            }
        }
        if (!converged) {  // the cap: the assignment of largest Q seen
            ++stat_cap_hits;
            SQGR_HIP(hipMemcpyAsync(comm.p, best_comm.p, (size_t)g.n * 4, hipMemcpyDeviceToDevice, st));
            SQGR_TRY(rebuild_tot(g));
        }
        return SQGR_OK;
    }

    int count_distinct(int64_t n, const int32_t* ids, int64_t* out) {
        SQGR_HIP(hipMemsetAsync(flags.p, 0, (size_t)n * 4, st));
        SQGR_HIP(hipMemsetAsync(&acc.p[0].count, 0, 8, st));
        k_flag<<<blocks(n), LD_T, 0, st>>>(n, ids, flags.p);
        SQGR_HIP(hipGetLastError());
        k_count_flags<<<blocks(n), LD_T, 0, st>>>(n, flags.p, acc.p);
        SQGR_HIP(hipGetLastError());
        Acc h[MX_LAYERS];
        SQGR_TRY(read_acc(h));
        *out = (int64_t)h[0].count;
        return SQGR_OK;
    }

    int refine(const MxLevelBuf& g) {
        for (int l = 0; l < MX_LAYERS; ++l) {  // rcomm and rsize are written by both launches, with the same values
            LaunchTimer t(ctx, "mleiden_refine_init");
            k_refine_init<<<wave_blocks(g.n), LD_T, 0, st>>>(g.l[l].view(), comm.p, rcomm.p, rtot[l].p, rext[l].p, rsize.p, vext[l].p);
            SQGR_HIP(hipGetLastError());
        }
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p[0].moves, 0, 8, st));
            SQGR_TRY(sweep<true>(g, (uint32_t)s));
            Acc h[MX_LAYERS];
            SQGR_TRY(read_acc(h));
            ++stat_sweeps;
            if (!h[0].moves) break;
        }
        return SQGR_OK;
    }

    int ensure_temp(size_t bytes) { return temp.ensure(std::max<size_t>(bytes, 16)); }

    // one layer's coarse CSR over the numbering nr: parallel entries summed, the inner weight on the self loop
    int coarse_layer(const LevelBuf& g, LevelBuf& out, int64_t nc) {
        const int64_t nnz = g.nnz;
        size_t tb = 0;
        int64_t m = 0;
        if (nnz) {
            k_edge_keys<<<blocks(nnz), LD_T, 0, st>>>(nnz, g.erow.p, g.indices.p, nr.p, keys_in.p);
            SQGR_HIP(hipGetLastError());
            SQGR_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys_in.p, keys_out.p, g.w.p, sw_out.p, (size_t)nnz, 0, 64, st));
            SQGR_TRY(ensure_temp(tb));
            {
                LaunchTimer t(ctx, "mleiden_sort");
                SQGR_HIP(rocprim::radix_sort_pairs(temp.p, tb, keys_in.p, keys_out.p, g.w.p, sw_out.p, (size_t)nnz, 0, 64, st));
            }
            SQGR_HIP(rocprim::reduce_by_key(nullptr, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p, rocprim::plus<int64_t>(),
                                            rocprim::equal_to<uint64_t>(), st));
            SQGR_TRY(ensure_temp(tb));
            {
                LaunchTimer t(ctx, "mleiden_reduce");
                SQGR_HIP(rocprim::reduce_by_key(temp.p, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p,
                                                rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), st));
            }
            SQGR_HIP(hipMemcpyAsync(&m, n_unique.p, 8, hipMemcpyDeviceToHost, st));
            SQGR_HIP(hipStreamSynchronize(st));
            if (m < 0 || m > nnz) {
                set_error("sqgr_leiden_multiplex: reduce_by_key returned %lld groups of %lld entries", (long long)m, (long long)nnz);
                return SQGR_ERR_HIP;
            }
            k_coarse_cols<<<blocks(m), LD_T, 0, st>>>(m, ukeys.p, out.indices.p);
            SQGR_HIP(hipGetLastError());
        }
        k_coarse_indptr<<<blocks(nc + 1), LD_T, 0, st>>>(nc, m, ukeys.p, out.indptr.p);  // m == 0: every row is empty
        SQGR_HIP(hipGetLastError());
        out.n = nc;
        out.nnz = m;
        return SQGR_OK;
    }

    // the refined communities of level g become the nodes of `out`; *n_coarse == g.n: nothing merged and `out` is not built
    int aggregate(const MxLevelBuf& g, MxLevelBuf& out, int64_t* n_coarse) {
        const int64_t n = g.n;
        SQGR_HIP(hipMemsetAsync(flags.p, 0, (size_t)n * 4, st));
        k_flag<<<blocks(n), LD_T, 0, st>>>(n, rcomm.p, flags.p);
        SQGR_HIP(hipGetLastError());
        size_t tb = 0;
        SQGR_HIP(rocprim::exclusive_scan(nullptr, tb, flags.p, newid.p, 0, (size_t)n, rocprim::plus<int32_t>(), st));
        SQGR_TRY(ensure_temp(tb));
        {
            LaunchTimer t(ctx, "mleiden_renumber");
            SQGR_HIP(rocprim::exclusive_scan(temp.p, tb, flags.p, newid.p, 0, (size_t)n, rocprim::plus<int32_t>(), st));
        }
        int32_t last[2];
        SQGR_HIP(hipMemcpyAsync(&last[0], newid.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipMemcpyAsync(&last[1], flags.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        const int64_t nc = (int64_t)last[0] + last[1];
        *n_coarse = nc;
        if (nc == n) return SQGR_OK;
        SQGR_HIP(hipMemsetAsync(pmin.p, 0x7f, (size_t)n * 4, st));
        k_relabel<<<blocks(n), LD_T, 0, st>>>(n, rcomm.p, newid.p, comm.p, nr.p, pmin.p);
        SQGR_HIP(hipGetLastError());
        k_coarse_comm<<<blocks(n), LD_T, 0, st>>>(n, nr.p, comm.p, pmin.p, ccomm.p);
        SQGR_HIP(hipGetLastError());
        k_compose<<<blocks(n0), LD_T, 0, st>>>(n0, nr.p, node_of.p);
        SQGR_HIP(hipGetLastError());
        for (int l = 0; l < MX_LAYERS; ++l) SQGR_TRY(coarse_layer(g.l[l], out.l[l], nc));
        out.n = nc;
        return SQGR_OK;
    }

    // one iteration from comm (level 0 ids); leaves node_of
    int iterate() {
        k_iota<<<blocks(n0), LD_T, 0, st>>>(n0, node_of.p);
        SQGR_HIP(hipGetLastError());
        MxLevelBuf* cur = &g0;
        for (;;) {
            ++stat_levels;
            Acc h[MX_LAYERS];
            SQGR_TRY(prepare(*cur, h));
            SQGR_TRY(rebuild_tot(*cur));
            SQGR_TRY(local_moving(*cur));
            int64_t kp = 0;
            SQGR_TRY(count_distinct(cur->n, comm.p, &kp));
            if (kp == cur->n) break;
            SQGR_TRY(refine(*cur));
            MxLevelBuf* next = cur == &ga ? &gb : &ga;
            int64_t nc = 0;
            SQGR_TRY(aggregate(*cur, *next, &nc));
            if (nc == cur->n) break;
            SQGR_HIP(hipMemcpyAsync(comm.p, ccomm.p, (size_t)nc * 4, hipMemcpyDeviceToDevice, st));
            cur = next;
        }
        return SQGR_OK;
    }
};

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_leiden_multiplex_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = LD_WEIGHT_BITS;
    out_info[1] = LD_SWEEP_CAP;
    out_info[2] = LD_ITER_CAP;
    out_info[3] = LD_CAP;
    out_info[4] = LD_SLOTS;
    out_info[5] = MX_STATS;  // entries of out_stats
    out_info[6] = MX_LAYERS;
    return SQGR_OK;
}

int sqgr_leiden_multiplex(sqgr_ctx* ctx, int64_t n, const int64_t* indptr0, const int32_t* indices0, const int32_t* weights0,
                          const int64_t* indptr1, const int32_t* indices1, const int32_t* weights1, double resolution0, double resolution1,
                          double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats) {
    SQGR_REQUIRE(ctx && indptr0 && indptr1 && out_labels && out_stats, "null argument");
    SQGR_REQUIRE(n >= 1, "sqgr_leiden_multiplex: n=%lld", (long long)n);
    SQGR_REQUIRE(std::isfinite(resolution0) && resolution0 > 0, "sqgr_leiden_multiplex: layer 0: resolution=%g must be finite and positive", resolution0);
    SQGR_REQUIRE(std::isfinite(resolution1) && resolution1 > 0, "sqgr_leiden_multiplex: layer 1: resolution=%g must be finite and positive", resolution1);
    SQGR_REQUIRE(std::isfinite(layer_ratio) && layer_ratio > 0, "sqgr_leiden_multiplex: layer_ratio=%g must be finite and positive", layer_ratio);
    SQGR_REQUIRE(n_iterations != 0, "sqgr_leiden_multiplex: n_iterations=0 (a positive count, or negative for: until an iteration changes nothing)");
    if (n >= ((int64_t)1 << 31) - 1) {
        set_error("sqgr_leiden_multiplex: n=%lld, vertex ids are 32-bit", (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    const int64_t* const indptr[MX_LAYERS] = {indptr0, indptr1};
    const int32_t* const indices[MX_LAYERS] = {indices0, indices1};
    const int32_t* const weights[MX_LAYERS] = {weights0, weights1};
    int64_t nnz[MX_LAYERS];
    for (int l = 0; l < MX_LAYERS; ++l) {
        SQGR_REQUIRE(indptr[l][0] == 0, "sqgr_leiden_multiplex: layer %d: indptr[0]=%lld", l, (long long)indptr[l][0]);
        for (int64_t i = 0; i < n; ++i)
            SQGR_REQUIRE(indptr[l][i + 1] >= indptr[l][i], "sqgr_leiden_multiplex: layer %d: indptr decreases at row %lld", l, (long long)i);
        nnz[l] = indptr[l][n];
        SQGR_REQUIRE(nnz[l] == 0 || (indices[l] && weights[l]), "null argument");
        if (nnz[l] >= ((int64_t)1 << 36)) {
            set_error("sqgr_leiden_multiplex: layer %d: nnz=%lld", l, (long long)nnz[l]);
            return SQGR_ERR_UNSUPPORTED;
        }
    }
    for (int i = 0; i < MX_STATS; ++i) out_stats[i] = 0;
    if (nnz[0] + nnz[1] == 0) {  // 2m_0 = 2m_1 = 0: every vertex is its own community
        for (int64_t i = 0; i < n; ++i) out_labels[i] = (int32_t)i;
        out_stats[0] = n;
        out_stats[9] = 1;
        return SQGR_OK;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    Multiplex S;
    S.ctx = ctx;
    S.st = ctx->stream;
    S.grid = 8u * (unsigned)std::max(ctx->cu_count, 1);
    S.P.gamma[0] = resolution0;
    S.P.gamma[1] = resolution1;
    S.P.ratio = layer_ratio;
    S.n0 = n;
    hipStream_t st = S.st;
    const size_t ncap = (size_t)n;
    size_t ecap_max = 0;
    for (int l = 0; l < MX_LAYERS; ++l) {  // a coarse level has fewer nodes and at most one self loop per node more
        S.ecap[l] = nnz[l] + n;
        ecap_max = std::max(ecap_max, (size_t)S.ecap[l]);
        SQGR_TRY(S.g0.l[l].alloc(n, nnz[l]));
        SQGR_TRY(S.ga.l[l].alloc(n, S.ecap[l]));
        SQGR_TRY(S.gb.l[l].alloc(n, S.ecap[l]));
        for (DevBuf<int64_t>* b : {&S.tot[l], &S.dk[l], &S.rtot[l], &S.rext[l], &S.vext[l], &S.mk_best[l], &S.mtot_target[l]}) SQGR_TRY(b->alloc(ncap));
        SQGR_TRY(S.mclaimed[l].alloc(ncap));
    }
    for (DevBuf<int32_t>* b : {&S.comm, &S.best_comm, &S.want, &S.rcomm, &S.rsize, &S.flags, &S.newid, &S.nr, &S.pmin, &S.ccomm, &S.node_of, &S.long_rows})
        SQGR_TRY(b->alloc(ncap));
    SQGR_TRY(S.mg_own.alloc(ncap));
    SQGR_TRY(S.mfirst.alloc(ncap));
    SQGR_TRY(S.sw_out.alloc(ecap_max));
    SQGR_TRY(S.keys_in.alloc(ecap_max));
    SQGR_TRY(S.keys_out.alloc(ecap_max));
    SQGR_TRY(S.ukeys.alloc(ecap_max));
    SQGR_TRY(S.acc.alloc(MX_LAYERS));
    SQGR_TRY(S.n_unique.alloc(1));
    SQGR_HIP(hipMemsetAsync(S.acc.p, 0, MX_LAYERS * sizeof(Acc), st));

    // upload and check
    DevBuf<int32_t> w32[MX_LAYERS];
    DevBuf<int> flags;
    SQGR_TRY(flags.alloc(5 * MX_LAYERS));
    SQGR_HIP(hipMemsetAsync(flags.p, 0, 5 * MX_LAYERS * sizeof(int), st));
    S.g0.n = n;
    for (int l = 0; l < MX_LAYERS; ++l) {
        LevelBuf& g = S.g0.l[l];
        g.n = n;
        g.nnz = nnz[l];
        SQGR_TRY(w32[l].alloc((size_t)nnz[l]));
        SQGR_HIP(hipMemcpyAsync(g.indptr.p, indptr[l], ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
        if (!nnz[l]) continue;
        SQGR_HIP(hipMemcpyAsync(g.indices.p, indices[l], (size_t)nnz[l] * 4, hipMemcpyHostToDevice, st));
        SQGR_HIP(hipMemcpyAsync(w32[l].p, weights[l], (size_t)nnz[l] * 4, hipMemcpyHostToDevice, st));
        k_widen<<<S.blocks(nnz[l]), LD_T, 0, st>>>(w32[l].p, nnz[l], g.w.p);
        SQGR_HIP(hipGetLastError());
    }
    Acc hacc[MX_LAYERS];
    SQGR_TRY(S.prepare(S.g0, hacc));  // erow (indptr alone decides it), k, 2m
    for (int l = 0; l < MX_LAYERS; ++l) {
        if (!nnz[l]) continue;
        LaunchTimer t(ctx, "mleiden_check");
        k_check<<<S.blocks(nnz[l]), LD_T, 0, st>>>(n, S.g0.l[l].indptr.p, S.g0.l[l].indices.p, w32[l].p, S.g0.l[l].erow.p, nnz[l], flags.p + 5 * l);
        SQGR_HIP(hipGetLastError());
    }
    int hf[5 * MX_LAYERS];
    for (int& f : hf) f = 1;
    SQGR_HIP(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < MX_LAYERS; ++l) {
        const int* f = hf + 5 * l;
        SQGR_REQUIRE(!f[4], "sqgr_leiden_multiplex: layer %d: a column index is outside [0, n)", l);
        SQGR_REQUIRE(!f[3], "sqgr_leiden_multiplex: layer %d: a weight is smaller than 1", l);
        SQGR_REQUIRE(!f[1], "sqgr_leiden_multiplex: layer %d: a row of the graph is not sorted or repeats an entry", l);
        SQGR_REQUIRE(!f[2], "sqgr_leiden_multiplex: layer %d: the graph has a self loop", l);
        SQGR_REQUIRE(!f[0], "sqgr_leiden_multiplex: layer %d: the graph is not symmetric (an entry without a mirror entry of equal weight)", l);
        const unsigned __int128 two_m128 = (unsigned __int128)hacc[l].two_m[0] + ((unsigned __int128)hacc[l].two_m[1] << 32);
        if (two_m128 >= ((unsigned __int128)1 << 62)) {
            set_error("sqgr_leiden_multiplex: layer %d: the sum of all weights reaches 2^62", l);
            return SQGR_ERR_UNSUPPORTED;
        }
        S.two_m[l] = (int64_t)two_m128;
        S.P.two_m[l] = (double)S.two_m[l];
    }

    std::vector<int32_t> ids((size_t)n), labels((size_t)n), prev((size_t)n);
    std::iota(prev.begin(), prev.end(), 0);  // the start: every vertex alone, which is canonical
    const int max_it = n_iterations < 0 ? LD_ITER_CAP : n_iterations;
    int64_t K = n, iterations = 0, settled = 0;
    for (int it = 0; it < max_it; ++it) {
        SQGR_HIP(hipMemcpyAsync(S.comm.p, prev.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        SQGR_TRY(S.iterate());
        SQGR_HIP(hipMemcpyAsync(ids.data(), S.node_of.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        const int64_t k_new = canonical_labels(ids, n, labels.data());
        ++iterations;
        if (labels == prev) {
            settled = 1;
            break;
        }
        prev.swap(labels);
        K = k_new;
    }
    // sum_c in^l_c of the result on the input layers
    SQGR_HIP(hipMemcpyAsync(S.comm.p, prev.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    for (int l = 0; l < MX_LAYERS; ++l) {
        SQGR_HIP(hipMemsetAsync(&S.acc.p[l].sum_in, 0, 8, st));
        if (!nnz[l]) continue;
        k_sum_in<<<S.blocks(nnz[l]), LD_T, 0, st>>>(nnz[l], S.g0.l[l].erow.p, S.g0.l[l].indices.p, S.g0.l[l].w.p, S.comm.p, &S.acc.p[l]);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_TRY(S.read_acc(hacc));
    std::copy(prev.begin(), prev.end(), out_labels);
    out_stats[0] = K;
    out_stats[1] = iterations;
    out_stats[2] = S.stat_levels;
    out_stats[3] = S.stat_sweeps;
    out_stats[4] = hacc[0].sum_in;
    out_stats[5] = S.two_m[0];
    out_stats[6] = hacc[1].sum_in;
    out_stats[7] = S.two_m[1];
    out_stats[8] = S.stat_cap_hits;
    out_stats[9] = settled;
    return SQGR_OK;
}
