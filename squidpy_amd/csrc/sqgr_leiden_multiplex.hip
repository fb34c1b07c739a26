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
//
// This file holds what sees both layers at once: k_best2, k_apply2, k_long_rows2, the sweep that launches them, the mixed Q, and
// the entry points.  The per-layer kernels are in sqgr_leiden.h; the host driver is sqgr_leiden.hip's, in sqgr_leiden_driver.h.
#include "sqgr_leiden_driver.h"

namespace sqgr {
namespace {

constexpr int MX_LAYERS = 2;

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

struct TwoLayers {
    static constexpr const char* NAME = "sqgr_leiden_multiplex";
    static std::string where(int l) { return std::string(NAME) + ": layer " + std::to_string(l); }

    template <class D>
    static MxParams params(const D& d) {
        return MxParams{{d.gamma[0], d.gamma[1]}, {(double)d.two_m[0], (double)d.two_m[1]}, d.ratio};
    }

    template <class D>
    static int long_rows(D& d, const Level<MX_LAYERS>& g) {
        k_long_rows2<<<d.blocks(g.n), LD_T, 0, d.st>>>(g.n, g.l[0].indptr.p, g.l[1].indptr.p, d.long_rows.p, d.acc.p);
        SQGR_HIP(hipGetLastError());
        return SQGR_OK;
    }

    template <bool REFINE, class D>
    static int sweep(D& d, const Level<MX_LAYERS>& g, uint32_t s) {
        sqgr_ctx* const ctx = d.ctx;
        hipStream_t const st = d.st;
        const MxLevel G{{g.l[0].view(), g.l[1].view()}};
        const MxParams P = params(d);
        const MxMove M{{d.mk_best[0].p, d.mk_best[1].p}, d.mg_own.p, {d.mtot_target[0].p, d.mtot_target[1].p}, {d.mclaimed[0].p, d.mclaimed[1].p},
                       d.mfirst.p};
        if (!REFINE) {
            SQGR_HIP(hipMemsetAsync(d.mclaimed[0].p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(d.mclaimed[1].p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(d.mfirst.p, 0xff, (size_t)g.n * 8, st));
        }
        const MxRefine R = REFINE ? MxRefine{d.rcomm.p, d.rsize.p, {d.rtot[0].p, d.rtot[1].p}, {d.rext[0].p, d.rext[1].p}, {d.vext[0].p, d.vext[1].p}}
                                  : MxRefine{nullptr, nullptr, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
        {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_best" : "mleiden_move_best");
            k_best2<false, REFINE><<<d.wave_blocks(g.n), LD_T, 0, st>>>(G, d.comm.p, d.tot[0].p, d.tot[1].p, R, P, nullptr, 0, nullptr, nullptr, nullptr,
                                                                       d.want.p, d.dk[0].p, d.dk[1].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        if (d.n_long) {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_best_long" : "mleiden_move_best_long");
            k_best2<true, REFINE><<<(unsigned)std::min<int64_t>(d.n_long, d.grid), LD_T, 0, st>>>(G, d.comm.p, d.tot[0].p, d.tot[1].p, R, P, d.long_rows.p,
                                                                                                 d.n_long, d.tkeys.p, d.tvals[0].p, d.tvals[1].p, d.want.p,
                                                                                                 d.dk[0].p, d.dk[1].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, REFINE ? "mleiden_refine_apply" : "mleiden_move_apply");
            if (REFINE)
                k_apply2<true><<<d.wave_blocks(g.n), LD_T, 0, st>>>(G, d.want.p, d.dk[0].p, d.dk[1].p, s, d.rcomm.p, d.rtot[0].p, d.rtot[1].p, d.rsize.p,
                                                                    d.rext[0].p, d.rext[1].p, d.vext[0].p, d.vext[1].p, d.acc.p, M, P);
            else
                k_apply2<false><<<d.wave_blocks(g.n), LD_T, 0, st>>>(G, d.want.p, d.dk[0].p, d.dk[1].p, s, d.comm.p, d.tot[0].p, d.tot[1].p, nullptr,
                                                                     nullptr, nullptr, nullptr, nullptr, d.acc.p, M, P);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    // Q = (double)two_m_0 * q_0 + layer_ratio * ((double)two_m_1 * q_1), q_l the single-layer expression, 0 for a layer without weight
    template <class D>
    static double quality(const D& d, const Acc* h) {
        double part[MX_LAYERS];
        for (int l = 0; l < MX_LAYERS; ++l)
            part[l] = d.two_m[l] ? (double)d.two_m[l] * ld_quality(h[l].sum_in, ld_join_sq(h[l]), d.gamma[l], d.two_m[l]) : 0.0;
        return mx_mix(params(d), part[0], part[1]);
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
    out_info[5] = ld_n_stats(MX_LAYERS);  // entries of out_stats
    out_info[6] = MX_LAYERS;
    return SQGR_OK;
}

int sqgr_leiden_multiplex(sqgr_ctx* ctx, int64_t n, const int64_t* indptr0, const int32_t* indices0, const int32_t* weights0,
                          const int64_t* indptr1, const int32_t* indices1, const int32_t* weights1, double resolution0, double resolution1,
                          double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats) {
    return sqgr_leiden_multiplex_hook(ctx, n, indptr0, indices0, weights0, indptr1, indices1, weights1, resolution0, resolution1, layer_ratio,
                                      n_iterations, out_labels, out_stats, 0);
}

int sqgr_leiden_multiplex_hook(sqgr_ctx* ctx, int64_t n, const int64_t* indptr0, const int32_t* indices0, const int32_t* weights0,
                               const int64_t* indptr1, const int32_t* indices1, const int32_t* weights1, double resolution0, double resolution1,
                               double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats, int32_t grid_blocks) {
    const int64_t* const indptr[MX_LAYERS] = {indptr0, indptr1};
    const int32_t* const indices[MX_LAYERS] = {indices0, indices1};
    const int32_t* const weights[MX_LAYERS] = {weights0, weights1};
    const double resolution[MX_LAYERS] = {resolution0, resolution1};
    return leiden_run<MX_LAYERS, TwoLayers>(ctx, n, indptr, indices, weights, resolution, layer_ratio, n_iterations, out_labels, out_stats,
                                            grid_blocks);
}
