// libsqgr: sqgr_leiden — Leiden community detection on a symmetric weighted graph with exact integer weights: what the reference's
// `neighborhood` and `utag` niche flavours get from `sc.tl.leiden` (gr/_niche.py:1428), as a deterministic synchronous variant.
//
// Quality: Q = sum_c (in_c / 2m - gamma (tot_c / 2m)^2) (leidenalg's RBConfigurationVertexPartition).  The caller quantises the weights
// to int32 >= 1; every k_v, k_{v,c}, tot_c, in_c and 2m of every level is an exact int64, so the 64-bit integer atomics below do not
// make a result depend on their order.  The only floating point is
//     gain(v, c) = (double)k_vc - gamma * (double)k_v * (double)(tot_c - [c == comm(v)] k_v) / (double)two_m
// evaluated left to right, every operation rounded on its own (no FMA).  Candidates are ordered by (gain descending, community id
// ascending); a move needs gain(v, c) > gain(v, comm(v)) strictly.  A self loop of a coarse node counts in k_v and never in k_vc.
//
// One iteration walks levels.  Per level:
//   local moving  synchronous sweeps: k_best finds every vertex's best target on the state the sweep started from; k_apply moves a
//                 vertex that wants to move when its priority (ld_hash(vertex, sweep), then the smaller vertex) beats every neighbour
//                 that wants to move too — the movers of a sweep are pairwise non-adjacent, so each k_vc is exact for its move.
//                 Against overshoot (a hub's thousand leaves joining it in one sweep, each on the gain of joining alone): of the
//                 vertices that want into one community the one of best priority may move; any other only if its gain, with tot
//                 of the target raised by the k of ALL of them, still beats staying.
//                 Stops at zero moves or after LD_SWEEP_CAP sweeps; at the cap the assignment of largest Q seen is kept.
//   refinement    the same two kernels from singletons, targets restricted to the vertex's community; only a vertex that is still alone
//                 moves, vertex and target must be well connected (k_{S, C - S} >= gamma tot_S (tot_C - tot_S) / 2m), the target must
//                 be adjacent.  Greedy (theta -> 0).  Every move ends one singleton, so it terminates; LD_SWEEP_CAP bounds it anyway.
//   aggregation   refined communities renumbered ascending (rocPRIM scan), coarse CSR by radix sort and reduce-by-key of
//                 (row, column) keys; self loops carry the inner weight; the coarse level starts from the non-refined partition.
// The levels end when local moving leaves every node alone or refinement merges nothing; the nodes of the last level are the
// communities, so every community is a refined community of refined communities: connected by construction.
//
// k_best: a row of up to LD_CAP entries is one wave's, its neighbour communities in an LDS table of LD_SLOTS slots (open addressing,
// 32-bit compare-and-swap on the key, 64-bit LDS add on the weight); longer rows (hubs, coarse levels) are one block's each, with a
// table of twice the row's length in global memory.  Both paths form the same integers and pick by the same order.
//
// This file holds k_best, k_apply, the sweep that launches them, Q, and the entry points; the kernels that see one CSR are in
// sqgr_leiden.h, and the host driver, which the two-layer sqgr_leiden_multiplex.hip runs too, is in sqgr_leiden_driver.h.
#include "sqgr_leiden_driver.h"

namespace sqgr {
namespace {

struct RefineView {  // refinement state; all null in local moving
    const int32_t* rcomm;
    const int64_t* rtot;
    const int64_t* rext;  // weight between a refined community and the rest of its community
    const int32_t* rsize;
    const int64_t* vext;  // weight between a vertex and the rest of its community
};

struct MoveView {  // local moving only
    int64_t* k_best;                // k_{v,want}
    double* g_own;                  // gain(v, comm(v))
    int64_t* tot_target;            // tot of the target when the sweep began
    unsigned long long* claimed;    // per community: sum of k_v over the vertices that want to move into it (zeroed per sweep)
    unsigned long long* first;      // per community: the smallest priority among them (all ones per sweep)
};

// want[v] = the community v wants to move to, or -1;  dk[v] = k_{v,want} - k_{v,own} (local moving), k_{v,want} (refinement).
// LONG: one block per row of `rows` (n_rows of them), tables of 2 * len slots at 2 * indptr[v] in gkeys / gvals.
// !LONG: one wave per row, rows of more than LD_CAP entries are skipped.
template <bool LONG, bool REFINE>
__global__ __launch_bounds__(LD_T) void k_best(LevelView L, const int32_t* __restrict__ comm, const int64_t* __restrict__ tot, RefineView R,
                                               double gamma, double two_m, const int32_t* __restrict__ rows, int64_t n_rows,
                                               int32_t* __restrict__ gkeys, unsigned long long* __restrict__ gvals,
                                               int32_t* __restrict__ want, int64_t* __restrict__ dk, MoveView M, uint32_t sweep) {
    __shared__ int32_t s_keys[LONG ? 1 : LD_WAVES * LD_SLOTS];
    __shared__ unsigned long long s_vals[LONG ? 1 : LD_WAVES * LD_SLOTS];
    __shared__ double s_g[LD_WAVES], s_gown[LD_WAVES];
    __shared__ int32_t s_c[LD_WAVES];
    __shared__ long long s_k[LD_WAVES], s_kown[LD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = LONG ? (int)threadIdx.x : lane, gsize = LONG ? LD_T : 64;
    const int64_t n_items = LONG ? n_rows : L.n;
    const int64_t per_block = LONG ? 1 : LD_WAVES;
    for (int64_t base = blockIdx.x * per_block; base < n_items; base += (int64_t)gridDim.x * per_block) {  // uniform per block
        const int64_t item = LONG ? base : base + wave;
        int64_t v = -1, a = 0, b = 0;
        if (item < n_items) {
            v = LONG ? (int64_t)rows[item] : item;
            a = L.indptr[v];
            b = L.indptr[v + 1];
            if (!LONG && b - a > LD_CAP) v = -1;  // the long kernel's row
        }
        int32_t* keys = LONG ? gkeys + 2 * a : s_keys + wave * LD_SLOTS;
        unsigned long long* vals = LONG ? gvals + 2 * a : s_vals + wave * LD_SLOTS;
        const uint32_t nslots = LONG ? (uint32_t)(2 * (b - a)) : (uint32_t)LD_SLOTS;
        int32_t own = -1, C = -1;
        int64_t kv = 0, totC = 0;
        bool act = v >= 0;
        if (act) {
            kv = L.k[v];
            C = comm[v];
            own = REFINE ? R.rcomm[v] : C;
            if (REFINE) {
                totC = tot[C];
                act = R.rsize[own] == 1 && (double)R.vext[v] >= ld_penalty(gamma, kv, totC - kv, two_m);
            }
        }
        if (act)
            for (uint32_t s = gtid; s < nslots; s += gsize) {
                keys[s] = -1;
                vals[s] = 0;
            }
        __syncthreads();
        if (act) {
            if (gtid == 0) tbl_insert(keys, vals, nslots, own, 0);
            for (int64_t e = a + gtid; e < b; e += gsize) {
                const int32_t u = L.indices[e];
                if (u == v) continue;
                if (REFINE) {
                    if (comm[u] != C) continue;
                    tbl_insert(keys, vals, nslots, R.rcomm[u], L.w[e]);
                } else {
                    tbl_insert(keys, vals, nslots, comm[u], L.w[e]);
                }
            }
        }
        __syncthreads();
        Cand best{0.0, -1, 0};
        double g_own = -INFINITY;
        long long k_own = 0;
        if (act)
            for (uint32_t s = gtid; s < nslots; s += gsize) {
                const int32_t c = keys[s];
                if (c < 0) continue;
                const long long kvc = (long long)vals[s];
                Cand x;
                x.c = c;
                x.k = kvc;
                if (c == own) {
                    x.g = (double)kvc - ld_penalty(gamma, kv, (REFINE ? R.rtot[c] : tot[c]) - kv, two_m);
                    g_own = x.g;
                    k_own = kvc;
                } else if (REFINE) {
                    const int64_t ts = R.rtot[c];
                    if (!((double)R.rext[c] >= ld_penalty(gamma, ts, totC - ts, two_m))) continue;  // the target is not well connected
                    x.g = (double)kvc - ld_penalty(gamma, kv, ts, two_m);
                } else {
                    x.g = (double)kvc - ld_penalty(gamma, kv, tot[c], two_m);
                }
                if (cand_better(x, best)) best = x;
            }
        best = cand_wave_best(best);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            g_own = fmax(g_own, __shfl_xor(g_own, o, 64));
            k_own += __shfl_xor(k_own, o, 64);
        }
        if (LONG) {
            if (lane == 0) {
                s_g[wave] = best.g;
                s_c[wave] = best.c;
                s_k[wave] = best.k;
                s_gown[wave] = g_own;
                s_kown[wave] = k_own;
            }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 1; i < LD_WAVES; ++i) {
                    const Cand y{s_g[i], s_c[i], s_k[i]};
                    if (cand_better(y, best)) best = y;
                    g_own = fmax(g_own, s_gown[i]);
                    k_own += s_kown[i];
                }
        }
        if (v >= 0 && gtid == 0) {
            const bool move = act && best.c >= 0 && best.c != own && best.g > g_own;
            want[v] = move ? best.c : -1;
            dk[v] = move ? (REFINE ? best.k : best.k - k_own) : 0;
            if (!REFINE && move) {  // what k_apply's overshoot rule needs: the claim on the target and the sweep's own numbers
                M.k_best[v] = best.k;
                M.g_own[v] = g_own;
                M.tot_target[v] = tot[best.c];
                atomicAdd(&M.claimed[best.c], (unsigned long long)kv);
                atomicMin(&M.first[best.c], ld_priority((int32_t)v, sweep));
            }
        }
        __syncthreads();  // the tables and s_* are reused by the next row
    }
}

// a wave per row: the vertex moves unless a neighbour that wants to move has the better priority
template <bool REFINE>
__global__ __launch_bounds__(LD_T) void k_apply(LevelView L, const int32_t* __restrict__ want, const int64_t* __restrict__ dk, uint32_t sweep,
                                                int32_t* __restrict__ comm, int64_t* __restrict__ tot, int32_t* __restrict__ rsize,
                                                int64_t* __restrict__ rext, const int64_t* __restrict__ vext, Acc* __restrict__ acc, MoveView M,
                                                double gamma, double two_m) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)LD_T + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * LD_WAVES;
    for (int64_t v = wave0; v < L.n; v += n_waves) {
        const int32_t t = want[v];
        if (t < 0) continue;  // uniform per wave
        if (!REFINE && M.first[t] != ld_priority((int32_t)v, sweep)) {
            // not the first of those that want into t: moves only if its gain still beats staying after ALL of them have joined
            const int64_t kv = L.k[v];
            const int64_t crowded = M.tot_target[v] + (int64_t)M.claimed[t] - kv;
            if (!((double)M.k_best[v] - ld_penalty(gamma, kv, crowded, two_m) > M.g_own[v])) continue;
        }
        bool lose = false;
        for (int64_t e = L.indptr[v] + lane; e < L.indptr[v + 1]; e += 64) {
            const int32_t u = L.indices[e];
            if (u != v && want[u] >= 0 && !ld_beats((int32_t)v, u, sweep)) lose = true;
        }
        if (__any(lose)) continue;
        if (lane == 0) {
            const int32_t old = comm[v];
            const int64_t kv = L.k[v];
            comm[v] = t;
            atomicAdd((unsigned long long*)&tot[t], (unsigned long long)kv);
            atomicAdd((unsigned long long*)&tot[old], (unsigned long long)(-kv));
            if (REFINE) {
                atomicAdd(&rsize[t], 1);
                atomicSub(&rsize[old], 1);
                atomicAdd((unsigned long long*)&rext[t], (unsigned long long)(vext[v] - 2 * dk[v]));
            } else {
                atomicAdd((unsigned long long*)&acc->sum_in, (unsigned long long)(2 * dk[v]));
            }
            atomicAdd(&acc->moves, 1ull);
        }
    }
}

struct OneLayer {
    static constexpr const char* NAME = "sqgr_leiden";
    static std::string where(int) { return NAME; }

    template <bool REFINE, class D>
    static int sweep(D& d, const Level<1>& g, uint32_t s) {
        sqgr_ctx* const ctx = d.ctx;
        hipStream_t const st = d.st;
        const LevelView L = g.l[0].view();
        const double gamma = d.gamma[0], two_m = (double)d.two_m[0];
        const MoveView M{d.mk_best[0].p, d.mg_own.p, d.mtot_target[0].p, d.mclaimed[0].p, d.mfirst.p};
        if (!REFINE) {
            SQGR_HIP(hipMemsetAsync(d.mclaimed[0].p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(d.mfirst.p, 0xff, (size_t)g.n * 8, st));
        }
        const RefineView R = REFINE ? RefineView{d.rcomm.p, d.rtot[0].p, d.rext[0].p, d.rsize.p, d.vext[0].p}
                                    : RefineView{nullptr, nullptr, nullptr, nullptr, nullptr};
        {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_best" : "leiden_move_best");
            k_best<false, REFINE><<<d.wave_blocks(g.n), LD_T, 0, st>>>(L, d.comm.p, d.tot[0].p, R, gamma, two_m, nullptr, 0, nullptr, nullptr, d.want.p,
                                                                      d.dk[0].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        if (d.n_long) {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_best_long" : "leiden_move_best_long");
            k_best<true, REFINE><<<(unsigned)std::min<int64_t>(d.n_long, d.grid), LD_T, 0, st>>>(L, d.comm.p, d.tot[0].p, R, gamma, two_m, d.long_rows.p,
                                                                                                d.n_long, d.tkeys.p, d.tvals[0].p, d.want.p, d.dk[0].p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_apply" : "leiden_move_apply");
            if (REFINE)
                k_apply<true><<<d.wave_blocks(g.n), LD_T, 0, st>>>(L, d.want.p, d.dk[0].p, s, d.rcomm.p, d.rtot[0].p, d.rsize.p, d.rext[0].p, d.vext[0].p,
                                                                   d.acc.p, M, gamma, two_m);
            else
                k_apply<false><<<d.wave_blocks(g.n), LD_T, 0, st>>>(L, d.want.p, d.dk[0].p, s, d.comm.p, d.tot[0].p, nullptr, nullptr, nullptr, d.acc.p, M,
                                                                    gamma, two_m);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    // the single-layer expression itself, not the two-layer mix of it: one more multiplication could turn q > best_q into a tie
    template <class D>
    static double quality(const D& d, const Acc* h) {
        return ld_quality(h[0].sum_in, ld_join_sq(h[0]), d.gamma[0], d.two_m[0]);
    }
};

}  // namespace
}  // namespace sqgr

using namespace sqgr;

int sqgr_leiden_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = LD_WEIGHT_BITS;
    out_info[1] = LD_SWEEP_CAP;
    out_info[2] = LD_ITER_CAP;
    out_info[3] = LD_CAP;
    out_info[4] = LD_SLOTS;
    out_info[5] = ld_n_stats(1);  // entries of out_stats
    return SQGR_OK;
}

int sqgr_leiden(sqgr_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* weights, double resolution,
                int32_t n_iterations, int32_t* out_labels, int64_t* out_stats) {
    return sqgr_leiden_hook(ctx, n, indptr, indices, weights, resolution, n_iterations, out_labels, out_stats, 0);
}

int sqgr_leiden_hook(sqgr_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* weights, double resolution,
                     int32_t n_iterations, int32_t* out_labels, int64_t* out_stats, int32_t grid_blocks) {
    return leiden_run<1, OneLayer>(ctx, n, &indptr, &indices, &weights, &resolution, 1.0, n_iterations, out_labels, out_stats, grid_blocks);
}
