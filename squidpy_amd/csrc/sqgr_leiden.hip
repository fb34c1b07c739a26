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
#include "sqgr_leiden.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

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

struct Leiden {
    sqgr_ctx* ctx;
    hipStream_t st;
    unsigned grid;  // blocks of the grid-stride kernels
    double gamma, two_m_d;
    int64_t two_m;
    int64_t n0, nnz0;
    LevelBuf g0, ga, gb;
    DevBuf<int32_t> comm, best_comm, want, rcomm, rsize, flags, newid, nr, pmin, ccomm, node_of, long_rows, tkeys;
    DevBuf<int64_t> tot, dk, rtot, rext, vext, sw_out, mk_best, mtot_target;
    DevBuf<double> mg_own;
    DevBuf<unsigned long long> mclaimed, mfirst;
    DevBuf<unsigned long long> tvals;
    DevBuf<uint64_t> keys_in, keys_out, ukeys;
    DevBuf<char> temp;
    DevBuf<Acc> acc;
    DevBuf<int64_t> n_unique;
    int64_t n_long = 0;
    int64_t stat_levels = 0, stat_sweeps = 0, stat_cap_hits = 0;

    unsigned blocks(int64_t items) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, LD_T), grid)); }
    unsigned wave_blocks(int64_t rows) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, LD_WAVES), grid)); }

    int read_acc(Acc* h) {
        SQGR_HIP(hipMemcpyAsync(h, acc.p, sizeof(Acc), hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        return SQGR_OK;
    }

    // k, erow and the long rows of a level whose CSR is in place
    int prepare(LevelBuf& g) {
        SQGR_HIP(hipMemsetAsync(&acc.p->two_m, 0, 3 * sizeof(unsigned long long), st));  // two_m[2] and n_long
        {
            LaunchTimer t(ctx, "leiden_rows");
            k_rows<<<wave_blocks(g.n), LD_T, 0, st>>>(g.n, g.indptr.p, g.w.p, g.k.p, g.erow.p, long_rows.p, acc.p);
            SQGR_HIP(hipGetLastError());
        }
        Acc h;
        SQGR_TRY(read_acc(&h));
        n_long = (int64_t)h.n_long;
        if (n_long && !tkeys.p) {  // the global tables: two slots per stored entry of the largest level
            SQGR_TRY(tkeys.alloc_pooled(2 * (size_t)(nnz0 + n0)));
            SQGR_TRY(tvals.alloc_pooled(2 * (size_t)(nnz0 + n0)));
        }
        return SQGR_OK;
    }

    int rebuild_tot(const LevelBuf& g) {
        SQGR_HIP(hipMemsetAsync(tot.p, 0, (size_t)g.n * 8, st));
        LaunchTimer t(ctx, "leiden_tot");
        k_tot<<<blocks(g.n), LD_T, 0, st>>>(g.n, comm.p, g.k.p, tot.p);
        SQGR_HIP(hipGetLastError());
        return SQGR_OK;
    }

    template <bool REFINE>
    int sweep(const LevelBuf& g, uint32_t s) {
        const LevelView L = g.view();
        const MoveView M{mk_best.p, mg_own.p, mtot_target.p, mclaimed.p, mfirst.p};
        if (!REFINE) {
            SQGR_HIP(hipMemsetAsync(mclaimed.p, 0, (size_t)g.n * 8, st));
            SQGR_HIP(hipMemsetAsync(mfirst.p, 0xff, (size_t)g.n * 8, st));
        }
        const RefineView R = REFINE ? RefineView{rcomm.p, rtot.p, rext.p, rsize.p, vext.p} : RefineView{nullptr, nullptr, nullptr, nullptr, nullptr};
        {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_best" : "leiden_move_best");
            k_best<false, REFINE><<<wave_blocks(g.n), LD_T, 0, st>>>(L, comm.p, tot.p, R, gamma, two_m_d, nullptr, 0, nullptr, nullptr, want.p, dk.p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        if (n_long) {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_best_long" : "leiden_move_best_long");
            k_best<true, REFINE><<<(unsigned)std::min<int64_t>(n_long, grid), LD_T, 0, st>>>(L, comm.p, tot.p, R, gamma, two_m_d, long_rows.p, n_long,
                                                                                            tkeys.p, tvals.p, want.p, dk.p, M, s);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, REFINE ? "leiden_refine_apply" : "leiden_move_apply");
            if (REFINE)
                k_apply<true><<<wave_blocks(g.n), LD_T, 0, st>>>(L, want.p, dk.p, s, rcomm.p, rtot.p, rsize.p, rext.p, vext.p, acc.p, M, gamma, two_m_d);
            else
                k_apply<false><<<wave_blocks(g.n), LD_T, 0, st>>>(L, want.p, dk.p, s, comm.p, tot.p, nullptr, nullptr, nullptr, acc.p, M, gamma, two_m_d);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    int sumsq(const LevelBuf& g) {
        LaunchTimer t(ctx, "leiden_sumsq");
        k_sumsq<<<blocks(g.n), LD_T, 0, st>>>(g.n, tot.p, acc.p);
        SQGR_HIP(hipGetLastError());
        return SQGR_OK;
    }

    static unsigned __int128 join_sq(const Acc& h) { return ld_join_sq(h); }

    int local_moving(const LevelBuf& g) {
        SQGR_HIP(hipMemsetAsync(acc.p, 0, offsetof(Acc, two_m), st));  // moves, sum_in, sq
        if (g.nnz) {
            LaunchTimer t(ctx, "leiden_sum_in");
            k_sum_in<<<blocks(g.nnz), LD_T, 0, st>>>(g.nnz, g.erow.p, g.indices.p, g.w.p, comm.p, acc.p);
            SQGR_HIP(hipGetLastError());
        }
        SQGR_TRY(sumsq(g));
        Acc h;
        SQGR_TRY(read_acc(&h));
        double best_q = ld_quality(h.sum_in, join_sq(h), gamma, two_m);
        SQGR_HIP(hipMemcpyAsync(best_comm.p, comm.p, (size_t)g.n * 4, hipMemcpyDeviceToDevice, st));
        bool converged = false;
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p->moves, 0, 8, st));
            SQGR_HIP(hipMemsetAsync(&acc.p->sq, 0, 24, st));
            SQGR_TRY(sweep<false>(g, (uint32_t)s));
            SQGR_TRY(sumsq(g));
            SQGR_TRY(read_acc(&h));
            ++stat_sweeps;
            if (!h.moves) {
                converged = true;
                break;
            }
            const double q = ld_quality(h.sum_in, join_sq(h), gamma, two_m);
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
        SQGR_HIP(hipMemsetAsync(&acc.p->count, 0, 8, st));
        k_flag<<<blocks(n), LD_T, 0, st>>>(n, ids, flags.p);
        SQGR_HIP(hipGetLastError());
        k_count_flags<<<blocks(n), LD_T, 0, st>>>(n, flags.p, acc.p);
        SQGR_HIP(hipGetLastError());
        Acc h;
        SQGR_TRY(read_acc(&h));
        *out = (int64_t)h.count;
        return SQGR_OK;
    }

    int refine(const LevelBuf& g) {
        {
            LaunchTimer t(ctx, "leiden_refine_init");
            k_refine_init<<<wave_blocks(g.n), LD_T, 0, st>>>(g.view(), comm.p, rcomm.p, rtot.p, rext.p, rsize.p, vext.p);
            SQGR_HIP(hipGetLastError());
        }
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p->moves, 0, 8, st));
            SQGR_TRY(sweep<true>(g, (uint32_t)s));
            Acc h;
            SQGR_TRY(read_acc(&h));
            ++stat_sweeps;
            if (!h.moves) break;
        }
        return SQGR_OK;
    }

    int ensure_temp(size_t bytes) { return temp.ensure(std::max<size_t>(bytes, 16)); }

    // the refined communities of level g become the nodes of `out`; *n_coarse == g.n: nothing merged and `out` is not built
    int aggregate(const LevelBuf& g, LevelBuf& out, int64_t* n_coarse) {
        const int64_t n = g.n, nnz = g.nnz;
        SQGR_HIP(hipMemsetAsync(flags.p, 0, (size_t)n * 4, st));
        k_flag<<<blocks(n), LD_T, 0, st>>>(n, rcomm.p, flags.p);
        SQGR_HIP(hipGetLastError());
        size_t tb = 0;
        SQGR_HIP(rocprim::exclusive_scan(nullptr, tb, flags.p, newid.p, 0, (size_t)n, rocprim::plus<int32_t>(), st));
        SQGR_TRY(ensure_temp(tb));
        {
            LaunchTimer t(ctx, "leiden_renumber");
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
        int64_t m = 0;
        if (nnz) {
            k_edge_keys<<<blocks(nnz), LD_T, 0, st>>>(nnz, g.erow.p, g.indices.p, nr.p, keys_in.p);
            SQGR_HIP(hipGetLastError());
            SQGR_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys_in.p, keys_out.p, g.w.p, sw_out.p, (size_t)nnz, 0, 64, st));
            SQGR_TRY(ensure_temp(tb));
            {
                LaunchTimer t(ctx, "leiden_sort");
                SQGR_HIP(rocprim::radix_sort_pairs(temp.p, tb, keys_in.p, keys_out.p, g.w.p, sw_out.p, (size_t)nnz, 0, 64, st));
            }
            SQGR_HIP(rocprim::reduce_by_key(nullptr, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p, rocprim::plus<int64_t>(),
                                            rocprim::equal_to<uint64_t>(), st));
            SQGR_TRY(ensure_temp(tb));
            {
                LaunchTimer t(ctx, "leiden_reduce");
                SQGR_HIP(rocprim::reduce_by_key(temp.p, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p,
                                                rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), st));
            }
            SQGR_HIP(hipMemcpyAsync(&m, n_unique.p, 8, hipMemcpyDeviceToHost, st));
            SQGR_HIP(hipStreamSynchronize(st));
            if (m < 0 || m > nnz) {
                set_error("sqgr_leiden: reduce_by_key returned %lld groups of %lld entries", (long long)m, (long long)nnz);
                return SQGR_ERR_HIP;
            }
            k_coarse_cols<<<blocks(m), LD_T, 0, st>>>(m, ukeys.p, out.indices.p);
            SQGR_HIP(hipGetLastError());
        }
        k_coarse_indptr<<<blocks(nc + 1), LD_T, 0, st>>>(nc, m, ukeys.p, out.indptr.p);
        SQGR_HIP(hipGetLastError());
        out.n = nc;
        out.nnz = m;
        return SQGR_OK;
    }

    // one iteration from comm (level 0 ids); leaves node_of
    int iterate() {
        {
            k_iota<<<blocks(n0), LD_T, 0, st>>>(n0, node_of.p);
            SQGR_HIP(hipGetLastError());
        }
        LevelBuf* cur = &g0;
        for (;;) {
            ++stat_levels;
            SQGR_TRY(prepare(*cur));
            SQGR_TRY(rebuild_tot(*cur));
            SQGR_TRY(local_moving(*cur));
            int64_t kp = 0;
            SQGR_TRY(count_distinct(cur->n, comm.p, &kp));
            if (kp == cur->n) break;
            SQGR_TRY(refine(*cur));
            LevelBuf* next = cur == &ga ? &gb : &ga;
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

int sqgr_leiden_info(int64_t* out_info) {
    SQGR_REQUIRE(out_info, "null argument");
    out_info[0] = LD_WEIGHT_BITS;
    out_info[1] = LD_SWEEP_CAP;
    out_info[2] = LD_ITER_CAP;
    out_info[3] = LD_CAP;
    out_info[4] = LD_SLOTS;
    out_info[5] = 8;  // entries of out_stats
    return SQGR_OK;
}

int sqgr_leiden(sqgr_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* weights, double resolution,
                int32_t n_iterations, int32_t* out_labels, int64_t* out_stats) {
    SQGR_REQUIRE(ctx && indptr && out_labels && out_stats, "null argument");
    SQGR_REQUIRE(n >= 1, "sqgr_leiden: n=%lld", (long long)n);
    SQGR_REQUIRE(std::isfinite(resolution) && resolution > 0, "sqgr_leiden: resolution=%g must be finite and positive", resolution);
    SQGR_REQUIRE(n_iterations != 0, "sqgr_leiden: n_iterations=0 (a positive count, or negative for: until an iteration changes nothing)");
    if (n >= ((int64_t)1 << 31) - 1) {
        set_error("sqgr_leiden: n=%lld, vertex ids are 32-bit", (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    SQGR_REQUIRE(indptr[0] == 0, "sqgr_leiden: indptr[0]=%lld", (long long)indptr[0]);
    for (int64_t i = 0; i < n; ++i) SQGR_REQUIRE(indptr[i + 1] >= indptr[i], "sqgr_leiden: indptr decreases at row %lld", (long long)i);
    const int64_t nnz = indptr[n];
    SQGR_REQUIRE(nnz == 0 || (indices && weights), "null argument");
    if (nnz >= ((int64_t)1 << 36)) {
        set_error("sqgr_leiden: nnz=%lld", (long long)nnz);
        return SQGR_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < 8; ++i) out_stats[i] = 0;
    if (nnz == 0) {  // 2m = 0: every vertex is its own community
        for (int64_t i = 0; i < n; ++i) out_labels[i] = (int32_t)i;
        out_stats[0] = n;
        out_stats[7] = 1;
        return SQGR_OK;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    Leiden S;
    S.ctx = ctx;
    S.st = ctx->stream;
    S.grid = 8u * (unsigned)std::max(ctx->cu_count, 1);
    S.gamma = resolution;
    S.n0 = n;
    S.nnz0 = nnz;
    hipStream_t st = S.st;
    const size_t ncap = (size_t)n, ecap = (size_t)nnz + (size_t)n;  // a coarse level has fewer nodes and at most one self loop per node more
    SQGR_TRY(S.g0.alloc(n, nnz));
    SQGR_TRY(S.ga.alloc(n, (int64_t)ecap));
    SQGR_TRY(S.gb.alloc(n, (int64_t)ecap));
    for (DevBuf<int32_t>* b : {&S.comm, &S.best_comm, &S.want, &S.rcomm, &S.rsize, &S.flags, &S.newid, &S.nr, &S.pmin, &S.ccomm, &S.node_of, &S.long_rows})
        SQGR_TRY(b->alloc(ncap));
    for (DevBuf<int64_t>* b : {&S.tot, &S.dk, &S.rtot, &S.rext, &S.vext, &S.mk_best, &S.mtot_target}) SQGR_TRY(b->alloc(ncap));
    SQGR_TRY(S.mg_own.alloc(ncap));
    SQGR_TRY(S.mclaimed.alloc(ncap));
    SQGR_TRY(S.mfirst.alloc(ncap));
    SQGR_TRY(S.sw_out.alloc(ecap));
    SQGR_TRY(S.keys_in.alloc(ecap));
    SQGR_TRY(S.keys_out.alloc(ecap));
    SQGR_TRY(S.ukeys.alloc(ecap));
    SQGR_TRY(S.acc.alloc(1));
    SQGR_TRY(S.n_unique.alloc(1));
    SQGR_HIP(hipMemsetAsync(S.acc.p, 0, sizeof(Acc), st));

    // upload and check
    DevBuf<int32_t> w32;
    DevBuf<int> flags;
    SQGR_TRY(w32.alloc((size_t)nnz));
    SQGR_TRY(flags.alloc(5));
    SQGR_HIP(hipMemsetAsync(flags.p, 0, 5 * sizeof(int), st));
    SQGR_HIP(hipMemcpyAsync(S.g0.indptr.p, indptr, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(S.g0.indices.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemcpyAsync(w32.p, weights, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    S.g0.n = n;
    S.g0.nnz = nnz;
    k_widen<<<S.blocks(nnz), LD_T, 0, st>>>(w32.p, nnz, S.g0.w.p);
    SQGR_HIP(hipGetLastError());
    SQGR_TRY(S.prepare(S.g0));  // erow (indptr alone decides it), k, 2m
    {
        LaunchTimer t(ctx, "leiden_check");
        k_check<<<S.blocks(nnz), LD_T, 0, st>>>(n, S.g0.indptr.p, S.g0.indices.p, w32.p, S.g0.erow.p, nnz, flags.p);
        SQGR_HIP(hipGetLastError());
    }
    int hf[5] = {1, 1, 1, 1, 1};
    Acc hacc;
    SQGR_HIP(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    SQGR_TRY(S.read_acc(&hacc));
    SQGR_REQUIRE(!hf[4], "sqgr_leiden: a column index is outside [0, n)");
    SQGR_REQUIRE(!hf[3], "sqgr_leiden: a weight is smaller than 1");
    SQGR_REQUIRE(!hf[1], "sqgr_leiden: a row of the graph is not sorted or repeats an entry");
    SQGR_REQUIRE(!hf[2], "sqgr_leiden: the graph has a self loop");
    SQGR_REQUIRE(!hf[0], "sqgr_leiden: the graph is not symmetric (an entry without a mirror entry of equal weight)");
    const unsigned __int128 two_m128 = (unsigned __int128)hacc.two_m[0] + ((unsigned __int128)hacc.two_m[1] << 32);
    if (two_m128 >= ((unsigned __int128)1 << 62)) {
        set_error("sqgr_leiden: the sum of all weights reaches 2^62");
        return SQGR_ERR_UNSUPPORTED;
    }
    S.two_m = (int64_t)two_m128;
    S.two_m_d = (double)S.two_m;

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
    // sum_c in_c of the result on the input graph
    SQGR_HIP(hipMemcpyAsync(S.comm.p, prev.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    SQGR_HIP(hipMemsetAsync(&S.acc.p->sum_in, 0, 8, st));
    k_sum_in<<<S.blocks(nnz), LD_T, 0, st>>>(nnz, S.g0.erow.p, S.g0.indices.p, S.g0.w.p, S.comm.p, S.acc.p);
    SQGR_HIP(hipGetLastError());
    SQGR_TRY(S.read_acc(&hacc));
    std::copy(prev.begin(), prev.end(), out_labels);
    out_stats[0] = K;
    out_stats[1] = iterations;
    out_stats[2] = S.stat_levels;
    out_stats[3] = S.stat_sweeps;
    out_stats[4] = hacc.sum_in;
    out_stats[5] = S.two_m;
    out_stats[6] = S.stat_cap_hits;
    out_stats[7] = settled;
    return SQGR_OK;
}
