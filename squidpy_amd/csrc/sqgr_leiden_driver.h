// libsqgr: the host driver of sqgr_leiden.hip (NL = 1) and sqgr_leiden_multiplex.hip (NL = 2): the buffers, the walk over levels
// (local moving, refinement, aggregation), and the body of the entry point (argument checks, upload, the input check and its
// refusals, the outer iterations, out_stats).  Every rule of the algorithm that the host decides is here, once: keeping the
// assignment of largest Q at the sweep cap, when tot is rebuilt, when a level ends, when the global tables are allocated.
// The kernels of sqgr_leiden.h see one CSR at a time and run once per layer.  What sees all layers at once is the flavour's, F:
//   F::NAME, F::where(l)      the prefix of an error text, without and with the layer it speaks of
//   F::sweep<REFINE>(D, g, s) one synchronous sweep: the flavour's views, k_best / k_apply (k_best2 / k_apply2) and their timers
//   F::quality(D, h)          Q of the assignment whose split sums are in h[NL]
//   F::long_rows(D, g)        NL > 1 only: the rows of the global-memory path (one layer has k_rows list them)
// Timer names are "leiden_*" for one layer and "mleiden_*" for two: the tools and the profiles select by that prefix.
#ifndef SQGR_LEIDEN_DRIVER_H
#define SQGR_LEIDEN_DRIVER_H

#include "sqgr_leiden.h"

#include <rocprim/rocprim.hpp>

#include <cmath>
#include <cstddef>
#include <numeric>
#include <string>

namespace sqgr {
namespace {

constexpr int ld_n_stats(int nl) { return 6 + 2 * nl; }  // K, iterations, levels, sweeps, (sum_in, two_m) per layer, cap_hits, settled

#define LD_TIMER(var, what) LaunchTimer var(ctx, NL == 1 ? "leiden_" what : "mleiden_" what)

template <int NL>
struct Level {
    LevelBuf l[NL];  // the same n
    int64_t n = 0;
};

template <int NL, class F>
struct LeidenDriver {
    sqgr_ctx* ctx;
    hipStream_t st;
    unsigned grid;  // blocks of the grid-stride kernels
    double gamma[NL], ratio;
    int64_t two_m[NL];
    int64_t n0, ecap[NL];
    Level<NL> g0, ga, gb;
    DevBuf<int32_t> comm, best_comm, want, rcomm, rsize, flags, newid, nr, pmin, ccomm, node_of, long_rows, tkeys;
    DevBuf<int64_t> tot[NL], dk[NL], rtot[NL], rext[NL], vext[NL], mk_best[NL], mtot_target[NL];
    DevBuf<int64_t> sw_out;
    DevBuf<double> mg_own;
    DevBuf<unsigned long long> mclaimed[NL], mfirst, tvals[NL];
    DevBuf<uint64_t> keys_in, keys_out, ukeys;
    DevBuf<char> temp;
    DevBuf<Acc> acc;  // one per layer; moves, n_long and count live in acc[0]
    DevBuf<int64_t> n_unique;
    int64_t n_long = 0;
    int64_t stat_levels = 0, stat_sweeps = 0, stat_cap_hits = 0;

    unsigned blocks(int64_t items) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, LD_T), grid)); }
    unsigned wave_blocks(int64_t rows) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, LD_WAVES), grid)); }

    int read_acc(Acc* h) {  // Acc[NL]
        SQGR_HIP(hipMemcpyAsync(h, acc.p, NL * sizeof(Acc), hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
        return SQGR_OK;
    }

    // k, erow and 2m per layer, and the long rows, of a level whose CSRs are in place
    int prepare(Level<NL>& g, Acc* h) {
        for (int l = 0; l < NL; ++l) {
            SQGR_HIP(hipMemsetAsync(&acc.p[l].two_m, 0, 3 * sizeof(unsigned long long), st));  // two_m[2] and n_long
            LD_TIMER(t, "rows");
            k_rows<<<wave_blocks(g.n), LD_T, 0, st>>>(g.n, g.l[l].indptr.p, g.l[l].w.p, g.l[l].k.p, g.l[l].erow.p, NL == 1 ? long_rows.p : nullptr,
                                                     &acc.p[l]);
            SQGR_HIP(hipGetLastError());
        }
        if constexpr (NL > 1) SQGR_TRY(F::long_rows(*this, g));
        SQGR_TRY(read_acc(h));
        n_long = (int64_t)h[0].n_long;
        if (n_long && !tkeys.p) {  // the global tables: two slots per stored entry of all layers of the largest level
            const size_t slots = 2 * (size_t)std::accumulate(ecap, ecap + NL, (int64_t)0);
            SQGR_TRY(tkeys.alloc_pooled(slots));
            for (int l = 0; l < NL; ++l) SQGR_TRY(tvals[l].alloc_pooled(slots));
        }
        return SQGR_OK;
    }

    int rebuild_tot(const Level<NL>& g) {
        for (int l = 0; l < NL; ++l) {
            SQGR_HIP(hipMemsetAsync(tot[l].p, 0, (size_t)g.n * 8, st));
            LD_TIMER(t, "tot");
            k_tot<<<blocks(g.n), LD_T, 0, st>>>(g.n, comm.p, g.l[l].k.p, tot[l].p);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    int sumsq(const Level<NL>& g) {
        for (int l = 0; l < NL; ++l) {
            LD_TIMER(t, "sumsq");
            k_sumsq<<<blocks(g.n), LD_T, 0, st>>>(g.n, tot[l].p, &acc.p[l]);
            SQGR_HIP(hipGetLastError());
        }
        return SQGR_OK;
    }

    int local_moving(const Level<NL>& g) {
        Acc h[NL];
        for (int l = 0; l < NL; ++l) {
            SQGR_HIP(hipMemsetAsync(&acc.p[l], 0, offsetof(Acc, two_m), st));  // moves, sum_in, sq
            if (g.l[l].nnz) {
                LD_TIMER(t, "sum_in");
                k_sum_in<<<blocks(g.l[l].nnz), LD_T, 0, st>>>(g.l[l].nnz, g.l[l].erow.p, g.l[l].indices.p, g.l[l].w.p, comm.p, &acc.p[l]);
                SQGR_HIP(hipGetLastError());
            }
        }
        SQGR_TRY(sumsq(g));
        SQGR_TRY(read_acc(h));
        double best_q = F::quality(*this, h);
        SQGR_HIP(hipMemcpyAsync(best_comm.p, comm.p, (size_t)g.n * 4, hipMemcpyDeviceToDevice, st));
        bool converged = false;
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p[0].moves, 0, 8, st));
            for (int l = 0; l < NL; ++l) SQGR_HIP(hipMemsetAsync(&acc.p[l].sq, 0, 24, st));
            SQGR_TRY(F::template sweep<false>(*this, g, (uint32_t)s));
            SQGR_TRY(sumsq(g));
            SQGR_TRY(read_acc(h));
            ++stat_sweeps;
            if (!h[0].moves) {
                converged = true;
                break;
            }
            const double q = F::quality(*this, h);
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
        Acc h[NL];
        SQGR_TRY(read_acc(h));
        *out = (int64_t)h[0].count;
        return SQGR_OK;
    }

    int refine(const Level<NL>& g) {
        for (int l = 0; l < NL; ++l) {  // rcomm and rsize are written by every layer's launch, with the same values
            LD_TIMER(t, "refine_init");
            k_refine_init<<<wave_blocks(g.n), LD_T, 0, st>>>(g.l[l].view(), comm.p, rcomm.p, rtot[l].p, rext[l].p, rsize.p, vext[l].p);
            SQGR_HIP(hipGetLastError());
        }
        for (int s = 0; s < LD_SWEEP_CAP; ++s) {
            SQGR_HIP(hipMemsetAsync(&acc.p[0].moves, 0, 8, st));
            SQGR_TRY(F::template sweep<true>(*this, g, (uint32_t)s));
            Acc h[NL];
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
                LD_TIMER(t, "sort");
                SQGR_HIP(rocprim::radix_sort_pairs(temp.p, tb, keys_in.p, keys_out.p, g.w.p, sw_out.p, (size_t)nnz, 0, 64, st));
            }
            SQGR_HIP(rocprim::reduce_by_key(nullptr, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p, rocprim::plus<int64_t>(),
                                            rocprim::equal_to<uint64_t>(), st));
            SQGR_TRY(ensure_temp(tb));
            {
                LD_TIMER(t, "reduce");
                SQGR_HIP(rocprim::reduce_by_key(temp.p, tb, keys_out.p, sw_out.p, (size_t)nnz, ukeys.p, out.w.p, n_unique.p,
                                                rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), st));
            }
            SQGR_HIP(hipMemcpyAsync(&m, n_unique.p, 8, hipMemcpyDeviceToHost, st));
            SQGR_HIP(hipStreamSynchronize(st));
            if (m < 0 || m > nnz) {
                set_error("%s: reduce_by_key returned %lld groups of %lld entries", F::NAME, (long long)m, (long long)nnz);
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
    int aggregate(const Level<NL>& g, Level<NL>& out, int64_t* n_coarse) {
        const int64_t n = g.n;
        SQGR_HIP(hipMemsetAsync(flags.p, 0, (size_t)n * 4, st));
        k_flag<<<blocks(n), LD_T, 0, st>>>(n, rcomm.p, flags.p);
        SQGR_HIP(hipGetLastError());
        size_t tb = 0;
        SQGR_HIP(rocprim::exclusive_scan(nullptr, tb, flags.p, newid.p, 0, (size_t)n, rocprim::plus<int32_t>(), st));
        SQGR_TRY(ensure_temp(tb));
        {
            LD_TIMER(t, "renumber");
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
        for (int l = 0; l < NL; ++l) SQGR_TRY(coarse_layer(g.l[l], out.l[l], nc));
        out.n = nc;
        return SQGR_OK;
    }

    // one iteration from comm (level 0 ids); leaves node_of
    int iterate() {
        k_iota<<<blocks(n0), LD_T, 0, st>>>(n0, node_of.p);
        SQGR_HIP(hipGetLastError());
        Level<NL>* cur = &g0;
        for (;;) {
            ++stat_levels;
            Acc h[NL];
            SQGR_TRY(prepare(*cur, h));
            SQGR_TRY(rebuild_tot(*cur));
            SQGR_TRY(local_moving(*cur));
            int64_t kp = 0;
            SQGR_TRY(count_distinct(cur->n, comm.p, &kp));
            if (kp == cur->n) break;
            SQGR_TRY(refine(*cur));
            Level<NL>* next = cur == &ga ? &gb : &ga;
            int64_t nc = 0;
            SQGR_TRY(aggregate(*cur, *next, &nc));
            if (nc == cur->n) break;
            SQGR_HIP(hipMemcpyAsync(comm.p, ccomm.p, (size_t)nc * 4, hipMemcpyDeviceToDevice, st));
            cur = next;
        }
        return SQGR_OK;
    }

    int alloc(int64_t n, const int64_t* nnz) {
        const size_t ncap = (size_t)n;
        size_t ecap_max = 0;
        for (int l = 0; l < NL; ++l) {  // a coarse level has fewer nodes and at most one self loop per node more
            ecap[l] = nnz[l] + n;
            ecap_max = std::max(ecap_max, (size_t)ecap[l]);
            SQGR_TRY(g0.l[l].alloc(n, nnz[l]));
            SQGR_TRY(ga.l[l].alloc(n, ecap[l]));
            SQGR_TRY(gb.l[l].alloc(n, ecap[l]));
            for (DevBuf<int64_t>* b : {&tot[l], &dk[l], &rtot[l], &rext[l], &vext[l], &mk_best[l], &mtot_target[l]}) SQGR_TRY(b->alloc(ncap));
            SQGR_TRY(mclaimed[l].alloc(ncap));
        }
        for (DevBuf<int32_t>* b : {&comm, &best_comm, &want, &rcomm, &rsize, &flags, &newid, &nr, &pmin, &ccomm, &node_of, &long_rows})
            SQGR_TRY(b->alloc(ncap));
        SQGR_TRY(mg_own.alloc(ncap));
        SQGR_TRY(mfirst.alloc(ncap));
        SQGR_TRY(sw_out.alloc(ecap_max));
        SQGR_TRY(keys_in.alloc(ecap_max));
        SQGR_TRY(keys_out.alloc(ecap_max));
        SQGR_TRY(ukeys.alloc(ecap_max));
        SQGR_TRY(acc.alloc(NL));
        SQGR_TRY(n_unique.alloc(1));
        SQGR_HIP(hipMemsetAsync(acc.p, 0, NL * sizeof(Acc), st));
        return SQGR_OK;
    }
};

// the entry point: NL layers over the same n vertices, one resolution per layer; layer_ratio is read where NL > 1;
// grid_blocks >= 1 replaces the default grid of the grid-stride kernels (the *_hook entry points, tests)
template <int NL, class F>
int leiden_run(sqgr_ctx* ctx, int64_t n, const int64_t* const* indptr, const int32_t* const* indices, const int32_t* const* weights,
               const double* resolution, double layer_ratio, int32_t n_iterations, int32_t* out_labels, int64_t* out_stats, int32_t grid_blocks) {
    SQGR_REQUIRE(grid_blocks >= 0, "%s: grid_blocks=%d", F::NAME, grid_blocks);
    SQGR_REQUIRE(ctx && out_labels && out_stats && std::all_of(indptr, indptr + NL, [](const int64_t* p) { return p; }), "null argument");
    SQGR_REQUIRE(n >= 1, "%s: n=%lld", F::NAME, (long long)n);
    for (int l = 0; l < NL; ++l)
        SQGR_REQUIRE(std::isfinite(resolution[l]) && resolution[l] > 0, "%s: resolution=%g must be finite and positive", F::where(l).c_str(),
                     resolution[l]);
    if (NL > 1) SQGR_REQUIRE(std::isfinite(layer_ratio) && layer_ratio > 0, "%s: layer_ratio=%g must be finite and positive", F::NAME, layer_ratio);
    SQGR_REQUIRE(n_iterations != 0, "%s: n_iterations=0 (a positive count, or negative for: until an iteration changes nothing)", F::NAME);
    if (n >= ((int64_t)1 << 31) - 1) {
        set_error("%s: n=%lld, vertex ids are 32-bit", F::NAME, (long long)n);
        return SQGR_ERR_UNSUPPORTED;
    }
    int64_t nnz[NL];
    for (int l = 0; l < NL; ++l) {
        const std::string w = F::where(l);
        SQGR_REQUIRE(indptr[l][0] == 0, "%s: indptr[0]=%lld", w.c_str(), (long long)indptr[l][0]);
        for (int64_t i = 0; i < n; ++i) SQGR_REQUIRE(indptr[l][i + 1] >= indptr[l][i], "%s: indptr decreases at row %lld", w.c_str(), (long long)i);
        nnz[l] = indptr[l][n];
        SQGR_REQUIRE(nnz[l] == 0 || (indices[l] && weights[l]), "null argument");
        if (nnz[l] >= ((int64_t)1 << 36)) {
            set_error("%s: nnz=%lld", w.c_str(), (long long)nnz[l]);
            return SQGR_ERR_UNSUPPORTED;
        }
    }
    constexpr int N_STATS = ld_n_stats(NL);
    for (int i = 0; i < N_STATS; ++i) out_stats[i] = 0;
    if (std::accumulate(nnz, nnz + NL, (int64_t)0) == 0) {  // 2m = 0 in every layer: every vertex is its own community
        for (int64_t i = 0; i < n; ++i) out_labels[i] = (int32_t)i;
        out_stats[0] = n;
        out_stats[N_STATS - 1] = 1;
        return SQGR_OK;
    }
    SQGR_HIP(hipSetDevice(ctx->device));
    LeidenDriver<NL, F> S;
    S.ctx = ctx;
    S.st = ctx->stream;
    S.grid = grid_blocks ? (unsigned)grid_blocks : 8u * (unsigned)std::max(ctx->cu_count, 1);
    std::copy(resolution, resolution + NL, S.gamma);
    S.ratio = layer_ratio;
    S.n0 = n;
    hipStream_t st = S.st;
    SQGR_TRY(S.alloc(n, nnz));

    // upload and check
    DevBuf<int32_t> w32[NL];
    DevBuf<int> flags;
    SQGR_TRY(flags.alloc(5 * NL));
    SQGR_HIP(hipMemsetAsync(flags.p, 0, 5 * NL * sizeof(int), st));
    S.g0.n = n;
    for (int l = 0; l < NL; ++l) {
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
    Acc hacc[NL];
    SQGR_TRY(S.prepare(S.g0, hacc));  // erow (indptr alone decides it), k, 2m
    for (int l = 0; l < NL; ++l) {
        if (!nnz[l]) continue;
        LD_TIMER(t, "check");
        k_check<<<S.blocks(nnz[l]), LD_T, 0, st>>>(n, S.g0.l[l].indptr.p, S.g0.l[l].indices.p, w32[l].p, S.g0.l[l].erow.p, nnz[l], flags.p + 5 * l);
        SQGR_HIP(hipGetLastError());
    }
    int hf[5 * NL];
    for (int& f : hf) f = 1;
    SQGR_HIP(hipMemcpyAsync(hf, flags.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < NL; ++l) {
        const int* f = hf + 5 * l;
        const std::string w = F::where(l);
        SQGR_REQUIRE(!f[4], "%s: a column index is outside [0, n)", w.c_str());
        SQGR_REQUIRE(!f[3], "%s: a weight is smaller than 1", w.c_str());
        SQGR_REQUIRE(!f[1], "%s: a row of the graph is not sorted or repeats an entry", w.c_str());
        SQGR_REQUIRE(!f[2], "%s: the graph has a self loop", w.c_str());
        SQGR_REQUIRE(!f[0], "%s: the graph is not symmetric (an entry without a mirror entry of equal weight)", w.c_str());
        const unsigned __int128 two_m128 = (unsigned __int128)hacc[l].two_m[0] + ((unsigned __int128)hacc[l].two_m[1] << 32);
        if (two_m128 >= ((unsigned __int128)1 << 62)) {
            set_error("%s: the sum of all weights reaches 2^62", w.c_str());
            return SQGR_ERR_UNSUPPORTED;
        }
        S.two_m[l] = (int64_t)two_m128;
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
    for (int l = 0; l < NL; ++l) {
        SQGR_HIP(hipMemsetAsync(&S.acc.p[l].sum_in, 0, 8, st));
        if (!nnz[l]) continue;
        k_sum_in<<<S.blocks(nnz[l]), LD_T, 0, st>>>(nnz[l], S.g0.l[l].erow.p, S.g0.l[l].indices.p, S.g0.l[l].w.p, S.comm.p, &S.acc.p[l]);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_TRY(S.read_acc(hacc));
    std::copy(prev.begin(), prev.end(), out_labels);
    int64_t* o = out_stats;
    for (int64_t v : {K, iterations, S.stat_levels, S.stat_sweeps}) *o++ = v;
    for (int l = 0; l < NL; ++l) {
        *o++ = hacc[l].sum_in;
        *o++ = S.two_m[l];
    }
    *o++ = S.stat_cap_hits;
    *o++ = settled;
    return SQGR_OK;
}

#undef LD_TIMER

}  // namespace
}  // namespace sqgr

#endif  // SQGR_LEIDEN_DRIVER_H
