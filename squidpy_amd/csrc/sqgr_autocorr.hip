// libsqgr: Moran's I / Geary's C with row-permutation tests on the device-resident CSR graph.
//
// Reference semantics (/root/reference/src/squidpy/gr/_ppatterns.py):
//   :216       score = func(g, vals)                    func = scanpy.metrics.morans_i | gearys_c  (third party)
//   :258-280   per permutation p: idx = rng.permutation(N); score_perms[p] = func(g[idx, :], vals)
// i.e. the ROWS of the weight matrix are permuted, the values stay in place.  With z = x - mean(x):
//   Moran   I  = N/W * sum_i z_i (G z)_i / sum z^2            I_p = N/W * sum_i z_i y[idx_i] / sum z^2,  y = G z
//   Geary   C  = (N-1) sum_ij w_ij (z_i - z_j)^2 / (2 W sum z^2)
//           C_p = (N-1) [ sum_i z_i^2 r[idx_i] - 2 sum_i z_i y[idx_i] + sum_k q_k ] / (2 W sum z^2),
//                 r = G 1 (row sums), q = G z^2
// so 1000 permuted SpMVs per gene collapse into ONE SpMV plus 1000 gather-dots.
//
// Layout: genes are cut into tiles of 64 (one wavefront wide); Zt/Yt/Qt are stored [tile][spot][64] float64, so a
// "row" is 512 contiguous bytes and every gather y[idx_i] is one fully coalesced wave load.  The permutation kernel
// is launched tile-major so that the ~N*512 B working set of the tiles in flight stays in the 256 MB Infinity Cache.
// All reductions are two-stage with a fixed order => bit-reproducible run to run.
//
// The feature blocks come from the resident expression matrix (sqgr_matrix.hip); the LDS permutation dot walks bucket lists
// that sqgr_autocorr_lists.hip builds, schedules and caches (layout: sqgr_autocorr_lists.h).
#include "sqgr_common.h"
#include "sqgr_matrix.h"
#include "sqgr_autocorr_lists.h"
#include "sqgr_rng.h"
#include "sqgr_pcg.h"

#include <atomic>
#include <cstdlib>
#include <optional>

namespace sqgr {

constexpr int GT = 64;         // genes per tile
static_assert(GT == MATRIX_TILE, "the staged blocks are cut into the tiles the matrix expansions write");
constexpr int PERM_TILE = 32;  // permutations per block (8 per wave)
constexpr uint32_t AUTOCORR_STREAM = 0x5A17u;  // "library" word of the Philox counter: separate stream from nhood

// ---- per-gene statistics of a staged gene-major block X[gc][n]: mean and is-constant flag
__global__ __launch_bounds__(256) void k_gene_stats(const double* __restrict__ X, int64_t n, double* __restrict__ mean,
                                                    uint8_t* __restrict__ isconst, int64_t g0) {
    __shared__ double ssum[256];
    __shared__ int sdiff[256];
    const int g = blockIdx.x;
    const double* x = X + (size_t)g * n;
    const double first = x[0];
    double s = 0.0;
    int diff = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double v = x[i];
        s += v;
        diff |= (v != first);
    }
    ssum[threadIdx.x] = s;
    sdiff[threadIdx.x] = diff;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            sdiff[threadIdx.x] |= sdiff[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mean[g0 + g] = ssum[0] / (double)n;
        isconst[g0 + g] = sdiff[0] ? 0 : 1;
    }
}

// ---- Zt[tile][i][gl] = X[g][i] - mean[g]   (64 x 64 tile transpose through LDS; gc is a multiple of 64 or the tail)
__global__ __launch_bounds__(256) void k_center_transpose(const double* __restrict__ X, int64_t n, int gc, int64_t g0,
                                                          const double* __restrict__ mean, double* __restrict__ Zt) {
    __shared__ double tile[GT][GT + 1];
    const int64_t i0 = (int64_t)blockIdx.x * GT;
    const int gb = blockIdx.y * GT;  // gene offset inside the staged block
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < GT; r += 4) {  // r: gene inside tile, tx: spot
        const int g = gb + r;
        const int64_t i = i0 + tx;
        tile[r][tx] = (g < gc && i < n) ? X[(size_t)g * n + i] - mean[g0 + g] : 0.0;
    }
    __syncthreads();
    const int64_t tile_id = (g0 + gb) / GT;
    for (int r = ty; r < GT; r += 4) {  // r: spot inside tile, tx: gene
        const int64_t i = i0 + r;
        if (i < n) Zt[((size_t)tile_id * n + i) * GT + tx] = tile[tx][r];
    }
}

// ---- Yt = G Zt, Qt = G Zt^2 (row i, 64 genes per wave; CSR metadata is wave-uniform => scalar loads)
__global__ __launch_bounds__(256) void k_spmv_tiles(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                    const double* __restrict__ data, int64_t n, const double* __restrict__ Zt,
                                                    double* __restrict__ Yt, double* __restrict__ Qt) {
    const int gl = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double* Z = Zt + (size_t)blockIdx.y * n * GT;
    double y = 0.0, q = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
        const double w = data[e];
        const double zc = Z[(size_t)indices[e] * GT + gl];
        y += w * zc;
        q += w * (zc * zc);
    }
    const size_t o = ((size_t)blockIdx.y * n + i) * GT + gl;
    Yt[o] = y;
    Qt[o] = q;
}

__global__ void k_rowsum(const int64_t* __restrict__ indptr, const double* __restrict__ data, int64_t n, double* __restrict__ rs) {
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s += data[e];
    rs[i] = s;
}

// ---- column reductions over spots, stage 1: partial[tile][chunk][gl]
// MODE 0: sum A*B   1: sum A*A   2: sum A   3: Geary direct  sum_e w_e (z_i - z_col)^2
template <int MODE>
__global__ __launch_bounds__(256) void k_colsum(const double* __restrict__ A, const double* __restrict__ Bm, int64_t n, int R,
                                                const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                const double* __restrict__ data, double* __restrict__ partial) {
    __shared__ double red[4][GT];
    const int gl = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int chunk = blockIdx.x, tile = blockIdx.y;
    const int64_t per = (n + R - 1) / R;
    const int64_t i0 = chunk * per, i1 = min(n, i0 + per);
    const double* a = A + (size_t)tile * n * GT;
    const double* b = Bm ? Bm + (size_t)tile * n * GT : nullptr;
    double s = 0.0;
    for (int64_t i = i0 + sub; i < i1; i += 4) {
        const double av = a[(size_t)i * GT + gl];
        if (MODE == 0) s += av * b[(size_t)i * GT + gl];
        if (MODE == 1) s += av * av;
        if (MODE == 2) s += av;
        if (MODE == 3) {
            double t = 0.0;
            for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
                const double d = av - a[(size_t)indices[e] * GT + gl];
                t += data[e] * (d * d);
            }
            s += t;
        }
    }
    red[sub][gl] = s;
    __syncthreads();
    if (sub == 0) partial[((size_t)tile * R + chunk) * GT + gl] = (red[0][gl] + red[1][gl]) + (red[2][gl] + red[3][gl]);
}

__global__ void k_colsum_final(const double* __restrict__ partial, int R, int64_t G, double* __restrict__ out) {
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t tile = g / GT;
    const int gl = (int)(g % GT);
    double s = 0.0;
    for (int c = 0; c < R; ++c) s += partial[((size_t)tile * R + c) * GT + gl];
    out[g] = s;
}

// ---- permutation indices from the device generator: idx[p][i] = pi_p(i)
__global__ __launch_bounds__(256) void k_perm_indices(uint64_t seed, int64_t perm0, int64_t n, FeistelDomain dom,
                                                      int32_t* __restrict__ idx) {
    __shared__ uint32_t rk[8];
    const int64_t p = blockIdx.y;
    if (threadIdx.x == 0) {
        uint32_t k[8];
        round_keys(seed, (uint64_t)(perm0 + p), AUTOCORR_STREAM, k);
        for (int j = 0; j < 8; ++j) rk[j] = k[j];
    }
    __syncthreads();
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    idx[(size_t)p * n + i] = (int32_t)feistel_perm((uint32_t)i, dom, rk);
}

// ---- the hot kernel: partial sums of  S1[p][g] = sum_i z[i][g] * y[idx_p(i)][g]   (and, for Geary,
//      S2[p][g] = sum_i z[i][g]^2 * r[idx_p(i)])  over one row chunk.
// grid = (perm tiles, row chunks, gene tiles) — gene tile is the slowest grid dimension.
// block = 4 waves; wave w owns PERM_TILE/4 permutations of the block's PERM_TILE; lane = gene.
template <bool GEARY>
__global__ __launch_bounds__(256) void k_perm_dot(const double* __restrict__ Zt, const double* __restrict__ Yt,
                                                  const double* __restrict__ rowsum, const int32_t* __restrict__ idx, int64_t n,
                                                  int64_t nperm, int R, double* __restrict__ part1, double* __restrict__ part2) {
    constexpr int PW = PERM_TILE / 4;  // permutations per wave: each z row read serves PW gathers
    const int gl = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * PERM_TILE + wv * PW;
    if (p0 >= nperm) return;
    const int chunk = blockIdx.y, tile = blockIdx.z;
    const int64_t per = (n + R - 1) / R;
    const int64_t i0 = chunk * per, i1 = min(n, i0 + per);
    const double* Z = Zt + (size_t)tile * n * GT + gl;
    const double* Y = Yt + (size_t)tile * n * GT + gl;
    // clamp: the surplus permutations of the last wave recompute permutation nperm-1 and are not stored
    const int32_t* ix[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) ix[k] = idx + (size_t)min(p0 + k, nperm - 1) * n;
    double a[PW], b[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) a[k] = b[k] = 0.0;
#pragma unroll 2
    for (int64_t i = i0; i < i1; ++i) {
        const double z = Z[(size_t)i * GT];
        const double zz = z * z;
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int32_t row = ix[k][i];  // wave-uniform: scalar load
            a[k] = fma(z, Y[(size_t)row * GT], a[k]);
            if (GEARY) b[k] = fma(zz, rowsum[row], b[k]);  // (pre-gathering r[idx] into its own array measured slower)
        }
    }
    // partial layout [tile][p][chunk][gl]
    const size_t stride = (size_t)R * GT;
    double* o1 = part1 + ((size_t)tile * nperm * R + chunk) * GT + gl;
    double* o2 = GEARY ? part2 + ((size_t)tile * nperm * R + chunk) * GT + gl : nullptr;
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        if (p0 + k < nperm) {
            o1[(size_t)(p0 + k) * stride] = a[k];
            if (GEARY) o2[(size_t)(p0 + k) * stride] = b[k];
        }
    }
}

// ---- stage 2 + statistic:  sims[p][g]
template <bool GEARY>
__global__ __launch_bounds__(256) void k_perm_final(const double* __restrict__ part1, const double* __restrict__ part2, int R,
                                                    int64_t nperm, int64_t G, int64_t n, double W, const double* __restrict__ z2ss,
                                                    const double* __restrict__ qsum, const uint8_t* __restrict__ isconst,
                                                    double* __restrict__ sims) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (g >= G) return;
    const int64_t tile = g / GT;
    const int gl = (int)(g % GT);
    const size_t base = (((size_t)tile * nperm + p) * R) * GT + gl;
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < R; ++c) {
        s1 += part1[base + (size_t)c * GT];
        if (GEARY) s2 += part2[base + (size_t)c * GT];
    }
    double v;
    if (GEARY)
        v = ((double)(n - 1) * ((s2 - 2.0 * s1) + qsum[g])) / (2.0 * W * z2ss[g]);
    else
        v = (double)n / W * s1 / z2ss[g];
    sims[(size_t)p * G + g] = isconst[g] ? __builtin_nan("") : v;
}

// ================================================================================================================
// The LDS-bucketed permutation dot (the hot kernel for n_perms >= 512): both operands of z_i * y[idx_p(i)] on chip, every lane
// walking its permutation's bucket lists.  The scheme, the list layout and its constants: sqgr_autocorr_lists.h.

// Zp[tile2][i][c] = Zt[gene 2*tile2 + c][i]   (pair layout of the 64-gene tiles; genes past G read the tiles' zero padding)
__global__ __launch_bounds__(256) void k_repack_pairs(const double* __restrict__ Zt, int64_t n, int64_t ntiles, int64_t G2,
                                                      double* __restrict__ Zp) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;  // (i, gene) with gene fastest inside a 64-tile
    const int gl = (int)(t & 63);
    const int64_t i = (t >> 6) % n, tile = (t >> 6) / n;
    if (tile >= ntiles) return;
    const int64_t g = tile * GT + gl;
    if ((g >> 1) >= G2) return;
    Zp[((g >> 1) * n + i) * GP + (g & 1)] = Zt[t];
}

// grid (ceil(G2 / 256) * 256 * nch, perm blocks); block = 64 * (groups in a perm block) lanes, lane = permutation.
// Block -> (gene pair, chunk a) with XCD affinity: hardware places block b on XCD (b % 8); the 32 workgroups an XCD runs
// side by side own 32 different gene pairs and the SAME chunk a, so they walk the same lists in step and the lists
// (shared by all genes) are served by that XCD's L2 — only the Y chunks are private traffic.
// part1[((tile2 * pc + p) * nch + a) * 2 + c]
constexpr int LDS_STAGE = 5;  // rows per thread of one chunk at LDS_PERM_BLOCK threads (m <= 5 * 1024)
// RMODE 0: Moran's I.  Geary's C also needs sum_i z_i^2 r[idx_p(i)], r = the graph's row sums: RMODE 1 keeps r[chunk b] in LDS next to
// Y (a third random read per pair, 4092-spot chunks); RMODE 2 (round 4): the row sums take at most 8 DISTINCT values — a
// row-normalised graph has one per degree, a binary graph its degrees — so the list entry carries the class of r[j] in its top three
// bits and the kernel reads an 8-entry table: Moran's chunks, a read that meets in at most 8 addresses.
template <int RMODE>
__global__ __launch_bounds__(LDS_PERM_BLOCK) void k_perm_dot_lds(const double* __restrict__ Zp, const double* __restrict__ Yp,
                                                                 const double* __restrict__ rowsum, int64_t n, int64_t pc, int npg,
                                                                 int64_t G2, int m, int nch, const uint32_t* __restrict__ len,
                                                                 const uint32_t* __restrict__ off, const uint64_t* __restrict__ base,
                                                                 const uint32_t* __restrict__ lists, double* __restrict__ part1,
                                                                 double* __restrict__ part2, int a_per_xcd,
                                                                 const uint32_t* __restrict__ xlen, const uint32_t* __restrict__ xoff,
                                                                 const uint32_t* __restrict__ xlists) {
    // RMODE 3: the main loop is Moran's; the z^2 r term comes from the exception lists (see k_exc_offsets) and a constant
    constexpr bool SECOND = RMODE != 0, GEARY = RMODE == 1 || RMODE == 2, RARR = RMODE == 1, RCLS = RMODE == 2, REXC = RMODE == 3;
    // pairs per lane between two waits (register budget: 128; the class-table variant spills 6 registers at 8 and is still 8 % faster
    // than at 4: 70.8 vs 77.2 ms per 2048 genes x 1000 permutations)
    constexpr int UNR = RARR ? LIST_UNROLL / 2 : LIST_UNROLL;
    constexpr uint32_t JMASK = RCLS ? 0x1fffu : 0xffffu;        // RCLS: bits 29..31 of an entry hold the class of r[j]
    extern __shared__ double2 smem2[];
    double2* Zc = smem2;            // [m + ZERO_ROWS] rows (z of gene 0, z of gene 1); rows m .. = 0
    double2* Yc = smem2 + (m + ZERO_ROWS);  // [m]
    double* Rc = reinterpret_cast<double*>(Yc + m);  // RMODE 1: [m] row sums; RMODE 2: the table of the (<= 8) distinct row sums
    const int tid = threadIdx.x, nthr = blockDim.x;
    int a;
    int64_t tile2;
    {
        // XCD x runs blocks x, x + 8, ... : 32 of them side by side.  They own 32 / A gene pairs x A chunks: a bucket's lists are
        // fetched from the fabric once per XCD and (pair, A chunks) share the Y chunks.  A = 1 (long lists: many permutations)
        // gives 32 pairs walking ONE chunk's lists; the split variant's short lists weigh less than the Y chunks and take A = 4.
        const uint32_t bid = blockIdx.x, x = bid & 7, k = bid >> 3, slot = k & 31, group = k >> 5;
        const uint32_t A = (uint32_t)a_per_xcd, pslots = 32u / A, nag = ((uint32_t)nch + A - 1u) / A;
        a = (int)((group % nag) * A + slot % A);
        tile2 = (int64_t)(group / nag) * (8 * pslots) + x * pslots + slot / A;
    }
    if (tile2 >= G2 || a >= nch) return;  // whole workgroup
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg_raw = (int)blockIdx.y * (LDS_PERM_BLOCK / 64) + wave;
    const bool live = pg_raw < npg;  // waves past the last group only help with the chunk loads
    const int pg = live ? pg_raw : 0;
    const int64_t p = live ? (int64_t)pg * 64 + perm_slot(tid & 63) : pc;
    const double2* Zg = reinterpret_cast<const double2*>(Zp) + (size_t)tile2 * n;
    const double2* Yg = reinterpret_cast<const double2*>(Yp) + (size_t)tile2 * n;
    const bool staged = nthr * LDS_STAGE >= m;  // block-uniform: a whole chunk fits the threads' staging registers
    double2 sy[LDS_STAGE];
    double sr[LDS_STAGE];
#pragma unroll
    for (int u = 0; u < LDS_STAGE; ++u) {
        sy[u] = make_double2(0.0, 0.0);
        sr[u] = 0.0;
    }
    auto fetch = [&](int b) {  // chunk b of Y (and of the row sums) -> registers
        const int64_t j0 = (int64_t)b * m;
        const int mb = (int)min((int64_t)m, n - j0);
#pragma unroll
        for (int u = 0; u < LDS_STAGE; ++u) {
            const int t = tid + u * nthr;
            if (t < mb) {
                sy[u] = Yg[j0 + t];
                if (RARR) sr[u] = rowsum[j0 + t];
            }
        }
    };
    auto commit = [&](int b) {  // registers -> LDS
        const int mb = (int)min((int64_t)m, n - (int64_t)b * m);
#pragma unroll
        for (int u = 0; u < LDS_STAGE; ++u) {
            const int t = tid + u * nthr;
            if (t < mb) {
                Yc[t] = sy[u];
                if (RARR) Rc[t] = sr[u];
            }
        }
    };
    {
        const int64_t i0 = (int64_t)a * m;
        const int ma = (int)min((int64_t)m, n - i0);
        for (int t = tid; t < ma; t += nthr) Zc[t] = Zg[i0 + t];
        if (tid < ZERO_ROWS) Zc[m + tid] = make_double2(0.0, 0.0);
        if ((RCLS || REXC) && tid < 8) Rc[tid] = rowsum[tid];  // (`rowsum` points at the class table; RMODE 3: of r - r0)
    }
    if (staged) fetch(0);
    const size_t bk = ((size_t)pg * nch + a) * nch;
    const uint32_t* lst = lists + (size_t)base[pg] * 64 + (tid & 63);
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int b = 0; b < nch; ++b) {
        __syncthreads();  // the previous Y chunk is no longer read (first pass: nothing to wait for but the Z stores)
        if (staged) {
            commit(b);
        } else {
            const int64_t j0 = (int64_t)b * m;
            const int mb = (int)min((int64_t)m, n - j0);
            for (int t = tid; t < mb; t += nthr) {
                Yc[t] = Yg[j0 + t];
                if (RARR) Rc[t] = rowsum[j0 + t];
            }
        }
        __syncthreads();
        if (staged && b + 1 < nch) fetch(b + 1);  // in flight while this chunk is consumed
        const uint32_t L = live ? (uint32_t)__builtin_amdgcn_readfirstlane((int)len[bk + b]) : 0u;
        const uint32_t* q = lst + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)off[bk + b]) * 64;
        uint32_t code[UNR];
        if (L > 0) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) code[u] = q[u * 64];
        }
        for (uint32_t k = 0; k < L; k += UNR) {
            uint32_t cur[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) cur[u] = code[u];
            q += UNR * 64;
            if (k + UNR < L) {  // the next rows are in flight while these are consumed
#pragma unroll
                for (int u = 0; u < UNR; ++u) code[u] = q[u * 64];
            }
            double2 z[UNR], y[UNR];
            double r[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                z[u] = Zc[cur[u] & 0xffffu];
                y[u] = Yc[(cur[u] >> 16) & JMASK];
                if (RARR) r[u] = Rc[cur[u] >> 16];
                if (RCLS) r[u] = Rc[cur[u] >> 29];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                a0 = fma(z[u].x, y[u].x, a0);
                a1 = fma(z[u].y, y[u].y, a1);
                if (GEARY) {
                    b0 = fma(z[u].x * z[u].x, r[u], b0);
                    b1 = fma(z[u].y * z[u].y, r[u], b1);
                }
            }
        }
    }
    if (REXC && live) {  // the pairs whose j carries another row sum than most: z_i^2 (r[j] - r0), chunk a's Z rows are still in LDS
        const size_t xk = (size_t)pg * nch + a;
        const uint32_t Lx = (uint32_t)__builtin_amdgcn_readfirstlane((int)xlen[xk]);
        const uint32_t* q = xlists + (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)xoff[xk]) * 64 + (tid & 63);
        for (uint32_t k = 0; k < Lx; k += EXC_UNROLL) {
            uint32_t code[EXC_UNROLL];
#pragma unroll
            for (int u = 0; u < EXC_UNROLL; ++u) code[u] = q[(size_t)(k + u) * 64];
#pragma unroll
            for (int u = 0; u < EXC_UNROLL; ++u) {
                const double2 z = Zc[code[u] & 0xffffu];
                const double r = Rc[code[u] >> 29];
                b0 = fma(z.x * z.x, r, b0);
                b1 = fma(z.y * z.y, r, b1);
            }
        }
    }
    if (p < pc) {
        const size_t o = (((size_t)tile2 * pc + p) * nch + a) * GP;
        *reinterpret_cast<double2*>(part1 + o) = make_double2(a0, a1);
        if (SECOND) *reinterpret_cast<double2*>(part2 + o) = make_double2(b0, b1);
    }
}

// S virtual permutations per permutation (LDS_SPLIT variant; 1 otherwise): their partial sums are added in the order (s, a).
// part2 == nullptr with GEARY: uniform row sums — the z^2 r term is rs_const * sum z^2 whatever the permutation.
template <bool GEARY>
__global__ __launch_bounds__(256) void k_perm_final_lds(const double* __restrict__ part1, const double* __restrict__ part2, int nch, int S,
                                                        int64_t pc, int64_t G, int64_t n, double W, const double* __restrict__ z2ss,
                                                        const double* __restrict__ qsum, const uint8_t* __restrict__ isconst,
                                                        double* __restrict__ sims, double rs_const) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (g >= G) return;
    const size_t o = (((size_t)(g >> 1) * pc * S + p * S) * nch) * GP + (g & 1);
    double s1 = 0.0, s2 = 0.0;
    for (int a = 0; a < nch * S; ++a) {  // (s, a) is contiguous: [vp = p * S + s][a]
        s1 += part1[o + (size_t)a * GP];
        if (GEARY && part2) s2 += part2[o + (size_t)a * GP];
    }
    if (GEARY && !part2) s2 = rs_const * z2ss[g];
    else if (GEARY && rs_const != 0.0) s2 += rs_const * z2ss[g];  // (the exception lists hold the departures from r0 = rs_const)
    double v;
    if (GEARY)
        v = ((double)(n - 1) * ((s2 - 2.0 * s1) + qsum[g])) / (2.0 * W * z2ss[g]);
    else
        v = (double)n / W * s1 / z2ss[g];
    sims[(size_t)p * G + g] = isconst[g] ? __builtin_nan("") : v;
}

// What gr/_ppatterns.py:474-492 takes out of the (P, G) permutation scores, formed where they are: per feature g
//   ge  = #{p : sims[p][g] >= score[g]}                                   `(sims >= score).sum(axis=0)`
//   sum = sims[:, g].sum()                                                `sims.sum(axis=0)`
//   var = mean(|x - sum / P|^2), std = sqrt(var)                          `np.var(sims, axis=0)`, `sims.std(axis=0)`
// bit for bit: numpy reduces the leading axis of a C-contiguous array by one rounded add per row, in row order
// (pairwise summation only applies along the contiguous axis), `_var` forms `arrmean = sum / P`, `x = arr - arrmean`,
// `x * x`, sums the same way and divides by P.  One thread per feature; every operation rounded separately.
//
// ONE feature in the whole call (`genes="x"`): the (P, 1) array is contiguous along the reduced axis too and numpy takes its
// other route — `pairwise_sum` of umath/loops_utils.h (fewer than 8 elements: in order; up to 128: eight interleaved partial
// sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail in order; longer: split at n/2 rounded down to a multiple
// of 8), applied to every buffer-sized run of 8192 elements, the runs added in order.  np_contiguous_sum restates that.
template <typename F>
__device__ double np_pairwise(int64_t lo, int64_t n, const F& at) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += at(lo + i);
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = at(lo + j);
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += at(lo + i + j);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += at(lo + i);
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise(lo, n2, at) + np_pairwise(lo + n2, n - n2, at);
}
template <typename F>
__device__ double np_contiguous_sum(int64_t n, const F& at) {
    double res = 0.0;
    for (int64_t c = 0; c < n; c += 8192) res += np_pairwise(c, (n - c < 8192) ? n - c : 8192, at);
    return res;
}

__global__ __launch_bounds__(256) void k_perm_stats(const double* __restrict__ sims, int64_t P, int64_t G, const double* __restrict__ score,
                                                    long long* __restrict__ ge, double* __restrict__ sum, double* __restrict__ sd,
                                                    double* __restrict__ var, int contiguous_column) {
    const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= G) return;
    const double sc = score[g];
    if (contiguous_column) {  // G == 1 here
        long long cnt = 0;
        for (int64_t p = 0; p < P; ++p) cnt += (sims[p] >= sc) ? 1 : 0;
        const double total = np_contiguous_sum(P, [&](int64_t p) { return sims[p]; });
        const double m = total / (double)P;
        const double v = np_contiguous_sum(P, [&](int64_t p) { const double d = sims[p] - m; return d * d; }) / (double)P;
        ge[g] = cnt;
        sum[g] = total;
        var[g] = v;
        sd[g] = sqrt(v);
        return;
    }
    double acc = 0.0;
    long long cnt = 0;
#pragma unroll 8
    for (int64_t p = 0; p < P; ++p) {  // (the loads are independent of the add chain: eight in flight per thread)
        const double x = sims[(size_t)p * G + g];
        acc += x;
        cnt += (x >= sc) ? 1 : 0;
    }
    const double m = acc / (double)P;
    double acc2 = 0.0;
#pragma unroll 8
    for (int64_t p = 0; p < P; ++p) {
        const double d = sims[(size_t)p * G + g] - m;
        acc2 += d * d;
    }
    const double v = acc2 / (double)P;
    ge[g] = cnt;
    sum[g] = acc;
    var[g] = v;
    sd[g] = sqrt(v);
}

__global__ void k_scores(int mode, int64_t G, int64_t n, double W, const double* __restrict__ num, const double* __restrict__ z2ss,
                         const uint8_t* __restrict__ isconst, double* __restrict__ out) {
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (g >= G) return;
    double v = (mode == 0) ? (double)n / W * num[g] / z2ss[g] : ((double)(n - 1) * num[g]) / (2.0 * W * z2ss[g]);
    out[g] = isconst[g] ? __builtin_nan("") : v;
}

}  // namespace sqgr

using namespace sqgr;

struct sqgr_autocorr {
    sqgr_ctx* ctx = nullptr;
    const sqgr_graph* g = nullptr;
    int64_t n = 0, G = 0, ntiles = 0;
    double W = 0.0;
    int Rcol = 32;
    DevBuf<double> Zt, Yt, Qt, rowsum, mean, z2ss, qsum, tmpG, colpart;
    DevBuf<uint8_t> isconst;
    // permutation workspace
    DevBuf<int32_t> idx;
    DevBuf<double> part1, part2, sims;
    DevBuf<double> sims_all;  // [P][G] scores of a whole permutation test kept on the device (sqgr_autocorr_perm_stats)
    PcgWorkspace pcg_ws;          // numpy-stream permutations generated in place (sqgr_autocorr_perms_pcg64)
    DevBuf<uint64_t> pcg_states;
    // LDS-bucketed permutation dot: gene-pair layout of Z and Y, and the bucket lists of the permutations in flight
    DevBuf<double> Zp, Yp;
    bool pairs_ready = false;
    // Geary's C under permutation needs sum_i z_i^2 r[idx_p(i)] with r = the graph's row sums.  On a row-normalised graph
    // (`transformation=True`, the reference's default, gr/_ppatterns.py:212-214) every row sum is 1 up to an ulp: the term is
    // r * sum z^2 for every permutation, and Geary's permutations run through the Moran kernel (two LDS reads per pair, not three)
    bool rs_uniform = false;
    double rs_const = 0.0;
    // ... and when they take a few distinct values (one per degree): class of every spot's row sum + the table (k_perm_dot_lds RMODE 2)
    int rs_classes = 0;  // 2..8: table mode available
    uint64_t cls_serial = 0;  // identifies this plan's class assignment (bucket lists carry the classes: part of their cache key)
    DevBuf<uint8_t> rcls;
    DevBuf<double> rtab;
    // ... and when one class holds most spots (a grid: all but its border): r0 * sum z^2 + exception lists (k_perm_dot_lds RMODE 3)
    bool rs_exc = false;
    int rs_main = 0;         // the class of r0
    double rs_main_val = 0.0;
    DevBuf<double> rtab_x;   // r_c - r0
    // what crosses PCIe per call — the observed scores in, G x 4 reductions out — goes through ONE persistent device block
    // [score | sum | std | var | n_ge] and its pinned twin, both made with the plan: no allocation, no pageable-copy staging and
    // one copy each way per sqgr_autocorr_perm_stats (round 5: three hipMalloc / hipFree and five pageable copies per call)
    DevBuf<double> stat_dev;
    double* stat_host = nullptr;
    int ensure_stat() {
        if (stat_dev.p && stat_host) return SQGR_OK;
        SQGR_TRY(stat_dev.alloc((size_t)5 * G));
        SQGR_HIP(hipHostMalloc(reinterpret_cast<void**>(&stat_host), (size_t)5 * G * sizeof(double), hipHostMallocDefault));
        return SQGR_OK;
    }
    ~sqgr_autocorr() {
        if (stat_host) (void)hipHostFree(stat_host);
    }
};

// 0: the gather kernel (k_perm_dot), 1: the LDS-bucketed kernel.  SQGR_AUTOCORR_KERNEL=gather|lds overrides the choice
// (tests run both); the LDS kernel needs <= LDS_MAX_CHUNKS chunks and pays off with many permutations per gene block.
// 2: the LDS kernel on LDS_SPLIT virtual permutations per permutation (fewer than 512 permutations; SQGR_AUTOCORR_KERNEL=lds-split).
static int perm_kernel_choice(int64_t n, int64_t G, int64_t P, bool geary) {
    int nch = 0;
    (void)lds_chunk(n, geary, &nch);
    if (nch > LDS_MAX_CHUNKS) return 0;
    if (const char* env = getenv("SQGR_AUTOCORR_KERNEL")) {
        if (!strcmp(env, "lds")) return 1;
        if (!strcmp(env, "lds-split")) return 2;
        if (!strcmp(env, "gather")) return 0;
    }
    if (G < 256 || n < 4096) return 0;
    // (measured at config 3's shape, 2048 genes: the Y chunks every workgroup streams through LDS cost the same however few
    // permutations there are — the gather kernel wins below ~40 permutations)
    return P >= 512 ? 1 : (P >= 40 ? 2 : 0);
}

// which k_perm_dot_lds instantiation serves a statistic on this plan: 0 Moran's I — and Geary's C when all row sums are equal —,
// 3 Geary's C as Moran's loop + exception lists (<= 8 distinct row sums, one of them on at least 3 spots in 4), 2 Geary's C through
// the class table (<= 8 distinct row sums), 1 Geary's C with the row sums of the chunk in LDS
static int lds_rmode(const sqgr_autocorr* h, int32_t mode) {
    if (mode != 1 || h->rs_uniform) return 0;
    return h->rs_classes ? (h->rs_exc ? 3 : 2) : 1;
}

// permutation scores of the pc permutations behind the bucket lists `pl`, through the LDS-bucketed kernel -> h->sims
static int perms_pass_lds(sqgr_autocorr* h, int32_t mode, int64_t pc_real, const PermListsView& pl, int split) {
    sqgr_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int64_t n = h->n, G = h->G, G2 = (G + 1) / 2;
    const bool geary_stat = mode == 1;
    const int rmode = lds_rmode(h, mode);
    const bool geary = rmode == 1;   // the kernel with the chunk's row sums in LDS: 4092-spot chunks
    const bool second = rmode != 0;  // a second partial sum (z^2 r) per lane
    int nch = 0;
    const int m = lds_chunk(n, geary, &nch);
    const int64_t pc = pc_real * split;  // lanes of the dot kernel: virtual permutations
    const int npg = (int)ceil_div(pc, 64);
    if (!h->pairs_ready) {
        SQGR_TRY(h->Zp.ensure((size_t)G2 * n * GP));
        SQGR_TRY(h->Yp.ensure((size_t)G2 * n * GP));
        LaunchTimer t(ctx, "autocorr_repack");
        const int64_t total = h->ntiles * n * GT;
        k_repack_pairs<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(h->Zt.p, n, h->ntiles, G2, h->Zp.p);
        k_repack_pairs<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(h->Yt.p, n, h->ntiles, G2, h->Yp.p);
        SQGR_HIP(hipGetLastError());
        h->pairs_ready = true;
    }
    SQGR_TRY(h->part1.ensure((size_t)G2 * pc * nch * GP));
    if (second) SQGR_TRY(h->part2.ensure((size_t)G2 * pc * nch * GP));
    const size_t lds = ((size_t)(2 * m + ZERO_ROWS) * GP + (geary ? (size_t)m : (rmode >= 2 ? (size_t)8 : 0))) * sizeof(double);
    // the split variant always launches whole workgroups: waves without a permutation group still move the Y chunks (with fewer
    // than m / 5 threads a chunk does not fit the staging registers and its loads are no longer prefetched)
    const int threads = split > 1 ? LDS_PERM_BLOCK : 64 * std::min(npg, LDS_PERM_BLOCK / 64);
    // chunks per XCD round (see k_perm_dot_lds): the power of two nearest sqrt(32 * Y chunk bytes / list bytes of one bucket)
    int a_per_xcd = 1;
    if (split == 1) {
        // many permutations (measured at config 3's shape, 1000 permutations): Moran's I 66.2 ms with one chunk per round, 63.3 with 2,
        // 62.4 with 4; Geary's C (24 instead of 16 LDS bytes per pair, 4092-spot chunks) 99.6 / 100.6 / 106.9 ms
        a_per_xcd = geary ? 1 : 4;
    } else {
        const double list_bytes = (double)npg * ((double)n / split / ((double)nch * nch) * 1.5) * 256.0;  // rows of 64 entries, ~+50 % padding
        // (measured at config 3's shape, 50 / 100 / 256 permutations: 4-8 chunks per round, -14 ... -27 % against one; twice the
        // square-root estimate, at most 8)
        const double want = 2.0 * std::sqrt(32.0 * (double)m * GP * 8 / std::max(list_bytes, 1.0));
        while (a_per_xcd * 2 <= 8 && (double)a_per_xcd < want) a_per_xcd *= 2;
    }
    const int pslots = 32 / a_per_xcd;
    dim3 grid((unsigned)(ceil_div(G2, 8 * pslots) * ceil_div(nch, a_per_xcd) * 256), (unsigned)ceil_div(npg, LDS_PERM_BLOCK / 64));
    {
        LaunchTimer t(ctx, split > 1 ? (geary_stat ? "autocorr_perm_dot_lds_split_geary" : "autocorr_perm_dot_lds_split_moran")
                                     : (geary_stat ? "autocorr_perm_dot_lds_geary" : "autocorr_perm_dot_lds_moran"));
#define SQGR_DOT_LDS(RM, RSRC, P2)                                                                                                            \
    do {                                                                                                                                      \
        if (lds > 64 * 1024)                                                                                                                  \
            SQGR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_perm_dot_lds<RM>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        k_perm_dot_lds<RM><<<grid, threads, lds, st>>>(h->Zp.p, h->Yp.p, RSRC, n, pc, npg, G2, m, nch, pl.len, pl.off, pl.base, pl.lists,      \
                                                       h->part1.p, P2, a_per_xcd, pl.xlen, pl.xoff, pl.xlists);                              \
    } while (0)
        if (rmode == 1) SQGR_DOT_LDS(1, h->rowsum.p, h->part2.p);
        else if (rmode == 2) SQGR_DOT_LDS(2, h->rtab.p, h->part2.p);
        else if (rmode == 3) SQGR_DOT_LDS(3, h->rtab_x.p, h->part2.p);
        else SQGR_DOT_LDS(0, h->rowsum.p, nullptr);
#undef SQGR_DOT_LDS
        SQGR_HIP(hipGetLastError());
    }
    {
        LaunchTimer t(ctx, "autocorr_perm_final");
        dim3 g2((unsigned)ceil_div(G, 256), (unsigned)pc_real);
        if (geary_stat)
            k_perm_final_lds<true><<<g2, 256, 0, st>>>(h->part1.p, second ? h->part2.p : nullptr, nch, split, pc_real, G, n, h->W, h->z2ss.p, h->qsum.p,
                                                       h->isconst.p, h->sims.p, rmode == 3 ? h->rs_main_val : (second ? 0.0 : h->rs_const));
        else
            k_perm_final_lds<false><<<g2, 256, 0, st>>>(h->part1.p, nullptr, nch, split, pc_real, G, n, h->W, h->z2ss.p, h->qsum.p, h->isconst.p, h->sims.p,
                                                        0.0);
        SQGR_HIP(hipGetLastError());
    }
    return SQGR_OK;
}

static int column_sum(sqgr_autocorr* h, int mode, const double* A, const double* B, double* out_dev) {
    sqgr_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int R = h->Rcol;
    dim3 grid(R, (unsigned)h->ntiles);
    const sqgr_graph* g = h->g;
    {
        LaunchTimer t(ctx, "autocorr_colsum");
        switch (mode) {
            case 0: k_colsum<0><<<grid, 256, 0, st>>>(A, B, h->n, R, nullptr, nullptr, nullptr, h->colpart.p); break;
            case 1: k_colsum<1><<<grid, 256, 0, st>>>(A, nullptr, h->n, R, nullptr, nullptr, nullptr, h->colpart.p); break;
            case 2: k_colsum<2><<<grid, 256, 0, st>>>(A, nullptr, h->n, R, nullptr, nullptr, nullptr, h->colpart.p); break;
            default: k_colsum<3><<<grid, 256, 0, st>>>(A, nullptr, h->n, R, g->indptr.p, g->indices.p, g->data.p, h->colpart.p); break;
        }
        SQGR_HIP(hipGetLastError());
        k_colsum_final<<<(unsigned)ceil_div(h->G, 256), 256, 0, st>>>(h->colpart.p, R, h->G, out_dev);
        SQGR_HIP(hipGetLastError());
    }
    return SQGR_OK;
}

// vals: host block (gene-major, or cell-major when `cell_major`), or NULL when the features are columns of the matrix `dm` already
// resident on the device: dev_cols[0 .. G) (a device array) when dev_cols != NULL, else [dev_col0, dev_col0 + G)
static int autocorr_create(sqgr_ctx* ctx, const sqgr_graph* g, const double* vals, int64_t G, bool cell_major, sqgr_autocorr** out,
                           const sqgr_matrix* dm = nullptr, int64_t dev_col0 = 0, const int32_t* dev_cols = nullptr) {
    SQGR_REQUIRE(ctx && g && (vals || dm) && out, "null argument");
    *out = nullptr;
    SQGR_REQUIRE(g->ctx == ctx, "graph belongs to a different context");
    SQGR_REQUIRE(g->has_data || g->nnz == 0, "graph was uploaded without edge weights");
    SQGR_REQUIRE(G >= 1, "G=%lld", (long long)G);
    SQGR_HIP(hipSetDevice(ctx->device));
    const int64_t n = g->n;
    sqgr_autocorr* h = new sqgr_autocorr();
    h->ctx = ctx;
    h->g = g;
    h->n = n;
    h->G = G;
    h->ntiles = ceil_div(G, GT);
    hipStream_t st = ctx->stream;
    int rc = SQGR_OK;
    auto fail = [&](int code) {
        delete h;
        return code;
    };
    const size_t tsz = (size_t)h->ntiles * n * GT;
    if ((rc = h->Zt.alloc(tsz)) || (rc = h->Yt.alloc(tsz)) || (rc = h->Qt.alloc(tsz)) || (rc = h->rowsum.alloc((size_t)n)) ||
        (rc = h->mean.alloc((size_t)G)) || (rc = h->z2ss.alloc((size_t)G)) || (rc = h->qsum.alloc((size_t)G)) ||
        (rc = h->tmpG.alloc((size_t)G)) || (rc = h->isconst.alloc((size_t)G)) ||
        (rc = h->colpart.alloc((size_t)h->ntiles * h->Rcol * GT)))
        return fail(rc);
    // stage the gene-major input in blocks of <= 256 genes (and <= ~256 MB) when it comes from the host; a block cut out of a matrix
    // that is resident on the device is staged whole (<= 2 GB: no wait for the staging buffer between its pieces — seven stream
    // synchronisations per 2048-gene block of config 3)
    int64_t gc_max = std::max<int64_t>(GT, std::min<int64_t>(256, ((int64_t)1 << 28) / (n * 8) / GT * GT));
    if (dm && (int64_t)n * G * 8 <= ((int64_t)2 << 30)) gc_max = std::max<int64_t>(gc_max, ceil_div(G, GT) * GT);
    DevBuf<double> X, D;
    if ((rc = X.alloc_pooled((size_t)gc_max * n))) return fail(rc);
    hipError_t e = hipSuccess;
    if (cell_major && !dm) {  // one contiguous upload of vals[n][G]; the gene blocks are cut out of it on the device
        if ((rc = D.alloc((size_t)n * G))) return fail(rc);
        e = hipMemcpyAsync(D.p, vals, (size_t)n * G * 8, hipMemcpyHostToDevice, st);
    }
    // (a column range of a dense float64 matrix is a plain transpose like the host's cell-major block: not timed as an expansion)
    const bool dm_expands = dm && (dev_cols || dm->kind != 0 || dm->f32);
    for (int64_t g0 = 0; g0 < G && e == hipSuccess; g0 += gc_max) {
        const int gc = (int)std::min<int64_t>(gc_max, G - g0);
        if (dm) {  // a list or a range of columns of the resident matrix: the gene block is formed from it on the device
            std::optional<LaunchTimer> t;
            if (dm_expands) t.emplace(ctx, "autocorr_expand");
            e = dev_cols ? expand_column_list(dm, dev_cols + g0, gc, X.p, st) : expand_column_range(dm, dev_col0, g0, gc, X.p, st);
        } else if (cell_major) {
            e = expand_dense_f64(D.p, G, n, g0, gc, X.p, st);
        } else {
            e = hipMemcpyAsync(X.p, vals + (size_t)g0 * n, (size_t)gc * n * 8, hipMemcpyHostToDevice, st);
        }
        if (e != hipSuccess) break;
        {
            LaunchTimer t(ctx, "autocorr_prepare");
            k_gene_stats<<<gc, 256, 0, st>>>(X.p, n, h->mean.p, h->isconst.p, g0);
            k_center_transpose<<<dim3((unsigned)ceil_div(n, GT), (unsigned)ceil_div(gc, GT)), 256, 0, st>>>(X.p, n, gc, g0, h->mean.p,
                                                                                                       h->Zt.p);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);  // X is reused by the next block
    }
    if (e == hipSuccess) {
        LaunchTimer t(ctx, "autocorr_spmv");
        k_rowsum<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(g->indptr.p, g->data.p, n, h->rowsum.p);
        k_spmv_tiles<<<dim3((unsigned)ceil_div(n, 4), (unsigned)h->ntiles), 256, 0, st>>>(g->indptr.p, g->indices.p, g->data.p, n,
                                                                                        h->Zt.p, h->Yt.p, h->Qt.p);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        set_error("autocorr prepare failed: %s", hipGetErrorString(e));
        return fail(SQGR_ERR_HIP);
    }
    if ((rc = column_sum(h, 1, h->Zt.p, nullptr, h->z2ss.p)) || (rc = column_sum(h, 2, h->Qt.p, nullptr, h->qsum.p))) return fail(rc);
    // W = sum of all weights (float64 accumulation, CSR order)
    std::vector<double> rs((size_t)n);
    e = hipMemcpyAsync(rs.data(), h->rowsum.p, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("autocorr prepare failed: %s", hipGetErrorString(e));
        return fail(SQGR_ERR_HIP);
    }
    double W = 0.0;
    for (int64_t i = 0; i < n; ++i) W += rs[i];
    h->W = W;
    {   // distinct values of the row sums (exact comparison): 1 -> the z^2 r term of Geary's permutations is a constant; <= 8 -> classes
        const char* env = getenv("SQGR_AUTOCORR_ROWSUM_CLASSES");
        const bool allow = !(env && atoi(env) == 0);
        double vals8[8];
        int nv = 0;
        std::vector<uint8_t> cls((size_t)std::max<int64_t>(n, 1), 0);
        for (int64_t i = 0; allow && i < n && nv <= 8; ++i) {
            int c = 0;
            while (c < nv && vals8[c] != rs[i]) ++c;
            if (c == nv) {
                if (nv == 8) {
                    nv = 9;
                    break;
                }
                vals8[nv++] = rs[i];
            }
            cls[i] = (uint8_t)c;
        }
        h->rs_uniform = allow && n > 0 && nv == 1;
        h->rs_const = nv >= 1 ? vals8[0] : 0.0;
        h->rs_classes = (allow && nv >= 2 && nv <= 8) ? nv : 0;
        if (h->rs_classes) {
            static std::atomic<uint64_t> serial{0};
            h->cls_serial = ++serial;
            double tab[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tab_x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int c = 0; c < nv; ++c) tab[c] = vals8[c];
            // one class on at least 3 spots in 4 (SQGR_AUTOCORR_ROWSUM_EXCEPTIONS=<max share of the others, default 0.25>; 0 disables):
            // its row sum becomes a constant term, the other spots' departures from it go through exception lists
            int64_t pop[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int64_t i = 0; i < n; ++i) pop[cls[i]] += 1;
            int cmain = 0;
            for (int c = 1; c < nv; ++c)
                if (pop[c] > pop[cmain]) cmain = c;
            double max_share = 0.25;
            if (const char* ex = getenv("SQGR_AUTOCORR_ROWSUM_EXCEPTIONS")) max_share = atof(ex);
            h->rs_exc = max_share > 0.0 && (double)(n - pop[cmain]) <= max_share * (double)n;
            h->rs_main = cmain;
            h->rs_main_val = vals8[cmain];
            for (int c = 0; c < nv; ++c) tab_x[c] = vals8[c] - vals8[cmain];
            if ((rc = h->rcls.alloc((size_t)n)) || (rc = h->rtab.alloc(8)) || (rc = h->rtab_x.alloc(8))) return fail(rc);
            e = hipMemcpyAsync(h->rcls.p, cls.data(), (size_t)n, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h->rtab.p, tab, sizeof(tab), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(h->rtab_x.p, tab_x, sizeof(tab_x), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                set_error("autocorr prepare failed: %s", hipGetErrorString(e));
                return fail(SQGR_ERR_HIP);
            }
        }
    }
    if ((rc = h->ensure_stat())) return fail(rc);
    *out = h;
    return SQGR_OK;
}

extern "C" {

int sqgr_autocorr_create(sqgr_ctx* ctx, const sqgr_graph* g, const double* vals, int64_t G, sqgr_autocorr** out) {
    return autocorr_create(ctx, g, vals, G, false, out);
}

int sqgr_autocorr_create_cm(sqgr_ctx* ctx, const sqgr_graph* g, const double* vals, int64_t G, sqgr_autocorr** out) {
    return autocorr_create(ctx, g, vals, G, true, out);
}

int sqgr_autocorr_create_cols(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_matrix* m, int64_t col0, int64_t G, sqgr_autocorr** out) {
    SQGR_REQUIRE(ctx && g && m && out, "null argument");
    SQGR_REQUIRE(m->ctx == ctx, "matrix belongs to a different context");
    SQGR_REQUIRE(m->n_rows == g->n, "matrix has %lld rows, the graph %lld", (long long)m->n_rows, (long long)g->n);
    SQGR_REQUIRE(col0 >= 0 && G >= 1 && col0 + G <= m->n_cols, "columns [%lld, %lld) outside the matrix (%lld columns)", (long long)col0,
                 (long long)(col0 + G), (long long)m->n_cols);
    return autocorr_create(ctx, g, nullptr, G, true, out, m, col0);
}

int sqgr_autocorr_create_colidx(sqgr_ctx* ctx, const sqgr_graph* g, const sqgr_matrix* m, const int32_t* cols, int64_t G,
                                sqgr_autocorr** out) {
    SQGR_REQUIRE(ctx && g && m && cols && out, "null argument");
    SQGR_REQUIRE(m->ctx == ctx, "matrix belongs to a different context");
    SQGR_REQUIRE(m->n_rows == g->n, "matrix has %lld rows, the graph %lld", (long long)m->n_rows, (long long)g->n);
    SQGR_REQUIRE(G >= 1, "G=%lld", (long long)G);
    for (int64_t k = 0; k < G; ++k)
        SQGR_REQUIRE(cols[k] >= 0 && cols[k] < m->n_cols, "cols[%lld]=%d outside the matrix (%lld columns)", (long long)k, cols[k], (long long)m->n_cols);
    SQGR_HIP(hipSetDevice(ctx->device));
    SQGR_TRY(m->ensure_by_column());
    DevBuf<int32_t> d_cols;
    SQGR_TRY(d_cols.alloc((size_t)G));
    SQGR_HIP(hipMemcpyAsync(d_cols.p, cols, (size_t)G * 4, hipMemcpyHostToDevice, ctx->stream));
    return autocorr_create(ctx, g, nullptr, G, true, out, m, 0, d_cols.p);  // synchronous on return: d_cols may go
}

int sqgr_autocorr_destroy(sqgr_autocorr* h) {
    if (!h) return SQGR_OK;
    (void)hipSetDevice(h->ctx->device);
    delete h;
    return SQGR_OK;
}

int sqgr_autocorr_scores(sqgr_autocorr* h, int32_t mode, double* out_scores) {
    SQGR_REQUIRE(h && out_scores, "null argument");
    SQGR_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (moran) or 1 (geary)");
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (mode == 0)
        SQGR_TRY(column_sum(h, 0, h->Zt.p, h->Yt.p, h->tmpG.p));
    else
        SQGR_TRY(column_sum(h, 3, h->Zt.p, nullptr, h->tmpG.p));
    SQGR_TRY(h->ensure_stat());
    k_scores<<<(unsigned)ceil_div(h->G, 256), 256, 0, st>>>(mode, h->G, h->n, h->W, h->tmpG.p, h->z2ss.p, h->isconst.p, h->stat_dev.p);
    SQGR_HIP(hipGetLastError());
    SQGR_HIP(hipMemcpyAsync(h->stat_host, h->stat_dev.p, (size_t)h->G * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    memcpy(out_scores, h->stat_host, (size_t)h->G * 8);
    return SQGR_OK;
}

// permutation scores for permutations [perm_begin, perm_end): row permutations injected from the host (perm_idx), drawn
// from numpy's streams on the device (pcg_states, one row per permutation of the range) or from the device generator
static int autocorr_perms(sqgr_autocorr* h, int32_t mode, const int32_t* perm_idx, const uint64_t* pcg_states, uint64_t seed,
                          int64_t perm_begin, int64_t perm_end, double* out_sims, double* dev_all = nullptr) {
    SQGR_REQUIRE(h && (out_sims || dev_all), "null argument");
    SQGR_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (moran) or 1 (geary)");
    SQGR_REQUIRE(perm_begin >= 0 && perm_end >= perm_begin, "bad permutation range");
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = h->n, G = h->G, P = perm_end - perm_begin;
    if (P == 0) return SQGR_OK;
    // permutations per pass: bound idx (4 n B each) and the partials (ntiles*R*64*8 B each, x2 for Geary) to ~1 GiB each
    int R = (int)std::min<int64_t>(64, std::max<int64_t>(1, ceil_div(2048, ceil_div(std::min<int64_t>(P, 1024), PERM_TILE) * 4)));
    R = (int)std::min<int64_t>(R, std::max<int64_t>(1, n / 256));
    const int64_t by_idx = std::max<int64_t>(PERM_TILE, ((int64_t)1 << 30) / (n * 4));
    const int rmode = lds_rmode(h, mode);
    const bool geary_lds = rmode == 1;  // layout of the LDS kernel (chunk length): only the row-sum-array variant differs from Moran's
    const int kernel = perm_kernel_choice(n, G, P, geary_lds);
    const bool use_lds = kernel != 0;
    const int split = kernel == 2 ? LDS_SPLIT : 1;
    int64_t by_part = std::max<int64_t>(PERM_TILE, ((int64_t)1 << 30) / ((int64_t)h->ntiles * R * GT * 8));
    int lm = 0, lnch = 0;  // chunk length and chunks of the LDS kernel
    if (use_lds) {
        lm = lds_chunk(n, geary_lds, &lnch);
        by_part = std::max<int64_t>(64, ((int64_t)1 << 30) / (((G + 1) / 2) * lnch * GP * 8 * split));
    }
    // The joint list schedule (k_bucket_order_joint) makes a permutation's summation order depend on the 15 permutations it shares a
    // `ds_read_b128` lane group with, so the LDS kernel works on whole 16-aligned groups of the GLOBAL permutation index: with the
    // device generator the range is widened to [begin - lead, end rounded up to 16) and the extra ("ghost") permutations are
    // generated, scheduled, scored and dropped — INSIDE ONE KERNEL a permutation's score does not depend on how a range was cut.
    // (The kernel itself is chosen from the length of the call's range, perm_kernel_choice: pieces on different sides of its
    // thresholds sum in different orders — include/sqgr.h says so; the front end always passes the whole range.  Injected
    // permutations and numpy's streams always start at permutation 0.)
    const bool ghosts = use_lds && !perm_idx && !pcg_states;
    const int64_t galign = 16 / split;  // (perm_slot: a service group holds 16 consecutive lanes = permutations, or 2 x 8 sub-lists)
    const int64_t lead = ghosts ? (perm_begin & (galign - 1)) : 0;
    const int64_t PV = ghosts ? ((lead + P + galign - 1) & ~(galign - 1)) : P;  // permutations the passes run over
    int64_t chunk = std::min<int64_t>(std::min<int64_t>(PV, 32768), std::min(by_idx, by_part));  // grid.y limit
    const int64_t wg_perms = LDS_PERM_BLOCK / split;  // permutations per workgroup of the LDS kernel
    if (use_lds && chunk > wg_perms) chunk = chunk / wg_perms * wg_perms;  // whole workgroups of permutations
    else if (use_lds && chunk < PV) chunk = std::max<int64_t>(galign, chunk / galign * galign);  // every pass starts a lane group
    SQGR_TRY(h->idx.ensure((size_t)chunk * n));
    if (!use_lds) {
        SQGR_TRY(h->part1.ensure((size_t)h->ntiles * chunk * R * GT));
        if (mode == 1) SQGR_TRY(h->part2.ensure((size_t)h->ntiles * chunk * R * GT));
    }
    SQGR_TRY(h->sims.ensure((size_t)chunk * G));
    if (pcg_states) SQGR_TRY(h->pcg_states.ensure((size_t)chunk * 4));
    if (perm_idx)
        for (int64_t t = 0; t < P * n; ++t)
            SQGR_REQUIRE(perm_idx[t] >= 0 && perm_idx[t] < n, "perm_idx[%lld]=%d outside [0,%lld)", (long long)t, perm_idx[t], (long long)n);
    const FeistelDomain dom = make_domain((uint32_t)n);
    for (int64_t c0 = 0; c0 < PV; c0 += chunk) {
        const int64_t pc = std::min(chunk, PV - c0);
        const int64_t real_lo = std::max(c0, lead), real_hi = std::min(c0 + pc, lead + P);  // this pass's part of the caller's range
        auto fill_idx = [&]() -> int {  // the pass's permutations -> h->idx
            if (perm_idx) {
                SQGR_HIP(hipMemcpyAsync(h->idx.p, perm_idx + (size_t)c0 * n, (size_t)pc * n * 4, hipMemcpyHostToDevice, st));
            } else if (pcg_states) {
                SQGR_HIP(hipMemcpyAsync(h->pcg_states.p, pcg_states + (size_t)c0 * 4, (size_t)pc * 32, hipMemcpyHostToDevice, st));
                SQGR_TRY(pcg_permutations_dev(ctx, h->pcg_ws, n, h->pcg_states.p, pc, h->idx.p, st));
            } else {
                LaunchTimer t(ctx, "autocorr_perm_indices");
                k_perm_indices<<<dim3((unsigned)ceil_div(n, 256), (unsigned)pc), 256, 0, st>>>(seed, perm_begin - lead + c0, n, dom, h->idx.p);
                SQGR_HIP(hipGetLastError());
            }
            return SQGR_OK;
        };
        if (use_lds) {
            // the LDS kernel walks bucket lists that depend on the permutations alone: the context's are reused if they are these,
            // and the indices are only generated when they are not
            PermListKey key;
            key.n = n;
            key.pc = pc;
            key.perm0 = (perm_idx || pcg_states) ? c0 : perm_begin - lead + c0;
            key.m = lm;
            key.nch = lnch;
            key.source = perm_idx ? PermSource::injected : (pcg_states ? PermSource::numpy : PermSource::device);
            key.seed = seed;
            key.states = pcg_states ? pcg_states + (size_t)c0 * 4 : nullptr;
            key.split = split;
            key.order = list_order_mode(split);
            key.row_classes = rmode == 2;
            key.exceptions = rmode == 3;
            key.cls_serial = rmode >= 2 ? h->cls_serial : 0;
            PermListsView pl;
            SQGR_TRY(lists_for(ctx, key, fill_idx, h->idx.p, h->rcls.p, h->rs_main, rmode != 0, &pl));
            SQGR_TRY(perms_pass_lds(h, mode, pc, pl, split));
            if (real_hi > real_lo) {
                const double* from = h->sims.p + (size_t)(real_lo - c0) * G;
                const size_t to = (size_t)(real_lo - lead) * G, bytes = (size_t)(real_hi - real_lo) * G * 8;
                if (dev_all) SQGR_HIP(hipMemcpyAsync(dev_all + to, from, bytes, hipMemcpyDeviceToDevice, st));
                if (out_sims) SQGR_HIP(hipMemcpyAsync(out_sims + to, from, bytes, hipMemcpyDeviceToHost, st));
            }
            SQGR_HIP(hipStreamSynchronize(st));
            continue;
        }
        SQGR_TRY(fill_idx());
        dim3 grid((unsigned)ceil_div(pc, PERM_TILE), (unsigned)R, (unsigned)h->ntiles);
        {
            LaunchTimer t(ctx, mode == 1 ? "autocorr_perm_dot_geary" : "autocorr_perm_dot_moran");
            if (mode == 1)
                k_perm_dot<true><<<grid, 256, 0, st>>>(h->Zt.p, h->Yt.p, h->rowsum.p, h->idx.p, n, pc, R, h->part1.p, h->part2.p);
            else
                k_perm_dot<false><<<grid, 256, 0, st>>>(h->Zt.p, h->Yt.p, h->rowsum.p, h->idx.p, n, pc, R, h->part1.p, nullptr);
            SQGR_HIP(hipGetLastError());
        }
        {
            LaunchTimer t(ctx, "autocorr_perm_final");
            dim3 g2((unsigned)ceil_div(G, 256), (unsigned)pc);
            if (mode == 1)
                k_perm_final<true><<<g2, 256, 0, st>>>(h->part1.p, h->part2.p, R, pc, G, n, h->W, h->z2ss.p, h->qsum.p, h->isconst.p, h->sims.p);
            else
                k_perm_final<false><<<g2, 256, 0, st>>>(h->part1.p, nullptr, R, pc, G, n, h->W, h->z2ss.p, h->qsum.p, h->isconst.p, h->sims.p);
            SQGR_HIP(hipGetLastError());
        }
        if (dev_all) SQGR_HIP(hipMemcpyAsync(dev_all + (size_t)c0 * G, h->sims.p, (size_t)pc * G * 8, hipMemcpyDeviceToDevice, st));
        if (out_sims) SQGR_HIP(hipMemcpyAsync(out_sims + (size_t)c0 * G, h->sims.p, (size_t)pc * G * 8, hipMemcpyDeviceToHost, st));
        SQGR_HIP(hipStreamSynchronize(st));
    }
    return SQGR_OK;
}

int sqgr_autocorr_perms(sqgr_autocorr* h, int32_t mode, const int32_t* perm_idx, uint64_t seed, int64_t perm_begin,
                        int64_t perm_end, double* out_sims) {
    return autocorr_perms(h, mode, perm_idx, nullptr, seed, perm_begin, perm_end, out_sims);
}

int sqgr_autocorr_perms_pcg64(sqgr_autocorr* h, int32_t mode, const uint64_t* pcg_states, int64_t n_perms, double* out_sims) {
    SQGR_REQUIRE(pcg_states && n_perms >= 0, "pcg_states is NULL or n_perms < 0");
    return autocorr_perms(h, mode, nullptr, pcg_states, 0, 0, n_perms, out_sims);
}

int sqgr_autocorr_perm_stats(sqgr_autocorr* h, int32_t mode, const int32_t* perm_idx, const uint64_t* pcg_states, uint64_t seed,
                             int64_t perm_begin, int64_t perm_end, const double* score, int64_t* out_ge, double* out_sum,
                             double* out_std, double* out_var, int32_t only_feature) {
    SQGR_REQUIRE(h && score && out_ge && out_sum && out_std && out_var, "null argument");
    SQGR_REQUIRE(!only_feature || h->G == 1, "only_feature is set for a block of %lld features", (long long)h->G);
    SQGR_REQUIRE(!(perm_idx && pcg_states), "perm_idx and pcg_states are mutually exclusive");
    SQGR_REQUIRE(perm_begin >= 0 && perm_end > perm_begin, "bad permutation range");
    sqgr_ctx* ctx = h->ctx;
    SQGR_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t G = h->G, P = perm_end - perm_begin;
    SQGR_TRY(h->sims_all.ensure((size_t)P * G));
    SQGR_TRY(autocorr_perms(h, mode, perm_idx, pcg_states, seed, (perm_idx || pcg_states) ? 0 : perm_begin, (perm_idx || pcg_states) ? P : perm_end,
                            nullptr, h->sims_all.p));
    SQGR_TRY(h->ensure_stat());
    double* d = h->stat_dev.p;  // [score | sum | std | var | n_ge]
    static_assert(sizeof(long long) == sizeof(double), "the n_ge column shares the block");
    memcpy(h->stat_host, score, (size_t)G * 8);
    SQGR_HIP(hipMemcpyAsync(d, h->stat_host, (size_t)G * 8, hipMemcpyHostToDevice, st));
    {
        LaunchTimer t(ctx, "autocorr_perm_stats");
        k_perm_stats<<<(unsigned)ceil_div(G, 256), 256, 0, st>>>(h->sims_all.p, P, G, d, reinterpret_cast<long long*>(d + 4 * G), d + G, d + 2 * G, d + 3 * G,
                                                                 only_feature ? 1 : 0);
        SQGR_HIP(hipGetLastError());
    }
    SQGR_HIP(hipMemcpyAsync(h->stat_host + G, d + G, (size_t)4 * G * 8, hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    memcpy(out_sum, h->stat_host + G, (size_t)G * 8);
    memcpy(out_std, h->stat_host + 2 * G, (size_t)G * 8);
    memcpy(out_var, h->stat_host + 3 * G, (size_t)G * 8);
    memcpy(out_ge, h->stat_host + 4 * G, (size_t)G * 8);
    return SQGR_OK;
}

/* the device generator's permutation indices (parity hook): int32[(perm_end-perm_begin)][n] */
int sqgr_autocorr_perm_indices(sqgr_ctx* ctx, int64_t n, uint64_t seed, int64_t perm_begin, int64_t perm_end, int32_t* out_idx) {
    SQGR_REQUIRE(ctx && out_idx && n > 0 && n < (int64_t)0x7fffffff && perm_begin >= 0 && perm_end >= perm_begin, "bad argument");
    SQGR_HIP(hipSetDevice(ctx->device));
    const int64_t P = perm_end - perm_begin;
    if (P == 0) return SQGR_OK;
    SQGR_REQUIRE(P <= 32768, "at most 32768 permutations per call");
    DevBuf<int32_t> d;
    SQGR_TRY(d.alloc((size_t)P * n));
    k_perm_indices<<<dim3((unsigned)ceil_div(n, 256), (unsigned)P), 256, 0, ctx->stream>>>(seed, perm_begin, n, make_domain((uint32_t)n), d.p);
    SQGR_HIP(hipGetLastError());
    SQGR_HIP(hipMemcpyAsync(out_idx, d.p, (size_t)P * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SQGR_HIP(hipStreamSynchronize(ctx->stream));
    return SQGR_OK;
}

}  // extern "C"
