// libsqgr: builder, schedulers and cache of the bucket lists that spatial_autocorr's LDS permutation dot walks (layout and
// constants: sqgr_autocorr_lists.h).  The lists depend on the permutations alone; nothing here knows of genes.
#include "sqgr_autocorr_lists.h"

namespace sqgr {

// len[pg][a][b] = longest list (over the 64 permutations of group pg) of bucket (a, b), rounded up to LIST_ROUND.
// grid (a, pg), one wave; lane = permutation.  Permutations >= pc have empty lists.
// S > 1: lane = virtual permutation vp = p * S + s, which owns the spots i = s (mod S) of permutation p; pc counts virtual ones.
// exc_cls != nullptr (RMODE 3, see "exception lists" below): xlen[pg][a] = the longest list of pairs whose j is not of class exc_main
__global__ __launch_bounds__(64) void k_bucket_count(const int32_t* __restrict__ idx, int64_t n, int64_t pc, int m, int nch, int S,
                                                     int round, uint32_t* __restrict__ len, const uint8_t* __restrict__ exc_cls,
                                                     int exc_main, uint32_t* __restrict__ xlen) {
    extern __shared__ uint32_t cnt[];  // [b][lane]
    const int lane = threadIdx.x, a = blockIdx.x;
    const int64_t pg = blockIdx.y, vp = pg * 64 + perm_slot(lane), p = vp / S;
    const int sub = (int)(vp - p * S);
    for (int b = 0; b < nch; ++b) cnt[b * 64 + lane] = 0;
    const float inv_m = 1.0f / (float)m;
    const int64_t i0 = (int64_t)a * m, i1 = min(n, i0 + m);
    uint32_t xc = 0;
    if (vp < pc) {
        const int32_t* row = idx + (size_t)p * n;
        if (exc_cls) {
#pragma unroll 8
            for (int64_t i = i0 + (sub - i0 % S + S) % S; i < i1; i += S) {
                const uint32_t j = (uint32_t)row[i];
                cnt[chunk_of(j, (uint32_t)m, inv_m) * 64 + lane] += 1;
                xc += exc_cls[j] != exc_main ? 1u : 0u;
            }
        } else {
#pragma unroll 8
            for (int64_t i = i0 + (sub - i0 % S + S) % S; i < i1; i += S) cnt[chunk_of((uint32_t)row[i], (uint32_t)m, inv_m) * 64 + lane] += 1;
        }
    }
    if (exc_cls) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) xc = max(xc, (uint32_t)__shfl_xor((int)xc, o, 64));
        if (lane == 0) xlen[(size_t)pg * nch + a] = (xc + EXC_UNROLL - 1) / EXC_UNROLL * EXC_UNROLL;
    }
    for (int b = 0; b < nch; ++b) {
        uint32_t v = cnt[b * 64 + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
        if (lane == 0) len[((size_t)pg * nch + a) * nch + b] = (v + (uint32_t)round - 1) / (uint32_t)round * (uint32_t)round;
    }
}

// off[pg][a][b] = rows (of 64 entries) in front of bucket (a, b) inside group pg's lists; total[pg] = rows of the group,
// total[npg + pg] = its longest list
__global__ __launch_bounds__(256) void k_bucket_offsets(const uint32_t* __restrict__ len, int nb, uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ total) {
    __shared__ uint32_t part[256], longest[256];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nb;
    const int per = (nb + 255) / 256;
    const int j0 = min(nb, tid * per), j1 = min(nb, j0 + per);
    uint32_t s = 0, mx = 0;
    for (int j = j0; j < j1; ++j) {
        s += len[base + j];
        mx = max(mx, len[base + j]);
    }
    part[tid] = s;
    longest[tid] = mx;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0, m2 = 0;
        for (int t = 0; t < 256; ++t) {
            const uint32_t v = part[t];
            part[t] = run;
            run += v;
            m2 = max(m2, longest[t]);
        }
        total[blockIdx.x] = run;
        total[gridDim.x + blockIdx.x] = m2;
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int j = j0; j < j1; ++j) {
        off[base + j] = run;
        run += len[base + j];
    }
}

// base[pg] = rows in front of group pg (exclusive prefix of total), base[npg] = all rows, base[npg + 1] = the longest list
__global__ void k_bucket_bases(const uint32_t* __restrict__ total, int npg, uint64_t* __restrict__ base) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t run = 0;
    uint32_t mx = 0;
    for (int g = 0; g < npg; ++g) {
        base[g] = run;
        run += total[g];
        mx = max(mx, total[npg + g]);
    }
    base[npg] = run;
    base[npg + 1] = mx;
}

// lists[(base[pg] + off[pg][a][b] + k) * 64 + lane] = (i - a*m) | (idx_p(i) - b*m) << 16, pairs in ascending i; the rest of
// the bucket's len[pg][a][b] rows = the padding pair (m, 0): row m of the Z chunk is zero.
// rcls != nullptr: bits 29..31 of a pair <- the row-sum class of its j (k_perm_dot_lds RMODE 2; m < 8192)
__global__ __launch_bounds__(64) void k_bucket_fill(const int32_t* __restrict__ idx, int64_t n, int64_t pc, int m, int nch, int S,
                                                    const uint32_t* __restrict__ len, const uint32_t* __restrict__ off,
                                                    const uint64_t* __restrict__ base, uint32_t* __restrict__ lists,
                                                    const uint8_t* __restrict__ rcls, const uint8_t* __restrict__ exc_cls, int exc_main,
                                                    const uint32_t* __restrict__ xlen, const uint32_t* __restrict__ xoff,
                                                    uint32_t* __restrict__ xlists, uint16_t* __restrict__ nlen) {
    extern __shared__ uint32_t cur[];  // [b][lane], then the nch row offsets of this (pg, a)
    const int lane = threadIdx.x, a = blockIdx.x;
    const int64_t pg = blockIdx.y, vp = pg * 64 + perm_slot(lane), p = vp / S;
    const int sub = (int)(vp - p * S);
    for (int b = 0; b < nch; ++b) cur[b * 64 + lane] = 0;
    const float inv_m = 1.0f / (float)m;
    const size_t bk = ((size_t)pg * nch + a) * nch;
    uint32_t* offl = cur + nch * 64;
    for (int b = lane; b < nch; b += 64) offl[b] = off[bk + b];
    __syncthreads();
    uint32_t* out = lists + (size_t)base[pg] * 64 + lane;
    uint32_t* xout = exc_cls ? xlists + (size_t)xoff[(size_t)pg * nch + a] * 64 + lane : nullptr;
    uint32_t xk = 0;
    const int64_t i0 = (int64_t)a * m, i1 = min(n, i0 + m);
    if (vp < pc) {
        const int32_t* row = idx + (size_t)p * n;
#pragma unroll 4
        for (int64_t i = i0 + (sub - i0 % S + S) % S; i < i1; i += S) {
            const uint32_t j = (uint32_t)row[i], b = chunk_of(j, (uint32_t)m, inv_m);
            const uint32_t k = cur[b * 64 + lane];
            cur[b * 64 + lane] = k + 1;
            out[((size_t)offl[b] + k) * 64] = (uint32_t)(i - i0) | ((j - b * (uint32_t)m) << 16) | (rcls ? (uint32_t)rcls[j] << 29 : 0u);
            if (exc_cls) {
                const uint32_t c = exc_cls[j];
                if (c != (uint32_t)exc_main) {
                    xout[(size_t)xk * 64] = (uint32_t)(i - i0) | (c << 29);
                    ++xk;
                }
            }
        }
    }
    const uint32_t pad = (uint32_t)m;
    for (int b = 0; b < nch; ++b) {
        const uint32_t l = len[bk + b];
        if (nlen) nlen[(bk + b) * 64 + lane] = (uint16_t)cur[b * 64 + lane];  // (the schedule kernels choose by the lists' lengths)
        for (uint32_t k = cur[b * 64 + lane]; k < l; ++k) out[((size_t)offl[b] + k) * 64] = pad;
    }
    if (exc_cls)
        for (const uint32_t l = xlen[(size_t)pg * nch + a]; xk < l; ++xk) xout[(size_t)xk * 64] = pad;
}

// Exception lists (k_perm_dot_lds RMODE 3, Geary's C): when most spots share ONE row sum r0, sum_i z_i^2 r[idx_p(i)] is
// r0 * sum z^2 (the same for every permutation) + sum over the pairs whose j has another row sum of z_i^2 (r[j] - r0).  Those
// pairs — a few per cent on a grid: its border — get a list of their own per (group, chunk a), whatever the chunk of j: an entry
// is (i - a*m) | class of r[j] << 29, the padding pair (m, class 0) reads the zero row of Z.
// (counted and filled by k_bucket_count / k_bucket_fill in the same pass over the permutations' indices)
// xoff[.] = exclusive prefix of xlen (rows of 64 entries), xoff[count] = all rows; one workgroup
__global__ __launch_bounds__(256) void k_exc_offsets(const uint32_t* __restrict__ xlen, int count, uint32_t* __restrict__ xoff) {
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    const int per = (count + 255) / 256;
    const int j0 = min(count, tid * per), j1 = min(count, j0 + per);
    uint32_t sum = 0;
    for (int j = j0; j < j1; ++j) sum += xlen[j];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const uint32_t v = part[t];
            part[t] = run;
            run += v;
        }
        xoff[count] = run;
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int j = j0; j < j1; ++j) {
        xoff[j] = run;
        run += xlen[j];
    }
}

// Bank-aware order of every lane's list (any order of a list is valid; the sum order stays fixed by construction).
// A `ds_read_b128` serves a wave in 4 groups of 16 lanes, one LDS cycle per group when the 16 rows fall into 16 different
// 4-bank slots (row index mod 16); random rows collide ~3-way (tools/ubench_lds_read.hip: 11.1 instead of 4.2 clk).  Here
// lane l' of a group reads a Z row of class (k + l') mod 16 at step k: entry j of class c goes to step ((c - l') mod 16) + 16 j;
// classes with fewer entries than steps leave holes, which take the surplus entries of the fuller classes (in class order)
// and then the padding pair.  Simulated: 2.85 -> 1.46 cycles per group on the Z side (the Y side stays random).
// grid (nch * nch buckets, groups); one wave; lists longer than ORDER_MAX rows are left as they are.
constexpr int ORDER_MAX = 320;
// The rotation l' = (global permutation index) mod 16 — every ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...,
// MI355X_MICROARCH.md §LDS) holds each residue once — and the schedule runs over the lane's OWN length rounded up to 16, so the
// order of a permutation's list depends on that permutation alone: results stay bit-identical however a range is split.
// cls_shift 0: classes of the Z row (i mod 16); 16: classes of the Y row instead (the Y side then runs conflict-free and the Z side
// random: Geary's C, see build_perm_lists).
__global__ __launch_bounds__(64) void k_bucket_order(int m, int nb, int64_t perm0, const uint32_t* __restrict__ len,
                                                     const uint32_t* __restrict__ off, const uint64_t* __restrict__ base,
                                                     uint32_t* __restrict__ lists, int cls_shift) {
    __shared__ uint32_t ent[ORDER_MAX * 64];   // [k][lane] the list as built (ascending i)
    __shared__ uint16_t hole[ORDER_MAX * 64];  // [s][lane] step of the lane's s-th hole
    __shared__ uint16_t ncls[16 * 64], rank[16 * 64], sbase[16 * 64];  // per lane and class: entries, running rank, surplus offset
    const int lane = threadIdx.x;
    const int64_t pg = blockIdx.y;
    const size_t bk = (size_t)pg * nb + blockIdx.x;
    const int L = (int)len[bk];
    if (L == 0 || L > ORDER_MAX) return;
    uint32_t* lst = lists + ((size_t)base[pg] + off[bk]) * 64 + lane;
    const uint32_t pad = (uint32_t)m;
    const int lp = (int)((perm0 + pg * 64 + lane) & 15);
    for (int c = 0; c < 16; ++c) ncls[c * 64 + lane] = rank[c * 64 + lane] = 0;
    int cnt = 0;
    for (int k0 = 0; k0 < L; k0 += 16) {  // L is a multiple of LIST_ROUND = 16: sixteen loads in flight per lane
        uint32_t e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = lst[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            ent[(k0 + u) * 64 + lane] = e[u];
            if (e[u] != pad) {
                ncls[((e[u] >> cls_shift) & 15u) * 64 + lane] += 1;
                ++cnt;
            }
        }
    }
    const int Lo = (cnt + 15) & ~15, D = Lo >> 4;  // own length: D demands of every class
    int surplus = 0;
    for (int c = 0; c < 16; ++c) {
        sbase[c * 64 + lane] = (uint16_t)surplus;
        surplus += max(0, (int)ncls[c * 64 + lane] - D);
    }
    int nholes = 0;
    for (int k = 0; k < L; ++k) {  // holes in step order; they hold the padding pair unless a surplus entry lands there
        const int c = (k + lp) & 15;
        if (k >= Lo || (k >> 4) >= (int)ncls[c * 64 + lane]) {
            if (k < Lo) {
                hole[nholes * 64 + lane] = (uint16_t)k;
                ++nholes;
            }
            lst[(size_t)k * 64] = pad;
        }
    }
    for (int k = 0; k < L; ++k) {
        const uint32_t e = ent[k * 64 + lane];
        if (e == pad) continue;
        const int c = (int)((e >> cls_shift) & 15u);
        const int j = rank[c * 64 + lane];
        rank[c * 64 + lane] = (uint16_t)(j + 1);
        const int pos = j < D ? ((c - lp) & 15) + 16 * j : (int)hole[((int)sbase[c * 64 + lane] + j - D) * 64 + lane];
        lst[(size_t)pos * 64] = e;
    }
}

// The JOINT schedule (round 4, the default): the order above makes one side of a pair conflict-free and leaves the other random
// (1.46 + 2.84 LDS cycles per 16-lane group and pair).  A list may be walked in ANY order, and the 16 permutations that share a
// `ds_read_b128` lane group can agree on theirs: lane l' still reads a Z row of class (k + l') mod 16 at step k, and among its pairs
// of that class it takes one whose Y row class no other lane of the group has taken at that step.  Simulated 1.32 + 1.67 cycles.
//   cell (zc, yc) = (i mod 16, j mod 16) of a pair; pool (lane, zc) = the lane's pairs with Z class zc.
//   main phase: thread (group q, offset o) owns the steps k = o + 16 j and the pools (lane, (o + l') mod 16) of its group — no
//     other thread touches them.  Per step it visits the 16 lanes, smallest pool first (fixed order), and gives each a free Y
//     class of its pool (rotating start) or, failing that, any.
//   surplus phase: pools fuller than the lane has rounds keep pairs, emptier ones leave holes; every lane fills its holes with the
//     remaining pairs that collide least with what the main phase gave the other lanes at that step (Y first, then Z).
// The schedule of a lane depends on the 15 lanes it shares the group with: the caller builds lists for whole 16-aligned groups of
// the GLOBAL permutation index (perm_slot; sqgr_autocorr_perms generates the missing neighbours), so a split range stays bit-identical.
// Lists longer than ORDER_SEG rows are scheduled in independent segments of ORDER_SEG rows (grid.z).  Out of place: src -> dst.
constexpr int ORDER_SEG = 256;

template <int N>
__device__ __forceinline__ uint32_t row_ror(uint32_t v) {  // the value of the lane N places along the 16-lane row (rotating)
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 | N, 0xf, 0xf, false);
}
// lane of `ds_read_b128` group q that holds residue r = lane mod 16 (groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32)
__device__ __forceinline__ int group_lane(int q, int r) {
    const bool mid = r >= 4 && r < 12;
    return (q >> 1) * 32 + (((q & 1) != 0) == mid ? r : 16 + r);
}

// grid (buckets * 4 lane groups, groups of 64 permutations, segments); 16 threads: the schedule is a chain of dependent LDS accesses,
// what counts is how many groups a CU holds at once (15 KiB of LDS each)
__global__ __launch_bounds__(16) void k_bucket_order_joint(int m, int nb, const uint32_t* __restrict__ len, const uint32_t* __restrict__ off,
                                                           const uint64_t* __restrict__ base, const uint32_t* __restrict__ src,
                                                           uint32_t* __restrict__ dst, const uint16_t* __restrict__ nlen, int longer_than) {
    __shared__ uint16_t cw[256 * 16];    // [cell][r] pairs of the cell not yet placed << 8 | cursor into stp (mod 256; cells ascending)
    __shared__ uint8_t stp[256 * 16];    // [.][r] the steps given to the lane's pairs, grouped by cell
    __shared__ uint16_t amask[16 * 16];  // [zc][r] Y classes pool (lane r, zc) still holds
    __shared__ uint16_t psize[16 * 16];  // [zc][r] pairs in pool (lane r, zc)
    __shared__ uint16_t hbits[16 * 16];  // [o][r] bit j: step o + 16 j of lane r is taken
    __shared__ uint32_t yz[ORDER_SEG];   // [k] Y classes (bits 0..15) and Z classes (16..31) the group reads at step k
    __shared__ uint16_t Dl[16];          // rounds of lane r (its own length / 16, rounded up)
    __shared__ int saturated;
    const int t = threadIdx.x, q = (int)(blockIdx.x & 3u);
    const int lane = group_lane(q, t);
    const int64_t pg = blockIdx.y;
    const size_t bk = (size_t)pg * nb + (blockIdx.x >> 2);
    const int L = (int)len[bk], s0 = (int)blockIdx.z * ORDER_SEG;
    if (s0 >= L) return;
    if (longer_than > 0) {  // only the lane groups whose longest list exceeds `longer_than` rows (the others: k_bucket_order_steps)
        uint32_t h = nlen[bk * 64 + lane];
        h = max(h, row_ror<1>(h));
        h = max(h, row_ror<2>(h));
        h = max(h, row_ror<4>(h));
        if ((int)max(h, row_ror<8>(h)) <= longer_than) return;
    }
    const int Ls = min(ORDER_SEG, L - s0);  // a multiple of 16
    const size_t row0 = ((size_t)base[pg] + off[bk] + (size_t)s0) * 64;
    const uint32_t* a = src + row0 + lane;
    uint32_t* d = dst + row0 + lane;
    const uint32_t pad = (uint32_t)m;
    for (int i = t; i < 256 * 8; i += 16) reinterpret_cast<uint32_t*>(cw)[i] = 0;
    for (int i = t; i < ORDER_SEG; i += 16) yz[i] = 0;
    if (t == 0) saturated = 0;
    __syncthreads();
    // --- thread = lane r: the cells of its list
    int cnt = 0;
    bool sat = false;
    for (int k0 = 0; k0 < Ls; k0 += 16) {
        uint32_t e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = a[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if ((e[u] & 0xffffu) < pad) {
                const int cell = ((((e[u] & 15u) << 4) | ((e[u] >> 16) & 15u))) * 16 + t;
                const uint32_t w = cw[cell];
                sat |= w >= 0xff00u;
                cw[cell] = (uint16_t)(w + 0x100u);
                ++cnt;
            }
    }
    if (sat) saturated = 1;
    __syncthreads();
    if (saturated) {  // 256 pairs of one lane in one cell (an 8-bit counter): such a list has one order
        for (int k = 0; k < Ls; ++k) d[(size_t)k * 64] = a[(size_t)k * 64];
        return;
    }
    Dl[t] = (uint16_t)((cnt + 15) >> 4);
    {
        int run = 0;
        for (int zc = 0; zc < 16; ++zc) {
            uint32_t mask = 0;
            int ps = 0;
#pragma unroll
            for (int y = 0; y < 16; ++y) {
                const int c = cw[(zc * 16 + y) * 16 + t] >> 8;
                cw[(zc * 16 + y) * 16 + t] = (uint16_t)((c << 8) | (run & 255));
                run += c;
                ps += c;
                mask |= c ? (1u << y) : 0u;
            }
            amask[zc * 16 + t] = (uint16_t)mask;
            psize[zc * 16 + t] = (uint16_t)ps;
        }
    }
    __syncthreads();
    // --- thread = offset o: the steps k = o + 16 j and the pools (lane r, (o + r) mod 16)
    {
        const int o = t;
        int Dmax = 0;
        uint64_t visit = 0;  // residues in visiting order, 4 bits each: smallest pool first
        {
            uint32_t key[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                key[r] = ((uint32_t)psize[((o + r) & 15) * 16 + r] << 4) | (uint32_t)r;
                Dmax = max(Dmax, (int)Dl[r]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int rank = 0;
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2) rank += key[r2] < key[r] ? 1 : 0;
                visit |= (uint64_t)r << (4 * rank);
            }
        }
        uint32_t taken[16];  // per lane: bit j = step o + 16 j given away
#pragma unroll
        for (int r = 0; r < 16; ++r) taken[r] = 0;
        for (int j = 0; j < Dmax; ++j) {
            const int k = o + 16 * j;
            uint32_t used = 0, zused = 0, got = 0;
            for (int i = 0; i < 16; ++i) {
                const int r = (int)((visit >> (4 * i)) & 15u);
                if (j >= (int)Dl[r]) continue;
                const int zc = (o + r) & 15;
                const uint32_t avail = amask[zc * 16 + r];
                if (!avail) continue;
                uint32_t pick = avail & ~used;
                if (!pick) pick = avail;
                const int s = (j * 5 + o * 3 + r * 7) & 15;
                const uint32_t rot = ((pick >> s) | (pick << (16 - s))) & 0xffffu;
                const int y = (__builtin_ctz(rot) + s) & 15;
                const int cell = (zc * 16 + y) * 16 + r;
                const uint32_t w = cw[cell];
                cw[cell] = (uint16_t)(((w - 0x100u) & 0xff00u) | ((w + 1u) & 0xffu));
                if ((w >> 8) == 1u) amask[zc * 16 + r] = (uint16_t)(avail & ~(1u << y));
                stp[(w & 0xffu) * 16 + r] = (uint8_t)k;
                used |= 1u << y;
                zused |= 1u << zc;
                got |= 1u << r;
            }
            yz[k] = used | (zused << 16);
#pragma unroll
            for (int r = 0; r < 16; ++r) taken[r] |= ((got >> r) & 1u) << j;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) hbits[o * 16 + r] = (uint16_t)taken[r];
    }
    __syncthreads();
    // --- thread = lane r: the pairs left over go to the lane's holes, judged by the classes the OTHER lanes read at a hole's step (as
    // the main phase left them: the lanes do this side by side).  Three sweeps over the holes: a pair that collides on neither
    // side, then one whose Y row does not collide, then any.
    {
        const uint32_t dmask = (1u << Dl[t]) - 1u;
        uint32_t zrem = 0;
        int rem = cnt;
        for (int c = 0; c < 16; ++c) {
            zrem |= amask[c * 16 + t] ? (1u << c) : 0u;
            rem -= __builtin_popcount(hbits[c * 16 + t]);
        }
        for (int lvl = 0; lvl < 3; ++lvl)
            for (int o2 = 0; o2 < 16; ++o2) {
                uint32_t hb = hbits[o2 * 16 + t];
                for (uint32_t hh = rem ? (~hb & dmask) : 0u; hh && rem; hh &= hh - 1) {
                    const int j = __builtin_ctz(hh), k = o2 + 16 * j;
                    const uint32_t w = yz[k];
                    for (uint32_t zcand = lvl == 0 ? (zrem & ~(w >> 16)) : zrem; zcand; zcand &= zcand - 1) {
                        const int zc = __builtin_ctz(zcand);
                        uint32_t am = amask[zc * 16 + t];
                        const uint32_t ym = (lvl == 2 ? am : (am & ~w)) & 0xffffu;
                        if (!ym) continue;
                        const int y = __builtin_ctz(ym);
                        const int cell = (zc * 16 + y) * 16 + t;
                        const uint32_t v = cw[cell];
                        cw[cell] = (uint16_t)(((v - 0x100u) & 0xff00u) | ((v + 1u) & 0xffu));
                        if ((v >> 8) == 1u) {
                            am &= ~(1u << y);
                            amask[zc * 16 + t] = (uint16_t)am;
                            if (!am) zrem &= ~(1u << zc);
                        }
                        stp[(v & 0xffu) * 16 + t] = (uint8_t)k;
                        hb |= 1u << j;
                        --rem;
                        break;
                    }
                }
                hbits[o2 * 16 + t] = (uint16_t)hb;
            }
    }
    // --- (same thread) every pair to its step — the cursors now stand at the end of their cells —, the padding pair elsewhere
    // (a padding pair: the zero row of the lane's own Z class at that step, a Y row of a class the main phase left free there)
    for (int k = 0; k < Ls; ++k)
        if (!((hbits[(k & 15) * 16 + t] >> (k >> 4)) & 1u)) {
            const uint32_t yfree = ~yz[k] & 0xffffu;
            const uint32_t rot = ((yfree >> t) | (yfree << (16 - t))) & 0xffffu;
            const uint32_t yc = yfree ? (uint32_t)((__builtin_ctz(rot) + t) & 15) : 0u;
            d[(size_t)k * 64] = (pad + (((uint32_t)(k + t) - pad) & 15u)) | (yc << 16);
        }
    for (int k0 = 0; k0 < Ls; k0 += 16) {
        uint32_t e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = a[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if ((e[u] & 0xffffu) < pad) {
                const int cell = ((((e[u] & 15u) << 4) | ((e[u] >> 16) & 15u))) * 16 + t;
                const uint32_t v = (uint32_t)cw[cell] - 1u;
                cw[cell] = (uint16_t)v;  // (only the cursor byte is read from here on)
                d[(size_t)stp[(v & 0xffu) * 16 + t] * 64] = e[u];
            }
    }
}

// The STEP schedule (the default): the rotation above gives every Z class the same number of slots in a lane's list, so the ~9 % of
// a lane's pairs that exceed their class's share land in other classes' holes and collide there.  A list of row classes can be cut
// into steps in which all 16 lanes read DIFFERENT Z classes whatever the counts (an edge colouring of the lanes x classes
// multigraph: as many steps as the longest lane or the fullest class needs, and the group's longest list leaves that slack).
// Step by step, for one lane group:
//   Z side, every four steps: the classes, fullest first (most pairs left over all lanes), each take the lane with the most pairs
//     left among the lanes that hold the class and have no class yet; a lane keeps its class for the four steps (idle if the pool
//     runs dry: simulated no worse, the Y side gains from drawing on one pool); a lane that can no longer afford to idle takes any
//     class it holds.
//   Y side, every step: the 16 Y classes in turn (rotating start) each take, among the lanes whose pool (lane, its Z class) holds
//     the class, the one with the fewest alternatives; a lane no class took reads a colliding one.
//   An idle lane reads a padding pair: the zero row (ZERO_ROWS) of a Z class and a Y row of a class nobody reads at that step.
// Simulated 1.02 + 1.34 cycles per step and group (the rotation: 1.39 + 1.67; random rows: 2.85 + 2.85).  "Class c takes the best
// lane that holds it" is integer arithmetic on a DPP row (one lane group = 16 threads): the lanes' holdings move to their places in
// order of preference (ds_permute), 16 wave ballots give every class's holders in that order, the turns are scalar arithmetic
// (lowest set bit = best holder still free), the lanes read their class back (ds_bpermute).  A workgroup is two lane groups,
// 32 KiB of LDS, 5 per CU; the kernel is bound by instruction issue (PMC: 35 % VALU, 24 % SALU of its wave cycles).
constexpr int STEP_SEG = 384;  // rows scheduled at a time (longer lists: independent segments, the full ones without slack)

__device__ __forceinline__ uint32_t row_or(uint32_t v) {
    v |= row_ror<1>(v);
    v |= row_ror<2>(v);
    v |= row_ror<4>(v);
    return v | row_ror<8>(v);
}
// position of the n-th (0-based) set bit of a 16-bit mask (n < popcount)
__device__ __forceinline__ uint32_t nth_set_bit(uint32_t mask, uint32_t n) {
    uint32_t pos = 0, c = (uint32_t)__builtin_popcount(mask & 0xffu);
    if (n >= c) { n -= c; pos = 8; }
    c = (uint32_t)__builtin_popcount((mask >> pos) & 0xfu);
    if (n >= c) { n -= c; pos += 4; }
    c = (uint32_t)__builtin_popcount((mask >> pos) & 0x3u);
    if (n >= c) { n -= c; pos += 2; }
    return pos + (n >= ((mask >> pos) & 1u) ? 1u : 0u);
}
// the lanes of the own row whose (distinct) key is larger, as a mask over the wave's lanes; src[N] = 1 << (lane row_ror<N> reads)
#define SQGR_ROW_OTHERS(M) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
struct RowSources {
    uint32_t bit[16];
};
__device__ __forceinline__ uint32_t row_higher(uint32_t key, const RowSources& src) {
    uint32_t hp = 0;
#define SQGR_HP(N) hp |= row_ror<N>(key) > key ? src.bit[N] : 0u;
    SQGR_ROW_OTHERS(SQGR_HP)
#undef SQGR_HP
    return hp;
}

// grid (buckets, groups of 64 permutations); 64 threads = a whole wavefront = the four lane groups of a bucket's 64 lists (round 5:
// 32 threads — two lane groups, half of every wave instruction masked off — until then; the step array, 432 of a thread's 1010
// bytes of LDS, now lives in a global scratch array shaped like the lists: fire-and-forget stores during the turns, read back by
// the last pass — 36 KiB per workgroup, four per CU = 16 lane groups in flight instead of 10).
// "Class c takes the best lane that holds it" = one wave ballot of the holders + each lane's mask of the better lanes of its row.
__global__ __launch_bounds__(64) void k_bucket_order_steps(int m, int nb, const uint32_t* __restrict__ len, const uint32_t* __restrict__ off,
                                                           const uint64_t* __restrict__ base, const uint32_t* __restrict__ src,
                                                           uint32_t* __restrict__ dst, const uint16_t* __restrict__ nlen,
                                                           uint16_t* __restrict__ stp_scr) {
    __shared__ uint8_t cnt[256 * 64];            // [cell][t] pairs of the cell not yet placed
    __shared__ uint8_t cur[256 * 64];            // [cell][t] slot of the cell's next pair, counted from the start of its pool
    __shared__ uint16_t pstart[17 * 64];         // [zc][t] pairs in the pools below zc; [16]: all
    __shared__ uint16_t amask[16 * 64];          // [zc][t] Y classes pool (lane, zc) still holds
    __shared__ int saturated[4];                 // per lane group
    const int t = threadIdx.x, r = t & 15;
    const int lane = group_lane(t >> 4, r);
    const int64_t pg = blockIdx.y;
    const size_t bk = (size_t)pg * nb + blockIdx.x;
    const int L = (int)len[bk];
    if (L == 0) return;
    // A lane group whose longest list fits STEP_SEG rows is scheduled here, in one piece; the others keep the rotation schedule in
    // segments (k_bucket_order_joint): cut into full segments the step schedule has no slack to work with (measured at 30 000 spots,
    // lists of ~830 pairs: 18.5 vs 17.2 ms).  The choice looks at the group's own lists only (split invariance).
    uint32_t horizon = nlen[bk * 64 + lane];
    horizon = max(horizon, row_ror<1>(horizon));
    horizon = max(horizon, row_ror<2>(horizon));
    horizon = max(horizon, row_ror<4>(horizon));
    horizon = (max(horizon, row_ror<8>(horizon)) + 15u) & ~15u;  // the group's longest list, rounded up to 16: its steps
    const bool mine = horizon <= (uint32_t)STEP_SEG;
    if (!__builtin_amdgcn_ballot_w64(mine)) return;
    const int Ls = min(STEP_SEG, L);  // a multiple of 16
    const size_t row0 = ((size_t)base[pg] + off[bk]) * 64;
    const uint32_t* a = src + row0 + lane;
    uint32_t* d = dst + row0 + lane;
    uint16_t* stp = stp_scr + row0 + lane;       // [slot * 64]: the step given to the lane's pair of that slot (slots < the lane's pairs <= L)
    const uint32_t pad = (uint32_t)m;
    for (int i = t; i < 256 * 16; i += 64) reinterpret_cast<uint32_t*>(cnt)[i] = 0;
    if (t < 4) saturated[t] = 0;
    __syncthreads();
    // --- thread = lane: the cells of its list
    uint32_t rem = 0;
    bool sat = false;
    for (int k0 = 0; k0 < Ls; k0 += 16) {
        uint32_t e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = a[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (mine && (e[u] & 0xffffu) < pad) {
                const int cell = ((((e[u] & 15u) << 4) | ((e[u] >> 16) & 15u))) * 64 + t;
                const uint32_t c = cnt[cell];
                sat |= c == 255u;
                cnt[cell] = (uint8_t)(c + 1u);
                ++rem;
            }
    }
    uint32_t cand = 0;  // Z classes the lane still holds pairs of
    {
        uint32_t run = 0;
        for (int zc = 0; zc < 16; ++zc) {
            uint32_t mask = 0, ps = 0;
#pragma unroll
            for (int y = 0; y < 16; ++y) {
                const uint32_t c = cnt[(zc * 16 + y) * 64 + t];
                cur[(zc * 16 + y) * 64 + t] = (uint8_t)ps;
                ps += c;
                mask |= c ? (1u << y) : 0u;
            }
            sat |= ps > 255u;
            amask[zc * 64 + t] = (uint16_t)mask;
            pstart[zc * 64 + t] = (uint16_t)run;
            run += ps;
            cand |= mask ? (1u << zc) : 0u;
        }
        pstart[16 * 64 + t] = (uint16_t)run;
    }
    if (sat) saturated[t >> 4] = 1;
    __syncthreads();
    bool mine_sched = mine;
    if (mine && saturated[t >> 4]) {  // 256 pairs of one lane in one Z class (8-bit counters): the group's lists stay as built
        for (int k = 0; k < L; ++k) d[(size_t)k * 64] = a[(size_t)k * 64];
        mine_sched = false;
        rem = 0;
        cand = 0;
    }
    if (!__builtin_amdgcn_ballot_w64(mine_sched)) return;
    uint32_t cdeg = 0;  // thread r of a row also keeps class r: the pairs of that class all 16 lanes still hold
#pragma unroll
    for (int l2 = 0; l2 < 16; ++l2) cdeg += (uint32_t)pstart[(r + 1) * 64 + (t & 48) + l2] - (uint32_t)pstart[r * 64 + (t & 48) + l2];
    RowSources rs;
    rs.bit[0] = 0;
#define SQGR_SRC(N) rs.bit[N] = 1u << (row_ror<N>((uint32_t)t) & 31u);  // (one bit per lane of the own row: distinct within a row)
    SQGR_ROW_OTHERS(SQGR_SRC)
#undef SQGR_SRC
    uint32_t sig_lo = 0, sig_hi = 0;  // the classes, fullest first, 4 bits each
    uint32_t zpos = 0;                // (byte address of) the lane's place in its row by pairs left, most first
    const uint32_t rowbase = (uint32_t)(t & 48);
    // "The classes in turn each take the best lane that holds them": the lanes' holdings are moved to their places in order of
    // preference (ds_permute), 16 wave ballots give every class's holders in that order, the turns are scalar arithmetic on the
    // masks (lowest set bit = best holder still free, one 16-bit half per lane group), and the lanes read their class back.
    auto take_turns = [&](const uint64_t (&holders)[16], uint64_t (&won)[16]) {
        uint64_t free_places = ~0ull;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint64_t h = holders[i] & free_places;
            const uint64_t f0 = h & 0xffffull, f1 = h & 0xffff0000ull, f2 = h & 0xffff00000000ull, f3 = h & 0xffff000000000000ull;
            won[i] = (f0 & (0ull - f0)) | (f1 & (0ull - f1)) | (f2 & (0ull - f2)) | (f3 & (0ull - f3));
            free_places &= ~won[i];
        }
    };
    uint32_t zkeep = 16;  // the lane's Z class of the current four steps
    // The steps of a lane group: its own longest list — NOT the bucket's rows (the longest of all 64 lanes): the schedule of a group
    // must not depend on the other groups (split invariance); the rows past it hold padding pairs.
    const uint32_t hz = mine_sched ? horizon : 0u;
    const int steps = (int)max(max((uint32_t)__builtin_amdgcn_readlane((int)hz, 0), (uint32_t)__builtin_amdgcn_readlane((int)hz, 16)),
                               max((uint32_t)__builtin_amdgcn_readlane((int)hz, 32), (uint32_t)__builtin_amdgcn_readlane((int)hz, 48)));
    if (mine_sched)
        for (int k = (int)horizon; k < L; ++k) d[(size_t)k * 64] = (pad + (((uint32_t)r - pad) & 15u)) | ((uint32_t)r << 16);
    for (int k = 0; k < steps; ++k) {
        if ((k & 3) == 0) {
            // Z side, every FOUR steps (a lane whose pool runs dry in between idles until the next turn: simulated no worse — the Y side
            // even gains from drawing on one pool — and the lane groups read distinct classes all the same): the classes, fullest
            // first, each take the lane with the most pairs left among their holders without a class
            const uint32_t ck = (cdeg << 4) | (uint32_t)(15 - r);
            const uint32_t rank = (uint32_t)__builtin_popcount(row_higher(ck, rs));
            sig_lo = row_or(rank < 8 ? (uint32_t)r << (4 * rank) : 0u);
            sig_hi = row_or(rank >= 8 ? (uint32_t)r << (4 * (rank - 8)) : 0u);
            zpos = (rowbase + (uint32_t)__builtin_popcount(row_higher((rem << 4) | (uint32_t)(15 - r), rs))) << 2;
            const uint32_t held = (uint32_t)__builtin_amdgcn_ds_permute((int)zpos, (int)(rem ? cand : 0u));  // (by place)
            uint32_t zi[16];
            uint64_t holders[16], won[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                zi[i] = ((i < 8 ? sig_lo : sig_hi) >> (4 * (i & 7))) & 15u;
                holders[i] = __builtin_amdgcn_ballot_w64(((held >> zi[i]) & 1u) != 0);
            }
            take_turns(holders, won);
            uint32_t zp = 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) zp = __builtin_amdgcn_inverse_ballot_w64(won[i]) ? zi[i] : zp;
            zkeep = (uint32_t)__builtin_amdgcn_ds_bpermute((int)zpos, (int)zp);
        }
        uint32_t myz = (rem && zkeep < 16 && ((cand >> zkeep) & 1u)) ? zkeep : 16u;
        if (rem && myz == 16 && rem + (uint32_t)k >= horizon) myz = (uint32_t)__builtin_ctz(cand);  // no step to spare: a class some lane may read
        const bool active = myz < 16;
        const uint32_t zused = row_or(active ? (1u << myz) : 0u);
        cdeg -= ((zused >> r) & 1u) && cdeg ? 1u : 0u;
        // Y side: the classes in turn (rotating start) each take the lane with the fewest alternatives among the lanes whose pool holds them
        const uint32_t av = active ? (uint32_t)amask[myz * 64 + t] : 0u;
        uint32_t myy = 16;
        {
            const uint32_t ykey = active ? (((17u - (uint32_t)__builtin_popcount(av)) << 4) | (uint32_t)(15 - r)) : (uint32_t)(15 - r);
            const uint32_t ypos = (rowbase + (uint32_t)__builtin_popcount(row_higher(ykey, rs))) << 2;
            const uint32_t held = (uint32_t)__builtin_amdgcn_ds_permute((int)ypos, (int)av);
            const uint32_t y0 = (uint32_t)(k * 5);
            uint64_t holders[16], won[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) holders[i] = __builtin_amdgcn_ballot_w64(((held >> ((y0 + (uint32_t)i) & 15u)) & 1u) != 0);
            take_turns(holders, won);
            uint32_t yp = 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) yp = __builtin_amdgcn_inverse_ballot_w64(won[i]) ? ((y0 + (uint32_t)i) & 15u) : yp;
            myy = (uint32_t)__builtin_amdgcn_ds_bpermute((int)ypos, (int)yp);
        }
        const bool unas = active && myy == 16;
        if (active && unas) myy = (uint32_t)__builtin_ctz(av);  // every class of the pool is taken: collide
        // the idle lanes read padding pairs: the zero row of a Z class and a Y row of a class no lane reads at this step
        const uint32_t idle = row_or(active ? 0u : (1u << r));
        const uint32_t yused = row_or(active ? (1u << myy) : 0u);
        if (active) {
            const int cell = (int)(myz * 16 + myy) * 64 + t;
            const uint32_t c = cnt[cell], slot = (uint32_t)pstart[myz * 64 + t] + cur[cell];
            cnt[cell] = (uint8_t)(c - 1u);
            cur[cell] = (uint8_t)(cur[cell] + 1u);
            if (c == 1u) {
                const uint32_t nav = av & ~(1u << myy);
                amask[myz * 64 + t] = (uint16_t)nav;
                if (!nav) cand &= ~(1u << myz);
            }
            stp[(size_t)slot * 64] = (uint16_t)k;
            --rem;
        } else if (mine_sched && (uint32_t)k < horizon) {
            const uint32_t nth = (uint32_t)__builtin_popcount(idle & ((1u << r) - 1u));  // (at least as many free classes as idle lanes)
            const uint32_t zc = nth_set_bit(~zused & 0xffffu, nth), yc = nth_set_bit(~yused & 0xffffu, nth);
            d[(size_t)k * 64] = (pad + ((zc - pad) & 15u)) | (yc << 16);
        }
    }
    __threadfence_block();  // the step array is read back by the lane that wrote it
    __syncthreads();
    // --- every pair to its step: the cursors now stand at the end of their cells
    for (int k0 = 0; k0 < Ls; k0 += 16) {
        uint32_t e[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) e[u] = a[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (mine_sched && (e[u] & 0xffffu) < pad) {
                const uint32_t zc = e[u] & 15u;
                const int cell = (int)((zc << 4) | ((e[u] >> 16) & 15u)) * 64 + t;
                const uint32_t within = (uint32_t)cur[cell] - 1u;
                cur[cell] = (uint8_t)within;
                const uint32_t slot = (uint32_t)pstart[zc * 64 + t] + (within & 0xffu);
                const uint32_t k = (uint32_t)stp[(size_t)slot * 64];
                d[(size_t)k * 64] = e[u];
            }
    }
}
#undef SQGR_ROW_OTHERS

}  // namespace sqgr

using namespace sqgr;

// the context's lists (sqgr_ctx::autocorr_lists) and the key they were built for
struct PermLists : sqgr::CtxCache {
    bool valid = false;
    PermListKey key;
    std::vector<uint64_t> states;            // what key.states points at
    DevBuf<uint32_t> b_len, b_off, b_total, lists, lists_raw;
    DevBuf<uint16_t> n_len;                  // [group][a][b][lane] pairs in the lane's list (the schedule kernels choose by them)
    DevBuf<uint16_t> stp_scr;                // scratch of k_bucket_order_steps, shaped like the lists: the step given to every pair
    DevBuf<uint32_t> x_len, x_off, x_lists;  // exception lists (see k_exc_offsets), when the lists serve RMODE 3
    DevBuf<uint64_t> b_base;
};

static PermLists* perm_lists(sqgr_ctx* ctx) {
    if (!ctx->autocorr_lists) ctx->autocorr_lists = new PermLists();
    return static_cast<PermLists*>(ctx->autocorr_lists);
}

int sqgr::list_order_mode(int split) {
    if (const char* e = getenv("SQGR_AUTOCORR_ORDER_LISTS"))
        if (atoi(e) == 0) return 0;
    const char* e_order = getenv("SQGR_AUTOCORR_ORDER");
    // (the split variant — lane = (permutation, spots i = s mod 8), sub-lists of ~30 pairs on two Z classes each — takes the joint
    // schedules like any other list: a lane group is two permutations x 8 sub-lists; round 3's per-list order has no use for it)
    if (e_order && !strcmp(e_order, "single")) return split == 1 ? 1 : 0;
    if (e_order && !strcmp(e_order, "rotation")) return 2;
    return 3;
}

// bucket lists of the pc permutations whose indices are in idx (the first one is permutation `perm0` of its stream) -> pl
// (split > 1: pc counts VIRTUAL permutations, idx holds pc / split index rows)
static int build_perm_lists(sqgr_ctx* ctx, PermLists* pl, const int32_t* idx, int64_t n, int64_t pc, int64_t perm0, int m, int nch, int split,
                            int order, bool geary, const uint8_t* rcls, const uint8_t* exc_cls = nullptr, int exc_main = 0) {
    hipStream_t st = ctx->stream;
    const int npg = (int)ceil_div(pc, 64);
    const bool order_lists = order != 0;
    const bool joint = order >= 2 && (perm0 * split) % 16 == 0;  // (the lane groups must be those of the global permutation index)
    const int round = (split > 1 && !joint) ? LIST_ROUND_SPLIT : LIST_ROUND;
    const int nb = nch * nch;
    SQGR_TRY(pl->b_len.ensure((size_t)npg * nb));
    SQGR_TRY(pl->b_off.ensure((size_t)npg * nb));
    SQGR_TRY(pl->b_total.ensure((size_t)npg * 2));
    SQGR_TRY(pl->b_base.ensure((size_t)npg + 2));
    const size_t cnt_lds = (size_t)nch * 64 * sizeof(uint32_t);
    uint64_t rows_max[2] = {0, 0};  // all rows, the longest list
    LaunchTimer t(ctx, "autocorr_bucket_lists");
    const int xcnt = npg * nch;
    uint32_t xrows = 0;
    if (exc_cls) {  // the pairs whose j has another row sum than most (RMODE 3) get lists of their own, built in the same two passes
        SQGR_TRY(pl->x_len.ensure((size_t)xcnt));
        SQGR_TRY(pl->x_off.ensure((size_t)xcnt + 1));
    }
    k_bucket_count<<<dim3((unsigned)nch, (unsigned)npg), 64, cnt_lds, st>>>(idx, n, pc, m, nch, split, round, pl->b_len.p, exc_cls, exc_main, pl->x_len.p);
    k_bucket_offsets<<<(unsigned)npg, 256, 0, st>>>(pl->b_len.p, nb, pl->b_off.p, pl->b_total.p);
    k_bucket_bases<<<1, 64, 0, st>>>(pl->b_total.p, npg, pl->b_base.p);
    if (exc_cls) k_exc_offsets<<<1, 256, 0, st>>>(pl->x_len.p, xcnt, pl->x_off.p);
    SQGR_HIP(hipGetLastError());
    SQGR_HIP(hipMemcpyAsync(rows_max, pl->b_base.p + npg, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (exc_cls) SQGR_HIP(hipMemcpyAsync(&xrows, pl->x_off.p + xcnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SQGR_HIP(hipStreamSynchronize(st));
    if (exc_cls && (pl->x_lists.n < (size_t)xrows * 64 + 64 || !pl->x_lists.p)) SQGR_TRY(pl->x_lists.alloc_pooled((size_t)xrows * 64 + (size_t)xrows * 4 + 64));
    const uint64_t rows = rows_max[0];
    // (with headroom: the next seed's lists are a few rows longer or shorter, and a new buffer of this size costs milliseconds)
    if (pl->lists.n < (size_t)rows * 64 || !pl->lists.p) SQGR_TRY(pl->lists.alloc_pooled((size_t)rows * 64 + (size_t)rows * 4));
    uint32_t* fill_to = pl->lists.p;
    if (joint) {  // out of place: the lists as built -> lists_raw, scheduled -> lists
        SQGR_TRY(pl->n_len.ensure((size_t)npg * nb * 64));
        if (pl->lists_raw.n < (size_t)rows * 64 || !pl->lists_raw.p) SQGR_TRY(pl->lists_raw.alloc_pooled((size_t)rows * 64 + (size_t)rows * 4));
        if (order == 3 && (pl->stp_scr.n < (size_t)rows * 64 || !pl->stp_scr.p)) SQGR_TRY(pl->stp_scr.alloc_pooled((size_t)rows * 64 + (size_t)rows * 4));
        fill_to = pl->lists_raw.p;
    }
    k_bucket_fill<<<dim3((unsigned)nch, (unsigned)npg), 64, cnt_lds + (size_t)nch * sizeof(uint32_t), st>>>(idx, n, pc, m, nch, split, pl->b_len.p, pl->b_off.p,
                                                                                                          pl->b_base.p, fill_to, rcls, exc_cls, exc_main,
                                                                                                          pl->x_len.p, pl->x_off.p, pl->x_lists.p,
                                                                                                          joint ? pl->n_len.p : nullptr);
    SQGR_HIP(hipGetLastError());
    if (joint) {
        // the step schedule takes the lane groups whose longest list fits STEP_SEG rows, the rotation schedule the others (in segments)
        if (order == 3 && rows_max[1] > 0)
            k_bucket_order_steps<<<dim3((unsigned)nb, (unsigned)npg), 64, 0, st>>>(m, nb, pl->b_len.p, pl->b_off.p, pl->b_base.p, pl->lists_raw.p,
                                                                                 pl->lists.p, pl->n_len.p, pl->stp_scr.p);
        const int longer_than = order == 3 ? STEP_SEG : 0;
        const int segs = (int64_t)rows_max[1] > longer_than ? (int)ceil_div((int64_t)rows_max[1], (int64_t)ORDER_SEG) : 0;
        if (segs > 0)
            k_bucket_order_joint<<<dim3((unsigned)nb * 4u, (unsigned)npg, (unsigned)segs), 16, 0, st>>>(m, nb, pl->b_len.p, pl->b_off.p, pl->b_base.p,
                                                                                                      pl->lists_raw.p, pl->lists.p, pl->n_len.p, longer_than);
        SQGR_HIP(hipGetLastError());
    } else if (order_lists && split == 1) {  // (the schedule works in rounds of 16 row classes; a sub-list of the split variant holds 2)
        // Geary's C reads TWO arrays through the Y index (the y row and the row sum): its lists are scheduled by the classes of the Y
        // row (measured 99.6 -> 94.4 ms per 2048 genes x 1000 permutations); Moran's I keeps the Z classes (66.2 vs 65.6 ms: no difference)
        const int cls_shift = geary ? 16 : 0;
        k_bucket_order<<<dim3((unsigned)nb, (unsigned)npg), 64, 0, st>>>(m, nb, perm0, pl->b_len.p, pl->b_off.p, pl->b_base.p, pl->lists.p, cls_shift);
        SQGR_HIP(hipGetLastError());
    }
    return SQGR_OK;
}

int sqgr::lists_for(sqgr_ctx* ctx, const PermListKey& key, const std::function<int()>& fill_idx, const int32_t* idx, const uint8_t* rcls, int exc_main,
                    bool by_y, PermListsView* out) {
    PermLists* pl = perm_lists(ctx);
    if (!(pl->valid && pl->key == key)) {
        SQGR_TRY(fill_idx());
        pl->valid = false;  // until complete
        SQGR_TRY(build_perm_lists(ctx, pl, idx, key.n, key.pc * key.split, key.perm0, key.m, key.nch, key.split, key.order, by_y,
                                  key.row_classes ? rcls : nullptr, key.exceptions ? rcls : nullptr, exc_main));
        pl->key = key;
        if (key.states) {  // the caller's states may go: the stored key points at a copy
            pl->states.assign(key.states, key.states + (size_t)key.pc * 4);
            pl->key.states = pl->states.data();
        }
        pl->valid = true;
    }
    *out = PermListsView{pl->b_len.p, pl->b_off.p, pl->b_base.p, pl->lists.p, pl->x_len.p, pl->x_off.p, pl->x_lists.p};
    return SQGR_OK;
}
