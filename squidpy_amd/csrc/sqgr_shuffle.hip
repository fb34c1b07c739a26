// libsqgr: the label generators of the permutation tests over cluster labels (sqgr_shuffle.h) — neighbourhood enrichment
// (sqgr_nhood.hip) and ligrec (sqgr_ligrec.hip) draw their shuffled label vectors here, so a given (seed, permutation index)
// means the same arrangement of the label multiset in every sq.gr function.
//   k_shuffle : thread per spot; B keyed Feistel bijections -> shuffled labels written as ONE B-byte
//               row per spot: slab[spot][b] (uint8).  One 16/32-byte gather later serves B permutations.
//   k_shuffle_tab : the same labels for 16-wide rows without libraries on up to 2^20 spots, at launch-group size: the first
//               round of the per-permutation network depends on the spot only through the high digit of its group image, so
//               each block tabulates it in LDS per row pair (64 KB) and a spot reads it back — 3 packed instructions per
//               permutation pair instead of 10 (launch_shuffle_raw selects; SQGR_SHUFFLE_TABLE=0|1|2).  The tables of a launch's
//               row pairs are built once, by k_shuffle_tab_build in front of it, and copied (SQGR_SHUFFLE_PRETAB=0: built by
//               every block, as before).  On tables whose only sentinel labels are the ranks >= n it runs without the sentinel test, and
//   k_shuffle_fix : behind it, thread per out-of-range rank and permutation, writes the labels whose first sigma image left
//               [0, n) from the inverse networks (SQGR_SHUFFLE_FIX=0|2).
// The numpy streams (PCG64 + Generator.shuffle) are sqgr_pcg.hip's; k_gather_labels16 applies their permutations to 16-bit labels.
#include "sqgr_shuffle.h"

#include <algorithm>
#include <cstdlib>

namespace sqgr {

// ---------------------------------------------------------------------------------------------- key generation
__global__ void k_keygen(uint64_t seed, int64_t perm0, int nrows, int B, int n_libs, uint32_t* __restrict__ keys) {
    const int items = B / FEISTEL_GROUP + B / 2;  // per (row, library)
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= (int64_t)nrows * n_libs * items) return;
    const int item = (int)(t % items);
    const uint32_t lib = (uint32_t)((t / items) % n_libs);
    const int64_t row = t / ((int64_t)items * n_libs);
    uint32_t* out = keys + row * key_words_per_row(B, n_libs);
    const int64_t perm_row = perm0 + row * B;
    if (item < B / FEISTEL_GROUP) {
        uint32_t rk[8];
        group_keys(seed, (uint64_t)(perm_row / FEISTEL_GROUP + item), lib, rk);
#pragma unroll
        for (int i = 0; i < 8; ++i) out[((size_t)item * n_libs + lib) * 8 + i] = (rk[i] & 0xFFFFu) * 0x10001u;
    } else {
        const int tt = item - B / FEISTEL_GROUP;
        uint32_t ra[2], rb[2];
        sigma_keys(seed, (uint64_t)(perm_row + 2 * tt), lib, ra);
        sigma_keys(seed, (uint64_t)(perm_row + 2 * tt + 1), lib, rb);
        uint32_t* o = out + (size_t)(B / FEISTEL_GROUP) * n_libs * 8 + ((size_t)tt * n_libs + lib) * 2;
        o[0] = (ra[0] & 0xFFFFu) | (rb[0] << 16);
        o[1] = (ra[1] & 0xFFFFu) | (rb[1] << 16);
    }
}

// keys of the INDEPENDENT variant (SQGR_SHUFFLE_INDEPENDENT=1, bench.py's `nhood_independent_bijections` leg): every permutation
// its own 8-round bijection, keyed like a row permutation of spatial_autocorr (round_keys: Philox counter words j = 0, 1) —
// [pair t < 8][round r < 8] per row of 16, permutation perm_row + 2t in the low half, + 2t + 1 in the high half
__global__ void k_keygen_indep(uint64_t seed, int64_t perm0, int nrows, uint32_t* __restrict__ keys) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= (int64_t)nrows * 8) return;
    const int64_t row = t / 8;
    const int pair = (int)(t % 8);
    uint32_t ra[8], rb[8];
    round_keys(seed, (uint64_t)(perm0 + row * 16 + 2 * pair), 0u, ra);
    round_keys(seed, (uint64_t)(perm0 + row * 16 + 2 * pair + 1), 0u, rb);
    uint32_t* out = keys + row * key_words_per_row(16, 1) + pair * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) out[r] = (ra[r] & 0xFFFFu) | (rb[r] << 16);
}

// ---------------------------------------------------------------------------------------------- label shuffle
// A uniformly random arrangement of the label multiset does not depend on the order of the base vector, so
// the base is taken *sorted by label* (inside each library): the label at sorted rank x is
//   #{k >= 1 : cum[k] <= x},   cum[k] = number of spots with label < k   (cum[K] = UINT_MAX sentinel).
// No memory gather: rank x = a*B + b arrives as its two digits; one LDS word per high digit a (block table, see
// LabelShuffler::create) holds the label of the block's first rank (byte 0) and the low digit where the next label starts
// (bits 16-31, 0xFFFF: none), so the label is `lab0 + (b >= next)`.  The value K — one past the last label — is the
// SENTINEL: blocks the two-field form cannot describe (several label starts, skipped empty categories) carry lab0 = K,
// and in the block that reaches past the library's last rank "next" is the first low digit outside [0, n) when that
// block ends in label K-1 (so the cycle-walking case yields K as well).  Sentinel bytes are rare (ranks >= n: fewer than
// 1 in B') and take the exact route afterwards: re-walk where x >= n, then x against the boundary table.
//   slab[(batch*n + i)*B + b] = label_at_rank( sigma_p( pi_g( rank_i ) ) ),  p = perm_row + b, g = p / 16
// One evaluation of the 8-round group bijection per spot and 16 permutations; per permutation the 2-round sigma network
// (two permutations per packed-16 instruction) and the table look-up: the compare reads its operands as 16-bit halves
// in place and the add-with-carry writes the label straight into its byte of the output word (SDWA) — two VALU
// instructions per label after the LDS read.
// label byte J of `word` <- e.byte0 + (b.half H >= e.half1)
template <int J, int H>
__device__ __forceinline__ void put_label(uint32_t& word, uint32_t e, uint32_t bpk, uint32_t zero) {
#define SQGR_PUT(JS, HS)                                                                                                      \
    asm("v_cmp_le_u32_sdwa vcc, %1, %2 src0_sel:WORD_1 src1_sel:WORD_" HS "\n\t"                                              \
        "v_addc_co_u32_sdwa %0, vcc, %1, %3, vcc dst_sel:BYTE_" JS " dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0 src1_sel:DWORD\n\t" \
        "s_nop 0"                                                                                                            \
        : "+v"(word)                                                                                                         \
        : "v"(e), "v"(bpk), "v"(zero)                                                                                        \
        : "vcc")
    if constexpr (J == 0 && H == 0) SQGR_PUT("0", "0");
    else if constexpr (J == 1 && H == 1) SQGR_PUT("1", "1");
    else if constexpr (J == 2 && H == 0) SQGR_PUT("2", "0");
    else if constexpr (J == 3 && H == 1) SQGR_PUT("3", "1");
    else static_assert(J < 0, "byte J of the word holds the permutation of packed half J & 1");
#undef SQGR_PUT
}

template <int B, bool HAS_LIBS, bool SMALLK>
__global__ __launch_bounds__(256) void k_shuffle(int64_t n, const uint32_t* __restrict__ cum, int kpad, int blk_words, int K,
                                                 const uint32_t* __restrict__ keys, LibDom dom0, int n_libs, int nrows,
                                                 const int32_t* __restrict__ lib_of, const int32_t* __restrict__ rank_of,
                                                 const LibDom* __restrict__ libdoms, uint8_t* __restrict__ slab_all, int pw,
                                                 const int32_t* __restrict__ spot_of) {
    // spot_of != NULL (no libraries): the plan lives on a RENUMBERED twin of the caller's graph (sqgr_graph_renumbered) — slab row i
    // belongs to the caller's observation spot_of[i], whose rank the generator permutes: the labels are the ones the plan on the
    // caller's own graph gives that observation, stored where the renumbered edge lists look for them
    extern __shared__ uint32_t s_lds[];               // [blk_words] block table (byte offset 0), then [n_libs][kpad] boundaries
    uint32_t* s_cum = s_lds + blk_words;
    for (int t = threadIdx.x; t < n_libs * kpad; t += 256) s_cum[t] = cum[t];
    for (int t = threadIdx.x; t < blk_words; t += 256) s_lds[t] = cum[n_libs * kpad + t];
    __syncthreads();
    // A thread evaluates TWO groups of 16 permutations per spot, one in each 16-bit half of the packed registers, so the
    // 8-round group bijection costs one packed evaluation per 32 labels: the two groups of a 32-permutation row, or the
    // groups of two consecutive 16-permutation rows (blockIdx.y counts row pairs then).
    constexpr int NG = B / FEISTEL_GROUP;
    const int row0 = (NG == 2) ? blockIdx.y : 2 * blockIdx.y;
    const int row1 = (NG == 2) ? row0 : min(row0 + 1, nrows - 1);  // an odd last row is paired with itself (stored once)
    const bool store1 = (NG == 2) || row0 + 1 < nrows;
    const size_t row_words = key_words_per_row(B, n_libs);
    const uint32_t* kgA = keys + (size_t)row0 * row_words;                                   // group keys of group A ...
    const uint32_t* kgB = (NG == 2) ? kgA + (size_t)n_libs * 8 : keys + (size_t)row1 * row_words;  // ... and of group B
    const uint32_t* ksA = keys + (size_t)row0 * row_words + (size_t)NG * n_libs * 8;         // sigma keys of group A's 8 pairs
    const uint32_t* ksB = (NG == 2) ? ksA + (size_t)(FEISTEL_GROUP / 2) * n_libs * 2
                                    : keys + (size_t)row1 * row_words + (size_t)NG * n_libs * 8;
    const uint32_t zero = 0;
    // any label byte >= K ?  K <= 126: bytes are < 128, adding 128 - K sets bit 7 exactly for the sentinels
    const uint32_t sent_add = (uint32_t)(128 - K) * 0x01010101u;
    // grid-stride over spots (launch_shuffle_raw caps the grid)
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    LibDom ld = dom0;
    uint32_t x0 = (uint32_t)i, lib = 0;
    if (HAS_LIBS) {
        lib = (uint32_t)lib_of[i];
        ld = libdoms[lib];
        x0 = (uint32_t)rank_of[i];
    } else if (spot_of) {
        x0 = (uint32_t)spot_of[i];
    }
    const FeistelDomain dom = ld.dom;
    const uint32_t* tab = s_cum + lib * kpad + 1;  // tab[k] = cum[k + 1]
    // The block table sits at LDS byte offset 0 (this kernel has no static LDS, the dynamic segment starts at 0): reading it
    // through an explicit address-space-3 address spares the add of the segment base the compiler otherwise emits per look-up.
    typedef __attribute__((address_space(3))) const uint32_t lds_word;
    const uint32_t blk_base = HAS_LIBS ? ld.aoff * 4u : 0u;
    auto blk_at = [&](uint32_t byte_off) { return *reinterpret_cast<lds_word*>((uintptr_t)(blk_base + byte_off)); };
    const uint32_t a0 = x0 / dom.B, b0 = x0 - a0 * dom.B;  // one division per spot, shared by all permutations

    // pi_gA (low halves) and pi_gB (high halves) in one packed evaluation; cycle walk per half (rare: < 1/B of the ranks)
    u16x2 ga = (u16x2)((unsigned short)a0), gb = (u16x2)((unsigned short)b0);
    {
        uint32_t kp[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) kp[r] = (kgA[(size_t)lib * 8 + r] & 0xFFFFu) | (kgB[(size_t)lib * 8 + r] & 0xFFFF0000u);
        const uint32_t* const pg[1] = {kp};
        bool need0 = true, need1 = true;
        do {
            u16x2 na[1] = {ga}, nb[1] = {gb};
            feistel_rounds<1>(na, nb, dom, pg);
            if (need0) { ga.x = na[0].x; gb.x = nb[0].x; }
            if (need1) { ga.y = na[0].y; gb.y = nb[0].y; }
            need0 = __umul24((uint32_t)ga.x, dom.B) + (uint32_t)gb.x >= dom.n;
            need1 = __umul24((uint32_t)ga.y, dom.B) + (uint32_t)gb.y >= dom.n;
        } while (need0 | need1);
    }
    // the 16 labels of one group: sigma_p on the group's image (in both halves), two permutations per packed evaluation
    auto emit_group = [&](const u16x2 gsa, const u16x2 gsb, const uint32_t* ks, uint32_t (&out)[4]) {
#pragma unroll
        for (int w = 0; w < FEISTEL_GROUP / 4; ++w) {
            uint32_t word = 0;
            uint32_t apk[2], bpk[2];  // sigma images of the word's two pairs (kept for the exact route)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const uint32_t* const pk[1] = {ks + ((size_t)(w * 2 + jj) * n_libs + lib) * 2};
                u16x2 a[1] = {gsa}, b[1] = {gsb};
                sigma_rounds<1>(a, b, dom, pk);
                apk[jj] = __builtin_bit_cast(uint32_t, a[0]);
                bpk[jj] = __builtin_bit_cast(uint32_t, b[0]);
                const uint32_t a4 = apk[jj] << 2;  // both halves at once (a < 2^14): byte offsets into the block table
                const uint32_t e0 = blk_at(a4 & 0xFFFFu);
                const uint32_t e1 = blk_at(a4 >> 16);
                if (jj == 0) {
                    put_label<0, 0>(word, e0, bpk[jj], zero);
                    put_label<1, 1>(word, e1, bpk[jj], zero);
                } else {
                    put_label<2, 0>(word, e0, bpk[jj], zero);
                    put_label<3, 1>(word, e1, bpk[jj], zero);
                }
            }
            bool sentinel;
            if constexpr (SMALLK) {
                sentinel = ((word + sent_add) & 0x80808080u) != 0;
            } else {  // K = 256 has no sentinel value left in a byte: every label takes the exact route
                const uint32_t k = (uint32_t)K;
                sentinel = k > 255u || (word & 0xFFu) >= k || ((word >> 8) & 0xFFu) >= k || ((word >> 16) & 0xFFu) >= k || (word >> 24) >= k;
            }
            if (sentinel) {  // exact route (rare): re-walk sigma where the image left [0, n), then rank against the boundaries
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (K <= 255 && ((word >> (8 * j)) & 0xFFu) < (uint32_t)K) continue;
                    const int jj = j >> 1, sh = (j & 1) * 16;
                    const uint32_t* sk = ks + ((size_t)(w * 2 + jj) * n_libs + lib) * 2;
                    const uint32_t k0 = (sk[0] >> sh) & 0xFFFFu, k1 = (sk[1] >> sh) & 0xFFFFu;
                    uint32_t a = (apk[jj] >> sh) & 0xFFFFu, b = (bpk[jj] >> sh) & 0xFFFFu;
                    uint32_t x = a * dom.B + b;
                    while (x >= dom.n) {
                        uint32_t t = b + feistel_F1(a, k0, dom.bsh);
                        t = t >= dom.B ? t - dom.B : t;
                        b = t >= dom.B ? t - dom.B : t;
                        a = (a + feistel_F1(b, k1, dom.ash)) & (dom.A - 1u);
                        x = a * dom.B + b;
                    }
                    const uint32_t e = blk_at(a * 4u);  // the table again: nearly always enough
                    uint32_t l = (e & 0xFFFFu) + (b >= (e >> 16) ? 1u : 0u);
                    if (l >= (uint32_t)K) {  // a block the two-field form cannot describe: rank against the boundaries, from the
                        l = K <= 255 ? (e >> 8) & 0xFFu : 0u;  // block's first label on (skewed cluster sizes: 1-3 steps instead of ~K/2)
                        while (x >= tab[l]) ++l;  // sentinel UINT_MAX stops it
                    }
                    word = (word & ~(0xFFu << (8 * j))) | (l << (8 * j));
                }
            }
            out[w] = word;
        }
    };
    uint32_t outA[4], outB[4];
    emit_group((u16x2)(ga.x), (u16x2)(gb.x), ksA, outA);
    if (store1) emit_group((u16x2)(ga.y), (u16x2)(gb.y), ksB, outB);
    if constexpr (NG == 2) {
        uint4* dst = reinterpret_cast<uint4*>(slab_all + ((size_t)row0 * n + i) * B);
        dst[0] = make_uint4(outA[0], outA[1], outA[2], outA[3]);
        dst[1] = make_uint4(outB[0], outB[1], outB[2], outB[3]);
    } else {
        slab_store16(slab_all + (size_t)row0 * n * 16, n, i, pw, outA[0], outA[1], outA[2], outA[3]);
        if (store1) slab_store16(slab_all + (size_t)row1 * n * 16, n, i, pw, outB[0], outB[1], outB[2], outB[3]);
    }
    }
}

// k_shuffle<16, false, *> with sigma's FIRST round read from an LDS table (no libraries, A <= SHUF_TAB_MAX_A; selection:
// launch_shuffle_raw).  All 16 permutations of a group start sigma from the same image (a, b) = pi_g(rank_i), and the first
// round  b' = (b + F_B(a, k0_p)) mod B  takes from the spot only the high digit a < A ~ sqrt(n): k_shuffle evaluates F_B once per
// (spot, permutation pair) — 1e6 x 8 evaluations per group for 1024 x 8 distinct values at n = 1e6.  Here every block builds
//   T[g][a][t] = (F_B(a, k0 of permutation 2t) mod B) | (F_B(a, k0 of permutation 2t + 1) mod B) << 16,   g < 2, a < A, t < 8
// (32 bytes per a and group, the packing of the sigma keys) for its row pair before the spot loop; a spot then reads its two rows
// with two 16-byte LDS loads per group, and round 1 of a pair is add / subtract / min: the stored value is < B, so b + T < 2B <=
// 2^15 has no 16-bit carry and ONE conditional subtraction reduces it — the same b' as the two subtractions of b + F_B, since
// (b + F) mod B == (b + (F mod B)) mod B (tests/test_shuffle_table_cpu.py).  10 packed instructions per pair become 3; round 2
// and the block-table look-up are k_shuffle's.  1024-thread blocks, two per CU (2 x 69 KB of LDS at A = 1024): <= 64 VGPRs.
// LDS: [blk_words] block table at byte offset 0, [kpad] boundaries, then T at word tab_word0.
// The spot loop carries nothing a label does not need (same labels, bit for bit — tests/test_shuffle_valu_*.py;
// profiles/shuffle_valu_before_after.md): C1 sits in a VGPR so that the key is v_pk_mad_u16's one scalar operand; without a spot
// map the rank's digits advance by the grid stride's instead of being divided out; pi_g's first walk runs unmasked and only an
// image outside [0, n) enters the masked loop; sigma's high digit is carried as the block table's byte offset (the exact route
// shifts it back); a word's first label is written with zero padding.  The sentinel test and the exact route are k_shuffle's,
// per word: one test per 16 labels with an exact route that starts again from the group image was built and measured slower —
// a WAVE meets a sentinel in 37 % of its groups at 1e6 spots, and every such group then walked all its words.
constexpr int SHUF_TAB_THREADS = 1024;
constexpr uint32_t SHUF_TAB_MAX_A = 1024;  // 2 groups x A x 32 bytes = 64 KB: two blocks per CU
constexpr int SHUF_TAB_BLOCKS_PER_CU = 20;  // grid cap (launch_shuffle_raw)
constexpr int SHUF_TAB_MIN_TRIPS = 16;      // automatic selection: spots per thread of a resident block (launch_shuffle_raw)
static_assert(SHUF_TAB_MAX_A * 4u <= (1u << 12), "k_shuffle_tab carries the high digit scaled by 4 in a 16-bit half: ash - 2 >= 4, a << 2 < 2^12");

// feistel_F2 with the multiplier C1 (both halves) in a register the caller keeps opaque to the compiler: v_pk_mad_u16 may name
// ONE scalar register on gfx9, so with C1 a scalar constant every uniform key word was first copied into a VGPR (one v_mov_b32
// per evaluation); with C1 in a VGPR the key is the instruction's scalar operand.
__device__ __forceinline__ u16x2 shuf_tab_F2(u16x2 v, u16x2 k, u16x2 sh, u16x2 c1) {
    u16x2 x = v * c1 + k;
    x = xorshift7_2(x);
    x *= (u16x2)(FEISTEL_C2);
    return x >> sh;
}
// x + y in both 16-bit halves as ONE 32-bit add of the bit-cast words (v_add_u32 instead of v_pk_add_u16: 2.9 against 4.2 clk per
// SIMD, profiles/r06_ubench_ops.json).  Exact iff the low halves' sum stays below 2^16 — nothing then carries into the high half;
// every call site states its bound.  They follow from make_domain (sqgr_rng.h) for every n <= 2^27: A = 2^m, 16 <= B <= A <= 2^14,
// Bmask + 1 = 2^ceil(log2 B) < 2B, F_A = x >> ash < A, F_B = x >> bsh <= Bmask (tests/test_shuffle_pretab_cpu.py).
__device__ __forceinline__ u16x2 add_nocarry(u16x2 x, u16x2 y) {
    return __builtin_bit_cast(u16x2, __builtin_bit_cast(uint32_t, x) + __builtin_bit_cast(uint32_t, y));
}
// feistel_rounds<1> on shuf_tab_F2
__device__ __forceinline__ void shuf_tab_rounds(u16x2& a, u16x2& b, const uint32_t (&kp)[8], u16x2 am, u16x2 ash, u16x2 bsh, u16x2 BB,
                                                u16x2 c1) {
#pragma unroll
    for (int r = 0; r < FEISTEL_ROUNDS; r += 2) {
        a = add_nocarry(a, shuf_tab_F2(b, __builtin_bit_cast(u16x2, kp[r]), ash, c1)) & am;      // a < A, F_A < A: < 2A <= 2^15
        u16x2 t = add_nocarry(b, shuf_tab_F2(a, __builtin_bit_cast(u16x2, kp[r + 1]), bsh, c1));  // b < B, F_B < 2B: < 3B < 2^16
        t = __builtin_elementwise_min(t, (u16x2)(t - BB));
        b = __builtin_elementwise_min(t, (u16x2)(t - BB));
    }
}
// put_label<0, 0> as the FIRST label of a word: the other three bytes are written as zeros (no cleared register to preserve)
__device__ __forceinline__ uint32_t first_label(uint32_t e, uint32_t bpk, uint32_t zero) {
    uint32_t word;
    asm("v_cmp_le_u32_sdwa vcc, %1, %2 src0_sel:WORD_1 src1_sel:WORD_0\n\t"
        "v_addc_co_u32_sdwa %0, vcc, %1, %3, vcc dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\t"
        "s_nop 0"
        : "=v"(word)
        : "v"(e), "v"(bpk), "v"(zero)
        : "vcc");
    return word;
}
// The FIX instance's form of a two-field block-table entry  first | boundary << 16  (LabelShuffler::create; it reads no sentinel
// entry):  first << 16 | (2^16 - boundary) mod 2^16,  and  (first + 1) << 16  for a boundary of 0.  A low digit b < B <= 2^14 added
// to it carries out of the low half exactly when b >= boundary (0xFFFF, "none", leaves 1 there: never), so byte 2 of the sum is
// first + (b >= boundary) — one add per label in place of the compare / add-with-carry pair, no vcc (tests/test_shuffle_carry_cpu.py).
// LabelShuffler::create never writes a boundary of 0 (a label that starts on offset 0 is the block's first label; a one-event entry
// needs ev_pos > 0), so that branch is a guard no table reaches on the device; the CPU test covers it.
__device__ __forceinline__ uint32_t carry_entry(uint32_t e) {
    const uint32_t first = e & 0xFFu, boundary = e >> 16;
    return boundary == 0u ? (first + 1u) << 16 : first << 16 | ((0x10000u - boundary) & 0xFFFFu);
}

// The tables of ALL row pairs of a launch, once (k_shuffle_tab<.., PRETAB = true> copies them): tabs[y][g][a][t] for row pair y =
// blockIdx.y, the words of the in-block build — feistel_F2 on the pair's k0 keys, one conditional subtraction — in the same order.
// 2 * A * 8 words per row pair; an odd last row is paired with itself, as in k_shuffle_tab.
__global__ __launch_bounds__(256) void k_shuffle_tab_build(const uint32_t* __restrict__ keys, FeistelDomain dom, int nrows,
                                                           uint32_t* __restrict__ tabs) {
    const int row0 = 2 * blockIdx.y;
    const int row1 = min(row0 + 1, nrows - 1);
    constexpr size_t row_words = key_words_per_row(16, 1);
    const uint32_t* ksA = keys + (size_t)row0 * row_words + 8;
    const uint32_t* ksB = keys + (size_t)row1 * row_words + 8;
    const u16x2 BB = (u16x2)((unsigned short)dom.B);
    const u16x2 bsh = (u16x2)((unsigned short)dom.bsh);
    const int words = (int)dom.A * 8;
    uint32_t* out = tabs + (size_t)blockIdx.y * 2 * words;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < words; idx += gridDim.x * 256) {
        const u16x2 av = (u16x2)((unsigned short)(idx >> 3));
        const int t = idx & 7;
        u16x2 fa = feistel_F2(av, __builtin_bit_cast(u16x2, ksA[t * 2]), bsh);
        u16x2 fb = feistel_F2(av, __builtin_bit_cast(u16x2, ksB[t * 2]), bsh);
        fa = __builtin_elementwise_min(fa, (u16x2)(fa - BB));
        fb = __builtin_elementwise_min(fb, (u16x2)(fb - BB));
        out[idx] = __builtin_bit_cast(uint32_t, fa);
        out[words + idx] = __builtin_bit_cast(uint32_t, fb);
    }
}

// NOMAP: no spot map — the rank of slab row i is i itself, and its digits (a0, b0) advance with the grid stride instead of being
// divided out per spot.
// FIX (launch_shuffle_raw decides; SQGR_SHUFFLE_FIX): no sentinel test and no exact route.  The only labels that need the route
// on an eligible table (LabelShuffler::fix_why) are those whose first sigma image is one of the A*B - n ranks outside [0, n) —
// 4.5e-4 of them at 1e6 spots, which a WAVE nevertheless met in 11 % of its words — and k_shuffle_fix, launched behind this
// kernel, writes exactly those from the inverse networks.  Here the entries of the blocks that reach past rank n (the partial
// block, which eligibility requires to end in label K - 1, and with B clamped to 16 whole blocks behind it) are replaced while
// the table is copied into LDS by  K - 1 | 0xFFFF << 16 : every byte this kernel stores is a label < K, whatever runs later.
// The same copy stores every entry in carry form (carry_entry): a label is one add, a word's four labels are assembled by two
// v_perm_b32 and an or — seven instructions per word, none of them on vcc, where the two-field look-up takes eight and four
// hand-written wait states.
// PRETAB (launch_shuffle_raw decides; SQGR_SHUFFLE_PRETAB): T depends on the row pair's sigma keys alone, yet every one of the
// launch's blocks of a row pair (62 at 1e6 spots x 160 rows) built it again.  k_shuffle_tab_build, launched in front of this kernel,
// computes the tables of all row pairs once into `tabs` — [row pair][g][a][t], the LDS image — and a block copies its 2 * A * 32
// bytes with 16-byte loads and stores.  PRETAB = false keeps the in-block build (tabs is not read).
template <bool SMALLK, bool NOMAP, bool FIX, bool PRETAB>
__global__ __launch_bounds__(SHUF_TAB_THREADS, 8) void k_shuffle_tab(int64_t n, const uint32_t* __restrict__ cum, int kpad, int blk_words, int K,
                                                                  const uint32_t* __restrict__ keys, LibDom dom0, int nrows,
                                                                  uint8_t* __restrict__ slab_all, int pw, const int32_t* __restrict__ spot_of,
                                                                  int tab_word0, const uint32_t* __restrict__ tabs) {
    static_assert(!FIX || (SMALLK && NOMAP), "the FIX pair runs without a spot map and with K <= 126 only");
    extern __shared__ uint32_t s_lds[];
    uint32_t* s_cum = s_lds + blk_words;
    if constexpr (FIX) {  // (the boundaries are the exact route's: not read here)
        const int past = (int)((uint32_t)n / dom0.dom.B);  // first block that holds a rank >= n
        for (int t = threadIdx.x; t < blk_words; t += SHUF_TAB_THREADS)
            s_lds[t] = carry_entry(t >= past ? ((uint32_t)(K - 1) | (0xFFFFu << 16)) : cum[kpad + t]);
    } else {
        for (int t = threadIdx.x; t < kpad; t += SHUF_TAB_THREADS) s_cum[t] = cum[t];
        for (int t = threadIdx.x; t < blk_words; t += SHUF_TAB_THREADS) s_lds[t] = cum[kpad + t];
    }
    const FeistelDomain dom = dom0.dom;
    const int row0 = 2 * blockIdx.y;
    const int row1 = min(row0 + 1, nrows - 1);  // an odd last row is paired with itself (stored once)
    const bool store1 = row0 + 1 < nrows;
    constexpr size_t row_words = key_words_per_row(16, 1);
    const uint32_t* kgA = keys + (size_t)row0 * row_words;  // group keys, then the sigma keys of the group's 8 pairs
    const uint32_t* kgB = keys + (size_t)row1 * row_words;
    const uint32_t* ksA = kgA + 8;
    const uint32_t* ksB = kgB + 8;
    const u16x2 BB = (u16x2)((unsigned short)dom.B);
    if constexpr (PRETAB) {  // the two tables of this row pair as k_shuffle_tab_build left them: A * 4 rows of 16 bytes, linear
        const int rows16 = (int)dom.A * 4;
        const uint4* src = reinterpret_cast<const uint4*>(tabs) + (size_t)blockIdx.y * rows16;
        uint4* dst = reinterpret_cast<uint4*>(s_lds + tab_word0);  // tab_word0 is a multiple of 8 words
        for (int t = threadIdx.x; t < rows16; t += SHUF_TAB_THREADS) dst[t] = src[t];
    } else {  // the two tables of this row pair: F_B <= Bmask < 2B, one conditional subtraction stores it mod B
        const u16x2 bsh = (u16x2)((unsigned short)dom.bsh);
        const int words = (int)dom.A * 8;
        for (int idx = threadIdx.x; idx < words; idx += SHUF_TAB_THREADS) {
            const u16x2 av = (u16x2)((unsigned short)(idx >> 3));
            const int t = idx & 7;
            u16x2 fa = feistel_F2(av, __builtin_bit_cast(u16x2, ksA[t * 2]), bsh);
            u16x2 fb = feistel_F2(av, __builtin_bit_cast(u16x2, ksB[t * 2]), bsh);
            fa = __builtin_elementwise_min(fa, (u16x2)(fa - BB));
            fb = __builtin_elementwise_min(fb, (u16x2)(fb - BB));
            s_lds[tab_word0 + idx] = __builtin_bit_cast(uint32_t, fa);
            s_lds[tab_word0 + words + idx] = __builtin_bit_cast(uint32_t, fb);
        }
    }
    __syncthreads();
    const uint32_t zero = 0;
    const uint32_t sent_add = (uint32_t)(128 - K) * 0x01010101u;
    const uint32_t* tab = s_cum + 1;  // tab[k] = cum[k + 1]
    typedef __attribute__((address_space(3))) const uint32_t lds_word;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const u32x4 lds_row;
    auto blk_at = [&](uint32_t byte_off) { return *reinterpret_cast<lds_word*>((uintptr_t)byte_off); };
    const uint32_t tabA = (uint32_t)tab_word0 * 4u, tabB = tabA + dom.A * 32u;  // byte offsets (multiples of 32)
    const u16x2 am = (u16x2)((unsigned short)(dom.A - 1u));
    const u16x2 ash = (u16x2)((unsigned short)dom.ash), bsh = (u16x2)((unsigned short)dom.bsh);
    // the high digit is carried scaled by 4, the byte offset into the block table:  ((gsa + (x >> ash)) & am) << 2  ==
    // ((gsa << 2) + (x >> (ash - 2))) & (am << 2)  in every 16-bit half — the two low bits of x >> (ash - 2) never carry into a sum
    // that is masked above them, and ash >= 6 (A <= 1024) keeps a << 2 < 2^12 (tests/test_shuffle_valu_cpu.py)
    const uint32_t am4w = (dom.A - 1u) << 2;  // the mask of ONE half: 4 (A - 1) < 2^12
    const u16x2 ash4 = (u16x2)((unsigned short)(dom.ash - 2u));
    uint32_t c1w = FEISTEL_C1 * 0x10001u;
    asm volatile("" : "+v"(c1w));  // opaque: stays a VGPR (shuf_tab_F2)
    const u16x2 c1 = __builtin_bit_cast(u16x2, c1w);
    const uint32_t n32 = (uint32_t)n, stride = gridDim.x * (uint32_t)SHUF_TAB_THREADS;  // n <= 2^20
    uint32_t i = blockIdx.x * (uint32_t)SHUF_TAB_THREADS + threadIdx.x;
    // NOMAP: ONE division per thread; a trip then adds the stride's digits with one conditional wrap (sa * B + sb == stride)
    // (the stride's digits are kept in VGPRs: as scalars they stay live through the loop and push key words into spill lanes)
    uint32_t sa = 0, sb = 0, a0 = 0, b0 = 0;
    if constexpr (NOMAP) {
        sa = stride / dom.B;
        sb = stride - sa * dom.B;
        asm volatile("" : "+v"(sa), "+v"(sb));
        a0 = i / dom.B;
        b0 = i - a0 * dom.B;
    }
    uint32_t kp[8];  // pi_g's packed keys, in VGPRs: eight scalars fewer live through the loop
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        kp[r] = (kgA[r] & 0xFFFFu) | (kgB[r] & 0xFFFF0000u);
        asm volatile("" : "+v"(kp[r]));
    }
    for (; i < n32; i += stride) {
    if constexpr (!NOMAP) {
        const uint32_t x0 = (uint32_t)spot_of[i];
        a0 = x0 / dom.B;
        b0 = x0 - a0 * dom.B;
    }
    // pi_gA (low halves) and pi_gB (high halves) in one packed evaluation.  The first walk runs without masks; an image outside
    // [0, n) (fewer than 1 in B of them) is walked again per half in a cold loop, as in k_shuffle
    u16x2 ga = (u16x2)((unsigned short)a0), gb = (u16x2)((unsigned short)b0);
    {
        shuf_tab_rounds(ga, gb, kp, am, ash, bsh, BB, c1);
        bool need0 = __umul24((uint32_t)ga.x, dom.B) + (uint32_t)gb.x >= dom.n;
        bool need1 = __umul24((uint32_t)ga.y, dom.B) + (uint32_t)gb.y >= dom.n;
        while (__builtin_expect(need0 | need1, 0)) {
            u16x2 na = ga, nb = gb;
            shuf_tab_rounds(na, nb, kp, am, ash, bsh, BB, c1);
            if (need0) { ga.x = na.x; gb.x = nb.x; }
            if (need1) { ga.y = na.y; gb.y = nb.y; }
            need0 = __umul24((uint32_t)ga.x, dom.B) + (uint32_t)gb.x >= dom.n;
            need1 = __umul24((uint32_t)ga.y, dom.B) + (uint32_t)gb.y >= dom.n;
        }
    }
    if constexpr (NOMAP) {
        a0 += sa;
        b0 += sb;
        if (b0 >= dom.B) { b0 -= dom.B; ++a0; }
    }
    // the 16 labels of one group: round 1 of sigma_p from the table row of the group image's high digit, round 2 as in k_shuffle
    auto emit_group = [&](const uint32_t ga1, const uint32_t gb1, const uint32_t row_off, const uint32_t* ks, uint32_t (&out)[4]) {
        const u16x2 gsa4 = (u16x2)((unsigned short)(ga1 << 2)), gsb = (u16x2)((unsigned short)gb1);
        const u32x4 r0 = *reinterpret_cast<lds_row*>((uintptr_t)row_off);
        const u32x4 r1 = *reinterpret_cast<lds_row*>((uintptr_t)(row_off + 16u));
        const uint32_t f1[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (int w = 0; w < FEISTEL_GROUP / 4; ++w) {
            uint32_t word;
            uint32_t a4pk[2], bpk[2];  // sigma images of the word's two pairs, the high digits scaled by 4 (kept for the exact route)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const u16x2 t = add_nocarry(gsb, __builtin_bit_cast(u16x2, f1[w * 2 + jj]));  // gsb < B, T < B: < 2B <= 2^15
                const u16x2 b = __builtin_elementwise_min(t, (u16x2)(t - BB));
                const u16x2 k1 = __builtin_bit_cast(u16x2, ks[(w * 2 + jj) * 2 + 1]);
                bpk[jj] = __builtin_bit_cast(uint32_t, b);
                // gsa4 < 4A, x >> ash4 < 4A: < 8A <= 2^13 (A <= SHUF_TAB_MAX_A)
                // the sum is kept unmasked: each half is masked where it becomes an address (the high one in one instruction, half
                // select and mask) or, on the exact route, a digit
                a4pk[jj] = __builtin_bit_cast(uint32_t, add_nocarry(gsa4, shuf_tab_F2(b, k1, ash4, c1)));
                const uint32_t e0 = blk_at(a4pk[jj] & am4w);
                const uint32_t e1 = blk_at((a4pk[jj] >> 16) & am4w);
                if constexpr (FIX) {  // carry-form entries: the label is byte 2 of entry + b (carry_entry)
                    const uint32_t r0 = e0 + (bpk[jj] & 0xFFFFu), r1 = e1 + (bpk[jj] >> 16);
                    if (jj == 0) word = __builtin_amdgcn_perm(r1, r0, 0x0c0c0602u);  // bytes 0, 1; zeros above
                    else word |= __builtin_amdgcn_perm(r1, r0, 0x06020c0cu);         // bytes 2, 3; zeros below
                } else if (jj == 0) {
                    word = first_label(e0, bpk[jj], zero);
                    put_label<1, 1>(word, e1, bpk[jj], zero);
                } else {
                    put_label<2, 0>(word, e0, bpk[jj], zero);
                    put_label<3, 1>(word, e1, bpk[jj], zero);
                }
            }
            bool sentinel;
            if constexpr (FIX) {  // no label is K: the table holds none, and k_shuffle_fix rewrites the images outside [0, n)
                sentinel = false;
            } else if constexpr (SMALLK) {
                sentinel = ((word + sent_add) & 0x80808080u) != 0;
            } else {  // K = 256 has no sentinel value left in a byte: every label takes the exact route
                const uint32_t k = (uint32_t)K;
                sentinel = k > 255u || (word & 0xFFu) >= k || ((word >> 8) & 0xFFu) >= k || ((word >> 16) & 0xFFu) >= k || (word >> 24) >= k;
            }
            if (sentinel) {  // exact route (rare), k_shuffle's: re-walk sigma with the real keys where the image left [0, n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (K <= 255 && ((word >> (8 * j)) & 0xFFu) < (uint32_t)K) continue;
                    const int jj = j >> 1, sh = (j & 1) * 16;
                    const uint32_t* sk = ks + (w * 2 + jj) * 2;
                    uint32_t a = ((a4pk[jj] >> sh) & am4w) >> 2, b = (bpk[jj] >> sh) & 0xFFFFu;
                    uint32_t x = a * dom.B + b;
                    if (x >= dom.n) {
                        const uint32_t k0 = (sk[0] >> sh) & 0xFFFFu, k1 = (sk[1] >> sh) & 0xFFFFu;
                        do {
                            uint32_t t = b + feistel_F1(a, k0, dom.bsh);
                            t = t >= dom.B ? t - dom.B : t;
                            b = t >= dom.B ? t - dom.B : t;
                            a = (a + feistel_F1(b, k1, dom.ash)) & (dom.A - 1u);
                            x = a * dom.B + b;
                        } while (x >= dom.n);
                    }
                    const uint32_t e = blk_at(a * 4u);  // the table again: nearly always enough
                    uint32_t l = (e & 0xFFFFu) + (b >= (e >> 16) ? 1u : 0u);
                    if (l >= (uint32_t)K) {  // a block the two-field form cannot describe: rank against the boundaries
                        l = K <= 255 ? (e >> 8) & 0xFFu : 0u;
                        while (x >= tab[l]) ++l;  // sentinel UINT_MAX stops it
                    }
                    word = (word & ~(0xFFu << (8 * j))) | (l << (8 * j));
                }
            }
            // The word is complete here, and the empty statement keeps it so: without the hand-written label instructions nothing
            // orders the words, and the compiler sinks group A's sixteen look-ups below group B's arithmetic — 55 VGPRs instead of
            // 39, 28 more wait states and a slower kernel, measured (profiles/shuffle_carry_before_after.md).  It is an asm
            // statement without an instruction: a scheduling anchor whose worth rests on this compiler's scheduler — after a
            // toolchain change read the instance's register count and measure the bracket with and without it again
            if constexpr (FIX) asm volatile("" : "+v"(word));
            out[w] = word;
        }
    };
    uint32_t outA[4], outB[4];
    emit_group((uint32_t)ga.x, (uint32_t)gb.x, tabA + (uint32_t)ga.x * 32u, ksA, outA);
    if (store1) emit_group((uint32_t)ga.y, (uint32_t)gb.y, tabB + (uint32_t)ga.y * 32u, ksB, outB);
    slab_store16(slab_all + (size_t)row0 * n * 16, n, i, pw, outA[0], outA[1], outA[2], outA[3]);
    if (store1) slab_store16(slab_all + (size_t)row1 * n * 16, n, i, pw, outB[0], outB[1], outB[2], outB[3]);
    }
}

// Behind k_shuffle_tab<true, true, true>: the labels whose first sigma image left [0, n).  They are not searched for: one thread
// per (row, permutation j < 16, out-of-range rank y = n + e, e < E = A*B - n) inverts both networks to the spot whose first
// image is y (shuffle_fix_target), walks sigma forward from y as the exact route does, ranks the end of the walk against the
// boundaries (cum[K] = UINT_MAX) and stores that one byte where slab_store16 put the spot's label j.  No lists, no atomics:
// every affected (spot, permutation) is reached by exactly one thread and no other byte is touched.  448 x 16 threads per row at
// 1e6 spots against 1e6 x 16 labels.
__global__ __launch_bounds__(256) void k_shuffle_fix(int64_t n, const uint32_t* __restrict__ cum, int K, const uint32_t* __restrict__ keys,
                                                     FeistelDomain dom, int nrows, uint32_t E, uint8_t* __restrict__ slab_all, int pw) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= (int64_t)nrows * FEISTEL_GROUP * E) return;
    const uint32_t e = (uint32_t)(t % E);
    const int j = (int)((t / E) % FEISTEL_GROUP);
    const int64_t row = t / ((int64_t)E * FEISTEL_GROUP);
    const uint32_t* krow = keys + (size_t)row * key_words_per_row(16, 1);  // group keys (both halves alike), then sigma's pairs
    const uint32_t* sk = krow + 8 + (j >> 1) * 2;
    const int sh = (j & 1) * 16;
    uint32_t spot, x;
    if (!shuffle_fix_target(dom.n + e, dom, krow, (sk[0] >> sh) & 0xFFFFu, (sk[1] >> sh) & 0xFFFFu, &spot, &x)) return;
    uint32_t lo = 0, hi = (uint32_t)K - 1u;  // the label of rank x: the first l with x < cum[l + 1]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (x < cum[mid + 1]) hi = mid; else lo = mid + 1;
    }
    slab_all[(size_t)row * n * 16 + slab_label_offset(n, spot, pw, j)] = (uint8_t)lo;
}

// The generator WITHOUT its shortcut (what do 16 independent bijections cost?): slab label b of row `row` =
// label_at_rank(pi_p(rank_i)) with pi_p the full 8-round bijection of permutation p = perm_row + b itself — no group bijection
// shared by 16 permutations, no 2-round sigma network.  Two permutations per packed evaluation, 8 evaluations of 8 rounds per spot
// and row (the two-level kernel: half an evaluation of 8 rounds + 8 of 2).  Same label look-up (block table, sentinel, exact
// route), same slab layout; no libraries.  Restated in oracle/devrng.py (independent_label_permutations).
template <bool SMALLK>
__global__ __launch_bounds__(256) void k_shuffle_indep(int64_t n, const uint32_t* __restrict__ cum, int kpad, int blk_words, int K,
                                                       const uint32_t* __restrict__ keys, LibDom dom0, uint8_t* __restrict__ slab_all, int pw) {
    extern __shared__ uint32_t s_lds[];
    uint32_t* s_cum = s_lds + blk_words;
    for (int t = threadIdx.x; t < kpad; t += 256) s_cum[t] = cum[t];
    for (int t = threadIdx.x; t < blk_words; t += 256) s_lds[t] = cum[kpad + t];
    __syncthreads();
    const int row = blockIdx.y;
    const uint32_t* krow = keys + (size_t)row * key_words_per_row(16, 1);
    const uint32_t zero = 0;
    const uint32_t sent_add = (uint32_t)(128 - K) * 0x01010101u;
    const FeistelDomain dom = dom0.dom;
    const uint32_t* tab = s_cum + 1;
    typedef __attribute__((address_space(3))) const uint32_t lds_word;
    auto blk_at = [&](uint32_t byte_off) { return *reinterpret_cast<lds_word*>((uintptr_t)byte_off); };
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t x0 = (uint32_t)i;
        const uint32_t a0 = x0 / dom.B, b0 = x0 - a0 * dom.B;
        uint32_t out[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            uint32_t word = 0, apk[2], bpk[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const uint32_t* const pk[1] = {krow + (w * 2 + jj) * 8};
                u16x2 ga = (u16x2)((unsigned short)a0), gb = (u16x2)((unsigned short)b0);
                bool need0 = true, need1 = true;
                do {  // the bijection, cycle-walked per half
                    u16x2 na[1] = {ga}, nb[1] = {gb};
                    feistel_rounds<1>(na, nb, dom, pk);
                    if (need0) { ga.x = na[0].x; gb.x = nb[0].x; }
                    if (need1) { ga.y = na[0].y; gb.y = nb[0].y; }
                    need0 = __umul24((uint32_t)ga.x, dom.B) + (uint32_t)gb.x >= dom.n;
                    need1 = __umul24((uint32_t)ga.y, dom.B) + (uint32_t)gb.y >= dom.n;
                } while (need0 | need1);
                apk[jj] = __builtin_bit_cast(uint32_t, ga);
                bpk[jj] = __builtin_bit_cast(uint32_t, gb);
                const uint32_t a4 = apk[jj] << 2;
                const uint32_t e0 = blk_at(a4 & 0xFFFFu);
                const uint32_t e1 = blk_at(a4 >> 16);
                if (jj == 0) {
                    put_label<0, 0>(word, e0, bpk[jj], zero);
                    put_label<1, 1>(word, e1, bpk[jj], zero);
                } else {
                    put_label<2, 0>(word, e0, bpk[jj], zero);
                    put_label<3, 1>(word, e1, bpk[jj], zero);
                }
            }
            bool sentinel;
            if constexpr (SMALLK) {
                sentinel = ((word + sent_add) & 0x80808080u) != 0;
            } else {
                const uint32_t k = (uint32_t)K;
                sentinel = k > 255u || (word & 0xFFu) >= k || ((word >> 8) & 0xFFu) >= k || ((word >> 16) & 0xFFu) >= k || (word >> 24) >= k;
            }
            if (sentinel) {  // a block the two-field table form cannot describe: rank against the boundaries (the image is < n already)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (K <= 255 && ((word >> (8 * j)) & 0xFFu) < (uint32_t)K) continue;
                    const int jj = j >> 1, sh = (j & 1) * 16;
                    const uint32_t a = (apk[jj] >> sh) & 0xFFFFu, b = (bpk[jj] >> sh) & 0xFFFFu;
                    const uint32_t x = a * dom.B + b;
                    const uint32_t e = blk_at(a * 4u);
                    uint32_t l = (e & 0xFFFFu) + (b >= (e >> 16) ? 1u : 0u);
                    if (l >= (uint32_t)K) {
                        l = K <= 255 ? (e >> 8) & 0xFFu : 0u;  // (the block's first label: k_shuffle)
                        while (x >= tab[l]) ++l;
                    }
                    word = (word & ~(0xFFu << (8 * j))) | (l << (8 * j));
                }
            }
            out[w] = word;
        }
        slab_store16(slab_all + (size_t)row * n * 16, n, i, pw, out[0], out[1], out[2], out[3]);
    }
}

// More than 256 clusters: the same two-level generator writing 16-bit labels, slab16[(batch*n + i)*16 + b] (32-byte rows).
// Plain arithmetic on the unpacked digits; blocks the two-field table form cannot describe are frequent here (many label
// starts per block), so the exact route ranks x against the boundary table by binary search.
template <bool HAS_LIBS>
__global__ __launch_bounds__(256) void k_shuffle16(int64_t n, const uint32_t* __restrict__ cum, int kpad, int blk_words, int K,
                                                   const uint32_t* __restrict__ keys, LibDom dom0, int n_libs,
                                                   const int32_t* __restrict__ lib_of, const int32_t* __restrict__ rank_of,
                                                   const LibDom* __restrict__ libdoms, uint16_t* __restrict__ slab_all, int tab_lds) {
    extern __shared__ uint32_t s_lds[];
    uint32_t* s_cum = s_lds + blk_words;
    if (tab_lds)  // (else: the boundaries stay in global memory — LabelShuffler::tab_lds)
        for (int t = threadIdx.x; t < n_libs * kpad; t += 256) s_cum[t] = cum[t];
    for (int t = threadIdx.x; t < blk_words; t += 256) s_lds[t] = cum[n_libs * kpad + t];
    __syncthreads();
    constexpr int B = 16;
    const int batch = blockIdx.y;
    const uint32_t* kg = keys + (size_t)batch * key_words_per_row(B, n_libs);
    const uint32_t* ks = kg + (size_t)n_libs * 8;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        LibDom ld = dom0;
        uint32_t x0 = (uint32_t)i, lib = 0;
        if (HAS_LIBS) {
            lib = (uint32_t)lib_of[i];
            ld = libdoms[lib];
            x0 = (uint32_t)rank_of[i];
        }
        const FeistelDomain dom = ld.dom;
        const uint32_t* tab = s_cum + lib * kpad + 1;  // tab[k] = cum[k + 1]
        const uint32_t* gtab = cum + lib * kpad + 1;   // the same table where it lies in global memory (tab_lds == 0)
        const uint32_t* blk = s_lds + ld.aoff;
        uint32_t ga = x0 / dom.B, gb = x0 - ga * dom.B;
        const uint32_t* gk = kg + (size_t)lib * 8;
        do {  // pi_g (low halves of the packed key words)
            for (int r = 0; r < FEISTEL_ROUNDS; r += 2) {
                ga = (ga + feistel_F1(gb, gk[r], dom.ash)) & (dom.A - 1u);
                uint32_t t = gb + feistel_F1(ga, gk[r + 1], dom.bsh);
                t = t >= dom.B ? t - dom.B : t;
                gb = t >= dom.B ? t - dom.B : t;
            }
        } while (ga * dom.B + gb >= dom.n);
        uint32_t out[B / 2];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const uint32_t* sk = ks + ((size_t)(j >> 1) * n_libs + lib) * 2;
            const int sh = (j & 1) * 16;
            const uint32_t k0 = (sk[0] >> sh) & 0xFFFFu, k1 = (sk[1] >> sh) & 0xFFFFu;
            uint32_t a = ga, b = gb, x;
            do {  // sigma_p, cycle-walked
                uint32_t t = b + feistel_F1(a, k0, dom.bsh);
                t = t >= dom.B ? t - dom.B : t;
                b = t >= dom.B ? t - dom.B : t;
                a = (a + feistel_F1(b, k1, dom.ash)) & (dom.A - 1u);
                x = a * dom.B + b;
            } while (x >= dom.n);
            const uint32_t e = blk[a];
            uint32_t l = (e & 0xFFFFu) + (b >= (e >> 16) ? 1u : 0u);
            if (l >= (uint32_t)K) {  // largest l with cum[l] <= x  <=>  first l with x < tab[l]
                uint32_t lo = 0, hi = (uint32_t)K - 1u;
                if (tab_lds) {
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (x < tab[mid]) hi = mid; else lo = mid + 1;
                    }
                } else {
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (x < gtab[mid]) hi = mid; else lo = mid + 1;
                    }
                }
                l = lo;
            }
            if (j & 1) out[j >> 1] |= l << 16; else out[j >> 1] = l;
        }
        uint4* dst = reinterpret_cast<uint4*>(slab_all + ((size_t)batch * n + i) * B);
        dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
    }
}

// numpy streams with 16-bit labels: Generator.shuffle(x) leaves x[perm] behind, perm = the same generator's permutation(n)
// (both run the same Fisher-Yates on the same draws): slab16[(batch*n + i)*16 + b] = base16[idx[p][i]], p = p0 + batch*16 + b
__global__ __launch_bounds__(256) void k_gather_labels16(int64_t n, const uint16_t* __restrict__ base16, const int32_t* __restrict__ idx,
                                                         int64_t p0, int64_t p_valid, uint16_t* __restrict__ slab_all) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int batch = blockIdx.y;
    uint32_t out[8];
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int64_t p = p0 + (int64_t)batch * 16 + b;
        const uint32_t l = p < p_valid ? base16[idx[(size_t)p * n + i]] : 0u;
        if (b & 1) out[b >> 1] |= l << 16; else out[b >> 1] = l;
    }
    uint4* dst = reinterpret_cast<uint4*>(slab_all + ((size_t)batch * n + i) * 16);
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
}

// ---------------------------------------------------------------------------------------------- tables
int check_labels(const int32_t* labels, int64_t n, int K, bool allow_negative) {
    for (int64_t i = 0; i < n; ++i) {
        if (labels[i] >= K || (labels[i] < 0 && !allow_negative)) {
            set_error("labels[%lld]=%d outside [0,%d)", (long long)i, labels[i], K);
            return SQGR_ERR_INVALID;
        }
    }
    return SQGR_OK;
}

int LabelShuffler::create(sqgr_ctx* ctx, int64_t n, const int32_t* labels, int K, const int32_t* lib_ids, int n_libs, LabelShuffler* p) {
    SQGR_REQUIRE(K >= 2, "Expected at least `2` clusters, found `%d`.", K);
    if (K > 65535) {
        set_error("K=%d > 65535 clusters: the label generators write 16-bit labels", K);
        return SQGR_ERR_UNSUPPORTED;
    }
    if (n > (int64_t)1 << 27) {
        set_error("graph too large for 32-bit slab offsets (n=%lld, nnz=%lld)", (long long)n, 0LL);
        return SQGR_ERR_UNSUPPORTED;
    }
    if (labels) SQGR_TRY(check_labels(labels, n, K, false));
    SQGR_HIP(hipSetDevice(ctx->device));
    p->ctx = ctx;
    p->n = n;
    p->K = K;
    const bool libs_on = lib_ids && n_libs >= 1;
    p->has_libs = libs_on;
    p->n_libs = libs_on ? n_libs : 1;
    p->kpad = K + 1;  // K boundaries + UINT_MAX sentinel
    // label histogram per library -> boundaries cum[l][k] = #{members of l with label < k}, padded with UINT_MAX
    std::vector<int64_t> cnt((size_t)p->n_libs, 0);
    std::vector<uint32_t> hist((size_t)p->n_libs * K, 0);
    std::vector<int32_t> rank;
    if (libs_on) rank.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        int l = 0;
        if (libs_on) {
            l = lib_ids[i];
            SQGR_REQUIRE(l >= 0 && l < n_libs, "lib_ids[%lld]=%d outside [0,%d)", (long long)i, l, n_libs);
            rank[i] = (int32_t)cnt[l];  // ranks in position order == np.where(libraries == c)[0]
        }
        cnt[l]++;
        if (labels) hist[(size_t)l * K + labels[i]]++;
    }
    if (labels) {
        for (int k = 0; k < K; ++k) {
            int64_t tot = 0;
            for (int l = 0; l < p->n_libs; ++l) tot += hist[(size_t)l * K + k];
            p->max_label_count = (int)std::max<int64_t>(p->max_label_count, tot);
        }
    }
    std::vector<uint32_t> cum((size_t)p->n_libs * p->kpad, 0xFFFFFFFFu);
    std::vector<LibDom> doms((size_t)p->n_libs);
    size_t blk_total = 0;
    for (int l = 0; l < p->n_libs; ++l) {
        uint32_t run = 0;
        for (int k = 0; k < K; ++k) {
            cum[(size_t)l * p->kpad + k] = run;
            run += hist[(size_t)l * K + k];
        }
        doms[l].dom = make_domain((uint32_t)(cnt[l] > 0 ? cnt[l] : 1));
        doms[l].aoff = (uint32_t)blk_total;
        blk_total += doms[l].dom.A;
    }
    p->blk_words = (int)blk_total;
    // the boundary table rides in LDS next to the block table when both fit; the 16-bit generator (more than 256 labels)
    // otherwise reads the boundaries of its exact route from global memory (thousands of clusters: ligrec's shuffler)
    p->tab_lds = (size_t)p->n_libs * p->kpad * 4 + blk_total * 4 <= 150 * 1024;
    if (!p->tab_lds && (K <= 256 || blk_total * 4 > 150 * 1024)) {
        set_error("library/label tables (%zu bytes) exceed the LDS budget of the shuffle kernel",
                  (size_t)p->n_libs * p->kpad * 4 + blk_total * 4);
        return SQGR_ERR_UNSUPPORTED;
    }
    // block table (appended to the boundary table): one word per high digit a describing the ranks [a*B, (a+1)*B) of
    // the label-sorted base — byte 0 the label of rank a*B, bits 16-31 the low digit at which the NEXT label starts
    // (0xFFFF: none).  "Events" inside a block are label starts and the library's end (ranks >= n_l read as label K,
    // the sentinel that sends the kernel to its exact route); a block with one event whose label is lab + 1 fits the
    // two-field form, a block with no event too, everything else is marked with lab0 = K.
    std::vector<uint32_t> blk(blk_total, 0);
    for (int l = 0; l < p->n_libs; ++l) {
        const uint32_t* c = &cum[(size_t)l * p->kpad];
        const uint64_t n_l = (uint64_t)cnt[l];
        const uint32_t SENT = (uint32_t)K | (0xFFFFu << 16);  // bits 0-15: label K (byte 0 = K for K <= 255; K = 256 reads 0 + bit 8)
        uint32_t lab = 0;
        for (uint32_t a = 0; a < doms[l].dom.A; ++a) {
            const uint64_t lo = (uint64_t)a * doms[l].dom.B, hi = lo + doms[l].dom.B;
            uint32_t word;
            if (lo >= n_l) {
                word = SENT;
            } else {
                while (lab + 1 < (uint32_t)K && c[lab + 1] <= lo) ++lab;  // label of rank lo: the largest k with c[k] <= lo
                const uint64_t end = hi < n_l ? hi : n_l;
                uint32_t events = 0, ev_label = 0;
                uint64_t ev_pos = 0;
                for (uint32_t k2 = lab + 1; k2 < (uint32_t)K && c[k2] < end; ++k2) {  // label changes inside (lo, end)
                    const uint64_t nxt = k2 + 1 < (uint32_t)K ? c[k2 + 1] : n_l;
                    if (c[k2] >= nxt) continue;  // empty category: no rank carries it
                    if (events == 0) { ev_label = k2; ev_pos = c[k2] - lo; }
                    ++events;
                }
                if (hi > n_l) {  // the library ends inside this block: ranks >= n_l read as the sentinel label K
                    if (events == 0) { ev_label = (uint32_t)K; ev_pos = n_l - lo; }
                    ++events;
                }
                if (events == 0)
                    word = lab | (0xFFFFu << 16);
                else if (events == 1 && ev_label == lab + 1 && ev_pos > 0)
                    word = lab | ((uint32_t)ev_pos << 16);
                else  // the exact route ranks x against the boundaries: from this block's first label on (byte 1: free in the
                    word = SENT | (K <= 255 ? lab << 8 : 0u);  // two-field form, which reads byte 0 and the upper half)
            }
            blk[doms[l].aoff + a] = word;
        }
    }
    // k_shuffle_tab's FIX pair drops the sentinel test: these tables qualify when the only sentinel labels left are the ranks >= n
    if (libs_on) {
        p->fix_why = "libraries (per-library domains and keys)";
    } else if (K > 126) {
        p->fix_why = "more than 126 clusters";
    } else {
        const FeistelDomain& d = doms[0].dom;
        const uint32_t past = (uint32_t)n / d.B;  // first block that holds a rank >= n
        for (uint32_t a = 0; a < past && a < d.A && !p->fix_why; ++a)
            if ((blk[a] & 0xFFu) == (uint32_t)K)  // byte 0 (byte 1 of such a word holds the block's first label)
                p->fix_why = "a block of the label-sorted base has several label starts or skips an empty category (lab0 = K)";
        const uint32_t tail = (uint32_t)n - past * d.B;  // ranks of the partial block inside [0, n)
        if (!p->fix_why && tail > 0 && blk[past] != ((uint32_t)(K - 1) | (tail << 16)))
            p->fix_why = "the block that reaches past the last rank does not end in label K - 1 in two-field form";
    }
    cum.insert(cum.end(), blk.begin(), blk.end());
    p->dom0.dom = make_domain((uint32_t)n);
    p->dom0.aoff = 0;
    if (!libs_on) p->dom0 = doms[0];
    {   // numpy-compatible mode: labels in library-grouped position order + library offsets
        std::vector<uint32_t> off((size_t)p->n_libs + 1, 0);
        for (int l = 0; l < p->n_libs; ++l) off[l + 1] = off[l] + (uint32_t)cnt[l];
        std::vector<uint8_t> base((size_t)n, 0);
        if (labels)
            for (int64_t i = 0; i < n; ++i) base[libs_on ? off[lib_ids[i]] + (uint32_t)rank[i] : (uint32_t)i] = (uint8_t)labels[i];
        p->has_labels = labels != nullptr;
        if (K > 256 && labels) {  // 16-bit copy of the same vector
            std::vector<uint16_t> b16((size_t)n, 0);
            for (int64_t i = 0; i < n; ++i) b16[libs_on ? off[lib_ids[i]] + (uint32_t)rank[i] : (uint32_t)i] = (uint16_t)labels[i];
            SQGR_TRY(p->base16.alloc((size_t)n));
            if (hipMemcpy(p->base16.p, b16.data(), (size_t)n * 2, hipMemcpyHostToDevice) != hipSuccess) return SQGR_ERR_HIP;
        }
        SQGR_TRY(p->base_pos.alloc((size_t)n));
        SQGR_TRY(p->lib_off.alloc(off.size()));
        hipError_t e2 = hipMemcpy(p->base_pos.p, base.data(), (size_t)n, hipMemcpyHostToDevice);
        if (e2 == hipSuccess) e2 = hipMemcpy(p->lib_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice);
        if (e2 != hipSuccess) {
            set_error("label upload failed: %s", hipGetErrorString(e2));
            return SQGR_ERR_HIP;
        }
    }
    SQGR_TRY(p->cum.alloc(cum.size()));
    hipError_t e = hipMemcpy(p->cum.p, cum.data(), cum.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && libs_on) {
        SQGR_TRY(p->lib_of.alloc((size_t)n));
        SQGR_TRY(p->rank_of.alloc((size_t)n));
        SQGR_TRY(p->libs.alloc((size_t)n_libs));
        e = hipMemcpy(p->lib_of.p, lib_ids, (size_t)n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->rank_of.p, rank.data(), (size_t)n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->libs.p, doms.data(), (size_t)n_libs * sizeof(LibDom), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error("label upload failed: %s", hipGetErrorString(e));
        return SQGR_ERR_HIP;
    }
    return SQGR_OK;
}

// ---------------------------------------------------------------------------------------------- launches
int LabelShuffler::independent_mode(int B, bool* independent) const {
    const char* e = getenv("SQGR_SHUFFLE_INDEPENDENT");
    *independent = e && atoi(e) == 1;
    SQGR_REQUIRE(!*independent || (B == 16 && !has_libs && !wide()), "SQGR_SHUFFLE_INDEPENDENT needs 16-wide rows, K <= 256 and no libraries");
    return SQGR_OK;
}

int LabelShuffler::keygen(const char* timer, uint64_t seed, int64_t perm0, int nrows, int B, bool independent, uint32_t* keys,
                          hipStream_t st) const {
    if (timer) {
        LaunchTimer t(ctx, timer, st);
        return keygen(nullptr, seed, perm0, nrows, B, independent, keys, st);
    }
    const int64_t nk = (int64_t)nrows * n_libs * (B / FEISTEL_GROUP + B / 2);
    if (independent) k_keygen_indep<<<(unsigned)ceil_div((int64_t)nrows * 8, 256), 256, 0, st>>>(seed, perm0, nrows, keys);
    else k_keygen<<<(unsigned)ceil_div(nk, 256), 256, 0, st>>>(seed, perm0, nrows, B, n_libs, keys);
    SQGR_HIP(hipGetLastError());
    return SQGR_OK;
}

int LabelShuffler::ensure_tab_workspace(int B, int nb_max) {
    if (B != 16 || has_libs || wide() || dom0.dom.A > SHUF_TAB_MAX_A) return SQGR_OK;  // launch_shuffle_raw never picks the table kernel
    return tab_ws.ensure(tab_workspace_words((std::max(nb_max, 1) + 1) / 2));
}

int LabelShuffler::launch_shuffle_raw(int B, int nb, const uint32_t* keys, uint8_t* slab, hipStream_t st, bool independent, int pw) const {
    unsigned gx = (unsigned)ceil_div(n, 256);
    // ~96 blocks per CU over all batches of the launch, each walking several spots (grid stride): amortises the LDS table
    // set-up and the key loads — measured 7 % faster on MI355X than one block per 256 spots (tools/shuf_sweep.sh)
    int per_cu = 96;
    const char* env_blocks = getenv("SQGR_SHUFFLE_BLOCKS_PER_CU");
    if (env_blocks && atoi(env_blocks) > 0) per_cu = atoi(env_blocks);
    gx = std::min<unsigned>(gx, (unsigned)(per_cu * std::max(ctx->cu_count, 1)) / (unsigned)std::max(nb, 1) + 1);
    const char* env_fix = getenv("SQGR_SHUFFLE_FIX");
    const int fix_mode = env_fix ? atoi(env_fix) : -1;
    if (fix_mode == 2 && (wide() || independent)) {
        set_error("SQGR_SHUFFLE_FIX=2: the launch is not eligible: %s", wide() ? "more than 126 clusters" : "SQGR_SHUFFLE_INDEPENDENT=1");
        return SQGR_ERR_UNSUPPORTED;
    }
    LaunchTimer t(ctx, wide() ? "nhood_shuffle16" : "nhood_shuffle", st);
    const size_t lds =(tab_lds ? (size_t)n_libs * kpad * 4 : 0) + (size_t)blk_words * 4;
    if (wide()) {
        if (B != 16) {
            set_error("more than 256 clusters: 16 permutations per pass only");
            return SQGR_ERR_UNSUPPORTED;
        }
        uint16_t* slab16 = reinterpret_cast<uint16_t*>(slab);
        if (has_libs) {
            SQGR_TRY(allow_lds(k_shuffle16<true>, lds));
            k_shuffle16<true><<<dim3(gx, nb), 256, lds, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, n_libs, lib_of.p,
                                                              rank_of.p, libs.p, slab16, tab_lds ? 1 : 0);
        } else {
            SQGR_TRY(allow_lds(k_shuffle16<false>, lds));
            k_shuffle16<false><<<dim3(gx, nb), 256, lds, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, n_libs, lib_of.p,
                                                               rank_of.p, libs.p, slab16, tab_lds ? 1 : 0);
        }
        SQGR_HIP(hipGetLastError());
        return SQGR_OK;
    }
    if (independent) {  // every permutation its own 8-round bijection (bench.py's `nhood_independent_bijections`; keys: k_keygen_indep)
        if (B != 16 || has_libs) {
            set_error("SQGR_SHUFFLE_INDEPENDENT: 16 permutations per row and no libraries only");
            return SQGR_ERR_UNSUPPORTED;
        }
        if (K <= 126) k_shuffle_indep<true><<<dim3(gx, nb), 256, lds, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, slab, pw);
        else k_shuffle_indep<false><<<dim3(gx, nb), 256, lds, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, slab, pw);
        SQGR_HIP(hipGetLastError());
        return SQGR_OK;
    }
    const unsigned gy = (unsigned)(B == 32 ? nb : (nb + 1) / 2);  // 16-permutation rows are shuffled in pairs
    {   // k_shuffle_tab: sigma's first round from an LDS table.  SQGR_SHUFFLE_TABLE (read at every call): 0 never, 1 whenever the
        // input is eligible, 2 required (an input that is not eligible is an error that names the reason), unset: automatic
        const char* env_tab = getenv("SQGR_SHUFFLE_TABLE");
        const int mode = env_tab ? atoi(env_tab) : -1;
        const uint32_t A = dom0.dom.A;
        const size_t tab_word0 = (lds / 4 + 7) & ~(size_t)7;  // 32-byte rows behind the block table and the boundaries
        const size_t lds_tab = tab_word0 * 4 + (size_t)2 * A * 32;
        const char* why = nullptr;
        if (B != 16) why = "32 permutations per row";
        else if (has_libs) why = "libraries (per-library domains and keys)";
        else if (A > SHUF_TAB_MAX_A) why = "more than 2^20 spots (high digit A > 1024: the two tables exceed 64 KB)";
        else if (lds_tab > LDS_BUDGET / 2) why = "tables do not fit two blocks per CU";
        if (mode == 2 && why) {
            set_error("SQGR_SHUFFLE_TABLE=2: the table kernel does not take this input: %s", why);
            return SQGR_ERR_UNSUPPORTED;
        }
        // automatic: launches of at least SHUF_TAB_MIN_TRIPS spots per thread of a resident block (two per CU) — smaller ones cannot
        // both fill the CUs and amortise the table build (16 packed evaluations per thread at A = 1024, about a third of a spot's
        // work) and keep k_shuffle.  Measured on MI355X, ms per launch, k_shuffle | k_shuffle_tab, 30 clusters — 1e6 spots: 16 rows
        // (7.6 trips) 0.137 | 0.158, 32 rows (15) 0.260 | 0.252, 64 rows 0.508 | 0.453, 160 rows 1.284 | 1.059; 105 600 spots
        // (A = 512): 64 rows (6.5 trips) 0.091 | 0.091, 160 rows (16) 0.202 | 0.193.
        // With the FIX pair and the tables built once per launch the table kernel won at every size of a later sweep (30 clusters,
        // eligible tables only) — 1e6 spots: 4 rows (3.8 trips) 0.047 | 0.045, 16 rows 0.139 | 0.108, 32 rows 0.259 | 0.184; 105 600
        // spots: 16 rows (1.6 trips) 0.031 | 0.030, 64 rows 0.090 | 0.064 (profiles/shuffle_pretab_before_after.md).  The threshold
        // stays until the instances that keep the sentinel test (K > 126, spot maps, skewed sizes) are swept too.
        const int cus = std::max(ctx->cu_count, 1);
        const int64_t block_trips = ceil_div(n, SHUF_TAB_THREADS) * (int64_t)gy;  // (block, trip) units of the launch
        const bool big = block_trips >= (int64_t)SHUF_TAB_MIN_TRIPS * 2 * cus;
        // the FIX pair (k_shuffle_tab without its sentinel test, k_shuffle_fix behind it).  SQGR_SHUFFLE_FIX (read at every call):
        // 0 never, 2 required — the table kernel then takes an eligible input whatever the launch size, and a launch that is not
        // eligible is an error that names the reason —, unset: whenever the table kernel runs on eligible tables
        const char* fix_no = why ? why : mode == 0 ? "SQGR_SHUFFLE_TABLE=0" : spot_of.p ? "a spot map (the rank is not the slab row)" : fix_why;
        if (fix_mode == 2 && fix_no) {
            set_error("SQGR_SHUFFLE_FIX=2: the launch is not eligible: %s", fix_no);
            return SQGR_ERR_UNSUPPORTED;
        }
        const bool fix = fix_mode != 0 && !fix_no;
        if (!why && mode != 0 && (mode == 1 || mode == 2 || big || fix_mode == 2)) {
            int tab_per_cu = SHUF_TAB_BLOCKS_PER_CU;
            if (env_blocks && atoi(env_blocks) > 0) tab_per_cu = atoi(env_blocks);
            // grid cap as for k_shuffle, then the same number of trips for every block (105 600 spots x 160 rows: 104 blocks' worth
            // of spots on 65 blocks — some walk two trips, some one — 0.214 ms; on 52 blocks of two trips each 0.193).  1e6 spots x
            // 160 rows by the cap: 6 blocks per CU 1.168 ms, 8: 1.134, 12: 1.076, 16: 1.063, 20: 1.062, 32: 1.060, 48: 1.078, 96: 1.179
            const unsigned nblk = (unsigned)ceil_div(n, SHUF_TAB_THREADS);
            const unsigned cap = (unsigned)(tab_per_cu * cus) / gy + 1;
            const unsigned trips = (nblk + cap - 1) / cap;
            const unsigned tx = (nblk + trips - 1) / trips;
            // the row pairs' tables built once per launch (k_shuffle_tab_build) instead of once per block.  SQGR_SHUFFLE_PRETAB (read
            // at every call): 0 the in-block build, unset | 1 the prebuilt tables — every instance of the table kernel.  Same stream,
            // inside this launch's timer bracket: the build's time is the shuffle's
            const char* env_pre = getenv("SQGR_SHUFFLE_PRETAB");
            const bool pretab = !(env_pre && atoi(env_pre) == 0);
            if (pretab) {
                const size_t need = tab_workspace_words((int)gy);
                if (!tab_ws.p || tab_ws.n < need) {
                    set_error("the table workspace holds %zu words, a launch of %u row pairs takes %zu (LabelShuffler::ensure_tab_workspace)",
                              tab_ws.p ? tab_ws.n : (size_t)0, gy, need);
                    return SQGR_ERR_INVALID;
                }
                k_shuffle_tab_build<<<dim3((unsigned)ceil_div((int64_t)A * 8, 256), gy), 256, 0, st>>>(keys, dom0.dom, nb, tab_ws.p);
                SQGR_HIP(hipGetLastError());
            }
#define SQGR_SHUFFLE_TAB_P(SK, NOMAP, FIX, PRE)                                                                                          \
    do {                                                                                                                                \
        SQGR_TRY(allow_lds(k_shuffle_tab<SK, NOMAP, FIX, PRE>, lds_tab));                                                               \
        k_shuffle_tab<SK, NOMAP, FIX, PRE><<<dim3(tx, gy), SHUF_TAB_THREADS, lds_tab, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, nb, \
                                                                                          slab, pw, spot_of.p, (int)tab_word0, tab_ws.p); \
    } while (0)
#define SQGR_SHUFFLE_TAB(SK, NOMAP, FIX) \
    do { if (pretab) SQGR_SHUFFLE_TAB_P(SK, NOMAP, FIX, true); else SQGR_SHUFFLE_TAB_P(SK, NOMAP, FIX, false); } while (0)
            if (fix) {
                SQGR_SHUFFLE_TAB(true, true, true);
            } else if (K <= 126) {
                if (spot_of.p) SQGR_SHUFFLE_TAB(true, false, false); else SQGR_SHUFFLE_TAB(true, true, false);
            } else {
                if (spot_of.p) SQGR_SHUFFLE_TAB(false, false, false); else SQGR_SHUFFLE_TAB(false, true, false);
            }
#undef SQGR_SHUFFLE_TAB
#undef SQGR_SHUFFLE_TAB_P
            SQGR_HIP(hipGetLastError());
            const uint32_t E = A * dom0.dom.B - (uint32_t)n;  // ranks of the domain outside [0, n)
            if (fix && E > 0) {  // same stream, inside this launch's timer bracket: its time is the shuffle's
                const int64_t threads = (int64_t)nb * FEISTEL_GROUP * E;
                k_shuffle_fix<<<(unsigned)ceil_div(threads, 256), 256, 0, st>>>(n, cum.p, K, keys, dom0.dom, nb, E, slab, pw);
                SQGR_HIP(hipGetLastError());
            }
            return SQGR_OK;
        }
    }
#define SQGR_SHUFFLE(BB, LIBS, SK)                                                                                             \
    k_shuffle<BB, LIBS, SK><<<dim3(gx, gy), 256, lds, st>>>(n, cum.p, kpad, blk_words, K, keys, dom0, n_libs, nb, \
                                                            lib_of.p, rank_of.p, libs.p, slab, pw, spot_of.p)
#define SQGR_SHUFFLE_K(BB, LIBS) \
    if (K <= 126) SQGR_SHUFFLE(BB, LIBS, true); else SQGR_SHUFFLE(BB, LIBS, false)
    if (B == 32) {
        if (has_libs) { SQGR_SHUFFLE_K(32, true); } else { SQGR_SHUFFLE_K(32, false); }
    } else {
        if (has_libs) { SQGR_SHUFFLE_K(16, true); } else { SQGR_SHUFFLE_K(16, false); }
    }
#undef SQGR_SHUFFLE_K
#undef SQGR_SHUFFLE
    SQGR_HIP(hipGetLastError());
    return SQGR_OK;
}

int LabelShuffler::gather_labels16(const char* timer, int nb, int64_t p0, int64_t p_valid, uint16_t* slab16, hipStream_t st) const {
    LaunchTimer t(ctx, timer, st);
    k_gather_labels16<<<dim3((unsigned)ceil_div(n, 256), nb), 256, 0, st>>>(n, base16.p, perm_idx.p, p0, p_valid, slab16);
    SQGR_HIP(hipGetLastError());
    return SQGR_OK;
}

// ---------------------------------------------------------------------------------------------- sqgr_shuffle.h's functions
int label_shuffler_create(sqgr_ctx* ctx, int64_t n, const int32_t* labels, int K, LabelShuffler** out) {
    SQGR_REQUIRE(ctx && labels && out && n > 0, "ctx/labels/out is NULL or n <= 0");
    *out = nullptr;
    LabelShuffler* s = new LabelShuffler();
    const int rc = LabelShuffler::create(ctx, n, labels, K, nullptr, 0, s);
    if (rc != SQGR_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return SQGR_OK;
}

void label_shuffler_destroy(LabelShuffler* s) { delete s; }

bool label_shuffler_wide(const LabelShuffler* s) { return s->wide(); }

size_t label_shuffler_key_words16() { return (size_t)key_words_per_row(16, 1); }

int label_shuffler_philox16(LabelShuffler* s, uint64_t seed, int64_t perm0, int nb, uint32_t* keys_ws, uint16_t* slab16, hipStream_t st) {
    if (!s->wide() || perm0 % FEISTEL_GROUP != 0) {
        set_error("label_shuffler_philox16: needs more than 256 labels and perm0 (%lld) a multiple of %d", (long long)perm0, FEISTEL_GROUP);
        return SQGR_ERR_INVALID;
    }
    SQGR_TRY(s->keygen("ligrec_keygen", seed, perm0, nb, 16, false, keys_ws, st));
    return s->launch_shuffle_raw(16, nb, keys_ws, reinterpret_cast<uint8_t*>(slab16), st, false);
}

int label_shuffler_pcg64_16(LabelShuffler* s, const uint64_t* states_dev, int64_t pc, uint16_t* slab16, hipStream_t st) {
    if (!s->wide() || !s->base16.p) {
        set_error("label_shuffler_pcg64_16: needs more than 256 labels");
        return SQGR_ERR_INVALID;
    }
    const int64_t n = s->n;
    SQGR_TRY(s->perm_idx.ensure((size_t)pc * n));
    SQGR_TRY(pcg_permutations_dev(s->ctx, s->pcg_ws, n, states_dev, pc, s->perm_idx.p, st));
    return s->gather_labels16("ligrec_gather_labels16", (int)ceil_div(pc, 16), 0, pc, slab16, st);
}

int label_shuffler_philox(LabelShuffler* s, uint64_t seed, int64_t perm0, int nb, uint32_t* keys_ws, uint8_t* slab,
                          hipStream_t st) {
    if (perm0 % FEISTEL_GROUP != 0) {
        set_error("label_shuffler_philox: perm0=%lld is not a multiple of %d", (long long)perm0, FEISTEL_GROUP);
        return SQGR_ERR_INVALID;
    }
    SQGR_TRY(s->keygen("ligrec_keygen", seed, perm0, nb, 32, false, keys_ws, st));
    return s->launch_shuffle_raw(32, nb, keys_ws, slab, st, false);
}

int label_shuffler_pcg64(LabelShuffler* s, const uint64_t* states_dev, int64_t pc, int64_t stride, uint8_t* W, hipStream_t st) {
    return pcg_shuffle_labels(s->ctx, s->pcg_ws, s->n, 1, s->lib_off.p, s->base_pos.p, states_dev, pc, stride, W, st, "ligrec_pcg64_shuffle");
}

}  // namespace sqgr
