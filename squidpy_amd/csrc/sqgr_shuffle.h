// libsqgr internal: shuffled cluster-label vectors for permutation tests — the Philox-keyed Feistel generator and numpy's
// streams.  Implemented in sqgr_shuffle.hip; a neighbourhood-enrichment plan (sqgr_nhood.hip) holds one next to its graph,
// ligrec (sqgr_ligrec.hip) one on its own.
#pragma once
#include "sqgr_common.h"
#include "sqgr_pcg.h"
#include "sqgr_rng.h"

namespace sqgr {

// Keys of one slab row (B permutations perm_row .. perm_row + B - 1, perm_row a multiple of 16) — see sqgr_rng.h for the
// two-level construction.  Layout in 32-bit words, every word two packed 16-bit lanes (two permutations per packed-16
// instruction of the label shuffle):
//   group keys : [g][lib][8]   g < B/16: the 8 round keys of group perm_row/16 + g in both halves
//   sigma keys : [t][lib][2]   t < B/2 : the 2 round keys of permutations perm_row + 2t (low half) and + 2t + 1 (high half)
// (a row of 16 never takes fewer than 64 words: the independent-bijection variant of the generator, k_shuffle_indep, keeps the 8
// round keys of each of its 8 permutation pairs there)
__host__ __device__ constexpr int key_words_per_row(int B, int n_libs) {
    return n_libs * ((B / FEISTEL_GROUP) * 8 + (B / 2) * 2) < (B / 2) * 8 ? (B / 2) * 8 : n_libs * ((B / FEISTEL_GROUP) * 8 + (B / 2) * 2);
}

struct LibDom {
    FeistelDomain dom;
    uint32_t aoff;  // offset of this library's block table
};

// The 16 shuffled labels of spot i (4 words, label b in byte b & 3 of word b >> 2) into a batch's 16 * n bytes of the slab.
// pw = 16: row i of [n][16] — what k_count gathers.  pw = 8 | 4 | 2 | 1 (51 <= K <= 202 clusters, k_count_pass): 16 / pw PLANES
// [n][pw], plane q = permutations [q * pw, (q + 1) * pw) — a pass of pw permutations then gathers from dense rows of exactly
// the bytes it uses (round 5: out of 16-byte rows a pass of 4 pulled four times the cache lines through L1 and L2).
__device__ __forceinline__ void slab_store16(uint8_t* __restrict__ batch_base, int64_t n, int64_t i, int pw, uint32_t w0, uint32_t w1,
                                             uint32_t w2, uint32_t w3) {
    if (pw == 16) {
        *reinterpret_cast<uint4*>(batch_base + (size_t)i * 16) = make_uint4(w0, w1, w2, w3);
    } else if (pw == 8) {
        *reinterpret_cast<uint2*>(batch_base + (size_t)i * 8) = make_uint2(w0, w1);
        *reinterpret_cast<uint2*>(batch_base + (size_t)n * 8 + (size_t)i * 8) = make_uint2(w2, w3);
    } else if (pw == 4) {
        uint32_t* d = reinterpret_cast<uint32_t*>(batch_base) + i;
        d[0] = w0; d[(size_t)n] = w1; d[(size_t)2 * n] = w2; d[(size_t)3 * n] = w3;
    } else if (pw == 2) {
        uint16_t* d = reinterpret_cast<uint16_t*>(batch_base) + i;
        const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
        for (int q = 0; q < 8; ++q) d[(size_t)q * n] = (uint16_t)(w[q >> 1] >> (16 * (q & 1)));
    } else {
        uint8_t* d = batch_base + i;
        const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
        for (int q = 0; q < 16; ++q) d[(size_t)q * n] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
    }
}

// where slab_store16 puts label j < 16 of spot i, as a byte offset from batch_base: plane j / pw, row i, byte j % pw
__host__ __device__ inline size_t slab_label_offset(int64_t n, int64_t i, int pw, int j) {
    return (size_t)(j / pw) * (size_t)n * pw + (size_t)i * pw + (size_t)(j % pw);
}

// k_shuffle_fix's work for ONE out-of-range rank y in [n, A*B) and one permutation (gk: the 8 keys of its group, k0 | k1: its
// sigma keys; 16 bits each): the spot whose FIRST sigma image is y and the rank sigma's cycle walk ends on — or false when no
// spot's first image is y (sigma^-1(y) lies outside [0, n) itself; y is then reached only from another out-of-range rank, and
// that rank's call owns the spot).  sigma and pi_g are bijections of A x B, so over all y the spots returned are exactly those
// whose first image leaves [0, n), each once; the inverse of a cycle-walked permutation is the cycle-walked inverse.
__host__ __device__ inline bool shuffle_fix_target(uint32_t y, const FeistelDomain& d, const uint32_t* gk, uint32_t k0, uint32_t k1,
                                                   uint32_t* spot, uint32_t* rank_out) {
    const uint32_t ya = y / d.B, yb = y - ya * d.B;
    uint32_t a = ya, b = yb;
    sigma_inverse(a, b, d, k0, k1);
    if (a * d.B + b >= d.n) return false;
    do feistel_rounds_inverse(a, b, d, gk); while (a * d.B + b >= d.n);  // pi_g^-1, cycle-walked: the walk started inside [0, n)
    *spot = a * d.B + b;
    a = ya;
    b = yb;
    do {  // forward as the exact route of k_shuffle: sigma until the image is back inside (its cycle holds sigma^-1(y) < n)
        uint32_t t = b + feistel_F1(a, k0, d.bsh);
        t = t >= d.B ? t - d.B : t;
        b = t >= d.B ? t - d.B : t;
        a = (a + feistel_F1(b, k1, d.ash)) & (d.A - 1u);
    } while (a * d.B + b >= d.n);
    *rank_out = a * d.B + b;
    return true;
}

// every label in [0, K) (allow_negative: or below 0 — unlabelled), else an error that names the first offender
int check_labels(const int32_t* labels, int64_t n, int K, bool allow_negative);

// The label tables of one labelled set of n items (optionally grouped into libraries) and the two generators that read them.
struct LabelShuffler {
    sqgr_ctx* ctx = nullptr;
    int64_t n = 0;
    int K = 0;
    int n_libs = 1;
    bool has_libs = false;
    LibDom dom0{};
    int blk_words = 0;     // words of the block table (one per high digit and library)
    DevBuf<uint32_t> cum;  // [n_libs][kpad] label boundaries of the label-sorted base, then the block table
    int kpad = 0;
    bool tab_lds = true;   // the label-boundary table fits LDS next to the block table (create)
    DevBuf<int32_t> lib_of, rank_of;
    DevBuf<LibDom> libs;
    DevBuf<uint8_t> base_pos;   // base labels in library-grouped position order (numpy-compatible mode)
    DevBuf<uint16_t> base16;    // the same as 16-bit labels (more than 256 clusters)
    DevBuf<int32_t> perm_idx;   // numpy permutations of a chunk (more than 256 clusters: labels are gathered through them)
    DevBuf<uint32_t> lib_off;   // [n_libs + 1] first position of every library
    DevBuf<int32_t> spot_of;    // sqgr_nhood_set_spot_map: slab row i holds the labels of the caller's observation spot_of[i]
    PcgWorkspace pcg_ws;        // jump-ahead table and row workspace of the numpy-compatible shuffle (sqgr_pcg.hip)
    bool has_labels = false;
    int max_label_count = 0;    // largest cluster of the base labels (0: unknown — injected label vectors)
    const char* fix_why = nullptr;  // why these tables keep k_shuffle_tab's sentinel test (NULL: the FIX pair may run — create)
    DevBuf<uint32_t> tab_ws;    // k_shuffle_tab's round-1 tables of a launch, [row pair][2][A][8] words (k_shuffle_tab_build)
    size_t tab_workspace_words(int row_pairs) const { return (size_t)row_pairs * 2 * dom0.dom.A * 8; }
    bool wide() const { return K > 256; }  // 16-bit labels
    bool mapped() const { return spot_of.p != nullptr; }

    // Validates K in [2, 65535], n <= 2^27, the labels (NULL: none, for callers that inject label vectors) and the libraries
    // (lib_ids NULL: none), then builds and uploads the tables into *out.  On an error *out is left for its owner to destroy.
    static int create(sqgr_ctx* ctx, int64_t n, const int32_t* labels, int K, const int32_t* lib_ids, int n_libs, LabelShuffler* out);
    // *independent <- SQGR_SHUFFLE_INDEPENDENT=1 (read at every call): the generator without its shared group bijection, one
    // 8-round bijection per permutation (k_shuffle_indep) — for rows of B = 16 labels up to 256 without libraries only
    int independent_mode(int B, bool* independent) const;
    // keys of nrows slab rows of B permutations from permutation perm0 (a multiple of 16) on; timer: LaunchTimer name or NULL
    int keygen(const char* timer, uint64_t seed, int64_t perm0, int nrows, int B, bool independent, uint32_t* keys, hipStream_t st) const;
    // tab_ws for launches of up to nb_max batches of B permutations, where the table kernel can take them at all (16-wide rows, no
    // libraries, at most 2^20 spots and 256 clusters; 5 MB at 1e6 spots x 160 rows).  The owner of the key and slab buffers calls
    // it where it sizes those: launch_shuffle_raw allocates nothing
    int ensure_tab_workspace(int B, int nb_max);
    // slab rows of nb batches of B permutations from their keys; pw: plane width of a 16-wide batch (slab_store16)
    int launch_shuffle_raw(int B, int nb, const uint32_t* keys, uint8_t* slab, hipStream_t st, bool independent, int pw = 16) const;
    // numpy streams, 16-bit labels: nb batches of base16 gathered through the permutations p0 .. of perm_idx (zeros from p_valid on)
    int gather_labels16(const char* timer, int nb, int64_t p0, int64_t p_valid, uint16_t* slab16, hipStream_t st) const;
};

int label_shuffler_create(sqgr_ctx* ctx, int64_t n, const int32_t* labels, int K, LabelShuffler** out);
void label_shuffler_destroy(LabelShuffler* s);

// device generator (Philox-keyed Feistel bijections): slab[(q*n + i)*32 + b] = label of item i in permutation
// perm0 + q*32 + b, for q < nb.  keys_ws: nb*32*8 words of scratch.
int label_shuffler_philox(LabelShuffler* s, uint64_t seed, int64_t perm0, int nb, uint32_t* keys_ws, uint8_t* slab, hipStream_t st);

// numpy streams (PCG64 + Generator.shuffle): W[i*stride + q] = label of item i in the permutation generator q yields,
// q < pc.  states_dev: pc rows [state_hi, state_lo, inc_hi, inc_lo] on the device.
int label_shuffler_pcg64(LabelShuffler* s, const uint64_t* states_dev, int64_t pc, int64_t stride, uint8_t* W, hipStream_t st);

// More than 256 labels (K <= 65535): 16-bit label rows of 16 permutations, slab16[(q*n + i)*16 + b] = label of item i in
// permutation perm0 + q*16 + b (device generator; keys_ws: nb * label_shuffler_key_words16() words) or in the permutation
// generator q*16 + b yields (numpy streams; labels of generators >= pc are 0).
bool label_shuffler_wide(const LabelShuffler* s);
size_t label_shuffler_key_words16();
int label_shuffler_philox16(LabelShuffler* s, uint64_t seed, int64_t perm0, int nb, uint32_t* keys_ws, uint16_t* slab16, hipStream_t st);
int label_shuffler_pcg64_16(LabelShuffler* s, const uint64_t* states_dev, int64_t pc, uint16_t* slab16, hipStream_t st);

}  // namespace sqgr
