#pragma once
// The bucket lists of spatial_autocorr's LDS permutation dot: the layout that the builder (sqgr_autocorr_lists.hip) writes and the
// dot kernel (k_perm_dot_lds, sqgr_autocorr.hip) walks, and the context's cache of the last set of lists.
//
// The LDS-bucketed permutation dot (the hot kernel for n_perms >= 512): BOTH operands of z_i * y[idx_p(i)] on chip.
//
// The spots are cut into `nch` chunks of `m` consecutive spots; a pair (i, j = idx_p(i)) of permutation p belongs to
// bucket (a, b) = (i / m, j / m).  A workgroup owns (gene pair, chunk a): Z[chunk a] of its two genes stays in LDS, the
// Y chunks b = 0 .. nch-1 pass through LDS one after the other, and lane = permutation: every lane walks the list of ITS
// permutation's pairs of bucket (a, b) and accumulates z*y in registers — two random 16-byte LDS reads per pair and two
// genes, no global gather at all.  The lists are shared by all genes (the permutations are), so their construction
// (k_bucket_*, ~1e8 pairs at config 3) is amortised over the gene block; they are stored [group of 64 permutations]
// [a][b][k][lane], padded with a pair that points at a zero row of Z to the longest list of the group (a multiple of
// LIST_UNROLL), so a wave reads 256 contiguous bytes per step and needs no tail.  Sum order: list order (ascending i)
// inside (a, b), b ascending, then a ascending in k_perm_final_lds: fixed => bit-reproducible.
//
// An entry is (i - a*m) | (j - b*m) << 16; the padding pair is (m .. m + ZERO_ROWS - 1, any Y row).  Lists that serve Geary's C
// through the class table carry the class of r[j] in bits 29..31 (m < 8192); exception lists (one per group and chunk a) hold
// (i - a*m) | class of r[j] << 29.  len[pg][a][b] / off[pg][a][b] count rows of 64 entries, base[pg] the rows in front of group pg.
#include "sqgr_common.h"

#include <cstdlib>
#include <functional>

namespace sqgr {

constexpr int GP = 2;             // genes per LDS tile (one ds_read_b128 per operand)
constexpr int LIST_UNROLL = 8;    // pairs per lane between two waits
constexpr int LIST_ROUND = 16;    // list lengths are multiples of it (k_bucket_order schedules whole rounds of 16 classes)
constexpr int LDS_MAX_CHUNKS = 240;  // bucket kernels: (64 + 1) * nch counters in <= 64 KiB of LDS
constexpr int LDS_BYTES = 160 * 1024;
constexpr int LDS_PERM_BLOCK = 1024;  // lanes (= permutations) per workgroup
// Few permutations (the reference's everyday calls run 50-100, tests/graph/test_ppatterns.py): a workgroup of lane = permutation
// would be mostly empty.  The LDS kernel then runs on VIRTUAL permutations: permutation p is cut into LDS_SPLIT sub-lists (the
// spots i = s mod LDS_SPLIT), lane = (p, s); the kernel, the bucket lists and their layout do not change, only the list builder
// strides over the spots and k_perm_final_lds adds the LDS_SPLIT partial sums of a permutation (s ascending, then the chunks) —
// a fixed order, so a split permutation range stays bit-identical.  100 permutations fill 13 of a workgroup's 16 waves.
constexpr int LDS_SPLIT = 8;
constexpr int EXC_UNROLL = 4;         // rows of an exception list (k_perm_dot_lds RMODE 3) are multiples of it
constexpr int LIST_ROUND_SPLIT = 8;   // list lengths of the split variant (its lists are ~1/8 as long; no bank-aware order)

// The Z chunk ends in ZERO_ROWS rows of zeros, one of every bank class (row index mod 16): the padding pair of a lane that has
// no pair left points at one of them — and at any Y row — so the schedule can give it LDS banks nobody else reads at that step.
constexpr int ZERO_ROWS = 16;
// chunk length for n spots: (m + ZERO_ROWS) Z rows + m Y rows (+ m row sums for Geary) in 160 KiB
static inline int lds_chunk(int64_t n, bool geary, int* nch_out) {
    const int per_spot = 2 * GP * 8 + (geary ? 8 : 0);
    int m_max = ((LDS_BYTES - ZERO_ROWS * GP * 8 - 64) / per_spot) & ~3;  // (64 B: the row-sum class table of RMODE 2 / 3)
    if (const char* env = getenv("SQGR_AUTOCORR_LDS_CHUNK"))  // tests: several chunks on small inputs
        m_max = std::max(16, std::min(m_max, atoi(env) & ~3));
    const int64_t nch = ceil_div(n, m_max);
    *nch_out = (int)nch;
    return (int)((ceil_div(n, nch) + 3) & ~(int64_t)3);
}

// Lane -> slot of its (virtual) permutation inside a group of 64.  A `ds_read_b128` serves a wave in four fixed sets of 16 lanes
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32; MI355X_MICROARCH.md §LDS); the slots are numbered so that set q holds the slots
// 16 q .. 16 q + 15, slot mod 16 = lane mod 16: the 16 permutations that meet in a service group — the ones whose lists are scheduled
// against each other, k_bucket_order_* — are 16 CONSECUTIVE permutations, whatever 16-aligned index a pass starts at.
__device__ __forceinline__ int perm_slot(int lane) {
    const int x = lane & 31;
    const int odd = ((x >= 4 && x < 12) || (x >= 16 && x < 20) || x >= 28) ? 1 : 0;
    return ((lane >> 5) * 2 + odd) * 16 + (lane & 15);
}

// chunk of spot j (j < 2^24: exact in float; the estimate is off by at most one)
__device__ __forceinline__ uint32_t chunk_of(uint32_t j, uint32_t m, float inv_m) {
    uint32_t b = (uint32_t)((float)j * inv_m);
    if (b * m > j) --b;
    else if ((b + 1) * m <= j) ++b;
    return b;
}

// How the bucket lists are ordered.  0: as built (ascending i; SQGR_AUTOCORR_ORDER_LISTS=0, and the split variant: a sub-list holds
// two pairs per class), 1: SQGR_AUTOCORR_ORDER=single, the round-3 schedule (every list on its own: one side of a pair conflict-free),
// 2: SQGR_AUTOCORR_ORDER=rotation, the joint schedule of the 16 permutations of a `ds_read_b128` lane group on the fixed rotation of
// Z classes (k_bucket_order_joint), 3: the step schedule (k_bucket_order_steps; the default)
int list_order_mode(int split);

// The bucket lists depend on the permutations alone: every feature block of a call (and the next call with the same seed)
// walks the same ones, so they live in the context, keyed by what determines them — one field per fact.
enum class PermSource { device = 0, numpy = 1, injected = 2 };  // the device generator (seed), numpy's streams (states), host indices
struct PermListKey {
    int64_t n = 0, pc = 0, perm0 = 0;  // spots; permutations of the pass, the first of them in its stream
    int m = 0, nch = 0;                // chunk length and chunks (lds_chunk)
    PermSource source = PermSource::device;
    uint64_t seed = 0;                 // source device
    const uint64_t* states = nullptr;  // source numpy: the pc generator states, four words each (the caller's; the cache keeps a copy)
    int split = 1;                     // virtual permutations per permutation (LDS_SPLIT variant)
    int order = 0;                     // list_order_mode(split)
    bool row_classes = false;          // entries carry the class of r[j] (k_perm_dot_lds RMODE 2)
    bool exceptions = false;           // with exception lists (RMODE 3)
    uint64_t cls_serial = 0;           // either of the two: whose classes (sqgr_autocorr::cls_serial), else 0
    // Injected indices are not part of the key, so such lists never equal any — not even themselves.
    bool operator==(const PermListKey& o) const {
        if (n != o.n || pc != o.pc || perm0 != o.perm0 || m != o.m || nch != o.nch || source != o.source || split != o.split || order != o.order ||
            row_classes != o.row_classes || exceptions != o.exceptions || cls_serial != o.cls_serial)
            return false;
        if (source == PermSource::device) return seed == o.seed;
        return source == PermSource::numpy && states && o.states && !memcmp(states, o.states, (size_t)pc * 32);
    }
};

// what the dot kernel reads of a set of lists: device arrays owned by the context's cache, valid until the next lists_for
struct PermListsView {
    const uint32_t *len, *off;  // [group][a][b]
    const uint64_t* base;       // [group]
    const uint32_t* lists;
    const uint32_t *xlen, *xoff, *xlists;  // exception lists [group][a], when the key asks for them
};

// The lists of `key`: the context's when they are these; else — and only then — `fill_idx` is called to put the permutations'
// indices into idx[pc][n] (device), the cache is invalidated, the lists are built from idx and the key is stored once they are
// complete.  rcls: the row-sum class of every spot (keys with row_classes or exceptions), exc_main: the class that needs no
// exception; by_y: the per-list schedule (order 1) goes by the classes of the Y row, not the Z row (not part of the key).
int lists_for(sqgr_ctx* ctx, const PermListKey& key, const std::function<int()>& fill_idx, const int32_t* idx, const uint8_t* rcls, int exc_main,
              bool by_y, PermListsView* out);

}  // namespace sqgr
