"""The FIX pair of the table label shuffle without a GPU (tests/shuffle_fix_model.py on oracle/devrng.py): the labels whose first
sigma image leaves [0, n) are not searched for — both Feistel networks have closed-form inverses, so one thread per out-of-range
rank y in [n, A*B) and permutation finds the spot whose first image is y and stores its label; the table kernel then needs no
sentinel test.

Sizes (A x B, E = A B - n): 257 (32 x 16, 255), 300 (32 x 16, 212: chains of out-of-range ranks, E > A), 993 (32 x 32, 31 = A - 1),
1000 (32 x 32, 24), 1024 (32 x 32, 0), 4097 (128 x 33, 127)."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import devrng
from tests import shuffle_fix_model as M

SIZES = (257, 300, 993, 1000, 1024, 4097)
SEEDS = (0, 77, 2**40 + 3)
PERMS = np.arange(2**33 + 8, 2**33 + 24)  # 16 permutations of two groups, both packed halves of all eight pairs
K = 5


def test_domains_are_the_ones_the_cases_are_named_for():
    dims = {n: devrng.domain_dims(n)[:2] for n in SIZES}
    assert dims == {257: (32, 16), 300: (32, 16), 993: (32, 32), 1000: (32, 32), 1024: (32, 32), 4097: (128, 33)}
    assert [a * b - n for n, (a, b) in dims.items()] == [255, 212, 31, 24, 0, 127]
    assert len(set(PERMS // 16)) == 2


@pytest.mark.parametrize("n", SIZES)
def test_inverse_rounds_undo_the_forward_ones_on_the_whole_domain(n):
    A, B, Bmask = devrng.domain_dims(n)
    a0, b0 = np.meshgrid(np.arange(A, dtype=np.uint64), np.arange(B, dtype=np.uint64), indexing="ij")
    a0, b0 = np.tile(a0.ravel(), (len(PERMS), 1)), np.tile(b0.ravel(), (len(PERMS), 1))
    for seed in SEEDS:
        gk = devrng.group_keys(seed, PERMS // 16)
        sk = devrng.sigma_keys(seed, PERMS)
        g64 = gk.astype(np.uint64) & devrng.MASK16
        a, b = devrng._rounds(a0, b0, A, B, Bmask, lambda r: g64[:, r : r + 1])
        assert (a < A).all() and (b < B).all()
        a, b = M.rounds_inverse(a, b, gk, n)
        np.testing.assert_array_equal(a, a0)
        np.testing.assert_array_equal(b, b0)
        a, b = devrng._sigma(a0, b0, A, B, Bmask, sk.astype(np.uint64) & devrng.MASK16)
        a, b = M.sigma_inverse(a, b, sk, n)
        np.testing.assert_array_equal(a, a0)
        np.testing.assert_array_equal(b, b0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
def test_fix_threads_reach_exactly_the_spots_whose_first_image_leaves_the_range_with_the_oracles_label(n, seed):
    labels = np.random.default_rng(n).integers(0, K, n).astype(np.int32)
    cum = M.boundaries(labels, K)
    first = M.first_sigma_images(n, seed, PERMS)
    want_set = {(int(p), int(i)) for p, i in zip(*np.nonzero(first >= n))}
    expected = np.sort(labels)[devrng.label_permutations(n, seed, PERMS)]  # (P, n): the oracle's labels
    got = M.fix_threads(n, seed, PERMS, cum, K)
    assert len(got) == len({(p, s) for p, s, _ in got}), "a (spot, permutation) reached twice"
    assert {(p, s) for p, s, _ in got} == want_set, "missed or superfluous (spot, permutation)"
    for p, s, lab in got:
        assert lab == expected[p, s], (p, s)
    if n == 1024:
        assert not got and not want_set
    else:
        assert want_set
    if n == 300:  # chains: some out-of-range ranks are reached only through another one and store nothing
        A, B, _ = devrng.domain_dims(n)
        assert len(got) < (A * B - n) * len(PERMS)


def _assemble(n, seed, labels, k, blk):
    """The pair's output: table labels of the first images through the patched table, then the fix threads' stores."""
    first = M.first_sigma_images(n, seed, PERMS)
    out = M.table_label(M.patched(blk, n, k), first, n)
    assert (out < k).all(), "the table kernel stored a byte >= K"
    for p, s, lab in M.fix_threads(n, seed, PERMS, M.boundaries(labels, k), k):
        out[p, s] = lab
    return out


@pytest.mark.parametrize("n", SIZES)
def test_patched_table_plus_fix_threads_equal_the_oracle_on_eligible_tables(n):
    rng = np.random.default_rng(n + 1)
    done = 0
    for k, labels in ((2, rng.integers(0, 2, n)), (2, (np.arange(n) >= n // 3).astype(np.int64)), (3, np.minimum(np.arange(n) * 3 // n, 2))):
        labels = labels.astype(np.int32)
        blk = M.block_table(M.boundaries(labels, k), n, k)
        if M.refusal(blk, n, k) is not None:
            continue
        done += 1
        for seed in SEEDS:
            np.testing.assert_array_equal(_assemble(n, seed, labels, k, blk), np.sort(labels)[devrng.label_permutations(n, seed, PERMS)])
    assert done >= 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", (2, 30, 126))
def test_patched_table_maps_every_rank_of_the_domain_to_a_label_below_k(n, k):
    labels = np.random.default_rng(k).integers(0, k, n).astype(np.int32)
    blk = M.block_table(M.boundaries(labels, k), n, k)
    A, B, _ = devrng.domain_dims(n)
    x = np.arange(A * B)
    if M.refusal(blk, n, k) is None:
        lab = M.table_label(M.patched(blk, n, k), x, n)
        assert (lab < k).all()
        np.testing.assert_array_equal(lab[:n], np.sort(labels))
        assert (lab[n:] == k - 1).all()
    else:  # small clusters: blocks with several label starts — the unpatched sentinel is what refuses them
        assert (M.table_label(blk, x, n)[:n] >= k).any()


def _tables(sizes, n):
    k = len(sizes)
    labels = np.repeat(np.arange(k), sizes).astype(np.int32)
    assert len(labels) == n
    return M.block_table(M.boundaries(labels, k), n, k), k


def test_eligibility_on_hand_made_boundary_tables():
    n = 1000  # 32 x 32, the last block holds ranks 992 .. 999 and 24 ranks outside
    blk, k = _tables([500, 500], n)                    # one label start, inside block 15; the last block is all label 1
    assert M.refusal(blk, n, k) is None
    assert int(blk[31]) == 1 | (8 << 16) and int(blk[15]) == 0 | (20 << 16)
    blk, k = _tables([500, 10, 490], n)                # a cluster smaller than one block: two label starts in block 15
    assert M.refusal(blk, n, k) == "lab0 = K" and int(blk[15]) & 0xFF == k
    blk, k = _tables([500, 0, 500], n)                 # an empty category: the start in block 15 skips a label
    assert M.refusal(blk, n, k) == "lab0 = K" and int(blk[15]) & 0xFF == k
    blk, k = _tables([996, 4], n)                      # the last block ends K - 2 | K - 1 | out of range
    assert M.refusal(blk, n, k) == "does not end in label K - 1" and int(blk[31]) & 0xFF == k
    blk, k = _tables([1000, 0], n)                     # ... or in K - 2 with the last category empty
    assert M.refusal(blk, n, k) == "does not end in label K - 1"
    blk, k = _tables([512, 512], 1024)                 # E = 0: no block reaches past the last rank, the start sits on a block boundary
    assert M.refusal(blk, 1024, k) is None
    blk, k = _tables([7] * 125 + [125], n)             # 126 clusters, most of them smaller than a block
    assert k == 126 and M.refusal(blk, n, k) == "lab0 = K"
    assert M.refusal(np.zeros(32, dtype=np.int64), n, 127) == "more than 126 clusters"


def test_slab_offset_is_where_the_planes_put_the_label():
    """slab_store16's layouts written out: 16 / pw planes [n][pw], plane q = permutations [q * pw, (q + 1) * pw)."""
    n = 7
    for pw in (16, 8, 4, 2, 1):
        slab = np.full(16 * n, -1, dtype=np.int64)
        planes = slab.reshape(16 // pw, n, pw)
        for i in range(n):
            for j in range(16):
                planes[j // pw, i, j % pw] = i * 16 + j
        for i in range(n):
            for j in range(16):
                assert slab[M.slab_offset(n, i, pw, j)] == i * 16 + j
