"""The identities behind the leaner spot loop of the table label shuffle (sqgr_shuffle.hip: k_shuffle_tab), in numpy on the
arithmetic of oracle/devrng.py's restatement of the generator:

* the high digit of sigma's image may be carried scaled by 4 (the byte offset into the block table) through the second round;
* the digits (a, b) of the rank a thread handles may be advanced by the grid stride's digits instead of divided out per spot;
* one sentinel test on the OR of a group's four `word + (128 - K)` sums equals the four per-word tests (exact, but measured
  slower on the MI355X and not in the kernel: profiles/shuffle_valu_before_after.md)."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

from oracle import devrng

M16 = np.uint32(0xFFFF)


@pytest.mark.parametrize("A", [16, 32, 64, 128, 256, 512, 1024])
def test_high_digit_scaled_by_four_exhaustive(A):
    """((gsa + (x >> ash)) & am) << 2  ==  ((gsa << 2) + (x >> (ash - 2))) & (am << 2)  in 16-bit arithmetic, for EVERY 16-bit
    value x of the round function before its final shift and every group digit gsa < A; the result is a byte offset < 4 A."""
    abits = A.bit_length() - 1
    ash = 16 - abits                                   # sqgr_rng.h: make_domain
    assert ash >= 6, "the pre-scaled form needs two spare bits below the shift"
    am = np.uint32(A - 1)
    x = np.arange(1 << 16, dtype=np.uint32)[None, :]
    f = devrng._F(np.arange(8, dtype=np.uint64), np.uint64(0x1234), abits)
    assert int(f.max()) < A                            # the shift the identity models is the round function's own
    for g0 in range(0, A, 64):
        gsa = np.arange(g0, min(g0 + 64, A), dtype=np.uint32)[:, None]
        want = ((((gsa + (x >> np.uint32(ash))) & M16) & am) << np.uint32(2)) & M16
        got = (((gsa << np.uint32(2)) & M16) + (x >> np.uint32(ash - 2)) & M16) & (am << np.uint32(2))
        np.testing.assert_array_equal(got, want)
        assert int(got.max()) < 4 * A <= 1 << 12 and not (got & np.uint32(3)).any()


def _advance(start: np.ndarray, stride: int, B: int, trips: int):
    """The kernel's walk: ONE division per thread, then per trip the stride's digits and one conditional wrap."""
    sa, sb = divmod(stride, B)
    a, b = start // B, start % B
    for t in range(trips):
        yield t, a, b
        a = a + sa
        b = b + sb
        wrap = b >= B
        b = np.where(wrap, b - B, b)
        a = a + wrap


ADVANCE_CASES = [
    # (B, stride, trips): strides of the kernel are multiples of its 1024 threads; the other ones are there for the carry
    (16, 1024, 40),          # smallest low digit, stride % B == 0: b never moves
    (16, 1024 * 3, 9),
    (33, 1024 * 5, 30),      # 4 097 spots
    (207, 1024 * 52, 2),     # 105 600 spots x 160 rows: two trips per block
    (207, 1024, 104),
    (993, 1024 * 63, 17),    # 1 015 809 spots x 160 rows: sixteen trips, stride % B = 960 wraps nearly every trip
    (993, 1024, 993),        # stride % B = 31: a wrap every 32nd trip
    (993, 993 * 7, 50),      # stride % B == 0 with B odd
    (1024, 1024, 1024),      # 2**20 spots: stride = B
    (1024, 1024 * 64, 16),
    (977, 1023, 300),        # stride % B = 46, stride < 2 B
    (64, 63, 700),           # stride < B: the wrap carries alone
]


@pytest.mark.parametrize("B,stride,trips", ADVANCE_CASES)
def test_incremental_digits_equal_divmod(B, stride, trips):
    rng = np.random.default_rng(B + stride)
    start = np.unique(np.concatenate([np.arange(min(stride, 2048)), np.arange(max(stride - 2048, 0), stride),
                                      rng.integers(0, stride, 2048)])).astype(np.int64)
    wraps = 0
    for t, a, b in _advance(start, stride, B, trips):
        x = start + t * stride
        np.testing.assert_array_equal(a, x // B, err_msg=f"trip {t}")
        np.testing.assert_array_equal(b, x % B, err_msg=f"trip {t}")
        wraps += int(((x % B) + stride % B >= B).any())
    assert stride % B == 0 or wraps >= min(trips, 2), "the case must cross several wraps"


@pytest.mark.parametrize("K", [2, 30, 126])
def test_merged_sentinel_equals_per_word_tests(K):
    """K <= 126: label bytes are <= K < 128 and `word + (128 - K) * 0x01010101` sets bit 7 of exactly the bytes >= K without a
    carry between bytes.  One test of the OR of the four sums == the OR of the four tests, for every word of bytes around the
    sentinel and every way to place such words in a group."""
    vals = sorted({0, max(K - 2, 0), K - 1, K, K + 1})
    assert vals[-1] < 128
    words = np.array([b0 | b1 << 8 | b2 << 16 | b3 << 24 for b0, b1, b2, b3 in itertools.product(vals, repeat=4)], dtype=np.uint64)
    sent_add = np.uint64(((128 - K) * 0x01010101) & 0xFFFFFFFF)
    sums = (words + sent_add) & np.uint64(0xFFFFFFFF)
    hi = np.uint64(0x80808080)
    per_word = (sums & hi) != 0
    truth = np.array([any(((int(w) >> s) & 0xFF) >= K for s in (0, 8, 16, 24)) for w in words])
    np.testing.assert_array_equal(per_word, truth)                  # the per-word test is the byte comparison it stands for
    for s in (0, 8, 16, 24):                                        # ... byte by byte (what the exact route looks at)
        np.testing.assert_array_equal(((sums >> np.uint64(s + 7)) & np.uint64(1)) != 0, ((words >> np.uint64(s)) & np.uint64(0xFF)) >= K)
    # every ordered pair of words, the other two words clean and then flagged
    s0, s1 = sums[:, None], sums[None, :]
    for extra, extra_flag in ((np.uint64(0), False), (sums[truth.argmax()], True)):
        merged = ((s0 | s1 | extra | sums[0]) & hi) != 0
        np.testing.assert_array_equal(merged, per_word[:, None] | per_word[None, :] | extra_flag | per_word[0])
    # random groups of four
    idx = np.random.default_rng(K).integers(0, len(words), (200_000, 4))
    merged = (np.bitwise_or.reduce(sums[idx], axis=1) & hi) != 0
    np.testing.assert_array_equal(merged, per_word[idx].any(axis=1))
