"""The two identities the label shuffle's cheaper instructions rest on (sqgr_rng.h: xorshift7_2; sqgr_shuffle.hip: carry_entry and
the FIX instance's look-up), in numpy against oracle/devrng.py — its round function `_F` and its label rule (the label of rank x is
`np.sort(labels)[x]`; inside a block of the label-sorted base that is `first + (b >= boundary)`):

* `x ^= x >> 7` in both 16-bit halves of a packed word is `w ^= (w >> 7) & 0x01FF01FF` on the 32-bit word: the mask removes exactly
  the seven bits a 32-bit shift moves from the high half into the low half.  Checked through the whole round function with no final
  shift (the multiplies by odd constants are bijections of 16 bits, so every input of the xorshift is reached and every output bit
  is compared): every 16-bit value in one half against 0, 0xFFFF, 0x007F and 0xFF80 in the other, and four million random words.
* a block-table entry `first | boundary << 16` rewritten as `first << 16 | (2**16 - boundary) mod 2**16` — `(first + 1) << 16` for a
  boundary of 0 — gives the block's label of low digit b < B <= 2**14 as byte 2 of `entry + b`: the add carries out of the low half
  exactly when b >= boundary.  Every b at B = 16, 977 and 16 384, boundaries 0, 1, B - 1, B, 0xFFFF and a stride in between, first
  labels 0, K - 2 and 125; then whole tables of real label vectors, every rank of the domain, against the sorted base."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import devrng
from tests import shuffle_fix_model as M

U = np.uint64
C1_INV = pow(int(devrng.FEISTEL_C1), -1, 1 << 16)


# ---- the xorshift as 32-bit operations -----------------------------------------------------------------------------------------------
def _F2_word_form(vl, vh, kl, kh, bits_: int):
    """feistel_F2 on a packed word with xorshift7_2: multiply-add per half, the xorshift on the WORD, multiply and shift per half."""
    m = U(0xFFFF)
    xl = (vl * devrng.FEISTEL_C1 + kl) & m
    xh = (vh * devrng.FEISTEL_C1 + kh) & m
    w = xl | (xh << U(16))
    w = w ^ ((w >> U(7)) & U(0x01FF01FF))
    yl = ((w & m) * devrng.FEISTEL_C2) & m
    yh = ((w >> U(16)) * devrng.FEISTEL_C2) & m
    return yl >> U(16 - bits_), yh >> U(16 - bits_)


def _inputs_of(x):
    """v with v * C1 == x (mod 2**16): with a key of 0 the xorshift of the round function sees exactly x."""
    return (x * U(C1_INV)) & U(0xFFFF)


def _assert_word_form_is_the_oracle(xl, xh):
    vl, vh = _inputs_of(xl), _inputs_of(xh)
    zero = U(0)
    gl, gh = _F2_word_form(vl, vh, zero, zero, 16)
    np.testing.assert_array_equal(gl, devrng._F(vl, zero, 16))
    np.testing.assert_array_equal(gh, devrng._F(vh, zero, 16))


@pytest.mark.parametrize("other", [0x0000, 0xFFFF, 0x007F, 0xFF80])
def test_xorshift_word_form_every_value_of_one_half_against_the_patterns_of_the_other(other):
    every = np.arange(1 << 16, dtype=U)
    fixed = np.full(1 << 16, other, dtype=U)
    _assert_word_form_is_the_oracle(every, fixed)  # the low half takes every value: nothing of the high half may reach it
    _assert_word_form_is_the_oracle(fixed, every)  # ... and the high half's seven low bits take every value


def test_xorshift_word_form_on_four_million_random_words():
    rng = np.random.default_rng(7)
    w = rng.integers(0, 1 << 32, 4_000_000, dtype=np.uint64)
    _assert_word_form_is_the_oracle(w & U(0xFFFF), w >> U(16))


def test_the_round_function_with_keys_and_every_shift_of_a_table_domain():
    rng = np.random.default_rng(8)
    vl, vh, kl, kh = (rng.integers(0, 1 << 16, 200_000, dtype=np.uint64) for _ in range(4))
    for bits_ in range(4, 15):  # digits of 16 .. 2**14 values
        gl, gh = _F2_word_form(vl, vh, kl, kh, bits_)
        np.testing.assert_array_equal(gl, devrng._F(vl, kl, bits_))
        np.testing.assert_array_equal(gh, devrng._F(vh, kh, bits_))


def test_the_mask_is_what_makes_the_word_form_exact():
    w = U(0x007F0000)  # the high half's seven low bits set: an unmasked 32-bit shift moves them into bits 9-15 of the low half
    assert (w >> U(7)) & U(0xFFFF) == U(0xFE00) and (w >> U(7)) & U(0x01FF01FF) == U(0)


# ---- the label of a rank by a carry --------------------------------------------------------------------------------------------------
def carry_entry(e):
    """sqgr_shuffle.hip: carry_entry, on two-field entries first | boundary << 16."""
    e = np.asarray(e, dtype=np.int64)
    first, boundary = e & 0xFF, e >> 16
    return np.where(boundary == 0, (first + 1) << 16, (first << 16) | ((0x10000 - boundary) & 0xFFFF))


def carry_label(entry, b):
    """Byte 2 of the 32-bit sum entry + b."""
    return (((np.asarray(entry, dtype=np.int64) + b) & 0xFFFFFFFF) >> 16) & 0xFF


def _perm_b32(s0: int, s1: int, sel: int) -> int:
    """v_perm_b32: byte i of the result is the byte of the 64-bit value s0:s1 that selector byte i names (0-3: s1, 4-7: s0), 0x0c: zero."""
    src = s1 | (s0 << 32)
    out = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xFF
        assert s < 8 or s == 0x0C
        out |= (0 if s == 0x0C else (src >> (8 * s)) & 0xFF) << (8 * i)
    return out


@pytest.mark.parametrize("B", [16, 977, 16_384])
def test_carry_form_gives_first_plus_b_ge_boundary_for_every_low_digit(B):
    b = np.arange(B, dtype=np.int64)
    stride = max(1, B // 37)
    boundaries = sorted({0, 1, B - 1, B, 0xFFFF} | set(range(2, B - 1, stride)))
    for K in (2, 30, 126):
        for first in sorted({0, K - 2, 125}):
            for boundary in boundaries:
                e = first | (boundary << 16)
                want = first + (b >= boundary)
                got = carry_label(carry_entry(e), b)
                np.testing.assert_array_equal(got, want, err_msg=f"B {B} first {first} boundary {boundary}")
                assert int(got.max()) <= 126  # a byte, and below the bit the sentinel test of the other instances reads


def test_the_entry_forms_named_in_the_kernel():
    K = 30
    assert int(carry_entry((K - 1) | (0xFFFF << 16))) == ((K - 1) << 16) | 1      # past rank n: K - 1, no boundary
    assert int(carry_entry(7 | (0 << 16))) == 8 << 16                             # a boundary on offset 0
    assert int(carry_entry(7 | (1 << 16))) == (7 << 16) | 0xFFFF                  # ... on offset 1: only b = 0 keeps `first`
    assert int(carry_label(carry_entry(7 | (0xFFFF << 16)), (1 << 14) - 1)) == 7  # the largest low digit never reaches "none"


def test_a_words_four_labels_are_assembled_by_two_byte_permutes_and_an_or():
    rng = np.random.default_rng(9)
    for _ in range(200):
        r = [int(v) for v in rng.integers(0, 1 << 32, 4, dtype=np.uint64)]  # entry + b of the word's four labels, bytes 0, 1, 3 arbitrary
        word = _perm_b32(r[1], r[0], 0x0C0C0602) | _perm_b32(r[3], r[2], 0x06020C0C)
        assert word == sum(((r[j] >> 16) & 0xFF) << (8 * j) for j in range(4))


def _sized(sizes) -> np.ndarray:
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


TABLES = [
    # (cluster sizes, what the labeling puts into the table) — 993: 32 x 32, 1024: 32 x 32 and E = 0, 4097: 128 x 33
    ([64, 929], "a boundary on offset 0 of block 2: the block starts with its label, no event inside"),
    ([63, 930], "a boundary on offset B - 1 of block 1"),
    ([1, 992], "a boundary on offset 1 of block 0"),
    ([500, 493], "blocks without a boundary, the last cluster ends in the partial block"),
    ([512, 512], "no rank outside [0, n)"),
    ([33 * 40 + 32, 4097 - 33 * 40 - 32], "offset B - 1 at B = 33, a partial last block of 5 ranks"),
    ([137] * 29 + [4097 - 137 * 29], "30 clusters"),
]


@pytest.mark.parametrize("sizes,what", TABLES)
def test_whole_tables_in_carry_form_give_the_sorted_base_at_every_rank_of_the_domain(sizes, what):
    labels, K = _sized(sizes), len(sizes)
    n = len(labels)
    A, B, _ = devrng.domain_dims(n)
    blk = M.block_table(M.boundaries(labels, K), n, K)
    assert M.refusal(blk, n, K) is None, what
    table = carry_entry(M.patched(blk, n, K))
    x = np.arange(A * B, dtype=np.int64)
    got = carry_label(table[x // B], x % B)
    np.testing.assert_array_equal(got[:n], np.sort(labels), err_msg=what)  # devrng.shuffled_labels: sort(labels)[rank]
    assert (got[n:] == K - 1).all()  # ranks outside: a label < K until k_shuffle_fix rewrites them
    np.testing.assert_array_equal(got, M.table_label(M.patched(blk, n, K), x, n))  # the two-field look-up it replaces
