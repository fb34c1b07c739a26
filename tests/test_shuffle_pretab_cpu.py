"""What the table label shuffle (sqgr_shuffle.hip: k_shuffle_tab) rests on since its tables are built once per launch and its
carry-free packed sums are 32-bit adds, in numpy on the arithmetic of oracle/devrng.py's restatement of the generator:

* the four sums written as ONE 32-bit add of the bit-cast words (add_nocarry) stay below 2**16 in both halves on every domain
  make_domain yields up to 2**20 spots, so no carry crosses the halves:
      round 1 of the eight-word block   gsb + T            < 2B  <= 2**15
      round 2 of the eight-word block   gsa4 + (x >> ash4) < 8A  <= 2**13
      pi_g, high digit                  a + (x >> ash)     < 2A
      pi_g, low digit                   b + (x >> bsh)     < 3B
* the 32-bit form equals the packed form (v_pk_add_u16: each half modulo 2**16) for EVERY admissible operand pair in both
  halves on two small domains;
* the words k_shuffle_tab_build writes for the row pairs of a launch, at the place a block's linear copy reads them, are the
  words of the in-block formula  T[g][a][t] = (F_B(a, k0 of 2t) mod B) | (F_B(a, k0 of 2t + 1) mod B) << 16."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import devrng

M16 = np.uint32(0xFFFF)
SHUF_TAB_MAX_A = 1024


def _domains(n_max: int = 2**20) -> dict[tuple[int, int, int], int]:
    """Every (A, B, Bmask) devrng.domain_dims (= make_domain) yields on a sweep of [1, n_max]: all n up to 4096, a stride of 61
    above, and both sides of every place the domain changes (n = A B and A B + 1 for every B of every A, squares, powers of 2)."""
    ns = set(range(1, 4097)) | set(range(4097, n_max + 1, 61)) | {n_max}
    A = 16
    while A <= SHUF_TAB_MAX_A:
        for B in range(16, A + 1):
            ns.update((A * B - 1, A * B, A * B + 1))
        ns.update((A * A // 4, A * A // 4 + 1))
        A <<= 1
    ns.update(r * r + d for r in range(2, 1025) for d in (-1, 0, 1))
    out: dict[tuple[int, int, int], int] = {}
    for n in sorted(ns):
        if 1 <= n <= n_max:
            out.setdefault(devrng.domain_dims(n), n)
    return out


def _bits(A: int, Bmask: int) -> tuple[int, int]:
    return int(A).bit_length() - 1, int(Bmask + 1).bit_length() - 1


def test_the_sweep_meets_every_table_domain():
    doms = _domains()
    # A = 16 serves n <= 256 (B = 16 throughout); from there on A = 2^m serves n in (A^2 / 4, A^2]: every B in (A / 4, A], from 16 on
    want = {(16, 16)} | {(A, B) for A in (32, 64, 128, 256, 512, 1024) for B in range(max(A // 4 + 1, 16), A + 1)}
    assert {(A, B) for A, B, _ in doms} == want
    for A, B, Bmask in doms:
        assert A & (A - 1) == 0 and 16 <= B <= A <= SHUF_TAB_MAX_A and B - 1 <= Bmask < 2 * B and (Bmask + 1) & Bmask == 0


def test_carry_free_sums_stay_below_2_16_in_both_halves_on_every_domain():
    x = np.arange(1 << 16, dtype=np.uint64)  # every 16-bit value of the round function before its final shift
    checked = 0
    for (A, B, Bmask), n in _domains().items():
        abits, bbits = _bits(A, Bmask)
        ash, bsh = 16 - abits, 16 - bbits
        assert ash >= 6, "the table kernel carries the high digit scaled by 4"
        fa, fb, fa4 = int((x >> np.uint64(ash)).max()), int((x >> np.uint64(bsh)).max()), int((x >> np.uint64(ash - 2)).max())
        assert fa == A - 1 and fb == Bmask and fa4 == 4 * A - 1
        sums = {  # largest operands of a half, the bound stated in the kernel, what the bound is at most
            "round 1: gsb + T": (B - 1, B - 1, 2 * B, 2**15),
            "round 2: gsa4 + (x >> ash4)": (4 * (A - 1), fa4, 8 * A, 2**13),
            "pi_g: a + (x >> ash)": (A - 1, fa, 2 * A, 2**15),
            "pi_g: b + (x >> bsh)": (B - 1, fb, 3 * B, 2**16 - 1),
        }
        for name, (xm, ym, bound, cap) in sums.items():
            assert xm + ym < bound <= cap < 2**16, f"{name} on {A} x {B} (n = {n})"
            # both halves hold the same kind of value: at the largest operands of both the one add is the packed add
            xs, ys = np.uint32(xm), np.uint32(ym)
            assert _word_add(xs, xs, ys, ys) == _packed_add(xs, xs, ys, ys) == np.uint32((xm + ym) * 0x10001)
        checked += 1
    assert checked > 1500


def _packed_add(xl, xh, yl, yh):
    """v_pk_add_u16: each half modulo 2**16."""
    return ((xl + yl) & M16) | (((xh + yh) & M16) << np.uint32(16))


def _word_add(xl, xh, yl, yh):
    """add_nocarry: one 32-bit add of the bit-cast words."""
    return ((xl | (xh << np.uint32(16))) + (yl | (yh << np.uint32(16)))).astype(np.uint32)


@pytest.mark.parametrize("n", [300, 993])  # 32 x 16 (B clamped, Bmask = 15) and 32 x 32 (Bmask = 31)
def test_word_add_equals_packed_add_for_every_admissible_operand_pair(n):
    A, B, Bmask = devrng.domain_dims(n)
    abits, bbits = _bits(A, Bmask)
    u = lambda *a: np.arange(*a, dtype=np.uint32)  # noqa: E731
    cases = {
        "round 1": (u(B), u(B)),                                   # gsb < B, table entry < B
        "round 2": (u(0, 4 * A, 4), u(1 << (abits + 2))),          # gsa4 = 4 a, x >> (ash - 2) < 4A
        "pi_g a": (u(A), u(1 << abits)),                           # a < A, F_A < A
        "pi_g b": (u(B), u(1 << bbits)),                           # b < B, F_B <= Bmask
    }
    for name, (xs, ys) in cases.items():
        pl = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)  # every operand pair of ONE half
        assert int((pl[:, 0] + pl[:, 1]).max()) < 2**16
        for h0 in range(0, len(pl), 256):  # ... against every operand pair of the other half, in slices
            ph = pl[h0 : h0 + 256]
            got = _word_add(pl[:, None, 0], ph[None, :, 0], pl[:, None, 1], ph[None, :, 1])
            want = _packed_add(pl[:, None, 0], ph[None, :, 0], pl[:, None, 1], ph[None, :, 1])
            assert np.array_equal(got, want), f"{name} on {A} x {B}"
    # the form is NOT exact once a low half can reach 2**16: the bound is what makes it so
    assert _word_add(np.uint32(0xFFFF), np.uint32(0), np.uint32(1), np.uint32(0)) != _packed_add(np.uint32(0xFFFF), np.uint32(0), np.uint32(1), np.uint32(0))


# ---- the prebuilt tables -------------------------------------------------------------------------------------------------------------
ROW_WORDS = 64  # key_words_per_row(16, 1): 8 group-key words, 8 x 2 sigma-key words, padding


def _key_rows(seed: int, perm0: int, nrows: int) -> np.ndarray:
    """k_keygen's rows for 16-wide batches without libraries: [8] group keys in both halves, then per pair t the words
    k0(2t) | k0(2t + 1) << 16 and k1(2t) | k1(2t + 1) << 16."""
    keys = np.zeros((nrows, ROW_WORDS), dtype=np.uint32)
    for r in range(nrows):
        row = perm0 + 16 * r
        gk = devrng.group_keys(seed, np.array([row // 16]))[0].astype(np.uint32) & M16
        keys[r, :8] = gk * np.uint32(0x10001)
        sk = devrng.sigma_keys(seed, np.arange(row, row + 16)).astype(np.uint32)
        for t in range(8):
            keys[r, 8 + 2 * t] = (sk[2 * t, 0] & M16) | (sk[2 * t + 1, 0] << np.uint32(16))
            keys[r, 8 + 2 * t + 1] = (sk[2 * t, 1] & M16) | (sk[2 * t + 1, 1] << np.uint32(16))
    return keys


def _F2(av: np.ndarray, kword: np.ndarray, bbits: int) -> tuple[np.ndarray, np.ndarray]:
    """feistel_F2 on a packed word: the round function in each 16-bit half."""
    lo = devrng._F(av.astype(np.uint64), kword.astype(np.uint64) & np.uint64(0xFFFF), bbits)
    hi = devrng._F(av.astype(np.uint64), kword.astype(np.uint64) >> np.uint64(16), bbits)
    return lo.astype(np.uint32), hi.astype(np.uint32)


def _min_sub(f: np.ndarray, B: int) -> np.ndarray:
    """v_pk_min_u16(f, f - B) on one half."""
    return np.minimum(f, (f - np.uint32(B)) & M16)


def _build_model(keys: np.ndarray, A: int, B: int, bbits: int, nrows: int, grid_x: int) -> np.ndarray:
    """k_shuffle_tab_build thread by thread: grid (grid_x, row pairs) x 256 threads, grid-stride over the A * 8 words of a group."""
    gy = (nrows + 1) // 2
    words = A * 8
    tabs = np.full(gy * 2 * words, 0xDEADBEEF, dtype=np.uint32)
    written = np.zeros(tabs.shape, dtype=np.int32)
    for y in range(gy):
        row0 = 2 * y
        row1 = min(row0 + 1, nrows - 1)
        ksA, ksB = keys[row0, 8:], keys[row1, 8:]
        for bx in range(grid_x):
            start = bx * 256 + np.arange(256)
            for idx in (start + s for s in range(0, words, grid_x * 256)):
                idx = idx[idx < words]
                av, t = (idx >> 3).astype(np.uint32), idx & 7
                for g, ks in ((0, ksA), (1, ksB)):
                    lo, hi = _F2(av, ks[t * 2], bbits)
                    word = _min_sub(lo, B) | (_min_sub(hi, B) << np.uint32(16))
                    at = y * 2 * words + g * words + idx
                    tabs[at] = word
                    written[at] += 1
    assert (written == 1).all(), "every word of every row pair is written exactly once"
    return tabs


@pytest.mark.parametrize("n,nrows", [(300, 1), (300, 2), (993, 3), (4097, 33), (105_600, 3), (1_000_000, 2)])
def test_prebuilt_table_words_equal_the_in_block_formula(n, nrows):
    A, B, Bmask = devrng.domain_dims(n)
    _, bbits = _bits(A, Bmask)
    seed, perm0 = 77 + n, 16 * 5
    keys = _key_rows(seed, perm0, nrows)
    tabs = _build_model(keys, A, B, bbits, nrows, grid_x=-(-A * 8 // 256))
    # a block of row pair y copies A * 4 rows of 16 bytes from tabs + y * A * 4 rows; a spot with group image (a, .) then reads the
    # 32 bytes at tabA + a * 32 (group A) or tabB = tabA + A * 32 (group B): words [g][a][t]
    lds = tabs.reshape((nrows + 1) // 2, 2, A, 8)
    a = np.arange(A, dtype=np.uint64)
    for y in range(lds.shape[0]):
        for g in (0, 1):
            row = min(2 * y + g, nrows - 1)  # an odd last row is paired with itself
            k0 = devrng.sigma_keys(seed, np.arange(perm0 + 16 * row, perm0 + 16 * row + 16))[:, 0].astype(np.uint64) & np.uint64(0xFFFF)
            F = devrng._F(a[:, None], k0[None, :], bbits)  # (A, 16): F_B(a, k0 of permutation j)
            assert int(F.max()) <= Bmask < 2 * B
            T = (F % np.uint64(B)).astype(np.uint32)
            want = T[:, 0::2] | (T[:, 1::2] << np.uint32(16))  # (A, 8): permutation 2t low, 2t + 1 high
            np.testing.assert_array_equal(lds[y, g], want, err_msg=f"row pair {y}, group {g}")
