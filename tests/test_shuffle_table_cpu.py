"""The identity the table variant of the label shuffle rests on (sqgr_shuffle.hip: k_shuffle_tab), in numpy on oracle/devrng.py's
restatement of the generator: sigma's first round `b' = (b + F_B(a, k0)) mod B` may read `F_B(a, k0) mod B` from a table indexed
by the high digit and reduce the sum with ONE conditional subtraction in 16-bit arithmetic."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import devrng

U16 = np.uint64(0xFFFF)


def _min_sub_u16(t: np.ndarray, B: int) -> np.ndarray:
    """v_pk_sub_i16 / v_pk_min_u16 on one half: min(t, t - B) with both operands taken modulo 2**16."""
    t = t & U16
    return np.minimum(t, (t - np.uint64(B)) & U16)


@pytest.mark.parametrize("n", [1, 7, 300, 5000, 65_537, 1_000_000, 2**20])
def test_table_round_equals_two_step_reduction(n):
    A, B, Bmask = devrng.domain_dims(n)
    assert A <= 1024 and 16 <= B <= A
    bbits = int(Bmask + 1).bit_length() - 1
    rng = np.random.default_rng(n)
    # real sigma keys of a few permutations plus uniformly random 16-bit keys (only the low 16 bits enter the round function)
    keys = np.concatenate([devrng.sigma_keys(rng.integers(0, 2**63), np.arange(40, 56))[:, 0].astype(np.uint64) & U16,
                           rng.integers(0, 2**16, 48).astype(np.uint64), np.array([0, 1, 0xFFFF], dtype=np.uint64)])
    a = np.arange(A, dtype=np.uint64)                                             # every high digit
    b = np.unique(np.concatenate([np.arange(min(B, 64)), np.arange(max(B - 64, 0), B), rng.integers(0, B, 400)])).astype(np.uint64)
    for k0 in range(0, len(keys), 8):                                             # (in chunks: bounded memory)
        F = devrng._F(a[None, :, None], keys[k0 : k0 + 8, None, None], bbits)     # (keys, A, 1)
        assert int(F.max()) <= Bmask < 2 * B
        # the table entry: one conditional subtraction brings F_B <= Bmask < 2B into [0, B)
        T = _min_sub_u16(F, B)
        np.testing.assert_array_equal(T, F % np.uint64(B))
        # what the generator computes (sqgr_rng.h: sigma_rounds; devrng._sigma): two conditional subtractions of b + F
        t = b[None, None, :] + F
        t = np.where(t >= B, t - np.uint64(B), t)
        want = np.where(t >= B, t - np.uint64(B), t)
        np.testing.assert_array_equal(want, (b[None, None, :] + F) % np.uint64(B))
        # the table kernel: 16-bit add of the stored value, one min(t, t - B)
        s = b[None, None, :] + T
        assert int(s.max()) < 2 * B <= 2**15, "b + (F mod B) must not carry out of 16 bits (nor reach the wrapped range of t - B)"
        np.testing.assert_array_equal(_min_sub_u16(s, B), want)
