"""The FIX instance of the table label shuffle with its block table in carry form (sqgr_shuffle.hip: carry_entry — the label of a
rank is byte 2 of `entry + b`, a word's four labels are assembled by two byte permutes) and the round function's xorshift as 32-bit
operations (sqgr_rng.h: xorshift7_2), against oracle/devrng.py and against the kernels that keep the two-field look-up, bit for bit.

SQGR_SHUFFLE_FIX=2 requires the FIX pair (so the table kernel runs whatever the launch size), =0 keeps the sentinel test and the
compare / add-with-carry look-up on the same tables.  The round function is every kernel's: the same labels are asked of k_shuffle
(SQGR_SHUFFLE_TABLE=0) and of the independent-bijection kernel (SQGR_SHUFFLE_INDEPENDENT=1, against its own restatement).

Sizes (A x B, E = A B - n): 1024 (32 x 32, 0), 993 (32 x 32, 31), 4 097 (128 x 33, 127: a partial last block), 105 600 (512 x 207,
384).  The labelings are constructed — the first K - 1 clusters follow a pattern, the last takes the rest, so most blocks hold no
boundary and the last cluster ends in the partial block — and are eligible by the model's rule (tests/shuffle_fix_model.py):
  half    sizes h, B - h, h, ...     boundaries on offsets h and 0 of consecutive blocks
  edge    sizes B - 1, 1, B - 1, ... boundaries on offsets B - 1 and 0
  block   sizes B, B, ...            every boundary on offset 0: the blocks start with their label and hold no event
K = 126 needs 63 (125) blocks in front of the last: it runs from 4 097 (105 600) spots on."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O
from tests import shuffle_fix_model as M

pytestmark = pytest.mark.gpu

SEED = 77
SIZES = (1024, 993, 4097, 105_600)
KS = (2, 30, 126)
KINDS = ("half", "edge", "block")
PERMS = (1, 10)   # bytes 1 and 2 of a word: both packed halves, both byte permutes


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _sizes(n: int, k: int, kind: str) -> list[int] | None:
    """Cluster sizes of the constructed labeling, None where the pattern's K - 1 clusters do not end in front of the partial block."""
    _, B, _ = devrng.domain_dims(n)
    pattern = {"half": (B // 2, B - B // 2), "edge": (B - 1, 1), "block": (B, B)}[kind]
    head = [pattern[j % 2] for j in range(k - 1)]
    if sum(head) > (n // B) * B or sum(head) >= n:
        return None
    return head + [n - sum(head)]


@functools.lru_cache(maxsize=None)
def _labels(n: int, k: int, kind: str) -> np.ndarray | None:
    sizes = _sizes(n, k, kind)
    if sizes is None:
        return None
    labels = np.random.default_rng(n + k).permutation(np.repeat(np.arange(k), sizes)).astype(np.int32)
    labels.setflags(write=False)
    return labels


CASES = [(n, k, kind) for n in SIZES for k in KS for kind in KINDS if _sizes(n, k, kind) is not None]


def test_the_constructed_labelings_are_eligible_and_put_boundaries_where_the_cases_say():
    assert {(n, k) for n, k, _ in CASES} == {(n, k) for n in SIZES for k in (2, 30)} | {(4097, 126), (105_600, 126)}
    assert {kind for n, k, kind in CASES if (n, k) == (4097, 126)} == {"half", "edge"} and (105_600, 126, "block") in CASES
    for n, k, kind in CASES:
        labels = _labels(n, k, kind)
        _, B, _ = devrng.domain_dims(n)
        cum = M.boundaries(labels, k)
        blk = M.block_table(cum, n, k)
        assert M.refusal(blk, n, k) is None, (n, k, kind)
        offsets = {int(c) % B for c in cum[1:k]}
        assert offsets <= {"half": {B // 2, 0}, "edge": {B - 1, 0}, "block": {0}}[kind]
        assert (0 in offsets) == (k > 2 or kind == "block") and (kind != "edge" or B - 1 in offsets)
        past = n // B
        assert int(cum[k - 1]) <= past * B and np.any(blk[:past] >> 16 == 0xFFFF)  # the last cluster holds the partial block; blocks without a boundary
        assert not np.any(blk[:past] >> 16 == 0)  # a boundary on offset 0 is the block's first label, not an entry with boundary 0


@functools.lru_cache(maxsize=None)
def _perm(n: int, seed: int, perm: int) -> np.ndarray:
    """The oracle's permutation: it depends on (n, seed, perm) alone, so the cases of one size share it."""
    pi = devrng.label_permutations(n, seed, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def _perm_independent(n: int, seed: int, perm: int) -> np.ndarray:
    pi = devrng.independent_label_permutations(n, seed, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def _identity(n: int):
    return sp.identity(n, format="csr", dtype=np.float32)


def _path_graph(n: int):
    """Spot i next to i - 1 and i + 1: a graph of any size whose counts see every slab row."""
    one = np.ones(n - 1, dtype=np.float32)
    return sp.diags([one, one], [-1, 1], format="csr")


def _mode(monkeypatch, fix: str | None = None, table: str | None = None, independent: str | None = None) -> None:
    for name, val in (("SQGR_SHUFFLE_FIX", fix), ("SQGR_SHUFFLE_TABLE", table), ("SQGR_SHUFFLE_INDEPENDENT", independent)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


# ---- labels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,kind", CASES)
def test_shuffled_labels_of_the_carry_form_equal_the_oracle_and_the_two_field_kernels(L, ctx, n, k, kind, monkeypatch):
    labels = _labels(n, k, kind)
    base = np.sort(labels).astype(np.uint8)
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in PERMS:
        exp = base[_perm(n, SEED, perm)]
        _mode(monkeypatch, fix="2")  # the FIX pair: carry-form entries
        on = plan.shuffled_labels(SEED, perm)
        np.testing.assert_array_equal(on, exp, err_msg=f"perm {perm}, SQGR_SHUFFLE_FIX=2")
        _mode(monkeypatch, fix="0", table="2")  # the table kernel with the sentinel test: two-field entries
        np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), on, err_msg=f"perm {perm}, SQGR_SHUFFLE_FIX=0")
        _mode(monkeypatch, table="0")  # k_shuffle: both rounds of sigma on the round function
        np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), exp, err_msg=f"perm {perm}, SQGR_SHUFFLE_TABLE=0")
        _mode(monkeypatch, independent="1")  # k_shuffle_indep: eight rounds per permutation
        np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), base[_perm_independent(n, SEED, perm)],
                                      err_msg=f"perm {perm}, SQGR_SHUFFLE_INDEPENDENT=1")
    _mode(monkeypatch)
    plan.close()
    g.close()


# ---- launches of 1, 2 and 33 rows ----------------------------------------------------------------------------------------------------
ROWS_N, ROWS_K, ROWS_KIND, ROWS_MAX = 4097, 30, "half", 33


@functools.lru_cache(maxsize=None)
def _oracle_counts():
    """Counts of the oracle's labels for permutations 0 .. 16 * 33 - 1 of seed 31 on the path graph: computed once, read by every row count."""
    adj = _path_graph(ROWS_N)
    labels = _labels(ROWS_N, ROWS_K, ROWS_KIND)
    base = np.sort(labels)
    pis = devrng.label_permutations(ROWS_N, 31, np.arange(16 * ROWS_MAX))
    out = np.stack([O.nhood_counts(adj.indices, adj.indptr, base[pi], ROWS_K) for pi in pis]).astype(np.uint32)
    out.setflags(write=False)
    return adj, labels, out


def _run(plan, monkeypatch, fix, table, lo, hi):
    _mode(monkeypatch, fix=fix, table=table)
    out = plan.run(31, lo, hi, None, return_perms=True)
    _mode(monkeypatch)
    return out


def _assert_same(a, b):
    for x, y in zip(a, b):
        if x is None:
            assert y is None
        else:
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("rows", [1, 2, 33])
def test_every_permutation_of_a_launch_counts_as_the_oracles_labels(L, ctx, rows, monkeypatch):
    """33: an odd last row, paired with itself and stored once."""
    adj, labels, want = _oracle_counts()
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, ROWS_K)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    on = _run(plan, monkeypatch, "2", None, 0, 16 * rows)
    np.testing.assert_array_equal(on[2], want[: 16 * rows])
    _assert_same(_run(plan, monkeypatch, "0", "2", 0, 16 * rows), on)  # both moments and the counts
    plan.close()
    g.close()


RUN_CASES = [
    # (n, K, kind, rows of 16 per launch)
    (1024, 30, "block", 1),      # E = 0: no fix launch behind the table kernel
    (993, 2, "edge", 2),
    (4097, 126, "edge", 33),     # slab planes narrower than 16, a boundary on offset 0 and one on B - 1 in 62 blocks
    (105_600, 126, "half", 33),  # two trips per block
    (105_600, 30, "block", 2),
]


@pytest.mark.parametrize("n,k,kind,rows", RUN_CASES)
def test_moments_and_counts_of_the_carry_form_equal_the_two_field_kernels(L, ctx, n, k, kind, rows, monkeypatch):
    """Permutations 7 .. 16 rows + 16: the first row's head is masked, a short launch group of one row follows the full one."""
    adj = _path_graph(n)
    labels = _labels(n, k, kind)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    lo, hi = 7, 16 * rows + 16
    on = _run(plan, monkeypatch, "2", None, lo, hi)
    _assert_same(_run(plan, monkeypatch, "0", "2", lo, hi), on)
    _assert_same(_run(plan, monkeypatch, None, "0", lo, hi), on)  # k_shuffle
    for j in (0, hi - lo - 1):
        want = np.sort(labels)[_perm(n, 31, lo + j)]
        np.testing.assert_array_equal(on[2][j], O.nhood_counts(adj.indices, adj.indptr, want, k))
    plan.close()
    g.close()
