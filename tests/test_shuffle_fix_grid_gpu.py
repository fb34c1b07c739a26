"""k_shuffle_fix with the FIX pair FORCED on tables built to be eligible (sqgr_shuffle.hip) against oracle/devrng.py, label for
label.  Written for a (ranks, permutation, row) launch grid of that kernel, which measured no faster than the flat index it was
to replace (profiles/run_overhead_before_after.md) and was not kept; the cases hold for either launch shape.

Sizes (A x B, E = A * B - n ranks outside): 300 (32 x 16, E = 212), 993 (32 x 32, E = 31), 1024 (32 x 32, E = 0: no fix kernel —
a grid of zero blocks is an invalid configuration, which the launch check would report, so a run that succeeds launched none),
4 097 (128 x 33, E = 127), and 105 600 (512 x 207, E = 384: more ranks than one block of 256 threads; the one size here at
which K = 126, the most clusters the pair takes, can be forced).

The FIX pair runs on ELIGIBLE tables only (LabelShuffler::fix_why): every block of B ranks of the label-sorted base holds at most
one label start, so K - 1 <= n // B.  Where such labels exist — K = 2 at every size, K = 30 from 993 spots on — the cases below
build them and FORCE the pair (SQGR_SHUFFLE_FIX=2, SQGR_SHUFFLE_TABLE=2).  No labelling of (300, 30) or of K = 126 at the four
small sizes is eligible (at most 19, 32, 33 and 125 labels): those cases assert that forcing is refused and check the labels of
the launch the library then selects.  Every (n, K) additionally runs uniform random labels with the selection left to the library.

Launches of 1, 2, 3 and 33 rows are checked through the per-permutation counts of a path graph, for every permutation."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O

pytestmark = pytest.mark.gpu

SEED = 77
SIZES = (300, 993, 1024, 4097)
KS = (2, 30, 126)
PERMS = (1, 10)  # bytes 1 and 2 of a word: both packed halves


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@functools.lru_cache(maxsize=None)
def _perm(n: int, seed: int, perm: int) -> np.ndarray:
    pi = devrng.label_permutations(n, seed, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def _identity(n: int):
    return sp.identity(n, format="csr", dtype=np.float32)


def _eligible_labels(n: int, k: int, seed: int) -> np.ndarray | None:
    """Labels whose sorted base starts label j >= 1 strictly inside a full block of its own; None when K - 1 > n // B."""
    _, B, _ = devrng.domain_dims(n)
    past = n // B
    if k - 1 > past:
        return None
    starts = [((2 * j - 1) * past // (2 * (k - 1))) * B + 1 + j % (B - 1) for j in range(1, k)]
    assert len({s // B for s in starts}) == k - 1 and all(0 < s % B for s in starts) and starts[-1] < past * B
    sizes = np.diff(np.array([0] + starts + [n]))
    assert (sizes > 0).all()
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(k), sizes)).astype(np.int32)


def _mode(monkeypatch, fix: str | None) -> None:
    monkeypatch.setenv("SQGR_SHUFFLE_TABLE", "2")
    if fix is None:
        monkeypatch.delenv("SQGR_SHUFFLE_FIX", raising=False)
    else:
        monkeypatch.setenv("SQGR_SHUFFLE_FIX", fix)


def _check_labels(plan, labels, n, fix, monkeypatch):
    base = np.sort(labels).astype(np.uint8)
    _mode(monkeypatch, fix)
    for perm in PERMS:
        np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), base[_perm(n, SEED, perm)], err_msg=f"perm {perm}, FIX={fix}")


@pytest.mark.parametrize("n,k", [(n, k) for n in SIZES for k in KS] + [(105_600, 30), (105_600, 126)])
def test_labels_equal_the_oracle(L, ctx, n, k, monkeypatch):
    g = L.Graph(ctx, _identity(n))
    forced = _eligible_labels(n, k, seed=n + k)
    assert (forced is not None) == (k == 2 or (k == 30 and n >= 993) or n == 105_600)
    if forced is not None:
        plan = L.NhoodPlan(ctx, g, forced, k)
        _check_labels(plan, forced, n, "2", monkeypatch)
        _check_labels(plan, forced, n, "0", monkeypatch)  # the same table behind the sentinel test
        plan.close()
    uniform = np.random.default_rng(n + k).integers(0, k, n).astype(np.int32)
    plan = L.NhoodPlan(ctx, g, uniform, k)
    if forced is None:  # no eligible labelling at all: the uniform one is refused by name
        _mode(monkeypatch, "2")
        with pytest.raises(L.SqgrError, match="not eligible"):
            plan.shuffled_labels(SEED, 1)
    _check_labels(plan, uniform, n, None, monkeypatch)
    plan.close()
    g.close()


# ---- launches of 1, 2, 3 and 33 rows -------------------------------------------------------------------------------------------------
ROWS_N, ROWS_K, ROWS_MAX = 4097, 30, 33


@functools.lru_cache(maxsize=None)
def _oracle_counts():
    """Counts of the oracle's labels for permutations 0 .. 16 * 33 - 1 of seed 31 on the path graph: computed once, read by every row count."""
    one = np.ones(ROWS_N - 1, dtype=np.float32)
    adj = sp.diags([one, one], [-1, 1], format="csr")
    labels = _eligible_labels(ROWS_N, ROWS_K, seed=5)
    base = np.sort(labels)
    pis = devrng.label_permutations(ROWS_N, 31, np.arange(16 * ROWS_MAX))
    out = np.stack([O.nhood_counts(adj.indices, adj.indptr, base[pi], ROWS_K) for pi in pis]).astype(np.uint32)
    out.setflags(write=False)
    return adj, labels, out


@pytest.mark.parametrize("rows", [1, 2, 3, 33])
def test_every_permutation_of_a_forced_launch_counts_as_the_oracles_labels(L, ctx, rows, monkeypatch):
    adj, labels, want = _oracle_counts()
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, ROWS_K)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    _mode(monkeypatch, "2")
    got = plan.run(31, 0, 16 * rows, None, return_perms=True)
    np.testing.assert_array_equal(got[2], want[: 16 * rows])
    if rows == 3:  # planes of 8 and 4 permutations: the fixed byte lands where slab_store16 put the spot's label
        for pass_w in (8, 4):
            plan.tune(pass_w, 0, rows)
            np.testing.assert_array_equal(plan.run(31, 0, 16 * rows, None, return_perms=True)[2], want[: 16 * rows], err_msg=f"planes of {pass_w}")
    plan.close()
    g.close()
