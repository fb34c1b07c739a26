"""The leaner spot loop of the table label shuffle (sqgr_shuffle.hip: k_shuffle_tab — the rank's digits advanced instead of divided,
an unmasked first walk of the group bijection, the high digit carried as a byte offset that the exact route shifts back, a word's
first label written with zero padding) against k_shuffle and oracle/devrng.py, bit for bit.  SQGR_SHUFFLE_TABLE: 2 requires the
table kernel, 0 forbids it, unset selects by launch size.

Sizes (A x B, excess A B - n of the generator's domain): 300 (32 x 16, 212: 41 % of the images re-walk), 4 097 (128 x 33, 127),
105 600 (512 x 207, 384: two trips per block at 160 rows), 1 015 809 (1024 x 993, 1023 — the largest excess; sixteen trips at 160
rows, the digits wrap on nearly every one), 2**20 - 5 and 2**20 (1024 x 1024, 5 and 0: never re-walks)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O

pytestmark = pytest.mark.gpu

SEED = 77
SMALL_N = (300, 4097, 105_600)
BIG_N = (1_015_809, 2**20 - 5, 2**20)
KS = (2, 30, 126, 127, 255, 256)   # K <= 126: the bit-7 sentinel test; above: per byte; 256: every label on the exact route
DISTS = ("uniform", "dirichlet", "empty", "one_spot")
# permutation p fills byte p & 3 of word (p & 15) >> 2 from packed half p & 1: byte 0 (written with zero padding) and the others
PERMS_SMALL = (0, 1, 10, 15, 20, 2**33 + 5)
PERMS_BIG = (2**33 + 4, 17)


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def test_domains_are_the_ones_the_cases_are_named_for():
    dims = {n: devrng.domain_dims(n)[:2] for n in SMALL_N + BIG_N}
    assert dims == {300: (32, 16), 4097: (128, 33), 105_600: (512, 207), 1_015_809: (1024, 993), 2**20 - 5: (1024, 1024),
                    2**20: (1024, 1024)}
    assert [a * b - n for n, (a, b) in dims.items()] == [212, 127, 384, 1023, 5, 0]


def _labels(n: int, k: int, dist: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rng.integers(0, k, n).astype(np.int32)
    if dist == "dirichlet":  # skewed sizes: blocks of the label-sorted base the two-field table cannot describe (exact route)
        return rng.choice(k, size=n, p=rng.dirichlet(np.full(k, 0.5))).astype(np.int32)
    if dist == "empty":      # only every third category occurs: sentinel blocks wherever a label is skipped
        return (3 * rng.integers(0, (k + 2) // 3, n)).clip(0, k - 1).astype(np.int32)
    assert dist == "one_spot"  # the last cluster has one spot
    lab = rng.integers(0, max(k - 1, 1), n).astype(np.int32)
    lab[rng.integers(0, n)] = k - 1
    return lab


@functools.lru_cache(maxsize=None)
def _perm(n: int, perm: int) -> np.ndarray:
    """The oracle's permutation: it depends on (n, seed, perm) alone, so the cases of one size share it."""
    pi = devrng.label_permutations(n, SEED, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


def _expected(labels: np.ndarray, perm: int) -> np.ndarray:
    """devrng.shuffled_labels(labels, SEED, perm) with the permutation taken from the cache."""
    return np.sort(labels)[_perm(len(labels), perm)].astype(np.uint8)


def test_cached_expectation_is_the_oracles_shuffled_labels():
    for n, k, dist in ((300, 30, "empty"), (4097, 256, "dirichlet")):
        labels = _labels(n, k, dist, seed=1)
        for perm in PERMS_SMALL:
            np.testing.assert_array_equal(_expected(labels, perm), devrng.shuffled_labels(labels, SEED, perm).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _identity(n: int):
    return sp.identity(n, format="csr", dtype=np.float32)


def _mode(monkeypatch, mode: str | None) -> None:
    if mode is None:
        monkeypatch.delenv("SQGR_SHUFFLE_TABLE", raising=False)
    else:
        monkeypatch.setenv("SQGR_SHUFFLE_TABLE", mode)


# every K with every distribution at the three small sizes; at the three sizes of the largest domain every K once and every
# distribution at least once, K = 30 with two of them
BIG_PAIRS = ((2, "one_spot"), (30, "uniform"), (30, "dirichlet"), (126, "empty"), (127, "one_spot"), (255, "uniform"), (256, "dirichlet"))
CASES = [(n, k, d) for n in SMALL_N for k in KS for d in DISTS] + [(n, k, d) for n in BIG_N for k, d in BIG_PAIRS]


@pytest.mark.parametrize("n,k,dist", CASES)
def test_shuffled_labels_required_never_unset_equal_the_oracle(L, ctx, n, k, dist, monkeypatch):
    labels = _labels(n, k, dist, seed=n + k)
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in PERMS_BIG if n in BIG_N else PERMS_SMALL:
        exp = _expected(labels, perm)
        for mode in ("2", "0", None):
            _mode(monkeypatch, mode)
            np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), exp, err_msg=f"perm {perm}, SQGR_SHUFFLE_TABLE={mode}")
    plan.close()
    g.close()


def _path_graph(n: int):
    """Spot i next to i - 1 and i + 1: a graph of any size whose counts see every slab row."""
    one = np.ones(n - 1, dtype=np.float32)
    return sp.diags([one, one], [-1, 1], format="csr")


def _run(plan, monkeypatch, mode, lo, hi, return_perms=True):
    _mode(monkeypatch, mode)
    out = plan.run(31, lo, hi, None, return_perms=return_perms)
    _mode(monkeypatch, None)
    return out


def _assert_same(a, b):
    for x, y in zip(a, b):
        if x is None:
            assert y is None
        else:
            np.testing.assert_array_equal(x, y)


RUN_CASES = [
    # (n, K, distribution, rows of 16 per launch)
    (300, 30, "empty", 5),
    (300, 256, "uniform", 3),
    (4097, 126, "dirichlet", 9),
    (4097, 127, "one_spot", 9),
    (105_600, 30, "uniform", 160),     # two trips per block
    (105_600, 30, "dirichlet", 161),   # ... and an odd last row, stored once
    (105_600, 126, "empty", 161),
    (1_015_809, 30, "uniform", 160),   # sixteen trips per thread: the advanced digits wrap
    (2**20 - 5, 30, "one_spot", 160),
    (2**20, 2, "uniform", 161),
]


@pytest.mark.parametrize("n,k,dist,rows", RUN_CASES)
def test_counts_per_permutation_required_equals_never(L, ctx, n, k, dist, rows, monkeypatch):
    """One launch of `rows` rows (every label byte of every row enters the counts) under 2 and 0; single permutations against
    the oracle's labels."""
    adj = _path_graph(n)
    labels = _labels(n, k, dist, seed=n + k + rows)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    lo, hi = 16, 16 + 16 * rows
    on = _run(plan, monkeypatch, "2", lo, hi)
    off = _run(plan, monkeypatch, "0", lo, hi)
    _assert_same(on, off)
    for j in (0, 16 * rows - 1):
        want = np.sort(labels)[devrng.label_permutations(n, 31, np.array([lo + j]))[0]]
        np.testing.assert_array_equal(on[2][j], O.nhood_counts(adj.indices, adj.indptr, want, k))
    plan.close()
    g.close()


def test_spot_map_takes_the_division_path(L, ctx, monkeypatch):
    """A plan on a renumbered twin (set_spot_map) divides the mapped rank out per spot; the plan on the caller's own graph advances
    the digits.  Same counts per permutation, 161 rows of 105 600 spots (two trips)."""
    from squidpy_amd._synthetic import hex_grid_graph

    adj = hex_grid_graph(330, 320).tocsr()
    n = adj.shape[0]
    assert n == 105_600
    labels = _labels(n, 30, "dirichlet", seed=4)
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    twin = g.renumbered(order)
    plan = L.NhoodPlan(ctx, twin, labels[order], 30)
    plan.set_spot_map(order)
    ref = L.NhoodPlan(ctx, g, labels, 30)
    for p in (plan, ref):
        p.tune(0, 0, 161)
    want = _run(ref, monkeypatch, "0", 0, 16 * 161)
    _assert_same(_run(ref, monkeypatch, "2", 0, 16 * 161), want)
    _assert_same(_run(plan, monkeypatch, "2", 0, 16 * 161), want)
    _assert_same(_run(plan, monkeypatch, "0", 0, 16 * 161), want)
    plan.set_spot_map(None)
    plan.close()
    ref.close()
    g.close()


def test_split_invariance_of_both_moments(L, ctx, monkeypatch):
    """A permutation range in one call and in two gives the same two moments, under 2 and under 0."""
    n = 105_600
    labels = _labels(n, 30, "one_spot", seed=8)
    g = L.Graph(ctx, _path_graph(n), with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, 30)
    lo, cut, hi = 7, 7 + 2600, 7 + 5400
    s1, s2, _ = _run(plan, monkeypatch, "2", lo, hi, return_perms=False)
    for mode in ("2", "0"):
        a1, a2, _ = _run(plan, monkeypatch, mode, lo, cut, return_perms=False)
        b1, b2, _ = _run(plan, monkeypatch, mode, cut, hi, return_perms=False)
        np.testing.assert_array_equal(a1 + b1, s1)
        np.testing.assert_array_equal(a2 + b2, s2)
    plan.close()
    g.close()
