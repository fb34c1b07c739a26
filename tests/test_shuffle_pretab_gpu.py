"""The table label shuffle with its tables built once per launch (sqgr_shuffle.hip: k_shuffle_tab_build in front of
k_shuffle_tab<.., PRETAB>) against oracle/devrng.py and against the in-block build, bit for bit.  SQGR_SHUFFLE_PRETAB, read at
every call: 0 the in-block build, unset | 1 the prebuilt tables; it applies to every instance of the table kernel (the FIX pair or
the sentinel test, with or without a spot map, K <= 126 or above), so every case runs under SQGR_SHUFFLE_TABLE=1|2.

Sizes (A x B): 300 (32 x 16), 993 (32 x 32), 1024 (32 x 32, no rank outside), 4 097 (128 x 33), 105 600 (512 x 207).
`shuffled_labels` launches ONE row (paired with itself); launches of 1, 2, 3 and 33 rows — one table set per row pair, an odd
last row paired with itself — are checked through the per-permutation counts of a path graph against the counts of the oracle's
labels, for every permutation of the launch."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O

pytestmark = pytest.mark.gpu

SEED = 77
SIZES = (300, 993, 1024, 4097, 105_600)
KS = (2, 30, 126, 200)   # 126: the largest K of the FIX pair; 200: the instances that keep the byte compares
PERMS = (1, 10)          # bytes 1 and 2 of a word: both packed halves
PRETAB = ("0", "1", None)


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


def _labels(n: int, k: int, dist: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if dist == "uniform":
        return rng.integers(0, k, n).astype(np.int32)
    assert dist == "dirichlet"
    return rng.choice(k, size=n, p=rng.dirichlet(np.full(k, 0.5))).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _perm(n: int, seed: int, perm: int) -> np.ndarray:
    """The oracle's permutation: it depends on (n, seed, perm) alone, so the cases of one size share it."""
    pi = devrng.label_permutations(n, seed, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def _identity(n: int):
    return sp.identity(n, format="csr", dtype=np.float32)


def _path_graph(n: int):
    """Spot i next to i - 1 and i + 1: a graph of any size whose counts see every slab row."""
    one = np.ones(n - 1, dtype=np.float32)
    return sp.diags([one, one], [-1, 1], format="csr")


def _mode(monkeypatch, pretab: str | None, table: str | None = "2", fix: str | None = None) -> None:
    for name, val in (("SQGR_SHUFFLE_PRETAB", pretab), ("SQGR_SHUFFLE_TABLE", table), ("SQGR_SHUFFLE_FIX", fix)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _run(plan, monkeypatch, pretab, lo, hi, table="2", fix=None, return_perms=True):
    _mode(monkeypatch, pretab, table, fix)
    out = plan.run(31, lo, hi, None, return_perms=return_perms)
    _mode(monkeypatch, None, None, None)
    return out


def _assert_same(a, b):
    for x, y in zip(a, b):
        if x is None:
            assert y is None
        else:
            np.testing.assert_array_equal(x, y)


# ---- labels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,dist", [(n, k, d) for n in SIZES for k in KS for d in ("uniform", "dirichlet")])
def test_shuffled_labels_in_block_prebuilt_and_unset_equal_the_oracle(L, ctx, n, k, dist, monkeypatch):
    labels = _labels(n, k, dist, seed=n + k)
    base = np.sort(labels).astype(np.uint8)
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in PERMS:
        exp = base[_perm(n, SEED, perm)]
        for pretab in PRETAB:
            for fix in (None, "0"):  # the FIX pair where the table is eligible, and the sentinel test on every table
                _mode(monkeypatch, pretab, "2", fix)
                np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), exp, err_msg=f"perm {perm}, PRETAB={pretab} FIX={fix}")
    plan.close()
    g.close()


# ---- launches of 1, 2, 3 and 33 rows -------------------------------------------------------------------------------------------------
ROWS_N, ROWS_K, ROWS_MAX = 4097, 30, 33


@functools.lru_cache(maxsize=None)
def _oracle_counts():
    """Counts of the oracle's labels for permutations 0 .. 16 * 33 - 1 of seed 31 on the path graph: computed once, read by every row count."""
    adj = _path_graph(ROWS_N)
    labels = _labels(ROWS_N, ROWS_K, "uniform", seed=5)
    base = np.sort(labels)
    pis = devrng.label_permutations(ROWS_N, 31, np.arange(16 * ROWS_MAX))
    out = np.stack([O.nhood_counts(adj.indices, adj.indptr, base[pi], ROWS_K) for pi in pis]).astype(np.uint32)
    out.setflags(write=False)
    return adj, labels, out


@pytest.mark.parametrize("rows", [1, 2, 3, 33])
def test_every_permutation_of_a_launch_counts_as_the_oracles_labels(L, ctx, rows, monkeypatch):
    adj, labels, want = _oracle_counts()
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, ROWS_K)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    for pretab in PRETAB:
        for fix in (None, "0"):
            got = _run(plan, monkeypatch, pretab, 0, 16 * rows, fix=fix)
            np.testing.assert_array_equal(got[2], want[: 16 * rows], err_msg=f"PRETAB={pretab} FIX={fix}")
    plan.close()
    g.close()


# ---- a spot map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 200])
def test_a_plan_with_a_spot_map_gives_the_moments_of_the_plan_on_the_callers_graph(L, ctx, k, monkeypatch):
    from squidpy_amd._synthetic import hex_grid_graph

    adj = hex_grid_graph(60, 70).tocsr()
    n = adj.shape[0]
    labels = _labels(n, k, "uniform", seed=k)
    g = L.Graph(ctx, adj, with_data=False)
    ref = L.NhoodPlan(ctx, g, labels, k)
    want = _run(ref, monkeypatch, None, 3, 78, table="0")  # k_shuffle on the caller's own graph
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    twin = g.renumbered(order)
    plan = L.NhoodPlan(ctx, twin, labels[order], k)
    plan.set_spot_map(order)
    for pretab in PRETAB:
        _assert_same(_run(plan, monkeypatch, pretab, 3, 78), want)
    plan.set_spot_map(None)
    plan.close()
    ref.close()
    g.close()


# ---- moments -------------------------------------------------------------------------------------------------------------------------
RUN_CASES = [
    # (n, K, rows of 16 per launch)
    (300, 2, 3),          # an odd last row stored once
    (4097, 200, 3),       # the byte compares, slab planes
    (4097, 30, 32),
    (105_600, 126, 32),   # slab planes
    (105_600, 30, 161),   # two trips per block, odd last row, and a short last launch group behind the first
]


@pytest.mark.parametrize("n,k,rows", RUN_CASES)
def test_moments_and_counts_prebuilt_equal_in_block_with_a_masked_head(L, ctx, n, k, rows, monkeypatch):
    """Permutations 7 .. 16 rows + 16: the first row's head is masked, the last launch group is one row (161: after a full one)."""
    adj = _path_graph(n)
    labels = _labels(n, k, "uniform", seed=n + k + rows)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    lo, hi = 7, 16 * rows + 16
    off = _run(plan, monkeypatch, "0", lo, hi)
    _assert_same(_run(plan, monkeypatch, None, lo, hi), off)
    _assert_same(_run(plan, monkeypatch, "1", lo, hi, table="1"), off)
    for j in (0, hi - lo - 1):
        want = np.sort(labels)[_perm(n, 31, lo + j)]
        np.testing.assert_array_equal(off[2][j], O.nhood_counts(adj.indices, adj.indptr, want, k))
    plan.close()
    g.close()


def test_the_table_workspace_is_reused_by_a_launch_of_fewer_row_pairs(L, ctx, monkeypatch):
    """32 rows per launch, 35 rows per run: the second launch of a run builds 2 row pairs into the workspace the first left 16 in,
    and the first launch of the next run writes all 16 again."""
    n, k, rows = 4097, 30, 32
    adj = _path_graph(n)
    labels = _labels(n, k, "uniform", seed=12)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    lo, hi = 0, 16 * rows + 40
    first = _run(plan, monkeypatch, None, lo, hi)
    _assert_same(_run(plan, monkeypatch, None, lo, hi), first)
    _assert_same(_run(plan, monkeypatch, "0", lo, hi), first)
    for j in (16 * rows - 1, 16 * rows, hi - 1):  # the last permutation of the full launch, the first and last of the short one
        want = np.sort(labels)[_perm(n, 31, j)]
        np.testing.assert_array_equal(first[2][j], O.nhood_counts(adj.indices, adj.indptr, want, k))
    plan.close()
    g.close()


# ---- timers, allocations -------------------------------------------------------------------------------------------------------------
def test_the_build_launch_is_inside_the_shuffle_timer_one_bracket_per_launch_group(L, ctx, monkeypatch):
    n, k, rows = 105_600, 30, 32
    labels = _labels(n, k, "uniform", seed=9)
    g = L.Graph(ctx, _path_graph(n), with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    _run(plan, monkeypatch, "0", 0, 16, return_perms=False)  # the graph's lists are built once, by the first run
    ctx.timer_enable(True)
    reps = {}
    for pretab in PRETAB:
        ctx.timer_reset()
        _run(plan, monkeypatch, pretab, 0, 16 * rows * 3 + 16, return_perms=False)
        reps[pretab] = ctx.timer_report()
    ctx.timer_enable(False)
    assert reps["0"]["nhood_shuffle"][0] == 4
    for pretab in ("1", None):
        assert set(reps[pretab]) == set(reps["0"])
        assert {name: v[0] for name, v in reps[pretab].items()} == {name: v[0] for name, v in reps["0"].items()}
    plan.close()
    g.close()


def test_no_allocation_between_a_warm_up_run_and_the_next_run(L, ctx, monkeypatch):
    """The warm-up runs the in-block build: the table workspace is sized with the plan's other workspaces, not by the first launch
    that reads it."""
    n, k, rows = 105_600, 30, 32
    labels = _labels(n, k, "uniform", seed=11)
    g = L.Graph(ctx, _path_graph(n), with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    lo, hi = 0, 16 * rows + 16
    warm = _run(plan, monkeypatch, "0", lo, hi)
    a0 = ctx.alloc_counters()
    runs = [_run(plan, monkeypatch, pretab, lo, hi) for pretab in (None, "1", "0", None)]
    a1 = ctx.alloc_counters()
    assert a1["mallocs"] == a0["mallocs"] and a1["malloc_bytes"] == a0["malloc_bytes"]
    for r in runs:
        _assert_same(r, warm)
    plan.close()
    g.close()
