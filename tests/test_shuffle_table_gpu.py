"""The table variant of the 16-wide label shuffle (sqgr_shuffle.hip: k_shuffle_tab — sigma's first round read from an LDS table)
against the kernel it replaces and against oracle/devrng.py, bit for bit.  SQGR_SHUFFLE_TABLE, read at every call: 0 never,
1 whenever the input is eligible, 2 required (an input the table kernel does not take is an error), unset automatic."""

from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O

pytestmark = pytest.mark.gpu

PERMS = (0, 1, 17, 2**33 + 5)


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
    if dist == "dirichlet":  # skewed sizes: blocks of the label-sorted base the two-field table cannot describe (exact route)
        return rng.choice(k, size=n, p=rng.dirichlet(np.full(k, 0.5))).astype(np.int32)
    assert dist == "empty"   # only every third category occurs
    return (3 * rng.integers(0, (k + 2) // 3, n)).clip(0, k - 1).astype(np.int32)


def _mode(monkeypatch, mode: str | None) -> None:
    if mode is None:
        monkeypatch.delenv("SQGR_SHUFFLE_TABLE", raising=False)
    else:
        monkeypatch.setenv("SQGR_SHUFFLE_TABLE", mode)


# every n with 30 clusters; every K (both sentinel tests: K <= 126 and above; slab plane widths below 16 from K = 51 on) at two
# sizes; the largest domains (A = 1024) at the ends of the K range
CASES = (
    [(n, 30, d) for n in (1, 7, 49, 300, 5000, 100_003, 1_000_000, 1_048_576) for d in ("uniform", "dirichlet")]
    + [(n, k, d) for n in (5000, 100_003) for k in (2, 5, 127, 200, 256) for d in ("uniform", "dirichlet")]
    + [(n, k, "dirichlet") for n in (1_000_000, 1_048_576) for k in (2, 127, 256)]
    + [(n, k, "empty") for n, k in ((300, 30), (5000, 127), (100_003, 200), (1_048_576, 256))]
)


@pytest.mark.parametrize("n,k,dist", CASES)
def test_shuffled_labels_table_on_equals_off_equals_oracle(L, ctx, n, k, dist, monkeypatch):
    labels = _labels(n, k, dist, seed=n + k)
    g = L.Graph(ctx, sp.identity(n, format="csr", dtype=np.float32))
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in PERMS:
        _mode(monkeypatch, "2")
        on = plan.shuffled_labels(77, perm)
        _mode(monkeypatch, "0")
        off = plan.shuffled_labels(77, perm)
        _mode(monkeypatch, None)
        auto = plan.shuffled_labels(77, perm)
        exp = devrng.shuffled_labels(labels, 77, perm)
        np.testing.assert_array_equal(on, off, err_msg=f"perm {perm}")
        np.testing.assert_array_equal(auto, off, err_msg=f"perm {perm}")
        np.testing.assert_array_equal(on, exp.astype(np.uint8), err_msg=f"perm {perm}")
    plan.close()
    g.close()


def _graph(kind: str, rows: int, cols: int):
    from squidpy_amd._synthetic import hex_grid, hex_grid_graph, knn_directed_graph

    if kind == "hex":
        return hex_grid_graph(rows, cols).tocsr()
    rng = np.random.default_rng(rows)
    return knn_directed_graph(hex_grid(rows, cols) + rng.normal(0.0, 3.0, (rows * cols, 2)), 6).tocsr()


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


@pytest.mark.parametrize("kind,k", [("hex", 30), ("hex", 127), ("knn", 12), ("knn", 200)])
def test_run_75_permutations_masked_tail_and_odd_row_count(L, ctx, kind, k, monkeypatch):
    """P = 75 from permutation 5 on: rows of 16 start at 0, five rows (the last row pair stores one row), a masked head and tail."""
    adj = _graph(kind, 60, 70)
    labels = _labels(adj.shape[0], k, "dirichlet" if k == 12 else "uniform", seed=k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    on = _run(plan, monkeypatch, "2", 5, 80)
    off = _run(plan, monkeypatch, "0", 5, 80)
    auto = _run(plan, monkeypatch, None, 5, 80)
    _assert_same(on, off)
    _assert_same(auto, off)
    for j in (0, 10, 11, 74):  # ... and the oracle's generator
        np.testing.assert_array_equal(on[2][j], O.nhood_counts(adj.indices, adj.indptr, devrng.shuffled_labels(labels, 31, 5 + j), k))
    plan.close()
    g.close()


@pytest.mark.parametrize("kind,k", [("hex", 30), ("knn", 60)])
def test_run_at_real_launch_size_automatic_path(L, ctx, kind, k, monkeypatch):
    """P = 2 600 on more than 1e5 spots: one full launch group of 160 rows (the size the automatic selection hands to the table
    kernel) and a short one behind it; unset == required == never, per permutation and in both moments."""
    adj = _graph(kind, 330, 320)
    assert adj.shape[0] >= 100_000
    labels = _labels(adj.shape[0], k, "uniform", seed=k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    assert plan.info()["batches_per_launch"] == 160
    auto = _run(plan, monkeypatch, None, 0, 2600)
    on = _run(plan, monkeypatch, "2", 0, 2600)
    off = _run(plan, monkeypatch, "0", 0, 2600)
    _assert_same(auto, off)
    _assert_same(on, off)
    for j in (0, 2559, 2599):
        np.testing.assert_array_equal(off[2][j], O.nhood_counts(adj.indices, adj.indptr, devrng.shuffled_labels(labels, 31, j), k))
    plan.close()
    g.close()


def test_renumbered_twin_with_spot_map(L, ctx, monkeypatch):
    """A plan on a renumbered twin (set_spot_map): the table kernel permutes the ranks of the caller's observations as k_shuffle does."""
    adj = _graph("hex", 330, 320)
    n = adj.shape[0]
    labels = _labels(n, 30, "uniform", seed=4)
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    twin = g.renumbered(order)
    plan = L.NhoodPlan(ctx, twin, labels[order], 30)
    plan.set_spot_map(order)
    ref = L.NhoodPlan(ctx, g, labels, 30)
    want = _run(ref, monkeypatch, "0", 3, 78)
    _assert_same(_run(plan, monkeypatch, "2", 3, 78), want)
    _assert_same(_run(plan, monkeypatch, "0", 3, 78), want)
    big = _run(ref, monkeypatch, "0", 0, 2600, return_perms=False)
    _assert_same(_run(plan, monkeypatch, None, 0, 2600, return_perms=False), big)
    _assert_same(_run(plan, monkeypatch, "2", 0, 2600, return_perms=False), big)
    plan.set_spot_map(None)
    plan.close()
    ref.close()
    g.close()


def test_inputs_the_table_kernel_does_not_take(L, ctx, monkeypatch):
    """Libraries, more than 2**20 spots, 32-wide rows: unset and 1 run k_shuffle (the oracle's labels and counts), 2 names the reason."""
    # libraries
    adj = _graph("hex", 60, 70)
    n = adj.shape[0]
    labels = _labels(n, 9, "uniform", seed=1)
    libs = np.random.default_rng(2).integers(0, 3, n).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, 9, libs, 3)
    for mode in (None, "1", "0"):
        _mode(monkeypatch, mode)
        np.testing.assert_array_equal(plan.shuffled_labels(5, 19), devrng.shuffled_labels(labels, 5, 19, libs, 3))
    want = _run(plan, monkeypatch, "0", 0, 75)
    _assert_same(_run(plan, monkeypatch, None, 0, 75), want)
    _assert_same(_run(plan, monkeypatch, "1", 0, 75), want)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_TABLE=2.*libraries"):
        plan.shuffled_labels(5, 19)
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_TABLE=2.*libraries"):
        plan.run(31, 0, 75)
    _mode(monkeypatch, None)
    plan.close()
    # 32 permutations per row
    plan = L.NhoodPlan(ctx, g, labels, 9)
    plan.tune(32, 0, 0)
    want = _run(plan, monkeypatch, "0", 0, 75)
    _assert_same(_run(plan, monkeypatch, None, 0, 75), want)
    _assert_same(_run(plan, monkeypatch, "1", 0, 75), want)
    np.testing.assert_array_equal(want[2][70], O.nhood_counts(adj.indices, adj.indptr, devrng.shuffled_labels(labels, 31, 70), 9))
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_TABLE=2.*32 permutations per row"):
        plan.run(31, 0, 75)
    _mode(monkeypatch, None)
    plan.close()
    g.close()
    # one spot more than 2**20: the high digit has 2048 values
    n = 2**20 + 1
    labels = _labels(n, 30, "uniform", seed=3)
    g = L.Graph(ctx, sp.identity(n, format="csr", dtype=np.float32))
    plan = L.NhoodPlan(ctx, g, labels, 30)
    exp = devrng.shuffled_labels(labels, 5, 17)
    for mode in (None, "1", "0"):
        _mode(monkeypatch, mode)
        np.testing.assert_array_equal(plan.shuffled_labels(5, 17), exp)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_TABLE=2.*2\\^20 spots"):
        plan.shuffled_labels(5, 17)
    _mode(monkeypatch, None)
    plan.close()
    g.close()


def test_split_invariance_across_the_launch_size_threshold(L, ctx, monkeypatch):
    """One permutation range in one call (full launch groups: the table kernel) and in pieces — some of a few rows (k_shuffle),
    some of full launch groups — gives the same moments; so does either kernel alone."""
    adj = _graph("hex", 330, 320)
    labels = _labels(adj.shape[0], 30, "uniform", seed=8)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, 30)
    lo, hi = 7, 7 + 5400
    s1, s2, _ = _run(plan, monkeypatch, None, lo, hi, return_perms=False)
    cuts = [lo, 40, 41, 300, 2900, 2948, 5390, hi]   # pieces of 33, 1, 259, 2600, 48, 2442 and 17 permutations
    p1 = np.zeros_like(s1)
    p2 = np.zeros_like(s2)
    for a, b in zip(cuts[:-1], cuts[1:]):
        t1, t2, _ = _run(plan, monkeypatch, None, a, b, return_perms=False)
        p1 += t1
        p2 += t2
    np.testing.assert_array_equal(p1, s1)
    np.testing.assert_array_equal(p2, s2)
    for mode in ("0", "2"):
        t1, t2, _ = _run(plan, monkeypatch, mode, lo, hi, return_perms=False)
        np.testing.assert_array_equal(t1, s1)
        np.testing.assert_array_equal(t2, s2)
    plan.close()
    g.close()
