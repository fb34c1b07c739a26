"""The FIX pair of the table label shuffle (sqgr_shuffle.hip: k_shuffle_tab without its sentinel test, k_shuffle_fix behind it)
against oracle/devrng.py and against the kernels it replaces, bit for bit.  SQGR_SHUFFLE_FIX, read at every call: 0 never, 2 required
(the table kernel then takes an eligible input whatever the launch size; a launch that is not eligible is an error that names the
reason), unset: whenever the table kernel runs on eligible tables.  Eligibility of a label vector is the model's
(tests/shuffle_fix_model.py: refusal), so every case states what =2 must do with it.

Sizes (A x B, E = A B - n): 300 (32 x 16, 212 > A: chains of out-of-range ranks, whole blocks behind the last rank), 993 (32 x 32,
31), 1024 (E = 0: no fix launch), 4 097 (128 x 33, 127), 105 600 (512 x 207, 384), 2**20 - 5 (1024 x 1024, 5), 2**20 (0)."""

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
SIZES = (300, 993, 1024, 4097, 105_600, 2**20 - 5, 2**20)
KS = (2, 30, 126)   # 126: the largest K of the FIX pair, slab planes narrower than 16
PERMS = (1, 10, 2**33 + 5)   # bytes 1 and 2 of a word from both packed halves; a permutation index past 2**32


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


def _why_not(labels: np.ndarray, k: int) -> str | None:
    n = len(labels)
    return M.refusal(M.block_table(M.boundaries(labels, k), n, k), n, k)


@functools.lru_cache(maxsize=None)
def _perm(n: int, seed: int, perm: int) -> np.ndarray:
    """The oracle's permutation: it depends on (n, seed, perm) alone, so the cases of one size share it."""
    pi = devrng.label_permutations(n, seed, np.array([perm]))[0]
    pi.setflags(write=False)
    return pi


@functools.lru_cache(maxsize=None)
def _identity(n: int):
    return sp.identity(n, format="csr", dtype=np.float32)


def _mode(monkeypatch, fix: str | None, table: str | None = None) -> None:
    for name, val in (("SQGR_SHUFFLE_FIX", fix), ("SQGR_SHUFFLE_TABLE", table)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


CASES = [(n, k, d) for n in SIZES for k in KS for d in ("uniform", "dirichlet")]


def test_the_cases_hold_eligible_tables_at_every_size_and_cluster_count():
    ok = {(n, k) for n, k, d in CASES if _why_not(_labels(n, k, d, seed=n + k), k) is None}
    assert {n for n, _ in ok} == set(SIZES) and {k for _, k in ok} == set(KS)
    assert {(n, 126) for n in (105_600, 2**20 - 5, 2**20)} <= ok


# ---- labels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,dist", CASES)
def test_shuffled_labels_required_never_unset_equal_the_oracle(L, ctx, n, k, dist, monkeypatch):
    labels = _labels(n, k, dist, seed=n + k)
    why = _why_not(labels, k)
    base = np.sort(labels).astype(np.uint8)
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, k)
    for perm in PERMS:
        exp = base[_perm(n, SEED, perm)]
        _mode(monkeypatch, "2")
        if why is None:
            np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), exp, err_msg=f"perm {perm}, SQGR_SHUFFLE_FIX=2")
        else:
            with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2"):
                plan.shuffled_labels(SEED, perm)
        # never (on the table kernel), unset (k_shuffle at this launch size), unset on the table kernel (the pair where eligible)
        for fix, table in (("0", "2"), (None, None), (None, "1")):
            _mode(monkeypatch, fix, table)
            np.testing.assert_array_equal(plan.shuffled_labels(SEED, perm), exp, err_msg=f"perm {perm}, FIX={fix} TABLE={table}")
    plan.close()
    g.close()


# ---- moments -------------------------------------------------------------------------------------------------------------------------
def _path_graph(n: int):
    """Spot i next to i - 1 and i + 1: a graph of any size whose counts see every slab row."""
    one = np.ones(n - 1, dtype=np.float32)
    return sp.diags([one, one], [-1, 1], format="csr")


def _run(plan, monkeypatch, fix, table, lo, hi, return_perms=True):
    _mode(monkeypatch, fix, table)
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
    # (n, K, rows of 16 per launch)
    (300, 2, 3),          # E > A, an odd last row stored once
    (4097, 30, 32),
    (105_600, 30, 3),
    (105_600, 126, 32),   # slab planes
    (105_600, 30, 161),   # two trips per block, odd last row, and a short last launch group behind the first
    (2**20 - 5, 30, 161),
]


@pytest.mark.parametrize("n,k,rows", RUN_CASES)
def test_moments_and_counts_required_equal_never_with_a_masked_head(L, ctx, n, k, rows, monkeypatch):
    """Permutations 7 .. 16 rows + 16: the first row's head is masked, the last launch group is one row (161: after a full one)."""
    adj = _path_graph(n)
    labels = _labels(n, k, "uniform", seed=n + k + rows)
    assert _why_not(labels, k) is None
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    assert plan.info()["batches_per_launch"] == rows
    lo, hi = 7, 16 * rows + 16
    on = _run(plan, monkeypatch, "2", None, lo, hi)
    off = _run(plan, monkeypatch, "0", "2", lo, hi)
    auto = _run(plan, monkeypatch, None, "1", lo, hi)
    _assert_same(on, off)
    _assert_same(auto, off)
    for j in (0, hi - lo - 1):
        want = np.sort(labels)[devrng.label_permutations(n, 31, np.array([lo + j]))[0]]
        np.testing.assert_array_equal(on[2][j], O.nhood_counts(adj.indices, adj.indptr, want, k))
    plan.close()
    g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _sized(sizes, seed=3) -> np.ndarray:
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


@pytest.mark.parametrize(
    "sizes,reason",
    [
        ([500, 10, 490], "several label starts"),        # a cluster smaller than one block
        ([500, 0, 500], "several label starts"),         # an empty category
        ([996, 4], "does not end in label K - 1"),        # the last block: K - 2 | K - 1 | out of range
        ([1000] + [0] * 126, "more than 126 clusters"),
    ],
)
def test_tables_that_are_not_eligible_are_refused_with_the_reason_and_run_as_before(L, ctx, sizes, reason, monkeypatch):
    labels, k = _sized(sizes), len(sizes)
    n = len(labels)
    assert _why_not(labels, k) is not None
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, k)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*" + reason):
        plan.shuffled_labels(SEED, 17)
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*" + reason):
        plan.run(31, 0, 48)
    exp = np.sort(labels).astype(np.uint8)[_perm(n, SEED, 17)]
    for fix, table in ((None, None), (None, "1"), ("0", "2")):
        _mode(monkeypatch, fix, table)
        np.testing.assert_array_equal(plan.shuffled_labels(SEED, 17), exp)
    plan.close()
    g.close()


def test_launches_that_are_not_eligible_are_refused_with_the_reason_and_run_as_before(L, ctx, monkeypatch):
    """Libraries, a spot map, SQGR_SHUFFLE_TABLE=0, 32-wide rows, more than 2**20 spots — on tables that would qualify."""
    from squidpy_amd._synthetic import hex_grid_graph

    adj = hex_grid_graph(60, 70).tocsr()
    n = adj.shape[0]
    labels = _labels(n, 2, "uniform", seed=1)
    assert _why_not(labels, 2) is None
    g = L.Graph(ctx, adj, with_data=False)
    # libraries
    libs = np.random.default_rng(2).integers(0, 3, n).astype(np.int32)
    plan = L.NhoodPlan(ctx, g, labels, 2, libs, 3)
    want = _run(plan, monkeypatch, "0", None, 0, 75)
    _assert_same(_run(plan, monkeypatch, None, None, 0, 75), want)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*libraries"):
        plan.run(31, 0, 75)
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*libraries"):
        plan.shuffled_labels(5, 19)
    _mode(monkeypatch, None)
    np.testing.assert_array_equal(plan.shuffled_labels(5, 19), devrng.shuffled_labels(labels, 5, 19, libs, 3))
    plan.close()
    # a spot map: the plan on a renumbered twin
    order = np.random.default_rng(5).permutation(n).astype(np.int32)
    twin = g.renumbered(order)
    plan = L.NhoodPlan(ctx, twin, labels[order], 2)
    plan.set_spot_map(order)
    ref = L.NhoodPlan(ctx, g, labels, 2)
    want = _run(ref, monkeypatch, "2", None, 3, 78)
    _assert_same(_run(ref, monkeypatch, "0", "0", 3, 78), want)
    _assert_same(_run(plan, monkeypatch, None, "1", 3, 78), want)
    _assert_same(_run(plan, monkeypatch, "0", "2", 3, 78), want)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*spot map"):
        plan.run(31, 3, 78)
    _mode(monkeypatch, None)
    plan.set_spot_map(None)
    plan.close()
    # the table kernel switched off; 32-wide rows
    _mode(monkeypatch, "2", "0")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*SQGR_SHUFFLE_TABLE=0"):
        ref.run(31, 3, 78)
    ref.tune(32, 0, 0)
    _assert_same(_run(ref, monkeypatch, None, None, 0, 75), _run(ref, monkeypatch, "0", None, 0, 75))
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*32 permutations per row"):
        ref.run(31, 0, 75)
    _mode(monkeypatch, None)
    ref.close()
    g.close()
    # one spot more than 2**20
    n = 2**20 + 1
    labels = _labels(n, 2, "uniform", seed=3)
    g = L.Graph(ctx, _identity(n))
    plan = L.NhoodPlan(ctx, g, labels, 2)
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_SHUFFLE_FIX=2.*2\\^20 spots"):
        plan.shuffled_labels(5, 17)
    _mode(monkeypatch, None)
    np.testing.assert_array_equal(plan.shuffled_labels(5, 17), np.sort(labels).astype(np.uint8)[_perm(n, 5, 17)])
    plan.close()
    g.close()


# ---- timers, soak --------------------------------------------------------------------------------------------------------------------
def test_the_fix_launch_is_inside_the_shuffle_timer_same_name_same_launch_count(L, ctx, monkeypatch):
    n, k, rows = 105_600, 30, 32
    labels = _labels(n, k, "uniform", seed=9)
    assert _why_not(labels, k) is None
    g = L.Graph(ctx, _path_graph(n), with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    _run(plan, monkeypatch, "0", "2", 0, 16, return_perms=False)  # the graph's lists are built once, by the first run
    ctx.timer_enable(True)
    reps = {}
    for fix, table in (("0", "2"), ("2", None), (None, "1")):
        ctx.timer_reset()
        _run(plan, monkeypatch, fix, table, 0, 16 * rows * 3 + 16, return_perms=False)
        reps[fix] = ctx.timer_report()
    ctx.timer_enable(False)
    assert reps["0"]["nhood_shuffle"][0] == 4
    for fix in ("2", None):
        assert set(reps[fix]) == set(reps["0"])
        assert {name: v[0] for name, v in reps[fix].items()} == {name: v[0] for name, v in reps["0"].items()}
    plan.close()
    g.close()


def test_the_same_launch_twenty_times_gives_the_same_moments(L, ctx, monkeypatch):
    n, k, rows = 105_600, 30, 32
    labels = _labels(n, k, "uniform", seed=10)
    assert _why_not(labels, k) is None
    g = L.Graph(ctx, _path_graph(n), with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    plan.tune(0, 0, rows)
    first = _run(plan, monkeypatch, "0", "2", 0, 16 * rows, return_perms=False)
    for _ in range(20):
        _assert_same(_run(plan, monkeypatch, "2", None, 0, 16 * rows, return_perms=False), first)
    plan.close()
    g.close()
