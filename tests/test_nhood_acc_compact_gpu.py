"""One moment accumulator slot per (batch, plane, pair) on the 32-bit counter path (sqgr_nhood.hip: k_reduce sums d = count - shift
and d * d over the permutations of a pair inside the wave; k_finalize reads one layout for every counter mode).

What every case asserts: the per-permutation counts `==` the counts of the labels oracle/devrng.py generates, and
`s1 == sum_p (count_p - shift)`, `s2 == sum_p (count_p - shift)^2` formed in Python integers from the RETURNED counts — over
ranges that mask a head and a tail of the generator's groups of 16 (5 .. 37), none (0 .. 16) and a head only (16 .. 33).

K = 2, 3, 30, 50: 32-bit counters, 16 permutations per pass (K = 3: 144 slots, a partly filled last reduce block); K = 51, 101:
the 16-bit modes, whose k_reduce16 shares k_finalize.  Tunings: two batches per launch (several launch groups, a short last one),
32-wide rows (a pair is 32 lanes), planes of 8 and 4 permutations (one slot per plane and pair)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import devrng
from oracle import restate as O
from squidpy_amd._synthetic import hex_grid_graph

pytestmark = pytest.mark.gpu

SEED = 31
N = 300
NPERM = 37
RANGES = ((5, 37), (0, 16), (16, 33))
KS = (2, 3, 30, 50, 51, 101)


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@functools.lru_cache(maxsize=None)
def _graph(kind: str):
    if kind == "hex":
        adj = hex_grid_graph(20, 15).tocsr()
    else:
        one = np.ones(N - 1, dtype=np.float32)
        adj = sp.diags([one, one], [-1, 1], format="csr")
    assert adj.shape[0] == N
    return adj


@functools.lru_cache(maxsize=None)
def _perms():
    """The oracle's permutations 0 .. 36 of 300 items: they depend on (n, seed, perm) alone, every case reads them."""
    pis = devrng.label_permutations(N, SEED, np.arange(NPERM))
    pis.setflags(write=False)
    return pis


@functools.lru_cache(maxsize=None)
def _labels(k: int) -> np.ndarray:
    lab = np.random.default_rng(100 + k).integers(0, k, N).astype(np.int32)
    lab[:k] = np.arange(k)  # every cluster has a member
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _case(kind: str, k: int):
    """(adjacency, labels, shift = the observed counts, the oracle's counts of permutations 0 .. 36): computed once per case."""
    adj, lab = _graph(kind), _labels(k)
    base = np.sort(lab)
    want = np.stack([O.nhood_counts(adj.indices, adj.indptr, base[pi], k) for pi in _perms()]).astype(np.uint32)
    want.setflags(write=False)
    shift = O.nhood_counts(adj.indices, adj.indptr, lab, k).astype(np.int64)
    shift.setflags(write=False)
    return adj, lab, shift, want


def _moments(perms: np.ndarray, shift: np.ndarray):
    """sum_p d and sum_p d^2, d = count_p - shift, as exact Python integers -> (int64, uint64) arrays."""
    d = perms.astype(np.int64) - shift[None]
    s1 = d.sum(0)
    do = d.astype(object)
    s2 = (do * do).sum(0) if len(do) else np.zeros(d.shape[1:], dtype=object)
    return s1, s2


def _check_run(out, want, shift):
    s1, s2, perms = out
    np.testing.assert_array_equal(perms, want)
    e1, e2 = _moments(perms, shift)
    np.testing.assert_array_equal(s1, e1)
    assert s2.dtype == np.uint64 and (s2.astype(object) == e2).all()


def _check_plan(plan, shift, want, ranges=RANGES):
    for lo, hi in ranges:
        _check_run(plan.run(SEED, lo, hi, shift, return_perms=True), want[lo:hi], shift)


@pytest.mark.parametrize("kind", ["hex", "path"])
@pytest.mark.parametrize("k", KS)
def test_moments_are_the_sums_over_the_returned_counts(L, ctx, kind, k):
    adj, lab, shift, want = _case(kind, k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    assert plan.info()["counter_mode"] == (0 if k <= 50 else 2)
    _check_plan(plan, shift, want)
    plan.tune(0, 0, 2)  # 32 permutations per launch group: 0 .. 31, then a short group of one batch
    assert plan.info()["batches_per_launch"] == 2
    _check_plan(plan, shift, want)
    plan.close()
    g.close()


@pytest.mark.parametrize("kind", ["hex", "path"])
@pytest.mark.parametrize("k", [2, 3, 30, 50])
def test_few_partials_per_batch_are_walked_by_one_lane(L, ctx, kind, k):
    """k_reduce walks up to 16 partials per batch with one lane per slot (256 slots per block) and shares more among four slices
    (64 slots per block): both sides of that threshold, with automatic batches and with two per launch group."""
    adj, lab, shift, want = _case(kind, k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    seen = set()
    for blocks in (8, 15, 16, 17):
        plan.tune(0, blocks, 0)
        seen.add(plan.info()["blocks_per_batch"])
        _check_plan(plan, shift, want, ranges=((5, 37),))
    assert min(seen) <= 16 < max(seen), seen
    plan.tune(0, 8, 2)
    _check_plan(plan, shift, want)
    plan.close()
    g.close()


@pytest.mark.parametrize("kind", ["hex", "path"])
def test_rows_of_32_permutations(L, ctx, kind):
    k = 5
    adj, lab, shift, want = _case(kind, k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    plan.tune(32, 0, 0)
    assert plan.info()["slab_width"] == 32
    _check_plan(plan, shift, want)
    plan.tune(32, 0, 1)  # one row of 32 per launch group
    _check_plan(plan, shift, want)
    plan.tune(32, 8, 0)  # few partials per batch: one lane per slot walks them
    _check_plan(plan, shift, want, ranges=((5, 37),))
    plan.close()
    g.close()


@pytest.mark.parametrize("kind", ["hex", "path"])
@pytest.mark.parametrize("pass_w", [8, 4, 2, 1])
def test_planes_of_fewer_permutations_keep_a_slot_per_plane_and_pair(L, ctx, kind, pass_w):
    k = 30
    adj, lab, shift, want = _case(kind, k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    plan.tune(pass_w, 0, 0)
    info = plan.info()
    assert info["perms_per_pass"] == pass_w and info["counter_mode"] == 0
    _check_plan(plan, shift, want)
    plan.tune(pass_w, 0, 2)
    _check_plan(plan, shift, want, ranges=((5, 37),))
    plan.tune(pass_w, 8, 0)  # few partials per batch: one lane per slot walks them
    _check_plan(plan, shift, want, ranges=((5, 37),))
    plan.close()
    g.close()


def test_two_runs_on_one_plan_do_not_see_each_others_sums(L, ctx):
    """A second run over another range, and over an EMPTY one, starts from cleared accumulators."""
    k = 30
    adj, lab, shift, want = _case("hex", k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    _check_run(plan.run(SEED, 0, 37, shift, return_perms=True), want[0:37], shift)
    _check_run(plan.run(SEED, 16, 33, shift, return_perms=True), want[16:33], shift)
    s1, s2, _ = plan.run(SEED, 7, 7, shift)
    assert not s1.any() and not s2.any()
    _check_run(plan.run(SEED, 5, 37, None, return_perms=True), want[5:37], np.zeros((k, k), dtype=np.int64))
    plan.close()
    g.close()


@pytest.mark.parametrize("k", [3, 30, 101])
def test_counts_batch_of_injected_label_vectors(L, ctx, k):
    adj, lab, _, want = _case("hex", k)
    base = np.sort(lab)
    vectors = np.stack([base[pi] for pi in _perms()[:19]])  # 19: a batch of 16 and a partly filled one
    g = L.Graph(ctx, adj, with_data=False)
    np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, vectors, k), want[:19])
    g.close()


@pytest.mark.parametrize("k", [3, 30, 101])
def test_numpy_streams(L, ctx, k):
    """run_pcg64 against the reference loop restated with numpy's own generators (oracle/restate.py)."""
    from squidpy_amd._utils import pcg64_states

    adj, lab, shift, _ = _case("hex", k)
    P, seed = 21, 11
    ref = O.nhood_perm_counts_numpy(adj.indices, adj.indptr, lab, k, seed, P).astype(np.uint32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    _check_run(plan.run_pcg64(pcg64_states(seed, P), shift, return_perms=True), ref, shift)
    plan.close()
    g.close()


def test_no_allocation_between_a_warm_up_run_and_three_further_runs(L, ctx):
    """Accumulators, the moments' device block and its pinned twin are sized with the plan's workspace, never inside a run."""
    k = 30
    adj, lab, shift, want = _case("hex", k)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, lab, k)
    plan.run(SEED, 0, 37, shift, return_perms=True)
    a0 = ctx.alloc_counters()
    runs = [plan.run(SEED, lo, hi, shift, return_perms=True) for lo, hi in ((0, 37), (5, 37), (16, 33))]
    a1 = ctx.alloc_counters()
    assert a1["mallocs"] == a0["mallocs"] and a1["malloc_bytes"] == a0["malloc_bytes"] and a1["frees"] == a0["frees"]
    for out, (lo, hi) in zip(runs, ((0, 37), (5, 37), (16, 33))):
        _check_run(out, want[lo:hi], shift)
    plan.close()
    g.close()
