"""The segment path of the permutation test's count kernel (sqgr_nhood.hip: k_count_seg over sqgr_graph::ensure_seg's list, k_count
over the residual edges) against the model of the list (tests/segments_model.py), against numpy counts of the full edge list and
against the path it replaces, all with ==.  SQGR_COUNT_SEGMENTS, read at every call: 0 never, 2 required (a plan the segment kernel
does not take is an error that names the reason), unset automatic (segments covering at least 90 % of the half edges)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import segments_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from squidpy_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    return L.default_context()


@functools.lru_cache(maxsize=None)
def _graph(name: str) -> sp.csr_matrix:
    from squidpy_amd._synthetic import hex_grid, hex_grid_graph, knn_directed_graph

    if name == "hex40x37":          # n = 1480: neither n nor the row width is a multiple of 16; segments and residual edges
        return hex_grid_graph(40, 37).tocsr()
    if name == "hex7x5":
        return hex_grid_graph(7, 5).tocsr()
    if name == "hex3x3":            # n = 9, below one segment
        return hex_grid_graph(3, 3).tocsr()
    if name == "path9":             # n = 9 and ONE dense entry: its 16 rows end 7 rows past the last spot
        return M.square_grid_graph(1, 9)
    if name == "sq4":
        return M.square_grid_graph(30, 30)
    if name == "sq8":
        return M.square_grid_graph(30, 30, diagonals=True)
    if name == "hex_extra":         # 200 random symmetric extra edges: both launches under one timer
        return M.with_extra_edges(_graph("hex40x37"), 200, seed=3)
    if name == "hex_random":        # random order: the segment list is empty
        return M.renumber(_graph("hex40x37"), np.random.default_rng(1).permutation(1480))
    if name == "hex_empty_rows":    # spots without a neighbour: a block of rows and every seventh spot
        keep = np.ones(1480, dtype=np.float32)
        keep[np.concatenate([np.arange(100, 140), np.arange(0, 1480, 7)])] = 0
        a = (sp.diags(keep) @ _graph("hex40x37") @ sp.diags(keep)).tocsr()
        a.eliminate_zeros()
        a.sort_indices()
        return a
    if name == "self_loops":
        a = (_graph("hex40x37") + sp.identity(1480, format="csr", dtype=np.float32)).tocsr()
        a.sort_indices()
        return a
    assert name == "directed"
    rng = np.random.default_rng(40)
    return knn_directed_graph(hex_grid(40, 37) + rng.normal(0.0, 3.0, (1480, 2)), 6).tocsr()


SEGMENTABLE = ("hex40x37", "hex7x5", "hex3x3", "path9", "sq4", "sq8", "hex_extra", "hex_random", "hex_empty_rows")
REFUSED = {"self_loops": "self loops", "directed": "not structurally symmetric"}


def _mode(monkeypatch, mode: str | None) -> None:
    if mode is None:
        monkeypatch.delenv("SQGR_COUNT_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("SQGR_COUNT_SEGMENTS", mode)


@functools.lru_cache(maxsize=None)
def _labels(name: str, k: int) -> np.ndarray:
    n = _graph(name).shape[0]
    return np.random.default_rng(1000 * k + n).integers(0, k, (40, n)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(name: str, k: int) -> np.ndarray:
    return M.counts_reference(_graph(name), _labels(name, k), k)


# ---- the list builder -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEGMENTABLE)
def test_segment_list_is_the_model_and_holds_every_half_edge_once(L, ctx, name):
    adj = _graph(name)
    g = L.Graph(ctx, adj, with_data=False)
    seg, res, nseg = g.segments()
    g.close()
    want_seg, want_res = M.segment_model(adj)
    ent = seg[:nseg].astype(np.int64)
    np.testing.assert_array_equal(ent, want_seg)                                   # the same entries in the order (r0, d)
    np.testing.assert_array_equal(M.sorted_edges(res), M.sorted_edges(want_res))
    both = np.concatenate([M.expand(ent), res.astype(np.int64).reshape(-1, 2)])
    np.testing.assert_array_equal(M.sorted_edges(both), M.sorted_edges(M.half_edges(adj)))  # triu(adj, 1): each edge exactly once
    fill = np.array([bin(int(m)).count("1") for m in ent[:, 2]], dtype=np.int64)
    assert np.all(fill >= 8) and np.all(ent[:, 0] % 16 == 0) and np.all(ent[:, 1] > 0)
    assert np.all(np.diff(ent[:, 0] * (1 << 32) + ent[:, 1]) > 0)
    assert len(seg) % 64 == 0 and len(seg) >= nseg + 7 * 64                        # whole iterations + the kernel's look-ahead
    assert not seg[nseg:].any()                                                    # the padding: zero masks (and rows 0, offset 0)
    if name == "hex_random":
        assert nseg == 0
    if name == "hex40x37":
        assert (nseg, len(res)) == (270, 163)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_graphs_without_a_segment_list(L, ctx, name):
    g = L.Graph(ctx, _graph(name), with_data=False)
    assert g.segments() is None
    g.close()


# ---- counts of injected label vectors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 30, 50])
@pytest.mark.parametrize("name", SEGMENTABLE)
def test_counts_batch_equals_numpy_in_every_mode(L, ctx, name, k, monkeypatch):
    g = L.Graph(ctx, _graph(name), with_data=False)
    for mode in ("2", "0", None):
        _mode(monkeypatch, mode)
        got = L.nhood_counts_batch(ctx, g, _labels(name, k), k)
        np.testing.assert_array_equal(got, _reference(name, k), err_msg=f"SQGR_COUNT_SEGMENTS={mode}")
    g.close()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_required_mode_refuses_with_a_reason_and_automatic_runs_as_before(L, ctx, name, monkeypatch):
    g = L.Graph(ctx, _graph(name), with_data=False)
    for mode in ("0", None):
        _mode(monkeypatch, mode)
        np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, _labels(name, 5), 5), _reference(name, 5))
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_COUNT_SEGMENTS=2.*" + REFUSED[name]):
        L.nhood_counts_batch(ctx, g, _labels(name, 5), 5)
    g.close()


def test_required_mode_refuses_51_clusters(L, ctx, monkeypatch):
    g = L.Graph(ctx, _graph("hex40x37"), with_data=False)
    _mode(monkeypatch, None)
    np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, _labels("hex40x37", 51), 51), _reference("hex40x37", 51))
    _mode(monkeypatch, "2")
    with pytest.raises(L.SqgrError, match="SQGR_COUNT_SEGMENTS=2.*50 clusters"):
        L.nhood_counts_batch(ctx, g, _labels("hex40x37", 51), 51)
    g.close()


def test_a_failed_list_build_falls_back_and_is_tried_again(L, ctx, monkeypatch):
    """The list is an optimisation: when its build fails (SQGR_SEG_FAIL_BUILD stands in for an allocation that fails), automatic mode
    counts on the half list as before — on that call and on the next —, required mode returns the error, and a later call builds it."""
    name, k = "hex_extra", 30
    g = L.Graph(ctx, _graph(name), with_data=False)
    monkeypatch.setenv("SQGR_SEG_FAIL_BUILD", "1")
    ctx.timer_enable(True)
    ctx.timer_reset()
    for _ in range(2):
        _mode(monkeypatch, None)
        np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, _labels(name, k), k), _reference(name, k))
        _mode(monkeypatch, "2")
        with pytest.raises(L.SqgrError, match="SQGR_SEG_FAIL_BUILD"):
            L.nhood_counts_batch(ctx, g, _labels(name, k), k)
    rep = ctx.timer_report()
    assert rep["nhood_count_b16_half"][0] >= 2 and rep.get("nhood_count_seg_half", (0, 0.0))[0] == 0
    monkeypatch.delenv("SQGR_SEG_FAIL_BUILD")
    ctx.timer_reset()
    _mode(monkeypatch, None)
    np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, _labels(name, k), k), _reference(name, k))
    rep = ctx.timer_report()
    ctx.timer_enable(False)
    assert rep["nhood_count_seg_half"][0] >= 1 and rep["nhood_count_b16_half"][0] == 0
    g.close()


def test_automatic_mode_builds_no_list_for_a_graph_without_segments(L, ctx, monkeypatch):
    """Random order: the coverage is counted on the CSR (graph_seg_coverage) and the list (graph_seg_list) is never built."""
    name, k = "hex_random", 5
    g = L.Graph(ctx, _graph(name), with_data=False)
    _mode(monkeypatch, None)
    ctx.timer_enable(True)
    ctx.timer_reset()
    np.testing.assert_array_equal(L.nhood_counts_batch(ctx, g, _labels(name, k), k), _reference(name, k))
    rep = ctx.timer_report()
    ctx.timer_enable(False)
    assert rep["graph_seg_coverage"][0] == 1 and rep.get("graph_seg_list", (0, 0.0))[0] == 0
    g.close()


# ---- plan.run ------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name,k", [("hex40x37", 30), ("hex_extra", 30), ("hex_extra", 50), ("sq8", 7)])
def test_run_75_permutations_masked_head_and_odd_row_count(L, ctx, name, k, monkeypatch):
    """P = 75 from permutation 5 on: five rows of 16, a masked head and tail; per-permutation counts and both moments."""
    from oracle import devrng
    from oracle import restate as O

    adj = _graph(name)
    labels = np.random.default_rng(k).integers(0, k, adj.shape[0]).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, k)
    ctx.timer_enable(True)
    ctx.timer_reset()
    on = _run(plan, monkeypatch, "2", 5, 80)
    rep = ctx.timer_report()
    ctx.timer_enable(False)
    assert rep["nhood_count_seg_half"][0] >= 1 and not any(t.startswith("nhood_count_b16") and c[0] for t, c in rep.items())  # both launches: ONE timer
    off = _run(plan, monkeypatch, "0", 5, 80)
    auto = _run(plan, monkeypatch, None, 5, 80)
    _assert_same(on, off)
    _assert_same(auto, off)
    for j in (0, 11, 74):
        np.testing.assert_array_equal(on[2][j], O.nhood_counts(adj.indices, adj.indptr, devrng.shuffled_labels(labels, 31, 5 + j), k))
    plan.close()
    g.close()


def test_renumbered_twin_with_spot_map(L, ctx, monkeypatch):
    """A plan on a renumbered twin (here: the scan order restored from a shuffled input) with a spot map, on the segment path."""
    scan = _graph("hex40x37")
    n = scan.shape[0]
    shuffled_of = np.random.default_rng(5).permutation(n).astype(np.int32)
    adj = M.renumber(scan, shuffled_of)                       # the caller's graph: a lattice in no spatial order
    order = np.argsort(shuffled_of).astype(np.int32)         # order[new] = old: the twin is the scan-order lattice again
    labels = np.random.default_rng(6).integers(0, 30, n).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    twin = g.renumbered(order)
    seg, res, nseg = twin.segments()
    assert nseg == 270
    plan = L.NhoodPlan(ctx, twin, labels[order], 30)
    plan.set_spot_map(order)
    ref = L.NhoodPlan(ctx, g, labels, 30)
    want = _run(ref, monkeypatch, "0", 5, 80)
    _assert_same(_run(plan, monkeypatch, "2", 5, 80), want)
    _assert_same(_run(plan, monkeypatch, None, 5, 80), want)
    _assert_same(_run(plan, monkeypatch, "0", 5, 80), want)
    plan.set_spot_map(None)
    plan.close()
    ref.close()
    g.close()


def test_run_at_real_launch_size_automatic_path(L, ctx, monkeypatch):
    """2 600 permutations on hex 250 x 400 (1e5 spots, 30 clusters): a full launch group of 160 rows and a short one; the automatic
    rule takes the segment kernel (timer report) and the moments == those of the half-list kernel."""
    from squidpy_amd._synthetic import hex_grid_graph

    adj = hex_grid_graph(250, 400).tocsr()
    labels = np.random.default_rng(30).integers(0, 30, adj.shape[0]).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    seg, res, nseg = g.segments()
    assert (nseg, len(M.half_edges(adj))) == (18_700, 298_701)
    plan = L.NhoodPlan(ctx, g, labels, 30)
    assert plan.info()["list_edges"] == 298_701
    ctx.timer_enable(True)
    ctx.timer_reset()
    auto = _run(plan, monkeypatch, None, 0, 2600, return_perms=False)
    rep = ctx.timer_report()
    ctx.timer_reset()
    off = _run(plan, monkeypatch, "0", 0, 2600, return_perms=False)
    rep_off = ctx.timer_report()
    ctx.timer_enable(False)
    assert rep["nhood_count_seg_half"][0] == 2 and rep.get("nhood_count_b16_half", (0, 0.0))[0] == 0
    assert rep_off["nhood_count_b16_half"][0] == 2 and rep_off["nhood_count_seg_half"][0] == 0  # (a reset keeps the names)
    _assert_same(auto, off)
    plan.close()
    g.close()


def test_split_invariance_in_required_mode(L, ctx, monkeypatch):
    adj = _graph("hex_extra")
    labels = np.random.default_rng(8).integers(0, 30, adj.shape[0]).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, 30)
    lo, hi = 7, 7 + 400
    s1, s2, _ = _run(plan, monkeypatch, "2", lo, hi, return_perms=False)
    p1, p2 = np.zeros_like(s1), np.zeros_like(s2)
    cuts = [lo, 40, 41, 300, 390, hi]
    for a, b in zip(cuts[:-1], cuts[1:]):
        t1, t2, _ = _run(plan, monkeypatch, "2", a, b, return_perms=False)
        p1 += t1
        p2 += t2
    np.testing.assert_array_equal(p1, s1)
    np.testing.assert_array_equal(p2, s2)
    _assert_same(_run(plan, monkeypatch, "0", lo, hi, return_perms=False)[:2], (s1, s2))
    plan.close()
    g.close()


def test_soak_same_launch_50_times(L, ctx, monkeypatch):
    """The same small launch 50 times, all results equal: increments still in flight at the flush barrier would show as a count that
    comes and goes (the explicit wait in front of the barrier, as in k_count)."""
    adj = _graph("hex_extra")
    labels = np.random.default_rng(9).integers(0, 30, adj.shape[0]).astype(np.int32)
    g = L.Graph(ctx, adj, with_data=False)
    plan = L.NhoodPlan(ctx, g, labels, 30)
    first = _run(plan, monkeypatch, "2", 0, 160)
    for _ in range(49):
        _assert_same(_run(plan, monkeypatch, "2", 0, 160), first)
    _assert_same(_run(plan, monkeypatch, "0", 0, 160), first)
    plan.close()
    g.close()
