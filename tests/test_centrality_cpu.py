"""CPU: ``sq.gr.centrality_scores``'s host side against the reference's literal source and networkx
(tests/golden/centrality_reference.npz, made by tests/golden/make_centrality_golden.py): the signature and the enum, ``score``
parsing, the ``_build_graph`` restatements, and the numpy restatement of the bit-mask BFS and of the triangle counts that the GPU
tests compare the device integers with."""

from __future__ import annotations

import inspect
import json
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import squidpy_amd as sq
from squidpy_amd import AnnDataLite
from squidpy_amd._constants import Centrality, Key
from squidpy_amd.gr import _nhood

from tests import centrality_oracle as CO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "centrality_reference.npz"))
CASES = [str(c) for c in GOLD["cases"]]


def conn(name: str) -> sp.csr_matrix:
    n = len(GOLD[f"{name}/codes"])
    return sp.csr_matrix((GOLD[f"{name}/conn_data"], GOLD[f"{name}/conn_indices"], GOLD[f"{name}/conn_indptr"]), shape=(n, n))


def literal_adj(name: str) -> sp.csr_matrix:
    n = len(GOLD[f"{name}/codes"])
    indices = GOLD[f"{name}/adj_indices"]
    return sp.csr_matrix((np.ones(len(indices), np.float64), indices, GOLD[f"{name}/adj_indptr"]), shape=(n, n))


def test_signature_matches_reference():
    ref = json.loads(str(GOLD["signature"]))
    params = list(inspect.signature(sq.gr.centrality_scores).parameters.values())
    pos = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == [a["name"] for a in ref["positional"]]
    for p, a in zip(pos, ref["positional"]):
        assert p.default == (inspect.Parameter.empty if a["default"] is None else eval(a["default"])), p.name
    kwonly = {p.name: p for p in params if p.kind == p.KEYWORD_ONLY}
    assert {a["name"] for a in ref["keyword_only"]} | {"device"} == set(kwonly)
    assert all(p.default is None for p in kwonly.values())


def test_enum_and_slot_match_reference():
    assert [[m.name, m.value] for m in Centrality] == json.loads(str(GOLD["enum"]))
    assert Key.uns.centrality_scores("leiden") == "leiden_centrality_scores"
    assert tuple(m.s for m in Centrality) == CO.COLUMNS


def test_score_parsing():
    P = _nhood.parse_centralities
    assert P(None) == [Centrality.DEGREE, Centrality.CLUSTERING, Centrality.CLOSENESS]
    assert P("closeness_centrality") == [Centrality.CLOSENESS]
    assert P(Centrality.DEGREE) == [Centrality.DEGREE]
    assert P(["closeness_centrality", Centrality.DEGREE]) == [Centrality.CLOSENESS, Centrality.DEGREE]
    assert P(("average_clustering",)) == [Centrality.CLUSTERING]
    assert P(c for c in ["degree_centrality", "degree_centrality"]) == [Centrality.DEGREE]
    assert P([]) == []
    with pytest.raises(ValueError, match=r"Invalid option `betweenness` for `Centrality`. Valid options are:"):
        P("betweenness")
    with pytest.raises(ValueError, match="Invalid option `nope`"):
        P(["degree_centrality", "nope"])


def _adata(g, codes, n_cls) -> AnnDataLite:
    obs = pd.DataFrame({"cluster": pd.Categorical.from_codes(codes, [f"c{i}" for i in range(n_cls)])})
    return AnnDataLite(X=None, obs=obs, obsp={"spatial_connectivities": g})


def test_checks_raise_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_nhood, "default_context", boom)
    ad = _adata(conn("cancel12"), GOLD["cancel12/codes"], 2)
    with pytest.raises(ValueError, match="Invalid option `foo` for `Centrality`"):
        sq.gr.centrality_scores(ad, "cluster", score="foo")
    with pytest.raises(KeyError, match="Cluster key `nope` not found"):
        sq.gr.centrality_scores(ad, "nope")
    with pytest.raises(KeyError, match="Spatial connectivity key `other_connectivities` not found"):
        sq.gr.centrality_scores(ad, "cluster", connectivity_key="other")
    with pytest.raises(ValueError, match="Number of cores"):
        sq.gr.centrality_scores(ad, "cluster", n_jobs=0)
    ad.obs["number"] = np.arange(12.0)
    with pytest.raises(TypeError, match="to be `categorical`"):
        sq.gr.centrality_scores(ad, "number")
    with pytest.raises(AssertionError, match="the device was touched"):
        sq.gr.centrality_scores(ad, "cluster")


@pytest.mark.parametrize("name", CASES)
def test_build_graph_restatements_equal_literal(name):
    """The oracle's and the front end's ``_build_graph`` == the literal CSR: self loops, stored zeros and weights that cancel are no
    edges, rows sorted; the caller's matrix is left alone."""
    g = conn(name)
    before = (g.indptr.copy(), g.indices.copy(), g.data.copy())
    for build in (CO.build_graph, _nhood.centrality_graph):
        adj = build(g)
        assert np.array_equal(adj.indptr, GOLD[f"{name}/adj_indptr"]) and np.array_equal(adj.indices, GOLD[f"{name}/adj_indices"])
        assert adj.has_sorted_indices and (adj.data != 0).all() and (adj.diagonal() == 0).all()
    for a, b in zip(before, (g.indptr, g.indices, g.data)):
        assert np.array_equal(a, b)
    e = GOLD[f"{name}/edges"]  # what the reference hands rustworkx: the strict upper triangle, each edge once
    up = sp.triu(literal_adj(name), k=1).tocoo()
    assert np.array_equal(e, np.c_[up.row, up.col][np.lexsort((up.col, up.row))])


def test_cancel_case_has_what_it_says():
    g = conn("cancel12")
    assert (g.data == 0).sum() == 3 and (g.diagonal() != 0).sum() == 2
    adj = literal_adj("cancel12")
    assert adj[0, 6] == 0 and adj[2, 9] == 0 and adj[3, 8] == 0 and adj[0, 1] == 1 and adj[1, 0] == 1
    assert g[0, 6] == 1.5 and g[6, 0] == -1.5


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_golden(name):
    """Restatement == networkx for closeness and degree (``==``), == the literal ``_local_clustering`` for the coefficients and their
    group means (``==``); networkx's ``average_clustering`` (sequential sum) within assert_allclose's default tolerance."""
    adj, codes, K = literal_adj(name), GOLD[f"{name}/codes"], int(GOLD[f"{name}/n_cls"])
    cc = CO.local_clustering(adj, CO.two_triangles(adj))
    assert np.array_equal(cc, GOLD[f"{name}/cc"])
    got = CO.scores(adj, codes, K)
    for c in CO.COLUMNS:
        assert np.array_equal(got[c], GOLD[f"{name}/{c}"]), c
    np.testing.assert_allclose(got["average_clustering"], GOLD[f"{name}/nx_average_clustering"])
    pinned = GOLD[f"{name}/pinned"]
    size = np.bincount(codes[codes >= 0], minlength=K)
    assert np.array_equal(pinned, (size > 0) & (size < len(codes)))
    for c in CO.COLUMNS:
        assert (got[c][~pinned] == 0.0).all()


def test_host_floats_equal_oracle():
    """The front end's float formation (``centrality_from_counts``) from the restatement's integers == the oracle's columns."""
    for name in CASES:
        adj, codes, K = literal_adj(name), GOLD[f"{name}/codes"], int(GOLD[f"{name}/n_cls"])
        adjacent, dist_sum, _, _ = CO.group_bfs(adj, codes, K)
        cols = _nhood.centrality_from_counts(list(Centrality), adj.shape[0], codes, K, np.diff(adj.indptr), CO.two_triangles(adj), adjacent, dist_sum)
        for c in CO.COLUMNS:
            assert cols[c].dtype == np.float64 and np.array_equal(cols[c], GOLD[f"{name}/{c}"]), (name, c)


def test_unpinned_groups_score_zero():
    """A category without observations and one that holds every node: 0.0 in all three columns."""
    adj = literal_adj("hex257")
    codes = np.zeros(257, np.int32)
    adjacent, dist_sum, reached, levels = CO.group_bfs(adj, codes, 2)
    assert not adjacent.any() and not dist_sum.any() and not reached.any() and levels == 0
    two_tri = CO.two_triangles(adj)
    assert two_tri.any()  # the nodes do have triangles: the 0.0 of the clustering column is the rule, not the data
    cols = _nhood.centrality_from_counts(list(Centrality), 257, codes, 2, np.diff(adj.indptr), two_tri, adjacent, dist_sum)
    got = CO.scores(adj, codes, 2)
    for c in CO.COLUMNS:
        assert np.array_equal(cols[c], [0.0, 0.0]) and np.array_equal(got[c], [0.0, 0.0]), c


def test_oracle_closed_forms():
    """Path with group {0}: dist_sum = n (n - 1) / 2, n - 1 levels; an in-place sweep in index order walks it in one level, so the
    case tells the two sweeps apart in natural order.  Hex interior: two_tri = 12; a clique with a hub: cc = 1."""
    n = 300
    g = CO.build_graph(CO.path_graph(n))
    codes = np.full(n, -1, np.int32)
    codes[0] = 0
    adjacent, dist_sum, reached, levels = CO.group_bfs(g, codes, 1)
    assert (adjacent[0], dist_sum[0], reached[0], levels) == (1, n * (n - 1) // 2, n - 1, n - 1)
    wrong = CO.group_bfs(g, codes, 1, in_place=True)
    assert wrong[1][0] == n - 1 and wrong[3] == 1
    tt = CO.two_triangles(literal_adj("hex40x50"))
    assert tt[50 * 20 + 25] == 12 and GOLD["hex40x50/cc"][50 * 20 + 25] == 0.4
    assert (GOLD["hub5000/cc"][1:41] == 1.0).all() and np.diff(GOLD["hub5000/adj_indptr"])[0] == 5000


@pytest.mark.parametrize("side", [2, 7, 40])
def test_lattice_closed_form_equals_the_oracle(side):
    """The closed form the GPU test of the 640 000-node lattice relies on, against the BFS restatement at the same construction."""
    adj, codes = CO.build_graph(CO.lattice_graph(side)), CO.lattice_codes(side)
    assert adj.shape[0] == side * side and adj.nnz == 4 * side * (side - 1)
    got, want = CO.group_bfs(adj, codes, 2), CO.lattice_closed_form(side)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert got[3] == want[3]


def test_unreached_component_adds_nothing():
    """Group 0 of the two-component cases has no member in the second component: those nodes add 0 to its distance sum."""
    adj, codes = literal_adj("comp70_k3"), GOLD["comp70_k3/codes"]
    assert not (codes[40:] == 0).any() and (codes == -1).sum() == 5 and np.diff(adj.indptr)[69] == 0
    _, _, reached, _ = CO.group_bfs(adj, codes, 3)
    assert reached[0] == 40 - (codes[:40] == 0).sum()


def test_oracle_against_live_networkx():
    nx = pytest.importorskip("networkx")
    for name in ("comp70_k65", "cancel12", "hex257"):
        adj, codes, K = CO.build_graph(conn(name)), GOLD[f"{name}/codes"], int(GOLD[f"{name}/n_cls"])
        G = nx.from_scipy_sparse_array(adj)
        got = CO.scores(adj, codes, K)
        for g in np.flatnonzero(GOLD[f"{name}/pinned"]):
            idx = [int(i) for i in np.flatnonzero(codes == g)]
            assert got["closeness_centrality"][g] == nx.group_closeness_centrality(G, idx)
            assert got["degree_centrality"][g] == nx.group_degree_centrality(G, idx)
            np.testing.assert_allclose(got["average_clustering"][g], nx.average_clustering(G, idx))
