"""CPU: the numpy restatement of ``sqgr_leiden`` (tests/niche_leiden_oracle.py) pinned to what can be checked without leidenalg, and
everything ``niche_leiden`` and the two niche drop-ins do without a device.

- Every case x resolution: a valid canonical labelling; every community connected in the input graph (Leiden's guarantee; it holds by
  construction); after ``n_iterations=-1`` no vertex has a strictly better neighbouring community, compared in exact
  rational arithmetic — asserted wherever the stats report no sweep cap hit and a settled run, and the stats must say so otherwise.
- Planted cases: labels ``==`` the planted canonical labels at resolution 0.25, 0.5, 1, 2.
- Quality against networkx's Louvain on the same quantised graph at seeds 0-4, one helper for both:
  ``Q_ours >= min Q_nx - (max Q_nx - min Q_nx)``; where networkx is unanimous the margin is zero.
- Quantisation and refusals; the front ends with the device calls replaced by host twins."""

from __future__ import annotations

import inspect

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import squidpy_amd as sq
from squidpy_amd.gr import _niche_graph as G
from squidpy_amd.gr import _niche_leiden as L

from tests import niche_leiden_cases as LC
from tests import niche_leiden_oracle as LO
from tests import niche_neighbors_oracle as NO

PAIRS = [(name, r) for name in LC.CASES for r in LC.RESOLUTIONS]
PLANTED_PAIRS = [(name, r) for name in LC.PLANTED for r in LC.PLANTED_RESOLUTIONS]
NETWORKX_PAIRS = [(name, r) for name in LC.NETWORKX_CASES for r in (LC.PLANTED_RESOLUTIONS if name in LC.PLANTED else LC.RESOLUTIONS)]


@pytest.mark.parametrize("name,resolution", PAIRS)
def test_labels_are_canonical_and_communities_connected(name, resolution):
    indptr, indices, _ = LC.graph(name)
    labels, stats = LC.expected(name, resolution)
    assert labels.dtype == np.int32 and labels.shape == (indptr.shape[0] - 1,)
    LO.assert_canonical(labels)
    assert stats["n_communities"] == int(labels.max()) + 1
    LO.assert_connected(indptr, indices, labels)


@pytest.mark.parametrize("name,resolution", PAIRS)
def test_node_stability(name, resolution):
    indptr, indices, weights = LC.graph(name)
    labels, stats = LC.expected(name, resolution)
    if stats["cap_hits"] or not stats["settled"]:
        assert stats["iterations"] == LO.ITER_CAP or stats["cap_hits"] > 0  # the stats say why stability is not promised
        return
    assert LO.unstable_vertices(indptr, indices, weights, labels, resolution) == []


def test_lattice_reports_its_sweeps():
    """Ties everywhere: whether the lattice reaches a sweep without a move is reported, never hidden."""
    for resolution in LC.RESOLUTIONS:
        stats = LC.expected("lattice12", resolution)[1]
        assert stats["sweeps"] >= stats["levels"] >= stats["iterations"] >= 1
        assert 0 <= stats["cap_hits"] <= stats["levels"]


@pytest.mark.parametrize("name,resolution", PLANTED_PAIRS)
def test_planted_partitions_are_recovered(name, resolution):
    assert np.array_equal(LC.expected(name, resolution)[0], LC.planted(name))


@pytest.mark.parametrize("name,resolution", NETWORKX_PAIRS)
def test_quality_against_networkx_louvain(name, resolution):
    pytest.importorskip("networkx", reason="networkx is the yardstick of this test")
    graph = LC.graph(name)
    ours = LO.quality(*graph, LC.expected(name, resolution)[0], resolution)
    theirs = LO.louvain_qualities(*graph, resolution)
    print(f"{name} gamma={resolution}: ours {ours!r} networkx {theirs!r}")
    assert ours >= min(theirs) - (max(theirs) - min(theirs))


def test_tiny_inputs():
    assert LC.expected("n1", 1.0)[0].tolist() == [0]
    assert LC.expected("n5_empty", 1.0)[0].tolist() == [0, 1, 2, 3, 4]
    assert LC.expected("n2_edge", 1.0)[0].tolist() == [0, 0]
    assert LC.expected("disjoint_cliques", 1.0)[0].tolist() == [0] * 7 + [1] * 5 + [2] * 5 + [3] * 3 + [4, 5]


def test_stats_hold_the_exact_integers():
    indptr, indices, weights = LC.graph("knn_blobs6")
    labels, stats = LC.expected("knn_blobs6", 1.0)
    rows = np.repeat(np.arange(labels.shape[0]), np.diff(indptr))
    assert stats["two_m"] == int(weights.astype(np.int64).sum())
    assert stats["sum_in"] == int(weights.astype(np.int64)[labels[rows] == labels[indices]].sum())


# ---- quantisation and refusals ------------------------------------------------------------------------------------------------------------
def test_quantise_weights_matches_the_oracle_and_clamps():
    for name in ("knn_blobs8", "wide_weights", "ring_cliques"):
        q = sq.gr.quantise_weights(LC.matrix(name))
        indptr, indices, weights = LC.graph(name)
        assert q.dtype == np.int32 and np.array_equal(q.indptr, indptr) and np.array_equal(q.indices, indices)
        assert np.array_equal(q.data, weights)
    wide = LC.graph("wide_weights")[2]
    assert wide.min() == 1 and wide.max() == 2**24  # 2**-30 of the largest weight is clamped to 1


def test_quantise_weights_leaves_the_input_alone_and_canonicalises():
    a = sparse.coo_matrix(([0.5, 0.5, 0.25, 0.25, 0.25, 0.25, 0.0], ([0, 1, 2, 0, 0, 2, 1], [1, 0, 0, 2, 2, 0, 2])), shape=(3, 3))
    before = a.copy()
    q = sq.gr.quantise_weights(a)
    assert (a != before).nnz == 0
    assert q.has_canonical_format and q.toarray().tolist() == [[0, 2**24, 2**24], [2**24, 0, 0], [2**24, 0, 0]]


@pytest.mark.parametrize("bad", ["asymmetric_value", "asymmetric_structure", "negative", "nan", "self_loop", "not_square"])
def test_quantise_weights_refuses(bad):
    a = sparse.lil_matrix((4, 4))
    a[0, 1] = a[1, 0] = 1.0
    a[2, 3] = a[3, 2] = 0.5
    if bad == "asymmetric_value":
        a[3, 2] = 0.25
    elif bad == "asymmetric_structure":
        a[0, 3] = 1.0
    elif bad == "negative":
        a[0, 1] = a[1, 0] = -1.0
    elif bad == "nan":
        a[0, 1] = a[1, 0] = np.nan
    elif bad == "self_loop":
        a[2, 2] = 1.0
    else:
        a = a[:3]
    with pytest.raises(ValueError):
        sq.gr.quantise_weights(a.tocsr())


def test_oracle_refuses_what_the_device_refuses():
    indptr, indices, weights = (x.copy() for x in LC.graph("ring_cliques"))
    for damage in ("asymmetric", "self_loop", "unsorted", "weight"):
        i, j, w = indptr.copy(), indices.copy(), weights.copy()
        if damage == "asymmetric":
            w[0] += 1
        elif damage == "self_loop":
            j[0] = 0
        elif damage == "unsorted":
            j[[0, 1]] = j[[1, 0]]
        else:
            w[0] = 0
        with pytest.raises(ValueError):
            LO.leiden(i, j, w, 1.0)


@pytest.fixture()
def host_twin(monkeypatch):
    """The device calls of the front ends replaced by host restatements."""
    calls = []

    def leiden(ctx, indptr, indices, weights, resolution, n_iterations=-1):
        calls.append((resolution, n_iterations))
        return LO.leiden(indptr, indices, weights, resolution, n_iterations)

    def neighbors(data, n_neighbors=15, *, device=None):
        x = np.asarray(data, dtype=np.float64)
        idx, d2 = NO.knn(x, n_neighbors - 1)
        dist = np.sqrt(d2)
        vals = NO.fuzzy(dist, float(dist.sum() / (x.shape[0] * n_neighbors))).vals
        return G.NicheNeighborsResult(None, NO.connectivities(idx, vals), idx, dist, None, None)

    def profile(adata, groups, key="spatial_connectivities", distance=1, abs_nhood=False, n_hop_weights=None, *, table_key=None, device=None):
        onehot = pd.get_dummies(adata.obs[groups]).to_numpy(dtype=np.float64)
        p = adata.obsp[key] @ onehot
        return p / np.maximum(p.sum(1, keepdims=True), 1.0)

    def utag(adata, key="spatial_connectivities", n_comps=None, *, table_key=None, device=None):
        a = adata.obsp[key]
        f = sparse.diags(1.0 / np.maximum(np.asarray(a.sum(1)).ravel(), 1.0)) @ a @ adata.X
        f = f - f.mean(0)
        return f @ np.linalg.svd(f, full_matrices=False)[2][:8].T

    monkeypatch.setattr(L, "_leiden", leiden)
    monkeypatch.setattr(L, "default_context", lambda device=None: None)
    monkeypatch.setattr(L, "niche_neighbors", neighbors)
    monkeypatch.setattr(L.N, "niche_nhood_profile", profile)
    monkeypatch.setattr(L.N, "niche_utag_embedding", utag)
    return calls


@pytest.mark.parametrize("resolution", [0.0, -1.0, float("nan"), float("inf")])
def test_resolution_is_refused(host_twin, resolution):
    with pytest.raises(ValueError):
        sq.gr.niche_leiden(LC.matrix("ring_cliques"), resolution)
    with pytest.raises(ValueError):
        LO.leiden(*LC.graph("ring_cliques"), resolution)
    assert host_twin == []


def test_two_m_limit_is_not_implemented():
    L._check_two_m(2**62 - 1)
    with pytest.raises(NotImplementedError):
        L._check_two_m(2**62)


def test_niche_leiden_refuses_before_the_device(host_twin):
    bad = LC.matrix("ring_cliques").copy().tolil()
    bad[0, 1] = 0.5
    with pytest.raises(ValueError):
        sq.gr.niche_leiden(bad.tocsr())
    with pytest.raises(ValueError):
        sq.gr.niche_leiden(LC.matrix("ring_cliques"), n_iterations=0)
    with pytest.raises(KeyError):
        sq.gr.niche_leiden(LC.lattice_adata(6))
    assert host_twin == []


# ---- front ends ----------------------------------------------------------------------------------------------------------------------------
def test_niche_leiden_result_for_a_matrix(host_twin):
    res = sq.gr.niche_leiden(LC.matrix("two_level"), 0.5)
    labels, stats = LC.expected("two_level", 0.5)
    assert isinstance(res, sq.gr.LeidenResult) and np.array_equal(res.labels, labels)
    assert (res.n_communities, res.iterations, res.levels, res.sweeps) == (4, stats["iterations"], stats["levels"], stats["sweeps"])
    assert res.quality == LO.quality(*LC.graph("two_level"), labels, 0.5)
    assert host_twin == [(0.5, -1)]


def test_niche_leiden_slots_and_keys(host_twin):
    adata = LC.lattice_adata(6)
    conn = LC.matrix("ring_cliques")[:36][:, :36]
    adata.obsp["connectivities"] = conn
    adata.obsp["other_connectivities"] = LC.matrix("two_level")[:36][:, :36]
    adata.uns["neighbors"] = {"connectivities_key": "connectivities"}
    adata.uns["other"] = {"connectivities_key": "other_connectivities"}
    assert sq.gr.niche_leiden(adata) is None
    col = adata.obs["leiden"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(i) for i in range(len(col.cat.categories))]
    assert np.array_equal(col.astype(int).to_numpy(), sq.gr.niche_leiden(conn).labels)
    assert adata.uns["leiden"] == {"params": {"resolution": 1.0, "n_iterations": -1}}
    res = sq.gr.niche_leiden(adata, 0.5, neighbors_key="other", key_added="coarse", n_iterations=2, copy=True)
    assert "coarse" not in adata.obs and "coarse" not in adata.uns
    sq.gr.niche_leiden(adata, 0.5, neighbors_key="other", key_added="coarse", n_iterations=2)
    assert np.array_equal(adata.obs["coarse"].astype(int).to_numpy(), res.labels)
    assert np.array_equal(res.labels, sq.gr.niche_leiden(adata.obsp["other_connectivities"], 0.5, n_iterations=2).labels)
    assert adata.uns["coarse"] == {"params": {"resolution": 0.5, "n_iterations": 2}}
    assert host_twin[-1] == (0.5, 2)


def test_many_categories_are_in_numeric_order(host_twin):
    adata = LC.lattice_adata(6)
    adata.obsp["connectivities"] = sparse.csr_matrix((36, 36))
    adata.uns["neighbors"] = {"connectivities_key": "connectivities"}
    sq.gr.niche_leiden(adata)
    assert list(adata.obs["leiden"].cat.categories) == [str(i) for i in range(36)]  # "10" after "9", not after "1"


# gr/_niche.py:275-290 and :352-362 of the reference, typed in: (name, default); `device` is this library's keyword-only addition
_EMPTY = inspect.Parameter.empty
NEIGHBORHOOD_SIGNATURE = [
    ("data", _EMPTY), ("groups", _EMPTY), ("resolutions", _EMPTY), ("n_neighbors", 15), ("spatial_connectivities_key", "spatial_connectivities"),
    ("scale", True), ("distance", 1), ("abs_nhood", False), ("n_hop_weights", None), ("min_niche_size", None), ("mask", None),
    ("library_key", None), ("inplace", True), ("table_key", None),
]
UTAG_SIGNATURE = [
    ("data", _EMPTY), ("resolutions", _EMPTY), ("n_neighbors", 15), ("spatial_connectivities_key", "spatial_connectivities"),
    ("min_niche_size", None), ("mask", None), ("library_key", None), ("inplace", True), ("table_key", None),
]


@pytest.mark.parametrize("func,expected", [("calculate_niche_neighborhood", NEIGHBORHOOD_SIGNATURE), ("calculate_niche_utag", UTAG_SIGNATURE)])
def test_drop_in_signatures(func, expected):
    params = list(inspect.signature(getattr(sq.gr, func)).parameters.values())
    positional = [p for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.default) for p in positional] == expected
    rest = [p for p in params if p.kind is not inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.kind, p.default) for p in rest] == [("device", inspect.Parameter.KEYWORD_ONLY, None)]


def test_niche_leiden_signature():
    params = list(inspect.signature(sq.gr.niche_leiden).parameters.values())
    assert [(p.name, p.default) for p in params] == [("data", _EMPTY), ("resolution", 1.0), ("neighbors_key", None), ("key_added", "leiden"),
                                                     ("n_iterations", -1), ("copy", False), ("device", None)]
    assert [p.kind for p in params[2:]] == [inspect.Parameter.KEYWORD_ONLY] * 5


@pytest.mark.parametrize("flavour", ["neighborhood", "utag"])
def test_columns_for_a_float_and_a_list(host_twin, flavour):
    base = "nhood_niche" if flavour == "neighborhood" else "utag_niche"

    def run(adata, resolutions, **kw):
        if flavour == "neighborhood":
            return sq.gr.calculate_niche_neighborhood(adata, "cell_type", resolutions, **kw)
        return sq.gr.calculate_niche_utag(adata, resolutions, **kw)

    adata = LC.lattice_adata(12)
    before = set(adata.obs.columns)
    assert run(adata, 0.5) is None
    assert set(adata.obs.columns) - before == {f"{base}_res=0.5"}
    col = adata.obs[f"{base}_res=0.5"]
    assert all(isinstance(v, str) for v in col) and set(col) == {str(i) for i in range(col.nunique())}
    assert [r for r, _ in host_twin] == [0.5]

    adata = LC.lattice_adata(12)
    out = run(adata, [0.5, 1], inplace=False)
    assert set(adata.obs.columns) == before and set(out.obs.columns) - before == {f"{base}_res=0.5", f"{base}_res=1"}
    assert list(out.obs[f"{base}_res=0.5"]) == list(col)


def test_mask_min_size_and_library(host_twin):
    adata = LC.lattice_adata(12)
    plain = sq.gr.calculate_niche_neighborhood(adata, "cell_type", 1.0, inplace=False).obs["nhood_niche_res=1.0"]
    mask = pd.Series(np.arange(144) % 3 != 0, index=adata.obs.index)
    masked = sq.gr.calculate_niche_neighborhood(adata, "cell_type", 1.0, mask=mask, inplace=False).obs["nhood_niche_res=1.0"]
    assert (masked[~mask] == "not_a_niche").all() and (masked[mask] == plain[mask]).all()
    counts = plain.value_counts()
    limit = int(counts.iloc[0])  # only the largest niches survive
    sized = sq.gr.calculate_niche_neighborhood(adata, "cell_type", 1.0, min_niche_size=limit, inplace=False).obs["nhood_niche_res=1.0"]
    small = plain.isin(counts[counts < limit].index)
    assert (sized[small] == "not_a_niche").all() and (sized[~small] == plain[~small]).all()

    by_lib = sq.gr.calculate_niche_utag(adata, [1.0], library_key="library", inplace=False).obs["utag_niche_res=1.0"]
    for lib in ("A", "B"):
        rows = (adata.obs["library"] == lib).to_numpy()
        alone = sq.gr.calculate_niche_utag(adata[rows, :], [1.0], inplace=False).obs["utag_niche_res=1.0"]
        assert list(by_lib[rows]) == [f"lib={lib}_{v}" for v in alone]
    both = sq.gr.calculate_niche_utag(adata, 1.0, library_key="library", mask=mask, inplace=False).obs["utag_niche_res=1.0"]
    assert set(both[~mask]) == {"lib=A_not_a_niche", "lib=B_not_a_niche"}


def test_drop_ins_refuse_before_anything_runs(host_twin):
    adata = LC.lattice_adata(12)
    before = adata.obs.copy()
    with pytest.raises(KeyError):
        sq.gr.calculate_niche_neighborhood(adata, "missing", 1.0)
    with pytest.raises(ValueError):
        sq.gr.calculate_niche_neighborhood(adata, "cell_type", [1.0, -1.0])
    with pytest.raises(TypeError):
        sq.gr.calculate_niche_neighborhood(adata, "cell_type", 1.0, n_neighbors=2.5)
    with pytest.raises(KeyError):
        sq.gr.calculate_niche_utag(adata, 1.0, spatial_connectivities_key="missing")
    with pytest.raises(KeyError):
        sq.gr.calculate_niche_utag(adata, 1.0, library_key="missing")
    with pytest.raises(ValueError):
        sq.gr.calculate_niche_utag(adata, 1.0, n_neighbors=100, library_key="library")  # 72 rows per library
    assert host_twin == [] and adata.obs.equals(before)
