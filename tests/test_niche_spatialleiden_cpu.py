"""CPU: the numpy restatement of ``sqgr_leiden_multiplex`` (tests/niche_spatialleiden_oracle.py) pinned to what can be checked without
spatialleiden or leidenalg, and everything ``niche_spatialleiden`` and its drop-in do without a device.

- Every case x resolution pair x layer ratio: a valid canonical labelling; every community connected in the union of the layers; after
  ``n_iterations=-1`` no vertex has a strictly better neighbouring community under the multiplex objective in exact rational arithmetic
  — asserted wherever the stats report a settled run without a sweep-cap hit, and the stats must say so otherwise.
- Anchors, exact by the contract, on every case of tests/niche_leiden_cases.py whose single-layer run hits no sweep cap (asserted
  first): ``(G, empty)`` returns the single-layer labels and shared stats at any ratio (``x + r * 0.0`` is ``x``); ``(G, G)`` with equal
  resolutions and ratio 1 or 2**6 returns the single-layer labels (``x + 2**j * x`` orders as ``x`` does).
- ``ring_pair``: ratio 2**-6 recovers layer 0's planted cliques, ratio 2**6 layer 1's.
- The multiplex ``Q`` of the multiplex labels >= that of single-layer Leiden's labels on either layer alone, exact, zero margin.
- ``quantise_layers``; the front ends with the device call replaced by the restatement; the drop-in's signature against the
  reference's (tests/golden/spatialleiden_signature.json); refusals leave the object untouched."""

from __future__ import annotations

import inspect
import json
import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import squidpy_amd as sq
from squidpy_amd.gr import _niche_spatialleiden as S

from tests import niche_leiden_cases as LC
from tests import niche_leiden_oracle as LO
from tests import niche_spatialleiden_cases as MC
from tests import niche_spatialleiden_oracle as MO

SINGLE_PAIRS = [(name, r) for name in LC.CASES for r in LC.RESOLUTIONS]


@pytest.mark.parametrize("name,resolutions,ratio", MC.COMBOS)
def test_labels_are_canonical_and_communities_connected(name, resolutions, ratio):
    layers = MC.layers(name)
    labels, stats = MC.expected(name, resolutions, ratio)
    assert labels.dtype == np.int32 and labels.shape == (layers[0][0].shape[0] - 1,)
    LO.assert_canonical(labels)
    assert stats["n_communities"] == int(labels.max()) + 1 and tuple(stats) == MO.STATS
    MO.assert_connected_in_union(*layers, labels)
    rows = [np.repeat(np.arange(labels.shape[0]), np.diff(lay[0])) for lay in layers]
    for l, lay in enumerate(layers):  # the stats hold the exact integers
        w = lay[2].astype(np.int64)
        assert stats[f"two_m_{l}"] == int(w.sum()) and stats[f"sum_in_{l}"] == int(w[labels[rows[l]] == labels[lay[1]]].sum())


@pytest.mark.parametrize("name,resolutions,ratio", MC.COMBOS)
def test_node_stability(name, resolutions, ratio):
    labels, stats = MC.expected(name, resolutions, ratio)
    if stats["cap_hits"] or not stats["settled"]:
        assert stats["iterations"] == LO.ITER_CAP or stats["cap_hits"] > 0  # the stats say why stability is not promised
        return
    assert MO.unstable_vertices(*MC.layers(name), labels, resolutions, ratio) == []


def _assert_single_layer(name, resolution, labels, stats, layer):
    expected_labels, expected_stats = LC.expected(name, resolution)
    assert np.array_equal(labels, expected_labels)
    assert {k: stats[k] for k in MO.SHARED_STATS} == {k: expected_stats[k] for k in MO.SHARED_STATS}
    assert (stats[f"sum_in_{layer}"], stats[f"two_m_{layer}"]) == (expected_stats["sum_in"], expected_stats["two_m"])


@pytest.mark.parametrize("name,resolution", SINGLE_PAIRS)
def test_anchor_empty_second_layer(name, resolution):
    assert LC.expected(name, resolution)[1]["cap_hits"] == 0  # the anchor's condition
    graph = LC.graph(name)
    ratio = MC.RATIOS[SINGLE_PAIRS.index((name, resolution)) % len(MC.RATIOS)]  # any ratio: every one of them is used
    labels, stats = MO.leiden(graph, MC.empty_layer(graph[0].shape[0] - 1), (resolution, 1.0), ratio)
    _assert_single_layer(name, resolution, labels, stats, 0)
    assert (stats["sum_in_1"], stats["two_m_1"]) == (0, 0)


@pytest.mark.parametrize("ratio", [1.0, 2.0**6])
@pytest.mark.parametrize("name,resolution", SINGLE_PAIRS)
def test_anchor_same_graph_twice(name, resolution, ratio):
    assert LC.expected(name, resolution)[1]["cap_hits"] == 0  # the anchor's condition
    graph = LC.graph(name)
    labels, stats = MO.leiden(graph, graph, (resolution, resolution), ratio)
    _assert_single_layer(name, resolution, labels, stats, 0)
    _assert_single_layer(name, resolution, labels, stats, 1)


def test_anchor_empty_first_layer():
    graph = LC.graph("two_level")
    labels, stats = MO.leiden(MC.empty_layer(48), graph, (2.0, 0.5), 3.0)
    _assert_single_layer("two_level", 0.5, labels, stats, 1)


@pytest.mark.parametrize("resolutions", MC.RESOLUTIONS)
def test_ring_pair_recovers_the_heavier_layer(resolutions):
    assert np.array_equal(MC.expected("ring_pair", resolutions, 2.0**-6)[0], MC.planted("ring_pair", 0))
    assert np.array_equal(MC.expected("ring_pair", resolutions, 2.0**6)[0], MC.planted("ring_pair", 1))
    assert not np.array_equal(MC.planted("ring_pair", 0), MC.planted("ring_pair", 1))


@pytest.mark.parametrize("ratio", [1.0, 3.0])
@pytest.mark.parametrize("resolutions", MC.RESOLUTIONS)
@pytest.mark.parametrize("name", MC.QUALITY_CASES)
def test_quality_against_single_layer_leiden(name, resolutions, ratio):
    layers = MC.layers(name)
    ours = MO.multiplex_quality(*layers, MC.expected(name, resolutions, ratio)[0], resolutions, ratio)
    for l in range(2):
        alone = LO.leiden(*layers[l], resolutions[l])[0]
        theirs = MO.multiplex_quality(*layers, alone, resolutions, ratio)
        print(f"{name} gamma={resolutions} ratio={ratio}: multiplex {float(ours)!r} layer {l} alone {float(theirs)!r}")
        assert ours >= theirs


def test_tiny_inputs():
    assert MC.expected("n1", (1.0, 1.0), 1.0)[0].tolist() == [0]
    assert MC.expected("n5_empty", (1.0, 1.0), 1.0)[0].tolist() == [0, 1, 2, 3, 4]
    assert MC.expected("n2_edge", (1.0, 1.0), 1.0)[0].tolist() == [0, 0]
    assert np.diff(MC.layers("layer1_only")[0][0])[48:].tolist() == [0] * 12
    assert (MC.expected("layer1_only", (1.0, 1.0), 1.0)[0][48:] < 8).all()  # the vertices without a latent row are clustered


def test_capacity_split_straddles_the_boundary():
    l0, l1 = MC.layers("capacity_split")
    summed = np.diff(l0[0]) + np.diff(l1[0])
    assert summed[0] == LC.capacity() and summed[1] == LC.capacity() + 1
    assert min(np.diff(l0[0])[:2].min(), np.diff(l1[0])[:2].min()) >= LC.capacity() // 2  # the neighbours are split between the layers
    star = MC.layers("star_lattice")
    assert np.diff(star[1][0]).max() > LC.capacity() and np.diff(star[0][0]).max() <= 2


# ---- quantisation and refusals ------------------------------------------------------------------------------------------------------------
def test_quantise_layers_matches_the_oracle():
    for name in ("lattice900", "knn_blobs6_spatial", "ring_empty", "n5_empty"):
        got = sq.gr.quantise_layers(*MC.matrices(name))
        for q, (indptr, indices, weights) in zip(got, MC.layers(name)):
            assert q.dtype == np.int32 and q.has_canonical_format
            assert np.array_equal(q.indptr, indptr) and np.array_equal(q.indices, indices) and np.array_equal(q.data, weights)


def test_quantise_layers_common_scale_clamp_and_symmetrisation():
    latent = sparse.csr_matrix(([0.5, 0.5, 2.0**-30, 2.0**-30], ([0, 1, 1, 2], [1, 0, 2, 1])), shape=(3, 3))
    spatial = sparse.csr_matrix(([1.0, 1.0, 1.0], ([0, 1, 2], [1, 0, 0])), shape=(3, 3))  # 0 <-> 1 mutual, 2 -> 0 one way
    before = latent.copy(), spatial.copy()
    q0, q1 = sq.gr.quantise_layers(latent, spatial)
    assert (latent != before[0]).nnz == 0 and (spatial != before[1]).nnz == 0
    # W = A + A^T: latent 0-1 is 1.0, spatial 0-1 is 2.0 (the common w_max), spatial 0-2 is 1.0; 2**-29 of w_max is clamped to 1
    assert q0.toarray().tolist() == [[0, 2**23, 0], [2**23, 0, 1], [0, 1, 0]]
    assert q1.toarray().tolist() == [[0, 2**24, 2**23], [2**24, 0, 0], [2**23, 0, 0]]
    # use_weights as a pair: the latent layer becomes unit weights, 1 + 1 = 2 = w_max
    u0, u1 = sq.gr.quantise_layers(latent, spatial, (False, True))
    assert u0.toarray().tolist() == [[0, 2**24, 0], [2**24, 0, 2**24], [0, 2**24, 0]] and (u1 != q1).nnz == 0
    b0, b1 = sq.gr.quantise_layers(latent, spatial, False)
    assert (b0 != u0).nnz == 0 and b1.toarray().tolist() == [[0, 2**24, 2**23], [2**24, 0, 0], [2**23, 0, 0]]
    e0, e1 = sq.gr.quantise_layers(sparse.csr_matrix((3, 3)), spatial)
    assert e0.nnz == 0 and e0.shape == (3, 3) and (e1 != q1).nnz == 0


@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("bad", ["negative", "nan", "inf", "self_loop", "not_square", "shape_mismatch"])
def test_quantise_layers_refuses(bad, layer):
    a = sparse.lil_matrix((4, 4))
    a[0, 1] = a[1, 0] = 1.0
    a[2, 3] = 0.5
    good = a.tocsr()
    if bad == "negative":
        a[0, 1] = -1.0
    elif bad == "nan":
        a[0, 1] = np.nan
    elif bad == "inf":
        a[0, 1] = np.inf
    elif bad == "self_loop":
        a[2, 2] = 1.0
    elif bad == "not_square":
        a = a[:3]
    else:
        a = a[:3][:, :3]
    pair = (a.tocsr(), good) if layer == 0 else (good, a.tocsr())
    with pytest.raises(ValueError):
        sq.gr.quantise_layers(*pair)
    with pytest.raises(TypeError):
        sq.gr.quantise_layers(good, good, use_weights=1)


def test_oracle_refuses_what_the_device_refuses():
    good = LC.graph("ring_cliques")
    for layer in (0, 1):
        for damage in ("asymmetric", "self_loop", "unsorted", "weight"):
            i, j, w = (x.copy() for x in good)
            if damage == "asymmetric":
                w[0] += 1
            elif damage == "self_loop":
                j[0] = 0
            elif damage == "unsorted":
                j[[0, 1]] = j[[1, 0]]
            else:
                w[0] = 0
            with pytest.raises(ValueError, match=f"layer {layer}"):
                MO.leiden(*(((i, j, w), good) if layer == 0 else (good, (i, j, w))))
    for kw in ({"resolutions": (0.0, 1.0)}, {"resolutions": (1.0, float("nan"))}, {"layer_ratio": 0.0}, {"layer_ratio": float("inf")}, {"n_iterations": 0}):
        with pytest.raises(ValueError):
            MO.leiden(good, good, **kw)


# ---- front ends ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def host_twin(monkeypatch):
    """The device call of the front ends replaced by the restatement."""
    calls = []

    def leiden_multiplex(ctx, layer0, layer1, resolutions=(1.0, 1.0), layer_ratio=1.0, n_iterations=-1):
        calls.append((tuple(resolutions), layer_ratio, n_iterations))
        return MO.leiden(layer0, layer1, resolutions, layer_ratio, n_iterations)

    monkeypatch.setattr(S, "_leiden_multiplex", leiden_multiplex)
    monkeypatch.setattr(S, "default_context", lambda device=None: None)
    return calls


def two_layer_adata(side: int = 12):
    adata = LC.lattice_adata(side)
    adata.obsp["connectivities"] = MC._knn_of(np.asarray(adata.X))
    return adata


def test_niche_spatialleiden_result_for_a_pair(host_twin):
    res = sq.gr.niche_spatialleiden(MC.matrices("lattice900"), (0.5, 2.0), layer_ratio=3.0)
    labels, stats = MC.expected("lattice900", (0.5, 2.0), 3.0)
    assert isinstance(res, sq.gr.MultiplexLeidenResult) and np.array_equal(res.labels, labels)
    assert (res.n_communities, res.iterations, res.levels, res.sweeps) == (stats["n_communities"], stats["iterations"], stats["levels"], stats["sweeps"])
    assert res.sum_in == (stats["sum_in_0"], stats["sum_in_1"]) and res.two_m == (stats["two_m_0"], stats["two_m_1"])
    assert res.quality == float(MO.multiplex_quality(*MC.layers("lattice900"), labels, (0.5, 2.0), 3.0))
    assert host_twin == [((0.5, 2.0), 3.0, -1)]


def test_niche_spatialleiden_slots_and_keys(host_twin):
    adata = two_layer_adata()
    adata.obsp["other"] = adata.obsp["spatial_connectivities"][::-1][:, ::-1].tocsr()
    assert sq.gr.niche_spatialleiden(adata) is None
    col = adata.obs["spatialleiden"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(i) for i in range(len(col.cat.categories))]
    pair = sq.gr.niche_spatialleiden((adata.obsp["connectivities"], adata.obsp["spatial_connectivities"]))
    assert np.array_equal(col.astype(int).to_numpy(), pair.labels)
    assert adata.uns["spatialleiden"] == {"params": {"resolution": (1.0, 1.0), "layer_ratio": 1.0, "use_weights": (True, True), "n_iterations": -1}}
    kw = dict(spatial_connectivities_key="other", layer_ratio=0.5, use_weights=(True, False), n_iterations=2, key_added="coarse")
    res = sq.gr.niche_spatialleiden(adata, 0.5, copy=True, **kw)
    assert "coarse" not in adata.obs and "coarse" not in adata.uns
    sq.gr.niche_spatialleiden(adata, 0.5, **kw)
    assert np.array_equal(adata.obs["coarse"].astype(int).to_numpy(), res.labels)
    direct = sq.gr.niche_spatialleiden((adata.obsp["connectivities"], adata.obsp["other"]), (0.5, 0.5), layer_ratio=0.5, use_weights=(True, False),
                                       n_iterations=2)
    assert np.array_equal(res.labels, direct.labels)
    assert host_twin[-1] == ((0.5, 0.5), 0.5, 2)


def test_niche_spatialleiden_refuses_before_the_device(host_twin):
    adata = two_layer_adata()
    before = adata.obs.copy()
    latent, spatial = adata.obsp["connectivities"], adata.obsp["spatial_connectivities"]
    bad = spatial.copy().tolil()
    bad[0, 0] = 1.0
    for args, kw, exc in [((adata,), {"latent_connectivities_key": "missing"}, KeyError), ((adata,), {"spatial_connectivities_key": "missing"}, KeyError),
                          ((adata, 0.0), {}, ValueError), ((adata, (1.0, float("nan"))), {}, ValueError), ((adata, (1.0, 1.0, 1.0)), {}, ValueError),
                          ((adata, "1"), {}, TypeError), ((adata,), {"layer_ratio": 0.0}, ValueError), ((adata,), {"layer_ratio": "1"}, TypeError),
                          ((adata,), {"use_weights": 1}, TypeError), ((adata,), {"n_iterations": 0}, ValueError),
                          (((latent, bad.tocsr()),), {}, ValueError), (((latent, spatial[:100][:, :100]),), {}, ValueError),
                          (((latent,),), {}, ValueError)]:
        with pytest.raises(exc):
            sq.gr.niche_spatialleiden(*args, **kw)
    assert host_twin == [] and adata.obs.equals(before) and "spatialleiden" not in adata.uns


def test_signatures():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatialleiden_signature.json")) as fh:
        ref = json.load(fh)
    assert ref["function"] == "calculate_niche_spatialleiden" and ref["keyword_only"] == []
    params = list(inspect.signature(sq.gr.calculate_niche_spatialleiden).parameters.values())
    positional = [p for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    ours = [{"name": p.name, "default": None if p.default is inspect.Parameter.empty else repr(p.default)} for p in positional]
    assert ours == [{"name": p["name"], "default": None if p["default"] is None else repr(eval(p["default"]))} for p in ref["positional"]]
    rest = [p for p in params if p.kind is not inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.kind, p.default) for p in rest] == [("device", inspect.Parameter.KEYWORD_ONLY, None)]

    params = list(inspect.signature(sq.gr.niche_spatialleiden).parameters.values())
    empty = inspect.Parameter.empty
    assert [(p.name, p.default) for p in params] == [
        ("data", empty), ("resolution", 1.0), ("latent_connectivities_key", "connectivities"), ("spatial_connectivities_key", "spatial_connectivities"),
        ("layer_ratio", 1.0), ("use_weights", True), ("n_iterations", -1), ("key_added", "spatialleiden"), ("copy", False), ("device", None)]
    assert [p.kind for p in params[2:]] == [inspect.Parameter.KEYWORD_ONLY] * 8


def test_columns_for_a_float_a_tuple_and_a_list(host_twin):
    adata = two_layer_adata()
    before = set(adata.obs.columns)
    assert sq.gr.calculate_niche_spatialleiden(adata, 0.5) is None
    assert set(adata.obs.columns) - before == {"spatialleiden_res=0.5"}
    col = adata.obs["spatialleiden_res=0.5"]
    assert all(isinstance(v, str) for v in col) and set(col) == {str(i) for i in range(col.nunique())}
    assert list(col) == list(sq.gr.niche_spatialleiden(adata, 0.5, copy=True).labels.astype(str))

    adata = two_layer_adata()
    out = sq.gr.calculate_niche_spatialleiden(adata, [0.5, (1.0, 0.5), 1], layer_ratio=2.0, n_iterations=2, use_weights=(True, False), inplace=False)
    assert set(adata.obs.columns) == before
    assert set(out.obs.columns) - before == {"spatialleiden_res=0.5", "spatialleiden_res=(1.0, 0.5)", "spatialleiden_res=1"}
    expected = sq.gr.niche_spatialleiden(adata, (1.0, 0.5), layer_ratio=2.0, n_iterations=2, use_weights=(True, False), copy=True)
    assert list(out.obs["spatialleiden_res=(1.0, 0.5)"]) == list(expected.labels.astype(str))
    assert [c[:2] for c in host_twin[-4:-1]] == [((0.5, 0.5), 2.0), ((1.0, 0.5), 2.0), ((1.0, 1.0), 2.0)]

    out = sq.gr.calculate_niche_spatialleiden(two_layer_adata(), (1.0, 0.5), inplace=False)  # a tuple is one resolution, not a list
    assert set(out.obs.columns) - before == {"spatialleiden_res=(1.0, 0.5)"}


def test_mask_min_size_prefix_and_library(host_twin):
    adata = two_layer_adata()
    key = "spatialleiden_res=1.0"
    plain = sq.gr.calculate_niche_spatialleiden(adata, 1.0, inplace=False).obs[key]
    mask = pd.Series(np.arange(144) % 3 != 0, index=adata.obs.index)
    masked = sq.gr.calculate_niche_spatialleiden(adata, 1.0, mask=mask, inplace=False).obs[key]
    assert (masked[~mask] == "not_a_niche").all() and (masked[mask] == plain[mask]).all()
    counts = plain.value_counts()
    limit = int(counts.iloc[0])  # only the largest niches survive
    sized = sq.gr.calculate_niche_spatialleiden(adata, 1.0, min_niche_size=limit, inplace=False).obs[key]
    small = plain.isin(counts[counts < limit].index)
    assert (sized[small] == "not_a_niche").all() and (sized[~small] == plain[~small]).all()
    prefixed = sq.gr.calculate_niche_spatialleiden(adata, 1.0, mask=mask, prefix="s1_", inplace=False).obs[key]
    assert list(prefixed) == ["s1_" + v for v in masked]

    by_lib = sq.gr.calculate_niche_spatialleiden(adata, [1.0], prefix="ignored_", library_key="library", inplace=False).obs[key]
    for lib in ("A", "B"):
        rows = (adata.obs["library"] == lib).to_numpy()
        alone = sq.gr.calculate_niche_spatialleiden(adata[rows, :], [1.0], inplace=False).obs[key]
        assert list(by_lib[rows]) == [f"lib={lib}_{v}" for v in alone]
    both = sq.gr.calculate_niche_spatialleiden(adata, 1.0, library_key="library", mask=mask, inplace=False).obs[key]
    assert set(both[~mask]) == {"lib=A_not_a_niche", "lib=B_not_a_niche"}
    assert key not in adata.obs  # inplace=False left the input untouched


def test_drop_in_refuses_before_anything_runs(host_twin):
    adata = two_layer_adata()
    before = adata.obs.copy()
    bad = adata.obsp["spatial_connectivities"].copy().tolil()
    bad[0, 1] = -1.0
    adata.obsp["negative"] = bad.tocsr()
    for args, kw, exc in [((1.0,), {"latent_connectivities_key": "missing"}, KeyError), ((1.0,), {"spatial_connectivities_key": "negative"}, ValueError),
                          (([1.0, -1.0],), {}, ValueError), (([],), {}, ValueError), (([1.0, (1.0, 2.0, 3.0)],), {}, ValueError),
                          ((1.0,), {"layer_ratio": -1.0}, ValueError), ((1.0,), {"n_iterations": 2.5}, TypeError), ((1.0,), {"use_weights": "yes"}, TypeError),
                          ((1.0,), {"random_state": 1.5}, TypeError), ((1.0,), {"random_state": None}, TypeError), ((1.0,), {"prefix": 3}, TypeError),
                          ((1.0,), {"library_key": "missing"}, KeyError)]:
        with pytest.raises(exc):
            sq.gr.calculate_niche_spatialleiden(adata, *args, **kw)
    assert host_twin == [] and adata.obs.equals(before)
    sq.gr.calculate_niche_spatialleiden(adata, 1.0, random_state=7)  # an int is accepted and has no effect
    assert list(adata.obs["spatialleiden_res=1.0"]) == list(sq.gr.niche_spatialleiden(adata, copy=True).labels.astype(str))
