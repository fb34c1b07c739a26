"""CPU: the numpy restatement of the niche feature kernels (tests/niche_features_oracle.py) against the reference's literal code
(tests/golden/niche_features_reference.npz, written by tests/golden/make_niche_features_golden.py), and the host side of the three
front ends — validation and refusals — without a device.

Integers (shell structure, visit counts, profiles of unit-weight graphs) must be equal.  Every float result must lie within a bound
derived from the test's own inputs (``niche_features_oracle.sum_bound`` / ``variance_bound``): the reference sums the same rounded
products, possibly in another order."""

from __future__ import annotations

import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

from squidpy_amd import gr
from squidpy_amd._anndata_lite import AnnDataLite
from squidpy_amd.gr import _niche

from tests import niche_features_cases as FC
from tests import niche_features_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niche_features_reference.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


graph_of, setting_tag = FC.stored_graph, FC.setting_tag


def test_the_case_generators_reproduce_the_stored_inputs(ref):
    graphs = FC.golden_graphs()
    assert list(ref["graphs"]) == list(graphs)
    for name, a in graphs.items():
        b = graph_of(ref, name)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data), name
        n = a.shape[0]
        assert np.array_equal(FC.expression(n, FC.N_VARS, 100 + n).toarray(), ref[f"in/{name}/x"])
        assert np.array_equal(FC.label_codes(n, 200 + n), ref[f"in/{name}/codes"])
        assert n <= 400 and FC.N_VARS <= 9
    assert (graphs["weighted"].data != 1).any() and (graph_of(ref, "knn_loops").diagonal() == 1).all()
    assert (np.diff(graphs["isolated"].indptr) == 0).sum() >= 14


@pytest.mark.parametrize("name", FC.UNIT_GRAPHS)
def test_shells_equal_the_literal_hop_recurrence(ref, name):
    for k, (hop, vis) in enumerate(O.shells(graph_of(ref, name), 3), start=1):
        assert np.array_equal(hop.indptr, ref[f"shell/{name}/{k}/hop_indptr"]), (name, k)
        assert np.array_equal(hop.indices, ref[f"shell/{name}/{k}/hop_indices"]), (name, k)
        assert np.array_equal(vis.indptr, ref[f"shell/{name}/{k}/vis_indptr"]), (name, k)
        assert np.array_equal(vis.indices, ref[f"shell/{name}/{k}/vis_indices"]), (name, k)
        assert np.array_equal(vis.data, ref[f"shell/{name}/{k}/vis_counts"]), (name, k)


def test_shells_are_not_a_breadth_first_search(ref):
    """On a hexagonal lattice two paths of length 2 lead from a spot to each of its neighbours (through their two common
    neighbours), more than its one visit: every 1-hop neighbour of an interior spot is in shell 2 again."""
    a = graph_of(ref, "hex")
    (hop1, _), (hop2, _) = O.shells(a, 2)
    interior = np.flatnonzero(np.diff(a.indptr) == 6)
    assert len(interior) > 50
    again = hop1.multiply(hop2).tocsr()
    assert (np.diff(again.indptr)[interior] == 6).all()
    assert (hop2.diagonal()[interior] == 1).all()  # six paths lead back to the spot itself, visited once


def test_path_count_limit_is_refused(ref):
    with pytest.raises(OverflowError):
        O.shells(graph_of(ref, "hex"), 2, limit=2)
    O.shells(graph_of(ref, "hex"), 1, limit=2)


@pytest.mark.parametrize("aggregation", ["mean", "variance"])
@pytest.mark.parametrize("name", FC.UNIT_GRAPHS)
def test_cellcharter_features_within_the_derived_bound(ref, name, aggregation):
    a, x = graph_of(ref, name), ref[f"in/{name}/x"]
    nv = x.shape[1]
    shells = O.shells(a, 3)
    got = O.cellcharter(a, sparse.csr_matrix(x), 3, aggregation)
    want = ref[f"cc/{name}/{aggregation}/csr/3"]
    assert got.shape == want.shape == (a.shape[0], 4 * nv) and got.flags.c_contiguous
    assert np.array_equal(got[:, :nv], x) and np.array_equal(want[:, :nv], x)
    for k in (1, 2, 3):
        bound = O.shell_bound(shells[k - 1][0], x, aggregation)
        err = np.abs(got[:, k * nv : (k + 1) * nv] - want[:, k * nv : (k + 1) * nv])
        print(name, aggregation, k, "max |error|", err.max(), "max bound", bound.max())
        assert (err <= bound).all(), (name, aggregation, k)
        if name in FC.AGGREGATE_GRAPHS:
            assert (np.abs(got[:, k * nv : (k + 1) * nv] - ref[f"agg/{name}/{aggregation}/{k}"]) <= bound).all()
    assert not bool(ref[f"cc_dense_ok/{name}/{aggregation}"])  # the literal source refuses a dense X here; the product takes one


def test_cellcharter_features_of_a_smaller_distance_are_a_prefix(ref):
    a, x = graph_of(ref, "knn"), ref["in/knn/x"]
    for distance in (1, 2):
        want = ref[f"cc/knn/mean/csr/{distance}"]
        assert np.array_equal(want, ref["cc/knn/mean/csr/3"][:, : want.shape[1]])
        assert O.cellcharter(a, x, distance, "mean").shape == want.shape


@pytest.mark.parametrize("name", list(FC.UNIT_GRAPHS) + ["weighted"])
def test_utag_features_within_the_derived_bound(ref, name):
    a, x = graph_of(ref, name), ref[f"in/{name}/x"]
    got = O.utag(a, x)
    bound = O.sum_bound(a.indptr, a.indices, O.utag_coefficients(a), x)
    for kind in ("csr", "dense"):
        err = np.abs(got - ref[f"utag/{name}/{kind}"])
        print(name, kind, "max |error|", err.max(), "max bound", bound.max())
        assert (err <= bound).all(), (name, kind)
    assert (got[np.diff(a.indptr) == 0] == 0).all()


def profile_inputs(ref, name, labels):
    return FC.profile_inputs(ref[f"in/{name}/codes"], labels)


@pytest.mark.parametrize("labels", ["categorical", "plain"])
@pytest.mark.parametrize("name", FC.UNIT_GRAPHS)
def test_profiles_of_unit_weight_graphs_equal_the_reference(ref, name, labels):
    a = graph_of(ref, name)
    codes, n_categories = profile_inputs(ref, name, labels)
    raw = O.label_hops(a, codes, n_categories, 3, normalise=False)
    assert (raw == np.round(raw)).all() and raw.sum(axis=2).max() < 2**24  # every sum is an integer that float32 and float64 hold exactly
    for distance, abs_nhood, weights in FC.PROFILE_SETTINGS:
        given = None if weights is None else list(weights)
        got = O.nhood_profile(a, codes, n_categories, distance, abs_nhood, given)
        want = ref[f"profile/{name}/{labels}/{setting_tag(distance, abs_nhood, weights)}"]
        assert got.shape == want.shape == (a.shape[0], n_categories)
        assert np.array_equal(got, want), (name, labels, distance, abs_nhood, weights)
        assert given == (None if weights is None else list(weights))
    if labels == "categorical":
        assert (ref[f"profile/{name}/categorical/d3_rel_none"][:, FC.CATEGORIES.index("empty")] == 0).all()


def test_profiles_of_a_weighted_graph_within_the_relative_bound(ref):
    """Non-negative weights: the relative bound of ``niche_features_oracle.profile_relative_bound`` (its reasoning is written there)."""
    a = graph_of(ref, "weighted")
    assert (a.data > 0).all()
    for labels in ("categorical", "plain"):
        codes, n_categories = profile_inputs(ref, "weighted", labels)
        for distance, abs_nhood, weights in FC.PROFILE_SETTINGS:
            got = O.nhood_profile(a, codes, n_categories, distance, abs_nhood, None if weights is None else list(weights))
            want = ref[f"profile/weighted/{labels}/{setting_tag(distance, abs_nhood, weights)}"]
            rel = O.profile_relative_bound(a, distance, abs_nhood, n_categories)
            err = np.abs(got - want)
            print(labels, distance, abs_nhood, weights, "max relative error", (err / np.where(want != 0, np.abs(want), 1)).max(), "bound", rel)
            assert (err <= rel * np.abs(want)).all(), (labels, distance, abs_nhood, weights)


# ---- the host side of the front ends: no device -------------------------------------------------------------------------------------
class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*_a, **_k):
        raise _DeviceTouched()

    monkeypatch.setattr(_niche, "default_context", refuse)


def table(ref, name="knn", x=None, column=None):
    a = graph_of(ref, name)
    codes = ref[f"in/{name}/codes"]
    obs = pd.DataFrame({"cell_type": FC.categorical(codes) if column is None else column}, index=[f"c{i}" for i in range(a.shape[0])])
    return AnnDataLite(X=ref[f"in/{name}/x"] if x is None else x, obs=obs, obsp={"spatial_connectivities": a})


def test_front_ends_are_exported():
    for name in ("niche_nhood_profile", "niche_utag_features", "niche_cellcharter_features"):
        assert callable(getattr(gr, name)) and name in gr.__all__


def test_refusals_come_before_the_device(ref, no_device):
    adata = table(ref)
    with pytest.raises(KeyError):
        gr.niche_nhood_profile(adata, "nope")
    with pytest.raises(KeyError):
        gr.niche_utag_features(adata, "other_connectivities")
    with pytest.raises(KeyError):
        gr.niche_cellcharter_features(adata, spatial_connectivities_key="other_connectivities")
    for bad in (0, -1):
        with pytest.raises(ValueError, match="'distance' must be at least 1"):
            gr.niche_cellcharter_features(adata, distance=bad)
        with pytest.raises(ValueError, match="'distance' must be at least 1"):
            gr.niche_nhood_profile(adata, "cell_type", distance=bad)
    with pytest.raises(TypeError):
        gr.niche_cellcharter_features(adata, distance=2.0)
    with pytest.raises(NotImplementedError):
        gr.niche_cellcharter_features(adata, distance=65)
    with pytest.raises(ValueError, match="Invalid aggregation method 'median'. Please choose either 'mean' or 'variance'."):
        gr.niche_cellcharter_features(adata, aggregation="median")
    with pytest.raises(NotImplementedError, match="stored values are all 1"):
        gr.niche_cellcharter_features(table(ref, "weighted"))
    with pytest.raises(TypeError):
        gr.niche_nhood_profile(adata, "cell_type", distance=2, n_hop_weights=(1.0, 0.5))
    with pytest.raises(ValueError):
        gr.niche_nhood_profile(adata, "cell_type", distance=2, n_hop_weights=[1.0, float("nan")])
    with pytest.raises(ValueError):
        gr.niche_nhood_profile(adata, "cell_type", distance=2, n_hop_weights=[])
    bad_x = ref["in/knn/x"].copy()
    bad_x[3, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        gr.niche_utag_features(table(ref, x=bad_x))
    with pytest.raises(ValueError):
        gr.niche_utag_features(table(ref, x=ref["in/knn/x"][:-1]))
    with pytest.raises(TypeError, match="table_key"):
        gr.niche_utag_features(type("SData", (), {"tables": {"t": adata}})())
    # valid requests get as far as the device, and only then
    for call in (lambda: gr.niche_nhood_profile(adata, "cell_type", distance=3, n_hop_weights=[-1.0, 0.0]),
                 lambda: gr.niche_utag_features(adata), lambda: gr.niche_cellcharter_features(adata, aggregation="variance"),
                 lambda: gr.niche_utag_features(type("SData", (), {"tables": {"t": adata}})(), table_key="t")):
        with pytest.raises(_DeviceTouched):
            call()


def test_use_rep_none_keeps_raising_its_message(ref):
    with pytest.raises(NotImplementedError, match="needs `use_rep` here"):
        gr.calculate_niche_cellcharter(table(ref), use_rep=None)


def test_a_plain_column_is_converted_with_the_reference_warning_and_left_alone(ref, no_device):
    plain = FC.plain_labels(ref["in/knn/codes"])
    adata = table(ref, column=plain)
    with pytest.warns(UserWarning, match="Since adata.obs\\[groups\\] does not already have categorical dtype"), pytest.raises(_DeviceTouched):
        gr.niche_nhood_profile(adata, "cell_type")
    assert adata.obs["cell_type"].dtype == object and list(adata.obs.columns) == ["cell_type"]


def test_hop_weights_follow_the_literal_source():
    given = [2.0, 0.25]
    assert _niche.hop_weights(given, 3) == [2.0, 0.25, 0.25] and given == [2.0, 0.25]  # extended with the last value, never mutated
    assert _niche.hop_weights(None, 3) == [1.0, 1.0, 1.0]
    assert _niche.hop_weights([1.0, 2.0, 3.0, 4.0], 2) == [1.0, 2.0, 3.0, 4.0]  # kept whole: sum(weights) counts the surplus
    assert _niche.hop_weights([5.0], 1) is None
    rng = np.random.default_rng(5)
    hops = rng.random((3, 40, 4))
    for abs_nhood in (False, True):
        for weights in ([2.0, 0.25, 0.25], [1.0, 2.0, 3.0, 4.0], [-1.0, 0.0, 0.5]):
            want = weights[0] * hops[0]
            for h in (1, 2):
                want += weights[h] * hops[h]
            want = want if abs_nhood else want / sum(weights)
            got = _niche.combine_hop_profiles(hops, weights, abs_nhood)
            assert np.array_equal(got, want) and got.flags.c_contiguous
    assert np.array_equal(_niche.combine_hop_profiles(hops[:1], None, False), hops[0])


def test_the_hub_graph_straddles_a_capacity_of_512():
    """The planted rows of the GPU test's hub graph: one expansion exactly at the capacity, one just above, one far above."""
    a, nodes = FC.hub_graph(512)
    lens = np.diff(a.indptr)
    hop1 = O.shells(a, 1)[0][0]
    expansion = np.asarray(hop1 @ lens.reshape(-1, 1)).ravel()
    assert expansion[nodes["at"]] == 512 and expansion[nodes["above"]] == 544 and expansion[nodes["hub"]] > 4000
    assert a.has_canonical_format and (a.data == 1).all()
