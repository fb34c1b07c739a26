"""GPU: ``sq.gr.niche_nhood_profile`` / ``niche_utag_features`` / ``niche_cellcharter_features`` and the entry points of
``csrc/sqgr_niche.hip`` behind them.

On the golden cases (tests/golden/niche_features_reference.npz) every device result ``==`` the numpy restatement
(tests/niche_features_oracle.py) bit for bit, and lies within the derived bounds of the reference's literal result (integers: equal).
On larger generated inputs — a 20 000-spot hex lattice, a directed kNN-6 graph of 20 000 points, and a hub graph built from the
exported on-chip capacity so that one row sits exactly at it and others take the global-memory path; ``n_vars`` 1, 7, 65; 2 and 30
categories; distance 3 — the device ``==`` the restatement.  A path count at a lowered limit is refused, two identical calls return
the same bytes, nothing is written into ``adata``, and the CellCharter features feed ``gmm_fit`` end to end."""

from __future__ import annotations

import functools
import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import squidpy_amd as sq
from squidpy_amd import AnnDataLite, _lib
from squidpy_amd._lib import Graph, HopShells, SqgrError, default_context
from squidpy_amd.gr import _niche

from tests import niche_features_cases as FC
from tests import niche_features_oracle as O

pytestmark = pytest.mark.gpu

REF = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niche_features_reference.npz"))
KEY = "spatial_connectivities"


def adata_of(a, x=None, codes=None, column=None) -> AnnDataLite:
    n = a.shape[0]
    if column is None:
        column = FC.categorical(codes) if codes is not None else pd.Categorical(np.zeros(n, dtype=int))
    return AnnDataLite(X=x, obs=pd.DataFrame({"cell_type": column}, index=[f"c{i}" for i in range(n)]), obsp={KEY: a})


def assert_same_csr(got, want, what):
    assert np.array_equal(got.indptr, want.indptr), what
    assert np.array_equal(got.indices, want.indices), what
    assert np.array_equal(got.data, want.data), what


def assert_bytes_equal(got: np.ndarray, want: np.ndarray, what) -> None:
    assert got.dtype == np.float64 and got.flags.c_contiguous and got.shape == want.shape, what
    same = got.view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)
    assert same.all(), (what, int((~same).sum()), "elements differ; largest difference", float(np.abs(got - want).max()))


@functools.lru_cache(maxsize=None)
def oracle_shells(name: str):
    return O.shells(FC.stored_graph(REF, name), 3)


# ---- golden cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.UNIT_GRAPHS)
def test_golden_shells_equal_restatement_and_reference(name):
    a = FC.stored_graph(REF, name)
    got = _niche.hop_shells(a, 3)
    for k, ((hop, vis), (ohop, ovis)) in enumerate(zip(got, oracle_shells(name)), start=1):
        assert_same_csr(hop, ohop, (name, k, "hop"))
        assert_same_csr(vis, ovis, (name, k, "vis"))
        assert np.array_equal(hop.indices, REF[f"shell/{name}/{k}/hop_indices"]) and np.array_equal(vis.data, REF[f"shell/{name}/{k}/vis_counts"])


@pytest.mark.parametrize("aggregation", ["mean", "variance"])
@pytest.mark.parametrize("name", FC.UNIT_GRAPHS)
def test_golden_cellcharter_features(name, aggregation):
    a, x = FC.stored_graph(REF, name), REF[f"in/{name}/x"]
    nv = x.shape[1]
    want = O.cellcharter(a, x, 3, aggregation)
    ref = REF[f"cc/{name}/{aggregation}/csr/3"]
    for kind, xin in (("csr", sparse.csr_matrix(x)), ("csc", sparse.csc_matrix(x)), ("dense", x)):
        got = sq.gr.niche_cellcharter_features(adata_of(a, xin), 3, aggregation)
        assert_bytes_equal(got, want, (name, aggregation, kind))
    for k in (1, 2, 3):
        bound = O.shell_bound(oracle_shells(name)[k - 1][0], x, aggregation)
        assert (np.abs(got[:, k * nv : (k + 1) * nv] - ref[:, k * nv : (k + 1) * nv]) <= bound).all(), (name, aggregation, k)
    assert np.array_equal(got[:, :nv], ref[:, :nv])
    if name == "knn" and aggregation == "mean":
        for distance in (1, 2):
            assert_bytes_equal(sq.gr.niche_cellcharter_features(adata_of(a, x), distance), want[:, : (distance + 1) * nv], distance)


@pytest.mark.parametrize("name", list(FC.UNIT_GRAPHS) + ["weighted"])
def test_golden_utag_features(name):
    a, x = FC.stored_graph(REF, name), REF[f"in/{name}/x"]
    want = O.utag(a, x)
    bound = O.sum_bound(a.indptr, a.indices, O.utag_coefficients(a), x)
    for kind, xin in (("csr", sparse.csr_matrix(x)), ("dense", x)):
        got = sq.gr.niche_utag_features(adata_of(a, xin))
        assert_bytes_equal(got, want, (name, kind))
        assert (np.abs(got - REF[f"utag/{name}/{kind}"]) <= bound).all(), (name, kind)
    got32 = sq.gr.niche_utag_features(adata_of(a.astype(np.float32), x.astype(np.float32)))  # widened exactly
    assert_bytes_equal(got32, O.utag(a.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64)), (name, "float32"))


@pytest.mark.parametrize("labels", ["categorical", "plain"])
@pytest.mark.parametrize("name", list(FC.UNIT_GRAPHS) + ["weighted"])
def test_golden_nhood_profiles(name, labels):
    a = FC.stored_graph(REF, name)
    codes, n_categories = FC.profile_inputs(REF[f"in/{name}/codes"], labels)
    column = FC.categorical(REF[f"in/{name}/codes"]) if labels == "categorical" else FC.plain_labels(REF[f"in/{name}/codes"])
    for distance, abs_nhood, weights in FC.PROFILE_SETTINGS:
        given = None if weights is None else list(weights)
        adata = adata_of(a, column=column)
        if labels == "plain":
            with pytest.warns(UserWarning, match="converting it into categorical type"):
                got = sq.gr.niche_nhood_profile(adata, "cell_type", KEY, distance, abs_nhood, given)
            assert adata.obs["cell_type"].dtype == object
        else:
            got = sq.gr.niche_nhood_profile(adata, "cell_type", KEY, distance, abs_nhood, given)
        assert given == (None if weights is None else list(weights))
        what = (name, labels, distance, abs_nhood, weights)
        assert_bytes_equal(got, O.nhood_profile(a, codes, n_categories, distance, abs_nhood, given), what)
        ref = REF[f"profile/{name}/{labels}/{FC.setting_tag(distance, abs_nhood, weights)}"]
        if name == "weighted":
            assert (np.abs(got - ref) <= O.profile_relative_bound(a, distance, abs_nhood, n_categories) * np.abs(ref)).all(), what
        else:
            assert np.array_equal(got, ref), what


# ---- larger generated inputs --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_graph(name: str):
    if name == "hex":
        return FC.hex_lattice(125, 160)  # 20 000 spots
    if name == "knn":
        return FC.knn_graph(20000, 6, 31)
    return FC.hub_graph(_lib.niche_info()["shell_capacity"])[0]


@functools.lru_cache(maxsize=None)
def big_shells(name: str):
    return O.shells(big_graph(name), 3)


@pytest.mark.parametrize("name", ["hex", "knn", "hub"])
def test_big_shells_equal_restatement(name):
    a = big_graph(name)
    ctx = default_context()
    g = Graph(ctx, a, with_data=False)
    shells = HopShells(ctx, g, 3)
    try:
        for k, (ohop, ovis) in enumerate(big_shells(name), start=1):
            hop, vis = shells.read(k)
            assert_same_csr(hop, ohop, (name, k, "hop"))
            assert_same_csr(vis, ovis, (name, k, "vis"))
        if name == "hub":  # rows on both sides of the capacity, and one exactly at it
            info = shells.info(2)
            assert info["spilled_rows"] >= 2 and info["rows_at_capacity"] >= 1 and info["spilled_rows"] < a.shape[0], info
            assert shells.info(3)["spilled_rows"] > info["spilled_rows"]
        else:
            assert shells.info(2)["spilled_rows"] == 0 and shells.info(3)["spilled_rows"] == 0
    finally:
        shells.close()
        g.close()


def big_expression(n: int, n_vars: int, kind: str):
    x = FC.expression(n, n_vars, 300 + n_vars, density=0.3)
    if kind == "csr32":
        return x.astype(np.float32)
    if kind == "csc":
        return x.tocsc()
    return x.toarray()


@pytest.mark.parametrize(
    "name,n_vars,kind,aggregation",
    [("hex", 7, "csr32", "mean"), ("hex", 65, "dense", "variance"), ("knn", 1, "csc", "variance"), ("knn", 65, "csr32", "mean"),
     ("hub", 7, "dense", "variance"), ("hub", 1, "csr32", "mean")],
)
def test_big_cellcharter_features_equal_restatement(name, n_vars, kind, aggregation):
    a = big_graph(name)
    x = big_expression(a.shape[0], n_vars, kind)
    x64 = O.dense64(x)
    want = np.hstack([x64] + [O.shell_block(hop, x64, aggregation) for hop, _ in big_shells(name)])
    got = sq.gr.niche_cellcharter_features(adata_of(a, x), 3, aggregation)
    assert_bytes_equal(got, want, (name, n_vars, kind, aggregation))


@pytest.mark.parametrize("name,n_vars,kind", [("hex", 65, "csr32"), ("knn", 7, "dense"), ("hub", 1, "csc")])
def test_big_utag_features_equal_restatement(name, n_vars, kind):
    a = big_graph(name)
    if name == "knn":
        a = FC.spectral(a)
    x = big_expression(a.shape[0], n_vars, kind)
    adata = adata_of(a, x)
    got = sq.gr.niche_utag_features(adata)
    assert_bytes_equal(got, O.utag(a, x), (name, n_vars, kind))
    assert_bytes_equal(sq.gr.niche_utag_features(adata), got, "a second call")


@pytest.mark.parametrize("name,n_categories,abs_nhood", [("hex", 30, False), ("knn", 2, True), ("knn", 30, False), ("hub", 2, False)])
def test_big_nhood_profiles_equal_restatement(name, n_categories, abs_nhood):
    a = big_graph(name)
    if name == "knn" and n_categories == 30:
        a = FC.spectral(a)  # float weights
    codes = np.random.default_rng(40 + n_categories).integers(0, n_categories, a.shape[0]).astype(np.int32)
    if n_categories == 30:
        codes[codes == 17] = -1  # missing labels belong to no category
    column = pd.Categorical.from_codes(codes, categories=[f"t{i:02d}" for i in range(n_categories)])
    adata = adata_of(a, column=column)
    got = sq.gr.niche_nhood_profile(adata, "cell_type", distance=3, abs_nhood=abs_nhood, n_hop_weights=[1.0, 0.5])
    assert_bytes_equal(got, O.nhood_profile(a, codes, n_categories, 3, abs_nhood, [1.0, 0.5]), (name, n_categories, abs_nhood))
    assert_bytes_equal(sq.gr.niche_nhood_profile(adata, "cell_type", distance=3, abs_nhood=abs_nhood, n_hop_weights=[1.0, 0.5]), got, "a second call")


# ---- refusals, determinism, side effects, composition -------------------------------------------------------------------------------
def test_a_path_count_at_the_limit_is_refused(monkeypatch):
    """Reaching 2^24 itself needs a graph of some 2^24 edges; the builder takes a lowered limit for tests.  On a hex lattice two paths
    of length 2 reach every neighbour: a limit of 2 is reached in shell 2, not in shell 1, and a limit of 3 only by the six ways back."""
    a = FC.hex_lattice(12, 14)
    ctx = default_context()
    g = Graph(ctx, a, with_data=False)
    try:
        HopShells(ctx, g, 1, count_limit=2).close()
        with pytest.raises(SqgrError) as err:
            HopShells(ctx, g, 2, count_limit=2)
        assert err.value.status == -4 and "path count" in str(err.value)
        with pytest.raises(SqgrError) as err:
            HopShells(ctx, g, 2, count_limit=6)
        assert err.value.status == -4
        HopShells(ctx, g, 2, count_limit=7).close()  # the largest count of shell 2 is 6
        assert max(int((O.shells(a, 1)[0][0] @ sparse.csr_matrix(a)).max()), 0) == 6
    finally:
        g.close()
    monkeypatch.setattr(_niche, "HopShells", lambda c, gr_, d: HopShells(c, gr_, d, 2))
    with pytest.raises(NotImplementedError, match="path count"):
        sq.gr.niche_cellcharter_features(adata_of(a, np.ones((a.shape[0], 2))), 2)


def test_identical_calls_return_identical_bytes_and_leave_adata_alone():
    a = big_graph("knn")
    x = big_expression(a.shape[0], 7, "csr32")
    adata = adata_of(a, x, codes=FC.label_codes(a.shape[0], 5))
    before = (adata.obs.copy(), x.copy(), a.copy(), list(adata.obsp), list(adata.obsm), list(adata.uns))
    for aggregation in ("mean", "variance"):
        first = sq.gr.niche_cellcharter_features(adata, 3, aggregation)
        assert first.tobytes() == sq.gr.niche_cellcharter_features(adata, 3, aggregation).tobytes()
    first = sq.gr.niche_nhood_profile(adata, "cell_type", distance=2)
    assert first.tobytes() == sq.gr.niche_nhood_profile(adata, "cell_type", distance=2).tobytes()
    assert adata.obs.equals(before[0]) and (adata.X != before[1]).nnz == 0 and (adata.obsp[KEY] != before[2]).nnz == 0
    assert (list(adata.obsp), list(adata.obsm), list(adata.uns)) == before[3:]


def test_sdata_and_empty_shapes():
    a, x = FC.stored_graph(REF, "knn"), REF["in/knn/x"]
    adata = adata_of(a, x)
    sdata = type("SData", (), {"tables": {"t": adata}})()
    assert_bytes_equal(sq.gr.niche_utag_features(sdata, table_key="t"), O.utag(a, x), "sdata")
    assert sq.gr.niche_cellcharter_features(adata_of(a, np.zeros((a.shape[0], 0))), 2).shape == (a.shape[0], 0)


def test_cellcharter_features_feed_the_mixture():
    """A smoke test of the composition, not a parity claim: on a lattice whose halves express different genes, a two-component
    mixture on the shell features recovers the halves."""
    a, x, domain = FC.two_domains(40, 50, 4, 9)
    feats = sq.gr.niche_cellcharter_features(adata_of(a, x), distance=2)
    assert feats.shape == (2000, 12)
    fit = sq.gr._niche.gmm_fit(feats[:, :12], 2, random_state=0)
    agree = (fit.labels == domain).mean()
    assert max(agree, 1 - agree) >= 0.97, agree
