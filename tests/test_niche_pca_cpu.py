"""CPU: the numpy restatement of ``niche_pca`` (tests/niche_pca_oracle.py) against sklearn's ``PCA(svd_solver="arpack", random_state=0)``
— scanpy's default ``sc.tl.pca`` on a dense matrix — on the planted cases of tests/niche_pca_cases.py; the restated chain of the
cellcharter flavour's ``use_rep=None`` path against the reference's literal features -> sklearn PCA -> sklearn ``GaussianMixture``
(tests/golden/niche_pca_reference.npz, written by tests/golden/make_niche_pca_golden.py); and the host side of the new front ends —
the ``n_comps`` rule, the sign rule, every refusal — without a device.

The tolerance.  Two eigensolvers that are each backward stable for a symmetric matrix of norm ``lambda_1`` return eigenvectors that
differ by about ``eps * lambda_1 / gap_j`` (Davis-Kahan; ``gap_j`` the distance from ``lambda_j`` to its nearest other eigenvalue) and
eigenvalues that differ by about ``eps * lambda_1`` (Weyl).  The constant in front depends on LAPACK and ARPACK and was measured, not
assumed: over the committed cases the restatement's largest ratio to sklearn, in units of ``eps * lambda_1 / gap_j * max |scores|`` for
the scores and ``eps * lambda_1 / gap_j`` for the components, was 21.34 (case shifted_1e3; the other cases 1.6 to 17.6; explained
variances at most 10.3 in units of ``eps * lambda_1``, their ratios 10.9 in units of ``eps * ratio_1``).  ``C`` = 8 x 21.34 -> 171.
Every case keeps ``eps * lambda_1 / gap_j <= 1e-10`` (measured: at most 1.5e-11), checked below."""

from __future__ import annotations

import functools
import logging
import os

import numpy as np
import pandas as pd
import pytest

from squidpy_amd import gr
from squidpy_amd._anndata_lite import AnnDataLite
from squidpy_amd.gr import _niche

from tests import niche_features_oracle as FO
from tests import niche_pca_cases as PC
from tests import niche_pca_oracle as O

C = PC.C  # 171 = 8 x the largest measured ratio (21.34), see the header
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niche_pca_reference.npz")
KEY = "spatial_connectivities"


def library_or_skip():
    try:
        return PC.chunk_rows()
    except OSError:
        pytest.skip("libsqgr.so is not built")


def test_the_chunk_cases_sit_on_the_librarys_chunk():
    chunk = library_or_skip()
    assert {PC.case("chunk_plus_1").n, PC.case("chunk_minus_1").n} == {chunk + 1, chunk - 1}
    assert chunk == PC.CHUNK_FALLBACK, "NAMES is generated without the library"


@pytest.mark.parametrize("name", PC.NAMES)
def test_cases_keep_the_gap_condition(name):
    c, ref = PC.case(name), PC.reference(name)
    assert c.c < min(c.n, c.d) and PC.data(name).shape == (c.n, c.d)
    cond = PC.EPS * ref.spectrum[0] / O.gaps(ref.spectrum, c.c)
    print(name, "largest eps * lambda_1 / gap_j:", cond.max())
    assert cond.max() <= PC.GAP_CONDITION


@pytest.mark.parametrize("name", PC.NAMES)
def test_restatement_agrees_with_sklearns_arpack_pca(name):
    c, ref, x = PC.case(name), PC.reference(name), PC.data64(name)
    got = O.pca(x, c.c)
    unit = PC.tolerances(name, 1.0)  # eps * lambda_1 / gap_j
    top = np.abs(ref.scores).max()
    figures = {
        "scores": (np.abs(got.X_pca - ref.scores).max(axis=0) / (unit * top)).max(),
        "components": (np.abs(got.components - ref.components).max(axis=1) / unit).max(),
        "variance": (np.abs(got.explained_variance - ref.explained_variance) / (PC.EPS * ref.spectrum[0])).max(),
        "ratio": (np.abs(got.explained_variance_ratio - ref.explained_variance_ratio) / (PC.EPS * ref.explained_variance_ratio[0])).max(),
    }
    print(name, {k: round(float(v), 2) for k, v in figures.items()})
    assert got.X_pca.shape == (c.n, c.c) and got.X_pca.dtype == np.float64
    for j in range(c.c):
        assert np.abs(got.X_pca[:, j] - ref.scores[:, j]).max() <= C * unit[j] * top, (name, j)
        assert np.abs(got.components[j] - ref.components[j]).max() <= C * unit[j], (name, j)
    assert np.abs(got.explained_variance - ref.explained_variance).max() <= C * PC.EPS * ref.spectrum[0]
    assert np.abs(got.explained_variance_ratio - ref.explained_variance_ratio).max() <= C * PC.EPS * ref.explained_variance_ratio[0]
    # the mean: two orders of n - 1 additions and a division
    assert (np.abs(got.mean - ref.mean) <= 2 * O.exact_mean_and_bound(x)[1]).all()
    assert np.all(np.diff(got.explained_variance) <= 0) and (got.explained_variance >= 0).all()


def test_shifted_case_keeps_its_small_components():
    """Centring before the product: the component of the shifted case that is 1e-3 of the first one is still resolved."""
    ref = PC.reference("shifted_1e3")
    got = O.pca(PC.data64("shifted_1e3"), PC.case("shifted_1e3").c)
    last = PC.case("shifted_1e3").c - 1
    assert ref.explained_variance[last] / ref.explained_variance[0] < 5e-3
    assert abs(got.explained_variance[last] / ref.explained_variance[last] - 1) < 1e-9


def test_the_host_side_matches_the_restatement():
    """``pca_components`` (what ``niche_pca`` runs between the two kernels) == the restatement's, on every case's exact scatter."""
    for name in PC.NAMES:
        c, x = PC.case(name), PC.data64(name)
        _, scatter = O.moments(x)
        comps, var = _niche.pca_components(scatter, c.n, c.c)
        want_c, want_v = O.components_of(scatter, c.n, c.c)
        assert np.array_equal(comps, want_c) and np.array_equal(var, want_v), name


def test_n_comps_rule():
    assert _niche.pca_n_comps(1000, 200) == 50 and _niche.pca_n_comps(1000, 51) == 50 and _niche.pca_n_comps(51, 1000) == 50
    assert _niche.pca_n_comps(1000, 50) == 49 and _niche.pca_n_comps(50, 1000) == 49 and _niche.pca_n_comps(3, 2) == 1
    assert _niche.pca_n_comps(1000, 200, 7) == 7
    for n, d in ((1000, 200), (30, 80), (400, 36)):
        assert _niche.pca_n_comps(n, d) == O.n_comps_rule(n, d)


def test_sign_rule():
    comps = np.array([[0.1, -0.7, 0.7], [-0.5, 0.5, 0.2], [0.3, 0.2, -0.1], [-0.2, -0.9, 0.1]])
    got = O.sign_rule(comps)
    # the entry of largest magnitude, the first on ties, is positive
    assert np.array_equal(got, np.array([[-0.1, 0.7, -0.7], [0.5, -0.5, -0.2], [0.3, 0.2, -0.1], [0.2, 0.9, -0.1]]))
    # and the product applies the same rule: a symmetric matrix whose eigenvectors are known
    q, _ = np.linalg.qr(np.random.default_rng(0).normal(size=(6, 6)))
    scatter = (q * np.array([9.0, 7.0, 5.0, 3.0, 2.0, 1.0])) @ q.T
    comps, var = _niche.pca_components((scatter + scatter.T) / 2 * 10, 11, 3)
    for r in range(3):
        pivot = np.argmax(np.abs(comps[r]))
        assert comps[r, pivot] > 0 and abs(abs(comps[r] @ q[:, r]) - 1) < 1e-12
    assert np.allclose(var, [9.0, 7.0, 5.0])


def test_negative_eigenvalues_are_clamped():
    scatter = np.diag([4.0, 1.0, -1e-3, -2e-3])
    _, var = _niche.pca_components(scatter, 2, 3)
    assert np.array_equal(var, [4.0, 1.0, 0.0])


# ---- refusals: nothing reaches the device ----------------------------------------------------------------------------------------------
def test_niche_pca_refusals():
    x = np.random.default_rng(0).normal(size=(30, 8))
    with pytest.raises(ValueError, match="2-D"):
        gr.niche_pca(x[0])
    with pytest.raises(NotImplementedError, match="2 to 4096 features"):
        gr.niche_pca(np.zeros((3, 4097)))
    with pytest.raises(NotImplementedError, match="2 to 4096 features"):
        gr.niche_pca(np.zeros((30, 1)))
    with pytest.raises(NotImplementedError, match="2 to 4096 features"):
        gr.niche_pca(np.zeros((1, 8)))
    with pytest.raises(NotImplementedError, match="at most 64 components"):
        gr.niche_pca(np.zeros((100, 80)), 65)
    with pytest.raises(NotImplementedError, match=r"fewer than min\(n_obs, n_features\) = 8"):
        gr.niche_pca(x, 8)
    with pytest.raises(NotImplementedError, match=r"fewer than min\(n_obs, n_features\) = 5"):
        gr.niche_pca(x[:5], 5)
    with pytest.raises(ValueError, match="positive"):
        gr.niche_pca(x, 0)
    with pytest.raises(TypeError, match="`n_comps`"):
        gr.niche_pca(x, 2.5)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[3, 2] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            gr.niche_pca(y)


def small_adata(n_vars: int = 3) -> AnnDataLite:
    a, x, _ = PC.chain_inputs("hex_d2")
    obs = pd.DataFrame({"lib": ["a"] * 200 + ["b"] * 200}, index=[f"c{i}" for i in range(400)])
    return AnnDataLite(X=np.array(x[:, :n_vars]), obs=obs, obsp={KEY: a}, obsm={"rep": np.array(x[:, :12])})


def test_embedding_refusals():
    adata = small_adata()
    with pytest.raises(KeyError, match="missing"):
        gr.niche_cellcharter_embedding(adata, spatial_connectivities_key="missing")
    with pytest.raises(ValueError, match="Invalid aggregation method 'median'"):
        gr.niche_cellcharter_embedding(adata, aggregation="median")
    with pytest.raises(ValueError, match="at least 1"):
        gr.niche_cellcharter_embedding(adata, distance=0)
    with pytest.raises(NotImplementedError, match="at most 64 components"):
        gr.niche_cellcharter_embedding(small_adata(12), distance=7, n_comps=65)
    with pytest.raises(NotImplementedError, match="fewer than min"):
        gr.niche_cellcharter_embedding(adata, distance=1, n_comps=6)
    with pytest.raises(NotImplementedError, match="fewer than min"):
        gr.niche_utag_embedding(adata, n_comps=3)
    with pytest.raises(KeyError, match="missing"):
        gr.niche_utag_embedding(adata, "missing")
    weighted = small_adata()
    weighted.obsp[KEY] = weighted.obsp[KEY] * 0.5
    with pytest.raises(NotImplementedError, match="stored values are all 1"):
        gr.niche_cellcharter_embedding(weighted)
    wide = AnnDataLite(X=np.zeros((400, 1400)), obs=adata.obs, obsp=adata.obsp)
    with pytest.raises(NotImplementedError, match="2 to 4096 features"):
        gr.niche_cellcharter_embedding(wide, distance=3)


def test_proxy_pca_keyword():
    adata = small_adata()
    with pytest.raises(NotImplementedError, match="use_rep"):
        gr.calculate_niche_cellcharter(adata)  # the default leaves `use_rep=None` as it was
    with pytest.raises(NotImplementedError, match="use_rep"):
        gr.calculate_niche_cellcharter(adata, proxy_pca=False)
    with pytest.raises(ValueError, match="proxy_pca=True"):
        gr.calculate_niche_cellcharter(adata, use_rep="rep", proxy_pca=True)
    with pytest.raises(TypeError):
        gr.calculate_niche_cellcharter(adata, 3, "mean", 42, KEY, 10, None, None, None, None, True, None, True)  # keyword-only
    with pytest.raises(TypeError, match="unexpected keyword argument 'proxy'"):
        gr.calculate_niche_cellcharter(adata, use_rep="rep", proxy=True)
    with pytest.raises(ValueError, match="Invalid aggregation method"):
        gr.calculate_niche_cellcharter(adata, aggregation="sum", proxy_pca=True)
    with pytest.raises(KeyError, match="nolib"):
        gr.calculate_niche_cellcharter(adata, library_key="nolib", proxy_pca=True)
    with pytest.raises(KeyError, match="missing"):
        gr.calculate_niche_cellcharter(adata, spatial_connectivities_key="missing", proxy_pca=True)
    assert "cellcharter_niche" not in adata.obs


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_features(graph_name: str, lib: int) -> np.ndarray:
    name = next(n for n in PC.CHAIN_NAMES if PC.CHAINS[n].graph == graph_name)
    a, x, library = PC.chain_inputs(name)
    rows = np.flatnonzero(library == lib)
    sub = a[rows][:, rows].tocsr()
    sub.sort_indices()
    return FO.cellcharter(sub, x[rows], PC.CHAINS[name].distance, "mean")


def test_chain_shapes():
    assert restated_features("hex", 0).shape == (400, 36) and restated_features("knn", 0).shape == (1500, 80)
    assert O.n_comps_rule(400, 36) == 35 and O.n_comps_rule(1500, 80) == 50
    _, _, library = PC.chain_inputs("two_libraries")
    assert np.bincount(library).tolist() == [210, 192] and (np.diff(library) != 0).sum() > 10  # the libraries' rows are interleaved


@pytest.mark.parametrize("name", PC.CHAIN_NAMES)
def test_restated_chain_equals_sklearns_chain(name):
    ch = PC.CHAINS[name]
    _, _, library = PC.chain_inputs(name)
    recorded = np.load(GOLDEN)
    rows_of = [np.flatnonzero(library == lib) for lib in range(ch.libraries)]
    by_rows = {len(rows): lib for lib, rows in enumerate(rows_of)}
    # sklearn's chain behind the restated features == the recorded chain behind the reference's literal features
    live = PC.sklearn_chain(lambda sub, x, distance: restated_features(ch.graph, by_rows[sub.shape[0]]), name)
    print(name, "margin", live.margin, "recorded", float(recorded[f"{name}/margin"]), "n_iter", live.n_iter, "features differ by",
          float(recorded[f"{name}/features_max_abs_diff"]))
    assert live.margin >= PC.MIN_MARGIN and float(recorded[f"{name}/margin"]) >= PC.MIN_MARGIN
    assert np.array_equal(live.labels, recorded[f"{name}/labels"])
    assert list(live.n_iter) == list(recorded[f"{name}/n_iter"]) and list(live.converged) == list(recorded[f"{name}/converged"])
    # the restated chain == sklearn's
    for lib, rows in enumerate(rows_of):
        fit = O.chain(restated_features(ch.graph, lib), ch.k, ch.random_state)
        assert np.array_equal(fit.labels, live.labels[rows]), (name, lib)
        assert fit.n_iter == live.n_iter[lib] and fit.converged == live.converged[lib], (name, lib)


def test_proxy_warning_sentence_is_the_references():
    assert _niche.PROXY_PCA_MSG.startswith("CellCharter recommends to use a dimensionality reduced embedding of the data, e.g. a scVI embedding.")
    assert _niche.PROXY_PCA_MSG.endswith("Since 'use_rep' is not provided, PCA will be used as proxy - performance may be suboptimal.")
    assert isinstance(_niche.logg, logging.Logger)
