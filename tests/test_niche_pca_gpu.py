"""GPU: ``csrc/sqgr_pca.hip`` and the front ends on it (``niche_pca``, ``niche_utag_embedding``, ``niche_cellcharter_embedding``,
``calculate_niche_cellcharter(use_rep=None, proxy_pca=True)``) on the cases of tests/niche_pca_cases.py.

- Means and scatter against exactly rounded references (``math.fsum`` of error-free products) within the order-free bound
  ``gamma(n + 2) * sum |terms|`` — derived, not measured; exactly symmetric; two calls, the same bytes.
- The projection ``==`` the numpy restatement (tests/niche_pca_oracle.py: a loop over j, vectorised over the rows) bit for bit, given the
  device's own mean and the same components.
- ``niche_pca`` scores against sklearn's ``PCA(svd_solver="arpack")`` within ``tol_j = C eps lambda_1 / gap_j max |scores|``, ``C`` = 171
  as measured and derived in tests/test_niche_pca_cpu.py.
- The device-side fill of the feature blocks ``==`` the host round trip, bit for bit.
- Launch-geometry seams (``PC.SEAM_CASES``: chunks of more than 512 rows, the chunk cap of the scatter, D = 4096): means within the same
  exact bound; the scatter of the narrow case exactly over all pairs, of the two wide cases as a whole against float64 ``z.T @ z``
  within ``2 gamma(n + 2) |z|.T @ |z|`` (device and BLAS each lie within one ``gamma`` of the exact value) and exactly on a seeded sample
  of 2 000 entries plus the four corners; exact symmetry; two calls, the same bytes; the projection bit for bit on seeded orthonormal rows.
- The chain's labels ``==`` sklearn's chain behind the reference's literal features (tests/golden/niche_pca_reference.npz)."""

from __future__ import annotations

import functools
import logging
import os

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import squidpy_amd as sq
from squidpy_amd import AnnDataLite
from squidpy_amd._lib import DevicePCA, SqgrError, default_context
from squidpy_amd.gr import _niche

from tests import niche_features_cases as FC
from tests import niche_pca_cases as PC
from tests import niche_pca_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niche_pca_reference.npz"))
KEY = "spatial_connectivities"
C = PC.C


@functools.lru_cache(maxsize=None)
def device_moments(name: str):
    """``(mean, scatter)`` of the case from the device, twice."""
    x = PC.data(name)
    pca = DevicePCA(default_context(None), *x.shape)
    try:
        pca.upload(x)
        return pca.moments(), pca.moments()
    finally:
        pca.close()


@functools.lru_cache(maxsize=None)
def exact_moments(name: str):
    x = PC.data64(name)
    mean, mean_bound = O.exact_mean_and_bound(x)
    device_mean = device_moments(name)[0][0]
    scatter, scatter_bound = O.exact_scatter_and_bound(x, device_mean)
    return mean, mean_bound, scatter, scatter_bound


@pytest.mark.parametrize("name", PC.NAMES)
def test_means_and_scatter_within_the_order_free_bound(name):
    (mean, scatter), (mean2, scatter2) = device_moments(name)
    want_mean, mean_bound, want_scatter, scatter_bound = exact_moments(name)
    print(name, "mean error / bound", float(np.max(np.abs(mean - want_mean) / np.maximum(mean_bound, 1e-300))), "scatter error / bound",
          float(np.max(np.abs(scatter - want_scatter) / np.maximum(scatter_bound, 1e-300))))
    assert (np.abs(mean - want_mean) <= mean_bound).all()
    assert (np.abs(scatter - want_scatter) <= scatter_bound).all()
    assert np.array_equal(scatter, scatter.T)
    assert mean.tobytes() == mean2.tobytes() and scatter.tobytes() == scatter2.tobytes()
    if PC.case(name).constant_column:
        j = PC.case(name).d // 2
        assert mean[j] == 3.25 and not scatter[j].any() and not scatter[:, j].any()


@pytest.mark.parametrize("name", PC.NAMES)
def test_projection_equals_the_restatement_bit_for_bit(name):
    x, c = PC.data(name), PC.case(name)
    pca = DevicePCA(default_context(None), c.n, c.d)
    try:
        pca.upload(x)
        mean, scatter = pca.moments()
        components, _ = O.components_of(scatter, c.n, c.c)
        got = pca.project(components)
    finally:
        pca.close()
    want = O.project(PC.data64(name), mean, components)
    assert got.shape == (c.n, c.c) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", PC.NAMES)
def test_scores_agree_with_sklearn(name):
    c, ref = PC.case(name), PC.reference(name)
    got = sq.gr.niche_pca(PC.data(name), c.c)
    unit = PC.tolerances(name, 1.0)
    top = np.abs(ref.scores).max()
    print(name, "largest score error / (eps lambda_1 / gap_j max|scores|):", float((np.abs(got.X_pca - ref.scores).max(axis=0) / (unit * top)).max()))
    assert got.X_pca.dtype == np.float64 and got.X_pca.shape == (c.n, c.c)
    for j in range(c.c):
        assert np.abs(got.X_pca[:, j] - ref.scores[:, j]).max() <= C * unit[j] * top, (name, j)
        assert np.abs(got.components[j] - ref.components[j]).max() <= C * unit[j], (name, j)
    assert np.abs(got.explained_variance - ref.explained_variance).max() <= C * PC.EPS * ref.spectrum[0]
    assert np.abs(got.explained_variance_ratio - ref.explained_variance_ratio).max() <= C * PC.EPS * ref.explained_variance_ratio[0]
    assert got.mean.tobytes() == device_moments(name)[0][0].tobytes()
    again = sq.gr.niche_pca(PC.data(name), c.c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


# ---- launch-geometry seams ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_run(name: str):
    """``(mean, scatter, second call returned the same bytes, projection)`` of a seam case from the device."""
    x, c = PC.data(name), PC.case(name)
    pca = DevicePCA(default_context(None), c.n, c.d)
    try:
        pca.upload(x)
        mean, scatter = pca.moments()
        mean2, scatter2 = pca.moments()
        same = mean.tobytes() == mean2.tobytes() and scatter.tobytes() == scatter2.tobytes()
        del scatter2
        return mean, scatter, same, pca.project(PC.seam_components(name))
    finally:
        pca.close()


@pytest.mark.parametrize("name", PC.SEAM_NAMES)
def test_seam_means_within_the_order_free_bound(name):
    mean = seam_run(name)[0]
    want, bound = O.exact_mean_and_bound(PC.data64(name))
    print(name, "mean error / bound", float(np.max(np.abs(mean - want) / np.maximum(bound, 1e-300))), "max |error|", float(np.abs(mean - want).max()))
    assert (np.abs(mean - want) <= bound).all()


def test_seam_scatter_of_the_narrow_case_exactly():
    mean, scatter, same, _ = seam_run("mean_cap")
    want, bound = O.exact_scatter_and_bound(PC.data64("mean_cap"), mean)
    print("mean_cap scatter error / bound", float(np.max(np.abs(scatter - want) / np.maximum(bound, 1e-300))), "max |error|",
          float(np.abs(scatter - want).max()), "max |S|", float(np.abs(want).max()))
    assert (np.abs(scatter - want) <= bound).all()
    assert np.array_equal(scatter, scatter.T) and same


@pytest.mark.parametrize("name", ("limit_d4096", "capped_chunks"))
def test_seam_scatter_of_a_wide_case(name):
    c = PC.case(name)
    mean, scatter, same, _ = seam_run(name)
    assert np.array_equal(scatter, scatter.T) and same
    z = PC.data64(name) - mean
    blas = z.T @ z
    az = np.abs(z)
    bound = 2.0 * O.gamma(c.n + 2) * (az.T @ az)
    err = np.abs(scatter - blas)
    print(name, "whole scatter vs float64 z.T @ z: error / bound", float(np.max(err / np.maximum(bound, 1e-300))), "max |error|", float(err.max()),
          "max |S|", float(np.abs(blas).max()))
    assert (err <= bound).all()
    rng = np.random.default_rng(c.seed + 2000)
    pairs = np.r_[rng.integers(0, c.d, (2000, 2)), [[0, 0], [0, c.d - 1], [c.d - 1, 0], [c.d - 1, c.d - 1]]]
    want, exact_bound = O.exact_scatter_pairs_and_bound(PC.data64(name), mean, pairs)
    got = scatter[pairs[:, 0], pairs[:, 1]]
    print(name, "sampled entries vs exact: error / bound", float(np.max(np.abs(got - want) / np.maximum(exact_bound, 1e-300))), "max |error|",
          float(np.abs(got - want).max()))
    assert (np.abs(got - want) <= exact_bound).all()


@pytest.mark.parametrize("name", PC.SEAM_NAMES)
def test_seam_projection_equals_the_restatement_bit_for_bit(name):
    c = PC.case(name)
    mean, _, _, got = seam_run(name)
    components = PC.seam_components(name)
    assert components.shape == (c.c, c.d) and np.abs(components @ components.T - np.eye(c.c)).max() < 1e-12
    want = O.project(PC.data64(name), mean, components)
    assert got.shape == (c.n, c.c) and got.tobytes() == want.tobytes()


def test_default_n_comps_and_column_upload():
    x = PC.data("n700_d130_c50")
    assert sq.gr.niche_pca(x).X_pca.shape == (700, 50) and sq.gr.niche_pca(x[:40]).X_pca.shape == (40, 39)
    # a column range of a wider array goes up through its row pitch
    assert sq.gr.niche_pca(x[:, 10:75], 5).X_pca.tobytes() == sq.gr.niche_pca(np.ascontiguousarray(x[:, 10:75]), 5).X_pca.tobytes()


# ---- the feature path: filled on the device == the host round trip -----------------------------------------------------------------------
def adata_of(a, x) -> AnnDataLite:
    return AnnDataLite(X=x, obs=pd.DataFrame(index=[f"c{i}" for i in range(a.shape[0])]), obsp={KEY: a})


def feature_inputs(x: np.ndarray):
    return {"dense64": x, "csr32": sparse.csr_matrix(x.astype(np.float32)), "csc64": sparse.csc_matrix(x)}


@pytest.mark.parametrize("kind", ("dense64", "csr32", "csc64"))
@pytest.mark.parametrize("aggregation", ("mean", "variance"))
def test_cellcharter_embedding_equals_pca_of_the_features(kind, aggregation):
    a = FC.golden_graphs()["knn_loops"]
    x = feature_inputs(FC.expression(a.shape[0], 7, 41).toarray())[kind]  # D = 28, not a multiple of four per block
    adata = adata_of(a, x)
    feats = sq.gr.niche_cellcharter_features(adata, 3, aggregation)
    for n_comps in (None, 9):
        got = sq.gr.niche_cellcharter_embedding(adata, 3, aggregation, n_comps=n_comps)
        want = sq.gr.niche_pca(feats, n_comps).X_pca
        assert got.shape == want.shape == (a.shape[0], 27 if n_comps is None else 9) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", ("dense64", "csr32", "csc64"))
def test_utag_embedding_equals_pca_of_the_features(kind):
    a = FC.golden_graphs()["weighted"]
    x = feature_inputs(FC.expression(a.shape[0], 70, 42).toarray())[kind]  # two aggregation blocks of columns
    adata = adata_of(a, x)
    got = sq.gr.niche_utag_embedding(adata)
    want = sq.gr.niche_pca(sq.gr.niche_utag_features(adata)).X_pca
    assert got.shape == (a.shape[0], 50) and got.tobytes() == want.tobytes()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def chain_adata(name: str) -> AnnDataLite:
    a, x, library = PC.chain_inputs(name)
    obs = pd.DataFrame({"library": pd.Categorical(np.where(library == 0, "s0", "s1"))}, index=[f"c{i}" for i in range(len(library))])
    return AnnDataLite(X=np.array(x), obs=obs, obsp={KEY: a.copy()})


def expected_column(name: str, index, prefixes, mask=None, min_niche_size=None) -> list[str]:
    """sklearn's chain labels behind the reference's literal features, through the reference's post-processing."""
    labels = GOLDEN[f"{name}/labels"].astype(np.int64)
    if prefixes is None and mask is None and min_niche_size is None:
        return list(labels)
    _, _, library = PC.chain_inputs(name)
    out = pd.Series("", index=index, dtype=object)
    for lib, prefix in enumerate(prefixes or [None]):
        rows = np.flatnonzero(library == lib) if prefixes else np.arange(len(library))
        obs = pd.DataFrame({"cellcharter_niche": pd.Categorical(labels[rows])}, index=index[rows])
        _niche.postprocess_niche_results(obs, ["cellcharter_niche"], mask, min_niche_size, prefix)
        out.iloc[rows] = obs["cellcharter_niche"].astype(str).to_numpy()
    return list(out)


@pytest.mark.parametrize("name", ("hex_d2", "knn_d3_k4", "knn_d3_k10"))
def test_chain_labels_equal_sklearns_chain(name, caplog):
    ch = PC.CHAINS[name]
    adata = chain_adata(name)
    before = adata.X.copy()
    with caplog.at_level(logging.WARNING, logger="squidpy_amd"):
        assert sq.gr.calculate_niche_cellcharter(adata, ch.distance, "mean", ch.random_state, n_components=ch.k, proxy_pca=True) is None
    assert _niche.PROXY_PCA_MSG in [r.getMessage() for r in caplog.records]
    got = adata.obs["cellcharter_niche"]
    assert isinstance(got.dtype, pd.CategoricalDtype) and list(got) == expected_column(name, adata.obs.index, None)
    assert np.array_equal(adata.X, before)
    if name != "hex_d2":
        return
    mask = pd.Series(np.arange(400) % 7 != 0, index=adata.obs.index)
    for kwargs in ({"mask": mask}, {"min_niche_size": 50}, {"mask": mask, "min_niche_size": 100}):
        out = sq.gr.calculate_niche_cellcharter(adata, ch.distance, "mean", ch.random_state, n_components=ch.k, proxy_pca=True, inplace=False, **kwargs)
        want = expected_column(name, adata.obs.index, None, kwargs.get("mask"), kwargs.get("min_niche_size"))
        assert list(out.obs["cellcharter_niche"]) == want and "not_a_niche" in want, kwargs


def test_chain_with_two_libraries():
    name = "two_libraries"
    ch = PC.CHAINS[name]
    adata = chain_adata(name)
    prefixes = [f"lib={lib}_" for lib in adata.obs["library"].unique()]
    assert prefixes == ["lib=s0_", "lib=s1_"] or prefixes == ["lib=s1_", "lib=s0_"]
    prefixes = ["lib=s0_", "lib=s1_"]  # by library number
    sq.gr.calculate_niche_cellcharter(adata, ch.distance, "mean", ch.random_state, n_components=ch.k, library_key="library", proxy_pca=True)
    assert list(adata.obs["cellcharter_niche"]) == expected_column(name, adata.obs.index, prefixes)
    mask = pd.Series(np.arange(adata.n_obs) % 5 != 0, index=adata.obs.index)
    # a fresh table: a column that exists before a `library_key` call is left as it is (the reference's rule)
    out = sq.gr.calculate_niche_cellcharter(chain_adata(name), ch.distance, "mean", ch.random_state, n_components=ch.k, library_key="library",
                                            mask=mask, min_niche_size=40, proxy_pca=True, inplace=False)
    want = expected_column(name, adata.obs.index, prefixes, mask, 40)
    assert list(out.obs["cellcharter_niche"]) == want and any(w.endswith("not_a_niche") for w in want)


# ---- allocations and limits --------------------------------------------------------------------------------------------------------------
def test_allocations_of_a_call():
    """``niche_pca`` asks the allocator for seven buffers whatever the size: F and the mean (create); the chunk sums of the means, the
    chunk partials of the scatter and S (moments); the transposed components and the scores (project) — and gives all seven back."""
    ctx = default_context(None)
    sq.gr.niche_pca(PC.data("n65_d5_c4"), 4)  # whatever a first call sets up is behind us
    deltas = []
    for name in ("n300_d12_c11", "n700_d130_c50"):
        before = ctx.alloc_counters()
        sq.gr.niche_pca(PC.data(name), PC.case(name).c)
        after = ctx.alloc_counters()
        deltas.append({k: after[k] - before[k] for k in ("mallocs", "malloc_bytes", "frees", "pool_hits", "pool_parks")})
        print(name, deltas[-1])
    for delta, name in zip(deltas, ("n300_d12_c11", "n700_d130_c50")):
        c = PC.case(name)
        assert delta["mallocs"] == 7 and delta["frees"] == 7 and delta["pool_hits"] == 0 and delta["pool_parks"] == 0
        assert delta["malloc_bytes"] >= 8 * (c.n * c.d + c.d + c.d * c.d + c.n * c.c)
    assert deltas[1]["malloc_bytes"] > deltas[0]["malloc_bytes"]
    # the float32 upload stages the values once more
    before = ctx.alloc_counters()
    sq.gr.niche_pca(PC.data("float32"), 16)
    after = ctx.alloc_counters()
    assert after["mallocs"] - before["mallocs"] == 8 and after["frees"] - before["frees"] == 8


def test_limits_through_the_c_abi_and_the_front_end():
    ctx = default_context(None)
    for n, d in ((10, 4097), (10, 1), (1, 10)):
        with pytest.raises(SqgrError) as exc:
            DevicePCA(ctx, n, d)
        assert exc.value.status == -4
    x = np.random.default_rng(5).normal(size=(100, 80))
    pca = DevicePCA(ctx, 100, 80)
    try:
        pca.upload(x)
        with pytest.raises(SqgrError, match="sqgr_pca_moments has not run") as exc:
            pca.project(np.zeros((3, 80)))
        assert exc.value.status == -1
        pca.moments()
        for c in (65, 80):
            with pytest.raises(SqgrError) as exc:
                pca.project(np.zeros((c, 80)))
            assert exc.value.status == -4
        assert pca.project(np.eye(80)[:64]).shape == (100, 64)
    finally:
        pca.close()
    small = DevicePCA(ctx, 20, 30)
    try:
        small.upload(x[:20, :30])
        small.moments()
        with pytest.raises(SqgrError) as exc:
            small.project(np.zeros((20, 30)))  # c = min(n, D)
        assert exc.value.status == -4
    finally:
        small.close()
    with pytest.raises(NotImplementedError):
        sq.gr.niche_pca(np.zeros((10, 4097)))
    with pytest.raises(NotImplementedError):
        sq.gr.niche_pca(x, 65)
    with pytest.raises(NotImplementedError):
        sq.gr.niche_pca(x[:20, :30], 20)
