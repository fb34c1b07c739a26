"""GPU: ``sq.gr.sepal`` on the MI355X against the reference's literal source (tests/golden/sepal_reference.npz) and the numpy
restatement (tests/sepal_oracle.py).  A gene's stop sweep must lie in its band: between the first sweep whose entropy change is at
most thresh + 1e-15 and the first at most thresh - 1e-15 (the entropy's float64 sums and log are not numpy's); the concentration
trajectory (``sqgr_sepal_trace``) must equal the restatement's bit for bit."""

from __future__ import annotations

import logging
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import squidpy_amd as sq
from squidpy_amd import AnnDataLite
from squidpy_amd._lib import DeviceMatrix, SepalPlan, default_context
from squidpy_amd.gr._sepal import sepal_lattice
from tests import sepal_oracle as SO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sepal_reference.npz"))
CASES = [str(c) for c in GOLD["cases"]]
DT, THRESH, DELTA = float(GOLD["dt"]), float(GOLD["thresh"]), 1e-15


def case(name: str) -> dict:
    n = len(GOLD[f"{name}/spatial"])
    g = sp.csr_matrix((GOLD[f"{name}/data"], GOLD[f"{name}/indices"], GOLD[f"{name}/indptr"]), shape=(n, n))
    return {"g": g, "spatial": GOLD[f"{name}/spatial"], "X": GOLD[f"{name}/X"], "K": int(GOLD[f"{name}/K"]), "n_iter": int(GOLD[f"{name}/n_iter"])}


def make_adata(g, spatial, X, fmt: str = "dense64") -> AnnDataLite:
    X = np.asarray(X)
    if fmt == "dense64":
        X = X.astype(np.float64)
    elif fmt == "dense32":
        X = X.astype(np.float32)
    elif fmt == "csr32":
        X = sp.csr_matrix(X.astype(np.float32))
    elif fmt == "csc64":
        X = sp.csc_matrix(X.astype(np.float64))
    var = pd.DataFrame(index=[f"g{j}" for j in range(X.shape[1])])
    return AnnDataLite(X=X, var=var, obsm={"spatial": spatial}, obsp={"spatial_connectivities": g})


def assert_in_band(score: float, band: tuple[int, int], what) -> None:
    lo, hi = band
    if lo < 0:  # no sweep within n_iter comes near the threshold
        assert np.isnan(score), (what, score)
        return
    assert not np.isnan(score), (what, band)
    i = int(round(score / DT))
    assert DT * float(i) == score
    assert lo <= i <= (hi if hi >= 0 else lo), (what, i, band)
    if hi != lo:
        print(f"band wider than one sweep: {what} {band}")


@pytest.mark.parametrize("fmt", ["dense64", "dense32", "csr32", "csc64"])
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_stop_in_band(name, fmt):
    c = case(name)
    X = c["X"]
    if fmt in ("dense32", "csr32") and not np.array_equal(X.astype(np.float32).astype(np.float64), X.astype(np.float64), equal_nan=True):
        X32 = X.astype(np.float32).astype(np.float64)  # values float32 cannot hold: bands of the widened genes from the restatement
        lat = SO.compute_idxs(c["g"], c["spatial"], c["K"])
        bands = [SO.band(SO.diffusion(X32[:, j], c["K"] == 6, c["n_iter"], lat, DT, THRESH)[1], THRESH) for j in range(X.shape[1])]
    else:
        bands = [tuple(b) for b in GOLD[f"{name}/band"]]
    ad = make_adata(c["g"], c["spatial"], X, fmt)
    df = sq.gr.sepal(ad, max_neighs=c["K"], n_iter=c["n_iter"], copy=True, show_progress_bar=False)
    assert list(df.columns) == ["sepal_score"] and sorted(df.index) == sorted(ad.var_names)
    for j in range(X.shape[1]):
        assert_in_band(df.loc[f"g{j}", "sepal_score"], bands[j], (name, fmt, j))


def _plan(g, spatial, K):
    ctx = default_context()
    sat, sat_idx, unsat, nearest = sepal_lattice(g, spatial, K)
    pos = np.empty(g.shape[0], np.int64)
    pos[sat] = np.arange(len(sat))
    return ctx, SepalPlan(ctx, g.shape[0], K, sat, sat_idx, unsat, pos[nearest] if len(unsat) else np.zeros(0, np.int32))


@pytest.mark.parametrize("name", ["hex20_shuffled", "squaregrid", "visium49"])
def test_trace_bit_identical(name):
    c = case(name)
    ctx, plan = _plan(c["g"], c["spatial"], c["K"])
    m = DeviceMatrix(ctx, np.ascontiguousarray(c["X"], dtype=np.float64))
    lat = SO.compute_idxs(c["g"], c["spatial"], c["K"])
    _, _, ents, _ = SO.diffusion(c["X"][:, 0], c["K"] == 6, 500, lat, DT, None)
    for k in (1, 7, 500):
        conc, ent = plan.trace(m, 0, k, DT)
        assert np.array_equal(conc, GOLD[f"{name}/conc{k}"], equal_nan=True), (name, k)
        assert np.all(np.abs(ent - ents[:k]) <= DELTA), (name, k, np.abs(ent - ents[:k]).max())
    m.close()
    plan.close()


def test_visium_size_grid():
    xy, g = SO.hex_grid(78, 64)
    X = SO.mixed_genes(xy, 16, seed=11)
    n_iter = 2500
    lat = SO.compute_idxs(g, xy, 6)
    bands = [SO.band(SO.diffusion(X[:, j], True, n_iter, lat, DT, THRESH)[1], THRESH) for j in range(16)]
    df = sq.gr.sepal(make_adata(g, xy, X), max_neighs=6, n_iter=n_iter, copy=True)
    for j in range(16):
        assert_in_band(df.loc[f"g{j}", "sepal_score"], bands[j], ("visium", j))
    assert np.isfinite(df["sepal_score"]).sum() >= 4


def test_grid_beyond_lds_capacity():
    """200 x 205 hex spots (41 000: the global route), quickly converging noise genes, and a trace against the restatement."""
    xy, g = SO.hex_grid(200, 205)
    rng = np.random.default_rng(4)
    X = rng.gamma(2.0, 1.0, size=(len(xy), 3))
    lat = SO.compute_idxs(g, xy, 6)
    n_iter = 1500
    bands = [SO.band(SO.diffusion(X[:, j], True, n_iter, lat, DT, THRESH)[1], THRESH) for j in range(3)]
    df = sq.gr.sepal(make_adata(g, xy, X), max_neighs=6, n_iter=n_iter, copy=True)
    for j in range(3):
        assert_in_band(df.loc[f"g{j}", "sepal_score"], bands[j], ("global", j))
    ctx, plan = _plan(g, xy, 6)
    m = DeviceMatrix(ctx, X)
    _, _, ents, kept = SO.diffusion(X[:, 1], True, 7, lat, DT, None, keep=(1, 7))
    for k in (1, 7):
        conc, ent = plan.trace(m, 1, k, DT)
        assert np.array_equal(conc, kept[k]), k
        assert np.all(np.abs(ent - ents[:k]) <= DELTA)
    m.close()
    plan.close()


def _hex_adata(n_genes=8, seed=3, rows=14, cols=16):
    xy, g = SO.hex_grid(rows, cols)
    return make_adata(g, xy, SO.mixed_genes(xy, n_genes, seed=seed))


def test_dense_sparse_alone_and_repeated_give_identical_frames():
    ad = _hex_adata()
    g, xy = ad.obsp["spatial_connectivities"], ad.obsm["spatial"]
    X = np.asarray(ad.X).astype(np.float32).astype(np.float64)  # values every format holds exactly
    ref = sq.gr.sepal(make_adata(g, xy, X), max_neighs=6, copy=True)
    for fmt in ("dense32", "csr32", "csc64"):
        pd.testing.assert_frame_equal(sq.gr.sepal(make_adata(g, xy, X, fmt), max_neighs=6, copy=True), ref)
    pd.testing.assert_frame_equal(sq.gr.sepal(make_adata(g, xy, X), max_neighs=6, copy=True), ref)  # a repeated call
    for gname in ("g1", "g5"):
        alone = sq.gr.sepal(make_adata(g, xy, X, "csr32"), max_neighs=6, genes=gname, copy=True)
        assert alone.shape == (1, 1) and alone.index[0] == gname
        np.testing.assert_array_equal(alone.loc[gname, "sepal_score"], ref.loc[gname, "sepal_score"])


def test_frame_layout_sort_and_uns_slot():
    ad = _hex_adata()
    assert sq.gr.sepal(ad, max_neighs=6) is None
    df = ad.uns["sepal_score"]
    assert list(df.columns) == ["sepal_score"] and df["sepal_score"].dtype == np.float64
    scores = df["sepal_score"].to_numpy()
    fin = scores[~np.isnan(scores)]
    assert np.all(np.diff(fin) <= 0)
    lat = SO.compute_idxs(ad.obsp["spatial_connectivities"], ad.obsm["spatial"], 6)
    raw = [SO.diffusion(np.asarray(ad.X)[:, j], True, 30000, lat, DT, THRESH)[0] for j in range(ad.shape[1])]
    expect = pd.DataFrame([DT * float(i) if i >= 0 else np.nan for i in raw], index=list(ad.var_names), columns=["sepal_score"])
    expect = expect.sort_values(by="sepal_score", ascending=False)
    assert list(df.index) == list(expect.index)


def test_gene_selection_layer_raw_and_hvg():
    ad = _hex_adata(n_genes=6)
    full = sq.gr.sepal(ad, max_neighs=6, copy=True)
    ad.var["highly_variable"] = np.array([True, False, True, False, False, True])
    hvg = sq.gr.sepal(ad, max_neighs=6, copy=True)
    assert sorted(hvg.index) == ["g0", "g2", "g5"]
    for gname in hvg.index:
        assert hvg.loc[gname, "sepal_score"] == full.loc[gname, "sepal_score"] or np.isnan(full.loc[gname, "sepal_score"])
    sub = sq.gr.sepal(ad, max_neighs=6, genes=["g4", "g1"], copy=True)
    assert sorted(sub.index) == ["g1", "g4"]
    ad.layers["shifted"] = np.asarray(ad.X)[:, ::-1].copy()
    lay = sq.gr.sepal(ad, max_neighs=6, genes=["g0"], layer="shifted", copy=True)
    assert lay.loc["g0", "sepal_score"] == full.loc["g5", "sepal_score"] or np.isnan(full.loc["g5", "sepal_score"])
    ad.raw = AnnDataLite(X=np.asarray(ad.X)[:, [3, 0]], var=pd.DataFrame(index=["g3", "g0"]), obsm=ad.obsm)
    rw = sq.gr.sepal(ad, max_neighs=6, genes=["g0", "g3", "g1"], use_raw=True, copy=True)
    assert sorted(rw.index) == ["g0", "g3"]
    for gname in rw.index:
        assert rw.loc[gname, "sepal_score"] == full.loc[gname, "sepal_score"] or np.isnan(full.loc[gname, "sepal_score"])


def test_use_raw_without_raw_warns_and_uses_X(caplog):
    ad = _hex_adata(n_genes=3)
    with caplog.at_level(logging.WARNING, logger="squidpy_amd"):
        df = sq.gr.sepal(ad, max_neighs=6, use_raw=True, copy=True)
    assert "Setting `use_raw=False`" in caplog.text
    pd.testing.assert_frame_equal(df, sq.gr.sepal(ad, max_neighs=6, copy=True))


def test_nan_scores_warn(caplog):
    ad = _hex_adata(n_genes=3)
    with caplog.at_level(logging.WARNING, logger="squidpy_amd"):
        df = sq.gr.sepal(ad, max_neighs=6, n_iter=20, copy=True)
    assert df["sepal_score"].isna().all()
    assert "Found `NaN` in sepal scores" in caplog.text
