"""CPU: ``sq.gr.sepal``'s host side against the reference's literal source (tests/golden/sepal_reference.npz, made by
tests/golden/make_sepal_golden.py): the numpy restatement's stop sweeps and trajectories, the host lattice, the signature, the
checks that raise before any device is touched, and the divergence that scores a lattice the reference's sklearn call rejects."""

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
from squidpy_amd.gr import _sepal

from tests import sepal_oracle as SO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sepal_reference.npz"))
CASES = [str(c) for c in GOLD["cases"]]
DT, THRESH = float(GOLD["dt"]), float(GOLD["thresh"])


def case(name: str) -> dict:
    n = len(GOLD[f"{name}/spatial"])
    g = sp.csr_matrix((GOLD[f"{name}/data"], GOLD[f"{name}/indices"], GOLD[f"{name}/indptr"]), shape=(n, n))
    return {"g": g, "spatial": GOLD[f"{name}/spatial"], "X": GOLD[f"{name}/X"], "K": int(GOLD[f"{name}/K"]), "n_iter": int(GOLD[f"{name}/n_iter"])}


def lattice(name: str) -> tuple:
    return tuple(GOLD[f"{name}/{k}"] for k in ("sat", "sat_idx", "unsat", "unsat_idx"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_lattice_equals_literal(name):
    c = case(name)
    for a, b in zip(SO.compute_idxs(c["g"], c["spatial"], c["K"]), lattice(name)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_host_lattice_equals_literal(name):
    """The front end's vectorised lattice == the literal ``_compute_idxs``: stored order, first saturated neighbour, L1 ties."""
    c = case(name)
    for a, b in zip(_sepal.sepal_lattice(c["g"], c["spatial"], c["K"]), lattice(name)):
        assert np.array_equal(a, b)


def test_host_lattice_l1_fallback_and_ties():
    """Unsaturated spots without a saturated neighbour take the saturated spot at the smallest L1 distance, the first on ties."""
    xy, g = SO.hex_grid(9, 9)
    g = g.tolil()
    for i in (0, 1, 9, 80):  # cut corner spots loose: they keep no saturated neighbour
        for j in list(g.rows[i]):
            g[i, j] = 0
            g[j, i] = 0
    g = g.tocsr()
    g.eliminate_zeros()
    g.sort_indices()
    ref = SO.compute_idxs(g, xy, 6)
    for a, b in zip(_sepal.sepal_lattice(g, xy, 6), ref):
        assert np.array_equal(a, b)
    xy_int = np.round(xy / 100.0)  # integer coordinates: many exact L1 ties
    for a, b in zip(_sepal.sepal_lattice(g, xy_int, 6), SO.compute_idxs(g, xy_int, 6)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_restatement_stop_sweeps_equal_literal(name):
    c = case(name)
    lat = lattice(name)
    for j in range(c["X"].shape[1]):
        stop, deltas, _, _ = SO.diffusion(c["X"][:, j], c["K"] == 6, c["n_iter"], lat, DT, THRESH)
        assert stop == GOLD[f"{name}/stop"][j], (name, j)
        assert SO.band(deltas, THRESH) == tuple(GOLD[f"{name}/band"][j]), (name, j)


@pytest.mark.parametrize("name", CASES)
def test_restatement_trajectory_bit_identical(name):
    c = case(name)
    _, _, _, kept = SO.diffusion(c["X"][:, 0], c["K"] == 6, 500, lattice(name), DT, None, keep=(1, 7, 500))
    for k in (1, 7, 500):
        assert np.array_equal(kept[k], GOLD[f"{name}/conc{k}"], equal_nan=True), (name, k)


def test_signature_matches_reference():
    ref = json.loads(str(GOLD["signature"]))
    params = list(inspect.signature(sq.gr.sepal).parameters.values())
    pos = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == [a["name"] for a in ref["positional"]]
    special = {"Key.obsp.spatial_conn()": "spatial_connectivities", "Key.obsm.spatial": "spatial"}
    for p, a in zip(pos, ref["positional"]):
        want = inspect.Parameter.empty if a["default"] is None else special.get(a["default"]) or eval(a["default"])
        assert p.default == want, p.name
    kwonly = {p.name: p for p in params if p.kind == p.KEYWORD_ONLY}
    assert {a["name"] for a in ref["keyword_only"]} | {"device"} == set(kwonly)
    assert kwonly["device"].default is None
    assert any("backend" in d for d in ref["decorators"])


def _adata(g, n_genes: int = 3, **kw) -> AnnDataLite:
    n = g.shape[0]
    xy = kw.pop("spatial", np.zeros((n, 2)))
    X = np.random.default_rng(0).random((n, n_genes))
    return AnnDataLite(X=X, obsm={"spatial": xy}, obsp={"spatial_connectivities": g}, **kw)


@pytest.fixture
def no_device(monkeypatch):
    """Fail loudly if the front end reaches the device."""

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_sepal, "default_context", boom)
    monkeypatch.setattr(_sepal, "SepalPlan", boom)
    monkeypatch.setattr(_sepal, "DeviceMatrix", boom)


def test_checks_raise_before_the_device(no_device):
    xy, g = SO.hex_grid(6, 6)
    ad = _adata(g, spatial=xy)
    with pytest.raises(ValueError, match=r"Expected `max_neighs` to be either `4` or `6`, found `5`."):
        sq.gr.sepal(ad, max_neighs=5)
    with pytest.raises(ValueError, match=r"Expected `max_neighs=4`, found node with `6` neighbors."):
        sq.gr.sepal(ad, max_neighs=4)
    with pytest.raises(ValueError, match="No genes have been selected."):
        sq.gr.sepal(ad, max_neighs=6, genes=[])
    with pytest.raises(KeyError, match="Layer `nope` not found"):
        sq.gr.sepal(ad, max_neighs=6, layer="nope")
    with pytest.raises(KeyError):
        sq.gr.sepal(AnnDataLite(X=ad.X, obsm={"spatial": xy}, obsp={}), max_neighs=6)
    with pytest.warns(FutureWarning, match="backend"):
        with pytest.raises(ValueError):
            sq.gr.sepal(ad, max_neighs=5, backend="loky")


def test_zeros_in_the_graph_are_eliminated_on_a_copy(no_device):
    """A stored zero does not count as a neighbour (the reference's ``eliminate_zeros``), and the caller's matrix keeps it."""
    xy, g = SO.hex_grid(6, 6)
    rows = [list(zip(g.indices[a:b], g.data[a:b])) for a, b in zip(g.indptr[:-1], g.indptr[1:])]
    i = 14  # an interior spot gets a seventh stored entry, an explicit zero
    j = next(c for c in range(36) if c != i and c not in g.indices[g.indptr[i] : g.indptr[i + 1]])
    rows[i].append((j, 0.0))
    indptr = np.cumsum([0] + [len(r) for r in rows])
    g = sp.csr_matrix(([v for r in rows for _, v in r], [c for r in rows for c, _ in r], indptr), shape=(36, 36))
    assert np.diff(g.indptr).max() == 7
    nnz = g.nnz
    ad = _adata(g, spatial=xy)
    with pytest.raises(AssertionError, match="the device was touched"):
        sq.gr.sepal(ad, max_neighs=6)
    assert ad.obsp["spatial_connectivities"].nnz == nnz


def test_lattice_without_distance_query_is_scored(monkeypatch):
    """No unsaturated spot lacks a saturated neighbour (a hex grid without its two corner spots): the reference hands sklearn a
    distance query on zero rows, which raises; the drop-in scores the lattice."""
    from sklearn.metrics import pairwise_distances

    xy, g = SO.hex_grid(8, 8)
    assert len(SO.fallback_rows(g, 6)) == 2  # the corners: the full grid does take the L1 route
    xy, g = SO.drop_spots(xy, g, SO.fallback_rows(g, 6))
    assert np.diff(g.indptr).max() == 6 and len(SO.fallback_rows(g, 6)) == 0
    ref = SO.compute_idxs(g, xy, 6)
    sat, sat_idx, unsat, nearest = _sepal.sepal_lattice(g, xy, 6)
    for a, b in zip((sat, sat_idx, unsat, nearest), ref):
        assert np.array_equal(a, b)
    assert len(unsat) > 0
    with pytest.raises(ValueError):  # what the reference's `pairwise_distances(spatial[un_unsat], spatial[sat], metric="l1")` does here
        pairwise_distances(xy[np.zeros(0, np.int64)], xy[sat], metric="l1")
    seen = {}

    class FakePlan:
        def __init__(self, ctx, n, K, s, nb, u, src):
            seen["src"] = np.asarray(src)

        def run(self, m, cols, n_iter, dt, thresh):
            return np.array([3, -1, 0], dtype=np.int32)[: len(cols)]

        def close(self):
            pass

    class FakeMatrix:
        def __init__(self, ctx, x):
            pass

        def close(self):
            pass

    monkeypatch.setattr(_sepal, "default_context", lambda device=None: None)
    monkeypatch.setattr(_sepal, "SepalPlan", FakePlan)
    monkeypatch.setattr(_sepal, "DeviceMatrix", FakeMatrix)
    ad = _adata(g, spatial=xy)
    df = sq.gr.sepal(ad, max_neighs=6, copy=True)
    assert list(df.columns) == ["sepal_score"]
    assert df["sepal_score"].tolist()[:2] == [0.001 * 3.0, 0.0] and np.isnan(df["sepal_score"].iloc[2])
    assert np.array_equal(sat[seen["src"]], nearest)  # positions in sat[] of the nearest saturated spots
