"""GPU: the mask kernels (csrc/sqgr_mask.hip) against the numpy code of gr/_mask.py — answers, classes and path counts `==`."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import squidpy_amd as sq
from squidpy_amd import _lib
from squidpy_amd.gr._mask import Polygon, _flat_rings, _polygons, segments_within
from tests import mask_graph_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context(None)


@pytest.fixture(scope="module")
def cap():
    return _lib.mask_info()["param_cap"]


@pytest.fixture(scope="module")
def solved(cap):
    """Every case with the host's answer and path counts, computed once."""
    return {name: (a, b, mask, MC.oracle(a, b, mask)) for name, a, b, mask in MC.cases(cap)}


CASE_NAMES = [name for name, *_ in MC.cases(256)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_segments_within_equals_host(solved, cap, name):
    a, b, mask, o = solved[name]
    got, stats = segments_within(a, b, mask, device=None, return_stats=True)
    assert got.dtype == np.bool_
    np.testing.assert_array_equal(got, o["within"])
    assert stats["touched"] == int(o["touched"].sum()) and stats["cut"] == int(o["cut"].sum()), (stats, name)
    # the host recomputation must not be what makes the answer right: it runs for the comb's crossing segments and nowhere else
    assert stats["overflow"] == int((o["n_param"] > cap).sum()) == (MC.COMB_CROSSING if name == "comb" else 0), (stats, name)
    assert stats["launches"] >= 2


@pytest.mark.parametrize("name", CASE_NAMES)
def test_classes_and_raw_codes_equal_host(solved, ctx, cap, name):
    a, b, mask, o = solved[name]
    code, _, classes = _lib.segments_within(ctx, a, b, *_flat_rings(_polygons(mask)), return_classes=True)
    np.testing.assert_array_equal(classes[0], o["ca"])
    np.testing.assert_array_equal(classes[1], o["cb"])
    np.testing.assert_array_equal(classes[2], o["mid"])
    over = o["n_param"] > cap
    np.testing.assert_array_equal(code == 2, over)
    np.testing.assert_array_equal(code[~over] == 1, o["within"][~over])


def test_low_pair_limit_splits_into_launches(solved, ctx):
    a, b, mask, o = solved["wobbly_300"]
    rings = _flat_rings(_polygons(mask))
    n_edges = len(rings[0]) - len(rings[2])
    whole, stats_whole, _ = _lib.segments_within(ctx, a, b, *rings)
    code, stats, classes = _lib.segments_within(ctx, a, b, *rings, pairs_per_launch=700 * n_edges, return_classes=True)
    assert stats["launches"] >= 3 and stats["launches"] > stats_whole["launches"]
    assert stats["launches"] >= -(-3 * len(a) // 700) + -(-len(a) // 700)  # 3 E points and E segments, 700 per launch
    np.testing.assert_array_equal(code, whole)
    np.testing.assert_array_equal(code == 1, o["within"])
    np.testing.assert_array_equal(classes[2], o["mid"])
    assert {k: stats[k] for k in ("touched", "cut", "overflow")} == {k: stats_whole[k] for k in ("touched", "cut", "overflow")}


def test_two_calls_return_the_same_bytes(solved, ctx):
    a, b, mask, _ = solved["wobbly_300"]
    rings = _flat_rings(_polygons(mask))
    first, second = (_lib.segments_within(ctx, a, b, *rings, return_classes=True) for _ in range(2))
    assert first[0].tobytes() == second[0].tobytes() and first[2].tobytes() == second[2].tobytes() and first[1] == second[1]


def test_no_segments(ctx):
    poly = Polygon(MC.SQUARE)
    got, stats = segments_within(np.zeros((0, 2)), np.zeros((0, 2)), poly, device=None, return_stats=True)
    assert got.shape == (0,) and got.dtype == np.bool_ and stats == {"touched": 0, "cut": 0, "overflow": 0, "launches": 0}


def test_invalid_arguments(ctx):
    a, b = np.array([[1.0, 1.0]]), np.array([[2.0, 2.0]])
    closed = np.array([(0, 0), (4, 0), (4, 4), (0, 4), (0, 0)], dtype=np.float64)
    with pytest.raises(_lib.SqgrError, match="not closed") as err:
        _lib.segments_within(ctx, a, b, closed[:4], [0, 4], [0])
    assert err.value.status == -1  # SQGR_ERR_INVALID
    with pytest.raises(_lib.SqgrError, match="at least 4") as err:
        _lib.segments_within(ctx, a, b, closed[[0, 1, 0]], [0, 3], [0])
    assert err.value.status == -1
    with pytest.raises(_lib.SqgrError, match="not finite") as err:
        _lib.segments_within(ctx, a * np.inf, b, closed, [0, 5], [0])
    assert err.value.status == -1
    with pytest.raises(ValueError, match="finite"):
        segments_within(np.array([[np.nan, 1.0]]), b, Polygon(MC.SQUARE), device=None)
    with pytest.raises(ValueError, match="finite"):
        segments_within(a, b, Polygon([(0, 0), (4, 0), (np.inf, 4), (0, 4)]), device=None)
    assert _lib.segments_within(ctx, a, b, closed, [0, 5], [0])[0][0] == 1


def _table(unsorted: bool):
    """A kNN-like graph on a jittered lattice around the M of the reference's test; distances sparser than connectivities in one row."""
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(-1, 6, 0.5), np.arange(-1, 10, 0.5))
    pts = np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-0.1, 0.1, (gx.size, 2))
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    near = (d > 0) & (d < 0.9)
    conn = sp.csr_matrix(near.astype(np.float64))
    dist = sp.csr_matrix(np.where(near, d, 0.0))
    dist.data[3] = 0.0  # an explicit zero among the stored distances
    if unsorted:
        for m in (conn, dist):
            for r in range(m.shape[0]):
                s, e = m.indptr[r], m.indptr[r + 1]
                m.indices[s:e], m.data[s:e] = m.indices[s:e][::-1].copy(), m.data[s:e][::-1].copy()
            m.has_sorted_indices = False
            assert not m.has_canonical_format
    adata = sq.AnnDataLite(X=np.zeros((len(pts), 2)), obs=pd.DataFrame(index=[str(i) for i in range(len(pts))]), obsm={"spatial": pts})
    adata.obsp["spatial_connectivities"], adata.obsp["spatial_distances"] = conn, dist
    return adata


def _same(x, y):
    assert x.shape == y.shape and x.dtype == y.dtype and type(x) is type(y)
    np.testing.assert_array_equal(x.indptr, y.indptr)
    np.testing.assert_array_equal(x.indices, y.indices)
    np.testing.assert_array_equal(x.data, y.data)


@pytest.mark.parametrize("unsorted", [False, True])
@pytest.mark.parametrize("negative_mask", [False, True])
def test_mask_graph_equals_host(negative_mask, unsorted):
    poly = Polygon(MC.M_SHAPE)
    host, dev = _table(unsorted), _table(unsorted)
    want = sq.gr.mask_graph(host, None, poly, negative_mask=negative_mask, copy=True)
    got = sq.gr.mask_graph(dev, None, poly, negative_mask=negative_mask, copy=True, device=None)
    assert 0 < want[0].nnz < host.obsp["spatial_connectivities"].nnz
    _same(got[0], want[0])
    _same(got[1], want[1])
    assert "mask_spatial_connectivities" not in dev.obsp
    # the slot writes
    assert sq.gr.mask_graph(host, None, poly, negative_mask=negative_mask) is None
    assert sq.gr.mask_graph(dev, None, poly, negative_mask=negative_mask, device=None) is None
    for key in ("mask_spatial_connectivities", "mask_spatial_distances"):
        _same(dev.obsp[key], host.obsp[key])
    assert dev.uns["mask_spatial_neighbors"] == host.uns["mask_spatial_neighbors"]
